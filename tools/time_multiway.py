"""Timings of the multiway entry and the scene pass (profiles/multiway.md): a report, not a pass / fail.

  (a) yoho_edge_information with K = 1, 8, 64 sources of `--points` points against one target of as many, gate 0.05 m, beside the only
      way the library had to get the pair counts of K registrations into one fragment: K separate yoho_eval_transforms calls, each of
      which rebuilds the grid over the target (and gives no matrix).
  (b) a whole synthetic scene: `--fragments` fragments of `--points` points, windows of one surface cloud, every pair whose windows
      share at least 30 % registered (the ground truth 0.5 degrees / 1 cm off, one registration in twenty false), multiway.scene_edges
      and multiway.optimize timed apart.

    python tools/time_multiway.py [--repeats 5] [--points 300000] [--fragments 60] [--out FILE]

Inputs resident on the device; host clock around work that ends in a device synchronise (scene_edges ends in its one read-back); every
variant warmed twice; the variants alternate `--repeats` times; median and [min, max]; the shader clock the library's one-wave probe
sees right after each table."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from yoho_amd import hip, multiway, synth  # noqa: E402
import refine_ref as RR  # noqa: E402
from time_refine import alternate, cu  # noqa: E402
from time_keypoints import shader_mhz  # noqa: E402

GATE = 0.05


def rigid(rs, deg, shift):
    T = np.eye(4)
    T[:3] = RR.perturbed(np.eye(4)[:3], rs, deg, shift)
    return T


def inverse(X):
    Y = np.eye(4)
    Y[:3, :3] = X[:3, :3].T
    Y[:3, 3] = -X[:3, :3].T @ X[:3, 3]
    return Y


def one_target(c, args, lines):
    n = args.points
    rs = np.random.RandomState(n)
    pc = synth.surface_cloud(n, seed=3, extent=3.0)
    tgt = cu(pc.astype(np.float32))
    srcs, rows = [], []
    for _ in range(64):
        X = rigid(rs, 60.0 * rs.rand(), 1.0)                           # the source's own frame
        Xi = inverse(X)
        srcs.append(cu((pc[rs.permutation(n)] @ Xi[:3, :3].T + Xi[:3, 3] + 0.002 * rs.randn(n, 3)).astype(np.float32)))
        rows.append((rigid(rs, 0.5, 0.01) @ X)[:3])                    # its registration: the truth 0.5 degrees / 1 cm off
    T = cu(np.stack(rows))
    lines += ["", f"(a) one target of {n} points, K sources of {n} points each, gate {GATE} m", "",
              "| K | variant | median ms per call | min | max | pairs per edge |", "|---|---|---|---|---|---|"]
    for K in (1, 8, 64):
        src = torch.cat(srcs[:K], dim=0)
        soff = (np.arange(K + 1) * n).astype(np.int32)
        Tk = T[:K].contiguous()
        single = [T[k:k + 1].contiguous() for k in range(K)]
        npairs, rmse, _ = c.edge_information(src, soff, tgt, Tk, GATE)
        en = torch.cat([c.eval_transforms(srcs[k], tgt, single[k], GATE)[0] for k in range(K)])
        assert torch.equal(npairs, en)

        def separate():
            for k in range(K):
                c.eval_transforms(srcs[k], tgt, single[k], GATE)

        res = alternate([("yoho_edge_information", lambda: c.edge_information(src, soff, tgt, Tk, GATE)),
                         (f"{K} x yoho_eval_transforms", separate)], args.repeats)
        for name, (med, lo, hi) in res.items():
            lines.append(f"| {K} | {name} | {med:.3f} | {lo:.3f} | {hi:.3f} | {int(npairs.min())} - {int(npairs.max())} |")
        del src
    lines.append(f"shader clock right after: {shader_mhz(torch, c):.0f} MHz")


def scene(c, args, lines):
    F, m = args.fragments, args.points
    width = 0.15
    n = int(round(m / width))
    rs = np.random.RandomState(F)
    pc = synth.surface_cloud(n, seed=5, extent=6.0)
    order = np.argsort(pc[:, 0], kind="stable")
    step = (1.0 - width) / max(F - 1, 1)
    Xg = [np.eye(4)] + [rigid(rs, 60.0 * rs.rand(), 1.0) for _ in range(F - 1)]
    clouds = []
    for f in range(F):
        lo = int(round(f * step * n))
        rows = order[lo:lo + m]
        Xi = inverse(Xg[f])
        clouds.append(cu((pc[rows] @ Xi[:3, :3].T + Xi[:3, 3] + 0.002 * rs.randn(len(rows), 3)).astype(np.float32)))
    reach = int(np.floor(0.7 * width / step))
    pairs, T, false = [], [], []
    for i in range(F):
        for j in range(i + 1, min(F, i + reach + 1)):
            Tt = inverse(Xg[i]) @ Xg[j]
            bad = j - i > 1 and rs.rand() < 0.05
            Tm = np.eye(4)
            Tm[:3] = RR.perturbed(Tt[:3], rs, 40.0, 0.3) if bad else RR.perturbed(Tt[:3], rs, 0.5, 0.01)
            pairs.append((i, j)); T.append(Tm); false.append(bad)
    pairs, T, false = np.array(pairs, np.int64), np.stack(T), np.array(false)
    chunks = multiway.edge_chunks(pairs, [x.shape[0] for x in clouds])
    out = {}

    def edges():
        out["ed"] = multiway.scene_edges(c, clouds, pairs, T, GATE)

    res = alternate([("scene_edges", edges)], args.repeats)
    ed = out["ed"]
    ts = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        r = multiway.optimize(F, pairs, T, ed["info"])
        ts.append((time.perf_counter() - t0) * 1e3)
    deg = max(RR.rot_error_deg(a[:3, :3], b[:3, :3]) for a, b, ok in zip(r["poses"], Xg, r["reached"]) if ok)
    lines += ["", f"(b) a scene of {F} fragments of {m} points: {len(pairs)} registrations (|i - j| <= {reach}), {int(false.sum())} of them false, "
                  f"{len(chunks)} device calls, gate {GATE} m", "",
              "| stage | median ms | min | max |", "|---|---|---|---|",
              "| multiway.scene_edges (device, one read-back) | {:.1f} | {:.1f} | {:.1f} |".format(*res["scene_edges"]),
              f"| multiway.optimize (host, float64 numpy) | {np.median(ts):.1f} | {min(ts):.1f} | {max(ts):.1f} |", "",
              f"pairs per edge: true {int(ed['npairs'][~false].min())} - {int(ed['npairs'][~false].max())}, false "
              f"{int(ed['npairs'][false].min()) if false.any() else 0} - {int(ed['npairs'][false].max()) if false.any() else 0}; pruned {int(r['pruned'].sum())} "
              f"(the false ones exactly: {bool(np.array_equal(r['pruned'] | r['dropped'], false))}), dropped {int(r['dropped'].sum())}, "
              f"{len(r['history_stage1']) - 1} + {len(r['history_stage2']) - 1} accepted iterations, largest rotation error against the ground truth {deg:.3f} degrees",
              f"shader clock right after: {shader_mhz(torch, c):.0f} MHz"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--fragments", type=int, default=60)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_multiway.py measures on the GPU; there is none here")
    c = hip.get_context()
    lines = [f"device: {torch.cuda.get_device_name(0)}"]
    one_target(c, args, lines)
    scene(c, args, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
