"""Timings of the refinement entries (profiles/refine.md):

  (a) yoho_refit_matches at M = 3233 matches (the match count of the 5000-keypoint bench pair), 4 iterations, per call.
  (b) yoho_icp_refine at 20 000 / 20 000 and 300 000 / 300 000 points, 30 iterations (tol < 0: every iteration is made), per call and
      per iteration, alternated in one process with the same iteration COMPOSED from the entries the library had before: the source
      transformed in torch f64 and cast, Context.nn_search (D = 3, squared) on the hash grid (yoho_set_nn_grid, cell = max_dist / 2: what is
      inside the gate is within the two cells the grid settles), the gate as a mask, and a torch f64 Kabsch (masked means, 3 x 3
      covariance, torch.linalg.svd, determinant fix) - no host read inside an iteration, as in the entry.

    python tools/time_refine.py [--repeats 10] [--iters 30] [--out FILE]        # the tables it prints go into profiles/refine.md

The inputs are the tests' own (tests/refine_ref.py: refit_case, icp_case - imported from tests/ on purpose, so that what is timed is
what is tested).

Host clock around work that ends in a device synchronise; every variant warmed; the variants alternate `--repeats` times.  The one speed
condition - an iteration of yoho_icp_refine takes less time than the composed iteration, at both sizes - is checked: the tool exits
non-zero when it does not hold."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from yoho_amd import hip, synth  # noqa: E402
import refine_ref as RR  # noqa: E402


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def window_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(variants, repeats):
    for _, fn in variants:
        for _ in range(2):
            fn()
    times = {name: [] for name, _ in variants}
    for _ in range(repeats):
        for name, fn in variants:
            times[name].append(window_ms(fn))
    return {name: (float(np.median(t)), min(t), max(t)) for name, t in times.items()}


def composed_icp(c, src, tgt, T, max_dist, iters):
    """the iteration from the entries the library had before this one; src / tgt f32 cuda, T (3,4) f64 cuda -> T"""
    s64, t64 = src.to(torch.float64), tgt.to(torch.float64)
    g2 = float(np.float32(max_dist) * np.float32(max_dist))
    fix = torch.ones(3, dtype=torch.float64, device=src.device)
    for _ in range(iters):
        q = (s64 @ T[:, :3].T + T[:, 3]).to(torch.float32)
        d2, idx = c.nn_search(q, tgt, want_dist=True, squared=True)
        w = (d2 < g2).to(torch.float64)[:, None]
        n = w.sum()
        a = t64[idx]
        c0, c1 = (w * a).sum(0) / n, (w * s64).sum(0) / n
        H = ((s64 - c1) * w).T @ (a - c0)
        U, S, Vh = torch.linalg.svd(H)
        d = fix.clone()
        d[2] = torch.sign(torch.linalg.det(Vh.T @ U.T))
        R = (Vh.T * d) @ U.T
        T = torch.cat([R, (c0 - R @ c1)[:, None]], dim=1)
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--sizes", type=int, nargs="*", default=[20000, 300000])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_refine.py measures on the GPU; there is none here")
    c = hip.get_context()
    lines = [f"device: {torch.cuda.get_device_name(0)}"]
    # (a)
    case = RR.refit_case(0, M=3233)
    k0, k1, T0 = cu(case["k0"]), cu(case["k1"]), cu(case["T0"])
    res = alternate([("yoho_refit_matches, 4 iterations", lambda: c.refit_matches(k0, k1, T0, case["inlier_dist"], 4))], args.repeats * 5)
    _, counts, info = c.refit_matches(k0, k1, T0, case["inlier_dist"], 4)
    lines += ["", f"(a) refit at M = 3233: counts {counts.cpu().numpy().tolist()}, (iterate kept, iterates evaluated) = {info.cpu().numpy().tolist()}", "",
              "| variant | median ms per call | min | max |", "|---|---|---|---|"]
    for name, (med, lo, hi) in res.items():
        lines.append(f"| {name} | {med:.4f} | {lo:.4f} | {hi:.4f} |")
    # (b)
    held = True
    for n in args.sizes:
        ic = RR.icp_case(n=n, seed=3) if n <= 50000 else None
        if ic is None:                                     # the large pair: a 3 m scene, as tools/time_trainset.py's clouds
            pc = synth.surface_cloud(n, seed=3, extent=3.0)
            small = RR.icp_case(n=1000, seed=3)
            T_gt = small["T_gt"]
            ic = {"src": np.ascontiguousarray((pc - T_gt[:, 3]) @ T_gt[:, :3], np.float32), "tgt": np.ascontiguousarray(pc, np.float32), "T_gt": T_gt,
                  "T0": small["T0"], "max_dist": 0.1}
        src, tgt, T0, md = cu(ic["src"]), cu(ic["tgt"]), cu(ic["T0"]), ic["max_dist"]
        c.set_nn_grid(md / 2)
        try:
            res = alternate([("yoho_icp_refine", lambda: c.icp_refine(src, tgt, T0, md, args.iters, -1.0)),
                             ("composed: torch transform + nn_search on the grid + torch f64 Kabsch", lambda: composed_icp(c, src, tgt, T0, md, args.iters))],
                            args.repeats)
            T_dev, npairs, rmse, info = c.icp_refine(src, tgt, T0, md, args.iters, -1.0)
            T_cmp = composed_icp(c, src, tgt, T0, md, args.iters)
        finally:
            c.set_nn_grid(0)
        gt = ic["T_gt"]
        e_dev, e_cmp = RR.rot_error_deg(gt[:, :3], T_dev.cpu().numpy()[:, :3]), RR.rot_error_deg(gt[:, :3], T_cmp.cpu().numpy()[:, :3])
        lines += ["", f"(b) ICP at {n} / {n} points, gate {md} m, {args.iters} iterations: pairs {int(npairs[0])} -> {int(npairs[-1])}, rmse {float(rmse[0]):.5f} -> "
                      f"{float(rmse[-1]):.5f}; rotation error after the run {e_dev:.2e} degrees (composed: {e_cmp:.2e})", "",
                  "| variant | median ms per call | per iteration | min | max |", "|---|---|---|---|---|"]
        for name, (med, lo, hi) in res.items():
            lines.append(f"| {name} | {med:.3f} | {med / args.iters:.4f} | {lo:.3f} | {hi:.3f} |")
        ours, theirs = res["yoho_icp_refine"][0], [v for k, v in res.items() if k != "yoho_icp_refine"][0][0]
        lines += ["", f"speed condition (an iteration of the entry below the composed iteration): {ours / args.iters:.4f} < {theirs / args.iters:.4f}: {ours < theirs}"]
        held = held and ours < theirs
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if not held:
        raise SystemExit("the speed condition of yoho_icp_refine does not hold: its iteration is not faster than the composed one")


if __name__ == "__main__":
    main()
