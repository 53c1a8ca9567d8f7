"""Timings of the fused scene (profiles/fuse.md): a report, not a pass / fail.

  yoho_fuse_clouds on F = 1, 8, 60 fragments of `--points` points - windows of one surface cloud, each in its own frame under its own
  pose, 2 mm of noise - at voxels of 0.01 and 0.025 m, beside the same fusion done with tensor-library device ops, which is what a
  user had before: the poses applied in float64, floor, an int64 key, unique with inverse indices and counts, index_add_ of the
  float64 points, the quotient.  That path is timed here and is not code under test.  It gives no fragment count per voxel and its sums
  are float atomics; the table says whether two runs of either path gave the same bytes.

    python tools/time_fuse.py [--repeats 5] [--points 300000] [--out FILE]
    rocprofv3 --kernel-trace -d DIR -- python tools/time_fuse.py --breakdown      (then tools/rocpd_stats.py DIR: the kernels of F = 60, 0.025 m)

Inputs resident on the device; host clock around work that ends in a device synchronise; every variant warmed twice; the variants
alternate `--repeats` times; median and [min, max]; the shader clock the library's one-wave probe sees right after each table."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from yoho_amd import hip, synth  # noqa: E402
from time_refine import alternate, cu  # noqa: E402
from time_keypoints import shader_mhz  # noqa: E402
from time_multiway import inverse, rigid  # noqa: E402

FRAGMENTS = (1, 8, 60)
VOXELS = (0.01, 0.025)


def make_scene(F, m):
    """F windows of m points of one surface cloud (6 m, the windows 15 % of its sorted x wide), each stored in its own frame (f32) with
    2 mm of noise -> (src (F m,3) f32 cuda, soff, T (F,3,4) f64 cuda, frag (F m) int64 cuda)"""
    width = 0.15
    n = int(round(m / width))
    rs = np.random.RandomState(F)
    pc = cu(synth.surface_cloud(n, seed=5, extent=6.0))
    pc = pc[torch.argsort(pc[:, 0], stable=True)]
    n = pc.shape[0]
    step = (1.0 - width) / max(F - 1, 1)
    g = torch.Generator(device="cuda")
    g.manual_seed(F)
    clouds, Ts = [], []
    for f in range(F):
        lo = min(int(round(f * step * n)), n - m)
        X = np.eye(4) if f == 0 else rigid(rs, 60.0 * rs.rand(), 1.0)
        Xi = cu(inverse(X))
        w = pc[lo:lo + m] + 0.002 * torch.randn((m, 3), dtype=torch.float64, device="cuda", generator=g)
        clouds.append((w @ Xi[:3, :3].T + Xi[:3, 3]).to(torch.float32))
        Ts.append(X[:3])
    src = torch.cat(clouds, dim=0)
    soff = (np.arange(F + 1) * m).astype(np.int32)
    frag = torch.arange(F, device="cuda").repeat_interleave(m)
    return src, soff, cu(np.stack(Ts)), frag


def torch_fuse(src, frag, T, voxel):
    """the tensor-library path -> (pts (M,3) f32, count (M) int64)"""
    Tp = T[frag]
    s = src.to(torch.float64)
    q = torch.stack([(Tp[:, i, 0] * s[:, 0] + Tp[:, i, 1] * s[:, 1]) + Tp[:, i, 2] * s[:, 2] + Tp[:, i, 3] for i in range(3)], dim=1)
    c = torch.floor(q * (1.0 / voxel)).to(torch.int64) + (1 << 20)
    key = (c[:, 2] << 42) | (c[:, 1] << 21) | c[:, 0]
    _, inv, count = torch.unique(key, return_inverse=True, return_counts=True)
    sums = torch.zeros((count.shape[0], 3), dtype=torch.float64, device=src.device).index_add_(0, inv, q)
    return (sums / count[:, None].to(torch.float64)).to(torch.float32), count


def same(a, b):
    return all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))


def table(c, args, lines):
    lines += ["", f"fragments of {args.points} points, min_count = min_frags = 1, no normals; ms per fusion", "",
              "| F | points | voxel m | voxels M | yoho: count call + read + sized call | yoho: one sized call | torch unique + index_add_ | same bytes twice: yoho / torch | "
              "max abs difference of the means | voxels with nfrag >= 2 |", "|---|---|---|---|---|---|---|---|---|---|"]
    for F in FRAGMENTS:
        src, soff, T, frag = make_scene(F, args.points)
        for voxel in VOXELS:
            out = c.fuse_clouds(src, soff, T, voxel)
            M = out["M"]
            again = c.fuse_clouds(src, soff, T, voxel)
            keys = ("pts", "count", "nfrag", "row_of")
            y_same = same([out[k] for k in keys], [again[k] for k in keys])
            tp, tc = torch_fuse(src, frag, T, voxel)
            t_same = same(torch_fuse(src, frag, T, voxel), (tp, tc))
            assert tp.shape[0] == M and torch.equal(tc.to(torch.int32), out["count"])
            diff = float((tp.to(torch.float64) - out["pts"].to(torch.float64)).abs().max())
            shared = int((out["nfrag"] >= 2).sum())
            del out, again, tp, tc
            res = alternate([("two", lambda: c.fuse_clouds(src, soff, T, voxel)),
                             ("one", lambda: c.fuse_clouds(src, soff, T, voxel, capacity=M)),
                             ("torch", lambda: torch_fuse(src, frag, T, voxel))], args.repeats)
            cell = lambda r: f"{r[0]:.2f} [{r[1]:.2f}, {r[2]:.2f}]"       # noqa: E731
            lines.append(f"| {F} | {src.shape[0]} | {voxel} | {M} | {cell(res['two'])} | {cell(res['one'])} | {cell(res['torch'])} | "
                         f"{'yes' if y_same else 'NO'} / {'yes' if t_same else 'no'} | {diff:.3g} | {shared} |")
        del src, T, frag
        torch.cuda.empty_cache()
    lines.append(f"shader clock right after: {shader_mhz(torch, c):.0f} MHz")


def breakdown(c, args):
    """what a kernel trace is taken of: F = 60 at 0.025 m, one sized call, three times after one warm-up pair"""
    src, soff, T, _ = make_scene(60, args.points)
    M = c.fuse_clouds(src, soff, T, 0.025)["M"]
    for _ in range(3):
        c.fuse_clouds(src, soff, T, 0.025, capacity=M)
    torch.cuda.synchronize()
    print(f"breakdown: 60 fragments of {args.points} points, voxel 0.025 m, M = {M}: 1 count call + 4 sized calls")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--breakdown", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_fuse.py measures on the GPU; there is none here")
    c = hip.get_context()
    if args.breakdown:
        breakdown(c, args)
        return
    lines = [f"device: {torch.cuda.get_device_name(0)}"]
    table(c, args, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
