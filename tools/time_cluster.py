"""Timings of the density-cluster entry (profiles/cluster.md): a report, not a pass / fail.

  N points of synth.surface_cloud (f32), eps = 4 point spacings, a spacing being sqrt(surface area / N), min_pts = 4:
    yoho_dbscan, all outputs        one grid build and three walks (count, union over the core rows, nearest core neighbour of the
                                    rows that are not core) plus the numbering
    yoho_knn_within, count only     the floor of the same run and box: one grid build and one walk

    python tools/time_cluster.py [--sizes 20000,100000,300000] [--rounds 5] [--out FILE]
    python tools/time_cluster.py --resources         # the compiler's report on csrc/cluster.hip: needs no GPU
    python tools/time_cluster.py --lib other/libyoho_hip.so      # the same windows on another build of the library
    python tools/time_cluster.py --once N            # one warmed call of each at one size and nothing else: for a kernel trace

The protocol is tools/time_clean.py's: one process, inputs resident on the device, every variant warmed twice, device events around a
window of calls that lasts at least `--window` seconds, the variants of a size taking turns `--rounds` times; median and [min, max]
of the per-call times."""
import argparse
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
from time_clean import AREA, alternate  # noqa: E402

MIN_PTS = 4


def resources():
    from yoho_amd import build
    cmd = [build._hipcc()] + build.FLAGS + build.EXTRA["cluster.hip"] + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                                                                        os.path.join(build.CSRC, "cluster.hip"), "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    field = lambda name: re.findall(name + r": (\S+)", err)      # noqa: E731
    lines = ["| kernel | VGPRs | SGPRs | LDS bytes / workgroup | scratch bytes / lane | occupancy (waves / SIMD) |", "|---|---|---|---|---|---|"]
    demangle = lambda n: re.sub(r"^_ZN4yoho\d+(cu_[a-z]+_kernel).*$", r"\1", n)      # noqa: E731
    for row in zip(field("Function Name"), field(r"\bVGPRs"), field("TotalSGPRs"), field(r"LDS Size \[bytes/block\]"), field(r"ScratchSize \[bytes/lane\]"),
                   field(r"Occupancy \[waves/SIMD\]")):
        lines.append(f"| `{demangle(row[0])}` | " + " | ".join(row[1:]) + " |")
    return lines


def cloud(torch, N):
    from yoho_amd import synth
    return torch.from_numpy(synth.surface_cloud(N, seed=1).astype(np.float32)).cuda(), 4.0 * float(np.sqrt(AREA / N))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20000,100000,300000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--once", type=int, default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="load this build of libyoho_hip.so instead of the tree's")
    args = ap.parse_args()
    if args.resources:
        print("\n".join(resources()))
        return
    import torch
    from yoho_amd import hip
    if not torch.cuda.is_available():
        raise SystemExit("time_cluster.py measures on the GPU; there is none here")
    if args.lib:
        hip._LIB_PATH = os.path.abspath(args.lib)
    c = hip.get_context()
    if args.once is not None:
        p, r = cloud(torch, args.once)
        for _ in range(3):
            c.dbscan(p, r, MIN_PTS)
            c.knn_within(p, p, r, 1, skip_same_row=True, want_idx=False, want_d2=False)
        torch.cuda.synchronize()
        return
    lines = [f"device: {torch.cuda.get_device_name(0)}; library {hip._LIB_PATH if args.lib else 'of the tree'}", "",
             f"min_pts = {MIN_PTS}, eps = 4 sqrt(area / N); ms per call: median [min, max] of {args.rounds} alternated windows of >= {args.window} s (calls per window)", "",
             "| N | eps m | neighbours inside: median / max | clusters / core rows / noise rows | variant | ms per call | calls |", "|---|---|---|---|---|---|---|"]
    cell = lambda r: f"{r[0]:.3f} [{r[1]:.3f}, {r[2]:.3f}] | {r[3]}"       # noqa: E731
    ratios = []
    for N in [int(v) for v in args.sizes.split(",")]:
        p, r = cloud(torch, N)
        out = c.dbscan(p, r, MIN_PTS)
        cnt = c.knn_within(p, p, r, 1, skip_same_row=True, want_idx=False, want_d2=False)[2]
        assert torch.equal(out["count"], cnt) and int(out["sizes"].sum()) == N - int(out["n"][2])
        head = f"| {N} | {r:.4f} | {int(cnt.median())} / {int(cnt.max())} | {' / '.join(str(int(v)) for v in out['n'])} |"
        del out, cnt
        res = alternate(torch, [("yoho_dbscan, all outputs", lambda: c.dbscan(p, r, MIN_PTS)),
                                ("yoho_knn_within, count only (the floor)", lambda: c.knn_within(p, p, r, 1, skip_same_row=True, want_idx=False, want_d2=False))],
                        args.rounds, args.window)
        for name, v in res.items():
            lines.append(f"{head} {name} | {cell(v)} |")
            head = "| | | | |"
        d, f = res["yoho_dbscan, all outputs"], res["yoho_knn_within, count only (the floor)"]
        ratios.append(f"N = {N}: yoho_dbscan takes {d[0] / f[0]:.2f} times the count-only call ({d[0]:.3f} [{d[1]:.3f}, {d[2]:.3f}] against {f[0]:.3f} "
                      f"[{f[1]:.3f}, {f[2]:.3f}] ms)")
        del p
        torch.cuda.empty_cache()
    lines += [""] + ratios
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
