"""Timings of the outlier-filter entries (profiles/clean.md): a report, not a pass / fail.

  N points of synth.surface_cloud (f32), k = 16, max_dist = 4 point spacings, a spacing being sqrt(surface area / N):
    yoho_statistical_outliers   against the only exact route the library had before: yoho_knn_search(D = 3, squared) of the cloud on itself
                                (brute force, Ns x Nt distances; k = 16 there holds the point itself and 15 others, one neighbour fewer)
                                plus the gate, the means, mu, sigma and the mask with tensor-library ops
    yoho_knn_within             with all three outputs, against the same yoho_knn_search
    yoho_knn_within, count only against yoho_estimate_normals on the same radius: the same walk plus a covariance and an eigenvector
    yoho_nn_within              for scale: the same grid build and rf_walk, one neighbour

    python tools/time_clean.py [--sizes 20000,100000,300000] [--rounds 5] [--out FILE]
    python tools/time_clean.py --resources           # the compiler's report on csrc/clean.hip: needs no GPU
    python tools/time_clean.py --lib other/libyoho_hip.so      # the same windows on another build of the library

One process, inputs resident on the device, every variant warmed twice, device events around a window of calls that lasts at least
`--window` seconds, the variants of a size taking turns `--rounds` times; median and [min, max] of the per-call times."""
import argparse
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

K = 16
AREA = 4 * 1.2 ** 2 + 4 * np.pi * (0.3 * 1.2) ** 2          # synth.surface_cloud(extent = 1.2): four planes and a sphere


def resources():
    from yoho_amd import build
    cmd = [build._hipcc()] + build.FLAGS + build.EXTRA["clean.hip"] + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                                                                      os.path.join(build.CSRC, "clean.hip"), "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    field = lambda name: re.findall(name + r": (\S+)", err)      # noqa: E731
    lines = ["| kernel | VGPRs | SGPRs | LDS bytes / workgroup | scratch bytes / lane | occupancy (waves / SIMD) |", "|---|---|---|---|---|---|"]
    demangle = lambda n: re.sub(r"^_ZN4yoho\d+(cl_[a-z]+_kernel)(?:ILi(\d+)E)?.*$", lambda m: m.group(1) + (f"<{m.group(2)}>" if m.group(2) else ""), n)      # noqa: E731
    for row in zip(field("Function Name"), field(r"\bVGPRs"), field("TotalSGPRs"), field(r"LDS Size \[bytes/block\]"), field(r"ScratchSize \[bytes/lane\]"),
                   field(r"Occupancy \[waves/SIMD\]")):
        lines.append(f"| `{demangle(row[0])}` | " + " | ".join(row[1:]) + " |")
    return lines


def per_call_ms(torch, fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def alternate(torch, variants, rounds, window):
    calls = {}
    for name, fn in variants:
        fn()
        fn()
        torch.cuda.synchronize()
        calls[name] = max(1, int(np.ceil(window * 1e3 / max(per_call_ms(torch, fn, 1), 1e-3))))
    times = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            times[name].append(per_call_ms(torch, fn, calls[name]))
    return {name: (float(np.median(t)), min(t), max(t), calls[name]) for name, t in times.items()}


def verdict(new, old):
    """(median, min, max, calls) of the new entry and of its yardstick -> words: faster or slower only when the windows do not overlap"""
    ratio = old[0] / new[0]
    if new[2] < old[1]:
        return f"{ratio:.1f}x faster, beyond the spread (slowest window {new[2]:.3f} ms against the yardstick's fastest {old[1]:.3f} ms)"
    if old[2] < new[1]:
        return f"{1 / ratio:.1f}x SLOWER, beyond the spread (fastest window {new[1]:.3f} ms against the yardstick's slowest {old[2]:.3f} ms)"
    return f"within the spread ({new[0]:.3f} [{new[1]:.3f}, {new[2]:.3f}] against {old[0]:.3f} [{old[1]:.3f}, {old[2]:.3f}] ms)"


def brute_statistical(torch, c, p, max_dist, std_ratio=2.0):
    """the route of before: the 15 nearest others by brute force, the gate, mean, mu, sigma and mask with tensor ops -> (keep, m)"""
    d2 = c.knn_search(p, p, K, want_dist=True, squared=True)[0][:, 1:]
    g2 = float(np.float32(max_dist) * np.float32(max_dist))
    inside = d2 < g2
    found = inside.sum(dim=1)
    m = (torch.sqrt(d2.to(torch.float64)) * inside).sum(dim=1) / found
    valid = found >= 1
    mv = m[valid]
    thr = mv.mean() + std_ratio * mv.std()
    return valid & (m <= thr), m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20000,100000,300000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="load this build of libyoho_hip.so instead of the tree's")
    args = ap.parse_args()
    if args.resources:
        print("\n".join(resources()))
        return
    import torch
    from yoho_amd import hip, synth
    if not torch.cuda.is_available():
        raise SystemExit("time_clean.py measures on the GPU; there is none here")
    if args.lib:
        hip._LIB_PATH = os.path.abspath(args.lib)
    c = hip.get_context()
    lines = [f"device: {torch.cuda.get_device_name(0)}; library {hip._LIB_PATH if args.lib else 'of the tree'}", "",
             f"k = {K}, max_dist = 4 sqrt(area / N); ms per call: median [min, max] of {args.rounds} alternated windows of >= {args.window} s (calls per window)", "",
             "| N | max_dist m | neighbours inside: median / max | kept | variant | ms per call | calls |", "|---|---|---|---|---|---|---|"]
    cell = lambda r: f"{r[0]:.3f} [{r[1]:.3f}, {r[2]:.3f}] | {r[3]}"       # noqa: E731
    verdicts = []
    for N in [int(v) for v in args.sizes.split(",")]:
        p = torch.from_numpy(synth.surface_cloud(N, seed=1).astype(np.float32)).cuda()
        r = 4.0 * float(np.sqrt(AREA / N))
        out = c.statistical_outliers(p, r, k=K)
        cnt = out["count"]
        keep_b, m_b = brute_statistical(torch, c, p, r)
        full = cnt >= K                                                  # the brute-force route has 15 neighbours, the entry 16: compare where it matters
        agree = int((keep_b == out["keep"].bool()).sum())
        d2, idx, cnt2 = c.knn_within(p, p, r, K)
        kd, ki = c.knn_search(p, p, K, want_dist=True, squared=True)
        assert torch.equal(cnt2 - 1, cnt) and torch.equal(idx[full], ki[full]) and torch.equal(d2[full], kd[full])
        assert torch.equal(c.knn_within(p, p, r, 1, want_idx=False, want_d2=False)[2], c.estimate_normals(p, r, 3)[1])
        head = f"| {N} | {r:.4f} | {int(cnt.median())} / {int(cnt.max())} | {int(out['n_keep'][0])} ({agree} of {N} as the 15-neighbour route) |"
        del out, keep_b, m_b, d2, idx, cnt2, kd, ki
        res = alternate(torch, [("yoho_statistical_outliers", lambda: c.statistical_outliers(p, r, k=K)),
                                ("yoho_knn_search + tensor ops (the route of before)", lambda: brute_statistical(torch, c, p, r)),
                                ("yoho_knn_within, idx + d2 + count", lambda: c.knn_within(p, p, r, K)),
                                ("yoho_knn_search, idx + d2", lambda: c.knn_search(p, p, K, want_dist=True, squared=True)),
                                ("yoho_knn_within, count only", lambda: c.knn_within(p, p, r, 1, want_idx=False, want_d2=False)),
                                ("yoho_estimate_normals", lambda: c.estimate_normals(p, r, 3)),
                                ("yoho_nn_within (the same grid build, the plain walk)", lambda: c.nn_within(p, p, r))], args.rounds, args.window)
        for name, v in res.items():
            lines.append(f"{head} {name} | {cell(v)} |")
            head = "| | | | |"
        s, b = res["yoho_statistical_outliers"], res["yoho_knn_search + tensor ops (the route of before)"]
        w, kb = res["yoho_knn_within, idx + d2 + count"], res["yoho_knn_search, idx + d2"]
        verdicts.append(f"N = {N}: the filter against the route of before: {verdict(s, b)}; the search against yoho_knn_search: {verdict(w, kb)}")
        del p
        torch.cuda.empty_cache()
    lines += [""] + verdicts
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
