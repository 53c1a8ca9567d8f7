"""Nearest-neighbour timings on the bench's descriptors (5000 x 5000 x 32) and on a 3-D cloud (5000 x 300 000):

  * mutual NN: pre-filter vs brute force (the round-4 table);
  * k nearest neighbours (yoho_knn_search), one row per k, next to yoho_nn_search on the same inputs and to the reference's own
    formulation on the same device in the same process: chunks of 500 source rows, explicit-difference pdist, torch.topk(-dist, k)
    (utils/knn_search.py:68-106 written out with torch ops; its per-chunk copies to the host are left out, which favours it).

    python tools/time_nn.py [--repeats 5] [--window 0.3] [--out profiles/knn_search_timings.md]
    python tools/time_nn.py --brute-only [--lib other/libyoho_hip.so]      # the brute-force searches alone (nn32seg_kernel's family):
                                                                           # yoho_nn_search 'L2' at 5000 x 5000 and, below 2^20 pairs,
                                                                           # at 1000 x 1000, x 32 and x 3; mutual NN with the pre-filter
                                                                           # off; yoho_knn_search at k = 1, 4, 16; --lib times another
                                                                           # build of the library (a parent commit's) in a process of
                                                                           # its own

One process, every variant warmed up, HIP events on the stream, a timed window repeats the call until it lasts `--window` seconds (a
single call is tens of microseconds and would measure the launch), the variants alternate `--repeats` times; median and [min, max] of
the windows' per-call times are printed, with the shader clock the library's one-wave probe saw while the windows ran."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from yoho_amd import hip, synth  # noqa: E402
from yoho_amd.power import ClockProbe  # noqa: E402


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def torch_knn(src, tgt, k, squared=False, chunk=500):
    """modified_knn_matcher.find_knn_gpu / pdist with torch ops on the device"""
    ds, ids = [], []
    for i in range(0, src.shape[0], chunk):
        d = torch.sum((src[i:i + chunk].unsqueeze(1) - tgt.unsqueeze(0)).pow(2), 2)
        if not squared:
            d = torch.sqrt(d + 1e-7)
        v, ind = torch.topk(-d, k, dim=1)
        ds.append(-v)
        ids.append(ind)
    return torch.cat(ds, 0), torch.cat(ids, 0)


def per_call_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(variants, repeats, window, probe=None):
    """variants: [(name, fn)] -> {name: (median, min, max, calls per window)} of per-call milliseconds, the variants taking turns"""
    reps = {}
    for name, fn in variants:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps[name] = max(1, int(np.ceil(window * 1e3 / max(per_call_ms(fn, 3), 1e-4))))
    times = {name: [] for name, _ in variants}
    for _ in range(repeats):
        for name, fn in variants:
            if probe is not None:
                probe.queue(2)                       # on the probe's own high-priority stream, beside the window
            times[name].append(per_call_ms(fn, reps[name]))
    return {name: (float(np.median(t)), min(t), max(t), reps[name]) for name, t in times.items()}


def table(title, res, lines):
    lines.append("")
    lines.append(title)
    lines.append("")
    lines.append("| variant | k | median ms per call | min | max | calls per window |")
    lines.append("|---|---|---|---|---|---|")
    for (name, k), (med, lo, hi, n) in res.items():
        lines.append(f"| {name} | {k} | {med:.4f} | {lo:.4f} | {hi:.4f} | {n} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds a timed window lasts at least")
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    ap.add_argument("--skip-3d", action="store_true")
    ap.add_argument("--brute-only", action="store_true", help="only the brute-force searches: nn_search 'L2' at D = 32 and D = 3, mutual NN without the pre-filter")
    ap.add_argument("--lib", default=None, help="load this build of libyoho_hip.so instead of the tree's")
    args = ap.parse_args()
    if args.lib:
        hip._LIB_PATH = os.path.abspath(args.lib)
    c = hip.Context(0)
    probe = ClockProbe(c, us=200)
    lines = [f"device: {torch.cuda.get_device_name(0)}; {args.repeats} alternated windows of >= {args.window} s per variant"]

    pr = synth.make_pair(5000, seed=10)
    a, b = cu(np.mean(pr["feat0"], -1)), cu(np.mean(pr["feat1"], -1))
    if args.brute_only:
        rs = np.random.RandomState(3)
        q3, t3 = cu(rs.rand(5000, 3).astype(np.float32) * 3), cu(rs.rand(5000, 3).astype(np.float32) * 3)
        c.set_nn_grid(0)
        c.set_nn_prefilter(False)
        variants = [(("yoho_nn_search, 5000 x 5000 x 32, 'L2'", 1), lambda: c.nn_search(a, b, want_dist=True)),
                    (("yoho_nn_search, 5000 x 5000 x 3, 'L2'", 1), lambda: c.nn_search(q3, t3, want_dist=True)),
                    (("mutual_nn, brute force, 5000 x 5000 x 32", "-"), lambda: c.mutual_nn(a, b)),
                    (("yoho_nn_search, 1000 x 1000 x 32, 'L2'", 1), lambda: c.nn_search(a[:1000], b[:1000], want_dist=True)),
                    (("yoho_nn_search, 1000 x 1000 x 3, 'L2'", 1), lambda: c.nn_search(q3[:1000], t3[:1000], want_dist=True))]
        for k in (1, 4, 16):
            variants.append((("yoho_knn_search, 5000 x 5000 x 32, 'L2'", k), lambda k=k: c.knn_search(a, b, k)))
        res = alternate(variants, args.repeats, args.window, probe)
        c.set_nn_prefilter(True)
        lines[0] += f"; library {hip._LIB_PATH if args.lib else 'of the tree'}"
        table("brute-force searches", res, lines)
        lines.append("")
        lines.append(f"shader clock while the windows ran (one-wave probes of 200 us): {probe.summary()}")
        text = "\n".join(lines)
        print(text)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    variants = []
    for on in (True, False):
        def mutual(on=on):
            c.set_nn_prefilter(on)
            return c.mutual_nn(a, b)
        variants.append((("mutual_nn, pre-filter" if on else "mutual_nn, brute force", "-"), mutual))
    res = alternate(variants, args.repeats, args.window, probe)
    c.set_nn_prefilter(True)
    table("mutual NN, 5000 x 5000 x 32", res, lines)

    variants = [(("yoho_nn_search", 1), lambda: c.nn_search(a, b, want_dist=True))]
    for k in (1, 2, 8, 16):
        variants.append((("yoho_knn_search", k), lambda k=k: c.knn_search(a, b, k)))
        variants.append((("torch pdist + topk, chunks of 500", k), lambda k=k: torch_knn(a, b, k)))
    res = alternate(variants, args.repeats, args.window, probe)
    table("k nearest neighbours, 5000 x 5000 x 32, 'L2' with distances", res, lines)
    for k in (2, 8):                                       # the two formulations agree (neighbours; distances to fp32 rounding)
        d0, i0 = c.knn_search(a, b, k)
        d1, i1 = torch_knn(a, b, k)
        lines.append(f"k = {k}: {int((i0 != i1).any(1).sum())} of 5000 rows differ from the torch formulation in an index, "
                     f"largest distance difference {float((d0 - d1).abs().max()):.2e}")

    if not args.skip_3d:
        rs = np.random.RandomState(3)
        q, cloud = cu(rs.rand(5000, 3).astype(np.float32) * 3), cu(rs.rand(300000, 3).astype(np.float32) * 3)
        c.set_nn_grid(0)
        variants = [(("yoho_nn_search (brute force)", 1), lambda: c.nn_search(q, cloud, want_dist=True)),
                    (("yoho_knn_search", 8), lambda: c.knn_search(q, cloud, 8)),
                    (("torch pdist + topk, chunks of 500", 8), lambda: torch_knn(q, cloud, 8))]
        res = alternate(variants, args.repeats, args.window, probe)
        table("k nearest neighbours, 5000 x 300 000 x 3, 'L2' with distances", res, lines)
        d0, i0 = c.knn_search(q, cloud, 8)
        d1, i1 = torch_knn(q, cloud, 8)
        lines.append(f"k = 8: {int((i0 != i1).any(1).sum())} of 5000 rows differ from the torch formulation in an index")

    lines.append("")
    lines.append(f"shader clock while the windows ran (one-wave probes of 200 us): {probe.summary()}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
