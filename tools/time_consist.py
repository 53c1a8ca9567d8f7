"""Timings of the consensus entries (profiles/consist.md): a report, not a pass / fail.

  yoho_consistency_graph, yoho_sc2_scores and yoho_consensus_hypotheses (K = 8 and 64) at M = 3233 (the bench pair's match count) and
  M = 16384 (YOHO_CONSIST_MAX_M), on consist_ref.planted_case's cube at tol = 0.05 with 100 planted matches, and - the score kernel only -
  on a graph of the same M with every pair compatible (k1 = k0: deg = M - 1, the cost of the walk at its worst).  Beside the device's
  time per call: the word operations the walk needs (M deg W, from the degrees the device returned), their rate, and at M = 3233 the
  numpy restatement's CPU time for the same step, for orientation only.

    python tools/time_consist.py [--repeats 20] [--out FILE]        # the tables it prints go into profiles/consist.md

Inputs resident on the device; every call warmed twice; HIP events around `--repeats` back-to-back calls of one entry, five such
windows per entry, alternating between the entries; median and [min, max] of a window's time per call."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from yoho_amd import hip  # noqa: E402
import consist_ref as CR  # noqa: E402


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def windows(calls, repeats, rounds=5):
    """calls: [(name, fn)] -> {name: (median, min, max) ms per call}"""
    for _, fn in calls:
        fn()
        fn()
    torch.cuda.synchronize()
    got = {name: [] for name, _ in calls}
    for _ in range(rounds):
        for name, fn in calls:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(repeats):
                fn()
            b.record()
            b.synchronize()
            got[name].append(a.elapsed_time(b) / repeats)
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="*", default=[3233, 16384])
    ap.add_argument("--cpu-limit", type=int, default=4000, help="largest M at which the numpy restatement is timed as well")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_consist.py measures on the GPU; there is none here")
    c = hip.get_context()
    lines = [f"device: {torch.cuda.get_device_name(0)}"]
    for M in args.sizes:
        W = (M + 63) // 64
        p = CR.planted_case(M, 100, 1)
        k0, k1 = cu(p["k0"]), cu(p["k1"])
        bits, deg = c.consistency_graph(k0, k1, 0.05)
        s2 = c.sc2_scores(bits)
        full, fdeg = c.consistency_graph(k0, k0, 0.05)
        assert bool((fdeg == M - 1).all())
        mean_deg = float(deg.double().mean())
        info = [int(v) for v in c.consensus_hypotheses(k0, k1, bits, s2, 64)[3]]
        res = windows([("yoho_consistency_graph", lambda: c.consistency_graph(k0, k1, 0.05)),
                       ("yoho_sc2_scores", lambda: c.sc2_scores(bits)),
                       ("yoho_consensus_hypotheses, K = 8", lambda: c.consensus_hypotheses(k0, k1, bits, s2, 8)),
                       ("yoho_consensus_hypotheses, K = 64", lambda: c.consensus_hypotheses(k0, k1, bits, s2, 64))], args.repeats)
        res.update(windows([("yoho_sc2_scores, complete graph", lambda: c.sc2_scores(full))], max(1, args.repeats // 10)))
        ops = {"yoho_sc2_scores": float(deg.double().sum()) * W, "yoho_sc2_scores, complete graph": float(M) * (M - 1) * W,
               "yoho_consistency_graph": 2.0 * M * W * 64}
        unit = {"yoho_consistency_graph": "f64 square roots"}
        lines += ["", f"M = {M}, W = {W}: mean degree {mean_deg:.1f} at tol 0.05, Kc = {info[0]} of 64", "",
                  "| entry | median ms per call | min | max | work | rate |", "|---|---|---|---|---|---|"]
        for name, (med, lo, hi) in res.items():
            work = f"{ops[name]:.3g} {unit.get(name, 'word operations')}" if name in ops else ""
            rate = f"{ops[name] / med * 1e-6:.1f} G/s" if name in ops else ""
            lines.append(f"| {name} | {med:.3f} | {lo:.3f} | {hi:.3f} | {work} | {rate} |")
        if M <= args.cpu_limit:
            t0 = time.perf_counter()
            rb, _ = CR.graph_ref(p["k0"], p["k1"], 0.05)
            t1 = time.perf_counter()
            rs2 = CR.sc2_ref(rb, M)
            t2 = time.perf_counter()
            CR.consensus_ref(p["k0"], p["k1"], rb, rs2, 8)
            t3 = time.perf_counter()
            assert np.array_equal(bits.cpu().numpy().view(np.uint64), rb) and np.array_equal(s2.cpu().numpy(), rs2)
            lines += ["", f"numpy restatement on this host's CPU, one run each, for orientation only: graph {1e3 * (t1 - t0):.0f} ms, scores {1e3 * (t2 - t1):.0f} ms "
                      f"(a dense f64 matrix product), hypotheses K = 8 {1e3 * (t3 - t2):.0f} ms"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
