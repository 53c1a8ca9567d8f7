"""Timings of the verification entries (profiles/verify.md): a report, not a pass / fail.

  (a) yoho_eval_transforms at K = 1, 8, 64 on 20 000 / 20 000 and 300 000 / 300 000 points, gate 0.1 m, beside its baseline: K calls of
      yoho_icp_refine(iters = 1) on the same clouds, which is what the library offered before (each call rebuilds the grid over the
      target and runs the covariance and solve launches that an evaluation does not need).
  (b) the same call on a source sorted by its own grid cell beforehand (a stable sort on the host side of the call, not timed): what the
      walk gains when the lanes of a wave visit the same buckets.  The figures of a sorted source are those of another summation
      order, so this is a measurement of the lever described in DESIGN 3.14, not a variant of the entry.
  (c) yoho_verify_hypotheses at H = 1000 positions, K = 8 and 64, distinct_tol 0.05.

    python tools/time_verify.py [--repeats 5] [--out FILE]        # the tables it prints go into profiles/verify.md

Inputs resident on the device; host clock around work that ends in a device synchronise; every variant warmed twice; the variants
alternate `--repeats` times; median and [min, max]."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from yoho_amd import hip  # noqa: E402
import refine_ref as RR  # noqa: E402
from time_plane import pair_of  # noqa: E402
from time_refine import alternate, cu  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=[20000, 300000])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_verify.py measures on the GPU; there is none here")
    c = hip.get_context()
    lines = [f"device: {torch.cuda.get_device_name(0)}"]
    for n in args.sizes:
        ic, _ = pair_of(n)
        src, tgt, md, gt = cu(ic["src"]), cu(ic["tgt"]), ic["max_dist"], ic["T_gt"]
        rs = np.random.RandomState(n)
        rows = np.stack([gt] + [RR.perturbed(gt, rs, 5.0 * rs.rand(), 0.1 * rs.rand()) for _ in range(63)])
        T = cu(rows)
        cell = (src / (md * (1.0 + 2.0 ** -10))).floor().to(torch.int64) + (1 << 20)
        perm = torch.argsort((cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2], stable=True)
        src_sorted = src[perm].contiguous()
        npairs, _, cost = c.eval_transforms(src, tgt, T, md)
        np_s, _, cost_s = c.eval_transforms(src_sorted, tgt, T, md)
        assert torch.equal(npairs, np_s) and torch.allclose(cost, cost_s, rtol=1e-12)
        lines += ["", f"(a, b) {n} / {n} points, gate {md} m; pairs per row min {int(npairs.min())} max {int(npairs.max())}", "",
                  "| K | variant | median ms per call | min | max |", "|---|---|---|---|---|"]
        for K in (1, 8, 64):
            Tk = T[:K].contiguous()
            single = [T[k].contiguous() for k in range(K)]

            def baseline():
                for t in single:
                    c.icp_refine(src, tgt, t, md, 1, -1.0)

            res = alternate([("yoho_eval_transforms", lambda: c.eval_transforms(src, tgt, Tk, md)),
                             (f"{K} x yoho_icp_refine(iters = 1)", baseline),
                             ("yoho_eval_transforms, source sorted by cell", lambda: c.eval_transforms(src_sorted, tgt, Tk, md))], args.repeats)
            for name, (med, lo, hi) in res.items():
                lines.append(f"| {K} | {name} | {med:.3f} | {lo:.3f} | {hi:.3f} |")
        H = 1000
        hyp = cu(rows[rs.randint(64, size=H)] + 0.01 * (rs.rand(H, 3, 4) - 0.5))
        counts = cu(rs.randint(0, 15, size=H).astype(np.int32))
        order = cu(rs.permutation(H).astype(np.int64))
        lines += ["", f"(c) yoho_verify_hypotheses, {n} / {n} points, H = {H}, distinct_tol 0.05", "", "| K | rows taken | median ms per call | min | max |",
                  "|---|---|---|---|---|"]
        for K in (8, 64):
            res = alternate([("v", lambda: c.verify_hypotheses(src, tgt, hyp, counts, K, md, order=order, distinct_tol=0.05))], args.repeats)
            info = c.verify_hypotheses(src, tgt, hyp, counts, K, md, order=order, distinct_tol=0.05)[5]
            med, lo, hi = res["v"]
            lines.append(f"| {K} | {int(info[0])} | {med:.3f} | {lo:.3f} | {hi:.3f} |")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
