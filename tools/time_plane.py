"""Timings of the normals / point-to-plane entries (profiles/plane_icp.md): a report, not a pass / fail.

  (a) yoho_estimate_normals at 20 000 points (radius 0.06 m) and 300 000 points of a 3 m scene (radius 0.03 m), per call.
  (b) yoho_icp_plane beside yoho_icp_refine at 20 000 / 20 000 and 300 000 / 300 000 points, gate 0.1 m, `--iters` iterations with
      tol < 0 (every iteration is made), per call and per iteration, alternated in one process.

    python tools/time_plane.py [--repeats 10] [--iters 30] [--out FILE]        # the tables it prints go into profiles/plane_icp.md
    python tools/time_plane.py --lib other/libyoho_hip.so                      # the same on another build of the library

The inputs are the tests' own (tests/refine_ref.py icp_case; the large pair is tools/time_refine.py's).  Host clock around work that
ends in a device synchronise; every variant warmed twice; the variants alternate `--repeats` times; median and [min, max]."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from yoho_amd import hip, synth  # noqa: E402
import refine_ref as RR  # noqa: E402
from time_refine import alternate, cu  # noqa: E402


def pair_of(n):
    if n <= 50000:
        return RR.icp_case(n=n, seed=3), 0.06
    pc = synth.surface_cloud(n, seed=3, extent=3.0)
    small = RR.icp_case(n=1000, seed=3)
    T_gt = small["T_gt"]
    return {"src": np.ascontiguousarray((pc - T_gt[:, 3]) @ T_gt[:, :3], np.float32), "tgt": np.ascontiguousarray(pc, np.float32), "T_gt": T_gt,
            "T0": small["T0"], "max_dist": 0.1}, 0.03


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--sizes", type=int, nargs="*", default=[20000, 300000])
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="load this build of libyoho_hip.so instead of the tree's")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_plane.py measures on the GPU; there is none here")
    if args.lib:
        hip._LIB_PATH = os.path.abspath(args.lib)
    c = hip.get_context()
    lines = [f"device: {torch.cuda.get_device_name(0)}; library {hip._LIB_PATH if args.lib else 'of the tree'}"]
    for n in args.sizes:
        ic, radius = pair_of(n)
        src, tgt, T0, md, gt = cu(ic["src"]), cu(ic["tgt"]), cu(ic["T0"]), ic["max_dist"], ic["T_gt"]
        res = alternate([(f"yoho_estimate_normals, radius {radius}", lambda: c.estimate_normals(tgt, radius))], args.repeats)
        nrm, cnt = c.estimate_normals(tgt, radius)
        cnt_h = cnt.cpu().numpy()
        lines += ["", f"(a) normals at {n} points: neighbours min {cnt_h.min()} median {int(np.median(cnt_h))} max {cnt_h.max()}, "
                      f"{int((nrm == 0).all(dim=1).sum())} invalid", "", "| variant | median ms per call | min | max |", "|---|---|---|---|"]
        for name, (med, lo, hi) in res.items():
            lines.append(f"| {name} | {med:.3f} | {lo:.3f} | {hi:.3f} |")
        res = alternate([("yoho_icp_plane", lambda: c.icp_plane(src, tgt, nrm, T0, md, args.iters, -1.0)),
                         ("yoho_icp_refine", lambda: c.icp_refine(src, tgt, T0, md, args.iters, -1.0))], args.repeats)
        T_pl, npairs, rmse, _ = c.icp_plane(src, tgt, nrm, T0, md, args.iters, -1.0)
        T_pt = c.icp_refine(src, tgt, T0, md, args.iters, -1.0)[0]
        e_pl, e_pt = RR.rot_error_deg(gt[:, :3], T_pl.cpu().numpy()[:, :3]), RR.rot_error_deg(gt[:, :3], T_pt.cpu().numpy()[:, :3])
        lines += ["", f"(b) ICP at {n} / {n} points, gate {md} m, {args.iters} iterations: pairs {int(npairs[0])} -> {int(npairs[-1])}, point-to-plane rms "
                      f"{float(rmse[0]):.5f} -> {float(rmse[-1]):.2e}; rotation error after the run {e_pl:.2e} degrees (point-to-point: {e_pt:.2e})", "",
                  "| variant | median ms per call | per iteration | min | max |", "|---|---|---|---|---|"]
        for name, (med, lo, hi) in res.items():
            lines.append(f"| {name} | {med:.3f} | {med / args.iters:.4f} | {lo:.3f} | {hi:.3f} |")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
