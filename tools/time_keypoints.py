"""Timings of farthest-point sampling (profiles/keypoints.md): a report, not a pass / fail.

  kernels     yoho_fps on seeded surface clouds, k = 5000: the one-workgroup path at m = FPS_ONE_WG_MAX (and half of it), the per-pick
              path at the same m - the figure FPS_ONE_WG_MAX is chosen by - and at 30 k, 100 k and 300 k points; device events around
              `--repeats` back-to-back calls, five windows per case, the cases alternating; beside it the host time the per-pick path's
              call takes to return (its k launches queued) from an idle stream
  extractor   yoho_extractor.run, wall ms per fragment on the cloud of bench.py's fcgf leg (300 k points, 5000 keypoints, voxel 0.025)
              with keypoints="random" and "fps", the two alternating, and the coverage radius both leave on the voxel-sampled cloud

    python tools/time_keypoints.py [--part kernels|extractor|all] [--out FILE]
    python tools/time_keypoints.py --part extractor --modes random --repo OTHER_CHECKOUT      # the same leg of another (built) checkout

The last form is how the parent commit's "random" figure is taken on the same box: it imports yoho_amd from OTHER_CHECKOUT and passes
no keypoint option, so it runs on a tree that has none."""
import argparse
import os
import sys
import time

import numpy as np


def windows(torch, calls, repeats, rounds=5):
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


def shader_mhz(torch, ctx):
    t = ctx.clock_probe(50)
    torch.cuda.synchronize()
    t = [int(v) for v in t.cpu()]
    return t[0] / t[1] * t[2] / 1000 if t[1] else float("nan")


def kernels(torch, hip, synth, args, lines):
    c = hip.get_context()
    k = args.k
    cases, enq = [], []
    for m, paths in ((hip.FPS_ONE_WG_MAX // 2, ("one_wg", "per_pick")), (hip.FPS_ONE_WG_MAX, ("one_wg", "per_pick")), (30000, ("per_pick",)),
                     (100000, ("per_pick",)), (300000, ("per_pick",))):
        p = torch.from_numpy(synth.surface_cloud(m, seed=1, extent=3.0).astype(np.float32)).cuda()
        outs = {path: c.fps(p, k, path=path) for path in paths}
        torch.cuda.synchronize()
        first = [x.cpu().numpy().tobytes() for x in outs[paths[0]]]
        for path in paths[1:]:
            assert [x.cpu().numpy().tobytes() for x in outs[path]] == first, (m, path)
        for path in paths:
            cases.append((f"{path}, m = {m}", lambda p=p, path=path: c.fps(p, k, path=path)))
        if "per_pick" in paths:                          # host time until the call returns, from an idle stream
            ts = []
            for _ in range(7):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                c.fps(p, k, path="per_pick")
                ts.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            enq.append((m, float(np.median(ts)), min(ts), max(ts)))
    res = windows(torch, cases, args.repeats)
    mhz = shader_mhz(torch, c)
    lines += ["", f"yoho_fps, k = {k}, device events around {args.repeats} back-to-back calls, 5 windows per case (shader clock right after: {mhz:.0f} MHz)", "",
              "| path, points | median ms per call | min | max | us per pick |", "|---|---|---|---|---|"]
    for name, (med, lo, hi) in res.items():
        lines.append(f"| {name} | {med:.3f} | {lo:.3f} | {hi:.3f} | {1e3 * med / k:.2f} |")
    lines += ["", f"host time until the per-pick call returns ({k} launches queued from an idle stream), 7 calls", "",
              "| points | median ms | min | max | us per launch |", "|---|---|---|---|---|"]
    for m, med, lo, hi in enq:
        lines.append(f"| {m} | {med:.3f} | {lo:.3f} | {hi:.3f} | {1e3 * med / k:.2f} |")


def extractor(torch, hip, synth, W, args, lines):
    from yoho_amd.yoho_extract import yoho_extractor
    fsd = W.synth_state_dict(W.FCGF_SPEC, 3)
    ck = {"config": {"model": "ResUNetBN2C", "model_n_out": 32, "normalize_feature": True, "conv1_kernel_size": 7}, "state_dict": fsd}
    sd1 = W.synth_state_dict(W.PARTI_SPEC, 7)
    pc = synth.surface_cloud(300000, seed=1, extent=3.0)
    # ONE extractor, its mode switched between calls: two extractors would take turns loading their weights into the process-wide
    # library context, a second per call that no user pays (on a checkout without the option the attribute is simply never read)
    ex = yoho_extractor(fcgf_ckpt=ck, yoho_ckpt=sd1)
    wall = {mode: [] for mode in args.modes}
    kpts = {}
    for rep in range(args.runs + 1):                     # the first call of a mode sizes the workspaces
        for mode in args.modes:
            np.random.seed(rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ex.keypoints = mode
            kpts[mode] = ex.run(pc, voxel_size=0.025, nkpts=args.k)[0]
            torch.cuda.synchronize()
            wall[mode].append((time.perf_counter() - t0) * 1e3)
    c = hip.get_context()
    mhz = shader_mhz(torch, c)
    radius, ncand = {}, ""
    if hasattr(hip.Context, "fps"):
        from yoho_amd import keypoints as KP
        _, cand = KP.candidates(c, torch.from_numpy(pc).cuda(), 0.025)
        ncand = f"; {cand.shape[0]} candidates"
        for mode in args.modes:
            radius[mode] = KP.coverage_radius(c, cand, torch.from_numpy(kpts[mode].astype(np.float32)).cuda())
    lines += ["", f"yoho_extractor.run, 300 k-point cloud of bench.py's fcgf leg, nkpts = {args.k}, voxel 0.025: wall ms per fragment, {args.runs} calls per mode "
              f"after one untimed, the modes alternating (shader clock right after: {mhz:.0f} MHz); tree: {args.repo or 'this one'}{ncand}", "",
              "| keypoints | median | min | max | coverage radius on the voxel-sampled cloud |", "|---|---|---|---|---|"]
    for mode in args.modes:
        w = sorted(wall[mode][1:])
        lines.append(f"| {mode} | {float(np.median(w)):.2f} | {w[0]:.2f} | {w[-1]:.2f} | {radius[mode]:.4f} |" if mode in radius else
                     f"| {mode} | {float(np.median(w)):.2f} | {w[0]:.2f} | {w[-1]:.2f} | |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernels", "extractor", "all"), default="all")
    ap.add_argument("--modes", nargs="*", default=["random", "fps"])
    ap.add_argument("--k", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--repo", default=None, help="import yoho_amd from this (built) checkout instead of the one the tool lies in")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo) if args.repo else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from yoho_amd import hip, synth
    from yoho_amd import weights as W
    if not torch.cuda.is_available():
        raise SystemExit("time_keypoints.py measures on the GPU; there is none here")
    lines = [f"device: {torch.cuda.get_device_name(0)}"]
    if args.part in ("kernels", "all"):
        kernels(torch, hip, synth, args, lines)
    if args.part in ("extractor", "all"):
        extractor(torch, hip, synth, W, args, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
