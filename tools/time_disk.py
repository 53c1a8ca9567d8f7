"""Timings of the Poisson-disk thinning (profiles/disk.md): a report, not a pass / fail.  The method is tools/time_keypoints.py's.

  entry       yoho_disk_sample on seeded surface clouds of 20 k, 100 k and 300 k points at the radius that holds about 50 neighbours
              (found on the device with the count-only yoho_knn_within call), with Context.disk_sample's default rounds and with
              YOHO_DISK_MAX_ROUNDS; beside it that count-only call in the same windows - one grid build and one walk, the floor of
              anything built on them; device events around `--repeats` back-to-back calls, five windows per case, the cases
              alternating.  The rounds the device reports (n_out[1]) and the share of round launches that found nothing to do
  extractor   yoho_extractor.run, wall ms per fragment on the cloud of bench.py's fcgf leg (300 k points, 5000 keypoints, voxel 0.025)
              with keypoints="random", "fps" and "disk" - at the radius keypoints.disk_radius finds for 5000 keypoints on that
              cloud -, the modes alternating, and the coverage radius each leaves on the voxel-sampled cloud

    python tools/time_disk.py [--part entry|extractor|all] [--out FILE]
    python tools/time_disk.py --part extractor --modes random --repo OTHER_CHECKOUT      # the same leg of another (built) checkout
    python tools/time_disk.py --part entry --lib other/libyoho_hip.so                    # this tree's Python over another build of the library

The last form is how the parent commit's figures are taken on the same box, in processes of its own before and between."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_keypoints import shader_mhz, windows  # noqa: E402


def entry(torch, hip, synth, args, lines):
    c = hip.get_context()
    cases, rows = [], []
    for m in (20000, 100000, 300000):
        p = torch.from_numpy(synth.surface_cloud(m, seed=1, extent=3.0).astype(np.float32)).cuda()
        r = 0.1 * np.sqrt(100000 / m)
        for _ in range(3):                               # count ~ r^2 on a surface: two corrections land within a few per cent of 50
            mean = float(c.knn_within(p, p, r, 1, skip_same_row=True, want_idx=False, want_d2=False)[2].double().mean().item())
            r = float(r * np.sqrt(50.0 / max(mean, 1e-9)))
        mean = float(c.knn_within(p, p, r, 1, skip_same_row=True, want_idx=False, want_d2=False)[2].double().mean().item())
        state, n = c.disk_sample(p, r, rounds=hip.DISK_MAX_ROUNDS)
        kept, ran, left = (int(v) for v in n.tolist())
        assert left == 0, (m, n.tolist())
        d = c.disk_sample(p, r)                          # the default rounds: the same bytes when they suffice
        assert int(d[1][2]) > 0 or d[0].cpu().numpy().tobytes() == state.cpu().numpy().tobytes()
        rows.append((m, r, mean, kept, ran, int(d[1][2])))
        cases.append((f"disk_sample, rounds = {hip.DISK_DEFAULT_ROUNDS}, m = {m}", lambda p=p, r=r: c.disk_sample(p, r)))
        cases.append((f"disk_sample, rounds = {hip.DISK_MAX_ROUNDS}, m = {m}", lambda p=p, r=r: c.disk_sample(p, r, rounds=hip.DISK_MAX_ROUNDS)))
        cases.append((f"knn_within, count only, m = {m}", lambda p=p, r=r: c.knn_within(p, p, r, 1, skip_same_row=True, want_idx=False, want_d2=False)))
    res = windows(torch, cases, args.repeats)
    mhz = shader_mhz(torch, c)
    lines += ["", "yoho_disk_sample on synth.surface_cloud(m, seed=1, extent=3.0), seed 0", "",
              f"| points | radius | neighbours per row | kept | rounds that ran (n_out[1]) | undecided after {hip.DISK_DEFAULT_ROUNDS} rounds | empty round launches of "
              f"{hip.DISK_DEFAULT_ROUNDS} | of {hip.DISK_MAX_ROUNDS} |", "|---|---|---|---|---|---|---|---|"]
    for m, r, mean, kept, ran, left in rows:
        lines.append(f"| {m} | {r:.5f} | {mean:.1f} | {kept} | {ran} | {left} | {max(0, hip.DISK_DEFAULT_ROUNDS - ran)} ({max(0, hip.DISK_DEFAULT_ROUNDS - ran) / hip.DISK_DEFAULT_ROUNDS:.0%}) | "
                     f"{hip.DISK_MAX_ROUNDS - ran} ({(hip.DISK_MAX_ROUNDS - ran) / hip.DISK_MAX_ROUNDS:.0%}) |")
    lines += ["", f"device events around {args.repeats} back-to-back calls, 5 windows per case, the cases alternating (shader clock right after: {mhz:.0f} MHz)", "",
              "| call | median ms per call | min | max |", "|---|---|---|---|"]
    for name, (med, lo, hi) in res.items():
        lines.append(f"| {name} | {med:.3f} | {lo:.3f} | {hi:.3f} |")


def extractor(torch, hip, synth, W, args, lines):
    from yoho_amd.yoho_extract import yoho_extractor
    fsd = W.synth_state_dict(W.FCGF_SPEC, 3)
    ck = {"config": {"model": "ResUNetBN2C", "model_n_out": 32, "normalize_feature": True, "conv1_kernel_size": 7}, "state_dict": fsd}
    sd1 = W.synth_state_dict(W.PARTI_SPEC, 7)
    pc = synth.surface_cloud(300000, seed=1, extent=3.0)
    c = hip.get_context()
    # ONE extractor, its mode switched between calls (tools/time_keypoints.py says why)
    ex = yoho_extractor(fcgf_ckpt=ck, yoho_ckpt=sd1)
    note = ""
    if "disk" in args.modes:
        from yoho_amd import keypoints as KP
        _, cand = KP.candidates(c, torch.from_numpy(pc).cuda(), 0.025)
        r, _, info = KP.disk_radius(c, cand, args.k, 0.1)
        ex.keypoint_radius, ex.keypoint_seed = r, 0
        note = f"; \"disk\" at radius {r:.5f} (keypoints.disk_radius from 0.1: {info['kept']} kept in {info['rounds']} rounds, {info['calls']} call)"
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
    mhz = shader_mhz(torch, c)
    radius, ncand = {}, ""
    if hasattr(hip.Context, "fps"):
        from yoho_amd import keypoints as KP
        _, cand = KP.candidates(c, torch.from_numpy(pc).cuda(), 0.025)
        ncand = f"; {cand.shape[0]} candidates"
        for mode in args.modes:
            radius[mode] = KP.coverage_radius(c, cand, torch.from_numpy(kpts[mode].astype(np.float32)).cuda())
    lines += ["", f"yoho_extractor.run, 300 k-point cloud of bench.py's fcgf leg, nkpts = {args.k}, voxel 0.025: wall ms per fragment, {args.runs} calls per mode "
              f"after one untimed, the modes alternating (shader clock right after: {mhz:.0f} MHz); tree: {args.repo or 'this one'}{ncand}{note}", "",
              "| keypoints | median | min | max | keypoints returned | coverage radius on the voxel-sampled cloud |", "|---|---|---|---|---|---|"]
    for mode in args.modes:
        w = sorted(wall[mode][1:])
        lines.append(f"| {mode} | {float(np.median(w)):.2f} | {w[0]:.2f} | {w[-1]:.2f} | {len(kpts[mode])} | {radius[mode]:.4f} |" if mode in radius else
                     f"| {mode} | {float(np.median(w)):.2f} | {w[0]:.2f} | {w[-1]:.2f} | {len(kpts[mode])} | |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("entry", "extractor", "all"), default="all")
    ap.add_argument("--modes", nargs="*", default=["random", "fps", "disk"])
    ap.add_argument("--k", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--repo", default=None, help="import yoho_amd from this (built) checkout instead of the one the tool lies in")
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="load this build of libyoho_hip.so instead of the tree's")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo) if args.repo else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from yoho_amd import hip, synth
    from yoho_amd import weights as W
    if not torch.cuda.is_available():
        raise SystemExit("time_disk.py measures on the GPU; there is none here")
    if args.lib:
        hip._LIB_PATH = os.path.abspath(args.lib)
    lines = [f"device: {torch.cuda.get_device_name(0)}; library {hip._LIB_PATH if args.lib else 'of the tree'}"]
    if args.part in ("entry", "all"):
        entry(torch, hip, synth, args, lines)
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
