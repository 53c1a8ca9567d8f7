"""Timings of the salient-keypoint entries (profiles/salient.md): a report, not a pass / fail.  The method is tools/time_disk.py's:
device events around `--repeats` back-to-back calls, five windows per case, the cases alternating; a thinning to the end is a chain
of calls with host reads between them, so it is timed by a host clock around work that ends in a synchronise.

  registers   csrc/salient.hip compiled with the flags of the build: VGPRs, scratch and occupancy of every kernel (needs no GPU)
  saliency    yoho_iss_saliency beside yoho_estimate_normals - the same walk - on seeded surface clouds of 20 k, 100 k and 300 k points
              at the radius that holds about 50 neighbours
  thin        yoho_disk_sample_prio with a constant priority beside yoho_disk_sample (the price of the 64-bit key), and
              keypoints._thin to the end in the order of the cloud's saliency (taken at twice the radius) with tiers None, 64, 8, 4 and 2:
              rounds, calls, ms
  extractor   yoho_extractor.run, wall ms per fragment on tools/bench_extract.py's cloud (300 k points, voxel 0.025) with keypoints="disk"
              at radius 0.074, without keypoint_saliency, with {} and with {"tiers": None}, alternating

    python tools/time_salient.py [--part registers|saliency|thin|extractor|all] [--out FILE]
    python tools/time_salient.py --part thin --lib other/libyoho_hip.so      # the same part on another build of the library

Every part (for saliency and thin: every cloud size) runs in a child process of its own under its own time limit, so a step that
hangs ends there and the parts behind it are not started."""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
SIZES = (20000, 100000, 300000)
LIMITS = {"registers": 300, "saliency": 240, "thin": 300, "extractor": 420}            # seconds per child


def cloud_and_radius(torch, c, synth, m):
    """time_disk.py's cloud and the radius that holds about 50 neighbours"""
    p = torch.from_numpy(synth.surface_cloud(m, seed=1, extent=3.0).astype(np.float32)).cuda()
    r = 0.1 * np.sqrt(100000 / m)
    for _ in range(3):
        mean = float(c.knn_within(p, p, r, 1, skip_same_row=True, want_idx=False, want_d2=False)[2].double().mean().item())
        r = float(r * np.sqrt(50.0 / max(mean, 1e-9)))
    mean = float(c.knn_within(p, p, r, 1, skip_same_row=True, want_idx=False, want_d2=False)[2].double().mean().item())
    return p, r, mean


def registers(args):
    from yoho_amd import build
    err = ""
    for src in ("salient.hip", "disk.hip"):              # the saliency kernel, and the thinning kernels of both entries (K = DkHashed, DkStored)
        cmd = [build._hipcc()] + build.FLAGS + build.EXTRA[src] + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                                                                  os.path.join(build.CSRC, src), "-o", os.devnull]
        err += subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    names = [m[0] + (f"<{m[1]}>" if m[1] else "") for m in re.findall(r"Function Name: \w*?((?:sl|dk)_\w+?_kernel)(?:I\w*?\d+(Dk\w+?)E)?\w*", err)]
    cols = [re.findall(rf"{k}: (\d+)", err) for k in (r"\bVGPRs", r"ScratchSize \[bytes/lane\]", r"Occupancy \[waves/SIMD\]")]
    lines = ["", "csrc/salient.hip and csrc/disk.hip, hipcc -O3 -ffp-contract=off, gfx950", "", "| kernel | VGPRs | scratch bytes per lane | waves per SIMD |", "|---|---|---|---|"]
    return lines + [f"| {n} | {v} | {s} | {o} |" for n, v, s, o in zip(names, *cols)]


def saliency(args):
    import torch
    from time_keypoints import shader_mhz, windows
    from yoho_amd import hip, synth
    c = hip.get_context()
    p, r, mean = cloud_and_radius(torch, c, synth, args.m)
    prio, count = c.iss_saliency(p, r)
    elig = int((~torch.isnan(prio)).sum().item())
    res = windows(torch, [("iss_saliency", lambda: c.iss_saliency(p, r)), ("iss_saliency, want_eig", lambda: c.iss_saliency(p, r, want_eig=True)),
                          ("estimate_normals", lambda: c.estimate_normals(p, r))], args.repeats)
    mhz = shader_mhz(torch, c)
    return [f"| {args.m} | {r:.5f} | {mean:.1f} | {elig} | " + " | ".join(f"{res[k][0]:.3f} ({res[k][1]:.3f} - {res[k][2]:.3f})" for k in res) + f" | {mhz:.0f} |"]


def thin(args):
    import torch
    from time_keypoints import shader_mhz, windows
    from yoho_amd import hip, keypoints, synth
    c = hip.get_context()
    p, r, mean = cloud_and_radius(torch, c, synth, args.m)
    const = torch.zeros((args.m,), dtype=torch.float32, device="cuda")
    a, na = c.disk_sample(p, r)
    b, nb = c.disk_sample_prio(p, r, const)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() and na.tolist() == nb.tolist()
    res = windows(torch, [("disk_sample", lambda: c.disk_sample(p, r)), ("disk_sample_prio, constant", lambda: c.disk_sample_prio(p, r, const))], args.repeats)
    mhz = shader_mhz(torch, c)
    out = [f"A | {args.m} | {r:.5f} | {mean:.1f} | {int(na[0])} | {int(na[1])} | " + " | ".join(f"{res[k][0]:.3f} ({res[k][1]:.3f} - {res[k][2]:.3f})" for k in res) + f" | {mhz:.0f} |"]
    prio = c.iss_saliency(p, 2 * r)[0]
    elig = int((~torch.isnan(prio)).sum().item())
    for tiers in (None, 64, 8, 4, 2):
        pt = prio if tiers is None else keypoints.tier_classes(prio, tiers)
        ms = []
        for _ in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows, info = keypoints._thin(c, p, r, 0, "time_salient", prio=pt)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        ms = sorted(ms[1:])
        out.append(f"B | {args.m} | {elig} | {tiers} | {info['kept']} | {info['rounds']} | {info['calls']} | {float(np.median(ms)):.2f} ({ms[0]:.2f} - {ms[-1]:.2f}) |")
    return out


def extractor(args):
    import torch
    from yoho_amd import hip, synth
    from yoho_amd import weights as W
    from yoho_amd.yoho_extract import yoho_extractor
    fsd = W.synth_state_dict(W.FCGF_SPEC, 3)
    ck = {"config": {"model": "ResUNetBN2C", "model_n_out": 32, "normalize_feature": True, "conv1_kernel_size": 7}, "state_dict": fsd}
    ex = yoho_extractor(fcgf_ckpt=ck, yoho_ckpt=W.synth_state_dict(W.PARTI_SPEC, 7), keypoints="disk", keypoint_radius=0.074)
    pc = synth.surface_cloud(300000, seed=1, extent=3.0)
    modes = (("disk", None), ("disk, keypoint_saliency={}", {}), ("disk, keypoint_saliency={\"tiers\": None}", {"tiers": None}))
    wall, n = {name: [] for name, _ in modes}, {}
    for rep in range(args.runs + 1):                     # the first call of a mode sizes the workspaces
        for name, sal in modes:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ex.keypoint_saliency = sal
            n[name] = len(ex.run(pc, voxel_size=0.025, nkpts=5000)[0])
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)
    lines = ["", f"yoho_extractor.run, tools/bench_extract.py's cloud (300 k points, voxel 0.025, nkpts 5000), keypoints=\"disk\" at radius 0.074: wall ms per fragment, "
             f"{args.runs} calls per mode after one untimed, the modes alternating", "", "| mode | median | min | max | keypoints returned |", "|---|---|---|---|---|"]
    for name, _ in modes:
        w = sorted(wall[name][1:])
        lines.append(f"| {name} | {float(np.median(w)):.2f} | {w[0]:.2f} | {w[-1]:.2f} | {n[name]} |")
    return lines


STEPS = {"registers": registers, "saliency": saliency, "thin": thin, "extractor": extractor}


def child(step, m, args):
    """one step in a process of its own under its time limit -> its lines; raises when it fails or runs out of time"""
    cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--m", str(m), "--repeats", str(args.repeats), "--runs", str(args.runs)]
    if args.lib:
        cmd += ["--lib", args.lib]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[step])
    if r.returncode != 0:
        raise SystemExit(f"time_salient.py: step {step} (m = {m}) failed with {r.returncode}; nothing more is started\n{r.stderr[-3000:]}")
    return [ln[2:] for ln in r.stdout.splitlines() if ln.startswith("> ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=tuple(STEPS) + ("all",), default="all")
    ap.add_argument("--step", choices=tuple(STEPS), default=None, help="internal: run one step in this process and print its lines")
    ap.add_argument("--m", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="load this build of libyoho_hip.so instead of the tree's")
    args = ap.parse_args()
    if args.lib:
        from yoho_amd import hip
        hip._LIB_PATH = args.lib = os.path.abspath(args.lib)
    if args.step:
        for ln in STEPS[args.step](args):
            print("> " + ln)
        return
    parts = tuple(STEPS) if args.part == "all" else (args.part,)
    lines = [f"library: {args.lib or 'of the tree'}"]
    if "registers" in parts:
        lines += child("registers", 0, args)
    if "saliency" in parts:
        lines += ["", "yoho_iss_saliency beside yoho_estimate_normals on synth.surface_cloud(m, seed=1, extent=3.0): median ms per call (min - max), device events "
                  f"around {args.repeats} back-to-back calls, 5 windows per case, the cases alternating", "",
                  "| points | radius | neighbours per row | eligible rows | iss_saliency | iss_saliency, want_eig | estimate_normals | shader MHz right after |", "|---|---|---|---|---|---|---|---|"]
        for m in SIZES:
            lines += child("saliency", m, args)
    if "thin" in parts:
        rows = [ln for m in SIZES for ln in child("thin", m, args)]
        lines += ["", "yoho_disk_sample_prio with a constant priority beside yoho_disk_sample, 16 rounds per call, seed 0 (the same bytes, asserted): median ms per call (min - max)", "",
                  "| points | radius | neighbours per row | kept | rounds that ran | disk_sample | disk_sample_prio, constant | shader MHz right after |", "|---|---|---|---|---|---|---|---|"]
        lines += [ln[2:] for ln in rows if ln.startswith("A ")]
        lines += ["", "keypoints._thin to the end in the order of the cloud's saliency (yoho_iss_saliency at twice the radius, default gammas), 16 rounds per call: host clock "
                  "around the calls and their host reads, median ms of 5 after one untimed (min - max)", "",
                  "| points | eligible rows | tiers | kept | rounds to the end | calls | ms |", "|---|---|---|---|---|---|---|"]
        lines += [ln[2:] for ln in rows if ln.startswith("B ")]
    if "extractor" in parts:
        lines += child("extractor", 0, args)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
