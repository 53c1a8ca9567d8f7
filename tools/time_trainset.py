"""Timings of the training-set generation (profiles/trainset.md):

  (a) yoho_radius_pairs at 5000 x 5000 with ~0.1 % and ~1 % of the pairs inside the radius, alternated in one process with the
      formulation it replaces run on the same device: (torch.norm(k0[:,None]-k1[None], dim=-1) < r).nonzero()  (YOHO_Trainset.py:57-61
      with its copy of the (N0,N1) matrix to the host left out, which favours it).  Context.radius_pairs as the driver calls it
      (a read of the count, a second call when 4 max(Na, Nb) pairs were not enough) and the entry alone with room for every pair.
  (b) trainset_create.PC_random_rot_feat per fragment (5 random rotations x 60 group elements, .npz written) beside
      testset_create.Feature_extracting per fragment (60 group elements, .npy written) on the same clouds in the same run.
  (c) batch assembly per pair: trainset() on a scene of `--pairs` pairs whose feature files exist (upload of the two (5,kn,32,60)
      blocks, labels, two gathers of 320 rows, 10 .pth items written), cold blocks and blocks resident in yoho_amd.store.

    python tools/time_trainset.py [--repeats 20] [--points 300000] [--keys 5000] [--fragments 3] [--out profiles/trainset_timings.md]

Host clock around work that ends in a device synchronise (every variant of (a) ends in a host read of its own); every variant warmed;
(a) alternates the variants `--repeats` times, one window = `--calls` calls.  The one speed condition - Context.radius_pairs' median below
the torch formulation's at both densities - is checked: the tool exits non-zero when it does not hold."""
import argparse
import os
import shutil
import sys
import tempfile
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from yoho_amd import hip, store, synth, weights as W  # noqa: E402


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def torch_pairs(k0, k1, r):
    return (torch.norm(k0[:, None, :] - k1[None, :, :], dim=-1) < r).nonzero()


def window_ms(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def alternate(variants, repeats, calls):
    for _, fn in variants:
        for _ in range(3):
            fn()
    times = {name: [] for name, _ in variants}
    for _ in range(repeats):
        for name, fn in variants:
            times[name].append(window_ms(fn, calls))
    return {name: (float(np.median(t)), min(t), max(t)) for name, t in times.items()}


def part_a(c, args, lines):
    """-> True when the speed condition held at every density"""
    import ctypes as C
    rs = np.random.RandomState(1)
    k0, k1 = cu(rs.rand(5000, 3).astype(np.float32)), cu(rs.rand(5000, 3).astype(np.float32))
    lib = c._lib
    held = True
    guess = 4 * max(k0.shape[0], k1.shape[0])          # Context.radius_pairs' first capacity
    for share, r in ((0.001, 0.0635), (0.01, 0.1395)):
        M = int(c.radius_pairs(k0, k1, r).shape[0])
        pairs = torch.empty((M, 2), dtype=torch.int64, device="cuda")
        count = torch.empty((1,), dtype=torch.int64, device="cuda")

        def entry():
            rc = lib.yoho_radius_pairs(c._h, C.c_void_p(k0.data_ptr()), 5000, C.c_void_p(k1.data_ptr()), 5000, r, C.c_void_p(pairs.data_ptr()), M,
                                       C.c_void_p(count.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0
            return int(count.item())
        res = alternate([("Context.radius_pairs", lambda: c.radius_pairs(k0, k1, r)), ("yoho_radius_pairs, capacity = M, count read", entry),
                         ("torch.norm + nonzero", lambda: torch_pairs(k0, k1, r))], args.repeats, args.calls)
        t = torch_pairs(k0, k1, r)
        g = c.radius_pairs(k0, k1, r)
        same = t.shape == g.shape and bool((t == g).all())
        lines.append("")
        lines.append(f"(a) 5000 x 5000, radius {r}: M = {M} pairs ({M / 25e6:.2%} of all; second call of the wrapper: {'yes' if M > guess else 'no'}); "
                     f"list identical to the torch formulation's: {same}" + ("" if same else f" (torch has {t.shape[0]})"))
        lines.append("")
        lines.append(f"| variant | median ms per call | min | max | windows x calls |")
        lines.append("|---|---|---|---|---|")
        for name, (med, lo, hi) in res.items():
            lines.append(f"| {name} | {med:.4f} | {lo:.4f} | {hi:.4f} | {args.repeats} x {args.calls} |")
        ours, theirs = res["Context.radius_pairs"][0], res["torch.norm + nonzero"][0]
        lines.append("")
        lines.append(f"speed condition (kernel path's median below the torch formulation's): {ours:.4f} < {theirs:.4f}: {ours < theirs}")
        held = held and ours < theirs
    return held


def part_b(args, lines):
    from yoho_amd.YOHO_testset import testset_create
    from yoho_amd.YOHO_Trainset import trainset_create
    fsd = W.synth_state_dict(W.FCGF_SPEC, 3)
    ck = {"config": {"model": "ResUNetBN2C", "model_n_out": 32, "normalize_feature": True, "conv1_kernel_size": 7}, "state_dict": fsd}
    clouds = [synth.surface_cloud(args.points, seed=1 + i, extent=3.0) for i in range(args.fragments)]
    rs = np.random.RandomState(0)
    kidx = [np.sort(rs.permutation(len(cl))[:args.keys]) for cl in clouds]

    class DS:
        name = "synth/room"
        pc_ids = [str(i) for i in range(args.fragments)]
        pair_ids = []
        get_pc = staticmethod(lambda i: clouds[int(i)])
        get_kps = staticmethod(lambda i: clouds[int(i)][kidx[int(i)]])

    lines.append("")
    lines.append(f"(b) {args.fragments} fragments of {args.points} points, {args.keys} keys, voxel 0.025, two backbone lanes; host clock around the whole stage "
                 "(reading ahead, passes, copy, file written), first round = warm-up (workspaces grow)")
    lines.append("")
    lines.append("| round | testset_create.Feature_extracting ms per fragment | trainset_create.PC_random_rot_feat ms per fragment | ratio |")
    lines.append("|---|---|---|---|")
    for rnd in range(3):
        tmp = tempfile.mkdtemp(prefix="yoho_trainset_")
        try:
            cfg = types.SimpleNamespace(model=ck, voxel_size=0.025, dataset="synth", datasetname="synth", output_dir=tmp, origin_dir=tmp,
                                        datasets={"wholesetname": "synth", "valscenes": [], "room": DS()})
            tt = testset_create(cfg)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            tt.Feature_extracting()
            torch.cuda.synchronize(); t_test = (time.perf_counter() - t0) / args.fragments * 1e3
            tc = trainset_create(cfg)
            os.makedirs(f"{tmp}/Filtered_Keys/synth/room")
            for i in range(args.fragments):
                np.save(f"{tmp}/Filtered_Keys/synth/room/{i}_index.npy", kidx[i])
            torch.cuda.synchronize(); t0 = time.perf_counter()
            tc.PC_random_rot_feat()
            torch.cuda.synchronize(); t_train = (time.perf_counter() - t0) / args.fragments * 1e3
            lines.append(f"| {rnd}{' (warm-up)' if rnd == 0 else ''} | {t_test:.1f} | {t_train:.1f} | {t_train / t_test:.2f} |")
        finally:
            shutil.rmtree(tmp)


def part_c(c, args, lines):
    from yoho_amd.YOHO_Trainset import trainset_create
    kn, nfrag = args.keys, args.pairs + 1
    rs = np.random.RandomState(2)
    base = rs.rand(kn, 3)
    keys = [base + 0.008 * rs.randn(kn, 3) for _ in range(nfrag)]

    class DS:
        name = "synth/room"
        pc_ids = [str(i) for i in range(nfrag)]
        pair_ids = [(str(i), str(i + 1)) for i in range(args.pairs)]
        get_kps = staticmethod(lambda i: keys[int(i)])
        get_transform = staticmethod(lambda a, b: np.eye(4, dtype=np.float32)[:3])

    tmp = tempfile.mkdtemp(prefix="yoho_trainset_")
    try:
        os.makedirs(f"{tmp}/Rotated_Features/synth/room")
        os.makedirs(f"{tmp}/Pairs_0.03/synth/room")
        from yoho_amd.utils import random_rotation_matrix
        for i in range(nfrag):
            Rs = np.stack([random_rotation_matrix(5 * i + r) for r in range(5)])
            np.savez(f"{tmp}/Rotated_Features/synth/room/{i}_feats.npz", Rs=Rs, feats=rs.rand(5, kn, 32, 60).astype(np.float32))
        ncorr = []
        for a, b in DS.pair_ids:
            p = c.radius_pairs(cu(keys[int(a)].astype(np.float32)), cu(keys[int(b)].astype(np.float32)), 0.02).cpu().numpy()
            np.save(f"{tmp}/Pairs_0.03/synth/room/{a}-{b}.npy", p)
            ncorr.append(len(p))
        cfg = types.SimpleNamespace(model=None, voxel_size=0.025, datasetname="synth", output_dir=tmp, origin_dir=tmp,
                                    datasets={"wholesetname": "synth", "valscenes": [], "room": DS()})
        lines.append("")
        lines.append(f"(c) trainset() on {args.pairs} pairs of fragments with {kn} filtered keys ({5 * kn * 32 * 60 * 4 / 1e6:.0f} MB per feature block, {min(ncorr)}-{max(ncorr)} correspondences "
                     "per pair): labels, 2 x yoho_trainset_gather of 320 rows, 10 items written per pair; host clock around the whole call")
        lines.append("")
        lines.append("| run | ms per pair |")
        lines.append("|---|---|")
        tc = trainset_create(cfg, ctx=c)
        store.clear()
        for run in ("blocks read from disk and uploaded (first run)", "blocks resident in yoho_amd.store", "blocks resident in yoho_amd.store (again)"):
            shutil.rmtree(f"{tmp}/Train_val_list", ignore_errors=True)
            np.random.seed(0)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            tc.trainset()
            torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / args.pairs * 1e3
            lines.append(f"| {run} | {dt:.1f} |")
        # the gather alone
        _, f_d = tc._block("synth/room", "0")
        rot, key = rs.randint(0, 5, 320), rs.randint(0, kn, 320)
        for _ in range(3):
            c.trainset_gather(f_d, rot, key)
        g = window_ms(lambda: c.trainset_gather(f_d, rot, key), 200)
        lines.append("")
        lines.append(f"yoho_trainset_gather alone, 320 rows of 7680 B: {g * 1e3:.1f} us per call (host clock over 200 calls, output allocation included)")
    finally:
        shutil.rmtree(tmp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10, help="calls per timed window of (a)")
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--keys", type=int, default=5000)
    ap.add_argument("--fragments", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--only", default="abc")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_trainset.py measures on the GPU; there is none here")
    c = hip.get_context()
    lines = [f"device: {torch.cuda.get_device_name(0)}"]
    held = True
    if "a" in args.only:
        held = part_a(c, args, lines)
    if "b" in args.only:
        part_b(args, lines)
    if "c" in args.only:
        part_c(c, args, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if not held:
        raise SystemExit("the speed condition of yoho_radius_pairs does not hold: its median is not below the torch formulation's")


if __name__ == "__main__":
    main()
