"""CPU tests of the training-set generation: the contract of yoho_radius_pairs (tests/trainset_ref.py) against the reference's own
pair lists, the host labels and the random-stream consumption of yoho_amd.YOHO_Trainset against the reference's own run
(tests/golden/trainset.npz, written by tools/gen_golden_trainset.py on the set of tests/trainset_fixture.py), the fixture against a
fresh run of the reference where its tree exists, and the symbols of include/yoho_trainset.h."""
import os
import pickle
import random
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import trainset_ref as TR  # noqa: E402
import trainset_fixture as TF  # noqa: E402


@pytest.fixture(scope="module")
def ts():
    return TF.build_dataset()


def host_creator(ts, tables, out_dir, origin=None):
    """a trainset_create without a device context: the host stages only"""
    from yoho_amd.YOHO_Trainset import trainset_create
    tc = object.__new__(trainset_create)
    tc.config = types.SimpleNamespace()
    tc.dataset_name = TF.NAME
    tc.output_dir = str(out_dir)
    tc.datasets = ts.datasets()
    tc.valscenes = tc.datasets["valscenes"]
    tc.Rgroup = tables.R64
    tc.stats = {}
    return patch_device_hooks(tc, out_dir)


def patch_device_hooks(tc, out_dir):
    """the two places where trainset() / valset() touch the device, replaced on the object by numpy; every gather is recorded"""
    tc.gathers = []

    def gather(feats, rot, key, stream):
        tc.gathers.append((np.array(rot), np.array(key)))
        return torch.from_numpy(feats[np.asarray(rot), np.asarray(key)])

    def block(name, pc_id):
        with np.load(f"{out_dir}/Rotated_Features/{name}/{pc_id}_feats.npz") as z:
            return z["Rs"], z["feats"]
    tc._gather_to_host, tc._block = gather, block
    return tc


def write_stage_files(ts, g, out_dir):
    """Pairs_0.03 and Rotated_Features as the earlier stages leave them, from the fixture"""
    for scene, d in ts.scenes.items():
        os.makedirs(f"{out_dir}/Pairs_0.03/{d.name}", exist_ok=True)
        for p0, p1 in d.pair_ids:
            np.save(f"{out_dir}/Pairs_0.03/{d.name}/{p0}-{p1}.npy", g[f"{scene}_{p0}-{p1}_pairs"].astype(np.int64))
    ts.write_rotated_features(out_dir, lambda scene, pc_id: g[f"{scene}_{pc_id}_Rs"])


def test_ref_reproduces_every_reference_pair_list(ts, gold):
    """the f32 contract equals torch.norm + np.where of the reference on every pair of the fixture, order included (the generator
    asserts that no f64 distance is within 1e-5 relative of the threshold)"""
    g = gold("trainset.npz")
    n = 0
    for scene, d in ts.scenes.items():
        for pc_id in d.pc_ids:
            assert np.array_equal(g[f"{scene}_{pc_id}_ok"], ts.ok_index(scene, pc_id))
        for p0, p1 in d.pair_ids:
            k0 = d.get_kps(p0)[ts.ok_index(scene, p0)].astype(np.float32)
            k1 = d.get_kps(p1)[ts.ok_index(scene, p1)].astype(np.float32)
            want = g[f"{scene}_{p0}-{p1}_pairs"]
            assert np.array_equal(TR.radius_pairs_ref(k0, k1, 0.02), want), (scene, p0, p1)
            assert np.array_equal(TR.radius_pairs_ref(k0, k1, 0.02, rows_per_block=7), want)
            n += len(want)
    assert n > 300


def test_ref_threshold_band_and_order():
    """the helper itself: the band of threshold_points straddles the radius ulp by ulp, pairs are strict (`<`), NaN never pairs"""
    for r in (0.02, 0.5, 3.0):
        pts = TR.threshold_points(r, 64)
        assert pts[32, 0] == np.float32(r) and (np.diff(pts[:, 0]) > 0).all()
        p = TR.radius_pairs_ref(np.zeros((1, 3), np.float32), pts, r)
        assert 0 < len(p) < 64 and (p[:, 0] == 0).all() and (np.diff(p[:, 1]) == 1).all()
        x = pts[:, 0]
        assert np.array_equal(p[:, 1], np.where(np.sqrt(x * x) < np.float32(r))[0])
    a = np.array([[0, 0, 0], [np.nan, 0, 0], [1, 0, 0]], np.float32)
    assert TR.radius_pairs_ref(a, a, 1.0).tolist() == [[0, 0], [2, 2]]
    assert TR.radius_pairs_ref(a, a, 1.5).tolist() == [[0, 0], [0, 2], [2, 0], [2, 2]]
    assert TR.radius_pairs_ref(a, a, 0.0).shape == (0, 2) and TR.radius_pairs_ref(a[:0], a, 1.0).shape == (0, 2)


def test_host_labels_equal_the_reference(ts, gold, tables, tmp_path):
    """R2DR_id / DeltaR over the 25 rotations of every pair: true_idx exactly; deltaR and R within 1e-6 absolute (the project's f32
    standard: the f64 eigenvectors of two LAPACK builds differ by ~1e-15, what is left is one f32 rounding)"""
    g = gold("trainset.npz")
    tc = host_creator(ts, tables, tmp_path)
    for scene, d in ts.scenes.items():
        for p0, p1 in d.pair_ids:
            R, idx, dR = tc.pair_labels(g[f"{scene}_{p0}_Rs"], g[f"{scene}_{p1}_Rs"], d.get_transform(p0, p1)[0:3, 0:3])
            assert np.array_equal(idx, g[f"{scene}_{p0}-{p1}_true_idx"]), (scene, p0, p1)
            assert np.abs(dR - g[f"{scene}_{p0}-{p1}_deltaR"]).max() <= 1e-6
            assert np.abs(R - g[f"{scene}_{p0}-{p1}_R"]).max() <= 1e-6
            assert tc.R2DR_id(R[2, 3]) == idx[2, 3] and np.abs(tc.DeltaR(R[2, 3], idx[2, 3]) - dR[2, 3]).max() <= 1e-12
    # a group element itself is its own nearest element, with the identity as the residual
    for gi in (0, 17, 59):
        assert tc.R2DR_id(tables.R64[gi]) == gi
        assert np.abs(np.abs(tc.DeltaR(tables.R64[gi], gi)) - [1, 0, 0, 0]).max() < 1e-7


def test_random_rotation_matrix_and_R_diff(gold, tables):
    from yoho_amd.utils import random_rotation_matrix, compute_R_diff, group_R_diff
    g = gold("trainset.npz")
    for s in range(4):
        R = random_rotation_matrix(seed=s)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1) < 1e-14
        assert np.abs(R - g["rrm"][s]).max() <= 1e-15, s
    st = np.random.get_state()[1].copy()
    a, b = random_rotation_matrix(), random_rotation_matrix()
    assert np.abs(a - b).max() > 1e-6                              # unseeded: two calls differ ...
    assert np.array_equal(np.random.get_state()[1], st)           # ... and the global stream is not consumed
    Rs = np.stack([random_rotation_matrix(seed=s) for s in range(6)])
    D = group_R_diff(tables.R64, Rs)
    one = np.array([[compute_R_diff(tables.R64[gi], R) for gi in range(60)] for R in Rs])
    assert D.shape == (6, 60) and np.abs(D - one).max() < 1e-9
    assert abs(compute_R_diff(np.eye(3), tables.R64[0] @ tables.R64[0].T)) < 1e-5
    c = np.cos(np.deg2rad(30.0)); s_ = np.sin(np.deg2rad(30.0))
    assert abs(compute_R_diff(np.eye(3), np.array([[c, -s_, 0], [s_, c, 0], [0, 0, 1.0]])) - 30.0) < 1e-9


def test_trainset_consumes_the_random_stream_as_the_reference(ts, gold, tables, tmp_path):
    """trainset() with the device gather replaced by numpy: the drawn (pps, Index_i, Index_j) of all 40 batches, train.pkl /
    train_pcp.pkl and every item equal the reference's run under the same seed"""
    g = gold("trainset.npz")
    write_stage_files(ts, g, tmp_path)
    tc = host_creator(ts, tables, tmp_path)
    np.random.seed(TF.SEED_NP)
    random.seed(TF.SEED_PY)
    tc.trainset()
    pcp = pickle.load(open(f"{tmp_path}/Train_val_list/train_pcp.pkl", "rb"))
    want = list(zip(g["train_pcp_name"].tolist(), g["train_pcp_pc0"].tolist(), g["train_pcp_pc1"].tolist(), g["train_pcp_i"].tolist()))
    assert pcp == want and len(pcp) == 40
    assert pickle.load(open(f"{tmp_path}/Train_val_list/train.pkl", "rb")) == list(range(40))
    assert ("synth_train/edge", "0", "1", 0) in pcp and not any(t[:3] == ("synth_train/edge", "0", "2") for t in pcp)      # the repeat branch is in, the pair of 7 is not
    # what was drawn, read off the gathers: per pair one call per side with (Index_i, pps[:, 0]) and (Index_j, pps[:, 1]) of its 10 batches
    assert len(tc.gathers) == 2 * 4 and all(r.shape == k.shape == (320,) for r, k in tc.gathers)
    Ii = np.concatenate([tc.gathers[2 * n][0] for n in range(4)]).reshape(40, 32)
    Ij = np.concatenate([tc.gathers[2 * n + 1][0] for n in range(4)]).reshape(40, 32)
    pps = np.stack([np.concatenate([tc.gathers[2 * n][1] for n in range(4)]), np.concatenate([tc.gathers[2 * n + 1][1] for n in range(4)])], 1).reshape(40, 32, 2)
    assert np.array_equal(pps, g["train_pps"]) and np.array_equal(Ii, g["train_Ii"]) and np.array_equal(Ij, g["train_Ij"])
    TF.check_train_items(tmp_path, g)
    # complete: a second call draws nothing and writes nothing
    st = np.random.get_state()[1].copy()
    mt = os.stat(f"{tmp_path}/Train_val_list/trainset/0.pth").st_mtime_ns
    tc.trainset()
    assert np.array_equal(np.random.get_state()[1], st) and os.stat(f"{tmp_path}/Train_val_list/trainset/0.pth").st_mtime_ns == mt


def test_trainset_interrupted_between_scenes_is_made_again(ts, gold, tables, tmp_path):
    """the lists are rewritten after every scene, so a run that stopped after the first training scene leaves train.pkl / train_pcp.pkl
    that name that scene's 30 batches only, with all of them on disk: trainset() must not take that for a finished set.  It makes the
    whole set again (from the first pair: the same seed gives the reference's 40 batches), and only then does a further call do nothing."""
    g = gold("trainset.npz")
    write_stage_files(ts, g, tmp_path)
    tc = host_creator(ts, tables, tmp_path)
    np.random.seed(TF.SEED_NP)
    tc.trainset()
    lst = f"{tmp_path}/Train_val_list"
    pcp = pickle.load(open(f"{lst}/train_pcp.pkl", "rb"))
    first = [t for t in pcp if t[0] == "synth_train/trainA"]
    assert len(first) == 30 and pcp[:30] == first
    pickle.dump(first, open(f"{lst}/train_pcp.pkl", "wb"))
    pickle.dump(list(range(30)), open(f"{lst}/train.pkl", "wb"))
    for i in range(30, 40):
        os.remove(f"{lst}/trainset/{i}.pth")
    assert not tc._trainset_complete(f"{lst}/trainset")
    np.random.seed(TF.SEED_NP)
    tc.trainset()
    assert pickle.load(open(f"{lst}/train_pcp.pkl", "rb")) == pcp and pickle.load(open(f"{lst}/train.pkl", "rb")) == list(range(40))
    TF.check_train_items(tmp_path, g)
    assert tc._trainset_complete(f"{lst}/trainset")
    # complete lists with an item missing, or a pair list missing, are not a finished set either
    os.remove(f"{lst}/trainset/17.pth")
    assert not tc._trainset_complete(f"{lst}/trainset")
    np.random.seed(TF.SEED_NP)
    tc.trainset()
    TF.check_train_items(tmp_path, g)
    os.rename(f"{tmp_path}/Pairs_0.03/synth_train/edge/0-1.npy", f"{tmp_path}/pairs.npy")
    assert tc._expected_train_list() is None and not tc._trainset_complete(f"{lst}/trainset")
    os.rename(f"{tmp_path}/pairs.npy", f"{tmp_path}/Pairs_0.03/synth_train/edge/0-1.npy")
    assert tc._expected_train_list() == pcp


def test_valset_consumes_the_random_streams_as_the_reference(ts, gold, tables, tmp_path):
    g = gold("trainset.npz")
    write_stage_files(ts, g, tmp_path)
    tc = host_creator(ts, tables, tmp_path)
    np.random.seed(TF.SEED_NP)
    random.seed(TF.SEED_PY)
    tc.trainset()                             # valset() continues the streams trainset() leaves, as in run()
    tc.valset()
    TF.check_val_items(tmp_path, g)
    # val_pcp.pkl exists now: nothing is drawn, an item that exists is kept, a missing one is written again
    os.remove(f"{tmp_path}/Train_val_list/valset/3.pth")
    st, mt = np.random.get_state()[1].copy(), os.stat(f"{tmp_path}/Train_val_list/valset/0.pth").st_mtime_ns
    tc.valset()
    assert np.array_equal(np.random.get_state()[1], st) and os.stat(f"{tmp_path}/Train_val_list/valset/0.pth").st_mtime_ns == mt
    TF.check_val_items(tmp_path, g)


def test_train_scene_table():
    """'3dmatch_train': 54 scenes, the six validation scenes among them (scene names and fragment counts are data of the reference)"""
    from yoho_amd import dataset as D
    scenes, counts = D._SCENES["3dmatch_train"]
    assert len(scenes) == len(set(scenes)) == len(counts) == 54 and sum(counts) == 1763 and min(counts) == 4 and max(counts) == 96
    assert len(D._TRAIN_VALSCENES) == 6 and set(D._TRAIN_VALSCENES) <= set(scenes)
    assert dict(zip(scenes, counts))["7-scenes-heads"] == 18 and scenes[0] == "bundlefusion-apt0" and scenes[-1] == "rgbd-scenes-v2-scene_13"


def trainset_header_functions():
    txt = open(os.path.join(REPO, "include", "yoho_trainset.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(yoho_[a-zA-Z0-9_]+)\s*\(", txt)))


def test_library_exports_trainset_header_symbols():
    """include/yoho_trainset.h: every function it declares is exported, the set is hip.TRAINSET_SYMBOLS and shares nothing with
    hip.SYMBOLS / hip.KNN_SYMBOLS, the header's limit is the binding's, and nothing of it leaked into the two pinned headers"""
    import ctypes as C
    from yoho_amd import build, hip
    lib_path = build.build(verbose=False)
    assert os.path.exists(lib_path)
    lib = hip.load_library()
    fns = trainset_header_functions()
    assert fns == ["yoho_radius_pairs", "yoho_trainset_gather"]
    for f in fns:
        assert hasattr(lib, f), f"libyoho_hip.so does not export {f}"
    assert set(fns) == set(hip.TRAINSET_SYMBOLS)
    assert not set(hip.TRAINSET_SYMBOLS) & set(hip.SYMBOLS) and not set(hip.TRAINSET_SYMBOLS) & set(hip.KNN_SYMBOLS)
    assert lib.yoho_radius_pairs.restype is C.c_int and len(lib.yoho_radius_pairs.argtypes) == 10
    assert lib.yoho_trainset_gather.restype is C.c_int and len(lib.yoho_trainset_gather.argtypes) == 9
    hdr = open(os.path.join(REPO, "include", "yoho_trainset.h")).read()
    assert eval(re.search(r"#define\s+YOHO_RADIUS_MAX_POINTS\s+\(([^)]*)\)", hdr).group(1)) == hip.RADIUS_MAX_POINTS == 1 << 20
    for older in ("yoho_hip.h", "yoho_knn.h"):
        txt = open(os.path.join(REPO, "include", older)).read()
        assert "yoho_radius" not in txt and "yoho_trainset" not in txt, older
    assert "radius.hip" in build.SOURCES and build.EXTRA["radius.hip"] == ["-ffp-contract=off"]


def test_fixture_regenerates_from_the_reference(gold, tmp_path):
    """where the reference tree exists (the build machine), tools/gen_golden_trainset.py gives tests/golden/trainset.npz again, array
    for array except the f64 labels, which may move by the last bits of another LAPACK build.  The generator patches numpy and torch
    for the reference's sake, so it runs as a child process."""
    import gen_golden_trainset as G
    if not G.reference_available():
        pytest.skip("the reference tree is not on this machine")
    dst = str(tmp_path / "fresh.npz")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "gen_golden_trainset.py"), "--out", dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    fresh, g = np.load(dst), gold("trainset.npz")
    assert sorted(fresh.files) == sorted(g.files)
    for key in g.files:
        a, b = fresh[key], g[key]
        assert a.dtype == b.dtype and a.shape == b.shape, key
        if a.dtype.kind == "f" and (key.endswith(("_deltaR", "_R")) or key in ("train_deltaR", "train_R", "val_R")):
            assert np.abs(a - b).max() <= 1e-6, key
        else:
            assert a.tobytes() == b.tobytes(), key


def test_radius_kernels_use_no_scratch(tmp_path):
    """csrc/radius.hip compiled for gfx950 with the flags of the build: the compiler's resource report names the four kernels, none
    with scratch (a spill), the pair kernels with their one LDS tile"""
    from yoho_amd import build
    cmd = [build._hipcc()] + build.FLAGS + build.EXTRA["radius.hip"] + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                                                                       os.path.join(build.CSRC, "radius.hip"), "-o", str(tmp_path / "radius.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(lds) == 4, names
    assert sum("radius_kernel" in n for n in names) == 2 and any("radius_scan_kernel" in n for n in names) and any("trainset_gather_kernel" in n for n in names)
    assert scratch == [0, 0, 0, 0], dict(zip(names, scratch))
    assert all(3 * 4096 * 4 <= b <= 64 * 1024 for n, b in zip(names, lds) if "radius_kernel" in n)
