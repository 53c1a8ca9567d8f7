"""Training-set generation on the GPU (-m gpu): yoho_radius_pairs against tests/trainset_ref.py (the contract, order included),
yoho_trainset_gather against numpy fancy indexing, both entries' refusals driven through ctypes as tests/test_gpu_abi.py does for
include/yoho_hip.h, and yoho_amd.YOHO_Trainset.trainset_create stage by stage and end to end against the reference's own output
(tests/golden/trainset.npz, written by tools/gen_golden_trainset.py), closed by a PartI training run on the generated files."""
import ctypes as C
import os
import pickle
import random
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import trainset_ref as TR  # noqa: E402
import trainset_fixture as TF  # noqa: E402
from yoho_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
EINVAL, ENOMEM = -1, -4
TILE = 4096                       # RP_TILE of csrc/radius.hip: points of b per LDS tile


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.Context()


def cloud(n, seed, scale=1.0):
    return (np.random.RandomState(seed).rand(n, 3) * scale).astype(np.float32)


def pairs_of(c, a, b, r):
    p = c.radius_pairs(cu(a), cu(b), r)
    assert p.dtype == torch.int64 and p.is_cuda and p.dim() == 2 and p.shape[1] == 2
    return p.cpu().numpy()


def raw_call(hip, c, a_d, b_d, r, capacity, guard=64, fill=-7):
    """the C entry itself with a pairs buffer of `capacity` rows followed by `guard` rows that must keep their pattern -> (M, pairs, guard ok)"""
    lib = hip.load_library()
    buf = torch.full((capacity + guard, 2), fill, dtype=torch.int64, device="cuda")
    count = torch.full((2,), fill, dtype=torch.int64, device="cuda")
    rc = lib.yoho_radius_pairs(c._h, C.c_void_p(a_d.data_ptr()), a_d.shape[0], C.c_void_p(b_d.data_ptr()), b_d.shape[0], float(r),
                               C.c_void_p(buf.data_ptr()) if capacity else None, capacity, C.c_void_p(count.data_ptr()), None)
    assert rc == 0, lib.yoho_last_error().decode()
    torch.cuda.synchronize()
    assert int(count[1]) == fill
    return int(count[0]), buf[:capacity].cpu().numpy(), bool((buf[capacity:] == fill).all())


def test_radius_pairs_equals_ref_on_the_fixture_pairs(ctx, gold):
    """the filtered keys of the fixture's set: the pair lists of the reference itself (torch.norm + np.where), exactly and in order"""
    g = gold("trainset.npz")
    ds = TF.build_dataset()
    n = 0
    for scene, d in ds.scenes.items():
        for p0, p1 in d.pair_ids:
            k0 = d.get_kps(p0)[g[f"{scene}_{p0}_ok"]].astype(np.float32)
            k1 = d.get_kps(p1)[g[f"{scene}_{p1}_ok"]].astype(np.float32)
            want = g[f"{scene}_{p0}-{p1}_pairs"].astype(np.int64)
            got = pairs_of(ctx, k0, k1, 0.02)
            assert np.array_equal(got, want), (scene, p0, p1)
            assert np.array_equal(TR.radius_pairs_ref(k0, k1, 0.02), want)
            n += 1
    assert n >= 4


def test_radius_pairs_ragged_sizes_around_wave_and_tile_edges(ctx):
    sizes = (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 5000)
    total = 0
    for na in sizes:
        for nb in sizes:
            a, b = cloud(na, 3 * na + 1), cloud(nb, 5 * nb + 2)
            r = 0.5 if na * nb < 10000 else 0.05
            want = TR.radius_pairs_ref(a, b, r)
            got = pairs_of(ctx, a, b, r)
            assert np.array_equal(got, want), (na, nb, len(got), len(want))
            total += len(want)
    assert total > 100000
    # Nb above one LDS tile, by several tiles and raggedly; Na not a multiple of the rows of a workgroup
    for na, nb in ((37, 3 * TILE + 17), (1001, 2 * TILE + 1)):
        a, b = cloud(na, 11), cloud(nb, 12)
        want = TR.radius_pairs_ref(a, b, 0.06)
        assert len(want) > na
        assert np.array_equal(pairs_of(ctx, a, b, 0.06), want), (na, nb)


def test_radius_pairs_on_and_one_ulp_beside_the_threshold(ctx):
    """points whose distance from the query is the radius itself and its f32 neighbours, in both argument orders and for radii whose
    square is and is not exactly representable; the restatement decides which of them pair"""
    for r in (0.02, 0.03, 0.5, 1.0, 3.0, 1e-3, 1234.5):
        pts = TR.threshold_points(r, 64)
        o = np.zeros((1, 3), np.float32)
        want = TR.radius_pairs_ref(o, pts, r)
        assert 0 < len(want) < 64                       # the band straddles the threshold
        assert np.array_equal(pairs_of(ctx, o, pts, r), want), r
        assert np.array_equal(pairs_of(ctx, pts, o, r), TR.radius_pairs_ref(pts, o, r)), r
        # the same band moved off the axis and into a crowd of far points, beyond one tile
        shift = np.array([[0.25, -0.5, 0.125]], np.float32)
        far = cloud(TILE + 100, 4) + np.float32(10 * max(r, 1.0))
        b = np.concatenate([far[:TILE - 10], pts + shift, far[TILE - 10:]], 0)
        want = TR.radius_pairs_ref(shift, b, r)
        assert len(want) > 0
        assert np.array_equal(pairs_of(ctx, shift, b, r), want), r
    # radii outside the range where the kernel's shortcut bounds are used: every sum takes the exact path
    for r in (1e-20, 1e20, np.inf):
        a, b = cloud(100, 1), cloud(300, 2)
        assert np.array_equal(pairs_of(ctx, a, b, r), TR.radius_pairs_ref(a, b, r)), r
    a = np.zeros((3, 3), np.float32)
    assert len(pairs_of(ctx, a, a, 1e-20)) == 9          # d = 0 < radius


def test_radius_pairs_nan_inf_all_and_none(ctx):
    a, b = cloud(300, 5), cloud(700, 6)
    a[3] = np.nan; a[10, 1] = np.inf; a[11, 2] = -np.inf
    b[0, 0] = np.nan; b[65] = np.inf; b[699] = np.nan; b[128] = np.inf
    for r in (0.1, 2.0, np.inf):
        want = TR.radius_pairs_ref(a, b, r)
        got = pairs_of(ctx, a, b, r)
        assert np.array_equal(got, want), r
        assert not np.isin(got[:, 0], [3, 10, 11]).any() and not np.isin(got[:, 1], [0, 65, 128, 699]).any()
    a, b = cloud(130, 7), cloud(257, 8)
    every = pairs_of(ctx, a, b, 10.0)                    # all pairs: np.where's order is the row-major enumeration
    assert np.array_equal(every, np.stack(np.divmod(np.arange(130 * 257), 257), 1))
    for r in (1e-6, 0.0, -1.0, -np.inf):                 # none; radius <= 0 pairs nothing, not even coincident points
        assert pairs_of(ctx, a, a, r).shape == (130 if r > 0 else 0, 2)
    assert pairs_of(ctx, a, b, 1e-6).shape == (0, 2)
    assert pairs_of(ctx, a[:0], b, 1.0).shape == (0, 2) and pairs_of(ctx, a, b[:0], 1.0).shape == (0, 2)


def test_radius_pairs_count_only_and_short_capacity(ctx, hip):
    a, b = cloud(1000, 21), cloud(TILE + 500, 22)
    want = TR.radius_pairs_ref(a, b, 0.08)
    M = len(want)
    assert M > 5000
    a_d, b_d = cu(a), cu(b)
    m, _, ok = raw_call(hip, ctx, a_d, b_d, 0.08, 0)
    assert m == M and ok                                 # count only: pairs NULL, capacity 0
    for cap in (1, 63, M // 2, M - 1, M, M + 100):
        m, p, ok = raw_call(hip, ctx, a_d, b_d, 0.08, cap)
        assert m == M, cap                               # the full count also when the buffer is short
        assert ok, ("wrote behind the buffer", cap)
        k = min(cap, M)
        assert np.array_equal(p[:k], want[:k]), cap      # exactly the first `capacity` pairs of the order
        assert (p[k:] == -7).all(), cap
    # the wrapper's second call: more pairs than its guess of 4 max(Na, Nb)
    a, b = cloud(200, 23, 0.1), cloud(300, 24, 0.1)
    want = TR.radius_pairs_ref(a, b, 0.5)
    assert len(want) == 200 * 300 > 4 * 300
    assert np.array_equal(pairs_of(ctx, a, b, 0.5), want)


def test_radius_pairs_ignores_scratch_contents_and_call_count(hip):
    c = hip.Context()
    a, b = cloud(5000, 31), cloud(5000, 32)
    want = TR.radius_pairs_ref(a, b, 0.03)
    assert len(want) > 1000
    assert np.array_equal(pairs_of(c, a, b, 0.03), want)
    for pattern in (0xFFFFFFFF, 0x7FC00000, 0x01010101):
        c.poison_scratch(pattern)
        assert np.array_equal(pairs_of(c, a, b, 0.03), want), hex(pattern)
        assert np.array_equal(pairs_of(c, a, b, 0.03), want), (hex(pattern), "second call")
    small = TR.radius_pairs_ref(a[:77], b[:130], 0.2)    # a smaller call in the workspace the larger one left behind
    assert np.array_equal(pairs_of(c, a[:77], b[:130], 0.2), small)


def test_radius_pairs_workspace_refusal_is_enomem_and_leaves_the_context_usable(hip, monkeypatch):
    """12 bytes per row of a: 200000 rows ask for 2.4 MB, refused by a context whose workspace may not exceed 1 MiB"""
    monkeypatch.setenv("YOHO_WS_LIMIT_MB", "1")
    c = hip.Context()
    monkeypatch.delenv("YOHO_WS_LIMIT_MB")
    big = cu(np.zeros((200000, 3), np.float32))
    one = cu(np.ones((1, 3), np.float32))
    with pytest.raises(hip.YohoError) as e:
        c.radius_pairs(big, one, 0.5)
    assert e.value.code == ENOMEM and "workspace" in str(e.value)
    a, b = cloud(500, 41), cloud(900, 42)
    assert np.array_equal(pairs_of(c, a, b, 0.1), TR.radius_pairs_ref(a, b, 0.1))


def test_trainset_gather_equals_fancy_indexing(ctx):
    rs = np.random.RandomState(3)
    for nr, kn, B in ((5, 300, 320), (1, 1, 1), (5, 77, 1500), (2, 1000, 512), (3, 9, 513)):
        feats = rs.randn(nr, kn, 32, 60).astype(np.float32)
        feats.view(np.uint32)[0, 0, 0, :4] = [0x7FC00001, 0xFFFFFFFF, 0x00000001, 0x80000000]      # bytes, not values
        rot, key = rs.randint(0, nr, B), rs.randint(0, kn, B)
        out = ctx.trainset_gather(cu(feats), rot, key)
        assert out.dtype == torch.float32 and tuple(out.shape) == (B, 32, 60) and out.is_cuda
        assert out.cpu().numpy().tobytes() == feats[rot, key].tobytes(), (nr, kn, B)
    f_d = cu(feats)
    assert tuple(ctx.trainset_gather(f_d, [], []).shape) == (0, 32, 60)
    for rot, key, text in (([0, 3, 1], [0, 0, 0], "rot[1]=3"), ([0, -1, 5], [0, 0, 0], "rot[1]=-1"), ([0, 1, 2], [8, 9, 1], "key[1]=9"),
                           ([2, 2, 2], [0, 1, -4], "key[2]=-4")):
        with pytest.raises(ctx_error()) as e:
            ctx.trainset_gather(f_d, rot, key)
        assert e.value.code == EINVAL and "yoho_trainset_gather" in str(e.value) and text in str(e.value), str(e.value)


def ctx_error():
    from yoho_amd import hip
    return hip.YohoError


def test_entries_refuse_bad_arguments(ctx, hip):
    lib = hip.load_library()
    h = ctx._h
    a, b = cu(cloud(9, 1)), cu(cloud(40, 2))
    pairs = torch.full((64, 2), -7, dtype=torch.int64, device="cuda")
    count = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    feats = cu(np.random.RandomState(0).randn(2, 10, 32, 60).astype(np.float32))
    out = torch.full((5, 32, 60), -3.0, dtype=torch.float32, device="cuda")
    rot = np.array([0, 1, 1, 0], np.int64)
    key = np.array([0, 9, 3, 4], np.int64)
    bad_rot = np.array([0, 1, 2, 0], np.int64)
    bad_key = np.array([0, 9, 10, 4], np.int64)
    p = lambda t: C.c_void_p(t.data_ptr())
    off = lambda t, nbytes: C.c_void_p(t.data_ptr() + nbytes)
    hp = lambda x: x.ctypes.data_as(C.c_void_p)
    N = None
    cases = {
        "yoho_radius_pairs": [
            ((N, p(a), 9, p(b), 40, 0.5, p(pairs), 64, p(count), N), "bad argument"),
            ((h, N, 9, p(b), 40, 0.5, p(pairs), 64, p(count), N), "NULL"),
            ((h, p(a), 9, N, 40, 0.5, p(pairs), 64, p(count), N), "NULL"),
            ((h, p(a), 9, p(b), 40, 0.5, p(pairs), 64, N, N), "bad argument"),
            ((h, p(a), -1, p(b), 40, 0.5, p(pairs), 64, p(count), N), "Na=-1"),
            ((h, p(a), 9, p(b), -2, 0.5, p(pairs), 64, p(count), N), "Nb=-2"),
            ((h, p(a), (1 << 20) + 1, p(b), 40, 0.5, p(pairs), 64, p(count), N), "YOHO_RADIUS_MAX_POINTS"),
            ((h, p(a), 9, p(b), (1 << 20) + 1, 0.5, p(pairs), 64, p(count), N), "YOHO_RADIUS_MAX_POINTS"),
            ((h, p(a), 9, p(b), 40, float("nan"), p(pairs), 64, p(count), N), "NaN"),
            ((h, p(a), 9, p(b), 40, 0.5, N, 64, p(count), N), "capacity=64"),
            ((h, p(a), 9, p(b), 40, 0.5, p(pairs), -1, p(count), N), "capacity=-1"),
            ((h, off(a, 2), 8, p(b), 40, 0.5, p(pairs), 64, p(count), N), "4-byte aligned"),
            ((h, p(a), 9, off(b, 1), 39, 0.5, p(pairs), 64, p(count), N), "4-byte aligned"),
            ((h, p(a), 9, p(b), 40, 0.5, off(pairs, 4), 60, p(count), N), "8-byte aligned"),
            ((h, p(a), 9, p(b), 40, 0.5, p(pairs), 64, off(count, 4), N), "8-byte aligned"),
            ((h, p(a), 0, p(b), 40, float("nan"), p(pairs), 64, p(count), N), "NaN"),       # no rows does not excuse a bad radius
        ],
        "yoho_trainset_gather": [
            ((N, p(feats), 2, 10, hp(rot), hp(key), 4, p(out), N), "bad argument"),
            ((h, N, 2, 10, hp(rot), hp(key), 4, p(out), N), "NULL"),
            ((h, p(feats), 2, 10, N, hp(key), 4, p(out), N), "NULL"),
            ((h, p(feats), 2, 10, hp(rot), N, 4, p(out), N), "NULL"),
            ((h, p(feats), 2, 10, hp(rot), hp(key), 4, N, N), "NULL"),
            ((h, p(feats), -1, 10, hp(rot), hp(key), 4, p(out), N), "nr=-1"),
            ((h, p(feats), 2, -10, hp(rot), hp(key), 4, p(out), N), "kn=-10"),
            ((h, p(feats), 2, 10, hp(rot), hp(key), -4, p(out), N), "B=-4"),
            ((h, p(feats), 1 << 20, 1 << 20, hp(rot), hp(key), 4, p(out), N), "2^31"),
            ((h, off(feats, 4), 2, 9, hp(rot), hp(key), 4, p(out), N), "16-byte aligned"),
            ((h, p(feats), 2, 10, hp(rot), hp(key), 4, off(out, 8), N), "16-byte aligned"),
            ((h, p(feats), 2, 10, hp(bad_rot), hp(key), 4, p(out), N), "rot[2]=2"),
            ((h, p(feats), 2, 10, hp(rot), hp(bad_key), 4, p(out), N), "key[2]=10"),
            ((h, p(feats), 0, 10, hp(rot), hp(key), 4, p(out), N), "rot[0]=0"),
        ],
    }
    assert set(cases) == set(hip.TRAINSET_SYMBOLS)       # every entry of include/yoho_trainset.h has its refusals here
    for fn, rows in cases.items():
        for args, text in rows:
            rc = getattr(lib, fn)(*args)
            msg = lib.yoho_last_error().decode()
            assert rc == EINVAL, (fn, args, rc, msg)
            assert fn in msg and text in msg, (fn, text, msg)
    torch.cuda.synchronize()
    assert bool((pairs == -7).all()) and bool((count == -7).all()) and bool((out == -3.0).all())     # nothing was launched
    # counts of 0: valid with NULL data pointers; the count is still delivered
    assert lib.yoho_radius_pairs(h, N, 0, p(b), 40, 0.5, N, 0, p(count), N) == 0
    torch.cuda.synchronize()
    assert count.tolist() == [0, -7]
    count.fill_(-7)
    assert lib.yoho_radius_pairs(h, p(a), 9, N, 0, 0.5, p(pairs), 64, p(count), N) == 0
    assert lib.yoho_trainset_gather(h, N, 0, 0, N, N, 0, N, N) == 0
    torch.cuda.synchronize()
    assert count.tolist() == [0, -7] and bool((pairs == -7).all()) and bool((out == -3.0).all())
    # valid calls on rows of 12 bytes that are not 16-byte aligned, and the context works as before
    rc = lib.yoho_radius_pairs(h, off(a, 12), 8, off(b, 12), 39, 0.5, p(pairs), 64, p(count), N)
    assert rc == 0, lib.yoho_last_error().decode()
    torch.cuda.synchronize()
    want = TR.radius_pairs_ref(a.cpu().numpy()[1:], b.cpu().numpy()[1:], 0.5)
    assert int(count[0]) == len(want) and np.array_equal(pairs[:min(64, len(want))].cpu().numpy(), want[:64])
    rc = lib.yoho_trainset_gather(h, p(feats), 2, 10, hp(rot), hp(key), 4, p(out), N)
    assert rc == 0, lib.yoho_last_error().decode()
    torch.cuda.synchronize()
    assert np.array_equal(out[:4].cpu().numpy(), feats.cpu().numpy()[rot, key]) and bool((out[4:] == -3.0).all())


# ---- yoho_amd.YOHO_Trainset.trainset_create -----------------------------------------------------------------------------------------

def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - b)) / max(np.max(np.abs(b)), 1e-30))


def tree_state(root):
    return {os.path.join(d, f): os.stat(os.path.join(d, f)).st_mtime_ns for d, _, fs in os.walk(root) for f in fs}


def test_create_PC_random_rot_feat_equals_the_testset_pipeline_and_the_oracle(tmp_path, tables, monkeypatch):
    """two surface clouds, synthetic backbone weights: block r of a fragment's features is, bit for bit, what testset_create computes
    for the cloud rotated by R_r on the host; three group elements of one block agree with the oracle chain (voxelise, backbone, f64
    NN gather) within the 1e-4 relative of test_testset_create_from_point_clouds; one lane writes the same bytes as two"""
    import fcgf_oracle as fo
    import yoho_oracle as orc
    from yoho_amd import weights as W
    from yoho_amd.YOHO_Trainset import trainset_create
    from yoho_amd.YOHO_testset import testset_create
    fsd = W.synth_state_dict(W.FCGF_SPEC, 3)
    ck = {"config": {"model": "ResUNetBN2C", "model_n_out": 32, "normalize_feature": True, "conv1_kernel_size": 7}, "state_dict": fsd}
    clouds = {"0": synth.surface_cloud(2200, seed=11), "1": synth.surface_cloud(1800, seed=12)}
    rs = np.random.RandomState(0)
    kidx = {k: np.sort(rs.permutation(len(v))[:40]) for k, v in clouds.items()}

    class DS:
        name = "synth/room"
        pc_ids = ["0", "1"]
        pair_ids = []
        get_pc = staticmethod(lambda i: clouds[i])

    def creator(out, lanes):
        monkeypatch.setenv("YOHO_FCGF_LANES", str(lanes))
        cfg = types.SimpleNamespace(model=ck, voxel_size=0.025, datasetname="synth", output_dir=str(out), origin_dir=str(tmp_path), rot_seed=5,
                                    datasets={"wholesetname": "synth", "valscenes": [], "room": DS()})
        tc = trainset_create(cfg)
        assert tc.lanes == lanes
        for pid in DS.pc_ids:
            os.makedirs(f"{out}/Filtered_Keys/synth/room", exist_ok=True)
            np.save(f"{out}/Filtered_Keys/synth/room/{pid}_index.npy", kidx[pid])
        tc.PC_random_rot_feat()
        assert tc.stats["rot_feat"]["fragments"] == 2
        return tc
    tc = creator(tmp_path / "two", 2)
    creator(tmp_path / "one", 1)
    tt = testset_create(types.SimpleNamespace(model=ck, voxel_size=0.025, dataset="synth", output_dir=str(tmp_path), origin_dir=str(tmp_path),
                                              datasets={"wholesetname": "synth"}))
    for pid in DS.pc_ids:
        z = np.load(f"{tmp_path}/two/Rotated_Features/synth/room/{pid}_feats.npz")
        Rs, feats = z["Rs"], z["feats"]
        assert feats.shape == (5, 40, 32, 60) and feats.dtype == np.float32 and Rs.shape == (5, 3, 3) and Rs.dtype == np.float64
        assert np.array_equal(np.load(f"{tmp_path}/two/Rotated_Features/synth/room/{pid}_Rs.npy"), Rs)
        z1 = np.load(f"{tmp_path}/one/Rotated_Features/synth/room/{pid}_feats.npz")
        assert np.array_equal(z1["Rs"], Rs) and z1["feats"].tobytes() == feats.tobytes(), pid       # rot_seed: the same rotations; lanes: the same bytes
        assert np.abs(Rs[0] - Rs[1]).max() > 1e-3
        for r in range(5):
            assert np.abs(Rs[r] @ Rs[r].T - np.eye(3)).max() < 1e-14
            pc_r = clouds[pid] @ Rs[r].T
            want = tt.fragment_group_features(pc_r, pc_r[kidx[pid]]).cpu().numpy()
            assert want.tobytes() == feats[r].tobytes(), (pid, r)
    pc_r = clouds["1"] @ Rs[3].T
    assert np.array_equal(tc.FCGF_Group_Feature_Extractor(None, pc_r, kidx["1"]), feats[3])
    for g in (0, 23, 59):
        pcg = pc_r @ tables.R64[g].T
        sel, Fg = fo.extract_features(pcg, 0.025, fsd)
        ref = orc.group_gather_one(pc_r[kidx["1"]], pcg[sel].astype(np.float32), Fg, tables.R64[g])[0]
        assert rel(feats[3][:, :, g], ref) < 1e-4, g
    # nothing left to do: a second call reads no cloud and writes nothing
    before = tree_state(tmp_path / "two")
    tc.PC_random_rot_feat(tc.config)                        # the reference's signature: its argparse namespace
    assert tc.stats["rot_feat"]["fragments"] == 0 and tree_state(tmp_path / "two") == before


@pytest.fixture(scope="module")
def generated(tmp_path_factory, gold):
    """run() on the fixture's set: inputs on disk, Rotated_Features from the fixture's seeds and stored rotations (so the backbone
    stage finds nothing to do and no checkpoint is read), np.random / random seeded as the generator seeded them for the reference"""
    from yoho_amd.YOHO_Trainset import trainset_create
    g = gold("trainset.npz")
    root = tmp_path_factory.mktemp("trainset")
    ts = TF.build_dataset().write_inputs(f"{root}/origin")
    out = f"{root}/out"
    ts.write_rotated_features(out, lambda scene, pc_id: g[f"{scene}_{pc_id}_Rs"])
    cfg = types.SimpleNamespace(model="/nonexistent/checkpoint.pth", voxel_size=0.025, datasetname=TF.NAME, output_dir=out, origin_dir=f"{root}/origin",
                                datasets=ts.datasets())
    tc = trainset_create(cfg)
    np.random.seed(TF.SEED_NP)
    random.seed(TF.SEED_PY)
    tc.run()
    return ts, tc, out


def test_run_on_the_fixture_equals_the_reference(generated, gold):
    """every file of the reference's layout: filtered keys and pair lists exactly, every .pth item (indices and labels exactly, deltaR
    and R within 1e-6, feature digests exactly: rows are copied), the four lists; a second run() writes nothing"""
    ts, tc, out = generated
    g = gold("trainset.npz")
    for scene, d in ts.scenes.items():
        for k, pc_id in enumerate(d.pc_ids):
            ok = g[f"{scene}_{pc_id}_ok"]
            idx, coor = np.load(f"{out}/Filtered_Keys/{d.name}/{pc_id}_index.npy"), np.load(f"{out}/Filtered_Keys/{d.name}/{pc_id}_coor.npy")
            assert idx.dtype == np.int64 and np.array_equal(idx, d.key_idx[k][ok]) and coor.dtype == np.float64 and np.array_equal(coor, d.get_kps(pc_id)[ok])
        for p0, p1 in d.pair_ids:
            pairs = np.load(f"{out}/Pairs_0.03/{d.name}/{p0}-{p1}.npy")
            assert pairs.dtype == np.int64 and np.array_equal(pairs, g[f"{scene}_{p0}-{p1}_pairs"]), (scene, p0, p1)
    pcp = pickle.load(open(f"{out}/Train_val_list/train_pcp.pkl", "rb"))
    assert pcp == list(zip(g["train_pcp_name"].tolist(), g["train_pcp_pc0"].tolist(), g["train_pcp_pc1"].tolist(), g["train_pcp_i"].tolist()))
    assert pickle.load(open(f"{out}/Train_val_list/train.pkl", "rb")) == list(range(len(pcp)))
    TF.check_train_items(out, g)
    TF.check_val_items(out, g)
    before = tree_state(out)
    st = np.random.get_state()[1].copy()
    tc.run()
    assert tree_state(out) == before and np.array_equal(np.random.get_state()[1], st)


def test_trainer_partI_trains_from_the_generated_files(generated, tmp_path):
    """closing the loop: Trainer_partI with the file-based dataset classes reads the generated train_pcp.pkl / val_pcp.pkl and the
    .pth items, runs its epochs and validations; every loss is finite and both checkpoints have the reference's four keys.  No claim
    that the loss falls: the fixture's features are noise."""
    from yoho_amd import weights as W
    from yoho_amd.train import trainer
    ts, tc, out = generated
    cfg = types.SimpleNamespace(SO3_related_files=None, model_fn=str(tmp_path), train_network_type="PartI_train", trainset_type="Enhanced_train_dataset_PartI",
                                batch_size=32, worker_num=0, lr_init=1e-3, lr_decay_rate=0.5, lr_decay_step=100, loss_type="Batch_hard_Rindex_loss",
                                val_type="Val_partI", epochs=2, train_log_step=10, val_interval=40, save_interval=40,
                                train_pcpair_list_fn=f"{out}/Train_val_list/train_pcp.pkl", val_pppair_list_fn=f"{out}/Train_val_list/val_pcp.pkl",
                                output_cache_fn=out)
    torch.manual_seed(1)
    tr = trainer.name2trainer["PartI"](cfg)
    assert isinstance(tr.train_set.dataset, trainer.Enhanced_train_dataset_PartI) and len(tr.train_set) == 40 and len(tr.val_set) == 98 // 32
    losses, vals = [], []
    step0, val0 = tr.train_step, tr.val_evaluator

    def step(data, s):
        losses.append(float(step0(data, s)))
        return torch.tensor(losses[-1])

    def val(net, ds):
        vals.append(val0(net, ds))
        return vals[-1]
    tr.train_step, tr.val_evaluator = step, val
    tr.run()
    assert len(losses) == 80 and np.isfinite(losses).all()
    assert len(vals) == 2 and all(np.isfinite(float(v["val_loss"])) and 0.0 <= float(v["whole_recall"]) <= 1.0 for v in vals)
    for fn in ("model.pth", "model_best.pth"):
        ck = torch.load(os.path.join(str(tmp_path), "PartI_train", fn), weights_only=False)
        assert set(ck.keys()) == {"step", "best_para", "network_state_dict", "optimizer_state_dict"}
        assert set(ck["network_state_dict"].keys()) == {n for n, _ in W.PARTI_SPEC}
