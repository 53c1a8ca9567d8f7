"""yoho_fps on the GPU (-m gpu): indices and dist2 bits against the numpy restatement (tests/keypoints_ref.py) exactly, on both paths, at
the wave, workgroup, block and capacity edges the header's constants give; ties, duplicates, non-finite rows; a cross-check against
yoho_nn_search; poisoned scratch, a fresh context, a side stream; the refusals through raw ctypes; and the extractor's keypoint option."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keypoints_ref as KR  # noqa: E402
import test_keypoints_cpu as TC  # noqa: E402
from yoho_amd import synth  # noqa: E402
from yoho_amd import weights as W  # noqa: E402

pytestmark = pytest.mark.gpu
EINVAL, ENOMEM = -1, -4
f32 = np.float32
PATTERNS = (0xFFFFFFFF, 0x7FC00000, 0x00000001, 0xDEADBEEF, 0x7F800000)
MAXP, ONE, B, PATHS = TC.header_constants()


def cu(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()                    # (a copy: the cached clouds are read-only)


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.Context()


@functools.lru_cache(maxsize=None)
def cloud(m, seed=0):
    p = np.random.RandomState(1000 * seed + m % 997).rand(m, 3).astype(f32)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def ref(m, k, start, seed=0):
    """the restatement on cloud(m, seed): computed once, shared by the tests that need it"""
    idx, d2 = KR.fps_ref(cloud(m, seed), k, start)
    idx.setflags(write=False)
    d2.setflags(write=False)
    return idx, d2


def run(c, p, k, start=0, path="auto"):
    idx, d2 = c.fps(p if isinstance(p, torch.Tensor) else cu(p), k, start=start, path=path)
    assert idx.dtype == torch.int64 and d2.dtype == torch.float32 and tuple(idx.shape) == (k,) and tuple(d2.shape) == (k,)
    return idx.cpu().numpy(), d2.cpu().numpy()


def check(c, p, k, start, want, what, paths=None):
    """every path that takes m gives the reference's indices and dist2 bits"""
    m = len(p)
    paths = paths or (("auto", "one_wg", "per_pick") if m <= ONE else ("auto", "per_pick"))
    p_d = cu(p)
    for path in paths:
        idx, d2 = run(c, p_d, k, start, path)
        assert np.array_equal(idx, want[0]), (what, path, int(np.argmax(idx != want[0])))
        assert d2.tobytes() == want[1].tobytes(), (what, path)


def k_of(m):
    return m if m <= 1025 else 500


# ---- sizes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 1023, 1024, 1025, ONE - 1, ONE])
def test_one_workgroup_edges(ctx, m):
    """wave (64), workgroup (1024) and capacity edges of the one-workgroup path; the per-pick path and auto give the same bytes"""
    k = k_of(m)
    check(ctx, cloud(m), k, 0, ref(m, k, 0), ("m", m))


@pytest.mark.parametrize("m", [1, 255, 257, B - 1, B, B + 1, 2 * B + 1, 65 * B + 1])
def test_per_pick_edges(ctx, m):
    """one block, ragged blocks, several blocks and more partials than one wave reduces in a step (65 blocks + 1 point: 66 partials)"""
    k = 32 if m == 65 * B + 1 else k_of(m)
    check(ctx, cloud(m), k, 0, ref(m, k, 0), ("m", m))


@pytest.mark.parametrize("k", [1, 2, 500])
def test_pick_counts(ctx, k):
    m = 3 * B + 5
    want = ref(m, 500, 7)
    check(ctx, cloud(m), k, 7, (want[0][:k], want[1][:k]), ("k", k))                             # a shorter selection is a prefix


def test_start_positions(ctx):
    m = 2 * B + 7
    for start in (0, m - 1, 2 * B + 3):                                                            # the last one inside the ragged last block
        check(ctx, cloud(m), 40, start, ref(m, 40, start), ("start", start))


def test_k_zero_and_an_empty_cloud(ctx):
    idx, d2 = ctx.fps(cu(cloud(10)), 0)
    assert tuple(idx.shape) == (0,) and tuple(d2.shape) == (0,)
    idx, d2 = ctx.fps(torch.empty((0, 3), dtype=torch.float32, device="cuda"), 0, want_dist2=False)
    assert tuple(idx.shape) == (0,) and d2 is None
    idx, d2 = ctx.fps(cu(cloud(10)), 3, want_dist2=False)
    assert d2 is None and np.array_equal(idx.cpu().numpy(), ref(10, 3, 0)[0])
    with pytest.raises(ValueError):
        ctx.fps(cu(cloud(10)), 3, path="fast")
    with pytest.raises(ValueError):
        ctx.fps(cu(np.zeros((10, 2), f32)), 3)


# ---- ties -------------------------------------------------------------------------------------------------------------------------------
def lattice():
    return np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(f32)


def test_ties_on_an_integer_lattice(ctx):
    """8 x 8 x 8 integer points: exact float32 ties at every pick, the lowest index wins inside a wave and across waves"""
    p = lattice()
    want = KR.fps_ref(p, 512, 0)
    assert sorted(want[0].tolist()) == list(range(512))
    check(ctx, p, 512, 0, want, "lattice")
    check(ctx, p, 100, 511, KR.fps_ref(p, 100, 511), "lattice from its last point")


def test_ties_across_waves_and_workgroups(ctx):
    """the lattice tiled to 2 B + 7 points (p[i] = base[i % 512]): every tie spans waves and workgroups, and the copy with the lowest
    index must win each of them - the first 512 picks are all below 512"""
    m = 2 * B + 7
    p = lattice()[np.arange(m) % 512]
    want = KR.fps_ref(p, 600, 0)
    assert (want[0][:512] < 512).all() and (want[1][512:] == 0).all()
    check(ctx, p, 600, 0, want, "tiled lattice")
    idx, _ = run(ctx, p, 512, 0, "per_pick")
    assert (idx < 512).all()


def test_a_cloud_of_one_repeated_point(ctx):
    p = np.tile(np.array([[0.25, -1.5, 3.0]], f32), (300, 1))
    want = KR.fps_ref(p, 300, 17)
    assert want[0].tolist() == [17] + [i for i in range(300) if i != 17]                           # the sentinel: never a picked point again
    check(ctx, p, 300, 17, want, "duplicates")
    for path in ("one_wg", "per_pick"):
        assert sorted(run(ctx, p, 300, 17, path)[0].tolist()) == list(range(300))


# ---- against an existing kernel ---------------------------------------------------------------------------------------------------------
def test_dist2_is_the_nn_search_maximum(ctx):
    """dist2[s] = max over the cloud of yoho_nn_search's squared distance to picks 0 .. s - 1, bit for bit: the same arithmetic"""
    m = 2 * B + 77
    p_d = cu(cloud(m, 3))
    for path in ("one_wg", "per_pick"):
        idx, d2 = ctx.fps(p_d, 300, start=5, path=path)
        for s in (1, 2, 63, 150, 299):
            d, _ = ctx.nn_search(p_d, p_d[idx[:s]].contiguous(), want_dist=True, squared=True)
            assert d.max().cpu().numpy().tobytes() == d2[s].cpu().numpy().tobytes(), (path, s)
            assert d[idx[s]].cpu().numpy().tobytes() == d2[s].cpu().numpy().tobytes()              # and the pick is a point that attains it
    assert float(d2[0]) == np.inf


# ---- hygiene ----------------------------------------------------------------------------------------------------------------------------
def test_bytes_repeat_over_poisoned_scratch_contexts_and_streams(hip):
    m, k = 5 * B + 321, 96
    p_d = cu(cloud(m, 2))
    want = ref(m, k, 9, 2)
    first = None
    for rep in range(7):
        if rep in (0, 5):
            cx = hip.Context()                                           # repeat 5 on a context of its own
        cx.poison_scratch(PATTERNS[rep % 5])
        if rep == 6:                                                     # the last repeat on a side stream
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                outs = [cx.fps(p_d, k, start=9, path=path) for path in ("per_pick", "one_wg", "auto")]
            st.synchronize()
        else:
            outs = [cx.fps(p_d, k, start=9, path=path) for path in ("per_pick", "one_wg", "auto")]
        got = [x.cpu().numpy().tobytes() for o in outs for x in o]
        if first is None:
            first = got
            assert got[0] == want[0].tobytes() and got[1] == want[1].tobytes()
        assert got == first, rep
        assert got[0] == got[2] == got[4] and got[1] == got[3] == got[5]


def test_non_finite_rows_still_give_distinct_indices(ctx):
    m, k = 2 * B + 9, 200
    p = cloud(m, 4).copy()
    p[37] = np.nan
    p[B + 3] = (np.inf, 0.5, -np.inf)
    p[2 * B + 1, 1] = np.nan
    for path in ("one_wg", "per_pick"):
        for start in (0, 37):
            idx, _ = run(ctx, p, k, start, path)
            assert len(set(idx.tolist())) == k and idx.min() >= 0 and idx.max() < m and idx[0] == start, (path, start)
    idx, _ = run(ctx, p[:300], 300, 0, "per_pick")
    assert sorted(idx.tolist()) == list(range(300))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_arguments(ctx, hip):
    lib = hip.load_library()
    h = ctx._h
    p_d = cu(cloud(64))
    idx = torch.full((12,), -7, dtype=torch.int64, device="cuda")
    d2 = torch.full((12,), -3.0, dtype=torch.float32, device="cuda")
    big = torch.empty((1,), dtype=torch.float32, device="cuda")          # never read: the sizes below are refused before any launch
    p = lambda x: C.c_void_p(x.data_ptr())                               # noqa: E731
    off = lambda x, nbytes: C.c_void_p(x.data_ptr() + nbytes)            # noqa: E731
    N = None

    def a(ctx_=h, pts=p(p_d), m=64, k=8, start=0, path=0, idx_=p(idx), d2_=p(d2)):
        return (ctx_, pts, m, k, start, path, idx_, d2_, N)

    rows = [
        (a(ctx_=N), "NULL"), (a(pts=N), "NULL"), (a(idx_=N), "NULL"),
        (a(m=-1, k=0), "m=-1"), (a(pts=p(big), m=MAXP + 1), "YOHO_FPS_MAX_POINTS"),
        (a(k=-1), "k=-1"), (a(k=65), "k=65"),
        (a(start=-1), "start=-1"), (a(start=64), "start=64"),
        (a(path=3), "path=3"), (a(path=-1), "path=-1"),
        (a(pts=p(big), m=ONE + 1, path=PATHS["one_wg"]), "YOHO_FPS_ONE_WG_MAX"),
        (a(pts=off(p_d, 2), m=60), "4-byte aligned"), (a(d2_=off(d2, 2)), "4-byte aligned"), (a(idx_=off(idx, 4)), "8-byte aligned"),
    ]
    for args, text in rows:
        rc = lib.yoho_fps(*args)
        msg = lib.yoho_last_error().decode()
        assert rc == EINVAL, (text, rc, msg)
        assert "yoho_fps" in msg and text in msg, (text, msg)
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((d2 == -3.0).all())         # nothing was launched
    # k = 0 is valid and launches nothing, whatever start is; dist2 may be NULL
    assert lib.yoho_fps(*a(k=0, start=99)) == 0 and lib.yoho_fps(*a(m=0, k=0)) == 0, lib.yoho_last_error().decode()
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((d2 == -3.0).all())
    # a good call afterwards, written inside its k rows only
    want = ref(64, 8, 3)
    for path in (PATHS["one_wg"], PATHS["per_pick"]):
        assert lib.yoho_fps(*a(start=3, path=path, idx_=off(idx, 8), d2_=off(d2, 4))) == 0, lib.yoho_last_error().decode()
        torch.cuda.synchronize()
        assert np.array_equal(idx[1:9].cpu().numpy(), want[0]) and idx[0] == -7 and bool((idx[9:] == -7).all())
        assert d2[1:9].cpu().numpy().tobytes() == want[1].tobytes() and d2[0] == -3.0 and bool((d2[9:] == -3.0).all())
        idx[1:9] = -7
        d2[1:9] = -3.0
    assert lib.yoho_fps(*a(start=3, path=PATHS["per_pick"], d2_=N)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(idx[:8].cpu().numpy(), want[0]) and bool((d2 == -3.0).all())


def test_workspace_refusal_is_enomem_and_leaves_the_context_usable(hip, monkeypatch):
    """the per-pick path at 2^20 points asks for 4 MiB of running minima, refused by a context whose workspace may not exceed 1 MiB
    before anything is launched; the one-workgroup path takes no workspace and runs on the refusing context"""
    monkeypatch.setenv("YOHO_WS_LIMIT_MB", "1")
    c = hip.Context()
    monkeypatch.delenv("YOHO_WS_LIMIT_MB")
    p = torch.zeros((1 << 20, 3), dtype=torch.float32, device="cuda")
    with pytest.raises(hip.YohoError) as e:
        c.fps(p, 4, path="per_pick")
    assert e.value.code == ENOMEM and "workspace" in str(e.value)
    m = 2 * B + 7
    check(c, cloud(m), 40, 0, ref(m, 40, 0), "after the refusal")


# ---- the module and the extractor -------------------------------------------------------------------------------------------------------
def test_select_candidates_and_coverage(ctx):
    from yoho_amd import keypoints
    pc = synth.surface_cloud(6000, seed=5)
    pc_d = cu(pc)
    sel, pts = keypoints.candidates(ctx, pc_d, 0.05)
    want_sel = KR.voxel_first_ref(pc, 0.05)
    assert np.array_equal(sel.cpu().numpy(), want_sel) and np.array_equal(pts.cpu().numpy(), pc[want_sel].astype(f32)) and len(want_sel) < 6000
    sel, pts = keypoints.candidates(ctx, pc_d, None)
    assert np.array_equal(sel.cpu().numpy(), np.arange(6000)) and np.array_equal(pts.cpu().numpy(), pc.astype(f32))
    for voxel, start in ((0.05, 0), (None, 11)):
        kidx, d2 = keypoints.select(ctx, pc_d, 150, voxel=voxel, start=start)
        assert np.array_equal(kidx.cpu().numpy(), KR.select_ref(pc, 150, voxel=voxel, start=start))
    kidx, d2 = keypoints.select(ctx, pc_d, 10 ** 6, voxel=0.2)                                   # more keypoints than candidates: all of them
    assert sorted(kidx.cpu().numpy().tolist()) == KR.voxel_first_ref(pc, 0.2).tolist()
    # the coverage radius of a selection over its own candidates is what the next pick would have had
    p32 = cu(pc.astype(f32))
    kidx, d2 = keypoints.select(ctx, pc_d, 151, voxel=None)
    r = keypoints.coverage_radius(ctx, p32, p32[kidx[:150]].contiguous())
    assert r == float(np.sqrt(np.float64(d2[150].item())))
    rnd = np.random.RandomState(0).permutation(6000)[:150]
    assert r < keypoints.coverage_radius(ctx, p32, p32[cu(rnd)].contiguous())


class StubFCGF:               # as tests/test_gpu_dropin.py: any object with run(pc, voxel_size) can stand in for the backbone
    def run(self, pc, voxel_size):
        ds = pc[::3].astype(np.float32)
        rs = np.random.RandomState(len(ds))
        f = rs.randn(len(ds), 32).astype(np.float32)
        return ds, f / np.linalg.norm(f, axis=1, keepdims=True)


def same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_extractor_with_a_stub_backbone(sd1):
    from yoho_amd.yoho_extract import yoho_extractor
    pc = np.random.RandomState(0).rand(3000, 3)
    want = KR.select_ref(pc, 200, voxel=0.025)
    assert len(want) == 200
    ex = yoho_extractor(yoho_ckpt=sd1, fcgf=StubFCGF(), keypoints="fps")
    np.random.seed(5)
    state = np.random.get_state()
    kpts, inv, eqv = ex.run(pc, voxel_size=0.025, nkpts=200)
    assert same_state(state, np.random.get_state())                                                # no draw from the global generator
    assert np.array_equal(kpts, pc[want]) and tuple(inv.shape) == (200, 32) and tuple(eqv.shape) == (200, 32, 60)
    k2, i2, e2 = ex.run(pc, voxel_size=0.025, nkpts=100)
    assert np.array_equal(k2, kpts[:100]) and torch.equal(i2, inv[:100]) and torch.equal(e2, eqv[:100])    # a prefix, rows and all
    coarse = yoho_extractor(yoho_ckpt=sd1, fcgf=StubFCGF(), keypoints="fps", keypoint_voxel=0.1)
    assert np.array_equal(coarse.run(pc, voxel_size=0.025, nkpts=50)[0], pc[KR.select_ref(pc, 50, voxel=0.1)])
    # the default is the reference's draw, as before
    rnd = yoho_extractor(yoho_ckpt=sd1, fcgf=StubFCGF())
    assert rnd.keypoints == "random"
    np.random.seed(5)
    kr = rnd.run(pc, voxel_size=0.025, nkpts=200)[0]
    np.random.seed(5)
    assert np.array_equal(kr, pc[np.random.permutation(len(pc))[0:200]])
    with pytest.raises(ValueError):
        yoho_extractor(yoho_ckpt=sd1, fcgf=StubFCGF(), keypoints="grid")


def test_extractor_with_the_hip_backbone(sd1, monkeypatch):
    """the lane pipeline: the keypoints are the reference selection, and the keypoint source changes nothing else - the group features
    are the bytes of a "random" run that is handed the same indices; run_many yields what run returns"""
    from yoho_amd.yoho_extract import yoho_extractor
    fsd = W.synth_state_dict(W.FCGF_SPEC, 3)
    ck = {"config": {"model": "ResUNetBN2C", "model_n_out": 32, "normalize_feature": True, "conv1_kernel_size": 7},
          "state_dict": {k: torch.from_numpy(np.array(v)) for k, v in fsd.items()}}
    pcs = [synth.surface_cloud(2500, seed=3), synth.surface_cloud(2300, seed=4)]
    pc = pcs[0]
    want = KR.select_ref(pc, 64, voxel=0.025)
    ex = yoho_extractor(fcgf_ckpt=ck, yoho_ckpt=sd1, keypoints="fps")
    state = np.random.get_state()
    kpts, inv, eqv = ex.run(pc, voxel_size=0.025, nkpts=64)
    assert same_state(state, np.random.get_state())
    assert np.array_equal(kpts, pc[want]) and tuple(eqv.shape) == (64, 32, 60)
    feats = ex._last_group_feats.clone()
    one = [(kpts, inv, eqv), ex.run(pcs[1], voxel_size=0.025, nkpts=64)]
    assert np.array_equal(one[1][0], pcs[1][KR.select_ref(pcs[1], 64, voxel=0.025)])
    many = list(ex.run_many(pcs, voxel_size=0.025, nkpts=64))
    assert len(many) == 2
    for a, b in zip(one, many):
        assert np.array_equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert same_state(state, np.random.get_state())
    # the same indices through the random path
    rnd = yoho_extractor(fcgf_ckpt=ck, yoho_ckpt=sd1)
    rest = np.setdiff1d(np.arange(len(pc)), want)
    monkeypatch.setattr(np.random, "permutation", lambda n: np.concatenate([want, rest]))
    k3, i3, e3 = rnd.run(pc, voxel_size=0.025, nkpts=64)
    monkeypatch.undo()
    assert np.array_equal(k3, kpts)
    assert rnd._last_group_feats.cpu().numpy().tobytes() == feats.cpu().numpy().tobytes()
    assert torch.equal(i3, inv) and torch.equal(e3, eqv)
