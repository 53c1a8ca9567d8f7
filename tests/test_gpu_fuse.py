"""yoho_fuse_clouds on the GPU (-m gpu): every output as bytes against the numpy restatement of the contract (tests/fuse_ref.py) - sizes
around the sort's 256-point blocks and the scan's tiles, fragment counts across the 64-entry table, cells that make all eight digit
passes move, the filters, capacities with guard bytes, the optional arguments, repeats over poisoned scratch and another stream, the
refusals through raw ctypes, the workspace limit in a child process, and the Python wrappers.  Nothing here has a tolerance."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuse_ref as FR  # noqa: E402
from test_gpu_verify import PATTERNS, cu  # noqa: E402

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOMEM = -1, -4
f32, f64 = np.float32, np.float64
GUARD = 3                                                               # rows of 0x7B bytes behind every output
OUT_KEYS = ("pts", "normals", "count", "nfrag")


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.Context()


def raw(hip, ctx, src, soff, T, voxel, mc=1, mf=1, nrm=None, cap=None, want_nrm=None, want_row_of=True, ref=None):
    """one call through the C ABI on buffers with guard rows -> fuse_ref's dict, cut to min(M, cap) rows; cap None: the reference's M.
    Asserts that nothing at or behind row min(M, cap) of any output, and nothing behind row_of's S rows, was written."""
    lib = hip.load_library()
    S = src.shape[0]
    want_nrm = (nrm is not None) if want_nrm is None else want_nrm
    if cap is None:
        cap = (ref if ref is not None else FR.fuse_ref(src, soff, T, voxel, mc, mf))["M"]
    src_d, T_d = cu(np.asarray(src, f32)), cu(np.ascontiguousarray(T, f64))
    nrm_d = cu(np.asarray(nrm, f32)) if nrm is not None else None
    soff = np.ascontiguousarray(soff, np.int32)
    fill = lambda rows, cols, dt: torch.full((rows * cols * 4,), 0x7B, dtype=torch.uint8, device="cuda").view(dt).reshape((rows, cols) if cols > 1 else (rows,))      # noqa: E731
    pts, onr = fill(cap + GUARD, 3, torch.float32), fill(cap + GUARD, 3, torch.float32)
    cnt, nfr, rof = fill(cap + GUARD, 1, torch.int32), fill(cap + GUARD, 1, torch.int32), fill(S + GUARD, 1, torch.int32)
    n_out = torch.full((2,), -99, dtype=torch.int64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())                              # noqa: E731
    rc = lib.yoho_fuse_clouds(ctx._h, p(src_d), soff.ctypes.data_as(C.c_void_p), len(soff) - 1, p(T_d), p(nrm_d) if nrm is not None else None, float(voxel), mc, mf,
                              p(pts) if cap else None, p(onr) if want_nrm and cap else None, p(cnt) if cap else None, p(nfr) if cap else None,
                              p(rof) if want_row_of else None, cap, p(n_out), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.yoho_last_error().decode()
    torch.cuda.current_stream().synchronize()
    M = int(n_out[0])
    assert int(n_out[1]) == -99
    m = min(M, cap)
    g = np.uint8(0x7B)
    for name, t in (("pts", pts), ("normals", onr), ("count", cnt), ("nfrag", nfr)):
        lo = m if (name != "normals" or want_nrm) else 0
        assert (t[lo:].contiguous().view(torch.uint8).cpu().numpy() == g).all(), (name, "written at or behind row", lo)
    assert (rof[S if want_row_of else 0:].contiguous().view(torch.uint8).cpu().numpy() == g).all(), "row_of guard"
    return {"pts": pts[:m].cpu().numpy(), "normals": onr[:m].cpu().numpy() if want_nrm else None, "count": cnt[:m].cpu().numpy(),
            "nfrag": nfr[:m].cpu().numpy(), "row_of": rof[:S].cpu().numpy() if want_row_of else None, "M": M}


def cut(ref, m, want_nrm=True, want_row_of=True):
    """the reference cut to its first m rows (row_of whole)"""
    out = {k: (None if ref[k] is None else ref[k][:m]) for k in OUT_KEYS}
    if not want_nrm:
        out["normals"] = None
    out["row_of"] = ref["row_of"] if want_row_of else None
    out["M"] = ref["M"]
    return out


# ---- sizes -------------------------------------------------------------------------------------------------------------------------------
def size_case(S, mode, seed):
    """S points in two fragments (one when S = 1) under generic poses.  mode 'own': every point a voxel of its own - the points of a
    jittered lattice of side 2, voxel 1, in random order; 'one': all points in one voxel - the points within 1 cm of a spot 3 m from
    the origin, voxel 8; 'runs': about 40 points per voxel, so that runs straddle the sort's 256-point blocks"""
    rs = np.random.RandomState(seed)
    X = [FR.pose(rs.randn(3), 70.0 * rs.rand(), rs.randn(3)) for _ in range(2)]
    if mode == "own":
        side = int(np.ceil(S ** (1 / 3.0)))
        cells = np.stack(np.unravel_index(rs.permutation(side ** 3)[:S], (side,) * 3), axis=1) - side // 2
        world, voxel = cells * 2.0 + 0.5 + 0.2 * (rs.rand(S, 3) - 0.5), 1.0
    elif mode == "one":
        world, voxel = np.array([3.0, 3.0, 3.0]) + 0.01 * rs.rand(S, 3), 8.0
    else:
        side = max(1.0, (S / 40.0) ** (1 / 3.0))
        world, voxel = (rs.rand(S, 3) - 0.5) * side, 1.0
    n0 = S // 2 if S > 1 else 1
    parts = [world[:n0], world[n0:]] if S > 1 else [world]
    clouds = [((w - X[k][:3, 3]) @ X[k][:3, :3]).astype(f32) for k, w in enumerate(parts)]
    return np.concatenate(clouds), FR.soff_of(clouds), np.stack(X[:len(parts)])[:, :3, :], voxel, rs.randn(S, 3).astype(f32)


@pytest.mark.parametrize("mode", ["own", "one", "runs"])
@pytest.mark.parametrize("S", [1, 255, 256, 257, 1023, 70001])
def test_sizes_around_the_blocks(hip, ctx, S, mode):
    src, soff, T, voxel, nrm = size_case(S, mode, S + len(mode))
    ref = FR.fuse_ref(src, soff, T, voxel, 1, 1, nrm)
    if mode == "own":
        assert ref["M"] == S and (ref["count"] == 1).all()
    if mode == "one":
        assert ref["M"] == 1 and ref["count"][0] == S                  # S = 70 001: a run longer than any block
    if mode == "runs" and S >= 1023:
        assert ref["count"].max() > 20 and ref["M"] > 8
    got = raw(hip, ctx, src, soff, T, voxel, 1, 1, nrm, ref=ref)
    assert FR.same_bytes(got, ref) == [], (S, mode)


# ---- fragment counts and filters ------------------------------------------------------------------------------------------------------------
_FRAGS = {}


def frag_case(K):
    """K fragments of 1 .. 700 points (the first of 1, the second of 700 when there is one), every fragment a random part of one
    surface of a 2 m room stored in its own frame; the first and the last fragment both hold the point (0.31, 0.32, 0.33) of the room"""
    if K not in _FRAGS:
        rs = np.random.RandomState(500 + K)
        lens = [1, 700][:K] + [int(1 + 699 * rs.rand()) for _ in range(max(K - 2, 0))]
        room = np.stack([rs.rand(4000) * 2, rs.rand(4000) * 2, 0.02 * rs.randn(4000)], axis=1)
        spot = np.array([0.31, 0.32, 0.33])
        clouds, Ts = [], []
        for k, n in enumerate(lens):
            X = FR.pose(rs.randn(3), 180.0 * rs.rand(), rs.randn(3))
            w = room[rs.randint(4000, size=n)] + 0.002 * rs.randn(n, 3)
            if k in (0, K - 1):
                w[-1] = spot
            clouds.append(((w - X[:3, 3]) @ X[:3, :3]).astype(f32))
            Ts.append(X[:3])
        _FRAGS[K] = (np.concatenate(clouds), FR.soff_of(clouds), np.stack(Ts), 0.05)
    return _FRAGS[K]


@pytest.mark.parametrize("K", [1, 2, 64, 65, 130])
def test_fragment_counts_across_the_table_and_the_filters(hip, ctx, K):
    src, soff, T, voxel = frag_case(K)
    S = src.shape[0]
    nrm = np.random.RandomState(K).randn(S, 3).astype(f32)
    base = FR.fuse_ref(src, soff, T, voxel, 1, 1, nrm)
    if K >= 2:
        assert base["row_of"][0] == base["row_of"][S - 1] >= 0         # one voxel fed by the first and the last fragment
        assert base["nfrag"].max() >= min(K, 3)
    for mc in (1, 2, 3):
        for mf in (1, 2, 3):
            ref = base if (mc, mf) == (1, 1) else FR.fuse_ref(src, soff, T, voxel, mc, mf, nrm)
            got = raw(hip, ctx, src, soff, T, voxel, mc, mf, nrm, ref=ref)
            assert FR.same_bytes(got, ref) == [], (K, mc, mf)
            assert K < 64 or ref["M"] < base["M"] or (mc, mf) == (1, 1)


# ---- digit passes ---------------------------------------------------------------------------------------------------------------------------
def test_every_digit_pass_moves_something(hip, ctx):
    """cells over the whole range on every axis, the corners +-(2^20 - 1) and one step beyond them: 63 key bits and the outside bit,
    so all eight digit passes run, and every digit of the packed key takes more than one value"""
    rs = np.random.RandomState(11)
    lim = (1 << 20) - 1
    cells = rs.randint(-lim, lim + 1, size=(3000, 3))
    cells[:8] = [[lim, lim, lim], [-lim, -lim, -lim], [lim + 1, 0, 0], [0, -lim - 1, 0], [0, 0, lim + 1], [lim, -lim, 5], [-lim - 1, lim, lim], [-lim, 7, lim]]
    cells = np.concatenate([cells, cells[100:400]])                     # some voxels twice, from the second fragment
    voxel = 0.25
    src = (cells * voxel + voxel / 2).astype(f32)                       # exact in f32: 21 + 3 bits
    assert np.array_equal(np.floor(src.astype(f64) / voxel), cells)
    soff = np.array([0, 3000, 3300], np.int32)
    T = np.tile(np.eye(4)[:3], (2, 1, 1))
    ref = FR.fuse_ref(src, soff, T, voxel)
    inside = ref["row_of"] >= 0
    assert (~inside).sum() == 4 and ref["nfrag"].max() == 2
    packed = sum((cells[inside, a] + lim).astype(np.uint64) << np.uint64(21 * a) for a in range(3))
    packed = np.concatenate([packed, [np.uint64(1) << np.uint64(63)]])
    for d in range(8):
        assert len(np.unique((packed >> np.uint64(8 * d)) & np.uint64(255))) > 1, d
    for mf in (1, 2):
        r = ref if mf == 1 else FR.fuse_ref(src, soff, T, voxel, 1, 2)
        assert FR.same_bytes(raw(hip, ctx, src, soff, T, voxel, 1, mf, ref=r), r) == [], mf


# ---- capacity and the optional arguments ----------------------------------------------------------------------------------------------------
def test_capacity_and_optional_arguments(hip, ctx):
    src, soff, T, voxel = frag_case(65)
    nrm = np.random.RandomState(1).randn(src.shape[0], 3).astype(f32)
    ref = FR.fuse_ref(src, soff, T, voxel, 2, 2, nrm)
    M = ref["M"]
    assert M > 10
    for cap in (0, M - 1, M, M + 5):
        got = raw(hip, ctx, src, soff, T, voxel, 2, 2, nrm, cap=cap)
        assert got["M"] == M and FR.same_bytes(got, cut(ref, min(M, cap))) == [], cap
    for has_nrm, want_nrm in ((True, True), (True, False), (False, False)):
        for want_row_of in (True, False):
            got = raw(hip, ctx, src, soff, T, voxel, 2, 2, nrm if has_nrm else None, cap=M, want_nrm=want_nrm, want_row_of=want_row_of)
            assert FR.same_bytes(got, cut(ref, M, want_nrm, want_row_of)) == [], (has_nrm, want_nrm, want_row_of)
    # a count-only call may still ask for row_of, and gets all of it
    got = raw(hip, ctx, src, soff, T, voxel, 2, 2, None, cap=0, want_row_of=True)
    assert got["row_of"].tobytes() == ref["row_of"].tobytes() and got["row_of"].max() == M - 1


# ---- determinism ----------------------------------------------------------------------------------------------------------------------------
def test_bits_repeat_over_poisoned_scratch_streams_and_contexts(hip, ctx):
    src, soff, T, voxel = frag_case(130)
    nrm = np.random.RandomState(2).randn(src.shape[0], 3).astype(f32)
    ref = FR.fuse_ref(src, soff, T, voxel, 1, 2, nrm)
    small = size_case(257, "runs", 9)
    ref_small = FR.fuse_ref(*small[:4], 1, 1, small[4])
    for rep in range(5):                                               # five repeats, the scratch left as the call before left it
        assert FR.same_bytes(raw(hip, ctx, src, soff, T, voxel, 1, 2, nrm, ref=ref), ref) == [], rep
    cx = hip.Context()
    for pat in PATTERNS:
        cx.poison_scratch(pat)
        assert FR.same_bytes(raw(hip, cx, src, soff, T, voxel, 1, 2, nrm, ref=ref), ref) == [], hex(pat)
        cx.poison_scratch(pat)
        assert FR.same_bytes(raw(hip, cx, *small[:4], 1, 1, small[4], ref=ref_small), ref_small) == [], hex(pat)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side
        assert FR.same_bytes(raw(hip, ctx, src, soff, T, voxel, 1, 2, nrm, ref=ref), ref) == []
    torch.cuda.synchronize()


# ---- the C ABI's refusals ------------------------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_arguments(ctx, hip):
    lib = hip.load_library()
    h = ctx._h
    rs = np.random.RandomState(3)
    src_h = rs.rand(30, 3).astype(f32)
    s, n = cu(src_h), cu(rs.randn(30, 3).astype(f32))
    T = cu(np.tile(np.eye(4)[:3], (4, 1, 1)))
    pts = torch.full((40, 3), -3.0, dtype=torch.float32, device="cuda")
    onr = torch.full((40, 3), -3.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((40,), -7, dtype=torch.int32, device="cuda")
    nfr = torch.full((40,), -7, dtype=torch.int32, device="cuda")
    rof = torch.full((40,), -7, dtype=torch.int32, device="cuda")
    nout = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())                              # noqa: E731
    off = lambda x, nbytes: C.c_void_p(x.data_ptr() + nbytes)           # noqa: E731
    N, d = None, C.c_double
    big = hip.REFINE_MAX_POINTS + 1
    keep = []

    def so(*v):
        a = np.array(v, np.int32)
        keep.append(a)
        return a.ctypes.data_as(C.c_void_p)

    def fc(ctx_=h, src=p(s), soff=None, K=2, T_=p(T), nrm=p(n), voxel=d(0.1), mc=1, mf=1, pts_=p(pts), onr_=p(onr), cnt_=p(cnt), nfr_=p(nfr), rof_=p(rof),
           cap=30, nout_=p(nout)):
        return (ctx_, src, so(0, 9, 30) if soff is None else soff, K, T_, nrm, voxel, mc, mf, pts_, onr_, cnt_, nfr_, rof_, cap, nout_, N)

    rows = [
        (fc(ctx_=N), "bad argument"),
        (fc(src=N), "NULL"), (fc(soff=C.c_void_p(None)), "NULL"), (fc(T_=N), "NULL"), (fc(nout_=N), "NULL"),
        (fc(pts_=N), "NULL"), (fc(cnt_=N), "NULL"), (fc(nfr_=N), "NULL"),
        (fc(nrm=N), "out_nrm"),                                         # out_nrm without nrm
        (fc(K=0), "K=0"), (fc(K=-1), "K=-1"), (fc(K=1025, soff=so(*range(1026))), "YOHO_FUSE_MAX_K"),
        (fc(voxel=d(0.0)), "voxel"), (fc(voxel=d(-0.1)), "voxel"), (fc(voxel=d(np.inf)), "voxel"), (fc(voxel=d(np.nan)), "voxel"),
        (fc(mc=0), "min_count=0"), (fc(mf=0), "min_frags=0"), (fc(mc=-2), "min_count=-2"), (fc(mf=-1), "min_frags=-1"),
        (fc(cap=-1), "capacity=-1"),
        (fc(soff=so(1, 9, 30)), "soff[0]=1"),
        (fc(soff=so(0, 9, 9)), "strictly increasing"), (fc(soff=so(0, 0, 30)), "strictly increasing"), (fc(soff=so(0, 20, 9)), "strictly increasing"),
        (fc(soff=so(0, -5, 30)), "strictly increasing"),
        (fc(soff=so(0, big, big + 1)), "YOHO_REFINE_MAX_POINTS"),
        (fc(K=17, soff=so(*[k * hip.REFINE_MAX_POINTS for k in range(18)])), "YOHO_FUSE_MAX_POINTS"),
        (fc(src=off(s, 2)), "4-byte aligned"), (fc(nrm=off(n, 1)), "4-byte aligned"), (fc(T_=off(T, 4)), "8-byte aligned"), (fc(pts_=off(pts, 2)), "4-byte aligned"),
        (fc(onr_=off(onr, 2)), "4-byte aligned"), (fc(cnt_=off(cnt, 2)), "4-byte aligned"), (fc(nfr_=off(nfr, 1)), "4-byte aligned"),
        (fc(rof_=off(rof, 2)), "4-byte aligned"), (fc(nout_=off(nout, 4)), "8-byte aligned"),
    ]
    assert hip.FUSE_SYMBOLS == ["yoho_fuse_clouds"]
    for args, text in rows:
        rc = lib.yoho_fuse_clouds(*args)
        msg = lib.yoho_last_error().decode()
        assert rc == EINVAL, (text, rc, msg)
        assert "yoho_fuse_clouds" in msg and text in msg, (text, msg)
    torch.cuda.synchronize()
    # nothing was launched: every output keeps its pattern
    assert bool((pts == -3.0).all()) and bool((onr == -3.0).all()) and all(bool((x == -7).all()) for x in (cnt, nfr, rof, nout))
    # the context works as before: rows of 12 bytes that are not 16-byte aligned, outputs inside their rows only
    assert lib.yoho_fuse_clouds(*fc(src=off(s, 12), soff=so(0, 9, 29), T_=off(T, 96), nrm=off(n, 12), pts_=off(pts, 12), onr_=off(onr, 12), cnt_=off(cnt, 4),
                                    nfr_=off(nfr, 4), rof_=off(rof, 4), nout_=off(nout, 8), voxel=d(0.3), cap=38)) == 0, lib.yoho_last_error().decode()
    torch.cuda.synchronize()
    ref = FR.fuse_ref(src_h[1:], [0, 9, 29], np.tile(np.eye(4)[:3], (2, 1, 1)), 0.3, 1, 1, n.cpu().numpy()[1:])
    M = ref["M"]
    assert 2 < M < 29 and int(nout[1]) == M and int(nout[0]) == -7
    got = {"pts": pts[1:1 + M].cpu().numpy(), "normals": onr[1:1 + M].cpu().numpy(), "count": cnt[1:1 + M].cpu().numpy(), "nfrag": nfr[1:1 + M].cpu().numpy(),
           "row_of": rof[1:30].cpu().numpy(), "M": M}
    assert FR.same_bytes(got, ref) == []
    assert bool((pts[0] == -3.0).all()) and bool((pts[1 + M:] == -3.0).all()) and cnt[0] == -7 and bool((cnt[1 + M:] == -7).all())
    assert rof[0] == -7 and bool((rof[30:] == -7).all())
    # the binding refuses a table that does not cover src before the library sees it
    with pytest.raises(ValueError):
        ctx.fuse_clouds(s, np.array([0, 9, 29], np.int32), T[:2], 0.1)


CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import fuse_ref as FR
from yoho_amd import hip
cx = hip.Context()
rs = np.random.RandomState(0)
big = torch.from_numpy(rs.rand(200000, 3).astype(np.float32)).cuda()
T = torch.from_numpy(np.tile(np.eye(4)[:3], (2, 1, 1))).cuda()
try:
    cx.fuse_clouds(big, np.array([0, 100000, 200000], np.int32), T, 0.01)
    print("NOT REFUSED")
except hip.YohoError as e:
    print("CODE", e.code, "workspace" in str(e))
small = rs.rand(300, 3).astype(np.float32)
out = cx.fuse_clouds(torch.from_numpy(small).cuda(), np.array([0, 100, 300], np.int32), T, 0.2, nrm=None)
ref = FR.fuse_ref(small, [0, 100, 300], np.tile(np.eye(4)[:3], (2, 1, 1)), 0.2)
got = {k: (None if out[k] is None else out[k].cpu().numpy()) for k in FR.KEYS}
got["M"] = out["M"]
print("AFTER", FR.same_bytes(got, ref), ref["M"])
"""


def test_workspace_refusal_in_a_fresh_process(tmp_path):
    """YOHO_WS_LIMIT_MB=1 in a child process of its own (the limit is read when a context is created): 200 000 points ask for about
    8 MB, the entry returns YOHO_ENOMEM, and the same context then fuses 300 points correctly"""
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, YOHO_WS_LIMIT_MB="1")
    r = subprocess.run([sys.executable, str(script), REPO], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[0] == f"CODE {ENOMEM} True", r.stdout
    assert lines[1].startswith("AFTER [] ") and int(lines[1].split()[-1]) > 10, r.stdout


# ---- the Python wrappers --------------------------------------------------------------------------------------------------------------------
def test_fuse_registered_on_the_ghost_scene(ctx):
    """fuse.fuse_registered on the CPU test's ghost scene, the result dict of register_scene standing in with the scene's poses and one
    unreached (NaN) fragment: the restatement's result, per fragment; min_frags = 2 removes the ghost exactly"""
    from yoho_amd import fuse as FU
    g = FR.ghost_scene()
    poses = g["poses"].copy()
    poses[2] = np.nan
    clouds_d = [cu(c) for c in g["clouds"]]
    src, soff, k = np.concatenate(g["clouds"]), FR.soff_of(g["clouds"]), g["ghost"]
    for mf in (1, 2):
        ref = FR.fuse_ref(src, soff, poses[:, :3, :], g["voxel"], 1, mf)
        out = FU.fuse_registered(ctx, clouds_d, ({"npairs": None}, {"poses": poses}) if mf == 1 else {"poses": poses}, g["voxel"], min_frags=mf)
        assert out["M"] == ref["M"] and out["normals"] is None and len(out["row_of"]) == 7
        got = {"pts": out["pts"].cpu().numpy(), "normals": None, "count": out["count"].cpu().numpy(), "nfrag": out["nfrag"].cpu().numpy(),
               "row_of": torch.cat(out["row_of"]).cpu().numpy(), "M": out["M"]}
        assert FR.same_bytes(got, ref) == [], mf
        assert bool((out["row_of"][2] == -1).all())                    # the unreached fragment
        assert bool((out["row_of"][k] == -1).all()) if mf == 2 else bool((out["row_of"][k] >= 0).all())
    # normals and f64 clouds are taken too
    nrm = [cu(np.random.RandomState(f).randn(len(c), 3).astype(f32)) for f, c in enumerate(g["clouds"])]
    out = FU.fuse_clouds(ctx, [c.to(torch.float64) for c in clouds_d], poses, g["voxel"], min_frags=2, normals=nrm)
    ref = FR.fuse_ref(src, soff, poses[:, :3, :], g["voxel"], 1, 2, torch.cat(nrm).cpu().numpy())
    assert out["normals"].cpu().numpy().tobytes() == ref["normals"].tobytes() and out["pts"].cpu().numpy().tobytes() == ref["pts"].tobytes()


def test_context_reads_the_count_once_or_not_at_all(ctx, monkeypatch):
    src, soff, T, voxel = frag_case(64)
    ref = FR.fuse_ref(src, soff, T, voxel, 1, 2)
    src_d, T_d = cu(src), cu(T)
    torch.cuda.synchronize()
    reads = []
    for name in ("item", "cpu", "tolist", "numpy", "__int__", "__index__", "__bool__"):
        orig = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, (lambda o, nm: lambda self, *a, **k: (reads.append(nm), o(self, *a, **k))[1])(orig, name))
    out = ctx.fuse_clouds(src_d, soff, T_d, voxel, 1, 2)
    assert reads == ["item"], reads
    del reads[:]
    cap = ref["M"] + 5
    out2 = ctx.fuse_clouds(src_d, soff, T_d, voxel, 1, 2, capacity=cap)
    assert reads == [], reads
    monkeypatch.undo()
    assert out["M"] == ref["M"] and isinstance(out2["M"], torch.Tensor) and int(out2["M"][0]) == ref["M"] and out2["pts"].shape[0] == cap
    for k in OUT_KEYS[:1] + OUT_KEYS[2:]:
        assert out[k].cpu().numpy().tobytes() == ref[k].tobytes() == out2[k][:ref["M"]].cpu().numpy().tobytes(), k
    assert out["row_of"].cpu().numpy().tobytes() == ref["row_of"].tobytes() == out2["row_of"].cpu().numpy().tobytes()
