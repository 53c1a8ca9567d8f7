"""The density-cluster entry on the GPU (-m gpu): yoho_dbscan against the numpy restatement of its contract (tests/cluster_ref.py).
Everything it returns is an integer: labels, count, core, sizes and n_out are compared for equality, count also with the count-only
yoho_knn_within call it is defined by.  The cases are those tests/test_cluster_cpu.py holds the restatement itself to."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_ref as CL  # noqa: E402

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOMEM = -1, -4
f32, f64 = np.float32, np.float64
KEYS = ("labels", "count", "core", "sizes", "n")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.Context()


def device_dbscan(c, pts, eps, min_pts, **want):
    r = c.dbscan(cu(pts), eps, min_pts, **want)
    n = pts.shape[0]
    assert r["labels"].dtype == torch.int32 and tuple(r["labels"].shape) == (n,) and r["n"].dtype == torch.int32 and tuple(r["n"].shape) == (3,)
    assert r["count"] is None or (r["count"].dtype == torch.int32 and tuple(r["count"].shape) == (n,))
    assert r["core"] is None or (r["core"].dtype == torch.uint8 and tuple(r["core"].shape) == (n,))
    assert r["sizes"] is None or (r["sizes"].dtype == torch.int32 and tuple(r["sizes"].shape) == (n,))
    return {k: (None if v is None else v.cpu().numpy()) for k, v in r.items()}


def check(c, pts, eps, min_pts, what="", ref=None):
    """device == restatement, every output as integers -> the reference"""
    ref = CL.dbscan_ref(pts, eps, min_pts) if ref is None else ref
    got = device_dbscan(c, pts, eps, min_pts)
    for k in KEYS:
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (what, k, min_pts, np.nonzero(got[k] != ref[k])[0][:8])
    return ref


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 1023])
def test_dbscan_sizes_and_densities(ctx, N):
    """a mixed cloud of surface, clumps, duplicates and far points (1e6 r away, and 3e6 r away in the grid's clamped cells) at both
    sides of the block size, from Euclidean components (min_pts = 1) to all noise (min_pts = N + 1)"""
    r = 0.1
    pts = CL.mixed_cloud(N, r)
    count = ctx.knn_within(cu(pts), cu(pts), r, 1, skip_same_row=True, want_idx=False, want_d2=False)[2].cpu().numpy()
    seen = set()
    for min_pts in (1, 4, 16, N + 1):
        ref = check(ctx, pts, r, min_pts, f"N={N}")
        assert ref["count"].tobytes() == count.tobytes()
        seen |= {("core", bool(ref["n"][1])), ("noise", bool(ref["n"][2])), ("border", bool(((ref["core"] == 0) & (ref["labels"] >= 0)).any()))}
        if min_pts == N + 1:
            assert ref["n"].tolist() == [0, 0, N] and (ref["sizes"] == 0).all()
        if min_pts == 1:
            assert ref["n"][1] == N and ref["n"][2] == 0
    if N >= 255:
        assert seen == {(k, b) for k in ("core", "noise", "border") for b in (False, True)}


# ---- chains --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["ascending", "descending", "rotated", "shuffled_row0_end", "shuffled_row0_middle"])
def test_the_snake_is_one_cluster_in_every_row_order(ctx, order):
    """2049 points 0.9 eps apart along a polyline through more than a thousand cells and nine workgroups: one cluster, label 0, whatever
    the order of the rows - the shape on which a propagation that needs a round per hop, or a union that trusts a stale parent, fails"""
    eps = 0.05
    pts = CL.snake(2049, eps)[CL.snake_orders(2049)[order]]
    for min_pts in (1, 3):
        ref = check(ctx, pts, eps, min_pts, order)
        assert (ref["labels"] == 0).all() and ref["n"].tolist() == [1, 2049 if min_pts == 1 else 2047, 0] and ref["sizes"][0] == 2049


@pytest.mark.parametrize("swap", [False, True])
def test_two_snakes_and_a_bridge(ctx, swap):
    """two chains 1.1 eps apart stay two clusters; a point within eps of one row of each joins its nearer core neighbour's cluster while
    it is not core (min_pts = 4: it has two neighbours) and makes them one when it is (min_pts = 3)"""
    eps = 0.05
    pts, lo, up, _ = CL.two_snakes(eps, swap=swap)
    ref = check(ctx, pts, eps, 4, "two snakes")
    assert ref["n"][0] == 2 and (ref["labels"][lo] == (1 if swap else 0)).all() and (ref["labels"][up] == (0 if swap else 1)).all()
    pts, lo, up, b = CL.two_snakes(eps, bridge=True, swap=swap)
    ref = check(ctx, pts, eps, 4, "bridge, not core")
    assert ref["n"][0] == 2 and not ref["core"][b] and ref["labels"][b] == ref["labels"][lo[0]] != ref["labels"][up[0]]
    ref = check(ctx, pts, eps, 3, "bridge, core")
    assert ref["n"][0] == 1 and ref["core"][b] and (ref["labels"] == 0).all()


def test_ties_the_gate_and_duplicates(ctx):
    for swap in (False, True):                                                    # integer lattice: d2 = 1 to the core rows of two clusters
        pts, ra, rb, rp = CL.tie_cloud(swap)
        ref = check(ctx, pts, 1.2, 5, "tie")
        assert ref["labels"][rp] == ref["labels"][min(ra, rb)] == 0 and ref["labels"][max(ra, rb)] == 1 and not ref["core"][rp]
    line = np.zeros((300, 3), f32)
    line[:, 0] = 0.5 * np.arange(300)                                             # d2 == gate2: not neighbours
    ref = check(ctx, line, 0.5, 1, "gate")
    assert np.array_equal(ref["labels"], np.arange(300)) and (ref["sizes"] == 1).all() and ref["n"].tolist() == [300, 300, 0]
    assert check(ctx, line, 0.5, 2, "gate")["n"].tolist() == [0, 0, 300]
    assert check(ctx, line, np.nextafter(f32(0.5), f32(1)), 2, "above the gate")["n"].tolist() == [1, 300, 0]
    dup = np.tile(np.array([[0.25, 0.5, 0.75]], f32), (40, 1))
    for min_pts in (1, 40):
        ref = check(ctx, dup, 0.1, min_pts, "duplicates")
        assert (ref["labels"] == 0).all() and ref["sizes"][0] == 40 and ref["n"].tolist() == [1, 40, 0]
    assert check(ctx, dup, 0.1, 41, "duplicates")["n"].tolist() == [0, 0, 40]


def test_non_finite_rows_and_the_numbering(ctx):
    pts = CL.mixed_cloud(1023, 0.1)
    bad, good = CL.with_bad_rows(pts)
    rest = np.setdiff1d(np.arange(len(bad)), good)
    for min_pts in (1, 4):
        a, b = check(ctx, pts, 0.1, min_pts, "finite"), check(ctx, bad, 0.1, min_pts, "non-finite rows")
        assert (b["labels"][rest] == -1).all() and (b["count"][rest] == 0).all() and (b["core"][rest] == 0).all() and len(rest) > 100
        assert all(np.array_equal(a[k], b[k][good]) for k in ("labels", "count", "core"))
    perm = np.random.RandomState(3).permutation(1023)
    b = check(ctx, pts[perm], 0.1, 4, "permuted")
    lab = b["labels"][b["core"].astype(bool)]
    assert np.array_equal(lab[np.sort(np.unique(lab, return_index=True)[1])], np.arange(b["n"][0]))      # numbered by lowest core row
    assert not np.array_equal(a["labels"][perm], b["labels"]) and np.array_equal(a["labels"][perm] < 0, b["labels"] < 0)


# ---- outputs and determinism -----------------------------------------------------------------------------------------------------------------
def test_every_subset_of_the_optional_outputs(ctx):
    pts = CL.mixed_cloud(1023, 0.1)
    ref = check(ctx, pts, 0.1, 4)
    for wc, wk, ws in itertools.product((False, True), repeat=3):
        got = device_dbscan(ctx, pts, 0.1, 4, want_count=wc, want_core=wk, want_sizes=ws)
        assert (got["count"] is None) == (not wc) and (got["core"] is None) == (not wk) and (got["sizes"] is None) == (not ws)
        for k in KEYS:
            assert got[k] is None or got[k].tobytes() == ref[k].tobytes(), (k, wc, wk, ws)


def test_bits_repeat_over_poisoned_scratch_streams_and_contexts(hip, ctx):
    clouds = [(CL.mixed_cloud(1023, 0.1, 1), 0.1, 4), (CL.snake(2049, 0.05)[CL.snake_orders(2049, 1)["shuffled_row0_middle"]], 0.05, 3),
              (CL.mixed_cloud(257, 0.1, 2), 0.1, 1)]

    def run(c):
        out = []
        for pts, eps, min_pts in clouds:
            got = device_dbscan(c, pts, eps, min_pts)
            out += [got[k].tobytes() for k in KEYS]
        return out

    first = run(ctx)
    for rep in range(4):
        assert run(ctx) == first, rep
    cx = hip.Context()
    for pat in (0xFFFFFFFF, 0x7F7F7F7F):
        for rep in range(2):
            cx.poison_scratch(pat)                                                 # between calls: the workspace holds the pattern
            assert run(cx) == first, (hex(pat), rep)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side
        assert run(ctx) == first
    torch.cuda.synchronize()
    for k, (pts, eps, min_pts) in enumerate(clouds):
        ref = CL.dbscan_ref(pts, eps, min_pts)
        assert first[5 * k:5 * k + 5] == [ref[key].tobytes() for key in KEYS]


# ---- the C ABI's refusals ----------------------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_arguments(ctx, hip):
    lib = hip.load_library()
    h = ctx._h
    host = np.random.RandomState(3).rand(31, 3).astype(f32)
    q = cu(host)
    labels = torch.full((32,), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((32,), -7, dtype=torch.int32, device="cuda")
    core = torch.full((32,), 9, dtype=torch.uint8, device="cuda")
    sizes = torch.full((32,), -7, dtype=torch.int32, device="cuda")
    n_out = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())                              # noqa: E731
    off = lambda x, nbytes: C.c_void_p(x.data_ptr() + nbytes)           # noqa: E731
    N, fl = None, C.c_float
    big = hip.REFINE_MAX_POINTS + 1

    def db(ctx_=h, pts=p(q), n=31, eps=fl(0.2), mp=4, lab=p(labels), cnt_=p(cnt), core_=p(core), sizes_=p(sizes), n_=p(n_out)):
        return (ctx_, pts, n, eps, mp, lab, cnt_, core_, sizes_, n_, N)

    rows = [(db(ctx_=N), "bad argument"), (db(n=0), "N=0"), (db(n=-3), "N=-3"), (db(n=big), "YOHO_REFINE_MAX_POINTS"),
            (db(eps=fl(0.0)), "eps"), (db(eps=fl(-1.0)), "eps"), (db(eps=fl(np.nan)), "eps"), (db(eps=fl(np.inf)), "eps"),
            (db(mp=0), "min_pts=0"), (db(mp=-2), "min_pts=-2"), (db(pts=N), "pts is NULL"), (db(lab=N), "labels is NULL"), (db(n_=N), "n_out is NULL"),
            (db(pts=off(q, 2)), "4-byte aligned"), (db(lab=off(labels, 2)), "4-byte aligned"), (db(cnt_=off(cnt, 1)), "4-byte aligned"),
            (db(sizes_=off(sizes, 2)), "4-byte aligned"), (db(n_=off(n_out, 2)), "4-byte aligned")]
    assert hip.CLUSTER_SYMBOLS == ["yoho_dbscan"]
    for args, text in rows:
        rc = lib.yoho_dbscan(*args)
        msg = lib.yoho_last_error().decode()
        assert rc == EINVAL, (text, rc, msg)
        assert "yoho_dbscan" in msg and text in msg, (text, msg)
    torch.cuda.synchronize()
    # nothing was launched: every output keeps its pattern
    assert bool((labels == -7).all()) and bool((cnt == -7).all()) and bool((core == 9).all()) and bool((sizes == -7).all()) and bool((n_out == -7).all())
    # the context works as before: rows that are not 16-byte aligned, outputs inside their rows only; min_pts above N is valid
    assert lib.yoho_dbscan(*db(pts=off(q, 12), n=30, mp=3, lab=off(labels, 4), cnt_=off(cnt, 4), core_=off(core, 1), sizes_=off(sizes, 4), n_=off(n_out, 4))) == 0, \
        lib.yoho_last_error().decode()
    torch.cuda.synchronize()
    ref = CL.dbscan_ref(host[1:], 0.2, 3)
    for t, k, pat in ((labels, "labels", -7), (cnt, "count", -7), (core, "core", 9), (sizes, "sizes", -7)):
        assert np.array_equal(t[1:31].cpu().numpy(), ref[k]) and int(t[0]) == pat and int(t[31]) == pat, k
    assert n_out.cpu().numpy().tolist() == [-7] + ref["n"].tolist() and 0 < ref["n"][1] < 30
    assert lib.yoho_dbscan(*db(mp=2 ** 31 - 1, cnt_=N, core_=N, sizes_=N)) == 0, lib.yoho_last_error().decode()
    torch.cuda.synchronize()
    assert bool((labels[:31] == -1).all()) and n_out.cpu().numpy().tolist()[:3] == [0, 0, 31]
    # the binding refuses other shapes before the library sees them
    with pytest.raises(ValueError):
        ctx.dbscan(q[:, :2], 0.2)
    with pytest.raises(hip.YohoError, match="yoho_dbscan"):
        ctx.dbscan(q, 0.2, 0)


CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import cluster_ref as CL
from yoho_amd import hip
cx = hip.Context()
rs = np.random.RandomState(0)
big = torch.from_numpy(rs.rand(200000, 3).astype(np.float32)).cuda()
try:
    cx.dbscan(big, 0.01)
    print("NOT REFUSED")
except hip.YohoError as e:
    print("CODE", e.code, "workspace" in str(e))
small = CL.mixed_cloud(300, 0.1)
got = cx.dbscan(torch.from_numpy(small).cuda(), 0.1, 4)
ref = CL.dbscan_ref(small, 0.1, 4)
print("AFTER", all(np.array_equal(got[k].cpu().numpy(), ref[k]) for k in ref), int(ref["n"][0]))
"""


def test_workspace_refusal_in_a_fresh_process(tmp_path):
    """YOHO_WS_LIMIT_MB=1 in a child process of its own (the limit is read when a context is created): the layout over 200 000 points asks
    for more than 10 MB, the entry returns YOHO_ENOMEM, and the same context then answers 300 points correctly"""
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, YOHO_WS_LIMIT_MB="1")
    r = subprocess.run([sys.executable, str(script), REPO], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[0] == f"CODE {ENOMEM} True", r.stdout
    assert lines[1].startswith("AFTER True ") and int(lines[1].split()[-1]) > 3, r.stdout


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
def test_keep_large_and_select_on_the_motivating_cloud(ctx, seed):
    """cluster_ref.clump_cloud(seed), 20 120 / 20 360 points: the device equals the restatement; cluster.keep_large(min_size = 100) meets
    the conditions tests/test_cluster_cpu.py holds the restatement to; keypoints.select with the cluster filter, on the device from the
    f64 cloud to the cloud indices, places no pick in a clump - and one in every clump without it"""
    from test_cluster_cpu import motivating_conditions
    from yoho_amd import clean, cluster, keypoints
    pts, clump, ref = CL.motivating(seed)
    assert len(pts) == (20120, 20360)[seed]
    check(ctx, pts, 0.04, 4, "motivating", ref=ref)
    r = cluster.keep_large(ctx, cu(pts), 0.04, min_pts=4, min_size=100)
    keep = CL.keep_large_ref(ref, min_size=100)
    assert r["keep"].dtype == torch.bool and np.array_equal(r["keep"].cpu().numpy(), keep) and np.array_equal(r["sel"].cpu().numpy(), np.nonzero(keep)[0])
    assert np.array_equal(r["labels"].cpu().numpy(), ref["labels"]) and np.array_equal(r["n"].cpu().numpy(), ref["n"])
    pc_d = cu(pts.astype(f64))
    got, dist2 = keypoints.select(ctx, pc_d, 500, clean={"method": "cluster", "eps": 0.04, "min_size": 100})
    got = got.cpu().numpy()
    motivating_conditions(pts, clump, r["keep"].cpu().numpy(), got)
    kept = np.nonzero(keep)[0]
    assert np.array_equal(got, kept[CL.KR.fps_ref(pts[kept], 500, 0)[0]]) and dist2.shape == (500,)
    plain = keypoints.select(ctx, pc_d, 500)[0].cpu().numpy()
    print(f"seed {seed}: clumps picked {len(np.unique(clump[plain][clump[plain] >= 0]))} of {clump.max() + 1} without the filter, picks in clumps with it "
          f"{int((clump[got] >= 0).sum())}; clusters {ref['n'].tolist()}")
    assert len(np.unique(clump[plain][clump[plain] >= 0])) == clump.max() + 1
    sel, kept_d = clean.clean_cloud(ctx, pc_d, method="cluster", eps=0.04, min_size=100)
    assert np.array_equal(sel.cpu().numpy(), kept) and torch.equal(kept_d, pc_d[sel])
    big = cluster.keep_large(ctx, cu(pts), 0.04, largest=1)["keep"].cpu().numpy()
    assert np.array_equal(big, CL.keep_large_ref(ref, largest=1)) and 0 < big.sum() <= keep.sum()
