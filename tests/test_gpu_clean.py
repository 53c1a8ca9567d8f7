"""The outlier-filter entries on the GPU (-m gpu): yoho_knn_within and yoho_statistical_outliers against the numpy restatement of their
contracts (tests/clean_ref.py).  idx, d2 and count of the search, and keep, count and n_keep of the filter, are compared as bits;
mean_dist, mu, sigma and thr within 4 ulp (f64) - only the device's sqrt can differ from numpy's -, on inputs whose m_i stay away from
thr (clean_ref.assert_away_from_threshold).  The two identities tie the search to yoho_nn_within and yoho_knn_search, which share no
code with it.  Every comparison with a tolerance prints its figure before it asserts; profiles/clean.md records them."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_ref as CR  # noqa: E402

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOMEM = -1, -4
f32, f64 = np.float32, np.float64
KS = (1, 2, 8, 9, 16, 17, 32)                                           # both sides of every list capacity (8, 16, 32)
PATTERNS = (0xFFFFFFFF, 0x7FC00000, 0x00000001, 0xDEADBEEF, 0x7F800000)
ULPS = 4.0
_cache = {}


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.Context()


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def mixed_cloud(n, seed):
    """a cloud whose density falls steeply away from a corner, and a few far points: with radius 0.1 rows with no candidate, with a few
    and with a hundred"""
    rs = np.random.RandomState(seed)
    pts = rs.rand(n, 3) ** 3.0 * 1.2
    pts[::17] += 40.0
    return np.ascontiguousarray(pts.astype(f32))


def device_knn(c, q, tgt, r, k, skip=False, want=(True, True, True)):
    d2, idx, cnt = c.knn_within(cu(q), cu(tgt), r, k, skip_same_row=skip, want_idx=want[0], want_d2=want[1], want_count=want[2])
    assert (idx is None) == (not want[0]) and (d2 is None) == (not want[1]) and (cnt is None) == (not want[2])
    assert idx is None or (idx.dtype == torch.int64 and tuple(idx.shape) == (q.shape[0], k))
    assert d2 is None or (d2.dtype == torch.float32 and tuple(d2.shape) == (q.shape[0], k))
    assert cnt is None or (cnt.dtype == torch.int32 and tuple(cnt.shape) == (q.shape[0],))
    return tuple(None if t is None else t.cpu().numpy() for t in (idx, d2, cnt))


def check_knn(c, q, tgt, r, ks, skip=False, what=""):
    """the device against the restatement for every k of ks (the reference at k = 32, whose first k columns are k's answer) -> count"""
    ri, rd, rc = CR.knn_within_ref(q, tgt, r, CR.KNN3_MAX, skip)
    for k in ks:
        idx, d2, cnt = device_knn(c, q, tgt, r, k, skip)
        assert np.array_equal(cnt, rc), (what, k, "count")
        assert np.array_equal(idx, ri[:, :k]), (what, k, "idx")
        assert d2.tobytes() == np.ascontiguousarray(rd[:, :k]).tobytes(), (what, k, "d2")
    return rc


# ---- yoho_knn_within against the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nq,Nt", [(1, 1), (1, 1023), (255, 1023), (256, 256), (257, 255), (1023, 257), (1023, 1), (1023, 1023)])
def test_knn_within_sizes_and_list_capacities(ctx, Nq, Nt):
    tgt = mixed_cloud(Nt, 100 + Nt)
    q = mixed_cloud(Nq, 200 + Nq) if Nq > 1 else tgt[:1] + f32(0.01)
    rc = check_knn(ctx, q, tgt, 0.1, KS, what=f"Nq = {Nq}, Nt = {Nt}")
    if Nq >= 1023 and Nt >= 1023:
        assert (rc == 0).any()
        for k in KS:                                                     # rows short of k, with exactly k and beyond it
            assert ((0 < rc) & (rc < k)).any() or k == 1
            assert (rc == k).any() and (rc > k).any(), k
    if Nq == Nt:
        rs = check_knn(ctx, tgt, tgt, 0.1, KS, skip=True, what=f"N = {Nt}, the row itself skipped")
        assert np.array_equal(rs, check_knn(ctx, tgt, tgt, 0.1, (3,), what="self") - 1)
    check_knn(ctx, q, tgt, 100.0, (1, 9, 32), what="one cell holds the whole cloud")


def test_knn_within_identities_with_nn_within_and_knn_search(ctx):
    """column 0 is yoho_nn_within's (idx, d2) bit for bit; a row whose k-th d2 is below the gate is yoho_knn_search(D = 3, squared)'s"""
    q, tgt = mixed_cloud(700, 1), mixed_cloud(1023, 2)
    tq, tt = cu(q), cu(tgt)
    for r in (0.05, 0.1, 0.4):
        nd, ni = ctx.nn_within(tq, tt, r)
        for k in (1, 5, 16, 32):
            d2, idx, cnt = ctx.knn_within(tq, tt, r, k)
            assert torch.equal(idx[:, 0], ni) and torch.equal(d2[:, 0].view(torch.int32), nd.view(torch.int32)), (r, k)
            if k <= 16:
                kd, ki = ctx.knn_search(tq, tt, k, want_dist=True, squared=True)
                full = cnt >= k
                assert r < 0.1 or int(full.sum()) > (300 if r == 0.4 else 0)
                assert torch.equal(idx[full], ki[full]) and torch.equal(d2[full].view(torch.int32), kd[full].view(torch.int32)), (r, k)


# ---- ties and edges ----------------------------------------------------------------------------------------------------------------------
def test_knn_within_ties_the_gate_and_non_finite_rows(ctx):
    dup = np.tile(np.array([[0.25, 0.5, 0.75]], f32), (40, 1))
    idx, d2, cnt = device_knn(ctx, dup, dup, 0.1, 32)
    assert (cnt == 40).all() and (d2 == 0).all() and (idx == np.arange(32)[None, :]).all()      # the order is by index
    idx, d2, cnt = device_knn(ctx, dup, dup, 0.1, 32, skip=True)
    assert (cnt == 39).all() and (d2 == 0).all()
    for i in range(40):
        assert np.array_equal(idx[i], np.delete(np.arange(40), i)[:32]), i
    idx, d2, cnt = device_knn(ctx, dup, dup[:10], 0.1, 17)
    assert (cnt == 10).all() and (idx[:, :10] == np.arange(10)).all() and (idx[:, 10:] == -1).all() and (d2[:, 10:] == np.inf).all()
    check_knn(ctx, dup, dup, 0.1, KS, skip=True, what="40 copies")
    # 0.25 is exact in f32 and its square is the gate: a neighbour at exactly that distance is out, one ulp more radius takes it in
    line = np.array([[0, 0, 0], [0.25, 0, 0], [0.5, 0, 0], [0.5, 0.25, 0]], f32)
    assert np.array_equal(device_knn(ctx, line, line, 0.25, 4)[2], [1, 1, 1, 1])
    assert np.array_equal(device_knn(ctx, line, line, float(np.nextafter(f32(0.25), f32(1))), 4)[2], [2, 3, 3, 2])
    check_knn(ctx, line, line, 0.25, (1, 4), what="on the gate")
    # NaN and inf in queries and in targets
    rs = np.random.RandomState(9)
    tgt, q = rs.rand(600, 3).astype(f32), rs.rand(300, 3).astype(f32)
    tgt[5], tgt[77], tgt[300] = [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [-np.inf, np.nan, 0.0]
    q[0], q[1], q[2] = [np.nan] * 3, [0.5, 0.5, np.inf], [0.5, -np.inf, 0.5]
    rc = check_knn(ctx, q, tgt, 0.2, (1, 8, 20), what="NaN and inf")
    assert (rc[:3] == 0).all() and (rc[3:] > 0).all()
    bad = tgt.copy()
    bad[3] = tgt[5]
    rc = check_knn(ctx, bad, bad, 0.2, (4, 32), skip=True, what="NaN and inf, the cloud on itself")
    assert rc[3] == 0 and rc[5] == 0 and rc[77] == 0 and rc[300] == 0


# ---- buckets and cells -------------------------------------------------------------------------------------------------------------------
def slots27(q, r, nt):
    """rfgrid.h's rf_cell / rf_slot in numpy: the 27 slots around every row of q for a grid over nt targets of radius r -> (Nq,27) uint64"""
    cell = max(float(r) * (1.0 + 2.0 ** -10), 2.0 ** -60)
    inv = 1.0 / cell
    clamp = (1 << 20) - 1
    bits = 8
    while bits < 23 and (1 << bits) < 2 * nt:
        bits += 1
    c = np.clip(np.floor(np.asarray(q, f64) * inv), -clamp, clamp).astype(np.int64)
    out = []
    for k in range(27):
        o = np.array([k % 3 - 1, (k // 3) % 3 - 1, k // 9 - 1])
        n = (np.clip(c + o, -clamp, clamp) + (1 << 20)).astype(np.uint64)
        key = (n[:, 0] << np.uint64(42)) | (n[:, 1] << np.uint64(21)) | n[:, 2]
        with np.errstate(over="ignore"):
            out.append(((key * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(33)) & np.uint64((1 << bits) - 1))
    return np.stack(out, axis=1)


def met_twice(q, tgt, r):
    """the queries for which a walk over all 27 slots, duplicates included, would meet a candidate twice"""
    s = slots27(q, r, len(tgt))
    own = slots27(tgt, r, len(tgt))[:, 13]                              # offset (0, 0, 0): the target's own bucket
    cnt = CR.knn_within_ref(q, tgt, r, 1)[2]
    twice = np.zeros(len(q), bool)
    for j in range(len(tgt)):
        d = CR.KR.dist2_ref(np.asarray(q, f32), np.asarray(tgt[j], f32))
        twice |= ((s == own[j]).sum(axis=1) >= 2) & (d < CR.RR.gate2_of(r))
    return twice & (cnt > 0)


@pytest.mark.parametrize("Nt", [1, 2, 3])
def test_knn_within_counts_once_where_cells_share_a_bucket(ctx, Nt):
    """a table of 256 slots for 27 cells: for most queries two of them share a bucket.  The test's own rf_slot says for which queries
    the shared bucket is a candidate's, and the count there is still the restatement's"""
    rs = np.random.RandomState(40 + Nt)
    tgt = (rs.rand(Nt, 3) * 0.05 + 0.5).astype(f32)
    q = (rs.rand(1023, 3) * 0.3 + 0.375).astype(f32)
    twice = met_twice(q, tgt, 0.1)
    print(f"Nt = {Nt}: {int(twice.sum())} of 1023 queries have a candidate in a bucket that two of their 27 cells share")
    assert twice.sum() >= 10
    rc = check_knn(ctx, q, tgt, 0.1, (1, 3, 9), what=f"Nt = {Nt}")
    assert rc.max() == Nt and (rc[twice] > 0).all()
    assert np.array_equal(device_knn(ctx, q, tgt, 0.1, 1, want=(False, False, True))[2], rc)


R_FAR = 1.5e-3                                                          # 4000 / R_FAR is beyond 2^20 cells


def test_knn_within_counts_once_in_the_clamped_cells(ctx):
    """coordinates beyond 2^20 cells on either side: the outer neighbour of a clamped cell is that cell again, so 19 of the 27 cells
    around a point clamped on all axes repeat another one, and a walk that does not skip them counts its neighbours up to 8 times"""
    rs = np.random.RandomState(50)
    far = (rs.rand(600, 3) * 0.004).astype(f32)
    far[:200] += f32(4000.0)
    far[200:400] -= f32(4000.0)
    far[400:450, 0] += f32(4000.0)                                       # clamped on one axis only
    s = slots27(far, R_FAR, 600)
    distinct = np.array([len(set(row)) for row in s.tolist()])
    assert distinct[:400].max() <= 8 and distinct[400:450].max() <= 18 and distinct[450:].min() > 18      # a clamped axis has two cells, not three
    rc = check_knn(ctx, far, far, R_FAR, (1, 8, 17, 32), what="beyond the clamp")
    assert rc[:400].min() >= 2 and rc[:400].max() > 32
    rs_ = check_knn(ctx, far, far, R_FAR, (16,), skip=True, what="beyond the clamp, the row skipped")
    assert np.array_equal(rs_, rc - 1)
    assert np.array_equal(device_knn(ctx, far, far, R_FAR, 1, want=(False, False, True))[2], rc)


# ---- NULL outputs ------------------------------------------------------------------------------------------------------------------------
def test_knn_within_every_subset_of_outputs_and_the_normals_count(ctx):
    pts = mixed_cloud(1023, 7)
    q = mixed_cloud(257, 8)
    for k, skip, qq in ((9, False, q), (32, True, pts)):
        full = device_knn(ctx, qq, pts, 0.1, k, skip)
        for want in itertools.product((False, True), repeat=3):
            if not any(want):
                continue
            got = device_knn(ctx, qq, pts, 0.1, k, skip, want=want)
            for g, f, w in zip(got, full, want):
                assert (g is None) == (not w) and (g is None or g.tobytes() == f.tobytes()), (k, want)
    cnt = device_knn(ctx, pts, pts, 0.1, 1, want=(False, False, True))[2]
    ncount = ctx.estimate_normals(cu(pts), 0.1, 3)[1].cpu().numpy()
    assert np.array_equal(cnt, ncount) and cnt.min() >= 1 and cnt.max() > 32


# ---- yoho_statistical_outliers ----------------------------------------------------------------------------------------------------------
def ulps(a, b):
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(invalid="ignore"):
        return np.where(same, 0.0, np.abs(a - b) / np.spacing(np.abs(b)))


def device_stat(c, pts, r, k, min_found=1, ratio=2.0, **want):
    out = c.statistical_outliers(cu(pts), r, k=k, min_found=min_found, std_ratio=ratio, **want)
    assert out["keep"].dtype == torch.uint8 and out["stats"].dtype == torch.float64 and out["n_keep"].dtype == torch.int32
    return {k_: (None if v is None else v.cpu().numpy()) for k_, v in out.items()}


def check_stat(c, pts, r, k, min_found=1, ratio=2.0, what="", ref=None, away=True):
    """-> (reference, the largest difference in ulps over mean_dist and stats)"""
    ref = CR.statistical_ref(pts, r, k, min_found, ratio) if ref is None else ref
    if away:
        CR.assert_away_from_threshold(ref, 1e-9)
    got = device_stat(c, pts, r, k, min_found, ratio)
    um = ulps(got["mean_dist"], ref["mean_dist"])
    us = ulps(got["stats"], ref["stats"])
    print(f"{what}: N = {len(pts)}, k = {k}, n_valid {int(ref['stats'][0])}, n_keep {ref['n_keep']}; largest difference mean_dist {um.max():.1f} ulp, "
          f"n_valid / mu / sigma / thr {us.tolist()} ulp")
    assert np.array_equal(got["count"], ref["count"]), (what, "count")
    assert np.array_equal(np.isnan(got["mean_dist"]), ~ref["valid"]), (what, "the valid set")
    assert um.max() <= ULPS and us.max() <= ULPS and got["stats"][0] == ref["stats"][0], (what, um.max(), us)
    assert np.array_equal(got["keep"], ref["keep"].astype(np.uint8)), (what, "keep")
    assert int(got["n_keep"][0]) == ref["n_keep"] == int(got["keep"].sum()), (what, "n_keep")
    return ref, max(um.max(), us.max())


def motivating():
    def make():
        pts, stray = CR.stray_cloud(0)
        return pts, stray, CR.statistical_ref(pts, 0.05, 16, 1, 2.0)
    return cached("motivating", make)


@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 1023, 20200])
def test_statistical_outliers_sizes(ctx, N):
    if N == 20200:
        pts, stray, ref = motivating()
        check_stat(ctx, pts, 0.05, 16, what="the motivating cloud", ref=ref)
        assert (ref["keep"] & stray).sum() <= 20 and ref["n_keep"] > 19000
        return
    pts = mixed_cloud(N, 300 + N)
    for k, min_found, ratio in ((16, 1, 2.0), (8, 2, 1.0), (9, 1, 0.5), (32, 5, 3.0), (1, 1, 2.0)):
        ref, _ = check_stat(ctx, pts, 0.1, k, min_found, ratio, what=f"mixed cloud, min_found {min_found}, ratio {ratio}")
        if N >= 255:
            assert 0 < ref["n_keep"] <= ref["stats"][0] < N and (ratio > 1.0 or ref["n_keep"] < ref["stats"][0])
    got = device_stat(ctx, pts, 0.1, 16, want_mean_dist=False, want_count=False)
    ref = CR.statistical_ref(pts, 0.1, 16)
    assert got["mean_dist"] is None and got["count"] is None and np.array_equal(got["keep"], ref["keep"].astype(np.uint8))


def test_statistical_outliers_edge_values(ctx):
    far = np.array([[0, 0, 0], [5, 0, 0], [0, 5, 0], [np.nan, 0, 0]], f32)
    ref, _ = check_stat(ctx, far, 1.0, 4, what="n_valid = 0")
    assert ref["stats"].tolist() == [0, 0, 0, 0] and ref["n_keep"] == 0
    chain = np.array([[0, 0, 0], [0.75, 0, 0], [1.5, 0, 0], [9, 9, 9]], f32)            # the middle point alone has two neighbours
    # with one valid point, or sigma = 0, m_i == mu == thr exactly on both sides whatever the sqrt gives: no distance from thr to ask for
    ref, _ = check_stat(ctx, chain, 1.0, 4, min_found=2, what="n_valid = 1", away=False)
    assert ref["stats"].tolist() == [1, 0.75, 0, 0.75] and ref["keep"].tolist() == [False, True, False, False]
    ref, _ = check_stat(ctx, chain, 1.0, 4, min_found=2, ratio=-1.0, what="n_valid = 1, a negative ratio", away=False)
    assert ref["keep"].tolist() == [False, True, False, False]
    pair = np.array([[0, 0, 0], [0.5, 0, 0], [9, 9, 9]], f32)
    ref, _ = check_stat(ctx, pair, 1.0, 4, what="n_valid = 2", away=False)
    assert ref["stats"].tolist() == [2, 0.5, 0, 0.5] and ref["keep"].tolist() == [True, True, False]
    pts = mixed_cloud(700, 11)
    ref, _ = check_stat(ctx, pts, 0.1, 8, ratio=0.0, what="ratio 0")
    assert ref["stats"][3] == ref["stats"][1] and 0 < ref["n_keep"] < ref["stats"][0]
    ref, _ = check_stat(ctx, pts, 0.1, 8, ratio=-0.5, what="ratio -0.5")
    assert ref["stats"][3] < ref["stats"][1] and 0 < ref["n_keep"]
    ref, _ = check_stat(ctx, pts, 0.1, 8, ratio=-100.0, what="ratio -100")
    assert ref["n_keep"] == 0 and ref["stats"][0] > 300
    ref, _ = check_stat(ctx, pts, 0.1, 8, min_found=9, what="min_found > k")
    assert ref["stats"].tolist() == [0, 0, 0, 0] and ref["n_keep"] == 0 and np.isnan(ref["mean_dist"]).all() and ref["count"].max() > 9
    ref, _ = check_stat(ctx, pts, 0.1, 8, ratio=np.inf, what="ratio +inf", away=False)
    assert ref["n_keep"] == ref["stats"][0]


# ---- determinism -------------------------------------------------------------------------------------------------------------------------
def test_bits_repeat_over_poisoned_scratch_streams_and_contexts(hip, ctx):
    pts, small = mixed_cloud(3001, 21), mixed_cloud(257, 22)

    def run(c):
        out = []
        for p in (pts, small):
            out += [x.tobytes() for x in device_knn(c, p[:200], p, 0.1, 17)]
            out += [x.tobytes() for x in device_knn(c, p, p, 0.1, 1, True, want=(False, False, True)) if x is not None]
            s = device_stat(c, p, 0.1, 16)
            out += [s[k].tobytes() for k in ("keep", "mean_dist", "count", "stats", "n_keep")]
        return out

    first = run(ctx)
    for rep in range(2):
        assert run(ctx) == first, rep
    cx = hip.Context()
    for pat in PATTERNS:
        cx.poison_scratch(pat)
        assert run(cx) == first, hex(pat)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side
        assert run(ctx) == first
    torch.cuda.synchronize()


# ---- the C ABI's refusals ----------------------------------------------------------------------------------------------------------------
def test_entries_refuse_bad_arguments(ctx, hip):
    lib = hip.load_library()
    h = ctx._h
    rs = np.random.RandomState(3)
    host = rs.rand(31, 3).astype(f32)
    q, t = cu(host), cu(host.copy())
    idx = torch.full((31, 4), -7, dtype=torch.int64, device="cuda")
    d2 = torch.full((31, 4), -3.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((32,), -7, dtype=torch.int32, device="cuda")
    md = torch.full((32,), -3.0, dtype=torch.float64, device="cuda")
    keep = torch.full((32,), 9, dtype=torch.uint8, device="cuda")
    stats = torch.full((5,), -3.0, dtype=torch.float64, device="cuda")
    nk = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())                              # noqa: E731
    off = lambda x, nbytes: C.c_void_p(x.data_ptr() + nbytes)           # noqa: E731
    N, fl, db = None, C.c_float, C.c_double
    big = hip.REFINE_MAX_POINTS + 1

    def kw(ctx_=h, q_=p(q), Nq=31, t_=p(t), Nt=31, r=fl(0.2), k=4, skip=0, idx_=p(idx), d2_=p(d2), cnt_=p(cnt)):
        return (ctx_, q_, Nq, t_, Nt, r, k, skip, idx_, d2_, cnt_, N)

    def so(ctx_=h, pts=p(q), n=31, r=fl(0.2), k=4, mf=1, ratio=db(2.0), md_=p(md), cnt_=p(cnt), keep_=p(keep), stats_=p(stats), nk_=p(nk)):
        return (ctx_, pts, n, r, k, mf, ratio, md_, cnt_, keep_, stats_, nk_, N)

    rows = [
        ("yoho_knn_within", kw(ctx_=N), "bad argument"), ("yoho_knn_within", kw(Nq=-1), "Nq=-1"), ("yoho_knn_within", kw(Nt=0), "Nt=0"),
        ("yoho_knn_within", kw(Nq=big), "YOHO_REFINE_MAX_POINTS"), ("yoho_knn_within", kw(Nt=big), "YOHO_REFINE_MAX_POINTS"),
        ("yoho_knn_within", kw(r=fl(0.0)), "max_dist"), ("yoho_knn_within", kw(r=fl(-1.0)), "max_dist"), ("yoho_knn_within", kw(r=fl(np.inf)), "max_dist"),
        ("yoho_knn_within", kw(r=fl(np.nan)), "max_dist"),
        ("yoho_knn_within", kw(k=0), "YOHO_KNN3_MAX"), ("yoho_knn_within", kw(k=33), "k=33"), ("yoho_knn_within", kw(k=-2), "k=-2"),
        ("yoho_knn_within", kw(skip=1, Nq=30), "skip_same_row"), ("yoho_knn_within", kw(skip=1, Nt=30), "skip_same_row"),
        ("yoho_knn_within", kw(q_=N), "NULL"), ("yoho_knn_within", kw(t_=N), "NULL"), ("yoho_knn_within", kw(idx_=N, d2_=N, cnt_=N), "all NULL"),
        ("yoho_knn_within", kw(q_=off(q, 2)), "4-byte aligned"), ("yoho_knn_within", kw(t_=off(t, 1)), "4-byte aligned"),
        ("yoho_knn_within", kw(d2_=off(d2, 2)), "4-byte aligned"), ("yoho_knn_within", kw(cnt_=off(cnt, 2)), "4-byte aligned"),
        ("yoho_knn_within", kw(idx_=off(idx, 4)), "8-byte aligned"),
        ("yoho_statistical_outliers", so(ctx_=N), "bad argument"), ("yoho_statistical_outliers", so(n=0), "N=0"), ("yoho_statistical_outliers", so(n=-3), "N=-3"),
        ("yoho_statistical_outliers", so(n=big), "YOHO_REFINE_MAX_POINTS"),
        ("yoho_statistical_outliers", so(r=fl(0.0)), "max_dist"), ("yoho_statistical_outliers", so(r=fl(np.inf)), "max_dist"),
        ("yoho_statistical_outliers", so(r=fl(np.nan)), "max_dist"), ("yoho_statistical_outliers", so(r=fl(-0.5)), "max_dist"),
        ("yoho_statistical_outliers", so(k=0), "YOHO_KNN3_MAX"), ("yoho_statistical_outliers", so(k=33), "k=33"),
        ("yoho_statistical_outliers", so(mf=0), "min_found=0"), ("yoho_statistical_outliers", so(mf=-1), "min_found=-1"),
        ("yoho_statistical_outliers", so(ratio=db(np.nan)), "std_ratio"),
        ("yoho_statistical_outliers", so(pts=N), "NULL"), ("yoho_statistical_outliers", so(keep_=N), "NULL"), ("yoho_statistical_outliers", so(stats_=N), "NULL"),
        ("yoho_statistical_outliers", so(nk_=N), "NULL"),
        ("yoho_statistical_outliers", so(pts=off(q, 2)), "4-byte aligned"), ("yoho_statistical_outliers", so(cnt_=off(cnt, 1)), "4-byte aligned"),
        ("yoho_statistical_outliers", so(nk_=off(nk, 2)), "4-byte aligned"), ("yoho_statistical_outliers", so(md_=off(md, 4)), "8-byte aligned"),
        ("yoho_statistical_outliers", so(stats_=off(stats, 4)), "8-byte aligned"),
    ]
    assert hip.CLEAN_SYMBOLS == ["yoho_knn_within", "yoho_statistical_outliers"]
    for fn, args, text in rows:
        rc = getattr(lib, fn)(*args)
        msg = lib.yoho_last_error().decode()
        assert rc == EINVAL, (fn, text, rc, msg)
        assert fn in msg and text in msg, (fn, text, msg)
    torch.cuda.synchronize()
    # nothing was launched: every output keeps its pattern
    assert bool((idx == -7).all()) and bool((d2 == -3.0).all()) and bool((cnt == -7).all()) and bool((md == -3.0).all()) and bool((keep == 9).all())
    assert bool((stats == -3.0).all()) and bool((nk == -7).all())
    # Nq = 0 is valid, launches nothing and looks at no pointer
    assert lib.yoho_knn_within(*kw(Nq=0, q_=N, idx_=N, d2_=N, cnt_=N)) == 0, lib.yoho_last_error().decode()
    # the context works as before: rows of 12 bytes that are not 16-byte aligned, outputs inside their rows only
    assert lib.yoho_knn_within(*kw(q_=off(q, 12), Nq=30, t_=off(t, 12), Nt=30, skip=1, idx_=off(idx, 32), d2_=off(d2, 16), cnt_=off(cnt, 4))) == 0, \
        lib.yoho_last_error().decode()
    assert lib.yoho_statistical_outliers(*so(pts=off(q, 12), n=30, md_=off(md, 8), cnt_=N, keep_=off(keep, 1), stats_=off(stats, 8), nk_=off(nk, 4))) == 0, \
        lib.yoho_last_error().decode()
    torch.cuda.synchronize()
    ri, rd, rc_ = CR.knn_within_ref(host[1:], host[1:], 0.2, 4, True)
    assert np.array_equal(idx[1:].cpu().numpy(), ri) and d2[1:].cpu().numpy().tobytes() == rd.tobytes() and np.array_equal(cnt[1:31].cpu().numpy(), rc_)
    assert bool((idx[0] == -7).all()) and bool((d2[0] == -3.0).all()) and int(cnt[0]) == -7 and int(cnt[31]) == -7
    ref = CR.statistical_ref(host[1:], 0.2, 4)
    assert np.array_equal(keep[1:31].cpu().numpy(), ref["keep"].astype(np.uint8)) and int(keep[0]) == 9 and int(keep[31]) == 9
    assert int(nk[1]) == ref["n_keep"] and int(nk[0]) == -7 and float(stats[0]) == -3.0 and float(stats[1]) == ref["stats"][0]
    assert ulps(md[1:31].cpu().numpy(), ref["mean_dist"]).max() <= ULPS and float(md[0]) == -3.0 and float(md[31]) == -3.0
    # the binding refuses other shapes before the library sees them
    with pytest.raises(ValueError):
        ctx.knn_within(q[:, :2], t, 0.2, 4)
    with pytest.raises(ValueError):
        ctx.statistical_outliers(q.reshape(-1), 0.2)
    with pytest.raises(hip.YohoError, match="yoho_knn_within"):
        ctx.knn_within(q, t, 0.2, 33)


CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import clean_ref as CR
from yoho_amd import hip
cx = hip.Context()
rs = np.random.RandomState(0)
big = torch.from_numpy(rs.rand(200000, 3).astype(np.float32)).cuda()
for call in (lambda: cx.knn_within(big[:10], big, 0.01, 4), lambda: cx.statistical_outliers(big, 0.01)):
    try:
        call()
        print("NOT REFUSED")
    except hip.YohoError as e:
        print("CODE", e.code, "workspace" in str(e))
small = rs.rand(300, 3).astype(np.float32)
t = torch.from_numpy(small).cuda()
d2, idx, cnt = cx.knn_within(t, t, 0.2, 9, skip_same_row=True)
ri, rd, rc = CR.knn_within_ref(small, small, 0.2, 9, True)
print("AFTER", np.array_equal(idx.cpu().numpy(), ri), d2.cpu().numpy().tobytes() == rd.tobytes(), np.array_equal(cnt.cpu().numpy(), rc))
out = cx.statistical_outliers(t, 0.2, k=9)
ref = CR.statistical_ref(small, 0.2, 9)
print("AFTER", np.array_equal(out["keep"].cpu().numpy(), ref["keep"].astype(np.uint8)), int(out["n_keep"][0]) == ref["n_keep"], ref["n_keep"])
"""


def test_workspace_refusal_in_a_fresh_process(tmp_path):
    """YOHO_WS_LIMIT_MB=1 in a child process of its own (the limit is read when a context is created): the grid over 200 000 points asks for
    about 9 MB, both entries return YOHO_ENOMEM, and the same context then answers 300 points correctly"""
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, YOHO_WS_LIMIT_MB="1")
    r = subprocess.run([sys.executable, str(script), REPO], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[0] == lines[1] == f"CODE {ENOMEM} True", r.stdout
    assert lines[2] == "AFTER True True True" and lines[3].startswith("AFTER True True ") and int(lines[3].split()[-1]) > 100, r.stdout


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def test_select_and_statistical_on_the_motivating_cloud(ctx):
    """keypoints.select(..., clean=...) and clean.statistical on clean_ref.stray_cloud(0), on the device from the f64 cloud to the cloud
    indices: the restatement's picks, none of which is a stray any more"""
    from yoho_amd import clean, keypoints
    pts, stray, ref = motivating()
    r = clean.statistical(ctx, cu(pts), k=16, std_ratio=2.0, max_dist=0.05)
    assert r["keep"].dtype == torch.bool and np.array_equal(r["keep"].cpu().numpy(), ref["keep"])
    assert np.array_equal(r["sel"].cpu().numpy(), np.nonzero(ref["keep"])[0]) and ulps(r["stats"].cpu().numpy(), ref["stats"]).max() <= ULPS
    pc_d = cu(pts.astype(f64))
    kept = np.nonzero(ref["keep"])[0]
    want = kept[CR.KR.fps_ref(pts[kept], 500, 0)[0]]                    # clean_ref.select_clean_ref on the shared reference (test_clean_cpu.py holds the two equal)
    got, dist2 = keypoints.select(ctx, pc_d, 500, clean={"max_dist": 0.05})
    assert np.array_equal(got.cpu().numpy(), want) and dist2.shape == (500,)
    plain = keypoints.select(ctx, pc_d, 500)[0].cpu().numpy()
    print(f"strays among 500 picks: {int(stray[plain].sum())} without the filter, {int(stray[want].sum())} with it")
    assert stray[plain].sum() >= 100 and stray[want].sum() <= 5
    sel, kept = clean.clean_cloud(ctx, pc_d, max_dist=0.05)
    assert np.array_equal(sel.cpu().numpy(), np.nonzero(ref["keep"])[0]) and torch.equal(kept, pc_d[sel])
    rr = clean.radius(ctx, cu(pts), 0.05, 8)
    assert np.array_equal(rr["keep"].cpu().numpy(), ref["count"] >= 8) and rr["mean_dist"] is None
