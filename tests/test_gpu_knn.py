"""yoho_knn_search on the GPU (-m gpu): indices and distance BITS against tests/knn_ref.py (the stable argsort of the oracle's fp32
distances - the contract), column 0 against yoho_nn_search, constructed ties, poisoned scratch and guard rows, the C ABI's refusals
driven through ctypes as tests/test_gpu_abi.py does for include/yoho_hip.h, and the utils/knn_search.py mirror against the
reference's own answers (tests/golden/knn.npz)."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_ref as KR  # noqa: E402
from yoho_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
EINVAL, ENOMEM = -1, -4
TIE_CAP = 0.01
KS = (1, 2, 3, 8, 16)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.Context()


def search(c, src, tgt, k, sq, want_dist=True):
    d, i = c.knn_search(src, tgt, k, want_dist=want_dist, squared=sq)
    assert i.dtype == torch.int64 and tuple(i.shape) == (src.shape[0], k) and i.is_cuda
    assert d is None or (d.dtype == torch.float32 and tuple(d.shape) == (src.shape[0], k))
    return (None if d is None else d.cpu().numpy()), i.cpu().numpy()


def assert_rows_valid(i, Nt, what):
    assert i.min() >= 0 and i.max() < Nt, what
    s = np.sort(i, axis=1)
    assert (np.diff(s, axis=1) > 0).all(), (what, "a row repeats an index")


def check_against_ref(c, src, tgt, ks, sq, what, nn_column=True):
    """every k of `ks` against knn_ref (one oracle evaluation: the stable order's first k columns ARE knn_ref(k)), twice, and column 0 /
    k = 1 against nn_search; returns the reference with one column more than the largest k (what tie_rows wants)"""
    Nt = tgt.shape[0]
    ridx, rdist = KR.knn_ref_more(src, tgt, max(ks), sq)
    sd, td = cu(src), cu(tgt)
    if nn_column:
        nd, ni = c.nn_search(sd, td, want_dist=True, squared=sq)
        nd, ni = nd.cpu().numpy(), ni.cpu().numpy()
    for k in ks:
        d, i = search(c, sd, td, k, sq)
        w = (what, "k", k, "squared", sq)
        assert_rows_valid(i, Nt, w)
        assert np.array_equal(i, ridx[:, :k]), w
        assert np.array_equal(bits(d), bits(rdist[:, :k])), w
        d2, i2 = search(c, sd, td, k, sq)
        assert np.array_equal(i2, i) and np.array_equal(bits(d2), bits(d)), (w, "second call")
        _, i3 = search(c, sd, td, k, sq, want_dist=False)
        assert np.array_equal(i3, i), (w, "without distances")
        if nn_column:
            assert np.array_equal(i[:, 0], ni) and np.array_equal(bits(d[:, 0]), bits(nd)), (w, "column 0 is not nn_search")
    return ridx, rdist


def inputs(D, ns, nt, seed):
    rs = np.random.RandomState(seed)
    if D == 32:
        a = rs.randn(ns, 32).astype(np.float32)
        b = rs.randn(nt, 32).astype(np.float32)
        return a / np.linalg.norm(a, axis=1, keepdims=True).astype(np.float32), b / np.linalg.norm(b, axis=1, keepdims=True).astype(np.float32)
    return rs.rand(ns, 3).astype(np.float32), rs.rand(nt, 3).astype(np.float32)


@pytest.mark.parametrize("D", [32, 3])
@pytest.mark.parametrize("sq", [False, True], ids=["L2", "SquareL2"])
def test_grid_of_sizes_equals_ref(ctx, D, sq):
    """ragged row and target counts on both sides of the 2^20-pair switch between the single launch and the segmented search"""
    n = 0
    for ns in (1, 31, 33, 1000):
        for nt in (255, 257, 4001):
            a, b = inputs(D, ns, nt, 1000 * ns + nt)
            check_against_ref(ctx, a, b, KS, sq, (D, ns, nt))
            n += 1
        for k in KS:                                   # as few targets as there can be: Nt = k and k + 1
            for nt in (k, k + 1):
                a, b = inputs(D, ns, nt, 7 * ns + nt)
                check_against_ref(ctx, a, b, (k,), sq, (D, ns, nt))
                n += 1
    # segmented with a ragged last row block, with more segments than k, and with one row
    for ns, nt in ((300, 4001), (33, 40001), (1, 1 << 20)):
        a, b = inputs(D, ns, nt, ns + nt)
        check_against_ref(ctx, a, b, KS, sq, (D, ns, nt))
        n += 1
    print(f"D = {D}, squared = {sq}: {n} shapes x k in {KS} identical to knn_ref in indices and distance bits")


def test_full_size_descriptors(ctx):
    """5000 x 5000 descriptors as the matcher sees them (numpy-order group means of synth.make_pair(5000, seed=2)), k = 2 and 8"""
    pr = synth.make_pair(5000, seed=2)
    a, b = np.mean(pr["feat0"], -1), np.mean(pr["feat1"], -1)
    for sq in (False, True):
        ridx, rdist = check_against_ref(ctx, a, b, (2, 8), sq, "5000 x 5000")
        ties = KR.tie_rows(rdist, 8)
        print(f"5000 x 5000, squared = {sq}: {len(ties)} rows with a tie among their first 9 distances (never excluded from the comparison above)")
        assert len(ties) <= TIE_CAP * 5000


def test_constructed_ties(ctx):
    for D in (32, 3):
        a = np.zeros((5, D), np.float32)
        b = np.ones((700, D), np.float32)
        b[[3, 300, 699]] = 0.5
        for sq in (False, True):
            _, i = search(ctx, cu(a), cu(b), 2, sq)
            assert (i == [3, 300]).all()
            _, i = search(ctx, cu(a), cu(b), 4, sq)
            assert (i == [3, 300, 699, 0]).all()
            check_against_ref(ctx, a, b, KS, sq, ("equal targets", D))
            one = inputs(D, 1, 1, 5)[1]
            check_against_ref(ctx, inputs(D, 40, 1, 6)[0], np.repeat(one, 64, 0), KS, sq, ("64 copies", D))
            for k in KS:
                _, i = search(ctx, cu(inputs(D, 40, 1, 6)[0]), cu(np.repeat(one, 64, 0)), k, sq)
                assert (i == np.arange(k)).all()


@pytest.mark.parametrize("D", [32, 3])
def test_ties_that_only_the_rounded_l2_distance_has(ctx, D):
    """D2 = 2e-15 at the LOWER index and 1e-15 at the higher one: both give fl(D2 + 1e-7) = 1e-7f, i.e. equal L2 distance bits - under
    L2 the lower index comes first, under SquareL2 the smaller D2 (the higher index).  Once with both indices on one lane of the
    search (congruent mod 16) and once not, in the first tile of 256 targets and in the second.  Column 0 is yoho_nn_search's answer
    here too (tests/test_gpu_nn.py has its own cases)."""
    a = np.zeros((5, D), np.float32)
    for base in (0, 256):
        for lo, hi in ((base + 2, base + 18), (base + 2, base + 4)):
            b = np.ones((700, D), np.float32)
            b[lo] = 0; b[lo, 0] = np.float32(4.4721360e-8)
            b[hi] = 0; b[hi, 0] = np.float32(3.1622776e-8)
            d2 = KR.orc.pdist_l2(a[:1], b[[lo, hi]], squared=True)[0]
            dl = KR.orc.pdist_l2(a[:1], b[[lo, hi]], squared=False)[0]
            assert d2[0] > d2[1] > 0 and bits(dl)[0] == bits(dl)[1]
            for k in (1, 2, 3):
                want_l2, want_sq = [lo, hi, 0][:k], [hi, lo, 0][:k]
                assert (KR.knn_ref(a, b, k, False)[0] == want_l2).all() and (KR.knn_ref(a, b, k, True)[0] == want_sq).all()   # the contract, on the CPU
                _, i = search(ctx, cu(a), cu(b), k, False)
                assert (i == want_l2).all(), (D, lo, hi, k, i[0])
                _, i = search(ctx, cu(a), cu(b), k, True)
                assert (i == want_sq).all(), (D, lo, hi, k, i[0])
            for sq in (False, True):
                check_against_ref(ctx, a, b, (1, 2, 3), sq, ("rounded ties", D, lo, hi), nn_column=True)


def test_result_ignores_switches_scratch_and_call_count(hip):
    """the same bits with the matcher's pre-filter off, the 3-D hash grid on, a workspace poisoned with NaN patterns, and a workspace
    that an earlier, larger call left behind"""
    c = hip.Context()
    for D, ns, nt in ((32, 1000, 4001), (3, 1000, 4001), (32, 33, 257)):
        a, b = inputs(D, ns, nt, 99)
        sd, td = cu(a), cu(b)
        for sq in (False, True):
            clean = {k: search(c, sd, td, k, sq) for k in (1, 8, 16)}
            ridx, rdist = KR.knn_ref(a, b, 16, sq)
            assert all(np.array_equal(i, ridx[:, :k]) and np.array_equal(bits(d), bits(rdist[:, :k])) for k, (d, i) in clean.items())
            c.set_nn_prefilter(False)
            c.set_nn_grid(0.05)
            try:
                for k, (d, i) in clean.items():
                    d1, i1 = search(c, sd, td, k, sq)
                    assert np.array_equal(i1, i) and np.array_equal(bits(d1), bits(d)), ("switches", D, k, sq)
            finally:
                c.set_nn_prefilter(True)
                c.set_nn_grid(0)
            for pattern in (0xFFFFFFFF, 0x7FC00000):
                c.poison_scratch(pattern)
                for k, (d, i) in clean.items():
                    d1, i1 = search(c, sd, td, k, sq)
                    assert np.array_equal(i1, i) and np.array_equal(bits(d1), bits(d)), ("poisoned", hex(pattern), D, k, sq)


def test_outputs_are_written_inside_their_rows_only(ctx, hip):
    """idx / dist handed to the library as the middle of larger buffers: the guard rows in front and behind keep their pattern, and with
    dist = NULL only idx is written"""
    lib = hip.load_library()
    G = 64
    for D, ns, nt, k in ((32, 1000, 4001, 8), (32, 33, 257, 16), (3, 31, 255, 3), (3, 1000, 4001, 1)):
        a, b = inputs(D, ns, nt, 5)
        sd, td = cu(a), cu(b)
        ridx, rdist = KR.knn_ref(a, b, k, False)
        for want_dist in (True, False):
            ibuf = torch.full((ns + 2 * G, k), -7, dtype=torch.int64, device="cuda")
            dbuf = torch.full((ns + 2 * G, k), -3.0, dtype=torch.float32, device="cuda")
            rc = lib.yoho_knn_search(ctx._h, C.c_void_p(sd.data_ptr()), ns, C.c_void_p(td.data_ptr()), nt, D, 0, k,
                                     C.c_void_p(ibuf[G:].data_ptr()), C.c_void_p(dbuf[G:].data_ptr()) if want_dist else None, None)
            assert rc == 0, lib.yoho_last_error().decode()
            torch.cuda.synchronize()
            assert bool((ibuf[:G] == -7).all()) and bool((ibuf[G + ns:] == -7).all()) and bool((dbuf[:G] == -3.0).all()) and bool((dbuf[G + ns:] == -3.0).all())
            assert np.array_equal(ibuf[G:G + ns].cpu().numpy(), ridx)
            if want_dist:
                assert np.array_equal(bits(dbuf[G:G + ns]), bits(rdist))
            else:
                assert bool((dbuf == -3.0).all())


def test_non_finite_rows_get_distinct_in_range_indices(ctx):
    """NaN / inf are outside what is pinned against the reference; they must not fault, hang or repeat an index, and finite rows of the
    same call keep their exact answer"""
    for D in (32, 3):
        for ns, nt in ((64, 300), (1000, 4001)):
            a, b = inputs(D, ns, nt, 3)
            bad_a, bad_b = a.copy(), b.copy()
            bad_a[1, 0] = np.nan; bad_a[2, 1] = np.inf; bad_a[3] = np.nan
            for sq in (False, True):
                for k in (1, 8, 16):
                    d, i = search(ctx, cu(bad_a), cu(b), k, sq)
                    assert_rows_valid(i, nt, ("NaN / inf queries", D, ns, nt, k))
                    ridx, rdist = KR.knn_ref(a[4:], b, k, sq)
                    assert np.array_equal(i[4:], ridx) and np.array_equal(bits(d[4:]), bits(rdist))
            bad_b[5, 0] = np.nan; bad_b[6] = np.inf; bad_b[nt - 1, D - 1] = -np.inf
            for k in (1, 16):
                d, i = search(ctx, cu(a), cu(bad_b), k, False)
                assert_rows_valid(i, nt, ("NaN / inf targets", D, ns, nt, k))
            _, i = search(ctx, cu(np.full((5, D), np.nan, np.float32)), cu(np.full((40, D), np.nan, np.float32)), 16, False)
            assert_rows_valid(i, 40, "all NaN")


def test_entry_refuses_bad_arguments(ctx, hip):
    lib = hip.load_library()
    h = ctx._h
    src, tgt = cu(inputs(32, 8, 40, 1)[0]), cu(inputs(32, 8, 40, 1)[1])
    s3, t3 = cu(inputs(3, 8, 40, 1)[0]), cu(inputs(3, 8, 40, 1)[1])
    idx = torch.full((9, 4), -7, dtype=torch.int64, device="cuda")
    dist = torch.full((9, 4), -3.0, dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    off = lambda t, nbytes: C.c_void_p(t.data_ptr() + nbytes)
    N = None
    # (arguments after the entry's name, text the message must contain beside the entry's name)
    cases = [
        ((N, p(src), 8, p(tgt), 40, 32, 0, 4, p(idx), N, N), "bad argument"),
        ((h, N, 8, p(tgt), 40, 32, 0, 4, p(idx), N, N), "NULL"),
        ((h, p(src), 8, N, 40, 32, 0, 4, p(idx), N, N), "NULL"),
        ((h, p(src), 8, p(tgt), 40, 32, 0, 4, N, p(dist), N), "NULL"),
        ((h, p(src), -1, p(tgt), 40, 32, 0, 4, p(idx), N, N), "Ns=-1"),
        ((h, p(src), 8, p(tgt), 0, 32, 0, 4, p(idx), N, N), "Nt=0"),
        ((h, p(src), 8, p(tgt), 40, 32, 0, 0, p(idx), N, N), "k=0"),
        ((h, p(src), 8, p(tgt), 40, 32, 0, -2, p(idx), N, N), "k=-2"),
        ((h, p(src), 8, p(tgt), 40, 32, 0, 17, p(idx), N, N), "YOHO_KNN_MAX"),
        ((h, p(src), 8, p(tgt), 3, 32, 0, 4, p(idx), N, N), "Nt = 3"),
        ((h, p(src), 8, p(tgt), 40, 7, 0, 4, p(idx), N, N), "D must be 32 or 3"),
        ((h, p(src), 8, p(tgt), 40, 32, 2, 4, p(idx), N, N), "dist_type"),
        ((h, p(src), 8, p(tgt), 40, 32, -1, 4, p(idx), N, N), "dist_type"),
        ((h, off(src, 4), 7, p(tgt), 40, 32, 0, 4, p(idx), N, N), "16-byte aligned"),
        ((h, p(src), 8, off(tgt, 8), 39, 32, 0, 4, p(idx), N, N), "16-byte aligned"),
        ((h, off(s3, 2), 7, p(t3), 40, 3, 0, 4, p(idx), N, N), "4-byte aligned"),
        ((h, p(src), 8, p(tgt), 40, 32, 0, 4, off(idx, 4), N, N), "8-byte aligned"),
        ((h, p(src), 8, p(tgt), 40, 32, 0, 4, p(idx), off(dist, 2), N), "4-byte aligned"),
        ((h, p(src), 0, p(tgt), 40, 32, 0, 17, p(idx), N, N), "YOHO_KNN_MAX"),       # no rows does not excuse a bad k
    ]
    seen = set()
    for args, text in cases:
        rc = lib.yoho_knn_search(*args)
        msg = lib.yoho_last_error().decode()
        assert rc == EINVAL, (args, rc, msg)
        assert "yoho_knn_search" in msg and text in msg, (args, text, msg)
        seen.add("yoho_knn_search")
    assert set(hip.KNN_SYMBOLS) == seen                        # every entry of include/yoho_knn.h has a refusal above
    # no rows: valid with NULL data pointers, nothing launched, nothing written
    assert lib.yoho_knn_search(h, N, 0, N, 40, 32, 0, 4, N, N, N) == 0
    assert lib.yoho_knn_search(h, N, 0, N, 1, 3, 1, 1, N, N, N) == 0
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((dist == -3.0).all())
    # an unaligned 3-D call that IS valid (rows of 12 bytes), and the context works as before
    rc = lib.yoho_knn_search(h, off(s3, 12), 7, off(t3, 12), 39, 3, 1, 4, p(idx), p(dist), N)
    assert rc == 0, lib.yoho_last_error().decode()
    torch.cuda.synchronize()
    ri, rd = KR.knn_ref(s3.cpu().numpy()[1:], t3.cpu().numpy()[1:], 4, True)
    assert np.array_equal(idx[:7].cpu().numpy(), ri) and np.array_equal(bits(dist[:7]), bits(rd)) and bool((idx[7:] == -7).all())
    check_against_ref(ctx, src.cpu().numpy(), tgt.cpu().numpy(), (1, 4), False, "after the refusals")


def test_workspace_allocation_failure_is_enomem_and_leaves_no_sticky_error(hip, monkeypatch):
    """a context whose workspace may not exceed 1 MiB: the segmented search of 1000 x 4001 at k = 16 (4 MB of segment keys) returns
    YOHO_ENOMEM, and the next calls that fit - one segmented, one not - run and are right: the failed allocation left no HIP error behind"""
    monkeypatch.setenv("YOHO_WS_LIMIT_MB", "1")
    c = hip.Context()
    monkeypatch.delenv("YOHO_WS_LIMIT_MB")
    a, b = inputs(32, 1000, 4001, 8)
    with pytest.raises(hip.YohoError) as e:
        c.knn_search(cu(a), cu(b), 16)
    assert e.value.code == ENOMEM and "workspace" in str(e.value)
    check_against_ref(c, a[:300], b, (2,), False, "after YOHO_ENOMEM, segmented")
    check_against_ref(c, a[:100], b[:2000], (16,), False, "after YOHO_ENOMEM")


def test_mirror_equals_reference_fixture(hip, gold):
    """knn_module.KNN(k): find_knn_gpu and __call__ on the fixture's inputs return the reference's shapes and indices as host tensors
    (rows with a tie among the reference's distances - at most 1 %, none in this fixture - left out: torch.topk's tie order is open),
    SquareL2 distances bit for bit and L2 to 1 ulp; the contract itself (knn_ref) on every row"""
    from yoho_amd.knn_search import knn_module
    g = gold("knn.npz")
    for case in KR.FIXTURE_CASES:
        D, ns, nt, k, dt, seed = case
        name = KR.case_name(*case)
        src, tgt = KR.fixture_inputs(D, ns, nt, seed)
        ridx, rdist = g[name + "_idx"].astype(np.int64), g[name + "_dist"]
        ties = KR.tie_rows(rdist, k)
        print(f"{name}: {len(ties)} rows with a tie in the reference's distances")
        assert len(ties) <= TIE_CAP * ns
        keep = np.setdiff1d(np.arange(ns), ties)
        cidx, cdist = KR.knn_ref(src, tgt, k, dt == "SquareL2")
        m = knn_module.KNN(k)
        dists, inds = m.find_knn_gpu(torch.from_numpy(src), torch.from_numpy(tgt), dist_type=dt)
        assert not dists.is_cuda and not inds.is_cuda and inds.dtype == torch.int64 and dists.dtype == torch.float32
        assert list(dists.shape) == g[name + "_shape_dists"].tolist() and tuple(inds.shape) == (ns, k)
        assert np.array_equal(inds.numpy(), cidx) and np.array_equal(bits(dists.numpy()[:, 0, :]), bits(cdist))
        assert np.array_equal(inds.numpy()[keep], ridx[keep])
        assert KR.ulp_diff(dists.numpy()[:, 0, :], rdist) <= (0 if dt == "SquareL2" else 1)
        only = m.find_knn_gpu(torch.from_numpy(src), torch.from_numpy(tgt), return_distance=False, dist_type=dt)
        assert torch.equal(only, inds)
        tF, sF = torch.from_numpy(np.ascontiguousarray(tgt.T))[None], torch.from_numpy(np.ascontiguousarray(src.T))[None]
        with warnings.catch_warnings():
            warnings.simplefilter("error")                     # the mirror must not lean on the deprecated .T of a 3-D tensor
            d, i = m(tF, sF, dist_type=dt)
        assert not d.is_cuda and not i.is_cuda
        assert list(d.shape) == g[name + "_shape_call_d"].tolist() and list(i.shape) == g[name + "_shape_call_idx"].tolist()
        assert torch.equal(i[0], inds.T) and torch.equal(d[0, :, 0, :], dists[:, 0, :].T)
    # the limits: beyond YOHO_KNN_MAX is not implemented (and says so), beyond the targets is torch.topk's RuntimeError
    src, tgt = KR.fixture_inputs(32, 20, 30, 1)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x.T))[None]
    with pytest.raises(NotImplementedError, match="16"):
        knn_module.KNN(17)(T(tgt), T(src))
    with pytest.raises(RuntimeError):
        knn_module.KNN(8)(T(tgt[:5]), T(src))
    # k < 2 is the nearest-neighbour path as before
    d, i = knn_module.KNN(1)(T(tgt), T(src))
    assert tuple(d.shape) == (1, 1, 20) and np.array_equal(i[0, 0].numpy(), KR.knn_ref(src, tgt, 1, False)[0][:, 0])
