"""GPU tests (-m gpu): every entry point on memory that works against it.

The workspace and the pair scratch of a context are reused, and output tensors come from torch.empty, so a kernel that reads bytes it
never wrote (the unwritten blocks of a ragged column tile, the padded rows of a 16-row tile, K padding) finds either a fresh
allocation or valid leftovers of an earlier call - and passes.  Here those bytes are made hostile:

- scratch poisoning (yoho_poison_scratch): the whole workspace of a context that runs nothing but PartI / PartII passes is filled with a
  32-bit pattern before the call (their workspace holds only numbers; the other entries keep indices there, which must never be
  poisoned);
- output poisoning: torch.empty / torch.empty_like hand every floating-point tensor out filled with the pattern (integer tensors are
  left alone).

Each case runs once clean and is checked against the float64 oracle, then once per pattern; the poisoned outputs must be BIT-identical
to the clean ones (raw bytes: NaN == NaN), and in the fp16 modes no range flag may be raised by any call (a spurious flag would be
absorbed by the bf16x3 repeat of the range guard and show only as lost speed)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import fcgf_oracle as fo  # noqa: E402
import yoho_oracle as orc  # noqa: E402
from yoho_amd import synth, weights as W  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-4
PATTERNS = (0xFFFFFFFF,      # NaN in fp32, fp16 and e4m3
            0x7BFF7BFF,      # the largest finite fp16 in both halves
            0x7C007C00,      # fp16 +inf
            0x7F800000)      # fp32 +inf
SIZES_I = (1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 1000)
SIZES_II = (1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 700)
ORC_I = np.r_[0:512, 960:1000, 4960:5000]         # PartI input rows the oracle is evaluated on (every pass below reads a prefix)
ORC_II = np.r_[0:257, 660:700]                    # PartII match rows the oracle is evaluated on


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rel_rows(a, b):
    a, b = np.asarray(a, np.float64).reshape(len(a), -1), np.asarray(b, np.float64).reshape(len(b), -1)
    return float(np.max(np.max(np.abs(a - b), axis=1) / np.maximum(np.max(np.abs(b), axis=1), 1e-30)))


def raw(x):
    """the bytes of a tensor / array (NaN payloads included)"""
    if isinstance(x, torch.Tensor):
        x = x.detach().contiguous().cpu().numpy()
    return np.ascontiguousarray(x).tobytes()


def same_bits(a, b, what):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            same_bits(a[k], b[k], (what, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            same_bits(x, y, (what, i))
    elif a is None:
        assert b is None, what
    else:
        assert raw(a) == raw(b), what


class OutputPoison:
    """torch.empty / torch.empty_like with every floating-point tensor filled with `pattern` (None: plain)"""

    def __init__(self):
        self.pattern = None

    def fill(self, t):
        if self.pattern is None or not t.is_floating_point() or not t.is_cuda or t.numel() == 0:
            return t
        flat = t.view(-1)
        if t.element_size() == 2:
            p = self.pattern & 0xFFFF
            flat.view(torch.int16).fill_(p - (1 << 16) if p >= 1 << 15 else p)
        else:
            p = self.pattern
            flat.view(torch.int32).fill_(p - (1 << 32) if p >= 1 << 31 else p)
        return t


@pytest.fixture
def outp(monkeypatch):
    po = OutputPoison()
    empty, empty_like = torch.empty, torch.empty_like
    monkeypatch.setattr(torch, "empty", lambda *a, **k: po.fill(empty(*a, **k)))
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: po.fill(empty_like(*a, **k)))
    yield po
    po.pattern = None


def poisoned_runs(outp, run, clean, what, ctx=None):
    """run() once per pattern with the outputs (and, given a context, its scratch) poisoned: bit-identical to `clean`"""
    for p in PATTERNS:
        if ctx is not None:
            ctx.poison_scratch(p)
        outp.pattern = p
        try:
            got = run()
        except AssertionError as e:
            raise AssertionError(f"{what} poisoned with {p:#010x}: {e}") from e
        finally:
            outp.pattern = None
        same_bits(clean, got, (what, hex(p)))


@pytest.fixture(scope="module")
def net(hip, sd1, sd2):
    """(clean, poisoned): two contexts with both networks; the first is never given a pattern, the second runs PartI / PartII only"""
    cs = []
    for _ in range(2):
        c = hip.Context()
        c.load_partI(sd1)
        c.load_partII(sd2)
        cs.append(c)
    yield cs
    for c in cs:
        assert c.range_fallbacks == 0, c.range_report()


@pytest.fixture(scope="module")
def data_I(sd1, tables):
    X = synth.unit_features(5000, seed=601)
    e, i = orc.partI_forward(X[ORC_I], sd1, tables.N)
    pos = np.full(len(X), -1, np.int64)
    pos[ORC_I] = np.arange(len(ORC_I))
    return X, cu(X), e, i, pos


def check_partI_oracle(out, rows, data, what):
    """rows: the input row of every output row; the ones the oracle covers must agree to 1e-4 per row"""
    _, _, e, i, pos = data
    rows = np.asarray(rows)
    k = pos[rows] >= 0
    assert k.any(), what
    eqv, inv, inv_np = (out[n].cpu().numpy()[k] for n in ("eqv", "inv", "inv_np"))
    eo, io = e[pos[rows[k]]], i[pos[rows[k]]]
    assert np.isfinite(eqv).all() and np.isfinite(inv).all() and np.isfinite(inv_np).all(), what
    errs = rel_rows(eqv, eo), rel_rows(inv, io), rel_rows(inv_np, np.mean(eo, axis=-1))      # inv_np: the plain group mean of eqv
    assert max(errs) < TOL, (what, errs)


def checked(c, fn):
    """fn() on context c, then no range flag of either network may have been raised"""
    out = fn()
    flags = c.range_status()
    assert flags == (False, False), f"range flag raised (PartI, PartII) = {flags}"
    return out


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "fp16x2", "fourier", "fgemm", "fgemm256", "fgemm128", "fgemm8"])
def test_partI_poisoned(net, data_I, outp, mode):
    clean, pois = net
    for c in net:
        c.set_gconv_mode(mode)
    Xd = data_I[1]
    for B in SIZES_I:
        x = Xd[:B]
        run = lambda c: checked(c, lambda: c.partI_forward(x, want_inv=True, want_inv_np=True, check_range=False))
        ref = run(clean)
        check_partI_oracle(ref, np.arange(B), data_I, (mode, B))
        poisoned_runs(outp, lambda: run(pois), ref, (mode, B), ctx=pois)
    for c in net:
        assert c.range_fallbacks == 0 and c.range_repeats == {"gconv": 0, "partII": 0}


@pytest.mark.parametrize("mode", ["fgemm", "fgemm8"])
def test_partI_pair_poisoned(net, data_I, outp, mode):
    clean, pois = net
    for c in net:
        c.set_gconv_mode(mode)
    Xd = data_I[1]
    for B0, B1 in ((17, 33), (255, 257), (1, 4999)):
        x0, x1 = Xd[:B0], Xd[B0:B0 + B1]
        run = lambda c: checked(c, lambda: c.partI_forward_pair(x0, x1, want_inv=True, want_inv_np=True, check_range=False))
        ref = run(clean)
        check_partI_oracle(ref, np.arange(B0 + B1), data_I, (mode, B0, B1))
        poisoned_runs(outp, lambda: run(pois), ref, (mode, B0, B1), ctx=pois)
    for c in net:
        assert c.range_fallbacks == 0


def test_partI_chunked_and_split_passes_poisoned(net, sd1, tables, outp):
    """the depth-first schedule on two streams (chunks of 1024 keypoints, a ragged last chunk) and the split of a pass above 16384
    keypoints, in the default mode"""
    clean, pois = net
    for c in net:
        c.set_gconv_mode("fgemm")
    B = 16384 + 17
    X = synth.unit_features(B, seed=602)
    rows = np.r_[0:17, 2048:2065, 16384:16401]
    e, i = orc.partI_forward(X[rows], sd1, tables.N)
    pos = np.full(B, -1, np.int64)
    pos[rows] = np.arange(len(rows))
    data = (X, None, e, i, pos)
    Xd = cu(X)
    try:
        for c in net:
            c.set_partI_schedule(1024, 2)
        x = Xd[:2 * 1024 + 17]
        run = lambda c: checked(c, lambda: c.partI_forward(x, want_inv=True, want_inv_np=True, check_range=False))
        ref = run(clean)
        check_partI_oracle(ref, np.arange(x.shape[0]), data, "chunked")
        poisoned_runs(outp, lambda: run(pois), ref, "chunked", ctx=pois)
    finally:
        for c in net:
            c.set_partI_schedule(0, 1)
    run = lambda c: checked(c, lambda: c.partI_forward(Xd, want_inv=True, want_inv_np=True, check_range=False))
    ref = run(clean)
    check_partI_oracle(ref, np.arange(B), data, "split")
    poisoned_runs(outp, lambda: run(pois), ref, "split", ctx=pois)
    for c in net:
        assert c.range_fallbacks == 0


@pytest.fixture(scope="module")
def data_II(sd2, tables):
    A, Bf, Cf, Df = (synth.unit_features(700, seed=sd) for sd in (611, 612, 613, 614))
    dr = np.random.RandomState(615).randint(0, 60, size=700).astype(np.int64)
    q = orc.partII_forward(A[ORC_II], Bf[ORC_II], Cf[ORC_II], Df[ORC_II], dr[ORC_II], sd2, tables.N, tables.P)
    pos = np.full(700, -1, np.int64)
    pos[ORC_II] = np.arange(len(ORC_II))
    return (A, Bf, Cf, Df), [cu(x) for x in (A, Bf, Cf, Df, dr)], q, pos


def check_partII_oracle(q, data, what):
    _, _, qo, pos = data
    q = q.cpu().numpy()
    assert np.isfinite(q).all(), what
    k = pos[:len(q)] >= 0
    assert rel_rows(q[k], qo[pos[:len(q)][k]]) < TOL, (what, rel_rows(q[k], qo[pos[:len(q)][k]]))


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "fp16x2", "cgemm", "cgemm8"])
def test_partII_poisoned(net, data_II, outp, mode):
    clean, pois = net
    for c in net:
        c.set_partII_mode(mode)
    dev = data_II[1]
    for M in SIZES_II:
        args = [t[:M] for t in dev]
        run = lambda c: checked(c, lambda: c.partII_forward(*args, check_range=False))
        ref = run(clean)
        check_partII_oracle(ref, data_II, (mode, M))
        poisoned_runs(outp, lambda: run(pois), ref, (mode, M), ctx=pois)
    for c in net:
        assert c.range_fallbacks == 0 and c.range_repeats == {"gconv": 0, "partII": 0}


@pytest.mark.parametrize("mode", ["fp16x2", "cgemm", "cgemm8"])
def test_partII_matched_poisoned(net, data_II, outp, mode):
    """the row-indexed entry: the inputs stored in a shuffled row order and read back through the match list, so that the rows it
    gathers are the oracle's"""
    clean, pois = net
    for c in net:
        c.set_partII_mode(mode)
    (A, Bf, Cf, Df), dev, _, _ = data_II
    rs = np.random.RandomState(616)
    p0, p1 = rs.permutation(700), rs.permutation(700)
    feat0, feat1, eqv0, eqv1 = cu(Bf[p0]), cu(A[p1]), cu(Df[p0]), cu(Cf[p1])
    i0, i1 = np.argsort(p0), np.argsort(p1)
    for M in (17, 257):
        match = cu(np.stack([i0[:M], i1[:M]], 1).astype(np.int64))
        dr = dev[4][:M]
        run = lambda c: checked(c, lambda: c.partII_forward_matched(feat0, feat1, eqv0, eqv1, match, dr, check_range=False))
        ref = run(clean)
        check_partII_oracle(ref, data_II, (mode, M))
        poisoned_runs(outp, lambda: run(pois), ref, (mode, M), ctx=pois)
    for c in net:
        assert c.range_fallbacks == 0


# ---- the other entry points: outputs poisoned only (their workspace holds indices) ------------------------------------------------

@pytest.fixture(scope="module")
def octx(hip, sd2):
    c = hip.Context()
    c.load_partII(sd2)
    yield c
    assert c.range_fallbacks == 0


def near_tie_ok(idx, cor_ref):
    """coarse rotation index against the oracle: equal, or the oracle's top two within fp32 summation error of each other"""
    ref = np.argmax(cor_ref, axis=1)
    top2 = np.sort(cor_ref, axis=1)[:, -2:]
    differ = idx != ref
    return bool(((top2[:, 1] - top2[:, 0])[differ] < 1e-4).all())


@pytest.mark.parametrize("Na,Nb", [(1, 1), (17, 33), (255, 257), (1500, 3001)])
def test_matching_outputs_poisoned(octx, tables, outp, Na, Nb):
    c = octx
    rs = np.random.RandomState(Na + 7 * Nb)
    e0 = synth.unit_features(Na, seed=620 + Na)
    e1 = synth.unit_features(Nb, seed=621 + Nb)
    a32, b32 = np.mean(e0, -1), np.mean(e1, -1)
    a3, b3 = (rs.rand(Na, 3) * 1.5).astype(np.float32), (rs.rand(Nb, 3) * 1.5).astype(np.float32)
    ad, bd, a3d, b3d, e0d, e1d = (cu(x) for x in (a32, b32, a3, b3, e0, e1))
    # nearest neighbours: 32-D descriptors and 3-D points, brute force and through the hash grid
    fwd, back = orc.find_nn(a32, b32), orc.find_nn(b32, a32)
    ref32 = orc.pdist_l2(a32, b32).min(1)
    refs3 = {sq: orc.pdist_l2(a3, b3, squared=sq) for sq in (False, True)}
    for cell in (0.0, 0.05):
        c.set_nn_grid(cell)
        try:
            for src, tgt, sq, oi, od in ((ad, bd, False, fwd, ref32),
                                         (a3d, b3d, False, np.argmin(refs3[False], 1), refs3[False].min(1)),
                                         (a3d, b3d, True, np.argmin(refs3[True], 1), refs3[True].min(1))):
                run = lambda: c.nn_search(src, tgt, squared=sq)
                d, i = run()
                what = ("nn_search", Na, Nb, src.shape[1], sq, cell)
                assert np.array_equal(i.cpu().numpy(), oi), what
                assert np.allclose(d.cpu().numpy(), od, rtol=2.5e-7, atol=0), what
                poisoned_runs(outp, run, (d, i), what)
        finally:
            c.set_nn_grid(0)
    # mutual matches, with and without the pre-filter
    mref = orc.mutual_match(a32, b32)
    assert np.array_equal(mref[:, 1], fwd[mref[:, 0]]) and (back[fwd[mref[:, 0]]] == mref[:, 0]).all()
    for pre in (True, False):
        c.set_nn_prefilter(pre)
        try:
            run = lambda: c.mutual_nn(ad, bd)
            m = run()
            assert np.array_equal(m.cpu().numpy(), mref), ("mutual_nn", Na, Nb, pre)
            poisoned_runs(outp, run, m, ("mutual_nn", Na, Nb, pre))
        finally:
            c.set_nn_prefilter(True)
    # group mean, coarse rotation index (with its correlation), and the row-indexed variant on the match list
    run = lambda: c.group_mean_np(e0d)
    g = run()
    assert rel_rows(g.cpu().numpy(), orc.group_mean_np(e0)) < TOL
    poisoned_runs(outp, run, g, ("group_mean_np", Na))
    k = min(Na, Nb)
    d1, d2 = e1d[:k], e0d[:k]
    cor_ref = orc.des2r_cor(e1[:k], e0[:k], tables.P)
    run = lambda: c.des2r(d1, d2, want_cor=True)
    idx, cor = run()
    assert near_tie_ok(idx.cpu().numpy(), cor_ref) and rel_rows(cor.cpu().numpy(), cor_ref) < TOL, ("des2r", k)
    poisoned_runs(outp, run, (idx, cor), ("des2r", k))
    if len(mref):
        match = cu(mref)
        run = lambda: c.des2r_matched(e1d, e0d, match)
        idx = run()
        assert near_tie_ok(idx.cpu().numpy(), orc.des2r_cor(e1[mref[:, 1]], e0[mref[:, 0]], tables.P)), ("des2r_matched", Na, Nb)
        poisoned_runs(outp, run, idx, ("des2r_matched", Na, Nb))


def test_estimators_outputs_poisoned(octx, tables, outp):
    c = octx
    M, H, I = 333, 77, 51
    ec = synth.estimator_case(M, M, seed=631)
    k0, k1, dr = ec["k0"], ec["k1"], ec["dr"]
    rs = np.random.RandomState(632)
    q = rs.randn(M, 4).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    k0d, k1d, qd, drd = cu(k0), cu(k1), cu(q), cu(dr)
    # hypotheses from quaternions
    run = lambda: c.hyp_from_quat(qd, drd, k0d, k1d)
    T = run()
    assert np.allclose(T.cpu().numpy(), orc.hyp_from_quat(q, dr, k0, k1, tables.R32), rtol=0, atol=1e-12)
    poisoned_runs(outp, run, T, "hyp_from_quat")
    # YOHO-O vote over H of the M hypotheses
    order = rs.permutation(M).astype(np.int64)
    Td, od = cu(ec["T"]), cu(order)
    run = lambda: c.o_score(k0d, k1d, Td, od, H, 0.09)
    res, counts = run()
    bid, cnt, _ = orc.yohoo_select(k0, k1, ec["T"], order, 0.09, H)
    assert tuple(res.cpu().numpy()) == (bid, cnt)
    assert np.array_equal(counts.cpu().numpy(), [orc.inlier_count(k0, k1, ec["T"][order[h]], 0.09) for h in range(H)])
    poisoned_runs(outp, run, (res, counts), "o_score")
    # YOHO-C on host-drawn triples (proper rotations), every hypothesis returned
    tri = np.stack([rs.choice(M, 3, replace=False) for _ in range(I)]).astype(np.int64)
    trid = cu(tri)
    run = lambda: c.c_ransac(k0d, k1d, trid, None, 0.07, want_all=True)
    best_T, res, T_all, counts = run()
    To = np.stack([orc.threepps2tran(k0[t], k1[t], proper=True)[0] for t in tri])
    assert np.allclose(T_all.cpu().numpy(), To, rtol=0, atol=1e-9)
    assert np.array_equal(counts.cpu().numpy(), [orc.inlier_count(k0, k1, T, 0.07) for T in To])
    it, cntc, Tc, _ = orc.yohoc_select(k0, k1, tri, 0.07, proper=True)
    assert tuple(res.cpu().numpy()) == (it, cntc) and np.allclose(best_T.cpu().numpy(), Tc[:3], rtol=0, atol=1e-9)
    poisoned_runs(outp, run, (best_T, res, T_all, counts), "c_ransac")
    # YOHO-C with the sampling on the device
    run = lambda: c.c_ransac_device(k0d, k1d, drd, I, 17, 0.07, want_triples=True)
    best_T, res, trd = run()
    tri2 = orc.yohoc_device_triples(dr, I, 17)
    assert np.array_equal(trd.cpu().numpy(), tri2)
    it, cntc, Tc, _ = orc.yohoc_select(k0, k1, tri2, 0.07, proper=True)
    assert tuple(res.cpu().numpy()) == (it, cntc) and np.allclose(best_T.cpu().numpy(), Tc[:3], rtol=0, atol=1e-9)
    poisoned_runs(outp, run, (best_T, res, trd), "c_ransac_device")


@pytest.mark.parametrize("K", [17, 300])
def test_register_pair_outputs_poisoned(net, octx, outp, K):
    clean = net[0]
    clean.set_gconv_mode("fgemm")
    pr = synth.make_pair(K, seed=640 + K)
    f0, f1 = cu(pr["feat0"]), cu(pr["feat1"])
    o0 = clean.partI_forward(f0, want_inv=False, want_inv_np=True)
    o1 = clean.partI_forward(f1, want_inv=False, want_inv_np=True)
    args = (f0, f1, o0["eqv"], o1["eqv"], o0["inv_np"], o1["inv_np"], cu(pr["keys0"]), cu(pr["keys1"]))
    for est in ("yohoo", "yohoc"):
        run = lambda: octx.register_pair(*args, estimator=est, max_iter=200 if est == "yohoc" else 1000, seed=5)
        ref = run()
        assert not ref["range_flag"] and ref["matches"] > 0, ref
        for p in PATTERNS:
            outp.pattern = p
            try:
                got = run()
            finally:
                outp.pattern = None
            assert got.keys() == ref.keys()
            for k in ref:
                assert raw(np.asarray(got[k])) == raw(np.asarray(ref[k])), (est, K, hex(p), k)


def test_group_gather_and_transfer_outputs_poisoned(octx, tables, outp):
    """an odd number of copies into a poisoned (K, 32, 60) buffer: the columns written equal the clean run's, the others keep the
    pattern (nothing is written outside the copies asked for); the transfer's rotated-keypoint scratch is a poisoned tensor too"""
    c = octx
    rs = np.random.RandomState(650)
    K, n = 301, 2500
    keys = rs.rand(K, 3) * 1.5
    pts = cu(rs.rand(4000, 3) * 1.5)
    kidx = cu(rs.permutation(4000)[:K].astype(np.int64))
    gs = (0, 7, 33, 41, 59)
    tg = [cu((rs.rand(n + g, 3) * 1.5).astype(np.float32)) for g in gs]
    tf = [cu(rs.randn(n + g, 32).astype(np.float32)) for g in gs]
    Rs = [tables.R64[g] for g in gs]
    for cell in (0.0, 0.05):
        c.set_nn_grid(cell)
        try:
            def gather():
                out = torch.empty((K, 32, 60), dtype=torch.float32, device="cuda")
                idx = [c.group_gather(cu(keys), tg[j], tf[j], g, out, want_idx=True) for j, g in enumerate(gs)]
                return out, idx

            def transfer():
                out = torch.empty((K, 32, 60), dtype=torch.float32, device="cuda")
                c.group_transfer_batch(pts, kidx, Rs, tg, tf, 11, out)
                return out

            for name, fn, cols in (("group_gather", gather, list(gs)), ("group_transfer_batch", transfer, list(range(11, 11 + len(gs))))):
                ref = fn()
                out0 = (ref[0] if isinstance(ref, tuple) else ref)[:, :, cols].cpu().numpy()
                assert np.isfinite(out0).all(), (name, cell)
                for p in PATTERNS:
                    outp.pattern = p
                    try:
                        got = fn()
                    finally:
                        outp.pattern = None
                    o = got[0] if isinstance(got, tuple) else got
                    assert raw(o[:, :, cols]) == raw(out0), (name, cell, hex(p))
                    if isinstance(got, tuple):
                        same_bits(ref[1], got[1], (name, cell, hex(p), "idx"))
                    rest = [g for g in range(60) if g not in cols]
                    sp = p - (1 << 32) if p >= 1 << 31 else p
                    assert bool((o[:, :, rest].contiguous().view(torch.int32) == sp).all()), (name, cell, hex(p), "wrote outside its copies")
            # the gather against the oracle (the transfer equals per-copy calls: test_gpu_kernels)
            out, idx = gather()
            for j, g in enumerate(gs[:2]):
                _, idx_o = orc.group_gather_one(keys, tg[j].cpu().numpy(), tf[j].cpu().numpy(), tables.R64[g])
                assert np.array_equal(idx[j].cpu().numpy(), idx_o), (cell, g)
        finally:
            c.set_nn_grid(0)


@pytest.fixture(scope="module")
def fsd():
    return W.synth_state_dict(W.FCGF_SPEC, 3)


def test_fcgf_outputs_poisoned(hip, fsd, tables, outp):
    c = hip.Context()
    c.load_fcgf(fsd)
    clouds = [synth.surface_cloud(1500, seed=1), synth.surface_cloud(6000, seed=2), synth.surface_cloud(1500, seed=3)[:9].copy()]
    # rotated voxelisation of an odd number of copies
    Rs = [tables.R64[g] for g in (0, 7, 41)]
    for pc in clouds:
        pd = cu(pc)
        run = lambda: c.fcgf_voxelize_rotated_batch(pd, Rs, 0.025)
        ref = run()
        for R, (sel, coords, ps) in zip(Rs, ref):
            s0, c0 = fo.voxelize(pc @ R.T, 0.025)
            assert np.array_equal(sel.cpu().numpy(), s0) and np.array_equal(coords.cpu().numpy(), c0)
            assert np.allclose(ps.cpu().numpy(), (pc @ R.T)[s0].astype(np.float32), rtol=0, atol=5e-7)
        poisoned_runs(outp, run, ref, ("voxelize_rotated_batch", len(pc)))
    # the backbone, one cloud per call and three clouds in one call
    coords = [cu(fo.voxelize(pc, 0.025)[1]) for pc in clouds]
    singles = []
    for pc, cd in zip(clouds, coords):
        run = lambda: c.fcgf_forward(cd)
        F = run()
        if len(pc) < 100:                       # the sizes of test_gpu_fcgf against the oracle there; the tiny cloud here
            F0 = fo.extract_features(pc, 0.025, fsd)[1]
            assert F.shape == F0.shape and float(np.abs(F.cpu().numpy() - F0).max()) < 1e-5
        assert torch.isfinite(F).all()
        poisoned_runs(outp, run, F, ("fcgf_forward", len(pc)))
        singles.append(F)
    run = lambda: c.fcgf_forward_batch(coords)
    ref = run()
    for F, Fs in zip(ref, singles):
        assert F.shape == Fs.shape and (F - Fs).abs().max().item() < 2e-5
    poisoned_runs(outp, run, ref, "fcgf_forward_batch")
