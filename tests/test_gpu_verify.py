"""The verification entries on the GPU (-m gpu): yoho_eval_transforms and yoho_verify_hypotheses against the numpy restatement of their
contracts (tests/verify_ref.py) - positions, pair counts and info exactly, rmse and cost by their bits, T_out by its bytes -, against
yoho_icp_refine and yoho_o_score where the header ties them to those, their refusals through raw ctypes, and the pipeline's verify
option.  Nothing here has a tolerance: both entries are exact contracts."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_ref as RR  # noqa: E402
import verify_ref as VR  # noqa: E402
from yoho_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
EINVAL, ENOMEM = -1, -4
f32, f64 = np.float32, np.float64
I34 = VR.IDENTITY
PATTERNS = (0xFFFFFFFF, 0x7FC00000, 0x00000001, 0xDEADBEEF, 0x7F800000)


ROW_OF = np.concatenate([np.arange(16), 4 + np.arange(48) % 12])


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits64(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, f64).view(np.uint64)


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.Context()


def cloud_pair(Ns, Nt, seed):
    """tgt: Nt points of the unit cube; src: Ns of them, drawn with repeats, moved by 3 cm of noise: most have a partner inside 0.1"""
    rs = np.random.RandomState(seed)
    tgt = rs.rand(Nt, 3).astype(f32)
    src = (tgt[rs.randint(Nt, size=Ns)] + 0.03 * rs.randn(Ns, 3)).astype(f32)
    return src, tgt


def eval_rows(seed):
    """64 transforms: the identity, one 100 m away (no pair), one with a NaN entry, one with an infinite one, 12 up to 8 degrees / 0.1 off,
    and those 12 four more times (row k >= 16 is row ROW_OF[k]): the reference evaluates 16 rows, the device all 64"""
    rs = np.random.RandomState(seed)
    T = np.stack([RR.perturbed(I34, rs, 8.0 * rs.rand(), 0.1 * rs.rand()) for _ in range(16)])[ROW_OF]
    T[0] = I34
    T[1] = I34
    T[1, :, 3] = 100.0
    T[2, 1, 1] = np.nan
    T[3, 2, 3] = np.inf
    return T


def eval_dev(c, src, tgt, T, max_dist):
    npairs, rmse, cost = c.eval_transforms(cu(src), cu(tgt), cu(T), max_dist)
    K = T.shape[0]
    assert npairs.dtype == torch.int32 and rmse.dtype == cost.dtype == torch.float64 and tuple(npairs.shape) == tuple(rmse.shape) == tuple(cost.shape) == (K,)
    return npairs.cpu().numpy(), rmse.cpu().numpy(), cost.cpu().numpy()


# ---- yoho_eval_transforms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nt", [1, 65, 4097])
def test_eval_transforms_ragged_sizes_against_the_reference(ctx, Nt):
    """Ns around the wave and block sizes and in 17 blocks, K = 1 (a generic row), 2 (the row without pairs and the NaN row) and 64: one
    reference per size, a row's figures do not depend on its neighbours"""
    T = eval_rows(Nt)
    for Ns in (1, 63, 64, 65, 255, 256, 257, 4097):
        src, tgt = cloud_pair(Ns, Nt, 100 + Ns)
        rn, rr, rc = (x[ROW_OF] for x in VR.eval_ref(src, tgt, T[:16], 0.1))
        assert rn[1] == 0 and rn[2] == 0 and rn[3] == 0 and rr[1] == np.inf and rc[1] == RR.tree_sum(np.full((Ns,), f64(RR.gate2_of(0.1))))
        assert rn[0] > Ns // 2 and rn[4:].max() > 0 and len(set(rn[4:].tolist())) > 1      # the generic rows differ
        for lo, K in ((4, 1), (1, 2), (0, 64)):
            n, r, co = eval_dev(ctx, src, tgt, T[lo:lo + K], 0.1)
            what = (Ns, Nt, K)
            assert np.array_equal(n, rn[lo:lo + K]), (what, "npairs", n, rn[lo:lo + K])
            assert np.array_equal(bits64(r), bits64(rr[lo:lo + K])), (what, "rmse bits")
            assert np.array_equal(bits64(co), bits64(rc[lo:lo + K])), (what, "cost bits")


def test_eval_transforms_row_is_one_icp_iteration(ctx):
    """K = 1: npairs and rmse are yoho_icp_refine(iters = 1)'s, bit for bit; and a second, tighter gate on the same clouds"""
    c = RR.icp_case(n=4000)
    for T0, md in ((c["T0"], c["max_dist"]), (c["T_gt"], 0.02)):
        _, inp, irm, _ = ctx.icp_refine(cu(c["src"]), cu(c["tgt"]), cu(T0), md, 1, -1.0)
        n, r, co = eval_dev(ctx, c["src"], c["tgt"], T0[None], md)
        print(f"icp_case(4000), gate {md}: {n[0]} pairs, rmse {r[0]:.6f}, cost {co[0]:.6f}")
        assert n.tolist() == inp.cpu().numpy().tolist() and 0 < n[0] <= 4000
        assert np.array_equal(bits64(r), bits64(irm))
        g2 = f64(RR.gate2_of(md))
        assert co[0] >= 0 and abs(co[0] - (r[0] ** 2 * n[0] + (4000 - n[0]) * g2)) <= 1e-9 * max(co[0], g2)


# ---- yoho_verify_hypotheses ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    """96 hypotheses in 24 clusters of 4 (entries within 0.004 of the cluster's first), one of them with a NaN entry, on a 300 / 400 point
    pair; their figures at gate 0.1 are computed when first asked for and kept"""
    rs = np.random.RandomState(77)
    src, tgt = cloud_pair(300, 400, 5)
    rows = []
    for _ in range(24):
        base = RR.perturbed(I34, rs, 10.0 * rs.rand(), 0.15 * rs.rand())
        rows += [base] + [base + 0.004 * (rs.rand(3, 4) - 0.5) for _ in range(3)]
    rows = np.stack(rows)
    rows[41, 0, 2] = np.nan
    memo = {}

    def evaluate(R):
        for row in R:
            if row.tobytes() not in memo:
                n, r, c = VR.eval_ref(src, tgt, row[None], 0.1)
                memo[row.tobytes()] = (n[0], r[0], c[0])
        got = [memo[row.tobytes()] for row in R]
        return np.array([g[0] for g in got], np.int32), np.array([g[1] for g in got], f64), np.array([g[2] for g in got], f64)

    return {"src": src, "tgt": tgt, "rows": rows, "evaluate": evaluate, "src_d": cu(src), "tgt_d": cu(tgt)}


def verify_dev(c, src_d, tgt_d, T, order, counts, K, max_dist, min_count, tol):
    out = c.verify_hypotheses(src_d, tgt_d, cu(T), cu(counts), K, max_dist, order=None if order is None else cu(order), min_count=min_count, distinct_tol=tol)
    T_out, top, npairs, rmse, cost, info = out
    assert tuple(T_out.shape) == (3, 4) and tuple(info.shape) == (4,) and all(tuple(x.shape) == (K,) for x in (top, npairs, rmse, cost))
    assert top.dtype == npairs.dtype == info.dtype == torch.int32 and T_out.dtype == rmse.dtype == cost.dtype == torch.float64
    return [x.cpu().numpy() for x in out]


def check_verify(got, ref, what):
    T_out, top, npairs, rmse, cost, info = got
    assert np.array_equal(top, ref["top"]), (what, "top", top, ref["top"])
    assert np.array_equal(npairs, ref["npairs"]), (what, "npairs")
    assert np.array_equal(info, ref["info"]), (what, "info", info, ref["info"])
    assert np.array_equal(bits64(rmse), bits64(ref["rmse"])), (what, "rmse bits")
    assert np.array_equal(bits64(cost), bits64(ref["cost"])), (what, "cost bits")
    assert T_out.tobytes() == ref["T_out"].tobytes(), (what, "T_out bytes")


@pytest.mark.parametrize("H", [0, 1, 255, 256, 257, 5000])
def test_verify_hypotheses_against_the_reference(ctx, pool, H):
    """counts 0 .. 5, so every count is shared by a sixth of the positions; hypotheses drawn from the pool with repeats, so that equal
    rows (equal costs) and near-duplicates both occur; order NULL and a permutation; K, distinct_tol and min_count crossed"""
    rs = np.random.RandomState(H)
    counts = rs.randint(0, 6, size=H).astype(np.int32)
    T = pool["rows"][rs.randint(96, size=H)].reshape(H, 3, 4)
    perm = rs.permutation(H).astype(np.int64)
    seen = set()
    for order in (None, perm):
        for K in (1, 8, 64):
            for tol in (0.0, 0.01):
                for mc in (1, 3):
                    what = (H, "perm" if order is not None else "NULL", K, tol, mc)
                    ref = VR.verify_ref(pool["src"], pool["tgt"], T, order, counts, K, 0.1, mc, tol, evaluate=pool["evaluate"])
                    got = verify_dev(ctx, pool["src_d"], pool["tgt_d"], T, order, counts, K, 0.1, mc, tol)
                    check_verify(got, ref, what)
                    seen.add((ref["Kc"] == K, ref["Kc"] == 0))
    if H == 0:
        assert seen == {(False, True)}
    if H == 5000:
        assert (True, False) in seen and (False, False) in seen      # the suppression leaves fewer than 64 of 96 pool rows


def test_decoy_pairs_end_to_end(ctx):
    """the four pairs of tests/test_verify_cpu.py with the vote's own counts: yoho_o_score -> yoho_verify_hypotheses, nothing read back in
    between; top[0] is the vote's winner, the verified transform is the true cluster's"""
    for seed in range(4):
        c = VR.decoy_case(seed)
        src_d, tgt_d, T_d, order_d = cu(c["src"]), cu(c["tgt"]), cu(c["T"]), cu(c["order"])
        res, counts_d = ctx.o_score(cu(c["k0"]), cu(c["k1"]), T_d, order_d, 200, c["inlier_dist"])
        counts = counts_d.cpu().numpy()
        best_h, best_count = (int(v) for v in res.cpu().numpy())
        assert best_count == counts.max() == 14 and np.array_equal(counts, c["counts"])
        gt = c["T_gt"][:, :3]
        for K, tol in ((8, 0.1), (8, 0.0), (1, 0.0)):
            out = ctx.verify_hypotheses(src_d, tgt_d, T_d, counts_d, K, c["max_dist"], order=order_d, distinct_tol=tol)
            got = [x.cpu().numpy() for x in out]
            ref = VR.verify_ref(c["src"], c["tgt"], c["T"], c["order"], counts, K, c["max_dist"], 1, tol)
            check_verify(got, ref, (seed, K, tol))
            T_out, top, npairs, rmse, cost, info = got
            err = RR.rot_error_deg(gt, T_out[:, :3])
            print(f"seed {seed}, K {K}, tol {tol}: Kc {info[0]}, picked row {info[1]} (position {info[2]}, {info[3]} inliers), {err:.2f} deg off, "
                  f"pairs {npairs[:info[0]].tolist()}, cost {np.round(cost[:info[0]], 3).tolist()}")
            assert top[0] == best_h                                      # the vote's strict '>'
            if tol > 0:
                assert 4 <= info[0] <= 8 and err < 1.0 and cost[info[1]] <= cost[0] - 0.5
            else:
                assert info[0] == K and err > 50.0
        # the verified transform chains into the refit on the device: counts[0] there is the vote's count of the picked position
        T_ver, _, _, _, _, info = ctx.verify_hypotheses(src_d, tgt_d, T_d, counts_d, 8, c["max_dist"], order=order_d, distinct_tol=0.1)
        _, rcounts, _ = ctx.refit_matches(cu(c["k0"]), cu(c["k1"]), T_ver, c["inlier_dist"], 2)
        assert int(rcounts[0]) == int(info[3]) == 12


def test_verify_bits_repeat_over_poisoned_scratch_and_contexts(hip):
    c = VR.decoy_case(1)
    src, tgt = cloud_pair(4097, 4097, 9)
    rows = eval_rows(9)
    first = None
    for rep in range(6):
        if rep in (0, 5):
            cx = hip.Context()                                           # the last repeat on a context of its own
        cx.poison_scratch(PATTERNS[rep % 5])
        a = verify_dev(cx, cu(c["src"]), cu(c["tgt"]), c["T"], c["order"], c["counts"], 8, c["max_dist"], 1, 0.1)
        cx.poison_scratch(PATTERNS[(rep + 1) % 5])
        b = eval_dev(cx, src, tgt, rows, 0.1)
        got = [x.tobytes() for x in list(a) + list(b)]
        if first is None:
            first = got
        assert got == first, rep


# ---- the C ABI's refusals ------------------------------------------------------------------------------------------------------------
def test_entries_refuse_bad_arguments(ctx, hip):
    lib = hip.load_library()
    h = ctx._h
    rs = np.random.RandomState(3)
    s, t = cu(rs.rand(9, 3).astype(f32)), cu(rs.rand(41, 3).astype(f32))
    T = cu(np.tile(I34, (8, 1, 1)))
    order = cu(np.arange(8, dtype=np.int64))
    counts = cu(np.arange(8, dtype=np.int32) + 1)
    To = torch.full((16,), -3.0, dtype=torch.float64, device="cuda")
    top = torch.full((80,), -7, dtype=torch.int32, device="cuda")
    npr = torch.full((80,), -7, dtype=torch.int32, device="cuda")
    info = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    rm = torch.full((80,), -3.0, dtype=torch.float64, device="cuda")
    co = torch.full((80,), -3.0, dtype=torch.float64, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())
    off = lambda x, nbytes: C.c_void_p(x.data_ptr() + nbytes)
    N, f, dbl = None, C.c_float, C.c_double
    big = hip.REFINE_MAX_POINTS + 1

    def ev(ctx_=h, src=p(s), Ns=9, tgt=p(t), Nt=41, T_=p(T), K=2, md=f(0.1), n_=p(npr), r_=p(rm), c_=p(co)):
        return (ctx_, src, Ns, tgt, Nt, T_, K, md, n_, r_, c_, N)

    def vh(ctx_=h, src=p(s), Ns=9, tgt=p(t), Nt=41, T_=p(T), order_=p(order), counts_=p(counts), H=8, K=2, mc=1, tol=dbl(0.0), md=f(0.1), To_=p(To), top_=p(top),
           n_=p(npr), r_=p(rm), c_=p(co), info_=p(info)):
        return (ctx_, src, Ns, tgt, Nt, T_, order_, counts_, H, K, mc, tol, md, To_, top_, n_, r_, c_, info_, N)

    cases = {
        "yoho_eval_transforms": [
            (ev(ctx_=N), "bad argument"),
            (ev(src=N), "NULL"), (ev(tgt=N), "NULL"), (ev(T_=N), "NULL"), (ev(n_=N), "NULL"), (ev(r_=N), "NULL"), (ev(c_=N), "NULL"),
            (ev(Ns=0), "Ns=0"), (ev(Ns=-1), "Ns=-1"), (ev(Nt=0), "Nt=0"),
            (ev(Ns=big), "YOHO_REFINE_MAX_POINTS"), (ev(Nt=big), "YOHO_REFINE_MAX_POINTS"),
            (ev(K=0), "K=0"), (ev(K=-1), "K=-1"), (ev(K=65), "YOHO_VERIFY_MAX_K"),
            (ev(md=f(0.0)), "max_dist"), (ev(md=f(-1.0)), "max_dist"), (ev(md=f(np.inf)), "max_dist"), (ev(md=f(np.nan)), "max_dist"),
            (ev(src=off(s, 2), Ns=8), "4-byte aligned"), (ev(tgt=off(t, 1), Nt=40), "4-byte aligned"), (ev(T_=off(T, 4)), "8-byte aligned"),
            (ev(n_=off(npr, 2)), "4-byte aligned"), (ev(r_=off(rm, 4)), "8-byte aligned"), (ev(c_=off(co, 4)), "8-byte aligned"),
        ],
        "yoho_verify_hypotheses": [
            (vh(ctx_=N), "bad argument"),
            (vh(src=N), "NULL"), (vh(tgt=N), "NULL"), (vh(T_=N), "NULL"), (vh(counts_=N), "NULL"), (vh(To_=N), "NULL"), (vh(top_=N), "NULL"),
            (vh(n_=N), "NULL"), (vh(r_=N), "NULL"), (vh(c_=N), "NULL"), (vh(info_=N), "NULL"),
            (vh(Ns=0), "Ns=0"), (vh(Nt=0), "Nt=0"), (vh(Nt=-3), "Nt=-3"),
            (vh(Ns=big), "YOHO_REFINE_MAX_POINTS"), (vh(Nt=big), "YOHO_REFINE_MAX_POINTS"),
            (vh(H=-1), "H=-1"), (vh(H=big), "YOHO_REFINE_MAX_POINTS"),
            (vh(K=0), "K=0"), (vh(K=65), "YOHO_VERIFY_MAX_K"),
            (vh(mc=0), "min_count=0"), (vh(mc=-2), "min_count=-2"),
            (vh(tol=dbl(-0.1)), "distinct_tol"), (vh(tol=dbl(np.nan)), "distinct_tol"), (vh(tol=dbl(np.inf)), "distinct_tol"),
            (vh(md=f(0.0)), "max_dist"), (vh(md=f(np.inf)), "max_dist"), (vh(md=f(np.nan)), "max_dist"),
            (vh(H=0, md=f(np.nan)), "max_dist"),                                          # no hypotheses does not excuse a bad gate
            (vh(src=off(s, 2), Ns=8), "4-byte aligned"), (vh(tgt=off(t, 3), Nt=40), "4-byte aligned"), (vh(T_=off(T, 4), H=7), "8-byte aligned"),
            (vh(order_=off(order, 4), H=7), "8-byte aligned"), (vh(counts_=off(counts, 2), H=7), "4-byte aligned"), (vh(To_=off(To, 4)), "8-byte aligned"),
            (vh(top_=off(top, 2)), "4-byte aligned"), (vh(n_=off(npr, 1)), "4-byte aligned"), (vh(r_=off(rm, 4)), "8-byte aligned"),
            (vh(c_=off(co, 4)), "8-byte aligned"), (vh(info_=off(info, 2)), "4-byte aligned"),
        ],
    }
    assert set(cases) == set(hip.VERIFY_SYMBOLS)                        # every entry of include/yoho_verify.h has its refusals
    for name, rows in cases.items():
        fn = getattr(lib, name)
        for args, text in rows:
            rc = fn(*args)
            msg = lib.yoho_last_error().decode()
            assert rc == EINVAL, (name, text, rc, msg)
            assert name in msg and text in msg, (name, text, msg)
    torch.cuda.synchronize()
    # nothing was launched: every output keeps its pattern
    assert bool((To == -3.0).all()) and bool((top == -7).all()) and bool((npr == -7).all()) and bool((info == -7).all())
    assert bool((rm == -3.0).all()) and bool((co == -3.0).all())
    # the context works as before: rows of 12 bytes that are not 16-byte aligned, outputs written inside their K rows only
    assert lib.yoho_eval_transforms(*ev(src=off(s, 12), Ns=8, tgt=off(t, 12), Nt=40, n_=off(npr, 4), r_=off(rm, 8), c_=off(co, 8), md=f(0.3))) == 0, lib.yoho_last_error().decode()
    # H = 0 with NULL hypotheses: valid
    n2, r2, c2 = torch.full((4,), -7, dtype=torch.int32, device="cuda"), torch.full((4,), -3.0, dtype=torch.float64, device="cuda"), torch.full((4,), -3.0, dtype=torch.float64, device="cuda")
    assert lib.yoho_verify_hypotheses(*vh(T_=N, order_=N, counts_=N, H=0, K=3, n_=p(n2), r_=p(r2), c_=p(c2))) == 0, lib.yoho_last_error().decode()
    torch.cuda.synchronize()
    rn, rr, rc_ = VR.eval_ref(s.cpu().numpy()[1:], t.cpu().numpy()[1:], np.tile(I34, (2, 1, 1)), 0.3)
    assert np.array_equal(npr[1:3].cpu().numpy(), rn) and np.array_equal(bits64(rm[1:3]), bits64(rr)) and np.array_equal(bits64(co[1:3]), bits64(rc_))
    assert npr[0] == -7 and bool((npr[3:] == -7).all()) and rm[0] == -3.0 and bool((rm[3:] == -3.0).all()) and co[0] == -3.0 and bool((co[3:] == -3.0).all())
    assert top[:4].tolist() == [-1, -1, -1, -7] and info[:5].tolist() == [0, -1, -1, 0, -7] and np.array_equal(To[:12].cpu().numpy().reshape(3, 4), I34)
    assert To[12] == -3.0 and n2.tolist() == [-1, -1, -1, -7] and r2.tolist() == [-1.0, -1.0, -1.0, -3.0] and c2.tolist() == [-1.0, -1.0, -1.0, -3.0]


def test_verify_workspace_refusal_is_enomem_and_leaves_the_context_usable(hip, monkeypatch):
    """64 rows of 200 000 points ask for 1.6 MB of partial sums and the grid for more, refused by a context whose workspace may not
    exceed 1 MiB"""
    monkeypatch.setenv("YOHO_WS_LIMIT_MB", "1")
    c = hip.Context()
    monkeypatch.delenv("YOHO_WS_LIMIT_MB")
    big = cu(np.random.RandomState(0).rand(200000, 3).astype(f32))
    T = cu(np.tile(I34, (64, 1, 1)))
    counts = cu(np.ones((64,), np.int32))
    src, tgt = cloud_pair(257, 65, 4)
    rows = eval_rows(4)[:5]
    rn, rr, rc = VR.eval_ref(src, tgt, rows, 0.1)
    for call in (lambda: c.eval_transforms(big, big, T, 0.01), lambda: c.verify_hypotheses(big, big, T, counts, 64, 0.01)):
        with pytest.raises(hip.YohoError) as e:
            call()
        assert e.value.code == ENOMEM and "workspace" in str(e.value)
        n, r, co = eval_dev(c, src, tgt, rows, 0.1)
        assert np.array_equal(n, rn) and np.array_equal(bits64(r), bits64(rr)) and np.array_equal(bits64(co), bits64(rc))


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------------
def test_run_pair_verify_leaves_every_existing_field_as_it_is(hip, sd1, sd2):
    from yoho_amd import pipeline
    c = hip.Context()
    c.load_partI(sd1)
    c.load_partII(sd2)
    pr = synth.make_pair(96, seed=3)
    f0, f1, k0, k1 = cu(pr["feat0"]), cu(pr["feat1"]), cu(pr["keys0"]), cu(pr["keys1"])
    old = ("match", "dr_index", "quat", "trans_pre", "best_h", "best_count", "trans", "order", "range_repeats", "hyp_rows", "matches", "trans_refined", "refine")
    assert pipeline.PairResult.__slots__[-2:] == ("trans_verified", "verify")

    def same(a, b, what):
        if isinstance(a, torch.Tensor):
            assert torch.equal(a, b), what
        elif isinstance(a, np.ndarray):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what
        else:
            assert a == b and type(a) is type(b), what

    for kw in (dict(estimator="yohoo"), dict(estimator="yohoo", hypotheses="selected", max_iter=20)):
        plain = pipeline.run_pair(c, f0, f1, k0, k1, order_rng=np.random.RandomState(0), **kw)
        assert plain.trans_verified is None and plain.verify is None and plain.best_count > 0
        ver = pipeline.run_pair(c, f0, f1, k0, k1, order_rng=np.random.RandomState(0), verify=8, **kw)
        for name in old:
            same(getattr(plain, name), getattr(ver, name), (kw, name))
        v = ver.verify
        assert set(v) == {"top", "counts", "npairs", "rmse", "cost", "best", "fitness"}
        assert all(v[k].shape == (8,) for k in ("top", "counts", "npairs", "rmse", "cost")) and ver.trans_verified.shape == (3, 4)
        print(f"{kw}: winner {plain.best_count} inliers of {plain.matches} matches; verified: top {v['top'].tolist()}, counts {v['counts'].tolist()}, "
              f"pairs {v['npairs'].tolist()}, best {v['best']}, fitness {v['fitness']:.3f}")
        assert v["top"][0] == plain.best_h and v["counts"][0] == plain.best_count and v["best"] >= 0
        pos = int(v["top"][v["best"]])
        row = pos if ver.hyp_rows is not None else int(ver.order[pos])
        same(ver.trans_verified, ver.trans_pre[row].cpu().numpy(), (kw, "trans_verified"))
        assert v["fitness"] == v["npairs"][v["best"]] / k1.shape[0] and 0 <= v["fitness"] <= 1
        # the figures are those of the entry on the keypoint sets, which serve as the clouds here
        rows = ver.trans_pre.cpu().numpy()[[int(p_) if ver.hyp_rows is not None else int(ver.order[int(p_)]) for p_ in v["top"] if p_ >= 0]]
        rn, rr, rc = VR.eval_ref(pr["keys1"].astype(f32), pr["keys0"].astype(f32), rows, 0.09)
        Kc = rows.shape[0]
        assert np.array_equal(v["npairs"][:Kc], rn) and np.array_equal(bits64(v["cost"][:Kc]), bits64(rc)) and (v["npairs"][Kc:] == -1).all()
        # with a refit behind it: the refit starts from the verified transform, whose vote count is counts[best]
        fit = pipeline.run_pair(c, f0, f1, k0, k1, order_rng=np.random.RandomState(0), verify=8, refine="refit", **kw)
        same(fit.trans_verified, ver.trans_verified, (kw, "trans_verified with refit"))
        assert fit.refine["refit_counts"][0] == fit.verify["counts"][fit.verify["best"]]
        # clouds, gate, suppression and the floor reach the entry
        cl = (k0.to(torch.float32).contiguous(), k1.to(torch.float32).contiguous())
        opt = pipeline.run_pair(c, f0, f1, k0, k1, order_rng=np.random.RandomState(0), verify=3, verify_dist=0.2, verify_distinct=0.05, verify_min_count=2, clouds=cl, **kw)
        assert opt.verify["top"].shape == (3,) and (opt.verify["counts"][opt.verify["top"] >= 0] >= 2).all() and opt.verify["top"][0] == plain.best_h
    with pytest.raises(ValueError):
        pipeline.run_pair(c, f0, f1, k0, k1, estimator="yohoc", verify=8)
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError):
            pipeline.run_pair(c, f0, f1, k0, k1, verify=bad)
