"""The consensus entries on the GPU (-m gpu): yoho_consistency_graph, yoho_sc2_scores and yoho_consensus_hypotheses against the numpy
restatement of their contracts (tests/consist_ref.py) - words, degrees, scores, seeds, sizes and info exactly; a transform against the
EXACT Kabsch answer over the same set inside refine_ref.device_tolerance, the rule of tests/test_gpu_refine.py -, consensus.register_matches
on the pairs of tests/test_consist_cpu.py, the refusals through raw ctypes, and the pipeline's consensus option."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import consist_ref as CR  # noqa: E402
import refine_ref as RR  # noqa: E402
import verify_ref as VR  # noqa: E402
import test_consist_cpu as TC  # noqa: E402
from yoho_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
EINVAL, ENOMEM = -1, -4
f32, f64 = np.float32, np.float64
I34 = CR.IDENTITY
PATTERNS = (0xFFFFFFFF, 0x7FC00000, 0x00000001, 0xDEADBEEF, 0x7F800000)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def words(t):
    """the int64 carrier of the graph -> uint64"""
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.Context()


def graph_dev(c, k0, k1, tol, min_len=0.0):
    bits, deg = c.consistency_graph(cu(k0), cu(k1), tol, min_len)
    M = k0.shape[0]
    assert bits.dtype == torch.int64 and deg.dtype == torch.int32 and tuple(bits.shape) == (M, (M + 63) // 64) and tuple(deg.shape) == (M,)
    s2 = c.sc2_scores(bits)
    assert s2.dtype == torch.int32 and tuple(s2.shape) == (M,)
    return bits, deg, s2


def check_graph(c, k0, k1, tol, min_len, what):
    """bits, deg and s2 of the device against the reference, bit for bit -> the reference's (bits, deg, s2)"""
    rb, rd = CR.graph_ref(k0, k1, tol, min_len)
    rs = CR.sc2_ref(rb, k0.shape[0])
    bits, deg, s2 = graph_dev(c, k0, k1, tol, min_len)
    assert np.array_equal(words(bits), rb), (what, "bits")
    assert np.array_equal(deg.cpu().numpy(), rd), (what, "deg")
    assert np.array_equal(s2.cpu().numpy(), rs), (what, "s2")
    return rb, rd, rs


# ---- graph and scores ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 3, 63, 64, 65, 127, 129, 257, 1000, 2100])
def test_graph_and_scores_by_bits(ctx, M):
    """the word edges (63 .. 65, 127, 129), a single word, ragged last words, two row blocks of the graph kernel (257), and every lane layout
    of the score kernel's one-word form: W = 1, 2, 3, 5, 16 and 33 words against groups of 1, 2, 4, 8, 16 and 64 lanes.  Inputs: a cube with a
    planted third (tol 0.3 below 257 matches, so that the small graphs hold triangles; 0.05 above), the same with a NaN row, an infinite
    row and duplicated keypoints at min_len = 0 and > 0"""
    p = CR.planted_case(M, M // 3, M)
    tol = 0.3 if M < 257 else 0.05
    rb, rd, rs = check_graph(ctx, p["k0"], p["k1"], tol, 0.0, (M, "planted"))
    if M >= 63:
        assert rd.max() >= 3 and rs.max() >= 1
    print(f"M {M}: mean degree {rd.mean():.1f}, largest s2 {rs.max() if M else 0}")
    k0, k1 = p["k0"].copy(), p["k1"].copy()
    if M >= 3:
        k0[2], k1[2] = k0[1], k1[1]                               # a = b = 0
    if M >= 70:
        k0[69], k1[69] = k0[5], k1[5]                             # and across a word edge
    k0[0, 1] = np.nan
    k1[M - 1, 2] = np.inf
    for min_len in (0.0, 0.25):
        nb, nd, _ = check_graph(ctx, k0, k1, tol, min_len, (M, "special values", min_len))
        assert nd[0] == 0 and nd[M - 1] == 0
        if M >= 4:
            assert bool((int(nb[1, 0]) >> 2) & 1) == (min_len == 0.0)


def test_graph_thresholds_on_the_lattice(ctx):
    """tests/test_consist_cpu.py's three matches with exact lengths: '<' at tol, '>=' at min_len, one ulp either side"""
    up = lambda x: float(np.nextafter(f64(x), f64(np.inf)))
    k0, k1 = TC.lattice_case()
    for tol, min_len, want in ((1.0, 0.0, [4, 4, 3]), (up(1.0), 0.0, [6, 5, 3]), (up(1.0), 3.0, [6, 5, 3]), (up(1.0), up(3.0), [4, 4, 3]),
                               (up(1.0), up(4.0), [0, 4, 2])):
        rb, _, _ = check_graph(ctx, k0, k1, tol, min_len, ("lattice", tol, min_len))
        assert rb[:, 0].tolist() == want


def test_scores_of_wide_rows(ctx):
    """W = 65 words: the score kernel's second form (a wave per neighbour) and a ragged last word of one bit, on a random symmetric graph
    of 2 % density - no geometry, the entry takes the words as given - with garbage in the tail bits, which it ignores"""
    M = 4097
    rs = np.random.RandomState(5)
    C = np.triu(rs.rand(M, M) < 0.02, 1)
    C = C | C.T
    bits = CR.pack(C)
    ref = CR.sc2_ref(bits, M)
    assert ref.max() > 50
    dirty = bits.copy()
    dirty[:, -1] |= np.uint64(0xFFFFFFFFFFFFFFFE)
    for b in (bits, dirty):
        s2 = ctx.sc2_scores(cu(b.view(np.int64)))
        assert np.array_equal(s2.cpu().numpy(), ref)


# ---- hypotheses ------------------------------------------------------------------------------------------------------------------------
def two_cluster_case(M, seed):
    """planted_case with a second cluster of 12 matches about another transform behind the first"""
    p = CR.planted_case(M, 25, seed)
    rs = np.random.RandomState(900 + seed)
    T2 = RR.perturbed(p["T_gt"], rs, 60, 0.2)
    k0, k1 = p["k0"].copy(), p["k1"].copy()
    k0[25:37] = k1[25:37] @ T2[:, :3].T + T2[:, 3] + 0.01 * rs.randn(12, 3)
    return k0, k1


def hyp_dev(c, k0, k1, bits, s2, K):
    T, seeds, sizes, info = c.consensus_hypotheses(cu(k0), cu(k1), bits, s2, K)
    assert T.dtype == torch.float64 and tuple(T.shape) == (K, 3, 4) and seeds.dtype == sizes.dtype == info.dtype == torch.int32
    assert tuple(seeds.shape) == tuple(sizes.shape) == (K,) and tuple(info.shape) == (2,)
    return T.cpu().numpy(), seeds.cpu().numpy(), sizes.cpu().numpy(), info.cpu().numpy()


def exact_gap(Tr, ref, r, k0, k1):
    """row r of the device against the EXACT Kabsch answer over the reference's set r -> (gap, bound, err, floor); the exact answer and
    its bound are computed once per (reference, row) and shared by every K that asks"""
    memo = ref.setdefault("_exact", {})
    if r not in memo:
        sel = ref["sets"][r]
        Tx = RR.kabsch_exact(k0[sel], k1[sel])
        memo[r] = (Tx,) + tuple(RR.device_tolerance(ref["T"][r], Tx, (k0, k1)))
    Tx, bound, err, floor = memo[r]
    return float(np.abs(Tr - Tx).max()), bound, err, floor


def check_rows(got, ref, K, k0, k1, what):
    """seeds, sizes and info exactly; rows behind Kc; NaN rows; every fitted row against the exact Kabsch answer over its set"""
    T, seeds, sizes, info = got
    Kc = min(K, ref["Kc"])
    assert info.tolist() == [Kc, k0.shape[0]], (what, info)
    assert np.array_equal(seeds[:Kc], ref["seeds"][:Kc]) and np.array_equal(sizes[:Kc], ref["sizes"][:Kc]), (what, seeds, sizes, ref["seeds"], ref["sizes"])
    assert (seeds[Kc:] == -1).all() and (sizes[Kc:] == 0).all() and np.array_equal(T[Kc:], np.tile(I34, (K - Kc, 1, 1))), (what, "rows behind Kc")
    worst = (0.0, 0.0, 0.0)
    for r in range(Kc):
        if sizes[r] < 0:
            assert np.isnan(T[r]).all(), (what, r)
            continue
        assert sizes[r] == ref["sets"][r].sum() >= 3 and np.isfinite(T[r]).all(), (what, r)
        dev, bound, err, floor = exact_gap(T[r], ref, r, k0, k1)
        worst = max(worst, (dev / bound, dev, bound))
        assert dev <= bound, (what, r, dev, err, floor, bound)
    return worst


@pytest.mark.parametrize("M,tol", [(129, 0.05), (257, 0.1), (1000, 0.05)])
def test_hypotheses_against_the_reference(ctx, M, tol):
    """K = 1, 8 and 64 from one graph: the greedy rows of a smaller K are the first rows of a larger one, so one reference (K = 64) serves
    all three.  (129, 0.05) runs out of seeds before 64 rows (K > Kc), (1000, 0.05) does not; 257 has two row blocks with one match in the
    second"""
    k0, k1 = two_cluster_case(M, M)
    rb, rd, rs2 = CR.graph_ref(k0, k1, tol)[0], None, None
    rs2 = CR.sc2_ref(rb, M)
    bits, deg, s2 = graph_dev(ctx, k0, k1, tol)
    assert np.array_equal(words(bits), rb) and np.array_equal(s2.cpu().numpy(), rs2)
    ref = CR.consensus_ref(k0, k1, rb, rs2, 64)
    print(f"M {M}, tol {tol}: Kc {ref['Kc']} of 64, seeds {ref['seeds'][:8].tolist()}, sizes {ref['sizes'][:8].tolist()}, negative sizes {(ref['sizes'] < 0).sum()}")
    assert ref["sizes"][0] >= 20 and ref["seeds"][0] < 25 and 25 <= ref["seeds"][1] < 37
    if M == 129:
        assert 2 <= ref["Kc"] < 64
    if M == 1000:
        assert ref["Kc"] == 64
    for K in (1, 8, 64):
        w = check_rows(hyp_dev(ctx, k0, k1, bits, s2, K), ref, K, k0, k1, (M, tol, K))
        print(f"  K {K}: worst row against the exact Kabsch: device {w[1]:.2e}, bound {w[2]:.2e}")


def test_hypotheses_of_a_wide_graph(ctx):
    """planted_case(4500, 100, 5) at tol 0.05, mean degree 165: W = 71 words and 18 blocks of 256 matches.  The graph and the scores by bits
    (the score kernel's second form on a geometric graph), then K = 8 and 64 against the reference: cs_seed_kernel strides 18 times over
    the matches, cs_sval_kernel's lanes 0 .. 6 take a second word of each row, cs_sum1_kernel takes the maximum over 18 blocks, and the
    fit sums 18 slab rows per hypothesis.  Row 0 is the planted hundred, exactly; all 64 rows are taken and fitted"""
    M = 4500
    p = CR.planted_case(M, 100, 5)
    k0, k1 = p["k0"], p["k1"]
    rb, rd, rs2 = check_graph(ctx, k0, k1, 0.05, 0.0, "wide")
    ref = CR.consensus_ref(k0, k1, rb, rs2, 64)
    print(f"M {M}: mean degree {rd.mean():.1f}, Kc {ref['Kc']}, seeds {ref['seeds'][:8].tolist()}, sizes {ref['sizes'][:8].tolist()}")
    assert ref["Kc"] == 64 and ref["seeds"][0] < 100 and ref["sizes"][0] == 100 and ref["sets"][0][:100].all() and (ref["sizes"] >= 3).all()
    assert RR.rot_error_deg(p["T_gt"][:, :3], ref["T"][0][:, :3]) < 0.5
    bits, _, s2 = graph_dev(ctx, k0, k1, 0.05)
    for K in (8, 64):
        w = check_rows(hyp_dev(ctx, k0, k1, bits, s2, K), ref, K, k0, k1, (M, K))
        print(f"  K {K}: worst row against the exact Kabsch: device {w[1]:.2e}, bound {w[2]:.2e}")


def test_degenerate_sets_give_nan_rows(ctx):
    """a collinear planted set keeps all its distances and has rank below 2; a seed whose set is itself and one partner (the graph of
    tests/test_consist_cpu.py, given as words): NaN rows, negative sizes, and yoho_o_score counts nothing for them"""
    line = np.arange(40, dtype=f64)[:, None] * np.array([[1.0, 2.0, -2.0]]) * 0.125
    rs = np.random.RandomState(4)
    k0 = np.vstack([line, (rs.rand(60, 3) - 0.5) * 3])
    k1 = np.vstack([line + 0.5, (rs.rand(60, 3) - 0.5) * 3])
    rb, _, rs2 = check_graph(ctx, k0, k1, 1e-9, 0.0, "collinear")                  # the line's lengths are exact: a tolerance that admits nobody else
    ref = CR.consensus_ref(k0, k1, rb, rs2, 4)
    assert ref["sizes"].tolist() == [-40, 0, 0, 0] and ref["seeds"][0] == 0
    bits, _, s2 = graph_dev(ctx, k0, k1, 1e-9)
    T, seeds, sizes, info = hyp_dev(ctx, k0, k1, bits, s2, 4)
    check_rows((T, seeds, sizes, info), ref, 4, k0, k1, "collinear")
    assert sizes[0] == -40 and np.isnan(T[0]).all()
    _, counts = ctx.o_score(cu(k0), cu(k1), cu(T), None, 4, 0.09)
    assert int(counts[0]) == 0
    Cm = np.zeros((7, 7), bool)
    for k in range(2, 7):
        Cm[0, k] = Cm[k, 0] = Cm[1, k] = Cm[k, 1] = True
    Cm[0, 1] = Cm[1, 0] = True
    rb = CR.pack(Cm)
    rs2 = CR.sc2_ref(rb, 7)
    ref = CR.consensus_ref(k0[40:47], k1[40:47], rb, rs2, 2)
    assert ref["sizes"].tolist() == [-2, 0]
    bits_d = cu(rb.view(np.int64))
    s2_d = ctx.sc2_scores(bits_d)
    assert s2_d.cpu().numpy().tolist() == rs2.tolist() == [10, 10, 2, 2, 2, 2, 2]
    check_rows(hyp_dev(ctx, k0[40:47], k1[40:47], bits_d, s2_d, 2), ref, 2, k0[40:47], k1[40:47], "a set of two")


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_decoy_pairs_end_to_end(ctx):
    """the four pairs of tests/test_consist_cpu.py through consensus.register_matches, clouds given: the same assertions, the sets taken
    from the reference once seeds and sizes are seen to be its own"""
    from yoho_amd import consensus
    for seed in range(4):
        c, ref, rcounts, v = TC.decoy_consensus(seed)
        k0, k1 = cu(c["k0"]), cu(c["k1"])
        out = consensus.register_matches(ctx, k0, k1, None, 0.03, K=8, inlier_dist=c["inlier_dist"], clouds=(cu(c["tgt"]), cu(c["src"])), max_dist=c["max_dist"])
        assert out["Kc"] == ref["Kc"] and np.array_equal(out["seeds"], ref["seeds"]) and np.array_equal(out["sizes"], ref["sizes"]), (seed, out["seeds"], out["sizes"])
        assert np.array_equal(out["counts"], rcounts), (seed, out["counts"], rcounts)
        T, _, _, _ = ctx.consensus_hypotheses(k0, k1, *graph_dev(ctx, c["k0"], c["k1"], 0.03)[::2], 8)
        sets = [np.nonzero(s)[0].tolist() for s in ref["sets"][:2]]
        err = TC.check_decoy(seed, c, sets, T.cpu().numpy(), out["counts"], out["row"])
        assert np.array_equal(out["top"], v["top"]) and np.array_equal(out["npairs"], v["npairs"]) and out["best"] == v["best"]
        assert out["trans"].tobytes() == T[1].cpu().numpy().tobytes()
        print(f"seed {seed}: seeds {out['seeds'].tolist()}, sizes {out['sizes'].tolist()}, counts {out['counts'].tolist()}, picked row {out['row']} ({err:.2f} deg off), "
              f"refit {out['refit_counts'].tolist()}, {RR.rot_error_deg(c['T_gt'][:, :3], out['trans_refit'][:, :3]):.2f} deg off")
        assert out["inliers"] >= out["counts"][out["row"]] == 12 and out["refit_counts"][0] == 12
        assert RR.rot_error_deg(c["T_gt"][:, :3], out["trans_refit"][:, :3]) < 2.0


def test_planted_case_end_to_end(ctx):
    """planted_case(1000, 30, 1), 3 % inliers, no clouds (the keypoint sets serve), K = 8 and the K = 1 shortcut; the match list given as
    rows into shuffled keypoint arrays"""
    from yoho_amd import consensus
    p = CR.planted_case(1000, 30, 1)
    rs = np.random.RandomState(0)
    p0, p1 = rs.permutation(1000), rs.permutation(1000)
    keys0, keys1 = np.empty_like(p["k0"]), np.empty_like(p["k1"])
    keys0[p0], keys1[p1] = p["k0"], p["k1"]
    match = cu(np.stack([p0, p1], axis=1).astype(np.int64))
    rb, _ = CR.graph_ref(p["k0"], p["k1"], 0.05)
    ref = CR.consensus_ref(p["k0"], p["k1"], rb, CR.sc2_ref(rb, 1000), 8)
    for K in (8, 1):
        out = consensus.register_matches(ctx, cu(keys0), cu(keys1), match, 0.05, K=K, inlier_dist=0.09)
        assert np.array_equal(out["seeds"], ref["seeds"][:K]) and np.array_equal(out["sizes"], ref["sizes"][:K]) and out["Kc"] == K
        err, err_fit = (RR.rot_error_deg(p["T_gt"][:, :3], out[k][:, :3]) for k in ("trans", "trans_refit"))
        print(f"K {K}: seeds {out['seeds'].tolist()}, sizes {out['sizes'].tolist()}, counts {out['counts'].tolist()}, row {out['row']}: {err:.2f} deg off; "
              f"refit {out['refit_counts'].tolist()}: {err_fit:.2f} deg off")
        assert out["seeds"][0] < 30 and out["sizes"][0] == 30 and out["counts"][0] == 30
        assert out["row"] >= 0 and out["counts"][out["row"]] == 30 and err < 0.5
        assert out["inliers"] >= out["counts"][out["row"]] and out["refit_counts"][0] == out["counts"][out["row"]]
        if K == 1:
            assert out["row"] == 0 and out["top"] is None and out["cost"] is None and out["best"] is None
        else:
            assert out["top"].shape == out["cost"].shape == (8,) and 0 < out["fitness"] <= 1


def test_without_clouds_the_whole_keypoint_sets_are_verified(ctx):
    """400 matches of planted_case(1000, 30, 1) as rows into the 1000 keypoints: the verification's figures are those of
    Context.verify_hypotheses on all 1000 keypoints of each side, not on the 400 matched rows; an empty match list runs nothing"""
    from yoho_amd import consensus
    p = CR.planted_case(1000, 30, 1)
    keys0, keys1 = cu(p["k0"]), cu(p["k1"])
    rows = torch.arange(400, dtype=torch.int64, device="cuda")
    match = torch.stack([rows, rows], dim=1)
    out = consensus.register_matches(ctx, keys0, keys1, match, 0.05, K=8, inlier_dist=0.09)
    k0, k1 = keys0[:400].contiguous(), keys1[:400].contiguous()
    bits, _ = ctx.consistency_graph(k0, k1, 0.05, 0.0)
    T, seeds, sizes, info = ctx.consensus_hypotheses(k0, k1, bits, ctx.sc2_scores(bits), 8)
    assert np.array_equal(out["seeds"], seeds.cpu().numpy()) and out["Kc"] == int(info[0]) == 8
    _, counts = ctx.o_score(k0, k1, T, None, 8, 0.09)
    assert np.array_equal(out["counts"], counts.cpu().numpy())
    got = {}
    for name, (src, tgt) in (("whole", (keys1, keys0)), ("matched", (k1, k0))):
        _, top, npairs, rmse, cost, vinfo = ctx.verify_hypotheses(src.float().contiguous(), tgt.float().contiguous(), T, counts, 8, 0.09)
        got[name] = (top.cpu().numpy(), npairs.cpu().numpy(), cost.cpu().numpy())
    assert not np.array_equal(got["whole"][2], got["matched"][2])                      # the two readings differ on this pair
    for k, name in enumerate(("top", "npairs", "cost")):
        assert out[name].tobytes() == got["whole"][k].tobytes(), name
    assert out["fitness"] == float(out["npairs"][out["best"]]) / 1000
    for K in (1, 8):
        e = consensus.register_matches(ctx, keys0, keys1, match[:0], 0.05, K=K, refit_iters=3)
        assert set(e) == set(out) and e["Kc"] == 0 and e["row"] == -1 and e["inliers"] == 0 and e["refit_counts"].tolist() == [0, -1, -1, -1]
        assert np.array_equal(e["trans"], I34) and np.array_equal(e["trans_refit"], I34) and (e["seeds"] == -1).all() and not e["sizes"].any()
        assert (e["top"] is None) == (K == 1) and (e["best"] is None) == (K == 1)


# ---- hygiene ---------------------------------------------------------------------------------------------------------------------------
def test_bits_repeat_over_poisoned_scratch_and_contexts(hip):
    k0, k1 = two_cluster_case(1000, 7)
    first = None
    for rep in range(6):
        if rep in (0, 5):
            cx = hip.Context()                                           # the last repeat on a context of its own
        cx.poison_scratch(PATTERNS[rep % 5])
        bits, deg, s2 = graph_dev(cx, k0, k1, 0.05)
        cx.poison_scratch(PATTERNS[(rep + 1) % 5])
        out = cx.consensus_hypotheses(cu(k0), cu(k1), bits, s2, 64)
        got = [x.cpu().numpy().tobytes() for x in (bits, deg, s2) + tuple(out)]
        if first is None:
            first = got
        assert got == first, rep


def test_entries_refuse_bad_arguments(ctx, hip):
    lib = hip.load_library()
    h = ctx._h
    rs = np.random.RandomState(3)
    k0, k1 = cu(rs.rand(9, 3)), cu(rs.rand(9, 3))
    bits = torch.full((12,), -7, dtype=torch.int64, device="cuda")
    deg = torch.full((12,), -7, dtype=torch.int32, device="cuda")
    s2 = torch.full((12,), -7, dtype=torch.int32, device="cuda")
    To = torch.full((40,), -3.0, dtype=torch.float64, device="cuda")
    seeds = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    sizes = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    info = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())
    off = lambda x, nbytes: C.c_void_p(x.data_ptr() + nbytes)
    N, dbl = None, C.c_double
    big = hip.CONSIST_MAX_M + 1

    def cg(ctx_=h, a=p(k0), b=p(k1), M=9, tol=dbl(0.1), ml=dbl(0.0), bits_=p(bits), deg_=p(deg)):
        return (ctx_, a, b, M, tol, ml, bits_, deg_, N)

    def sc(ctx_=h, bits_=p(bits), M=9, s2_=p(s2)):
        return (ctx_, bits_, M, s2_, N)

    def ch(ctx_=h, a=p(k0), b=p(k1), M=9, bits_=p(bits), s2_=p(s2), K=2, To_=p(To), seeds_=p(seeds), sizes_=p(sizes), info_=p(info)):
        return (ctx_, a, b, M, bits_, s2_, K, To_, seeds_, sizes_, info_, N)

    cases = {
        "yoho_consistency_graph": [
            (cg(ctx_=N), "bad argument"),
            (cg(a=N), "NULL"), (cg(b=N), "NULL"), (cg(bits_=N), "NULL"), (cg(deg_=N), "NULL"),
            (cg(M=0), "M=0"), (cg(M=-1), "M=-1"), (cg(M=big), "YOHO_CONSIST_MAX_M"),
            (cg(tol=dbl(0.0)), "tol"), (cg(tol=dbl(-0.1)), "tol"), (cg(tol=dbl(np.nan)), "tol"), (cg(tol=dbl(np.inf)), "tol"),
            (cg(ml=dbl(-1e-300)), "min_len"), (cg(ml=dbl(np.nan)), "min_len"), (cg(ml=dbl(np.inf)), "min_len"),
            (cg(a=off(k0, 4), M=8), "8-byte aligned"), (cg(b=off(k1, 4), M=8), "8-byte aligned"), (cg(bits_=off(bits, 4)), "8-byte aligned"),
            (cg(deg_=off(deg, 2)), "4-byte aligned"),
        ],
        "yoho_sc2_scores": [
            (sc(ctx_=N), "bad argument"), (sc(bits_=N), "NULL"), (sc(s2_=N), "NULL"),
            (sc(M=0), "M=0"), (sc(M=-5), "M=-5"), (sc(M=big), "YOHO_CONSIST_MAX_M"),
            (sc(bits_=off(bits, 4)), "8-byte aligned"), (sc(s2_=off(s2, 1)), "4-byte aligned"),
        ],
        "yoho_consensus_hypotheses": [
            (ch(ctx_=N), "bad argument"),
            (ch(a=N), "NULL"), (ch(b=N), "NULL"), (ch(bits_=N), "NULL"), (ch(s2_=N), "NULL"), (ch(To_=N), "NULL"), (ch(seeds_=N), "NULL"),
            (ch(sizes_=N), "NULL"), (ch(info_=N), "NULL"),
            (ch(M=0), "M=0"), (ch(M=big), "YOHO_CONSIST_MAX_M"),
            (ch(K=0), "K=0"), (ch(K=-1), "K=-1"), (ch(K=65), "YOHO_CONSIST_MAX_K"),
            (ch(a=off(k0, 4), M=8), "8-byte aligned"), (ch(b=off(k1, 4), M=8), "8-byte aligned"), (ch(bits_=off(bits, 4)), "8-byte aligned"),
            (ch(To_=off(To, 4)), "8-byte aligned"), (ch(s2_=off(s2, 2)), "4-byte aligned"), (ch(seeds_=off(seeds, 2)), "4-byte aligned"),
            (ch(sizes_=off(sizes, 1)), "4-byte aligned"), (ch(info_=off(info, 2)), "4-byte aligned"),
        ],
    }
    assert set(cases) == set(hip.CONSIST_SYMBOLS)                       # every entry of include/yoho_consist.h has its refusals
    for name, rows in cases.items():
        fn = getattr(lib, name)
        for args, text in rows:
            rc = fn(*args)
            msg = lib.yoho_last_error().decode()
            assert rc == EINVAL, (name, text, rc, msg)
            assert name in msg and text in msg, (name, text, msg)
    torch.cuda.synchronize()
    # nothing was launched: every output keeps its pattern
    for t, v in ((bits, -7), (deg, -7), (s2, -7), (seeds, -7), (sizes, -7), (info, -7), (To, -3.0)):
        assert bool((t == v).all())
    # the context works as before, and outputs are written inside their rows only: M = 9 is one word per row, K = 2
    assert lib.yoho_consistency_graph(*cg(tol=dbl(0.4), bits_=off(bits, 8), deg_=off(deg, 4))) == 0, lib.yoho_last_error().decode()
    assert lib.yoho_sc2_scores(*sc(bits_=off(bits, 8), s2_=off(s2, 4))) == 0, lib.yoho_last_error().decode()
    assert lib.yoho_consensus_hypotheses(*ch(bits_=off(bits, 8), s2_=off(s2, 4), To_=off(To, 8), seeds_=off(seeds, 4), sizes_=off(sizes, 4), info_=off(info, 4))) == 0, lib.yoho_last_error().decode()
    torch.cuda.synchronize()
    a, b = k0.cpu().numpy(), k1.cpu().numpy()
    rb, rd = CR.graph_ref(a, b, 0.4)
    rs2 = CR.sc2_ref(rb, 9)
    ref = CR.consensus_ref(a, b, rb, rs2, 2)
    assert rs2.max() >= 1 and ref["Kc"] >= 1
    assert np.array_equal(words(bits[1:10]), rb[:, 0]) and bits[0] == -7 and bool((bits[10:] == -7).all())
    assert np.array_equal(deg[1:10].cpu().numpy(), rd) and deg[0] == -7 and bool((deg[10:] == -7).all())
    assert np.array_equal(s2[1:10].cpu().numpy(), rs2) and s2[0] == -7 and bool((s2[10:] == -7).all())
    assert np.array_equal(seeds[1:3].cpu().numpy(), ref["seeds"]) and seeds[0] == -7 and bool((seeds[3:] == -7).all())
    assert np.array_equal(sizes[1:3].cpu().numpy(), ref["sizes"]) and sizes[0] == -7 and bool((sizes[3:] == -7).all())
    assert info.tolist() == [-7, ref["Kc"], 9, -7] and To[0] == -3.0 and bool((To[25:] == -3.0).all()) and bool((To[1:25] != -3.0).all())


def test_workspace_refusal_is_enomem_and_leaves_the_context_usable(hip, monkeypatch):
    """yoho_consensus_hypotheses at M = 16384, K = 64 asks for 4 MiB of S values, 1 MiB of member flags and 0.5 MiB of partial sums, refused
    by a context whose workspace may not exceed 1 MiB; the refusal comes before anything is launched, so the graph need not be a real one.
    yoho_consistency_graph and yoho_sc2_scores take no workspace at all (their scratch is LDS): they cannot be refused and are not part of
    this case - they run, at the limit, on the refusing context instead"""
    monkeypatch.setenv("YOHO_WS_LIMIT_MB", "1")
    c = hip.Context()
    monkeypatch.delenv("YOHO_WS_LIMIT_MB")
    M = hip.CONSIST_MAX_M
    k = cu(np.random.RandomState(0).rand(M, 3))
    bits = torch.zeros((M, M // 64), dtype=torch.int64, device="cuda")
    s2 = torch.zeros((M,), dtype=torch.int32, device="cuda")
    with pytest.raises(hip.YohoError) as e:
        c.consensus_hypotheses(k, k, bits, s2, 64)
    assert e.value.code == ENOMEM and "workspace" in str(e.value)
    p = CR.planted_case(129, 43, 129)
    rb, rd, rs2 = check_graph(c, p["k0"], p["k1"], 0.3, 0.0, "after the refusal")
    ref = CR.consensus_ref(p["k0"], p["k1"], rb, rs2, 8)
    bits_d, _, s2_d = graph_dev(c, p["k0"], p["k1"], 0.3)
    check_rows(hyp_dev(c, p["k0"], p["k1"], bits_d, s2_d, 8), ref, 8, p["k0"], p["k1"], "after the refusal")
    # the two entries without a workspace at the limit: k against itself keeps every distance - the complete graph
    b, d = c.consistency_graph(k, k, 0.01)
    assert bool((d == M - 1).all())
    s = c.sc2_scores(b[:1024, :16].contiguous())                        # the 1024 x 1024 corner: complete as well
    assert bool((s == 1023 * 1022).all())


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------------
def test_run_pair_consensus_leaves_every_existing_field_as_it_is(hip, sd1, sd2):
    from yoho_amd import pipeline
    c = hip.Context()
    c.load_partI(sd1)
    c.load_partII(sd2)
    pr = synth.make_pair(96, seed=3)
    f0, f1, k0, k1 = cu(pr["feat0"]), cu(pr["feat1"]), cu(pr["keys0"]), cu(pr["keys1"])
    new = ("trans_consensus", "consensus")
    old = tuple(s for s in pipeline.PairResult.__slots__ if s not in new + ("eqv",))
    assert len(old) == len(pipeline.PairResult.__slots__) - 3 and "trans_verified" in old and "refine" in old

    def same(a, b, what):
        if isinstance(a, torch.Tensor):
            assert torch.equal(a, b), what
        elif isinstance(a, np.ndarray):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what
        elif isinstance(a, dict):
            assert set(a) == set(b), what
            for k in a:
                same(a[k], b[k], (what, k))
        else:
            assert a == b and type(a) is type(b), what

    for kw in (dict(estimator="yohoo"), dict(estimator="yohoo", verify=4, refine="refit"), dict(estimator="yohoc", max_iter=200, seed=11)):
        plain = pipeline.run_pair(c, f0, f1, k0, k1, order_rng=np.random.RandomState(0), **kw)
        assert plain.trans_consensus is None and plain.consensus is None and plain.best_count > 0
        con = pipeline.run_pair(c, f0, f1, k0, k1, order_rng=np.random.RandomState(0), consensus=8, **kw)
        for name in old:
            same(getattr(plain, name), getattr(con, name), (kw, name))
        d = con.consensus
        assert set(d) == {"trans", "trans_refit", "refit_counts", "refit_best", "inliers", "row", "Kc", "seeds", "sizes", "counts", "top", "npairs", "rmse", "cost",
                          "best", "fitness"}
        assert con.trans_consensus.shape == (3, 4) and con.trans_consensus.tobytes() == d["trans_refit"].tobytes()
        assert d["seeds"].shape == d["sizes"].shape == d["counts"].shape == d["top"].shape == (8,)
        # the figures are those of the entries on the matched keypoints at tol = inlier_dist
        m = con.match.cpu().numpy()
        a, b = pr["keys0"][m[:, 0]], pr["keys1"][m[:, 1]]
        rb, _ = CR.graph_ref(a, b, 0.09)
        ref = CR.consensus_ref(a, b, rb, CR.sc2_ref(rb, a.shape[0]), 8)
        assert d["Kc"] == ref["Kc"] and np.array_equal(d["seeds"], ref["seeds"]) and np.array_equal(d["sizes"], ref["sizes"])
        print(f"{kw}: estimator {plain.best_count} inliers of {plain.matches} matches; consensus: Kc {d['Kc']}, sizes {d['sizes'].tolist()}, counts {d['counts'].tolist()}, "
              f"row {d['row']}, refit {d['refit_counts'].tolist()}")
        if d["row"] >= 0:
            assert d["inliers"] >= d["counts"][d["row"]]
    # tol and min_len reach the entry
    opt = pipeline.run_pair(c, f0, f1, k0, k1, order_rng=np.random.RandomState(0), consensus=3, consensus_tol=0.05, consensus_min_len=0.2)
    rb, _ = CR.graph_ref(a, b, 0.05, 0.2)
    ref = CR.consensus_ref(a, b, rb, CR.sc2_ref(rb, a.shape[0]), 3)
    assert np.array_equal(opt.consensus["seeds"], ref["seeds"]) and np.array_equal(opt.consensus["sizes"], ref["sizes"])
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError):
            pipeline.run_pair(c, f0, f1, k0, k1, consensus=bad)
