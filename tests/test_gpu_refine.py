"""The refinement entries on the GPU (-m gpu): yoho_nn_within, yoho_refit_matches and yoho_icp_refine against the numpy restatement
of their contracts (tests/refine_ref.py) - indices, counts and the bits of d2 / rmse exactly, transforms against the EXACT Kabsch
answer within a tolerance taken from numpy-f64's own error -, their refusals through raw ctypes, and the pipeline's refine option.

The tolerance of a transform (RR.device_tolerance): numpy-f64's worst entry error against the exact answer on the same inputs,
times 8 (the device sums in another order and decomposes by Jacobi instead of LAPACK: a few ulps each), or 4 ulp of the largest
coordinate magnitude where that is larger (a luckily exact numpy run must not make the bound unreachable).  Every test prints both
figures before it asserts; profiles/refine.md records the measured ones (only the timings there are unmeasured)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_ref as RR  # noqa: E402
import estim_ref as ER  # noqa: E402
from yoho_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
EINVAL = -1
SIZES = (1, 63, 64, 65, 4097, 20000)
RADII = (0.02, 0.1, 0.35)          # below, at and far above the point spacing of 20 000 points in the unit cube: three cell sizes
ORTHO = 32 * 2.0 ** -52            # |R R^T - I| and |det R - 1|: R is a sum of three outer products of unit vectors, each normalised
                                   # to a few ulps - an entry of R R^T carries at most a dozen roundings of values <= 1


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits32(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits64(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.Context()


# ---- yoho_nn_within ------------------------------------------------------------------------------------------------------------------
def within(c, q, t, r, want_d2=True):
    d2, idx = c.nn_within(cu(q), cu(t), r, want_d2=want_d2)
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (q.shape[0],)
    return idx.cpu().numpy(), (None if d2 is None else d2.cpu().numpy())


def check_within(c, q, t, r, what, nn=True):
    ridx, rd2 = RR.nn_within_ref(q, t, r)
    idx, d2 = within(c, q, t, r)
    assert np.array_equal(idx, ridx), (what, "indices")
    assert np.array_equal(bits32(d2), bits32(rd2)), (what, "d2 bits")
    if nn and q.shape[0]:
        nd, ni = c.nn_search(cu(q), cu(t), want_dist=True, squared=True)
        has = ridx >= 0
        assert np.array_equal(ni.cpu().numpy()[has], idx[has]) and np.array_equal(bits32(nd)[has], bits32(d2)[has]), (what, "nn_search")
    return ridx


def test_nn_within_ragged_sizes_and_three_cell_sizes(ctx):
    rs = np.random.RandomState(7)
    n = 0
    for nq in SIZES:
        for nt in SIZES:
            q, t = rs.rand(nq, 3).astype(np.float32), rs.rand(nt, 3).astype(np.float32)
            for r in RADII:
                ridx = check_within(ctx, q, t, r, (nq, nt, r))
                n += 1
                if nq == nt == 20000:
                    print(f"20000 x 20000, radius {r}: {int((ridx >= 0).sum())} queries have a partner")
    print(f"{n} (Nq, Nt, radius) cases identical to the reference in indices and d2 bits, and to nn_search where a partner exists")


def test_nn_within_ties_gate_non_finite_and_clamp(ctx):
    rs = np.random.RandomState(8)
    # duplicate targets: the lower index wins
    base = rs.rand(300, 3).astype(np.float32)
    t = np.concatenate([base, base[::-1], base])
    q = np.concatenate([base[:100], rs.rand(200, 3).astype(np.float32)])
    ridx = check_within(ctx, q, t, 0.08, "duplicates")
    assert (ridx[:100] == np.arange(100)).all()
    # exactly on the gate is out, one ulp inside is in; no partner; NaN / inf queries; a NaN target
    t = np.array([[0, 0, 0], [np.nan, 0, 0], [4, 0, 0], [0, np.nan, 9]], np.float32)
    q = np.array([[0.5, 0, 0], [np.nextafter(np.float32(0.5), np.float32(0)), 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [3.75, 0, 0], [0, -np.inf, 0],
                  [100, 100, 100], [0.3, 0.4, 0]], np.float32)
    idx, d2 = within(ctx, q, t, 0.5)
    assert idx.tolist() == [-1, 0, -1, -1, 2, -1, -1, -1], idx.tolist()            # (0.3, 0.4, 0): 0.09 + 0.16 rounds to >= 0.25
    assert np.isposinf(d2[[0, 2, 3, 5, 6]]).all() and d2[4] == np.float32(0.0625)
    check_within(ctx, q, t, 0.5, "gate", nn=False)
    # coordinates beyond the cell clamp: radius 1e-3 clamps cells at |x| ~ 1049; points around +-5000 with the f32 spacing 2^-11 there
    far = np.zeros((400, 3), np.float32)
    far[:, 0] = np.where(np.arange(400) % 2 == 0, 5000.0, -5000.0) + rs.randint(-14, 15, 400) * 2.0 ** -11
    far[:, 1] = rs.randint(-3, 4, 400) * 2.0 ** -11
    far[:, 2] = 2000.0 + rs.randint(-3, 4, 400) * 2.0 ** -11
    near = rs.rand(500, 3).astype(np.float32) * 0.01
    t = np.concatenate([far[:200], near[:250]])
    q = np.concatenate([far[200:], near[250:], far[:20]])
    ridx = check_within(ctx, q, t, 1e-3, "clamp")
    assert (ridx[:200] >= 0).sum() > 50 and (ridx[:200] < 0).sum() > 5 and (ridx[-20:] == np.arange(20)).all()
    # a gate that holds everything, and one that holds nothing
    q, t = rs.rand(100, 3).astype(np.float32), rs.rand(1000, 3).astype(np.float32)
    assert (check_within(ctx, q, t, 50.0, "huge gate") >= 0).all()
    assert (check_within(ctx, q, t, 1e-6, "tiny gate") == -1).all()
    assert (check_within(ctx, q, t, 1e-30, "gate below the f32 squares", nn=False) == -1).all()
    assert (check_within(ctx, q, t, 3e38, "gate whose square overflows") >= 0).all()
    # no queries, and no distances wanted
    idx, d2 = within(ctx, q[:0], t, 0.1)
    assert idx.shape == (0,) and d2.shape == (0,)
    idx, d2 = within(ctx, q, t, 0.1, want_d2=False)
    assert d2 is None and np.array_equal(idx, RR.nn_within_ref(q, t, 0.1)[0])


def test_nn_within_ignores_switches_scratch_and_call_count(hip):
    c = hip.Context()
    rs = np.random.RandomState(9)
    q, t = rs.rand(4097, 3).astype(np.float32), rs.rand(20000, 3).astype(np.float32)
    ridx, rd2 = RR.nn_within_ref(q, t, 0.03)
    assert 0 < (ridx < 0).sum() < 4097
    for step in range(5):
        if step == 1:
            c.set_nn_grid(0.05); c.set_nn_prefilter(False)
        if step == 2:
            c.poison_scratch(0xFFFFFFFF)
        if step == 3:
            c.poison_scratch(0x7FC00000)
            within(c, t, t, 0.2)                              # a larger call in between leaves its scratch behind
        idx, d2 = within(c, q, t, 0.03)
        assert np.array_equal(idx, ridx) and np.array_equal(bits32(d2), bits32(rd2)), step


# ---- yoho_refit_matches ----------------------------------------------------------------------------------------------------------------
def refit(c, k0, k1, T, d, iters):
    T_out, counts, info = c.refit_matches(cu(k0), cu(k1), cu(T), d, iters)
    return T_out.cpu().numpy(), counts.cpu().numpy(), info.cpu().numpy()


def assert_proper(R, what):
    defect, det = ER.frame_defect(R)
    print(f"{what}: |R R^T - I| = {defect:.2e}, det - 1 = {det - 1.0:.2e}")
    assert defect <= ORTHO and abs(det - 1.0) <= 3 * ORTHO, what


def check_refit(c, case, iters, what):
    k0, k1, T0, d = case["k0"], case["k1"], case["T0"], case["inlier_dist"]
    r = RR.refit_ref(k0, k1, T0, d, iters)
    assert r["margin"] > 1e-6, (what, "the reference itself sits on the threshold")
    T, counts, info = refit(c, k0, k1, T0, d, iters)
    print(f"{what}: counts {counts.tolist()} (reference {r['counts'].tolist()}), info {info.tolist()}")
    assert np.array_equal(counts, r["counts"]), what
    assert info.tolist() == [r["best"], r["evaluated"]], what
    _, voted = c.o_score(cu(k0), cu(k1), cu(T0[None]), None, 1, d)
    assert voted.cpu().numpy().tolist() == [counts[0]], (what, "counts[0] is not o_score's count")
    if r["best"] == 0:
        assert np.array_equal(bits64(T), bits64(T0)), what
    else:
        sel = r["masks"][r["best"] - 1]
        Tx = RR.kabsch_exact(k0[sel], k1[sel])
        bound, err, floor = RR.device_tolerance(r["T"][r["best"]], Tx, (k0, k1))
        dev = float(np.abs(T - Tx).max())
        print(f"{what}: iterate {r['best']} over {int(sel.sum())} matches against the exact Kabsch: device {dev:.2e}, numpy {err:.2e}, 4-ulp floor {floor:.2e}, bound {bound:.2e}")
        assert dev <= bound, what
        assert_proper(T[:, :3], what)
    return r, T, counts


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_refit_counts_and_transform(ctx, seed):
    case = RR.refit_case(seed)
    r, T, counts = check_refit(ctx, case, 8, f"refit seed {seed}")
    assert counts[r["best"]] >= counts[0]
    # fewer iterations: a prefix of the same counts
    for iters in (1, 2):
        _, c2, info2 = refit(ctx, case["k0"], case["k1"], case["T0"], case["inlier_dist"], iters)
        assert np.array_equal(c2, r["counts"][:iters + 1])
    # the output chains: refitting the result again starts from its count
    _, c3, _ = refit(ctx, case["k0"], case["k1"], T, case["inlier_dist"], 2)
    assert c3[0] == counts[r["best"]]


@pytest.mark.parametrize("seed", [1, 5, 11, 9])
def test_refit_returns_the_earliest_best_iterate_when_a_later_one_is_worse(ctx, seed):
    case = RR.noisy_small_case(seed)
    r, T, counts = check_refit(ctx, case, 6, f"noisy seed {seed}")
    c = r["counts"][:r["evaluated"]]
    assert (np.diff(c) < 0).any() and r["best"] < r["evaluated"] - 1, "the case was built so that a later iterate is worse"
    assert r["best"] == int(np.argmax(c)) and counts[r["best"]] == c.max()


def test_refit_edges(ctx):
    case = RR.refit_case(0)
    k0, k1, T0, d = case["k0"], case["k1"], case["T0"], case["inlier_dist"]
    n0 = int((RR.residual2(T0, k0, k1) < d * d).sum())
    T, counts, info = refit(ctx, k0, k1, T0, d, 0)
    assert np.array_equal(bits64(T), bits64(T0)) and counts.tolist() == [n0] and info.tolist() == [0, 1]
    T, counts, info = refit(ctx, k0[:0], k1[:0], T0, d, 3)
    assert np.array_equal(bits64(T), bits64(T0)) and counts.tolist() == [0, -1, -1, -1] and info.tolist() == [0, 1]
    inl = np.nonzero(RR.residual2(T0, k0, k1) < d * d)[0][:2]
    T, counts, info = refit(ctx, k0[inl], k1[inl], T0, d, 3)
    assert np.array_equal(bits64(T), bits64(T0)) and counts.tolist() == [2, -1, -1, -1] and info.tolist() == [0, 1]
    I = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    # collinear and coincident inliers: counted, no transform formed
    line = np.outer(np.linspace(-1, 1, 50), [1.0, 2.0, -0.5]) + [0.3, 0.1, 0.2]
    for pts, what in ((line, "collinear"), (np.tile([[0.25, -1.5, 3.0]], (40, 1)), "coincident")):
        assert RR.refit_ref(pts, pts, I, 0.1, 4)["counts"].tolist() == [len(pts), -1, -1, -1, -1]
        T, counts, info = refit(ctx, pts, pts, I, 0.1, 4)
        assert np.array_equal(bits64(T), bits64(I)) and counts.tolist() == [len(pts), -1, -1, -1, -1] and info.tolist() == [0, 1], what
    # one side collinear only
    rs = np.random.RandomState(4)
    other = line + 0.01 * rs.randn(50, 3)
    T, counts, info = refit(ctx, other, line, I, 0.1, 4)
    assert counts.tolist() == RR.refit_ref(other, line, I, 0.1, 4)["counts"].tolist() == [50, -1, -1, -1, -1]
    # planar inliers must still solve
    plane = np.concatenate([rs.rand(60, 2), np.zeros((60, 1))], axis=1)
    Tg = np.concatenate([RR.rot_axis_angle([1, 2, 3], 25.0), [[0.1], [0.2], [0.3]]], axis=1)
    pc = {"k0": plane @ Tg[:, :3].T + Tg[:, 3], "k1": plane, "T0": RR.perturbed(Tg, rs, 3.0, 0.02), "inlier_dist": 0.05}
    r, T, counts = check_refit(ctx, pc, 4, "planar")
    assert 3 <= counts[0] < 60 and r["best"] >= 1 and counts[r["best"]] == 60 and np.abs(T - Tg).max() < 1e-12


# ---- yoho_icp_refine -----------------------------------------------------------------------------------------------------------------
def icp(c, src, tgt, T, max_dist, iters, tol):
    T_out, npairs, rmse, info = c.icp_refine(cu(src), cu(tgt), cu(T), max_dist, iters, tol)
    return T_out.cpu().numpy(), npairs.cpu().numpy(), rmse.cpu().numpy(), info.cpu().numpy()


@pytest.fixture(scope="module")
def icp_pair():
    c = RR.icp_case()
    return c, RR.icp_ref(c["src"], c["tgt"], c["T0"], c["max_dist"], 30, 0.0)


def lock_step(c, case, ref_T, what):
    """every iteration alone (iters = 1) from the reference's iterate: npairs and the bits of rmse equal, T within the tolerance"""
    src, tgt, md = case["src"], case["tgt"], case["max_dist"]
    worst = (0.0, 0.0, 0.0)
    for i, Ti in enumerate(ref_T):
        n, e, Tn, why, idx = RR.icp_step(src, tgt, Ti, md)
        T, npairs, rmse, info = icp(c, src, tgt, Ti, md, 1, -1.0)
        assert npairs.tolist() == [n] and np.array_equal(bits64(rmse), bits64(np.array([e]))), (what, i, npairs, rmse, n, e)
        assert Tn is not None and info.tolist() == [1, RR.ICP_ITERS]
        sel = idx >= 0
        Tx = RR.kabsch_exact(tgt[idx[sel]].astype(np.float64), src[sel].astype(np.float64))
        bound, err, floor = RR.device_tolerance(Tn, Tx, (src, tgt))
        dev = float(np.abs(T - Tx).max())
        print(f"{what} iteration {i}: {n} pairs, rmse {e:.6f}; against the exact Kabsch: device {dev:.2e}, numpy {err:.2e}, floor {floor:.2e}, bound {bound:.2e}")
        assert dev <= bound, (what, i)
        worst = max(worst, (bound, err, dev))
    return worst


def test_icp_lock_step_with_the_reference(ctx, icp_pair):
    case, ref = icp_pair
    lock_step(ctx, case, ref["T"][:ref["done"]], "surface pair")
    part = RR.icp_case(overlap=0.7)
    pref = RR.icp_ref(part["src"], part["tgt"], part["T0"], part["max_dist"], 3, 0.0)
    assert (pref["npairs"] < 0.8 * part["src"].shape[0]).all() and (pref["npairs"] > 1000).all()       # many source points have no partner
    lock_step(ctx, part, pref["T"][:3], "70 % overlap")


def test_icp_lock_step_on_independent_samplings(ctx):
    """two independent samplings of the surface: no exact partners, near-ties and a pair count that moves from iteration to iteration.
    Early iterations, and late ones near the sampling floor where the correspondences stay non-trivial; a short full run from the start
    must give the reference's pair counts and rmse (the same pairs, iteration by iteration) unless a pair flipped, which is printed."""
    case = RR.icp_halves_case()
    src, tgt, md = case["src"], case["tgt"], case["max_dist"]
    ref = RR.icp_ref(src, tgt, case["T0"], md, 6, 0.0)
    assert ref["done"] == 6 and len(set(ref["npairs"].tolist())) > 1 and (ref["npairs"] < src.shape[0]).any()
    lock_step(ctx, case, ref["T"][:6], "independent halves")
    # near the floor: start from the ground truth, where the iteration has nowhere to go but the pairs are as ambiguous as they get
    late = RR.icp_ref(src, tgt, case["T_gt"], md, 3, 0.0)
    lock_step(ctx, case, late["T"][:3], "independent halves at the floor")
    assert (late["rmse"][:3] > 0.005).all()                       # correspondences are NOT exact here (sampling distance)
    # a gate of the order of the point spacing: about 4 % of the source has no partner and the pair count moves every iteration
    tight = dict(case, max_dist=0.02)
    tref = RR.icp_ref(src, tgt, RR.perturbed(case["T_gt"], np.random.RandomState(1), 0.3, 0.005), 0.02, 4, 0.0)
    assert tref["done"] == 4 and len(set(tref["npairs"].tolist())) == 4 and (tref["npairs"] < 0.97 * src.shape[0]).all()
    lock_step(ctx, tight, tref["T"][:4], "independent halves, gate 0.02")
    T, npairs, rmse, info = icp(ctx, src, tgt, case["T0"], md, 6, -1.0)
    flips = int((npairs != ref["npairs"]).sum())
    print(f"independent halves, 6 iterations in one call: pairs {npairs.tolist()} (reference {ref['npairs'].tolist()}), {flips} iterations with another count, "
          f"final T {float(np.abs(T - ref['T_out']).max()):.2e} from the reference's")
    assert info.tolist() == [6, RR.ICP_ITERS] and npairs[0] == ref["npairs"][0] and np.array_equal(bits64(rmse[:1]), bits64(ref["rmse"][:1]))
    if flips == 0:
        assert np.abs(T - ref["T_out"]).max() < 1e-12


def test_icp_full_run(ctx, icp_pair):
    case, ref = icp_pair
    src, tgt, md, gt = case["src"], case["tgt"], case["max_dist"], case["T_gt"]
    T, npairs, rmse, info = icp(ctx, src, tgt, case["T0"], md, 30, 0.0)
    # the yardstick at the reference's last step
    last = ref["T"][-2] if len(ref["T"]) > 1 else ref["T"][0]
    n, e, Tn, _, idx = RR.icp_step(src, tgt, last, md)
    sel = idx >= 0
    bound, err, floor = RR.device_tolerance(Tn, RR.kabsch_exact(tgt[idx[sel]].astype(np.float64), src[sel].astype(np.float64)), (src, tgt))
    dev = float(np.abs(T - ref["T_out"]).max())
    rot = RR.rot_error_deg(gt[:, :3], T[:, :3])
    print(f"full run: device {info.tolist()} (iterations, reason), reference ({ref['done']}, {ref['reason']}); final T against the reference's: {dev:.2e} "
          f"(10 x tolerance = {10 * bound:.2e}); {rot:.2e} degrees and {np.linalg.norm(gt[:, 3] - T[:, 3]):.2e} m from the ground truth")
    assert dev <= 10 * bound
    assert rot < 0.01
    done = int(info[0])
    assert 1 <= done <= 30 and info[1] in (RR.ICP_ITERS, RR.ICP_CONVERGED)
    k = min(done, ref["done"])
    # the first iteration starts from the same bits; later ones from transforms that differ in their last bits, where a pair on the gate or
    # a near-tie may flip: printed, not asserted
    assert npairs[0] == ref["npairs"][0] and np.array_equal(bits64(rmse[:1]), bits64(ref["rmse"][:1]))
    assert (npairs[done:] == -1).all() and (rmse[done:] == -1.0).all() and (npairs[:done] >= 3).all()
    print(f"full run: npairs differ from the reference's in {int((npairs[:k] != ref['npairs'][:k]).sum())} of {k} iterations, rmse by at most "
          f"{float(np.abs(rmse[:k] / ref['rmse'][:k] - 1.0).max()):.2e} relative")
    assert_proper(T[:, :3], "ICP result")


def test_icp_stop_reasons_and_tol(ctx, icp_pair):
    case, ref = icp_pair
    src, tgt, md, T0 = case["src"], case["tgt"], case["max_dist"], case["T0"]
    # iters reached; iters = 0
    T, npairs, rmse, info = icp(ctx, src, tgt, T0, md, 2, 0.0)
    assert info.tolist() == [2, RR.ICP_ITERS] and np.array_equal(npairs, ref["npairs"][:2]) and np.array_equal(bits64(rmse[:1]), bits64(ref["rmse"][:1]))
    T, npairs, rmse, info = icp(ctx, src, tgt, T0, md, 0, 0.0)
    assert np.array_equal(bits64(T), bits64(T0)) and info.tolist() == [0, RR.ICP_ITERS] and npairs.shape == (0,)
    # tol: the reference's steps are far from the tolerances used here, so the device stops at the same iteration
    deltas = [float(np.abs(b - a).max()) for a, b in zip(ref["T"][:-1], ref["T"][1:])]
    print("reference steps max |T_{i+1} - T_i|:", " ".join(f"{d:.2e}" for d in deltas))
    for tol in (1e9, 1e-3):
        stop = next(i for i, d in enumerate(deltas) if d <= tol)
        assert all(abs(d - tol) > 1e-3 * tol for d in deltas[:stop + 1])
        T, npairs, rmse, info = icp(ctx, src, tgt, T0, md, 30, tol)
        assert info.tolist() == [stop + 1, RR.ICP_CONVERGED], (tol, info.tolist(), stop)
        assert np.abs(T - ref["T"][stop + 1]).max() < 1e-9 and (npairs[stop + 1:] == -1).all()      # T_{i+1} was accepted
    # a negative tol never stops, even at the fixed point the reference converged to
    T, npairs, rmse, info = icp(ctx, src, tgt, ref["T_out"], md, 4, -1.0)
    assert info.tolist() == [4, RR.ICP_ITERS] and (npairs > 0).all()
    # fewer than 3 pairs: T_in is kept
    away = T0.copy(); away[:, 3] += 100.0
    T, npairs, rmse, info = icp(ctx, src, tgt, away, md, 5, 0.0)
    assert np.array_equal(bits64(T), bits64(away)) and info.tolist() == [1, RR.ICP_FEW_PAIRS]
    assert npairs.tolist() == [0, -1, -1, -1, -1] and np.isposinf(rmse[0]) and (rmse[1:] == -1.0).all()
    two = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    I = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    T, npairs, rmse, info = icp(ctx, two, two, I, md, 3, 0.0)
    assert np.array_equal(bits64(T), bits64(I)) and info.tolist() == [1, RR.ICP_FEW_PAIRS] and npairs.tolist() == [2, -1, -1] and rmse[0] == 0.0
    # rank below 2: a cloud on a line
    line = np.outer(np.linspace(-1, 1, 500), [1.0, 2.0, -0.5]).astype(np.float32)
    r = RR.icp_ref(line, line, I, md, 3, 0.0)
    assert (r["done"], r["reason"]) == (1, RR.ICP_RANK)
    T, npairs, rmse, info = icp(ctx, line, line, I, md, 3, 0.0)
    assert np.array_equal(bits64(T), bits64(I)) and info.tolist() == [1, RR.ICP_RANK] and npairs.tolist() == [500, -1, -1]


def test_icp_and_refit_bits_repeat_over_poisoned_scratch(hip, icp_pair):
    c = hip.Context()
    case, _ = icp_pair
    rc = RR.refit_case(2)
    first = None
    for rep in range(5):
        c.poison_scratch((0xFFFFFFFF, 0x7FC00000, 0x00000001, 0xDEADBEEF, 0x7F800000)[rep])
        a = icp(c, case["src"], case["tgt"], case["T0"], case["max_dist"], 6, 0.0)
        b = refit(c, rc["k0"], rc["k1"], rc["T0"], rc["inlier_dist"], 8)
        got = [x.tobytes() for x in a + b]
        if first is None:
            first = got
        assert got == first, rep


# ---- the C ABI's refusals ------------------------------------------------------------------------------------------------------------
def test_entries_refuse_bad_arguments(ctx, hip):
    lib = hip.load_library()
    h = ctx._h
    rs = np.random.RandomState(3)
    q, t = cu(rs.rand(9, 3).astype(np.float32)), cu(rs.rand(41, 3).astype(np.float32))
    k0, k1 = cu(rs.rand(9, 3)), cu(rs.rand(9, 3))
    T = cu(np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1))
    idx = torch.full((16,), -7, dtype=torch.int64, device="cuda")
    d2 = torch.full((16,), -3.0, dtype=torch.float32, device="cuda")
    To = torch.full((16,), -3.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((80,), -7, dtype=torch.int32, device="cuda")
    info = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    rm = torch.full((80,), -3.0, dtype=torch.float64, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())
    off = lambda x, nbytes: C.c_void_p(x.data_ptr() + nbytes)
    N, f, dbl = None, C.c_float, C.c_double
    big = hip.REFINE_MAX_POINTS + 1
    cases = {
        "yoho_nn_within": [
            ((N, p(q), 8, p(t), 40, f(0.1), p(idx), p(d2), N), "bad argument"),
            ((h, N, 8, p(t), 40, f(0.1), p(idx), p(d2), N), "NULL"),
            ((h, p(q), 8, N, 40, f(0.1), p(idx), p(d2), N), "NULL"),
            ((h, p(q), 8, p(t), 40, f(0.1), N, p(d2), N), "NULL"),
            ((h, p(q), -1, p(t), 40, f(0.1), p(idx), N, N), "Nq=-1"),
            ((h, p(q), 8, p(t), 0, f(0.1), p(idx), N, N), "Nt=0"),
            ((h, p(q), big, p(t), 40, f(0.1), p(idx), N, N), "YOHO_REFINE_MAX_POINTS"),
            ((h, p(q), 8, p(t), big, f(0.1), p(idx), N, N), "YOHO_REFINE_MAX_POINTS"),
            ((h, p(q), 8, p(t), 40, f(0.0), p(idx), N, N), "max_dist"),
            ((h, p(q), 8, p(t), 40, f(-1.0), p(idx), N, N), "max_dist"),
            ((h, p(q), 8, p(t), 40, f(np.inf), p(idx), N, N), "max_dist"),
            ((h, p(q), 8, p(t), 40, f(np.nan), p(idx), N, N), "max_dist"),
            ((h, p(q), 0, p(t), 40, f(np.nan), p(idx), N, N), "max_dist"),                  # no rows does not excuse a bad radius
            ((h, off(q, 2), 8, p(t), 40, f(0.1), p(idx), N, N), "4-byte aligned"),
            ((h, p(q), 8, off(t, 1), 40, f(0.1), p(idx), N, N), "4-byte aligned"),
            ((h, p(q), 8, p(t), 40, f(0.1), off(idx, 4), N, N), "8-byte aligned"),
            ((h, p(q), 8, p(t), 40, f(0.1), p(idx), off(d2, 2), N), "4-byte aligned"),
        ],
        "yoho_refit_matches": [
            ((N, p(k0), p(k1), 9, p(T), dbl(0.1), 2, p(To), p(cnt), p(info), N), "bad argument"),
            ((h, N, p(k1), 9, p(T), dbl(0.1), 2, p(To), p(cnt), p(info), N), "NULL"),
            ((h, p(k0), N, 9, p(T), dbl(0.1), 2, p(To), p(cnt), p(info), N), "NULL"),
            ((h, p(k0), p(k1), 9, N, dbl(0.1), 2, p(To), p(cnt), p(info), N), "NULL"),
            ((h, p(k0), p(k1), 9, p(T), dbl(0.1), 2, N, p(cnt), p(info), N), "NULL"),
            ((h, p(k0), p(k1), 9, p(T), dbl(0.1), 2, p(To), N, p(info), N), "NULL"),
            ((h, p(k0), p(k1), 9, p(T), dbl(0.1), 2, p(To), p(cnt), N, N), "NULL"),
            ((h, N, N, 0, N, dbl(0.1), 2, p(To), p(cnt), p(info), N), "NULL"),                # M = 0 still needs T_in
            ((h, p(k0), p(k1), -1, p(T), dbl(0.1), 2, p(To), p(cnt), p(info), N), "M=-1"),
            ((h, p(k0), p(k1), big, p(T), dbl(0.1), 2, p(To), p(cnt), p(info), N), "YOHO_REFINE_MAX_POINTS"),
            ((h, p(k0), p(k1), 9, p(T), dbl(0.1), -1, p(To), p(cnt), p(info), N), "iters=-1"),
            ((h, p(k0), p(k1), 9, p(T), dbl(0.1), 33, p(To), p(cnt), p(info), N), "YOHO_REFIT_MAX_ITERS"),
            ((h, p(k0), p(k1), 9, p(T), dbl(np.nan), 2, p(To), p(cnt), p(info), N), "inlier_dist"),
            ((h, p(k0), p(k1), 9, p(T), dbl(np.inf), 2, p(To), p(cnt), p(info), N), "inlier_dist"),
            ((h, p(k0), p(k1), 9, p(T), dbl(-0.1), 2, p(To), p(cnt), p(info), N), "inlier_dist"),
            ((h, off(k0, 4), p(k1), 8, p(T), dbl(0.1), 2, p(To), p(cnt), p(info), N), "8-byte aligned"),
            ((h, p(k0), p(k1), 9, off(T, 4), dbl(0.1), 2, p(To), p(cnt), p(info), N), "8-byte aligned"),
            ((h, p(k0), p(k1), 9, p(T), dbl(0.1), 2, off(To, 4), p(cnt), p(info), N), "8-byte aligned"),
            ((h, p(k0), p(k1), 9, p(T), dbl(0.1), 2, p(To), off(cnt, 2), p(info), N), "4-byte aligned"),
            ((h, p(k0), p(k1), 9, p(T), dbl(0.1), 2, p(To), p(cnt), off(info, 1), N), "4-byte aligned"),
        ],
        "yoho_icp_refine": [
            ((N, p(q), 9, p(t), 41, p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "bad argument"),
            ((h, N, 9, p(t), 41, p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "NULL"),
            ((h, p(q), 9, N, 41, p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "NULL"),
            ((h, p(q), 9, p(t), 41, N, f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "NULL"),
            ((h, p(q), 9, p(t), 41, p(T), f(0.1), 2, dbl(0.0), N, p(cnt), p(rm), p(info), N), "NULL"),
            ((h, p(q), 9, p(t), 41, p(T), f(0.1), 2, dbl(0.0), p(To), N, p(rm), p(info), N), "NULL"),
            ((h, p(q), 9, p(t), 41, p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), N, p(info), N), "NULL"),
            ((h, p(q), 9, p(t), 41, p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), N, N), "NULL"),
            ((h, p(q), 0, p(t), 41, p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "Ns=0"),
            ((h, p(q), 9, p(t), 0, p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "Nt=0"),
            ((h, p(q), big, p(t), 41, p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "YOHO_REFINE_MAX_POINTS"),
            ((h, p(q), 9, p(t), big, p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "YOHO_REFINE_MAX_POINTS"),
            ((h, p(q), 9, p(t), 41, p(T), f(0.1), -1, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "iters=-1"),
            ((h, p(q), 9, p(t), 41, p(T), f(0.1), 65, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "YOHO_ICP_MAX_ITERS"),
            ((h, p(q), 9, p(t), 41, p(T), f(0.0), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "max_dist"),
            ((h, p(q), 9, p(t), 41, p(T), f(np.inf), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "max_dist"),
            ((h, p(q), 9, p(t), 41, p(T), f(np.nan), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "max_dist"),
            ((h, p(q), 9, p(t), 41, p(T), f(0.1), 2, dbl(np.nan), p(To), p(cnt), p(rm), p(info), N), "tol"),
            ((h, off(q, 2), 8, p(t), 41, p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "4-byte aligned"),
            ((h, p(q), 9, p(t), 41, off(T, 4), f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "8-byte aligned"),
            ((h, p(q), 9, p(t), 41, p(T), f(0.1), 2, dbl(0.0), off(To, 4), p(cnt), p(rm), p(info), N), "8-byte aligned"),
            ((h, p(q), 9, p(t), 41, p(T), f(0.1), 2, dbl(0.0), p(To), off(cnt, 2), p(rm), p(info), N), "4-byte aligned"),
            ((h, p(q), 9, p(t), 41, p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), off(rm, 4), p(info), N), "8-byte aligned"),
        ],
    }
    assert set(cases) == set(hip.REFINE_SYMBOLS)                       # every entry of include/yoho_refine.h has its refusals
    for name, rows in cases.items():
        fn = getattr(lib, name)
        for args, text in rows:
            rc = fn(*args)
            msg = lib.yoho_last_error().decode()
            assert rc == EINVAL, (name, text, rc, msg)
            assert name in msg and text in msg, (name, text, msg)
    torch.cuda.synchronize()
    # nothing was launched: every output keeps its pattern
    assert bool((idx == -7).all()) and bool((d2 == -3.0).all()) and bool((To == -3.0).all()) and bool((cnt == -7).all())
    assert bool((info == -7).all()) and bool((rm == -3.0).all())
    # no queries: valid with NULL data pointers, nothing written; and the context works as before
    assert lib.yoho_nn_within(h, N, 0, N, 40, f(0.1), N, N, N) == 0
    torch.cuda.synchronize()
    assert bool((idx == -7).all())
    # unaligned to 16 but valid rows of 12 bytes, written inside their rows only
    rc = lib.yoho_nn_within(h, off(q, 12), 8, off(t, 12), 40, f(0.3), off(idx, 8), off(d2, 4), N)
    assert rc == 0, lib.yoho_last_error().decode()
    torch.cuda.synchronize()
    ri, rd = RR.nn_within_ref(q.cpu().numpy()[1:], t.cpu().numpy()[1:], 0.3)
    assert np.array_equal(idx[1:9].cpu().numpy(), ri) and np.array_equal(bits32(d2[1:9]), bits32(rd))
    assert idx[0] == -7 and bool((idx[9:] == -7).all()) and d2[0] == -3.0 and bool((d2[9:] == -3.0).all())


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------------
def test_run_pair_refit_leaves_every_existing_field_as_it_is(hip, sd1, sd2):
    from yoho_amd import pipeline
    c = hip.Context()
    c.load_partI(sd1)
    c.load_partII(sd2)
    pr = synth.make_pair(96, seed=3)
    f0, f1, k0, k1 = cu(pr["feat0"]), cu(pr["feat1"]), cu(pr["keys0"]), cu(pr["keys1"])
    old = ("match", "dr_index", "quat", "trans_pre", "best_h", "best_count", "trans", "order", "range_repeats", "hyp_rows", "matches")

    def same(a, b, what):
        if isinstance(a, torch.Tensor):
            assert torch.equal(a, b), what
        elif isinstance(a, np.ndarray):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what
        else:
            assert a == b and type(a) is type(b), what

    for kw in (dict(estimator="yohoo"), dict(estimator="yohoo", hypotheses="selected", max_iter=20), dict(estimator="yohoc", max_iter=200, seed=11, inlier_dist=0.07)):
        plain = pipeline.run_pair(c, f0, f1, k0, k1, order_rng=np.random.RandomState(0), **kw)
        fit = pipeline.run_pair(c, f0, f1, k0, k1, order_rng=np.random.RandomState(0), refine="refit", **kw)
        for name in old:
            same(getattr(plain, name), getattr(fit, name), (kw, name))
        assert plain.trans_refined is None and plain.refine is None
        assert plain.best_count > 0 and fit.trans_refined.shape == (3, 4)
        st = fit.refine
        print(f"{kw}: winner {plain.best_count} inliers of {plain.matches} matches, refit counts {st['refit_counts'].tolist()}, kept iterate {st['refit_best']}")
        assert st["refit_counts"][0] == plain.best_count                 # the vote's own count of the winner
        assert st["inliers"] >= plain.best_count
        assert_proper(fit.trans_refined[:, :3], "refined") if st["refit_best"] > 0 else same(fit.trans_refined, plain.trans, "kept")
    with pytest.raises(ValueError):
        pipeline.run_pair(c, f0, f1, k0, k1, refine="icp")
    # refit + ICP on clouds: the keypoints themselves serve as the two clouds here
    cl = (k0.to(torch.float32).contiguous(), k1.to(torch.float32).contiguous())
    both = pipeline.run_pair(c, f0, f1, k0, k1, order_rng=np.random.RandomState(0), refine="refit+icp", clouds=cl, max_dist=0.2, icp_iters=5)
    assert both.refine["icp_reason"] in hip.ICP_REASONS and both.trans_refined.shape == (3, 4) and both.refine["icp_npairs"].shape == (5,)


# ---- the plug-in ------------------------------------------------------------------------------------------------------------------------
def npz_arrays(path):
    """the arrays of an .npz as (name, dtype, shape, bytes): two np.savez of the same arrays differ in the zip's time stamps, not in these"""
    with np.load(path, allow_pickle=True) as z:
        return [(k, str(z[k].dtype), z[k].shape, z[k].tobytes()) for k in sorted(z.files)]


def test_yohoo_refit_plugin_through_the_evaluator(tmp_path, gold, sd1, sd2):
    """cfg.estimator = 'yohoo_refit' on the drop-in work tree of tests/test_gpu_dropin.py: the evaluator resolves it, the files under
    YOHO_O/ are what a plain yohoo run from the same random state writes (arrays and pre.log byte for byte), the refits go to
    YOHO_O_refit/ with inliers >= inliers_pre and a pre.log of their own, and a pair without a winner keeps yohoo's eye(4)."""
    import types
    from test_gpu_dropin import _make_workdir, prelog_numbers
    from yoho_amd import estimator, evaluator, extractor
    w = _make_workdir(tmp_path, gold, sd1, sd2, "chain.npz")
    assert set(estimator.name2estimator) == {"yohoc", "yohoc_mul", "yohoo"} and set(estimator.extra_estimators) == {"yohoo_refit"}
    assert estimator.get_estimator("yohoo") is estimator.yohoo and estimator.get_estimator("yohoo_refit") is estimator.yohoo_refit
    with pytest.raises(KeyError):
        estimator.get_estimator("nope")

    def cfg(est, dist=0.09):
        c = w.cfg("PartII")
        c.extractor, c.matcher, c.estimator, c.ransac_o_inlinerdist = "PartII", "Match", est, dist
        return c

    extractor.extractor_PartI(w.cfg("PartI")).Extract(w.ds)               # the PartII evaluator reads cached PartI descriptors
    mdir = f"{w.cache}/Match"
    ev0 = evaluator.Evaluator_PartII(cfg("yohoo"), 1000)
    assert type(ev0.estimator) is estimator.yohoo and ev0.yoho_sign == "YOHO_O"
    np.random.seed(1234)
    ev0.run_onescene(w.ds)
    plain_npz, plain_log = npz_arrays(f"{mdir}/YOHO_O/1000iters/0-1.npz"), open(f"{mdir}/YOHO_O/1000iters/pre.log", "rb").read()
    assert not os.path.exists(f"{mdir}/YOHO_O_refit")
    os.remove(f"{mdir}/YOHO_O/1000iters/0-1.npz")
    os.remove(f"{mdir}/YOHO_O/1000iters/pre.log")

    ev1 = evaluator.Evaluator_PartII(cfg("yohoo_refit"), 1000)
    assert type(ev1.estimator) is estimator.yohoo_refit and ev1.yoho_sign == "YOHO_O_refit"
    np.random.seed(1234)
    ev1.run_onescene(w.ds)
    assert npz_arrays(f"{mdir}/YOHO_O/1000iters/0-1.npz") == plain_npz
    assert open(f"{mdir}/YOHO_O/1000iters/pre.log", "rb").read() == plain_log
    z = np.load(f"{mdir}/YOHO_O_refit/1000iters/0-1.npz")
    pre = np.load(f"{mdir}/YOHO_O/1000iters/0-1.npz")
    print(f"yohoo_refit: {int(z['inliers_pre'])} -> {int(z['inliers'])} inliers, counts {z['counts'].tolist()}")
    assert z["trans"].shape == (3, 4) and int(z["recalltime"]) == int(pre["recalltime"])
    assert int(z["inliers"]) >= int(z["inliers_pre"]) > 0 and z["counts"][0] == z["inliers_pre"] and z["counts"].max() == z["inliers"]
    pps = np.load(f"{mdir}/0-1.npy")
    k0, k1 = w.ds.get_kps("0")[pps[:, 0]], w.ds.get_kps("1")[pps[:, 1]]
    for T, n in ((pre["trans"], z["inliers_pre"]), (z["trans"], z["inliers"])):
        assert int((RR.residual2(np.asarray(T)[:3], k0, k1) < 0.09 ** 2).sum()) == int(n)
    log = open(f"{mdir}/YOHO_O_refit/1000iters/pre.log").read()
    assert log == estimator.format_log_entry("0", "1", 2, z["trans"])                    # write_pre_log's one record
    nums = prelog_numbers(log)
    assert nums.shape == (19,) and nums[:3].tolist() == [0, 1, 2] and np.array_equal(nums[3:15].reshape(3, 4), z["trans"])

    # no hypothesis with an inlier: yohoo saves eye(4) and recalltime 0, the plug-in passes them on
    ev2 = evaluator.Evaluator_PartII(cfg("yohoo_refit", dist=0.0), 20)       # no residual is below 0
    np.random.seed(7)
    ev2.estimator.ransac(w.ds, 20)
    z0, z1 = np.load(f"{mdir}/YOHO_O/20iters/0-1.npz"), np.load(f"{mdir}/YOHO_O_refit/20iters/0-1.npz")
    assert np.array_equal(z0["trans"], np.eye(4)) and np.array_equal(z1["trans"], np.eye(4)) and int(z1["recalltime"]) == 0
    assert int(z1["inliers"]) == int(z1["inliers_pre"]) == 0 and (z1["counts"] == -1).all()
    assert os.path.exists(f"{mdir}/YOHO_O_refit/20iters/pre.log")
