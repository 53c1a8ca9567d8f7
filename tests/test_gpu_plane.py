"""The normals / point-to-plane entries on the GPU (-m gpu): yoho_estimate_normals and yoho_icp_plane against the numpy restatement of
their contracts (tests/plane_ref.py) - counts, pair counts and the bits of rmse exactly, normals and transforms against the same
arithmetic at 80 digits within bounds built from numpy-f64's own error -, their refusals through raw ctypes, and the refine options.

The bound of a transform entry is RR.device_tolerance's (profiles/refine.md): the larger of 8 x numpy's worst entry error against the
exact step on the same pairs and 4 ulp of the largest coordinate.  The bound of a normal's angle (PR.normal_bound): the larger of 8 x
numpy's worst angle against the exact normals of the case and the Davis-Kahan figure 4 n 2^-53 / relgap of the point, plus the rounding
of a unit vector to f32.  Every test prints the figures before it asserts; profiles/plane_icp.md records them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_ref as PR  # noqa: E402
import refine_ref as RR  # noqa: E402
import estim_ref as ER  # noqa: E402
from yoho_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
EINVAL, ENOMEM = -1, -4
I34 = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits64(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.Context()


# ---- yoho_estimate_normals -----------------------------------------------------------------------------------------------------------
def normals(c, pts, radius, min_nbrs=6, view=(0.0, 0.0, 0.0)):
    n, cnt, cv = c.estimate_normals(cu(pts), radius, min_nbrs, view, want_curv=True)
    assert n.dtype == torch.float32 and tuple(n.shape) == (pts.shape[0], 3) and cnt.dtype == torch.int32 and cv.dtype == torch.float32
    return n.cpu().numpy(), cnt.cpu().numpy(), cv.cpu().numpy()


def check_normals(c, pts, radius, what, min_nbrs=6, view=(0.0, 0.0, 0.0), exact=64):
    """-> (reference, device normals, worst device angle, worst bound)"""
    pts = np.ascontiguousarray(pts, np.float32)
    N = pts.shape[0]
    ref = PR.normals_ref(pts, radius, min_nbrs, view)
    n, cnt, cv = normals(c, pts, radius, min_nbrs, view)
    assert np.array_equal(cnt, ref["count"]), (what, "count")
    valid = (n != 0).any(axis=1)
    with np.errstate(invalid="ignore"):
        band = (ref["count"] >= min_nbrs) & (np.abs(ref["ratio"] / PR.COLLINEAR_TOL - 1.0) <= PR.BAND)
    assert band.sum() <= 0.01 * N and np.array_equal(valid[~band], ref["valid"][~band]), (what, "the invalid set")
    assert (cv[~valid] == -1).all() and (n[~valid] == 0).all(), what
    both = np.nonzero(valid & ref["valid"])[0]
    if both.size == 0:
        print(f"{what}: {N} points, no valid normal")
        return ref, n, 0.0, 0.0
    lam = ref["lam"][both]
    relgap = (lam[:, 1] - lam[:, 0]) / lam[:, 2]
    sample = both[np.unique(np.linspace(0, both.size - 1, min(exact, both.size)).astype(int))]
    ex = [PR.normal_exact(pts, i, radius) for i in sample]
    numpy_worst = max(PR.angle_to_exact(ref["n64"][i], e) for i, e in zip(sample, ex))
    worst = (0.0, 0.0)
    for i, e in zip(sample, ex):
        assert e["count"] == cnt[i]
        ang, bound = PR.angle_to_exact(n[i], e), PR.normal_bound(numpy_worst, e["count"], e["relgap"])
        worst = max(worst, (ang / bound, ang, bound))
    ang = PR.angle_between(n[both], ref["n64"][both])
    bound = np.array([PR.normal_bound(numpy_worst, k, g) for k, g in zip(ref["count"][both], relgap)])
    print(f"{what}: {N} points, {both.size} valid, neighbours median {int(np.median(cnt))}; numpy's worst angle to the exact normal on {len(sample)} points "
          f"{numpy_worst:.2e}; device: {worst[1]:.2e} to the exact normal (bound {worst[2]:.2e}), {ang.max():.2e} to numpy's on all (smallest bound {bound.min():.2e})")
    assert worst[0] <= 1.0, (what, "angle to the exact normal")
    assert (ang <= bound).all(), (what, "angle to numpy's normal")
    # curvature: the same relative figure, and the absolute error of an eigenvalue of an n-term f64 sum (Weyl: 4 n 2^-53 l3, below 4 n 2^-53 of the trace)
    cr = ref["curv"][both].astype(np.float64)
    assert (np.abs(cv[both].astype(np.float64) - cr) <= bound * np.abs(cr) + 4.0 * ref["count"][both] * 2.0 ** -53).all(), (what, "curvature")
    # orientation: a component of the output carries half an f32 ulp, so the product may miss 0 by 2^-25 |v - p|_1
    d = np.asarray(view, np.float32).astype(np.float64) - pts[both].astype(np.float64)
    dot = (n[both].astype(np.float64) * d).sum(axis=1)
    assert (dot >= -2.0 ** -25 * np.abs(d).sum(axis=1)).all(), (what, "orientation")
    assert np.abs(np.linalg.norm(n[both].astype(np.float64), axis=1) - 1.0).max() <= 2 * PR.ROUND32
    return ref, n, worst[1], worst[2]


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 3000])
def test_normals_ragged_sizes_and_three_cell_sizes(ctx, N):
    """points in the unit cube; three radii: a third of the 30-neighbour radius (cells much smaller than the cloud, most points
    below min_nbrs), the 30-neighbour radius, and 2.0 (one cell holds the whole cloud); two viewpoints"""
    rs = np.random.RandomState(100 + N)
    pts = rs.rand(N, 3).astype(np.float32)
    r30 = min(0.9, float((30.0 / (N * 4.19)) ** (1.0 / 3.0)))
    for radius, view in ((r30 / 3, (0.0, 0.0, 0.0)), (r30, (3.0, -2.0, 5.0)), (2.0, (0.0, 0.0, 0.0))):
        check_normals(ctx, pts, radius, f"N = {N}, radius {radius:.3f}", view=view)
    # a surface: the normals mean something
    if N >= 1000:
        check_normals(ctx, synth.surface_cloud(N, seed=5), 0.15 if N == 3000 else 0.25, f"surface cloud, N = {N}", view=(0.5, 0.5, 3.0))


def test_normals_cell_boundaries_gate_duplicates_and_non_finite(ctx):
    rs = np.random.RandomState(21)
    # radius 0.25 is exact in f32 and so is its cell side 0.25 (1 + 2^-10): a lattice of step 0.25 (neighbours at d2 == gate2 exactly: out), points
    # exactly on cell boundaries and one ulp to either side of them, and a jittered copy that fills the neighbourhoods
    radius, cell = 0.25, 0.25 * (1.0 + 2.0 ** -10)
    k = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), axis=-1).reshape(-1, 3)
    lattice = (k * 0.25).astype(np.float32) + np.float32(8.0)
    ref = PR.normals_ref(lattice, radius, 3)
    assert (ref["count"] == 1).all()                                     # every lattice neighbour sits exactly on the gate
    n, cnt, cv = normals(ctx, lattice, radius, 3)
    assert (cnt == 1).all() and (n == 0).all() and (cv == -1).all()
    edge = (k * cell).astype(np.float32)
    assert np.array_equal(edge.astype(np.float64), k * cell)             # exactly on the boundaries
    up, down = edge.copy(), edge.copy()
    up[:, 0], down[:, 1] = np.nextafter(edge[:, 0], np.float32(9)), np.nextafter(edge[:, 1], np.float32(-9))
    cloud = np.concatenate([edge, up, down, -edge, (k * 0.25).astype(np.float32), (rs.rand(400, 3) * 0.8 - 0.05).astype(np.float32)])
    check_normals(ctx, cloud, radius, "cell boundaries and the gate", min_nbrs=3)
    # duplicates are neighbours of their own; a NaN and an infinite point have count 0 and are nobody's neighbour
    base = rs.rand(300, 3).astype(np.float32)
    cloud = np.concatenate([base, base[:100], base[:50]])
    cloud[17] = [np.nan, 0.5, 0.5]
    cloud[333] = [0.5, np.inf, 0.5]
    ref, n, _, _ = check_normals(ctx, cloud, 0.2, "duplicates, NaN, inf")
    assert ref["count"][17] == 0 and ref["count"][333] == 0 and (ref["count"][300:317] >= 2).all()
    # far beyond the cell clamp
    far = (rs.rand(200, 3) * 0.004).astype(np.float32)
    far[:100] += np.float32(4000.0)
    check_normals(ctx, far, 1e-3, "beyond the clamp", min_nbrs=3)


def test_normals_degenerate_neighbourhoods_and_an_exact_plane(ctx):
    rs = np.random.RandomState(22)
    line = (np.outer(np.arange(50), [1.0, 2.0, -0.5]) / 64).astype(np.float32) + np.float32(0.5)
    ref, n, _, _ = check_normals(ctx, line, 0.25, "collinear")
    assert not ref["valid"].any() and ref["count"].min() >= 6
    n, cnt, cv = normals(ctx, line, 0.25, 6)
    assert (n == 0).all() and (cv == -1).all()
    # min_nbrs decides: the same cloud with 8 and with 40
    pts = rs.rand(500, 3).astype(np.float32)
    ref, n, _, _ = check_normals(ctx, pts, 0.15, "min_nbrs = 8", min_nbrs=8)
    assert 0 < ref["valid"].sum() < 500
    n, cnt, cv = normals(ctx, pts, 0.15, 40)
    assert (cnt < 40).all() and (n == 0).all() and (cv == -1).all()
    # an exact plane z = 0.5: +-(0, 0, 1) by the viewpoint, curvature 0
    plane = np.concatenate([rs.rand(700, 2), np.full((700, 1), 0.5)], axis=1).astype(np.float32)
    for view, sign in (((0.0, 0.0, 5.0), 1.0), ((0.0, 0.0, -5.0), -1.0), ((0.3, 0.3, 0.5), 1.0)):
        ref, n, _, _ = check_normals(ctx, plane, 0.1, f"exact plane seen from {view}", view=view)
        ok = (n != 0).any(axis=1)
        assert ok.sum() > 600 and PR.angle_between(n[ok], np.tile([[0.0, 0.0, 1.0]], (int(ok.sum()), 1))).max() <= PR.ROUND32
        assert (np.sign(n[ok, 2]) == sign).all()


# ---- yoho_icp_plane ------------------------------------------------------------------------------------------------------------------
def icp(c, src, tgt, nrm, T, max_dist, iters, tol):
    T_out, npairs, rmse, info = c.icp_plane(cu(src), cu(tgt), cu(nrm), cu(T), max_dist, iters, tol)
    return T_out.cpu().numpy(), npairs.cpu().numpy(), rmse.cpu().numpy(), info.cpu().numpy()


def lock_case(name):
    kind = "same" if name == "same" else "halves"
    c = dict(PR.plane_pair(kind, 3000))
    if name == "halves, half the normals zeroed":
        nrm = c["normals"].copy()
        nrm[::2] = 0.0
        nrm[1] = np.nan                                               # and one that is not finite
        c["normals"] = nrm
    return c


@pytest.mark.parametrize("name", ["same", "halves", "halves, half the normals zeroed"])
def test_icp_plane_lock_step_with_the_reference(ctx, name):
    """every iteration alone (iters = 1) from the reference's iterate: npairs and the bits of rmse equal, T_{i+1} within the bound of the
    exact step"""
    c = lock_case(name)
    src, tgt, nrm, md = c["src"], c["tgt"], c["normals"], c["max_dist"]
    ref = PR.icp_plane_ref(src, tgt, nrm, c["T0"], md, 6, 1e-12)
    assert ref["done"] >= 5
    for i, Ti in enumerate(ref["T"][:ref["done"]]):
        s = PR.plane_step(src, tgt, nrm, Ti, md)
        T, npairs, rmse, info = icp(ctx, src, tgt, nrm, Ti, md, 1, -1.0)
        assert npairs.tolist() == [s["n"]] and np.array_equal(bits64(rmse), bits64(np.array([s["rmse"]]))), (name, i, npairs, rmse, s["n"], s["rmse"])
        assert s["T"] is not None and info.tolist() == [1, RR.ICP_ITERS]
        Tx = PR.plane_step_exact(tgt, nrm, Ti, s)
        bound, err, floor = RR.device_tolerance(s["T"], Tx, (src, tgt))
        dev = float(np.abs(T - Tx).max())
        defect, det = ER.frame_defect(T[:, :3])
        print(f"{name} iteration {i}: {s['n']} pairs, rmse {s['rmse']:.6f}; against the exact step: device {dev:.2e}, numpy {err:.2e}, floor {floor:.2e}, "
              f"bound {bound:.2e}; |R R^T - I| = {defect:.2e}, det - 1 = {det - 1.0:.2e}")
        assert dev <= bound, (name, i)
    if name != "same":
        assert (ref["npairs"][:ref["done"]] < 3000).any()
    if name.endswith("zeroed"):
        assert (ref["npairs"][:ref["done"]] < 1600).all() and (ref["npairs"][:ref["done"]] > 1000).all()


@pytest.mark.parametrize("kind", ["same", "halves"])
def test_icp_plane_full_run(ctx, kind):
    """the 20 000-point pairs with the device's own normals at radius 0.06: the device stops at the iteration and for the reason the
    reference does (tol = 1e-12), its final transform within 10 x the step bound of the reference's - so the convergence figures of
    tests/test_plane_cpu.py hold on the device"""
    c = (RR.icp_case if kind == "same" else RR.icp_halves_case)()
    src, tgt, md, gt = c["src"], c["tgt"], c["max_dist"], c["T_gt"]
    n_d, cnt_d = ctx.estimate_normals(cu(tgt), 0.06)
    nrm, cnt = n_d.cpu().numpy(), cnt_d.cpu().numpy()
    invalid = int((nrm == 0).all(axis=1).sum())
    print(f"{kind}: neighbours min {cnt.min()} median {int(np.median(cnt))}, {invalid} invalid normals of 20 000")
    assert invalid <= 20 and np.median(cnt) > 20
    ref = PR.icp_plane_ref(src, tgt, nrm, c["T0"], md, 30, 1e-12)
    assert ref["reason"] == RR.ICP_CONVERGED and all(abs(d - 1e-12) > 1e-13 for d in ref["deltas"])
    T, npairs, rmse, info = icp(ctx, src, tgt, nrm, c["T0"], md, 30, 1e-12)
    last = ref["T"][-2]
    s = PR.plane_step(src, tgt, nrm, last, md)
    bound, err, floor = RR.device_tolerance(s["T"], PR.plane_step_exact(tgt, nrm, last, s), (src, tgt))
    dev = float(np.abs(T - ref["T_out"]).max())
    rot = RR.rot_error_deg(gt[:, :3], T[:, :3])
    print(f"{kind} full run: device {info.tolist()} (iterations, reason), reference ({ref['done']}, {ref['reason']}); steps " + " ".join(f"{d:.1e}" for d in ref["deltas"])
          + f"; final T against the reference's {dev:.2e} (10 x bound = {10 * bound:.2e}, numpy {err:.2e}); {rot:.2e} degrees and "
          f"{np.linalg.norm(gt[:, 3] - T[:, 3]):.2e} m from the ground truth")
    assert info.tolist() == [ref["done"], ref["reason"]]
    assert dev <= 10 * bound
    done = ref["done"]
    assert npairs[0] == ref["npairs"][0] and np.array_equal(bits64(rmse[:1]), bits64(ref["rmse"][:1]))
    assert (npairs[done:] == -1).all() and (rmse[done:] == -1.0).all() and (npairs[:done] >= 6).all()
    print(f"{kind} full run: npairs differ from the reference's in {int((npairs[:done] != ref['npairs'][:done]).sum())} of {done} iterations")
    if kind == "halves":
        assert rot <= 0.02 and done <= 20                              # no sampling floor: point-to-point stops at 0.056 here
    else:
        assert rot <= 1e-6 and ref["deltas"][5] <= 1e-8


def test_icp_plane_stop_rules_and_fills(ctx):
    c = PR.plane_pair("same", 3000)
    src, tgt, nrm, md, T0 = c["src"], c["tgt"], c["normals"], c["max_dist"], c["T0"]
    ref = PR.icp_plane_ref(src, tgt, nrm, T0, md, 8, -1.0)
    # iters = 0
    T, npairs, rmse, info = icp(ctx, src, tgt, nrm, T0, md, 0, 0.0)
    assert np.array_equal(bits64(T), bits64(T0)) and info.tolist() == [0, RR.ICP_ITERS] and npairs.shape == (0,) and rmse.shape == (0,)
    # iters reached
    T, npairs, rmse, info = icp(ctx, src, tgt, nrm, T0, md, 2, 0.0)
    assert info.tolist() == [2, RR.ICP_ITERS] and npairs.tolist() == ref["npairs"][:2].tolist() and np.array_equal(bits64(rmse[:1]), bits64(ref["rmse"][:1]))
    assert np.abs(T - ref["T"][2]).max() < 1e-12
    # a large tol: converged after one iteration, T_1 accepted; a negative one never stops, even at the fixed point
    print("reference steps max |T_{i+1} - T_i|:", " ".join(f"{d:.2e}" for d in ref["deltas"]))
    T, npairs, rmse, info = icp(ctx, src, tgt, nrm, T0, md, 7, 1e9)
    assert info.tolist() == [1, RR.ICP_CONVERGED] and np.abs(T - ref["T"][1]).max() < 1e-12
    assert npairs.tolist() == [ref["npairs"][0]] + [-1] * 6 and rmse[0] > 0 and (rmse[1:] == -1.0).all()
    stop = next(i for i, d in enumerate(ref["deltas"]) if d <= 1e-5)
    assert all(abs(d - 1e-5) > 1e-8 for d in ref["deltas"]) and stop >= 2
    T, npairs, rmse, info = icp(ctx, src, tgt, nrm, T0, md, 8, 1e-5)
    assert info.tolist() == [stop + 1, RR.ICP_CONVERGED] and np.abs(T - ref["T"][stop + 1]).max() < 1e-12 and (npairs[stop + 1:] == -1).all()
    T, npairs, rmse, info = icp(ctx, src, tgt, nrm, ref["T_out"], md, 4, -1.0)
    assert info.tolist() == [4, RR.ICP_ITERS] and (npairs == 3000).all() and (rmse >= 0).all()
    # five source points: fewer than 6 pairs, T_in kept, rmse owed all the same
    few = PR.icp_plane_ref(src[:5], tgt, nrm, c["T_gt"], md, 3, 0.0)
    assert (few["done"], few["reason"]) == (1, RR.ICP_FEW_PAIRS) and few["npairs"][0] == 5
    T, npairs, rmse, info = icp(ctx, src[:5], tgt, nrm, c["T_gt"], md, 3, 0.0)
    assert np.array_equal(bits64(T), bits64(c["T_gt"])) and info.tolist() == [1, RR.ICP_FEW_PAIRS] and npairs.tolist() == [5, -1, -1]
    assert np.array_equal(bits64(rmse), bits64(few["rmse"]))
    # no pair at all
    away = T0.copy()
    away[:, 3] += 100.0
    T, npairs, rmse, info = icp(ctx, src, tgt, nrm, away, md, 3, 0.0)
    assert np.array_equal(bits64(T), bits64(away)) and info.tolist() == [1, RR.ICP_FEW_PAIRS] and npairs.tolist() == [0, -1, -1]
    assert np.isposinf(rmse[0]) and (rmse[1:] == -1.0).all()
    # every normal (0, 0, 0): the neighbours exist, no pair is kept
    T, npairs, rmse, info = icp(ctx, src, tgt, np.zeros_like(nrm), T0, md, 2, 0.0)
    assert np.array_equal(bits64(T), bits64(T0)) and info.tolist() == [1, RR.ICP_FEW_PAIRS] and npairs.tolist() == [0, -1]
    # an exact plane with the caller's (0, 0, 1) normals: rank 3, T_in returned
    rs = np.random.RandomState(1)
    flat = np.concatenate([rs.rand(500, 2), np.zeros((500, 1))], axis=1).astype(np.float32)
    up = np.tile(np.array([[0, 0, 1]], np.float32), (500, 1))
    r = PR.icp_plane_ref(flat, flat, up, I34, 0.1, 3, 0.0)
    assert (r["done"], r["reason"]) == (1, RR.ICP_RANK)
    T, npairs, rmse, info = icp(ctx, flat, flat, up, I34, 0.1, 3, 0.0)
    assert np.array_equal(bits64(T), bits64(I34)) and info.tolist() == [1, RR.ICP_RANK] and npairs.tolist() == [500, -1, -1]
    assert np.array_equal(bits64(rmse), bits64(r["rmse"])) and rmse[0] == 0.0


def test_plane_bits_repeat_over_poisoned_scratch_switches_and_calls(hip):
    c = hip.Context()
    p = PR.plane_pair("halves", 3000)
    src, tgt, md = p["src"], p["tgt"], p["max_dist"]

    def old():
        return [x.cpu().numpy().tobytes() for x in c.icp_refine(cu(src), cu(tgt), cu(p["T0"]), md, 3, 0.0)]

    pp = RR.icp_ref(src, tgt, p["T0"], md, 3, 0.0)
    before = old()
    assert before[1] == pp["npairs"].tobytes() and before[2][:8] == pp["rmse"][:1].tobytes()       # icp_refine's own contract
    first = None
    for rep in range(6):
        if rep < 5:
            c.poison_scratch((0xFFFFFFFF, 0x7FC00000, 0x00000001, 0xDEADBEEF, 0x7F800000)[rep])
        if rep == 2:
            c.set_nn_grid(0.05)
            c.set_nn_prefilter(False)
        if rep == 4:
            c.estimate_normals(cu(np.random.RandomState(0).rand(20000, 3).astype(np.float32)), 0.3)      # a larger call leaves its scratch behind
        n, cnt, cv = c.estimate_normals(cu(tgt), p["normal_radius"], 6, (0.1, 0.2, 0.3), want_curv=True)
        got = [x.cpu().numpy().tobytes() for x in (n, cnt, cv)] + [x.tobytes() for x in icp(c, src, tgt, p["normals"], p["T0"], md, 5, 0.0)]
        if first is None:
            first = got
        assert got == first, rep
    assert old() == before


# ---- the C ABI's refusals ------------------------------------------------------------------------------------------------------------
def test_plane_entries_refuse_bad_arguments(ctx, hip):
    lib = hip.load_library()
    h = ctx._h
    rs = np.random.RandomState(3)
    q, t, nr = cu(rs.rand(9, 3).astype(np.float32)), cu(rs.rand(41, 3).astype(np.float32)), cu(rs.rand(41, 3).astype(np.float32))
    T = cu(I34)
    out = torch.full((160,), -3.0, dtype=torch.float32, device="cuda")
    cv = torch.full((48,), -3.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((80,), -7, dtype=torch.int32, device="cuda")
    To = torch.full((16,), -3.0, dtype=torch.float64, device="cuda")
    info = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    rm = torch.full((80,), -3.0, dtype=torch.float64, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())
    off = lambda x, nbytes: C.c_void_p(x.data_ptr() + nbytes)
    N, f, dbl = None, C.c_float, C.c_double
    z = f(0.0)
    big = hip.REFINE_MAX_POINTS + 1
    cases = {
        "yoho_estimate_normals": [
            ((N, p(t), 41, f(0.1), 6, z, z, z, p(out), p(cnt), p(cv), N), "bad argument"),
            ((h, N, 41, f(0.1), 6, z, z, z, p(out), p(cnt), p(cv), N), "NULL"),
            ((h, p(t), 41, f(0.1), 6, z, z, z, N, p(cnt), p(cv), N), "NULL"),
            ((h, p(t), 41, f(0.1), 6, z, z, z, p(out), N, p(cv), N), "NULL"),
            ((h, p(t), 0, f(0.1), 6, z, z, z, p(out), p(cnt), p(cv), N), "N=0"),
            ((h, p(t), -1, f(0.1), 6, z, z, z, p(out), p(cnt), p(cv), N), "N=-1"),
            ((h, p(t), big, f(0.1), 6, z, z, z, p(out), p(cnt), p(cv), N), "YOHO_REFINE_MAX_POINTS"),
            ((h, p(t), 41, f(0.0), 6, z, z, z, p(out), p(cnt), p(cv), N), "radius"),
            ((h, p(t), 41, f(-1.0), 6, z, z, z, p(out), p(cnt), p(cv), N), "radius"),
            ((h, p(t), 41, f(np.inf), 6, z, z, z, p(out), p(cnt), p(cv), N), "radius"),
            ((h, p(t), 41, f(np.nan), 6, z, z, z, p(out), p(cnt), p(cv), N), "radius"),
            ((h, p(t), 41, f(0.1), 2, z, z, z, p(out), p(cnt), p(cv), N), "min_nbrs=2"),
            ((h, p(t), 41, f(0.1), -5, z, z, z, p(out), p(cnt), p(cv), N), "min_nbrs=-5"),
            ((h, p(t), 41, f(0.1), 6, f(np.nan), z, z, p(out), p(cnt), p(cv), N), "viewpoint"),
            ((h, p(t), 41, f(0.1), 6, z, f(np.inf), z, p(out), p(cnt), p(cv), N), "viewpoint"),
            ((h, p(t), 41, f(0.1), 6, z, z, f(-np.inf), p(out), p(cnt), p(cv), N), "viewpoint"),
            ((h, off(t, 2), 40, f(0.1), 6, z, z, z, p(out), p(cnt), p(cv), N), "4-byte aligned"),
            ((h, p(t), 41, f(0.1), 6, z, z, z, off(out, 1), p(cnt), p(cv), N), "4-byte aligned"),
            ((h, p(t), 41, f(0.1), 6, z, z, z, p(out), off(cnt, 2), p(cv), N), "4-byte aligned"),
            ((h, p(t), 41, f(0.1), 6, z, z, z, p(out), p(cnt), off(cv, 3), N), "4-byte aligned"),
        ],
        "yoho_icp_plane": [
            ((N, p(q), 9, p(t), 41, p(nr), p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "bad argument"),
            ((h, N, 9, p(t), 41, p(nr), p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "NULL"),
            ((h, p(q), 9, N, 41, p(nr), p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "NULL"),
            ((h, p(q), 9, p(t), 41, N, p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "NULL"),
            ((h, p(q), 9, p(t), 41, p(nr), N, f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "NULL"),
            ((h, p(q), 9, p(t), 41, p(nr), p(T), f(0.1), 2, dbl(0.0), N, p(cnt), p(rm), p(info), N), "NULL"),
            ((h, p(q), 9, p(t), 41, p(nr), p(T), f(0.1), 2, dbl(0.0), p(To), N, p(rm), p(info), N), "NULL"),
            ((h, p(q), 9, p(t), 41, p(nr), p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), N, p(info), N), "NULL"),
            ((h, p(q), 9, p(t), 41, p(nr), p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), N, N), "NULL"),
            ((h, p(q), 9, p(t), 41, N, p(T), f(0.1), 0, dbl(0.0), p(To), N, N, p(info), N), "NULL"),                    # iters = 0 still needs the normals
            ((h, p(q), 0, p(t), 41, p(nr), p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "Ns=0"),
            ((h, p(q), 9, p(t), 0, p(nr), p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "Nt=0"),
            ((h, p(q), big, p(t), 41, p(nr), p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "YOHO_REFINE_MAX_POINTS"),
            ((h, p(q), 9, p(t), big, p(nr), p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "YOHO_REFINE_MAX_POINTS"),
            ((h, p(q), 9, p(t), 41, p(nr), p(T), f(0.1), -1, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "iters=-1"),
            ((h, p(q), 9, p(t), 41, p(nr), p(T), f(0.1), 65, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "YOHO_ICP_MAX_ITERS"),
            ((h, p(q), 9, p(t), 41, p(nr), p(T), f(0.0), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "max_dist"),
            ((h, p(q), 9, p(t), 41, p(nr), p(T), f(np.inf), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "max_dist"),
            ((h, p(q), 9, p(t), 41, p(nr), p(T), f(np.nan), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "max_dist"),
            ((h, p(q), 9, p(t), 41, p(nr), p(T), f(0.1), 2, dbl(np.nan), p(To), p(cnt), p(rm), p(info), N), "tol"),
            ((h, off(q, 2), 8, p(t), 41, p(nr), p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "4-byte aligned"),
            ((h, p(q), 9, p(t), 41, off(nr, 1), p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "4-byte aligned"),
            ((h, p(q), 9, p(t), 41, p(nr), off(T, 4), f(0.1), 2, dbl(0.0), p(To), p(cnt), p(rm), p(info), N), "8-byte aligned"),
            ((h, p(q), 9, p(t), 41, p(nr), p(T), f(0.1), 2, dbl(0.0), off(To, 4), p(cnt), p(rm), p(info), N), "8-byte aligned"),
            ((h, p(q), 9, p(t), 41, p(nr), p(T), f(0.1), 2, dbl(0.0), p(To), off(cnt, 2), p(rm), p(info), N), "4-byte aligned"),
            ((h, p(q), 9, p(t), 41, p(nr), p(T), f(0.1), 2, dbl(0.0), p(To), p(cnt), off(rm, 4), p(info), N), "8-byte aligned"),
        ],
    }
    assert set(cases) == set(hip.PLANE_SYMBOLS)                        # every entry of include/yoho_plane.h has its refusals
    for name, rows in cases.items():
        fn = getattr(lib, name)
        for args, text in rows:
            rc = fn(*args)
            msg = lib.yoho_last_error().decode()
            assert rc == EINVAL, (name, text, rc, msg)
            assert name in msg and text in msg, (name, text, msg)
    torch.cuda.synchronize()
    # nothing was launched: every output keeps its pattern
    assert bool((out == -3.0).all()) and bool((cv == -3.0).all()) and bool((cnt == -7).all()) and bool((To == -3.0).all())
    assert bool((info == -7).all()) and bool((rm == -3.0).all())
    # rows of 12 bytes that are not 16-byte aligned, curv NULL: valid, written inside their rows only
    rc = lib.yoho_estimate_normals(h, off(t, 12), 40, f(0.4), 3, z, z, z, off(out, 12), off(cnt, 4), N, N)
    assert rc == 0, lib.yoho_last_error().decode()
    torch.cuda.synchronize()
    ref = PR.normals_ref(t.cpu().numpy()[1:], 0.4, 3)
    assert np.array_equal(cnt[1:41].cpu().numpy(), ref["count"]) and bool((cnt[0] == -7)) and bool((cnt[41:] == -7).all())
    got = out[3:123].cpu().numpy().reshape(40, 3)
    assert (PR.angle_between(got[ref["valid"]], ref["n64"][ref["valid"]]) < 1e-6).all() and ref["valid"].sum() > 20
    assert bool((out[:3] == -3.0).all()) and bool((out[123:] == -3.0).all()) and bool((cv == -3.0).all())


def test_plane_workspace_refusal_is_enomem_and_leaves_the_context_usable(hip, monkeypatch):
    """the grid of 200 000 points asks for several MB, refused by a context whose workspace may not exceed 1 MiB"""
    monkeypatch.setenv("YOHO_WS_LIMIT_MB", "1")
    c = hip.Context()
    monkeypatch.delenv("YOHO_WS_LIMIT_MB")
    big = cu(np.random.RandomState(0).rand(200000, 3).astype(np.float32))
    small = PR.plane_pair("same", 3000)
    for call in (lambda: c.estimate_normals(big, 0.01), lambda: c.icp_plane(big, big, big, cu(I34), 0.01, 2, 0.0)):
        with pytest.raises(hip.YohoError) as e:
            call()
        assert e.value.code == ENOMEM and "workspace" in str(e.value)
        n, cnt = c.estimate_normals(cu(small["tgt"]), small["normal_radius"])
        assert np.array_equal(cnt.cpu().numpy(), small["nref"]["count"])
        T, npairs, rmse, info = icp(c, small["src"], small["tgt"], small["normals"], small["T0"], small["max_dist"], 1, -1.0)
        s = PR.plane_step(small["src"], small["tgt"], small["normals"], small["T0"], small["max_dist"])
        assert npairs.tolist() == [s["n"]] and np.array_equal(bits64(rmse), bits64(np.array([s["rmse"]])))


# ---- the Python layers ---------------------------------------------------------------------------------------------------------------
def test_run_pair_plane_leaves_every_existing_field_and_the_point_path_as_they_are(hip, sd1, sd2):
    from yoho_amd import pipeline, refine
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

    cl = (k0.to(torch.float32).contiguous(), k1.to(torch.float32).contiguous())       # the keypoints serve as the two clouds here
    plain = pipeline.run_pair(c, f0, f1, k0, k1, order_rng=np.random.RandomState(0))
    plane = pipeline.run_pair(c, f0, f1, k0, k1, order_rng=np.random.RandomState(0), refine="refit+icp_plane", clouds=cl, max_dist=0.2, icp_iters=5,
                              normal_radius=0.4)
    point = pipeline.run_pair(c, f0, f1, k0, k1, order_rng=np.random.RandomState(0), refine="refit+icp", clouds=cl, max_dist=0.2, icp_iters=5)
    for name in old:
        same(getattr(plain, name), getattr(plane, name), name)
    assert plain.best_count > 0 and plain.refine is None
    st = plane.refine
    print(f"refit+icp_plane: reason {st['icp_reason']}, iterations {st['icp_iters']}, pairs {st['icp_npairs'].tolist()}, rmse {st['icp_rmse'].tolist()}")
    assert st["icp_mode"] == "plane" and point.refine["icp_mode"] == "point"
    assert st["icp_reason"] in hip.ICP_REASONS and plane.trans_refined.shape == (3, 4) and st["icp_npairs"].shape == (5,) and st["icp_rmse"].shape == (5,)
    assert set(st) == set(point.refine) and np.array_equal(plane.trans_refined, st["trans_icp"])
    for key in ("trans_refit", "refit_counts", "refit_best", "refit_evaluated", "inliers"):
        same(st[key], point.refine[key], key)
    # normal_radius = None means max_dist
    a = pipeline.run_pair(c, f0, f1, k0, k1, order_rng=np.random.RandomState(0), refine="refit+icp_plane", clouds=cl, max_dist=0.4, icp_iters=3)
    b = pipeline.run_pair(c, f0, f1, k0, k1, order_rng=np.random.RandomState(0), refine="refit+icp_plane", clouds=cl, max_dist=0.4, icp_iters=3, normal_radius=0.4)
    assert a.refine["trans_icp"].tobytes() == b.refine["trans_icp"].tobytes() and a.refine["icp_rmse"].tobytes() == b.refine["icp_rmse"].tobytes()
    with pytest.raises(ValueError):
        pipeline.run_pair(c, f0, f1, k0, k1, refine="icp")
    with pytest.raises(ValueError):
        pipeline.run_pair(c, f0, f1, k0, k1, refine="refit+icp_plane")
    # icp = "point" through refine_pair is the entries chained by hand, bit for bit
    T0 = cu(np.ascontiguousarray(plain.trans[:3]))
    m0, m1 = k0[plain.match[:, 0]].contiguous(), k1[plain.match[:, 1]].contiguous()
    T_fit, counts, _ = c.refit_matches(m0, m1, T0, 0.09, 4)
    T_icp, npairs, rmse, iinfo = c.icp_refine(cl[1], cl[0], T_fit, 0.2, 5, 0.0)
    for kw in (dict(), dict(icp="point")):
        got = refine.refine_pair(c, k0, k1, plain.match, T0, 0.09, clouds=cl, max_dist=0.2, icp_iters=5, **kw)
        assert got["trans_icp"].tobytes() == T_icp.cpu().numpy().tobytes() and got["icp_rmse"].tobytes() == rmse.cpu().numpy().tobytes()
        assert got["icp_npairs"].tolist() == npairs.cpu().numpy().tolist() and got["icp_mode"] == "point"
        assert got["trans_refit"].tobytes() == T_fit.cpu().numpy().tobytes() and got["refit_counts"].tolist() == counts.cpu().numpy().tolist()
    with pytest.raises(ValueError):
        refine.refine_pair(c, k0, k1, plain.match, T0, 0.09, clouds=cl, max_dist=0.2, icp="lines")
