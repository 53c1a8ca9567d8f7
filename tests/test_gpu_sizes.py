"""The entries whose host-side plan depends on the input size, past the sizes at which the plan changes (-m gpu; the plans and the
inputs are tests/size_plan.py's, the conditions on the inputs tests/test_sizes_cpu.py's):

  the cell-sorted grid (rfgrid.hip)   one stable digit pass up to 128 targets, two up to 32 768, three beyond: yoho_nn_within at both sides
                                      of both thresholds and at 100 003 targets (18 bits), every other grid user once at 32 769 - each
                                      walks start / pk with a loop of its own -, and DBSCAN's union on a 65 537-point chain
  yoho_fuse_clouds' scan (fuse.hip)   one level of tile sums up to 2048^2 scanned elements, two beyond: S = 2048^2 and 2048^2 + 1

Everything is compared with the numpy restatements as integers or bytes through the helpers of the entries' own test files; the normals
keep plane_ref.normal_bound (check_normals) and the two ICP steps refine_ref.device_tolerance.  One case is one test: a reference of a
few seconds on the CPU and one call on the device.  profiles/size_thresholds.md holds the measured times."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import size_plan as SP  # noqa: E402
from size_plan import FR, PR, RR  # noqa: E402
import estim_ref as ER  # noqa: E402
from test_gpu_clean import check_knn, check_stat  # noqa: E402
from test_gpu_cluster import KEYS, check as check_dbscan, device_dbscan  # noqa: E402
from test_gpu_fuse import raw  # noqa: E402
from test_gpu_multiway import call as edge_call  # noqa: E402
from test_gpu_plane import check_normals, icp as icp_plane  # noqa: E402
from test_gpu_refine import check_within, lock_step  # noqa: E402
from test_gpu_verify import bits64, cu, eval_dev  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.Context()


# ---- the grid's thresholds through yoho_nn_within ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nt,radius", sorted(set(SP.WITHIN + SP.WITHIN_WINDOW)))
def test_nn_within_at_both_sides_of_the_digit_passes(ctx, Nt, radius):
    """4097 queries on Nt targets of the unit cube: indices and d2 bits are the reference's, and nn_search's where a partner exists"""
    q, tgt = SP.within_case(Nt)
    ridx = check_within(ctx, q, tgt, radius, (Nt, radius, f"{SP.grid_bits(Nt)} bits, {SP.grid_passes(Nt)} passes"))
    has = int((ridx >= 0).sum())
    assert has >= 100 and SP.NQ - has >= 100


def test_nn_within_ties_and_clamped_cells_at_three_passes(ctx):
    """32 769 targets whose last 300 repeat the first 300 (the lower index wins: the sort is stable through all three passes), and the
    far points of test_nn_within_ties_gate_non_finite_and_clamp in the clamped cells"""
    c = SP.ties_case()
    ridx = check_within(ctx, c["q"], c["tgt"], SP.TIES_RADIUS, "duplicates and the clamp, three passes")
    assert (ridx[:100] == np.arange(100)).all() and (ridx[c["far"]] >= 0).sum() > 50 and (ridx[c["far"]] < 0).sum() > 5
    assert np.array_equal(ridx[c["own"]], c["own_idx"])


# ---- every other grid user at 32 769 targets ---------------------------------------------------------------------------------------------
def test_knn_within_at_three_passes(ctx):
    pts = SP.knn_cloud()
    rc = check_knn(ctx, pts, pts, SP.KNN_RADIUS, (SP.KNN_K,), skip=True, what="32 769 self-queries")
    assert (rc == 0).any() and (rc == SP.KNN_K).any() and (rc > SP.KNN_K).any()


def test_statistical_outliers_at_three_passes(ctx):
    ref, _ = check_stat(ctx, SP.knn_cloud(), SP.KNN_RADIUS, SP.KNN_K, what="32 769 points of the unit cube", ref=SP.statistical())
    assert 0 < ref["n_keep"] < ref["stats"][0] < SP.NT_GRID


def test_estimate_normals_at_three_passes(ctx):
    ref, n, _, _ = check_normals(ctx, SP.surface(), SP.NORMAL_RADIUS, "surface cloud, 32 769 points", view=(0.5, 0.5, 3.0))
    assert ref["valid"].mean() >= 0.3 and (~ref["valid"]).sum() >= 1 and 8 <= ref["count"].mean() <= 15


def test_dbscan_at_three_passes(ctx):
    ref = check_dbscan(ctx, SP.dbscan_cloud(), SP.DBSCAN_EPS, SP.DBSCAN_MIN_PTS, "32 769 points of the unit cube", ref=SP.dbscan())
    assert ref["n"][0] >= 1000 and ref["n"][2] >= 5000 and ((ref["core"] == 0) & (ref["labels"] >= 0)).sum() >= 5000


def test_edge_information_at_three_passes(ctx):
    c = SP.pair_case()
    rn, rr, rM = SP.edge_info()
    n, r, M = edge_call(ctx, c["srcs"], cu(c["tgt"]), c["T"], SP.PAIR_GATE)
    assert np.array_equal(n, rn), ("npairs", n, rn)
    assert np.array_equal(bits64(r), bits64(rr)), "rmse bits"
    assert np.array_equal(M, rM), ("info", np.nonzero(M != rM))
    assert (rn > 0).all() and (rn < np.diff(c["soff"])).all()


def test_eval_transforms_at_three_passes(ctx):
    c = SP.pair_case()
    rn, rr, rc = SP.eval_two()
    n, r, co = eval_dev(ctx, c["srcs"][0], c["tgt"], c["T"][:2], SP.PAIR_GATE)
    assert np.array_equal(n, rn), ("npairs", n, rn)
    assert np.array_equal(bits64(r), bits64(rr)) and np.array_equal(bits64(co), bits64(rc)), "rmse / cost bits"
    assert rn[0] != rn[1] and (rn > 0).all() and (rn < SP.NQ).all()


def test_icp_refine_step_at_three_passes(ctx):
    """one iteration (iters = 1) from the reference's iterate: npairs and the bits of rmse equal, T within RR.device_tolerance of the exact
    Kabsch answer over the reference's pairs (test_gpu_refine.lock_step)"""
    c = SP.icp_case()
    n = SP.icp_point_step()[0]
    assert 3 <= n < SP.NQ
    lock_step(ctx, c, [c["T0"]], "4097 on 32 769 surface points")


def test_icp_plane_step_at_three_passes(ctx):
    """test_icp_plane_lock_step_with_the_reference's iteration, once: the target's normals are the reference's, some of them invalid"""
    c = SP.icp_case()
    s = SP.icp_plane_step()
    src, tgt, nrm, md, T0 = c["src"], c["tgt"], c["normals"], c["max_dist"], c["T0"]
    T, npairs, rmse, info = icp_plane(ctx, src, tgt, nrm, T0, md, 1, -1.0)
    assert npairs.tolist() == [s["n"]] and np.array_equal(bits64(rmse), bits64(np.array([s["rmse"]]))), (npairs, rmse, s["n"], s["rmse"])
    assert s["T"] is not None and info.tolist() == [1, RR.ICP_ITERS] and s["n"] < int((s["idx"] >= 0).sum())
    Tx = PR.plane_step_exact(tgt, nrm, T0, s)
    bound, err, floor = RR.device_tolerance(s["T"], Tx, (src, tgt))
    dev = float(np.abs(T - Tx).max())
    defect, det = ER.frame_defect(T[:, :3])
    print(f"4097 on 32 769 surface points: {s['n']} pairs, rmse {s['rmse']:.6f}; against the exact step: device {dev:.2e}, numpy {err:.2e}, floor {floor:.2e}, "
          f"bound {bound:.2e}; |R R^T - I| = {defect:.2e}, det - 1 = {det - 1.0:.2e}")
    assert dev <= bound


# ---- DBSCAN's union on a chain inside the three-pass grid --------------------------------------------------------------------------------
@pytest.mark.parametrize("order", SP.CHAIN_ORDERS)
def test_the_long_snake_is_one_cluster(ctx, order):
    """65 537 points 0.9 eps apart, 257 workgroups: one cluster with label 0, every row core but the two ends.  The expected outputs are
    analytic; tests/test_sizes_cpu.py holds cluster_ref.dbscan_ref against them"""
    pts, _ = SP.chain(order)
    want = SP.chain_expected(order)
    got = device_dbscan(ctx, pts, SP.CHAIN_EPS, 3)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (order, k, np.nonzero(got[k] != want[k])[0][:8])
    assert got["n"].tolist() == [1, 65535, 0] and got["sizes"][0] == 65537


# ---- yoho_fuse_clouds around the second level of its scan --------------------------------------------------------------------------------
def fuse_check(hip, c, S, voxel, min_frags):
    src, soff, T = SP.fuse_case(S)
    ref = SP.fuse_expected(S, voxel, min_frags)
    assert ref["M"] > (2048 ** 2 // 2 if voxel == 0.25 else 2048)
    got = raw(hip, c, src, soff, T, voxel, 1, min_frags, ref=ref)
    assert FR.same_bytes(got, ref) == [], (S, voxel, min_frags, got["M"], ref["M"])


@pytest.mark.parametrize("voxel,min_frags", SP.FUSE_RUNS)
@pytest.mark.parametrize("S", SP.FUSE_S)
def test_fuse_around_the_second_scan_level(hip, ctx, S, voxel, min_frags):
    """three fragments of a 40 m cube: every output and row_of as bytes, guard rows included.  S = 2048^2 scans both its arrays with one
    level and a full top tile; one point more and both take two"""
    assert SP.fuse_scan_levels(S) == SP.fuse_scan_levels(256 * ((S + 255) // 256)) == (1 if S == SP.FUSE_S[0] else 2)
    fuse_check(hip, ctx, S, voxel, min_frags)


def test_fuse_two_scan_levels_over_poisoned_scratch(hip):
    c = hip.Context()
    c.poison_scratch(0xFFFFFFFF)
    fuse_check(hip, c, SP.FUSE_S[1], 0.25, 1)
