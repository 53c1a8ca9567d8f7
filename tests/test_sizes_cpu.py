"""tests/size_plan.py on the CPU: the restated plans at both sides of their thresholds, the constants they rest on against the two
sources, and every reference tests/test_gpu_sizes.py uses on its own inputs, with the conditions that make a case worth running - so
that a change to a generator cannot empty a case unnoticed.  No GPU, no library."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import size_plan as SP  # noqa: E402
from size_plan import CL, CR, PR, RR  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOVE_GRID = ("tests/test_gpu_sizes.py pins the grid's digit passes with size_plan.WITHIN (128 / 129 and 32 768 / 32 769 targets, 100 003 for 18 bits), "
             "NT_GRID = 32 769 for every other grid user and CHAIN_N = 65 537: move them to both sides of the new thresholds")
MOVE_FUSE = ("tests/test_gpu_sizes.py pins fu_scan's levels with size_plan.FUSE_S = (4 194 304, 4 194 305) = FU_TILE^2 and FU_TILE^2 + 1 points: "
             "move them to both sides of the new two-level threshold")


def source(name):
    with open(os.path.join(REPO, "yoho_amd", "csrc", name)) as f:
        return f.read()


# ---- the plans ---------------------------------------------------------------------------------------------------------------------------
def test_grid_plan_at_its_thresholds():
    assert [SP.grid_passes(n) for n in (1, 128, 129, 32768, 32769, 100003, 1 << 22)] == [1, 1, 2, 2, 3, 3, 3], MOVE_GRID
    assert [SP.grid_bits(n) for n in (1, 128, 129, 32768, 32769, 100003, 1 << 22)] == [8, 8, 9, 16, 17, 18, 23], MOVE_GRID
    assert SP.grid_bits(20000) == 16 and SP.grid_passes(20360) == 2                # the largest targets of the other GPU files: two passes
    assert SP.grid_passes(SP.NT_GRID) == 3 and SP.grid_passes(SP.CHAIN_N) == 3, MOVE_GRID
    assert [SP.grid_passes(n) for n, _ in SP.WITHIN] == [1, 2, 2, 3, 3] and {n for n, _ in SP.WITHIN} == {n for n, _ in SP.WITHIN_WINDOW}, MOVE_GRID
    assert (1 << SP.grid_bits(SP.NT_GRID)) + 1 > 65537                             # start[] beyond 16 bits of slots


def test_fuse_scan_plan_at_its_thresholds():
    assert [SP.fuse_scan_levels(n) for n in (1, 2048, 2049, 4194304, 4194560)] == [0, 0, 1, 1, 2], MOVE_FUSE
    assert SP.fuse_scan_levels(1 << 33) == 2 and SP.fuse_scan_levels(70001) == 1   # two levels at most; test_gpu_fuse.py's largest S
    lo, hi = SP.FUSE_S
    counts = lambda S: 256 * ((S + 255) // 256)                                    # noqa: E731  the [digit][block] table of a pass
    assert (SP.fuse_scan_levels(lo), SP.fuse_scan_levels(counts(lo))) == (1, 1), MOVE_FUSE
    assert (SP.fuse_scan_levels(hi), SP.fuse_scan_levels(counts(hi))) == (2, 2), MOVE_FUSE
    assert lo == SP.FU_TILE ** 2 and (lo + SP.FU_TILE - 1) // SP.FU_TILE == SP.FU_TILE           # a full top tile at one level


def test_the_sources_still_hold_the_constants_of_the_restatement():
    grid, fuse = source("rfgrid.hip"), source("fuse.hip")
    layout = grid[grid.index("void rf_grid_layout("):grid.index("int rf_build_grid(")]
    assert "w.bits = 8;" in layout, "rf_grid_layout no longer starts at w.bits = 8: restate it in size_plan.grid_bits.  " + MOVE_GRID
    m = re.search(r"while \(w\.bits < (\d+) && \(1u << w\.bits\) < (\d+)u \* \(unsigned\)Nt\) \+\+w\.bits;", layout)
    assert m, "rf_grid_layout's loop over w.bits changed: restate it in size_plan.grid_bits.  " + MOVE_GRID
    assert (int(m.group(1)), int(m.group(2))) == (SP.GRID_MAX_BITS, SP.GRID_FILL) == (23, 2), "the cap 23 or the factor 2u * changed.  " + MOVE_GRID
    assert "for (int shift = 0; shift < w.bits; shift += 8)" in grid, "rf_build_grid no longer runs one pass per 8 bits.  " + MOVE_GRID
    assert "constexpr int FU_TILE = 2048;" in fuse, "FU_TILE = 2048 changed: restate it in size_plan.FU_TILE.  " + MOVE_FUSE
    assert "while (n > (size_t)FU_TILE && w.levels < 2)" in fuse, "fu_scan_layout's loop changed: restate it in size_plan.fuse_scan_levels.  " + MOVE_FUSE
    assert "hist = ar.take<int>(256 * (size_t)nblk);" in fuse and "fu_scan_layout(ar, 256 * (size_t)nblk, hs);" in fuse and "fu_scan_layout(ar, (size_t)S, fs);" in fuse, \
        "the arrays yoho_fuse_clouds scans changed.  " + MOVE_FUSE


# ---- the references on the inputs of the GPU file --------------------------------------------------------------------------------------
@pytest.mark.parametrize("Nt,radius", sorted(set(SP.WITHIN + SP.WITHIN_WINDOW)))
def test_nn_within_cases_have_both_kinds_of_query(Nt, radius):
    q, tgt = SP.within_case(Nt)
    assert q.shape == (SP.NQ, 3) and tgt.shape == (Nt, 3) and q.dtype == tgt.dtype == np.float32
    idx, d2 = RR.nn_within_ref(q, tgt, radius)
    has = int((idx >= 0).sum())
    print(f"Nt = {Nt}, radius {radius}: {has} of {SP.NQ} queries have a partner")
    assert has >= 100 and SP.NQ - has >= 100
    if (Nt, radius) in SP.WITHIN_WINDOW:
        assert 0.1 * SP.NQ <= has <= 0.9 * SP.NQ


def test_nn_within_ties_and_clamped_cells_at_three_passes():
    c = SP.ties_case()
    assert c["tgt"].shape == (SP.NT_GRID, 3) and np.array_equal(c["tgt"][:300], c["tgt"][-300:])
    assert np.abs(c["tgt"][300:500, 0]).min() / (SP.TIES_RADIUS * (1 + 2.0 ** -10)) > 2 ** 20      # beyond the cell clamp
    idx, d2 = RR.nn_within_ref(c["q"], c["tgt"], SP.TIES_RADIUS)
    assert (idx[:100] == np.arange(100)).all() and (d2[:100] == 0).all()          # not the copy at 32 469 + i
    far = idx[c["far"]]
    assert (far >= 0).sum() > 50 and (far < 0).sum() > 5 and ((far < 0) | ((far >= 300) & (far < 500))).all()
    assert np.array_equal(idx[c["own"]], c["own_idx"])


def test_clean_references_at_three_passes():
    pts = SP.knn_cloud()
    assert pts.shape == (SP.NT_GRID, 3)
    ref = SP.statistical()
    rc = ref["count"]
    assert (rc == 0).any() and ((0 < rc) & (rc < SP.KNN_K)).any() and (rc == SP.KNN_K).any() and (rc > SP.KNN_K).any()
    assert 0 < ref["n_keep"] < ref["stats"][0] < SP.NT_GRID
    assert CR.assert_away_from_threshold(ref, 1e-9) > 1e-9
    # the k-NN reference itself on a thousand rows: statistical_ref's counts, the row itself skipped
    idx, d2, cnt = CR.knn_within_ref(pts[:1000], pts, SP.KNN_RADIUS, SP.KNN_K)
    assert np.array_equal(cnt - 1, rc[:1000]) and (idx[:, 0] == np.arange(1000)).all() and (d2[:, 0] == 0).all()


def test_normals_reference_at_three_passes():
    ref = SP.surface_normals()
    print(f"surface cloud: mean count {ref['count'].mean():.1f}, {int(ref['valid'].sum())} valid normals of {SP.NT_GRID}")
    assert ref["count"].shape == (SP.NT_GRID,) and 8 <= ref["count"].mean() <= 15
    assert ref["valid"].mean() >= 0.3 and (~ref["valid"]).sum() >= 1


def test_dbscan_reference_at_three_passes():
    ref = SP.dbscan()
    border = int(((ref["core"] == 0) & (ref["labels"] >= 0)).sum())
    print(f"uniform cube: n = {ref['n'].tolist()}, {border} border rows")
    assert ref["labels"].shape == (SP.NT_GRID,) and ref["n"][0] >= 1000 and border >= 5000 and ref["n"][2] >= 5000
    assert ref["n"][1] + border + ref["n"][2] == SP.NT_GRID


@pytest.mark.parametrize("order", SP.CHAIN_ORDERS)
def test_chain_reference_is_the_analytic_answer(order):
    pts, ends = SP.chain(order)
    assert pts.shape == (SP.CHAIN_N, 3) and ends.shape == (2,)
    want = SP.chain_expected(order)
    assert want["n"].tolist() == [1, 65535, 0] and want["sizes"][0] == 65537 and (want["count"] == 2).sum() == 65535
    ref = CL.dbscan_ref(pts, SP.CHAIN_EPS, 3)
    for k in ("labels", "count", "core", "sizes", "n"):
        assert ref[k].dtype == want[k].dtype and np.array_equal(ref[k], want[k]), (order, k)


def test_pair_references_at_three_passes():
    c = SP.pair_case()
    lens = np.diff(c["soff"])
    assert c["tgt"].shape == (SP.NT_GRID, 3) and lens.tolist() == list(SP.EDGE_LENGTHS) and lens[0] == SP.NQ
    n, r, M = SP.edge_info()
    assert ((n > 0.1 * lens) & (n < 0.9 * lens)).all() and np.isfinite(r).all() and (M[:, 0, 0] == n).all()
    en, er, ec = SP.eval_two()
    assert en[0] == n[0] and er[0] == r[0] and en[1] != en[0] and 0.1 * SP.NQ < en[1] < 0.9 * SP.NQ and (ec > 0).all()


def test_icp_steps_at_three_passes():
    c = SP.icp_case()
    assert c["src"].shape == (SP.NQ, 3) and c["tgt"].shape == (SP.NT_GRID, 3)
    n, e, Tn, why, idx = SP.icp_point_step()
    assert Tn is not None and 0.5 * SP.NQ < n < SP.NQ                              # some source points have no partner
    s = SP.icp_plane_step()
    assert s["T"] is not None and PR.MIN_PAIRS <= s["n"] < n and int((s["idx"] >= 0).sum()) == n     # some partners have no normal


@pytest.mark.parametrize("S", SP.FUSE_S)
def test_fuse_references_around_the_second_scan_level(S):
    src, soff, T = SP.fuse_case(S)
    assert src.shape == (S, 3) and soff.tolist() == [0, S // 3, 2 * S // 3, S] and T.shape == (3, 3, 4)
    coarse = SP.fuse_expected(S, 1.0, 1)
    assert coarse["inside"] == S and coarse["M"] > 2048 and coarse["count"].max() > 32
    both = SP.fuse_expected(S, 1.0, 2)
    assert 2048 < both["M"] <= coarse["M"] and (both["nfrag"] >= 2).all() and coarse["nfrag"].max() == 3
    fine = SP.fuse_expected(S, 0.25, 1)
    print(f"S = {S}: voxel 1.0 gives M = {coarse['M']} (two fragments: {both['M']}), largest count {coarse['count'].max()}; voxel 0.25 gives M = {fine['M']}")
    assert fine["M"] > 2048 ** 2 // 2
    # the last point alone lies behind the flags' first 2048 tiles: its voxel must not be its own, or the carry would not matter to row_of
    assert coarse["row_of"][S - 1] >= 0 and fine["row_of"][S - 1] >= 0
    if S == SP.FUSE_S[1]:
        # the [digit][block] table of a pass: only the counts of digit 255 in the last blocks lie behind its first 2048 tiles (entries
        # >= 2048^2).  The first pass sees the points in row order and its digit is the low byte of cx - min cx once x spans 256 cells:
        # at voxel 0.25 some point of those blocks has that digit, so a wrong carry there moves points
        nblk = (S + 255) // 256
        block = SP.FU_TILE ** 2 - 255 * nblk
        assert 0 < block < nblk, MOVE_FUSE
        R = T[np.repeat(np.arange(3), np.diff(soff)), 0]
        s = src.astype(np.float64)
        cx = np.floor((((R[:, 0] * s[:, 0] + R[:, 1] * s[:, 1]) + R[:, 2] * s[:, 2]) + R[:, 3]) * (1.0 / 0.25)).astype(np.int64)
        assert cx.max() - cx.min() >= 255 and (((cx - cx.min()) & 255)[256 * block:] == 255).any(), MOVE_FUSE
