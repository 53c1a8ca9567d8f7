"""The contracts of include/yoho_verify.h on the CPU (helper of tests/test_verify_cpu.py and tests/test_gpu_verify.py, not a conftest).

  eval_ref      K transforms evaluated on two clouds: pairs inside the gate, rmse, truncated cost - on refine_ref's transform_f32,
                nn_within_ref, tree_sum and gate2_of, so rmse and cost are the header's bits
  top_ref       the greedy selection: largest count, lowest position among equal counts, near-duplicates suppressed
  verify_ref    selection + evaluation + pick
  decoy_case    the seeded pair on which the vote picks a decoy cluster and the truncated cost does not
"""
import numpy as np

import refine_ref as RR

f32, f64 = np.float32, np.float64
IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)


def eval_ref(src, tgt, T, max_dist):
    """src (Ns,3), tgt (Nt,3) f32, T (K,3,4) f64 -> (npairs (K) int32, rmse (K) f64, cost (K) f64)"""
    src, tgt = np.ascontiguousarray(src, f32).reshape(-1, 3), np.ascontiguousarray(tgt, f32).reshape(-1, 3)
    T = np.asarray(T, f64).reshape(-1, 3, 4)
    K = T.shape[0]
    g2 = f64(RR.gate2_of(max_dist))
    npairs, rmse, cost = np.zeros((K,), np.int32), np.zeros((K,), f64), np.zeros((K,), f64)
    for k in range(K):
        with np.errstate(all="ignore"):
            q = RR.transform_f32(T[k], src)
        idx, d2 = RR.nn_within_ref(q, tgt, max_dist)
        sel = idx >= 0
        n = int(sel.sum())
        d = np.where(sel, d2, f32(0)).astype(f64)
        npairs[k] = n
        rmse[k] = np.sqrt(RR.tree_sum(d) / f64(n)) if n else f64(np.inf)
        cost[k] = RR.tree_sum(np.where(sel, d, g2))
    return npairs, rmse, cost


def rows_of(T, order, H):
    """the hypotheses the H positions stand for, (H,3,4)"""
    T = np.asarray(T, f64).reshape(-1, 3, 4)
    return T[:H] if order is None else T[np.asarray(order, np.int64)[:H]]


def top_ref(T, order, counts, K, min_count=1, distinct_tol=0.0):
    """-> the positions taken, in the order taken (a list of at most K)"""
    counts = np.asarray(counts, np.int64)
    H = counts.shape[0]
    rows = rows_of(T, order, H).reshape(H, 12)
    alive = counts >= min_count
    top = []
    for _ in range(K):
        if not alive.any():
            break
        h = int(np.argmax(np.where(alive, counts, -1)))       # first maximum: the lowest position among equal counts
        top.append(h)
        alive[h] = False
        if distinct_tol > 0:
            with np.errstate(invalid="ignore"):
                close = (np.abs(rows - rows[h]) < distinct_tol).all(axis=1)       # a NaN difference is not less
            alive &= ~close
    return top


def verify_ref(src, tgt, T, order, counts, K, max_dist, min_count=1, distinct_tol=0.0, evaluate=None):
    """-> dict(T_out (3,4), top / npairs (K) int32, rmse / cost (K) f64, info (4) int32, Kc, best).  evaluate: rows (n,3,4) ->
    eval_ref(src, tgt, rows, max_dist)'s tuple, for a caller that has those answers already (a row's figures depend on that row alone)"""
    counts = np.asarray(counts, np.int32)
    H = counts.shape[0]
    sel = top_ref(T, order, counts, K, min_count, distinct_tol)
    Kc = len(sel)
    top, npairs = np.full((K,), -1, np.int32), np.full((K,), -1, np.int32)
    rmse, cost = np.full((K,), -1.0, f64), np.full((K,), -1.0, f64)
    out = {"Kc": Kc, "best": -1, "T_out": IDENTITY.copy(), "info": np.array([0, -1, -1, 0], np.int32)}
    if Kc:
        rows = rows_of(T, order, H)[sel]
        top[:Kc] = sel
        npairs[:Kc], rmse[:Kc], cost[:Kc] = eval_ref(src, tgt, rows, max_dist) if evaluate is None else evaluate(rows)
        best = 0
        for i in range(1, Kc):
            if cost[i] < cost[best]:
                best = i
        out.update(best=best, T_out=rows[best].copy(), info=np.array([Kc, best, sel[best], counts[sel[best]]], np.int32))
    out.update(top=top, npairs=npairs, rmse=rmse, cost=cost)
    return out


def o_counts(T, k0, k1, inlier_dist):
    """the vote's inlier counts of the hypotheses T (H,3,4) over the matches (k0, k1), refine_ref.residual2's predicate"""
    d2 = f64(inlier_dist) * f64(inlier_dist)
    return np.array([int((RR.residual2(t, k0, k1) < d2).sum()) for t in np.asarray(T, f64).reshape(-1, 3, 4)], np.int32)


_DECOY = {}


def decoy_case(seed):
    """a 900-point pair with 60 % overlap and 200 matches, one hypothesis per match: 12 matches and hypotheses about the ground truth,
    14 about a decoy 60 degrees / 0.2 m away, the rest anywhere; counts at inlier distance 0.09 in a random vote order; gate 0.05 ->
    dict(src, tgt (f32), T (200,3,4), order (200) int64, counts (200) int32 by position, T_gt, T_d, max_dist, inlier_dist).  Computed
    once per seed and shared: the callers do not modify it."""
    if seed in _DECOY:
        return _DECOY[seed]
    c = RR.icp_case(n=1500, seed=seed, overlap=0.6)
    rs = np.random.RandomState(50 + seed)
    T_gt = c["T_gt"]
    T_d = RR.perturbed(T_gt, rs, 60, 0.2)
    M = 200
    src64 = c["src"].astype(f64)
    k1 = src64[rs.permutation(src64.shape[0])[:M]]
    k0 = (rs.rand(M, 3) - 0.5) * 3.0                       # refine_ref.refit_case's cube
    k0[:12] = k1[:12] @ T_gt[:, :3].T + T_gt[:, 3] + 0.01 * rs.randn(12, 3)
    k0[12:26] = k1[12:26] @ T_d[:, :3].T + T_d[:, 3] + 0.01 * rs.randn(14, 3)
    T = np.empty((M, 3, 4), f64)
    for m in range(M):
        if m < 12:
            T[m] = RR.perturbed(T_gt, rs, 0.5, 0.005)
        elif m < 26:
            T[m] = RR.perturbed(T_d, rs, 0.5, 0.005)
        else:
            T[m] = RR.perturbed(T_gt, rs, 180 * rs.rand(), 1.0)
    order = rs.permutation(M).astype(np.int64)
    counts = o_counts(T[order], k0, k1, 0.09)
    _DECOY[seed] = {"src": c["src"], "tgt": c["tgt"], "T": T, "order": order, "counts": counts, "T_gt": T_gt, "T_d": T_d, "k0": k0, "k1": k1,
                    "max_dist": 0.05, "inlier_dist": 0.09}
    return _DECOY[seed]
