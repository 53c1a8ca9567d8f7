"""The contracts of include/yoho_refine.h on the CPU (helper of tests/test_refine_cpu.py and tests/test_gpu_refine.py, not a conftest).

  nn_within_ref      the nearest target strictly inside the gate, elementwise f32 in the header's order, first minimum
  tree_sum           the header's "THE SUM": the one order in which every f64 sum of the entries is taken
  kabsch_step        the header's "THE KABSCH STEP" in numpy f64 (np.linalg.svd for the 3 x 3)
  refit_ref / icp_ref   the two iterations with their stop rules
  kabsch_exact       the same step with exact sums (integers) and the 3 x 3 decomposition at 80 digits (mpmath), the way
                     oracle/estim_ref.py treats three points: the yardstick of the tolerance
  refit_case / icp_case   the seeded inputs of the tests
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle"))
import estim_ref as ER  # noqa: E402

RANK_TOL = 1e-13
ICP_ITERS, ICP_CONVERGED, ICP_FEW_PAIRS, ICP_RANK = 0, 1, 2, 3
f32, f64 = np.float32, np.float64


# ---- nearest neighbour inside a radius -------------------------------------------------------------------------------------------
def gate2_of(max_dist):
    with np.errstate(over="ignore", under="ignore"):
        return f32(max_dist) * f32(max_dist)


def _d2(q, t):
    """(nq,3) x (nt,3) f32 -> (nq,nt) f32: ((dx^2 + dy^2) + dz^2), every operation rounded to f32"""
    with np.errstate(all="ignore"):
        d = q[:, None, 0] - t[None, :, 0]
        s = d * d
        d = q[:, None, 1] - t[None, :, 1]
        s = s + d * d
        d = q[:, None, 2] - t[None, :, 2]
        return s + d * d


def nn_within_ref(q, tgt, max_dist, chunk=512, prefilter=True):
    """-> (idx (Nq) int64, d2 (Nq) f32): idx -1 / d2 +inf without a candidate.  prefilter: the queries are walked in ascending x, a
    chunk of them only looks at the targets whose x lies within 1.001 max_dist of the chunk's x range - a target outside has
    |dx| > 1.001 max_dist for every query of the chunk, hence d2 >= fl(fl(dx)^2) > gate2: never a candidate.  The targets kept
    stay in ascending index order, so the first minimum is the lowest index.  tests/test_refine_cpu.py holds it against the plain
    all-pairs form."""
    q, tgt = np.ascontiguousarray(q, f32).reshape(-1, 3), np.ascontiguousarray(tgt, f32).reshape(-1, 3)
    g2 = gate2_of(max_dist)
    nq = q.shape[0]
    idx = np.full((nq,), -1, np.int64)
    d2o = np.full((nq,), np.inf, f32)
    fin = np.isfinite(q).all(axis=1)                  # a NaN / inf query has no finite d2
    rows = np.nonzero(fin)[0]
    prefilter = prefilter and 1e-15 < float(max_dist) < 1e15
    if prefilter:
        rows = rows[np.argsort(q[rows, 0], kind="stable")]
        tx = tgt[:, 0].astype(f64)
        order = np.argsort(tx, kind="stable")         # NaN last
        txs = tx[order]
        reach = float(max_dist) * 1.001
    for s in range(0, rows.shape[0], chunk):
        r = rows[s:s + chunk]
        if prefilter:
            lo = np.searchsorted(txs, float(q[r, 0].min()) - reach, side="left")
            hi = np.searchsorted(txs, float(q[r, 0].max()) + reach, side="right")
            cand = np.sort(order[lo:hi])
            if cand.size == 0:
                continue
        else:
            cand = np.arange(tgt.shape[0])
        d = _d2(q[r], tgt[cand])
        with np.errstate(invalid="ignore"):
            d = np.where(d < g2, d, f32(np.inf))
        j = np.argmin(d, axis=1)
        best = d[np.arange(r.shape[0]), j]
        ok = best < np.inf
        idx[r[ok]] = cand[j[ok]]
        d2o[r[ok]] = best[ok]
    return idx, d2o


# ---- the sum and the Kabsch step ----------------------------------------------------------------------------------------------------
def tree_sum(v):
    """v (N,) or (N,K) f64 -> () or (K,): runs of 64 by halving, the four runs of a 256-block in order, the blocks in order"""
    v = np.asarray(v, f64)
    one = v.ndim == 1
    v = v.reshape(v.shape[0], int(np.prod(v.shape[1:])))
    n, K = v.shape
    nb = max(1, (n + 255) // 256)
    x = np.zeros((nb * 256, K), f64)
    x[:n] = v
    x = x.reshape(nb, 4, 64, K)
    for o in (32, 16, 8, 4, 2, 1):
        x = x[:, :, :o] + x[:, :, o:2 * o]
    x = x[:, :, 0]
    b = ((x[:, 0] + x[:, 1]) + x[:, 2]) + x[:, 3]
    s = np.zeros((K,), f64)
    for i in range(nb):
        s = s + b[i]
    return s[0] if one else s


def rotation_of(H):
    """H = U S V^T -> R = V diag(1, 1, det(V U^T)) U^T, or None when the rank is below 2 (s1 = 0 or s2 <= 1e-13 s1)"""
    U, S, Vt = np.linalg.svd(H)
    if not (S[0] > 0.0) or not (S[1] > RANK_TOL * S[0]):
        return None
    d = 1.0 if np.linalg.det(Vt.T @ U.T) > 0 else -1.0
    return Vt.T @ np.diag([1.0, 1.0, d]) @ U.T


def kabsch_step(a, b, sel):
    """a (N,3) fragment 0's side, b (N,3) fragment 1's, sel (N,) bool -> T (3,4) or None (rank below 2); rows outside sel may hold
    anything finite"""
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    m = sel[:, None]
    n = int(sel.sum())
    c0 = tree_sum(np.where(m, a, 0.0)) / f64(n)
    c1 = tree_sum(np.where(m, b, 0.0)) / f64(n)
    ac, bc = a - c0, b - c1
    prod = (bc[:, :, None] * ac[:, None, :]).reshape(-1, 9)
    H = tree_sum(np.where(m, prod, 0.0)).reshape(3, 3)
    R = rotation_of(H)
    if R is None:
        return None
    t = c0 - ((R[:, 0] * c1[0] + R[:, 1] * c1[1]) + R[:, 2] * c1[2])
    return np.concatenate([R, t[:, None]], axis=1)


def kabsch_exact(a, b):
    """the Kabsch step over ALL rows of a, b (N,3) f64 with exact sums and an 80-digit decomposition -> T (3,4) rounded once to f64.
    With A, B the coordinates as integers over a common power of two: n a - SUM a and n b - SUM b are integers, so is n^2 H."""
    import mpmath as mp
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    n = a.shape[0]
    A, Ea = ER._scaled(a)
    B, Eb = ER._scaled(b)
    sa, sb = A.sum(axis=0), B.sum(axis=0)
    ac, bc = A * n - sa, B * n - sb
    Hn = [[int((bc[:, i] * ac[:, j]).sum()) for j in range(3)] for i in range(3)]
    with mp.workdps(ER.DPS):
        scale = mp.mpf(n) ** 2 * mp.mpf(2) ** (Ea + Eb)
        H = mp.matrix([[mp.mpf(Hn[i][j]) / scale for j in range(3)] for i in range(3)])
        U, S, Vt = mp.svd_r(H)
        o = sorted(range(3), key=lambda k: -S[k])
        u1, u2 = [U[r, o[0]] for r in range(3)], [U[r, o[1]] for r in range(3)]
        v1, v2 = [Vt[o[0], r] for r in range(3)], [Vt[o[1], r] for r in range(3)]
        cr = lambda x, y: [x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]]
        u3, v3 = cr(u1, u2), cr(v1, v2)         # (v1 x v2)(u1 x u2)^T = det(V U^T) v3 u3^T: the determinant fix
        R = [[v1[i] * u1[j] + v2[i] * u2[j] + v3[i] * u3[j] for j in range(3)] for i in range(3)]
        c0 = [mp.mpf(int(sa[j])) / (n * mp.mpf(2) ** Ea) for j in range(3)]
        c1 = [mp.mpf(int(sb[j])) / (n * mp.mpf(2) ** Eb) for j in range(3)]
        t = [c0[i] - sum(R[i][j] * c1[j] for j in range(3)) for i in range(3)]
        return np.array([[float(R[i][0]), float(R[i][1]), float(R[i][2]), float(t[i])] for i in range(3)])


def device_tolerance(T_numpy, T_exact, coords):
    """the bound of the issue: the larger of 8 x numpy-f64's own worst entry error against the exact answer and 4 ulp of the largest
    coordinate magnitude -> (bound, numpy's error, the 4-ulp floor)"""
    err = float(np.abs(np.asarray(T_numpy) - np.asarray(T_exact)).max())
    floor = 4.0 * float(np.spacing(f64(max(np.abs(c).max() for c in coords))))
    return max(8.0 * err, floor), err, floor


# ---- refit -------------------------------------------------------------------------------------------------------------------------
def residual2(T, k0, k1):
    r = k0 - (k1 @ T[:, :3].T + T[:, 3])
    return np.sum(r * r, axis=1)


def refit_ref(k0, k1, T_in, inlier_dist, iters):
    """-> dict(T (list of the iterates evaluated), counts (iters + 1, -1 behind the last), best, evaluated, T_out, masks, margin =
    the smallest |residual^2 - d^2| / d^2 over all evaluated iterates and matches)"""
    k0, k1 = np.asarray(k0, f64).reshape(-1, 3), np.asarray(k1, f64).reshape(-1, 3)
    d2 = f64(inlier_dist) * f64(inlier_dist)
    Ts, masks = [np.array(T_in, f64).reshape(3, 4)], []
    counts = np.full((iters + 1,), -1, np.int32)
    margin, best, best_count = np.inf, 0, -1
    for i in range(iters + 1):
        s = residual2(Ts[i], k0, k1)
        sel = s < d2
        if s.size and d2 > 0:
            margin = min(margin, float(np.abs(s - d2).min() / d2))
        masks.append(sel)
        counts[i] = n = int(sel.sum())
        if n > best_count:
            best, best_count = i, n
        if i == iters or n < 3 or (i > 0 and np.array_equal(sel, masks[i - 1])):
            break
        T = kabsch_step(k0, k1, sel)
        if T is None:
            break
        Ts.append(T)
    return {"T": Ts, "counts": counts, "best": best, "evaluated": len(masks), "T_out": Ts[best], "masks": masks, "margin": margin}


# ---- ICP -----------------------------------------------------------------------------------------------------------------------------
def transform_f32(T, src):
    """q = (float)(((r0 sx + r1 sy) + r2 sz) + t) per coordinate, in f64"""
    s = np.asarray(src, f32).astype(f64)
    T = np.asarray(T, f64)
    return np.stack([((T[i, 0] * s[:, 0] + T[i, 1] * s[:, 1]) + T[i, 2] * s[:, 2]) + T[i, 3] for i in range(3)], axis=1).astype(f32)


def icp_step(src, tgt, T, max_dist):
    """one iteration from T -> (n, rmse, T_next or None, why None: ICP_FEW_PAIRS / ICP_RANK)"""
    src, tgt = np.ascontiguousarray(src, f32), np.ascontiguousarray(tgt, f32)
    idx, d2 = nn_within_ref(transform_f32(T, src), tgt, max_dist)
    sel = idx >= 0
    n = int(sel.sum())
    rmse = np.sqrt(tree_sum(np.where(sel, d2.astype(f64), 0.0)) / f64(n)) if n else f64(np.inf)
    if n < 3:
        return n, rmse, None, ICP_FEW_PAIRS, idx
    Tn = kabsch_step(tgt[np.maximum(idx, 0)].astype(f64), src.astype(f64), sel)
    return n, rmse, Tn, (ICP_RANK if Tn is None else None), idx


def icp_ref(src, tgt, T_in, max_dist, iters, tol):
    """-> dict(T (the transform in front of every iteration made, then T_out last), npairs / rmse (iters, -1 behind the last), done, reason, T_out)"""
    T = np.array(T_in, f64).reshape(3, 4)
    Ts = [T]
    npairs, rmse = np.full((iters,), -1, np.int32), np.full((iters,), -1.0, f64)
    done, reason = 0, ICP_ITERS
    for i in range(iters):
        n, e, Tn, why, _ = icp_step(src, tgt, T, max_dist)
        npairs[i], rmse[i], done = n, e, i + 1
        if Tn is None:
            reason = why
            break
        delta = float(np.abs(Tn - T).max())
        T = Tn
        Ts.append(T)
        if delta <= tol:
            reason = ICP_CONVERGED
            break
    return {"T": Ts, "npairs": npairs, "rmse": rmse, "done": done, "reason": reason, "T_out": T}


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def rot_axis_angle(axis, deg):
    a = np.asarray(axis, f64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def rot_error_deg(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1.0) / 2.0
    return float(np.rad2deg(np.arccos(np.clip(c, -1.0, 1.0))))


def perturbed(T_gt, rs, deg, shift):
    """T_gt with its rotation turned by `deg` about a random axis and its translation moved by `shift` in a random direction"""
    R = rot_axis_angle(rs.randn(3), deg) @ T_gt[:, :3]
    d = rs.randn(3)
    return np.concatenate([R, (T_gt[:, 3] + shift * d / np.linalg.norm(d))[:, None]], axis=1)


def refit_case(seed, M=1500, inlier_share=0.3, noise=0.01):
    """matched keypoints of a pair: k0 = R k1 + t + 1 cm noise for 30 % of the matches, unrelated points for the rest, and a start
    4 degrees / 4.7 cm off -> dict(k0, k1, T_gt, T0, inlier_dist)"""
    rs = np.random.RandomState(1000 + seed)
    T_gt = np.concatenate([rot_axis_angle(rs.randn(3), 20.0 + 100.0 * rs.rand()), (rs.rand(3, 1) - 0.5) * 2.0], axis=1)
    k1 = (rs.rand(M, 3) - 0.5) * 3.0
    k0 = k1 @ T_gt[:, :3].T + T_gt[:, 3] + noise * rs.randn(M, 3)
    out = rs.permutation(M)[int(round(inlier_share * M)):]
    k0[out] = (rs.rand(out.size, 3) - 0.5) * 3.0
    return {"k0": np.ascontiguousarray(k0), "k1": np.ascontiguousarray(k1), "T_gt": T_gt, "T0": perturbed(T_gt, rs, 4.0, 0.047), "inlier_dist": 0.09}


def icp_case(n=20000, seed=3, deg=2.0, shift=0.045, overlap=1.0):
    """an n-point synth.surface_cloud seen from two poses: tgt = the cloud, src = the same points moved by the inverse of a known
    transform (both rounded to f32), and a start `deg` degrees / `shift` metres off -> dict(src, tgt (f32), T_gt, T0, max_dist).
    Both sides hold the same surface points, so the ground truth is a fixed point of the iteration and the bound of 0.01 degrees can
    be met: two INDEPENDENT samplings of the surface (the halves of a 40 000-point cloud) were tried and stop at their sampling
    floor, 0.056 degrees after 60 iterations, whatever runs them (icp_halves_case: held in lock-step without that bound).  overlap < 1: tgt keeps the points with x below that quantile and
    src those above 1 - it, so that part of either side has no partner."""
    from yoho_amd import synth
    rs = np.random.RandomState(2000 + seed)
    pc = synth.surface_cloud(n, seed=seed)
    T_gt = np.concatenate([rot_axis_angle(rs.randn(3), 35.0), np.array([[0.3], [-0.2], [0.5]])], axis=1)
    keep_t = keep_s = np.ones((n,), bool)
    if overlap < 1.0:
        keep_t = pc[:, 0] < np.quantile(pc[:, 0], overlap)
        keep_s = pc[:, 0] > np.quantile(pc[:, 0], 1.0 - overlap)
    src = (pc[keep_s] - T_gt[:, 3]) @ T_gt[:, :3]       # R^T (p - t): T_gt maps it back onto the surface
    return {"src": np.ascontiguousarray(src, f32), "tgt": np.ascontiguousarray(pc[keep_t], f32), "T_gt": T_gt, "T0": perturbed(T_gt, rs, deg, shift),
            "max_dist": 0.1}


def noisy_small_case(seed, M=40, noise=0.06, inlier_dist=0.1):
    """a few matches whose noise is comparable to the threshold: the inlier set keeps changing and a later iterate can hold FEWER inliers
    than an earlier one (seeds 1, 5, 11, 9 do: counts [24, 23, 23], [17, 20, 19, 19], [19, 23, 22, 23, 23], [24, 25, 26, 24, 26, 26, 26]) ->
    refit_case's dict"""
    rs = np.random.RandomState(seed)
    T = np.concatenate([rot_axis_angle(rs.randn(3), 30.0), rs.rand(3, 1)], axis=1)
    k1 = rs.rand(M, 3) - 0.5
    k0 = k1 @ T[:, :3].T + T[:, 3] + noise * rs.randn(M, 3)
    return {"k0": np.ascontiguousarray(k0), "k1": np.ascontiguousarray(k1), "T_gt": T, "T0": perturbed(T, rs, 3.0, 0.03), "inlier_dist": inlier_dist}


def icp_halves_case(n=20000, seed=3, deg=2.0, shift=0.045):
    """two INDEPENDENT n-point samplings of one synth.surface_cloud surface (the halves of a 2n-point cloud, which is shuffled), the
    source moved by the inverse of a known transform: no point has an exact partner, the correspondences stay non-trivial at
    convergence and the pair count varies -> icp_case's dict.  The iteration stops at the sampling floor (0.056 degrees), so no bound
    on the distance to the ground truth goes with this pair."""
    from yoho_amd import synth
    rs = np.random.RandomState(2000 + seed)
    pc = synth.surface_cloud(2 * n, seed=seed)
    T_gt = np.concatenate([rot_axis_angle(rs.randn(3), 35.0), np.array([[0.3], [-0.2], [0.5]])], axis=1)
    src = (pc[n:] - T_gt[:, 3]) @ T_gt[:, :3]
    return {"src": np.ascontiguousarray(src, f32), "tgt": np.ascontiguousarray(pc[:n], f32), "T_gt": T_gt, "T0": perturbed(T_gt, rs, deg, shift),
            "max_dist": 0.1}
