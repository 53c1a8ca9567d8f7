"""The contracts of include/yoho_plane.h on the CPU (helper of tests/test_plane_cpu.py and tests/test_gpu_plane.py, not a conftest).

  normals_ref        brute-force f32 neighbour predicate, one-pass f64 covariance about the point, np.linalg.eigh, the orientation and
                     the invalid rule
  normal_exact       the same covariance and its eigenvectors at 80 digits (mpmath) for one point
  plane_step         one iteration of yoho_icp_plane in numpy f64 with refine_ref's tree_sum / nn_within_ref / the rounded transform
  plane_step_exact   the same 28 sums, the 6 x 6 solve and the exponential at 80 digits: the yardstick of the tolerance
  icp_plane_ref      the loop with its stop rules
  plane_pair         the seeded inputs: refine_ref's two pairs with the target's normals
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_ref as RR  # noqa: E402

f32, f64 = np.float32, np.float64
MIN_PAIRS = 6
PIVOT_TOL = 1e-13
COLLINEAR_TOL = 1e-12
BAND = 1e-9                                  # |l2 / l3 - 1e-12| within 1e-9 relative: either side of the invalid rule
DPS = 80
ROUND32 = float(np.sqrt(3.0) * 2.0 ** -25)   # a unit vector rounded to f32: half an ulp (2^-25 below 1) on each of three components


# ---- normals -------------------------------------------------------------------------------------------------------------------------
def neighbour_mask(p, cand, gate2):
    """p (m,3), cand (k,3) f32 -> (m,k) bool: d2 < gate2 with yoho_nn_within's arithmetic (false for a NaN / inf on either side)"""
    with np.errstate(invalid="ignore"):
        return RR._d2(p, cand) < gate2


def orient(n, p, view):
    """n (N,3) f64 unit, p (N,3) f32, view (3) -> n turned so that n . (v - p) >= 0, at 0 the first non-zero component positive"""
    v = np.asarray(view, f32).astype(f64)
    p = p.astype(f64)
    with np.errstate(invalid="ignore"):
        dot = (n[:, 0] * (v[0] - p[:, 0]) + n[:, 1] * (v[1] - p[:, 1])) + n[:, 2] * (v[2] - p[:, 2])
    first = np.where(n[:, 0] != 0, n[:, 0], np.where(n[:, 1] != 0, n[:, 1], n[:, 2]))
    flip = (dot < 0) | ((dot == 0) & (first < 0))
    return np.where(flip[:, None], -n, n)


def normals_ref(pts, radius, min_nbrs=6, view=(0.0, 0.0, 0.0), chunk=256):
    """-> dict(normals (N,3) f32, n64 (N,3) f64 the same before rounding, count (N) int32, curv (N) f32, valid (N) bool, lam (N,3) f64
    ascending, ratio (N) l2 / l3 (nan where l3 is not > 0)).  The rows are walked in ascending x and a chunk looks at the points whose x
    lies within 1.001 radius of its range only (nn_within_ref's prefilter: a point outside is nobody's neighbour there)."""
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    N = pts.shape[0]
    g2 = RR.gate2_of(radius)
    count = np.zeros((N,), np.int32)
    C = np.zeros((N, 3, 3), f64)
    fin = np.isfinite(pts).all(axis=1)
    rows = np.nonzero(fin)[0]
    pre = 1e-15 < float(radius) < 1e15
    if pre:
        rows = rows[np.argsort(pts[rows, 0], kind="stable")]
        xs = pts[rows, 0].astype(f64)
        reach = float(radius) * 1.001
    for s in range(0, rows.shape[0], chunk):
        r = rows[s:s + chunk]
        cand = rows
        if pre:
            lo = np.searchsorted(xs, float(pts[r, 0].min()) - reach, side="left")
            hi = np.searchsorted(xs, float(pts[r, 0].max()) + reach, side="right")
            cand = rows[lo:hi]
        m = neighbour_mask(pts[r], pts[cand], g2)
        d = np.where(m[:, :, None], pts[cand].astype(f64)[None, :, :] - pts[r].astype(f64)[:, None, :], 0.0)
        n = m.sum(axis=1)
        S1 = d.sum(axis=1)
        S2 = np.einsum("mki,mkj->mij", d, d)
        count[r] = n
        with np.errstate(invalid="ignore", divide="ignore"):
            C[r] = np.where((n > 0)[:, None, None], S2 - S1[:, :, None] * S1[:, None, :] / np.maximum(n, 1)[:, None, None], 0.0)
    lam, V = np.linalg.eigh(C)
    l1, l2, l3 = lam[:, 0], lam[:, 1], lam[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(l3 > 0, l2 / np.where(l3 > 0, l3, 1.0), np.nan)
        valid = (count >= min_nbrs) & (l3 > 0) & (l2 > COLLINEAR_TOL * l3)
        curv = np.where(valid, l1 / np.where(valid, (l1 + l2) + l3, 1.0), -1.0).astype(f32)
    n64 = V[:, :, 0] / np.linalg.norm(V[:, :, 0], axis=1, keepdims=True)
    n64 = np.where(valid[:, None], orient(n64, pts, view), 0.0)
    return {"normals": n64.astype(f32), "n64": n64, "count": count, "curv": curv, "valid": valid, "lam": lam, "ratio": ratio}


def normal_exact(pts, i, radius):
    """point i's covariance and eigenvectors at 80 digits -> dict(n: mp column (the unit eigenvector of l1, sign open), lam (3 mp,
    ascending), count, relgap = (l2 - l1) / l3 as float)"""
    import mpmath as mp
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    m = neighbour_mask(pts[i:i + 1], pts, RR.gate2_of(radius))[0]
    nb = pts[m].astype(f64)
    with mp.workdps(DPS):
        p = [mp.mpf(float(x)) for x in pts[i].astype(f64)]
        d = [[mp.mpf(float(x)) - p[k] for k, x in enumerate(row)] for row in nb]
        n = len(d)
        S1 = [mp.fsum(r[k] for r in d) for k in range(3)]
        C = mp.matrix(3, 3)
        for a in range(3):
            for b in range(3):
                C[a, b] = mp.fdot([r[a] for r in d], [r[b] for r in d]) - S1[a] * S1[b] / n
        E, Q = mp.eigsy(C)
        o = sorted(range(3), key=lambda k: E[k])
        lam = [E[k] for k in o]
        v = [Q[r, o[0]] for r in range(3)]
        ln = mp.sqrt(sum(x * x for x in v))
        return {"n": [x / ln for x in v], "lam": lam, "count": n, "relgap": float((lam[1] - lam[0]) / lam[2]) if lam[2] > 0 else 0.0}


def angle_to_exact(n, exact):
    """the angle between a normal (3 floats, either sign) and normal_exact's, taken at 80 digits -> float (radians)"""
    import mpmath as mp
    with mp.workdps(DPS):
        a = [mp.mpf(float(x)) for x in n]
        e = exact["n"]
        cr = [a[1] * e[2] - a[2] * e[1], a[2] * e[0] - a[0] * e[2], a[0] * e[1] - a[1] * e[0]]
        dot = abs(sum(x * y for x, y in zip(a, e)))
        return float(mp.atan2(mp.sqrt(sum(x * x for x in cr)), dot))


def angle_between(a, b):
    """a, b (N,3) -> (N) angles in radians, the sign of either vector ignored, accurate for small angles"""
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs((a * b).sum(axis=1)))


def normal_bound(numpy_worst, count, relgap):
    """the bound of the issue on the angle of a device normal to the exact one: the larger of 8 x numpy's own worst angle and the
    Davis-Kahan figure 4 n 2^-53 / relgap of an n-term f64 sum, plus the rounding of the output to f32"""
    dk = 4.0 * count * 2.0 ** -53 / relgap if relgap > 0 else np.inf          # l1 = l2: the normal is open
    return max(8.0 * numpy_worst, dk) + ROUND32


# ---- one iteration ---------------------------------------------------------------------------------------------------------------------
def transform_f64(T, src):
    """x = ((r0 sx + r1 sy) + r2 sz) + t per coordinate, in f64, every operation rounded"""
    s = np.asarray(src, f32).astype(f64)
    T = np.asarray(T, f64)
    return np.stack([((T[i, 0] * s[:, 0] + T[i, 1] * s[:, 1]) + T[i, 2] * s[:, 2]) + T[i, 3] for i in range(3)], axis=1)


def pairs_of(src, tgt, normals, T, max_dist):
    """-> (x (Ns,3) f64, idx (Ns) int64 yoho_nn_within's answer, kept (Ns) bool)"""
    x = transform_f64(T, src)
    idx, _ = RR.nn_within_ref(RR.transform_f32(T, src), tgt, max_dist)          # q = (float)x
    nr = np.asarray(normals, f32)[np.maximum(idx, 0)]
    kept = (idx >= 0) & np.isfinite(nr).all(axis=1) & (nr != 0).any(axis=1)
    return x, idx, kept


def cholesky_solve6(A, b):
    """A z = -b by an unpivoted Cholesky decomposition -> z, or None when a pivot d_k is not > 1e-13 A_kk"""
    L = np.zeros((6, 6), f64)
    for k in range(6):
        d = A[k, k]
        for q in range(k):
            d = d - L[k, q] * L[k, q]
        if not (d > PIVOT_TOL * A[k, k]):
            return None
        L[k, k] = np.sqrt(d)
        for i in range(k + 1, 6):
            s = A[i, k]
            for q in range(k):
                s = s - L[i, q] * L[k, q]
            L[i, k] = s / L[k, k]
    y = np.zeros(6, f64)
    for k in range(6):
        s = -b[k]
        for q in range(k):
            s = s - L[k, q] * y[q]
        y[k] = s / L[k, k]
    z = np.zeros(6, f64)
    for k in range(5, -1, -1):
        s = y[k]
        for q in range(k + 1, 6):
            s = s - L[q, k] * z[q]
        z[k] = s / L[k, k]
    return z


def exp_so3(w):
    """exp([w]x) by Rodrigues, a series below |w|^2 = 1e-4"""
    w = np.asarray(w, f64)
    t2 = float(w @ w)
    if t2 < 1e-4:
        a = 1.0 - t2 / 6.0 * (1.0 - t2 / 20.0 * (1.0 - t2 / 42.0))
        b = 0.5 - t2 / 24.0 * (1.0 - t2 / 30.0 * (1.0 - t2 / 56.0))
    else:
        th = np.sqrt(t2)
        h = np.sin(0.5 * th) / (0.5 * th)
        a, b = np.sin(th) / th, 0.5 * h * h
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], f64)
    return np.eye(3) + a * K + b * (np.outer(w, w) - t2 * np.eye(3))


def plane_step(src, tgt, normals, T, max_dist):
    """one iteration from T -> dict(n, rmse, T (3,4) or None, why (None / ICP_FEW_PAIRS / ICP_RANK), x, idx, kept, A, b, cond = the
    reciprocal condition number of A)"""
    src, tgt, normals = np.ascontiguousarray(src, f32), np.ascontiguousarray(tgt, f32), np.ascontiguousarray(normals, f32)
    T = np.asarray(T, f64).reshape(3, 4)
    x, idx, kept = pairs_of(src, tgt, normals, T, max_dist)
    n = int(kept.sum())
    out = {"n": n, "x": x, "idx": idx, "kept": kept, "T": None, "why": None, "cond": 0.0}
    m = kept[:, None]
    c = RR.tree_sum(np.where(m, x, 0.0)) / f64(n) if n else np.zeros(3)
    j = np.maximum(idx, 0)
    nr, p = normals[j].astype(f64), tgt[j].astype(f64)
    with np.errstate(invalid="ignore", over="ignore"):
        u = x - c
        r = ((nr[:, 0] * (x[:, 0] - p[:, 0])) + nr[:, 1] * (x[:, 1] - p[:, 1])) + nr[:, 2] * (x[:, 2] - p[:, 2])
        a = np.stack([u[:, 1] * nr[:, 2] - u[:, 2] * nr[:, 1], u[:, 2] * nr[:, 0] - u[:, 0] * nr[:, 2], u[:, 0] * nr[:, 1] - u[:, 1] * nr[:, 0]], axis=1)
        J = np.concatenate([a, nr], axis=1)
        cols = [J[:, k] * J[:, l] for k in range(6) for l in range(k, 6)] + [J[:, k] * r for k in range(6)] + [r * r]
    S = RR.tree_sum(np.where(m, np.stack(cols, axis=1), 0.0))
    out["rmse"] = np.sqrt(S[27] / f64(n)) if n else f64(np.inf)
    if n < MIN_PAIRS:
        out["why"] = RR.ICP_FEW_PAIRS
        return out
    A = np.zeros((6, 6), f64)
    q = 0
    for k in range(6):
        for l in range(k, 6):
            A[k, l] = A[l, k] = S[q]
            q += 1
    b = S[21:27]
    out.update(A=A, b=b, c=c)
    z = cholesky_solve6(A, b)
    if z is None:
        out["why"] = RR.ICP_RANK
        return out
    out["cond"] = float(1.0 / np.linalg.cond(A))
    dR = exp_so3(z[:3])
    R, t = T[:, :3], T[:, 3]
    d = t - c
    Rn = np.stack([(dR[:, 0] * R[0, jj] + dR[:, 1] * R[1, jj]) + dR[:, 2] * R[2, jj] for jj in range(3)], axis=1)
    tn = (((dR[:, 0] * d[0] + dR[:, 1] * d[1]) + dR[:, 2] * d[2]) + c) + z[3:]
    out["T"] = np.concatenate([Rn, tn[:, None]], axis=1)
    return out


def plane_step_exact(tgt, normals, T, step):
    """the step over plane_step's own pairs (its x, the rounded transform of the contract, its idx / kept) with the centroid, the 28
    sums, the 6 x 6 solve and the exponential at 80 digits -> T_next (3,4) rounded once to f64"""
    import mpmath as mp
    tgt, normals = np.ascontiguousarray(tgt, f32), np.ascontiguousarray(normals, f32)
    T = np.asarray(T, f64).reshape(3, 4)
    sel = np.nonzero(step["kept"])[0]
    j = step["idx"][sel]
    with mp.workdps(DPS):
        col = lambda arr, k: [mp.mpf(float(v)) for v in arr[:, k]]
        X = [col(step["x"][sel], k) for k in range(3)]
        P = [col(tgt[j].astype(f64), k) for k in range(3)]
        Nn = [col(normals[j].astype(f64), k) for k in range(3)]
        n = len(sel)
        c = [mp.fsum(X[k]) / n for k in range(3)]
        U = [[v - c[k] for v in X[k]] for k in range(3)]
        r = [Nn[0][e] * (X[0][e] - P[0][e]) + Nn[1][e] * (X[1][e] - P[1][e]) + Nn[2][e] * (X[2][e] - P[2][e]) for e in range(n)]
        cross = lambda a, b: [U[a][e] * Nn[b][e] - U[b][e] * Nn[a][e] for e in range(n)]
        J = [cross(1, 2), cross(2, 0), cross(0, 1)] + Nn
        A = mp.matrix(6, 6)
        for k in range(6):
            for l in range(k, 6):
                A[k, l] = A[l, k] = mp.fdot(J[k], J[l])
        b = mp.matrix([-mp.fdot(J[k], r) for k in range(6)])
        z = mp.lu_solve(A, b)
        w = [z[0], z[1], z[2]]
        t2 = sum(v * v for v in w)
        th = mp.sqrt(t2)
        ca, cb = (mp.sin(th) / th, (1 - mp.cos(th)) / t2) if th > 0 else (mp.mpf(1), mp.mpf(1) / 2)
        K = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
        dR = [[(1 if a == bb else 0) + ca * K[a][bb] + cb * (w[a] * w[bb] - (t2 if a == bb else 0)) for bb in range(3)] for a in range(3)]
        R = [[mp.mpf(float(T[a, bb])) for bb in range(3)] for a in range(3)]
        d = [mp.mpf(float(T[a, 3])) - c[a] for a in range(3)]
        out = np.zeros((3, 4), f64)
        for a in range(3):
            for bb in range(3):
                out[a, bb] = float(sum(dR[a][k] * R[k][bb] for k in range(3)))
            out[a, 3] = float(sum(dR[a][k] * d[k] for k in range(3)) + c[a] + z[3 + a])
        return out


def icp_plane_ref(src, tgt, normals, T_in, max_dist, iters, tol):
    """-> dict(T (the transform in front of every iteration made, then T_out last), npairs / rmse (iters; -1 behind the last), done,
    reason, T_out, deltas (max |T_{i+1} - T_i| of every accepted step), cond)"""
    T = np.array(T_in, f64).reshape(3, 4)
    Ts, deltas, conds = [T], [], []
    npairs, rmse = np.full((iters,), -1, np.int32), np.full((iters,), -1.0, f64)
    done, reason = 0, RR.ICP_ITERS
    for i in range(iters):
        s = plane_step(src, tgt, normals, T, max_dist)
        npairs[i], rmse[i], done = s["n"], s["rmse"], i + 1
        if s["T"] is None:
            reason = s["why"]
            break
        delta = float(np.abs(s["T"] - T).max())
        T = s["T"]
        Ts.append(T)
        deltas.append(delta)
        conds.append(s["cond"])
        if delta <= tol:
            reason = RR.ICP_CONVERGED
            break
    return {"T": Ts, "npairs": npairs, "rmse": rmse, "done": done, "reason": reason, "T_out": T, "deltas": deltas, "cond": conds}


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
NORMAL_RADIUS = {3000: 0.15, 20000: 0.06}


@functools.lru_cache(maxsize=None)
def plane_pair(kind, n):
    """kind 'same' (refine_ref.icp_case: the same points on both sides) or 'halves' (icp_halves_case: two independent samplings), n =
    3000 (normal radius 0.15 m) or 20 000 (0.06 m) -> the case's dict with normal_radius and normals = normals_ref of the target (every
    caller shares the one result: treat it as read-only)"""
    c = dict((RR.icp_case if kind == "same" else RR.icp_halves_case)(n=n))
    c["normal_radius"] = NORMAL_RADIUS[n]
    c["nref"] = normals_ref(c["tgt"], c["normal_radius"])
    c["normals"] = c["nref"]["normals"]
    return c
