"""The contract of include/yoho_multiway.h and a plain pose-graph solver on the CPU (helper of tests/test_multiway_cpu.py and
tests/test_gpu_multiway.py, not a conftest).

  edge_info_ref     K edges into one target: pairs inside the gate, rmse, the 6 x 6 information matrix - on refine_ref's transform_f32,
                    nn_within_ref, tree_sum and gate2_of, so rmse and the ten sums are the header's bits
  info_literal      SUM G^T G, G = [I | -[p]x], one point at a time in float64: what the matrix is
  optimize_ref      a deliberately plain solver for graphs WITHOUT outliers: Gauss-Newton on the stacked whitened residuals with a
                    central-difference Jacobian; it shares no code with yoho_amd/multiway.py
  outlier_case      the seeded synthetic pose graphs of the tests; scene_case the six-fragment scene cut from one surface
"""
import numpy as np

import refine_ref as RR

f32, f64 = np.float32, np.float64


# ---- the device entry ----------------------------------------------------------------------------------------------------------------------
def edge_info_ref(src, soff, tgt, T, max_dist):
    """src (S,3) f32, soff (K+1), tgt (Nt,3) f32, T (K,3,4) f64 -> (npairs (K) int32, rmse (K) f64, info (K,6,6) f64)"""
    src, tgt = np.ascontiguousarray(src, f32).reshape(-1, 3), np.ascontiguousarray(tgt, f32).reshape(-1, 3)
    soff = np.asarray(soff, np.int64)
    T = np.asarray(T, f64).reshape(-1, 3, 4)
    K = soff.shape[0] - 1
    assert T.shape[0] == K and soff[0] == 0 and soff[-1] == src.shape[0] and (np.diff(soff) > 0).all()
    npairs, rmse, info = np.zeros((K,), np.int32), np.zeros((K,), f64), np.zeros((K, 6, 6), f64)
    for k in range(K):
        s = src[soff[k]:soff[k + 1]]                     # the LOCAL index: the sums start at the source's first point
        with np.errstate(all="ignore"):
            q = RR.transform_f32(T[k], s)
        idx, d2 = RR.nn_within_ref(q, tgt, max_dist)
        sel = idx >= 0
        n = int(sel.sum())
        d = np.where(sel, d2, f32(0)).astype(f64)
        npairs[k] = n
        rmse[k] = np.sqrt(RR.tree_sum(d) / f64(n)) if n else f64(np.inf)
        p = np.where(sel[:, None], tgt[np.maximum(idx, 0)].astype(f64), 0.0)
        sx, sy, sz = RR.tree_sum(p)
        Sxx, Sxy, Sxz, Syy, Syz, Szz = RR.tree_sum(np.stack([p[:, 0] * p[:, 0], p[:, 0] * p[:, 1], p[:, 0] * p[:, 2], p[:, 1] * p[:, 1],
                                                             p[:, 1] * p[:, 2], p[:, 2] * p[:, 2]], axis=1))
        M = info[k]
        M[0, 0] = M[1, 1] = M[2, 2] = f64(n)
        M[:3, 3:] = [[0.0, sz, -sy], [-sz, 0.0, sx], [sy, -sx, 0.0]]
        M[3:, :3] = M[:3, 3:].T
        M[3:, 3:] = [[Syy + Szz, -Sxy, -Sxz], [-Sxy, Sxx + Szz, -Syz], [-Sxz, -Syz, Sxx + Syy]]
    return npairs, rmse, info + 0.0                      # + 0.0: no negative zeros (the sign of a zero is not part of the contract)


def cross_matrix(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]], f64)


def info_literal(p):
    """p (n,3) -> SUM G^T G in float64, G = [I | -[p]x], one point after another"""
    M = np.zeros((6, 6), f64)
    for x in np.asarray(p, f64):
        G = np.concatenate([np.eye(3), -cross_matrix(x)], axis=1)
        M += G.T @ G
    return M


# ---- rigid motions, one at a time ----------------------------------------------------------------------------------------------------------
def rot_of(w):
    w = np.asarray(w, f64)
    th = np.linalg.norm(w)
    K = cross_matrix(w)
    if th < 1e-9:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / th ** 2 * K @ K


def rotvec_of(R):
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], f64)
    s, c = 0.5 * np.linalg.norm(v), 0.5 * (np.trace(R) - 1.0)
    th = np.arctan2(s, c)
    if s < 1e-9:
        assert c > 0, "a half turn: not met by these tests"
        return 0.5 * v
    return v * (0.5 * th / s)


def motion(w, t):
    X = np.eye(4)
    X[:3, :3], X[:3, 3] = rot_of(w), t
    return X


def inverse(X):
    Y = np.eye(4)
    Y[:3, :3] = X[:3, :3].T
    Y[:3, 3] = -X[:3, :3].T @ X[:3, 3]
    return Y


def step_of(d):
    """the update of a pose: [rot(d[3:]) | d[:3]]"""
    return motion(d[3:], d[:3])


def residual_of(Xi, Xj, Tinv):
    D = inverse(Xi) @ Xj @ Tinv
    return np.concatenate([D[:3, 3], rotvec_of(D[:3, :3])])


def pose_error(Xa, Xb):
    """the largest rotation (degrees) and translation (metres) difference over two stacks of poses"""
    deg = max(float(np.degrees(np.linalg.norm(rotvec_of(a[:3, :3].T @ b[:3, :3])))) for a, b in zip(Xa, Xb))
    return deg, max(float(np.linalg.norm(a[:3, 3] - b[:3, 3])) for a, b in zip(Xa, Xb))


# ---- the plain solver ----------------------------------------------------------------------------------------------------------------------
def optimize_ref(F, pairs, T, info, X0, anchor=0, h=1e-6, stop=1e-12, max_iters=40):
    """least squares sum_e xi_e' info_e xi_e over the poses, X_anchor = I: Gauss-Newton on the stacked residuals W_e^T xi_e
    (info_e = W_e W_e^T, Cholesky) with a central-difference Jacobian of step h, from X0, until the largest step entry is below
    `stop` -> poses (F,4,4).  For graphs without outliers only: no damping, no robust weight."""
    X = [np.array(x, f64) for x in X0]
    X[anchor] = np.eye(4)
    E = len(pairs)
    Tinv = [inverse(np.vstack([np.asarray(t, f64)[:3], [0, 0, 0, 1.0]])) for t in T]
    W = [np.linalg.cholesky(np.asarray(m, f64)) for m in info]
    col = {f: 6 * c for c, f in enumerate(f for f in range(F) if f != anchor)}
    for _ in range(max_iters):
        J = np.zeros((6 * E, 6 * (F - 1)), f64)
        r = np.zeros((6 * E,), f64)
        for e, (i, j) in enumerate(pairs):
            r[6 * e:6 * e + 6] = W[e].T @ residual_of(X[i], X[j], Tinv[e])
            for f in (i, j):
                if f == anchor:
                    continue
                for k in range(6):
                    d = np.zeros((6,), f64)
                    d[k] = h
                    Xp, Xm = X[f] @ step_of(d), X[f] @ step_of(-d)
                    rp = residual_of(Xp, X[j], Tinv[e]) if f == i else residual_of(X[i], Xp, Tinv[e])
                    rm = residual_of(Xm, X[j], Tinv[e]) if f == i else residual_of(X[i], Xm, Tinv[e])
                    J[6 * e:6 * e + 6, col[f] + k] = W[e].T @ (rp - rm) / (2.0 * h)
        d = np.linalg.lstsq(J, -r, rcond=None)[0]
        for f, c in col.items():
            X[f] = X[f] @ step_of(d[c:c + 6])
        if np.abs(d).max() < stop:
            break
    return np.stack(X)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
def info_from_points(p):
    """the matrix in closed form from n points, float64 (numpy's own summation order)"""
    p = np.asarray(p, f64)
    S, PP = p.sum(axis=0), p.T @ p
    M = np.zeros((6, 6), f64)
    M[:3, :3] = p.shape[0] * np.eye(3)
    M[:3, 3:] = -cross_matrix(S)
    M[3:, :3] = -cross_matrix(S).T
    M[3:, 3:] = np.trace(PP) * np.eye(3) - PP
    return M


def random_direction(rs):
    d = rs.randn(3)
    return d / np.linalg.norm(d)


_CASES = {}


def outlier_case(F, seed):
    """A pose graph with false registrations -> dict(F, Xg (F,4,4) ground truth with Xg[0] = I, pairs (E,2), T (E,4,4), info (E,6,6),
    consecutive (E,) bool, outlier (E,) bool).  Ground-truth rotations up to 70 degrees about random axes, translations of about 2 m
    (normal, sigma 1.2 m per axis).  Every consecutive pair and 60 % of the others.  An inlier edge is the ground truth times
    Exp of normal noise, sigma 1 cm / 0.5 degrees per axis, its information built from 800 - 2300 points of a 2 m cube somewhere
    in fragment id0's frame.  A quarter of the non-consecutive edges are false: the rotation about 57 degrees (0.8 - 1.2 rad) and
    the translation about 1 m (0.8 - 1.2 m) off, 200 - 500 points - fewer than any inlier edge, as false registrations have.
    Computed once per (F, seed) and shared: the callers do not modify it."""
    if (F, seed) in _CASES:
        return _CASES[(F, seed)]
    rs = np.random.RandomState(7000 + 100 * F + seed)
    Xg = [np.eye(4)] + [motion(random_direction(rs) * np.deg2rad(70.0) * rs.rand(), rs.randn(3) * 1.2) for _ in range(F - 1)]
    pairs, T, info, consecutive, outlier = [], [], [], [], []
    for i in range(F):
        for j in range(i + 1, F):
            if j - i > 1 and rs.rand() >= 0.6:
                continue
            Tt = inverse(Xg[i]) @ Xg[j]
            bad = j - i > 1 and rs.rand() < 0.25
            if bad:
                Tm = Tt @ motion(random_direction(rs) * (0.8 + 0.4 * rs.rand()), np.zeros(3))
                Tm[:3, 3] = Tt[:3, 3] + random_direction(rs) * (0.8 + 0.4 * rs.rand())
                npts = int(200 + 300 * rs.rand())
            else:
                Tm = Tt @ motion(rs.randn(3) * np.deg2rad(0.5), rs.randn(3) * 0.01)
                npts = int(800 + 1500 * rs.rand())
            p = rs.rand(npts, 3) * 2.0 - 1.0 + rs.randn(3)
            pairs.append((i, j)); T.append(Tm); info.append(info_from_points(p)); consecutive.append(j - i == 1); outlier.append(bad)
    c = {"F": F, "Xg": np.stack(Xg), "pairs": np.array(pairs, np.int64), "T": np.stack(T), "info": np.stack(info),
         "consecutive": np.array(consecutive), "outlier": np.array(outlier)}
    _CASES[(F, seed)] = c
    return c


_CLEAN = {}


def clean_solution(F, seed):
    """optimize_ref on the outlier-free graph of outlier_case(F, seed), started from the ground truth; computed once and shared"""
    if (F, seed) not in _CLEAN:
        c = outlier_case(F, seed)
        ok = ~c["outlier"]
        _CLEAN[(F, seed)] = optimize_ref(F, [tuple(p) for p in c["pairs"][ok]], c["T"][ok], c["info"][ok], c["Xg"])
    return _CLEAN[(F, seed)]


_SCENE = {}


def scene_case(seed=0, n=12000, frag=3000, F=6):
    """Six fragments of about 3000 points cut with overlap from one 12 000-point synth.surface_cloud: fragment f holds a random 3000 of
    the points whose x lies between the quantiles 0.1 f and 0.1 f + 0.5, stored in its own frame (f32); the pairs are those whose
    windows share at least 0.2 (|i - j| <= 3).  Pairwise transforms: the ground truth turned by 0.5 degrees and moved by 1 cm
    (refine_ref.perturbed), and the pair (1, 3) replaced by the ground truth turned by 40 degrees and moved by 10 cm: a false
    registration that still finds a hundred or more partners inside the gate -> dict(clouds [F x (n_f,3) f32], Xg, pairs (E,2), T (E,4,4), bad = index of the false pair, max_dist)."""
    if seed in _SCENE:
        return _SCENE[seed]
    from yoho_amd import synth
    rs = np.random.RandomState(9000 + seed)
    pc = synth.surface_cloud(n, seed=seed)
    qx = np.argsort(np.argsort(pc[:, 0])) / float(n)
    Xg = [np.eye(4)] + [motion(random_direction(rs) * np.deg2rad(60.0) * rs.rand(), rs.randn(3) * 0.5) for _ in range(F - 1)]
    clouds = []
    for f in range(F):
        rows = np.nonzero((qx >= 0.1 * f) & (qx < 0.1 * f + 0.5))[0]
        rows = np.sort(rs.permutation(rows)[:frag])
        Xi = inverse(Xg[f])
        clouds.append(np.ascontiguousarray(pc[rows] @ Xi[:3, :3].T + Xi[:3, 3], f32))
    pairs, T = [], []
    for i in range(F):
        for j in range(i + 1, min(F, i + 4)):
            Tt = inverse(Xg[i]) @ Xg[j]
            Tm = np.eye(4)
            Tm[:3] = RR.perturbed(Tt[:3], rs, 40.0, 0.1) if (i, j) == (1, 3) else RR.perturbed(Tt[:3], rs, 0.5, 0.01)
            pairs.append((i, j)); T.append(Tm)
    pairs = np.array(pairs, np.int64)
    _SCENE[seed] = {"clouds": clouds, "Xg": np.stack(Xg), "pairs": pairs, "T": np.stack(T),
                    "bad": int(np.nonzero((pairs == (1, 3)).all(axis=1))[0][0]), "max_dist": 0.05}
    return _SCENE[seed]


def scene_edges_ref(clouds, pairs, T, max_dist):
    """multiway.scene_edges on the CPU, edge by edge -> its dict"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    T = np.asarray(T, f64)
    E = pairs.shape[0]
    npairs, rmse, info = np.zeros((E,), np.int32), np.zeros((E,), f64), np.zeros((E, 6, 6), f64)
    for e, (i, j) in enumerate(pairs):
        n, r, m = edge_info_ref(clouds[j], [0, len(clouds[j])], clouds[i], T[e][None, :3, :], max_dist)
        npairs[e], rmse[e], info[e] = n[0], r[0], m[0]
    sizes = np.array([len(clouds[j]) for j in pairs[:, 1]], f64)
    return {"npairs": npairs, "overlap": npairs / sizes, "rmse": rmse, "info": info}
