"""Multiway registration: a scene's pairwise results turned into one consistent set of fragment poses.

    edges = multiway.scene_edges(ctx, clouds_d, pairs, T, 0.05)        # per edge: pairs inside the gate, overlap, rmse, 6 x 6 information
    res = multiway.optimize(F, pairs, T, edges["info"])                # robust pose graph: poses, the registrations it pruned
    edges, res = multiway.register_scene(ctx, clouds_d, pairs, T)      # both
    multiway.write_scene(cfg, dataset)                                 # pre.log -> {sign}_MW/poses.log + pre.log, scored by RR_cal as it is
    multiway.write_gt_info(dataset)                                    # gt.info beside gt.log: makes an own dataset scorable

Conventions.  A pair (id0, id1) with transform T maps fragment id1 into fragment id0's frame - pre.log's and gt.log's convention; the
target of the edge is id0.  A pose X_f (4 x 4) maps fragment f into the scene frame, X_anchor = I; the pair transform the poses imply
is X_id0^-1 X_id1.  Exp(d) of d = (v, w) is [exp([w]x) | v]: the rotation by the rotation vector w beside the translation v, and
xi(D) = (translation of D, rotation vector of D) is its inverse.

The information matrices are the hot path and come from the device (Context.edge_information, include/yoho_multiway.h): a 60-fragment
scene has up to 1770 edges, each a nearest-neighbour pass over the dense clouds, grouped here by target so that a scene builds one
grid per fragment.  The solve has 6 F unknowns and takes milliseconds: it stays on the host in float64 numpy, like YOHO-C's stacked
SVD, and involves no device at all (`optimize` can be run on matrices from anywhere, a .info file included).
"""
import os

import numpy as np

from . import RR_cal

f64 = np.float64
MAX_K = 64                                  # hip.MULTIWAY_MAX_K
MAX_SOURCE_POINTS = 1 << 26                 # hip.MULTIWAY_MAX_SOURCE_POINTS


# ---- SE(3) in batches ------------------------------------------------------------------------------------------------------------------
def skew(v):
    """(...,3) -> (...,3,3): [v]x"""
    v = np.asarray(v, f64)
    S = np.zeros(v.shape[:-1] + (3, 3), f64)
    S[..., 0, 1], S[..., 0, 2] = -v[..., 2], v[..., 1]
    S[..., 1, 0], S[..., 1, 2] = v[..., 2], -v[..., 0]
    S[..., 2, 0], S[..., 2, 1] = -v[..., 1], v[..., 0]
    return S


def so3_exp(w):
    """(...,3) rotation vectors -> (...,3,3)"""
    w = np.asarray(w, f64)
    th2 = np.sum(w * w, axis=-1)
    th = np.sqrt(th2)
    small = th < 1e-6
    ths, th2s = np.where(small, 1.0, th), np.where(small, 1.0, th2)
    a = np.where(small, 1.0 - th2 / 6.0, np.sin(ths) / ths)
    b = np.where(small, 0.5 - th2 / 24.0, (1.0 - np.cos(ths)) / th2s)
    K = skew(w)
    return np.eye(3) + a[..., None, None] * K + b[..., None, None] * (K @ K)


def so3_log(R):
    """(...,3,3) rotations -> (...,3) rotation vectors, angle in [0, pi]"""
    R = np.asarray(R, f64)
    v = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], axis=-1)
    s = 0.5 * np.sqrt(np.sum(v * v, axis=-1))
    c = 0.5 * (np.trace(R, axis1=-2, axis2=-1) - 1.0)
    th = np.arctan2(s, c)
    small = s < 1e-6
    k = np.where(small & (c > 0), 0.5 + th * th / 12.0, 0.5 * th / np.where(small, 1.0, s))
    out = k[..., None] * v
    flip = small & (c <= 0)                                            # a half turn: the axis from the symmetric part
    if np.any(flip):
        Rf, vf = R[flip], v[flip]
        A = 0.5 * (Rf + np.eye(3))
        i = np.argmax(np.diagonal(A, axis1=-2, axis2=-1), axis=-1)
        n = np.arange(A.shape[0])
        ax = A[n, :, i] / np.sqrt(A[n, i, i])[:, None]
        ax = np.where((np.sum(ax * vf, axis=-1) < 0)[:, None], -ax, ax)
        out[flip] = ax * th[flip][:, None]
    return out


def so3_jr_inv(phi):
    """the inverse right Jacobian of the SO(3) logarithm at phi (...,3): log(Exp(phi) Exp(d)) = phi + Jr^-1(phi) d + O(d^2)"""
    phi = np.asarray(phi, f64)
    th2 = np.sum(phi * phi, axis=-1)
    th = np.sqrt(th2)
    small = th < 1e-4
    ths, th2s = np.where(small, 1.0, th), np.where(small, 1.0, th2)
    # 1 / th^2 - (1 + cos th) / (2 th sin th); sin(pi) = 0 is guarded, the coefficient is 1 / pi^2 there
    sn = np.sin(ths)
    tail = np.where(np.abs(sn) < 1e-12, 0.0, (1.0 + np.cos(ths)) / (2.0 * ths * np.where(np.abs(sn) < 1e-12, 1.0, sn)))
    g = np.where(small, 1.0 / 12.0 + th2 / 720.0, 1.0 / th2s - tail)
    K = skew(phi)
    return np.eye(3) + 0.5 * K + g[..., None, None] * (K @ K)


def se3(R, t):
    X = np.zeros(np.shape(t)[:-1] + (4, 4), f64)
    X[..., :3, :3], X[..., :3, 3], X[..., 3, 3] = R, t, 1.0
    return X


def se3_inv(X):
    Rt = np.swapaxes(X[..., :3, :3], -1, -2)
    return se3(Rt, -np.einsum("...ij,...j->...i", Rt, X[..., :3, 3]))


def se3_exp(d):
    """(...,6) (v, w) -> [exp([w]x) | v]"""
    d = np.asarray(d, f64)
    return se3(so3_exp(d[..., 3:]), d[..., :3])


def se3_xi(D):
    """(...,4,4) -> (...,6): (translation, rotation vector)"""
    return np.concatenate([D[..., :3, 3], so3_log(D[..., :3, :3])], axis=-1)


def as_4x4(T):
    """(E,3,4) or (E,4,4) -> (E,4,4) f64"""
    T = np.asarray(T, f64)
    if T.ndim != 3 or T.shape[1:] not in ((3, 4), (4, 4)):
        raise ValueError("transforms must be (E,3,4) or (E,4,4)")
    if T.shape[1] == 4:
        return T.copy()
    out = np.zeros((T.shape[0], 4, 4), f64)
    out[:, :3], out[:, 3, 3] = T, 1.0
    return out


# ---- the objective -----------------------------------------------------------------------------------------------------------------------
def edge_residuals(X, ij, Tinv):
    """xi_e of D_e = X_i^-1 X_j T_e^-1 for the edges ij (E,2) -> (xi (E,6), D (E,4,4), A = X_i^-1 X_j (E,4,4))"""
    A = se3_inv(X[ij[:, 0]]) @ X[ij[:, 1]]
    D = A @ Tinv
    return se3_xi(D), D, A


def edge_jacobians(xi, D, A, Tinv):
    """d xi_e / d delta_i and d xi_e / d delta_j (E,6,6 each) under X_f <- X_f Exp(delta_f), exact at delta = 0:
       D' = Exp(d_i)^-1 D:              t' = Exp(-w) (t_D - v),            R' = R_D Exp(-R_D^T w)
       D' = A Exp(d_j) T^-1:            t' = t_A + R_A (v + Exp(w) t_m),   R' = R_D Exp(R_m^T w),    T^-1 = [R_m | t_m]"""
    E = xi.shape[0]
    Jri = so3_jr_inv(xi[:, 3:])
    RD, tD, RA, Rm, tm = D[:, :3, :3], D[:, :3, 3], A[:, :3, :3], Tinv[:, :3, :3], Tinv[:, :3, 3]
    Ji, Jj = np.zeros((E, 6, 6), f64), np.zeros((E, 6, 6), f64)
    Ji[:, :3, :3] = -np.eye(3)
    Ji[:, :3, 3:] = skew(tD)
    Ji[:, 3:, 3:] = -Jri @ np.swapaxes(RD, -1, -2)
    Jj[:, :3, :3] = RA
    Jj[:, :3, 3:] = -RA @ skew(tm)
    Jj[:, 3:, 3:] = Jri @ np.swapaxes(Rm, -1, -2)
    return Ji, Jj


def line_weights(rbar, certain, tau):
    """the closed-form line process l_e = (tau^2 / (tau^2 + rbar_e))^2, 1 for the certain edges"""
    l = (tau * tau / (tau * tau + rbar)) ** 2
    return np.where(certain, 1.0, l)


def _evaluate(X, ij, Tinv, info, n, certain, tau, line):
    xi, D, A = edge_residuals(X, ij, Tinv)
    r = np.einsum("ei,eij,ej->e", xi, info, xi)
    rbar = r / n
    l = line_weights(rbar, certain, tau) if line else np.ones_like(r)
    f = float(np.sum(l * r + n * tau * tau * (np.sqrt(l) - 1.0) ** 2))
    return f, l, rbar, xi, D, A


def objective(poses, pairs, T, info, certain=None, tau=0.2):
    """sum_e l_e r_e + n_e tau^2 (sqrt(l_e) - 1)^2 at the poses (F,4,4), l_e the closed form of its own minimum over l (1 for the
    certain edges): the function `optimize`'s first stage decreases.  Every edge given is used."""
    ij, Tinv, info, n, certain = _prepare(pairs, T, info, certain)
    return _evaluate(np.asarray(poses, f64), ij, Tinv, info, n, certain, tau, True)[0]


def gradient(poses, pairs, T, info, certain=None, tau=0.2):
    """the gradient of `objective` with respect to the local updates X_f <- X_f Exp(delta_f) at delta = 0, (F,6).  l_e minimises the
    objective over l, so d objective = sum_e l_e d r_e (the envelope), d r_e = 2 xi_e' info_e d xi_e."""
    ij, Tinv, info, n, certain = _prepare(pairs, T, info, certain)
    X = np.asarray(poses, f64)
    _, l, _, xi, D, A = _evaluate(X, ij, Tinv, info, n, certain, tau, True)
    Ji, Jj = edge_jacobians(xi, D, A, Tinv)
    w = 2.0 * l[:, None] * np.einsum("eij,ej->ei", info, xi)
    g = np.zeros((X.shape[0], 6), f64)
    np.add.at(g, ij[:, 0], np.einsum("eji,ej->ei", Ji, w))
    np.add.at(g, ij[:, 1], np.einsum("eji,ej->ei", Jj, w))
    return g


def _prepare(pairs, T, info, certain):
    ij = np.asarray(pairs, np.int64).reshape(-1, 2)
    info = np.asarray(info, f64).reshape(-1, 6, 6)
    E = ij.shape[0]
    T4 = as_4x4(T)
    if T4.shape[0] != E or info.shape[0] != E:
        raise ValueError("pairs (E,2), T (E,3,4) or (E,4,4) and info (E,6,6) must have one row per edge")
    certain = np.zeros((E,), bool) if certain is None else np.asarray(certain, bool).reshape(-1)
    if certain.shape[0] != E:
        raise ValueError("certain must have one flag per edge")
    return ij, se3_inv(T4), info, info[:, 0, 0].copy(), certain


# ---- the solve ---------------------------------------------------------------------------------------------------------------------------
def _component(F, ij, use, anchor):
    """the fragments the edges `use` connect to the anchor"""
    reached = np.zeros((F,), bool)
    reached[anchor] = True
    grew = True
    while grew:
        a, b = reached[ij[use, 0]], reached[ij[use, 1]]
        new = a != b
        grew = bool(new.any())
        reached[ij[use, 0][new]] = True
        reached[ij[use, 1][new]] = True
    return reached


def spanning_tree_poses(F, ij, T4, Tinv, n, use, anchor):
    """poses along the tree grown from the anchor, always taking the reachable edge with the largest n_e, the first among equals"""
    X = np.full((F, 4, 4), np.nan, f64)
    X[anchor] = np.eye(4)
    reached = np.zeros((F,), bool)
    reached[anchor] = True
    order = [e for e in np.argsort(-n, kind="stable") if use[e]]
    while True:
        for e in order:
            i, j = ij[e]
            if reached[i] != reached[j]:
                if reached[i]:
                    X[j] = X[i] @ T4[e]
                else:
                    X[i] = X[j] @ Tinv[e]
                reached[i] = reached[j] = True
                break
        else:
            return X, reached


def _solve(X, free, ij, Tinv, info, n, certain, tau, line, max_iters, history):
    """Levenberg-Marquardt from X over the edges given (all inside the anchor's component); free (F,) bool: the fragments that move"""
    F = X.shape[0]
    col = np.full((F,), -1, np.int64)
    col[free] = np.arange(int(free.sum()))
    nf = int(free.sum())
    f, l, rbar, xi, D, A = _evaluate(X, ij, Tinv, info, n, certain, tau, line)
    history.append(f)
    lam = 1e-6
    for _ in range(max_iters):
        if nf == 0 or ij.shape[0] == 0:
            break
        Ji, Jj = edge_jacobians(xi, D, A, Tinv)
        L = l[:, None, None] * info
        H = np.zeros((nf, nf, 6, 6), f64)
        g = np.zeros((nf, 6), f64)
        Lxi = np.einsum("eij,ej->ei", L, xi)
        for a, Ja in ((0, Ji), (1, Jj)):
            ca = col[ij[:, a]]
            ma = ca >= 0
            np.add.at(g, ca[ma], np.einsum("eji,ej->ei", Ja, Lxi)[ma])
            JaL = np.einsum("eji,ejk->eik", Ja, L)
            for b, Jb in ((0, Ji), (1, Jj)):
                cb = col[ij[:, b]]
                m = ma & (cb >= 0)
                np.add.at(H, (ca[m], cb[m]), (JaL @ Jb)[m])
        H = H.transpose(0, 2, 1, 3).reshape(6 * nf, 6 * nf)
        g = g.reshape(-1)
        dH = np.diag(np.diag(H))
        accepted = False
        while lam <= 1e12:
            try:
                d = np.linalg.solve(H + lam * dH, -g)
            except np.linalg.LinAlgError:
                lam *= 10.0
                continue
            if not np.all(np.isfinite(d)):
                lam *= 10.0
                continue
            Xn = X.copy()
            Xn[free] = X[free] @ se3_exp(d.reshape(nf, 6))
            new = _evaluate(Xn, ij, Tinv, info, n, certain, tau, line)
            if new[0] < f:
                accepted = True
                break
            lam *= 10.0
        if not accepted:
            break
        rel = (f - new[0]) / max(f, 1e-300)
        X = Xn
        f, l, rbar, xi, D, A = new
        history.append(f)
        lam = max(lam / 10.0, 1e-9)
        if rel < 1e-15 or np.abs(d).max() < 1e-13:
            break
    return X, l, rbar


def optimize(F, pairs, T, info, certain=None, tau=0.2, prune=0.25, anchor=0, min_pairs=10, max_iters=100):
    """Robust pose graph over the registered pairs of a scene: F fragments, pairs (E,2) (id0, id1), T (E,3,4) or (E,4,4) fragment id1
    into id0's frame, info (E,6,6) the edges' information matrices (info[e,0,0] = n_e, the pairs of the overlap).  float64 numpy.

    Edges with n_e < min_pairs are dropped up front.  The residual of edge e = (i, j) is xi_e = xi(X_i^-1 X_j T_e^-1),
    r_e = xi_e' info_e xi_e, rbar_e = r_e / n_e - the mean squared displacement of the overlap, what the registration benchmark
    thresholds at 0.2^2.  Stage 1 minimises the line-process objective of Choi, Zhou, Koltun (CVPR 2015),
    sum_e l_e r_e + n_e tau^2 (sqrt(l_e) - 1)^2 with l_e = (tau^2 / (tau^2 + rbar_e))^2 (l_e = 1 for the `certain` edges; by default
    none is: any registration can be wrong), from the spanning tree grown from the anchor along the edges with the most pairs, by
    Levenberg-Marquardt with the anchor fixed, the update X_f <- X_f Exp(delta_f) and the exact Jacobians of the residual; a step is
    accepted only if the objective decreases; it stops at max |delta| < 1e-13, a relative decrease < 1e-15 or max_iters.  An edge is
    PRUNED iff it is uncertain and l_e < prune (at 0.25: rbar_e > tau^2, the edge fails the benchmark's criterion against the
    optimised poses).  Stage 2 is the same solve from stage 1's poses over the kept edges with every l_e = 1.

    -> dict: poses (F,4,4), poses[anchor] = I exactly, NaN for the fragments the kept edges do not connect to the anchor;
       reached (F,) bool; weights (E,) stage 1's l_e (0 for a dropped edge); pruned (E,) bool; dropped (E,) bool; rbar (E,) against the
       final poses (NaN where a fragment is not reached); history: the objective at the start of each stage and after every accepted
       iteration, stage 1 then stage 2 (history_stage1 / history_stage2 apart)."""
    ij, Tinv, info, n, certain = _prepare(pairs, T, info, certain)
    T4 = se3_inv(Tinv)
    E = ij.shape[0]
    F, anchor = int(F), int(anchor)
    if not 0 <= anchor < F or (E and (ij.min() < 0 or ij.max() >= F)) or np.any(ij[:, 0] == ij[:, 1]):
        raise ValueError("optimize: fragment ids must be in [0, F), the two of a pair distinct, the anchor one of them")
    dropped = ~(n >= min_pairs)                                        # a NaN count is dropped too
    use = ~dropped
    X, reached = spanning_tree_poses(F, ij, T4, Tinv, n, use, anchor)
    use1 = use & reached[ij[:, 0]] & reached[ij[:, 1]]
    free = reached.copy()
    free[anchor] = False
    hist1, hist2 = [], []
    sel = np.nonzero(use1)[0]
    Xs = np.where(reached[:, None, None], X, np.eye(4))
    Xs, l1, _ = _solve(Xs, free, ij[sel], Tinv[sel], info[sel], n[sel], certain[sel], tau, True, max_iters, hist1)
    weights = np.zeros((E,), f64)
    weights[sel] = l1
    pruned = np.zeros((E,), bool)
    pruned[sel] = ~certain[sel] & (l1 < prune)
    keep = use1 & ~pruned
    reached2 = _component(F, ij, keep, anchor)
    keep &= reached2[ij[:, 0]] & reached2[ij[:, 1]]
    free2 = reached2.copy()
    free2[anchor] = False
    sel2 = np.nonzero(keep)[0]
    Xs, _, _ = _solve(Xs, free2, ij[sel2], Tinv[sel2], info[sel2], n[sel2], certain[sel2], tau, False, max_iters, hist2)
    poses = np.where(reached2[:, None, None], Xs, np.nan)
    poses[anchor] = np.eye(4)
    rbar = np.full((E,), np.nan, f64)
    both = reached2[ij[:, 0]] & reached2[ij[:, 1]] & (n > 0)
    if both.any():
        xi = edge_residuals(Xs, ij[both], Tinv[both])[0]
        rbar[both] = np.einsum("ei,eij,ej->e", xi, info[both], xi) / n[both]
    return {"poses": poses, "reached": reached2, "weights": weights, "pruned": pruned, "dropped": dropped, "rbar": rbar,
            "history": hist1 + hist2, "history_stage1": hist1, "history_stage2": hist2}


def implied_transforms(poses, pairs):
    """X_id0^-1 X_id1 for every pair, (E,4,4); NaN where a pose is"""
    ij = np.asarray(pairs, np.int64).reshape(-1, 2)
    poses = np.asarray(poses, f64)
    return se3_inv(poses[ij[:, 0]]) @ poses[ij[:, 1]]


# ---- the edges of a scene, on the device ---------------------------------------------------------------------------------------------------
def edge_chunks(pairs, sizes, max_k=MAX_K, max_points=MAX_SOURCE_POINTS):
    """the edges grouped by target (id0) in ascending target order, each group cut into chunks of at most max_k sources and at most
    max_points source points, in the order of `pairs` -> [(target, [edge indices])]"""
    ij = np.asarray(pairs, np.int64).reshape(-1, 2)
    chunks = []
    for t in np.unique(ij[:, 0]):
        cur, pts = [], 0
        for e in np.nonzero(ij[:, 0] == t)[0]:
            m = int(sizes[ij[e, 1]])
            if cur and (len(cur) == max_k or pts + m > max_points):
                chunks.append((int(t), cur))
                cur, pts = [], 0
            cur.append(int(e))
            pts += m
        chunks.append((int(t), cur))
    return chunks


def scene_edges(ctx, clouds_d, pairs, T, max_dist):
    """clouds_d: the F fragments as (n_f,3) device tensors (f32, or anything .to(float32) takes), pairs (E,2), T (E,3,4) or (E,4,4)
    -> dict(npairs (E) int32, overlap (E) = npairs / source points, rmse (E), info (E,6,6)) in the order of `pairs`, numpy.  One
    Context.edge_information call per chunk of edge_chunks - one grid per target -, everything read back once at the end."""
    import torch
    ij = np.asarray(pairs, np.int64).reshape(-1, 2)
    E = ij.shape[0]
    T34 = np.ascontiguousarray(as_4x4(T)[:, :3, :])
    if T34.shape[0] != E:
        raise ValueError("scene_edges: one transform per pair")
    clouds = [c if c.dtype == torch.float32 and c.is_contiguous() else c.to(torch.float32).contiguous() for c in clouds_d]
    sizes = np.array([c.shape[0] for c in clouds], np.int64)
    if E and (ij.min() < 0 or ij.max() >= len(clouds)):
        raise ValueError("scene_edges: a pair names a fragment that is not there")
    out_n, out_r, out_i, order = [], [], [], []
    for t, es in edge_chunks(ij, sizes):
        srcs = [clouds[ij[e, 1]] for e in es]
        soff = np.concatenate([[0], np.cumsum([s.shape[0] for s in srcs])]).astype(np.int32)
        src = srcs[0] if len(srcs) == 1 else torch.cat(srcs, dim=0)
        T_d = torch.from_numpy(T34[es]).to(src.device)
        n, r, i = ctx.edge_information(src, soff, clouds[t], T_d, max_dist)
        out_n.append(n); out_r.append(r); out_i.append(i); order += es
    npairs, rmse, info = np.zeros((E,), np.int32), np.zeros((E,), f64), np.zeros((E, 6, 6), f64)
    if E:
        order = np.asarray(order, np.int64)
        npairs[order] = torch.cat(out_n).cpu().numpy()
        rmse[order] = torch.cat(out_r).cpu().numpy()
        info[order] = torch.cat(out_i).cpu().numpy()
    return {"npairs": npairs, "overlap": npairs / np.maximum(sizes[ij[:, 1]], 1).astype(f64), "rmse": rmse, "info": info}


def register_scene(ctx, clouds_d, pairs, T, max_dist=0.05, **optimize_kwargs):
    """scene_edges, then optimize(len(clouds_d), pairs, T, info, ...) -> (edges, result)"""
    edges = scene_edges(ctx, clouds_d, pairs, T, max_dist)
    return edges, optimize(len(clouds_d), pairs, T, edges["info"], **optimize_kwargs)


# ---- files -------------------------------------------------------------------------------------------------------------------------------
def _device_edges(ctx):
    import torch
    from . import hip
    ctx = hip.get_context() if ctx is None else ctx

    def edges(clouds, pairs, T, max_dist):
        clouds_d = [torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)).cuda() for c in clouds]
        return scene_edges(ctx, clouds_d, pairs, T, max_dist)
    return edges


def _scene_clouds(dataset):
    return [np.ascontiguousarray(np.asarray(dataset.get_pc(cid), dtype=np.float64)[:, :3], dtype=np.float32) for cid in dataset.get_cloud_ids()]


def write_scene(cfg, dataset, yoho_sign='YOHO_O', max_iter=1000, max_dist=0.05, ctx=None, edges=None, **optimize_kwargs):
    """The multiway result of one scene.  Reads result_dir(cfg, dataset, yoho_sign, max_iter)/pre.log (what run_dataset left) and the
    dataset's clouds, registers the scene and writes, under the sign f'{yoho_sign}_MW':
        poses.log   the F absolute poses (RR_cal.write_trajectory, header "f f F"; an unreached fragment holds nan)
        pre.log     the transform the poses imply for every pair of dataset.pair_ids (estimator.format_log_entry); a pair that
                    touches an unreached fragment keeps its pairwise estimate
    so that RR_cal.benchmark(cfg, datasets, max_iter, yoho_sign=f'{yoho_sign}_MW') scores it as it is.
    edges(clouds, pairs, T, max_dist) -> scene_edges' dict, on host arrays, replaces the device pass (tests).  -> (edges, result)"""
    from .estimator import format_log_entry
    from .run_dataset import result_dir
    keys, traj = RR_cal.read_pre_trajectory(os.path.join(result_dir(cfg, dataset, yoho_sign, max_iter), 'pre.log'))
    pairs = np.array([[int(float(k[0])), int(float(k[1]))] for k in keys], np.int64).reshape(-1, 2)
    clouds = _scene_clouds(dataset)
    F = len(clouds)
    edges = _device_edges(ctx) if edges is None else edges
    ed = edges(clouds, pairs, traj, max_dist)
    res = optimize(F, pairs, traj, ed["info"], **optimize_kwargs)
    out_dir = result_dir(cfg, dataset, f'{yoho_sign}_MW', max_iter)
    os.makedirs(out_dir, exist_ok=True)
    RR_cal.write_trajectory(res["poses"], [(f, f, F) for f in range(F)], os.path.join(out_dir, 'poses.log'))
    pairwise = {(int(a), int(b)): traj[e] for e, (a, b) in enumerate(pairs)}
    text = []
    for id0, id1 in dataset.pair_ids:
        a, b = int(id0), int(id1)
        if res["reached"][a] and res["reached"][b]:
            trans = implied_transforms(res["poses"], [(a, b)])[0]
        elif (a, b) in pairwise:
            trans = pairwise[(a, b)]
        else:
            continue
        text.append(format_log_entry(a, b, F, trans))
    with open(os.path.join(out_dir, 'pre.log'), 'w') as fh:
        fh.write("".join(text))
    return ed, res


def gt_info_path(dataset):
    return dataset.gt_dir[:dataset.gt_dir.rfind('.')] + '.info'


def write_gt_info(dataset, max_dist=0.05, ctx=None, overwrite=False, edges=None):
    """gt.info beside gt.log: the information matrix of every ground-truth pair under its ground-truth transform, in gt.log's order -
    per pair one header line "id0 id1 n_fragments" and six rows, the Redwood format RR_cal.read_trajectory_info reads.  RR_cal.benchmark
    needs it and only the downloaded datasets carry one; with keypoints.write_keypoints this makes an own dataset scorable.  An
    existing file is left alone (overwrite=True: replaced).  edges: as in write_scene.  -> the path, or None when the file was left."""
    path = gt_info_path(dataset)
    if os.path.exists(path) and not overwrite:
        return None
    keys, traj = RR_cal.read_trajectory(dataset.gt_dir)
    pairs = np.array([[int(float(k[0])), int(float(k[1]))] for k in keys], np.int64).reshape(-1, 2)
    clouds = _scene_clouds(dataset)
    F = len(clouds)
    edges = _device_edges(ctx) if edges is None else edges
    info = np.asarray(edges(clouds, pairs, traj, max_dist)["info"], f64)
    with open(path, 'w') as fh:
        for (a, b), M in zip(pairs, info):
            fh.write(f"{a}\t{b}\t{F}\n")
            fh.write("".join("\t".join(repr(float(v)) for v in row) + "\n" for row in M))
    return path
