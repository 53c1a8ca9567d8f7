"""yoho_fuse_clouds restated in numpy (include/yoho_fuse.h), twice.

fuse_ref: float64 elementwise (numpy fuses nothing), keys as uint64, a stable argsort, the sums with np.add.at - which applies its
operands one after another in index order, here ascending global row, onto zeros.  fuse_dict shares no code with it: Python floats
(IEEE doubles, every operation rounded), a dictionary from the cell triple to the list of its rows, a plain loop per voxel.  Both
return dict(pts (M,3) f32, normals (M,3) f32 or None, count (M) int32, nfrag (M) int32, row_of (S) int32, M, inside = the number of
inside points, all_count = the counts of ALL voxels, kept or not)."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
CELL_MAX = (1 << 20) - 1


def soff_of(clouds):
    return np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int32)


def fuse_ref(src, soff, T, voxel, min_count=1, min_frags=1, nrm=None):
    src = np.asarray(src, f32).reshape(-1, 3)
    soff = np.asarray(soff, np.int64)
    T = np.asarray(T, f64)[:, :3, :]
    S, K = src.shape[0], len(soff) - 1
    assert soff[0] == 0 and soff[-1] == S and np.all(np.diff(soff) > 0) and T.shape == (K, 3, 4)
    frag = np.repeat(np.arange(K), np.diff(soff))
    Tp = T[frag]                                                      # (S,3,4)
    s = src.astype(f64)
    with np.errstate(all="ignore"):
        q = np.stack([((Tp[:, i, 0] * s[:, 0] + Tp[:, i, 1] * s[:, 1]) + Tp[:, i, 2] * s[:, 2]) + Tp[:, i, 3] for i in range(3)], axis=1)
        inv = f64(1.0) / f64(voxel)
        c = np.floor(q * inv)
        inside = np.all((c >= -CELL_MAX) & (c <= CELL_MAX), axis=1)   # a NaN compares false
    rows = np.nonzero(inside)[0]                                      # ascending global row
    ci = c[rows].astype(np.int64) + (1 << 20)
    key = (ci[:, 2].astype(np.uint64) << np.uint64(42)) | (ci[:, 1].astype(np.uint64) << np.uint64(21)) | ci[:, 0].astype(np.uint64)
    ukey, vox = np.unique(key, return_inverse=True)                   # voxels in ascending key; vox[i] = the voxel of rows[i]
    V = ukey.shape[0]
    count = np.bincount(vox, minlength=V).astype(np.int64)
    nfrag = np.bincount(np.unique(vox.astype(np.int64) * K + frag[rows]) // K, minlength=V).astype(np.int64)
    sums = np.zeros((V, 3), f64)
    np.add.at(sums, vox, q[rows])                                     # one after another in ascending row, from +0.0
    kept = (count >= min_count) & (nfrag >= min_frags)
    krow = np.cumsum(kept) - 1
    M = int(kept.sum())
    row_of = np.full((S,), -1, np.int32)
    row_of[rows] = np.where(kept[vox], krow[vox], -1)
    with np.errstate(all="ignore"):
        pts = (sums[kept] / count[kept, None].astype(f64)).astype(f32)
    out_nrm = None
    if nrm is not None:
        n = np.asarray(nrm, f32).reshape(S, 3).astype(f64)
        with np.errstate(all="ignore"):
            nr = np.stack([(Tp[:, i, 0] * n[:, 0] + Tp[:, i, 1] * n[:, 1]) + Tp[:, i, 2] * n[:, 2] for i in range(3)], axis=1)
            ns = np.zeros((V, 3), f64)
            np.add.at(ns, vox, nr[rows])
            ns = ns[kept]
            ln = np.sqrt((ns[:, 0] * ns[:, 0] + ns[:, 1] * ns[:, 1]) + ns[:, 2] * ns[:, 2])
            ok = np.isfinite(ln) & (ln > 0)
            out_nrm = np.where(ok[:, None], ns / ln[:, None], 0.0).astype(f32)
    return {"pts": pts, "normals": out_nrm, "count": count[kept].astype(np.int32), "nfrag": nfrag[kept].astype(np.int32), "row_of": row_of, "M": M,
            "inside": int(rows.shape[0]), "all_count": count.astype(np.int32)}


def fuse_dict(src, soff, T, voxel, min_count=1, min_frags=1, nrm=None):
    src = np.asarray(src, f32).reshape(-1, 3)
    T = np.asarray(T, f64)
    S, K = src.shape[0], len(soff) - 1
    inv = 1.0 / float(voxel)
    cells, q_of, n_of, frag_of = {}, {}, {}, {}
    for k in range(K):
        R = [[float(T[k][i][j]) for j in range(4)] for i in range(3)]
        for e in range(int(soff[k]), int(soff[k + 1])):
            x, y, z = float(src[e, 0]), float(src[e, 1]), float(src[e, 2])
            q = [((R[i][0] * x + R[i][1] * y) + R[i][2] * z) + R[i][3] for i in range(3)]
            if not all(math.isfinite(v) and math.isfinite(v * inv) for v in q):
                continue
            c = tuple(math.floor(v * inv) for v in q)
            if any(abs(v) > CELL_MAX for v in c):
                continue
            cells.setdefault((c[2], c[1], c[0]), []).append(e)          # rows arrive in ascending order
            q_of[e], frag_of[e] = q, k
            if nrm is not None:
                a, b, d = float(nrm[e][0]), float(nrm[e][1]), float(nrm[e][2])
                n_of[e] = [(R[i][0] * a + R[i][1] * b) + R[i][2] * d for i in range(3)]
    pts, nrms, counts, nfrags, all_count = [], [], [], [], []
    row_of = [-1] * S
    for zyx in sorted(cells):                                          # (cz, cy, cx) ascending = ascending key
        rows = cells[zyx]
        all_count.append(len(rows))
        nf = len({frag_of[e] for e in rows})
        if len(rows) < min_count or nf < min_frags:
            continue
        acc, nac = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
        for e in rows:
            for i in range(3):
                acc[i] = acc[i] + q_of[e][i]
                if nrm is not None:
                    nac[i] = nac[i] + n_of[e][i]
            row_of[e] = len(pts)
        pts.append([acc[i] / float(len(rows)) for i in range(3)])
        counts.append(len(rows))
        nfrags.append(nf)
        if nrm is not None:
            sq = (nac[0] * nac[0] + nac[1] * nac[1]) + nac[2] * nac[2]
            ln = math.sqrt(sq) if sq >= 0.0 and math.isfinite(sq) else float("nan")     # an overflowing square gives inf, as sqrt(inf) would: zeros
            nrms.append([nac[i] / ln for i in range(3)] if math.isfinite(ln) and ln > 0.0 else [0.0, 0.0, 0.0])
    M = len(pts)
    with np.errstate(all="ignore"):
        return {"pts": np.asarray(pts, f64).reshape(M, 3).astype(f32), "normals": None if nrm is None else np.asarray(nrms, f64).reshape(M, 3).astype(f32),
                "count": np.asarray(counts, np.int32).reshape(M), "nfrag": np.asarray(nfrags, np.int32).reshape(M), "row_of": np.asarray(row_of, np.int32), "M": M,
                "inside": int(sum(all_count)), "all_count": np.asarray(all_count, np.int32)}


KEYS = ("pts", "normals", "count", "nfrag", "row_of")


def same_bytes(a, b, keys=KEYS):
    """the names of the outputs in which two results differ as bytes (None only equals None)"""
    bad = []
    for k in keys:
        x, y = a[k], b[k]
        if (x is None) != (y is None) or (x is not None and (x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes())):
            bad.append(k)
    if int(a["M"]) != int(b["M"]):
        bad.append("M")
    return bad


_GHOST = {}


def ghost_scene(seed=0):
    """multiway_ref.scene_case's six fragments under their ground-truth poses, plus a seventh: 400 points of a 0.3 m cube whose nearest
    corner lies 1 m beyond the scene's bounding box on every axis, under the identity -> dict(clouds (7), poses (7,4,4), ghost = 6,
    voxel = 0.05).  Computed once and shared; the callers do not modify it."""
    if seed not in _GHOST:
        import multiway_ref as MR
        c = MR.scene_case(seed)
        world = np.concatenate([x.astype(f64) @ X[:3, :3].T + X[:3, 3] for x, X in zip(c["clouds"], c["Xg"])])
        rs = np.random.RandomState(77 + seed)
        ghost = (world.max(axis=0) + 1.0 + 0.3 * rs.rand(400, 3)).astype(f32)
        _GHOST[seed] = {"clouds": list(c["clouds"]) + [ghost], "poses": np.concatenate([c["Xg"], np.eye(4)[None]]), "ghost": 6, "voxel": 0.05}
    return _GHOST[seed]


def rot(axis, deg):
    a = np.asarray(axis, f64) / np.linalg.norm(axis)
    t = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], f64)
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * (Kx @ Kx)


def pose(axis, deg, t):
    X = np.eye(4)
    X[:3, :3], X[:3, 3] = rot(axis, deg), t
    return X


def seeded_case(seed, n=300):
    """Six fragments that hold what the contract has words for -> dict(clouds, soff, src, T (6,3,4), nrm (S,3), voxel = 0.125):
      0  identity pose: lattice points k * voxel, k in -4 .. 4 per axis - exactly on voxel faces, q * inv an integer, negative ones
         included -, every third one twice, and n random points of [-1, 1]^3
      1  a generic pose, n points
      2  a pose with a NaN entry
      3  a pure translation by 2^20 voxel - 1 along x: points with x in [-1.5, 1.5] voxel land in the cells 2^20 - 3 .. 2^20, the last
         of which is beyond the range; one row is the point with cell 2^20 - 1 exactly and one the point with cell 2^20 exactly
      4  a generic pose, n points, one of them NaN and one infinite
      5  fragment 1's points again under fragment 1's pose: every voxel of fragment 1 is seen by two fragments"""
    rs = np.random.RandomState(seed)
    v = 0.125
    lat = np.stack(np.meshgrid(*[np.arange(-4, 5)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)[rs.permutation(729)[:120]] * v
    f0 = np.concatenate([lat, lat[::3], rs.rand(n, 3) * 2 - 1]).astype(f32)
    f1 = (rs.rand(n, 3) * 2 - 1).astype(f32)
    f2 = (rs.rand(50, 3)).astype(f32)
    f3 = np.concatenate([np.stack([rs.rand(60) * 3 * v - 1.5 * v, rs.rand(60), rs.rand(60)], axis=1), [[0.0, 0.5, 0.5], [v, 0.5, 0.5]]]).astype(f32)
    f4 = (rs.rand(n, 3) * 2 - 1).astype(f32)
    f4[7, 1] = np.nan
    f4[11, 2] = np.inf
    X1 = pose(rs.randn(3), 50.0, rs.randn(3) * 0.2)
    X2 = pose(rs.randn(3), 20.0, rs.randn(3))
    X2[1, 2] = np.nan
    X3 = pose([0, 0, 1], 0.0, [((1 << 20) - 1) * v, 0.0, 0.0])
    X4 = pose(rs.randn(3), 130.0, rs.randn(3) * 0.2)
    clouds = [f0, f1, f2, f3, f4, f1.copy()]
    T = np.stack([np.eye(4), X1, X2, X3, X4, X1])[:, :3, :]
    src = np.concatenate(clouds)
    nrm = rs.randn(src.shape[0], 3).astype(f32)
    nrm[5] = np.nan
    nrm[40:44] = 0.0
    return {"clouds": clouds, "soff": soff_of(clouds), "src": src, "T": np.ascontiguousarray(T), "nrm": nrm, "voxel": v}
