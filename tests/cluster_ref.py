"""numpy restatement of include/yoho_cluster.h (yoho_dbscan), twice, and the cloud the feature is motivated by.

  dbscan_ref            the contract's own arithmetic: keypoints_ref.dist2_ref in float32 on every pair of rows a window on x cannot
                        rule out (clean_ref.knn_within_ref's neighbourhood), a union-find of its own over the edges between core rows,
                        the border rows by smallest (d2, j), the clusters numbered by lowest core row
  dbscan_independent    scipy's cKDTree in float64 and csgraph.connected_components: shares no code with the first and no arithmetic
                        with the device, so the two are compared only on clouds on which no pair distance lies close to eps
                        (clean_ref.separated_cloud asserts it), and - the order in which a library visits border points being its own
                        affair - on the core set, the partition of the core rows, the noise set and the admissible labels of a border row
  keep_large_ref        yoho_amd.cluster.keep_large on a dbscan_ref result
  clump_cloud           synth.surface_cloud plus stray clumps: the strays the filters of yoho_clean.h keep
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import keypoints_ref as KR  # noqa: E402
import refine_ref as RR  # noqa: E402

f32, f64 = np.float32, np.float64


# ---- the contract's arithmetic -------------------------------------------------------------------------------------------------------------
def neighbours_ref(pts, eps):
    """-> list over the rows of (j ascending int64, d2 f32): the rows j != i with d2 < gate2, yoho_knn_within's candidates with
    skip_same_row; a row with a NaN or infinite coordinate has none and is nobody's"""
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    n = pts.shape[0]
    g2 = RR.gate2_of(eps)
    none = (np.zeros((0,), np.int64), np.zeros((0,), f32))
    out = [none] * n
    window = 1e-15 < float(eps) < 1e15
    if window:
        tx = pts[:, 0].astype(f64)
        order = np.argsort(tx, kind="stable")             # NaN last
        txs = tx[order]
        reach = float(eps) * 1.001
    every = np.arange(n)
    with np.errstate(all="ignore"):
        for i in np.nonzero(np.isfinite(pts).all(axis=1))[0]:
            if window:
                lo = np.searchsorted(txs, float(pts[i, 0]) - reach, side="left")
                hi = np.searchsorted(txs, float(pts[i, 0]) + reach, side="right")
                cand = np.sort(order[lo:hi])
            else:
                cand = every
            cand = cand[cand != i]
            if cand.size == 0:
                continue
            d = KR.dist2_ref(pts[cand], pts[i])
            inside = d < g2                                # false for a NaN, and for d2 == gate2
            out[i] = (cand[inside].astype(np.int64), d[inside])
    return out


def _find(parent, x):
    r = x
    while parent[r] != r:
        r = parent[r]
    while parent[x] != r:
        parent[x], x = r, parent[x]
    return r


def dbscan_ref(pts, eps, min_pts):
    """-> dict(labels (N) int32, count (N) int32, core (N) uint8, sizes (N) int32, n (3) int32 = clusters, core rows, noise rows)"""
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    n = pts.shape[0]
    assert n >= 1 and min_pts >= 1 and np.isfinite(eps) and eps > 0
    nb = neighbours_ref(pts, eps)
    count = np.array([len(j) for j, _ in nb], np.int32)
    finite = np.isfinite(pts).all(axis=1)
    core = finite & (count.astype(np.int64) + 1 >= min_pts)
    parent = list(range(n))
    for i in np.nonzero(core)[0]:
        j = nb[i][0]
        for k in j[(j < i) & core[j]]:
            a, b = _find(parent, int(i)), _find(parent, int(k))
            if a != b:
                parent[max(a, b)] = min(a, b)              # the root is the lowest row of its tree
    root = np.full((n,), -1, np.int64)
    for i in np.nonzero(core)[0]:
        root[i] = _find(parent, int(i))
    for i in np.nonzero(~core & (count > 0))[0]:
        j, d = nb[i]
        c = core[j]
        if c.any():
            j, d = j[c], d[c]
            root[i] = root[j[np.lexsort((j, d))[0]]]       # the core neighbour with the smallest (d2, j)
    roots = np.nonzero(core & (root == np.arange(n)))[0]   # ascending: the numbering
    rank = np.full((n,), -1, np.int64)
    rank[roots] = np.arange(roots.size)
    labels = np.where(root >= 0, rank[np.maximum(root, 0)], -1).astype(np.int32)
    sizes = np.zeros((n,), np.int32)
    sizes[:roots.size] = np.bincount(labels[labels >= 0], minlength=roots.size)[:roots.size] if roots.size else 0
    return {"labels": labels, "count": count, "core": core.astype(np.uint8), "sizes": sizes,
            "n": np.array([roots.size, int(core.sum()), int((labels < 0).sum())], np.int32)}


def keep_large_ref(ref, min_size=None, largest=None):
    """yoho_amd.cluster.keep_large's keep on a dbscan_ref result"""
    assert (min_size is None) != (largest is None)
    labels, sizes = ref["labels"], ref["sizes"]
    if largest is None:
        big = sizes >= min_size
    else:
        order = np.lexsort((np.arange(sizes.size), -sizes.astype(np.int64)))      # most members first, ties: the lower id
        big = np.zeros(sizes.shape, bool)
        big[order[:largest]] = True
        big &= sizes > 0
    return (labels >= 0) & big[np.maximum(labels, 0)]


# ---- the independent restatement -----------------------------------------------------------------------------------------------------------
def dbscan_independent(pts, eps, min_pts):
    """float64, finite rows only -> dict(core (N) bool, comp (N) int64: the connected component of a core row among the core rows, -1
    for the others, noise (N) bool, border: {row: the core rows within eps of it} for the rows that are neither)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    p = np.asarray(pts, f64).reshape(-1, 3)
    n = p.shape[0]
    tree = cKDTree(p)
    pairs = tree.query_pairs(float(eps), output_type="ndarray")          # i < j, distance <= eps; no distance is near eps here
    count = np.bincount(pairs.reshape(-1), minlength=n)
    core = count + 1 >= min_pts
    both = core[pairs[:, 0]] & core[pairs[:, 1]]
    e = pairs[both]
    ncomp, comp = connected_components(coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n)), directed=False)
    comp = np.where(core, comp, -1).astype(np.int64)
    border = {}
    for a, b in pairs[core[pairs[:, 0]] != core[pairs[:, 1]]]:
        c, o = (a, b) if core[a] else (b, a)
        border.setdefault(int(o), []).append(int(c))
    noise = ~core
    noise[list(border)] = False
    return {"core": core, "comp": comp, "noise": noise, "border": {k: np.array(sorted(v)) for k, v in border.items()}}


def assert_agree(ref, ind):
    """dbscan_ref's result against dbscan_independent's: the core set, the partition of the core rows up to renaming, the noise set,
    and every border row in the cluster of one of its core neighbours"""
    core = ref["core"].astype(bool)
    assert np.array_equal(core, ind["core"])
    assert np.array_equal(ref["labels"] < 0, ind["noise"])
    a, b = ref["labels"][core], ind["comp"][core]
    pairs = set(zip(a.tolist(), b.tolist()))
    assert len(pairs) == len(set(a.tolist())) == len(set(b.tolist())) == int(ref["n"][0])      # a bijection of the names
    for i, nbrs in ind["border"].items():
        assert not core[i] and ref["labels"][i] in ref["labels"][nbrs], i
    assert len(ind["border"]) == int((~core & (ref["labels"] >= 0)).sum())


# ---- clouds ----------------------------------------------------------------------------------------------------------------------------------
def clump_cloud(seed, n=20000, centres=20, per_clump=30, sigma=0.004, clear=0.15):
    """the motivating scan: synth.surface_cloud(n, seed), then stray clumps - `centres` centres uniform in [-0.2, 1.4]^3 from
    RandomState(7 + seed), those farther than `clear` from every surface point kept (4 for seed 0, 12 for seed 1), per_clump points
    N(0, sigma^2) around each -> (pts (n + clump points,3) f32, clump (rows) int64: the clump of a row, -1 for a surface row)"""
    from yoho_amd import synth
    surf = synth.surface_cloud(n, seed)
    rs = np.random.RandomState(7 + seed)
    c = rs.rand(centres, 3) * 1.6 - 0.2
    far = np.array([np.sqrt(((surf - x) ** 2).sum(-1).min()) > clear for x in c])
    c = c[far]
    blobs = [x + rs.randn(per_clump, 3) * sigma for x in c]
    pts = np.concatenate([surf] + blobs).astype(f32)
    clump = np.concatenate([np.full((len(surf),), -1, np.int64)] + [np.full((per_clump,), k, np.int64) for k in range(len(c))])
    return np.ascontiguousarray(pts), clump


_MOTIVATING = {}


def motivating(seed):
    """clump_cloud(seed) with dbscan_ref(eps = 0.04, min_pts = 4) of it, computed once -> (pts, clump, ref)"""
    if seed not in _MOTIVATING:
        pts, clump = clump_cloud(seed)
        _MOTIVATING[seed] = (pts, clump, dbscan_ref(pts, 0.04, 4))
    return _MOTIVATING[seed]


def mixed_cloud(n, r, seed=0):
    """n rows, shuffled: surface points about r apart, two clumps, copies of one surface point, and a few far points - 1e6 r and
    3e6 r away, the latter in the grid's clamped cells, two of them neighbours of each other"""
    from yoho_amd import synth
    rs = np.random.RandomState(100 + seed)
    far = np.array([[1e6 * r, 0, 0], [3e6 * r, 0, 0], [3e6 * r, 0.25 * r, 0], [-3e6 * r, 3e6 * r, -1e6 * r]])[:0 if n < 2 else min(4, 1 + n // 64)]
    n_dup, n_clump = n // 16, n // 8
    surf = synth.surface_cloud(1200, seed)[:n - len(far) - n_dup - n_clump]
    centre = np.array([[0.3, 1.5, 0.2], [1.6, 0.1, 0.9]])
    clump = centre[np.arange(n_clump) % 2] + rs.randn(n_clump, 3) * (r / 6)
    pts = np.concatenate([surf, clump, np.tile(surf[:1], (n_dup, 1)), far])
    assert pts.shape == (n, 3)
    return np.ascontiguousarray(pts[rs.permutation(n)].astype(f32))


def snake(n, eps, spacing=0.9, run=120, turn=4, z=0.0):
    """n points `spacing` eps apart along a planar polyline: `run` steps along +x, `turn` along +y, `run` along -x, ... in chain order.
    With spacing 0.9 a point's neighbours are the two beside it in the chain; with 0.48 the four."""
    step = np.zeros((n, 3))
    k = np.arange(1, n) - 1
    phase = k % (2 * (run + turn))
    step[1:, 0] = np.where(phase < run, 1.0, np.where((phase >= run + turn) & (phase < 2 * run + turn), -1.0, 0.0))
    step[1:, 1] = np.where(step[1:, 0] == 0, 1.0, 0.0)
    pts = np.cumsum(step * (spacing * eps), axis=0)
    pts[:, 2] = z
    return pts.astype(f32)


def snake_orders(n, seed=0):
    """{name: perm}: row k of the test cloud is chain point perm[k]"""
    rs = np.random.RandomState(seed)
    end = np.concatenate([[0], 1 + rs.permutation(n - 1)])
    mid = end.copy()
    mid[mid == n // 2], mid[0] = 0, n // 2
    return {"ascending": np.arange(n), "descending": np.arange(n)[::-1].copy(), "rotated": np.roll(np.arange(n), n // 2),
            "shuffled_row0_end": end, "shuffled_row0_middle": mid}


def two_snakes(eps, n=400, bridge=False, swap=False):
    """two chains 0.48 eps dense and 1.1 eps apart in z (`swap`: the upper one first), and optionally one point beside chain point 30
    of both, 0.901 eps from the lower and 0.960 eps from the upper one and more than eps from every other row
    -> (pts, rows of the lower chain, rows of the upper chain, the bridge's row or None)"""
    lo, up = snake(n, eps, spacing=0.48), snake(n, eps, spacing=0.48, z=1.1 * eps)
    parts = [up, lo] if swap else [lo, up]
    rows_lo, rows_up = (np.arange(n, 2 * n), np.arange(n)) if swap else (np.arange(n), np.arange(n, 2 * n))
    if bridge:
        b = lo[30].astype(f64) + np.array([0.0, -0.75 * eps, 0.5 * eps])
        parts.append(b[None].astype(f32))
    return np.ascontiguousarray(np.concatenate(parts)), rows_lo, rows_up, (2 * n if bridge else None)


def tie_cloud(swap=False):
    """integer lattice, eps = 1.2, min_pts = 5: two core points a = (0,0,0) and b = (2,0,0), each with five helpers one unit away that
    only it sees, and P = (1,0,0), one unit from both: P is a border point with equal d2 to two clusters
    -> (pts, row of a, row of b, row of P); swap exchanges the rows of a and b"""
    a, b = np.array([0, 0, 0]), np.array([2, 0, 0])
    ha = a + np.array([[-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    hb = b + np.array([[1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    first, second = (b, a) if swap else (a, b)
    pts = np.concatenate([ha, first[None], np.array([[1, 0, 0]]), hb, second[None]]).astype(f32)
    ra, rb = (12, 5) if swap else (5, 12)
    return pts, ra, rb, 6


def with_bad_rows(pts, seed=0, every=7):
    """pts with NaN and infinite rows sprinkled in -> (the new cloud, the rows the old ones went to)"""
    rs = np.random.RandomState(seed)
    n = len(pts)
    m = n + max(3, n // every)
    good = np.sort(rs.permutation(m)[:n])
    out = np.empty((m, 3), f32)
    bad = np.setdiff1d(np.arange(m), good)
    pick = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [np.nan] * 3, [-np.inf, np.inf, 0.1], [0.3, 0.2, -np.inf]], f32)
    out[bad] = pick[np.arange(len(bad)) % len(pick)]
    ok = rs.rand(len(bad)) < 0.5                                          # half of them keep two finite coordinates of a real point
    out[bad[ok], 1:] = pts[rs.randint(0, n, ok.sum()), 1:]
    out[bad[ok], 0] = np.nan
    out[good] = pts
    return out, good
