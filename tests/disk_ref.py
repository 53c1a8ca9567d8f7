"""numpy restatement of include/yoho_disk.h (yoho_disk_sample), twice, and the clouds its tests run on.

  disk_greedy_ref       THE SET as the header defines it: one sequential pass over the finite rows in ascending key order, a row kept
                        iff none of its neighbours is kept already; the neighbours are cluster_ref.neighbours_ref's - keypoints_ref.dist2_ref
                        in float32 on every pair a window on x cannot rule out (clean_ref.knn_within_ref's candidates)
  disk_rounds_ref       ROUNDS as the header defines them: the synchronous rounds on an edge list of its own - a float64 cKDTree (or, without
                        scipy, every pair) proposes the pairs within 1.001 radius, the float32 distance written out here decides - and
                        the state after every round.  The two share no code (not the keys either: mix32 / key_of_row)
  chain                 the adversarial cloud: a line of points whose keys ascend along it, one decision per round
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_ref as CL  # noqa: E402

f32, f64 = np.float32, np.float64
MAX_ROUNDS = 64                                                            # YOHO_DISK_MAX_ROUNDS
HEADER_VECTORS = (((0, 0), 0x00000000), ((1, 0), 0x688990C0), ((12345, 0), 0x912EFCF7), ((2048, 12345), 0x72C087EC))


def mix32(x):
    """the header's mixer on an array of integers, modulo 2^32 -> uint64 holding uint32 values"""
    m = np.uint64(0xFFFFFFFF)
    x = np.asarray(x).astype(np.uint64) & m
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & m
    return x ^ (x >> np.uint64(16))


def keys(n, seed=0):
    """key(i) = mix32(i ^ seed) of rows 0 .. n-1 -> (n) int64"""
    return mix32(np.arange(n, dtype=np.uint64) ^ np.uint64(int(seed) & 0xFFFFFFFF)).astype(np.int64)


# ---- the set: a sequential pass ------------------------------------------------------------------------------------------------------------
def disk_greedy_ref(pts, radius, seed=0):
    """-> dict(state (N) uint8 = 1 kept / 2 dropped or not finite, kept = the kept rows in ascending key order (int64), n = their number)"""
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    n = pts.shape[0]
    nb = CL.neighbours_ref(pts, radius)
    key = keys(n, seed)
    state = np.full((n,), 2, np.uint8)
    finite = np.isfinite(pts).all(axis=1)
    kept = []
    for i in np.argsort(key, kind="stable"):
        if finite[i] and not (state[nb[i][0]] == 1).any():                 # those of higher key are not decided yet: still 2
            state[i] = 1
            kept.append(i)
    return {"state": state, "kept": np.asarray(kept, np.int64), "n": len(kept)}


# ---- the rounds: an edge list of its own ---------------------------------------------------------------------------------------------------
def key_of_row(i, seed):
    """the mixer once more, on Python integers"""
    x = (int(i) ^ int(seed)) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def lower_key_edges(pts, radius, seed=0):
    """-> (a, b) int64: every ordered pair of neighbours with key(b) < key(a)"""
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    fin = np.nonzero(np.isfinite(pts).all(axis=1))[0]
    p64 = pts[fin].astype(f64)
    try:
        from scipy.spatial import cKDTree
        pr = cKDTree(p64).query_pairs(float(radius) * 1.001, output_type="ndarray").astype(np.int64).reshape(-1, 2)
    except ImportError:
        rows = []
        for i in range(len(fin) - 1):
            d = np.sqrt(((p64[i + 1:] - p64[i]) ** 2).sum(1))
            j = np.nonzero(d <= float(radius) * 1.001)[0] + i + 1
            rows.append(np.stack([np.full_like(j, i), j], 1))
        pr = np.concatenate(rows).astype(np.int64) if rows else np.zeros((0, 2), np.int64)
    a, b = fin[pr[:, 0]], fin[pr[:, 1]]
    with np.errstate(all="ignore"):
        dx = pts[a, 0] - pts[b, 0]
        dy = pts[a, 1] - pts[b, 1]
        dz = pts[a, 2] - pts[b, 2]
        d2 = (dx * dx + dy * dy) + dz * dz                                   # float32 throughout, one rounding per operation
        assert d2.dtype == f32
        gate2 = f32(radius) * f32(radius)
        inside = d2 < gate2
    a, b = a[inside], b[inside]
    k = np.array([key_of_row(i, seed) for i in range(pts.shape[0])], np.int64)
    swap = k[a] < k[b]
    return np.where(swap, b, a), np.where(swap, a, b)


def disk_rounds_ref(pts, radius, seed=0, max_rounds=None, state0=None, edges=None):
    """-> states (R + 1, N) uint8: states[0] the state at entry (state0, or 0 for a finite row and 2 otherwise), states[r] the state
    after round r; R = the rounds that ran - until no row is undecided, or max_rounds of them"""
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    n = pts.shape[0]
    a, b = lower_key_edges(pts, radius, seed) if edges is None else edges
    s = np.where(np.isfinite(pts).all(axis=1), 0, 2).astype(np.uint8) if state0 is None else np.array(state0, np.uint8)
    out = [s]
    while (s == 0).any() and (max_rounds is None or len(out) <= max_rounds):
        has_kept = np.bincount(a[s[b] == 1], minlength=n) > 0
        has_open = np.bincount(a[s[b] == 0], minlength=n) > 0
        new = np.where(has_kept, 2, np.where(has_open, 0, 1)).astype(np.uint8)
        s = np.where(s == 0, new, s)
        out.append(s)
    return np.stack(out)


def n_out_of(states):
    """the entry's n_out for a call that went through `states`"""
    return np.array([(states[-1] == 1).sum(), len(states) - 1, (states[-1] == 0).sum()], np.int32)


# ---- properties ----------------------------------------------------------------------------------------------------------------------------
def assert_is_the_set(pts, radius, seed, state, edges=None):
    """state holds THE SET: finite rows are 1 or 2, the others 2; no two kept rows are neighbours; every finite row is kept or has a
    kept neighbour; and a row is kept iff no neighbour of lower key is - the property that makes the set unique"""
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    n = pts.shape[0]
    a, b = lower_key_edges(pts, radius, seed) if edges is None else edges
    fin = np.isfinite(pts).all(axis=1)
    kept = state == 1
    assert ((state == 1) | (state == 2)).all() and not kept[~fin].any()
    assert not (kept[a] & kept[b]).any()
    near_kept = (np.bincount(a[kept[b]], minlength=n) + np.bincount(b[kept[a]], minlength=n)) > 0
    assert (kept | near_kept)[fin].all()
    lower_kept = np.bincount(a[kept[b]], minlength=n) > 0
    assert np.array_equal(kept[fin], ~lower_kept[fin])


def select_disk_ref(pc, radius, nkpts=None, voxel=None, seed=0):
    """yoho_amd.keypoints.select_disk without a filter: cloud indices in ascending key order of the candidate rows, cut at nkpts
    -> (indices, the number kept before the cut)"""
    sel = np.arange(len(pc), dtype=np.int64) if voxel is None else CL.KR.voxel_first_ref(pc, voxel)
    pts = np.asarray(pc, dtype=f64)[sel].astype(f32)
    kept = disk_greedy_ref(pts, radius, seed)["kept"]
    return sel[kept if nkpts is None else kept[:nkpts]], len(kept)


def coverage(p, keys_):
    """the largest distance from a row of p to its nearest row of keys_ (float64; a figure, not a bit pattern)"""
    p, keys_ = np.asarray(p, f64), np.asarray(keys_, f64)
    try:
        from scipy.spatial import cKDTree
        return float(cKDTree(keys_).query(p)[0].max())
    except ImportError:
        return CL.KR.coverage_radius_ref(p, keys_)


# ---- clouds --------------------------------------------------------------------------------------------------------------------------------
def chain(n, radius, seed=0, spacing=0.9):
    """n points `spacing` radius apart on a line, chain position t at row argsort(key)[t]: the keys ascend along the chain, position 0
    is decided by round 1 and position t by round t + 1 -> (pts (n,3) f32, row_of (n) int64: the row of chain position t)"""
    row_of = np.argsort(keys(n, seed), kind="stable")
    pts = np.zeros((n, 3), f32)
    pts[row_of, 0] = (np.arange(n) * (spacing * float(radius))).astype(f32)
    pts[:, 1], pts[:, 2] = f32(0.25), f32(-0.5)
    return pts, row_of


SURFACE_AREA = 6.0                                                        # of synth.surface_cloud's unit-extent surface, roughly: sizes radius_for


def radius_for(n, target):
    """the radius inside which a row of mixed(n, .) has about `target` other rows: target = density pi r^2 on a surface"""
    return float(np.sqrt(target * SURFACE_AREA / (np.pi * max(n, 8))))


def mixed(n, r, seed=0):
    """cluster_ref.mixed_cloud's recipe for any n up to a few thousand: n rows, shuffled - surface points, two clumps of spread r / 6,
    copies of one surface point, and a few far points 1e6 r and 3e6 r away, the latter in the grid's clamped cells"""
    from yoho_amd import synth
    rs = np.random.RandomState(200 + seed)
    far = np.array([[1e6 * r, 0, 0], [3e6 * r, 0, 0], [3e6 * r, 0.25 * r, 0], [-3e6 * r, 3e6 * r, -1e6 * r]])[:0 if n < 2 else min(4, 1 + n // 64)]
    n_dup, n_clump = n // 32, n // 16
    surf = synth.surface_cloud(4000, seed)[:n - len(far) - n_dup - n_clump]
    centre = np.array([[0.3, 1.5, 0.2], [1.6, 0.1, 0.9]])
    clump = centre[np.arange(n_clump) % 2] + rs.randn(n_clump, 3) * (r / 6)
    pts = np.concatenate([surf, clump, np.tile(surf[:1], (n_dup, 1)), far])
    assert pts.shape == (n, 3)
    return np.ascontiguousarray(pts[rs.permutation(n)].astype(f32))


def gate_line(n, step=0.5):
    line = np.zeros((n, 3), f32)
    line[:, 0] = step * np.arange(n)
    return line
