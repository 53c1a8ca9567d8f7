"""numpy restatement of include/yoho_salient.h (yoho_iss_saliency, yoho_disk_sample_prio) and the scene its tests run on (helper of
tests/test_salient_cpu.py and tests/test_gpu_salient.py, not a conftest).

  saliency_ref           neighbours by plane_ref.neighbour_mask (yoho_nn_within's f32 predicate), the one-pass f64 covariance about the
                         point divided by the count, np.linalg.eigh, the clamp at 0
  eig_exact              the same covariance and its eigenvalues at 80 digits (mpmath) for one point
  prio_of                the eligibility rule in f64 on (eig, count) -> the f32 priorities, NaN for the ineligible rows
  ord_of / key64_of_row  PRIORITY on Python integers; ord32 / key64 the same on arrays (uint64)
  disk_prio_greedy_ref   THE SET: one sequential pass over the undecided rows in ascending key64 order (cluster_ref.neighbours_ref's
                         neighbours)
  disk_prio_rounds_ref   ROUNDS with START: synchronous rounds over disk_ref.lower_key_edges' pairs, re-oriented by key64, from state0
  crease_scene           three orthogonal planes and a box on one of them, with the segments of their creases
"""
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_ref as CL  # noqa: E402
import disk_ref as DR  # noqa: E402
import plane_ref as PR  # noqa: E402
import refine_ref as RR  # noqa: E402

f32, f64 = np.float32, np.float64
MAX_ROUNDS = 64                                                            # YOHO_SALIENT_MAX_ROUNDS
QNAN = 0x7FC00000
# (i, seed, prio bits) -> key64, as include/yoho_salient.h prints them
HEADER_VECTORS = (((0, 0, 0x3F800000), 0x407FFFFF00000000), ((1, 0, 0xBF800000), 0xBF800000688990C0),
                  ((12345, 0, 0x7FC00000), 0xFFFFFFFF912EFCF7), ((2048, 12345, 0x00000000), 0x7FFFFFFF72C087EC))


# ---- saliency --------------------------------------------------------------------------------------------------------------------------
def saliency_ref(pts, radius, chunk=256):
    """-> dict(count (N) int32, eig (N,3) f64 ascending and clamped at 0, (0, 0, 0) where count is 0, trace (N) f64 of the covariance).
    plane_ref.normals_ref's walk: rows in ascending x, a chunk looks at the points whose x lies within 1.001 radius of its range."""
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    N = pts.shape[0]
    g2 = RR.gate2_of(radius)
    count = np.zeros((N,), np.int32)
    C = np.zeros((N, 3, 3), f64)
    rows = np.nonzero(np.isfinite(pts).all(axis=1))[0]
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
        m = PR.neighbour_mask(pts[r], pts[cand], g2)
        d = np.where(m[:, :, None], pts[cand].astype(f64)[None, :, :] - pts[r].astype(f64)[:, None, :], 0.0)
        n = m.sum(axis=1)
        S1 = d.sum(axis=1)
        S2 = np.einsum("mki,mkj->mij", d, d)
        count[r] = n
        nn = np.maximum(n, 1).astype(f64)[:, None, None]
        C[r] = np.where((n > 0)[:, None, None], (S2 - S1[:, :, None] * S1[:, None, :] / nn) / nn, 0.0)
    eig = np.maximum(np.linalg.eigh(C)[0], 0.0)
    return {"count": count, "eig": np.sort(eig, axis=1), "trace": np.trace(C, axis1=1, axis2=2)}


def eig_exact(pts, i, radius):
    """point i's covariance (S2 - S1 S1^T / n) / n and its eigenvalues at 80 digits -> dict(lam (3 mp, ascending), count, trace (float))"""
    import mpmath as mp
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    m = PR.neighbour_mask(pts[i:i + 1], pts, RR.gate2_of(radius))[0]
    nb = pts[m].astype(f64)
    with mp.workdps(PR.DPS):
        p = [mp.mpf(float(x)) for x in pts[i].astype(f64)]
        d = [[mp.mpf(float(x)) - p[k] for k, x in enumerate(row)] for row in nb]
        n = len(d)
        S1 = [mp.fsum(r[k] for r in d) for k in range(3)]
        C = mp.matrix(3, 3)
        for a in range(3):
            for b in range(3):
                C[a, b] = (mp.fdot([r[a] for r in d], [r[b] for r in d]) - S1[a] * S1[b] / n) / n
        E = mp.eigsy(C, eigvals_only=True)
        lam = sorted(max(E[k], mp.mpf(0)) for k in range(3))
        return {"lam": lam, "count": n, "trace": float(C[0, 0] + C[1, 1] + C[2, 2])}


def exact_error(value, exact):
    """|value - exact| of a float against an mp number, taken at 80 digits -> float"""
    import mpmath as mp
    with mp.workdps(PR.DPS):
        return float(abs(mp.mpf(float(value)) - exact))


def eig_bound(numpy_worst, count, trace):
    """the bound of the issue on an eigenvalue of the device against the exact one: the larger of 8 x numpy's own worst error and the
    Weyl figure 4 n 2^-53 trace of an n-term f64 sum"""
    return max(8.0 * numpy_worst, 4.0 * count * 2.0 ** -53 * trace)


def prio_of(eig, count, min_nbrs=5, gamma21=0.975, gamma32=0.975):
    """the eligibility rule on eig (N,3) f64 and count (N) -> prio (N) f32: l1 rounded once where eligible, the quiet NaN elsewhere"""
    eig = np.asarray(eig, f64).reshape(-1, 3)
    l1, l2, l3 = eig[:, 0], eig[:, 1], eig[:, 2]
    elig = (np.asarray(count) >= min_nbrs) & (l2 < f64(gamma21) * l3) & (l1 < f64(gamma32) * l2)
    out = np.full((eig.shape[0],), QNAN, np.uint32).view(f32)
    with np.errstate(under="ignore", over="ignore"):
        out[elig] = l1[elig].astype(f32)
    return out


# ---- the key ---------------------------------------------------------------------------------------------------------------------------
def ord_of(bits):
    """ord on the 32 bits of an f32, as a Python integer"""
    bits = int(bits) & 0xFFFFFFFF
    if (bits >> 23) & 0xFF == 0xFF and bits & 0x7FFFFF:
        return 0
    return (~bits) & 0xFFFFFFFF if bits >> 31 else bits | 0x80000000


def key64_of_row(i, seed, p):
    """key64 of row i with priority p (a float, rounded to f32) on Python integers, with disk_ref.key_of_row's mixer"""
    bits = struct.unpack("<I", struct.pack("<f", float(p)))[0] if not isinstance(p, (int, np.integer)) else int(p)
    return (((~ord_of(bits)) & 0xFFFFFFFF) << 32) | DR.key_of_row(i, seed)


def ord32(prio):
    """ord on an f32 array -> uint64 holding uint32 values"""
    prio = np.ascontiguousarray(prio, f32)
    b = prio.view(np.uint32).astype(np.uint64)
    m = np.uint64(0xFFFFFFFF)
    o = np.where(b >> np.uint64(31) != 0, ~b & m, b | np.uint64(0x80000000))
    return np.where(np.isnan(prio), np.uint64(0), o)


def key64(prio, seed=0):
    """key64 of rows 0 .. N-1 -> (N) uint64, with disk_ref.mix32 (the vectorised mixer)"""
    prio = np.ascontiguousarray(prio, f32).reshape(-1)
    n = prio.shape[0]
    lo = DR.mix32(np.arange(n, dtype=np.uint64) ^ np.uint64(int(seed) & 0xFFFFFFFF))
    return ((~ord32(prio) & np.uint64(0xFFFFFFFF)) << np.uint64(32)) | lo


# ---- the set: a sequential pass ------------------------------------------------------------------------------------------------------------
def start_state(pts, state0=None):
    """START: 0 for a finite row and 2 for every other; with state0 its bytes, a non-finite row handed in as 0 set to 2"""
    fin = np.isfinite(np.ascontiguousarray(pts, f32).reshape(-1, 3)).all(axis=1)
    if state0 is None:
        return np.where(fin, 0, 2).astype(np.uint8)
    s = np.array(state0, np.uint8)
    s[(s == 0) & ~fin] = 2
    return s


def disk_prio_greedy_ref(pts, radius, prio, seed=0, state0=None):
    """-> dict(state (N) uint8, kept = the rows the pass kept in ascending key64 order (int64), n = rows with state 1).  A row undecided
    at the start is kept iff no neighbour that precedes it has state 1 - kept by the pass, or handed in so."""
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    nb = CL.neighbours_ref(pts, radius)
    key = np.array([key64_of_row(i, seed, p) for i, p in enumerate(np.ascontiguousarray(prio, f32).view(np.uint32))], dtype=object)
    state = start_state(pts, state0)
    todo = [i for i in np.nonzero(state == 0)[0]]
    todo.sort(key=lambda i: key[i])
    kept = []
    for i in todo:
        j = nb[i][0]
        if any(state[t] == 1 and key[t] < key[i] for t in j):
            state[i] = 2
        else:
            state[i] = 1
            kept.append(i)
    return {"state": state, "kept": np.asarray(kept, np.int64), "n": int((state == 1).sum())}


# ---- the rounds ------------------------------------------------------------------------------------------------------------------------------
def pairs(pts, radius):
    """every unordered pair of neighbours once -> (a, b) int64 (disk_ref.lower_key_edges' pairs, whose orientation is not used)"""
    return DR.lower_key_edges(pts, radius, 0)


def preceding_edges(pts, radius, prio, seed=0, pr=None):
    """-> (a, b) int64: every ordered pair of neighbours with key64(b) < key64(a)"""
    a, b = pairs(pts, radius) if pr is None else pr
    k = key64(prio, seed)
    swap = k[a] < k[b]
    return np.where(swap, b, a), np.where(swap, a, b)


def disk_prio_rounds_ref(pts, radius, prio, seed=0, max_rounds=None, state0=None, pr=None):
    """-> states (R + 1, N) uint8: states[0] the start state, states[r] the state after round r; R = the rounds that ran - until no row
    is undecided, or max_rounds of them"""
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    n = pts.shape[0]
    a, b = preceding_edges(pts, radius, prio, seed, pr)
    s = start_state(pts, state0)
    out = [s]
    while (s == 0).any() and (max_rounds is None or len(out) <= max_rounds):
        has_kept = np.bincount(a[s[b] == 1], minlength=n) > 0
        has_open = np.bincount(a[s[b] == 0], minlength=n) > 0
        new = np.where(has_kept, 2, np.where(has_open, 0, 1)).astype(np.uint8)
        s = np.where(s == 0, new, s)
        out.append(s)
    return np.stack(out)


def assert_is_the_set(pts, radius, prio, seed, state, state0=None, pr=None):
    """no two rows kept by the thinning are neighbours, and every row undecided at the start is kept or has a kept neighbour that
    precedes it; a row decided at the start keeps its byte"""
    pts = np.ascontiguousarray(pts, f32).reshape(-1, 3)
    n = pts.shape[0]
    s0 = start_state(pts, state0)
    a, b = preceding_edges(pts, radius, prio, seed, pr)
    und = s0 == 0
    assert np.array_equal(state[~und], s0[~und]) and ((state[und] == 1) | (state[und] == 2)).all()
    new = und & (state == 1)
    assert not (new[a] & new[b]).any()
    lower_kept = np.bincount(a[state[b] == 1], minlength=n) > 0
    assert np.array_equal(new[und], ~lower_kept[und])


def tier_classes_ref(prio, tiers):
    """keypoints.tier_classes in numpy: the rank class tiers - 1 - floor(tiers * descending rank / eligible), equal responses ranked in
    row order; NaN for the ineligible rows"""
    prio = np.ascontiguousarray(prio, f32)
    elig = np.nonzero(~np.isnan(prio))[0]
    out = np.full(prio.shape, QNAN, np.uint32).view(f32)
    order = elig[np.argsort(-prio[elig].astype(f64), kind="stable")]
    rank = np.arange(len(elig), dtype=np.int64)
    out[order] = ((int(tiers) - 1) - (int(tiers) * rank) // max(len(elig), 1)).astype(f32)
    return out


def priorities(n, seed):
    """the priorities of the tests: random; random with half the values tied; +-0.0, +-inf and NaN mixed in; constant"""
    rs = np.random.RandomState((900 + int(seed)) % (1 << 32))
    rnd = rs.rand(n).astype(f32)
    tied = np.where(rs.rand(n) < 0.5, f32(0.5), rs.rand(n)).astype(f32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0], f32)
    mixed = np.where(rs.rand(n) < 0.5, special[rs.randint(0, len(special), n)], rs.randn(n)).astype(f32)
    return {"random": rnd, "tied": tied, "special": mixed, "constant": np.full((n,), 0.25, f32)}


# ---- the scene -------------------------------------------------------------------------------------------------------------------------------
BOX = ((0.4, 0.7), (0.35, 0.65), (0.0, 0.2))                              # on the plane z = 0


def _faces():
    """(origin, u, v) of every rectangle of the scene: the three unit squares on the coordinate planes, the box's four sides and top"""
    (x0, x1), (y0, y1), (z0, z1) = BOX
    o = np.array
    return [(o([0., 0, 0]), o([1., 0, 0]), o([0., 1, 0])), (o([0., 0, 0]), o([1., 0, 0]), o([0., 0, 1])), (o([0., 0, 0]), o([0., 1, 0]), o([0., 0, 1])),
            (o([x0, y0, z0]), o([x1 - x0, 0, 0]), o([0, 0, z1 - z0])), (o([x0, y1, z0]), o([x1 - x0, 0, 0]), o([0, 0, z1 - z0])),
            (o([x0, y0, z0]), o([0, y1 - y0, 0]), o([0, 0, z1 - z0])), (o([x1, y0, z0]), o([0, y1 - y0, 0]), o([0, 0, z1 - z0])),
            (o([x0, y0, z1]), o([x1 - x0, 0, 0]), o([0, y1 - y0, 0]))]


def crease_segments():
    """the segments where two faces meet: the three axes of the corner and the twelve edges of the box -> (15, 2, 3) f64"""
    (x0, x1), (y0, y1), (z0, z1) = BOX
    seg = [((0, 0, 0), (1, 0, 0)), ((0, 0, 0), (0, 1, 0)), ((0, 0, 0), (0, 0, 1))]
    for z in (z0, z1):
        seg += [((x0, y0, z), (x1, y0, z)), ((x0, y1, z), (x1, y1, z)), ((x0, y0, z), (x0, y1, z)), ((x1, y0, z), (x1, y1, z))]
    seg += [((x, y, z0), (x, y, z1)) for x in (x0, x1) for y in (y0, y1)]
    return np.array(seg, f64)


def crease_distance(p):
    """p (m,3) -> (m) f64: the distance to the nearest crease segment"""
    p = np.asarray(p, f64)
    best = np.full((p.shape[0],), np.inf)
    for s0, s1 in crease_segments():
        d = s1 - s0
        t = np.clip(((p - s0) @ d) / (d @ d), 0.0, 1.0)
        best = np.minimum(best, np.linalg.norm(p - (s0 + t[:, None] * d), axis=1))
    return best


def crease_scene(n, seed):
    """n points drawn uniformly by area over the faces of the scene (the part of z = 0 under the box left out), jittered by a normal
    deviate of 0.1 of the point spacing sqrt(area / n) in every coordinate -> (pts (n,3) f64, spacing)"""
    rs = np.random.RandomState(7000 + seed)
    faces = _faces()
    area = np.array([np.linalg.norm(np.cross(u, v)) for _, u, v in faces])
    (x0, x1), (y0, y1), _ = BOX
    total = area.sum() - (x1 - x0) * (y1 - y0)
    spacing = float(np.sqrt(total / n))
    out = []
    while sum(len(o) for o in out) < n:
        f = rs.choice(len(faces), size=n, p=area / area.sum())
        uv = rs.rand(n, 2)
        o = np.stack([fc[0] for fc in faces])[f] + uv[:, :1] * np.stack([fc[1] for fc in faces])[f] + uv[:, 1:] * np.stack([fc[2] for fc in faces])[f]
        under = (f == 0) & (o[:, 0] > x0) & (o[:, 0] < x1) & (o[:, 1] > y0) & (o[:, 1] < y1)
        out.append(o[~under])
    pts = np.concatenate(out)[:n]
    return np.ascontiguousarray(pts + rs.randn(n, 3) * (0.1 * spacing)), spacing
