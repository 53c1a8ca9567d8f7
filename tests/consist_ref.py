"""The contracts of include/yoho_consist.h on the CPU (helper of tests/test_consist_cpu.py and tests/test_gpu_consist.py, not a conftest).

  graph_ref       the compatibility graph in the header's expression order, packed into uint64 words, and the row degrees
  unpack          the words back to a boolean matrix
  sc2_ref         the second-order scores s2 and, when asked, the matrix S itself
  consensus_ref   greedy seeds, the half-of-maximum rule, refine_ref.kabsch_step over each set
  planted_case    the seeded match lists of the tests: n_in matches about one transform, the rest anywhere in a 3 m cube
"""
import numpy as np

import refine_ref as RR

f64 = np.float64
IDENTITY = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)


def _len(k):
    """(M,3) -> (M,M): sqrt((dx dx + dy dy) + dz dz), every operation rounded to f64"""
    with np.errstate(all="ignore"):
        d = k[:, None, 0] - k[None, :, 0]
        s = d * d
        d = k[:, None, 1] - k[None, :, 1]
        s = s + d * d
        d = k[:, None, 2] - k[None, :, 2]
        return np.sqrt(s + d * d)


def compat_ref(k0, k1, tol, min_len=0.0):
    """-> C (M,M) bool; a comparison with a NaN is false"""
    k0, k1 = np.asarray(k0, f64).reshape(-1, 3), np.asarray(k1, f64).reshape(-1, 3)
    a, b = _len(k0), _len(k1)
    with np.errstate(invalid="ignore"):
        C = (np.abs(a - b) < f64(tol)) & (a >= f64(min_len)) & (b >= f64(min_len))
    np.fill_diagonal(C, False)
    return C


def pack(C):
    """C (M,M) bool -> (M, W) uint64: bit j % 64 of word j // 64"""
    M = C.shape[0]
    W = (M + 63) // 64
    padded = np.zeros((M, W * 64), np.uint8)
    padded[:, :M] = C
    return np.packbits(padded.reshape(M, W, 64), axis=2, bitorder="little").reshape(M, W, 8).copy().view("<u8").reshape(M, W).astype(np.uint64)


def unpack(bits, M):
    """(M, W) uint64 (or its int64 carrier) -> (M, W * 64) bool, the tail columns included"""
    b = np.ascontiguousarray(np.asarray(bits).view(np.uint64)).astype("<u8")
    return np.unpackbits(b.view(np.uint8).reshape(M, -1), axis=1, bitorder="little").astype(bool)


def graph_ref(k0, k1, tol, min_len=0.0):
    """-> (bits (M, W) uint64, deg (M) int32)"""
    C = compat_ref(k0, k1, tol, min_len)
    return pack(C), C.sum(axis=1).astype(np.int32)


def sc2_ref(bits, M, want_S=False):
    """-> s2 (M) int32 [, S (M,M) int64]: S[i][j] = C[i][j] ? |row_i & row_j| : 0, s2 = its row sums"""
    C = unpack(bits, M)[:, :M]
    Cf = C.astype(f64)                                        # 0 / 1 products summed in f64: exact far beyond M = 2^14
    S = (Cf @ Cf.T).astype(np.int64) * C                      # row_i & row_j counted over the columns: no symmetry assumed
    s2 = S.sum(axis=1).astype(np.int32)
    return (s2, S) if want_S else s2


def consensus_ref(k0, k1, bits, s2, K):
    """-> dict(T (K,3,4), seeds / sizes (K) int32, info (2) int32, Kc, sets (the Kc boolean member masks))"""
    k0, k1 = np.asarray(k0, f64).reshape(-1, 3), np.asarray(k1, f64).reshape(-1, 3)
    M = k0.shape[0]
    C = unpack(bits, M)[:, :M]
    Cf = C.astype(f64)
    s2 = np.asarray(s2, np.int64)
    alive = s2 >= 1
    T = np.tile(IDENTITY, (K, 1, 1))
    seeds, sizes = np.full((K,), -1, np.int32), np.zeros((K,), np.int32)
    sets = []
    for r in range(K):
        if not alive.any():
            break
        s = int(np.argmax(np.where(alive, s2, -1)))           # first maximum: the smallest index among equal scores
        seeds[r] = s
        alive[s] = False
        alive &= ~C[s]
        S = (Cf @ Cf[s]).astype(np.int64) * C[s]              # S[s][j], 0 off the seed's row
        smax = int(S[C[s]].max()) if C[s].any() else -1
        sel = C[s] & (2 * S >= smax)
        sel[s] = True
        n = int(sel.sum())
        sets.append(sel)
        Tr = RR.kabsch_step(k0, k1, sel) if n >= 3 else None
        if Tr is None:
            T[r] = np.nan
            sizes[r] = -n
        else:
            T[r] = Tr
            sizes[r] = n
    Kc = len(sets)
    return {"T": T, "seeds": seeds, "sizes": sizes, "info": np.array([Kc, M], np.int32), "Kc": Kc, "sets": sets}


_PLANTED = {}


def planted_case(M, n_in, seed):
    """M matches in a 3 m cube, the first n_in about one transform 90 degrees / 0.5 m from the identity with 1 cm of noise ->
    dict(k0, k1, T_gt).  Computed once per argument triple and shared: the callers do not modify it."""
    key = (M, n_in, seed)
    if key not in _PLANTED:
        rs = np.random.RandomState(seed)
        T_gt = RR.perturbed(IDENTITY, rs, 90, 0.5)
        k1 = (rs.rand(M, 3) - 0.5) * 3
        k0 = (rs.rand(M, 3) - 0.5) * 3
        k0[:n_in] = k1[:n_in] @ T_gt[:, :3].T + T_gt[:, 3] + 0.01 * rs.randn(n_in, 3)
        _PLANTED[key] = {"k0": np.ascontiguousarray(k0), "k1": np.ascontiguousarray(k1), "T_gt": T_gt}
    return _PLANTED[key]
