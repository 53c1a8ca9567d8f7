"""High-precision reference for the f64 estimators (csrc/estim.hip)  --  TEST INFRASTRUCTURE ONLY.

Every float64 is a dyadic rational, so the inputs are taken as exact numbers:

  kabsch_ref   the 3-point Kabsch answer at 80 digits (mpmath SVD): centroids, m = (a1 - c1)^T (a0 - c0), singular values, the
               proper rotation R = v1 u1^T + v2 u2^T + (v1 x v2)(u1 x u2)^T, t = c0 - R c1, the optimal objective
               f_min = |a0c|^2 + |a1c|^2 - 2 (s1 + s2) and the rank class of the triple, decided with exact rationals.
  objective    sum_p |a0c_p - R a1c_p|^2 for a float64 R handed in, as an exact rational.
  vote_exact   per (hypothesis, match) the squared residual as an exact scaled integer, the exact comparison with
               d2 = fl(d * d) and an ambiguity bound per decision.

mpmath is imported by kabsch_ref only: everything a GPU test calls (objective, frame_defect, vote_exact, centroids) needs
nothing but the standard library and numpy.  No product file imports this module.
"""
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -52
DPS = 80


# ----------------------------------------------------------------------------------------
# exact helpers (rationals)
# ----------------------------------------------------------------------------------------
def _fr(a):
    """float64 array -> nested lists of Fractions (exact)."""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 0:
        return Fraction(float(a))
    return [_fr(x) for x in a]


def centred(a):
    """(3,3) float64 points -> (centroid [3], centred points [3][3]) as Fractions."""
    p = _fr(a)
    c = [(p[0][j] + p[1][j] + p[2][j]) / 3 for j in range(3)]
    return c, [[p[i][j] - c[j] for j in range(3)] for i in range(3)]


def covariance(a0, a1):
    """m = (a1 - c1)^T (a0 - c0) as Fractions, with both centroids and N = |a0c|^2 + |a1c|^2."""
    c0, x0 = centred(a0)
    c1, x1 = centred(a1)
    m = [[sum(x1[p][i] * x0[p][j] for p in range(3)) for j in range(3)] for i in range(3)]
    N = sum(v * v for r in x0 for v in r) + sum(v * v for r in x1 for v in r)
    return m, c0, c1, N


def rank_class(a0, a1):
    """'rank2' / 'rank1' / 'rank0' of m in exact arithmetic (three centred points: rank <= 2)."""
    m = covariance(a0, a1)[0]
    if all(v == 0 for r in m for v in r):
        return "rank0"
    for i in range(3):
        for j in range(i + 1, 3):
            for k in range(3):
                for l in range(k + 1, 3):
                    if m[i][k] * m[j][l] - m[i][l] * m[j][k] != 0:
                        return "rank2"
    return "rank1"


def objective(R, a0, a1):
    """sum_p |a0c_p - R a1c_p|^2 as a Fraction, R (3,3) float64 taken as exact."""
    Rf = _fr(R)
    _, x0 = centred(a0)
    _, x1 = centred(a1)
    tot = Fraction(0)
    for p in range(3):
        for i in range(3):
            e = x0[p][i] - sum(Rf[i][j] * x1[p][j] for j in range(3))
            tot += e * e
    return tot


def frame_defect(R):
    """(max |R R^T - I|, det R) of a float64 (3,3) R, evaluated exactly and rounded once."""
    Rf = _fr(R)
    worst = Fraction(0)
    for i in range(3):
        for j in range(3):
            g = sum(Rf[i][k] * Rf[j][k] for k in range(3)) - (1 if i == j else 0)
            worst = max(worst, abs(g))
    det = (Rf[0][0] * (Rf[1][1] * Rf[2][2] - Rf[1][2] * Rf[2][1]) - Rf[0][1] * (Rf[1][0] * Rf[2][2] - Rf[1][2] * Rf[2][0])
           + Rf[0][2] * (Rf[1][0] * Rf[2][1] - Rf[1][1] * Rf[2][0]))
    return float(worst), float(det)


def translation_defect(T, a0, a1):
    """(max_i |t_i - (c0 - R c1)_i|, |c0| + |c1|) for a float64 T (3,4) with the exact centroids (Euclidean norms)."""
    Tf = _fr(T)
    c0, _ = centred(a0)
    c1, _ = centred(a1)
    worst = max(abs(Tf[i][3] - (c0[i] - sum(Tf[i][j] * c1[j] for j in range(3)))) for i in range(3))
    return float(worst), float(sum(v * v for v in c0)) ** 0.5 + float(sum(v * v for v in c1)) ** 0.5


# ----------------------------------------------------------------------------------------
# Kabsch at 80 digits
# ----------------------------------------------------------------------------------------
def kabsch_ref(a0, a1):
    """a0, a1 (3,3) float64: target / source points.  Returns a dict:
       cls 'rank2' | 'rank1' | 'rank0' (exact), s1, s2 (float), c0, c1 (float64 [3], rounded from the exact centroids),
       N = |a0c|^2 + |a1c|^2 (float), f_min as (hi, lo) float64 pair, and for rank2 R (3,3), t (3) rounded to float64."""
    import mpmath as mp
    cls = rank_class(a0, a1)
    m, c0, c1, N = covariance(a0, a1)
    out = {"cls": cls, "c0": np.array([float(v) for v in c0]), "c1": np.array([float(v) for v in c1]), "N": float(N), "R": None, "t": None}
    with mp.workdps(DPS):
        to_mp = lambda q: mp.mpf(q.numerator) / mp.mpf(q.denominator)
        if cls == "rank0":
            s1 = s2 = mp.mpf(0)
        elif cls == "rank1":
            s1, s2 = mp.sqrt(to_mp(sum(v * v for r in m for v in r))), mp.mpf(0)      # one singular value: the Frobenius norm
        else:
            A = mp.matrix([[to_mp(v) for v in r] for r in m])
            U, S, Vt = mp.svd_r(A)
            order = sorted(range(3), key=lambda k: -S[k])
            i1, i2 = order[0], order[1]
            s1, s2 = S[i1], S[i2]
            u1, u2 = [U[r, i1] for r in range(3)], [U[r, i2] for r in range(3)]
            v1, v2 = [Vt[i1, r] for r in range(3)], [Vt[i2, r] for r in range(3)]
            cr = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
            u3, v3 = cr(u1, u2), cr(v1, v2)
            R = [[v1[i] * u1[j] + v2[i] * u2[j] + v3[i] * u3[j] for j in range(3)] for i in range(3)]
            t = [to_mp(c0[i]) - sum(R[i][j] * to_mp(c1[j]) for j in range(3)) for i in range(3)]
            out["R"] = np.array([[float(v) for v in r] for r in R])
            out["t"] = np.array([float(v) for v in t])
        f = to_mp(N) - 2 * (s1 + s2)
        hi = float(f)
        out["f_min"] = (hi, float(f - mp.mpf(hi)))
        out["s1"], out["s2"] = float(s1), float(s2)
    return out


# ----------------------------------------------------------------------------------------
# the inlier vote with exact integers
# ----------------------------------------------------------------------------------------
def _scaled(x):
    """float64 array -> (object array I of Python ints, E) with x == I * 2**-E exactly."""
    x = np.asarray(x, dtype=np.float64)
    assert np.all(np.isfinite(x))
    mant, ex = np.frexp(x)
    mi = (mant * 2.0 ** 53).astype(np.int64).reshape(-1)
    ex = (ex.astype(np.int64) - 53).reshape(-1)
    nz = mi != 0
    E = int(-ex[nz].min()) if nz.any() else 0
    E = max(E, 0)
    out = np.empty(mi.shape, dtype=object)
    for k in range(mi.size):
        out[k] = (int(mi[k]) << int(ex[k] + E)) if mi[k] else 0
    return out.reshape(x.shape), E


def vote_exact(k0, k1, T, d):
    """k0, k1 (M,3), T (H,3,4) float64, d float.  Per (hypothesis h, match m), all exact:
         e = k0[m] - (R_h k1[m] + t_h),  s = |e|^2,  inlier = s < d2 with d2 = fl(d * d)  (strict, as the reference),
         b = 2 eps (8 P sum_i |e_i| + 4 s),  P = max_i (sum_j |k1_j| |T_ij| + |T_i3|) + max |k0|,  sure = |s - d2| > b.
       Returns dict(inl (H,M) bool, sure (H,M) bool, s (H,M) float64 (rounded once), b (H,M) float64, d2)."""
    k0 = np.asarray(k0, dtype=np.float64).reshape(-1, 3)
    k1 = np.asarray(k1, dtype=np.float64).reshape(-1, 3)
    T = np.asarray(T, dtype=np.float64).reshape(-1, 3, 4)
    M, H = k0.shape[0], T.shape[0]
    d2 = float(np.float64(d) * np.float64(d))
    A, Ea = _scaled(k0)
    B, Eb = _scaled(k1)
    Ti, Et = _scaled(T)
    D, Ed = _scaled(np.array([d2]))
    Es = max(Ea, Eb + Et, (Ed + 1) // 2)
    A = A * (1 << (Es - Ea))
    up = 1 << (Es - Eb - Et)
    d2i = int(D[0]) << (2 * Es - Ed)
    one = 1 << (2 * Es)
    inl = np.zeros((H, M), dtype=bool)
    sure = np.zeros((H, M), dtype=bool)
    sf = np.zeros((H, M))
    bf = np.zeros((H, M))
    absk1, maxa = np.abs(k1), np.max(np.abs(k0), axis=1)
    for h in range(H):
        s = np.zeros(M, dtype=object)
        sabs = np.zeros(M, dtype=object)
        for i in range(3):
            p = (B[:, 0] * Ti[h, i, 0] + B[:, 1] * Ti[h, i, 1] + B[:, 2] * Ti[h, i, 2] + Ti[h, i, 3] * (1 << Eb)) * up
            e = A[:, i] - p
            s = s + e * e
            sabs = sabs + np.abs(e)
        aT = np.abs(T[h])
        P = np.max(np.stack([((absk1[:, 0] * aT[i, 0] + absk1[:, 1] * aT[i, 1]) + absk1[:, 2] * aT[i, 2]) + aT[i, 3] for i in range(3)]), axis=0) + maxa
        s_f = np.array([int(v) / one for v in s])
        e1_f = np.array([int(v) / (1 << Es) for v in sabs])
        b = 2.0 * EPS * (8.0 * P * e1_f + 4.0 * s_f)
        diff = np.array([abs(int(v) - d2i) / one for v in s])
        inl[h] = np.array([int(v) < d2i for v in s])
        sure[h] = diff > b
        sf[h], bf[h] = s_f, b
    return {"inl": inl, "sure": sure, "s": sf, "b": bf, "d2": d2}
