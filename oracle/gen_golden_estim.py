"""tests/golden/estim_edges.npz: reference answers for the f64 estimators at degenerate triples, ties and thresholds.

    python oracle/gen_golden_estim.py            (needs mpmath; about ten seconds of host time)

The inputs are rebuilt from seeds wherever they are needed (kabsch_families / vote_families below: numpy RandomState and
yoho_amd.synth, element-wise IEEE operations only); the file holds what cannot be recomputed cheaply or without mpmath:
per Kabsch triple the 80-digit rotation, singular values and optimal objective (oracle/estim_ref.py), per rank-2 family the
error of the LAPACK path on the same inputs (e_np), per vote family the exact decisions as packed bits, and a sha256 of every
input array so that a generator that drifts is noticed.  tests/test_estim_ref_cpu.py regenerates the file and compares.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import estim_ref as er  # noqa: E402
import yoho_oracle as orc  # noqa: E402
from yoho_amd import synth  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "estim_edges.npz")
S12_CAP = 2e12
N_FAM = 32


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ----------------------------------------------------------------------------------------
# Kabsch families: name -> (a0 (n,3,3), a1 (n,3,3), class)
# ----------------------------------------------------------------------------------------
def _rot(rs):
    q = rs.randn(4)
    q = q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return synth.quat_to_mat64(q)


def _direction(rs):
    v = rs.randn(3)
    return v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def _triangle(rs, size, offset, height=None, shape=None):
    """three points with edge ~ size whose centroid lies ~ offset from the origin; height: height / base of a thin triangle;
    shape: fixed local 2-D coordinates instead of a jittered well-shaped triangle"""
    if shape is not None:
        loc = np.array(shape, dtype=np.float64)
    elif height is not None:
        loc = np.array([[0.0, 0.0], [1.0, 0.0], [0.2 + 0.6 * rs.rand(), height]])
    else:
        loc = np.array([[0.0, 0.0], [1.0, 0.0], [0.3 + 0.4 * rs.rand(), 0.6 + 0.4 * rs.rand()]])
    loc3 = np.concatenate([loc, np.zeros((3, 1))], axis=1) * size
    return synth._apply_rt(loc3, _rot(rs), _direction(rs) * offset)


def _moved(rs, a1, offset, noise):
    """a rigid motion of a1 (+ noise) whose centroid lies ~ offset from the origin"""
    R = _rot(rs)
    c = (a1[0] + a1[1] + a1[2]) / 3.0
    x = synth._apply_rt(a1 - c, R, _direction(rs) * offset)
    return x + noise * rs.randn(3, 3)


EQUILATERAL = [[0.0, 0.0], [1.0, 0.0], [0.5, 0.8660254037844386]]
ISOSCELES = [[0.0, 0.0], [1.0, 0.0], [0.5, 1.75]]


def kabsch_families():
    fam = {}

    def add(name, seed, cls, make, n=N_FAM):
        rs = np.random.RandomState(seed)
        pairs = [make(rs, i) for i in range(n)]
        fam[name] = (np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), cls)

    def congruent(size, offset, noise=0.01):
        def make(rs, i):
            a1 = _triangle(rs, size, offset)
            return _moved(rs, a1, offset, noise), a1
        return make

    def unrelated(size0, size1, offset, h0=None, h1=None):
        return lambda rs, i: (_triangle(rs, size0, offset, height=h0), _triangle(rs, size1, offset, height=h1))

    seed = 7000
    for size in (0.5, 1.5):
        add(f"nominal/congruent/{size}", seed, "rank2", congruent(size, 3.0)); seed += 1
        add(f"nominal/unrelated/{size}", seed, "rank2", unrelated(size, size, 3.0)); seed += 1
    for off in (1e3, 1e5):
        add(f"far/congruent/{off:g}", seed, "rank2", congruent(1.0, off)); seed += 1
        add(f"far/unrelated/{off:g}", seed, "rank2", unrelated(1.0, 1.0, off)); seed += 1
    for h in (1e-3, 1e-6):
        add(f"thin/both/{h:g}", seed, "rank2", unrelated(1.0, 1.0, 3.0, h0=h, h1=h)); seed += 1
    for h in (1e-3, 1e-6, 1e-9):
        add(f"thin/one/{h:g}", seed, "rank2", unrelated(1.0, 1.0, 3.0, h1=h)); seed += 1
    for size in (1e-3, 1e-6, 1e-8):
        add(f"small/both/{size:g}", seed, "rank2", unrelated(size, size, 3.0)); seed += 1
    for size in (1e-6, 1e-9):
        add(f"small/one/{size:g}", seed, "rank2", unrelated(1.0, size, 3.0)); seed += 1

    def mirrored(shape):
        def make(rs, i):
            a1 = _triangle(rs, 1.0, 3.0, shape=shape)
            return _moved(rs, a1[[1, 0, 2]], 3.0, 0.0), a1          # the base vertices exchanged: the mirror image in the plane
        return make
    add("equal/equilateral", seed, "rank2", mirrored(EQUILATERAL)); seed += 1
    add("equal/isosceles", seed, "rank2", mirrored(ISOSCELES)); seed += 1

    # a match drawn twice: the index patterns of a bucket sampled with replacement
    for pat in ((0, 0, 1), (0, 1, 0), (1, 0, 0)):
        def make(rs, i, pat=pat):
            a0, a1 = congruent(1.0, 3.0)(rs, i) if i % 2 == 0 else unrelated(1.0, 1.0, 3.0)(rs, i)
            return a0[list(pat)], a1[list(pat)]
        add("repeat2/" + "".join("ab"[k] for k in pat), seed, "rank1", make, n=16); seed += 1

    # three distinct, exactly collinear points: dyadic coordinates (multiples of 2^-10), so collinear as numbers
    def dyadic_line(rs, axis=None):
        p = rs.randint(-3072, 3073, size=3) / 1024.0
        v = rs.randint(-256, 257, size=3) / 1024.0
        if axis is not None:
            v = np.zeros(3); v[axis] = rs.randint(1, 257) / 1024.0
        if not np.any(v):
            v[0] = 0.125
        k = np.array([0, 1 + rs.randint(3), 4 + rs.randint(3)])[rs.permutation(3)]
        return p[None, :] + k[:, None] * v[None, :]

    add("collinear/both", seed, "rank1", lambda rs, i: (dyadic_line(rs), dyadic_line(rs)), n=16); seed += 1
    add("collinear/axis", seed, "rank1", lambda rs, i: (dyadic_line(rs, i % 3), dyadic_line(rs, (i // 3) % 3)), n=16); seed += 1
    add("collinear/one", seed, "rank1", lambda rs, i: ((_triangle(rs, 1.0, 3.0), dyadic_line(rs)) if i % 2 else
                                                      (dyadic_line(rs), _triangle(rs, 1.0, 3.0))), n=16); seed += 1

    # the same match three times
    # the same match three times: full 53-bit coordinates, so that (p + p + p) / 3 != p in floating point for one coordinate in
    # five and the centred points are rounding noise instead of 0
    rs = np.random.RandomState(seed); seed += 1
    p1 = rs.rand(512, 3) * 3.0
    p0 = synth._apply_rt(p1, _rot(rs), rs.rand(3) - 0.5) + 0.01 * rs.randn(512, 3)
    fam["repeat3"] = (np.repeat(p0[:, None, :], 3, axis=1), np.repeat(p1[:, None, :], 3, axis=1), "rank0")

    def half(rs, i):
        t, p = _triangle(rs, 1.0, 3.0), np.repeat((rs.rand(1, 3) * 3.0), 3, axis=0)
        return (t, p) if i % 2 else (p, t)
    add("half", seed, "rank0", half); seed += 1
    return fam


# ----------------------------------------------------------------------------------------
# vote families: name -> dict(k0, k1 (1500,3), T (H,3,4), d, and family-specific marks)
# ----------------------------------------------------------------------------------------
VOTE_M = 1500
ON = [(96, 0, 0), (64, 64, 32)]                 # |e|^2 = 9216 grid steps^2 = (3/32)^2 exactly, e in multiples of 2^-10


def _signed_perms():
    import itertools
    out = []
    for perm in itertools.permutations(range(3)):
        for sg in itertools.product((1.0, -1.0), repeat=3):
            R = np.zeros((3, 3))
            for i in range(3):
                R[i, perm[i]] = sg[i]
            out.append(R)
    return out


def dyadic_family():
    """every operation exact in any order; match m is tied to hypothesis m % H; class by m % 20:
    0 on the threshold, 1 one grid step inside, 2 one grid step outside, 3..11 inliers, others anywhere"""
    rs = np.random.RandomState(7100)
    Rs = _signed_perms()
    H, M = len(Rs), VOTE_M
    T = np.zeros((H, 3, 4))
    for h in range(H):
        T[h, :, :3] = Rs[h]
        T[h, :, 3] = rs.randint(-1024, 1025, size=3) / 1024.0
    k1 = rs.randint(-2048, 2049, size=(M, 3)) / 1024.0
    k0 = rs.randint(-3072, 3073, size=(M, 3)) / 1024.0
    kind = np.full(M, 3, dtype=np.int8)          # 0 on, 1 inside, 2 outside, 3 free
    for m in range(M):
        c = m % 20
        if c > 11:
            continue
        h = m % H
        p = synth._apply_rt(k1[m:m + 1], T[h, :, :3], T[h, :, 3])[0]
        if c <= 2:
            e = np.array(ON[rs.randint(2)], dtype=np.float64)
            e[0] += (0, -1, 1)[c]                                          # one grid step inside / outside
            e = e[rs.permutation(3)] * rs.choice([-1.0, 1.0], size=3)
            kind[m] = c
        else:
            e = rs.randint(-50, 51, size=3).astype(np.float64)
        k0[m] = p + e / 1024.0
    return dict(k0=k0, k1=k1, T=T, d=0.09375, kind=kind)


def near_family(d, seed):
    """realistic keypoints, hypotheses from the group rotations; every fifth match m is moved along its residual under
    hypothesis m % H so that s = d2 +- 4 b or d2 +- 64 b (b: the ambiguity bound of that decision): as close as is still sure"""
    H = 60
    ec = synth.estimator_case(VOTE_M, VOTE_M, seed=seed)
    k0, k1, T = ec["k0"].copy(), ec["k1"], np.ascontiguousarray(ec["T"][:H])
    d2 = float(np.float64(d) * np.float64(d))
    rs = np.random.RandomState(seed + 1)
    kind = np.zeros(VOTE_M, dtype=np.int8)       # 0 untouched; +-1: 4 b outside / inside; +-2: 64 b
    for m in range(0, VOTE_M, 5):
        h = m % H
        mult, sign = ((4.0, 1.0), (4.0, -1.0), (64.0, 1.0), (64.0, -1.0))[(m // 5) % 4]
        p = synth._apply_rt(k1[m:m + 1], T[h, :, :3], T[h, :, 3])[0]
        for attempt in range(20):
            u = _direction(rs)
            b = er.vote_exact((p + u * d)[None], k1[m:m + 1], T[h:h + 1], d)["b"][0, 0]
            cand = p + u * np.sqrt(d2 + sign * mult * b)
            v = er.vote_exact(cand[None], k1[m:m + 1], T[h:h + 1], d)
            off = (v["s"][0, 0] - d2) * sign
            if v["sure"][0, 0] and bool(v["inl"][0, 0]) == (sign < 0) and 0.5 * mult * b < off < 2.0 * mult * b:
                break
        else:
            raise AssertionError(("near: no sure member", m))
        k0[m] = cand
        kind[m] = int(sign) * (1 if mult == 4.0 else 2)
    return dict(k0=k0, k1=k1, T=T, d=d, kind=kind)


def random_family():
    ec = synth.estimator_case(VOTE_M, 1000, seed=4)
    return dict(k0=ec["k0"], k1=ec["k1"], T=np.ascontiguousarray(ec["T"][:100]), d=0.09, kind=np.zeros(VOTE_M, dtype=np.int8))


def vote_families():
    return {"dyadic": dyadic_family(), "near/0.09": near_family(0.09, 7200), "near/0.07": near_family(0.07, 7300), "random": random_family()}


# ----------------------------------------------------------------------------------------
def key(name):
    return name.replace("/", "__")


def generate(verbose=True):
    out = {}
    names, summary = [], []
    for name, (a0, a1, cls) in kabsch_families().items():
        n = a0.shape[0]
        refs = [er.kabsch_ref(a0[i], a1[i]) for i in range(n)]
        got = {r["cls"] for r in refs}
        assert got == {cls}, (name, got)
        k = key(name)
        out[f"kab__{k}__sha"] = np.array(sha(a0) + sha(a1))
        out[f"kab__{k}__cls"] = np.array(cls)
        e_np = ratio = 0.0
        if cls != "rank0":
            out[f"kab__{k}__fmin"] = np.array([r["f_min"] for r in refs])
            out[f"kab__{k}__s"] = np.array([[r["s1"], r["s2"]] for r in refs])
        if cls == "rank2":
            R = np.stack([r["R"] for r in refs])
            out[f"kab__{k}__R"] = R
            ratio = max(r["s1"] / r["s2"] for r in refs)
            assert ratio <= S12_CAP, (name, ratio)
            Rl = np.stack([orc.threepps2tran(a0[i], a1[i], proper=True)[0][:, :3] for i in range(n)])
            e_np = float(np.max(np.abs(Rl - R)))
            assert np.isfinite(e_np) and e_np > 0
            out[f"kab__{k}__e_np"] = np.array(e_np)
        names.append(name)
        summary.append(f"{name:28s} {cls}  n={n:3d}  s1/s2 <= {ratio:9.3g}  e_np {e_np:9.3g}")
    out["kab_names"] = np.array(names)
    vnames = []
    for name, f in vote_families().items():
        v = er.vote_exact(f["k0"], f["k1"], f["T"], f["d"])
        unsure = ~v["sure"]
        if name == "dyadic":
            # no rounding anywhere (grid 2^-10, |values| < 8): a plain float64 evaluation carries the exact s, so every decision
            # is determined, the ones with s == d2 included (not inliers: the comparison is strict)
            s_np = np.stack([np.sum(np.square(f["k0"] - orc.transform_points(f["k1"], T)), axis=-1) for T in f["T"]])
            assert np.array_equal(s_np, v["s"]) and np.all(v["s"] * 2.0 ** 20 == np.round(v["s"] * 2.0 ** 20))
            unsure = np.zeros_like(unsure)
        k = key(name)
        out[f"vote__{k}__sha"] = np.array(sha(f["k0"]) + sha(f["k1"]) + sha(f["T"]))
        out[f"vote__{k}__inl"] = np.packbits(v["inl"], axis=1)
        out[f"vote__{k}__unsure_n"] = np.array(int(unsure.sum()))
        if unsure.any():
            out[f"vote__{k}__unsure"] = np.packbits(unsure, axis=1)
        if name != "random":
            assert not unsure.any(), (name, int(unsure.sum()))
        else:
            assert unsure.sum() * 100000 <= unsure.size, (name, int(unsure.sum()))
        vnames.append(name)
        summary.append(f"vote {name:12s} H={f['T'].shape[0]:3d} M={VOTE_M} inliers {int(v['inl'].sum()):6d} unsure {int(unsure.sum())}")
    out["vote_names"] = np.array(vnames)
    if verbose:
        print("\n".join(summary))
    return out


if __name__ == "__main__":
    data = generate()
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes")
