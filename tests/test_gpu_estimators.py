"""The f64 estimators (csrc/estim.hip) at degenerate triples, ties and thresholds (-m gpu).

Everything goes through the Python entries (Context.c_ransac, .o_score, .c_ransac_device, .hyp_from_quat).  The references are
oracle/estim_ref.py (80-digit Kabsch, exact-integer vote) through tests/golden/estim_edges.npz: the inputs are rebuilt from
seeds by oracle/gen_golden_estim.py and checked against the sha256 the file holds; nothing here imports mpmath.

What is pinned: the three rank classes of a sampled triple (a bucket is sampled with replacement, so repeated matches are the
common case), the strict threshold of the vote, the first maximum of the counts at every wave / stride edge of argbest_kernel,
the device sampler at the segment edges of cstat_kernel and around the `sum p < 1e-4` rule, and hyp_kernel's clamped index.
What is not pinned, by design: the last bit of the squared residual.
"""
import os
import sys
import time
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import estim_ref as er  # noqa: E402
import gen_golden_estim as gen  # noqa: E402
import yoho_oracle as orc  # noqa: E402
from yoho_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
EYE = np.eye(4)[:3]
KAB = gen.kabsch_families()
CLOCK = {}


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module", autouse=True)
def module_clock():
    CLOCK["t0"] = time.time()           # the module's first test starts here (collection happens long before in a full run)


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.Context()


@pytest.fixture(scope="module")
def edges(gold):
    return gold("estim_edges.npz")


@pytest.fixture(scope="module")
def votes(edges):
    fams = gen.vote_families()
    for name, f in fams.items():
        k = gen.key(name)
        assert str(edges[f"vote__{k}__sha"]) == gen.sha(f["k0"]) + gen.sha(f["k1"]) + gen.sha(f["T"]), name
        f["inl"] = np.unpackbits(edges[f"vote__{k}__inl"], axis=1)[:, :gen.VOTE_M].astype(bool)
        f["unsure_n"] = int(edges[f"vote__{k}__unsure_n"])
        f["unsure"] = (np.unpackbits(edges[f"vote__{k}__unsure"], axis=1)[:, :gen.VOTE_M].astype(bool) if f["unsure_n"]
                       else np.zeros_like(f["inl"]))
    return fams


# ----------------------------------------------------------------------------------------
# Kabsch
# ----------------------------------------------------------------------------------------
BLOCK = 10          # triples per call: 30 matches + 2 from the next block = the 32-match set the counts are taken on


def run_blocks(ctx, a0, a1, reflect, d):
    """row i of the result = fixture triple i; -> T (n,3,4), counts (n,), and per row the match set it voted on"""
    n = a0.shape[0]
    Ts, cs, sets = [], [], []
    for s in range(0, n, BLOCK):
        e = min(n, s + BLOCK)
        nb = e - s
        pad = (e % n)
        k0 = np.concatenate([a0[s:e].reshape(-1, 3), a0[pad, :2]])
        k1 = np.concatenate([a1[s:e].reshape(-1, 3), a1[pad, :2]])
        tri = np.arange(3 * nb, dtype=np.int64).reshape(nb, 3)
        refl = cu(np.ones(nb, dtype=np.uint8)) if reflect else None
        _, _, T_all, counts = ctx.c_ransac(cu(k0), cu(k1), cu(tri), refl, d, want_all=True)
        Ts.append(T_all.cpu().numpy()); cs.append(counts.cpu().numpy())
        sets += [(k0, k1)] * nb
    return np.concatenate(Ts), np.concatenate(cs), sets


@pytest.mark.parametrize("reflect", [False, True], ids=["proper", "reflected"])
@pytest.mark.parametrize("name", list(KAB))
def test_kabsch_family(ctx, edges, name, reflect):
    a0, a1, cls = KAB[name]
    k = gen.key(name)
    assert str(edges[f"kab__{k}__sha"]) == gen.sha(a0) + gen.sha(a1), "the generator's inputs drifted from the fixture"
    assert str(edges[f"kab__{k}__cls"]) == cls
    n = a0.shape[0]
    d = 0.07
    T, counts, sets = run_blocks(ctx, a0, a1, reflect, d)
    bad = []
    if not np.all(np.isfinite(T)):
        rows = np.nonzero(~np.all(np.isfinite(T.reshape(n, -1)), axis=1))[0]
        pytest.fail(f"{name}: {len(rows)} of {n} rows are not finite (first rows {rows[:8].tolist()}), e.g. T[{rows[0]}] = {T[rows[0]].tolist()}")
    worst = dict(orth=0.0, det=0.0, t=0.0, obj=0.0, R=0.0)
    for i in range(n):
        R = T[i, :, :3]
        orth, det = er.frame_defect(R)
        worst["orth"] = max(worst["orth"], orth / EPS)
        if orth > 64 * EPS:
            bad.append(f"row {i}: max|R R^T - I| = {orth / EPS:.3g} eps > 64 eps")
        want = [1.0] if not reflect else ([-1.0] if cls != "rank0" else [1.0, -1.0])
        ddet = min(abs(det - w) for w in want)
        worst["det"] = max(worst["det"], ddet / EPS)
        if ddet > 64 * EPS:
            bad.append(f"row {i}: det R = {det!r}, wanted {want}")
        td, cn = er.translation_defect(T[i], a0[i], a1[i])
        worst["t"] = max(worst["t"], td / (EPS * cn))
        if td > 8 * EPS * cn:
            bad.append(f"row {i}: |t - (c0 - R c1)| = {td / (EPS * cn):.3g} eps (|c0| + |c1|) > 8")
        if not reflect:
            N = er.covariance(a0[i], a1[i])[3]
            fmin = Fraction(0)
            if cls != "rank0":
                hi, lo = edges[f"kab__{k}__fmin"][i]
                fmin = Fraction(float(hi)) + Fraction(float(lo))
            else:
                fmin = N            # s1 = s2 = 0
            gap = er.objective(R, a0[i], a1[i]) - fmin
            if N > 0:
                worst["obj"] = max(worst["obj"], float(gap / N) / EPS)
            if gap > 64 * Fraction(EPS) * N:
                bad.append(f"row {i}: objective(R) - f_min = {float(gap / N) / EPS if N else float(gap):.3g} eps (|a0c|^2 + |a1c|^2) > 64")
            if cls == "rank2":
                worst["R"] = max(worst["R"], float(np.max(np.abs(R - edges[f"kab__{k}__R"][i]))))
    # the reported count is the exact vote of the row's own T on the 32 matches of its call, up to unsure decisions
    for s in range(0, n, BLOCK):
        e = min(n, s + BLOCK)
        v = er.vote_exact(sets[s][0], sets[s][1], T[s:e], d)
        lo = (v["inl"] & v["sure"]).sum(axis=1)
        hi = lo + (~v["sure"]).sum(axis=1)
        for i in range(s, e):
            if not lo[i - s] <= counts[i] <= hi[i - s]:
                bad.append(f"row {i}: count {counts[i]} outside [{lo[i - s]}, {hi[i - s]}] of the exact vote of its own T")
            if name == "repeat3" and counts[i] < 1:
                bad.append(f"row {i}: a thrice-drawn match must count itself, count = {counts[i]}")
    line = f"kabsch {name:26s} {cls} {'reflected' if reflect else 'proper   '} n={n:3d} orth {worst['orth']:5.2f} eps  det {worst['det']:5.2f} eps  t {worst['t']:5.2f} eps"
    if not reflect:
        line += f"  objective {worst['obj']:8.3g} eps"
        if cls == "rank2":
            e_np = float(edges[f"kab__{k}__e_np"])
            line += f"  |R - R_ref| {worst['R']:9.3g}  e_np {e_np:9.3g}  ratio {worst['R'] / e_np:7.3g}"
            if worst["R"] > 8 * max(e_np, 4 * EPS):
                bad.append(f"max|R_dev - R_ref| = {worst['R']:.3g} > 8 * max(e_np = {e_np:.3g}, 4 eps)")
    print(line)
    assert not bad, f"{name} ({cls}, {'reflected' if reflect else 'proper'}): {len(bad)} failures, first: " + "; ".join(bad[:4])


def test_kabsch_same_bits_at_every_slot(ctx):
    """the same triple at iteration slots 0, 1, 255, 256 and I - 1 of one call, and in a second call: the same bits"""
    I, slots = 300, [0, 1, 255, 256, 299]
    for name in ("nominal/congruent/0.5", "thin/both/1e-06", "small/both/1e-08", "repeat2/aba", "collinear/axis", "repeat3", "half"):
        a0, a1, _ = KAB[name]
        k0 = np.concatenate([a0[0], a0[1], a0[2:11, 0], a0[2:11, 1], a0[2:10, 2]])          # 32 matches; triple under test = rows 0..2
        k1 = np.concatenate([a1[0], a1[1], a1[2:11, 0], a1[2:11, 1], a1[2:10, 2]])
        assert k0.shape == (32, 3)
        tri = np.tile(np.array([3, 4, 5], dtype=np.int64), (I, 1))
        tri[slots] = [0, 1, 2]
        runs = []
        for _ in range(2):
            _, _, T_all, counts = ctx.c_ransac(cu(k0), cu(k1), cu(tri), None, 0.07, want_all=True)
            runs.append((bits(T_all.cpu().numpy()), counts.cpu().numpy()))
        Tb, cb = runs[0]
        assert np.all(np.isfinite(Tb.view(np.float64))), name
        for s in slots:
            assert np.array_equal(Tb[s], Tb[0]) and cb[s] == cb[0], (name, s)
        rest = np.setdiff1d(np.arange(I), slots)
        assert np.all(Tb[rest] == Tb[rest[0]]) and np.all(cb[rest] == cb[rest[0]]), name
        assert np.array_equal(runs[1][0], Tb) and np.array_equal(runs[1][1], cb), name


# ----------------------------------------------------------------------------------------
# the vote
# ----------------------------------------------------------------------------------------
VOTE_MS = [1, 2, 63, 64, 65, 255, 256, 257, 1500]


def first_max(c):
    """(index, value) of the first strict maximum above 0, as `if overlap > best_overlap` with best = 0 leaves it"""
    c = np.asarray(c)
    return (int(np.argmax(c)), int(c.max())) if c.max() > 0 else (0, 0)


@pytest.mark.parametrize("name", ["dyadic", "near/0.09", "near/0.07", "random"])
def test_vote_at_the_threshold(ctx, votes, name):
    f = votes[name]
    k0, k1, T, d, inl, unsure, kind = f["k0"], f["k1"], f["T"], f["d"], f["inl"], f["unsure"], f["kind"]
    H = T.shape[0]
    if name == "random":
        assert f["unsure_n"] * 100000 <= inl.size
    else:
        assert f["unsure_n"] == 0
    m = np.arange(gen.VOTE_M)
    if name == "dyadic":
        on = kind == 0
        assert on.sum() >= 0.05 * gen.VOTE_M and (kind == 1).sum() == on.sum() == (kind == 2).sum()
        s = np.stack([np.sum(np.square(k0 - orc.transform_points(k1, Th)), axis=-1) for Th in T])      # exact: no rounding on this grid
        assert np.all(s[m[on] % H, m[on]] == d * d) and not inl[m[on] % H, m[on]].any(), "on the threshold is not an inlier"
        assert inl[m[kind == 1] % H, m[kind == 1]].all() and not inl[m[kind == 2] % H, m[kind == 2]].any()
        assert np.array_equal(inl, s < d * d)
    elif name.startswith("near"):
        assert (kind != 0).sum() >= 0.05 * gen.VOTE_M
        assert inl[m[kind < 0] % H, m[kind < 0]].all() and not inl[m[kind > 0] % H, m[kind > 0]].any()
    rs = np.random.RandomState(5)
    Td = cu(T)
    for M in VOTE_MS:
        lo_all = (inl[:, :M] & ~unsure[:, :M]).sum(axis=1)
        hi_all = lo_all + unsure[:, :M].sum(axis=1)
        k0d, k1d = cu(k0[:M]), cu(k1[:M])
        for order in (None, rs.permutation(H).astype(np.int64)):
            res, counts = ctx.o_score(k0d, k1d, Td, cu(order) if order is not None else None, H, d)
            c = counts.cpu().numpy()
            o = np.arange(H) if order is None else order
            lo, hi = lo_all[o], hi_all[o]
            wrong = np.nonzero((c < lo) | (c > hi))[0]
            assert len(wrong) == 0, (f"{name} M={M} order={'perm' if order is not None else 'None'}: {len(wrong)} of {H} counts differ from the "
                                     f"exact vote, first: slot {wrong[0]} (hypothesis {o[wrong[0]]}) device {c[wrong[0]]} exact [{lo[wrong[0]]}, {hi[wrong[0]]}]")
            assert tuple(res.cpu().numpy()) == first_max(c), (name, M)
    print(f"vote {name:10s} H={H} M<=1500: unsure decisions {f['unsure_n']} of {inl.size}")


# ----------------------------------------------------------------------------------------
# the first maximum
# ----------------------------------------------------------------------------------------
ARG_HS = [1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1000, 4097]
GROUPS = (3, 4, 5, 6)            # a hypothesis of group c has exactly c inliers; group 0 has none


def tie_matches():
    """dyadic matches in groups: the c members of group c are k0 = k1 + (16 c, 0, 0), so the translation (16 c, 0, 0) counts c;
    group 0: three matches whose k0 triangle is four times the k1 triangle (no rigid motion fits, and none of the others)"""
    rs = np.random.RandomState(11)
    k1, k0, first = [], [], {}
    for c in GROUPS:
        first[c] = len(k1)
        for _ in range(c):
            p = rs.randint(-2048, 2049, size=3) / 1024.0
            k1.append(p); k0.append(p + np.array([16.0 * c, 0.0, 0.0]))
    first[0] = len(k1)
    for _ in range(3):
        p = rs.randint(-2048, 2049, size=3) / 1024.0
        k1.append(p); k0.append(4.0 * p + np.array([0.0, 200.0, 0.0]))
    return np.array(k0), np.array(k1), first


def tie_patterns(H):
    """(label, counts (H,)) with the maximal count 6 at chosen slots over a base of counts in {0, 3, 4}"""
    rs = np.random.RandomState(H)
    base = rs.choice([0, 3, 4], size=H)
    out = []

    def put(label, slots):
        if max(slots) < H and min(slots) >= 0 and len(set(slots)) == len(slots):
            c = base.copy(); c[list(slots)] = 6
            out.append((f"{label}{tuple(slots)}", c))
    for h in (0, 5, 63):
        put("pair+64", (h, h + 64)); put("pair+256", (h, h + 256)); put("pair+64 in the next stride", (h + 256, h + 320))
    put("wave edge", (63, 64)); put("stride edge", (255, 256)); put("ends", (0, H - 1)); put("last alone", (H - 1,))
    # a lower lane that holds a later slot of its 256-stride loop: the lane order is not the slot order
    put("lower lane, later stride", (10, 261)); put("lower lane, later stride, wave 1", (70, 321)); put("lane 0 holds the last slot", (10, H - 1))
    put("three waves", (20, 100, 191)); put("three waves, lowest slot in the last wave", (200, 266, 356))
    put("three waves, second stride first", (300, 400, 460)); put("four waves", (H - 1, H - 65, H - 129, H - 193))
    out.append(("every count equal", np.full(H, 4)))
    out.append(("every count 0", np.zeros(H, dtype=np.int64)))
    return out


def test_first_maximum_wins(ctx):
    k0, k1, first = tie_matches()
    M = k0.shape[0]
    d = 0.09375
    # what a hypothesis of each group counts, from the oracle on the host (LAPACK Kabsch for the c_ransac triples)
    T_of = {c: np.concatenate([np.eye(3), [[16.0 * c], [0.0], [0.0]]], axis=1) for c in GROUPS}
    T_of[0] = np.concatenate([np.eye(3), [[0.0], [-500.0], [0.0]]], axis=1)
    tri_of = {c: np.arange(first[c], first[c] + 3, dtype=np.int64) for c in (0,) + GROUPS}
    for c in (0,) + GROUPS:
        assert orc.inlier_count(k0, k1, T_of[c], d) == c
        assert orc.inlier_count(k0, k1, orc.threepps2tran(k0[tri_of[c]], k1[tri_of[c]], proper=True)[0], d) == c
    k0d, k1d = cu(k0), cu(k1)
    ncase = 0
    for H in ARG_HS:
        for label, cnt in tie_patterns(H):
            want = first_max(cnt)
            T = np.stack([T_of[int(c)] for c in cnt])
            res, counts = ctx.o_score(k0d, k1d, cu(T), None, H, d)
            assert np.array_equal(counts.cpu().numpy(), cnt), (H, label)
            assert tuple(res.cpu().numpy()) == want, f"o_score H={H} {label}: device {tuple(res.cpu().numpy())}, first maximum {want}"
            tri = np.stack([tri_of[int(c)] for c in cnt])
            best_T, res, T_all, counts = ctx.c_ransac(k0d, k1d, cu(tri), None, d, want_all=True)
            assert np.array_equal(counts.cpu().numpy(), cnt), (H, label)
            it, bc = (int(v) for v in res.cpu().numpy())
            if want[1] == 0:
                assert (it, bc) == (0, 0) and np.array_equal(best_T.cpu().numpy(), EYE), (H, label, it, bc)
            else:
                assert (it, bc) == (want[0] + 1, want[1]), f"c_ransac H={H} {label}: device {(it, bc)}, first maximum {(want[0] + 1, want[1])}"
                assert np.array_equal(bits(best_T.cpu().numpy()), bits(T_all.cpu().numpy()[want[0]])), (H, label)
            ncase += 1
    print(f"first maximum: {ncase} count patterns over H in {ARG_HS}, through o_score and c_ransac")


# ----------------------------------------------------------------------------------------
# the device sampler
# ----------------------------------------------------------------------------------------
SAMPLER_MS = [1, 2, 5, 6, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3233, 16384, 65537]
ITERS = [1, 257, 1000]
SEEDS = [0, 2 ** 32 - 1, 2 ** 64 - 1]


def sampler_layouts(M, rs):
    """name -> dr_index (M,) int64"""
    out = {"all in 0": np.zeros(M, dtype=np.int64), "all in 59": np.full(M, 59, dtype=np.int64),
           "round robin": np.arange(M, dtype=np.int64) % 60, "random": rs.randint(0, 60, size=M).astype(np.int64)}
    wild = rs.randint(0, 60, size=M).astype(np.int64)
    pick = rs.rand(M) < 0.3
    wild[pick] = rs.choice(np.array([-1, 60, 2 ** 40, -2 ** 40, 61], dtype=np.int64), size=int(pick.sum()))
    out["outside 0..59"] = wild

    def among_singletons(sizes):
        """buckets of the given sizes, every other match alone in a bucket of its own; None if 60 buckets do not suffice"""
        if sum(sizes) > M or len(sizes) + (M - sum(sizes)) > 60:
            return None
        dr = np.concatenate([np.full(n, b, dtype=np.int64) for b, n in enumerate(sizes)] + [np.arange(len(sizes), len(sizes) + M - sum(sizes), dtype=np.int64)])
        return (dr + 7) % 60 if M > 8 else dr
    for n in (2, 3, 5, 6, 8):
        dr = among_singletons([n])
        if dr is not None:
            out[f"one bucket of {n}"] = dr[rs.permutation(M)]
    dr = among_singletons([5, 5])
    if dr is not None:
        out["two buckets of 5"] = dr[rs.permutation(M)]
    return out


def test_device_sampler_sizes_and_layouts(ctx):
    d = 0.07
    rs = np.random.RandomState(21)
    ncase = nvalid = 0
    seen = set()
    for M in SAMPLER_MS:
        k1 = rs.rand(M, 3) * 3.0
        k0 = synth._apply_rt(k1, synth.quat_to_mat64(np.array([0.5, 0.5, -0.5, 0.5])), np.array([0.3, -0.2, 0.1])) + 0.01 * rs.randn(M, 3)
        out = rs.rand(M) < 0.6
        k0[out] = rs.rand(int(out.sum()), 3) * 3.0
        # the strided `match` form: the same matches addressed through index columns into longer key arrays
        n0, n1 = M + 17, M + 5
        m0, m1 = rs.permutation(n0)[:M], rs.permutation(n1)[:M]
        keys0, keys1 = rs.rand(n0, 3), rs.rand(n1, 3)
        keys0[m0], keys1[m1] = k0, k1
        match = cu(np.stack([m0, m1], axis=1).astype(np.int64))
        k0d, k1d, keys0d, keys1d = cu(k0), cu(k1), cu(keys0), cu(keys1)
        for li, (lname, dr) in enumerate(sampler_layouts(M, rs).items()):
            # every max_iter and seed meets every size and layout family over the run; the small sizes take the full product
            combos = [(it, sd) for it in ITERS for sd in SEEDS] if M in (5, 6, 65, 1025) else [(ITERS[(ncase + j) % 3], SEEDS[(ncase // 3 + j) % 3]) for j in range(2)]
            drd = cu(dr)
            for (I, seed) in combos:
                ncase += 1
                seen.add((I, seed))
                tag = f"M={M} layout='{lname}' max_iter={I} seed={seed}"
                want = orc.yohoc_device_triples(dr, I, seed)
                best_T, res, tri = ctx.c_ransac_device(k0d, k1d, drd, I, seed, d, want_triples=True)
                best_T2, res2, tri2 = ctx.c_ransac_device(keys0d, keys1d, drd, I, seed, d, match=match, want_triples=True)
                bT, (it, bc) = best_T.cpu().numpy(), (int(v) for v in res.cpu().numpy())
                assert np.array_equal(bits(best_T2.cpu().numpy()), bits(bT)) and torch.equal(res2, res), "strided match form differs: " + tag
                if want is None:
                    assert (it, bc) == (50001, 0) and np.array_equal(bT, EYE), f"{tag}: no bucket weight, device says {(it, bc)}"
                    continue
                nvalid += 1
                assert it != 50001, f"{tag}: the oracle samples, the device reports no estimate"
                assert np.array_equal(tri.cpu().numpy(), want), f"{tag}: sampled triples differ from the oracle's"
                assert torch.equal(tri2, tri), tag
                # the same triples through the host-sampled entry: same Kabsch, same vote, same first maximum
                hT, hres, _, _ = ctx.c_ransac(k0d, k1d, tri, None, d, want_all=True)
                assert tuple(int(v) for v in hres.cpu().numpy()) == (it, bc), f"{tag}: device-sampled {(it, bc)}, host-sampled {tuple(hres.cpu().numpy())}"
                assert np.array_equal(bits(hT.cpu().numpy()), bits(bT)), tag
                assert np.all(np.isfinite(bT)), tag
    assert seen == {(it, sd) for it in ITERS for sd in SEEDS}
    # the weight rule itself, in the oracle's own words: n = 2 weighs exactly 0, one bucket of 5 is below 1e-4, one of 6 above
    assert orc.yohoc_device_triples(np.array([0, 0] + list(range(1, 40))), 1, 0) is None
    assert orc.yohoc_device_triples(np.array([0] * 5 + list(range(1, 40))), 1, 0) is None
    assert orc.yohoc_device_triples(np.array([0] * 6 + list(range(1, 40))), 1, 0) is not None
    assert orc.yohoc_device_triples(np.array([0] * 5 + [1] * 5 + list(range(2, 40))), 1, 0) is not None
    print(f"device sampler: {ncase} (size, layout, max_iter, seed) cases, {nvalid} with a valid statistic, {ncase - nvalid} without")


# ----------------------------------------------------------------------------------------
# hypotheses from quaternions
# ----------------------------------------------------------------------------------------
def hyp_case(M, offset, seed):
    rs = np.random.RandomState(seed)
    q = rs.randn(M, 4).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    idx = rs.randint(0, 60, size=M).astype(np.int64)
    idx[:: 4] = np.array([-1, 0, 59, 60], dtype=np.int64)[np.arange(len(idx[:: 4])) % 4]
    k0 = rs.rand(M, 3) * 3.0 + offset
    k1 = rs.rand(M, 3) * 3.0 + offset
    return q, idx, k0, k1


@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_hyp_clamped_index(ctx, tables, M):
    """idx outside 0..59 is clamped; tolerance of test_estimators_outputs_poisoned"""
    q, idx, k0, k1 = hyp_case(M, 0.0, 300 + M)
    T = ctx.hyp_from_quat(cu(q), cu(idx), cu(k0), cu(k1)).cpu().numpy()
    ref = orc.hyp_from_quat(q, np.clip(idx, 0, 59), k0, k1, tables.R32)
    err = float(np.max(np.abs(T - ref)))
    print(f"hyp M={M}: max|T - oracle| = {err:.3g}")
    assert np.allclose(T, ref, rtol=0, atol=1e-12)


def hyp_t_defect(T, k0, k1):
    """per row the worst |t_i - (k0_i - sum_j R_ij k1_j)| with the device's own R, exactly, over the magnitude
    |k0_i| + sum_j |R_ij| |k1_j| that the roundings act on"""
    worst = 0.0
    for m in range(T.shape[0]):
        Tf, a, b = er._fr(T[m]), er._fr(k0[m]), er._fr(k1[m])
        for i in range(3):
            exact = a[i] - sum(Tf[i][j] * b[j] for j in range(3))
            mag = abs(a[i]) + sum(abs(Tf[i][j] * b[j]) for j in range(3))
            worst = max(worst, float(abs(Tf[i][3] - exact) / mag))
    return worst


@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_hyp_far_keys_vs_exact(ctx, tables, M):
    """keys 1e5 from the origin, idx at -1, 0, 59, 60: R against the oracle at the tolerance of test_estimators_outputs_poisoned,
    t against the exact value of k0 - R k1 for the device's own R, whatever order the oracle's BLAS takes on the host of the
    day.  hyp_kernel rounds three times on the way to t (two fused multiply-adds and a product, then the subtraction), each at
    most half an ulp of a partial sum below |k0_i| + sum |R_ij k1_j|: 2 eps of that magnitude bounds them."""
    q, idx, k0, k1 = hyp_case(M, 1e5, 400 + M)
    T = ctx.hyp_from_quat(cu(q), cu(idx), cu(k0), cu(k1)).cpu().numpy()
    ref = orc.hyp_from_quat(q, np.clip(idx, 0, 59), k0, k1, tables.R32)
    assert np.allclose(T[:, :, :3], ref[:, :, :3], rtol=0, atol=1e-12)
    defect = hyp_t_defect(T, k0, k1)
    print(f"hyp far M={M}: |t - exact(k0 - R k1)| <= {defect / EPS:.3g} eps of the magnitude")
    assert defect <= 2 * EPS


@pytest.mark.parametrize("M", [1, 255, 256, 257])
def test_hyp_far_keys(ctx, tables, M):
    """keys 1e5 from the origin, idx at -1, 0, 59, 60, against orc.hyp_from_quat at the tolerance of
    test_estimators_outputs_poisoned (atol = 1e-12).  An ulp of a translation of this size is 1.5e-11 ... 5.8e-11, so this
    passes only with the bits of the oracle's `k1 @ R.T`: hyp_kernel evaluates that product in numpy's order (the product of
    index 1 rounded, indices 0 and 2 fused onto it; measured on AVX-512 Intel and Zen 5 hosts, 100 % of 9000 products).
    With the plain 0, 1, 2 order the device was one ulp off the oracle for 15 % of the rows (5.8e-11 here)."""
    q, idx, k0, k1 = hyp_case(M, 1e5, 400 + M)
    T = ctx.hyp_from_quat(cu(q), cu(idx), cu(k0), cu(k1)).cpu().numpy()
    ref = orc.hyp_from_quat(q, np.clip(idx, 0, 59), k0, k1, tables.R32)
    err_R, err_t = float(np.max(np.abs(T[:, :, :3] - ref[:, :, :3]))), float(np.max(np.abs(T[:, :, 3] - ref[:, :, 3])))
    print(f"hyp far M={M}: max|R - oracle| = {err_R:.3g}, max|t - oracle| = {err_t:.3g}")
    assert np.allclose(T, ref, rtol=0, atol=1e-12)


def test_module_wall_time():
    """runs last: the module must stay cheap (the whole -m gpu run has a 1200 s limit)"""
    dt = time.time() - CLOCK["t0"]
    print(f"tests/test_gpu_estimators.py: {dt:.1f} s from the first test to the last")
    assert dt < 120.0
