"""The nearest-neighbour contract at the inputs where a search kernel can go wrong (helper of tests/test_nn_cpu.py and
tests/test_gpu_nn.py, not a conftest; plain numpy).

The contract is the oracle's: per row `argmin` of `orc.pdist_l2(a, b, squared)` (first minimum) and `orc.mutual_match`.  Nothing here
replaces it - `nn_ref` only evaluates it once per DISTINCT source row.  The rest builds inputs and emulates what the device does
BEFORE the exact distance decides, so that the CPU suite can show the inputs reach the places they are meant to reach:

  * `rounded_tie_targets` / `mutual_tie_case`: two targets whose D2 differ by more than 1e-6 relative and whose 'L2' distances
    sqrt(D2 + 1e-7) have the same bits - the reference answers the lower index, a rule that looks at D2 alone the later one
    (`kernel_rule_before_fix`: the 16-lane rule nn32seg_kernel (one and two rows per thread) had; `kernel_rule`: the one they have now);
  * `band_case`: a query whose true neighbour loses against a rival in the fp16 Gram scores of the matcher's pre-filter
    (csrc/matchf.hip) by a large share of the candidate band - every magnitude sits at an fp16 rounding midpoint;
    `emu_prefilter` restates those scores, the row minimum and `band_of`, with the band's leading constant and the set its maximum
    norm is taken from as parameters, so that mutants of the band can be run on the CPU."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle"))
import yoho_oracle as orc  # noqa: E402

TIE_SCALES = (4.47e-8, 1.2e-5, 2.5e-5)      # distance of the tie pair from the zero query: D2 = 2e-15, 1.4e-10, 6.3e-10
TIE_GAP = 4e-6                              # relative difference of the two distances (8e-6 of D2: the old shortcut's 1e-6 calls it clear)
NN_LANES = 16                               # targets t, t + 16, t + 32, ... of a segment are visited by one thread
NN_TILE = 256                               # target rows per LDS tile of nn32seg_kernel (NN_TT, csrc/nntile.h)
SEG_PAIRS = 1 << 20                         # Ns * Nt from which yoho_nn_search / yoho_mutual_nn take the segmented / pre-filter path
F1 = np.float32(1.0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ulps(x, y):
    """distance of two non-negative fp32 numbers in units of the last place"""
    return int(abs(int(bits(np.float32(x)).reshape(-1)[0]) - int(bits(np.float32(y)).reshape(-1)[0])))


def nn_ref(src, tgt, squared=False, chunk=250):
    """-> (idx (Ns) int64, dist (Ns) f32): argmin / min of orc.pdist_l2 per row.  The oracle is a function of the row's content, so it
    is evaluated once per distinct source row (the tie cases repeat two rows thousands of times)."""
    src, tgt = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)
    uniq, inv = np.unique(src, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    ui = np.empty(len(uniq), np.int64)
    ud = np.empty(len(uniq), np.float32)
    for s in range(0, len(uniq), chunk):
        d = orc.pdist_l2(uniq[s:s + chunk], tgt, squared=squared)
        ui[s:s + chunk] = np.argmin(d, axis=1)
        ud[s:s + chunk] = d.min(axis=1)
    return ui[inv], ud[inv]


# ---------------------------------------------------------------------------------------------------------------------------------
# rounded ties
# ---------------------------------------------------------------------------------------------------------------------------------
def _assert_rounded_tie(q, far, near):
    """on the oracle: D2(q, far) > D2(q, near) > 0 by more than 1e-6 relative, and equal 'L2' bits"""
    two = np.stack([far, near])
    d2 = orc.pdist_l2(q[None], two, squared=True)[0]
    dl = orc.pdist_l2(q[None], two, squared=False)[0]
    assert d2[0] > d2[1] > 0, d2
    assert bits(dl)[0] == bits(dl)[1], (d2, dl)
    assert (float(d2[0]) - float(d2[1])) / float(d2[0]) > 1e-6, d2          # what makes `d2 < best (1 - 1e-6)` true
    return d2, dl


def rounded_tie_targets(D, Nt, pairs, scale):
    """(Nt, D) targets for a ZERO query: ones, and for every (lo_idx, hi_idx) of `pairs` the row lo_idx at distance `scale` along
    the diagonal and the row hi_idx at scale (1 - TIE_GAP).  Under 'L2' both have the same distance bits (first minimum: the lowest
    lo_idx), under 'SquareL2' the smaller D2 wins (the lowest hi_idx)."""
    tgt = np.ones((Nt, D), np.float32)
    far = np.full(D, scale / np.sqrt(D), np.float32)
    near = np.full(D, scale * (1.0 - TIE_GAP) / np.sqrt(D), np.float32)
    _assert_rounded_tie(np.zeros(D, np.float32), far, near)
    used = set()
    for lo, hi in pairs:
        assert 0 <= lo < hi < Nt and lo not in used and hi not in used, (lo, hi, Nt)
        used.update((lo, hi))
        tgt[lo], tgt[hi] = far, near
    return tgt


def tie_sources(D, Ns, rows=(0, 7, 15, 16, 31, -1)):
    """(Ns, D) sources for rounded_tie_targets: the zero query at `rows` (-1: the last row; rows beyond Ns dropped), ones elsewhere
    (their nearest neighbour is the first row of ones, at D2 = 0).  Rows r and r + 16 of a block of 32 share a thread of
    nn32seg_kernel: 0 / 16 and 15 / 31 are two tie rows in one thread, 7 a tie row beside a row of ones."""
    src = np.ones((Ns, D), np.float32)
    for r in rows:
        r = Ns - 1 if r < 0 else r
        if r < Ns:
            src[r] = 0
    return src


def seg_len(Ns, Nt, nCU):
    """nn_segment_plan's cut of the targets (csrc/nntile.h; 32 rows per workgroup, no single-segment rule: launch_nn32seg's call):
    -> (segLen, nseg)"""
    rb = (Ns + 31) // 32
    nseg = (4 * nCU + rb - 1) // rb
    maxseg = (Nt + 63) // 64
    nseg = max(1, min(nseg, maxseg))
    seg = (Nt + nseg - 1) // nseg
    seg = (seg + 15) // 16 * 16
    return seg, (Nt + seg - 1) // seg


def tie_placements(Nt, seg=None):
    """{name: (lo, hi)} inside Nt targets cut into segments of `seg` rows (None: one segment, the one-row nn32seg_kernel).  One thread visits the
    targets of a segment that are congruent mod 16, tile after tile of 256 from the segment's start."""
    seg = Nt if seg is None or seg > Nt else seg
    out = {"i, i + 16": (2, 18), "i, i + 256": (2, 2 + NN_TILE), "i, i + 2": (2, 4),
           "across the first tile boundary": (NN_TILE - 13, NN_TILE + 3),
           "up to the last row": (Nt - 17, Nt - 1)}         # inside the last, ragged tile wherever that has more than 16 rows
    if seg < Nt:
        out["across a segment boundary"] = (seg - 13, seg + 3)
    return {k: v for k, v in out.items() if 0 <= v[0] < v[1] < Nt}


def same_thread(lo, hi, Nt, seg=None):
    """do the targets lo < hi meet in one thread of the search (same segment, congruent mod 16)?  Then the thread's own rule decides
    between them; otherwise the exact (distance, index) keys of two lanes or two segments do."""
    seg = Nt if seg is None or seg > Nt else seg
    return lo // seg == hi // seg and (hi - lo) % NN_LANES == 0


def _dist(d2):
    return np.sqrt(np.float32(d2) + np.float32(1e-7))


def _lanes(d2_row, take, seg=None):
    """the per-lane scan (targets sp, sp + 16, ... of a segment in order, `take(d2, best)` decides) and the merge of the lanes of
    all segments by (rounded distance, index): the shape of nn32seg_kernel with one row per thread (seg=None) and with two"""
    d2_row = np.asarray(d2_row, np.float32)
    n = len(d2_row)
    seg = n if seg is None or seg > n else seg
    best_key = None
    for t0 in range(0, n, seg):
        t1 = min(t0 + seg, n)
        for sp in range(min(NN_LANES, t1 - t0)):
            best, bi = np.float32(np.inf), 0
            for t in range(t0 + sp, t1, NN_LANES):
                if take(d2_row[t], best):
                    best, bi = d2_row[t], t
            key = (float(_dist(best)), bi)
            if best_key is None or key < best_key:
                best_key = key
    return best_key[1]


def kernel_rule_before_fix(d2_row, seg=None):
    """'L2' index of nn32seg_kernel (either row count) as it was: a later target of the lane wins without a square root when
    d2 < best (1 - 1e-6), a relative test on D2"""
    c = np.float32(F1 - np.float32(1e-6))

    def take(d2, best):
        return bool(d2 < best) and (bool(d2 < np.float32(best * c)) or bool(_dist(d2) < _dist(best)))
    return _lanes(d2_row, take, seg)


def kernel_rule(d2_row, seg=None):
    """'L2' index under nn_closer (csrc/nnmath.h): no square root where one fma on D2 proves the sums D2 + 1e-7 more than 9e-7
    apart, the rounded distances otherwise (the fma through f64: the product is exact there, the one extra rounding can move the
    threshold by an ulp, which the proof's slack covers)"""
    c, k = np.float64(np.float32(F1 - np.float32(1e-6))), np.float64(np.float32(1.1e-13))

    def take(d2, best):
        if not d2 < best:
            return False
        with np.errstate(invalid="ignore"):
            return bool(d2 < np.float32(np.float64(best) * c - k)) or bool(_dist(d2) < _dist(best))
    return _lanes(d2_row, take, seg)


def mutual_tie_case(Na, Nb, fwd, back, scale, filler="random", seed=0):
    """Two 32-D sets with rounded ties in BOTH search directions.  fwd: [(q, lo, hi)] - row q of a has the tie pair (lo, hi) in b;
    back: [(q, lo, hi)] - row q of b has it in a.  Cluster k sits at +-4 on axis 16 + k / 2 (queries exactly there) and its pair is
    displaced in the first 16 coordinates only, so that every difference is exact, as for a zero query.  Fillers: random rows of
    norm ~1 ('random'), or one row repeated through both sets ('identical': every filler pair is a candidate of the pre-filter and
    its list overflows).  The oracle must answer (q, lo) in each cluster: asserted here on the query rows.  -> a, b, expected pairs"""
    assert len(fwd) + len(back) <= 32
    for mine, theirs, n in ((fwd, back, (Na, Nb)), (back, fwd, (Nb, Na))):          # no row serves two clusters
        rows = [q for q, _, _ in mine] + [x for _, lo, hi in theirs for x in (lo, hi)]
        assert len(set(rows)) == len(rows) and all(0 <= r < n[0] for r in rows), rows
    rs = np.random.RandomState(seed)
    if filler == "identical":
        one = (rs.randn(1, 32) / np.sqrt(32)).astype(np.float32)
        a, b = np.repeat(one, Na, 0), np.repeat(one, Nb, 0)
    else:
        a = (rs.randn(Na, 32) / np.sqrt(32)).astype(np.float32)
        b = (rs.randn(Nb, 32) / np.sqrt(32)).astype(np.float32)
    far = np.zeros(32, np.float32)
    near = np.zeros(32, np.float32)
    far[:16] = scale / 4
    near[:16] = scale * (1.0 - TIE_GAP) / 4
    expect = []
    for k, (q, lo, hi) in enumerate(list(fwd) + list(back)):
        own, oth = (a, b) if k < len(fwd) else (b, a)
        c = np.zeros(32, np.float32)
        c[16 + k // 2] = 4.0 if k % 2 == 0 else -4.0
        assert lo < hi
        own[q], oth[lo], oth[hi] = c, c + far, c + near
        expect.append((q, lo) if k < len(fwd) else (lo, q))
    for k, (q, lo, hi) in enumerate(list(fwd) + list(back)):
        own, oth = (a, b) if k < len(fwd) else (b, a)
        _assert_rounded_tie(own[q], oth[lo], oth[hi])
        assert int(np.argmin(orc.pdist_l2(own[q:q + 1], oth)[0])) == lo
        assert int(np.argmin(orc.pdist_l2(own[q:q + 1], oth, squared=True)[0])) == hi
        assert int(np.argmin(orc.pdist_l2(oth[lo:lo + 1], own)[0])) == q
    return a, b, sorted(expect)


# ---------------------------------------------------------------------------------------------------------------------------------
# the pre-filter's band
# ---------------------------------------------------------------------------------------------------------------------------------
def band_case(No, Nt, queries, winners, rivals, flips=(1, 2, 1, 2), base=2.0 ** -3, fracs=(0.49, 0.51), query_mag=None, other_scale=1.0,
              limit=None, fillers="normal", seed=0):
    """One search direction of the matcher, `own` (No, 32) searching `other` (Nt, 32); -> own, other, clusters.

    base is an fp16 number, step the fp16 spacing above it; lo = f32(base + fracs[0] step) rounds DOWN to base in fp16 (0.49),
    hi = f32(base + fracs[1] step) rounds UP (0.51; a fraction below 0.5 rounds to base too).  Cluster k: signs s1, and s2 = s1 flipped in flips[k] places;
        own[queries[k]]   = query_mag s1 where s1 = s2, 0 elsewhere      (query_mag: an fp16 number, default base)
        other[winners[k]] = other_scale lo s1                            (the oracle's nearest neighbour)
        other[rivals[k]]  = other_scale hi s2                            (what the fp16 Gram scores prefer)
    other_scale is a power of two (the midpoints stay midpoints).  The other rows are N(0, (base / 2)^2), those of `other` times
    other_scale, clipped to +-limit where given (fillers='normal'); or rows of random signs, base in `own` and other_scale hi in
    `other` - the rival's norm exactly ('signs': once the sets differ in scale, small rows would lie between query and winner).  Asserted on the oracle for every cluster: the query's first minimum over `other` is
    the winner, the rival comes second, and the winner's nearest row of `own` is the query (the pair is a mutual match).
    clusters: [{q, w, r, ulps: 'L2' gap winner -> rival in fp32 ulps}]"""
    rs = np.random.RandomState(seed)
    step = float(np.spacing(np.float16(base)))
    lo, hi = np.float32(base + fracs[0] * step), np.float32(base + fracs[1] * step)
    assert float(np.float16(base)) == base and lo != hi
    for v, f in ((lo, fracs[0]), (hi, fracs[1])):
        assert -0.25 < f < 1 and float(np.float16(v)) == (base if f < 0.5 else base + step), (base, v, f)
    qm = np.float32(base if query_mag is None else query_mag)
    assert float(np.float16(qm)) == float(qm)
    sc = np.float32(other_scale)
    assert np.log2(float(sc)) == int(np.log2(float(sc)))
    if fillers == "signs":
        own = np.float32(base) * rs.choice(np.array([-1.0, 1.0], np.float32), (No, 32))
        other = sc * hi * rs.choice(np.array([-1.0, 1.0], np.float32), (Nt, 32))
    else:
        assert fillers == "normal"
        own = (rs.randn(No, 32) * 0.5 * base).astype(np.float32)
        other = (rs.randn(Nt, 32) * 0.5 * base).astype(np.float32) * sc
    if limit is not None:
        own, other = np.clip(own, -limit, limit), np.clip(other, -limit * float(sc), limit * float(sc))
    assert len(set(queries)) == len(queries) and not set(winners) & set(rivals)
    for k, (q, w, r) in enumerate(zip(queries, winners, rivals)):
        s1 = rs.choice(np.array([-1.0, 1.0], np.float32), 32)
        s2 = s1.copy()
        s2[rs.permutation(32)[:flips[k % len(flips)]]] *= -1
        own[q] = qm * s1 * (s1 == s2)
        other[w] = sc * lo * s1
        other[r] = sc * hi * s2
    clusters = []
    for q, w, r in zip(queries, winners, rivals):
        d = orc.pdist_l2(own[q:q + 1], other)[0]
        order = np.argsort(d, kind="stable")
        assert (int(order[0]), int(order[1])) == (w, r), (q, w, r, order[:3], d[order[:3]])
        assert int(np.argmin(orc.pdist_l2(other[w:w + 1], own)[0])) == q
        clusters.append({"q": q, "w": w, "r": r, "ulps": ulps(d[w], d[r])})
    return own, other, clusters


def as_sets(own, other, direction):
    """(a, b) of yoho_mutual_nn: direction 0 - the rows of a search b; 1 - the rows of b search a"""
    return (own, other) if direction == 0 else (other, own)


def pair_of(cluster, direction):
    """the (row of a, row of b) match of a cluster"""
    return (cluster["q"], cluster["w"]) if direction == 0 else (cluster["w"], cluster["q"])


class Prefilter:
    """what emu_prefilter returns: score (No, Nt) f32, rowmin (No), band (No), cand (No, Nt) bool"""

    def __init__(self, score, rowmin, band):
        self.score, self.rowmin, self.band = score, rowmin, band
        self.cand = score <= (rowmin + band)[:, None]

    def share(self, q, w):
        """the part of the query's band that the true winner's score lies above the row minimum"""
        return float((np.float64(self.score[q, w]) - np.float64(self.rowmin[q])) / np.float64(self.band[q]))


def prefilter_declines(a, b):
    """mf_norms_kernel's range check: non-finite, a squared norm above 1e30 or a magnitude above 6.0e4 -> brute force answers"""
    for x in (a, b):
        x = np.asarray(x, np.float32)
        n2 = (x.astype(np.float64) ** 2).sum(1)
        if not np.isfinite(x).all() or not (n2 <= 1e30).all() or not (np.abs(x) <= np.float32(6.0e4)).all():
            return True
    return False


def emu_prefilter(a, b, c0=4.5e-3, max_from="other"):
    """The rows of a searching b as mf_gram_kernel sees them (csrc/matchf.hip): score_ij = |b_j|^2 - 2 G_ij with G from the
    fp16-rounded rows (products exact, summed in f64, rounded once to f32 - the MFMA's own order differs by < 32 * 2^-24 relative),
    the row minimum, and band_of's formula
        band_i = c0 |a_i| M + 2e-5 (|a_i| + M)^2 + 4e-6 (|a_i| + M) + 1e-30,   norms times 1.000001
    with M the largest norm of b (max_from='other', what ships) or of a ('own': the mutant that reads the wrong maximum)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    with np.errstate(over="ignore"):
        a16, b16 = a.astype(np.float16).astype(np.float64), b.astype(np.float16).astype(np.float64)
    G = (a16 @ b16.T).astype(np.float32)
    na2 = (a.astype(np.float64) ** 2).sum(1).astype(np.float32)
    nb2 = (b.astype(np.float64) ** 2).sum(1).astype(np.float32)
    score = nb2[None, :] - np.float32(2) * G
    rowmin = score.min(1)
    m2 = nb2.max() if max_from == "other" else na2.max()
    assert max_from in ("other", "own")
    k = np.float32(1.000001)
    mine, oth = np.sqrt(na2) * k, np.sqrt(m2) * k
    s = mine + oth
    band = np.float32(c0) * mine * oth + np.float32(2e-5) * s * s + np.float32(4e-6) * s + np.float32(1e-30)
    return Prefilter(score, rowmin, band.astype(np.float32))


def candidate_cap(Na, Nb):
    """mutual_prefilter_layout's room for candidates (a pair inside both its bands is listed once per direction)"""
    return 32 * (Na + Nb) + 4000


def emu_candidates(a, b):
    """candidates of both directions under the shipped band: above candidate_cap the list overflows and brute force answers"""
    return int(emu_prefilter(a, b).cand.sum()) + int(emu_prefilter(b, a).cand.sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases both suites run
# ---------------------------------------------------------------------------------------------------------------------------------
BAND_SIZES = ((1024, 1024), (1153, 1000), (1025, 1023))     # (Na, Nb): exactly 2^20 pairs; ragged against 128 own rows and 32-row tiles;
#                                                             one pair short of the switch (brute force answers)


def band_rows(No, Nt, winner_first=False):
    """queries at own rows 0, 127, 128 and the last one (the edges of the 128 rows a workgroup owns); rivals in tile 0 of the other
    set, winners at its end - the last, ragged 32-row tile (its last four rows, so up to three sit in the tile before when the
    ragged one is shorter).  winner_first: the two swapped (for a tie of the rounded distances the lower index has to be the winner)"""
    q = [0, 127, 128, No - 1]
    first, last = [0, 5, 17, 31], [Nt - 1, Nt - 2, Nt - 3, Nt - 4]
    return (q, first, last) if winner_first else (q, last, first)


def band_standard(Na, Nb, direction):
    """the construction of band_case at 2^-3 in one direction -> a, b, clusters"""
    No, Nt = (Na, Nb) if direction == 0 else (Nb, Na)
    q, w, r = band_rows(No, Nt)
    own, other, cl = band_case(No, Nt, q, w, r, seed=100 + direction)
    return as_sets(own, other, direction) + (cl,)


# name -> (keyword arguments of band_case, winner_first, does the band read from the wrong set's maximum lose the winner?)
BAND_VARIANTS = {
    # the other set 32 times larger: the own set's maximum norm gives a band 8 times too narrow.  The query at 4 x base, or the
    # norm term 32 |b|^2 of the score (exact in fp32, in the winner's favour) eats most of the Gram term's deficit.
    "other x 32": (dict(other_scale=32.0, query_mag=4 * 2.0 ** -3, fillers="signs"), False, True),
    # the other set 32 times smaller: the score is the dot product alone, the winner has the LARGER one, and rounding is monotone -
    # the most the fp16 scores can do is to call the two equal (both round to base) and let the norm term prefer the rival.  The own
    # set's maximum gives a WIDER band here: this mutant cannot lose the winner.
    "other / 32": (dict(other_scale=1.0 / 32, fracs=(0.49, -0.24), fillers="signs"), False, False),
    # fp16 subnormals (spacing 2^-24 whatever the magnitude: the rounding error is absolute).  D2 is ~1e-10, far below the 1e-7 of
    # the sum: the winner's lead is 2 - 4 ulps of the 'L2' distance.  It sits at the lower index (tile 0), the rival at the end.
    "fp16 subnormal": (dict(base=2.0 ** -16), True, False),
    # magnitudes up to exactly 6.0e4, the last value the range check admits (fp16 spacing 32): hi rounds up to 6.0e4, the query is 6.0e4
    "up to 6.0e4": (dict(base=6.0e4 - 32, query_mag=6.0e4, limit=6.0e4), False, False),
}
VARIANT_SIZE = (1153, 1000)


def band_variant(name, direction):
    """-> a, b, clusters"""
    kw, winner_first, _ = BAND_VARIANTS[name]
    Na, Nb = VARIANT_SIZE
    No, Nt = (Na, Nb) if direction == 0 else (Nb, Na)
    q, w, r = band_rows(No, Nt, winner_first)
    own, other, cl = band_case(No, Nt, q, w, r, seed=200 + direction, **kw)
    return as_sets(own, other, direction) + (cl,)


MUTUAL_TIE_SIZES = {"below 2^20 pairs": (1025, 1023), "above": (1153, 1000)}


def mutual_tie_rows(Na, Nb):
    """tie clusters of both directions: query rows at the edges of a 32-row block, pairs one thread apart (i, i + 16), a tile apart
    (i, i + 256), in two threads, and at the end of the set (the last row is a query of the other direction)"""
    fwd = [(0, 2, 18), (15, 3, 3 + NN_TILE), (16, 5, 7), (31, Nb - 18, Nb - 2), (Na - 1, 40, 56)]
    back = [(0, 2, 18), (15, 3, 3 + NN_TILE), (16, 5, 7), (31, Na - 17, Na - 2), (Nb - 1, 40, 56)]
    return fwd, back
