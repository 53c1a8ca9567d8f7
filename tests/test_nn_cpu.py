"""The inputs of tests/test_gpu_nn.py, checked where no device is needed: every generator of tests/nn_ref.py is shown on the oracle
(and on emulations of what the device does before the exact distance decides) to reach the place it is built for.

  * rounded ties: the oracle answers the lower index under 'L2' and the higher one under 'SquareL2'; the rule
    nn32seg_kernel had answers the higher one under 'L2' wherever one thread visits both (same segment, congruent mod 16), the rule
    they have now (nn_closer) the oracle's;
  * the pre-filter's band: in every standard case the true neighbour's fp16 Gram score lies >= 0.35 of the shipped band above the row
    minimum (a band half as wide would keep a 30 % margin, a leading constant of 1.5e-3 loses the neighbour); the asymmetric, fp16
    subnormal and 6.0e4 variants with the share of the band each reaches (printed; `pytest -s`, profiles/nn_ties.md)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nn_ref as R  # noqa: E402

orc = R.orc
SEGS = {700: (None,), 513: (None,), 1024: (64,), 257: (64,), 600: (304,)}       # target counts of the GPU cases with a segment length they meet


@pytest.mark.parametrize("D", [32, 3])
@pytest.mark.parametrize("scale", R.TIE_SCALES)
def test_rounded_ties_oracle_and_both_rules(D, scale):
    z = np.zeros((1, D), np.float32)
    hit = 0
    for Nt, segs in SEGS.items():
        for seg in segs:
            for name, (lo, hi) in R.tie_placements(Nt, seg).items():
                tgt = R.rounded_tie_targets(D, Nt, [(lo, hi)], scale)
                d2 = orc.pdist_l2(z, tgt, squared=True)[0]
                dl = orc.pdist_l2(z, tgt)[0]
                what = (D, scale, Nt, seg, name, lo, hi)
                assert int(np.argmin(dl)) == lo and int(np.argmin(d2)) == hi, what
                assert R.bits(dl)[lo] == R.bits(dl)[hi] and d2[lo] > d2[hi], what
                assert R.nn_ref(z, tgt)[0][0] == lo and R.nn_ref(z, tgt, squared=True)[0][0] == hi, what
                one = R.same_thread(lo, hi, Nt, seg)
                assert R.kernel_rule_before_fix(d2, seg) == (hi if one else lo), what
                assert R.kernel_rule(d2, seg) == lo, what
                hit += one
    assert hit >= 8                                        # the placements do meet in one thread


def test_rule_equals_oracle_around_its_margin():
    """rows of D2 values spaced around the margin of nn_closer (sums 1e-6 apart) and far inside it, at magnitudes from far below
    the 1e-7 of the sum to far above it: the first minimum of the rounded distances, whatever the order of the targets"""
    rs = np.random.RandomState(5)
    n = 0
    for mag in (1e-15, 1e-10, 1e-8, 1e-7, 1e-6, 1e-3, 1.0, 1e4):
        for spread in (1e-8, 1e-7, 5e-7, 1e-6, 2e-6, 1e-5):
            for _ in range(6):
                base = (mag + 1e-7) * (1.0 + spread * rs.randint(-4, 5, 96)) - 1e-7
                d2 = np.maximum(base, 0).astype(np.float32)
                want = int(np.argmin(np.sqrt(d2 + np.float32(1e-7))))
                assert R.kernel_rule(d2) == want and R.kernel_rule(d2, 32) == want, (mag, spread)
                n += 1
    assert n == 288


@pytest.mark.parametrize("size", list(R.MUTUAL_TIE_SIZES))
@pytest.mark.parametrize("filler", ["random", "identical"])
def test_mutual_tie_cases(size, filler):
    """mutual_tie_case asserts the ties on the oracle; here: which path of yoho_mutual_nn the case takes, by the emulated pre-filter"""
    Na, Nb = R.MUTUAL_TIE_SIZES[size]
    fwd, back = R.mutual_tie_rows(Na, Nb)
    for scale in R.TIE_SCALES:
        a, b, expect = R.mutual_tie_case(Na, Nb, fwd, back, scale, filler)
        assert len(expect) == len(fwd) + len(back)
        assert (Na * Nb >= R.SEG_PAIRS) == (size == "above")
        assert not R.prefilter_declines(a, b)
        n, cap = R.emu_candidates(a, b), R.candidate_cap(Na, Nb)
        assert (n > cap) == (filler == "identical"), (n, cap)              # identical fillers: the list overflows, the fallback answers
        for q, lo, hi in fwd:                                              # both rows of a pair are candidates of their query
            assert R.emu_prefilter(a[q:q + 1], b).cand[0, [lo, hi]].all()
        # the rule the brute-force kernels had returns the later row of each pair one thread visits
        for q, lo, hi in fwd:
            d2 = orc.pdist_l2(a[q:q + 1], b, squared=True)[0]
            assert R.kernel_rule(d2) == lo
            assert R.kernel_rule_before_fix(d2) == (hi if R.same_thread(lo, hi, Nb) else lo)


def _figures(own, other, cl):
    e = R.emu_prefilter(own, other)
    narrow = R.emu_prefilter(own, other, c0=1.5e-3)
    wrong = R.emu_prefilter(own, other, max_from="own")
    return [(c, e.share(c["q"], c["w"]), bool(e.cand[c["q"], c["w"]]), narrow.share(c["q"], c["w"]), bool(narrow.cand[c["q"], c["w"]]),
             wrong.share(c["q"], c["w"]), bool(wrong.cand[c["q"], c["w"]]), int(np.argmin(e.score[c["q"]]))) for c in cl]


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("size", R.BAND_SIZES)
def test_band_standard_cases(size, direction):
    a, b, cl = R.band_standard(*size, direction)
    own, other = (a, b) if direction == 0 else (b, a)
    assert not R.prefilter_declines(a, b) and R.emu_candidates(a, b) < R.candidate_cap(*size) // 4
    for c, share, kept, nshare, nkept, wshare, wkept, pref in _figures(own, other, cl):
        print(f"{size[0]} x {size[1]}, direction {direction}, query {c['q']}: winner {c['w']} ahead by {c['ulps']} ulps of the distance; "
              f"its score {share:.3f} of the band above the rival's ({nshare:.3f} of a band with 1.5e-3)")
        assert pref == c["r"]                              # the fp16 scores prefer the rival
        assert share >= 0.35
        assert kept and not nkept


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("name", list(R.BAND_VARIANTS))
def test_band_variants(name, direction):
    a, b, cl = R.band_variant(name, direction)
    own, other = (a, b) if direction == 0 else (b, a)
    separates = R.BAND_VARIANTS[name][2]
    assert not R.prefilter_declines(a, b) and R.emu_candidates(a, b) < R.candidate_cap(*R.VARIANT_SIZE) // 2
    if name == "fp16 subnormal":
        assert max(np.abs(own).max(), np.abs(other).max()) < 6.1e-5
    if name == "up to 6.0e4":
        assert np.abs(own).max() == 6.0e4 and np.abs(other).max() == 6.0e4 and (other.astype(np.float16) == 6.0e4).any()
    for c, share, kept, nshare, nkept, wshare, wkept, pref in _figures(own, other, cl):
        print(f"{name}, direction {direction}, query {c['q']}: winner {c['w']} ahead by {c['ulps']} ulps; {share:.4f} of the shipped band, "
              f"{wshare:.4f} of the band from the wrong set's maximum ({'lost' if not wkept else 'kept'})")
        assert pref == c["r"] and share > 0                # the rival is preferred: the winner is found through the band only
        assert kept
        assert wkept == (not separates)
