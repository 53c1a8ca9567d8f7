"""Nearest-neighbour searches on the GPU (-m gpu) at rounded ties and at the edge of the pre-filter's band.  Every assertion is
against the oracle (tests/nn_ref.py: argmin of orc.pdist_l2 per row, orc.mutual_match): indices exactly, distances as bits, no
device path compared with another alone.  tests/test_nn_cpu.py shows on the CPU that these inputs reach what they are built for.

  * rounded ties: two targets whose D2 differ by 8e-6 relative and whose 'L2' distances sqrt(D2 + 1e-7) have equal bits, the larger
    D2 at the lower index.  The reference answers the lower index under 'L2', the higher under 'SquareL2'.  yoho_nn_search (nn32seg_kernel:
    one row per thread below 2^20 pairs, two from there), yoho_knn_search(k = 1) and the four paths of yoho_mutual_nn.  Until nn_closer
    (csrc/nnmath.h) the brute-force kernels decided on D2 alone and returned the later index wherever one thread visited both
    targets (same segment, indices congruent mod 16): those cases failed for yoho_nn_search, for yoho_mutual_nn below 2^20 pairs,
    with the pre-filter off, and behind an overflowing candidate list;
  * band cases: the true neighbour's fp16 Gram score lies 0.40 of the candidate band above a rival's (0.34 / 0.22 / 0.08 / 0.01 in the
    variants): a narrower band, a band from the wrong set's maximum norm, or a row minimum lost between column splits or in a ragged
    tile drops the neighbour and the match list differs from the oracle's."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nn_ref as R  # noqa: E402

orc = R.orc
pytestmark = pytest.mark.gpu
SMALL = ((5, 700), (33, 513))                                           # one-row nn32seg_kernel: below 2^20 pairs
SEGMENTED = ((1024, 1024), (33, 32000), (4100, 257), (16384, 600))      # nn32seg_kernel; the last one has two tiles per segment


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.Context()


@pytest.fixture(scope="module")
def split_ctxs(hip):
    """contexts created with YOHO_NN_SPLITS unset (two workgroups per CU: ~30 column splits of two tiles at these sizes), 1 and 3"""
    old = os.environ.pop("YOHO_NN_SPLITS", None)
    out = {}
    try:
        for s in (None, 1, 3):
            if s is not None:
                os.environ["YOHO_NN_SPLITS"] = str(s)
            out[s] = hip.Context()
    finally:
        os.environ.pop("YOHO_NN_SPLITS", None)
        if old is not None:
            os.environ["YOHO_NN_SPLITS"] = old
    return out


_oracle = {}


def mutual_ref(key, a, b):
    """orc.mutual_match, once per data set"""
    if key not in _oracle:
        _oracle[key] = orc.mutual_match(a, b)
    return _oracle[key]


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def tie_cases(D, Ns, Nt):
    """(what, src, tgt, lo, hi, one thread visits both) for every placement and scale of a shape"""
    segmented = Ns * Nt >= R.SEG_PAIRS
    seg = R.seg_len(Ns, Nt, n_cu())[0] if segmented else None           # nn_segment_plan's segLen, restated (tests/nn_ref.py)
    src = R.tie_sources(D, Ns)
    for name, (lo, hi) in R.tie_placements(Nt, seg).items():
        for scale in R.TIE_SCALES:
            yield (D, Ns, Nt, seg, name, lo, hi, scale), src, R.rounded_tie_targets(D, Nt, [(lo, hi)], scale), lo, hi, R.same_thread(lo, hi, Nt, seg)


@pytest.mark.parametrize("D", [32, 3])
@pytest.mark.parametrize("sq", [False, True], ids=["L2", "SquareL2"])
def test_nn_search_rounded_ties(ctx, D, sq):
    """tie pairs at (i, i + 16), (i, i + 256), (i, i + 2), across a tile and a segment boundary and up to the last row (inside the
    last, ragged tile at 700, 1024, 32000 and 600 targets); the zero query at rows 0, 7, 15, 16, 31 and Ns - 1 (both rows of a thread
    of nn32seg_kernel, one of the two, and its clamped tail), ones elsewhere.  Indices and distance bits of yoho_nn_search and of
    yoho_knn_search(k = 1) equal the oracle's."""
    assert all(ns * nt < R.SEG_PAIRS for ns, nt in SMALL) and all(ns * nt >= R.SEG_PAIRS for ns, nt in SEGMENTED)
    n = met = 0
    for Ns, Nt in SMALL + SEGMENTED:
        sd = None
        shape_met = 0
        for what, src, tgt, lo, hi, one in tie_cases(D, Ns, Nt):
            sd = cu(src) if sd is None else sd
            td = cu(tgt)
            ri, rd = R.nn_ref(src, tgt, sq)
            zero = ~src.any(1)
            assert (ri[zero] == (hi if sq else lo)).all() and (ri[~zero] == min(set(range(3)) - {lo, hi})).all(), what
            d, i = ctx.nn_search(sd, td, want_dist=True, squared=sq)
            assert np.array_equal(i.cpu().numpy(), ri), (what, "yoho_nn_search", i.cpu().numpy()[zero][:1], ri[zero][:1])
            assert np.array_equal(R.bits(d.cpu().numpy()), R.bits(rd)), (what, "yoho_nn_search distances")
            _, i0 = ctx.nn_search(sd, td, want_dist=False, squared=sq)
            assert np.array_equal(i0.cpu().numpy(), ri), (what, "yoho_nn_search without distances")
            kd, ki = ctx.knn_search(sd, td, 1, squared=sq)
            assert np.array_equal(ki.cpu().numpy()[:, 0], ri) and np.array_equal(R.bits(kd.cpu().numpy()[:, 0]), R.bits(rd)), (what, "yoho_knn_search(1)")
            n += 1
            shape_met += one
        assert shape_met >= 3, (Ns, Nt)                    # every shape has pairs that one thread visits
        met += shape_met
    print(f"D = {D}, squared = {sq}: {n} tie cases ({met} with both targets in one thread) identical to the oracle in indices and distance bits")


MUTUAL_PATHS = {
    # name: (size, fillers, pre-filter)
    "below 2^20 pairs": ("below 2^20 pairs", "random", True),
    "brute force": ("above", "random", False),
    "pre-filter": ("above", "random", True),
    "pre-filter, candidate list full": ("above", "identical", True),
}


@pytest.mark.parametrize("path", list(MUTUAL_PATHS))
def test_mutual_nn_rounded_ties(hip, path):
    """ties in both directions (rows of a against b, rows of b against a) through nn32seg_kernel (one and two rows per thread), the pre-filter's exact
    candidates, and the fallback behind a candidate list that identical rows overflow: the match list is orc.mutual_match's and holds
    (query, lower index) of every cluster"""
    size, filler, pre = MUTUAL_PATHS[path]
    Na, Nb = R.MUTUAL_TIE_SIZES[size]
    fwd, back = R.mutual_tie_rows(Na, Nb)
    c = hip.Context()
    c.set_nn_prefilter(pre)
    for scale in R.TIE_SCALES:
        a, b, expect = R.mutual_tie_case(Na, Nb, fwd, back, scale, filler)
        ref = mutual_ref(("ties", size, filler, scale), a, b)
        have = set(map(tuple, ref.tolist()))
        assert all(p in have for p in expect)
        m = c.mutual_nn(cu(a), cu(b)).cpu().numpy()
        wrong = [p for p in expect if p not in set(map(tuple, m.tolist()))]
        assert m.shape == ref.shape and np.array_equal(m, ref), (path, scale, "missing", wrong)


def check_band(ctxs, key, a, b, cl, direction):
    ref = mutual_ref(key, a, b)
    have = set(map(tuple, ref.tolist()))
    assert all(R.pair_of(c, direction) in have for c in cl)
    ad, bd = cu(a), cu(b)
    for s, c in ctxs.items():
        m = c.mutual_nn(ad, bd).cpu().numpy()
        got = set(map(tuple, m.tolist()))
        lost = [R.pair_of(x, direction) for x in cl if R.pair_of(x, direction) not in got]
        assert m.shape == ref.shape and np.array_equal(m, ref), (key, "YOHO_NN_SPLITS", s, "adversarial pairs lost", lost)
    return len(ref)


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("size", R.BAND_SIZES, ids=lambda s: "%dx%d" % s)
def test_mutual_nn_band_cases(split_ctxs, size, direction):
    """adversarial queries at own rows 0, 127, 128 and the last one, their rivals in tile 0 of the other set and the true
    neighbours at its end (the last, ragged tile), so that rival and neighbour fall into different column splits unless there is one
    split.  1025 x 1023 is one pair short of the pre-filter's threshold: the one-row nn32seg_kernel answers, and has to give the same list."""
    a, b, cl = R.band_standard(*size, direction)
    assert (size[0] * size[1] >= R.SEG_PAIRS) == (size != (1025, 1023))
    n = check_band(split_ctxs, ("band", size, direction), a, b, cl, direction)
    print(f"{size[0]} x {size[1]}, direction {direction}: {n} matches identical to the oracle with 1, 3 and the default column splits")


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("name", list(R.BAND_VARIANTS))
def test_mutual_nn_band_variants(split_ctxs, name, direction):
    """one set 32 times larger / smaller than the other (a band from the wrong set's maximum is 8 times too narrow in the first),
    fp16 subnormals, and magnitudes up to exactly 6.0e4, the last the range check admits"""
    a, b, cl = R.band_variant(name, direction)
    check_band(split_ctxs, ("variant", name, direction), a, b, cl, direction)


def test_poisoned_scratch_two_contexts(hip):
    """a context whose workspace is filled with NaN / all-ones patterns before every call, beside one that never is: the oracle's
    answers from both, the same bytes, twice"""
    clean, dirty = hip.Context(), hip.Context()
    calls = []
    for D, (Ns, Nt) in ((32, (1024, 1024)), (3, (4100, 257)), (32, (33, 513))):
        what, src, tgt, lo, hi, one = next(x for x in tie_cases(D, Ns, Nt) if x[5])
        ri, rd = R.nn_ref(src, tgt)
        sd, td = cu(src), cu(tgt)
        calls.append((what, lambda c, sd=sd, td=td: c.nn_search(sd, td)[::-1], (ri, rd)))
        calls.append((what, lambda c, sd=sd, td=td: tuple(x[:, 0] for x in c.knn_search(sd, td, 1)[::-1]), (ri, rd)))
    Na, Nb = R.MUTUAL_TIE_SIZES["above"]
    for filler in ("random", "identical"):
        a, b, _ = R.mutual_tie_case(Na, Nb, *R.mutual_tie_rows(Na, Nb), R.TIE_SCALES[1], filler)
        ad, bd = cu(a), cu(b)
        calls.append((("ties", filler), lambda c, ad=ad, bd=bd: (c.mutual_nn(ad, bd),), (mutual_ref(("ties", "above", filler, R.TIE_SCALES[1]), a, b),)))
    for key, (a, b, cl) in ((("band", (1153, 1000), 0), R.band_standard(1153, 1000, 0)), (("variant", "fp16 subnormal", 1), R.band_variant("fp16 subnormal", 1))):
        ad, bd = cu(a), cu(b)
        calls.append((key, lambda c, ad=ad, bd=bd: (c.mutual_nn(ad, bd),), (mutual_ref(key, a, b),)))
    for pre in (True, False):
        clean.set_nn_prefilter(pre)
        dirty.set_nn_prefilter(pre)
        for what, run, ref in calls:
            first = [x.cpu().numpy() for x in run(clean)]
            for got, want in zip(first, ref):
                assert got.shape == want.shape and got.tobytes() == np.ascontiguousarray(want, got.dtype).tobytes(), (what, pre)
            for pattern in (0xFFFFFFFF, 0x7FC00000, 0x00000000):
                for rep in range(2):
                    dirty.poison_scratch(pattern)
                    again = [x.cpu().numpy() for x in run(dirty)]
                    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, again)), (what, pre, hex(pattern), rep)
            assert all(x.cpu().numpy().tobytes() == y.tobytes() for x, y in zip(run(clean), first)), (what, pre, "second call")
