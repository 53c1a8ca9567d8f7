"""GPU tests (-m gpu): the irrep GEMMs of the two large PartI layers on the 16x16x32 MFMA (K32 stages), in the three blockings
(fgemm: 256 x 256 tiles in eight waves, the default | fgemm256: four waves | fgemm128: 256 x 128 tiles).

Sizes at the edges of the 32-keypoint slab tile and of the 256-column GEMM tile, and a pair pass whose fragment boundary (33 + 31) lies
inside a column tile.  Every case runs once clean and is checked against the float64 oracle at the tolerance test_gpu_kernels.py uses
for these modes; then it must give the same bits on a repeat, with the context's scratch and the outputs poisoned the way
test_gpu_scratch.py does it, and in all three blockings (they issue the same products in the same order per accumulator).  No call may
raise the fp16 range flag, and no pass may be repeated in bf16x3."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import yoho_oracle as orc  # noqa: E402
from yoho_amd import synth  # noqa: E402
from test_gpu_kernels import TOL, rel, rel_rows, cu  # noqa: E402
from test_gpu_scratch import outp, poisoned_runs, same_bits, checked  # noqa: E402,F401  (outp: fixture)

pytestmark = pytest.mark.gpu
MODES = ("fgemm", "fgemm256", "fgemm128")
SIZES = (1, 31, 32, 33, 255, 256, 257)
PAIR = (33, 31)


@pytest.fixture(scope="module")
def data(sd1, tables):
    """257 rows for the single passes (each reads a prefix) and 64 more for the pair pass; the oracle once, over all of them"""
    X = synth.unit_features(max(SIZES) + sum(PAIR), seed=811)
    e, i = orc.partI_forward(X, sd1, tables.N)
    return cu(X), e, i


@pytest.fixture(scope="module")
def ctxs(hip, sd1):
    cs = {}
    for m in MODES:
        c = hip.Context()
        c.load_partI(sd1)
        c.set_gconv_mode(m)
        cs[m] = c
    yield cs
    for c in cs.values():
        assert c.range_fallbacks == 0, c.range_report()


def check_oracle(out, e, i, what):
    eqv, inv, inv_np = (out[n].cpu().numpy() for n in ("eqv", "inv", "inv_np"))
    assert np.isfinite(eqv).all() and np.isfinite(inv).all(), what
    errs = rel(eqv, e), rel(inv, i), rel_rows(eqv, e), rel_rows(inv, i), rel_rows(inv_np, np.mean(e, axis=-1))
    assert max(errs) < TOL, (what, errs)


def run_everywhere(ctxs, outp, call, e, i, what):
    """call(context) in every blocking: oracle, repeat, poisoned scratch and outputs, then the blockings against one another"""
    refs = {}
    for m, c in ctxs.items():
        run = lambda: checked(c, lambda: call(c))
        ref = run()
        check_oracle(ref, e, i, (m, what))
        same_bits(ref, run(), (m, what, "repeat"))
        poisoned_runs(outp, run, ref, (m, what), ctx=c)
        refs[m] = ref
        assert c.range_fallbacks == 0, (m, what, c.range_report())
    for m in MODES[1:]:
        same_bits(refs[MODES[0]], refs[m], (MODES[0], m, what))


@pytest.mark.parametrize("B", SIZES)
def test_partI_sizes(ctxs, data, outp, B):
    Xd, e, i = data
    x = Xd[:B]
    run_everywhere(ctxs, outp, lambda c: c.partI_forward(x, want_inv=True, want_inv_np=True, check_range=False), e[:B], i[:B], B)


def test_partI_pair_with_the_fragment_boundary_inside_a_column_tile(ctxs, data, outp):
    Xd, e, i = data
    lo = max(SIZES)
    x0, x1 = Xd[lo:lo + PAIR[0]], Xd[lo + PAIR[0]:lo + sum(PAIR)]
    run_everywhere(ctxs, outp, lambda c: c.partI_forward_pair(x0, x1, want_inv=True, want_inv_np=True, check_range=False),
                   e[lo:lo + sum(PAIR)], i[lo:lo + sum(PAIR)], PAIR)
