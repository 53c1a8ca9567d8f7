"""GPU tests (-m gpu): several tiles per workgroup in the two large irrep GEMMs (fgemm3k_kernel, csrc/gemmf2.hip).

A context created under YOHO_FGEMM_TILES=R lets a workgroup of the 256 -> 512 and 512 -> 256 launches take up to R tiles, drawn one by one
from a per-XCD ticket counter, with the next tile's DMA issued behind the last stage of the current one.  The tiles, the product order
per accumulator and the epilogue are those of one tile per workgroup, so every R must give the bits of R = 1 (the static work map, no
ticket) and of the two reference blockings fgemm256 / fgemm128, which have no tickets at all.

Shapes: up to 256 keypoints are 120 tiles of the 256 -> 512 launch, 15 per XCD - a list no longer than an XCD's 32 CUs, which the launch
leaves on the static map whatever R says (every tile has a CU to itself): these sizes pin that decision at the edges of the slab and column
tiles.  1500 keypoints are 720 tiles, 90 per XCD, handed out by tickets to ceil(90 / R) + 31 workgroups per XCD: with R = 2 that is more
workgroups than CUs, so late workgroups find few tickets or none; with R = 16 or 64 about as many workgroups as CUs walk the list three
tiles deep, through irreps of different dimension and stage count.  The 4100-keypoint case has 120 tiles per XCD and chunk.  Before every pass the
workspace and the outputs are filled with the largest finite fp16 / fp16 +inf: a tile nobody took leaves that in the descriptors and
raises the range flag.  The ticket counters must be zero again when a launch ends: passes are queued back to back, the first on OTHER
keypoints, without a host wait in between - counters that were not cleared hand out no tile in the second pass, which then returns the
first one's coefficients."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import yoho_oracle as orc  # noqa: E402
from yoho_amd import synth  # noqa: E402
from test_gpu_kernels import TOL, rel, rel_rows, cu  # noqa: E402
from test_gpu_scratch import outp, same_bits, checked  # noqa: E402,F401  (outp: fixture)

pytestmark = pytest.mark.gpu
TILES = (1, 2, 3, 16, 64)
REFS = ("fgemm256", "fgemm128")
SIZES = (1, 33, 255, 256, 257, 1500)
PAIR = (33, 31)
PATTERNS = (0x7BFF7BFF, 0x7C007C00)
NX = max(SIZES) + sum(PAIR)
ORC = np.r_[0:257, max(SIZES) - 40:NX]           # input rows the oracle is evaluated on: the small passes, the tail of the large one, the pair


@pytest.fixture(scope="module")
def data(sd1, tables):
    X = synth.unit_features(NX, seed=823)
    e, i = orc.partI_forward(X[ORC], sd1, tables.N)
    pos = np.full(NX, -1, np.int64)
    pos[ORC] = np.arange(len(ORC))
    return cu(X), e, i, pos


@pytest.fixture(scope="module")
def ctxs(hip, sd1):
    """contexts by tiles per workgroup (mode 'fgemm'), and the two blockings without tickets"""
    cs = {}
    with pytest.MonkeyPatch.context() as mp:
        for R in TILES:
            mp.setenv("YOHO_FGEMM_TILES", str(R))
            cs[R] = hip.Context()
    for m in REFS:
        cs[m] = hip.Context()
    for k, c in cs.items():
        c.load_partI(sd1)
        c.set_gconv_mode(k if k in REFS else "fgemm")
    yield cs
    for c in cs.values():
        assert c.range_fallbacks == 0, c.range_report()


def check_oracle(out, rows, data, what):
    _, e, i, pos = data
    k = pos[rows]
    sel = k >= 0
    assert sel.any(), what
    eqv, inv, inv_np = (out[n].cpu().numpy()[sel] for n in ("eqv", "inv", "inv_np"))
    e, i = e[k[sel]], i[k[sel]]
    assert np.isfinite(out["eqv"].cpu().numpy()).all() and np.isfinite(out["inv"].cpu().numpy()).all(), what
    errs = rel(eqv, e), rel(inv, i), rel_rows(eqv, e), rel_rows(inv, i), rel_rows(inv_np, np.mean(e, axis=-1))
    assert max(errs) < TOL, (what, errs)


def poisoned(c, outp, pattern, call):
    """call(c) with the context's scratch and the outputs filled with `pattern`; no range flag, no repeat"""
    c.poison_scratch(pattern)
    outp.pattern = pattern
    try:
        out = checked(c, lambda: call(c))
    finally:
        outp.pattern = None
    assert c.range_fallbacks == 0, c.range_report()
    return out


def run_everywhere(ctxs, outp, call, rows, data, what):
    ref = None
    for k, c in ctxs.items():
        for p in PATTERNS:
            out = poisoned(c, outp, p, call)
            if ref is None:
                ref = out
            check_oracle(out, rows, data, (k, what, hex(p)))
            same_bits(ref, out, (k, what, hex(p)))
        same_bits(ref, checked(c, lambda: call(c)), (k, what, "repeat"))


@pytest.mark.parametrize("B", SIZES)
def test_partI_sizes(ctxs, data, outp, B):
    x = data[0][:B]
    run_everywhere(ctxs, outp, lambda c: c.partI_forward(x, want_inv=True, want_inv_np=True, check_range=False), np.arange(B), data, B)


def test_partI_pair(ctxs, data, outp):
    lo = max(SIZES)
    x0, x1 = data[0][lo:lo + PAIR[0]], data[0][lo + PAIR[0]:lo + sum(PAIR)]
    run_everywhere(ctxs, outp, lambda c: c.partI_forward_pair(x0, x1, want_inv=True, want_inv_np=True, check_range=False),
                   np.arange(lo, lo + sum(PAIR)), data, PAIR)


@pytest.mark.parametrize("B", (257, 1500))
def test_ticket_counters_are_zero_again_when_a_launch_ends(ctxs, data, outp, B):
    Xd = data[0]
    x, other = Xd[:B], Xd[NX - B:]
    call = lambda c, v: c.partI_forward(v, want_inv=True, want_inv_np=True, check_range=False)
    ref, ref_other = call(ctxs[1], x), call(ctxs[1], other)
    for R in TILES[1:]:
        c = ctxs[R]
        for p in PATTERNS:
            c.poison_scratch(p)
            outp.pattern = p
            try:
                first = call(c, other)          # queued back to back: no host wait between these two
                second = call(c, x)
                assert c.range_status() == (False, False), (R, hex(p))
                c.poison_scratch(p)
                third = call(c, x)
                assert c.range_status() == (False, False), (R, hex(p))
            finally:
                outp.pattern = None
            same_bits(ref_other, first, (R, hex(p), "first"))
            same_bits(ref, second, (R, hex(p), "second"))
            same_bits(ref, third, (R, hex(p), "third"))
        assert c.range_fallbacks == 0, c.range_report()


def test_two_stream_slots_of_counters(ctxs, outp):
    """depth-first schedule, chunks of 2048 keypoints alternating between two streams (each with its own counters), against breadth-first"""
    x = cu(synth.unit_features(4100, seed=829))
    call = lambda c: c.partI_forward(x, want_inv=True, want_inv_np=True, check_range=False)
    ref = checked(ctxs[1], lambda: call(ctxs[1]))
    assert torch.isfinite(ref["eqv"]).all()
    for R in TILES[1:]:
        c = ctxs[R]
        same_bits(ref, poisoned(c, outp, PATTERNS[0], call), (R, "breadth-first"))
        c.set_partI_schedule(2048, 2)
        try:
            for p in PATTERNS:
                same_bits(ref, poisoned(c, outp, p, call), (R, "2048x2", hex(p)))
        finally:
            c.set_partI_schedule(0, 1)
