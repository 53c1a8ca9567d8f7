"""GPU tests (-m gpu): PartII's 13-element cone layer as the implicit GEMM on K32 stages (cgemmk_kernel) in the DEFAULT mode fp16x2.

Match counts at every edge of the kernel's tiles: the ragged 16-match tile of cone1's planes (1, 15, 16, 17), the ragged 32-match tile of
the inverse transform (31, 32, 33), a 256-match column tile that is not full (255) and a second column tile (256, 257, 300).  For every
count, through the plain and the row-indexed entry:  mode fp16x2 against the oracle at the tolerance test_gpu_kernels.py applies to mode
cgemm;  mode fp16x2 and mode cgemm give equal bits (one kernel);  a repeat gives equal bits;  a second context created with
YOHO_PARTII_CONE=direct (the direct cone kernel) agrees with the oracle inside the same tolerance.  Before every pass the workspace is
filled with hostile bits - the largest finite fp16 (0x7BFF) and fp16 +inf (0x7C00) - so that a stale column of a ragged tile that reached
the range word or the output would raise the flag and be counted as a repeat: no pass may repeat and none may raise the flag.

Where the experiments library is built, the K16 loop (YOHO_FGEMM_DEBUG=k16) and the K32 loop run in one process and must agree to the
accumulation-order difference: 6e-7 of the largest value, the figure measured for the irrep GEMMs (profiles/fgemm_mfma_shape.md)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import yoho_oracle as orc  # noqa: E402
from yoho_amd import synth  # noqa: E402
from test_gpu_kernels import TOL, rel, rel_rows, cu  # noqa: E402  (TOL: what test_partII_cone_gemm_modes applies to mode cgemm)

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 300)
POISON = (0x7BFF7BFF, 0x7C007C00)            # the largest finite fp16 / fp16 +inf in both halves of every word
K16_K32_BOUND = 6e-7                         # of the largest value (profiles/fgemm_mfma_shape.md, 'Correctness of the new loop')


@pytest.fixture(scope="module")
def data(sd2, tables):
    """300 matches (every pass reads a prefix) and the oracle once, over all of them"""
    n = max(SIZES)
    A, B, Cf, D = (synth.unit_features(n, seed=s) for s in (911, 912, 913, 914))
    dr = np.random.RandomState(915).randint(0, 60, size=n).astype(np.int64)
    q = orc.partII_forward(A, B, Cf, D, dr, sd2, tables.N, tables.P)
    # the row-indexed entry reads the same rows through a match list from tensors stored in a shuffled order
    rs = np.random.RandomState(916)
    p0, p1 = rs.permutation(n), rs.permutation(n)
    stored = dict(feat0=cu(B[p0]), feat1=cu(A[p1]), eqv0=cu(D[p0]), eqv1=cu(Cf[p1]))
    match = cu(np.stack([np.argsort(p0), np.argsort(p1)], 1).astype(np.int64))
    return [cu(x) for x in (A, B, Cf, D, dr)], q, stored, match


@pytest.fixture(scope="module")
def ctxs(hip, sd2, data):
    """default (fp16x2), mode cgemm, and fp16x2 with the direct cone kernel (the switch is read once, when the context is created)"""
    def make(mode):
        c = hip.Context()
        c.load_partII(sd2)
        c.set_partII_mode(mode)
        c.partII_forward(*data[0])           # the workspace at its largest: the smaller passes then see stale stage blocks
        return c
    cs = {"fp16x2": make("fp16x2"), "cgemm": make("cgemm")}
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("YOHO_PARTII_CONE", "direct")
        cs["direct"] = make("fp16x2")
    assert cs["fp16x2"].partII_mode == "fp16x2" and cs["direct"].partII_mode == "fp16x2"
    yield cs
    for c in cs.values():
        assert c.range_fallbacks == 0, c.range_report()


def hostile_pass(c, pattern, call, what):
    """call() behind a workspace full of `pattern`: no flag, no repeat in bf16x3"""
    c.poison_scratch(pattern)
    q = call()
    assert c.range_fallbacks == 0 and c.range_repeats["partII"] == 0, (what, hex(pattern), c.range_report())
    assert c.range_status() == (False, False), (what, hex(pattern))
    return q


def check_entry(ctxs, call, qo, what):
    M = len(qo)
    q = hostile_pass(ctxs["fp16x2"], POISON[0], lambda: call(ctxs["fp16x2"]), what)
    qn = q.cpu().numpy()
    assert qn.shape == (M, 4) and np.isfinite(qn).all(), what
    errs = rel(qn, qo), rel_rows(qn, qo)
    print("%s: fp16x2 (cone GEMM) vs oracle %.3g, worst row %.3g" % (what, errs[0], errs[1]))
    assert max(errs) < TOL, (what, errs)
    # a repeat behind the other pattern, and mode cgemm: the same kernel, the same bits
    assert torch.equal(q, hostile_pass(ctxs["fp16x2"], POISON[1], lambda: call(ctxs["fp16x2"]), (what, "repeat"))), (what, "repeat")
    for p in POISON:
        assert torch.equal(q, hostile_pass(ctxs["cgemm"], p, lambda: call(ctxs["cgemm"]), (what, "cgemm"))), (what, "fp16x2 vs cgemm")
    # the direct cone kernel: another order of the sums, the same oracle tolerance
    qd = hostile_pass(ctxs["direct"], POISON[0], lambda: call(ctxs["direct"]), (what, "direct")).cpu().numpy()
    errd = rel(qd, qo), rel_rows(qd, qo), rel(qn, qd)
    print("%s: direct cone kernel vs oracle %.3g, worst row %.3g; vs the cone GEMM %.3g" % ((what,) + errd))
    assert max(errd) < TOL, (what, errd)
    return q


@pytest.mark.parametrize("M", SIZES)
def test_default_mode_runs_the_cone_gemm(ctxs, data, M):
    dev, qo, stored, match = data
    args = [t[:M] for t in dev]
    q = check_entry(ctxs, lambda c: c.partII_forward(*args), qo[:M], ("plain", M))
    m = match[:M].contiguous()
    qi = check_entry(ctxs, lambda c: c.partII_forward_matched(stored["feat0"], stored["feat1"], stored["eqv0"], stored["eqv1"], m, args[4]),
                     qo[:M], ("indexed", M))
    assert torch.equal(q, qi), ("plain vs indexed", M)


K16_K32_SCRIPT = r"""
import os, sys
import numpy as np, torch
from yoho_amd import hip, synth, weights as W
c = hip.Context(); c.load_partII(W.synth_state_dict(W.PARTII_SPEC, 8)); c.set_partII_mode("fp16x2")
cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
worst = 0.0
for M in (1, 33, 257, 300):
    args = [cu(synth.unit_features(M, seed=s)) for s in (911, 912, 913, 914)] + [cu(np.random.RandomState(915).randint(0, 60, size=M).astype(np.int64))]
    os.environ.pop("YOHO_FGEMM_DEBUG", None)
    q32 = c.partII_forward(*args); q32b = c.partII_forward(*args)
    os.environ["YOHO_FGEMM_DEBUG"] = "k16"
    q16 = c.partII_forward(*args)
    assert torch.equal(q32, q32b), M
    worst = max(worst, float((q32 - q16).abs().max() / q16.abs().max()))
assert c.range_fallbacks == 0
print("K16 vs K32 worst %.3g" % worst)
"""


def test_k16_and_k32_loops_agree_in_the_experiments_build():
    """The bound is the figure measured for the irrep GEMMs' two loops at PartI's outputs (6e-7 of the largest value).  MEASURED here, at
    PartII's quaternions (M = 1, 33, 257, 300): 1.43e-6 of the largest value - this test FAILS where the experiments library is built
    (profiles/cone_gemm_k32.md, section 4).  Both loops meet the oracle alike (2.2e-6; the direct cone kernel 2.1e-6, and it differs from
    the GEMM by 1.5e-6: another order of the same sums), the difference passes through two more layers and the normalisation before it
    is measured, and neither order is the more exact one; the bound is left where it was set."""
    lib = os.path.join(REPO, "yoho_amd", "lib", "libyoho_hip_exp.so")
    if not os.path.exists(lib):
        pytest.skip("no experiments library here (YOHO_EXPERIMENTS=1 python -m yoho_amd.build): the shipped one has no switch to the K16 loop")
    env = dict(os.environ, YOHO_LIB="exp", PYTHONPATH=REPO)
    env.pop("YOHO_FGEMM_DEBUG", None)
    r = subprocess.run([sys.executable, "-c", K16_K32_SCRIPT], env=env, cwd=REPO, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr[-2000:]
    worst = float(r.stdout.strip().split()[-1])
    assert worst <= K16_K32_BOUND, worst
