"""The float64 reference of the FCGF backbone (tests/fcgf_ref64.py), the emulation of its fp16x2 arithmetic and the budget built on them,
checked on the CPU: the reference does not depend on the activation scale, the fp32 oracle's distance from it (e_ref) does not either,
and the comparison the GPU tests use (fcgf_ref64.in_budget: emu(lam) + C_BUDGET * e_ref in rel and rel_rows) REJECTS results that carry
the defects a change to the split kernels can produce - subnormal lo planes flushed, one layer's lo plane or cross term gone, a descale
off by two, a ReLU that turns the NaN of an overflowed plane into 0 - while the parity tests of tests/test_gpu_fcgf.py (1e-5 against the
fp32 oracle at one activation scale) let most of them through.  Figures in profiles/precision.md, backbone section."""
import numpy as np
import pytest

import fcgf_ref64 as F

SWEEP = F.LAMBDAS_IN_RANGE + F.LAMBDAS_OVER[:1]      # 2^-12 .. 2^9


@pytest.fixture(scope="module")
def small():
    coords, sd = F.small_cloud(), F.state_dict()
    ref, eref = F.case(coords, sd)
    return coords, sd, ref, eref


_EMU = {}


def emu(coords, lam):
    """the faithful emulation at scale lam and its (rel, rel_rows) against float64, over its finite rows"""
    if lam not in _EMU:
        out = F.emulated(coords, F.state_dict(lam))
        fin = np.isfinite(out).all(axis=1)
        _EMU[lam] = (out, fin, F.errors(out[fin], F.resunet_forward64(coords, F.state_dict())[fin]))
    return _EMU[lam]


def test_reference_and_oracle_do_not_depend_on_the_activation_scale(small):
    coords, sd, ref, eref = small
    assert len(coords) == 4770 and ref.dtype == np.float64 and ref.shape == (4770, 32)
    assert np.allclose(np.sum(ref * ref, axis=1), 1.0, rtol=0, atol=1e-14)
    assert 1e-7 < eref < 1e-5                       # fp32 rounding through 21 convolutions: not more and not nothing
    o1 = F.oracle32(coords, sd)
    for lam in SWEEP:
        sdl = F.state_dict(lam)
        d = F.rel_rows(F.resunet_forward64(coords, sdl), ref)
        o = F.oracle32(coords, sdl)
        e = F.e_ref(o, ref)
        print("lam 2^%+d: float64 pass vs lam = 1 %.3g; e_ref %.4g, the oracle's bits %s" % (np.log2(lam), d, e, "equal" if np.array_equal(o, o1) else "DIFFER"))
        assert d < 1e-12
        assert np.array_equal(o, o1) and e == eref      # powers of two: every fp32 rounding of the oracle scales with the value


def test_activation_range_of_the_sweep(small):
    """where the sweep leaves the fp16 planes: inside at 2^8, and at 2^9 no convolution input near enough to the limit for the set of
    overflowing values to depend on the last bits of an fp32 sum"""
    coords, sd, _, _ = small
    ins = F.conv_inputs(coords, sd)
    assert set(ins) >= {"conv1", "block1.conv1", "block4.conv2", "conv4_tr", "block2_tr.conv2", "conv1_tr", "final"} and len(ins) == 23
    v = np.concatenate([np.abs(x).ravel() for k, x in ins.items() if k != "conv1"])
    print("largest convolution input at lam = 1: %.4g; above %g at 2^9: %d values, at 2^10: %d" % (
        v.max(), F.ACT_LIMIT, int((v * 512 >= F.ACT_LIMIT).sum()), int((v * 1024 >= F.ACT_LIMIT).sum())))
    assert v.max() * 2.0 ** 8 < F.ACT_LIMIT                              # 2.55e3
    assert v.max() * 2.0 ** 9 > F.ACT_LIMIT
    for lim in (F.ACT_LIMIT, F.F16_OVER / 16.0):                         # the documented limit and the exact one (4095)
        assert not (np.abs(v * 2.0 ** 9 / lim - 1.0) < 1e-3).any()


def test_faithful_emulation_follows_the_documented_limits(small):
    """between the limits the split arithmetic is fp32-accurate (ref64.FACTOR x e_ref, the bound of the PartI / PartII suite); below
    2^-7 per activation the lo plane is subnormal, its error absolute, and the row error grows like 1 / lam"""
    coords, sd, ref, eref = small
    worst = {}
    for lam in F.LAMBDAS_IN_RANGE:
        out, fin, errs = emu(coords, lam)
        worst[lam] = max(errs)
        print("lam 2^%+d: emulated rel %.3g rel_rows %.3g (%.2f e_ref)" % (np.log2(lam), errs[0], errs[1], max(errs) / eref))
        assert fin.all()
        assert F.in_budget(out, ref, errs, eref)[0]
    assert all(worst[lam] < F.R.FACTOR * eref for lam in F.LAMBDAS_IN_RANGE if lam >= 2.0 ** -4)
    assert worst[2.0 ** -8] > 4 * worst[1.0] and worst[2.0 ** -12] > 8 * worst[2.0 ** -8]
    assert worst[2.0 ** -12] < 1e-3                 # still a usable descriptor; the header states the decay


DEFECTS = [("flush_lo", None, 2.0 ** -4)] + [("drop_lo", layer, 1.0) for layer in ("conv2", "block3.conv2", "conv3_tr", "final")] + \
          [("drop_cross", "block2.conv1", 1.0), ("descale2", "block4_tr.conv2", 1.0), ("descale2", "conv1_tr", 1.0)]


@pytest.mark.parametrize("mode,layer,lam", DEFECTS, ids=["%s-%s-2^%d" % (m, l, np.log2(s)) for m, l, s in DEFECTS])
def test_budget_rejects_emulated_defect(small, mode, layer, lam):
    coords, sd, ref, eref = small
    _, _, errs = emu(coords, lam)
    bad = F.emulated(coords, F.state_dict(lam), mode=mode, layer=layer)
    ok, worst = F.in_budget(bad, ref, errs, eref)
    print("%s %s at 2^%+d: rel %.3g rel_rows %.3g; (error - emu) / e_ref %.1f against C_BUDGET %g; old check (rel against the fp32 oracle) %.3g" % (
        mode, layer or "everywhere", np.log2(lam), *F.errors(bad, ref), worst, F.C_BUDGET, F.rel(bad, F.oracle32(coords, sd).astype(np.float64))))
    assert np.isfinite(bad).all() and not ok
    assert worst > 2 * F.C_BUDGET                   # rejected with room, not by a hair


def test_flush_everywhere_at_scale_one_passes_the_old_tolerance(small):
    """why the sweep is needed: the flush is at the parity tests' TOL at the only scale they run, and 40 x further out at 2^-4"""
    coords, sd, ref, eref = small
    bad = F.emulated(coords, sd, mode="flush_lo")
    old = F.rel(bad, F.oracle32(coords, sd).astype(np.float64))
    print("lo planes flushed, lam = 1: %.3g against the fp32 oracle (TOL 1e-5)" % old)
    assert old < 2e-5
    assert not F.in_budget(bad, ref, emu(coords, 1.0)[2], eref)[0]


def test_overflow_marks_rows_and_a_swallowing_relu_hides_them(small):
    coords, sd, ref, eref = small
    lam = 2.0 ** 9
    out, fin, errs = emu(coords, lam)
    print("lam 2^9, NaN-propagating ReLU: %d of %d rows finite, their rel %.3g rel_rows %.3g" % (fin.sum(), len(fin), *errs))
    assert 0 < fin.sum() < len(fin)
    assert max(errs) < F.R.FACTOR * eref            # every finite row is a correct row
    for margin in (1e-3, -1e-3):                    # the set of overflowed rows does not hang on values near the limit
        assert np.array_equal(np.isfinite(F.emulated(coords, F.state_dict(lam), over_margin=margin)).all(axis=1), fin)
    bad = F.emulated(coords, F.state_dict(lam), relu=F.swallowing_relu)
    nfin = int(np.isfinite(bad).all(axis=1).sum())
    ok, worst = F.in_budget(bad, ref, errs, eref)
    print("lam 2^9, fmaxf ReLU: %d rows finite, rel_rows %.3g, (error - emu) / e_ref %.3g" % (nfin, F.rel_rows(bad, ref), worst))
    assert nfin == len(fin) and not ok and F.rel_rows(bad, ref) > 0.1        # finite, and wrong


def test_hooked_passes_are_not_cached_and_inputs_are_left_alone(small):
    coords, sd, ref, _ = small
    keep = {k: np.array(v, copy=True) for k, v in sd.items()}
    a = F.resunet_forward64(coords, sd, hook=lambda name, x, W: (x, W))
    assert a is not ref and np.array_equal(a, ref) and F.resunet_forward64(coords, sd) is ref and not ref.flags.writeable
    sdl = F.scale_activations(sd, 4.0)
    assert all(np.array_equal(sd[k], keep[k]) for k in sd)
    changed = {k for k in sd if not np.array_equal(sd[k], sdl[k])}
    assert "norm1.bn.weight" in changed and "norm1.bn.running_mean" not in changed and "block1.norm1.bn.weight" not in changed
    assert "block1.norm1.bn.running_mean" in changed and "final.bias" in changed and not any(k.endswith(".kernel") for k in changed)
