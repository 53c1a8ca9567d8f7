"""The fp16x2 contract of the FCGF backbone across activation scales, against a float64 reference (-m gpu).

tests/test_gpu_fcgf.py compares the backbone with the fp32 oracle at 1e-5, with one kind of weights: the largest input of any convolution
is 10, three orders of magnitude below the fp16 planes' limit, and a lo plane flushed to zero where subnormal sits exactly at that
tolerance.  Here the same network runs with every activation scaled by lam (fcgf_ref64.scale_activations: the unit-row output does not
change, one float64 reference serves the sweep) and must stay within

    emu(lam) + C_BUDGET * e_ref        in rel and in rel_rows

of float64, where emu(lam) is the error of the float64 emulation of the documented plane arithmetic (fcgf_ref64.emulate_fp16x2) and
e_ref the fp32 oracle's own distance from float64.  Below lam = 2^-4, where the plane rounding dominates, also within twice emu(lam) (a
denormal flush is twenty times that).  Past the upper limit a row either is non-finite or is right.  tests/test_fcgf_precision_cpu.py
proves on the CPU that this comparison rejects the defects it is there for; profiles/precision.md keeps one run of the printed figures."""
import hashlib
import os
import re

import numpy as np
import pytest
import torch

import fcgf_ref64 as F
from fcgf_ref64 import fo
from yoho_amd import synth

pytestmark = pytest.mark.gpu

CONTROL_LAMBDAS = (2.0 ** -16,) + F.LAMBDAS_IN_RANGE + F.LAMBDAS_OVER
lam_id = lambda lam: "2^%d" % int(np.log2(lam))


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def small():
    coords = F.small_cloud()
    ref, eref = F.case(coords, F.state_dict())
    return coords, cu(coords), ref, eref


_EMU = {}


def emu(coords, lam):
    """(finite-row mask, (rel, rel_rows) over the finite rows) of the faithful emulation on the small cloud at scale lam"""
    if lam not in _EMU:
        out = F.emulated(coords, F.state_dict(lam))
        fin = np.isfinite(out).all(axis=1)
        _EMU[lam] = (fin, F.errors(out[fin], F.resunet_forward64(coords, F.state_dict())[fin]) if fin.any() else None)
    return _EMU[lam]


@pytest.fixture(scope="module")
def ctx_for(hip):
    """default contexts by scale, one per state dict, made on first use"""
    made = {}

    def get(lam):
        if lam not in made:
            made[lam] = hip.Context()
            made[lam].load_fcgf(F.state_dict(lam))
        return made[lam]
    return get


def _report(what, got, ref, emu_errs, eref, rows=None):
    ok, worst = F.in_budget(got, ref, emu_errs, eref, rows=rows)
    g, r = (got, ref) if rows is None else (got[rows], ref[rows])
    errs = F.errors(g, r) if np.isfinite(g).all() else [float("nan")] * 2
    print("%s: e_ref %.3g; rel %.3g rel_rows %.3g = %.2f / %.2f e_ref; emulation %.3g %.3g; (error - emu) / e_ref %.2f of %g" % (
        what, eref, errs[0], errs[1], errs[0] / eref, errs[1] / eref, emu_errs[0], emu_errs[1], worst, F.C_BUDGET))
    return ok, errs


# ---- a. the small cloud: every level on the coarse split kernels ---------------------------------------------------------------------
@pytest.mark.parametrize("lam", F.LAMBDAS_IN_RANGE, ids=lam_id)
def test_small_cloud_error_budget(ctx_for, small, lam):
    coords, coords_d, ref, eref = small
    fin, emu_errs = emu(coords, lam)
    assert fin.all()
    got = ctx_for(lam).fcgf_forward(coords_d).cpu().numpy()
    assert np.isfinite(got).all()                                       # 2^8 included: inside the limit
    ok, errs = _report("backbone, 4770 voxels, lam %s" % lam_id(lam), got, ref, emu_errs, eref)
    assert ok
    if lam < 2.0 ** -4:
        print("    error / emulated: %.2f %.2f (must stay below 2; lo planes flushed where subnormal: > 20)" % (errs[0] / emu_errs[0], errs[1] / emu_errs[1]))
        assert errs[0] < 2 * emu_errs[0] and errs[1] < 2 * emu_errs[1]


# ---- b. the fine cloud: spconv16w_kernel<1|2>, the fused heads, conv1_mfma_kernel ------------------------------------------------------
# Its float64 pass and emulations take minutes: tests/golden/fcgf_fine64.npz (oracle/gen_golden_fcgf_precision.py) keeps 1024 rows of the
# reference, e_ref, the emulation's error at every scale that is in range for THIS cloud (its largest convolution input is not the small
# cloud's) and the overflow masks at the first scale that is not.
GFINE = np.load(os.path.join(F.R.REPO, "tests", "golden", "fcgf_fine64.npz"), allow_pickle=False)
FINE_LAMBDAS = tuple(float(v) for v in GFINE["lambdas"])
FINE_EMU = {lam: [float(e) for e in errs] for lam, errs in zip(FINE_LAMBDAS, GFINE["emu"])}


class Fine:
    pass


@pytest.fixture(scope="module")
def fine(hip):
    """one context for every scale; its outputs at lam = 1 (alone, and in a batch with the 37-point cloud) are the comparison target of
    the rows the fixture has no reference for: out(lam) and out(1) are each within their budget of the same float64 rows"""
    f = Fine()
    coords = fo.voxelize(synth.surface_cloud(60000, seed=31, extent=3.0), 0.025)[1]
    assert len(coords) >= 32768 and len(coords) == int(GFINE["n"])
    assert hashlib.sha256(np.ascontiguousarray(coords, np.int32).tobytes()).hexdigest() == str(GFINE["coords_sha"])
    assert float(GFINE["top"]) * max(FINE_LAMBDAS) < F.ACT_LIMIT < float(GFINE["top"]) * float(GFINE["lam_over"])
    f.tiny = fo.voxelize(synth.surface_cloud(37, seed=6), 0.025)[1]
    f.tiny_ref, f.tiny_eref = F.case(f.tiny, F.state_dict())
    fc, tc = cu(coords), cu(f.tiny)
    f.ctx = hip.Context()
    f.ctx.load_fcgf(F.state_dict())
    f.run = lambda: [f.ctx.fcgf_forward(fc).cpu().numpy()] + [o.cpu().numpy() for o in f.ctx.fcgf_forward_batch([fc, tc])]
    f.base = f.run()
    f.rows, f.ref_rows, f.eref = GFINE["rows"], GFINE["ref_rows"], float(GFINE["e_ref"])
    return f


def _fine_checks(f, lam, outs, emu_l, what, only=None):
    """outs = [the fine cloud alone, in a batch] at scale lam.  The sampled rows against float64 under the budget; every row against the
    same context's lam = 1 output, each of the two being within its own budget of the truth; rows outside `only` (a mask) are left out.
    -> the worst multiple of e_ref"""
    e1 = FINE_EMU[1.0]
    worst = 0.0
    for name, a, b in zip(("alone", "in a batch"), outs[:2], f.base[:2]):
        keep = np.ones(len(a), bool) if only is None else only
        sub = f.rows[keep[f.rows]]
        sel = np.isin(f.rows, sub)
        assert len(sub) and keep.any()
        ok, errs = _report("%s, lam %s, %s, %d sampled rows" % (what, lam_id(lam), name, len(sub)), a[sub], f.ref_rows[sel], emu_l, f.eref)
        assert ok
        worst = max(worst, *F.budget_multiples(a[sub], f.ref_rows[sel], emu_l, f.eref))
        d = F.errors(a[keep], b[keep].astype(np.float64))
        mult = [(e - x - y) / (2 * f.eref) for e, x, y in zip(d, emu_l, e1)]
        print("    all %d rows against lam = 1: rel %.3g rel_rows %.3g; (difference - emu(lam) - emu(1)) / 2 e_ref %.2f %.2f of %g" % (keep.sum(), d[0], d[1], mult[0], mult[1], F.C_BUDGET))
        if lam != 1.0:
            assert max(mult) < F.C_BUDGET
            worst = max(worst, *mult)
        if lam < 2.0 ** -4:                                              # the lo planes are subnormal: within twice the emulated error
            print("    error / emulated on the sampled rows: %.2f %.2f" % (errs[0] / emu_l[0], errs[1] / emu_l[1]))
            assert errs[0] < 2 * emu_l[0] and errs[1] < 2 * emu_l[1]
            assert all(e < 2 * x + y + F.C_BUDGET * f.eref for e, x, y in zip(d, emu_l, e1))
    return worst


@pytest.mark.parametrize("lam", FINE_LAMBDAS, ids=lam_id)
def test_fine_cloud_error_budget(fine, lam):
    f = fine
    try:
        f.ctx.load_fcgf(F.state_dict(lam))
        outs = f.run()
    finally:
        f.ctx.load_fcgf(F.state_dict())
    assert all(np.isfinite(o).all() for o in outs)
    _fine_checks(f, lam, outs, FINE_EMU[lam], "backbone, %d voxels" % len(outs[0]))
    # the 37-point cloud that shared the pass, against its own reference and emulation
    emu_t = F.errors(F.emulated(f.tiny, F.state_dict(lam)), f.tiny_ref)
    ok, errs = _report("    the 37-point cloud of the batch", outs[2], f.tiny_ref, emu_t, f.tiny_eref)
    assert ok
    if lam < 2.0 ** -4:
        assert errs[0] < 2 * emu_t[0] and errs[1] < 2 * emu_t[1]


# ---- c. control: the fp32 MFMA kernels a caller falls back to -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx32(hip):
    def get(sd):
        old = os.environ.get("YOHO_FCGF")
        os.environ["YOHO_FCGF"] = "f32"
        try:
            c = hip.Context()
            c.load_fcgf(sd)
        finally:
            if old is None:
                del os.environ["YOHO_FCGF"]
            else:
                os.environ["YOHO_FCGF"] = old
        return c
    return get


@pytest.mark.parametrize("lam", CONTROL_LAMBDAS, ids=lam_id)
def test_f32_kernels_are_fp32_accurate_at_every_scale(ctx32, small, lam):
    coords, coords_d, ref, eref = small
    got = ctx32(F.state_dict(lam)).fcgf_forward(coords_d).cpu().numpy()
    ok, _ = _report("YOHO_FCGF=f32, 4770 voxels, lam %s" % lam_id(lam), got, ref, [0.0, 0.0], eref)
    assert ok


# ---- d. ResUNetBN2B channels, first kernel 5 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", (2.0 ** -4, 2.0 ** 8), ids=lam_id)
def test_second_configuration(hip, lam):
    coords = F.cloud_2b()
    ref, eref = F.case(coords, F.state_dict_2b(), 5)
    top = max(float(np.abs(x).max()) for k, x in F.conv_inputs(coords, F.state_dict_2b(), 5).items() if k != "conv1")
    assert top * 2.0 ** 8 < F.ACT_LIMIT, top
    sd = F.state_dict_2b(lam)
    out = F.emulated(coords, sd, 5)
    assert np.isfinite(out).all()
    c = hip.Context()
    c.load_fcgf(sd, normalize_feature=False, **F.SPEC_2B)
    got = c.fcgf_forward(cu(coords)).cpu().numpy()
    ok, _ = _report("ResUNetBN2B / kernel 5, %d voxels, lam %s" % (len(coords), lam_id(lam)), got, ref, F.errors(out, ref), eref)
    assert ok


# ---- e. the weight side: one large entry pushes a layer's other lo planes toward the subnormals ----------------------------------------
def test_one_large_weight(hip, small):
    coords, coords_d, _, _ = small
    sd = F.state_dict_big_weight()
    ref, eref = F.case(coords, sd)
    out = F.emulated(coords, sd)
    assert np.isfinite(out).all()
    c = hip.Context()
    c.load_fcgf(sd)
    got = c.fcgf_forward(coords_d).cpu().numpy()
    ok, _ = _report("one entry of block2.conv1.kernel x 2^12", got, ref, F.errors(out, ref), eref)
    assert ok


# ---- f. past the upper limit ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", F.LAMBDAS_OVER, ids=lam_id)
def test_out_of_range_rows_are_non_finite_or_right(hip, ctx_for, small, lam):
    """include/yoho_hip.h: an activation of 4095 or more in front of a split convolution makes every output row it reaches non-finite.
    Either the call fails with an error that names the range, or every row the emulation marks as reached for certain (threshold moved
    up by 1e-3: at 2^10 a few inputs lie that close to it) is non-finite and every finite row is within the budget.  NaN arithmetic
    is ordinary arithmetic: nothing faults."""
    coords, coords_d, ref, eref = small
    fin_emu, emu_errs = emu(coords, lam)
    if emu_errs is None:
        emu_errs = emu(coords, 2.0 ** 8)[1]          # no row left to measure: the relative plane rounding is the same above 2^-4
    sure = ~np.isfinite(F.emulated(coords, F.state_dict(lam), over_margin=1e-3)).all(axis=1)
    assert sure.any() and not (sure & fin_emu).any()
    c = hip.Context()
    c.load_fcgf(F.state_dict(lam))
    lib = hip.load_library()
    try:
        got = c.fcgf_forward(coords_d).cpu().numpy()
    except hip.YohoError as e:
        print("lam %s: refused: %s" % (lam_id(lam), e))
        assert re.search(r"range|4094", str(e))
        got = None
    if got is not None:
        fin = np.isfinite(got).all(axis=1)
        print("lam %s: %d of %d rows finite on the device (emulation %d; overflowed for certain %d)" % (lam_id(lam), fin.sum(), len(fin), fin_emu.sum(), sure.sum()))
        hidden = int((fin & sure).sum())
        if fin.any():
            ok, errs = _report("    the finite rows", got, ref, emu_errs, eref, rows=fin)
        assert hidden == 0, "%d rows reached by an overflowed value came back finite" % hidden
        assert not fin.any() or ok
        assert lib.yoho_last_error() == b"", lib.yoho_last_error()
    # afterwards the context is as good as new
    c.load_fcgf(F.state_dict())
    assert torch.equal(c.fcgf_forward(coords_d), ctx_for(1.0).fcgf_forward(coords_d))
    assert lib.yoho_last_error() == b"", lib.yoho_last_error()


def test_out_of_range_on_the_fine_kernels(fine):
    """the same through spconv16w_kernel and the fused heads (whose ReLU sits between two MFMA products), at the first power of two that
    takes THIS cloud past the limit: the rows the fixture's emulation marks as overflowed for certain are non-finite, a finite row is a
    right row, and the 37-point cloud in the same batch - in range at that scale, or not - follows its own emulation"""
    f = fine
    lam = float(GFINE["lam_over"])
    n = int(GFINE["n"])
    sure = np.unpackbits(GFINE["sure_over"])[:n].astype(bool)
    fin_emu = np.unpackbits(GFINE["fin_over"])[:n].astype(bool)
    try:
        f.ctx.load_fcgf(F.state_dict(lam))
        outs = f.run()
    finally:
        f.ctx.load_fcgf(F.state_dict())
    for name, a in zip(("alone", "in a batch"), outs[:2]):
        fin = np.isfinite(a).all(axis=1)
        print("lam %s, %d voxels, %s: %d rows finite on the device (emulation %d; overflowed for certain %d)" % (lam_id(lam), n, name, fin.sum(), fin_emu.sum(), sure.sum()))
        assert not (fin & sure).any(), "%d rows reached by an overflowed value came back finite" % (fin & sure).sum()
        assert fin.any()
    fin = np.isfinite(outs[0]).all(axis=1) & np.isfinite(outs[1]).all(axis=1)
    _fine_checks(f, lam, outs, [float(e) for e in GFINE["emu_over"]], "out of range, %d voxels" % n, only=fin)
    t_emu = F.emulated(f.tiny, F.state_dict(lam))
    t_fin = np.isfinite(t_emu).all(axis=1)
    t_sure = ~np.isfinite(F.emulated(f.tiny, F.state_dict(lam), over_margin=1e-3)).all(axis=1)
    g_fin = np.isfinite(outs[2]).all(axis=1)
    print("    the 37-point cloud: %d rows finite on the device (emulation %d)" % (g_fin.sum(), t_fin.sum()))
    assert not (g_fin & t_sure).any()
    if g_fin.any():
        emu_t = F.errors(t_emu[t_fin], f.tiny_ref[t_fin]) if t_fin.any() else FINE_EMU[max(FINE_LAMBDAS)]
        assert _report("    its finite rows", outs[2], f.tiny_ref, emu_t, f.tiny_eref, rows=g_fin)[0]
    again = f.run()
    assert all(np.array_equal(a, b) for a, b in zip(again, f.base))
