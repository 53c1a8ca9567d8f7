"""PartI, PartII and the FCGF backbone on weights with the statistics of a trained network, against float64 (-m gpu).

Every other network test draws its weights from yoho_amd.weights.synth_state_dict: one scale per layer, gammas in [0.5, 1.5], running
variances in [0.5, 1.5].  tests/trained_like.py builds what a checkpoint brings instead - negative, zero and tiny gammas (the folded
scale s = gamma / sqrt(var + eps) changes sign or vanishes in every fused relu(s*x + t)), variances over nine decades, below eps and
exactly zero, heavy-tailed conv weights whose rows spread over 2^8 (cal8) or 2^14 (cal14) under the ONE power of two a weight pack
applies per layer, all-zero rows and columns - calibrated in float64 so that every stage stays far inside the fp16 planes
(tests/test_trained_like_cpu.py asserts a factor 2 for every case here: hence zero range repeats).

No tolerance is new.  PartI / PartII: ref64.within_budget, 12 x e_ref in rel and rel_rows (the header's per-product bound of the split
over fp32's roundoff), for every mode documented as fp32-accurate.  Backbone: fcgf_ref64.in_budget, the faithful float64 emulation of
the plane arithmetic plus C_BUDGET = 4.3 x e_ref.  e_ref is the fp32 oracle's own distance from float64 on the same weights and input.
Every test prints its figures as multiples of e_ref (profiles/precision.md, "trained-like weights", keeps one run)."""
import os
import warnings

import numpy as np
import pytest
import torch

import fcgf_ref64 as F
import ref64 as R
import trained_like as T
from test_gpu_kernels import TOL

pytestmark = pytest.mark.gpu


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_id5 = lambda cases: ["%s-%d-%s" % (T.case_id(fam, seed), n, mode) for fam, _, seed, n, mode in cases]


@pytest.fixture(scope="module")
def ctx_for(hip):
    """contexts by (network, family, seed, mode), made on first use and kept for the module; mode None: the library's default"""
    made = {}

    def get(net, lo, seed, mode):
        key = (net, lo, seed, mode)
        if key not in made:
            c = hip.Context()
            if net == "partI":
                c.load_partI(T.state_dict(net, seed, lo))
                if mode is not None:
                    c.set_gconv_mode(mode)
            else:
                c.load_partII(T.state_dict(net, seed, lo))
                c.set_partII_mode(mode)
            c.range_sticky_after = 0            # a flagged pass would be repeated every time: no test changes another's arithmetic
            made[key] = c
        return made[key]
    return get


def _report(what, got, ref, eref):
    ok, worst = R.within_budget(got, ref, eref)
    print("%s: e_ref %.3g, errors / e_ref %s, worst %.2f of %g" % (what, eref, " ".join("%.2f" % (e / eref) for e in R.errors(got, ref)), worst, R.FACTOR))
    return ok


def _no_repeat(c):
    assert c.range_status() == (False, False) and c.range_fallbacks == 0, c.range_report()


def _check_partI(c, out, ref, eref, what):
    eqv, inv, inv_np = (out[k].cpu().numpy() for k in ("eqv", "inv", "inv_np"))
    assert np.isfinite(eqv).all() and np.isfinite(inv).all() and np.isfinite(inv_np).all(), what
    assert _report(what, (eqv, inv), ref, eref), what
    e_np = R.rel_rows(inv_np, np.mean(ref[0], axis=-1))
    print("    inv_np against the group mean of the float64 eqv: rel_rows %.3g (TOL %g)" % (e_np, TOL))
    assert e_np < TOL, what
    _no_repeat(c)


# ---- PartI -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,lo,seed,B,mode", T.partI_cases(), ids=_id5(T.partI_cases()))
def test_partI_trained_like(ctx_for, tables, fam, lo, seed, B, mode):
    sd = T.state_dict("partI", seed, lo)
    x = R.partI_input(B)
    ref, eref, _ = R.partI_case(x, sd, tables.N)
    c = ctx_for("partI", lo, seed, mode)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = c.partI_forward(cu(x), want_inv=True, want_inv_np=True)
    _check_partI(c, out, ref, eref, "PartI %s seed %d %s B=%d" % (fam, seed, mode, B))


@pytest.mark.parametrize("fam,lo,seed", T.pair_cases(), ids=[T.case_id(f, s) for f, _, s in T.pair_cases()])
def test_partI_pair_trained_like(ctx_for, tables, fam, lo, seed):
    """both fragments in one pass, the fragment boundary (33 + 31) inside a column tile, in the library's default mode"""
    sd = T.state_dict("partI", seed, lo)
    x0, x1 = T.pair_input()
    ref, eref, _ = R.partI_case(np.concatenate([x0, x1]), sd, tables.N)
    c = ctx_for("partI", lo, seed, None)
    assert c.supports_pair(len(x0) + len(x1))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = c.partI_forward_pair(cu(x0), cu(x1), want_inv=True, want_inv_np=True)
    _check_partI(c, out, ref, eref, "PartI %s seed %d pair %d + %d (mode %s)" % (fam, seed, len(x0), len(x1), c.gconv_mode))


# ---- PartII ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,lo,seed,M,mode", T.partII_cases(), ids=_id5(T.partII_cases()))
def test_partII_trained_like(ctx_for, tables, fam, lo, seed, M, mode):
    sd = T.state_dict("partII", seed, lo)
    feats, pre = R.partII_input(M)
    q64, eref, _ = R.partII_case(*feats, pre, sd, tables.N, tables.P)
    c = ctx_for("partII", lo, seed, mode)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        q = c.partII_forward(*[cu(f) for f in feats], cu(pre)).cpu().numpy()
    what = "PartII %s seed %d %s M=%d" % (fam, seed, mode, M)
    assert q.shape == (M, 4) and np.isfinite(q).all(), what
    assert _report(what, q, q64, eref), what
    _no_repeat(c)


# ---- the backbone ----------------------------------------------------------------------------------------------------------------------
def _fcgf_context(hip, sd, kw, f32):
    old = os.environ.get("YOHO_FCGF")
    if f32:
        os.environ["YOHO_FCGF"] = "f32"
    else:
        os.environ.pop("YOHO_FCGF", None)
    try:
        c = hip.Context()
        c.load_fcgf(sd, **kw)
    finally:
        if old is None:
            os.environ.pop("YOHO_FCGF", None)
        else:
            os.environ["YOHO_FCGF"] = old
    return c


_REFS = {}


def _fcgf_ref(net, seed, lo, coords, k):
    """(float64 rows, e_ref, the faithful emulation's (rel, rel_rows)) of one cloud under one state dict, once per module"""
    key = (net, seed, lo, len(coords))
    if key not in _REFS:
        sd = T.state_dict(net, seed, lo)
        ref, eref = F.case(coords, sd, k)
        out = F.emulated(coords, sd, k)
        assert np.isfinite(out).all()
        _REFS[key] = (ref, eref, F.errors(out, ref))
    return _REFS[key]


def _check_fcgf(what, got, ref, emu_errs, eref):
    assert np.isfinite(got).all(), what
    n2 = np.sum(got.astype(np.float64) ** 2, axis=1)
    assert np.abs(n2 - 1.0).max() < 1e-5, (what, float(np.abs(n2 - 1.0).max()))
    ok, worst = F.in_budget(got, ref, emu_errs, eref)
    errs = F.errors(got, ref)
    print("%s: e_ref %.3g; rel %.3g rel_rows %.3g = %.2f / %.2f e_ref; emulation %.3g %.3g; (error - emu) / e_ref %.2f of %g" % (
        what, eref, errs[0], errs[1], errs[0] / eref, errs[1] / eref, emu_errs[0], emu_errs[1], worst, F.C_BUDGET))
    assert ok, what


_fcgf_ids = ["%s-%s" % (n, T.case_id(f, s)) for n, f, _, s in T.fcgf_cases()]


@pytest.mark.parametrize("f32", (False, True), ids=("default", "f32"))
@pytest.mark.parametrize("net,fam,lo,seed", T.fcgf_cases(), ids=_fcgf_ids)
def test_backbone_trained_like(hip, net, fam, lo, seed, f32):
    """every level on the coarse split kernels (default) and on the fp32 MFMA kernels (a context made under YOHO_FCGF=f32, whose budget
    has no emulated term); for the default configuration also both clouds in one batch"""
    cloud, k, kw = T.FCGF_NETS[net]
    coords = cloud()
    c = _fcgf_context(hip, T.state_dict(net, seed, lo), kw, f32)
    name = "%s %s seed %d, %s" % (net, fam, seed, "YOHO_FCGF=f32" if f32 else "default")
    ref, eref, emu = _fcgf_ref(net, seed, lo, coords, k)
    emu = [0.0, 0.0] if f32 else emu
    _check_fcgf("%s, %d voxels" % (name, len(coords)), c.fcgf_forward(cu(coords)).cpu().numpy(), ref, emu, eref)
    if net == "fcgf":
        other = F.cloud_2b()
        ref2, eref2, emu2 = _fcgf_ref(net, seed, lo, other, k)
        outs = c.fcgf_forward_batch([cu(coords), cu(other)])
        _check_fcgf("    in a batch, %d voxels" % len(coords), outs[0].cpu().numpy(), ref, emu, eref)
        _check_fcgf("    in a batch, %d voxels" % len(other), outs[1].cpu().numpy(), ref2, [0.0, 0.0] if f32 else emu2, eref2)
