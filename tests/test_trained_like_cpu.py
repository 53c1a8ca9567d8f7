"""The trained-like weight families of tests/trained_like.py, checked on the CPU: every generated state dict HAS the statistics it is there
for (negative, zero and tiny gammas, running variances over many decades and exactly zero, a dead row and a dead column per layer, row
scales spread under one plane scale); every case tests/test_gpu_trained_like.py runs stays a factor 2 inside the fp16 planes in
float64, which is the condition under which that file may demand zero range repeats; float64 emulations of the documented plane
arithmetic (per-layer power-of-two weight scale, two fp16 planes per operand, three products) stay inside the budgets the GPU file
uses; and the same emulations with a planted defect - |gamma| in the BatchNorm fold, eps left out of it, the weights' lo plane flushed
where it is subnormal - land at ten times the budget or more on at least one case each, so the cases have teeth.

Budgets: ref64.within_budget (FACTOR = 12 x e_ref) for PartI / PartII, fcgf_ref64.in_budget (emulation + C_BUDGET = 4.3 x e_ref) for
the backbone.  Neither is new here.  Figures in profiles/precision.md, "trained-like weights"."""
import numpy as np
import pytest

import fcgf_ref64 as F
import ref64 as R
import trained_like as T
from yoho_amd import weights as W

F32 = np.float32
CASES = T.cases()
IDS = [T.case_id(fam, seed) for fam, _, seed in CASES]
TEETH = 10.0                      # a planted defect must land at this many times the budget


# ---- a. the generated dicts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", T.NETS)
@pytest.mark.parametrize("fam,lo,seed", CASES, ids=IDS)
def test_generated_dict_has_the_statistics_of_a_trained_network(net, fam, lo, seed):
    sd, meta = T.build(net, seed, lo)
    base, spec = T.base_state_dict(net)
    W.check_state_dict(sd, spec)
    assert set(sd) == set(base) and all(sd[k].dtype == base[k].dtype and sd[k].shape == base[k].shape for k in sd)
    assert all(np.isfinite(v).all() for v in sd.values())
    assert T.build(net, seed, lo)[0] is sd and not sd[meta["bns"][0] + ".weight"].flags.writeable
    g = np.concatenate([sd[b + ".weight"] for b in meta["bns"]])
    v = np.concatenate([sd[b + ".running_var"] for b in meta["bns"]])
    neg = float((g < 0).mean())
    decades = float(np.log10(v[v > 0].max() / v[v > 0].min()))
    below = float((v < 1e-5).mean())
    print("%s %s seed %d: %d BatchNorms, %d channels; gamma < 0: %.3f; running_var %.3g .. %.3g (%.1f decades), %.3f of them below eps, %d exactly 0" % (
        net, fam, seed, len(meta["bns"]), len(g), neg, v[v > 0].min(), v.max(), decades, below, int((v == 0).sum())))
    assert 0.05 <= neg <= 0.35
    assert (v >= 0).all() and below > 0
    if fam == "cal8":
        assert decades >= 6.0
    for b in meta["bns"]:
        gb = sd[b + ".weight"]
        assert gb[meta["gamma_zero"][b]] == 0.0 and gb[meta["gamma_tiny"][b]] == F32(-2.0 ** -10)
    conv_of = T.conv_of_bn(net)
    assert len(conv_of) == len(meta["dead_row"]) == len(meta["bns"]) - (net == "partII")
    for b, conv in conv_of.items():
        w = sd[conv + (".kernel" if net.startswith("fcgf") else ".weight")]
        row, col = meta["dead_row"][conv], meta["dead_col"][conv]
        wo = np.moveaxis(w, -1, 0) if net.startswith("fcgf") else w                      # output channel first
        wi = np.moveaxis(w, -2, 0) if net.startswith("fcgf") else np.moveaxis(w, 1, 0)   # input channel first
        assert not wo[row].any() and (col is None) == (wi.shape[0] == 1)
        assert col is None or not wi[col].any()
        if conv + ".bias" in sd:
            assert sd[conv + ".bias"][row] == 0.0
        # the dead channel reaches its BatchNorm dead: mean 0 and variance 0 (s = gamma / sqrt(eps)), under a gamma of its own
        assert sd[b + ".running_mean"][row] == 0.0 and sd[b + ".running_var"][row] == 0.0
        assert row not in (meta["gamma_zero"][b], meta["gamma_tiny"][b])
        # row scales: the layer's rows spread over at least half of |lo| binades under ONE plane scale
        top = np.max(np.abs(wo.reshape(len(wo), -1)), axis=1)
        spread = float(np.log2(top.max() / top[top > 0].min()))
        assert spread >= 0.5 * abs(lo), (conv, spread)


def test_reference_modules_behave_as_before_for_plain_calls(tables):
    """the hook points added for the calibration are no stages and change no value: a pass with a pass-through hook equals the cached
    plain pass, whose stage tensors are the documented ones"""
    sd, _ = T.base_state_dict("partII")
    feats, pre = R.partII_input(3)
    seen = []
    q, st = R.partII_forward64(*feats, pre, sd, tables.N, tables.P, stages=True)
    q2, st2 = R.partII_forward64(*feats, pre, sd, tables.N, tables.P, stages=True, hook=lambda n, t: (seen.append(n), t)[1])
    assert seen == ["x_in", "a_in", "h0", "a0", "mid", "a1", "h2", "f1", "t1", "f2", "t2", "q"]
    assert list(st) == list(st2) == ["a_in", "h0", "a0", "mid", "a1", "h2", "t1", "t2", "q"]
    assert np.array_equal(q, q2) and all(np.array_equal(st[k], st2[k]) for k in st)
    assert R.partII_forward64(*feats, pre, sd, tables.N, tables.P) is q
    coords = F.cloud_2b()
    sdb = F.state_dict_2b()
    names = []
    ref = F.resunet_forward64(coords, sdb, 5)
    again = F.resunet_forward64(coords, sdb, 5, bn_hook=lambda n, x: names.append(n))
    assert again is not ref and np.array_equal(again, ref) and F.resunet_forward64(coords, sdb, 5) is ref
    assert names[:3] == ["norm1", "block1.norm1", "block1.norm2"] and len(names) == 21 and all(n + ".bn.weight" in sdb for n in names)


# ---- b. every GPU case is a factor 2 inside the planes -------------------------------------------------------------------------------
def _margin(st):
    a, c = R.stage_extent(st)
    return R.ACT_LIMIT / a, R.COEF_LIMIT / c


def test_partI_cases_are_inside_the_planes(tables):
    done = set()
    for fam, lo, seed, B, _ in T.partI_cases():
        if (fam, seed, B) in done:
            continue
        done.add((fam, seed, B))
        _, eref, st = R.partI_case(R.partI_input(B), T.state_dict("partI", seed, lo), tables.N)
        ma, mc = _margin(st)
        print("PartI %s seed %d B=%d: activations %.0f x inside, coefficients %.0f x; e_ref %.3g" % (fam, seed, B, ma, mc, eref))
        assert ma >= 2.0 and mc >= 2.0
    for fam, lo, seed in T.pair_cases():
        _, eref, st = R.partI_case(np.concatenate(T.pair_input()), T.state_dict("partI", seed, lo), tables.N)
        ma, mc = _margin(st)
        print("PartI %s seed %d pair %d + %d: %.0f x / %.0f x; e_ref %.3g" % (fam, seed, *T.PAIR, ma, mc, eref))
        assert ma >= 2.0 and mc >= 2.0


def test_partII_cases_are_inside_the_planes(tables):
    done = set()
    for fam, lo, seed, M, _ in T.partII_cases():
        if (fam, seed, M) in done:
            continue
        done.add((fam, seed, M))
        feats, pre = R.partII_input(M)
        _, eref, st = R.partII_case(*feats, pre, T.state_dict("partII", seed, lo), tables.N, tables.P)
        ma, mc = _margin(st)
        print("PartII %s seed %d M=%d: activations %.0f x inside, coefficients %.0f x; e_ref %.3g" % (fam, seed, M, ma, mc, eref))
        assert ma >= 2.0 and mc >= 2.0


def _fcgf_top(coords, sd, k):
    return max(float(np.abs(x).max()) for name, x in F.conv_inputs(coords, sd, k).items() if name != "conv1")


@pytest.mark.parametrize("net,fam,lo,seed", T.fcgf_cases(), ids=["%s-%s" % (n, T.case_id(f, s)) for n, f, _, s in T.fcgf_cases()])
def test_backbone_cases_are_inside_the_planes(net, fam, lo, seed):
    """16 x the largest input of a split convolution against the fp16 range (the planes hold 16 x the activation), a factor 2 inside;
    for the default configuration also on the second cloud of its batch, which the statistics were not calibrated on"""
    cloud, k, _ = T.FCGF_NETS[net]
    sd = T.state_dict(net, seed, lo)
    clouds = [cloud()] + ([F.cloud_2b()] if net == "fcgf" else [])
    for coords in clouds:
        top = _fcgf_top(coords, sd, k)
        print("%s %s seed %d, %d voxels: largest convolution input %.3g, %.0f x inside" % (net, fam, seed, len(coords), top, F.F16_OVER / (16.0 * top)))
        assert 2.0 * 16.0 * top < F.F16_OVER and 2.0 * top < F.ACT_LIMIT


# ---- c. the documented plane arithmetic stays inside the budgets, and a planted defect does not -------------------------------------
def _planes(v, scale):
    """(hi, lo) as float64 of v * scale: hi = fp16(.), lo = fp16(. - hi), through fp32 as the kernels do"""
    vs = (v * scale).astype(F32)
    hi = vs.astype(np.float16)
    return hi.astype(np.float64), (vs - hi.astype(F32)).astype(np.float16).astype(np.float64)


def _split_conv(x, w, b, N, flush_w):
    """ref64._conv with every product as hi*Wh + lo*Wh + hi*Wl (float64 sums: the plane rounding alone): activations times 16, weights
    times the layer's ONE power of two that puts the largest |w| in [2^9, 2^10)"""
    B, C, _ = x.shape
    O = w.shape[0]
    ws = F.split_scale(w)
    wh, wl = _planes(np.ascontiguousarray(w.astype(np.float64).reshape(O, C * R.NTAP).T), ws)
    if flush_w:
        wl = np.where(np.abs(wl) < 2.0 ** -14, 0.0, wl)
    xg = x[:, :, N.reshape(-1)].reshape(B, C, R.G, R.NTAP)
    ah, al = _planes(np.ascontiguousarray(xg.transpose(0, 2, 1, 3)).reshape(B * R.G, C * R.NTAP), 16.0)
    out = ((ah + al) @ wh + ah @ wl) / (16.0 * ws) + b.astype(np.float64)[None, :]
    return out.reshape(B, R.G, O).transpose(0, 2, 1)


def partI_emulated(x, sd, N, flush_w=False):
    """ref64.partI_forward64 in direct (13-tap) form on the split products; `sd` may carry a planted defect of the BatchNorm fold"""
    p, r = R._P1, R._R1
    conv = lambda v, name: _split_conv(v, sd[name + ".weight"], sd[name + ".bias"], N, flush_w)
    with np.errstate(all="ignore"):
        x64 = np.asarray(x, F32).astype(np.float64)
        h0 = conv(x64, p + "Conv_in.0")
        mid = conv(R._bn_relu(h0, sd, r + "comb_layer_in.0"), r + "comb_layer_in.2")
        h2 = conv(R._bn_relu(mid, sd, r + "comb_layer_out.0"), r + "comb_layer_out.2") + h0
        eqv = conv(R._bn_relu(h2, sd, p + "Conv_out.comb_layer.0"), p + "Conv_out.comb_layer.2") + x64
        inv = np.mean(eqv, axis=-1)
        n_e = np.maximum(np.sqrt(np.sum(eqv * eqv, axis=1, keepdims=True)), 1e-4)
        n_i = np.maximum(np.sqrt(np.sum(inv * inv, axis=1, keepdims=True)), 1e-4)
        return eqv / n_e, inv / n_i


def abs_gamma(sd, eps):
    """defect: the fold takes |gamma| (an epilogue that assumes a positive scale)"""
    return {k: np.abs(v) if k.endswith(".weight") and v.ndim == 1 else v for k, v in sd.items()}


def no_eps(sd, eps):
    """defect: s = gamma / sqrt(var).  Written as a float64 variance of var - eps, so that the passes' own var + eps gives var back (to
    1e-21 absolute, exactly for the dead channels, whose scale becomes infinite)"""
    return {k: v.astype(np.float64) - np.float64(eps) if k.endswith(".running_var") else v for k, v in sd.items()}


def no_eps_live(sd, eps):
    """the same on the live channels only (the dead ones alone would give it away as NaN): the channels whose variance is near or
    below eps, which the narrow synthetic family does not have, carry the rejection"""
    return {k: np.where(v > 0, v.astype(np.float64) - np.float64(eps), 0.0) if k.endswith(".running_var") else v for k, v in sd.items()}


DEFECTS = {"abs_gamma": (abs_gamma, False), "no_eps": (no_eps, False), "no_eps_live": (no_eps_live, False),
           "flush_weight_lo": (lambda sd, eps: sd, True)}


def emulate_flush_w(name, x, W):
    """fcgf_ref64.emulate_fp16x2('faithful') with the weights' lo plane flushed below 2^-14"""
    if x.shape[1] % 32 or W.shape[-1] % 32:
        return x, W
    hi, lo = F._planes(x.astype(F32) * F32(16.0), False)
    ws = F.split_scale(W)
    wh, wl = F._planes((W.astype(F32) * F32(ws)).astype(F32), False)
    wl = np.where(np.abs(wl) < F.F16_MIN_NORMAL, 0.0, wl)
    d = 1.0 / (ws * 16.0)
    return [((hi + lo) * d, wh), (hi * d, wl)]


@pytest.mark.parametrize("fam,lo,seed", CASES, ids=IDS)
def test_partI_plane_emulation_is_inside_the_budget(tables, fam, lo, seed):
    sd = T.state_dict("partI", seed, lo)
    x = R.partI_input(T.PARTI_B)
    ref, eref, _ = R.partI_case(x, sd, tables.N)
    ok, worst = R.within_budget(partI_emulated(x, sd, tables.N), ref, eref)
    print("PartI %s seed %d B=%d: e_ref %.3g, plane emulation %.2f e_ref of %g" % (fam, seed, T.PARTI_B, eref, worst, R.FACTOR))
    assert ok


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_partI_cases_reject_a_planted_defect(tables, defect):
    change, flush = DEFECTS[defect]
    x = R.partI_input(T.PARTI_B)
    worst = []
    for fam, lo, seed in CASES:
        sd = T.state_dict("partI", seed, lo)
        ref, eref, _ = R.partI_case(x, sd, tables.N)
        ok, w = R.within_budget(partI_emulated(x, change(sd, R.orc.BN_EPS), tables.N, flush_w=flush), ref, eref)
        print("PartI %s seed %d, %s: %.3g e_ref (budget %g)" % (fam, seed, defect, w, R.FACTOR))
        assert not ok or defect == "flush_weight_lo"          # the BatchNorm defects are rejected by every case
        worst.append(w)
    assert max(worst) >= TEETH * R.FACTOR


@pytest.mark.parametrize("net,fam,lo,seed", T.fcgf_cases(), ids=["%s-%s" % (n, T.case_id(f, s)) for n, f, _, s in T.fcgf_cases()])
def test_backbone_emulation_is_inside_the_budget(net, fam, lo, seed):
    cloud, k, _ = T.FCGF_NETS[net]
    coords, sd = cloud(), T.state_dict(net, seed, lo)
    ref, eref = F.case(coords, sd, k)
    out = F.emulated(coords, sd, k)
    errs = F.errors(out, ref)
    print("%s %s seed %d: e_ref %.3g, faithful emulation rel %.3g rel_rows %.3g = %.2f e_ref" % (net, fam, seed, eref, *errs, max(errs) / eref))
    assert np.isfinite(out).all() and np.allclose(np.sum(ref * ref, axis=1), 1.0, rtol=0, atol=1e-12)
    assert F.in_budget(out, ref, errs, eref)[0]
    assert max(errs) < R.FACTOR * eref                          # the documented arithmetic is fp32-accurate on these weights


@pytest.mark.parametrize("defect", list(DEFECTS))
def test_backbone_cases_reject_a_planted_defect(defect):
    change, flush = DEFECTS[defect]
    cloud, k, _ = T.FCGF_NETS["fcgf"]
    coords = cloud()
    worst = []
    for fam, lo, seed in CASES:
        sd = T.state_dict("fcgf", seed, lo)
        ref, eref = F.case(coords, sd, k)
        errs = F.errors(F.emulated(coords, sd, k), ref)
        with np.errstate(all="ignore"):
            bad = F.resunet_forward64(coords, change(sd, F.EPS), k, hook=emulate_flush_w if flush else F.emulate_fp16x2())
        ok, w = F.in_budget(bad, ref, errs, eref)
        print("backbone %s seed %d, %s: (error - emu) / e_ref %.3g (budget %g)" % (fam, seed, defect, w, F.C_BUDGET))
        assert not ok or defect == "flush_weight_lo"
        worst.append(w)
    assert max(worst) >= TEETH * F.C_BUDGET
