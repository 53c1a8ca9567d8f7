"""State dicts with the statistics of a TRAINED network, for PartI, PartII and the FCGF backbone (helper of
tests/test_trained_like_cpu.py and tests/test_gpu_trained_like.py, not a conftest; numpy only, deterministic).

yoho_amd.weights.synth_state_dict draws a narrow family: uniform conv weights of one scale per layer, BatchNorm gammas in [0.5, 1.5],
running variances in [0.5, 1.5], small means.  A trained checkpoint has none of that.  `state_dict(net, seed, lo)` starts from the
suite's synthetic weights of `net` and distorts them layer by layer, in forward order:

  a conv followed by a BatchNorm   every weight times |Student-t(3)| (heavy tails); output row o (weights and bias) times
                                   r_o = 2^U(lo, 0), so the rows of ONE layer spread over |lo| binades under the layer's single
                                   power-of-two plane scale; one output row all zero, bias included (a dead channel); one input
                                   column all zero
  a conv with none behind it       the tails, and r_o = 2^U(-4, 0)
  every BatchNorm                  gamma ~ N(0.6, 0.6) (about one in six negative), one gamma exactly 0, one -2^-10; beta ~ N(0, 0.3);
                                   running_mean / running_var = the float64 mean and biased variance of THAT BatchNorm's input over a
                                   calibration batch, cast to fp32

The calibration is what keeps such a network inside the fp16 planes (uncalibrated, the same distortions drive the stages past 1e5): it
is one hooked float64 pass (ref64 / fcgf_ref64), whose hook writes the statistics of a BatchNorm's input into the dict before the pass
reads them.  The variances then span many decades, fall below eps = 1e-5 for the small rows and are exactly 0, with mean 0, for the dead
row.  Where a conv's output takes a residual (h2 = conv(a1) + h0 in PartI) the dead row is the dead row of the layer that produced the
residual, so that the channel is dead in front of the BatchNorm as well.

Families: cal8 (lo = -8) and cal14 (lo = -14), SEEDS each.  `build` caches per (net, seed, lo) and also returns what was planted where.
"""
import numpy as np

import fcgf_ref64 as F
import ref64 as R

FAMILIES = {"cal8": -8.0, "cal14": -14.0}
# The first two seeds at which the cal8 dict of EVERY network spans six decades of running_var, the property
# tests/test_trained_like_cpu.py asserts: 2^U(-8, 0) row scales give 4.8 decades of variance, the tails and the layers' own scales the
# rest - 5.3 to 6.9 per dict over seeds 1 .. 62, fewer than half of them at 6 or more.  Nothing else entered the choice.
SEEDS = (25, 62)
LO_PLAIN = -4.0                      # row scales of a conv that no BatchNorm follows
CAL_SEED = 31337                     # unit_features seed of the calibration batches: no test input uses it (nor CAL_SEED + 1 .. + 4)
CAL_ROWS = {"partI": 64, "partII": 40}
NETS = ("partI", "partII", "fcgf", "fcgf_2b")

_P1, _R1, _R2 = R._P1, R._R1, R._R2
# (conv, the BatchNorm behind it or None, the stage the hook sees in front of that BatchNorm, the conv whose dead row it shares or None)
_LAYERS = {
    "partI": [(_P1 + "Conv_in.0", _R1 + "comb_layer_in.0", "h0", None),
              (_R1 + "comb_layer_in.2", _R1 + "comb_layer_out.0", "mid", None),
              (_R1 + "comb_layer_out.2", _P1 + "Conv_out.comb_layer.0", "h2", _P1 + "Conv_in.0"),
              (_P1 + "Conv_out.comb_layer.2", None, None, None)],
    "partII": [(None, "Conv_init.comb_layer.0", "x_in", None),
               ("Conv_init.comb_layer.2", _R2 + "comb_layer_in.0", "h0", None),
               (_R2 + "comb_layer_in.2", _R2 + "comb_layer_out.0", "mid", None),
               (_R2 + "comb_layer_out.2", None, None, None),
               ("PartII_To_R_FC.0", "PartII_To_R_FC.1", "f1", None),
               ("PartII_To_R_FC.3", "PartII_To_R_FC.4", "f2", None),
               ("PartII_To_R_FC.6", None, None, None)],
}


def base_state_dict(net):
    """the suite's own synthetic weights of `net`, and for the backbone the arguments of its load"""
    from yoho_amd import weights as W
    if net == "partI":
        return W.synth_state_dict(W.PARTI_SPEC, 7), W.PARTI_SPEC
    if net == "partII":
        return W.synth_state_dict(W.PARTII_SPEC, 8), W.PARTII_SPEC
    if net == "fcgf":
        return F.state_dict(), W.FCGF_SPEC
    assert net == "fcgf_2b"
    return F.state_dict_2b(), W.fcgf_spec((None, 32, 64, 128, 256), (None, 64, 64, 64, 64), 32, 5)


def calibration_input(net):
    from yoho_amd import synth
    if net == "partI":
        return synth.unit_features(CAL_ROWS[net], seed=CAL_SEED)
    if net == "partII":
        M = CAL_ROWS[net]
        return [synth.unit_features(M, seed=CAL_SEED + 1 + i) for i in range(4)], np.random.RandomState(CAL_SEED).randint(0, R.G, size=M).astype(np.int64)
    return F.small_cloud() if net == "fcgf" else F.cloud_2b()


def _distort_conv(rng, w, b, out_axis, in_axis, lo, dead, meta, name):
    """tails, row scales, a dead row and a dead column, in place on float64 copies -> (w, b) as fp32"""
    w = w.astype(np.float64) * np.abs(rng.standard_t(3, size=w.shape))
    O, I = w.shape[out_axis], w.shape[in_axis]
    r = 2.0 ** rng.uniform(lo, 0.0, size=O)
    shape = [1] * w.ndim
    shape[out_axis] = O
    w *= r.reshape(shape)
    if b is not None:
        b = b.astype(np.float64) * r.reshape(b.shape)
    if dead is not None:                                   # a layer that a BatchNorm follows
        row = int(rng.randint(O)) if dead < 0 else dead
        col = int(rng.randint(I)) if I > 1 else None       # the backbone's first conv has one input channel: it keeps it
        idx = [slice(None)] * w.ndim
        idx[out_axis] = row
        w[tuple(idx)] = 0.0
        if b is not None:
            b.reshape(-1)[row] = 0.0
        if col is not None:
            idx = [slice(None)] * w.ndim
            idx[in_axis] = col
            w[tuple(idx)] = 0.0
        meta["dead_row"][name], meta["dead_col"][name] = row, col
    return w.astype(np.float32), None if b is None else b.astype(np.float32)


def _distort_bn(rng, sd, prefix, avoid, meta):
    C = sd[prefix + ".weight"].shape[0]
    g = rng.normal(0.6, 0.6, size=C)
    free = [c for c in rng.permutation(C) if c != avoid]          # the dead channel keeps a gamma of its own: s = gamma / sqrt(eps)
    zero, tiny = int(free[0]), int(free[1])
    g[zero], g[tiny] = 0.0, -2.0 ** -10
    sd[prefix + ".weight"] = g.astype(np.float32)
    sd[prefix + ".bias"] = rng.normal(0.0, 0.3, size=C).astype(np.float32)
    meta["gamma_zero"][prefix], meta["gamma_tiny"][prefix] = zero, tiny


def _stats(x):
    """float64 mean and biased variance per channel (axis 1) -> fp32"""
    ax = tuple(a for a in range(x.ndim) if a != 1)
    return np.mean(x, axis=ax).astype(np.float32), np.var(x, axis=ax).astype(np.float32)


_BUILT = {}


def build(net, seed, lo):
    """-> (state dict, meta); meta: dead_row / dead_col by conv, gamma_zero / gamma_tiny by BatchNorm prefix, bns (prefixes in forward
    order).  Cached: every caller gets the same arrays (read-only)."""
    key = (net, int(seed), float(lo))
    if key in _BUILT:
        return _BUILT[key]
    assert net in NETS
    base, _ = base_state_dict(net)
    sd = {k: np.array(v, copy=True) for k, v in base.items()}
    rng = np.random.RandomState([int(seed), NETS.index(net)])
    meta = dict(dead_row={}, dead_col={}, gamma_zero={}, gamma_tiny={}, bns=[])
    if net in _LAYERS:
        stage_of = {}
        for conv, bn, stage, shares in _LAYERS[net]:
            if conv is not None:
                dead = None if bn is None else (-1 if shares is None else meta["dead_row"][shares])
                sd[conv + ".weight"], sd[conv + ".bias"] = _distort_conv(rng, sd[conv + ".weight"], sd[conv + ".bias"], 0, 1,
                                                                         lo if bn is not None else LO_PLAIN, dead, meta, conv)
            if bn is not None:
                _distort_bn(rng, sd, bn, meta["dead_row"].get(conv, -1), meta)
                stage_of[stage] = bn
                meta["bns"].append(bn)

        def hook(name, t):
            if name in stage_of:
                sd[stage_of[name] + ".running_mean"], sd[stage_of[name] + ".running_var"] = _stats(t)
            return t
        from yoho_amd.tables import default_tables
        tb = default_tables()
        if net == "partI":
            R.partI_forward64(calibration_input(net), sd, tb.N, hook=hook)
        else:
            feats, pre = calibration_input(net)
            R.partII_forward64(*feats, pre, sd, tb.N, tb.P, hook=hook)
    else:
        for k in [k for k in base if k.endswith(".kernel")]:                    # the spec's order is the forward order
            conv = k[:-len(".kernel")]
            bn = None if conv in ("conv1_tr", "final") else conv.replace("conv", "norm")
            w = sd[k]
            bias = sd["final.bias"] if conv == "final" else None
            w, bias = _distort_conv(rng, w, bias, w.ndim - 1, w.ndim - 2, lo if bn else LO_PLAIN, -1 if bn else None, meta, conv)
            sd[k] = w
            if bias is not None:
                sd["final.bias"] = bias
            if bn:
                _distort_bn(rng, sd, bn + ".bn", meta["dead_row"][conv], meta)
                meta["bns"].append(bn + ".bn")

        def bn_hook(name, x):
            sd[name + ".bn.running_mean"], sd[name + ".bn.running_var"] = _stats(x)
        F.resunet_forward64(calibration_input(net), sd, 7 if net == "fcgf" else 5, bn_hook=bn_hook)
    for v in sd.values():
        v.setflags(write=False)
    _BUILT[key] = (sd, meta)
    return _BUILT[key]


def state_dict(net, seed, lo):
    return build(net, seed, lo)[0]


def conv_of_bn(net):
    """{BatchNorm prefix: the conv in front of it} (PartII's first BatchNorm has none)"""
    if net in _LAYERS:
        return {bn: conv for conv, bn, _, _ in _LAYERS[net] if bn is not None and conv is not None}
    base, _ = base_state_dict(net)
    return {k[:-len(".kernel")].replace("conv", "norm") + ".bn": k[:-len(".kernel")] for k in base
            if k.endswith(".kernel") and k not in ("conv1_tr.kernel", "final.kernel")}


def cases():
    """[(family, lo, seed)] of the suite"""
    return [(fam, lo, seed) for fam, lo in FAMILIES.items() for seed in SEEDS]


# ----------------------------------------------------------------------------------------
# the cases of tests/test_gpu_trained_like.py (tests/test_trained_like_cpu.py asserts the range margins of every one of them)
# ----------------------------------------------------------------------------------------
# The smallest sizes that reach a ragged 32-keypoint tile and both 16-column halves of a slab tile (33, 17), a second, ragged
# 256-column tile (257), and a pair pass whose fragment boundary lies inside a column tile (33 + 31).  The large sizes and the pair run
# on the first seed of each family.
PARTI_MODES = ("fgemm", "fgemm128", "fp16x2", "fourier", "bf16x3", "f32")
PARTII_MODES = ("fp16x2", "cgemm", "bf16x3", "f32")
BIG_MODES = {"partI": ("fgemm", "f32"), "partII": ("fp16x2", "f32")}
PARTI_B, PARTII_M, BIG, PAIR = 33, 17, 257, (33, 31)
case_id = lambda fam, seed: "%s-s%d" % (fam, seed)


def partI_cases():
    """-> [(family, lo, seed, B, mode)]"""
    out = [(fam, lo, seed, PARTI_B, m) for fam, lo, seed in cases() for m in PARTI_MODES]
    return out + [(fam, lo, SEEDS[0], BIG, m) for fam, lo in FAMILIES.items() for m in BIG_MODES["partI"]]


def partII_cases():
    out = [(fam, lo, seed, PARTII_M, m) for fam, lo, seed in cases() for m in PARTII_MODES]
    return out + [(fam, lo, SEEDS[0], BIG, m) for fam, lo in FAMILIES.items() for m in BIG_MODES["partII"]]


def pair_cases():
    return [(fam, lo, SEEDS[0]) for fam, lo in FAMILIES.items()]


def pair_input():
    """the two fragments of the pair pass; the reference is the pass over their concatenation"""
    return R.partI_input(PAIR[0]), R.partI_input(PAIR[1])


FCGF_NETS = {"fcgf": (F.small_cloud, 7, {}), "fcgf_2b": (F.cloud_2b, 5, dict(normalize_feature=False, **F.SPEC_2B))}


def fcgf_cases():
    """-> [(net, family, lo, seed)]: each runs alone in a default context and in a YOHO_FCGF=f32 one; the default configuration also
    runs both clouds in one batch"""
    return [(net, fam, lo, seed) for net in FCGF_NETS for fam, lo, seed in cases()]
