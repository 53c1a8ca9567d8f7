"""The FCGF backbone in float64, an emulation of its fp16x2 split arithmetic inside that pass, and the error budget built on both
(helper of tests/test_fcgf_precision_cpu.py and tests/test_gpu_fcgf_precision.py, not a conftest).

`resunet_forward64` restates oracle/fcgf_oracle.py:resunet_forward with every step in float64 - the same operation sequence, the
oracle's own `stride_coords` and `kernel_map` (memoised per coordinate set: the maps depend on nothing else) - and normalises the rows
once (in float64 the second normalisation of fcgf_feat.py:48 changes nothing).  The fp32 oracle stays as it is and is the thing MEASURED:
`e_ref` is its distance from float64 (ref64.e_ref), and stands for fp32 accumulation in the budget.

`hook(name, x, W)` is called in front of every convolution (name = the state-dict prefix of its kernel: "conv1", "block1.conv1", ...,
"conv4_tr", ..., "conv1_tr", "final"; x the float64 input rows, W the float64 kernel) and returns either `(x, W)` or a list of such
pairs whose convolutions are summed - a split product is a sum of plane products, and one that leaves a cross term out cannot be
written as one pair.  A pass with a hook is never cached.  `relu=` replaces the ReLU (np.maximum: NaN stays NaN).  `bn_hook(name, x)` is
called with the input rows of every BatchNorm (name = its state-dict prefix without ".bn": "norm1", "block1.norm1", ...) before its
statistics are read from the state dict, so that a hook may write them there (tests/trained_like.py calibrates so); such a pass is not
cached either.

`emulate_fp16x2` is the hook that reproduces csrc/spconv.hip:split_pair_sp and csrc/sparse.hip:up_conv: activations through fp32, times
16, hi = fp16(.), lo = fp16(. - hi); weights times 2^(10 - exponent of the largest), the same two planes; the product lo*Wh + hi*Wl +
hi*Wh (no lo*Wl) in float64, descaled.  What remains between it and the device is the fp32 accumulation.  Its other modes are the defects
the CPU tests prove the budget rejects.

Scale sweep: `scale_activations(sd, lam)` returns a state dict whose every activation is lam times the original's (lam a power of two:
exactly, in fp32 and in float64) and whose unit-row output is therefore the same - one float64 reference serves every lam."""
import contextlib
import os
import sys

import numpy as np

import ref64 as R
from ref64 import rel, rel_rows, e_ref, within_budget, errors  # noqa: F401  (the suite's own measures, re-exported)

sys.path.insert(0, os.path.join(R.REPO, "oracle"))
import fcgf_oracle as fo  # noqa: E402

F64 = np.float64
EPS = F64(fo.EPS)

# ----------------------------------------------------------------------------------------
# the budget: a kernel's error against float64 may be emu(lam) + C_BUDGET * e_ref, in rel and in rel_rows, where emu(lam) is the
# faithful emulation's own error at that scale (plane rounding: it grows once the lo planes go subnormal) and e_ref the fp32 oracle's
# (fp32 accumulation).  C_BUDGET is twice the worst (error - emu) / e_ref measured on an MI355X over every case of
# tests/test_gpu_fcgf_precision.py; the factor two covers summation orders that change with the kernel choice.  One run, worst per group
# (profiles/precision.md, backbone section, has all of them): 4770-voxel cloud 1.13 (lam = 2^-4; 0.23 / -0.11 at 2^-12 / 2^-8, where the
# device is at 1.01 / 0.95 of the emulated error: gfx950 keeps the subnormal lo planes), fine cloud 0.83 in range and 0.98 on the finite
# rows past the limit, the 37-point cloud of its batch 2.14 (lam = 2^-8), YOHO_FCGF=f32 1.95 at every scale, ResUNetBN2B 1.16, one large
# weight 0.85.  Worst 2.14.  Every defect tests/test_fcgf_precision_cpu.py emulates is at 250 or more.
# ----------------------------------------------------------------------------------------
C_BUDGET = 4.3
ACT_LIMIT = 4094.0      # include/yoho_hip.h, FCGF section: 16 x rounds to a finite fp16 below 4095; the header promises 4094
F16_OVER = 65520.0      # the smallest magnitude that fp16 rounds to infinity
F16_MIN_NORMAL = 2.0 ** -14
LAMBDAS_IN_RANGE = (2.0 ** -12, 2.0 ** -8, 2.0 ** -4, 1.0, 2.0 ** 4, 2.0 ** 8)
LAMBDAS_OVER = (2.0 ** 9, 2.0 ** 10)


def budget_multiples(got, ref, emu_errs, eref, rows=None):
    """[(rel - emu_rel) / e_ref, (rel_rows - emu_rel_rows) / e_ref] of `got` against the float64 `ref` (over `rows` only, if given)"""
    if rows is not None:
        got, ref = np.asarray(got)[rows], ref[rows]
    return [(e - m) / eref for e, m in zip(errors(np.asarray(got), ref), emu_errs)]


def in_budget(got, ref, emu_errs, eref, c=None, rows=None):
    """THE acceptance test of the backbone's precision suite: finite, and error <= emu + c * e_ref in rel and in rel_rows.
    -> (ok, worst (error - emu) / e_ref)"""
    got = np.asarray(got)
    if not np.isfinite(got if rows is None else got[rows]).all():
        return False, float("inf")
    worst = max(budget_multiples(got, ref, emu_errs, eref, rows))
    return bool(worst < (C_BUDGET if c is None else c)), worst


# ----------------------------------------------------------------------------------------
# coordinate and kernel maps (the oracle's, memoised)
# ----------------------------------------------------------------------------------------
_MAPS = {}


def _levels(coords):
    c1 = np.ascontiguousarray(coords, dtype=np.int32)
    key = c1.tobytes()
    if key not in _MAPS:
        c2 = fo.stride_coords(c1, 2)
        c4 = fo.stride_coords(c2, 4)
        c8 = fo.stride_coords(c4, 8)
        _MAPS[key] = ((c1, c2, c4, c8), {})
    return _MAPS[key]


def _kmap(maps, cs, li, lo, ksize, ts, transpose):
    key = (li, lo, ksize, ts, transpose)
    if key not in maps:
        maps[key] = fo.kernel_map(cs[li], cs[lo], ksize, ts, transpose)
    return maps[key]


@contextlib.contextmanager
def _memoised_oracle_maps():
    """the fp32 oracle rebuilds the kernel map of every convolution (21 of them over 4 distinct coordinate sets): let it find them"""
    orig, memo = fo.kernel_map, {}

    def km(ci, co, ksize, ts, transpose=False):
        key = (np.asarray(ci).tobytes(), np.asarray(co).tobytes(), ksize, ts, transpose)
        if key not in memo:
            memo[key] = orig(ci, co, ksize, ts, transpose)
        return memo[key]
    fo.kernel_map = km
    try:
        yield
    finally:
        fo.kernel_map = orig


# ----------------------------------------------------------------------------------------
# the float64 pass
# ----------------------------------------------------------------------------------------
def _bn(x, sd, name, bn_hook=None):
    if bn_hook is not None:
        bn_hook(name, x)
    g, b = sd[name + ".bn.weight"].astype(F64), sd[name + ".bn.bias"].astype(F64)
    m, v = sd[name + ".bn.running_mean"].astype(F64), sd[name + ".bn.running_var"].astype(F64)
    s = g / np.sqrt(v + EPS)
    return x * s + (b - m * s)


def nan_relu(x):
    return np.maximum(x, 0.0)                  # NaN stays NaN


def swallowing_relu(x):
    """defect: fmaxf(v, 0.f) - a NaN comes out as 0"""
    return np.fmax(x, 0.0)


def _forward64(coords, sd, k1, hook, relu, bn_hook=None):
    (cs, maps) = _levels(coords)
    n = [len(c) for c in cs]

    def conv(name, x, li, lo, ksize, ts, transpose=False):
        W = sd[name + ".kernel"].astype(F64)
        terms = hook(name, x, W) if hook is not None else (x, W)
        if isinstance(terms, tuple):
            terms = [terms]
        out = None
        with np.errstate(invalid="ignore", over="ignore"):
            for xt, Wt in terms:
                if Wt.ndim == 2:
                    o = xt @ Wt
                else:
                    rows_all = _kmap(maps, cs, li, lo, ksize, ts, transpose)
                    o = np.zeros((n[lo], Wt.shape[2]), F64)
                    for k, rows in enumerate(rows_all):
                        m = rows >= 0
                        if m.any():
                            o[m] += xt[rows[m]] @ Wt[k]
                out = o if out is None else out + o
        return out

    def bn(x, name):
        return _bn(x, sd, name, bn_hook)

    def block(x, l, ts, name):
        out = relu(bn(conv(name + ".conv1", x, l, l, 3, ts), name + ".norm1"))
        out = bn(conv(name + ".conv2", out, l, l, 3, ts), name + ".norm2")
        return relu(out + x)

    x = np.ones((n[0], 1), F64)
    s1 = block(bn(conv("conv1", x, 0, 0, k1, 1), "norm1"), 0, 1, "block1")
    s2 = block(bn(conv("conv2", relu(s1), 0, 1, 3, 1), "norm2"), 1, 2, "block2")
    s4 = block(bn(conv("conv3", relu(s2), 1, 2, 3, 2), "norm3"), 2, 4, "block3")
    s8 = block(bn(conv("conv4", relu(s4), 2, 3, 3, 4), "norm4"), 3, 8, "block4")
    out = block(bn(conv("conv4_tr", relu(s8), 3, 2, 3, 4, True), "norm4_tr"), 2, 4, "block4_tr")
    out = np.concatenate([relu(out), s4], 1)
    out = block(bn(conv("conv3_tr", out, 2, 1, 3, 2, True), "norm3_tr"), 1, 2, "block3_tr")
    out = np.concatenate([relu(out), s2], 1)
    out = block(bn(conv("conv2_tr", out, 1, 0, 3, 1, True), "norm2_tr"), 0, 1, "block2_tr")
    out = np.concatenate([relu(out), s1], 1)
    out = relu(conv("conv1_tr", out, 0, 0, 1, 1))
    out = conv("final", out, 0, 0, 1, 1) + sd["final.bias"].astype(F64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return out / np.sqrt(np.sum(out * out, axis=1, keepdims=True))


_CACHE = {}


def _cached(kind, coords, sd, k1, fn):
    key = (kind, k1, R._digest(sd, [np.ascontiguousarray(coords, dtype=np.int32)]))
    if key not in _CACHE:
        res = fn()
        res.setflags(write=False)                 # shared among tests: nobody changes it
        _CACHE[key] = res
    return _CACHE[key]


def resunet_forward64(coords, sd, conv1_kernel_size=7, hook=None, relu=None, bn_hook=None):
    """coords (N,3) int distinct voxels -> (N, Cout) float64 unit rows, in input order"""
    if hook is not None or relu is not None or bn_hook is not None:
        return _forward64(coords, sd, conv1_kernel_size, hook, relu or nan_relu, bn_hook)
    return _cached("f64", coords, sd, conv1_kernel_size, lambda: _forward64(coords, sd, conv1_kernel_size, None, nan_relu))


def oracle32(coords, sd, conv1_kernel_size=7):
    """the fp32 oracle's unit rows on the same voxels (oracle.extract_features without its voxelisation), cached like the float64 pass"""
    def run():
        with _memoised_oracle_maps():
            F = fo.resunet_forward(np.asarray(coords, dtype=np.int32), sd, conv1_kernel_size, normalize_feature=True)
        return (F / np.linalg.norm(F, axis=1, keepdims=True)).astype(np.float32)
    return _cached("f32", coords, sd, conv1_kernel_size, run)


def case(coords, sd, conv1_kernel_size=7):
    """-> (float64 reference, e_ref): what a budget test compares against"""
    ref = resunet_forward64(coords, sd, conv1_kernel_size)
    return ref, e_ref(oracle32(coords, sd, conv1_kernel_size), ref)


def conv_inputs(coords, sd, conv1_kernel_size=7):
    """{convolution name: its float64 input rows} of the plain float64 pass"""
    rec = {}

    def hk(name, x, W):
        rec[name] = x
        return x, W
    resunet_forward64(coords, sd, conv1_kernel_size, hook=hk)
    return rec


# ----------------------------------------------------------------------------------------
# the scale sweep
# ----------------------------------------------------------------------------------------
def scale_activations(sd, lam):
    """a copy of `sd` whose every activation behind norm1 is `lam` times as large: norm1's weight and bias times lam (its input, a
    column of ones through conv1, is fixed, so its running mean stays), every other BatchNorm's bias and running mean times lam, the
    final bias times lam.  The network is positively homogeneous in these, so the unit-row output does not change."""
    lam = np.float32(lam)
    out = {}
    for k, v in sd.items():
        v = np.array(v, copy=True)
        if k in ("norm1.bn.weight", "norm1.bn.bias", "final.bias"):
            v = (v * lam).astype(np.float32)
        elif not k.startswith("norm1.bn.") and (k.endswith(".bn.bias") or k.endswith(".bn.running_mean")):
            v = (v * lam).astype(np.float32)
        out[k] = v
    return out


# ----------------------------------------------------------------------------------------
# the fp16x2 split, and its defects, inside the float64 pass
# ----------------------------------------------------------------------------------------
def _planes(v32, flush):
    """fp32 values (already scaled) -> (hi, lo) as float64: hi = fp16(v), lo = fp16(v - hi); past the fp16 range hi = inf, lo = NaN"""
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v32.astype(np.float16)
        lo = (v32 - hi.astype(np.float32)).astype(np.float16)
    hi, lo = hi.astype(F64), lo.astype(F64)
    if flush:
        lo = np.where(np.abs(lo) < F16_MIN_NORMAL, 0.0, lo)
    return hi, lo


def split_scale(W):
    """up_conv's weight scale: the largest |w| lands in [512, 1024)"""
    wmax = float(np.max(np.abs(W)))
    ex = np.frexp(np.float32(wmax))[1] if wmax > 0 and np.isfinite(wmax) else 0
    return 2.0 ** (10 - int(ex))


MODES = ("faithful", "flush_lo", "drop_lo", "drop_cross", "descale2")


def emulate_fp16x2(mode="faithful", layer=None, over_margin=0.0):
    """hook: every convolution the library runs on the split MFMA (cin and cout multiples of 32, i.e. all but conv1, whose input is
    occupancy bits) as the three plane products in float64.
      faithful     split_pair_sp and up_conv as written
      flush_lo     defect: lo planes (either operand) below 2^-14, i.e. subnormal in fp16, are zero - a denormal-flushing conversion or
                   MFMA input
      drop_lo      defect, in `layer` only: the activations' lo plane is gone (lo*Wh missing)
      drop_cross   defect, in `layer` only: hi*Wl missing
      descale2     defect, in `layer` only: the descale is off by a factor two
    over_margin != 0 moves the overflow threshold to 65520 * (1 + over_margin) (values between the two are treated as on the other side):
    the finite-row mask of such a pass tells which rows overflow for certain."""
    assert mode in MODES and (layer is None) == (mode in ("faithful", "flush_lo"))

    def hk(name, x, W):
        if x.shape[1] % 32 or W.shape[-1] % 32:
            return x, W
        here = name == layer
        xs = x.astype(np.float32) * np.float32(16.0)
        if over_margin:
            with np.errstate(invalid="ignore"):
                a = np.abs(xs)
                over = a >= F16_OVER * (1.0 + over_margin)
                xs = np.where(over, np.float32(np.inf), np.where(a >= F16_OVER, np.copysign(np.float32(65504.0), xs), xs)).astype(np.float32)
        hi, lo = _planes(xs, mode == "flush_lo")
        ws = split_scale(W)
        wh, wl = _planes((W.astype(np.float32) * np.float32(ws)).astype(np.float32), mode == "flush_lo")
        d = 1.0 / (ws * 16.0) * (2.0 if here and mode == "descale2" else 1.0)
        with np.errstate(invalid="ignore"):
            if here and mode == "drop_lo":
                return [(hi * d, wh + wl)]
            if here and mode == "drop_cross":
                return [((hi + lo) * d, wh)]
            return [((hi + lo) * d, wh), (hi * d, wl)]
    return hk


def emulated(coords, sd, conv1_kernel_size=7, mode="faithful", layer=None, relu=None, over_margin=0.0):
    return resunet_forward64(coords, sd, conv1_kernel_size, hook=emulate_fp16x2(mode, layer, over_margin), relu=relu or nan_relu)


# ----------------------------------------------------------------------------------------
# the inputs of the precision tests (one definition for the CPU and the GPU side)
# ----------------------------------------------------------------------------------------
def small_cloud():
    """the 4770-voxel cloud of test_backbone_vs_oracle: every level runs the coarse split kernels"""
    from yoho_amd import synth
    return fo.voxelize(synth.surface_cloud(6000, seed=2), 0.025)[1]


def state_dict(lam=1.0):
    from yoho_amd import weights as W
    sd = W.synth_state_dict(W.FCGF_SPEC, 3)
    return sd if lam == 1.0 else scale_activations(sd, lam)


SPEC_2B = dict(channels=(0, 32, 64, 128, 256), tr_channels=(0, 64, 64, 64, 64), conv1_kernel_size=5)


def cloud_2b():
    from yoho_amd import synth
    return fo.voxelize(synth.surface_cloud(2500, seed=4) - 1.7, 0.025)[1]


def state_dict_2b(lam=1.0):
    """ResUNetBN2B channels, conv1 kernel 5 (test_other_model_configs_and_tiny_clouds)"""
    from yoho_amd import weights as W
    sd = W.synth_state_dict(W.fcgf_spec((None, 32, 64, 128, 256), (None, 64, 64, 64, 64), 32, 5), 9)
    return sd if lam == 1.0 else scale_activations(sd, lam)


def state_dict_big_weight():
    """one entry of block2.conv1.kernel times 2^12: the layer's weight scale follows it, and the other weights' lo planes go
    toward the fp16 subnormals"""
    sd = {k: np.array(v, copy=True) for k, v in state_dict().items()}
    sd["block2.conv1.kernel"][13, 5, 7] *= np.float32(4096.0)
    return sd
