"""The PartI / PartII forward passes in float64, and the error budget measured against them (helper of tests/test_precision_cpu.py and
tests/test_gpu_precision.py, not a conftest).

`partI_forward64` / `partII_forward64` restate oracle.yoho_oracle.partI_forward / partII_forward with every step in float64: the same
operation sequence, the same clamps (1e-4 under both PartI norms, none under PartII's), the same normalisation, matmul where the
oracle's conv_1xk uses matmul.  Batch norm is applied before the 13-neighbour gather instead of after it (it acts per channel, so the
values are the same and a 13th of the work).  The fp32 oracle stays as it is; it is the thing MEASURED here: `e_ref` is its own
distance from float64, and the budget of a kernel is a fixed multiple of that.

Results are cached per (state dict, input) at module scope, so that the modes of a test share one evaluation.

`hook(name, tensor) -> tensor` lets a test emulate a defect of a kernel inside the float64 pass (tests/test_precision_cpu.py proves
with it that the comparison below rejects subtly wrong results); a pass with a hook is never cached.  PartI calls it on
    a0 / a1 / a2   the activations relu(bn(.)) in front of the 256->512, the 512->256 and the 256->32 conv
    h0, mid, h2, y the outputs of the four convs (h2 after the residual)
PartII on a_in, h0, a0, mid, a1, h2, t1, t2, q accordingly (t1 / t2: the activated 1x1 layers, q: the raw quaternion), and on three
tensors that are no stages (they are not among the returned stage tensors): x_in, the gathered input in front of the first BatchNorm,
and f1 / f2, the outputs of the 1x1 layers in front of theirs.  With these every BatchNorm of both networks has its input passed to
the hook before its statistics are read from the state dict: a hook may write them there (tests/trained_like.py calibrates so).
"""
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle"))
import yoho_oracle as orc  # noqa: E402

G, NTAP = orc.G, orc.NTAP
F64 = np.float64
CHUNK = 64                    # keypoints per matmul: bounds the gathered (chunk, 512, 60, 13) tensor to 200 MB
# The header's per-product bound of the 2-way fp16 split (3 * 2^-22, include/yoho_hip.h at yoho_set_gconv_mode) over fp32's unit
# roundoff 2^-24.  A kernel documented as fp32-accurate may be this many times as far from float64 as the fp32 oracle itself is.
FACTOR = (3.0 * 2.0 ** -22) / 2.0 ** -24
assert FACTOR == 12.0


# ----------------------------------------------------------------------------------------
# the comparison (the suite's own two measures, tests/test_gpu_kernels.py)
# ----------------------------------------------------------------------------------------
def rel(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))) / max(np.max(np.abs(b)), 1e-30))


def rel_rows(a, b):
    """the worst ROW: every keypoint's (match's) error against that row's own magnitude"""
    a, b = np.asarray(a, np.float64).reshape(len(a), -1), np.asarray(b, np.float64).reshape(len(b), -1)
    return float(np.max(np.max(np.abs(a - b), axis=1) / np.maximum(np.max(np.abs(b), axis=1), 1e-30)))


def errors(got, ref):
    """(rel, rel_rows) of every output of `got` against the float64 outputs `ref` (tuples of arrays, or one array), flattened"""
    if isinstance(got, np.ndarray):
        got, ref = (got,), (ref,)
    assert len(got) == len(ref)
    out = []
    for a, b in zip(got, ref):
        assert np.asarray(a).shape == np.asarray(b).shape and np.asarray(b).dtype == F64
        out += [rel(a, b), rel_rows(a, b)]
    return out


def e_ref(oracle_out, ref):
    """the reference's own rounding: the larger of rel and rel_rows of the fp32 oracle's outputs against float64"""
    return max(errors(oracle_out, ref))


def within_budget(got, ref, eref, factor=FACTOR):
    """THE acceptance test of the precision suite: every output of `got` is finite and within factor * e_ref of float64, in rel and
    in rel_rows.  Returns (ok, worst error as a multiple of e_ref)."""
    arrs = (got,) if isinstance(got, np.ndarray) else got
    if not all(np.isfinite(np.asarray(a)).all() for a in arrs):
        return False, float("inf")
    worst = max(errors(got, ref)) / eref
    return bool(worst < factor), worst


# ----------------------------------------------------------------------------------------
# float64 building blocks
# ----------------------------------------------------------------------------------------
def _bn_relu(x, sd, prefix):
    """relu(BatchNorm2d eval) on (B,C,60) in float64, the expression of oracle.bn_eval"""
    g, b = sd[prefix + ".weight"].astype(F64), sd[prefix + ".bias"].astype(F64)
    m, v = sd[prefix + ".running_mean"].astype(F64), sd[prefix + ".running_var"].astype(F64)
    inv = 1.0 / np.sqrt(v + F64(orc.BN_EPS))
    return np.maximum((x - m[None, :, None]) * inv[None, :, None] * g[None, :, None] + b[None, :, None], 0.0)


def _conv(x, w, b, N):
    """gather + Conv2d(Cin,Cout,(1,13)) on (B,Cin,60) -> (B,Cout,60), float64 matmul over (c, tap) as oracle.conv_1xk"""
    B, C, _ = x.shape
    O = w.shape[0]
    wt = np.ascontiguousarray(w.astype(F64).reshape(O, C * NTAP).T)
    bias = b.astype(F64)[None, :]
    Nf = N.reshape(-1)
    out = np.empty((B, O, G), F64)
    for s in range(0, B, CHUNK):
        xs = x[s:s + CHUNK]
        xg = xs[:, :, Nf].reshape(len(xs), C, G, NTAP)
        a = np.ascontiguousarray(xg.transpose(0, 2, 1, 3)).reshape(len(xs) * G, C * NTAP)
        out[s:s + CHUNK] = (a @ wt + bias).reshape(len(xs), G, O).transpose(0, 2, 1)
    return out


def _fc(v, sd, prefix):
    """the 1x1 conv of PartII's head at group element 0 only: (B,C) -> (B,O)"""
    return v @ sd[prefix + ".weight"][:, :, 0, 0].astype(F64).T + sd[prefix + ".bias"].astype(F64)[None, :]


def _bn_relu_vec(v, sd, prefix):
    return _bn_relu(v[:, :, None], sd, prefix)[:, :, 0]


_CACHE = {}


def _digest(sd, arrays):
    h = hashlib.blake2b(digest_size=16)
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k]).tobytes())
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype, a.shape)).encode())
        h.update(a.tobytes())
    return h.digest()


def _cached(kind, sd, arrays, hook, fn):
    if hook is not None:
        return fn(hook)
    key = (kind, _digest(sd, arrays))
    if key not in _CACHE:
        res = fn(lambda name, t: t)
        for a in list(res[:-1]) + list(res[-1].values()):
            a.setflags(write=False)                   # shared among tests: nobody changes it
        _CACHE[key] = res
    return _CACHE[key]


# ----------------------------------------------------------------------------------------
# PartI
# ----------------------------------------------------------------------------------------
def partI_forward64(x, sd, N, stages=False, hook=None):
    """x (B,32,60) -> eqv (B,32,60), inv (B,32) in float64 [, dict of the stage tensors h0, a0, mid, a1, h2, a2, y]"""
    def run(hk):
        p = "PartI_net."
        r = p + "SO3_Conv_layers.0."
        x64 = np.asarray(x, np.float32).astype(F64)
        h0 = hk("h0", _conv(x64, sd[p + "Conv_in.0.weight"], sd[p + "Conv_in.0.bias"], N))
        a0 = hk("a0", _bn_relu(h0, sd, r + "comb_layer_in.0"))
        mid = hk("mid", _conv(a0, sd[r + "comb_layer_in.2.weight"], sd[r + "comb_layer_in.2.bias"], N))
        a1 = hk("a1", _bn_relu(mid, sd, r + "comb_layer_out.0"))
        h2 = hk("h2", _conv(a1, sd[r + "comb_layer_out.2.weight"], sd[r + "comb_layer_out.2.bias"], N) + h0)
        a2 = hk("a2", _bn_relu(h2, sd, p + "Conv_out.comb_layer.0"))
        y = hk("y", _conv(a2, sd[p + "Conv_out.comb_layer.2.weight"], sd[p + "Conv_out.comb_layer.2.bias"], N))
        eqv = y + x64
        inv = np.mean(eqv, axis=-1)
        n_e = np.maximum(np.sqrt(np.sum(eqv * eqv, axis=1, keepdims=True)), 1e-4)
        n_i = np.maximum(np.sqrt(np.sum(inv * inv, axis=1, keepdims=True)), 1e-4)
        return eqv / n_e, inv / n_i, dict(h0=h0, a0=a0, mid=mid, a1=a1, h2=h2, a2=a2, y=y)
    eqv, inv, st = _cached("partI", sd, [x, N], hook, run)
    return (eqv, inv, st) if stages else (eqv, inv)


# ----------------------------------------------------------------------------------------
# PartII
# ----------------------------------------------------------------------------------------
def partII_forward64(bf0, bf1, af0, af1, pre_idx, sd, N, P, stages=False, hook=None):
    """-> q (B,4) in float64 [, dict of the stage tensors a_in, h0, a0, mid, a1, h2, t1, t2, q]; inputs are not modified"""
    def run(hk):
        B = bf0.shape[0]
        perm = P[np.asarray(pre_idx).astype(np.int64)]
        bi = np.arange(B)[:, None, None]
        fi = np.arange(bf0.shape[1])[None, :, None]
        xin = np.concatenate([bf0[bi, fi, perm[:, None, :]], bf1, af0[bi, fi, perm[:, None, :]], af1], axis=1)
        x64 = hk("x_in", np.asarray(xin, np.float32).astype(F64))
        r = "PartII_SO3_Conv_layers.0."
        a_in = hk("a_in", _bn_relu(x64, sd, "Conv_init.comb_layer.0"))
        h0 = hk("h0", _conv(a_in, sd["Conv_init.comb_layer.2.weight"], sd["Conv_init.comb_layer.2.bias"], N))
        a0 = hk("a0", _bn_relu(h0, sd, r + "comb_layer_in.0"))
        mid = hk("mid", _conv(a0, sd[r + "comb_layer_in.2.weight"], sd[r + "comb_layer_in.2.bias"], N))
        a1 = hk("a1", _bn_relu(mid, sd, r + "comb_layer_out.0"))
        h2 = hk("h2", _conv(a1, sd[r + "comb_layer_out.2.weight"], sd[r + "comb_layer_out.2.bias"], N) + h0)
        # the head keeps [:, :, 0, 0] of 1x1 layers: only group element 0 is ever read
        t1 = hk("t1", _bn_relu_vec(hk("f1", _fc(h2[:, :, 0], sd, "PartII_To_R_FC.0")), sd, "PartII_To_R_FC.1"))
        t2 = hk("t2", _bn_relu_vec(hk("f2", _fc(t1, sd, "PartII_To_R_FC.3")), sd, "PartII_To_R_FC.4"))
        q = hk("q", _fc(t2, sd, "PartII_To_R_FC.6"))
        return q / np.sqrt(np.sum(q * q, axis=1))[:, None], dict(a_in=a_in, h0=h0, a0=a0, mid=mid, a1=a1, h2=h2, t1=t1, t2=t2, q=q)
    qn, st = _cached("partII", sd, [bf0, bf1, af0, af1, np.asarray(pre_idx), N, P], hook, run)
    return (qn, st) if stages else qn


# ----------------------------------------------------------------------------------------
# the fp32 oracle on the same inputs, and the budget it sets
# ----------------------------------------------------------------------------------------
def oracle_partI(x, sd, N):
    """oracle.partI_forward, CHUNK keypoints at a time (what oracle.partI_extract does for eqv; the gathered tensor of a whole 257-row
    batch is 400 MB), cached like the float64 pass"""
    def run(_):
        parts = [orc.partI_forward(x[s:s + CHUNK], sd, N) for s in range(0, len(x), CHUNK)]
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), {}
    return _cached("oracle partI", sd, [x, N], None, run)[:2]


def oracle_partII(bf0, bf1, af0, af1, pre_idx, sd, N, P):
    def run(_):
        pre = np.asarray(pre_idx)
        return np.concatenate([orc.partII_forward(bf0[s:s + CHUNK], bf1[s:s + CHUNK], af0[s:s + CHUNK], af1[s:s + CHUNK], pre[s:s + CHUNK], sd, N, P)
                               for s in range(0, len(pre), CHUNK)]), {}
    return _cached("oracle partII", sd, [bf0, bf1, af0, af1, np.asarray(pre_idx), N, P], None, run)[0]


def partI_case(x, sd, N):
    """-> ((eqv64, inv64), e_ref, stages) of one input: everything a budget test compares against"""
    eqv, inv, st = partI_forward64(x, sd, N, stages=True)
    return (eqv, inv), e_ref(oracle_partI(x, sd, N), (eqv, inv)), st


def partII_case(bf0, bf1, af0, af1, pre_idx, sd, N, P):
    """-> (q64, e_ref, stages)"""
    q, st = partII_forward64(bf0, bf1, af0, af1, pre_idx, sd, N, P, stages=True)
    return q, e_ref(oracle_partII(bf0, bf1, af0, af1, pre_idx, sd, N, P), q), st


def spike(arrays, row, factor):
    """copies of the fp32 inputs with one row multiplied by `factor`"""
    out = []
    for a in arrays:
        a = np.array(a, dtype=np.float32, copy=True)
        a[row] *= np.float32(factor)
        out.append(a)
    return out


def partI_case_spiked(x, sd, N, row, factor):
    """partI_case of spike(x): both passes treat every keypoint on its own, so the base batch is evaluated once (cached) and only the
    spiked row anew.  -> (x spiked, (eqv64, inv64), e_ref, stages of the spiked row alone)"""
    (xs,) = spike([x], row, factor)
    ref, o32 = [a.copy() for a in partI_forward64(x, sd, N)], [a.copy() for a in oracle_partI(x, sd, N)]
    r1, _, st = partI_case(xs[row:row + 1], sd, N)
    o1 = oracle_partI(xs[row:row + 1], sd, N)
    for full, one in zip(ref + o32, list(r1) + list(o1)):
        full[row] = one[0]
    return xs, tuple(ref), e_ref(tuple(o32), tuple(ref)), st


def partII_case_spiked(feats, pre_idx, sd, N, P, row, factor):
    """the same for PartII: all four feature rows of match `row` multiplied by `factor`"""
    fs = spike(feats, row, factor)
    pre = np.asarray(pre_idx)
    ref, o32 = partII_forward64(*feats, pre, sd, N, P).copy(), oracle_partII(*feats, pre, sd, N, P).copy()
    one = [f[row:row + 1] for f in fs]
    r1, _, st = partII_case(*one, pre[row:row + 1], sd, N, P)
    ref[row], o32[row] = r1[0], oracle_partII(*one, pre[row:row + 1], sd, N, P)[0]
    return fs, ref, e_ref(o32, ref), st


# ----------------------------------------------------------------------------------------
# defects of a kernel, emulated in the float64 pass
# ----------------------------------------------------------------------------------------
def fp16_low_plane(t):
    """what the second plane of the 2-way fp16 split carries: t - fp16(t) (the planes hold a power-of-two multiple of t, which
    changes nothing away from the ends of the exponent range)"""
    return t - t.astype(np.float16).astype(F64)


def drop_low_plane(stage):
    """one of the three split products gone from a whole layer: the operand `stage` reaches its GEMM as its fp16 high plane alone"""
    return lambda name, t: t - fp16_low_plane(t) if name == stage else t


def drop_low_plane_trivial_irrep(stage):
    """the same on the trivial irrep only, whose coefficient is the group mean (times sqrt(60)): a plane offset off by one irrep"""
    return lambda name, t: t - np.mean(fp16_low_plane(t), axis=-1, keepdims=True) if name == stage else t


def scale_row(stage, row, factor):
    """one keypoint (match) of `stage` off by a relative `factor - 1`"""
    def hk(name, t):
        if name == stage:
            t = t.copy()
            t[row] *= factor
        return t
    return hk


# ----------------------------------------------------------------------------------------
# what the range tests need
# ----------------------------------------------------------------------------------------
ACT_LIMIT, COEF_LIMIT = 4094.0, 16376.0          # include/yoho_hip.h at yoho_range_status


def stage_extent(st, rows=slice(None)):
    """(largest |activation|, bound on the largest |Fourier coefficient|) over the stage tensors of `rows`.  The library's transform is
    unitary (csrc/gft16.hip: F = sqrt(d / 60) rho, the trivial coefficient is sqrt(60) * mean), so no coefficient of a channel exceeds
    the channel's l2 norm over the 60 group elements."""
    amax = cmax = 0.0
    for t in st.values():
        t = t[rows]
        amax = max(amax, float(np.max(np.abs(t))))
        if t.ndim == 3:
            cmax = max(cmax, float(np.max(np.sqrt(np.sum(t * t, axis=-1)))))
    return amax, cmax


def stage_floor(st, row):
    """the smallest of the per-stage maxima of one row: 'every stage of that keypoint exceeds ...'"""
    return min(float(np.max(np.abs(t[row]))) for t in st.values())


# ----------------------------------------------------------------------------------------
# the inputs of the precision tests (one definition for the CPU and the GPU side)
# ----------------------------------------------------------------------------------------
PARTI_B = (1, 31, 33, 255, 257)           # ragged 32-keypoint tile, a full and a just-overfull 256-column tile, kppad 256 / 512
PARTII_M = (1, 17, 40, 257)
SPIKE, MILD = 1e5, 1e2                    # one row times SPIKE leaves the fp16 planes at every stage; times MILD stays 2x inside them
PARTI_SPIKE_B = (257, 300)
PARTII_SPIKE_M = 257


def spike_rows(n):
    return sorted({r for r in (0, 31, 32, 127, 128, 255, 256, n - 1) if r < n})


def partI_input(B):
    from yoho_amd import synth
    return synth.unit_features(B, seed=100 + B)


def partII_input(M):
    """-> ([bf0, bf1, af0, af1], pre_idx): unit features and random coarse rotation indices"""
    from yoho_amd import synth
    feats = [synth.unit_features(M, seed=7000 + 10 * M + i) for i in range(4)]
    return feats, np.random.RandomState(500 + M).randint(0, G, size=M).astype(np.int64)


def partI_state_dict(name):
    """'seed7' (the suite's), two other seeds (nothing but 7 had ever gone through the weight packers), and seed 7 with every conv
    bias times 30 (+-3): the sqrt(60) * bias term of the d = 1 epilogue then dominates the trivial irrep"""
    from yoho_amd import weights as W
    if name == "bias30":
        sd = {k: v.copy() for k, v in W.synth_state_dict(W.PARTI_SPEC, 7).items()}
        for k in sd:
            if k.endswith(".bias") and sd[k[:-5] + ".weight"].ndim == 4:
                sd[k] = (sd[k] * np.float32(30.0)).astype(np.float32)
        return sd
    return W.synth_state_dict(W.PARTI_SPEC, {"seed7": 7, "seed11": 11, "seed23": 23}[name])


# ----------------------------------------------------------------------------------------
# one stage, one channel outside the fp16 planes: rescaled networks and the plan of a case (tests/test_gpu_range_stages.py)
# ----------------------------------------------------------------------------------------
# A power of two s moved between a layer and its consumer multiplies ONE channel of ONE stage by s and leaves every other value of the
# network as it was, exactly (in float64 and in fp32 alike: a power of two commutes with every rounding away from the ends of the
# exponent range).  kind 'conv': row o of the producing conv (weight and bias) times s, undone in the following BN (running_mean times
# s, gamma over s; running_var stays, eps would break exactness) or, for PartII's h2, in column o of the FC head.  y has no consumer:
# the output is normalised.  h2 carries the unscaled residual h0, so there the stage is not an exact multiple and the rescaled network
# is a network of its own.  kind 'act': gamma and beta of the BN times s, input column o of the next conv over s.
_P1, _R1, _R2 = "PartI_net.", "PartI_net.SO3_Conv_layers.0.", "PartII_SO3_Conv_layers.0."
RESCALE = {
    "partI": {
        "a0": ("act", _R1 + "comb_layer_in.0", _R1 + "comb_layer_in.2"),
        "mid": ("conv", _R1 + "comb_layer_in.2", _R1 + "comb_layer_out.0"),
        "a1": ("act", _R1 + "comb_layer_out.0", _R1 + "comb_layer_out.2"),
        "h2": ("conv", _R1 + "comb_layer_out.2", _P1 + "Conv_out.comb_layer.0"),
        "a2": ("act", _P1 + "Conv_out.comb_layer.0", _P1 + "Conv_out.comb_layer.2"),
        "y": ("conv", _P1 + "Conv_out.comb_layer.2", None),
    },
    "partII": {
        "a_in": ("act", "Conv_init.comb_layer.0", "Conv_init.comb_layer.2"),
        "a0": ("act", _R2 + "comb_layer_in.0", _R2 + "comb_layer_in.2"),
        "mid": ("conv", _R2 + "comb_layer_in.2", _R2 + "comb_layer_out.0"),
        "a1": ("act", _R2 + "comb_layer_out.0", _R2 + "comb_layer_out.2"),
        "h2": ("conv", _R2 + "comb_layer_out.2", "PartII_To_R_FC.0"),
    },
}
STAGE_COUT = {"partI": dict(a0=256, mid=512, a1=512, h2=256, a2=256, y=32), "partII": dict(a_in=128, a0=256, mid=512, a1=512, h2=256)}
TWIN = 2.0                    # row factor of the mild twin of a case (the spiked row of a case is the row times MILD)


def stage_kind(net, stage):
    return RESCALE[net][stage][0]


def rescale_stage(sd, net, stage, o, s):
    """a COPY of the state dict in which channel `o` of `stage` is multiplied by the power of two `s` and nothing else changes"""
    m, e = np.frexp(float(s))
    assert m == 0.5 and s >= 1, "s must be a power of two"
    kind, prod, cons = RESCALE[net][stage]
    out = {k: np.array(v, copy=True) for k, v in sd.items()}
    f = np.float32(s)
    if kind == "conv":
        out[prod + ".weight"][o] *= f
        out[prod + ".bias"][o] *= f
        if cons is None:
            pass
        elif cons + ".running_mean" in out:
            out[cons + ".running_mean"][o] *= f
            out[cons + ".weight"][o] /= f
        else:
            out[cons + ".weight"][:, o] /= f
    else:
        out[prod + ".weight"][o] *= f
        out[prod + ".bias"][o] *= f
        out[cons + ".weight"][:, o] /= f
    return out


def rescaled_stages(net, st, sd_r, stage, o, s, N):
    """the float64 stage tensors of the rescaled network, from those of the base network `st` (same rows): channel o of `stage` times
    s, everything else shared - except behind h2, whose tail (PartI: a2, y; PartII: t1, t2, q) is evaluated anew under `sd_r`"""
    out = dict(st)
    t = st[stage].copy()
    if stage != "h2":
        t[:, o] *= s
        out[stage] = t
        return out
    t[:, o] = s * (st["h2"][:, o] - st["h0"][:, o]) + st["h0"][:, o]
    out["h2"] = t
    if net == "partI":
        out["a2"] = _bn_relu(t, sd_r, _P1 + "Conv_out.comb_layer.0")
        out["y"] = _conv(out["a2"], sd_r[_P1 + "Conv_out.comb_layer.2.weight"], sd_r[_P1 + "Conv_out.comb_layer.2.bias"], N)
    else:
        out["t1"] = _bn_relu_vec(_fc(t[:, :, 0], sd_r, "PartII_To_R_FC.0"), sd_r, "PartII_To_R_FC.1")
        out["t2"] = _bn_relu_vec(_fc(out["t1"], sd_r, "PartII_To_R_FC.3"), sd_r, "PartII_To_R_FC.4")
        out["q"] = _fc(out["t2"], sd_r, "PartII_To_R_FC.6")
    return out


def coef_floor(t):
    """a LOWER bound on the largest |Fourier coefficient| of channels t (..., 60): the trivial coefficient is sqrt(60) * mean, and the
    60 coefficients of a unitary transform cannot all lie under l2 / sqrt(60)"""
    return float(np.max(np.maximum(np.sqrt(60.0) * np.abs(np.mean(t, axis=-1)), np.sqrt(np.sum(t * t, axis=-1) / 60.0))))


def channel_outside(kind, t):
    """how far OUTSIDE its plane the channel t (rows, 60) provably is (> 1: outside): activations by their largest value, conv outputs
    by the lower bound on their largest coefficient"""
    return float(np.max(np.abs(t))) / ACT_LIMIT if kind == "act" else coef_floor(t) / COEF_LIMIT


def channel_inside(kind, t):
    """how far INSIDE (> 1: inside): the l2 bound on the coefficients, and for activations the largest value as well (an activation
    goes into a plane itself, and so do its coefficients)"""
    c = COEF_LIMIT / max(float(np.max(np.sqrt(np.sum(t * t, axis=-1)))), 1e-300)
    return min(c, ACT_LIMIT / max(float(np.max(np.abs(t))), 1e-300)) if kind == "act" else c


def _scaled_channel(stage, st, o, s):
    if stage == "h2":
        return s * (st["h2"][:, o] - st["h0"][:, o]) + st["h0"][:, o]
    return s * st[stage][:, o]


def plan_stage_scale(net, stage, o, st_base, st_row, st_twin):
    """the planner: from the float64 stages of the BASE network for the base batch, the spiked row and its mild twin -> the smallest
    power of two s that puts channel o of `stage` a factor 2 outside its plane for the spiked row, or None where no such s leaves
    the channel a factor 2 inside for every base row and for the twin (a dead ReLU channel, a channel whose bounds are too loose)"""
    kind = stage_kind(net, stage)
    for e in range(0, 24):
        s = float(2 ** e)
        if channel_outside(kind, _scaled_channel(stage, st_row, o, s)) >= 2.0:
            ok = min(channel_inside(kind, _scaled_channel(stage, st_base, o, s)), channel_inside(kind, _scaled_channel(stage, st_twin, o, s))) >= 2.0
            return s if ok else None
    return None


def stage_margins(net, stage, o, str_base, str_row, str_twin):
    """the margins of a case from the float64 stages of the RESCALED network (rescaled_stages): 'out' - the spiked row's channel
    outside; 'base' / 'twin' - the same channel of the base rows / the twin inside; 'rest' - every other stage and channel of every
    row (base, spiked, twin) inside, by stage_extent.  A case is admissible iff all four are >= 2."""
    kind = stage_kind(net, stage)

    def rest(st):
        t = st[stage].copy()
        t[:, o] = 0.0
        a, c = stage_extent(dict(st, **{stage: t}))
        return min(ACT_LIMIT / a, COEF_LIMIT / c)
    return dict(out=channel_outside(kind, str_row[stage][:, o]), base=channel_inside(kind, str_base[stage][:, o]),
                twin=channel_inside(kind, str_twin[stage][:, o]), rest=min(rest(str_base), rest(str_row), rest(str_twin)))


# the cases of tests/test_gpu_range_stages.py (tests/test_precision_cpu.py plans every one of them without a device).  Channels: every
# slot of the 16 x 16 and of the 32 x 32 accumulator mapping - register o % 4, lane half o % 8 >= 4, second eight o % 16 >= 8, the next
# 16-row block, either side of a wave's 128 rows and of a 256-row tile, the last channel.
CHANNELS_ALL = (0, 3, 4, 7, 8, 15, 16, 127, 128, 255, -1)
CHANNELS_FEW = (0, 7, 8, -1)
# a prescribed channel the planner refuses (a dead ReLU channel, bounds too far apart), replaced by the next admissible one of its
# residue class mod 16 (the same register, lane half and eight): {(network, stage, B, row, prescribed): chosen}
CHANNEL_SUBST = {("partI", "h2", 33, 16, 4): 20}            # h2 channel 4: its bounds are too far apart for any power of two
SWEEP_CHANNEL = 8                          # the channel of the keypoint sweeps
SWEEP_ROWS = {33: (0, 15, 16, 31, 32), 257: (127, 128, 255, 256)}       # both 16-column tiles of a slab tile | wave halves, ragged tile


def _chan(net, stage, B, row, o):
    o = STAGE_COUT[net][stage] - 1 if o < 0 else o
    return CHANNEL_SUBST.get((net, stage, B, row, o), o)


def range_stage_cases():
    """-> [(network, mode, stage, channel, B, row)], every case once"""
    cases = []

    def add(net, mode, stage, chans, B, row):
        for o in chans:
            c = (net, mode, stage, _chan(net, stage, B, row, o), B, row)
            if c not in cases:
                cases.append(c)
    for stage in ("a0", "mid", "a1", "h2", "a2", "y"):
        add("partI", "fgemm", stage, CHANNELS_ALL if stage in ("mid", "h2") else CHANNELS_FEW, 33, 16)
    for stage in ("mid", "h2"):
        for B, rows in SWEEP_ROWS.items():
            for row in rows:
                add("partI", "fgemm", stage, (SWEEP_CHANNEL,), B, row)
    for mode in ("fgemm256", "fgemm128"):
        for stage in ("a0", "mid", "a1", "h2", "a2", "y"):
            add("partI", mode, stage, CHANNELS_FEW, 33, 16)
    for stage in ("a0", "a1", "a2"):
        add("partI", "fp16x2", stage, CHANNELS_FEW, 33, 16)
    for stage in ("mid", "h2"):
        add("partI", "fgemm8", stage, CHANNELS_FEW, 33, 16)
    for mode in ("fp16x2", "cgemm"):
        for stage in ("a_in", "a0", "mid", "a1", "h2"):
            add("partII", mode, stage, CHANNELS_FEW, 33, 16)
            add("partII", mode, stage, (SWEEP_CHANNEL,), 257, 128)
    return cases


def range_stage_plan(net, stage, o, B, row, sd, N, P=None):
    """everything of a case that does not depend on the mode, from float64 alone (cached base passes; one-row passes for the spiked
    row and the twin): dict(s, sd (rescaled), x / feats + pre (base inputs), margins, st (base, spiked, twin stages of the rescaled
    network)), or None where the planner refuses the channel"""
    if net == "partI":
        x = partI_input(B)
        st_b = partI_forward64(x, sd, N, stages=True)[2]
        one = lambda f: partI_forward64(spike([x], row, f)[0][row:row + 1], sd, N, stages=True)[2]
        inputs = dict(x=x)
    else:
        feats, pre = partII_input(B)
        st_b = partII_forward64(*feats, pre, sd, N, P, stages=True)[1]
        one = lambda f: partII_forward64(*[a[row:row + 1] for a in spike(feats, row, f)], pre[row:row + 1], sd, N, P, stages=True)[1]
        inputs = dict(feats=feats, pre=pre)
    st_r, st_t = one(MILD), one(TWIN)
    s = plan_stage_scale(net, stage, o, st_b, st_r, st_t)
    if s is None:
        return None
    sd_r = rescale_stage(sd, net, stage, o, s)
    st = tuple(rescaled_stages(net, t, sd_r, stage, o, s, N) for t in (st_b, st_r, st_t))
    return dict(inputs, s=s, sd=sd_r, margins=stage_margins(net, stage, o, *st), st=st)
