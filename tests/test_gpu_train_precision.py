"""The training kernels per element against a float64 autograd pass (-m gpu): yoho_gconv_layer (forward and transposed),
yoho_gconv_wgrad, yoho_bn_stats / _bn_relu_apply(_sub) / _bn_relu_backward, and the two trainable stacks of train/network.py.

tests/test_gpu_train.py compares them with torch's fp32 kernels in one max-norm per tensor and the whole step in a 19-number digest per
gradient; tests/test_train_precision_cpu.py shows what that lets through.  Here every random case must stay within
train_ref64.TRAIN_FACTOR x e_ref of tests/train_ref64.py's float64 pass, in rel over the array and over the worst row, where e_ref is
the same restatement's float32 run measured from the float64 one; every case prints its figures as multiples of e_ref
(profiles/precision.md, "Training kernels", keeps one run of them).  Besides the budget, as bits and without a tolerance: one-hot probes
of the tap relabelling, the (o,c) transposition and the channel padding; the bias; row independence across ragged tiles and across the
4096-row split of yoho_gconv_layer; determinism of the weight gradient; poisoned scratch and outputs.

ReLU: the kernel-level BatchNorm inputs are built with no pre-activation within 1e-3 channel-stds of zero (train_ref64.unkink) and the
device mask must then EQUAL float64's; in the stacks the float64 pass adopts the device's masks, and where those differ from float64's
own, |z64| must be under 64 * 2^-24 of the layer's largest, on at most 1e-4 of its elements.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import train_ref64 as TR
from test_gpu_scratch import PATTERNS, outp, same_bits  # noqa: F401  (outp is a fixture)
from yoho_amd import weights as W

pytestmark = pytest.mark.gpu
F32 = torch.float32


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.Context()


@pytest.fixture(scope="module")
def ctx_poisoned(hip):
    """a context that runs nothing but yoho_gconv_layer: that entry's workspace (train.hip, gconv_layer: packed input, raw output,
    packed weights, padded bias - four float buffers from bind_ws; the slot, neighbour and inverse-tap tables live in the context, not
    in the workspace) holds only numbers, so all of it may be poisoned"""
    return hip.Context()


@pytest.fixture(scope="module")
def inv(tables):
    return TR.tap_inverse(tables.N)


# ---- yoho_gconv_layer: the budget -----------------------------------------------------------------------------------------------------
CONV_B = (1, 31, 32, 33, 65)
# (cin, cout, forward, transposed); transposed runs the layer of effective size cout -> cin, so (20, 8) has effective cout 20, padded to 32
CONV_SHAPES = ((8, 8, True, True), (8, 40, True, True), (24, 32, True, True), (32, 256, True, True), (128, 64, True, True),
               (20, 8, False, True), (256, 32, False, True))


@pytest.mark.parametrize("B", CONV_B)
@pytest.mark.parametrize("cin,cout,fwd,tr", CONV_SHAPES)
def test_gconv_layer_budget(ctx, tables, cin, cout, fwd, tr, B):
    x, Wt, b, dy = TR.conv_case(cin, cout, B)
    r64 = TR.gconv_grads(x, Wt, b, tables.N, dy)
    r32 = TR.gconv_grads(x, Wt, b, tables.N, dy, F32)
    if fwd:
        y = host(ctx.gconv_layer(cu(x), cu(Wt), cu(b)))
        ok, worst = TR.check("gconv_layer forward %d->%d B=%d" % (cin, cout, B), y, r64[0], r32[0])
        assert ok, worst
    if tr:
        dx = host(ctx.gconv_layer(cu(dy), cu(Wt), None, transpose=True))
        ok, worst = TR.check("gconv_layer transposed %d->%d B=%d" % (cin, cout, B), dx, r64[1], r32[1])
        assert ok, worst


def test_gconv_layer_across_the_row_split(ctx, tables):
    """B = 4097 with 8 -> 8: yoho_gconv_layer runs 4096 rows and then 1.  Rows 0, 4095, 4096 against float64; every row bit-equal to the
    same row computed in a B = 33 launch"""
    B = 4097
    x, Wt, b, _ = TR.conv_case(8, 8, B)
    xd, wd, bd = cu(x), cu(Wt), cu(b)
    y = ctx.gconv_layer(xd, wd, bd)
    rows = [0, 4095, 4096]
    assert rows[-1] == B - 1
    ref = TR.npy(TR.gconv(TR.T(x[rows]), TR.T(Wt), TR.T(b), tables.N))
    r32 = TR.npy(TR.gconv(TR.T(x[rows], F32), TR.T(Wt, F32), TR.T(b, F32), tables.N))
    ok, worst = TR.check("gconv_layer forward 8->8 B=4097, rows %s" % rows, host(y[rows]), ref, r32)
    assert ok, worst
    for s in range(0, B, 33):
        part = ctx.gconv_layer(xd[s:s + 33].contiguous(), wd, bd)
        bad = (part != y[s:s + 33]).reshape(len(part), -1).any(1).nonzero().flatten().tolist()
        assert not bad, (s, bad[:8])
    assert torch.isfinite(y).all()


# ---- yoho_gconv_layer: exact probes ---------------------------------------------------------------------------------------------------
def _corners(B, C, k):
    """probe k of 13: (b, c, g) cycling through the first and last row of the ragged tile pair, the first and last channel of the first
    and last 8-channel chunk, and g = 0 / 59"""
    bs, cs, gs = (0, 31, 32, B - 1), (0, 7, C - 8, C - 1), (0, 59, 17)
    return bs[k % 4], cs[(k // 2) % 4], gs[k % 3]


def test_gconv_layer_one_hot_probes_forward(ctx, tables):
    """x = one-hot at (b, c, g), bias 0: row b of the output is W[:, c, k] at the g' with N[g', k] == g for each tap k and +0 everywhere
    else, as bits (cout = 40: two output blocks, the second padded)"""
    B, cin, cout = 33, 16, 40
    _, Wt, _, _ = TR.conv_case(cin, cout, 1, seed=9)
    N = tables.N.astype(np.int64)
    wd, zero = cu(Wt), torch.zeros(cout, device="cuda")
    for k in range(TR.NTAP):
        b, c, g = _corners(B, cin, k)
        x = np.zeros((B, cin, 60), np.float32)
        x[b, c, g] = 1.0
        want = np.zeros((B, cout, 60), np.float32)
        for t in range(TR.NTAP):
            (gp,) = np.nonzero(N[:, t] == g)
            assert len(gp) == 1
            want[b, :, gp[0]] = Wt[:, c, 0, t]
        got = host(ctx.gconv_layer(cu(x), wd, zero))
        assert got.tobytes() == want.tobytes(), (k, b, c, g, np.argwhere(got != want)[:4])


def test_gconv_layer_one_hot_probes_transposed(ctx, tables, inv):
    """dy = one-hot at (b, o, g): row b of the input gradient is W[o, :, inv[k]] at the g' with N[g', k] == g (cin = 20: effective
    cout 20, padded to 32)"""
    B, cin, cout = 33, 20, 16
    _, Wt, _, _ = TR.conv_case(cin, cout, 1, seed=10)
    N = tables.N.astype(np.int64)
    wd = cu(Wt)
    for k in range(TR.NTAP):
        b, o, g = _corners(B, cout, k)
        dy = np.zeros((B, cout, 60), np.float32)
        dy[b, o, g] = 1.0
        want = np.zeros((B, cin, 60), np.float32)
        for t in range(TR.NTAP):
            (gp,) = np.nonzero(N[:, t] == g)
            want[b, :, gp[0]] = Wt[o, :, 0, inv[t]]
        got = host(ctx.gconv_layer(cu(dy), wd, None, transpose=True))
        assert got.tobytes() == want.tobytes(), (k, b, o, g, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("cin,cout", ((8, 8), (16, 40), (32, 256)))
def test_gconv_layer_bias_alone(ctx, cin, cout):
    """W = 0: every output equals its channel's bias exactly, the channels of a padded output block (cout = 40, 8) included"""
    B = 33
    x, Wt, b, _ = TR.conv_case(cin, cout, B, seed=2)
    y = host(ctx.gconv_layer(cu(x), cu(np.zeros_like(Wt)), cu(b)))
    assert np.array_equal(y, np.broadcast_to(b[None, :, None], y.shape))


@pytest.mark.parametrize("cin,cout,transpose", ((24, 40, False), (20, 8, True)))
def test_gconv_layer_row_bits_do_not_depend_on_the_launch(ctx, cin, cout, transpose):
    """row b of a B = 33 launch equals the B = 1 launch of that row, and rows put in front (1 / 31 / 32: another lane, another tile)
    change nothing behind them"""
    B = 33
    x, Wt, b, dy = TR.conv_case(cin, cout, B, seed=3)
    src, wd, bd = cu(dy if transpose else x), cu(Wt), (None if transpose else cu(b))
    base = ctx.gconv_layer(src, wd, bd, transpose=transpose)
    for r in range(B):
        one = ctx.gconv_layer(src[r:r + 1].contiguous(), wd, bd, transpose=transpose)
        assert torch.equal(one[0], base[r]), r
    other = torch.randn(32, src.shape[1], 60, device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    for n in (1, 31, 32):
        o = ctx.gconv_layer(torch.cat([other[:n], src]), wd, bd, transpose=transpose)
        bad = (o[n:] != base).reshape(B, -1).any(1).nonzero().flatten().tolist()
        assert not bad, (n, bad[:8])


@pytest.mark.parametrize("cin,cout,fwd,tr", CONV_SHAPES)
def test_gconv_layer_on_poisoned_scratch(ctx, ctx_poisoned, outp, cin, cout, fwd, tr):
    """every shape and B once on a clean context, then once per pattern with the whole workspace (numbers only, see ctx_poisoned) and the
    output tensor poisoned: bit-identical"""
    for B in CONV_B:
        x, Wt, b, dy = TR.conv_case(cin, cout, B)
        xd, wd, bd, dyd = cu(x), cu(Wt), cu(b), cu(dy)
        clean = {}
        if fwd:
            clean["y"] = ctx.gconv_layer(xd, wd, bd)
        if tr:
            clean["dx"] = ctx.gconv_layer(dyd, wd, None, transpose=True)
        assert all(torch.isfinite(v).all() for v in clean.values())
        for p in PATTERNS:
            ctx_poisoned.poison_scratch(p)
            outp.pattern = p
            try:
                got = {}
                if fwd:
                    got["y"] = ctx_poisoned.gconv_layer(xd, wd, bd)
                if tr:
                    ctx_poisoned.poison_scratch(p)
                    got["dx"] = ctx_poisoned.gconv_layer(dyd, wd, None, transpose=True)
            finally:
                outp.pattern = None
            same_bits(clean, got, (cin, cout, B, hex(p)))


# ---- yoho_gconv_wgrad -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 2, 33))
@pytest.mark.parametrize("cin,cout", ((32, 32), (64, 32), (32, 96), (256, 32)))
def test_gconv_wgrad_budget_and_determinism(ctx, tables, cin, cout, B):
    x, Wt, b, dy = TR.conv_case(cin, cout, B)
    r64 = TR.gconv_grads(x, Wt, b, tables.N, dy)
    r32 = TR.gconv_grads(x, Wt, b, tables.N, dy, F32)
    xd, dyd = cu(x), cu(dy)
    dW, db = ctx.gconv_wgrad(xd, dyd)
    ok, worst = TR.check("gconv_wgrad dW %d->%d B=%d" % (cin, cout, B), host(dW), r64[2], r32[2])       # row = output channel
    assert ok, worst
    ok, worst = TR.check("gconv_wgrad db %d->%d B=%d" % (cin, cout, B), host(db), r64[3], r32[3])
    assert ok, worst
    dW2, db2 = ctx.gconv_wgrad(xd, dyd)                              # "deterministic sums" (train.hip)
    assert torch.equal(dW, dW2) and torch.equal(db, db2)
    guard = torch.full((cout,), float("nan"), device="cuda")         # a bias gradient that exists but is not asked for
    keep = guard.view(torch.int32).clone()
    dW3, none = ctx.gconv_wgrad(xd, dyd, want_bias=False)
    assert none is None and torch.equal(dW3, dW) and torch.equal(guard.view(torch.int32), keep)


def test_gconv_wgrad_one_hot_probes(ctx, tables):
    """x one-hot at (b, c, g0), dy one-hot at (b, o, g1) with value v: dW[o, c, 0, k] = v where N[g1, k] == g0, db[o] = v, +0 elsewhere"""
    B, cin, cout, v = 3, 64, 96, 0.75
    N = tables.N.astype(np.int64)
    cases = [(0, 0, 0, 0, 0), (B - 1, cin - 1, cout - 1, 59, 12), (1, 31, 32, 17, 5), (2, 32, 31, 59, 7), (0, 63, 64, 0, None)]
    for b, c, o, g1, k in cases:
        g0 = int(N[g1, k]) if k is not None else next(g for g in range(60) if g not in set(N[g1]))
        x, dy = np.zeros((B, cin, 60), np.float32), np.zeros((B, cout, 60), np.float32)
        x[b, c, g0], dy[b, o, g1] = 1.0, v
        wantW, wantb = np.zeros((cout, cin, 1, TR.NTAP), np.float32), np.zeros(cout, np.float32)
        wantW[o, c, 0] = v * (N[g1] == g0)
        wantb[o] = v
        assert int((wantW != 0).sum()) == (1 if k is not None else 0)
        dW, db = ctx.gconv_wgrad(cu(x), cu(dy))
        assert host(dW).tobytes() == wantW.tobytes() and host(db).tobytes() == wantb.tobytes(), (b, c, o, g1, k)


def test_gconv_wgrad_refuses_ragged_channels(ctx, hip):
    """cin = 24: YOHO_EINVAL, and dW is left as it was"""
    x, dy = torch.randn(2, 24, 60, device="cuda"), torch.randn(2, 32, 60, device="cuda")
    dW = torch.full((32, 24, 1, 13), 3.5, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = ctx._lib.yoho_gconv_wgrad(ctx._h, p(x), p(dy), 2, 24, 32, p(dW), None, None)
    torch.cuda.synchronize()
    assert rc == -1 and b"multiples of 32" in ctx._lib.yoho_last_error()
    assert bool((dW == 3.5).all())
    with pytest.raises(hip.YohoError):
        ctx.gconv_wgrad(x, dy)


# ---- BatchNorm + ReLU -----------------------------------------------------------------------------------------------------------------
GROUPS = {"plain": ("ordinary", "constant", "dead"), "r3": ("r3",), "r30": ("r30",), "r300": ("r300",)}
VGROUPS = {"tame": ("ordinary", "constant", "dead", "r3"), "steep": ("r30", "r300")}      # per-channel vectors: comparable scales together


def _sel(kinds, names):
    return np.nonzero(np.isin(kinds, names))[0]


@pytest.mark.parametrize("running", (False, True), ids=("batch", "running"))
@pytest.mark.parametrize("C,B", ((8, 1), (32, 4), (32, 5), (40, 33), (512, 3)))
def test_bn_relu_budget(ctx, C, B, running):
    """GroupBatchNorm (yoho_bn_stats, yoho_bn_relu_apply_sub, yoho_bn_relu_backward under autograd) on a tensor that mixes ordinary
    channels, channels with mean / std of 3, 30 and 300, constant channels (var = 0) and fully dead ones; every kind is compared on its own
    (one e_ref per kind: the r = 300 channels' honest fp32 error is 300 times an ordinary channel's and would hide it).
    The folded yoho_bn_relu_apply keeps its behaviour: it is held to the budget where the mean is small and its multiples are printed
    where it is not (measured with running statistics: 7.5 e_ref at r = 30, 69 at r = 300; profiles/precision.md)."""
    from yoho_amd.train.network import GroupBatchNorm
    c = TR.bn_case(C, B, running)
    kinds = c["kinds"]
    run = (c["rm"], c["rv"]) if running else None
    r64 = TR.bn_relu_grads(c["x"], c["gamma"], c["beta"], c["dy"], run)
    r32 = TR.bn_relu_grads(c["x"], c["gamma"], c["beta"], c["dy"], run, dtype=F32)
    assert TR.kink_count(r64["z"]) == 0
    m = GroupBatchNorm(C, hctx=ctx).cuda()
    with torch.no_grad():
        m.weight.copy_(cu(c["gamma"])); m.bias.copy_(cu(c["beta"]))
        m.running_mean.copy_(cu(c["rm"])); m.running_var.copy_(cu(c["rv"]))
    m.train(not running)
    x = cu(c["x"]).requires_grad_(True)
    y = m(x)
    y.backward(cu(c["dy"]))
    got = dict(y=host(y), dx=host(x.grad), dgamma=host(m.weight.grad), dbeta=host(m.bias.grad))
    tag = "bn C=%d B=%d %s" % (C, B, "running" if running else "batch")
    # the masks first: exclusion cap 0
    assert np.array_equal(got["y"] > 0, r64["z"] > 0), tag
    bad = []
    for g, names in GROUPS.items():
        i = _sel(kinds, names)
        for k in ("y", "dx"):
            ok, worst = TR.check("%s %s %s" % (tag, g, k), got[k][:, i], r64[k][:, i], r32[k][:, i])
            bad += [] if ok else [(g, k, worst)]
    vec = dict(dgamma=(got["dgamma"], r64["dgamma"], r32["dgamma"]), dbeta=(got["dbeta"], r64["dbeta"], r32["dbeta"]))
    if not running:
        mean, var = ctx.bn_stats(cu(c["x"]))
        vec.update(mean=(host(mean), r64["mean"], r32["mean"]), var=(host(var), r64["var"], r32["var"]))
        upd = [TR.running_update(TR.T(c["rm"], dt), TR.T(c["rv"], dt), TR.T(r["mean"], dt), TR.T(r["var"], dt), B)
               for dt, r in ((TR.F64, r64), (F32, r32))]                 # the buffers after one step, in float64 and in float32
        vec.update(running_mean=(host(m.running_mean), TR.npy(upd[0][0]), TR.npy(upd[1][0])),
                   running_var=(host(m.running_var), TR.npy(upd[0][1]), TR.npy(upd[1][1])))
    else:
        assert torch.equal(m.running_mean, cu(c["rm"])) and torch.equal(m.running_var, cu(c["rv"]))
    for g, names in VGROUPS.items():
        i = _sel(kinds, names)
        for k, (a, b64, b32) in vec.items():
            ok, worst = TR.check("%s %s %s" % (tag, g, k), a[i], b64[i], b32[i])
            bad += [] if ok else [(g, k, worst)]
    dead = _sel(kinds, ("dead",))
    assert (got["y"][:, dead] == 0).all() and (got["dx"][:, dead] == 0).all() and (got["dgamma"][dead] == 0).all() and \
        (got["dbeta"][dead] == 0).all(), tag
    # the folded entry, unchanged: scale / shift as its callers form them
    mean_d, var_d = (cu(c["rm"]), cu(c["rv"])) if running else ctx.bn_stats(cu(c["x"]))
    scale = cu(c["gamma"]) * torch.rsqrt(var_d + TR.BN_EPS)
    yf = host(ctx.bn_relu_apply(cu(c["x"]), scale.contiguous(), (cu(c["beta"]) - mean_d * scale).contiguous()))
    for g, names in GROUPS.items():
        i = _sel(kinds, names)
        ok, worst = TR.check("%s %s y, folded yoho_bn_relu_apply" % (tag, g), yf[:, i], r64["y"][:, i], r32["y"][:, i])
        if g in ("plain", "r3"):
            bad += [] if ok else [(g, "folded y", worst)]
    assert not bad, (tag, bad)


# ---- the whole stacks -----------------------------------------------------------------------------------------------------------------
def _device_stack(which, sd, feats, cots):
    from yoho_amd.train import network
    from yoho_amd.train.network import GroupBatchNorm
    cfg = types.SimpleNamespace(SO3_related_files=None)
    if which == "partI":
        net = network.PartI_network(cfg).cuda()
        net.load_state_dict({k[len("PartI_net."):]: torch.from_numpy(np.array(v)) for k, v in sd.items()})
        prefix, run = "PartI_net.", lambda x: (lambda o: (o["eqv"], o["inv"]))(net(x))
    else:
        net = network.PartII_train(cfg).cuda()
        net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=False)      # its PartI_net is not run
        prefix, run = "", lambda x: (net.PartII_SO3_Conv(x),)
    net.train()
    masks, hooks = {}, []
    for name, mod in net.named_modules():
        if isinstance(mod, GroupBatchNorm) and not name.startswith("PartI_net"):
            hooks.append(mod.register_forward_hook(lambda _m, _i, out, key=prefix + name: masks.__setitem__(key, host(out > 0))))
    out = run(cu(feats))
    sum((o * cu(ct)).sum() for o, ct in zip(out, cots)).backward()
    for h in hooks:
        h.remove()
    named = {prefix + k: v for k, v in net.named_parameters() if not k.startswith("PartI_net")}
    grads = {k: host(p.grad) for k, p in named.items() if p.grad is not None}
    buffers = {prefix + k: host(v) for k, v in net.named_buffers() if not k.startswith(("PartI_net", "PartII_To_R_FC")) and k.endswith(("running_mean", "running_var"))}
    return tuple(host(o) for o in out), grads, buffers, masks


@pytest.mark.parametrize("which,B,seed", (("partI", 6, 7), ("partI", 33, 7), ("partI", 6, 11), ("partI", 33, 11), ("partII", 6, 7),
                                          ("partII", 6, 11)))
def test_stack_per_element(tables, which, B, seed):
    """PartI_network / PartII_train.PartII_SO3_Conv in train mode: the outputs, EVERY parameter gradient element by element (row = output
    channel; per-channel vectors as one row; conv bias gradients against the mass of what they sum, train_ref64.shifted_by_mass) and
    every BatchNorm running buffer, for the scalar sum(out * cot) with a fixed random cotangent per output"""
    spec = W.PARTI_SPEC if which == "partI" else W.PARTII_SPEC
    sd = W.synth_state_dict(spec, seed)
    stack = TR.partI_network if which == "partI" else TR.partII_so3_conv
    feats = TR.stack_input(which, B)
    cots = TR.cotangents([(B, 32, 60), (B, 32)] if which == "partI" else [(B, 256, 60)], seed=40 + seed)
    out, grads, buffers, masks = _device_stack(which, sd, feats, cots)
    tag = "%s B=%d seed %d" % (which, B, seed)
    # the masks the device took against float64's own
    with torch.no_grad():
        own = TR.Pass(sd, tables.N)
        stack(own, feats)
    assert set(masks) == set(own.z) and len(masks) == 3
    for name, z in own.z.items():
        n, zrel = TR.mask_differences(masks[name], TR.npy(z))
        print("%s %s: %d of %d mask elements differ from float64's, largest |z| / max|z| among them %.2g" % (tag, name, n, z.numel(), zrel))
        assert zrel < TR.MASK_Z and n <= TR.MASK_SHARE * z.numel(), (name, n, zrel)
    r64 = TR.stack_case(stack, sd, tables.N, feats, cots, masks=masks)
    r32 = TR.stack_case(stack, sd, tables.N, feats, cots, dtype=F32, masks=masks)
    bad = []

    def cmp(what, a, b64, b32):
        ok, worst = TR.check("%s %s" % (tag, what), a, b64, b32)
        if not ok:
            bad.append((what, worst))

    for i, name in enumerate(("eqv", "inv") if which == "partI" else ("out",)):
        cmp(name, out[i], r64["out"][i], r32["out"][i])
    assert set(grads) == set(r64["grads"]) and len(grads) == (14 if which == "partI" else 12)
    for k in sorted(grads):
        if k in r64["mass"]:
            s = r64["mass"][k]
            cmp("grad " + k + " (+ mass)", TR.shifted_by_mass(grads[k], s), TR.shifted_by_mass(r64["grads"][k], s),
                TR.shifted_by_mass(r32["grads"][k], s))
        else:
            cmp("grad " + k, grads[k], r64["grads"][k], r32["grads"][k])
    assert set(buffers) == set(r64["buffers"]) and len(buffers) == 6
    for k in sorted(buffers):
        cmp(k, buffers[k], r64["buffers"][k], r32["buffers"][k])
    assert not bad, (tag, bad)
