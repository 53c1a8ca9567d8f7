"""The training-mode operations of yoho_amd/train/network.py restated in plain torch on the CPU, parameterised by dtype (helper of
tests/test_train_precision_cpu.py and tests/test_gpu_train_precision.py, not a conftest).

Written from the formulas in the header comments of yoho_amd/csrc/train.hip and from train/network.py:

    gconv     y[b,o,g]  = bias[o] + sum_k sum_c W[o,c,k] * x[b,c,N[g,k]]            accumulated tap by tap, nothing gathered to (B,C,60,13)
    bn_relu   y = relu((x - mean) * rstd * gamma + beta), rstd = 1 / sqrt(var + eps)  subtract-first, biased variance over (B, 60)
    running   r <- (1 - m) r + m * stat, var corrected by n / (n - 1) with n = B * 60 * 13, the size of the reference's gathered tensor

Run in float64 this is the reference (gradients: torch autograd in float64); run in float32 it is the thing MEASURED: `e_ref` is the
float32 pass's own distance from the float64 one, and a kernel is held to TRAIN_FACTOR times that.  The comparison itself (rel over
the array, rel over the worst row, row = leading index) is tests/ref64.py's, imported and not restated.

ReLU: with `mask=None` it is z > 0; with a mask it is multiplication by that mask, so that a float64 pass can adopt the masks a device
run took where a pre-activation sits within rounding of zero (what such a mask may differ in is asserted separately by the callers).
"""
import numpy as np
import torch

import ref64 as R
from ref64 import errors, within_budget, rel, rel_rows  # noqa: F401  (one comparison for the whole precision suite)

G, NTAP = R.G, R.NTAP
BN_EPS, MOMENTUM = 1e-5, 0.1
F64, F32 = torch.float64, torch.float32

# What the training kernels are held to, as a multiple of e_ref: twice the worst multiple measured on the device over all random cases of
# tests/test_gpu_train_precision.py, rounded up, never below 2 and never above ref64.FACTOR.  Measured (profiles/precision.md, "Training
# kernels"): 10.41, the 3328-product fp32 MFMA chain of a layer with 256 input channels; BatchNorm and the weight gradient are at 1 to 3.
# Twice that is 21, so the constant is the cap.
TRAIN_FACTOR = 12
assert 2 <= TRAIN_FACTOR <= R.FACTOR


def T(a, dtype=F64, grad=False):
    """an array / tensor as a fresh CPU tensor of `dtype` (values are fp32 inputs: the conversion is exact)"""
    t = torch.as_tensor(np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a)).to(dtype).clone()
    return t.requires_grad_(True) if grad else t


def npy(t):
    return t.detach().cpu().numpy()


# ----------------------------------------------------------------------------------------
# the two operations
# ----------------------------------------------------------------------------------------
def gconv(x, W, b, N):
    """x (B,C,60), W (O,C,1,13) or (O,C,13), b (O) or None, N (60,13) integer table -> (B,O,60); differentiable"""
    W = W.reshape(W.shape[0], W.shape[1], NTAP)
    N = torch.as_tensor(np.asarray(N).astype(np.int64))
    y = None
    for k in range(NTAP):
        t = torch.einsum("oc,bcg->bog", W[:, :, k], x[:, :, N[:, k]])
        y = t if y is None else y + t
    return y if b is None else y + b[None, :, None]


def gconv_grads(x, W, b, N, dy, dtype=F64):
    """-> (y, dx, dW (O,C,1,13), db) as numpy arrays, from autograd in `dtype`"""
    xt, Wt, dyt = T(x, dtype, True), T(W, dtype, True), T(dy, dtype)
    bt = T(b, dtype, True) if b is not None else None
    y = gconv(xt, Wt, bt, N)
    (y * dyt).sum().backward()
    return npy(y), npy(xt.grad), npy(Wt.grad).reshape(W.shape[0], W.shape[1], 1, NTAP), (npy(bt.grad) if bt is not None else None)


def batch_stats(x):
    """per-channel mean and biased variance over (B, 60), two-pass"""
    m = x.mean((0, 2))
    return m, ((x - m[None, :, None]) ** 2).mean((0, 2))


def bn_relu(x, gamma, beta, mean=None, var=None, eps=BN_EPS, mask=None):
    """relu(batch_norm(x)) of a (B,C,60) tensor.  mean / var None: batch statistics (differentiated through); given: running statistics.
    -> (y, z, mean, var): z is the pre-activation, y = z * mask when a mask is given and relu(z) otherwise"""
    if mean is None:
        mean, var = batch_stats(x)
    rstd = 1.0 / torch.sqrt(var + eps)
    z = (x - mean[None, :, None]) * rstd[None, :, None] * gamma[None, :, None] + beta[None, :, None]
    y = torch.relu(z) if mask is None else z * torch.as_tensor(mask).to(z.dtype)
    return y, z, mean, var


def running_update(rm, rv, mean, var, B, momentum=MOMENTUM):
    """GroupBatchNorm's buffer update: the unbiased-variance correction counts the gathered size B * 60 * 13"""
    n = B * G * NTAP
    return (1 - momentum) * rm + momentum * mean.detach(), (1 - momentum) * rv + momentum * var.detach() * (n / (n - 1))


def bn_relu_grads(x, gamma, beta, dy, running=None, dtype=F64, mask=None):
    """-> dict y, z, mean, var, dx, dgamma, dbeta (numpy) of one BatchNorm + ReLU under autograd in `dtype`"""
    xt, gt, bt = T(x, dtype, True), T(gamma, dtype, True), T(beta, dtype, True)
    rm, rv = (T(running[0], dtype), T(running[1], dtype)) if running is not None else (None, None)
    y, z, m, v = bn_relu(xt, gt, bt, rm, rv, mask=mask)
    (y * T(dy, dtype)).sum().backward()
    return dict(y=npy(y), z=npy(z), mean=npy(m), var=npy(v), dx=npy(xt.grad), dgamma=npy(gt.grad), dbeta=npy(bt.grad))


# ----------------------------------------------------------------------------------------
# the modules and the two stacks, on a state dict with the reference's key names
# ----------------------------------------------------------------------------------------
class Pass:
    """one training-mode pass: parameters as leaves of `dtype`, the running buffers it leaves, the pre-activations it saw"""

    def __init__(self, sd, N, dtype=F64, masks=None):
        self.N, self.dtype, self.masks = N, dtype, masks
        self.p = {k: T(v, dtype, grad=not k.endswith(("running_mean", "running_var"))) for k, v in sd.items()
                  if not k.endswith("num_batches_tracked")}
        self.buffers, self.z, self.conv_out = {}, {}, {}

    def conv(self, x, prefix):
        y = gconv(x, self.p[prefix + ".weight"], self.p[prefix + ".bias"], self.N)
        if y.requires_grad:
            y.retain_grad()
            self.conv_out[prefix] = y
        return y

    def bn(self, x, prefix):
        mask = self.masks[prefix] if self.masks is not None else None
        y, z, m, v = bn_relu(x, self.p[prefix + ".weight"], self.p[prefix + ".bias"], mask=mask)
        rm, rv = running_update(self.p[prefix + ".running_mean"], self.p[prefix + ".running_var"], m, v, x.shape[0])
        self.buffers[prefix + ".running_mean"], self.buffers[prefix + ".running_var"] = rm, rv
        self.z[prefix] = z.detach()
        return y

    def comb_conv(self, x, prefix):                     # Comb_Conv: BatchNorm + ReLU, then the conv (Sequential indices 0 and 2)
        return self.conv(self.bn(x, prefix + ".0"), prefix + ".2")

    def residual(self, x, prefix):                      # Residual_Comb_Conv with in_dim == out_dim: no short-cut layer
        return self.comb_conv(self.comb_conv(x, prefix + ".comb_layer_in"), prefix + ".comb_layer_out") + x

    def grads(self):
        return {k: npy(t.grad) for k, t in self.p.items() if t.requires_grad and t.grad is not None}

    def bias_mass(self):
        """{conv bias name: sum over (b, g) of |dy[b,o,g]|}: the mass of the terms a bias gradient sums (see shifted_by_mass)"""
        return {k + ".bias": npy(y.grad.abs().sum((0, 2))) for k, y in self.conv_out.items()}


def partI_network(ps, feats, prefix="PartI_net."):
    """PartI_network.forward in train mode: (B,32,60) -> eqv (B,32,60), inv (B,32)"""
    x = T(feats, ps.dtype)
    h = ps.conv(x, prefix + "Conv_in.0")
    h = ps.residual(h, prefix + "SO3_Conv_layers.0")
    eqv = ps.comb_conv(h, prefix + "Conv_out.comb_layer") + x
    inv = eqv.mean(-1)
    eqv = eqv / torch.clamp_min(torch.sqrt((eqv * eqv).sum(1, keepdim=True)), 1e-4)
    inv = inv / torch.clamp_min(torch.sqrt((inv * inv).sum(1, keepdim=True)), 1e-4)
    return eqv, inv


def partII_so3_conv(ps, feats, prefix=""):
    """PartII_train.PartII_SO3_Conv in train mode: (B,128,60) -> (B,256,60)"""
    h = ps.comb_conv(T(feats, ps.dtype), prefix + "Conv_init.comb_layer")
    return ps.residual(h, prefix + "PartII_SO3_Conv_layers.0")


def stack_case(stack, sd, N, feats, cots, dtype=F64, masks=None):
    """one pass of `stack` (partI_network / partII_so3_conv) and the gradients of sum(out * cot) over its outputs
    -> dict: out (tuple of arrays), grads {name: array}, buffers {name: array}, z {bn prefix: array}, mass {conv bias name: array}"""
    ps = Pass(sd, N, dtype, masks)
    out = stack(ps, feats)
    out = out if isinstance(out, tuple) else (out,)
    sum((o * T(c, dtype)).sum() for o, c in zip(out, cots)).backward()
    return dict(out=tuple(npy(o) for o in out), grads=ps.grads(), buffers={k: npy(v) for k, v in ps.buffers.items()},
                z={k: npy(v) for k, v in ps.z.items()}, mass=ps.bias_mass())


def shifted_by_mass(db, mass):
    """A conv bias gradient is the sum of dy over (b, g).  In front of a BatchNorm with batch statistics that sum is analytically zero
    (float64 leaves 1e-14 of it), so its error has no value of its own to be measured against: it is measured against the mass
    sum |dy| of the terms instead, by adding that mass (float64, from the reference pass) to the result and to the reference alike before
    the one comparison every tensor gets.  Used for every conv bias, zero or not."""
    return np.asarray(db, np.float64) + np.asarray(mass, np.float64)


# ----------------------------------------------------------------------------------------
# the comparison
# ----------------------------------------------------------------------------------------
def e_ref(ref32, ref):
    """the float32 restatement's own distance from float64: the larger of rel and rel_rows (ref64.errors) over the given outputs"""
    return max(errors(_f(ref32), _f(ref, np.float64)))


def _f(a, dtype=None):
    """arrays for ref64.errors; a per-channel VECTOR (mean, var, a BatchNorm or bias gradient, a running buffer) becomes one row: its
    elements are sums that may cancel to nearly nothing, and an element's error relative to that element alone measures the cancellation,
    not the kernel"""
    if isinstance(a, (tuple, list)):
        return tuple(_f(x, dtype) for x in a)
    a = np.asarray(a, dtype)
    return a.reshape(1, -1) if a.ndim == 1 else a


def check(what, got, ref, ref32, factor=None):
    """(ok, worst multiple of e_ref) of `got` (array or tuple) against float64 `ref`, e_ref from the float32 restatement `ref32`;
    prints the figures as test_gpu_precision.py does"""
    factor = TRAIN_FACTOR if factor is None else factor
    got, ref = _f(got), _f(ref, np.float64)
    er = e_ref(ref32, ref)
    if er == 0.0:                                       # the float32 restatement is exact here: so must the result be
        ok = max(errors(got, ref)) == 0.0
        print("%s: e_ref 0, exact %s" % (what, ok))
        return ok, 0.0 if ok else float("inf")
    ok, worst = within_budget(got, ref, er, factor)
    print("%s: e_ref %.3g, errors / e_ref %s, worst %.2f of %g" % (what, er, " ".join("%.2f" % (e / er) for e in errors(got, ref)), worst, factor))
    return ok, worst


# ----------------------------------------------------------------------------------------
# inputs (one definition for the CPU and the GPU side)
# ----------------------------------------------------------------------------------------
def conv_case(cin, cout, B, seed=0):
    """x (B,cin,60) ~ N(0,1), W (cout,cin,1,13) ~ U(+-sqrt(3 / fan_in)), bias U(+-0.1), dy (B,cout,60) ~ N(0,1); float32 arrays"""
    g = torch.Generator().manual_seed(1000003 * seed + 10007 * cin + 101 * cout + B)
    x = torch.randn(B, cin, G, generator=g)
    W = (torch.rand(cout, cin, 1, NTAP, generator=g) * 2 - 1) * float(np.sqrt(3.0 / (cin * NTAP)))
    b = (torch.rand(cout, generator=g) - 0.5) * 0.2
    dy = torch.randn(B, cout, G, generator=g)
    return x.numpy(), W.numpy(), b.numpy(), dy.numpy()


KINDS = ("ordinary", "r3", "r30", "r300", "constant", "dead")
KINK_REL, KINK_MOVE = 1e-3, 2e-3
CONSTANT = 1.5                      # k * 1.5 is exact in fp32 for every k of these sizes: mean = 1.5 and var = 0 in every precision


def bn_kinds(C):
    """channel kind of every channel: the six kinds in turn, so that C = 8 already holds each of them"""
    return np.array([KINDS[c % len(KINDS)] for c in range(C)])


def bn_case(C, B, running, seed=0):
    """One BatchNorm + ReLU case with every channel kind in one tensor and no pre-activation within KINK_REL channel-stds of zero.
    -> dict x (B,C,60), gamma, beta, dy, kinds, and rm / rv (the running statistics: given in `running` mode, the buffers before the
    step otherwise).  ordinary: N(0.3, 1.7^2); rN: N(N, 1); constant: 1.5 everywhere; dead: beta = -12, every output 0."""
    g = torch.Generator().manual_seed(7919 * seed + 131 * C + B + (50000 if running else 0))
    kinds = bn_kinds(C)
    x = torch.randn(B, C, G, generator=g)
    gamma = 0.5 + torch.rand(C, generator=g)
    beta = (torch.rand(C, generator=g) - 0.5) * 0.6
    rm = (torch.rand(C, generator=g) - 0.5) * 0.4
    rv = 0.5 + torch.rand(C, generator=g)
    for c, kind in enumerate(kinds):
        if kind == "ordinary":
            x[:, c] = x[:, c] * 1.7 + 0.3
        elif kind in ("r3", "r30", "r300"):
            r = float(kind[1:])
            x[:, c] += r
            rm[c] += r                                  # running statistics of such a channel are those of its data
        elif kind == "constant":
            x[:, c] = CONSTANT
            beta[c] = 0.25 if c % 2 else -0.25
        else:
            beta[c] = -12.0
    dy = torch.randn(B, C, G, generator=g)
    x = unkink(x, gamma, beta, (rm, rv) if running else None)
    return dict(x=x.numpy(), gamma=gamma.numpy(), beta=beta.numpy(), dy=dy.numpy(), kinds=kinds, rm=rm.numpy(), rv=rv.numpy())


def kink_count(z):
    """number of elements of z (B,C,60) with |z| < KINK_REL * (std of z over its channel)"""
    z = torch.as_tensor(z)
    s = z.std((0, 2), unbiased=False)
    return int((z.abs() < KINK_REL * s[None, :, None]).sum())


def unkink(x, gamma, beta, running=None):
    """move every element whose float64 pre-activation is within KINK_REL channel-stds of zero to KINK_MOVE stds, keeping its sign (x stays
    fp32; with batch statistics moving an element shifts the statistics a little, hence the loop)"""
    x = x.clone()
    for _ in range(20):
        x64 = x.to(F64)
        rm, rv = (running[0].to(F64), running[1].to(F64)) if running is not None else (None, None)
        _, z, m, v = bn_relu(x64, gamma.to(F64), beta.to(F64), rm, rv)
        s = z.std((0, 2), unbiased=False)[None, :, None]
        near = z.abs() < KINK_REL * 1.05 * s            # a little more than asserted: rounding x to fp32 must not put one back
        if not near.any():
            return x
        sign = torch.where(z >= 0, 1.0, -1.0).to(F64)
        slope = (gamma.to(F64) / torch.sqrt(v + BN_EPS))[None, :, None]
        x = torch.where(near, x64 + (sign * KINK_MOVE * s - z) / slope, x64).to(F32)
    raise AssertionError("kink control did not converge")


def stack_input(which, B):
    """the (B,32,60) PartI features of a synth.train_batch, or four unit-feature blocks side by side as PartII's (B,128,60) input"""
    from yoho_amd import synth
    from yoho_amd.tables import default_tables
    if which == "partI":
        return synth.train_batch(B, default_tables().P, seed=300 + B)["feats0"][0]
    return np.concatenate([synth.unit_features(B, seed=8000 + 10 * B + i) for i in range(4)], axis=1)


def cotangents(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(*s, generator=g).numpy() for s in shapes)


def tap_inverse(N):
    """inv[k] = the tap k' with N[N[g,k'],k] == g for every g (the tap set is closed under inversion), from the table alone"""
    N = np.asarray(N).astype(np.int64)
    inv = []
    for k in range(NTAP):
        ks = [k2 for k2 in range(NTAP) if np.array_equal(N[N[:, k2], k], np.arange(G))]
        assert len(ks) == 1
        inv.append(ks[0])
    return np.array(inv)


MASK_Z, MASK_SHARE = 64 * 2.0 ** -24, 1e-4      # a device mask may differ from float64's only under MASK_Z * max|z64|, on at most this share


def mask_differences(mask, z64):
    """(number of elements where mask != (z64 > 0), the largest |z64| among them over the layer's largest |z64|)"""
    diff = np.asarray(mask, bool) != (z64 > 0)
    zmax = float(np.abs(z64).max())
    return int(diff.sum()), (float(np.abs(z64[diff]).max()) / zmax if diff.any() else 0.0)
