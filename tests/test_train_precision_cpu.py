"""The float64 training reference of tests/train_ref64.py and the budget built on it, checked on the CPU.

- The reference is pinned to torch's own conv2d / batch_norm autograd in float64 on the materialised gather and to the golden vectors of
  the reference's training step (tests/golden/train.npz): both independent of this project's kernels.
- The comparison the GPU tests use (train_ref64.check: within TRAIN_FACTOR x e_ref of float64 per element, in rel and per row) REJECTS
  defects emulated inside the float32 restatement, each by more than 12 x e_ref - the cap of TRAIN_FACTOR - while the old checks (one
  max-norm rel against an fp32 result at 1e-5 / 1e-4, the 19-number digest at 2e-4) let several of them through.  The figures are in
  profiles/precision.md, "Training kernels".
- The constructions the GPU tests rely on: kink control leaves no pre-activation near zero, the chosen seeds keep the stacks' float64
  pre-activations away from zero, and two summation orders of an fp32 sum lie within a factor 2 of each other.
"""
import numpy as np
import pytest
import torch

import train_ref64 as TR
from yoho_amd import synth, weights as W

FEW = 4.0          # two honest fp32 evaluations of one function are each within ~1 e_ref of float64 (tests/test_precision_cpu.py)
CAP = 12.0         # ref64.FACTOR: the upper cap of TRAIN_FACTOR; every emulated defect must exceed it
OLD_REL, OLD_REL_W, OLD_DIGEST = 1e-5, 1e-4, 2e-4       # what tests/test_gpu_train.py asserts
F32 = torch.float32


def digest_err(a, b):
    """the whole-step tests' measure: largest difference of the 19-number digests over the l2 norm of the reference"""
    d, g = synth.tensor_digest(a), synth.tensor_digest(b)
    return float(np.abs(d - g).max() / max(g[0], 0.05))


def multiple(got, ref, ref32):
    return max(TR.errors(TR._f(got), TR._f(ref, np.float64))) / TR.e_ref(ref32, ref)


def row(name, got, ref, ref32, old_tol):
    """one line of the table: defect, old rel against the fp32 result, old digest error, multiples of e_ref"""
    m, r, d = multiple(got, ref, ref32), TR.rel(got, ref32), digest_err(got, ref32)
    print("| %s | %.2g (%s %.0e) | %.2g (%s 2e-4) | %.0f |" % (name, r, "passes" if r < old_tol else "fails", old_tol, d,
                                                            "passes" if d < OLD_DIGEST else "fails", m))
    return m


# ---- the reference itself ---------------------------------------------------------------------------------------------------------------
def test_ref64_agrees_with_torch_autograd_on_the_materialised_gather(tables):
    """gconv + bn_relu (batch and running statistics) in float64 against conv2d / batch_norm / relu of torch on the (B,C,60,13) gather"""
    B, cin, cout = 3, 8, 16
    x, Wt, b, dy = TR.conv_case(cin, cout, B, seed=5)
    nei = torch.from_numpy(tables.N.astype(np.int64).reshape(-1))
    for running in (False, True):
        c = TR.bn_case(cin, B, running, seed=5)
        # ours: bn_relu -> gconv
        xt, gt, bt = TR.T(c["x"], grad=True), TR.T(c["gamma"], grad=True), TR.T(c["beta"], grad=True)
        wt, cb = TR.T(Wt, grad=True), TR.T(b, grad=True)
        rm, rv = (TR.T(c["rm"]), TR.T(c["rv"])) if running else (None, None)
        a, _, m, v = TR.bn_relu(xt, gt, bt, rm, rv)
        y = TR.gconv(a, wt, cb, tables.N)
        (y * TR.T(dy)).sum().backward()
        nrm, nrv = TR.running_update(TR.T(c["rm"]), TR.T(c["rv"]), m, v, B)
        # torch: gather -> batch_norm -> relu -> conv2d
        xr, gr, br = TR.T(c["x"], grad=True), TR.T(c["gamma"], grad=True), TR.T(c["beta"], grad=True)
        wr, cr = TR.T(Wt, grad=True), TR.T(b, grad=True)
        trm, trv = TR.T(c["rm"]), TR.T(c["rv"])
        xg = xr[:, :, nei].reshape(B, cin, 60, 13)
        ar = torch.relu(torch.nn.functional.batch_norm(xg, trm, trv, gr, br, not running, TR.MOMENTUM, TR.BN_EPS))
        yr = torch.nn.functional.conv2d(ar, wr, cr)[:, :, :, 0]
        (yr * TR.T(dy)).sum().backward()
        for name, p, q in (("y", y, yr), ("dx", xt.grad, xr.grad), ("dgamma", gt.grad, gr.grad), ("dbeta", bt.grad, br.grad),
                           ("dW", wt.grad, wr.grad), ("db", cb.grad, cr.grad)):
            assert TR.rel(TR.npy(p), TR.npy(q)) < 1e-12, (running, name)
        if not running:
            assert TR.rel(TR.npy(nrm), TR.npy(trm)) < 1e-12 and TR.rel(TR.npy(nrv), TR.npy(trv)) < 1e-12


def test_ref64_agrees_with_the_golden_training_step(gold, sd1, tables):
    """PartI_network in train mode on the golden batch against the reference run's own outputs, to a few e_ref"""
    g = gold("train.npz")
    b = synth.train_batch(int(g["bn"]), tables.P, seed=int(g["seed"]))
    for key, feats, pick in (("p1_inv0", b["feats0"][0], 1), ("p1_eqv1", b["feats1"][0], 0)):
        ref = TR.partI_network(TR.Pass(sd1, tables.N), feats)[pick].detach().numpy()
        r32 = TR.partI_network(TR.Pass(sd1, tables.N, F32), feats)[pick].detach().numpy()
        ok, worst = TR.check("golden " + key, g[key], ref, r32, factor=FEW)
        assert ok, (key, worst)
        assert 1e-8 < TR.e_ref(r32, ref) < 1e-5


def test_transposed_conv_is_the_data_gradient(tables):
    """train.hip's header: dx = the same convolution with W transposed in (o,c) and the taps relabelled by inv; here in float64 against
    autograd, with inv derived from the table alone (test_gpu_train_precision.py probes the device against W[o,:,inv k])"""
    x, Wt, b, dy = TR.conv_case(8, 24, 2, seed=1)
    inv = TR.tap_inverse(tables.N)
    _, dx, _, _ = TR.gconv_grads(x, Wt, b, tables.N, dy)
    Wt64 = TR.T(Wt)[:, :, 0, :]
    dx2 = TR.npy(TR.gconv(TR.T(dy), Wt64.permute(1, 0, 2)[:, :, inv], None, tables.N))
    assert TR.rel(dx2, dx) < 1e-13


# ---- the constructions the GPU tests rely on ----------------------------------------------------------------------------------------
BN_SHAPES = ((8, 1), (32, 4), (32, 5), (40, 33), (512, 3))


@pytest.mark.parametrize("running", (False, True))
@pytest.mark.parametrize("C,B", BN_SHAPES)
def test_kink_control_leaves_nothing_under_the_threshold(C, B, running):
    c = TR.bn_case(C, B, running)
    r = TR.bn_relu_grads(c["x"], c["gamma"], c["beta"], c["dy"], (c["rm"], c["rv"]) if running else None)
    assert TR.kink_count(r["z"]) == 0
    assert set(c["kinds"]) == set(TR.KINDS)
    k = c["kinds"]
    assert (r["y"][:, k == "dead"] == 0).all()
    if not running:
        assert (r["var"][k == "constant"] == 0).all() and (r["mean"][k == "constant"] == TR.CONSTANT).all()
    for kind, ratio in (("r3", 3), ("r30", 30), ("r300", 300)):               # unit std by construction; kink control moves little
        assert np.all(np.abs(c["x"][:, k == kind] - ratio) < 6.0)


@pytest.mark.parametrize("which,B,seed", (("partI", 6, 7), ("partI", 33, 7), ("partI", 6, 11), ("partI", 33, 11), ("partII", 6, 7),
                                          ("partII", 6, 11)))
def test_chosen_seeds_stay_under_the_mask_cap(tables, which, B, seed):
    """the float64 pass alone: the share of a layer's pre-activations under MASK_Z * max|z| - where a device mask MAY differ - is at most
    MASK_SHARE for every layer of the stacks the GPU test runs"""
    sd = W.synth_state_dict(W.PARTI_SPEC if which == "partI" else W.PARTII_SPEC, seed)
    ps = TR.Pass(sd, tables.N)
    with torch.no_grad():
        (TR.partI_network if which == "partI" else TR.partII_so3_conv)(ps, TR.stack_input(which, B))
    assert len(ps.z) == 3
    for name, z in ps.z.items():
        share = float((z.abs() < TR.MASK_Z * z.abs().max()).double().mean())
        print("%s B=%d seed %d, %s: %.2g of the elements under the mask threshold" % (which, B, seed, name, share))
        assert share <= TR.MASK_SHARE, (name, share)


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_permuted_summation_order_stays_within_a_factor_two(seed):
    """why TRAIN_FACTOR is TWICE the worst measured multiple: two realisations of one fp32 sum (the terms of a 256-channel, 13-tap output
    in index order and in a permuted order, sequential fp32 accumulation) differ from float64 by amounts within a factor 2 of each other,
    as rel over 2048 such sums"""
    rs = np.random.RandomState(seed)
    n = 256 * 13
    terms = (rs.randn(2048, n) * rs.uniform(-1, 1, size=(2048, n))).astype(np.float32)
    exact = terms.astype(np.float64).sum(1)
    e = []
    for order in (np.arange(n), rs.permutation(n), rs.permutation(n)):
        s = np.cumsum(terms[:, order], axis=1, dtype=np.float32)[:, -1]
        e.append(TR.rel(s, exact))
    print("fp32 sums of %d terms, seed %d: rel against float64 in three orders %s" % (n, seed, " ".join("%.3g" % v for v in e)))
    assert max(e) / min(e) < 2.0


# ---- mutation checks ----------------------------------------------------------------------------------------------------------------
def round_mantissa(t, bits=10):
    """fp32 values rounded to `bits` explicit mantissa bits (what a reduced-precision matrix path feeds its multipliers), straight-through
    for autograd"""
    drop = 23 - bits
    i = t.detach().contiguous().view(torch.int32)
    r = ((i + (1 << (drop - 1))) & ~((1 << drop) - 1)).view(torch.float32)
    return t + (r - t).detach()


@pytest.fixture(scope="module")
def layer(tables):
    """one 32 -> 256 layer at B = 7 (a shape of the old kernel test): float64 and float32 restatement"""
    x, Wt, b, dy = TR.conv_case(32, 256, 7)
    return (x, Wt, b, dy), TR.gconv_grads(x, Wt, b, tables.N, dy), TR.gconv_grads(x, Wt, b, tables.N, dy, F32)


def test_a_reduced_precision_operands_are_rejected(layer, tables):
    """a. the operands of one layer rounded to 10 mantissa bits: forward, data gradient, weight gradient"""
    (x, Wt, b, dy), r64, r32 = layer
    xt, wt, bt = TR.T(x, F32, True), TR.T(Wt, F32, True), TR.T(b, F32, True)
    y = TR.gconv(round_mantissa(xt), round_mantissa(wt), bt, tables.N)
    (y * round_mantissa(TR.T(dy, F32))).sum().backward()
    got = (TR.npy(y), TR.npy(xt.grad), TR.npy(wt.grad))
    for name, g, i, tol in (("forward", got[0], 0, OLD_REL), ("data gradient", got[1], 1, OLD_REL), ("weight gradient", got[2], 2, OLD_REL_W)):
        assert multiple(r32[i], r64[i], r32[i]) <= 1.0                          # the restatement itself is accepted
        m = row("a. operands at 10 mantissa bits, 32->256 B=7: " + name, g, r64[i], r32[i], tol)
        assert m > CAP, (name, m)


def test_b_one_wgrad_block_off_is_rejected(tables):
    """b. one 32 x 32 block - the work of one wgrad_kernel workgroup - of a 512 x 256 weight gradient off by 1e-3 relative"""
    x, Wt, b, dy = TR.conv_case(256, 512, 2)
    dW64 = TR.gconv_grads(x, Wt, None, tables.N, dy)[2]
    dW32 = TR.gconv_grads(x, Wt, None, tables.N, dy, F32)[2]
    bad = dW32.copy()
    bad[32:64, 64:96] *= np.float32(1.0 + 1e-3)
    m = row("b. one 32x32 block of the 512x256 weight gradient off by 1e-3", bad, dW64, dW32, OLD_REL_W)
    assert m > CAP, m
    assert digest_err(bad, dW32) < OLD_DIGEST                                   # what the whole-step tests see: nothing


def _bn_r30(B=33, C=8):
    g = torch.Generator().manual_seed(77)
    x = torch.randn(B, C, TR.G, generator=g) + 30.0
    gamma, beta = 0.5 + torch.rand(C, generator=g), (torch.rand(C, generator=g) - 0.5) * 0.6
    x = TR.unkink(x, gamma, beta)
    return x.numpy(), gamma.numpy(), beta.numpy(), torch.randn(B, C, TR.G, generator=g).numpy()


def test_c_one_pass_variance_is_rejected():
    """c. the variance as E[x^2] - m^2 in fp32 at mean / std = 30"""
    x, gamma, beta, dy = _bn_r30()
    r64 = TR.bn_relu_grads(x, gamma, beta, dy)
    r32 = TR.bn_relu_grads(x, gamma, beta, dy, dtype=F32)
    xt = torch.from_numpy(x)
    m = xt.mean((0, 2))
    var = (xt * xt).mean((0, 2)) - m * m
    y = TR.npy(TR.bn_relu(xt, torch.from_numpy(gamma), torch.from_numpy(beta), m, var)[0])
    assert multiple(r32["y"], r64["y"], r32["y"]) <= 1.0
    mv = row("c. one-pass fp32 variance at r = 30: var", var.numpy(), r64["var"], r32["var"], OLD_REL)
    my = row("c. one-pass fp32 variance at r = 30: y", y, r64["y"], r32["y"], 2e-6)
    assert mv > CAP and my > CAP, (mv, my)


def test_d_fp32_index_order_reduction_is_measured():
    """d. sum dz * xhat of the BatchNorm backward accumulated in fp32 over B * 60 = 1980 terms in index order, instead of in f64.
    Measured: it does NOT clear 12 x e_ref (about 1 to 3 e_ref: a sequential fp32 sum of 1980 terms of mixed sign is an honest fp32
    evaluation, and the float32 restatement's own dgamma is no better), so it is reported in the table and not asserted as a rejection;
    what is asserted is that it stays an honest one, under the cap."""
    x = TR.conv_case(32, 32, 33, seed=3)[0]
    g = torch.Generator().manual_seed(78)
    gamma, beta = (0.5 + torch.rand(32, generator=g)).numpy(), ((torch.rand(32, generator=g) - 0.5) * 0.6).numpy()
    x = TR.unkink(torch.from_numpy(x), torch.from_numpy(gamma), torch.from_numpy(beta)).numpy()
    dy = torch.randn(33, 32, TR.G, generator=g).numpy()
    r64 = TR.bn_relu_grads(x, gamma, beta, dy)
    r32 = TR.bn_relu_grads(x, gamma, beta, dy, dtype=F32)
    xt = torch.from_numpy(x)
    m, v = TR.batch_stats(xt)
    xh = ((xt - m[None, :, None]) / torch.sqrt(v + TR.BN_EPS)[None, :, None]).numpy()
    dz = np.where(r32["z"] > 0, dy, np.float32(0))
    terms = np.ascontiguousarray((dz * xh).transpose(1, 0, 2)).reshape(32, -1).astype(np.float32)
    assert terms.shape[1] == 1980
    dgamma = np.cumsum(terms, axis=1, dtype=np.float32)[:, -1]
    mlt = row("d. fp32 index-order sum of dz * xhat over 1980 terms: dgamma", dgamma, r64["dgamma"], r32["dgamma"], 2e-5)
    assert mlt < CAP, mlt


def test_e_swapped_inverse_taps_are_rejected(layer, tables):
    """e. two taps of the inverse table swapped in the data gradient (the structural control: large)"""
    (x, Wt, b, dy), r64, r32 = layer
    inv = TR.tap_inverse(tables.N)
    moved = [k for k in range(TR.NTAP) if inv[k] != k]
    bad = inv.copy()
    bad[moved[0]], bad[moved[1]] = inv[moved[1]], inv[moved[0]]
    Wt32 = torch.from_numpy(Wt)[:, :, 0, :].permute(1, 0, 2)
    good = TR.npy(TR.gconv(torch.from_numpy(dy), Wt32[:, :, inv], None, tables.N))
    assert multiple(good, r64[1], r32[1]) < FEW
    got = TR.npy(TR.gconv(torch.from_numpy(dy), Wt32[:, :, bad], None, tables.N))
    m = row("e. two taps of the inverse table swapped: data gradient", got, r64[1], r32[1], OLD_REL)
    assert m > 1e4 and TR.rel(got, r32[1]) > OLD_REL


def test_check_rejects_non_finite_and_handles_an_exact_reference():
    ref = np.arange(6, dtype=np.float64).reshape(2, 3)
    assert TR.check("exact", ref.astype(np.float32), ref, ref.astype(np.float32)) == (True, 0.0)
    off = ref.astype(np.float32)
    off[1, 2] += 1e-6
    assert TR.check("exact, result off", off, ref, ref.astype(np.float32)) == (False, float("inf"))
    bad = ref.astype(np.float32)
    bad[0, 0] = np.nan
    assert TR.check("nan", bad, ref, off) == (False, float("inf"))
