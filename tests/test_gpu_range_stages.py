"""The fp16 range guard stage by stage, channel by channel (-m gpu).

tests/test_gpu_precision.py raises the range word by multiplying an INPUT row by 1e5: every stage of that row overflows, all channels at
once, so the first kernel that sees the row flags it and every later kernel - or a single register, lane half or row block of an
epilogue - could track nothing without a test noticing.  Here ONE channel of ONE stage leaves its fp16 plane, for one keypoint (match):
tests/ref64.py moves a power of two s between a layer and its consumer (rescale_stage: the network is the same function, channel o of
stage S is s times as large), and plans s from float64 alone so that the spiked row (times R.MILD) is a factor 2 outside the limit of
include/yoho_hip.h there and everything else - the same channel of every other row, every other channel and stage of every row, and
the whole mild twin (the same row times R.TWIN) - a factor 2 inside (tests/test_precision_cpu.py asserts that plan for every case
below without a device).  The only kernel that can then raise the word is the one that writes stage S, from the accumulator slot that
holds channel o (profiles/precision.md, 'range guard, stage by stage', names it per stage).

Every case, raw calls with check_range=False on a context of its own:  the unspiked batch raises nothing;  the mild twin raises
nothing, repeats nothing, warns of nothing;  the spiked row raises its network's word and leaves every other row's bits alone;  the
word is clear again on the next unspiked call.  At B = 33 the guarded call also warns, repeats once in bf16x3, restores the mode and
meets the 12 x e_ref budget for all rows against the float64 pass of the RESCALED network.

Two stages are not guarded and need no guard (UNGUARDED below): their values never enter an fp16 plane."""
import warnings

import numpy as np
import pytest
import torch

import ref64 as R

pytestmark = pytest.mark.gpu

CASES = R.range_stage_cases()
# PartII's mid (the cone layer's output) and h2 (the g = 0 layer's, residual added) stay in fp32 registers / fp32 buffers from the
# accumulators to the batch norm resp. the FC head in both modes: gconv16_kernel / cgemm_kernel fold BN + ReLU into their epilogue and
# write the ACTIVATION a1 as planes, cone1_kernel and mlp_head work in fp32.  No plane, no overflow: such a case must raise nothing and
# deliver the budget without a repeat (include/yoho_hip.h at yoho_range_status lists the guarded stages).
UNGUARDED = {("partII", "mid"), ("partII", "h2")}


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _reference(net, stage, p, sd, tables, row):
    """-> (float64 outputs, e_ref) of the spiked batch under the RESCALED network.  Where the rescaling is exact and has a consumer the
    base network's float64 pass and fp32 oracle are the rescaled network's (test_rescaled_network_is_the_base_network_but_for_one_channel);
    h2 and y are evaluated under the rescaled state dict."""
    d = p["sd"] if stage in ("h2", "y") else sd
    if net == "partI":
        _, ref, eref, _ = R.partI_case_spiked(p["x"], d, tables.N, row, R.MILD)
    else:
        _, ref, eref, _ = R.partII_case_spiked(p["feats"], p["pre"], d, tables.N, tables.P, row, R.MILD)
    return ref, eref


@pytest.mark.parametrize("net,mode,stage,o,B,row", CASES, ids=["%s-%s-%s-o%d-B%d-r%d" % c for c in CASES])
def test_one_channel_of_one_stage_outside(hip, sd1, sd2, tables, net, mode, stage, o, B, row):
    sd = sd1 if net == "partI" else sd2
    p = R.range_stage_plan(net, stage, o, B, row, sd, tables.N, tables.P)
    assert p is not None and min(p["margins"].values()) >= 2.0, p and p["margins"]
    what = "%s %s %s o=%d B=%d row %d, s = 2^%d" % (net, mode, stage, o, B, row, int(np.log2(p["s"])))
    c = hip.Context()
    if net == "partI":
        c.load_partI(p["sd"])
        c.set_gconv_mode(mode)
        base, which, flagged, keys = [p["x"]], "gconv", (True, False), ("eqv", "inv")

        def fwd(arrs, **kw):
            out = c.partI_forward(cu(arrs[0]), want_inv=True, **kw)
            return tuple(out[k] for k in keys)
    else:
        c.load_partII(p["sd"])
        c.set_partII_mode(mode)
        base, which, flagged, keys = p["feats"], "partII", (False, True), ("q",)
        pre = cu(p["pre"])

        def fwd(arrs, **kw):
            return (c.partII_forward(*[cu(a) for a in arrs], pre, **kw),)
    c.range_sticky_after = 0
    guarded = (net, stage) not in UNGUARDED
    current = lambda: c.gconv_mode if net == "partI" else c.partII_mode

    raw0 = fwd(base, check_range=False)
    assert c.range_status() == (False, False), what + ": the unspiked batch raises the word"

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        twin = fwd(R.spike(base, row, R.TWIN))
    assert c.range_status() == (False, False) and c.range_fallbacks == 0 and c.range_repeats[which] == 0, what + ": mild twin"
    assert all(torch.isfinite(t).all() for t in twin)

    spiked = R.spike(base, row, R.MILD)
    raw = fwd(spiked, check_range=False)
    status = c.range_status()
    print("%s: margins out %.2f base %.2f twin %.2f rest %.2f -> %s" % ((what,) + tuple(p["margins"][k] for k in ("out", "base", "twin", "rest")) + (status,)))
    assert status == (flagged if guarded else (False, False)), what
    keep = torch.ones(B, dtype=torch.bool, device=raw0[0].device)
    keep[row] = False
    for k, a, b in zip(keys, raw, raw0):
        a, b = a[keep].reshape(B - 1, -1), b[keep].reshape(B - 1, -1)
        if mode == "fgemm8":          # one fp8 scale per launch: a keypoint's bits depend on the launch (csrc/api.hip at partI_passG)
            assert torch.isfinite(a).all(), (what, k)
            d = float((a - b).abs().max() / b.abs().max())
            print("    fgemm8 %s: other rows within %.2g of the unspiked call" % (k, d))
            assert d < 1e-4, (what, k, d)
        else:
            bad = (a != b).any(1).nonzero().flatten().tolist()
            assert not bad, (what, k, bad[:8], len(bad))
    again = fwd(base, check_range=False)
    assert c.range_status() == (False, False), what + ": the word is still up on the next unspiked call"
    if mode != "fgemm8":
        assert all(torch.equal(a, b) for a, b in zip(again, raw0))

    if B != 33 or mode == "fgemm8":
        return
    ref, eref = _reference(net, stage, p, sd, tables, row)
    if guarded:
        with pytest.warns(RuntimeWarning, match="fp16 range") as rec:
            got = fwd(spiked)
        assert sum("fp16 range" in str(w.message) for w in rec) == 1 and c.range_fallbacks == 1 and c.range_repeats[which] == 1 and current() == mode, what
    else:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = fwd(spiked)
        assert c.range_fallbacks == 0 and current() == mode, what
    assert c.range_status() == (False, False)
    got = tuple(t.cpu().numpy() for t in got)
    got, ref = (got[0], ref) if net == "partII" else (got, ref)
    ok, worst = R.within_budget(got, ref, eref)
    print("    guarded call (%s): e_ref %.3g, worst %.2f e_ref of %g" % ("repeated in bf16x3" if guarded else "no repeat", eref, worst, R.FACTOR))
    assert ok, (what, worst)
