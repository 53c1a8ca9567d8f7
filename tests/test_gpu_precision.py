"""The precision contract of the PartI / PartII hot path against a float64 reference (-m gpu).

The parity tests of test_gpu_kernels.py assert 1e-4 against the fp32 oracle; a layer that drops one of the three products of the fp16
split sits at 1e-4, and one that drops it on a single irrep at 1e-5 (tests/test_precision_cpu.py emulates both).  Here every mode that is
documented as fp32-accurate must stay within 12 x e_ref of tests/ref64.py's float64 pass, in rel and in rel_rows, where e_ref is the
fp32 oracle's own distance from float64 on the same input and 12 = (3 * 2^-22) / 2^-24 is the header's per-product bound of the 2-way
fp16 split over fp32's unit roundoff (ref64.FACTOR; not taken from the code under test).  Besides the budget: a keypoint's bits do not
depend on the rows that share its launch, and the fp16 range word is raised from every tile position - and only when it must be.

Every test prints its figures as multiples of e_ref (profiles/precision.md keeps one run of them)."""
import warnings

import numpy as np
import pytest
import torch

import ref64 as R

pytestmark = pytest.mark.gpu

PARTI_MODES = ("f32", "bf16x3", "fp16x2", "fourier", "fgemm", "fgemm256", "fgemm128")        # fgemm8 keeps its own 5e-5 test
PARTII_MODES = ("f32", "bf16x3", "fp16x2", "cgemm")                                          # cgemm8 likewise


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def ctx_for(hip, sd2):
    """contexts by (network, mode, state dict name), made on first use and kept for the module"""
    made = {}

    def get(net, mode, sdname="seed7"):
        key = (net, mode, sdname)
        if key not in made:
            c = hip.Context()
            if net == "partI":
                c.load_partI(R.partI_state_dict(sdname))
                c.set_gconv_mode(mode)
            else:
                c.load_partII(sd2)
                c.set_partII_mode(mode)
            c.range_sticky_after = 0            # a flagged pass is repeated every time: no test here changes another's arithmetic
            made[key] = c
        return made[key]
    return get


def _partI(c, x, **kw):
    o = c.partI_forward(cu(x), want_inv=True, **kw)
    return o["eqv"].cpu().numpy(), o["inv"].cpu().numpy()


def _report(what, got, ref, eref):
    ok, worst = R.within_budget(got, ref, eref)
    print("%s: e_ref %.3g, errors / e_ref %s, worst %.2f of %g" % (what, eref, " ".join("%.2f" % (e / eref) for e in R.errors(got, ref)), worst, R.FACTOR))
    return ok


# ---- a. error budget, PartI -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", R.PARTI_B)
@pytest.mark.parametrize("mode", PARTI_MODES)
def test_partI_error_budget(ctx_for, tables, mode, B):
    sd = R.partI_state_dict("seed7")
    x = R.partI_input(B)
    ref, eref, _ = R.partI_case(x, sd, tables.N)
    c = ctx_for("partI", mode)
    got = _partI(c, x)
    assert _report("PartI %s B=%d" % (mode, B), got, ref, eref)
    assert c.range_fallbacks == 0


@pytest.mark.parametrize("B", (33, 257))
@pytest.mark.parametrize("mode", ("fgemm", "f32"))
@pytest.mark.parametrize("sdname", ("seed11", "seed23", "bias30"))
def test_partI_error_budget_other_weights(ctx_for, tables, sdname, mode, B):
    """two seeds that never went through the weight packers, and conv biases of +-3: the sqrt(60) * bias term of the d = 1 epilogue
    then dominates the trivial irrep"""
    sd = R.partI_state_dict(sdname)
    x = R.partI_input(B)
    ref, eref, _ = R.partI_case(x, sd, tables.N)
    c = ctx_for("partI", mode, sdname)
    got = _partI(c, x)
    assert _report("PartI %s %s B=%d" % (sdname, mode, B), got, ref, eref)
    assert c.range_fallbacks == 0


# ---- b. error budget, PartII ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", R.PARTII_M)
@pytest.mark.parametrize("mode", PARTII_MODES)
def test_partII_error_budget(ctx_for, sd2, tables, mode, M):
    feats, pre = R.partII_input(M)
    q64, eref, _ = R.partII_case(*feats, pre, sd2, tables.N, tables.P)
    c = ctx_for("partII", mode)
    q = c.partII_forward(*[cu(f) for f in feats], cu(pre)).cpu().numpy()
    assert q.shape == (M, 4)
    assert _report("PartII %s M=%d" % (mode, M), q, q64, eref)
    assert c.range_fallbacks == 0


# ---- c. keypoint independence, as bits --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", PARTI_MODES)
def test_partI_keypoint_bits_do_not_depend_on_the_launch(ctx_for, mode):
    """csrc/api.hip at partI_passG: 'a keypoint's arithmetic does not depend on which other keypoints share its launch' - so a row
    permutation of the input permutes the output, and rows put in front (1 / 31 / 32 / 255: every keypoint moves to another lane,
    another 32-keypoint tile, another 256-column tile) change nothing in the rows behind them"""
    from yoho_amd import synth
    c = ctx_for("partI", mode)
    keys = ("eqv", "inv", "inv_np")
    x = cu(R.partI_input(300))
    base = c.partI_forward(x, want_inv=True, want_inv_np=True)
    assert all(torch.isfinite(base[k]).all() for k in keys)
    perm = cu(np.random.RandomState(3).permutation(300))
    o = c.partI_forward(x[perm].contiguous(), want_inv=True, want_inv_np=True)
    for k in keys:
        assert torch.equal(o[k], base[k][perm]), (mode, "permutation", k)
    other = cu(synth.unit_features(255, seed=999))
    for n in (1, 31, 32, 255):
        o = c.partI_forward(torch.cat([other[:n], x]), want_inv=True, want_inv_np=True)
        for k in keys:
            bad = (o[k][n:] != base[k]).reshape(300, -1).any(1).nonzero().flatten().tolist()
            assert not bad, (mode, "rows in front", n, k, bad[:8], len(bad))
    assert c.range_fallbacks == 0


@pytest.mark.parametrize("mode", ("fp16x2", "cgemm"))
def test_partII_match_bits_do_not_depend_on_the_launch(ctx_for, mode):
    from yoho_amd import synth
    M = 257
    c = ctx_for("partII", mode)
    feats, pre = R.partII_input(M)
    feats, pre = [cu(f) for f in feats], cu(pre)
    base = c.partII_forward(*feats, pre)
    assert torch.isfinite(base).all()
    perm = cu(np.random.RandomState(4).permutation(M))
    q = c.partII_forward(*[f[perm].contiguous() for f in feats], pre[perm].contiguous())
    assert torch.equal(q, base[perm]), (mode, "permutation")
    other = [cu(synth.unit_features(255, seed=990 + i)) for i in range(4)]
    opre = cu(np.random.RandomState(5).randint(0, 60, size=255).astype(np.int64))
    for n in (1, 31, 32, 255):
        q = c.partII_forward(*[torch.cat([o[:n], f]) for o, f in zip(other, feats)], torch.cat([opre[:n], pre]))
        bad = (q[n:] != base).any(1).nonzero().flatten().tolist()
        assert not bad, (mode, "rows in front", n, bad[:8], len(bad))
    assert c.range_fallbacks == 0


# ---- d. the range word reports from every position --------------------------------------------------------------------------------------
def _margins(stages_base, stages_row):
    """the float64 stage maxima of the whole batch (base rows and the spiked row) against the limits of the fp16 planes"""
    a0, c0 = R.stage_extent(stages_base)
    a1, c1 = R.stage_extent(stages_row)
    return R.ACT_LIMIT / max(a0, a1), R.COEF_LIMIT / max(c0, c1)


@pytest.mark.parametrize("B", R.PARTI_SPIKE_B)
def test_partI_range_word_reports_from_every_position(hip, tables, B):
    """mode fgemm, raw calls: ONE keypoint of the batch times 1e5 - at the first and last lane of a 32-keypoint wave tile, either side of
    the wave halves of a 256-column tile, in the second (ragged) column tile, in the last row - must raise the PartI word, must leave
    every other row's bits alone, and the guarded call must deliver the budget for the spiked row too.  Times 1e2 the same keypoint
    stays a factor 2 inside the planes (asserted from the float64 stages): no flag, no repeat, the budget for every row."""
    sd = R.partI_state_dict("seed7")
    c = hip.Context()
    c.load_partI(sd)
    c.set_gconv_mode("fgemm")
    c.range_sticky_after = 0
    x = R.partI_input(B)
    _, _, st_base = R.partI_case(x, sd, tables.N)
    raw0 = c.partI_forward(cu(x), want_inv=True, check_range=False)
    assert c.range_status() == (False, False)
    rows = R.spike_rows(B)
    assert rows[-1] == B - 1 and {0, 31, 32, 127, 128, 255, 256} <= set(rows)

    def mild(row, repeats):
        xs, ref, eref, st = R.partI_case_spiked(x, sd, tables.N, row, R.MILD)
        ma, mc = _margins(st_base, st)
        assert ma >= 2.0 and mc >= 2.0, (B, row, ma, mc)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = _partI(c, xs)
        assert c.range_status() == (False, False) and c.range_fallbacks == repeats and c.range_repeats["gconv"] == repeats, (B, row)
        assert _report("PartI fgemm B=%d, row %d x %g (margins %.1f / %.1f)" % (B, row, R.MILD, ma, mc), got, ref, eref), (B, row)

    for row in rows:
        mild(row, 0)
    for n, row in enumerate(rows):
        xs, ref, eref, st = R.partI_case_spiked(x, sd, tables.N, row, R.SPIKE)
        assert R.stage_floor(st, 0) > 4.5e4 > 2 * R.COEF_LIMIT
        raw = c.partI_forward(cu(xs), want_inv=True, check_range=False)
        assert c.range_status() == (True, False), (B, row)
        keep = torch.ones(B, dtype=torch.bool, device=raw0["eqv"].device)
        keep[row] = False
        for k in ("eqv", "inv"):
            bad = (raw[k][keep] != raw0[k][keep]).reshape(B - 1, -1).any(1).nonzero().flatten().tolist()
            assert not bad, (B, row, k, bad[:8], len(bad))
        with pytest.warns(RuntimeWarning, match="fp16 range"):
            got = _partI(c, xs)
        assert c.range_fallbacks == n + 1 and c.gconv_mode == "fgemm"
        assert _report("PartI fgemm B=%d, row %d x %g (repeated in bf16x3)" % (B, row, R.SPIKE), got, ref, eref), (B, row)
    mild(rows[-1], len(rows))             # behind the flagged passes: the word was cleared, nothing stale leaks


def test_partII_range_word_reports_from_every_position(hip, sd2, tables):
    """the same pair of cases for PartII in fp16x2: one spiked match of 257 at 0, 127, 128 and 256"""
    M = R.PARTII_SPIKE_M
    c = hip.Context()
    c.load_partII(sd2)
    c.set_partII_mode("fp16x2")
    c.range_sticky_after = 0
    feats, pre = R.partII_input(M)
    _, _, st_base = R.partII_case(*feats, pre, sd2, tables.N, tables.P)
    raw0 = c.partII_forward(*[cu(f) for f in feats], cu(pre), check_range=False)
    assert c.range_status() == (False, False)
    rows = (0, 127, 128, M - 1)
    conv = ("a_in", "h0", "a0", "mid", "a1", "h2")

    def mild(row, repeats):
        fs, ref, eref, st = R.partII_case_spiked(feats, pre, sd2, tables.N, tables.P, row, R.MILD)
        ma, mc = _margins(st_base, st)
        assert ma >= 2.0 and mc >= 2.0, (row, ma, mc)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            q = c.partII_forward(*[cu(f) for f in fs], cu(pre)).cpu().numpy()
        assert c.range_status() == (False, False) and c.range_fallbacks == repeats and c.range_repeats["partII"] == repeats, row
        assert _report("PartII fp16x2 M=%d, match %d x %g (margins %.1f / %.1f)" % (M, row, R.MILD, ma, mc), q, ref, eref), row

    for row in rows:
        mild(row, 0)
    for n, row in enumerate(rows):
        fs, ref, eref, st = R.partII_case_spiked(feats, pre, sd2, tables.N, tables.P, row, R.SPIKE)
        assert R.stage_floor({k: st[k] for k in conv}, 0) > 2 * R.COEF_LIMIT
        raw = c.partII_forward(*[cu(f) for f in fs], cu(pre), check_range=False)
        assert c.range_status() == (False, True), row
        keep = torch.ones(M, dtype=torch.bool, device=raw0.device)
        keep[row] = False
        bad = (raw[keep] != raw0[keep]).any(1).nonzero().flatten().tolist()
        assert not bad, (row, bad[:8], len(bad))
        with pytest.warns(RuntimeWarning, match="fp16 range"):
            q = c.partII_forward(*[cu(f) for f in fs], cu(pre)).cpu().numpy()
        assert c.range_fallbacks == n + 1 and c.partII_mode == "fp16x2"
        assert _report("PartII fp16x2 M=%d, match %d x %g (repeated in bf16x3)" % (M, row, R.SPIKE), q, ref, eref), row
    mild(rows[-1], len(rows))
