"""The float64 reference of tests/ref64.py and the error budget built on it, checked on the CPU: the reference is pinned to the fp32
oracle and to the golden vectors captured from the reference run, and the comparison the GPU tests use (ref64.within_budget, 12 x the fp32
oracle's own distance from float64) REJECTS results that carry the defects a ring-loop or epilogue rewrite of the split-MFMA kernels
produces - a correction product gone from a layer, gone from one irrep only, one keypoint slightly off - while it accepts the fp32
oracle.  The asserted 1e-4 of the parity tests lets all of those through (figures in profiles/precision.md)."""
import numpy as np
import pytest

import ref64 as R
from ref64 import orc

FEW = 4.0        # "a few e_ref": two honest fp32 evaluations of one function are each within ~1 e_ref of float64, hence within 2 of each other


@pytest.fixture(scope="module")
def golden_partI(gold, sd1, tables):
    g = gold("partI.npz")
    ref, eref, _ = R.partI_case(g["x"], sd1, tables.N)
    return g, ref, eref


def test_ref64_pins_partI_oracle_and_golden(golden_partI, sd1, tables):
    g, ref, eref = golden_partI
    assert ref[0].dtype == np.float64 and ref[1].dtype == np.float64
    assert 1e-7 < eref < 1e-6                                   # fp32 rounding through four layers, not more and not nothing
    o = orc.partI_forward(g["x"], sd1, tables.N)
    r32 = tuple(a.astype(np.float32) for a in ref)
    vs_oracle = max(R.errors(r32, tuple(a.astype(np.float64) for a in o))) / eref
    vs_golden = max(R.errors(r32, (g["eqv"].astype(np.float64), g["inv"].astype(np.float64)))) / eref
    print("PartI: e_ref %.3g; float64 rounded to fp32 vs oracle %.2f e_ref, vs golden %.2f e_ref" % (eref, vs_oracle, vs_golden))
    assert vs_oracle < FEW and vs_golden < FEW
    assert R.within_budget((g["eqv"], g["inv"]), ref, eref, factor=FEW)[0]


def _chain_inputs(gold, sd1, tables):
    from yoho_amd import synth
    g = gold("chain.npz")
    pr = synth.make_pair(int(g["K"]), seed=int(g["pair_seed"]))
    e0 = orc.partI_extract(pr["feat0"], sd1, tables.N, batch=40)
    e1 = orc.partI_extract(pr["feat1"], sd1, tables.N, batch=40)
    m, dr = g["match"], g["dr_index"]
    b = orc.batch_create(pr["feat0"][m[:, 0]], pr["feat1"][m[:, 1]], e0[m[:, 0]], e1[m[:, 1]], dr)
    return g, [b[k] for k in ("before_eqv0", "before_eqv1", "after_eqv0", "after_eqv1")], dr


def test_ref64_pins_partII_oracle_and_golden(gold, sd1, sd2, tables):
    g, args, dr = _chain_inputs(gold, sd1, tables)
    keep = [a.copy() for a in args]
    q64, eref, st = R.partII_case(*args, dr, sd2, tables.N, tables.P)
    assert all(np.array_equal(a, k) for a, k in zip(args, keep)), "inputs must not be modified"
    assert q64.dtype == np.float64 and set(st) == {"a_in", "h0", "a0", "mid", "a1", "h2", "t1", "t2", "q"}
    assert 1e-7 < eref < 1e-5
    qo = orc.partII_forward(*args, dr, sd2, tables.N, tables.P)
    vs_oracle = max(R.errors(q64.astype(np.float32), qo.astype(np.float64))) / eref
    vs_golden = max(R.errors(q64[:16].astype(np.float32), g["quat16"].astype(np.float64))) / eref
    print("PartII: e_ref %.3g; float64 rounded to fp32 vs oracle %.2f e_ref, vs golden %.2f e_ref" % (eref, vs_oracle, vs_golden))
    assert vs_oracle < FEW and vs_golden < FEW
    assert np.allclose(np.sum(q64 * q64, axis=1), 1.0, rtol=0, atol=1e-14)


def test_ref64_rows_are_independent_and_results_are_cached(sd1, tables):
    """what partI_case_spiked relies on (a row's float64 value does not depend on its batch, here across the 64-row chunks of the
    matmul), and the module cache: one evaluation per (state dict, input), none for a pass with a hook, results read-only"""
    x = R.partI_input(70)
    eqv, inv, st = R.partI_forward64(x, sd1, tables.N, stages=True)
    assert set(st) == {"h0", "a0", "mid", "a1", "h2", "a2", "y"} and st["mid"].shape == (70, 512, 60)
    for r in (0, 63, 64, 69):
        e1, i1 = R.partI_forward64(x[r:r + 1], sd1, tables.N)
        assert np.abs(e1[0] - eqv[r]).max() < 1e-13 and np.abs(i1[0] - inv[r]).max() < 1e-13
    assert R.partI_forward64(x.copy(), dict(sd1), tables.N)[0] is eqv            # same contents, same entry
    assert R.partI_forward64(x, sd1, tables.N, hook=lambda n, t: t)[0] is not eqv
    with pytest.raises(ValueError):
        eqv[0, 0, 0] = 0.0
    xs, ref, eref, st1 = R.partI_case_spiked(x, sd1, tables.N, 64, 3.0)
    full = R.partI_forward64(xs, sd1, tables.N)
    assert np.abs(ref[0] - full[0]).max() < 1e-13 and np.abs(ref[1] - full[1]).max() < 1e-13 and np.array_equal(xs[:64], x[:64])
    o_full, o_base = R.oracle_partI(xs, sd1, tables.N), R.oracle_partI(x, sd1, tables.N)
    assert np.array_equal(o_full[0][:64], o_base[0][:64]) and 0.0 < eref < 1e-6       # the spliced fp32 oracle is the fp32 oracle


# ---- mutation checks: the comparison of the GPU tests rejects subtly wrong kernels -------------------------------------------------
PARTI_MUTANTS = {
    "fp16 low plane lost before GEMM 1 (256->512)": R.drop_low_plane("a0"),
    "the same on the trivial irrep only": R.drop_low_plane_trivial_irrep("a0"),
    "one keypoint of the last layer off by 1e-3": None,                     # needs the row: made per case below
    "fp16 low plane lost before GEMM 2 (512->256)": R.drop_low_plane("a1"),
    "the same on the trivial irrep only (GEMM 2)": R.drop_low_plane_trivial_irrep("a1"),
    "fp16 low plane of the residual lost": R.drop_low_plane("h0"),
    "one keypoint of the 512->256 layer off by 3e-4": None,
}
TABLED = list(PARTI_MUTANTS)[:3]


def _partI_mutant(name, B):
    if name.startswith("one keypoint of the last layer"):
        return R.scale_row("y", B - 1, 1.0 + 1e-3)
    if name.startswith("one keypoint of the 512"):
        return R.scale_row("h2", B // 2, 1.0 + 3e-4)
    return PARTI_MUTANTS[name]


@pytest.mark.parametrize("sdname,B,names", [("seed7", 33, TABLED), ("seed7", 1, list(PARTI_MUTANTS)), ("bias30", 2, list(PARTI_MUTANTS)),
                                             ("seed23", 2, TABLED)])
def test_partI_budget_rejects_mutants_and_accepts_the_oracle(tables, sdname, B, names):
    sd = R.partI_state_dict(sdname)
    x = R.partI_input(B)
    ref, eref, _ = R.partI_case(x, sd, tables.N)
    ok, worst = R.within_budget(R.oracle_partI(x, sd, tables.N), ref, eref)
    assert ok and worst <= 1.0 + 1e-12
    ok, _ = R.within_budget(tuple(a.astype(np.float32) for a in ref), ref, eref)
    assert ok
    for name in names:
        got = R.partI_forward64(x, sd, tables.N, hook=_partI_mutant(name, B))
        ok, worst = R.within_budget(got, ref, eref)
        print("PartI %s B=%d, %s: %.1f e_ref (rel eqv %.2g), budget %g" % (sdname, B, name, worst, R.errors(got, ref)[0], R.FACTOR))
        assert not ok, (name, worst)
    bad = [a.astype(np.float32) for a in ref]
    bad[0][B - 1, 3, 7] = np.nan
    assert R.within_budget(tuple(bad), ref, eref) == (False, float("inf"))


def test_partII_budget_rejects_mutants_and_accepts_the_oracle(sd2, tables):
    M = 17
    feats, pre = R.partII_input(M)
    q64, eref, _ = R.partII_case(*feats, pre, sd2, tables.N, tables.P)
    assert R.within_budget(R.oracle_partII(*feats, pre, sd2, tables.N, tables.P), q64, eref)[0]
    for name, hk in (("fp16 low plane lost before the first layer", R.drop_low_plane("a_in")),
                     ("the same on the trivial irrep only", R.drop_low_plane_trivial_irrep("a_in")),
                     ("fp16 low plane lost before the cone layer", R.drop_low_plane("a1")),
                     ("one match of the head off by 1e-3", R.scale_row("t2", M - 1, 1.0 + 1e-3))):
        got = R.partII_forward64(*feats, pre, sd2, tables.N, tables.P, hook=hk)
        ok, worst = R.within_budget(got, q64, eref)
        print("PartII M=%d, %s: %.1f e_ref, budget %g" % (M, name, worst, R.FACTOR))
        assert not ok, (name, worst)


# ---- the spiked inputs of the range tests do what those tests assume -----------------------------------------------------------------
def test_spiked_rows_leave_the_fp16_range_and_mild_ones_stay_inside(sd1, sd2, tables):
    """one row times SPIKE: every float64 stage of that row exceeds 4.5e4 in PartI, twice the larger limit in PartII's group-conv layers
    (limits: 4094 for activations, 16376 for coefficients); times
    MILD: the stage maxima and the bound on the coefficients stay a factor 2 under both limits.  The GPU tests assert the same from
    their own stage tensors; here it is checked without a device, for every position they use."""
    for B in R.PARTI_SPIKE_B:
        x = R.partI_input(B)
        for row in R.spike_rows(B):
            for f in (R.SPIKE, R.MILD):
                (xs,) = R.spike([x], row, f)
                _, _, st = R.partI_case(xs[row:row + 1], sd1, tables.N)
                amax, cmax = R.stage_extent(st)
                if f == R.SPIKE:
                    assert R.stage_floor(st, 0) > 4.5e4, (B, row)
                else:
                    assert 2 * amax < R.ACT_LIMIT and 2 * cmax < R.COEF_LIMIT and amax > 10.0, (B, row, amax, cmax)
    feats, pre = R.partII_input(R.PARTII_SPIKE_M)
    for row in (0, 127, 128, R.PARTII_SPIKE_M - 1):
        for f in (R.SPIKE, R.MILD):
            one = [a[row:row + 1] for a in R.spike(feats, row, f)]
            _, _, st = R.partII_case(*one, pre[row:row + 1], sd2, tables.N, tables.P)
            amax, cmax = R.stage_extent(st)
            if f == R.SPIKE:
                assert R.stage_floor({k: st[k] for k in ("a_in", "h0", "a0", "mid", "a1", "h2")}, 0) > 2 * R.COEF_LIMIT, row
            else:
                assert 2 * amax < R.ACT_LIMIT and 2 * cmax < R.COEF_LIMIT and amax > 10.0, (row, amax, cmax)


# ---- one stage, one channel outside: the rescaled networks and the plan of tests/test_gpu_range_stages.py -----------------------------
def _sd_of(net, sd1, sd2):
    return sd1 if net == "partI" else sd2


def test_range_stage_cases_are_all_admissible(sd1, sd2, tables):
    """every (network, stage, channel, row, B) the GPU tests use has a power of two s with all four float64 margins >= 2 - nothing is
    decided at run time there - and the table holds every mode, stage, channel slot and row the GPU file is to exercise"""
    cases = R.range_stage_cases()
    assert len(cases) == len(set(cases))
    assert R.partI_state_dict("seed7").keys() == sd1.keys()
    have = {(net, mode, stage) for net, mode, stage, *_ in cases}
    want = {("partI", m, s) for m in ("fgemm", "fgemm256", "fgemm128") for s in ("a0", "mid", "a1", "h2", "a2", "y")}
    want |= {("partI", "fp16x2", s) for s in ("a0", "a1", "a2")} | {("partI", "fgemm8", s) for s in ("mid", "h2")}
    want |= {("partII", m, s) for m in ("fp16x2", "cgemm") for s in ("a_in", "a0", "mid", "a1", "h2")}
    assert have == want
    for stage, cout in (("mid", 512), ("h2", 256)):
        got = {o for net, mode, st, o, B, row in cases if (net, mode, st, B, row) == ("partI", "fgemm", stage, 33, 16)}
        for o in (0, 3, 4, 7, 8, 15, 16, 127, 128, 255, cout - 1):
            assert any(g % 16 == o % 16 and (g == o or ("partI", stage, 33, 16, o) in R.CHANNEL_SUBST) for g in got), (stage, o)
        rows = {(B, row) for net, mode, st, o, B, row in cases if (net, mode, st) == ("partI", "fgemm", stage)}
        assert rows >= {(33, r) for r in (0, 15, 16, 31, 32)} | {(257, r) for r in (127, 128, 255, 256)}
    for k, o in R.CHANNEL_SUBST.items():
        assert o % 16 == k[4] % 16
    seen = set()
    for net, mode, stage, o, B, row in cases:
        key = (net, stage, o, B, row)
        if key in seen:
            continue
        seen.add(key)
        assert 0 <= o < R.STAGE_COUT[net][stage] and 0 <= row < B
        p = R.range_stage_plan(net, stage, o, B, row, _sd_of(net, sd1, sd2), tables.N, tables.P)
        assert p is not None, key
        m = p["margins"]
        print("%-6s %-4s o=%3d B=%3d row=%3d  s=2^%-2d  out %.2f  base %.2f  twin %.2f  rest %.2f"
              % (net, stage, o, B, row, int(np.log2(p["s"])), m["out"], m["base"], m["twin"], m["rest"]))
        assert min(m.values()) >= 2.0, (key, m)


EXACT = [("partI", s) for s in ("a0", "mid", "a1", "a2", "y")] + [("partII", s) for s in ("a_in", "a0", "mid", "a1")]


def _two_rows(net, sd, tables):
    """-> f(state dict) = (outputs, stages, fp32 oracle outputs) of rows 16 (times MILD) and 17 of the 33-row inputs"""
    if net == "partI":
        x = R.spike([R.partI_input(33)], 16, R.MILD)[0][16:18]
        return lambda d: (R.partI_forward64(x, d, tables.N, stages=True)[:2], R.partI_forward64(x, d, tables.N, stages=True)[2],
                          R.oracle_partI(x, d, tables.N))
    feats, pre = R.partII_input(33)
    fs = [a[16:18] for a in R.spike(feats, 16, R.MILD)]
    return lambda d: ((R.partII_forward64(*fs, pre[16:18], d, tables.N, tables.P),), R.partII_forward64(*fs, pre[16:18], d, tables.N, tables.P, stages=True)[1],
                      (R.oracle_partII(*fs, pre[16:18], d, tables.N, tables.P),))


@pytest.mark.parametrize("net,stage", EXACT)
def test_rescaled_network_is_the_base_network_but_for_one_channel(sd1, sd2, tables, net, stage):
    """every float64 stage tensor of the rescaled network equals the base network's to 1e-12, stage S channel o is s times the base
    bit for bit, and the fp32 oracle gives the same bits under both state dicts (a power of two commutes with its roundings too): the
    GPU tests reuse the base batch's float64 pass and its e_ref.  y has no consumer: there the outputs differ and are not compared.
    The helper returns copies and leaves its input alone."""
    sd = _sd_of(net, sd1, sd2)
    o, s = 7, 1024.0
    keep = {k: v.copy() for k, v in sd.items()}
    sd_r = R.rescale_stage(sd, net, stage, o, s)
    assert all(np.array_equal(sd[k], keep[k]) for k in keep) and sd_r.keys() == sd.keys()
    assert not any(np.shares_memory(sd_r[k], sd[k]) for k in sd)
    changed = sorted(k for k in sd if not np.array_equal(sd_r[k], sd[k]))
    assert len(changed) == (2 if stage == "y" else (4 if R.stage_kind(net, stage) == "conv" else 3)), changed
    run = _two_rows(net, sd, tables)
    (out0, st0, orc0), (out1, st1, orc1) = run(sd), run(sd_r)
    for k in st0:
        a, b = st0[k], st1[k]
        if k == stage:
            assert np.array_equal(b[:, o], s * a[:, o]) and np.abs(a[:, o]).max() > 0
            a, b = np.delete(a, o, axis=1), np.delete(b, o, axis=1)
        if stage == "y":
            continue
        assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max(), (stage, k)
    via = R.rescaled_stages(net, st0, sd_r, stage, o, s, tables.N)
    assert all(np.array_equal(via[k], st1[k]) if k == stage else via[k] is st0[k] for k in st0)
    if stage != "y":
        for a, b in zip(out0, out1):
            assert np.abs(a - b).max() <= 1e-12
        for a, b in zip(orc0, orc1):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("net", ("partI", "partII"))
def test_rescaled_h2_tail_is_the_full_pass(sd1, sd2, tables, net):
    """h2 carries the unscaled residual: the rescaled network is one of its own.  rescaled_stages evaluates its tail from the base
    stages (what the 257-row cases plan with); here against the full float64 pass under the rescaled state dict."""
    sd = _sd_of(net, sd1, sd2)
    o, s = 8, 512.0
    sd_r = R.rescale_stage(sd, net, "h2", o, s)
    run = _two_rows(net, sd, tables)
    st0, st1 = run(sd)[1], run(sd_r)[1]
    via = R.rescaled_stages(net, st0, sd_r, "h2", o, s, tables.N)
    assert via.keys() == st1.keys()
    for k in st1:
        assert np.abs(via[k] - st1[k]).max() <= 1e-12 * np.abs(st1[k]).max(), k
    res = st1["h2"][:, o] - s * (st0["h2"][:, o] - st0["h0"][:, o])
    assert np.abs(res - st0["h0"][:, o]).max() <= 1e-9 * np.abs(st1["h2"][:, o]).max()        # s x the conv + the residual as it was
