"""The salient-keypoint entries on the GPU (-m gpu): yoho_disk_sample_prio and yoho_iss_saliency against the numpy restatements of
their contracts (tests/salient_ref.py).  The thinning returns integers: state and n_out are compared byte for byte, after the final
round, after 1, 2 and 3 rounds, and over split calls.  The saliency: count exactly, every eigenvalue within the bound of the normals
test (the larger of 8 x numpy's own worst error against the same arithmetic at 80 digits and the Weyl figure 4 n 2^-53 trace), and
prio bit for bit from the DEVICE's eig and count.  Small shapes on purpose: a round-kernel workgroup holds 32 rows, a batch 8
candidates, a bucket can end in the middle of a batch."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clean_ref as CR  # noqa: E402
import disk_ref as DR  # noqa: E402
import salient_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOMEM = -1, -4
f32, f64 = np.float32, np.float64
SEEDS = (0, 1, 12345, 0xFFFFFFFF)
CLOUDS = [(300, 0.15, 0), (1500, 0.09, 1), (1500, 0.2, 7)]


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.Context()


def thin(c, d_pts, radius, d_prio, seed, rounds, state=None):
    st, n = c.disk_sample_prio(d_pts, radius, d_prio, seed=seed, rounds=rounds, state=None if state is None else cu(state))
    assert st.dtype == torch.uint8 and tuple(st.shape) == (d_pts.shape[0],) and n.dtype == torch.int32 and tuple(n.shape) == (3,)
    return st.cpu().numpy(), n.cpu().numpy()


def check(c, pts, radius, what, seeds=SEEDS, state0=None):
    """device == disk_prio_rounds_ref for the four kinds of priority and `seeds`: the state and n_out after the final round and after
    1, 2 and 3 rounds, 2 rounds and the rest in a resumed call; with the constant priority the bytes of Context.disk_sample"""
    pts = np.ascontiguousarray(pts, f32)
    n = len(pts)
    pr = SR.pairs(pts, radius)
    d = cu(pts)
    for seed in seeds:
        for name, prio in SR.priorities(n, seed).items():
            tag = (what, name, seed)
            st = SR.disk_prio_rounds_ref(pts, radius, prio, seed, max_rounds=SR.MAX_ROUNDS, state0=state0, pr=pr)
            assert (st[-1] != 0).all(), tag                                                        # the case finishes inside one call
            SR.assert_is_the_set(pts, radius, prio, seed, st[-1], state0=state0, pr=pr)
            dp = cu(prio)
            got, n_out = thin(c, d, radius, dp, seed, SR.MAX_ROUNDS, state0)
            assert got.tobytes() == st[-1].tobytes(), (tag, np.nonzero(got != st[-1])[0][:8])
            assert n_out.tobytes() == DR.n_out_of(st).tobytes(), (tag, n_out, DR.n_out_of(st))
            for k in (1, 2, 3):
                part = st[:k + 1]
                got_k, n_k = thin(c, d, radius, dp, seed, k, state0)
                assert got_k.tobytes() == part[-1].tobytes() and n_k.tobytes() == DR.n_out_of(part).tobytes(), (tag, k, n_k)
                if k == 2:                                                                         # the rest in a resumed call
                    rest = st[len(part) - 1:]
                    got_r, n_r = thin(c, d, radius, dp, seed, SR.MAX_ROUNDS - 2, got_k)
                    assert got_r.tobytes() == st[-1].tobytes() and n_r.tobytes() == DR.n_out_of(rest).tobytes(), (tag, "resumed", n_r)
            if name == "constant" and state0 is None:
                for k in (SR.MAX_ROUNDS, 1, 2, 3):
                    hashed, n_h = c.disk_sample(d, radius, seed=seed, rounds=k)
                    same, n_s = thin(c, d, radius, dp, seed, k)
                    assert hashed.cpu().numpy().tobytes() == same.tobytes() and n_h.cpu().numpy().tobytes() == n_s.tobytes(), (tag, k)


# ---- the thinning ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 31, 32, 33, 257])
def test_thinning_at_ragged_sizes(ctx, N):
    """disk_ref.mixed: surface, clumps, copies of a point and far points in the grid's clamped cells, at both sides of the 32 rows of a
    workgroup, about 12 neighbours per row"""
    r = DR.radius_for(N, 12)
    check(ctx, DR.mixed(N, r), r, f"N={N}")


@pytest.mark.parametrize("n,radius,cloud", CLOUDS)
def test_thinning_on_the_separated_clouds(ctx, n, radius, cloud):
    check(ctx, CR.separated_cloud(cloud, n, radius)[1], radius, f"separated {n} {radius}", seeds=SEEDS if n == 300 else SEEDS[1:3])


def test_thinning_copies_bad_rows_whole_cloud_and_masks(ctx):
    """five copies of every point (d2 = 0: the keys alone decide among them); 3 % rows with a NaN or an infinity; a radius that holds
    the whole cloud at N = 300; and a caller's mask: rows handed in as 2 and as 1, non-finite rows handed in as 0"""
    rs = np.random.RandomState(17)
    base = rs.rand(60, 3).astype(f32)
    check(ctx, np.repeat(base, 5, axis=0)[rs.permutation(300)], 0.2, "copies", seeds=SEEDS[:2])
    bad = DR.mixed(600, 0.1, 3).copy()
    rows = rs.permutation(600)[:18]
    bad[rows, rs.randint(0, 3, 18)] = np.array([np.nan, np.inf, -np.inf], f32)[rs.randint(0, 3, 18)]
    check(ctx, bad, 0.1, "bad rows", seeds=SEEDS[:2])
    check(ctx, rs.rand(300, 3).astype(f32), 2.0, "whole cloud", seeds=SEEDS[:2])
    state0 = rs.choice(np.array([0, 0, 0, 2, 2, 1, 7], np.uint8), 600)                             # the bad rows among them, some handed in as 0
    state0[rows[:5]] = 0
    check(ctx, bad, 0.1, "mask", seeds=SEEDS[:2], state0=state0)
    got, n = thin(ctx, cu(bad), 0.1, cu(np.zeros(600, f32)), 0, 64, state0)
    assert (got[rows][state0[rows] == 0] == 2).all() and (got[state0 == 7] == 7).all() and (got[state0 == 2] == 2).all()


def test_a_monotone_priority_over_resumed_calls(ctx):
    """prio = x on disk_ref.chain(300): one decision per round; the first call leaves the restatement's state after round 64, resumed
    calls finish it; 7 + 9 rounds leave the bytes of 16; keypoints._thin finishes it inside its bound"""
    from yoho_amd import keypoints
    pts, row_of = DR.chain(300, 0.05, 0)
    prio = pts[:, 0].copy()
    st = SR.disk_prio_rounds_ref(pts, 0.05, prio, 0)
    assert len(st) - 1 == 300
    d, dp = cu(pts), cu(prio)
    state, n = thin(ctx, d, 0.05, dp, 0, 64)
    assert state.tobytes() == st[64].tobytes() and n.tolist() == [32, 64, 236]
    a, na = thin(ctx, d, 0.05, dp, 0, 7)
    b, nb = thin(ctx, d, 0.05, dp, 0, 9, a)
    one, n1 = thin(ctx, d, 0.05, dp, 0, 16)
    assert b.tobytes() == one.tobytes() == st[16].tobytes() and na.tolist() == [4, 7, 293] and nb.tolist() == [8, 9, 284] and n1.tolist() == [8, 16, 284]
    rows, info = keypoints._thin(ctx, d, 0.05, 0, "select_salient", prio=dp)
    assert info["rounds"] == 300 and info["calls"] == -(-300 // 16) and info["kept"] == 150
    assert np.array_equal(rows.cpu().numpy(), row_of[::-1][::2])


# ---- independence --------------------------------------------------------------------------------------------------------------------------
def test_bits_repeat_over_poisoned_scratch_streams_and_settings(hip, ctx):
    chain = DR.chain(300, 0.05, 0)[0]
    crease = SR.crease_scene(3000, 3)[0].astype(f32)
    cases = [(DR.mixed(1023, 0.1, 1), 0.1, 0, 64, "special"), (chain, 0.05, 0, 7, None), (DR.mixed(257, 0.3, 2), 0.3, 5, 1, "tied"), (crease, 0.08, 9, 3, "random")]

    def run(c):
        out = []
        for pts, r, seed, rounds, kind in cases:
            d = cu(pts)
            dp = cu(pts[:, 0].copy() if kind is None else SR.priorities(len(pts), seed)[kind])
            state, n = c.disk_sample_prio(d, r, dp, seed=seed, rounds=rounds)
            out += [state.cpu().numpy().tobytes(), n.cpu().numpy().tobytes()]
            state, n = c.disk_sample_prio(d, r, dp, seed=seed, rounds=rounds, state=state)        # and one resumed call
            out += [state.cpu().numpy().tobytes(), n.cpu().numpy().tobytes()]
        prio, count, eig = c.iss_saliency(cu(crease), 0.16, want_eig=True)
        return out + [prio.cpu().numpy().tobytes(), count.cpu().numpy().tobytes(), eig.cpu().numpy().tobytes()]

    first = run(ctx)
    assert run(ctx) == first
    assert any((np.frombuffer(first[4 * k + 2], np.uint8) == 0).any() for k in range(len(cases)))  # some case is unfinished even then
    cx = hip.Context()
    for pat in (0xFFFFFFFF, 0x01010101):                                                           # the last: every byte reads "kept", every counter non-zero
        cx.poison_scratch(pat)                                                                     # between calls: the workspace holds the pattern
        assert run(cx) == first, hex(pat)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream() == side
        assert run(ctx) == first
    torch.cuda.synchronize()
    cs = hip.Context()                                                                             # a context of its own: the settings stay behind
    cs.set_nn_grid(0.0)
    cs.set_nn_prefilter(False)
    assert run(cs) == first
    cs.set_nn_grid(0.3)
    cs.set_nn_prefilter(True)
    assert run(cs) == first


# ---- the saliency ----------------------------------------------------------------------------------------------------------------------------
def saliency(c, pts, radius, **kw):
    prio, count, eig = c.iss_saliency(cu(pts), radius, want_eig=True, **kw)
    assert prio.dtype == torch.float32 and count.dtype == torch.int32 and eig.dtype == torch.float64 and tuple(eig.shape) == (len(pts), 3)
    return prio.cpu().numpy(), count.cpu().numpy(), eig.cpu().numpy()


def check_saliency(c, pts, radius, what, exact=24):
    pts = np.ascontiguousarray(pts, f32)
    ref = SR.saliency_ref(pts, radius)
    prio, count, eig = saliency(c, pts, radius)
    assert np.array_equal(count, ref["count"]), what
    assert (np.diff(eig, axis=1) >= 0).all() and (eig >= 0).all() and not np.signbit(eig).any() and (eig[count == 0] == 0).all()
    rows = np.nonzero(count > 1)[0]
    sample = rows[np.unique(np.linspace(0, rows.size - 1, min(exact, rows.size)).astype(int))]
    ex = [SR.eig_exact(pts, i, radius) for i in sample]
    numpy_worst = max(SR.exact_error(ref["eig"][i, k], e["lam"][k]) for i, e in zip(sample, ex) for k in range(3))
    worst = (0.0, 0.0, 0.0)
    for i, e in zip(sample, ex):
        assert e["count"] == count[i]
        bound = SR.eig_bound(numpy_worst, e["count"], e["trace"])
        for k in range(3):
            err = SR.exact_error(eig[i, k], e["lam"][k])
            worst = max(worst, (err / bound, err, bound))
    bound = np.maximum(8.0 * numpy_worst, 4.0 * ref["count"] * 2.0 ** -53 * ref["trace"])
    diff = np.abs(eig - ref["eig"]).max(axis=1)
    print(f"{what}: {len(pts)} points, neighbours median {int(np.median(count))}; numpy's worst eigenvalue error against the exact ones on {len(sample)} rows "
          f"{numpy_worst:.2e}; device: {worst[1]:.2e} to the exact eigenvalue (bound {worst[2]:.2e}), {diff.max():.2e} to numpy's on all "
          f"(worst ratio to the row's bound {(diff / np.maximum(bound, 1e-300)).max():.3f})")
    assert worst[0] <= 1.0, (what, "to the exact eigenvalues")
    assert (diff <= bound).all(), (what, "to numpy's eigenvalues")
    # prio from the device's own eig and count, bit for bit, NaN pattern included
    med = max(3, int(np.median(count)))
    for g21, g32, mn in ((0.975, 0.975, 5), (0.5, 0.5, 3), (0.975, 0.5, med), (0.5, 0.975, med), (1.0, 1.0, 3)):
        p, cnt2, eig2 = saliency(c, pts, radius, gamma21=g21, gamma32=g32, min_nbrs=mn)
        assert cnt2.tobytes() == count.tobytes() and eig2.tobytes() == eig.tobytes()
        want = SR.prio_of(eig, count, mn, g21, g32)
        assert p.view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), (what, g21, g32, mn)
    p0 = c.iss_saliency(cu(pts), radius)[0].cpu().numpy()                                          # without eig: the same prio
    assert p0.view(np.uint32).tobytes() == prio.view(np.uint32).tobytes()
    return prio, count, eig


@pytest.mark.parametrize("n,radius,cloud", CLOUDS)
def test_saliency_on_the_separated_clouds(ctx, n, radius, cloud):
    """no pair distance lies within 1e-6 relative of the radius: count is exactly the reference's"""
    prio, count, eig = check_saliency(ctx, CR.separated_cloud(cloud, n, radius)[1], radius, f"separated {n} {radius}")
    assert radius < 0.2 or 0 < np.isnan(prio).sum() < n


def test_saliency_on_the_crease_scene_and_degenerate_rows(ctx):
    pts = SR.crease_scene(2000, 4)[0].astype(f32)
    prio, count, eig = check_saliency(ctx, pts, 0.16, "crease scene")
    dist = SR.crease_distance(pts)
    near, far = np.nanmedian(prio[dist < 0.03]), np.nanmedian(prio[dist > 0.16])
    print(f"median response within 0.03 of a crease {near:.2e}, beyond 0.16 {far:.2e}")
    assert near > 10 * far                                                                         # the response is the creases'
    # rows with count 0, an isolated row, copies of one point (l3 = 0) and exactly collinear neighbours (l1 = l2 = 0): all ineligible
    dup = np.tile(np.array([[0.25, 0.5, 0.75]], f32), (40, 1))
    line = np.zeros((40, 3), f32)
    line[:, 0] = 2.0 + np.arange(40) * f32(0.015625)
    line[:, 1], line[:, 2] = f32(0.5), f32(-0.25)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [5.0, 5.0, 5.0]], f32)
    deg = np.concatenate([dup, line, bad])
    p, cnt, e = saliency(ctx, deg, 0.1, min_nbrs=3, gamma21=1.0, gamma32=1.0)
    assert (cnt[:40] == 40).all() and (e[:40] == 0).all()
    assert (cnt[40:80] >= 7).all() and (e[40:80, :2] == 0).all() and (e[40:80, 2] > 0).all()
    assert cnt[80:].tolist() == [0, 0, 0, 1] and (e[80:] == 0).all()
    assert (p.view(np.uint32) == SR.QNAN).all()
    ref = SR.saliency_ref(deg, 0.1)
    assert np.array_equal(cnt, ref["count"]) and np.abs(e - ref["eig"]).max() <= 4 * 13 * 2.0 ** -53 * ref["trace"].max()


# ---- composition ---------------------------------------------------------------------------------------------------------------------------
def test_select_salient_equals_the_reference_thinning_of_the_device_priorities(ctx):
    """keypoints.select_salient on the crease scene from the f64 cloud to the cloud indices: the reference thinning (tests/test_salient_cpu.py
    select_salient_ref) of the DEVICE's own prio, for "greedy" with fill both ways, "nms" and tiers = 8, with the default gammas and
    with gamma21 = 0.7, where half the rows are ineligible"""
    from test_salient_cpu import select_salient_ref
    from yoho_amd import keypoints
    pc = SR.crease_scene(2500, 1)[0]
    pc_d = cu(pc)
    radius = 0.08
    for g21, seed in ((0.975, 0), (0.7, 5)):
        prio = ctx.iss_saliency(cu(pc.astype(f32)), 2 * radius, gamma21=g21)[0].cpu().numpy()
        eligible = int((~np.isnan(prio)).sum())
        for kw in ({}, {"fill": False}, {"mode": "nms"}, {"tiers": 8}, {"tiers": None}):
            got, info = keypoints.select_salient(ctx, pc_d, radius, seed=seed, gamma21=g21, **kw)
            want, _ = select_salient_ref(pc, radius, prio, seed=seed, **kw)
            assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want), (g21, kw)
            assert info["kept"] == len(want) > 20 and info["eligible"] == eligible and info["mode"] == kw.get("mode", "greedy") and info["tiers"] == kw.get("tiers", None if kw.get("mode") == "nms" else keypoints.SALIENT_DEFAULT_TIERS)
            print(f"gamma21 {g21}, {kw}: {eligible} of {len(pc)} eligible, {info['kept']} kept in {info['rounds']} rounds and {info['calls']} calls")
        cut, cinfo = keypoints.select_salient(ctx, pc_d, radius, seed=seed, gamma21=g21, nkpts=25)
        assert np.array_equal(cut.cpu().numpy(), select_salient_ref(pc, radius, prio, seed=seed)[0][:25]) and cinfo["capped"]
        sel, pts = keypoints.candidates(ctx, pc_d, None)
        full = keypoints.select_salient(ctx, pc_d, radius, seed=seed, gamma21=g21)[0]
        assert keypoints.coverage_radius(ctx, pts, pts[full].contiguous()) < radius               # fill=True: select_disk's bound


# ---- the C ABI's refusals ------------------------------------------------------------------------------------------------------------------
def test_entries_refuse_bad_arguments(ctx, hip):
    lib = hip.load_library()
    h = ctx._h
    host = np.random.RandomState(3).rand(31, 3).astype(f32)
    q = cu(host)
    prio = cu(np.random.RandomState(4).rand(32).astype(f32))
    state = torch.full((32,), 9, dtype=torch.uint8, device="cuda")
    n_out = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    count = torch.full((32,), -7, dtype=torch.int32, device="cuda")
    eig = torch.full((32, 3), -7.0, dtype=torch.float64, device="cuda")
    out = torch.full((32,), -7.0, dtype=torch.float32, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())                              # noqa: E731
    off = lambda x, nbytes: C.c_void_p(x.data_ptr() + nbytes)           # noqa: E731
    N, fl, db = None, C.c_float, C.c_double
    big = hip.REFINE_MAX_POINTS + 1

    def ds(ctx_=h, pts=p(q), n=31, r=fl(0.2), pr=p(prio), seed=0, rounds=16, resume=0, st=p(state), n_=p(n_out)):
        return (ctx_, pts, n, r, pr, seed, rounds, resume, st, n_, N)

    rows = [(ds(ctx_=N), "bad argument"), (ds(n=0), "N=0"), (ds(n=-3), "N=-3"), (ds(n=big), "YOHO_REFINE_MAX_POINTS"),
            (ds(r=fl(0.0)), "radius"), (ds(r=fl(-1.0)), "radius"), (ds(r=fl(np.nan)), "radius"), (ds(r=fl(np.inf)), "radius"),
            (ds(rounds=0), "rounds=0"), (ds(rounds=65), "YOHO_SALIENT_MAX_ROUNDS"), (ds(resume=2), "resume=2"), (ds(resume=-1), "resume=-1"),
            (ds(pts=N), "pts is NULL"), (ds(pr=N), "prio is NULL"), (ds(st=N), "state is NULL"), (ds(n_=N), "n_out is NULL"),
            (ds(pts=off(q, 2)), "4-byte aligned"), (ds(pr=off(prio, 2)), "4-byte aligned"), (ds(n_=off(n_out, 2)), "4-byte aligned")]
    for args, text in rows:
        rc = lib.yoho_disk_sample_prio(*args)
        msg = lib.yoho_last_error().decode()
        assert rc == EINVAL, (text, rc, msg)
        assert "yoho_disk_sample_prio" in msg and text in msg, (text, msg)

    def sa(ctx_=h, pts=p(q), n=31, r=fl(0.2), mn=3, g21=db(0.975), g32=db(0.975), cnt=p(count), e=p(eig), pr=p(out)):
        return (ctx_, pts, n, r, mn, g21, g32, cnt, e, pr, N)

    rows = [(sa(ctx_=N), "bad argument"), (sa(n=0), "N=0"), (sa(n=big), "YOHO_REFINE_MAX_POINTS"), (sa(r=fl(0.0)), "radius"), (sa(r=fl(np.nan)), "radius"),
            (sa(r=fl(np.inf)), "radius"), (sa(mn=2), "min_nbrs=2"), (sa(g21=db(0.0)), "gamma21"), (sa(g21=db(1.5)), "gamma21"), (sa(g21=db(np.nan)), "gamma21"),
            (sa(g32=db(0.0)), "gamma32"), (sa(g32=db(1.5)), "gamma32"), (sa(g32=db(np.nan)), "gamma32"), (sa(g32=db(-0.5)), "gamma32"),
            (sa(pts=N), "pts is NULL"), (sa(cnt=N), "count is NULL"), (sa(pr=N), "prio is NULL"),
            (sa(pts=off(q, 2)), "4-byte aligned"), (sa(cnt=off(count, 2)), "4-byte aligned"), (sa(pr=off(out, 2)), "4-byte aligned"), (sa(e=off(eig, 4)), "8-byte aligned")]
    for args, text in rows:
        rc = lib.yoho_iss_saliency(*args)
        msg = lib.yoho_last_error().decode()
        assert rc == EINVAL, (text, rc, msg)
        assert "yoho_iss_saliency" in msg and text in msg, (text, msg)
    torch.cuda.synchronize()
    assert bool((state == 9).all()) and bool((n_out == -7).all()) and bool((count == -7).all()) and bool((eig == -7).all()) and bool((out == -7).all())
    # the contexts work as before: rows that are not 16-byte aligned, a state at an odd address, outputs inside their rows only
    assert lib.yoho_disk_sample_prio(*ds(pts=off(q, 12), n=30, pr=off(prio, 4), seed=0xFFFFFFFF, rounds=64, st=off(state, 1), n_=off(n_out, 4))) == 0, lib.yoho_last_error().decode()
    assert lib.yoho_iss_saliency(*sa(pts=off(q, 12), n=30, r=fl(0.3), cnt=off(count, 4), e=N, pr=off(out, 4))) == 0, lib.yoho_last_error().decode()
    torch.cuda.synchronize()
    hp = prio.cpu().numpy()
    st = SR.disk_prio_rounds_ref(host[1:], 0.2, hp[1:31], 0xFFFFFFFF)
    assert np.array_equal(state[1:31].cpu().numpy(), st[-1]) and int(state[0]) == 9 and int(state[31]) == 9
    assert n_out.cpu().numpy().tolist() == [-7] + DR.n_out_of(st).tolist() and 0 < (st[-1] == 1).sum() < 30
    ref = SR.saliency_ref(host[1:], 0.3)
    assert np.array_equal(count[1:31].cpu().numpy(), ref["count"]) and int(count[0]) == -7 and int(count[31]) == -7 and bool((eig == -7).all())
    assert float(out[0]) == -7 and float(out[31]) == -7 and not bool((out[1:31] == -7).any())
    # the bindings refuse other shapes before the library sees them
    with pytest.raises(ValueError):
        ctx.disk_sample_prio(q[:, :2], 0.2, prio[:31])
    with pytest.raises(ValueError):
        ctx.disk_sample_prio(q, 0.2, prio)
    with pytest.raises(ValueError):
        ctx.disk_sample_prio(q, 0.2, prio[:31].contiguous(), state=torch.zeros(30, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        ctx.iss_saliency(q[:, :2], 0.2)
    with pytest.raises(hip.YohoError, match="yoho_disk_sample_prio"):
        ctx.disk_sample_prio(q, 0.2, prio[:31].contiguous(), rounds=0)
    with pytest.raises(hip.YohoError, match="yoho_iss_saliency"):
        ctx.iss_saliency(q, 0.2, min_nbrs=2)


CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import disk_ref as DR, salient_ref as SR
from yoho_amd import hip
cx = hip.Context()
rs = np.random.RandomState(0)
big = torch.from_numpy(rs.rand(200000, 3).astype(np.float32)).cuda()
for call in (lambda: cx.disk_sample_prio(big, 0.01, big[:, 0].contiguous()), lambda: cx.iss_saliency(big, 0.01)):
    try:
        call()
        print("NOT REFUSED")
    except hip.YohoError as e:
        print("CODE", e.code, "workspace" in str(e))
small = DR.mixed(300, 0.1)
prio = SR.priorities(300, 4)["random"]
state, n = cx.disk_sample_prio(torch.from_numpy(small).cuda(), 0.1, torch.from_numpy(prio).cuda(), seed=4)
ref = SR.disk_prio_greedy_ref(small, 0.1, prio, 4)
count = cx.iss_saliency(torch.from_numpy(small).cuda(), 0.1)[1]
print("AFTER", np.array_equal(state.cpu().numpy(), ref["state"]), int(n[0]) == ref["n"], np.array_equal(count.cpu().numpy(), SR.saliency_ref(small, 0.1)["count"]), ref["n"])
"""


def test_workspace_refusal_in_a_fresh_process(tmp_path):
    """YOHO_WS_LIMIT_MB=1 in a child process of its own (the limit is read when a context is created): the layouts over 200 000 points
    ask for more than 1 MB, both entries return YOHO_ENOMEM, and the same context then answers 300 points correctly"""
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, YOHO_WS_LIMIT_MB="1")
    r = subprocess.run([sys.executable, str(script), REPO], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[0] == f"CODE {ENOMEM} True" and lines[1] == f"CODE {ENOMEM} True", r.stdout
    assert lines[2].startswith("AFTER True True True ") and int(lines[2].split()[-1]) > 3, r.stdout
