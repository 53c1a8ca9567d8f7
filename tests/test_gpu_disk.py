"""The Poisson-disk entry on the GPU (-m gpu): yoho_disk_sample against the numpy restatements of its contract (tests/disk_ref.py).
Everything it returns is an integer: state and n_out are compared byte for byte - the final state with the sequential greedy pass, the
rounds that ran and the state of an unfinished call with the synchronous rounds.  The cases are those tests/test_disk_cpu.py holds
the restatements themselves to."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_ref as CL  # noqa: E402
import disk_ref as DR  # noqa: E402
import keypoints_ref as KR  # noqa: E402
import size_plan as SP  # noqa: E402

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOMEM = -1, -4
f32, f64 = np.float32, np.float64


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.Context()


def device_disk(c, pts, radius, seed=0, rounds=DR.MAX_ROUNDS, state=None):
    st, n = c.disk_sample(cu(pts) if isinstance(pts, np.ndarray) else pts, radius, seed=seed, rounds=rounds, state=None if state is None else cu(state))
    assert st.dtype == torch.uint8 and tuple(st.shape) == (len(pts),) and n.dtype == torch.int32 and tuple(n.shape) == (3,)
    return st.cpu().numpy(), n.cpu().numpy()


def check(c, pts, radius, seed=0, what="", greedy=True):
    """device == restatements: the state with the greedy pass (greedy=False: with the rounds and the set's own properties), n_out with
    the rounds -> (state, n_out)"""
    edges = DR.lower_key_edges(pts, radius, seed)
    st = DR.disk_rounds_ref(pts, radius, seed, max_rounds=DR.MAX_ROUNDS, edges=edges)
    assert (st[-1] != 0).all(), what                                                               # the case finishes inside one call
    got, n = device_disk(c, pts, radius, seed)
    want = DR.disk_greedy_ref(pts, radius, seed)["state"] if greedy else st[-1]
    assert got.tobytes() == want.tobytes(), (what, seed, np.nonzero(got != want)[0][:8])
    assert n.tobytes() == DR.n_out_of(st).tobytes(), (what, seed, n, DR.n_out_of(st))
    DR.assert_is_the_set(pts, radius, seed, got, edges)
    return got, n


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 1023, 2049])
def test_disk_sizes_and_densities(ctx, N):
    """a mixed cloud of surface, clumps, duplicates and far points (1e6 r away, and 3e6 r away in the grid's clamped cells) at both
    sides of the block size, at radii that hold about 5 and about 50 neighbours, with two seeds"""
    for target in (5, 50):
        r = DR.radius_for(N, target)
        pts = DR.mixed(N, r)
        a, b = DR.lower_key_edges(pts, r, 0)
        med = float(np.median(np.bincount(np.concatenate([a, b]), minlength=N)))
        print(f"N = {N}, radius {r:.4f}: median {med:.0f} neighbours")
        assert N < 255 or 0.5 * target <= med <= 2 * target
        sets = [check(ctx, pts, r, seed, f"N={N} target={target}")[0] for seed in (0, 12345)]
        assert N < 255 or sets[0].tobytes() != sets[1].tobytes()


# ---- edges ---------------------------------------------------------------------------------------------------------------------------------
def test_the_gate_duplicates_and_non_finite_rows(ctx):
    line = DR.gate_line(300)                                                                       # d2 == gate2: not neighbours
    got, n = check(ctx, line, 0.5, 0, "gate")
    assert (got == 1).all() and n.tolist() == [300, 1, 0]
    r = float(np.nextafter(f32(0.5), f32(1)))
    for seed in (0, 5):
        got, n = check(ctx, line, r, seed, "above the gate")
        assert 100 <= n[0] <= 150 and not (got[1:] == 1)[got[:-1] == 1].any()                     # an alternation: no two in a row
    dup = np.tile(np.array([[0.25, 0.5, 0.75]], f32), (40, 1))
    for seed in (0, 9):
        got, n = check(ctx, dup, 0.1, seed, "duplicates")
        assert np.nonzero(got == 1)[0].tolist() == [int(np.argmin(DR.keys(40, seed)))] and n[0] == 1
    pts = DR.mixed(1023, 0.1)
    bad, good = CL.with_bad_rows(pts)
    rest = np.setdiff1d(np.arange(len(bad)), good)
    got, n = check(ctx, bad, 0.1, 3, "non-finite rows")
    assert (got[rest] == 2).all() and len(rest) > 100
    only_bad = bad[rest]
    got, n = device_disk(ctx, only_bad, 0.1)                                                       # nothing to decide: no round runs
    assert (got == 2).all() and n.tolist() == [0, 0, 0]


# ---- the grid ------------------------------------------------------------------------------------------------------------------------------
def test_where_cells_share_a_bucket_and_in_the_clamped_cells(ctx):
    """100 rows: a table of 256 slots for the 27 cells of a row, two of which mostly share a bucket - the test's own rf_slot
    (tests/test_gpu_clean.py) says for which rows the shared bucket holds a neighbour, met twice by the plain walk; and coordinates
    beyond 2^20 cells, where the outer neighbour of a clamped cell is that cell again and a neighbour is met up to 8 times"""
    from test_gpu_clean import R_FAR, slots27
    rs = np.random.RandomState(41)
    pts = (rs.rand(100, 3) * 0.3 + 0.375).astype(f32)
    s = slots27(pts, 0.1, 100)
    nb = CL.neighbours_ref(pts, 0.1)
    twice = np.array([any((s[i] == s[j, 13]).sum() >= 2 for j in nb[i][0]) for i in range(100)])
    print(f"{int(twice.sum())} of 100 rows meet a neighbour twice")
    assert twice.sum() >= 10
    for seed in (0, 1):
        check(ctx, pts, 0.1, seed, "shared buckets")
    far = (rs.rand(600, 3) * 0.004).astype(f32)
    far[:200] += f32(4000.0)
    far[200:400] -= f32(4000.0)
    far[400:450, 0] += f32(4000.0)                                                                 # clamped on one axis only
    distinct = np.array([len(set(row)) for row in slots27(far, R_FAR, 600).tolist()])
    assert distinct[:400].max() <= 8 and distinct[400:450].max() <= 18
    got, n = check(ctx, far, R_FAR, 0, "beyond the clamp")
    assert 0 < n[0] < 600


def test_the_size_at_which_the_grid_sort_takes_its_later_passes(ctx):
    """tests/size_plan.py's 32 769 targets: three digit passes of the grid's sort.  The greedy pass in numpy would take longer than the
    rest of the file; the state is compared with the synchronous rounds and held to the property that makes the set unique"""
    assert SP.grid_passes(SP.NT_GRID) > SP.grid_passes(SP.NT_GRID - 1)
    pts = SP.cube(SP.NT_GRID, 7)
    got, n = check(ctx, pts, 0.05, 0, "32769", greedy=False)
    assert 1000 < n[0] < 10000 and n[1] <= 16


# ---- the chain -----------------------------------------------------------------------------------------------------------------------------
def test_the_chain_at_64_rounds_a_call_and_at_one(ctx):
    """2049 rows, one decision per round: the first call leaves exactly the restatement's state after round 64, 1985 rows undecided;
    resumed calls finish it inside the bound ceil(N / rounds) + 1 with the greedy set; one round per call gives the same bytes after
    the 64th round and at the end"""
    pts, row_of = DR.chain(2049, 0.05, 0)
    st = DR.disk_rounds_ref(pts, 0.05, 0)
    greedy = DR.disk_greedy_ref(pts, 0.05, 0)["state"]
    assert len(st) - 1 == 2049 and st[-1].tobytes() == greedy.tobytes()
    d = cu(pts)
    state, n = ctx.disk_sample(d, 0.05, seed=0, rounds=64)
    assert state.cpu().numpy().tobytes() == st[64].tobytes() and n.cpu().numpy().tolist() == [32, 64, 1985]
    calls, bound = 1, -(-2049 // 64) + 1
    while int(n[2]) > 0 and calls < bound:                                                         # bounded: never more than `bound` calls
        state, n = ctx.disk_sample(d, 0.05, seed=0, rounds=64, state=state)
        calls += 1
        assert state.cpu().numpy().tobytes() == st[min(64 * calls, 2049)].tobytes(), calls
    assert n.cpu().numpy().tolist() == [1025, 1, 0] and calls == 33 and state.cpu().numpy().tobytes() == greedy.tobytes()
    state, n = ctx.disk_sample(d, 0.05, seed=0, rounds=64, state=state)                            # a finished state: no round runs
    assert n.cpu().numpy().tolist() == [1025, 0, 0] and state.cpu().numpy().tobytes() == greedy.tobytes()
    # one round per call (no host read between the calls)
    one, n1 = ctx.disk_sample(d, 0.05, seed=0, rounds=1)
    for k in range(2, 2050):
        one, n1 = ctx.disk_sample(d, 0.05, seed=0, rounds=1, state=one)
        if k == 64:
            at64, n64 = one.clone(), n1.clone()
    assert at64.cpu().numpy().tobytes() == st[64].tobytes() and n64.cpu().numpy().tolist() == [32, 1, 1985]
    assert one.cpu().numpy().tobytes() == greedy.tobytes() and n1.cpu().numpy().tolist() == [1025, 1, 0]
    # another seed on the same rows: a handful of rounds
    got, n = check(ctx, pts, 0.05, 1, "chain, seed 1")
    assert n[1] <= 16


# ---- independence --------------------------------------------------------------------------------------------------------------------------
def test_bits_repeat_over_poisoned_scratch_streams_and_settings(hip, ctx):
    chain = DR.chain(2049, 0.05, 0)[0]
    cases = [(DR.mixed(1023, 0.1, 1), 0.1, 0, 64), (chain, 0.05, 0, 7), (chain, 0.05, 0, 8), (DR.mixed(257, 0.3, 2), 0.3, 5, 1), (SP.cube(5000, 3), 0.08, 9, 3)]

    def run(c):
        out = []
        for pts, r, seed, rounds in cases:
            d = cu(pts)
            state, n = c.disk_sample(d, r, seed=seed, rounds=rounds)
            out += [state.cpu().numpy().tobytes(), n.cpu().numpy().tobytes()]
            state, n = c.disk_sample(d, r, seed=seed, rounds=rounds, state=state)                  # and one resumed call
            out += [state.cpu().numpy().tobytes(), n.cpu().numpy().tobytes()]
        return out

    first = run(ctx)
    for rep in range(3):
        assert run(ctx) == first, rep
    for k, (pts, r, seed, rounds) in enumerate(cases):                                             # an unfinished call: the rounds' own state
        st = DR.disk_rounds_ref(pts, r, seed, max_rounds=2 * rounds)
        a, b = st[:rounds + 1], st[min(rounds, len(st) - 1):]
        assert first[4 * k:4 * k + 4] == [a[-1].tobytes(), DR.n_out_of(a).tobytes(), b[-1].tobytes(), DR.n_out_of(b).tobytes()], k
    assert any((np.frombuffer(first[4 * k + 2], np.uint8) == 0).any() for k in range(len(cases)))  # some case is unfinished even then
    cx = hip.Context()
    for pat in (0xFFFFFFFF, 0x00000000, 0x01010101):                                               # the last: every byte reads "kept", every counter non-zero
        for rep in range(2):
            cx.poison_scratch(pat)                                                                 # between calls: the workspace holds the pattern
            assert run(cx) == first, (hex(pat), rep)
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


# ---- the C ABI's refusals ------------------------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_arguments(ctx, hip):
    lib = hip.load_library()
    h = ctx._h
    host = np.random.RandomState(3).rand(31, 3).astype(f32)
    q = cu(host)
    state = torch.full((32,), 9, dtype=torch.uint8, device="cuda")
    n_out = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())                              # noqa: E731
    off = lambda x, nbytes: C.c_void_p(x.data_ptr() + nbytes)           # noqa: E731
    N, fl = None, C.c_float
    big = hip.REFINE_MAX_POINTS + 1

    def ds(ctx_=h, pts=p(q), n=31, r=fl(0.2), seed=0, rounds=16, resume=0, st=p(state), n_=p(n_out)):
        return (ctx_, pts, n, r, seed, rounds, resume, st, n_, N)

    rows = [(ds(ctx_=N), "bad argument"), (ds(n=0), "N=0"), (ds(n=-3), "N=-3"), (ds(n=big), "YOHO_REFINE_MAX_POINTS"),
            (ds(r=fl(0.0)), "radius"), (ds(r=fl(-1.0)), "radius"), (ds(r=fl(np.nan)), "radius"), (ds(r=fl(np.inf)), "radius"),
            (ds(rounds=0), "rounds=0"), (ds(rounds=-1), "rounds=-1"), (ds(rounds=65), "YOHO_DISK_MAX_ROUNDS"), (ds(resume=2), "resume=2"), (ds(resume=-1), "resume=-1"),
            (ds(pts=N), "pts is NULL"), (ds(st=N), "state is NULL"), (ds(n_=N), "n_out is NULL"),
            (ds(pts=off(q, 2)), "4-byte aligned"), (ds(n_=off(n_out, 2)), "4-byte aligned")]
    assert hip.DISK_SYMBOLS == ["yoho_disk_sample"]
    for args, text in rows:
        rc = lib.yoho_disk_sample(*args)
        msg = lib.yoho_last_error().decode()
        assert rc == EINVAL, (text, rc, msg)
        assert "yoho_disk_sample" in msg and text in msg, (text, msg)
    torch.cuda.synchronize()
    assert bool((state == 9).all()) and bool((n_out == -7).all())                                  # nothing was launched
    # the context works as before: rows that are not 16-byte aligned, a state at an odd address, outputs inside their rows only
    assert lib.yoho_disk_sample(*ds(pts=off(q, 12), n=30, seed=0xFFFFFFFF, rounds=64, st=off(state, 1), n_=off(n_out, 4))) == 0, lib.yoho_last_error().decode()
    torch.cuda.synchronize()
    st = DR.disk_rounds_ref(host[1:], 0.2, 0xFFFFFFFF)
    assert np.array_equal(state[1:31].cpu().numpy(), st[-1]) and int(state[0]) == 9 and int(state[31]) == 9
    assert np.array_equal(st[-1], DR.disk_greedy_ref(host[1:], 0.2, 0xFFFFFFFF)["state"])
    assert n_out.cpu().numpy().tolist() == [-7] + DR.n_out_of(st).tolist() and 0 < (st[-1] == 1).sum() < 30
    # the binding refuses other shapes before the library sees them
    with pytest.raises(ValueError):
        ctx.disk_sample(q[:, :2], 0.2)
    with pytest.raises(ValueError):
        ctx.disk_sample(q, 0.2, state=torch.zeros(30, dtype=torch.uint8, device="cuda"))
    with pytest.raises(hip.YohoError, match="yoho_disk_sample"):
        ctx.disk_sample(q, 0.2, rounds=0)


CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import disk_ref as DR
from yoho_amd import hip
cx = hip.Context()
rs = np.random.RandomState(0)
big = torch.from_numpy(rs.rand(200000, 3).astype(np.float32)).cuda()
try:
    cx.disk_sample(big, 0.01)
    print("NOT REFUSED")
except hip.YohoError as e:
    print("CODE", e.code, "workspace" in str(e))
small = DR.mixed(300, 0.1)
state, n = cx.disk_sample(torch.from_numpy(small).cuda(), 0.1, seed=4)
ref = DR.disk_greedy_ref(small, 0.1, 4)
print("AFTER", np.array_equal(state.cpu().numpy(), ref["state"]), int(n[0]) == ref["n"], ref["n"])
"""


def test_workspace_refusal_in_a_fresh_process(tmp_path):
    """YOHO_WS_LIMIT_MB=1 in a child process of its own (the limit is read when a context is created): the layout over 200 000 points asks
    for more than 6 MB, the entry returns YOHO_ENOMEM, and the same context then answers 300 points correctly"""
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, YOHO_WS_LIMIT_MB="1")
    r = subprocess.run([sys.executable, str(script), REPO], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert lines[0] == f"CODE {ENOMEM} True", r.stdout
    assert lines[1].startswith("AFTER True True ") and int(lines[1].split()[-1]) > 3, r.stdout


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
def test_select_disk_and_disk_radius_on_the_device(ctx):
    """keypoints.select_disk from the f64 cloud to the cloud indices against the reference selection on a small voxelised cloud; the
    coverage bound on the device; the cap; disk_radius lands at or below the count it is asked for"""
    from yoho_amd import keypoints, synth
    pc = synth.surface_cloud(6000, seed=2)
    pc_d = cu(pc)
    for voxel, radius, seed in ((0.05, 0.12, 0), (None, 0.06, 3)):
        want, kept = DR.select_disk_ref(pc, radius, voxel=voxel, seed=seed)
        got, info = keypoints.select_disk(ctx, pc_d, radius, voxel=voxel, seed=seed)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
        assert info["kept"] == kept > 50 and info["calls"] == 1 and 1 <= info["rounds"] <= 16 and not info["capped"] and info["radius"] == radius
        cut, cinfo = keypoints.select_disk(ctx, pc_d, radius, nkpts=50, voxel=voxel, seed=seed)
        assert np.array_equal(cut.cpu().numpy(), want[:50]) and cinfo["capped"] and cinfo["kept"] == kept
        sel, pts = keypoints.candidates(ctx, pc_d, voxel)
        cov = keypoints.coverage_radius(ctx, pts, cu(pc[want].astype(f32)))
        assert cov < radius and keypoints.coverage_radius(ctx, pts, cu(pc[want[:50]].astype(f32))) > radius
    pts = cu(pc.astype(f32))
    r, rows, info = keypoints.disk_radius(ctx, pts, 300, 0.2)
    assert 270 <= info["kept"] <= 300 and info["radius"] == r
    assert np.array_equal(rows.cpu().numpy(), DR.disk_greedy_ref(pc.astype(f32), r, 0)["kept"])


def test_extractor_in_disk_mode_with_a_stub_backbone():
    """yoho_extractor(keypoints="disk"): the keypoints are the reference selection in key order, nkpts caps them, no draw from the
    global generator; the other modes are what they were (tests/test_gpu_keypoints.py)"""
    from test_gpu_keypoints import StubFCGF, same_state
    from yoho_amd import weights as W
    from yoho_amd.yoho_extract import yoho_extractor
    sd1 = W.synth_state_dict(W.PARTI_SPEC, 7)
    pc = np.random.RandomState(0).rand(3000, 3)
    want, kept = DR.select_disk_ref(pc, 0.11, voxel=0.025, seed=6)
    assert 100 < kept < 1000
    ex = yoho_extractor(yoho_ckpt=sd1, fcgf=StubFCGF(), keypoints="disk", keypoint_radius=0.11, keypoint_seed=6)
    np.random.seed(5)
    state = np.random.get_state()
    kpts, inv, eqv = ex.run(pc, voxel_size=0.025, nkpts=5000)
    assert same_state(state, np.random.get_state())
    assert np.array_equal(kpts, pc[want]) and tuple(inv.shape) == (kept, 32) and tuple(eqv.shape) == (kept, 32, 60)
    k2, i2, e2 = ex.run(pc, voxel_size=0.025, nkpts=100)
    assert np.array_equal(k2, kpts[:100]) and torch.equal(i2, inv[:100]) and torch.equal(e2, eqv[:100])
