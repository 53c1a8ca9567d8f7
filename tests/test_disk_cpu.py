"""CPU tests of the Poisson-disk thinning (include/yoho_disk.h, yoho_amd/keypoints.py select_disk / disk_radius): the
library builds and exports exactly the header's symbol and its kernels compile without scratch; the two numpy restatements of the
entry (tests/disk_ref.py), which share no code, agree on separated clouds; the restatement at the contract's edges and on the
adversarial chain; the motivating case - the coverage of farthest-point sampling at the same count, in a dozen rounds, and why the
priority is hashed -; and the Python layer over a host context built from the restatement: without the new arguments it does what it
did."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(REPO, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(REPO, "tests"))
import clean_ref as CR  # noqa: E402
import cluster_ref as CL  # noqa: E402
import disk_ref as DR  # noqa: E402
import keypoints_ref as KR  # noqa: E402

f32, f64 = np.float32, np.float64
# dk_init_kernel and dk_round_kernel are templates over the key policy: the hashed key of yoho_disk_sample, the stored key64 of yoho_disk_sample_prio
KERNELS = {"dk_zero_kernel": 1, "dk_init_kernel": 2, "dk_round_kernel": 2, "dk_tail_kernel": 1}
OLDER = ("yoho_hip.h", "yoho_knn.h", "yoho_trainset.h", "yoho_refine.h", "yoho_plane.h", "yoho_verify.h", "yoho_consist.h", "yoho_keypoints.h",
         "yoho_multiway.h", "yoho_fuse.h", "yoho_clean.h", "yoho_cluster.h")


# ---- the library ---------------------------------------------------------------------------------------------------------------------------
def test_library_exports_disk_header_symbol():
    """include/yoho_disk.h declares exactly hip.DISK_SYMBOLS, the library exports it with its 10 arguments, the list shares nothing
    with the other twelve, which are what they were, and nothing leaked into the older headers; the header states the mixer and
    vectors of it that tests/disk_ref.py's two restatements of it reproduce"""
    import ctypes as C
    from yoho_amd import build, hip
    assert os.path.exists(build.build(verbose=False))
    lib = hip.load_library()
    hdr = open(os.path.join(REPO, "include", "yoho_disk.h")).read()
    fns = sorted(set(re.findall(r"\b(yoho_[a-zA-Z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert fns == ["yoho_disk_sample"] and hip.DISK_SYMBOLS == fns
    at = lib.yoho_disk_sample.argtypes
    assert lib.yoho_disk_sample.restype is C.c_int and len(at) == 10
    assert at[2] is C.c_int and at[3] is C.c_float and at[4] is C.c_uint32 and at[5] is C.c_int and at[6] is C.c_int
    others = (hip.SYMBOLS + hip.KNN_SYMBOLS + hip.TRAINSET_SYMBOLS + hip.REFINE_SYMBOLS + hip.PLANE_SYMBOLS + hip.VERIFY_SYMBOLS + hip.CONSIST_SYMBOLS +
              hip.KEYPOINT_SYMBOLS + hip.MULTIWAY_SYMBOLS + hip.FUSE_SYMBOLS + hip.CLEAN_SYMBOLS + hip.CLUSTER_SYMBOLS)
    assert not set(fns) & set(others)
    assert hip.KEYPOINT_SYMBOLS == ["yoho_fps"] and hip.CLUSTER_SYMBOLS == ["yoho_dbscan"] and hip.CLEAN_SYMBOLS == ["yoho_knn_within", "yoho_statistical_outliers"]
    main = open(os.path.join(REPO, "include", "yoho_hip.h")).read()
    main_fns = set(re.findall(r"\b(yoho_[a-zA-Z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", main, flags=re.S)))
    assert main_fns == set(hip.SYMBOLS)                                                          # unchanged by the new entry
    for older in OLDER:
        text = open(os.path.join(REPO, "include", older)).read()
        assert "yoho_disk" not in text and "YOHO_DISK" not in text, older
    assert '#include "yoho_refine.h"' in hdr
    assert re.findall(r"#define\s+(\w+)", hdr) == ["YOHO_DISK_H", "YOHO_DISK_MAX_ROUNDS"]
    assert int(re.search(r"#define\s+YOHO_DISK_MAX_ROUNDS\s+(\d+)", hdr).group(1)) == hip.DISK_MAX_ROUNDS == DR.MAX_ROUNDS == 64
    assert 1 <= hip.DISK_DEFAULT_ROUNDS <= hip.DISK_MAX_ROUNDS
    assert build.EXTRA["disk.hip"] == ["-ffp-contract=off"] and "disk.hip" in build.SOURCES
    src = open(os.path.join(build.CSRC, "disk.hip")).read()
    assert re.findall(r'#include "([^"]+)"', src) == ["rfgrid.h", "dkthin.h", "yoho_disk.h", "yoho_salient.h"]
    # the mixer: the constants and the vectors the header gives, against both restatements
    for const in ("0x7feb352d", "0x846ca68b"):
        assert const in hdr and const in src
    vectors = re.findall(r"\((\d+), (\d+)\) -> (0x[0-9a-f]{8})", hdr)
    assert len(vectors) >= 3 and {((int(i), int(s)), int(k, 16)) for i, s, k in vectors} == set(DR.HEADER_VECTORS)
    for (i, s), k in DR.HEADER_VECTORS:
        assert DR.key_of_row(i, s) == k and int(DR.mix32(np.array([i ^ s]))[0]) == k
    assert np.array_equal(DR.keys(5000, 77), [DR.key_of_row(i, 77) for i in range(5000)]) and len(set(DR.keys(1 << 16, 3).tolist())) == 1 << 16


def test_disk_kernels_use_no_scratch(tmp_path):
    """csrc/disk.hip compiled for gfx950 with the flags of the build: its four kernels, the two templated ones once per key policy,
    none with scratch.  The VGPR counts are printed; no bound on them is asserted."""
    from yoho_amd import build
    cmd = [build._hipcc()] + build.FLAGS + build.EXTRA["disk.hip"] + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                                                                     os.path.join(build.CSRC, "disk.hip"), "-o", str(tmp_path / "disk.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r"\bVGPRs: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == sum(KERNELS.values()), names
    for k, n in KERNELS.items():
        assert sum(k in name for name in names) == n, (k, names)
    for k in ("dk_init_kernel", "dk_round_kernel"):
        assert sorted(p for name in names if k in name for p in ("DkHashed", "DkStored") if p in name) == ["DkHashed", "DkStored"], names
    print("disk.hip: " + ", ".join(f"{n} {v} VGPRs" for n, v in zip(names, vgprs)))
    assert scratch == [0] * len(names), dict(zip(names, scratch))


# ---- the restatements ----------------------------------------------------------------------------------------------------------------------
def consistent(states, n_out):
    last = states[-1]
    return n_out.tolist() == [int((last == 1).sum()), len(states) - 1, int((last == 0).sum())]


@pytest.mark.parametrize("n,radius,cloud", [(300, 0.15, 0), (1500, 0.09, 1), (1500, 0.2, 7)])
def test_the_two_restatements_agree(n, radius, cloud):
    """disk_greedy_ref (the sequential pass over a window on x) against disk_rounds_ref (synchronous rounds over a cKDTree's pairs) on
    clean_ref.separated_cloud, which asserts that no pair distance lies within 1e-6 relative of the radius; and on every result:
    no two kept rows are neighbours, every row is kept or has a kept neighbour, n is consistent with the state"""
    pts = CR.separated_cloud(cloud, n, radius)[1]
    sizes = []
    for seed in (0, 1, 12345, 0xFFFFFFFF):
        g = DR.disk_greedy_ref(pts, radius, seed)
        edges = DR.lower_key_edges(pts, radius, seed)
        st = DR.disk_rounds_ref(pts, radius, seed, edges=edges)
        assert np.array_equal(g["state"], st[-1]) and np.array_equal(np.nonzero(st[-1] == 1)[0], np.sort(g["kept"]))
        DR.assert_is_the_set(pts, radius, seed, st[-1], edges)
        n_out = DR.n_out_of(st)
        assert consistent(st, n_out) and n_out[0] == g["n"] and n_out[2] == 0 and 1 <= n_out[1] <= 16
        assert (np.diff(DR.keys(n, seed)[g["kept"]]) > 0).all()                                    # kept: in ascending key order
        # every prefix of the rounds is a state of its own: decided rows stay, undecided ones only ever leave 0
        for a, b in zip(st[:-1], st[1:]):
            assert np.array_equal(a[a != 0], b[a != 0]) and (b == 0).sum() < (a == 0).sum()
        # the same rounds in pieces
        half = DR.disk_rounds_ref(pts, radius, seed, max_rounds=2, edges=edges)
        rest = DR.disk_rounds_ref(pts, radius, seed, state0=half[-1], edges=edges)
        assert np.array_equal(half, st[:3]) and np.array_equal(rest, st[2:])
        sizes.append(g["n"])
    assert len(set(sizes)) > 1 and max(sizes) <= 1.25 * min(sizes)                                 # other seeds: other sets of about one size
    assert len({DR.disk_greedy_ref(pts, radius, s)["state"].tobytes() for s in (0, 1)}) == 2


def test_restatement_at_the_edges():
    """the gate, duplicates and non-finite rows - the cases tests/test_gpu_disk.py runs on the device, here on the restatements"""
    line = DR.gate_line(9)
    for seed in (0, 5):
        st = DR.disk_rounds_ref(line, 0.5, seed)                                                   # d2 = 0.25 = gate2: not neighbours
        assert (st[-1] == 1).all() and len(st) == 2 and (DR.disk_greedy_ref(line, 0.5, seed)["state"] == 1).all()
        r = np.nextafter(f32(0.5), f32(1))
        g = DR.disk_greedy_ref(line, r, seed)
        want = np.full(9, 2, np.uint8)
        for t in np.argsort(DR.keys(9, seed)):                                                     # the greedy alternation in key order
            if not any(0 <= u < 9 and want[u] == 1 for u in (t - 1, t + 1)):
                want[t] = 1
        assert np.array_equal(g["state"], want) and np.array_equal(DR.disk_rounds_ref(line, r, seed)[-1], want) and 4 <= g["n"] <= 5
    dup = np.tile(np.array([[0.25, 0.5, 0.75]], f32), (40, 1))
    for seed in (0, 9):
        g = DR.disk_greedy_ref(dup, 0.1, seed)
        assert g["kept"].tolist() == [int(np.argmin(DR.keys(40, seed)))] and np.array_equal(DR.disk_rounds_ref(dup, 0.1, seed)[-1], g["state"])
    pts = CL.mixed_cloud(257, 0.1)
    bad, good = CL.with_bad_rows(pts)
    rest = np.setdiff1d(np.arange(len(bad)), good)
    st = DR.disk_rounds_ref(bad, 0.1, 3)
    assert (st[:, rest] == 2).all() and np.array_equal(st[-1], DR.disk_greedy_ref(bad, 0.1, 3)["state"])
    DR.assert_is_the_set(bad, 0.1, 3, st[-1])
    # the rest is unaffected: the finite rows alone, with the keys they have in `bad`, give the same set
    a, b = DR.lower_key_edges(bad, 0.1, 3)
    assert np.isin(a, good).all() and np.isin(b, good).all()


def test_the_adversarial_chain():
    """2049 points 0.9 radius apart on a line, chain position t at row argsort(key)[t]: the keys ascend along the chain, every round
    decides exactly one row, the restatement needs 2049 rounds and keeps the even positions; after 64 rounds 1985 rows are undecided.
    With another seed the same rows need a handful of rounds (5)."""
    pts, row_of = DR.chain(2049, 0.05, 0)
    st = DR.disk_rounds_ref(pts, 0.05, 0)
    assert len(st) - 1 == 2049 and (st[64] == 0).sum() == 1985
    assert [(s == 0).sum() for s in st[:5]] == [2049, 2048, 2047, 2046, 2045]
    assert (st[-1][row_of[::2]] == 1).all() and (st[-1][row_of[1::2]] == 2).all()
    assert np.array_equal(st[-1], DR.disk_greedy_ref(pts, 0.05, 0)["state"])
    other = DR.disk_rounds_ref(pts, 0.05, 1)
    print(f"chain: seed 0 needs {len(st) - 1} rounds, seed 1 {len(other) - 1}")
    assert len(other) - 1 <= 16 and np.array_equal(other[-1], DR.disk_greedy_ref(pts, 0.05, 1)["state"])


# ---- the motivating case ---------------------------------------------------------------------------------------------------------------------
def test_thinning_covers_like_fps_in_a_dozen_rounds_and_needs_the_hash():
    """The extractor's benchmark cloud, synth.surface_cloud(300000, seed=1, extent=3.0), voxel 0.025: 87 824 candidates, 39.5
    neighbours per row inside r = 0.08.  Thinning keeps 4319 rows in 12 synchronous rounds (at most 16 asserted); they leave 0.0800
    uncovered (below r asserted), 1.027 times what 4319 picks of fps_ref leave, 0.0779 (at most 1.05 asserted), and a random draw of
    5000 leaves 0.175, more than twice that.  On the rows sorted by x at r = 0.07 the hashed priority needs 10 rounds (at most 16
    asserted) and row-order priority 258 (more than 100 asserted).  The two sets are printed, not compared: a sweep along x packs
    tighter than a pass in hashed order and keeps 7065 rows where the hash keeps 5607."""
    from yoho_amd import synth
    pc = synth.surface_cloud(300000, seed=1, extent=3.0)
    p = pc[KR.voxel_first_ref(pc, 0.025)].astype(f32)
    assert len(p) == 87824
    r = 0.08
    edges = DR.lower_key_edges(p, r, 0)
    st = DR.disk_rounds_ref(p, r, 0, edges=edges)
    DR.assert_is_the_set(p, r, 0, st[-1], edges)
    kept = np.nonzero(st[-1] == 1)[0]
    cov = DR.coverage(p, p[kept])
    fps = KR.fps_ref(p, len(kept), 0)[0]
    cov_fps = DR.coverage(p, p[fps])
    cov_rnd = DR.coverage(p, p[np.random.RandomState(0).permutation(len(p))[:5000]])
    print(f"r = {r}: {2 * len(edges[0]) / len(p):.1f} neighbours per row, {len(kept)} kept in {len(st) - 1} rounds (undecided after each: "
          f"{[int((s == 0).sum()) for s in st[1:]]}), coverage {cov:.4f}, fps_ref at the same count {cov_fps:.4f} (ratio {cov / cov_fps:.3f}), "
          f"a random 5000 {cov_rnd:.4f}")
    assert len(kept) == 4319 and len(st) - 1 <= 16
    assert cov < r and cov <= 1.05 * cov_fps and cov_rnd > 2 * cov
    ps = p[np.argsort(p[:, 0], kind="stable")]
    a, b = DR.lower_key_edges(ps, 0.07, 0)
    hashed = DR.disk_rounds_ref(ps, 0.07, 0, edges=(a, b))
    by_row = DR.disk_rounds_ref(ps, 0.07, 0, edges=(np.maximum(a, b), np.minimum(a, b)))          # key(i) = i: the lower row is the lower key
    n_h, n_r = int((hashed[-1] == 1).sum()), int((by_row[-1] == 1).sum())
    print(f"x-sorted rows, r = 0.07: hashed priority {len(hashed) - 1} rounds and {n_h} kept, row-order priority {len(by_row) - 1} rounds and {n_r} kept")
    assert len(hashed) - 1 <= 16 and len(by_row) - 1 > 100


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------
def host_context(rounds=3):
    from test_clean_cpu import HostContext

    class DiskContext(HostContext):
        """test_clean_cpu's host context with Context.disk_sample restated through disk_rounds_ref, `rounds` per call"""

        def disk_sample(self, pts, radius, seed=0, rounds=rounds, state=None):
            import torch
            self.calls.append(("disk_sample", pts.shape[0], radius, seed, state is not None))
            st = DR.disk_rounds_ref(pts.numpy(), radius, seed, max_rounds=rounds, state0=None if state is None else state.numpy())
            return torch.from_numpy(st[-1].copy()), torch.from_numpy(DR.n_out_of(st))

    return DiskContext()


def test_select_disk_order_cap_and_resumed_calls():
    import torch
    from test_clean_cpu import small_stray_cloud
    from yoho_amd import keypoints
    pc = small_stray_cloud(3)
    pc_d = torch.from_numpy(pc)
    ctx = host_context()
    for voxel, radius, seed in ((0.05, 0.15, 0), (None, 0.1, 7)):
        ctx.calls.clear()
        got, info = keypoints.select_disk(ctx, pc_d, radius, voxel=voxel, seed=seed)
        want, kept = DR.select_disk_ref(pc, radius, voxel=voxel, seed=seed)
        sel = np.arange(len(pc)) if voxel is None else KR.voxel_first_ref(pc, voxel)
        rounds = len(DR.disk_rounds_ref(pc[sel].astype(f32), radius, seed)) - 1
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want) and kept == len(want) > 20
        assert info == {"radius": radius, "kept": kept, "rounds": rounds, "calls": -(-rounds // 3), "capped": False} and rounds > 3
        assert [c[4] for c in ctx.calls] == [False] + [True] * (info["calls"] - 1) and {c[1:4] for c in ctx.calls} == {(len(sel), radius, seed)}
        # ascending key order of the candidate rows
        rows = np.searchsorted(sel, want)
        assert (np.diff(DR.keys(len(sel), seed)[rows]) > 0).all()
        # the cap: a prefix; at or above the kept count it changes nothing
        cut, cinfo = keypoints.select_disk(ctx, pc_d, radius, nkpts=20, voxel=voxel, seed=seed)
        assert np.array_equal(cut.numpy(), want[:20]) and cinfo == dict(info, capped=True)
        for nk in (kept, kept + 1, 5000):
            same, sinfo = keypoints.select_disk(ctx, pc_d, radius, nkpts=nk, voxel=voxel, seed=seed)
            assert np.array_equal(same.numpy(), want) and sinfo == info
    assert "NO LONGER HOLDS" in keypoints.select_disk.__doc__
    # the candidates go through the filter first, as select's do
    got, info = keypoints.select_disk(ctx, pc_d, 0.15, voxel=0.05, clean={"k": 8, "std_ratio": 1.0})
    sel = KR.voxel_first_ref(pc, 0.05)
    keep = CR.statistical_ref(pc[sel].astype(f32), 4 * 0.05, 8, 1, 1.0)["keep"]
    want = sel[keep][DR.disk_greedy_ref(pc[sel][keep].astype(f32), 0.15, 0)["kept"]]
    assert np.array_equal(got.numpy(), want) and 0 < keep.sum() < len(sel)


def test_resumed_calls_are_bounded():
    """the chain at 3 rounds per call: 40 rows need 40 rounds, 14 calls, inside the bound ceil(40 / 3) + 1 = 15; a context that never
    decides anything is given up on after exactly that many calls"""
    import torch
    from yoho_amd import keypoints
    pts, row_of = DR.chain(40, 0.05, 0)
    pc_d = torch.from_numpy(pts.astype(f64))
    ctx = host_context()
    got, info = keypoints.select_disk(ctx, pc_d, 0.05)
    assert np.array_equal(got.numpy(), row_of[::2]) and info["rounds"] == 40 and info["calls"] == 14 and len(ctx.calls) == 14

    class Stuck:
        calls = 0

        def disk_sample(self, pts, radius, seed=0, rounds=3, state=None):
            self.calls += 1
            n = pts.shape[0]
            return torch.zeros(n, dtype=torch.uint8), torch.tensor([0, rounds, n], dtype=torch.int32)

    stuck = Stuck()
    with pytest.raises(RuntimeError, match="undecided"):
        keypoints._thin(stuck, torch.from_numpy(pts), 0.05, 0, "select_disk")
    assert stuck.calls == 15


def test_disk_radius_follows_the_square_root_update():
    import torch
    from yoho_amd import keypoints, synth
    p = synth.surface_cloud(4000, 5).astype(f32)
    pts = torch.from_numpy(p)
    ctx = host_context(rounds=64)
    nk, r0 = 300, 0.2
    r, want_r, tried, best = float(f32(r0)), [], [], None
    for _ in range(6):                                                                             # the iteration, restated
        if r in want_r:
            break
        want_r.append(r)
        kept = DR.disk_greedy_ref(p, r, 2)["kept"]
        tried.append(len(kept))
        if len(kept) <= nk and (best is None or len(kept) > best[1]):
            best = (r, len(kept), kept)
        if len(kept) == nk:
            break
        r = float(f32(r * np.sqrt(len(kept) / nk)))
    print(f"disk_radius: radii {want_r}, counts {tried}")
    got_r, rows, info = keypoints.disk_radius(ctx, pts, nk, r0, seed=2)
    assert [c[2] for c in ctx.calls] == want_r and len(want_r) >= 3
    assert got_r == best[0] and info["kept"] == best[1] <= nk and np.array_equal(rows.numpy(), best[2]) and info["radius"] == got_r
    assert best[1] >= 0.9 * nk and tried[0] < 0.5 * nk                                             # the probe is far off, the answer is not
    ctx.calls.clear()
    assert keypoints.disk_radius(ctx, pts, nk, r0, steps=1, seed=2)[2]["kept"] == tried[0] and len(ctx.calls) == 1
    assert keypoints.disk_radius(ctx, pts, 10, 0.01, steps=1) == (None, None, None)                # every tested radius kept more
    with pytest.raises(ValueError, match="disk_radius"):
        keypoints.disk_radius(ctx, pts, 0, 0.1)
    assert "per-fragment" in keypoints.disk_radius.__doc__


def test_write_keypoints_takes_a_method_and_without_it_is_unchanged(tmp_path, monkeypatch):
    import torch
    from test_clean_cpu import small_stray_cloud
    from test_keypoints_cpu import make_dataset
    from yoho_amd import keypoints
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)                          # the host context's tensors stay where they are
    clouds = [small_stray_cloud(k)[:400 + 30 * k] for k in range(2)]
    ds = make_dataset(str(tmp_path / "scene"), clouds)
    ctx = host_context()
    assert keypoints.write_keypoints(ds, nkpts=16, voxel=0.1, ctx=ctx, method="disk", radius=0.3, seed=4) == ["0", "1"]
    for k in range(2):
        pc = ds.get_pc(str(k))
        want, kept = DR.select_disk_ref(pc, 0.3, nkpts=16, voxel=0.1, seed=4)
        assert np.array_equal(np.loadtxt(ds.kps_fn[k]).astype(int), want) and np.array_equal(np.load(ds.kps_pc_fn[k]), pc[want]) and kept > 16
    assert all(c[0] == "disk_sample" and c[2:4] == (0.3, 4) for c in ctx.calls) and ctx.calls
    # a selector passed in is called as before, whatever the method
    seen = []

    def stub(pc, nkpts, voxel):
        seen.append((len(pc), nkpts, voxel))
        return KR.select_ref(pc, nkpts, voxel=voxel)

    assert keypoints.write_keypoints(ds, nkpts=16, voxel=0.1, selector=stub, method="disk", radius=0.3, overwrite=True) == ["0", "1"]
    assert seen == [(400, 16, 0.1), (430, 16, 0.1)]
    # without the new arguments: the files of before, through the default selector
    assert keypoints.write_keypoints(ds, nkpts=16, voxel=0.1, ctx=ctx, overwrite=True) == ["0", "1"]
    for k in range(2):
        assert np.array_equal(np.loadtxt(ds.kps_fn[k]).astype(int), KR.select_ref(ds.get_pc(str(k)), 16, voxel=0.1))
    pc_d = torch.from_numpy(clouds[0])
    assert np.array_equal(keypoints.select(ctx, pc_d, 16, voxel=0.1)[0].numpy(), KR.select_ref(clouds[0], 16, voxel=0.1))
    for kw in ({"method": "disk"}, {"radius": 0.3}, {"method": "fps", "radius": 0.3}, {"method": "grid"}):
        with pytest.raises(ValueError, match="write_keypoints"):
            keypoints.write_keypoints(ds, nkpts=16, voxel=0.1, ctx=ctx, overwrite=True, **kw)


def test_extractor_argument_checks(monkeypatch):
    from yoho_amd import hip, yoho_extract
    from yoho_amd.yoho_extract import yoho_extractor

    class Reached(Exception):
        pass

    def no_context(*a, **k):
        raise Reached()

    monkeypatch.setattr(hip, "get_context", no_context)                                            # what the constructor does behind its checks
    assert yoho_extract.KEYPOINT_MODES == ("random", "fps", "disk")
    for kw in ({"keypoints": "disk"}, {"keypoints": "disk", "keypoint_radius": 0.0}, {"keypoints": "disk", "keypoint_radius": float("nan")},
               {"keypoints": "fps", "keypoint_radius": 0.07}, {"keypoints": "random", "keypoint_radius": 0.07}, {"keypoint_radius": 0.07}):
        with pytest.raises(ValueError, match="keypoint_radius"):
            yoho_extractor(fcgf_ckpt=None, yoho_ckpt={}, **kw)
    with pytest.raises(ValueError, match="keypoint_clean"):
        yoho_extractor(fcgf_ckpt=None, yoho_ckpt={}, keypoints="random", keypoint_clean={})
    for kw in ({"keypoints": "disk", "keypoint_radius": 0.07}, {"keypoints": "disk", "keypoint_radius": 0.07, "keypoint_seed": 5, "keypoint_clean": {}},
               {"keypoints": "fps", "keypoint_clean": {}}, {"keypoints": "fps"}, {}):
        with pytest.raises(Reached):
            yoho_extractor(fcgf_ckpt=None, yoho_ckpt={}, **kw)
