"""CPU tests of the salient keypoints (include/yoho_salient.h, yoho_amd/keypoints.py select_salient): the library builds
and exports exactly the header's two symbols and its kernels compile without scratch; the two numpy restatements of the thinning
(tests/salient_ref.py) agree and hold the contract's identities - a constant priority is the hashed entry, round 1 is non-maximum
suppression, split calls, masked rows -; the Python layer over a host context built from the restatements, which without the new
arguments does what it did; and what the feature is for, measured on the crease scene."""
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
import salient_ref as SR  # noqa: E402

f32, f64 = np.float32, np.float64
KERNELS = ["sl_saliency_kernel"]
OLDER = ("yoho_hip.h", "yoho_knn.h", "yoho_trainset.h", "yoho_refine.h", "yoho_plane.h", "yoho_verify.h", "yoho_consist.h", "yoho_keypoints.h",
         "yoho_multiway.h", "yoho_fuse.h", "yoho_clean.h", "yoho_cluster.h", "yoho_disk.h")
CLOUDS = [(300, 0.15, 0), (1500, 0.09, 1), (1500, 0.2, 7)]


# ---- the library ---------------------------------------------------------------------------------------------------------------------------
def test_library_exports_salient_header_symbols():
    """include/yoho_salient.h declares exactly hip.SALIENT_SYMBOLS, the library exports them with 11 and 11 arguments, the list shares
    nothing with the other thirteen, which are what they were, and nothing leaked into the older headers; the header's key vectors
    equal both restatements of key64"""
    import ctypes as C
    from yoho_amd import build, hip
    assert os.path.exists(build.build(verbose=False))
    lib = hip.load_library()
    hdr = open(os.path.join(REPO, "include", "yoho_salient.h")).read()
    fns = set(re.findall(r"\b(yoho_[a-zA-Z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert fns == {"yoho_iss_saliency", "yoho_disk_sample_prio"} and hip.SALIENT_SYMBOLS == ["yoho_iss_saliency", "yoho_disk_sample_prio"]
    a, b = lib.yoho_iss_saliency.argtypes, lib.yoho_disk_sample_prio.argtypes
    assert lib.yoho_iss_saliency.restype is C.c_int and lib.yoho_disk_sample_prio.restype is C.c_int and len(a) == 11 and len(b) == 11
    assert a[2] is C.c_int and a[3] is C.c_float and a[4] is C.c_int and a[5] is C.c_double and a[6] is C.c_double
    assert b[2] is C.c_int and b[3] is C.c_float and b[5] is C.c_uint32 and b[6] is C.c_int and b[7] is C.c_int
    others = (hip.SYMBOLS + hip.KNN_SYMBOLS + hip.TRAINSET_SYMBOLS + hip.REFINE_SYMBOLS + hip.PLANE_SYMBOLS + hip.VERIFY_SYMBOLS + hip.CONSIST_SYMBOLS +
              hip.KEYPOINT_SYMBOLS + hip.MULTIWAY_SYMBOLS + hip.FUSE_SYMBOLS + hip.CLEAN_SYMBOLS + hip.CLUSTER_SYMBOLS + hip.DISK_SYMBOLS)
    assert not fns & set(others)
    assert hip.DISK_SYMBOLS == ["yoho_disk_sample"] and hip.PLANE_SYMBOLS == ["yoho_estimate_normals", "yoho_icp_plane"]
    main = open(os.path.join(REPO, "include", "yoho_hip.h")).read()
    assert set(re.findall(r"\b(yoho_[a-zA-Z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", main, flags=re.S))) == set(hip.SYMBOLS)
    for older in OLDER:
        text = open(os.path.join(REPO, "include", older)).read()
        assert "yoho_iss" not in text and "sample_prio" not in text and "YOHO_SALIENT" not in text, older
    assert '#include "yoho_refine.h"' in hdr
    assert re.findall(r"#define\s+(\w+)", hdr) == ["YOHO_SALIENT_H", "YOHO_SALIENT_MAX_ROUNDS"]
    assert int(re.search(r"#define\s+YOHO_SALIENT_MAX_ROUNDS\s+(\d+)", hdr).group(1)) == hip.DISK_MAX_ROUNDS == SR.MAX_ROUNDS
    assert build.EXTRA["salient.hip"] == ["-ffp-contract=off"] and "salient.hip" in build.SOURCES
    src = open(os.path.join(build.CSRC, "salient.hip")).read()
    assert re.findall(r'#include "([^"]+)"', src) == ["rfgrid.h", "rffit.h", "dkthin.h", "yoho_salient.h"]
    for shared in ("_round_kernel", "_tail_kernel", "_zero_kernel", "0x1p-58", "0x7feb352d", "0x846ca68b"):      # the thinning is disk.hip's, the Jacobi rffit.h's
        assert shared not in src, shared
    vectors = re.findall(r"\((\d+), (\d+), (0x[0-9a-f]{8})\) -> (0x[0-9a-f]{16})", hdr)
    assert len(vectors) >= 3 and {((int(i), int(s), int(p, 16)), int(k, 16)) for i, s, p, k in vectors} == set(SR.HEADER_VECTORS)
    for (i, s, bits), k in SR.HEADER_VECTORS:
        prio = np.zeros(i + 1, np.uint32)
        prio[i] = bits
        assert SR.key64_of_row(i, s, bits) == k and int(SR.key64(prio.view(f32), s)[i]) == k
    rs = np.random.RandomState(0)
    p = rs.randint(0, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32).view(f32)
    assert [int(v) for v in SR.key64(p, 77)] == [SR.key64_of_row(i, 77, b) for i, b in enumerate(p.view(np.uint32))]
    # ord is monotone, every NaN is below -inf, and the order of the keys is the reverse
    v = np.array([-np.inf, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, np.inf], f32)
    o = SR.ord32(v)
    assert (np.diff(o.astype(np.int64)) > 0).all() and (SR.ord32(np.array([np.nan, -np.nan], f32)) == 0).all() and o.min() > 0


def test_salient_kernels_use_no_scratch(tmp_path):
    """csrc/salient.hip compiled for gfx950 with the flags of the build: its one kernel (the thinning kernels are disk.hip's,
    tests/test_disk_cpu.py), without scratch.  The VGPR count is printed; no bound on it is asserted."""
    from yoho_amd import build
    cmd = [build._hipcc()] + build.FLAGS + build.EXTRA["salient.hip"] + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                                                                        os.path.join(build.CSRC, "salient.hip"), "-o", str(tmp_path / "salient.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r"\bVGPRs: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == len(KERNELS), names
    for k in KERNELS:
        assert sum(k in name for name in names) == 1, (k, names)
    print("salient.hip: " + ", ".join(f"{n} {v} VGPRs" for n, v in zip(names, vgprs)))
    assert scratch == [0] * len(names), dict(zip(names, scratch))


def test_the_grid_family_shares_its_pieces():
    """each piece the entries on the cell-sorted grid share is written once: the bucket hash in rfgrid.h (gridnn.hip's grid is the
    one it was copied from; fourier.hip's sample hash and sparse.h's voxel hash use the same multiplier for other things and are
    listed, so a fifth file fails), the Jacobi's skip rule in rffit.h, the mixer in disk.hip; the names of the copies are gone.  The
    sparse backbone's helpers are sp_* as well, so that prefix is looked for outside its files (sp*.hip, sp*.h)."""
    from yoho_amd import build
    files = {f: open(os.path.join(build.CSRC, f)).read() for f in sorted(os.listdir(build.CSRC)) if f.endswith((".hip", ".h"))}
    where = lambda text: sorted(f for f, src in files.items() if text in src)      # noqa: E731
    assert where("0x9E3779B97F4A7C15") == ["fourier.hip", "gridnn.hip", "rfgrid.h", "sparse.h"]
    family = [f for f, src in files.items() if '#include "rfgrid.h"' in src]
    assert {"clean.hip", "cluster.hip", "disk.hip", "salient.hip", "plane.hip", "refine.hip", "verify.hip", "multiway.hip", "fuse.hip", "rfgrid.hip"} <= set(family)
    assert not [f for f in family if "0x9E3779B97F4A7C15" in files[f]]
    assert where("0x1p-58") == ["rffit.h"]
    assert where("0x7feb352d") == ["disk.hip"]
    for gone in ("cu_walk", "pl_eig3", "sl_eig3", "cu_load_row", "CL_SEEN", "CU_SEEN"):
        assert where(gone) == [], gone
    assert [f for f in where("sp_") if not f.startswith("sp")] == []
    # one walk over the distinct buckets and one Jacobi, each with the callers it had as copies
    assert where("rf_walk_each(") == ["clean.hip", "cluster.hip", "rfgrid.h"] and where("rf_moments(") == ["plane.hip", "rfgrid.h", "salient.hip"]
    assert where("rf_eig3<") == ["plane.hip", "salient.hip"] and where("dk_thin(") == ["disk.hip", "dkthin.h", "salient.hip"]


# ---- the restatements ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,radius,cloud", CLOUDS)
def test_the_two_restatements_agree(n, radius, cloud):
    """disk_prio_greedy_ref (the sequential pass) against disk_prio_rounds_ref (synchronous rounds) on clean_ref.separated_cloud with
    the four kinds of priority; on every result the set's properties; a constant priority reproduces disk_ref.disk_rounds_ref state
    by state; the state after round 1 is the set of strict local maxima, computed here from the neighbour lists"""
    pts = CR.separated_cloud(cloud, n, radius)[1]
    pr = SR.pairs(pts, radius)
    nb = CL.neighbours_ref(pts, radius)
    for seed in (0, 12345):
        for name, prio in SR.priorities(n, seed).items():
            st = SR.disk_prio_rounds_ref(pts, radius, prio, seed, pr=pr)
            g = SR.disk_prio_greedy_ref(pts, radius, prio, seed)
            assert np.array_equal(g["state"], st[-1]) and (st[-1] != 0).all(), name
            assert np.array_equal(np.sort(g["kept"]), np.nonzero(st[-1] == 1)[0]) and g["n"] == len(g["kept"])
            SR.assert_is_the_set(pts, radius, prio, seed, st[-1], pr=pr)
            key = SR.key64(prio, seed)
            assert (np.diff(key[g["kept"]].astype(object)) > 0).all()                               # kept: in ascending key order
            if name == "constant":
                assert np.array_equal(st, DR.disk_rounds_ref(pts, radius, seed))
            else:
                assert st[-1].tobytes() != DR.disk_rounds_ref(pts, radius, seed)[-1].tobytes()
            # round 1 is non-maximum suppression: kept iff no neighbour precedes the row
            nms = np.array([all(key[j] > key[i] for j in nb[i][0]) for i in range(n)])
            assert np.array_equal(st[1] == 1, nms) and not (st[1] == 2).any()
            # the same rounds in pieces
            half = SR.disk_prio_rounds_ref(pts, radius, prio, seed, max_rounds=2, pr=pr)
            rest = SR.disk_prio_rounds_ref(pts, radius, prio, seed, state0=half[-1], pr=pr)
            assert np.array_equal(half, st[:3]) and np.array_equal(rest, st[2:])


def test_masked_rows_and_non_finite_rows():
    """rows handed in as 2 are never kept and block nobody: the rest is thinned as if they were not in the cloud (with the keys it has
    in the full cloud); a row handed in as 1 blocks the neighbours it precedes only; a non-finite row handed in as 0 becomes 2"""
    n, radius = 600, 0.12
    pts = CR.separated_cloud(3, n, radius)[1]
    rs = np.random.RandomState(5)
    prio = rs.rand(n).astype(f32)
    mask = rs.rand(n) < 0.4
    state0 = np.where(mask, 2, 0).astype(np.uint8)
    st = SR.disk_prio_rounds_ref(pts, radius, prio, 3, state0=state0)
    g = SR.disk_prio_greedy_ref(pts, radius, prio, 3, state0=state0)
    assert np.array_equal(st[-1], g["state"]) and (st[:, mask] == 2).all() and 0 < (st[-1] == 1).sum() < (~mask).sum()
    SR.assert_is_the_set(pts, radius, prio, 3, st[-1], state0=state0)
    # without the masked rows: the same set on the rest.  The keys depend on the row number, so the rest is thinned in the order its
    # rows have in the full cloud: a priority that reproduces that order exactly
    rest = np.nonzero(~mask)[0]
    rank = np.empty(len(rest), f32)
    rank[np.argsort(SR.key64(prio, 3)[rest].astype(object))] = -np.arange(len(rest), dtype=f32)
    alone = SR.disk_prio_greedy_ref(pts[rest], radius, rank, 0)["state"]
    assert np.array_equal(alone, st[-1][rest])
    # a kept row handed in blocks only the rows it precedes
    first = int(np.argmax(SR.key64(prio, 3).astype(object)))                                     # the row every other precedes
    s1 = np.zeros(n, np.uint8)
    s1[first] = 1
    assert np.array_equal(SR.disk_prio_greedy_ref(pts, radius, prio, 3, state0=s1)["state"][np.arange(n) != first],
                          SR.disk_prio_greedy_ref(pts, radius, prio, 3)["state"][np.arange(n) != first])
    bad, good = CL.with_bad_rows(CL.mixed_cloud(257, 0.1))
    notfin = np.setdiff1d(np.arange(len(bad)), good)
    pb = np.random.RandomState(1).rand(len(bad)).astype(f32)
    st = SR.disk_prio_rounds_ref(bad, 0.1, pb, 3, state0=np.zeros(len(bad), np.uint8))
    assert (st[:, notfin] == 2).all() and np.array_equal(st, SR.disk_prio_rounds_ref(bad, 0.1, pb, 3))
    assert np.array_equal(st[-1], SR.disk_prio_greedy_ref(bad, 0.1, pb, 3)["state"])


def test_saliency_restatement_and_the_rule():
    """saliency_ref against eig_exact on a few rows, inside the bound the device is held to with room to spare; prio_of at its
    thresholds; tier classes"""
    pts, _ = SR.crease_scene(1500, 0)
    pts = pts.astype(f32)
    ref = SR.saliency_ref(pts, 0.2)
    assert ref["count"].min() >= 5 and (np.diff(ref["eig"], axis=1) >= 0).all() and (ref["eig"] >= 0).all()
    for i in (0, 700, 1499):
        ex = SR.eig_exact(pts, i, 0.2)
        assert ex["count"] == ref["count"][i]
        for k in range(3):
            assert SR.exact_error(ref["eig"][i, k], ex["lam"][k]) <= 4.0 * ex["count"] * 2.0 ** -53 * ex["trace"]
    eig = np.array([[1.0, 2.0, 4.0], [1.0, 2.0, 2.0], [2.0, 2.0, 4.0], [0.0, 0.0, 4.0], [0.0, 0.0, 0.0], [0.0, 1.0, 4.0], [1.0, 1.95, 2.0]])
    count = np.array([5, 5, 5, 5, 5, 5, 4])
    p = SR.prio_of(eig, count, 5, 0.975, 0.975)
    assert np.isnan(p).tolist() == [False, True, True, True, True, False, True] and p[0] == 1 and p[5] == 0
    assert (p.view(np.uint32)[np.isnan(p)] == SR.QNAN).all()
    assert np.isnan(SR.prio_of(eig, count, 5, 0.5, 0.5)).tolist() == [True, True, True, True, True, False, True]      # 2 < 0.5 * 4 is false
    assert not np.isnan(SR.prio_of(eig, count, 3, 1.0, 1.0))[[0, 5, 6]].any()
    t = SR.tier_classes_ref(np.array([0.5, np.nan, 0.1, 0.9, 0.5, 0.2], f32), 2)
    assert np.isnan(t[1]) and t[[3, 0, 4, 5, 2]].tolist() == [1, 1, 1, 0, 0]


def test_a_monotone_priority_builds_a_chain_and_thin_resumes_it():
    """prio = x on disk_ref.chain: the keys descend along the line, every round decides one row, more than 64 rounds; _thin finishes it
    through resumed calls inside its bound; 7 + 9 rounds in two calls leave the bytes of 16 in one"""
    import torch
    from yoho_amd import keypoints
    pts, row_of = DR.chain(100, 0.05, 0)
    prio = pts[:, 0].copy()
    st = SR.disk_prio_rounds_ref(pts, 0.05, prio, 0)
    assert len(st) - 1 == 100 > SR.MAX_ROUNDS and [(s == 0).sum() for s in st[:4]] == [100, 99, 98, 97]
    assert (st[-1][row_of[::-1][::2]] == 1).all() and (st[-1] == 1).sum() == 50                   # from the far end, every other one
    a = SR.disk_prio_rounds_ref(pts, 0.05, prio, 0, max_rounds=7)
    b = SR.disk_prio_rounds_ref(pts, 0.05, prio, 0, max_rounds=9, state0=a[-1])
    assert np.array_equal(b[-1], st[16]) and np.array_equal(SR.disk_prio_rounds_ref(pts, 0.05, prio, 0, max_rounds=16)[-1], st[16])
    ctx = host_context(rounds=16)
    rows, info = keypoints._thin(ctx, torch.from_numpy(pts), 0.05, 0, "select_salient", prio=torch.from_numpy(prio))
    assert info["rounds"] == 100 and info["calls"] == 7 and info["kept"] == 50
    assert np.array_equal(rows.numpy(), row_of[::-1][::2])                                         # key order: the highest x first
    assert [c[0] for c in ctx.calls] == ["disk_sample_prio"] * 7 and [c[4] for c in ctx.calls] == [False] + [True] * 6

    class Stuck:
        calls = 0

        def disk_sample_prio(self, pts, radius, prio, seed=0, rounds=3, state=None):
            self.calls += 1
            n = pts.shape[0]
            return torch.zeros(n, dtype=torch.uint8), torch.tensor([0, rounds, n], dtype=torch.int32)

    stuck = Stuck()
    with pytest.raises(RuntimeError, match="undecided"):
        keypoints._thin(stuck, torch.from_numpy(pts), 0.05, 0, "select_salient", prio=torch.from_numpy(prio))
    assert stuck.calls == -(-100 // 3) + 1                                                         # the bound on resumed calls is what it was


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------
def host_context(rounds=3):
    from test_disk_cpu import host_context as disk_context

    class SalientContext(type(disk_context(rounds))):
        """test_disk_cpu's host context with Context.iss_saliency and Context.disk_sample_prio restated through salient_ref"""

        def iss_saliency(self, pts, radius, min_nbrs=5, gamma21=0.975, gamma32=0.975, want_eig=False):
            import torch
            self.calls.append(("iss_saliency", pts.shape[0], radius, min_nbrs, gamma21, gamma32))
            r = SR.saliency_ref(pts.numpy(), radius)
            out = (torch.from_numpy(SR.prio_of(r["eig"], r["count"], min_nbrs, gamma21, gamma32)), torch.from_numpy(r["count"]))
            return out + (torch.from_numpy(r["eig"]),) if want_eig else out

        def disk_sample_prio(self, pts, radius, prio, seed=0, rounds=rounds, state=None):
            import torch
            self.calls.append(("disk_sample_prio", pts.shape[0], radius, seed, state is not None))
            st = SR.disk_prio_rounds_ref(pts.numpy(), radius, prio.numpy(), seed, max_rounds=rounds, state0=None if state is None else state.numpy())
            return torch.from_numpy(st[-1].copy()), torch.from_numpy(DR.n_out_of(st))

    return SalientContext()


def select_salient_ref(pc, radius, prio, mode="greedy", fill=True, tiers="default", seed=0, voxel=None):
    """keypoints.select_salient from the priorities on: cloud indices in key64 order"""
    if tiers == "default":
        from yoho_amd import keypoints
        tiers = keypoints.SALIENT_DEFAULT_TIERS if mode == "greedy" else None
    sel = np.arange(len(pc), dtype=np.int64) if voxel is None else KR.voxel_first_ref(pc, voxel)
    pts = np.asarray(pc, f64)[sel].astype(f32)
    elig = ~np.isnan(prio)
    if tiers is not None:
        prio = SR.tier_classes_ref(prio, tiers)
    masked = np.where(elig, 0, 2).astype(np.uint8)
    if mode == "nms":
        state = SR.disk_prio_rounds_ref(pts, radius, prio, seed, max_rounds=1, state0=masked)[-1]
    else:
        state = SR.disk_prio_greedy_ref(pts, radius, prio, seed, state0=None if fill else masked)["state"]
    kept = np.nonzero(state == 1)[0]
    return sel[kept[np.argsort(SR.key64(prio, seed)[kept].astype(object), kind="stable")]], int(elig.sum())


def test_select_salient_modes_order_and_cap():
    import torch
    from yoho_amd import keypoints
    pc, spacing = SR.crease_scene(2500, 1)
    pc_d = torch.from_numpy(pc)
    ctx = host_context(rounds=16)
    radius = 0.08
    for voxel, seed in ((None, 0), (0.03, 5)):
        sel = np.arange(len(pc)) if voxel is None else KR.voxel_first_ref(pc, voxel)
        r = SR.saliency_ref(pc[sel].astype(f32), 2 * radius)
        prio = SR.prio_of(r["eig"], r["count"], 5, 0.7, 0.975)                                    # l2 < 0.7 l3: the inside of a plane is out
        print(f"voxel {voxel}: {len(sel)} candidates, {int((~np.isnan(prio)).sum())} eligible at gamma21 = 0.7")
        assert 0.02 * len(sel) < (~np.isnan(prio)).sum() < 0.9 * len(sel)
        results = {}
        for kw in ({}, {"fill": False}, {"mode": "nms"}, {"tiers": 8}, {"tiers": 8, "fill": False}, {"tiers": None}, {"tiers": None, "fill": False}):
            ctx.calls.clear()
            got, info = keypoints.select_salient(ctx, pc_d, radius, voxel=voxel, seed=seed, gamma21=0.7, **kw)
            want, eligible = select_salient_ref(pc, radius, prio, seed=seed, voxel=voxel, **kw)
            assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want) and len(want) > 10, kw
            assert info["eligible"] == eligible and info["mode"] == kw.get("mode", "greedy") and info["tiers"] == kw.get("tiers", None if kw.get("mode") == "nms" else keypoints.SALIENT_DEFAULT_TIERS) and info["kept"] == len(want)
            assert info["radius"] == radius and not info["capped"] and ctx.calls[0] == ("iss_saliency", len(sel), 2 * radius, 5, 0.7, 0.975)
            assert all(c[0] == "disk_sample_prio" for c in ctx.calls[1:]) and info["calls"] == len(ctx.calls) - 1
            results[tuple(sorted(kw.items()))] = set(want.tolist())
        full, nofill, nms = results[(("tiers", None),)], results[(("fill", False), ("tiers", None))], results[(("mode", "nms"),)]
        assert nms < nofill < full                                                                 # in one order: the maxima, then the eligible rows, then the fill
        assert results[(("fill", False),)] < results[()]                                           # and in the order of the default rank classes
        full = results[()]
        # fill=True covers every candidate, as select_disk does
        want = np.array(sorted(full))
        assert DR.coverage(pc[sel], pc[want]) < radius
        cut, cinfo = keypoints.select_salient(ctx, pc_d, radius, voxel=voxel, seed=seed, nkpts=10, gamma21=0.7)
        ref = select_salient_ref(pc, radius, prio, seed=seed, voxel=voxel)[0]
        assert np.array_equal(cut.numpy(), ref[:10]) and cinfo["capped"] and cinfo["kept"] == len(ref)
    # other arguments reach the entry; a salient_radius of its own
    ctx.calls.clear()
    keypoints.select_salient(ctx, pc_d, radius, salient_radius=0.1, min_nbrs=7, gamma21=0.9, gamma32=0.8)
    assert ctx.calls[0] == ("iss_saliency", len(pc), 0.1, 7, 0.9, 0.8)
    for kw in ({"mode": "max"}, {"tiers": 0}, {"tiers": -3}, {"tiers": "auto"}):
        with pytest.raises(ValueError, match="select_salient"):
            keypoints.select_salient(ctx, pc_d, radius, **kw)
    # the torch restatement of the key equals the numpy one, in order
    p = torch.from_numpy(SR.priorities(4000, 2)["special"])
    k = keypoints.prio_key(p, 9).numpy().astype(object) + (1 << 63)
    assert [int(v) for v in k] == [int(v) for v in SR.key64(p.numpy(), 9)]
    assert np.array_equal(keypoints.tier_classes(p, 16).numpy().view(np.uint32), SR.tier_classes_ref(p.numpy(), 16).view(np.uint32))


def test_write_keypoints_takes_saliency_and_without_it_is_unchanged(tmp_path, monkeypatch):
    import torch
    from test_keypoints_cpu import make_dataset
    from yoho_amd import keypoints
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)                          # the host context's tensors stay where they are
    clouds = [SR.crease_scene(900 + 50 * k, 10 + k)[0] for k in range(2)]
    ds = make_dataset(str(tmp_path / "scene"), clouds)
    ctx = host_context()
    assert keypoints.write_keypoints(ds, nkpts=40, voxel=0.02, ctx=ctx, method="disk", radius=0.1, seed=4, saliency={"tiers": 4}) == ["0", "1"]
    for k in range(2):
        pc = ds.get_pc(str(k))
        sel = KR.voxel_first_ref(pc, 0.02)
        r = SR.saliency_ref(pc[sel].astype(f32), 0.2)
        want = select_salient_ref(pc, 0.1, SR.prio_of(r["eig"], r["count"]), tiers=4, seed=4, voxel=0.02)[0]
        assert len(want) > 40
        assert np.array_equal(np.loadtxt(ds.kps_fn[k]).astype(int), want[:40]) and np.array_equal(np.load(ds.kps_pc_fn[k]), pc[want[:40]])
    # {} means the defaults of select_salient
    assert keypoints.write_keypoints(ds, nkpts=5000, voxel=0.02, ctx=ctx, method="disk", radius=0.1, saliency={}, overwrite=True) == ["0", "1"]
    pc = ds.get_pc("0")
    sel = KR.voxel_first_ref(pc, 0.02)
    r = SR.saliency_ref(pc[sel].astype(f32), 0.2)
    want = select_salient_ref(pc, 0.1, SR.prio_of(r["eig"], r["count"]), tiers=keypoints.SALIENT_DEFAULT_TIERS, voxel=0.02)[0]
    assert np.array_equal(np.loadtxt(ds.kps_fn[0]).astype(int), want)
    # saliency=None: the bytes of the files the disk method wrote before, through calls of disk_sample alone
    ctx.calls.clear()
    assert keypoints.write_keypoints(ds, nkpts=40, voxel=0.02, ctx=ctx, method="disk", radius=0.1, seed=4, saliency=None, overwrite=True) == ["0", "1"]
    assert {c[0] for c in ctx.calls} == {"disk_sample"}
    before = [(open(ds.kps_fn[k], "rb").read(), open(ds.kps_pc_fn[k], "rb").read()) for k in range(2)]
    assert keypoints.write_keypoints(ds, nkpts=40, voxel=0.02, ctx=ctx, method="disk", radius=0.1, seed=4, overwrite=True) == ["0", "1"]
    assert before == [(open(ds.kps_fn[k], "rb").read(), open(ds.kps_pc_fn[k], "rb").read()) for k in range(2)]
    for k in range(2):
        want = DR.select_disk_ref(ds.get_pc(str(k)), 0.1, nkpts=40, voxel=0.02, seed=4)[0]
        assert np.array_equal(np.loadtxt(ds.kps_fn[k]).astype(int), want)
    assert keypoints.METHODS == ("fps", "disk")
    for kw in ({"method": "fps", "saliency": {}}, {"saliency": {}}, {"method": "disk", "radius": 0.1, "saliency": {"radius": 0.2}},
               {"method": "disk", "radius": 0.1, "saliency": 3}, {"method": "disk", "radius": 0.1, "saliency": {"nkpts": 5}}):
        with pytest.raises(ValueError, match="saliency"):
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
    for kw in ({"keypoint_saliency": {}}, {"keypoints": "fps", "keypoint_saliency": {}}, {"keypoints": "random", "keypoint_saliency": {"tiers": 8}},
               {"keypoints": "disk", "keypoint_radius": 0.07, "keypoint_saliency": {"seed": 1}},
               {"keypoints": "disk", "keypoint_radius": 0.07, "keypoint_saliency": "iss"}):
        with pytest.raises(ValueError, match="keypoint_saliency"):
            yoho_extractor(fcgf_ckpt=None, yoho_ckpt={}, **kw)
    with pytest.raises(ValueError, match="keypoint_radius"):
        yoho_extractor(fcgf_ckpt=None, yoho_ckpt={}, keypoints="disk", keypoint_saliency={})
    for kw in ({"keypoints": "disk", "keypoint_radius": 0.07, "keypoint_saliency": {}},
               {"keypoints": "disk", "keypoint_radius": 0.07, "keypoint_saliency": {"mode": "nms", "tiers": 8}, "keypoint_clean": {}},
               {"keypoints": "disk", "keypoint_radius": 0.07}):
        with pytest.raises(Reached):
            yoho_extractor(fcgf_ckpt=None, yoho_ckpt={}, **kw)


# ---- what it is for --------------------------------------------------------------------------------------------------------------------------
def test_salient_keypoints_sit_on_creases_and_repeat():
    """The crease scene sampled twice (A, B: 6000 points each, independent seeds), thinned at radius 0.08 with the saliency taken at
    0.16.  The share of kept keypoints within one salient_radius of a crease, and the share of A's keypoints that have a keypoint of B
    within radius / 2, for select_salient and for the hashed select_disk: printed, recorded in profiles/salient.md, and asserted in
    direction only - both are larger for select_salient."""
    import torch
    from scipy.spatial import cKDTree
    from yoho_amd import keypoints
    radius, sr = 0.08, 0.16
    ctx = host_context(rounds=64)
    kp = {}
    for name, seed in (("A", 21), ("B", 22)):
        pc, spacing = SR.crease_scene(6000, seed)
        pc_d = torch.from_numpy(pc)
        sal, sinfo = keypoints.select_salient(ctx, pc_d, radius, salient_radius=sr)
        dsk, dinfo = keypoints.select_disk(ctx, pc_d, radius)
        kp[name] = (pc[sal.numpy()], pc[dsk.numpy()])
        near = [float((SR.crease_distance(k) < sr).mean()) for k in kp[name]]
        share_all = float((SR.crease_distance(pc) < sr).mean())
        print(f"sampling {name}: spacing {spacing:.4f}, {share_all:.3f} of the points within {sr} of a crease; select_salient keeps {sinfo['kept']} "
              f"({sinfo['eligible']} eligible, {sinfo['rounds']} rounds), {near[0]:.3f} of them near a crease; select_disk keeps {dinfo['kept']} "
              f"({dinfo['rounds']} rounds), {near[1]:.3f} near a crease")
        assert near[0] > near[1]
    rep = [float((cKDTree(kp["B"][m]).query(kp["A"][m])[0] < radius / 2).mean()) for m in (0, 1)]
    print(f"repeatability A -> B within radius / 2 = {radius / 2}: select_salient {rep[0]:.3f}, select_disk {rep[1]:.3f}")
    assert rep[0] > rep[1]
