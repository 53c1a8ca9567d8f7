"""CPU tests of the density clusters (include/yoho_cluster.h, yoho_amd/cluster.py): the library builds and exports exactly
the header's symbol and its kernels compile without scratch; the two numpy restatements of the entry (tests/cluster_ref.py), which
share no code, agree on separated clouds; the restatement at the contract's edges; the motivating case - farthest-point sampling
gives every stray clump a keypoint and the statistical filter keeps the clumps, until the small clusters are dropped -; and the
Python layer and the opt-in consumers over a host context built from the restatement: without a "method" key they do what they did."""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(REPO, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(REPO, "tests"))
import clean_ref as CR  # noqa: E402
import cluster_ref as CL  # noqa: E402
import keypoints_ref as KR  # noqa: E402

f32, f64 = np.float32, np.float64
KERNELS = ["cu_count_kernel", "cu_union_kernel", "cu_root_kernel", "cu_scan_kernel", "cu_label_kernel"]


# ---- the library ---------------------------------------------------------------------------------------------------------------------------
def test_library_exports_cluster_header_symbol():
    """include/yoho_cluster.h declares exactly hip.CLUSTER_SYMBOLS, the library exports it with its 11 arguments, the list shares
    nothing with the other eleven, which are what they were, hip.SYMBOLS is still yoho_hip.h's set and nothing leaked into the older
    headers"""
    import ctypes as C
    from yoho_amd import build, hip
    assert os.path.exists(build.build(verbose=False))
    lib = hip.load_library()
    hdr = open(os.path.join(REPO, "include", "yoho_cluster.h")).read()
    fns = sorted(set(re.findall(r"\b(yoho_[a-zA-Z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert fns == ["yoho_dbscan"] and hip.CLUSTER_SYMBOLS == fns
    assert lib.yoho_dbscan.restype is C.c_int and len(lib.yoho_dbscan.argtypes) == 11
    assert lib.yoho_dbscan.argtypes[3] is C.c_float and lib.yoho_dbscan.argtypes[4] is C.c_int
    others = (hip.SYMBOLS + hip.KNN_SYMBOLS + hip.TRAINSET_SYMBOLS + hip.REFINE_SYMBOLS + hip.PLANE_SYMBOLS + hip.VERIFY_SYMBOLS + hip.CONSIST_SYMBOLS +
              hip.KEYPOINT_SYMBOLS + hip.MULTIWAY_SYMBOLS + hip.FUSE_SYMBOLS + hip.CLEAN_SYMBOLS)
    assert not set(fns) & set(others)
    assert hip.KNN_SYMBOLS == ["yoho_knn_search"] and hip.REFINE_SYMBOLS == ["yoho_nn_within", "yoho_refit_matches", "yoho_icp_refine"]
    assert hip.PLANE_SYMBOLS == ["yoho_estimate_normals", "yoho_icp_plane"] and hip.FUSE_SYMBOLS == ["yoho_fuse_clouds"] and hip.KEYPOINT_SYMBOLS == ["yoho_fps"]
    assert hip.CLEAN_SYMBOLS == ["yoho_knn_within", "yoho_statistical_outliers"] and hip.TRAINSET_SYMBOLS == ["yoho_radius_pairs", "yoho_trainset_gather"]
    assert hip.VERIFY_SYMBOLS == ["yoho_eval_transforms", "yoho_verify_hypotheses"] and hip.MULTIWAY_SYMBOLS == ["yoho_edge_information"]
    assert hip.CONSIST_SYMBOLS == ["yoho_consistency_graph", "yoho_sc2_scores", "yoho_consensus_hypotheses"]
    main = open(os.path.join(REPO, "include", "yoho_hip.h")).read()
    main_fns = set(re.findall(r"\b(yoho_[a-zA-Z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", main, flags=re.S)))
    assert main_fns == set(hip.SYMBOLS) and len(hip.SYMBOLS) == len(set(hip.SYMBOLS))            # unchanged by the new entry
    for older in ("yoho_hip.h", "yoho_knn.h", "yoho_trainset.h", "yoho_refine.h", "yoho_plane.h", "yoho_verify.h", "yoho_consist.h", "yoho_keypoints.h",
                  "yoho_multiway.h", "yoho_fuse.h", "yoho_clean.h"):
        assert "yoho_dbscan" not in open(os.path.join(REPO, "include", older)).read(), older
    assert '#include "yoho_refine.h"' in hdr
    assert re.findall(r"#define\s+(\w+)", hdr) == ["YOHO_CLUSTER_H"]
    assert build.EXTRA["cluster.hip"] == ["-ffp-contract=off"] and "cluster.hip" in build.SOURCES
    src = open(os.path.join(build.CSRC, "cluster.hip")).read()
    assert re.findall(r'#include "([^"]+)"', src) == ["rfgrid.h", "yoho_cluster.h"]


def test_cluster_kernels_use_no_scratch(tmp_path):
    """csrc/cluster.hip compiled for gfx950 with the flags of the build: its five kernels, none with scratch.  The VGPR counts are
    printed; no bound on them is asserted."""
    from yoho_amd import build
    cmd = [build._hipcc()] + build.FLAGS + build.EXTRA["cluster.hip"] + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                                                                        os.path.join(build.CSRC, "cluster.hip"), "-o", str(tmp_path / "cluster.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r"\bVGPRs: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == len(KERNELS), names
    for k in KERNELS:
        assert sum(k in name for name in names) == 1, (k, names)
    print("cluster.hip: " + ", ".join(f"{n} {v} VGPRs" for n, v in zip(names, vgprs)))
    assert scratch == [0] * len(names), dict(zip(names, scratch))


# ---- the restatements ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,eps,seed", [(300, 0.15, 0), (300, 0.15, 1), (1500, 0.09, 0), (1500, 0.09, 1)])
def test_the_two_restatements_agree(n, eps, seed):
    """dbscan_ref (f32, a window on x, its own union-find) against dbscan_independent (a float64 cKDTree, scipy's connected components)
    on clean_ref.separated_cloud, which asserts that no pair distance lies within 1e-6 relative of eps: the core set, the partition of
    the core rows up to renaming, the noise set, and every border row in the cluster of one of its core neighbours"""
    pytest.importorskip("scipy")
    pts = CR.separated_cloud(seed, n, eps)[1]
    for min_pts in (1, 4, 8):
        ref = CL.dbscan_ref(pts, eps, min_pts)
        CL.assert_agree(ref, CL.dbscan_independent(pts, eps, min_pts))
        assert np.array_equal(ref["count"], CR.knn_within_ref(pts, pts, eps, 1, skip_same_row=True)[2])
        nc, ncore, nnoise = ref["n"].tolist()
        assert ref["sizes"][:nc].sum() == n - nnoise and (ref["sizes"][:nc] > 0).all() and (ref["sizes"][nc:] == 0).all()
        if min_pts == 1:
            assert ncore == n and nnoise == 0 and nc > 1
        else:
            assert 0 < ncore < n and 0 < nnoise < n and nc > 1 and ((ref["core"] == 0) & (ref["labels"] >= 0)).any()      # cores, borders, noise


def first_appearance_is_ascending(ref):
    """the numbering rule: the labels of the core rows, in row order, first appear as 0, 1, 2, ..."""
    lab = ref["labels"][ref["core"].astype(bool)]
    _, first = np.unique(lab, return_index=True)
    return np.array_equal(lab[np.sort(first)], np.arange(int(ref["n"][0])))


def test_restatement_at_the_edges():
    """the snake in five row orders, two snakes with and without a bridge, the tie on a lattice, the gate, duplicates, non-finite
    rows and the numbering under a permutation - the cases tests/test_gpu_cluster.py runs on the device, here on dbscan_ref alone"""
    eps = 0.05
    chain = CL.snake(2049, eps)
    assert len(np.unique(np.floor(chain[:, :2] / eps), axis=0)) > 1000            # it crosses many cells
    for name, perm in CL.snake_orders(2049).items():
        for min_pts in (1, 3):
            ref = CL.dbscan_ref(chain[perm], eps, min_pts)
            assert (ref["labels"] == 0).all() and ref["n"].tolist() == [1, 2049 if min_pts == 1 else 2047, 0] and ref["sizes"][0] == 2049, (name, min_pts)
    for swap in (False, True):
        pts, lo, up, _ = CL.two_snakes(eps, swap=swap)
        ref = CL.dbscan_ref(pts, eps, 4)
        assert ref["n"][0] == 2 and (ref["labels"][lo] == (1 if swap else 0)).all() and (ref["labels"][up] == (0 if swap else 1)).all()
        pts, lo, up, b = CL.two_snakes(eps, bridge=True, swap=swap)
        ref = CL.dbscan_ref(pts, eps, 4)                                           # the bridge has two neighbours: not core
        assert ref["n"][0] == 2 and ref["count"][b] == 2 and not ref["core"][b] and ref["labels"][b] == ref["labels"][lo[0]] != ref["labels"][up[0]]
        ref = CL.dbscan_ref(pts, eps, 3)                                           # core: it joins the two
        assert ref["n"][0] == 1 and ref["core"][b] and (ref["labels"] == 0).all()
    for swap in (False, True):
        pts, ra, rb, rp = CL.tie_cloud(swap)
        ref = CL.dbscan_ref(pts, 1.2, 5)
        assert ref["n"].tolist() == [2, 2, 0] and ref["core"][ra] and ref["core"][rb] and not ref["core"][rp] and ref["count"][rp] == 2
        assert ref["labels"][rp] == ref["labels"][min(ra, rb)] == 0 and ref["labels"][max(ra, rb)] == 1      # equal d2: the lower row
    line = np.zeros((9, 3), f32)
    line[:, 0] = 0.5 * np.arange(9)                                               # d2 = 0.25 = gate2: not neighbours
    ref = CL.dbscan_ref(line, 0.5, 1)
    assert np.array_equal(ref["labels"], np.arange(9)) and (ref["count"] == 0).all() and (ref["sizes"] == 1).all() and ref["n"].tolist() == [9, 9, 0]
    assert (CL.dbscan_ref(line, 0.5, 2)["labels"] == -1).all()
    assert CL.dbscan_ref(line, np.nextafter(f32(0.5), f32(1)), 2)["n"].tolist() == [1, 9, 0]
    dup = np.tile(np.array([[0.25, 0.5, 0.75]], f32), (40, 1))
    for min_pts in (1, 40):
        ref = CL.dbscan_ref(dup, 0.1, min_pts)
        assert (ref["labels"] == 0).all() and (ref["count"] == 39).all() and ref["sizes"][0] == 40 and ref["n"].tolist() == [1, 40, 0]
    assert CL.dbscan_ref(dup, 0.1, 41)["n"].tolist() == [0, 0, 40]
    pts = CL.mixed_cloud(257, 0.1)
    bad, good = CL.with_bad_rows(pts)
    for min_pts in (1, 4):
        a, b = CL.dbscan_ref(pts, 0.1, min_pts), CL.dbscan_ref(bad, 0.1, min_pts)
        rest = np.setdiff1d(np.arange(len(bad)), good)
        assert (b["labels"][rest] == -1).all() and (b["count"][rest] == 0).all() and (b["core"][rest] == 0).all()
        for k in ("labels", "count", "core"):
            assert np.array_equal(a[k], b[k][good]), k                             # the others: as without them (the order of the rows is kept)
        assert b["n"].tolist() == [a["n"][0], a["n"][1], a["n"][2] + len(rest)]
    perm = np.random.RandomState(3).permutation(257)
    a, b = CL.dbscan_ref(pts, 0.1, 4), CL.dbscan_ref(pts[perm], 0.1, 4)
    assert first_appearance_is_ascending(a) and first_appearance_is_ascending(b) and not np.array_equal(a["labels"][perm], b["labels"])
    assert np.array_equal(a["core"][perm], b["core"]) and np.array_equal(a["labels"][perm] < 0, b["labels"] < 0)
    core = b["core"].astype(bool)
    assert len(set(zip(a["labels"][perm][core].tolist(), b["labels"][core].tolist()))) == a["n"][0] == b["n"][0]      # the same partition


# ---- the motivating case ---------------------------------------------------------------------------------------------------------------------
def motivating_conditions(pts, clump, keep, after):
    """what keep_large(min_size = 100) has to achieve on clump_cloud: no clump point kept, at least 99.9 % of the surface kept, and no
    pick of the 500 that follow (`after`: rows of pts) in a clump"""
    surface = clump < 0
    assert (keep & ~surface).sum() == 0
    assert (keep & surface).sum() >= 0.999 * surface.sum()
    assert (clump[after] >= 0).sum() == 0 and len(after) == 500


@pytest.mark.parametrize("seed,clumps", [(0, 4), (1, 12)])
def test_fps_picks_every_clump_until_the_small_clusters_are_dropped(seed, clumps):
    """cluster_ref.clump_cloud: synth.surface_cloud(20000, seed) plus 4 / 12 clumps of 30 points, sigma 0.004, more than 0.15 from the
    surface.  500 picks of keypoints_ref.fps_ref put a pick into every clump; statistical_ref(max_dist = 0.05, k = 16) keeps the clump
    points (all of them, 120 of 120 and 360 of 360; at least 90 % is asserted); dbscan_ref(eps = 0.04, min_pts = 4) with clusters
    below 100 members dropped keeps none of them, 19 996 and 20 000 of the 20 000 surface points, and no pick falls into a clump
    afterwards."""
    pts, clump, ref = CL.motivating(seed)
    nclump = 30 * clumps
    assert pts.shape == (20000 + nclump, 3) and clump.max() + 1 == clumps and (clump >= 0).sum() == nclump
    before = KR.fps_ref(pts, 500, 0)[0]
    hit = np.unique(clump[before][clump[before] >= 0])
    stat = CR.statistical_ref(pts, 0.05, 16)["keep"]
    keep = CL.keep_large_ref(ref, min_size=100)
    kept = np.nonzero(keep)[0]
    after = kept[KR.fps_ref(pts[kept], 500, 0)[0]]
    print(f"seed {seed}: {len(hit)} of {clumps} clumps picked before; statistical keeps {(stat & (clump >= 0)).sum()} of {nclump} clump points; clusters "
          f"{ref['n'].tolist()}, keep_large keeps {(keep & (clump >= 0)).sum()} clump and {(keep & (clump < 0)).sum()} surface points; picks in clumps after "
          f"{(clump[after] >= 0).sum()}")
    assert len(hit) == clumps
    assert (stat & (clump >= 0)).sum() >= 0.9 * nclump
    motivating_conditions(pts, clump, keep, after)


# ---- the Python layer and the consumers --------------------------------------------------------------------------------------------------------
def host_context():
    from test_clean_cpu import HostContext

    class ClusterContext(HostContext):
        """test_clean_cpu's host context with Context.dbscan restated through dbscan_ref"""

        def dbscan(self, pts, eps, min_pts=4, want_count=True, want_core=True, want_sizes=True):
            import torch
            self.calls.append(("dbscan", pts.shape[0], eps, min_pts))
            r = CL.dbscan_ref(pts.numpy(), eps, min_pts)
            return {"labels": torch.from_numpy(r["labels"]), "count": torch.from_numpy(r["count"]), "core": torch.from_numpy(r["core"]),
                    "sizes": torch.from_numpy(r["sizes"]), "n": torch.from_numpy(r["n"])}

    return ClusterContext()


def test_keep_large_and_clean_cloud_over_the_restatement():
    import torch
    from yoho_amd import clean, cluster
    ctx = host_context()
    pc = CL.mixed_cloud(1023, 0.1).astype(f64)
    pts = torch.from_numpy(pc.astype(f32))
    ref = CL.dbscan_ref(pc.astype(f32), 0.1, 4)
    r = cluster.dbscan(ctx, pts, 0.1)
    assert set(r) == {"labels", "count", "core", "sizes", "n"} and all(np.array_equal(r[k].numpy(), ref[k]) for k in r)
    one = cluster.components(ctx, pts, 0.1)
    assert ctx.calls[-1] == ("dbscan", 1023, 0.1, 1) and np.array_equal(one["labels"].numpy(), CL.dbscan_ref(pc.astype(f32), 0.1, 1)["labels"])
    sizes = ref["sizes"][:ref["n"][0]]
    assert len(set(sizes.tolist())) < len(sizes) and sizes.max() > 60 > sizes.min()                  # sizes tie, and 60 splits them
    got = cluster.keep_large(ctx, pts, 0.1, min_size=60)
    want = CL.keep_large_ref(ref, min_size=60)
    assert got["keep"].dtype == torch.bool and np.array_equal(got["keep"].numpy(), want) and 0 < want.sum() < (ref["labels"] >= 0).sum()
    assert np.array_equal(want, (ref["labels"] >= 0) & (ref["sizes"][np.maximum(ref["labels"], 0)] >= 60))
    assert np.array_equal(got["sel"].numpy(), np.nonzero(want)[0]) and got["sel"].dtype == torch.int64
    assert got["mean_dist"] is None and got["stats"] is None and set(got) == {"keep", "sel", "mean_dist", "stats", "labels", "sizes", "n"}
    assert np.array_equal(got["labels"].numpy(), ref["labels"]) and np.array_equal(got["sizes"].numpy(), ref["sizes"])
    # largest: by members, ties to the lower id
    order = sorted(range(len(sizes)), key=lambda c: (-int(sizes[c]), c))
    tied = [k for k in range(1, len(order)) if sizes[order[k]] == sizes[order[k - 1]]]
    for n in (1, 2, tied[0], tied[0] + 1, len(sizes), len(sizes) + 5):                              # tied[0]: a cut between two clusters of one size
        got = cluster.keep_large(ctx, pts, 0.1, largest=n)["keep"].numpy()
        assert np.array_equal(got, np.isin(ref["labels"], order[:n])) and np.array_equal(got, CL.keep_large_ref(ref, largest=n)), n
    assert order[tied[0] - 1] < order[tied[0]]
    for kw in ({}, {"min_size": 10, "largest": 1}, {"min_size": 0}, {"largest": 0}):
        with pytest.raises(ValueError, match="keep_large"):
            cluster.keep_large(ctx, pts, 0.1, **kw)
    with pytest.raises(ValueError, match="empty"):
        cluster.dbscan(ctx, pts[:0], 0.1)
    assert clean.METHODS["cluster"] is cluster.keep_large and sorted(clean.METHODS) == ["cluster", "radius", "statistical"]
    sel, kept = clean.clean_cloud(ctx, torch.from_numpy(pc), method="cluster", eps=0.1, min_size=60)
    assert np.array_equal(sel.numpy(), np.nonzero(want)[0]) and kept.dtype == torch.float64 and np.array_equal(kept.numpy(), pc[want])
    assert ctx.calls[-1] == ("dbscan", 1023, 0.1, 4)


def select_cluster_ref(pc, nkpts, voxel, eps, min_pts, min_size):
    sel = np.arange(len(pc), dtype=np.int64) if voxel is None else KR.voxel_first_ref(pc, voxel)
    pts = np.asarray(pc, dtype=f64)[sel].astype(f32)
    keep = CL.keep_large_ref(CL.dbscan_ref(pts, eps, min_pts), min_size=min_size)
    sel, pts = sel[keep], pts[keep]
    return sel[KR.fps_ref(pts, min(nkpts, len(sel)), 0)[0]]


def test_select_takes_a_method_and_without_it_is_unchanged():
    import torch
    from test_clean_cpu import small_stray_cloud
    from yoho_amd import keypoints
    pc = small_stray_cloud(3)
    pc_d = torch.from_numpy(pc)
    ctx = host_context()
    got = keypoints.select(ctx, pc_d, 60, voxel=0.05, clean={"method": "cluster", "min_size": 50})[0]
    assert ctx.calls[-1][0] == "dbscan" and ctx.calls[-1][2:] == (4 * 0.05, 4)                   # eps defaults to 4 voxels
    want = select_cluster_ref(pc, 60, 0.05, 4 * 0.05, 4, 50)
    assert np.array_equal(got.numpy(), want) and len(np.intersect1d(want, KR.select_ref(pc, 60, voxel=0.05))) < 60
    got = keypoints.select(ctx, pc_d, 60, voxel=None, clean={"method": "cluster", "eps": 0.15, "min_pts": 3, "largest": 1})[0]
    assert ctx.calls[-1] == ("dbscan", len(pc), 0.15, 3) and len(got) == 60
    with pytest.raises(ValueError, match="eps"):
        keypoints.select(ctx, pc_d, 60, voxel=None, clean={"method": "cluster", "min_size": 50})
    with pytest.raises(ValueError, match="method"):
        keypoints.select(ctx, pc_d, 60, voxel=0.05, clean={"method": "median"})
    got = keypoints.select(ctx, pc_d, 60, voxel=0.05, clean={"method": "radius", "min_nbrs": 3})[0]
    assert len(got) == 60
    # without the key, and with "statistical" spelled out: the calls and the selection of before
    ctx.calls.clear()
    for kw in ({}, {"k": 8, "std_ratio": 1.0}, {"max_dist": 0.1}):
        got = keypoints.select(ctx, pc_d, 60, voxel=0.05, clean=kw)[0]
        assert np.array_equal(got.numpy(), CR.select_clean_ref(pc, 60, voxel=0.05, clean=kw))
        again = keypoints.select(ctx, pc_d, 60, voxel=0.05, clean={"method": "statistical", **kw})[0]
        assert np.array_equal(again.numpy(), got.numpy())
    assert [c[1:] for c in ctx.calls] == [(0.2, 16, 1, 2.0)] * 2 + [(0.2, 8, 1, 1.0)] * 2 + [(0.1, 16, 1, 2.0)] * 2
    with pytest.raises(ValueError, match="max_dist"):
        keypoints.select(ctx, pc_d, 60, voxel=None, clean={})


def test_clean_fused_and_write_scene_cloud_take_a_method(tmp_path, monkeypatch):
    """fuse.clean_fused dispatches on "method" and without it calls the statistical filter with the arguments of before;
    write_scene_cloud defaults eps, not max_dist, to 4 voxels for "cluster" and hands the key on to its cleaner"""
    import torch
    from test_clean_cpu import small_stray_cloud
    from test_multiway_cpu import make_scene
    from yoho_amd import RR_cal
    from yoho_amd import fuse as FU
    from yoho_amd.run_dataset import result_dir
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)              # the host context's tensors stay where they are
    ctx = host_context()
    pts = small_stray_cloud(4).astype(f32)
    out = {"pts": pts, "normals": np.roll(pts, 1, axis=1), "count": np.arange(len(pts), dtype=np.int32), "nfrag": np.ones(len(pts), np.int32), "M": len(pts)}
    got = FU.clean_fused(ctx, out, {"method": "cluster", "eps": 0.2, "min_size": 50})
    keep = CL.keep_large_ref(CL.dbscan_ref(pts, 0.2, 4), min_size=50)
    assert ctx.calls == [("dbscan", len(pts), 0.2, 4)] and 0 < keep.sum() < len(pts) and got["M"] == keep.sum()
    for k in ("pts", "normals", "count", "nfrag"):
        assert got[k].tobytes() == out[k][keep].tobytes(), k
    ctx.calls.clear()
    got = FU.clean_fused(ctx, out, {"max_dist": 0.2, "k": 8})
    keep = CR.statistical_ref(pts, 0.2, 8)["keep"]
    assert ctx.calls == [(len(pts), 0.2, 8, 1, 2.0)] and got["pts"].tobytes() == pts[keep].tobytes()
    same = FU.clean_fused(ctx, out, {"method": "statistical", "max_dist": 0.2, "k": 8})
    assert same["pts"].tobytes() == got["pts"].tobytes() and ctx.calls[1] == ctx.calls[0]
    with pytest.raises(ValueError, match="method"):
        FU.clean_fused(ctx, out, {"method": "median"})

    cfg = types.SimpleNamespace(output_cache_fn=str(tmp_path / "cache"), RR_dist_threshold=0.2)
    ds, _, _ = make_scene(str(tmp_path / "data" / "sceneA"), "synthcl/sceneA", 0)
    out_dir = result_dir(cfg, ds, "YOHO_O_MW", 1000)
    os.makedirs(out_dir)
    RR_cal.write_trajectory(np.stack([np.eye(4)] * 5), [(f, f, 5) for f in range(5)], os.path.join(out_dir, "poses.log"))

    def host_fuse(clouds, poses, voxel, min_count, min_frags):
        import fuse_ref as FR
        return FR.fuse_ref(np.concatenate(clouds), FR.soff_of(clouds), poses[:, :3, :], voxel, min_count, min_frags, None)

    seen = []

    def host_clean(out, kw):
        seen.append(dict(kw))
        return FU.clean_fused(ctx, out, kw)

    path, full = FU.write_scene_cloud(cfg, ds, voxel=0.05, fuse=host_fuse)
    _, part = FU.write_scene_cloud(cfg, ds, voxel=0.05, fuse=host_fuse, clean={"method": "cluster", "largest": 1}, cleaner=host_clean)
    assert seen == [{"method": "cluster", "largest": 1, "eps": 4 * 0.05}]
    keep = CL.keep_large_ref(CL.dbscan_ref(full["pts"], 0.2, 4), largest=1)
    assert part["M"] == keep.sum() > 0 and FU.read_ply(path)["pts"].tobytes() == full["pts"][keep].tobytes()
    FU.write_scene_cloud(cfg, ds, voxel=0.05, fuse=host_fuse, clean={"method": "cluster", "eps": 0.3, "min_size": 5}, cleaner=host_clean)
    FU.write_scene_cloud(cfg, ds, voxel=0.05, fuse=host_fuse, clean={"k": 8}, cleaner=host_clean)
    assert seen[1:] == [{"method": "cluster", "eps": 0.3, "min_size": 5}, {"k": 8, "max_dist": 4 * 0.05}]
