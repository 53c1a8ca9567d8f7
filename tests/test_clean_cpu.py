"""CPU tests of the outlier filters (include/yoho_clean.h, yoho_amd/clean.py): the library builds and exports exactly the
header's two symbols and its kernels compile without scratch at every list capacity; the two numpy restatements of the entries
(tests/clean_ref.py), which share no code, agree on seeded clouds; the motivating case - farthest-point sampling picks strays until the
filter has run -; and the opt-in consumers, through host hooks: with clean=None they return what they returned before."""
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
import keypoints_ref as KR  # noqa: E402
import refine_ref as RR  # noqa: E402

f32, f64 = np.float32, np.float64
KERNELS = {"cl_knn_kernel": 4, "cl_stat_kernel": 3, "cl_mean_kernel": 1, "cl_var_kernel": 1, "cl_thr_kernel": 1, "cl_keep_kernel": 1}


# ---- the library ---------------------------------------------------------------------------------------------------------------------------
def test_library_exports_clean_header_symbols():
    """include/yoho_clean.h declares exactly hip.CLEAN_SYMBOLS, the library exports both with their 12 and 13 arguments, the list shares
    nothing with the other ten, hip.SYMBOLS is still yoho_hip.h's set, the header's limit is the binding's and nothing leaked into the
    older headers"""
    import ctypes as C
    from yoho_amd import build, hip
    assert os.path.exists(build.build(verbose=False))
    lib = hip.load_library()
    hdr = open(os.path.join(REPO, "include", "yoho_clean.h")).read()
    fns = sorted(set(re.findall(r"\b(yoho_[a-zA-Z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert fns == ["yoho_knn_within", "yoho_statistical_outliers"] and hip.CLEAN_SYMBOLS == fns
    assert lib.yoho_knn_within.restype is C.c_int and len(lib.yoho_knn_within.argtypes) == 12 and lib.yoho_knn_within.argtypes[5] is C.c_float
    assert lib.yoho_statistical_outliers.restype is C.c_int and len(lib.yoho_statistical_outliers.argtypes) == 13
    assert lib.yoho_statistical_outliers.argtypes[3] is C.c_float and lib.yoho_statistical_outliers.argtypes[6] is C.c_double
    others = (hip.SYMBOLS + hip.KNN_SYMBOLS + hip.TRAINSET_SYMBOLS + hip.REFINE_SYMBOLS + hip.PLANE_SYMBOLS + hip.VERIFY_SYMBOLS + hip.CONSIST_SYMBOLS +
              hip.KEYPOINT_SYMBOLS + hip.MULTIWAY_SYMBOLS + hip.FUSE_SYMBOLS)
    assert not set(fns) & set(others)
    assert hip.KNN_SYMBOLS == ["yoho_knn_search"] and hip.REFINE_SYMBOLS == ["yoho_nn_within", "yoho_refit_matches", "yoho_icp_refine"]
    assert hip.PLANE_SYMBOLS == ["yoho_estimate_normals", "yoho_icp_plane"] and hip.FUSE_SYMBOLS == ["yoho_fuse_clouds"] and hip.KEYPOINT_SYMBOLS == ["yoho_fps"]
    main = open(os.path.join(REPO, "include", "yoho_hip.h")).read()
    main_fns = set(re.findall(r"\b(yoho_[a-zA-Z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", main, flags=re.S)))
    assert main_fns == set(hip.SYMBOLS) and len(hip.SYMBOLS) == len(set(hip.SYMBOLS))            # unchanged by the new entries
    for older in ("yoho_hip.h", "yoho_knn.h", "yoho_trainset.h", "yoho_refine.h", "yoho_plane.h", "yoho_verify.h", "yoho_consist.h", "yoho_keypoints.h",
                  "yoho_multiway.h", "yoho_fuse.h"):
        text = open(os.path.join(REPO, "include", older)).read()
        assert "yoho_knn_within" not in text and "yoho_statistical_outliers" not in text, older
    assert '#include "yoho_refine.h"' in hdr
    assert re.findall(r"#define\s+(\w+)", hdr) == ["YOHO_CLEAN_H", "YOHO_KNN3_MAX"]
    assert int(re.search(r"#define\s+YOHO_KNN3_MAX\s+(\d+)\b", hdr).group(1)) == hip.KNN3_MAX == CR.KNN3_MAX == 32
    assert build.EXTRA["clean.hip"] == ["-ffp-contract=off"] and "clean.hip" in build.SOURCES
    src = open(os.path.join(build.CSRC, "clean.hip")).read()
    assert re.findall(r'#include "([^"]+)"', src) == ["rfgrid.h", "rffit.h", "yoho_clean.h"]


def test_clean_kernels_use_no_scratch(tmp_path):
    """csrc/clean.hip compiled for gfx950 with the flags of the build: the eleven kernels - the walk at list capacities 0 (count only), 8,
    16 and 32, the filter's at 8, 16 and 32 -, none with scratch: the list is indexed by compile-time constants only and the 27 slots
    are parked in LDS.  The VGPR counts are printed; no bound on them is asserted."""
    from yoho_amd import build
    cmd = [build._hipcc()] + build.FLAGS + build.EXTRA["clean.hip"] + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                                                                      os.path.join(build.CSRC, "clean.hip"), "-o", str(tmp_path / "clean.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r"\bVGPRs: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == sum(KERNELS.values()), names
    for k, n in KERNELS.items():
        assert sum(k in name for name in names) == n, (k, names)
    for cap in (0, 8, 16, 32):
        assert sum(f"cl_knn_kernelILi{cap}E" in name for name in names) == 1, (cap, names)
    print("clean.hip: " + ", ".join(f"{n} {v} VGPRs" for n, v in zip(names, vgprs)))
    assert scratch == [0] * len(names), dict(zip(names, scratch))


# ---- the restatements ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
def test_the_two_restatements_agree(seed):
    """knn_within_ref (f32, all pairs a window on x leaves, a lexicographic sort) against knn_within_tree (a float64 cKDTree) on
    clean_ref.separated_cloud, which asserts that no two candidate distances of a row, and no distance and the gate, lie within 1e-6
    relative: indices and counts equal, distances within the f32 arithmetic's 3e-7 relative (five roundings of d2, halved by the
    root; 1e-6 is asserted); then the two filters: keep equal, the statistics within 1e-6 relative"""
    max_dist = 0.2
    for nq, k, skip in ((None, 1, True), (None, 8, True), (None, 20, False), (300, 5, False), (300, 32, False)):
        q, tgt = CR.separated_cloud(seed, 700, max_dist, nq)                     # seeds on which the generator's assertion holds
        idx, d2, count = CR.knn_within_ref(q, tgt, max_dist, k, skip)
        ti, td, tc = CR.knn_within_tree(q, tgt, max_dist, k, skip)
        assert np.array_equal(count, tc) and np.array_equal(idx, ti), (nq, k, skip)
        assert k in (1, 5, 32) or ((count < k).any() and (count > k).any())                     # rows short of k and rows beyond it
        there = idx >= 0
        assert np.array_equal(there, np.isfinite(td)) and (np.abs(np.sqrt(d2[there].astype(f64)) - td[there]) <= 1e-6 * td[there]).all()
        with np.errstate(invalid="ignore"):
            assert (d2[~there] == np.inf).all() and (np.diff(d2.astype(f64), axis=1)[there[:, 1:]] >= 0).all()
        if not skip and nq is None:
            assert (idx[:, 0] == np.arange(700)).all() and (d2[:, 0] == 0).all()              # a point is its own nearest neighbour
        if skip:
            assert not (idx == np.arange(700)[:, None]).any()
    pts = CR.separated_cloud(seed, 700, max_dist)[1]
    for k, min_found, ratio in ((8, 1, 2.0), (16, 3, 1.0), (4, 1, -0.5)):
        a, b = CR.statistical_ref(pts, max_dist, k, min_found, ratio), CR.statistical_tree(pts, max_dist, k, min_found, ratio)
        assert CR.assert_away_from_threshold(a, 1e-5) > 1e-5
        assert np.array_equal(a["count"], b["count"]) and np.array_equal(a["valid"], b["valid"]) and np.array_equal(a["keep"], b["keep"])
        assert a["n_keep"] == b["n_keep"] and 0 < a["n_keep"] < a["stats"][0] <= 700
        v = a["valid"]
        assert np.abs(a["mean_dist"][v] / b["mean_dist"][v] - 1).max() < 1e-6 and np.isnan(a["mean_dist"][~v]).all()
        assert np.abs(a["stats"] / b["stats"] - 1).max() < 1e-6


def test_restatement_identities_and_edges():
    """column 0 of knn_within_ref is refine_ref.nn_within_ref (the all-pairs form); duplicates order by index and stay candidates of one
    another; a distance equal to the gate is out; NaN and inf rows; the filter's edge values"""
    rs = np.random.RandomState(5)
    q, tgt = rs.rand(200, 3).astype(f32), rs.rand(300, 3).astype(f32)
    tgt[7], q[3], q[4] = [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [np.nan] * 3
    idx, d2, count = CR.knn_within_ref(q, tgt, 0.2, 4)
    i1, d1 = RR.nn_within_ref(q, tgt, 0.2, prefilter=False)
    assert np.array_equal(idx[:, 0], i1) and d2[:, 0].tobytes() == d1.tobytes()
    assert count[3] == 0 and count[4] == 0 and not (idx == 7).any() and (count > 4).any() and (0 < count).any() and ((0 < count) & (count < 4)).any()
    dup = np.tile(np.array([[0.25, 0.5, 0.75]], f32), (40, 1))
    idx, d2, count = CR.knn_within_ref(dup, dup, 0.1, 32, skip_same_row=True)
    assert (count == 39).all() and (d2 == 0).all()
    for i in (0, 17, 39):
        assert np.array_equal(idx[i], np.delete(np.arange(40), i)[:32])
    line = np.array([[0, 0, 0], [0.25, 0, 0], [0.5, 0, 0]], f32)                   # 0.25 is exact, its square is the gate
    assert np.array_equal(CR.knn_within_ref(line, line, 0.25, 2)[2], [1, 1, 1])
    assert np.array_equal(CR.knn_within_ref(line, line, np.nextafter(f32(0.25), f32(1)), 2)[2], [2, 3, 2])
    one = CR.statistical_ref(line[:1], 1.0, 4)
    assert one["stats"].tolist() == [0, 0, 0, 0] and not one["keep"].any() and np.isnan(one["mean_dist"]).all()
    two = CR.statistical_ref(line[:2], 1.0, 4)
    assert two["stats"].tolist() == [2, 0.25, 0, 0.25] and two["keep"].all()
    assert CR.statistical_ref(line, 1.0, 4, std_ratio=-1.0)["keep"].tolist() == [False, True, False]
    assert not CR.statistical_ref(line, 1.0, 2, min_found=3)["keep"].any()


# ---- the motivating case ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fps_picks_strays_until_the_filter_has_run(seed):
    """clean_ref.stray_cloud: synth.surface_cloud(20000, seed) plus 200 uniform strays in [-0.2, 1.4]^3, shuffled; 500 picks of
    keypoints_ref.fps_ref before and after statistical_ref(k = 16, max_dist = 0.05, 2 sigma), the f32 restatement.  Measured with it,
    seeds 0 / 1 / 2: 141 / 139 / 140 of the 500 picks are strays before the filter and 0 / 1 / 0 after; 13 / 11 / 17 strays are kept
    (the ones that lie on the surface); 1.55 / 1.68 / 1.47 % of the surface points are dropped; the m_i closest to thr is 4.4e-5 /
    9.7e-5 / 1.9e-4 relative away from it."""
    pts, stray = CR.stray_cloud(seed)
    assert pts.shape == (20200, 3) and stray.sum() == 200
    before = KR.fps_ref(pts, 500, 0)[0]
    ref = CR.statistical_ref(pts, 0.05, 16, 1, 2.0)
    closest = CR.assert_away_from_threshold(ref, 1e-9)
    kept = np.nonzero(ref["keep"])[0]
    after = kept[KR.fps_ref(pts[kept], 500, 0)[0]]
    dropped = float((~ref["keep"] & ~stray).sum()) / float((~stray).sum())
    print(f"seed {seed}: strays among 500 picks {stray[before].sum()} -> {stray[after].sum()}; strays kept {(ref['keep'] & stray).sum()}; surface points "
          f"dropped {100 * dropped:.2f} %; closest m to thr {closest:.1e}; stats {ref['stats'].tolist()}")
    assert stray[before].sum() >= 100
    assert stray[after].sum() <= 5
    assert (ref["keep"] & stray).sum() <= 20
    assert dropped < 0.025
    assert np.array_equal(after, CR.select_clean_ref(pts.astype(f64), 500, clean={"max_dist": 0.05}))


# ---- consumers -------------------------------------------------------------------------------------------------------------------------------
class HostContext:
    """the four Context methods keypoints.select and clean.statistical call, restated on host tensors"""

    def __init__(self):
        self.calls = []

    def fcgf_voxelize(self, pc_d, voxel):
        import torch
        return (torch.from_numpy(KR.voxel_first_ref(pc_d.numpy(), voxel)),)

    def rotate_select(self, pc_d, R, sel):
        import torch
        assert R is None
        return pc_d[sel].to(torch.float32).contiguous()

    def fps(self, pts, k, start=0):
        import torch
        idx, d2 = KR.fps_ref(pts.numpy(), k, start)
        return torch.from_numpy(idx), torch.from_numpy(d2)

    def statistical_outliers(self, pts, max_dist, k=16, min_found=1, std_ratio=2.0):
        import torch
        self.calls.append((pts.shape[0], max_dist, k, min_found, std_ratio))
        r = CR.statistical_ref(pts.numpy(), max_dist, k, min_found, std_ratio)
        return {"keep": torch.from_numpy(r["keep"].astype(np.uint8)), "mean_dist": torch.from_numpy(r["mean_dist"]), "count": torch.from_numpy(r["count"]),
                "stats": torch.from_numpy(r["stats"]), "n_keep": torch.tensor([r["n_keep"]], dtype=torch.int32)}

    def knn_within(self, q, tgt, max_dist, k, skip_same_row=False, want_idx=True, want_d2=True, want_count=True):
        import torch
        assert not want_idx and not want_d2 and want_count
        return None, None, torch.from_numpy(CR.knn_within_ref(q.numpy(), tgt.numpy(), max_dist, k, skip_same_row)[2])


def small_stray_cloud(seed):
    from yoho_amd import synth
    rs = np.random.RandomState(seed)
    pc = np.concatenate([synth.surface_cloud(1500, seed), rs.rand(30, 3) * 1.6 - 0.2])
    return np.ascontiguousarray(pc[rs.permutation(len(pc))])


def test_select_with_clean_equals_the_restatement_and_without_it_is_unchanged():
    import torch
    from yoho_amd import clean, keypoints
    pc = small_stray_cloud(3)
    pc_d = torch.from_numpy(pc)
    ctx = HostContext()
    for voxel, kw in ((0.05, {}), (0.05, {"k": 8, "std_ratio": 1.0}), (None, {"max_dist": 0.15, "min_found": 2}), (0.04, {"max_dist": 0.1})):
        got, dist2 = keypoints.select(ctx, pc_d, 60, voxel=voxel, clean=kw)
        want = CR.select_clean_ref(pc, 60, voxel=voxel, clean=kw)
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want) and len(want) == 60 and dist2.shape == (60,)
        assert len(np.intersect1d(want, KR.select_ref(pc, 60, voxel=voxel))) < 60                 # the filter changed the selection
    assert [c[1:] for c in ctx.calls] == [(4 * 0.05, 16, 1, 2.0), (4 * 0.05, 8, 1, 1.0), (0.15, 16, 2, 2.0), (0.1, 16, 1, 2.0)]
    with pytest.raises(ValueError, match="max_dist"):
        keypoints.select(ctx, pc_d, 60, voxel=None, clean={})
    n_calls = len(ctx.calls)
    for voxel in (0.05, None):
        got = keypoints.select(ctx, pc_d, 60, voxel=voxel)[0]
        assert np.array_equal(got.numpy(), KR.select_ref(pc, 60, voxel=voxel))
        assert np.array_equal(keypoints.select(ctx, pc_d, 60, voxel=voxel, clean=None)[0].numpy(), got.numpy())
    assert len(ctx.calls) == n_calls                                                            # clean=None never reaches the filter
    # the module's own entries on the same host context
    pts = torch.from_numpy(pc.astype(f32))
    r = clean.statistical(ctx, pts, k=8, max_dist=0.15)
    ref = CR.statistical_ref(pc.astype(f32), 0.15, 8)
    assert r["keep"].dtype == torch.bool and np.array_equal(r["keep"].numpy(), ref["keep"]) and np.array_equal(r["sel"].numpy(), np.nonzero(ref["keep"])[0])
    assert r["stats"].numpy().tobytes() == ref["stats"].tobytes() and set(r) >= {"keep", "sel", "mean_dist", "stats"}
    rr = clean.radius(ctx, pts, 0.1, 5)
    want = CR.radius_ref(pc.astype(f32), 0.1, 5)["keep"]
    assert np.array_equal(rr["keep"].numpy(), want) and 0 < want.sum() < len(want) and set(rr) >= {"keep", "sel", "mean_dist", "stats"}
    sel, kept = clean.clean_cloud(ctx, pc_d, method="radius", radius=0.1, min_nbrs=5)
    assert np.array_equal(sel.numpy(), np.nonzero(want)[0]) and kept.dtype == torch.float64 and np.array_equal(kept.numpy(), pc[want])
    sel, kept = clean.clean_cloud(ctx, pc_d, k=8, max_dist=0.15)
    assert np.array_equal(sel.numpy(), np.nonzero(ref["keep"])[0]) and np.array_equal(kept.numpy(), pc[ref["keep"]])
    with pytest.raises(ValueError, match="max_dist"):
        clean.statistical(ctx, pts)
    with pytest.raises(ValueError, match="method"):
        clean.clean_cloud(ctx, pc_d, method="median")


def test_write_keypoints_forwards_clean_to_its_selector(tmp_path):
    """a selector is called with clean only when there is one: the three-argument selectors of before keep working, and the files hold
    the filtered selection"""
    from test_keypoints_cpu import make_dataset
    from yoho_amd import keypoints
    clouds = [small_stray_cloud(k)[:400 + 30 * k] for k in range(2)]
    ds = make_dataset(str(tmp_path / "scene"), clouds)
    old = lambda pc, nkpts, voxel: KR.select_ref(pc, nkpts, voxel=voxel)      # noqa: E731
    assert keypoints.write_keypoints(ds, nkpts=16, voxel=0.1, selector=old) == ["0", "1"]
    plain = [np.loadtxt(ds.kps_fn[k]).astype(int) for k in range(2)]
    seen = []

    def new(pc, nkpts, voxel, clean=None):
        seen.append(clean)
        return CR.select_clean_ref(pc, nkpts, voxel=voxel, clean=clean)

    kw = {"k": 6, "max_dist": 0.3, "std_ratio": 0.5}
    assert keypoints.write_keypoints(ds, nkpts=16, voxel=0.1, selector=new, clean=kw, overwrite=True) == ["0", "1"]
    assert seen == [kw, kw]
    for k in range(2):
        pc = ds.get_pc(str(k))
        want = CR.select_clean_ref(pc, 16, voxel=0.1, clean=kw)
        assert np.array_equal(np.loadtxt(ds.kps_fn[k]).astype(int), want) and np.array_equal(np.load(ds.kps_pc_fn[k]), pc[want])
        assert np.array_equal(plain[k], KR.select_ref(pc, 16, voxel=0.1)) and not np.array_equal(plain[k], want)
    with pytest.raises(TypeError):
        keypoints.write_keypoints(ds, nkpts=16, voxel=0.1, selector=old, clean=kw, overwrite=True)


def test_extractor_takes_keypoint_clean_in_fps_mode_only():
    from yoho_amd.yoho_extract import yoho_extractor
    with pytest.raises(ValueError, match="keypoint_clean"):
        yoho_extractor(fcgf_ckpt=None, yoho_ckpt={}, keypoints="random", keypoint_clean={"max_dist": 0.1})
    with pytest.raises(ValueError, match="keypoint_clean"):
        yoho_extractor(fcgf_ckpt=None, yoho_ckpt={}, keypoint_clean={})


def test_write_scene_cloud_filters_the_fused_rows(tmp_path):
    """scene.ply with clean: the rows the filter keeps, with their normals, count and nfrag; without: the bytes of before"""
    import fuse_ref as FR
    from test_multiway_cpu import make_scene
    from yoho_amd import RR_cal
    from yoho_amd import fuse as FU
    from yoho_amd.run_dataset import result_dir
    cfg = types.SimpleNamespace(output_cache_fn=str(tmp_path / "cache"), RR_dist_threshold=0.2)
    ds, _, _ = make_scene(str(tmp_path / "data" / "sceneA"), "synthcl/sceneA", 0)
    out_dir = result_dir(cfg, ds, "YOHO_O_MW", 1000)
    os.makedirs(out_dir)
    RR_cal.write_trajectory(np.stack([np.eye(4)] * 5), [(f, f, 5) for f in range(5)], os.path.join(out_dir, "poses.log"))

    def host_fuse(clouds, poses, voxel, min_count, min_frags):
        nrm = [np.roll(c, 1, axis=1).astype(f32) for c in clouds]
        return FR.fuse_ref(np.concatenate(clouds), FR.soff_of(clouds), poses[:, :3, :], voxel, min_count, min_frags, np.concatenate(nrm))

    seen = []

    def host_clean(out, kw):
        seen.append(kw)
        keep = CR.statistical_ref(out["pts"], kw["max_dist"], kw.get("k", 16), kw.get("min_found", 1), kw.get("std_ratio", 2.0))["keep"]
        return FU.filter_rows(out, np.nonzero(keep)[0])

    path, full = FU.write_scene_cloud(cfg, ds, voxel=0.05, fuse=host_fuse)
    raw = open(path, "rb").read()
    FU.write_ply(str(tmp_path / "again.ply"), full["pts"], full["normals"], full["count"], full["nfrag"])
    assert raw == open(str(tmp_path / "again.ply"), "rb").read() and "row_of" in full and seen == []
    path2, out = FU.write_scene_cloud(cfg, ds, voxel=0.05, fuse=host_fuse, clean={"k": 8, "std_ratio": 1.0}, cleaner=host_clean)
    assert path2 == path and seen == [{"k": 8, "std_ratio": 1.0, "max_dist": 4 * 0.05}]
    keep = CR.statistical_ref(full["pts"], 0.2, 8, 1, 1.0)["keep"]
    assert 0 < keep.sum() < full["M"] and out["M"] == keep.sum()
    back = FU.read_ply(path)
    for k in ("pts", "normals", "count", "nfrag"):
        assert back[k].tobytes() == full[k][keep].tobytes() == out[k].tobytes(), k
    FU.write_scene_cloud(cfg, ds, voxel=0.05, fuse=host_fuse, clean={"max_dist": 0.3}, cleaner=host_clean)
    assert seen[-1] == {"max_dist": 0.3}
