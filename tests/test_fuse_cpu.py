"""CPU tests of the fused scene (include/yoho_fuse.h, yoho_amd/fuse.py): the library builds and exports exactly the
header's symbol and its kernels compile without scratch; the two numpy restatements of the entry (tests/fuse_ref.py), which share no
code, agree in every output; a fragment that lies apart from the scene is removed exactly by min_frags = 2; no inside point is lost;
and the files: PLY round trips, scene.ply beside poses.log."""
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
import fuse_ref as FR  # noqa: E402
from yoho_amd import RR_cal  # noqa: E402
from yoho_amd import fuse as FU  # noqa: E402

f32, f64 = np.float32, np.float64
KERNELS = ("fu_key_kernel", "fu_plan_kernel", "fu_pack_kernel", "fu_hist_kernel", "fu_scatter_kernel", "fu_tile_sum_kernel", "fu_tile_scan_kernel",
           "fu_count_kernel", "fu_heads_kernel", "fu_emit_kernel")


# ---- the library ---------------------------------------------------------------------------------------------------------------------------
def test_library_exports_fuse_header_symbol():
    """include/yoho_fuse.h declares exactly hip.FUSE_SYMBOLS, the library exports it with its 17 arguments, the list shares nothing with
    the other nine, hip.SYMBOLS is still yoho_hip.h's set, the header's two limits are the binding's, nothing leaked into the older
    headers, and the header says in words what soff is"""
    import ctypes as C
    from yoho_amd import build, hip
    assert os.path.exists(build.build(verbose=False))
    lib = hip.load_library()
    hdr = open(os.path.join(REPO, "include", "yoho_fuse.h")).read()
    fns = sorted(set(re.findall(r"\b(yoho_[a-zA-Z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert fns == ["yoho_fuse_clouds"] and hip.FUSE_SYMBOLS == fns
    assert lib.yoho_fuse_clouds.restype is C.c_int and len(lib.yoho_fuse_clouds.argtypes) == 17
    assert lib.yoho_fuse_clouds.argtypes[6] is C.c_double and lib.yoho_fuse_clouds.argtypes[14] is C.c_int64
    others = (hip.SYMBOLS + hip.KNN_SYMBOLS + hip.TRAINSET_SYMBOLS + hip.REFINE_SYMBOLS + hip.PLANE_SYMBOLS + hip.VERIFY_SYMBOLS + hip.CONSIST_SYMBOLS +
              hip.KEYPOINT_SYMBOLS + hip.MULTIWAY_SYMBOLS)
    assert "yoho_fuse_clouds" not in others
    main = open(os.path.join(REPO, "include", "yoho_hip.h")).read()
    main_fns = set(re.findall(r"\b(yoho_[a-zA-Z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", main, flags=re.S)))
    assert main_fns == set(hip.SYMBOLS) and len(hip.SYMBOLS) == len(set(hip.SYMBOLS))            # unchanged by the new entry
    for older in ("yoho_hip.h", "yoho_knn.h", "yoho_trainset.h", "yoho_refine.h", "yoho_plane.h", "yoho_verify.h", "yoho_consist.h", "yoho_keypoints.h",
                  "yoho_multiway.h"):
        assert "yoho_fuse_clouds" not in open(os.path.join(REPO, "include", older)).read(), older
    assert '#include "yoho_refine.h"' in hdr
    assert re.findall(r"#define\s+(\w+)", hdr) == ["YOHO_FUSE_H", "YOHO_FUSE_MAX_K", "YOHO_FUSE_MAX_POINTS"]
    assert int(re.search(r"#define\s+YOHO_FUSE_MAX_K\s+(\d+)\b", hdr).group(1)) == hip.FUSE_MAX_K == 1024
    assert 1 << int(re.search(r"#define\s+YOHO_FUSE_MAX_POINTS\s+\(1 << (\d+)\)", hdr).group(1)) == hip.FUSE_MAX_POINTS == 1 << 26
    assert build.EXTRA["fuse.hip"] == ["-ffp-contract=off"] and "fuse.hip" in build.SOURCES
    assert "HOST array" in hdr and "by value" in hdr and "strictly increasing" in hdr and "ASCENDING GLOBAL ROW" in hdr


def test_fuse_kernels_use_no_scratch(tmp_path):
    """csrc/fuse.hip compiled for gfx950 with the flags of the build: the ten kernels (fu_emit_kernel with and without normals), none
    with scratch - the fragment table and the two buffer pairs passed by value are read with scalar loads and selects, not copied to
    private memory to be indexed.  The VGPR counts are printed; no bound on them has been measured, so none is asserted."""
    from yoho_amd import build
    cmd = [build._hipcc()] + build.FLAGS + build.EXTRA["fuse.hip"] + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                                                                     os.path.join(build.CSRC, "fuse.hip"), "-o", str(tmp_path / "fuse.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r"\bVGPRs: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == 11, names
    for k in KERNELS:
        assert sum(k in n for n in names) == (2 if k == "fu_emit_kernel" else 1), (k, names)
    print("fuse.hip: " + ", ".join(f"{n} {v} VGPRs" for n, v in zip(names, vgprs)))
    assert scratch == [0] * 11, dict(zip(names, scratch))


# ---- the restatements ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("mc,mf", [(1, 1), (2, 1), (1, 2), (3, 2)])
def test_the_two_restatements_agree(seed, mc, mf):
    """fuse_ref (numpy, uint64 keys, np.add.at) against fuse_dict (Python floats, a dictionary of cells) as bytes, on fuse_ref.seeded_case:
    negative coordinates, points exactly on voxel faces, duplicated points, a NaN pose, a NaN and an infinite point, a point beyond the
    cell range.  The case is what its docstring says: checked here once"""
    c = FR.seeded_case(seed)
    a = FR.fuse_ref(c["src"], c["soff"], c["T"], c["voxel"], mc, mf, c["nrm"])
    b = FR.fuse_dict(c["src"], c["soff"], c["T"], c["voxel"], mc, mf, c["nrm"])
    assert FR.same_bytes(a, b) == [] and a["inside"] == b["inside"] and a["all_count"].tobytes() == b["all_count"].tobytes()
    a0 = FR.fuse_ref(c["src"], c["soff"], c["T"], c["voxel"], mc, mf)
    b0 = FR.fuse_dict(c["src"], c["soff"], c["T"], c["voxel"], mc, mf)
    assert FR.same_bytes(a0, b0) == [] and a0["normals"] is None and FR.same_bytes(a, a0, ("pts", "count", "nfrag", "row_of")) == []
    so, ro = c["soff"], a["row_of"]
    if (mc, mf) == (1, 1):
        assert (ro[so[2]:so[3]] == -1).all()                             # the NaN pose removes its fragment
        assert ro[so[4] + 7] == -1 and ro[so[4] + 11] == -1 and (np.delete(ro[so[4]:so[5]], [7, 11]) >= 0).all()      # the NaN and the infinite point
        assert ro[so[4] - 2] >= 0 and ro[so[4] - 1] == -1                # cell 2^20 - 1 is inside, cell 2^20 is not
        assert (ro[so[3]:so[4]] == -1).sum() > 1 and (ro[so[3]:so[4]] >= 0).sum() > 10
        assert a["count"].max() >= 2 and a["M"] == len(a["all_count"]) and a["pts"][:, 0].min() < -0.5
        # a lattice point k * voxel lies in cell k, not k - 1: its voxel's mean is >= it on every axis
        lat = c["src"][:120]
        assert np.array_equal(np.floor(lat.astype(f64) / c["voxel"]) * c["voxel"], lat.astype(f64))
        assert (a["normals"] == 0).all(axis=1).sum() >= 1                # the NaN normal's voxel
    if mf == 2:
        assert np.array_equal(ro[so[1]:so[2]], ro[so[5]:so[6]]) and (mc > 2 or (ro[so[1]:so[2]] >= 0).all())      # fragment 1 and its copy: two points per voxel at least
        assert a["nfrag"].min() >= 2 and a["count"].min() >= mc and 0 < a["M"] < len(a["all_count"])


def test_ghost_fragment_is_removed_by_min_frags():
    """fuse_ref.ghost_scene: the six fragments of multiway_ref.scene_case under their poses and one fragment 1 m away from everything.
    It shares no voxel with the rest, so with min_frags = 2 none of its points has a row and with min_frags = 1 all of them have"""
    g = FR.ghost_scene()
    src, soff, T = np.concatenate(g["clouds"]), FR.soff_of(g["clouds"]), g["poses"][:, :3, :]
    k = g["ghost"]
    one = FR.fuse_ref(src, soff, T, g["voxel"], 1, 1)
    two = FR.fuse_ref(src, soff, T, g["voxel"], 1, 2)
    assert (one["row_of"] >= 0).all() and one["M"] == len(one["all_count"])
    assert (two["row_of"][soff[k]:soff[k + 1]] == -1).all()
    assert (two["row_of"][:soff[k]] >= 0).mean() > 0.5 and two["nfrag"].min() >= 2 and two["nfrag"].max() >= 4
    ghost_rows = np.unique(one["row_of"][soff[k]:soff[k + 1]])
    assert (one["nfrag"][ghost_rows] == 1).all() and not np.intersect1d(ghost_rows, one["row_of"][:soff[k]]).size
    assert two["M"] < one["M"] - len(ghost_rows) + 1


@pytest.mark.parametrize("mc,mf", [(1, 1), (2, 2)])
def test_no_inside_point_is_lost(mc, mf):
    """sum(count) over kept plus dropped voxels is the number of inside points; the kept counts are the counts of the rows row_of names"""
    c = FR.seeded_case(2)
    for fn in (FR.fuse_ref, FR.fuse_dict):
        a = fn(c["src"], c["soff"], c["T"], c["voxel"], mc, mf)
        assert int(a["all_count"].sum()) == a["inside"] and 0 < a["inside"] < len(c["src"])
        assert np.array_equal(np.bincount(a["row_of"][a["row_of"] >= 0], minlength=a["M"]), a["count"])
        assert int(a["count"].sum()) + int(a["all_count"].sum() - a["count"].sum()) == a["inside"]
        if (mc, mf) == (1, 1):
            assert (a["row_of"] >= 0).sum() == a["inside"]


# ---- files ---------------------------------------------------------------------------------------------------------------------------------
def test_ply_round_trip_is_byte_exact(tmp_path):
    c = FR.seeded_case(3)
    a = FR.fuse_ref(c["src"], c["soff"], c["T"], c["voxel"], 1, 1, c["nrm"])
    for name, kw in (("full", dict(normals=a["normals"], count=a["count"], nfrag=a["nfrag"])), ("bare", {}), ("counts", dict(count=a["count"], nfrag=a["nfrag"]))):
        p1, p2 = str(tmp_path / f"{name}.ply"), str(tmp_path / f"{name}2.ply")
        FU.write_ply(p1, a["pts"], **kw)
        back = FU.read_ply(p1)
        assert back["pts"].dtype == f32 and back["pts"].tobytes() == a["pts"].tobytes()
        for k in ("normals", "count", "nfrag"):
            want = kw.get(k)
            assert (back[k] is None) == (want is None) and (want is None or (back[k].dtype == want.dtype and back[k].tobytes() == want.tobytes())), k
        FU.write_ply(p2, back["pts"], back["normals"], back["count"], back["nfrag"])
        raw = open(p1, "rb").read()
        assert raw == open(p2, "rb").read()
        assert raw.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\n" % a["M"])
        per = 12 + (12 if "normals" in kw else 0) + (8 if "count" in kw else 0)
        assert len(raw) == raw.index(b"end_header\n") + 11 + per * a["M"]
    FU.write_ply(str(tmp_path / "empty.ply"), np.zeros((0, 3), f32), count=np.zeros((0,), np.int32))
    e = FU.read_ply(str(tmp_path / "empty.ply"))
    assert e["pts"].shape == (0, 3) and e["count"].shape == (0,) and e["normals"] is None and e["nfrag"] is None


def test_write_scene_cloud_beside_poses_log(tmp_path):
    """poses.log as multiway.write_scene leaves it (five poses, the last one nan) + the dataset's clouds -> scene.ply beside it, equal to
    the restatement on the poses AS READ from the log; the host hook replaces the device pass and sees what the device pass would"""
    from test_multiway_cpu import make_scene
    from yoho_amd.multiway import _scene_clouds
    from yoho_amd.run_dataset import result_dir
    import multiway_ref as MR
    cfg = types.SimpleNamespace(output_cache_fn=str(tmp_path / "cache"), RR_dist_threshold=0.2)
    ds, _, _ = make_scene(str(tmp_path / "data" / "sceneA"), "synthfu/sceneA", 0)
    rs = np.random.RandomState(0)
    rs.rand(700, 3)
    Xg = np.stack([np.eye(4)] + [MR.motion(MR.random_direction(rs) * 0.8 * rs.rand(), rs.randn(3) * 0.5) for _ in range(4)])      # make_scene's poses
    Xg[4] = np.nan
    out_dir = result_dir(cfg, ds, "YOHO_O_MW", 1000)
    os.makedirs(out_dir)
    RR_cal.write_trajectory(Xg, [(f, f, 5) for f in range(5)], os.path.join(out_dir, "poses.log"))
    calls = []

    def host_fuse(clouds, poses, voxel, min_count, min_frags):
        calls.append((len(clouds), poses.shape, voxel, min_count, min_frags))
        return FR.fuse_ref(np.concatenate(clouds), FR.soff_of(clouds), poses[:, :3, :], voxel, min_count, min_frags)

    path, out = FU.write_scene_cloud(cfg, ds, voxel=0.05, min_frags=2, fuse=host_fuse)
    assert path == os.path.join(out_dir, "scene.ply") and calls == [(5, (5, 4, 4), 0.05, 1, 2)]
    clouds = _scene_clouds(ds)
    _, poses = RR_cal.read_trajectory(os.path.join(out_dir, "poses.log"))
    assert np.isnan(poses[4]).all() and np.abs(poses[:4] - Xg[:4]).max() < 1e-11
    ref = FR.fuse_ref(np.concatenate(clouds), FR.soff_of(clouds), poses[:, :3, :], 0.05, 1, 2)
    back = FU.read_ply(path)
    assert FR.same_bytes({**back, "row_of": None, "M": len(back["pts"])}, {**ref, "row_of": None}) == []
    # the fragments are subsets of one cloud: under the right poses most voxels are seen twice, and the nan pose's fragment is gone
    so = FR.soff_of(clouds)
    assert ref["M"] > 100 and ref["nfrag"].min() >= 2 and ref["nfrag"].max() == 4 and (ref["row_of"][so[4]:] == -1).all()
    # the defaults: YOHO_O_MW, voxel 0.025, every voxel
    path2, out2 = FU.write_scene_cloud(cfg, ds, fuse=host_fuse)
    assert path2 == path and calls[1] == (5, (5, 4, 4), 0.025, 1, 1) and len(FU.read_ply(path)["pts"]) == out2["M"] > ref["M"]
