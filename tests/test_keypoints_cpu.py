"""CPU tests of the keypoint entry (include/yoho_keypoints.h): the library builds and exports exactly its symbol, its kernels
compile without scratch, the numpy restatement (tests/keypoints_ref.py) has the properties the header states, farthest-point sampling
covers the cloud that motivated it at least twice as well as the reference's random draw, and write_keypoints leaves the files
ThrDMatchPartDataset.get_kps reads."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(REPO, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(REPO, "tests"))
import keypoints_ref as KR  # noqa: E402

f32 = np.float32


def header():
    return open(os.path.join(REPO, "include", "yoho_keypoints.h")).read()


def header_constants():
    """(YOHO_FPS_MAX_POINTS, YOHO_FPS_ONE_WG_MAX, YOHO_FPS_BLOCK_POINTS, {path name: value}) as the header defines them"""
    hdr = header()
    num = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)\b", hdr).group(1))      # noqa: E731
    big = 1 << int(re.search(r"#define\s+YOHO_FPS_MAX_POINTS\s+\(1 << (\d+)\)", hdr).group(1))
    return big, num("YOHO_FPS_ONE_WG_MAX"), num("YOHO_FPS_BLOCK_POINTS"), {"auto": num("YOHO_FPS_AUTO"), "one_wg": num("YOHO_FPS_ONE_WG"), "per_pick": num("YOHO_FPS_PER_PICK")}


def test_library_exports_keypoint_header_symbol():
    """include/yoho_keypoints.h declares exactly hip.KEYPOINT_SYMBOLS, the library exports it, the list shares nothing with the other
    seven, hip.SYMBOLS is still yoho_hip.h's set, the header's constants are the binding's, and nothing leaked into the older headers"""
    import ctypes as C
    from yoho_amd import build, hip
    assert os.path.exists(build.build(verbose=False))
    lib = hip.load_library()
    hdr = header()
    fns = sorted(set(re.findall(r"\b(yoho_[a-zA-Z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert fns == ["yoho_fps"] and hip.KEYPOINT_SYMBOLS == ["yoho_fps"]
    assert hasattr(lib, "yoho_fps") and lib.yoho_fps.restype is C.c_int and len(lib.yoho_fps.argtypes) == 9
    others = hip.SYMBOLS + hip.KNN_SYMBOLS + hip.TRAINSET_SYMBOLS + hip.REFINE_SYMBOLS + hip.PLANE_SYMBOLS + hip.VERIFY_SYMBOLS + hip.CONSIST_SYMBOLS
    assert "yoho_fps" not in others
    main = open(os.path.join(REPO, "include", "yoho_hip.h")).read()
    main_fns = set(re.findall(r"\b(yoho_[a-zA-Z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", main, flags=re.S)))
    assert main_fns == set(hip.SYMBOLS) and len(hip.SYMBOLS) == len(set(hip.SYMBOLS))            # unchanged by the new entry
    for older in ("yoho_hip.h", "yoho_knn.h", "yoho_trainset.h", "yoho_refine.h", "yoho_plane.h", "yoho_verify.h", "yoho_consist.h"):
        assert "yoho_fps" not in open(os.path.join(REPO, "include", older)).read(), older
    assert '#include "yoho_hip.h"' in hdr
    assert re.findall(r"#define\s+(\w+)", hdr) == ["YOHO_KEYPOINTS_H", "YOHO_FPS_MAX_POINTS", "YOHO_FPS_ONE_WG_MAX", "YOHO_FPS_BLOCK_POINTS", "YOHO_FPS_AUTO",
                                                   "YOHO_FPS_ONE_WG", "YOHO_FPS_PER_PICK"]
    big, one, blk, paths = header_constants()
    assert big == hip.FPS_MAX_POINTS == 1 << 22 and one == hip.FPS_ONE_WG_MAX >= 8192 and blk == hip.FPS_BLOCK_POINTS >= 64
    assert paths == hip.FPS_PATHS == {"auto": 0, "one_wg": 1, "per_pick": 2}
    assert build.EXTRA["keypoints.hip"] == ["-ffp-contract=off"] and "keypoints.hip" in build.SOURCES


def test_keypoint_kernels_use_no_scratch(tmp_path):
    """csrc/keypoints.hip compiled for gfx950 with the flags of the build: the one-workgroup kernel in its five sizes and the per-pick
    kernel, none with scratch (a spill would put the running minima of the one-workgroup path into memory), the one-workgroup kernel
    within the 128 registers a thread of a 1024-thread workgroup may hold"""
    from yoho_amd import build
    cmd = [build._hipcc()] + build.FLAGS + build.EXTRA["keypoints.hip"] + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                                                                          os.path.join(build.CSRC, "keypoints.hip"), "-o", str(tmp_path / "keypoints.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r"\bVGPRs: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == 6, names
    assert sum("fps_one_wg_kernel" in n for n in names) == 5 and sum("fps_pick_kernel" in n for n in names) == 1
    print("keypoints.hip: " + ", ".join(f"{n} {v} VGPRs" for n, v in zip(names, vgprs)))
    assert scratch == [0] * 6, dict(zip(names, scratch))
    assert max(vgprs) <= 128, dict(zip(names, vgprs))


def small_clouds():
    rs = np.random.RandomState(11)
    yield "uniform", rs.rand(400, 3).astype(f32), 60
    yield "normal", rs.randn(257, 3).astype(f32), 257
    yield "lattice", np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(f32), 125
    yield "duplicates", np.repeat(rs.rand(20, 3).astype(f32), 7, axis=0), 140
    yield "one point", np.zeros((1, 3), f32), 1


@pytest.mark.parametrize("name,p,k", list(small_clouds()), ids=[c[0] for c in small_clouds()])
def test_reference_properties(name, p, k):
    """the properties the header promises, on the restatement itself"""
    m = len(p)
    for start in sorted({0, m // 3, m - 1}):
        idx, d2 = KR.fps_ref(p, k, start)
        assert idx[0] == start and d2[0] == np.inf and d2.dtype == f32 and idx.dtype == np.int64
        assert len(set(idx.tolist())) == k and idx.min() >= 0 and idx.max() < m                    # k distinct picks
        assert (np.diff(d2[1:]) <= 0).all() and (d2[1:] >= 0).all()                              # dist2[1:] does not increase
        for kk in (1, k // 2):                                                                    # a shorter selection is a prefix
            if kk >= 1:
                i2, e2 = KR.fps_ref(p, kk, start)
                assert np.array_equal(i2, idx[:kk]) and e2.tobytes() == d2[:kk].tobytes()
        # after s picks every point lies within sqrt(dist2[s]) of a pick (the float32 distances the rule itself uses)
        for s in sorted({1, k // 2, k - 1}):
            if 1 <= s < k:
                near = np.min(np.stack([KR.dist2_ref(p, p[c]) for c in idx[:s]]), axis=0)
                assert near.max() == d2[s], (name, start, s)
    if name == "duplicates":                                                                      # every distinct point once before any copy
        idx, d2 = KR.fps_ref(p, k, 0)
        assert len(np.unique(p[idx[:20]], axis=0)) == 20 and (d2[20:] == 0).all() and (d2[1:20] > 0).all()
    if name == "lattice":                                                                         # exact ties: the lowest index wins
        idx, d2 = KR.fps_ref(p, 3, 0)
        # (4,4,4) is farthest from the origin; then the six permutations of (0,2,4) tie at min(20, 20): (0,2,4) = index 14 is the lowest
        assert idx.tolist() == [0, 124, 14] and d2[1] == 48 and d2[2] == 20


def test_voxel_first_reference():
    pc = np.array([[0.01, 0.01, 0.01], [0.02, 0.02, 0.02], [0.03, 0.0, 0.0], [-0.02, 0.0, 0.0], [0.026, 0.001, 0.02], [0.0, 0.0, 0.0]])
    assert KR.voxel_first_ref(pc, 0.025).tolist() == [0, 2, 3]
    assert KR.select_ref(pc, 10, voxel=0.025).tolist() == [0, 3, 2] and KR.select_ref(pc, 2, voxel=None, start=5).tolist() == [5, 1]


@pytest.mark.parametrize("seed", range(5))
def test_fps_covers_the_skewed_wall_twice_as_well_as_the_random_draw(seed):
    """the reason for the feature, as a condition: on a cloud whose density falls with the distance, 500 farthest-point keys leave at
    most half the radius uncovered that 500 uniformly drawn scan points leave (the restatement alone gives ratios of 2.8 - 4.5)"""
    p, rnd = KR.skewed_wall(seed)
    assert p.shape == (20000, 3) and rnd.shape == (500,)
    idx, d2 = KR.fps_ref(p, 500, 0)
    r_fps, r_rnd = KR.coverage_radius_ref(p, p[idx]), KR.coverage_radius_ref(p, p[rnd])
    print(f"skewed_wall({seed}): coverage radius random {r_rnd:.4f}, fps {r_fps:.4f}, ratio {r_rnd / r_fps:.2f}")
    assert 2 * r_fps <= r_rnd
    # the running minimum bounds the radius from above: the next pick would be the worst-covered point
    assert r_fps <= np.sqrt(float(d2[-1])) * (1 + 1e-6)


def make_dataset(root, clouds):
    from yoho_amd.dataset import ThrDMatchPartDataset
    os.makedirs(os.path.join(root, "PointCloud"))
    for k, pc in enumerate(clouds):
        np.savetxt(os.path.join(root, "PointCloud", f"cloud_bin_{k}.txt"), pc, delimiter=",")
    with open(os.path.join(root, "PointCloud", "gt.log"), "w") as f:
        f.write("0 1 2\n1 0 0 0\n0 1 0 0\n0 0 1 0\n0 0 0 1\n")
    return ThrDMatchPartDataset(root, len(clouds))


def test_write_keypoints_leaves_the_files_get_kps_reads(tmp_path):
    """with a stub selector (no device): index and point files in get_kps's formats, read back as pc[indices]; get_kps no longer draws;
    existing index files are left alone unless overwrite is set"""
    from yoho_amd import keypoints
    rs = np.random.RandomState(4)
    clouds = [rs.rand(40 + 7 * k, 3) for k in range(3)]
    ds = make_dataset(str(tmp_path / "scene"), clouds)
    calls = []

    def stub(pc, nkpts, voxel):
        calls.append((len(pc), nkpts, voxel))
        return KR.select_ref(pc, nkpts, voxel=voxel)

    os.makedirs(os.path.dirname(ds.kps_fn[1]))
    np.savetxt(ds.kps_fn[1], np.array([5, 3, 1]))                                                  # cloud 1 already has its index file
    assert keypoints.write_keypoints(ds, nkpts=16, voxel=0.1, selector=stub) == ["0", "2"]
    assert calls == [(40, 16, 0.1), (54, 16, 0.1)]
    state = np.random.get_state()
    for k in (0, 2):
        pc = ds.get_pc(str(k))
        want = KR.select_ref(pc, 16, voxel=0.1)
        assert len(want) == 16
        assert np.array_equal(np.loadtxt(ds.kps_fn[k]).astype(int), want)
        assert np.array_equal(np.load(ds.kps_pc_fn[k]), pc[want])
        assert np.array_equal(ds.get_kps(str(k)), pc[want])
    assert np.array_equal(ds.get_kps("1"), ds.get_pc("1")[[5, 3, 1]])                             # left alone
    now = np.random.get_state()
    assert state[0] == now[0] and np.array_equal(state[1], now[1]) and state[2:] == now[2:]      # get_kps never reached its random draw
    assert keypoints.write_keypoints(ds, nkpts=16, voxel=0.1, selector=stub) == []                # nothing lacks its files now
    assert keypoints.write_keypoints(ds, nkpts=8, voxel=None, selector=stub, overwrite=True) == ["0", "1", "2"]
    assert np.array_equal(ds.get_kps("1"), ds.get_pc("1")[KR.select_ref(ds.get_pc("1"), 8)])


def test_extractor_refuses_an_unknown_keypoint_mode():
    from yoho_amd.yoho_extract import yoho_extractor
    with pytest.raises(ValueError, match="keypoints"):
        yoho_extractor(fcgf_ckpt=None, yoho_ckpt={}, keypoints="grid")
