"""CPU tests of the consensus entries (include/yoho_consist.h): the library builds and exports exactly their symbols, their
kernels compile without scratch, the numpy restatement of their contracts (tests/consist_ref.py) follows the header's rules on hand-made
inputs, and on the pairs that motivated them - verify_ref.decoy_case, where the vote's best 8 are all decoys - the match list alone gives
one hypothesis per cluster and the verification picks the true one."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import consist_ref as CR  # noqa: E402
import refine_ref as RR  # noqa: E402
import verify_ref as VR  # noqa: E402

f64 = np.float64
KERNELS = ("cg_graph_kernel", "cg_deg_kernel", "cg_sc2_kernel", "cs_seed_kernel", "cs_sval_kernel", "cs_sum1_kernel", "cs_mean_kernel", "cs_cov_kernel",
           "cs_solve_kernel")


def test_library_exports_consist_header_symbols():
    """include/yoho_consist.h declares exactly hip.CONSIST_SYMBOLS, the library exports them, the list shares nothing with the other
    six, the header's limits are the binding's, and nothing of it leaked into the older headers"""
    import ctypes as C
    from yoho_amd import build, hip
    assert os.path.exists(build.build(verbose=False))
    lib = hip.load_library()
    hdr = open(os.path.join(REPO, "include", "yoho_consist.h")).read()
    fns = sorted(set(re.findall(r"\b(yoho_[a-zA-Z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert fns == ["yoho_consensus_hypotheses", "yoho_consistency_graph", "yoho_sc2_scores"]
    for f in fns:
        assert hasattr(lib, f), f"libyoho_hip.so does not export {f}"
    assert set(fns) == set(hip.CONSIST_SYMBOLS) and len(hip.CONSIST_SYMBOLS) == 3
    assert not set(hip.CONSIST_SYMBOLS) & set(hip.SYMBOLS + hip.KNN_SYMBOLS + hip.TRAINSET_SYMBOLS + hip.REFINE_SYMBOLS + hip.PLANE_SYMBOLS + hip.VERIFY_SYMBOLS)
    for f, nargs in (("yoho_consistency_graph", 9), ("yoho_sc2_scores", 5), ("yoho_consensus_hypotheses", 12)):
        assert getattr(lib, f).restype is C.c_int and len(getattr(lib, f).argtypes) == nargs
    assert '#include "yoho_refine.h"' in hdr and re.findall(r"#define\s+(\w+)", hdr) == ["YOHO_CONSIST_H", "YOHO_CONSIST_MAX_M", "YOHO_CONSIST_MAX_K"]
    assert 1 << int(re.search(r"#define\s+YOHO_CONSIST_MAX_M\s+\(1 << (\d+)\)", hdr).group(1)) == hip.CONSIST_MAX_M == 1 << 14
    assert int(re.search(r"#define\s+YOHO_CONSIST_MAX_K\s+(\d+)", hdr).group(1)) == hip.CONSIST_MAX_K == hip.VERIFY_MAX_K == 64
    assert (hip.CONSIST_MAX_M - 1) * (hip.CONSIST_MAX_M - 2) < 2 ** 28                  # the header's bound on s2
    for older in ("yoho_hip.h", "yoho_knn.h", "yoho_trainset.h", "yoho_refine.h", "yoho_plane.h", "yoho_verify.h"):
        txt = open(os.path.join(REPO, "include", older)).read()
        assert not any(f in txt for f in fns), older
    assert build.EXTRA["consist.hip"] == ["-ffp-contract=off"] and "consist.hip" in build.SOURCES
    assert "SYMMETRIC BY" in hdr and "2^28" in hdr                                         # the two statements the header owes its callers


def test_consist_kernels_use_no_scratch(tmp_path):
    """csrc/consist.hip compiled for gfx950 with the flags of the build: the compiler's resource report names the nine kernels (the score
    kernel in its two forms), none with scratch (a spill)"""
    from yoho_amd import build
    cmd = [build._hipcc()] + build.FLAGS + build.EXTRA["consist.hip"] + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                                                                        os.path.join(build.CSRC, "consist.hip"), "-o", str(tmp_path / "consist.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r"\bVGPRs: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == 10, names
    for k in KERNELS:
        assert sum(k in n for n in names) == (2 if k == "cg_sc2_kernel" else 1), (k, names)
    print("consist.hip: " + ", ".join(f"{re.search(r'c[gs]_[a-z0-9]+_kernel', n).group(0)}{'<' + re.search(r'ILb(.)E', n).group(1) + '>' if 'sc2' in n else ''} {v} VGPRs" for n, v in zip(names, vgprs)))
    assert scratch == [0] * 10, dict(zip(names, scratch))


def lattice_case():
    """three matches whose lengths are exact: k0 sides 3, 4, 5; k1 sides 4, 4, sqrt(32).  Pair (0, 1) has a = 3, b = 4: |a - b| = 1 exactly"""
    k0 = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0]], f64)
    k1 = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], f64)
    return k0, k1


def test_reference_graph_rules():
    up, down = lambda x: np.nextafter(f64(x), f64(np.inf)), lambda x: np.nextafter(f64(x), f64(-np.inf))
    k0, k1 = lattice_case()
    # '<' at the tolerance: a difference of exactly 1 is out at tol = 1 and in one ulp above; (0, 2) differs by 0, (1, 2) by 0.657
    assert CR.compat_ref(k0, k1, 1.0).astype(int).tolist() == [[0, 0, 1], [0, 0, 1], [1, 1, 0]]
    assert CR.compat_ref(k0, k1, up(1.0)).astype(int).tolist() == [[0, 1, 1], [1, 0, 1], [1, 1, 0]]
    assert CR.compat_ref(k0, k1, down(1.0)).astype(int).tolist() == [[0, 0, 1], [0, 0, 1], [1, 1, 0]]
    # '>=' at the shortest length: a = 3 stays at min_len = 3 and leaves one ulp above; min_len looks at both sides (b = 4 of pair (0, 2))
    assert CR.compat_ref(k0, k1, up(1.0), 3.0).astype(int).tolist() == [[0, 1, 1], [1, 0, 1], [1, 1, 0]]
    assert CR.compat_ref(k0, k1, up(1.0), up(3.0)).astype(int).tolist() == [[0, 0, 1], [0, 0, 1], [1, 1, 0]]
    assert CR.compat_ref(k0, k1, up(1.0), up(4.0)).astype(int).tolist() == [[0, 0, 0], [0, 0, 1], [0, 1, 0]]
    # duplicated keypoints: a = b = 0 is compatible at min_len = 0 and not above; a NaN or infinite coordinate is compatible with nobody
    kd0, kd1 = np.vstack([k0, k0[1:2]]), np.vstack([k1, k1[1:2]])
    assert CR.compat_ref(kd0, kd1, 0.5)[1, 3] and not CR.compat_ref(kd0, kd1, 0.5, 1e-300)[1, 3]
    for bad in (np.nan, np.inf):
        kn = kd0.copy()
        kn[2, 1] = bad
        C = CR.compat_ref(kn, kd1, 100.0)
        assert not C[2].any() and not C[:, 2].any() and C[0, 1] and C[1, 3]
    # packing: symmetric, zero diagonal, zero tail bits, degrees, at the word edges
    for M in (1, 63, 64, 65, 129):
        p = CR.planted_case(M, M // 3, M)
        bits, deg = CR.graph_ref(p["k0"], p["k1"], 0.3)
        assert bits.shape == (M, (M + 63) // 64) and bits.dtype == np.uint64 and deg.dtype == np.int32
        C = CR.unpack(bits, M)
        assert np.array_equal(C[:, :M], C[:, :M].T) and not C[:, :M].diagonal().any() and not C[:, M:].any()
        assert np.array_equal(C[:, :M], CR.compat_ref(p["k0"], p["k1"], 0.3)) and np.array_equal(deg, C.sum(axis=1))
        if M >= 63:
            assert deg.max() > 0
        # bit j % 64 of word j // 64
        i, j = np.nonzero(C[:, :M])
        assert all((int(bits[a, b // 64]) >> (int(b) % 64)) & 1 for a, b in zip(i[:50], j[:50]))
        s2, S = CR.sc2_ref(bits, M, want_S=True)
        Ci = C[:, :M].astype(np.int64)
        assert np.array_equal(s2, ((Ci @ Ci) * Ci).sum(axis=1)) and np.array_equal(S, S.T) and s2.dtype == np.int32


def test_reference_seed_and_set_rules():
    # two triangles sharing nothing, and a pendant: seeds by score, lowest index among equals, a seed kills its neighbours
    C = np.zeros((9, 9), bool)
    for a, b in ((0, 1), (1, 2), (0, 2), (3, 4), (4, 5), (3, 5), (5, 6), (3, 6), (4, 6), (7, 0)):
        C[a, b] = C[b, a] = True
    bits = CR.pack(C)
    s2 = CR.sc2_ref(bits, 9)
    assert s2.tolist() == [2, 2, 2, 6, 6, 6, 6, 0, 0]                                  # 3 .. 6 are a 4-clique; 7 hangs on 0, 8 is alone
    rs = np.random.RandomState(0)
    k1 = rs.rand(9, 3)
    T_gt = RR.perturbed(CR.IDENTITY, rs, 40, 0.3)
    k0 = k1 @ T_gt[:, :3].T + T_gt[:, 3]
    r = CR.consensus_ref(k0, k1, bits, s2, 4)
    assert r["Kc"] == 2 and r["seeds"].tolist() == [3, 0, -1, -1] and r["sizes"].tolist() == [4, 3, 0, 0] and r["info"].tolist() == [2, 9]
    assert [np.nonzero(s)[0].tolist() for s in r["sets"]] == [[3, 4, 5, 6], [0, 1, 2]]   # 7 shares no neighbour with 0: 2 * 0 < Smax = 1
    assert np.abs(r["T"][:2] - T_gt).max() < 1e-12 and np.array_equal(r["T"][2:], np.tile(CR.IDENTITY, (2, 1, 1)))
    assert CR.consensus_ref(k0, k1, bits, s2, 1)["seeds"].tolist() == [3]
    # a set of two: the seed's best partner shares five neighbours with it, each of which shares only that partner - half of the maximum
    # keeps none of them, two matches leave the rotation open: a NaN row and a negative size.  (s2 >= 1 does not promise three members.)
    C = np.zeros((7, 7), bool)
    for k in range(2, 7):
        C[0, k] = C[k, 0] = C[1, k] = C[k, 1] = True
    C[0, 1] = C[1, 0] = True
    bits = CR.pack(C)
    s2 = CR.sc2_ref(bits, 7)
    assert s2.tolist() == [10, 10, 2, 2, 2, 2, 2]
    r = CR.consensus_ref(k0[:7], k1[:7], bits, s2, 2)
    assert r["Kc"] == 1 and r["seeds"].tolist() == [0, -1] and r["sizes"].tolist() == [-2, 0] and np.isnan(r["T"][0]).all()
    # collinear matches keep all their distances: one clique, one set, rank below 2
    line = np.arange(6, dtype=f64)[:, None] * np.array([[1.0, 2.0, -2.0]])
    bits, _ = CR.graph_ref(line, line + 5.0, 0.01)
    r = CR.consensus_ref(line, line + 5.0, bits, CR.sc2_ref(bits, 6), 3)
    assert r["Kc"] == 1 and r["sizes"].tolist() == [-6, 0, 0] and np.isnan(r["T"][0]).all() and np.array_equal(r["T"][1], CR.IDENTITY)
    # nobody in a triangle: no seed
    bits, _ = CR.graph_ref(k0[:2], k1[:2], 0.01)
    r = CR.consensus_ref(k0[:2], k1[:2], bits, CR.sc2_ref(bits, 2), 2)
    assert r["Kc"] == 0 and r["seeds"].tolist() == [-1, -1] and r["info"].tolist() == [0, 2]


def decoy_consensus(seed):
    """the consensus of a decoy pair at tol = 0.03, K = 8, with the vote's counts at 0.09 and the verification over the K rows ->
    (case, consensus_ref's dict, counts (8), verify_ref's dict)"""
    c = VR.decoy_case(seed)
    bits, _ = CR.graph_ref(c["k0"], c["k1"], 0.03)
    r = CR.consensus_ref(c["k0"], c["k1"], bits, CR.sc2_ref(bits, 200), 8)
    counts = np.where(np.arange(8) < r["Kc"], VR.o_counts(r["T"], c["k0"], c["k1"], c["inlier_dist"]), 0).astype(np.int32)
    return c, r, counts, VR.verify_ref(c["src"], c["tgt"], r["T"], None, counts, 8, c["max_dist"])


def check_decoy(seed, c, sets, T, counts, picked):
    """the assertions of the decoy pairs, shared with tests/test_gpu_consist.py: sets = the member lists of rows 0 and 1"""
    assert sets[0] == list(range(12, 26)), (seed, sets[0])                              # the decoy cluster, exactly
    assert set(sets[1]) <= set(range(12)) and len(sets[1]) >= 11, (seed, sets[1])       # the true cluster
    err = RR.rot_error_deg(c["T_gt"][:, :3], T[1][:, :3])
    assert err < 2.0, (seed, err)
    assert counts[0] == 14 and counts[1] == 12, (seed, counts)
    assert picked == 1, (seed, picked)
    return err


def test_decoy_pairs_from_the_matches_alone():
    """seeds 0-3: row 0 is the decoy cluster (14 matches, as the vote has it), row 1 the true one, within 2 degrees and with all 12 inliers at
    0.09; the truncated cost on the clouds picks row 1"""
    for seed in range(4):
        c, r, counts, v = decoy_consensus(seed)
        sets = [np.nonzero(s)[0].tolist() for s in r["sets"][:2]]
        err = check_decoy(seed, c, sets, r["T"], counts, int(v["top"][v["best"]]))
        print(f"seed {seed}: Kc {r['Kc']}, seeds {r['seeds'].tolist()}, sizes {r['sizes'].tolist()}, counts {counts.tolist()}, row 1 {err:.2f} deg off, "
              f"cost {np.round(v['cost'][:v['Kc']], 3).tolist()}, picked row {int(v['top'][v['best']])}")
        assert r["sizes"][0] == 14 and r["sizes"][1] in (11, 12) and r["seeds"][0] in range(12, 26) and r["seeds"][1] in range(12)


def test_planted_case_reference():
    """1000 matches, 30 of them true (3 %): row 0's seed is an inlier, its set the 30, 0.18 degrees off"""
    p = CR.planted_case(1000, 30, 1)
    bits, deg = CR.graph_ref(p["k0"], p["k1"], 0.05)
    r = CR.consensus_ref(p["k0"], p["k1"], bits, CR.sc2_ref(bits, 1000), 8)
    err = RR.rot_error_deg(p["T_gt"][:, :3], r["T"][0][:, :3])
    print(f"planted (1000, 30): mean degree {deg.mean():.1f}, seeds {r['seeds'].tolist()}, sizes {r['sizes'].tolist()}, row 0 {err:.2f} deg off")
    assert r["seeds"][0] < 30 and np.nonzero(r["sets"][0])[0].tolist() == list(range(30)) and err < 0.5
    assert VR.o_counts(r["T"][:1], p["k0"], p["k1"], 0.09)[0] == 30


def test_an_empty_match_list_runs_nothing():
    """consensus.register_matches with no match returns consensus.empty_result without touching the context (None here) or a device: the
    keys of a full result, no row taken, [I|0], and the refit's figures as yoho_refit_matches gives them at M = 0"""
    import torch
    from yoho_amd import consensus
    keys = torch.zeros((5, 3), dtype=torch.float64)
    for K in (1, 8):
        e = consensus.register_matches(None, keys, keys, torch.zeros((0, 2), dtype=torch.int64), 0.05, K=K, refit_iters=2)
        assert set(e) == {"trans", "trans_refit", "refit_counts", "refit_best", "inliers", "row", "Kc", "seeds", "sizes", "counts", "top", "npairs", "rmse", "cost",
                          "best", "fitness"}
        assert e["Kc"] == 0 and e["row"] == -1 and e["inliers"] == 0 and e["refit_best"] == 0 and e["refit_counts"].tolist() == [0, -1, -1]
        assert np.array_equal(e["trans"], CR.IDENTITY) and np.array_equal(e["trans_refit"], CR.IDENTITY) and e["trans"] is not e["trans_refit"]
        assert e["seeds"].tolist() == [-1] * K and e["sizes"].tolist() == e["counts"].tolist() == [0] * K
        if K == 1:
            assert all(e[k] is None for k in ("top", "npairs", "rmse", "cost", "best", "fitness"))
        else:
            assert e["top"].tolist() == [-1] * K and e["npairs"].tolist() == [-1] * K and e["best"] == -1 and e["fitness"] == 0.0
            assert (e["rmse"] == -1).all() and (e["cost"] == -1).all()
    with pytest.raises(ValueError):
        consensus.register_matches(None, keys, keys, torch.zeros((0, 2), dtype=torch.int64), 0.05, K=65)
