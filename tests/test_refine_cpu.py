"""CPU tests of the refinement entries (include/yoho_refine.h): the library builds and exports exactly their symbols, and the numpy
restatement of their contracts (tests/refine_ref.py) does what the GPU tests lean on - the refit gets closer to the ground truth
and keeps every residual away from the threshold, the ICP converges, the nearest-neighbour reference is the oracle's distance +
argmin + gate, the exact Kabsch agrees with oracle/estim_ref.py on three points."""
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import refine_ref as RR  # noqa: E402
import yoho_oracle as orc  # noqa: E402


def refine_header():
    return open(os.path.join(REPO, "include", "yoho_refine.h")).read()


def refine_header_functions():
    txt = re.sub(r"/\*.*?\*/", "", refine_header(), flags=re.S)
    return sorted(set(re.findall(r"\b(yoho_[a-zA-Z0-9_]+)\s*\(", txt)))


def test_library_exports_refine_header_symbols():
    """include/yoho_refine.h: every function it declares is exported, the set is hip.REFINE_SYMBOLS and shares nothing with the other
    three lists, the header's limits are the binding's, and nothing of it leaked into the pinned header"""
    import ctypes as C
    from yoho_amd import build, hip
    assert os.path.exists(build.build(verbose=False))
    lib = hip.load_library()
    fns = refine_header_functions()
    assert fns == ["yoho_icp_refine", "yoho_nn_within", "yoho_refit_matches"]
    for f in fns:
        assert hasattr(lib, f), f"libyoho_hip.so does not export {f}"
    assert set(fns) == set(hip.REFINE_SYMBOLS) and len(hip.REFINE_SYMBOLS) == 3
    assert not set(hip.REFINE_SYMBOLS) & set(hip.SYMBOLS + hip.KNN_SYMBOLS + hip.TRAINSET_SYMBOLS)
    for f, nargs in (("yoho_nn_within", 9), ("yoho_refit_matches", 11), ("yoho_icp_refine", 14)):
        assert getattr(lib, f).restype is C.c_int and len(getattr(lib, f).argtypes) == nargs
    hdr = refine_header()
    macro = lambda name: re.search(r"#define\s+" + name + r"\s+\(?([^)\s]+(?:\s*<<\s*\d+)?)", hdr).group(1)
    assert eval(macro("YOHO_REFINE_MAX_POINTS")) == hip.REFINE_MAX_POINTS == 1 << 22
    assert int(macro("YOHO_REFIT_MAX_ITERS")) == hip.REFIT_MAX_ITERS == 32 and int(macro("YOHO_ICP_MAX_ITERS")) == hip.ICP_MAX_ITERS
    assert [int(macro("YOHO_ICP_" + n.upper())) for n in hip.ICP_REASONS] == [0, 1, 2, 3]
    assert (RR.ICP_ITERS, RR.ICP_CONVERGED, RR.ICP_FEW_PAIRS, RR.ICP_RANK) == (0, 1, 2, 3)
    pinned = open(os.path.join(REPO, "include", "yoho_hip.h")).read()
    assert not any(f in pinned for f in fns)
    # the translation unit is built without contraction, like the other bit-exact ones
    assert build.EXTRA["refine.hip"] == ["-ffp-contract=off"] and "refine.hip" in build.SOURCES


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_refit_reference_gets_closer_and_stays_off_the_threshold(seed):
    """M = 1500, 30 % inliers at 1 cm noise, started 4 degrees / 4.7 cm off: the reference's answer is closer to the ground truth
    than the start in rotation and translation, never holds fewer inliers, and at every iterate no residual lies within 1e-6
    relative of the threshold - the guard that lets tests/test_gpu_refine.py demand equal counts from a device whose transforms
    differ in their last bits"""
    c = RR.refit_case(seed)
    assert c["k0"].shape == (1500, 3)
    gt, T0 = c["T_gt"], c["T0"]
    assert abs(RR.rot_error_deg(gt[:, :3], T0[:, :3]) - 4.0) < 1e-6 and abs(np.linalg.norm(gt[:, 3] - T0[:, 3]) - 0.047) < 1e-9
    r = RR.refit_ref(c["k0"], c["k1"], T0, c["inlier_dist"], 8)
    T = r["T_out"]
    e0, e1 = RR.rot_error_deg(gt[:, :3], T0[:, :3]), RR.rot_error_deg(gt[:, :3], T[:, :3])
    s0, s1 = np.linalg.norm(gt[:, 3] - T0[:, 3]), np.linalg.norm(gt[:, 3] - T[:, 3])
    print(f"seed {seed}: counts {r['counts'].tolist()}, best {r['best']}, rotation {e0:.3f} -> {e1:.4f} deg, translation {s0:.4f} -> {s1:.5f} m, "
          f"closest residual {r['margin']:.2e} relative from the threshold")
    assert e1 < e0 and s1 < s0
    assert r["counts"][r["best"]] == r["counts"][:r["evaluated"]].max() >= r["counts"][0] and r["best"] == int(np.argmax(r["counts"]))
    assert (r["counts"][r["evaluated"]:] == -1).all() and r["evaluated"] >= 2
    assert r["margin"] > 1e-6
    # every iterate is a proper rotation
    for Ti in r["T"][1:]:
        assert np.abs(Ti[:, :3] @ Ti[:, :3].T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(Ti[:, :3]) - 1.0) < 1e-14
    # the last iterate (the fit on all inliers) is the statistically right one: sigma / sqrt(n) of 1 cm noise on ~450 points
    last = r["T"][-1]
    assert RR.rot_error_deg(gt[:, :3], last[:, :3]) < 0.15 and np.linalg.norm(gt[:, 3] - last[:, 3]) < 0.003


def test_refit_reference_edges():
    c = RR.refit_case(0)
    k0, k1, T0, d = c["k0"], c["k1"], c["T0"], c["inlier_dist"]
    r = RR.refit_ref(k0, k1, T0, d, 0)
    assert r["evaluated"] == 1 and r["best"] == 0 and np.array_equal(r["T_out"], T0) and r["counts"].tolist() == [int((RR.residual2(T0, k0, k1) < d * d).sum())]
    r = RR.refit_ref(k0[:0], k1[:0], T0, d, 3)
    assert r["counts"].tolist() == [0, -1, -1, -1] and np.array_equal(r["T_out"], T0)
    # collinear inliers: the count is taken, no transform is formed
    line = np.outer(np.linspace(-1, 1, 50), [1.0, 2.0, -0.5])
    I = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    r = RR.refit_ref(line, line, I, 0.1, 4)
    assert r["counts"].tolist() == [50, -1, -1, -1, -1] and r["evaluated"] == 1
    # planar inliers solve
    rs = np.random.RandomState(5)
    plane = np.concatenate([rs.rand(60, 2), np.zeros((60, 1))], axis=1)
    T = np.concatenate([RR.rot_axis_angle([1, 2, 3], 25.0), [[0.1], [0.2], [0.3]]], axis=1)
    r = RR.refit_ref(plane @ T[:, :3].T + T[:, 3], plane, RR.perturbed(T, rs, 1.0, 0.01), 0.1, 4)
    assert r["evaluated"] >= 2 and np.abs(r["T"][1] - T).max() < 1e-12


def test_icp_reference_converges_on_the_surface_cloud_pair():
    """the 20 000-point synth.surface_cloud pair, 2 degrees and 4.5 cm off, gate 0.1 m: under 0.01 degrees"""
    c = RR.icp_case()
    assert c["src"].shape == c["tgt"].shape == (20000, 3) and c["max_dist"] == 0.1
    gt, T0 = c["T_gt"], c["T0"]
    assert abs(RR.rot_error_deg(gt[:, :3], T0[:, :3]) - 2.0) < 1e-6 and abs(np.linalg.norm(gt[:, 3] - T0[:, 3]) - 0.045) < 1e-9
    r = RR.icp_ref(c["src"], c["tgt"], T0, c["max_dist"], 30, 0.0)
    errs = [RR.rot_error_deg(gt[:, :3], T[:, :3]) for T in r["T"]]
    print(f"ICP reference: {r['done']} iterations, reason {r['reason']}, rotation error by iteration " + " ".join(f"{e:.4f}" for e in errs)
          + f", pairs {r['npairs'][:r['done']].tolist()}, final translation error {np.linalg.norm(gt[:, 3] - r['T_out'][:, 3]):.2e} m")
    assert errs[-1] < 0.01 and np.linalg.norm(gt[:, 3] - r["T_out"][:, 3]) < 1e-4
    assert r["reason"] in (RR.ICP_ITERS, RR.ICP_CONVERGED) and (r["npairs"][:r["done"]] >= 19000).all()
    assert (r["npairs"][r["done"]:] == -1).all() and (r["rmse"][r["done"]:] == -1.0).all()
    assert r["rmse"][r["done"] - 1] < r["rmse"][0]


def test_nn_within_reference_is_the_oracle_distance_argmin_and_gate():
    rs = np.random.RandomState(11)
    for nq, nt, r in ((300, 700, 0.05), (700, 300, 0.2), (65, 4097, 0.02), (1, 1, 0.5), (500, 500, 3.0)):
        q, t = rs.rand(nq, 3).astype(np.float32), rs.rand(nt, 3).astype(np.float32)
        t[nt // 2] = t[0]                                      # a duplicate target: the lower index wins
        q[0] = t[0]
        d = orc.pdist_l2(q, t, squared=True)
        j = np.argmin(d, axis=1)
        best = d[np.arange(nq), j]
        ok = best < RR.gate2_of(r)
        for pre in (True, False):
            idx, d2 = RR.nn_within_ref(q, t, r, chunk=128, prefilter=pre)
            assert np.array_equal(idx, np.where(ok, j, -1)) and np.array_equal(d2.view(np.uint32), np.where(ok, best, np.float32(np.inf)).view(np.uint32))
        assert idx[0] == 0 and d2[0] == 0.0
        print(f"{nq} x {nt}, radius {r}: {int(ok.sum())} of {nq} queries have a partner")
    # exactly on the gate is out, a hair inside is in; NaN / inf queries and NaN targets
    t = np.array([[0, 0, 0], [np.nan, 0, 0], [4, 0, 0]], np.float32)
    q = np.array([[0.5, 0, 0], [np.nextafter(np.float32(0.5), np.float32(0)), 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [3.75, 0, 0]], np.float32)
    idx, d2 = RR.nn_within_ref(q, t, 0.5)
    assert idx.tolist() == [-1, 0, -1, -1, 2] and np.isinf(d2[[0, 2, 3]]).all() and d2[4] == np.float32(0.0625)


def test_tree_sum_and_exact_kabsch():
    import math
    rs = np.random.RandomState(2)
    for n in (0, 1, 63, 64, 65, 256, 257, 1500):
        v = rs.randn(n, 3)
        s = RR.tree_sum(v)
        assert s.shape == (3,)
        for k in range(3):
            assert abs(s[k] - math.fsum(v[:, k])) <= 1e-13 * max(1.0, np.abs(v[:, k]).sum())
    assert RR.tree_sum(np.arange(300.0)) == 300 * 299 / 2
    # three points: oracle/estim_ref.py's own 80-digit answer
    import estim_ref as ER
    a1 = rs.rand(3, 3)
    T = np.concatenate([RR.rot_axis_angle([1, -1, 2], 40.0), [[0.5], [0.1], [-0.3]]], axis=1)
    a0 = a1 @ T[:, :3].T + T[:, 3] + 1e-3 * rs.randn(3, 3)
    ref = ER.kabsch_ref(a0, a1)
    Tx = RR.kabsch_exact(a0, a1)
    assert ref["cls"] == "rank2" and np.abs(Tx[:, :3] - ref["R"]).max() <= 2.3e-16 and np.abs(Tx[:, 3] - ref["t"]).max() <= 2.3e-16
    # many points: numpy's step is within a few ulps of the exact one, and the tolerance rule has its floor
    c = RR.refit_case(1)
    sel = RR.residual2(c["T_gt"], c["k0"], c["k1"]) < 0.09 ** 2
    Tn, Tx = RR.kabsch_step(c["k0"], c["k1"], sel), RR.kabsch_exact(c["k0"][sel], c["k1"][sel])
    bound, err, floor = RR.device_tolerance(Tn, Tx, (c["k0"], c["k1"]))
    print(f"numpy-f64 Kabsch step against the exact one on {int(sel.sum())} matches: worst entry error {err:.2e}; 4 ulp of the largest coordinate {floor:.2e}")
    assert err < 1e-14 and floor == 4 * np.spacing(np.abs(np.concatenate([c["k0"], c["k1"]])).max()) and bound == max(8 * err, floor)
