"""CPU tests of the normals / point-to-plane entries (include/yoho_plane.h): the library builds and exports exactly their symbols, the
numpy restatement of their contracts (tests/plane_ref.py) agrees with the same arithmetic at 80 digits - the figures the bounds of
tests/test_gpu_plane.py are built from are printed here -, and the reference reproduces the convergence table that motivated the
entries (profiles/plane_icp.md): no sampling floor on two independent samplings of one surface."""
import os
import re
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import plane_ref as PR  # noqa: E402
import refine_ref as RR  # noqa: E402


def plane_header():
    return open(os.path.join(REPO, "include", "yoho_plane.h")).read()


def test_library_exports_plane_header_symbols():
    """include/yoho_plane.h declares exactly hip.PLANE_SYMBOLS, the library exports them, the list shares nothing with the other
    four, no macro is added to the four reason codes, and nothing of it leaked into the older headers"""
    import ctypes as C
    from yoho_amd import build, hip
    assert os.path.exists(build.build(verbose=False))
    lib = hip.load_library()
    hdr = plane_header()
    fns = sorted(set(re.findall(r"\b(yoho_[a-zA-Z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert fns == ["yoho_estimate_normals", "yoho_icp_plane"]
    for f in fns:
        assert hasattr(lib, f), f"libyoho_hip.so does not export {f}"
    assert set(fns) == set(hip.PLANE_SYMBOLS) and len(hip.PLANE_SYMBOLS) == 2
    assert not set(hip.PLANE_SYMBOLS) & set(hip.SYMBOLS + hip.KNN_SYMBOLS + hip.TRAINSET_SYMBOLS + hip.REFINE_SYMBOLS)
    for f, nargs in (("yoho_estimate_normals", 12), ("yoho_icp_plane", 15)):
        assert getattr(lib, f).restype is C.c_int and len(getattr(lib, f).argtypes) == nargs
    assert '#include "yoho_refine.h"' in hdr and re.findall(r"#define\s+(\w+)", hdr) == ["YOHO_PLANE_H"]      # limits and reasons are yoho_refine.h's
    assert len(hip.REFINE_SYMBOLS) == 3 and len(hip.ICP_REASONS) == 4
    for older in ("yoho_hip.h", "yoho_knn.h", "yoho_trainset.h", "yoho_refine.h"):
        txt = open(os.path.join(REPO, "include", older)).read()
        assert not any(f in txt for f in fns), older
    assert build.EXTRA["plane.hip"] == ["-ffp-contract=off"] and "plane.hip" in build.SOURCES
    assert (PR.MIN_PAIRS, PR.PIVOT_TOL, PR.COLLINEAR_TOL) == (6, 1e-13, 1e-12)


def test_numpy_step_against_the_80_digit_step():
    """the two n = 3000 pairs, every iteration of the reference: numpy-f64's worst entry error against the exact step, the 4-ulp floor and
    the bound they give the device (RR.device_tolerance, the yardstick of profiles/refine.md)"""
    for kind in ("same", "halves"):
        c = PR.plane_pair(kind, 3000)
        nr = c["nref"]
        lam = nr["lam"]
        assert nr["valid"].all() and nr["count"].min() >= 6
        print(f"{kind}: normals of 3000 targets at radius {c['normal_radius']}: neighbours min {nr['count'].min()} median {int(np.median(nr['count']))}, "
              f"smallest (l2 - l1) / l3 {((lam[:, 1] - lam[:, 0]) / lam[:, 2]).min():.4f}")
        ref = PR.icp_plane_ref(c["src"], c["tgt"], c["normals"], c["T0"], c["max_dist"], 6, 1e-12)
        assert ref["done"] >= 5
        for i, Ti in enumerate(ref["T"][:ref["done"]]):
            s = PR.plane_step(c["src"], c["tgt"], c["normals"], Ti, c["max_dist"])
            Tx = PR.plane_step_exact(c["tgt"], c["normals"], Ti, s)
            bound, err, floor = RR.device_tolerance(s["T"], Tx, (c["src"], c["tgt"]))
            print(f"{kind} iteration {i}: {s['n']} pairs, rmse {s['rmse']:.6f}, 1 / cond(A) {s['cond']:.3f}; numpy against the exact step {err:.2e}, "
                  f"4-ulp floor {floor:.2e}, bound {bound:.2e}")
            assert err < 1e-13 and bound == max(8 * err, floor)
            assert 0.01 < s["cond"] < 0.2


def test_numpy_normals_against_the_80_digit_normals():
    """64 points spread over the independent-halves target: numpy's angle to the exact normal, and the Davis-Kahan figure beside it"""
    c = PR.plane_pair("halves", 3000)
    nr = c["nref"]
    worst, worst_share = 0.0, 0.0
    for i in np.linspace(0, 2999, 64).astype(int):
        ex = PR.normal_exact(c["tgt"], i, c["normal_radius"])
        assert ex["count"] == nr["count"][i]
        ang = PR.angle_to_exact(nr["n64"][i], ex)
        dk = 4.0 * ex["count"] * 2.0 ** -53 / ex["relgap"]
        worst, worst_share = max(worst, ang), max(worst_share, ang / dk)
        assert abs(float(ex["lam"][0] / (ex["lam"][0] + ex["lam"][1] + ex["lam"][2])) - float(nr["curv"][i])) <= 2.0 ** -24 * float(nr["curv"][i])
    print(f"numpy normals against the exact ones on 64 points: worst angle {worst:.2e} rad, at most {worst_share:.2f} of 4 n 2^-53 / relgap; "
          f"the rounding of the output to f32 adds {PR.ROUND32:.2e}")
    assert worst < 1e-13 and worst_share < 1.0


def test_normals_reference_rules():
    rs = np.random.RandomState(4)
    # an exact plane: +-(0, 0, 1), turned towards the viewpoint; curvature 0
    pl = np.concatenate([rs.rand(400, 2), np.zeros((400, 1))], axis=1).astype(np.float32)
    for view, sign in (((0, 0, 5), 1.0), ((0, 0, -5), -1.0)):
        r = PR.normals_ref(pl, 0.2, view=view)
        assert r["valid"].all() and np.array_equal(r["normals"], np.tile(np.array([[0, 0, sign]], np.float32), (400, 1))) and (r["curv"] == 0).all()
    # a viewpoint in the plane: the product is exactly 0 and the first non-zero component is positive
    assert (PR.normals_ref(pl, 0.2, view=(0.5, 0.5, 0))["normals"][:, 2] == 1).all()
    # collinear neighbours, too few neighbours, a NaN point
    line = (np.outer(np.arange(50), [1.0, 2.0, -0.5]) / 64).astype(np.float32)            # exact in f32
    r = PR.normals_ref(line, 0.25)
    assert not r["valid"].any() and (r["normals"] == 0).all() and (r["curv"] == -1).all() and r["count"].min() >= 5
    pts = rs.rand(300, 3).astype(np.float32)
    pts[7] = np.nan
    r = PR.normals_ref(pts, 0.15, min_nbrs=8)
    brute = (RR._d2(pts, pts) < RR.gate2_of(0.15)).sum(axis=1)
    assert np.array_equal(r["count"], brute) and r["count"][7] == 0 and np.array_equal(r["valid"], (brute >= 8) & (r["ratio"] > 1e-12))
    assert 0 < r["valid"].sum() < 300
    assert np.allclose(np.linalg.norm(r["n64"][r["valid"]], axis=1), 1.0, atol=1e-15)
    v = np.zeros(3) - pts[r["valid"]].astype(np.float64)
    assert ((r["n64"][r["valid"]] * v).sum(axis=1) >= 0).all()


def test_plane_reference_reproduces_the_convergence_table():
    """the motivation, kept checkable: on two independent 20 000-point samplings point-to-plane reaches 0.02 degrees or less after 20
    iterations (prototype: 0.0104) and at most half of point-to-point's error after the same 20 (prototype: 0.080); on the pair with
    the same points on both sides max |dT| is 1e-8 or less by iteration 6"""
    c = PR.plane_pair("halves", 20000)
    nr = c["nref"]
    print(f"halves, 20 000: normals at radius {c['normal_radius']}: neighbours min {nr['count'].min()} median {int(np.median(nr['count']))}, "
          f"{int((~nr['valid']).sum())} invalid")
    assert (~nr["valid"]).sum() <= 20
    gt = c["T_gt"]
    r = PR.icp_plane_ref(c["src"], c["tgt"], c["normals"], c["T0"], c["max_dist"], 20, -1.0)
    pp = RR.icp_ref(c["src"], c["tgt"], c["T0"], c["max_dist"], 20, -1.0)
    e_plane, e_point = RR.rot_error_deg(gt[:, :3], r["T_out"][:, :3]), RR.rot_error_deg(gt[:, :3], pp["T_out"][:, :3])
    print(f"halves, 20 000, 20 iterations: point-to-plane {e_plane:.4f} deg / {np.linalg.norm(gt[:, 3] - r['T_out'][:, 3]) * 1e3:.3f} mm, point-to-point "
          f"{e_point:.4f} deg / {np.linalg.norm(gt[:, 3] - pp['T_out'][:, 3]) * 1e3:.3f} mm; steps " + " ".join(f"{d:.1e}" for d in r["deltas"]))
    assert r["done"] == 20 and e_plane <= 0.02 and e_plane <= 0.5 * e_point
    s = PR.plane_pair("same", 20000)
    r = PR.icp_plane_ref(s["src"], s["tgt"], s["normals"], s["T0"], s["max_dist"], 8, -1.0)
    print("same points, 20 000: steps " + " ".join(f"{d:.1e}" for d in r["deltas"]) + f"; {RR.rot_error_deg(s['T_gt'][:, :3], r['T_out'][:, :3]):.2e} deg / "
          f"{np.linalg.norm(s['T_gt'][:, 3] - r['T_out'][:, 3]):.1e} m from the ground truth")
    assert r["deltas"][5] <= 1e-8
    # the stop rules of the reference
    few = PR.icp_plane_ref(s["src"][:5], s["tgt"], s["normals"], s["T_gt"], s["max_dist"], 3, 0.0)
    assert (few["done"], few["reason"]) == (1, RR.ICP_FEW_PAIRS) and few["npairs"].tolist() == [5, -1, -1] and few["rmse"][0] >= 0
    rs = np.random.RandomState(1)
    flat = np.concatenate([rs.rand(500, 2), np.zeros((500, 1))], axis=1).astype(np.float32)
    I = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    rank = PR.icp_plane_ref(flat, flat, np.tile(np.array([[0, 0, 1]], np.float32), (500, 1)), I, 0.1, 3, 0.0)
    assert (rank["done"], rank["reason"]) == (1, RR.ICP_RANK) and rank["npairs"].tolist() == [500, -1, -1] and np.array_equal(rank["T_out"], I)
