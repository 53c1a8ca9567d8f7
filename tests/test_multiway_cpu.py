"""CPU tests of multiway registration (include/yoho_multiway.h, yoho_amd/multiway.py): the library builds and exports
exactly the header's symbol and its kernels compile without scratch; the numpy restatement of the entry (tests/multiway_ref.py) gives
the matrix SUM G^T G and that matrix is the quadratic form the registration benchmark thresholds; the solver's Jacobians are those of
its objective; on seeded pose graphs with false registrations it prunes exactly those and lands on the minimum a plain solver finds on
the graph without them; and the files it writes are the ones RR_cal reads."""
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
import multiway_ref as MR  # noqa: E402
import refine_ref as RR  # noqa: E402
from yoho_amd import RR_cal  # noqa: E402
from yoho_amd import multiway as MW  # noqa: E402

f32, f64 = np.float32, np.float64


# ---- the library ---------------------------------------------------------------------------------------------------------------------------
def test_library_exports_multiway_header_symbol():
    """include/yoho_multiway.h declares exactly hip.MULTIWAY_SYMBOLS, the library exports it, the list shares nothing with the other
    eight, hip.SYMBOLS is still yoho_hip.h's set, the header's constants are the binding's, and nothing leaked into the older headers"""
    import ctypes as C
    from yoho_amd import build, hip
    assert os.path.exists(build.build(verbose=False))
    lib = hip.load_library()
    hdr = open(os.path.join(REPO, "include", "yoho_multiway.h")).read()
    fns = sorted(set(re.findall(r"\b(yoho_[a-zA-Z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert fns == ["yoho_edge_information"] and hip.MULTIWAY_SYMBOLS == fns
    assert lib.yoho_edge_information.restype is C.c_int and len(lib.yoho_edge_information.argtypes) == 12
    others = (hip.SYMBOLS + hip.KNN_SYMBOLS + hip.TRAINSET_SYMBOLS + hip.REFINE_SYMBOLS + hip.PLANE_SYMBOLS + hip.VERIFY_SYMBOLS + hip.CONSIST_SYMBOLS +
              hip.KEYPOINT_SYMBOLS)
    assert "yoho_edge_information" not in others
    main = open(os.path.join(REPO, "include", "yoho_hip.h")).read()
    main_fns = set(re.findall(r"\b(yoho_[a-zA-Z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", main, flags=re.S)))
    assert main_fns == set(hip.SYMBOLS) and len(hip.SYMBOLS) == len(set(hip.SYMBOLS))            # unchanged by the new entry
    for older in ("yoho_hip.h", "yoho_knn.h", "yoho_trainset.h", "yoho_refine.h", "yoho_plane.h", "yoho_verify.h", "yoho_consist.h", "yoho_keypoints.h"):
        assert "yoho_edge_information" not in open(os.path.join(REPO, "include", older)).read(), older
    assert '#include "yoho_refine.h"' in hdr
    assert re.findall(r"#define\s+(\w+)", hdr) == ["YOHO_MULTIWAY_H", "YOHO_MULTIWAY_MAX_K", "YOHO_MULTIWAY_MAX_SOURCE_POINTS"]
    assert int(re.search(r"#define\s+YOHO_MULTIWAY_MAX_K\s+(\d+)\b", hdr).group(1)) == hip.MULTIWAY_MAX_K == MW.MAX_K == 64
    assert 1 << int(re.search(r"#define\s+YOHO_MULTIWAY_MAX_SOURCE_POINTS\s+\(1 << (\d+)\)", hdr).group(1)) == hip.MULTIWAY_MAX_SOURCE_POINTS == MW.MAX_SOURCE_POINTS
    assert build.EXTRA["multiway.hip"] == ["-ffp-contract=off"] and "multiway.hip" in build.SOURCES
    # the header says in words what soff is
    assert "HOST array" in hdr and "by value" in hdr and "strictly increasing" in hdr


def test_multiway_kernels_use_no_scratch(tmp_path):
    """csrc/multiway.hip compiled for gfx950 with the flags of the build: two kernels, neither with scratch - in particular the edge
    table passed by value is read with scalar loads, not copied to private memory to be indexed"""
    from yoho_amd import build
    cmd = [build._hipcc()] + build.FLAGS + build.EXTRA["multiway.hip"] + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                                                                         os.path.join(build.CSRC, "multiway.hip"), "-o", str(tmp_path / "multiway.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r"\bVGPRs: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == 2, names
    assert sum("mw_eval_kernel" in n for n in names) == 1 and sum("mw_sum_kernel" in n for n in names) == 1
    print("multiway.hip: " + ", ".join(f"{n} {v} VGPRs" for n, v in zip(names, vgprs)))
    assert scratch == [0, 0], dict(zip(names, scratch))
    assert max(vgprs) <= 64, dict(zip(names, vgprs))                  # eight waves per SIMD


# ---- the matrix ----------------------------------------------------------------------------------------------------------------------------
def paired_case(n, seed, gate=0.1):
    """n source points that each have a partner: a cloud of 2 n + 7 points in the unit cube, n of them moved by 1 cm of noise"""
    rs = np.random.RandomState(seed)
    tgt = rs.rand(2 * n + 7, 3).astype(f32)
    src = (tgt[rs.permutation(2 * n + 7)[:n]] + 0.01 * rs.randn(n, 3)).astype(f32)
    return src, tgt, gate


@pytest.mark.parametrize("n", [50, 257, 1300, 5000])
def test_reference_matrix_is_the_literal_sum(n):
    """edge_info_ref's matrix against SUM G^T G taken one point at a time in float64: every entry within 1e-10 of the largest entry (a
    reordered float64 sum of n <= 5000 terms differs by at most n 2^-53 < 6e-13 of it; a margin of 100 on top), info[0,0] = npairs,
    symmetric, positive definite"""
    src, tgt, gate = paired_case(n, n)
    T = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)[None]
    npairs, rmse, info = MR.edge_info_ref(src, [0, n], tgt, T, gate)
    idx, _ = RR.nn_within_ref(src, tgt, gate)
    assert 50 <= npairs[0] <= 5000 and npairs[0] == (idx >= 0).sum() >= 0.9 * n
    lit = MR.info_literal(tgt[idx[idx >= 0]])
    M = info[0]
    assert np.abs(M - lit).max() <= 1e-10 * np.abs(lit).max(), np.abs(M - lit).max() / np.abs(lit).max()
    assert M[0, 0] == M[1, 1] == M[2, 2] == npairs[0]
    assert np.array_equal(M, M.T)
    assert np.linalg.eigvalsh(M).min() > 0
    assert np.abs(M - MR.info_from_points(tgt[idx[idx >= 0]])).max() <= 1e-10 * np.abs(lit).max()      # the closed form the cases are built with


def test_reference_rows_depend_on_the_local_index_only():
    """a row of a K = 3 call is the K = 1 call on that source: the sums run over the source's own index"""
    rs = np.random.RandomState(5)
    tgt = rs.rand(400, 3).astype(f32)
    srcs = [(tgt[rs.randint(400, size=m)] + 0.02 * rs.randn(m, 3)).astype(f32) for m in (300, 1, 257)]
    T = np.stack([RR.perturbed(np.eye(4)[:3], rs, 3.0, 0.02) for _ in srcs])
    soff = np.concatenate([[0], np.cumsum([len(s) for s in srcs])])
    n, r, M = MR.edge_info_ref(np.concatenate(srcs), soff, tgt, T, 0.1)
    for k, s in enumerate(srcs):
        n1, r1, M1 = MR.edge_info_ref(s, [0, len(s)], tgt, T[k:k + 1], 0.1)
        assert n1[0] == n[k] and r1.tobytes() == r[k:k + 1].tobytes() and M1.tobytes() == M[k:k + 1].tobytes()
    # a transform that pairs nothing: the zero matrix, rmse = +inf
    far = T[:1].copy()
    far[0, :, 3] = 100.0
    n0, r0, M0 = MR.edge_info_ref(srcs[0], [0, 300], tgt, far, 0.1)
    assert n0[0] == 0 and r0[0] == np.inf and not M0.any()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_matrix_is_the_benchmarks_quadratic_form(seed):
    """What RR_cal thresholds.  computeTransformationErr(D, info) is er' info er / n with er = (t, u), u the VECTOR PART OF THE
    QUATERNION of D's rotation: |u| = sin(theta / 2), half the rotation vector to first order.  Since info = SUM G^T G and
    G (t, u) = t + u x p, that quotient is mean |t + u x p|^2 exactly: the mean squared displacement of the paired target points under
    the motion D_u = [Exp(u) | t], linearised.  So the benchmark's 0.2^2 bounds the displacement under HALF the rotation of D - the
    factor is RR_cal's and the Redwood protocol's, not hidden here: the literal displacement is taken under D_u, and the quadratic
    form in the full rotation vector, xi' info xi / n (optimize's rbar), is checked against the literal displacement under D itself.

    Tolerance, from the small-angle remainder: Exp(u) p - p = u x p + rem, |rem| <= |u|^2 |p| / 2 (the series of Exp: the second-order
    term is (1 - cos|u|) / |u|^2 u x (u x p) <= |u|^2 |p| / 2 and the third-order remainder of the first term has the opposite sign).
    With a = t + u x p, |a| <= |t| + |u| |p|:  | |a + rem|^2 - |a|^2 | <= 2 |a| |rem| + |rem|^2, taken at the largest |p|; plus 1e-12
    relative for the float64 evaluation of either side."""
    rs = np.random.RandomState(40 + seed)
    gate = 0.1
    tgt = (rs.rand(3007, 3) * 2.0 + rs.randn(3)).astype(f32)             # a 2 m cube away from the origin, as fragments lie
    src = (tgt[rs.permutation(3007)[:1500]] + 0.01 * rs.randn(1500, 3)).astype(f32)
    T = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)[None]
    npairs, _, info = MR.edge_info_ref(src, [0, 1500], tgt, T, gate)
    idx, _ = RR.nn_within_ref(src, tgt, gate)
    p = tgt[idx[idx >= 0]].astype(f64)
    pmax = np.linalg.norm(p, axis=1).max()
    for _ in range(4):
        w = MR.random_direction(rs) * np.deg2rad(0.5) * rs.rand()
        t = MR.random_direction(rs) * 0.01 * rs.rand()
        D = MR.motion(w, t)
        q = RR_cal.mat2quat(D[:3, :3])
        u = q[1:]
        assert abs(np.linalg.norm(u) - np.sin(0.5 * np.linalg.norm(w))) <= 1e-15 and np.linalg.norm(u - 0.5 * w) <= np.linalg.norm(w) ** 3 / 48 + 1e-15
        for rot, got in ((u, RR_cal.computeTransformationErr(D, info[0]) / 1),
                         (w, float(np.concatenate([t, w]) @ info[0] @ np.concatenate([t, w])) / npairs[0])):
            Dm = MR.motion(rot, t)
            literal = float(np.mean(np.sum((p @ Dm[:3, :3].T + Dm[:3, 3] - p) ** 2, axis=1)))
            th = np.linalg.norm(rot)
            rem = 0.5 * th * th * pmax
            tol = 2.0 * (np.linalg.norm(t) + th * pmax) * rem + rem * rem + 1e-12 * literal
            assert abs(got - literal) <= tol, (got, literal, tol)
            assert tol <= 0.05 * literal or literal < 1e-8             # the bound is a few percent of the figure, not a blank cheque


# ---- the solver ----------------------------------------------------------------------------------------------------------------------------
def test_lie_helpers_round_trip():
    rs = np.random.RandomState(0)
    w = np.concatenate([rs.randn(200, 3), 1e-9 * rs.randn(20, 3), [[0, 0, 0]], [MR.random_direction(rs) * (np.pi - 1e-9)]])
    w = w[np.linalg.norm(w, axis=1) < np.pi]
    R = MW.so3_exp(w)
    assert np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3)).max() < 1e-14
    assert np.abs(MW.so3_log(R) - w).max() < 1e-6 and np.abs(MW.so3_log(R[:-1]) - w[:-1]).max() < 1e-12
    for k in range(0, len(w), 17):
        assert np.abs(R[k] - MR.rot_of(w[k])).max() < 1e-15
    # the inverse right Jacobian against central differences of log(Exp(phi) Exp(d))
    for phi in (rs.randn(3) * 0.5, rs.randn(3) * 1e-6, MR.random_direction(rs) * 2.5):
        J = MW.so3_jr_inv(phi)
        num = np.stack([(MW.so3_log(MW.so3_exp(phi) @ MW.so3_exp(d)) - MW.so3_log(MW.so3_exp(phi) @ MW.so3_exp(-d))) / 2e-6
                        for d in 1e-6 * np.eye(3)], axis=1)
        assert np.abs(J - num).max() < 1e-9
    X = MW.se3_exp(rs.randn(5, 6))
    assert np.abs(MW.se3_inv(X) @ X - np.eye(4)).max() < 1e-14 and np.abs(MW.se3_xi(X) - MW.se3_xi(MW.se3_exp(MW.se3_xi(X)))).max() < 1e-13


def test_gradient_is_the_objectives():
    """the analytic gradient (exact Jacobians, the inverse Jacobian of the SO(3) logarithm included, the line process by its envelope)
    against central differences of the objective itself, at a point 3 degrees / 10 cm of noise away from the ground truth of a graph
    with false registrations - nowhere near stationary, residuals of every size.  Central differences with h = 1e-6 carry a
    truncation error h^2 f''' / 6 ~ 1e-12 of the gradient's scale and a rounding error eps f / h ~ 2.2e-10 f; with f below 100 times
    the largest gradient entry here (asserted) that is 2.2e-8 of it: the bound is 1e-7 of the largest entry."""
    c = MR.outlier_case(8, 0)
    rs = np.random.RandomState(1)
    X = np.stack([c["Xg"][f] @ MR.motion(rs.randn(3) * 0.05, rs.randn(3) * 0.1) for f in range(8)])
    h = 1e-6
    for certain in (None, c["consecutive"]):
        g = MW.gradient(X, c["pairs"], c["T"], c["info"], certain=certain)
        f0 = MW.objective(X, c["pairs"], c["T"], c["info"], certain=certain)
        num = np.zeros_like(g)
        for f in range(8):
            for k in range(6):
                d = np.zeros(6)
                d[k] = h
                Xp, Xm = X.copy(), X.copy()
                Xp[f], Xm[f] = X[f] @ MR.step_of(d), X[f] @ MR.step_of(-d)
                num[f, k] = (MW.objective(Xp, c["pairs"], c["T"], c["info"], certain=certain) - MW.objective(Xm, c["pairs"], c["T"], c["info"], certain=certain)) / (2 * h)
        scale = np.abs(num).max()
        print(f"objective {f0:.3f}, largest gradient entry {scale:.3f}, largest difference {np.abs(g - num).max():.3e}")
        assert f0 <= 100 * scale and scale > 1.0
        assert np.abs(g - num).max() <= 1e-7 * scale


def test_optimize_returns_the_inputs_it_was_given_untouched_and_consistent_poses():
    """a graph without noise: the spanning tree is already the minimum, nothing is pruned, the poses are the ground truth"""
    c = MR.outlier_case(8, 1)
    ok = ~c["outlier"]
    Tt = np.stack([MR.inverse(c["Xg"][i]) @ c["Xg"][j] for i, j in c["pairs"][ok]])
    before = (c["pairs"].copy(), c["T"].copy(), c["info"].copy())
    r = MW.optimize(8, c["pairs"][ok], Tt[:, :3, :], c["info"][ok])                # (E,3,4) transforms are taken too
    assert all(np.array_equal(a, b) for a, b in zip(before, (c["pairs"], c["T"], c["info"])))
    assert r["reached"].all() and not r["pruned"].any() and not r["dropped"].any() and (r["weights"] > 0.999999).all()
    deg, m = MR.pose_error(r["poses"], c["Xg"])
    assert deg < 1e-9 and m < 1e-11 and r["rbar"].max() < 1e-20
    assert np.abs(MW.implied_transforms(r["poses"], c["pairs"][ok]) - Tt).max() < 1e-11
    with pytest.raises(ValueError):
        MW.optimize(8, c["pairs"][ok], Tt, c["info"][ok], anchor=8)
    with pytest.raises(ValueError):
        MW.optimize(3, c["pairs"][ok], Tt, c["info"][ok])


@pytest.mark.parametrize("F", [8, 20])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_false_registrations_are_pruned_exactly(F, seed):
    """multiway_ref.outlier_case, with the consecutive pairs certain and with no edge certain, tau = 0.2, prune = 0.25: `pruned` is
    the set of false registrations exactly; the final poses agree with optimize_ref on the graph without them, started from the
    ground truth, within 1e-6 degrees and 1e-7 m (largest differences measured over the 16 cases: 6.6e-8 degrees, 2.3e-9 m); the
    objective never increases along either stage's history; the anchor pose is the identity bit for bit"""
    c = MR.outlier_case(F, seed)
    assert c["outlier"].sum() >= 3 and not (c["outlier"] & c["consecutive"]).any() and c["consecutive"].sum() == F - 1
    n = c["info"][:, 0, 0]
    assert n[c["outlier"]].max() < n[~c["outlier"]].min()
    ref = MR.clean_solution(F, seed)
    for certain in (c["consecutive"], None):
        r = MW.optimize(F, c["pairs"], c["T"], c["info"], certain=certain)
        what = (F, seed, certain is None)
        assert np.array_equal(r["pruned"], c["outlier"]), (what, np.nonzero(r["pruned"] != c["outlier"])[0])
        assert r["reached"].all() and not r["dropped"].any()
        deg, m = MR.pose_error(r["poses"], ref)
        print(f"F {F} seed {seed} certain {'none' if certain is None else 'consecutive'}: {len(c['pairs'])} edges, {int(c['outlier'].sum())} false, "
              f"{len(r['history_stage1']) - 1} + {len(r['history_stage2']) - 1} accepted iterations, {deg:.2e} degrees / {m:.2e} m from the plain solver")
        assert deg <= 1e-6 and m <= 1e-7, (what, deg, m)
        for hist in (r["history_stage1"], r["history_stage2"]):
            assert len(hist) >= 2 and (np.diff(hist) < 0).all(), (what, hist)
        assert r["history"] == r["history_stage1"] + r["history_stage2"]
        assert r["poses"][0].tobytes() == np.eye(4).tobytes()
        # the pruned edges fail the benchmark's criterion against the final poses, the kept ones pass it
        assert (r["rbar"][r["pruned"]] > 0.2 ** 2).all() and (r["rbar"][~r["pruned"]] <= 0.2 ** 2).all()
        assert (r["weights"][r["pruned"]] < 0.25).all() and (r["weights"][~r["pruned"]] >= 0.25).all()
        if certain is not None:
            assert (r["weights"][certain] == 1.0).all()


def disconnect_case():
    """five fragments: 0 .. 3 registered exactly in every pair; fragment 4 hangs on four registrations whose translations are 8 cm
    off along x, two to each side.  Its pose settles between them (the robust weight is convex below tau / sqrt(3) = 11.5 cm), every
    one of the four keeps a residual of 6 - 10 cm, and a strict user (prune = 0.9: rbar > 0.054 tau^2 = (4.6 cm)^2) prunes all four."""
    rs = np.random.RandomState(12)
    Xg = [np.eye(4)] + [MR.motion(MR.random_direction(rs) * 0.6 * rs.rand(), rs.randn(3)) for _ in range(4)]
    pairs, T, info = [], [], []
    for i in range(5):
        for j in range(i + 1, 5):
            Tt = MR.inverse(Xg[i]) @ Xg[j]
            if j == 4:
                off = MR.inverse(Xg[i])[:3, :3] @ np.array([0.08 if i % 2 == 0 else -0.08, 0.0, 0.0])     # along the scene's x axis
                Tt = Tt.copy()
                Tt[:3, 3] += off
            pairs.append((i, j)); T.append(Tt); info.append(MR.info_from_points(rs.rand(1000, 3) * 2.0 - 1.0))
    return np.stack(Xg), np.array(pairs, np.int64), np.stack(T), np.stack(info)


def test_pruning_that_disconnects_a_fragment():
    Xg, pairs, T, info = disconnect_case()
    r = MW.optimize(5, pairs, T, info, prune=0.9)
    into4 = pairs[:, 1] == 4
    print("weights", np.round(r["weights"], 4), "rbar", r["rbar"])
    assert np.array_equal(r["pruned"], into4)
    assert r["reached"].tolist() == [True, True, True, True, False]
    assert np.isnan(r["poses"][4]).all() and np.isfinite(r["poses"][:4]).all()
    assert np.isnan(r["rbar"][into4]).all() and (r["rbar"][~into4] < 1e-6).all()
    deg, m = MR.pose_error(r["poses"][:4], Xg[:4])
    assert deg < 0.05 and m < 1e-3                                    # the pull of fragment 4 ended with its edges: stage 2 runs without them
    imp = MW.implied_transforms(r["poses"], pairs)
    assert np.isnan(imp[into4]).all() and np.isfinite(imp[~into4]).all()
    # the default threshold keeps them: 8 cm is inside the benchmark's 20 cm
    r2 = MW.optimize(5, pairs, T, info)
    assert not r2["pruned"].any() and r2["reached"].all()
    # edges below min_pairs are dropped up front, not pruned; a fragment only they reach is not reached
    few = info.copy()
    few[into4] *= 9.0 / 1000.0
    r3 = MW.optimize(5, pairs, T, few)
    assert np.array_equal(r3["dropped"], into4) and not r3["pruned"].any() and r3["reached"].tolist() == [True, True, True, True, False]
    assert (r3["weights"][into4] == 0).all() and len(r3["history_stage2"]) >= 1


# ---- the edges of a scene --------------------------------------------------------------------------------------------------------------------
class HostContext:
    """Context.edge_information on host tensors through the reference, counting its calls"""

    def __init__(self):
        self.calls = []

    def edge_information(self, src, soff, tgt, T, max_dist):
        import torch
        self.calls.append((np.asarray(soff).copy(), tgt.shape[0]))
        n, r, m = MR.edge_info_ref(src.numpy(), soff, tgt.numpy(), T.numpy(), max_dist)
        return torch.from_numpy(n), torch.from_numpy(r), torch.from_numpy(m)


def test_scene_edges_groups_by_target_and_keeps_the_order_of_pairs():
    import torch
    assert MW.edge_chunks([(0, 1), (2, 1), (0, 2), (0, 3)], [5, 6, 7, 8]) == [(0, [0, 2, 3]), (2, [1])]
    assert MW.edge_chunks([(0, 1)] * 130, [5, 6]) == [(0, list(range(64))), (0, list(range(64, 128))), (0, [128, 129])]
    assert MW.edge_chunks([(0, 1), (0, 2), (0, 1)], [5, 6, 7], max_points=13) == [(0, [0, 1]), (0, [2])]
    rs = np.random.RandomState(3)
    base = rs.rand(300, 3)
    clouds = [(base[rs.permutation(300)[:120 + 10 * f]]).astype(f32) for f in range(4)]
    pairs = np.array([(0, 1), (2, 3), (0, 2), (1, 3), (0, 3)] + [(0, 1)] * 64, np.int64)       # 67 edges into fragment 0: two chunks
    T = np.stack([np.vstack([RR.perturbed(np.eye(4)[:3], rs, 1.0, 0.01), [0, 0, 0, 1]]) for _ in pairs])
    ctx = HostContext()
    ed = MW.scene_edges(ctx, [torch.from_numpy(c) for c in clouds], pairs, T, 0.05)
    assert [len(s) - 1 for s, _ in ctx.calls] == [64, 3, 1, 1] and [nt for _, nt in ctx.calls] == [120, 120, 130, 140]
    ref = MR.scene_edges_ref(clouds, pairs, T, 0.05)
    for k in ("npairs", "overlap", "rmse", "info"):
        assert ed[k].tobytes() == ref[k].tobytes(), k
    assert ed["npairs"].min() >= 10 and (ed["overlap"] <= 1).all()
    ed2, res = MW.register_scene(ctx, [torch.from_numpy(c) for c in clouds], pairs[:5], T[:5], tau=0.2)
    assert ed2["info"].tobytes() == ref["info"][:5].tobytes() and res["reached"].all()


# ---- files ---------------------------------------------------------------------------------------------------------------------------------
def make_scene(root, name, seed, F=5, n=700, frag=420, false_pair=(1, 3), split=None):
    """a scene on disk: F fragments, random subsets of one n-point cloud of a 1 m cube, each in its own frame; gt.log with every pair;
    YOHO_O's pre.log = the ground truth turned by 0.3 degrees / moved by 5 mm, `false_pair` 40 degrees off about the target's centroid;
    split: the registrations into the last fragment moved by +-split along the scene's x instead -> (dataset, pairs, pre (E,4,4))"""
    from yoho_amd.dataset import ThrDMatchPartDataset
    rs = np.random.RandomState(seed)
    pc = rs.rand(n, 3)
    Xg = [np.eye(4)] + [MR.motion(MR.random_direction(rs) * 0.8 * rs.rand(), rs.randn(3) * 0.5) for _ in range(F - 1)]
    os.makedirs(os.path.join(root, "PointCloud"))
    clouds = []
    for f in range(F):
        Xi = MR.inverse(Xg[f])
        clouds.append(pc[np.sort(rs.permutation(n)[:frag])] @ Xi[:3, :3].T + Xi[:3, 3])
        np.savetxt(os.path.join(root, "PointCloud", f"cloud_bin_{f}.txt"), clouds[f], delimiter=",")
    pairs = [(i, j) for i in range(F) for j in range(i + 1, F)]
    gt = np.stack([MR.inverse(Xg[i]) @ Xg[j] for i, j in pairs])
    RR_cal.write_trajectory(gt, [(i, j, F) for i, j in pairs], os.path.join(root, "PointCloud", "gt.log"))
    ds = ThrDMatchPartDataset(root, F)
    ds.name = name
    pre = []
    for (i, j), Tt in zip(pairs, gt):
        Tm = np.eye(4)
        Tm[:3] = RR.perturbed(Tt[:3], rs, 0.3, 0.005)
        if (i, j) == false_pair:
            c = clouds[i].mean(axis=0)
            turn = np.eye(4)
            turn[:3, :3] = RR.rot_axis_angle(rs.randn(3), 40.0)
            turn[:3, 3] = c - turn[:3, :3] @ c
            Tm = turn @ Tt
        if split is not None:
            Tm = Tt.copy()
            if j == F - 1:
                Tm[:3, 3] += MR.inverse(Xg[i])[:3, :3] @ np.array([split if i % 2 == 0 else -split, 0.0, 0.0])
        pre.append(Tm)
    return ds, np.array(pairs, np.int64), np.stack(pre)


def host_edges(calls):
    def edges(clouds, pairs, T, max_dist):
        calls.append((len(clouds), len(pairs), max_dist))
        return MR.scene_edges_ref(clouds, pairs, T, max_dist)
    return edges


def test_write_gt_info_round_trip(tmp_path):
    """gt.info in the Redwood format: read_trajectory_info gives back the fragment count and the matrices of every ground-truth pair under
    its ground-truth transform, in gt.log's order, to the last bit; an existing file is left alone"""
    ds, pairs, _ = make_scene(str(tmp_path / "sceneA"), "synthmw/sceneA", 0)
    calls = []
    path = MW.write_gt_info(ds, max_dist=0.05, edges=host_edges(calls))
    assert path == str(tmp_path / "sceneA" / "PointCloud" / "gt.info") and calls == [(5, 10, 0.05)]
    n_frag, mats = RR_cal.read_trajectory_info(path)
    keys, traj = RR_cal.read_trajectory(ds.gt_dir)
    clouds = [ds.get_pc(c).astype(f32) for c in ds.get_cloud_ids()]
    ref = MR.scene_edges_ref(clouds, pairs, traj, 0.05)
    assert n_frag == 5 and mats.shape == (10, 6, 6) and mats.tobytes() == ref["info"].tobytes()
    assert ref["npairs"].min() >= 100                                  # every pair shares about 0.6 * 0.6 of the 700 points
    lines = open(path).read().splitlines()
    assert len(lines) == 70 and lines[0].split() == ["0", "1", "5"] and lines[63].split() == ["3", "4", "5"] and all(len(l.split()) == 6 for l in lines[1:7])
    text = open(path).read()
    assert MW.write_gt_info(ds, edges=host_edges(calls)) is None and len(calls) == 1 and open(path).read() == text
    with open(path, "w") as fh:
        fh.write("stale\n")
    assert MW.write_gt_info(ds, edges=host_edges(calls), overwrite=True) == path and open(path).read() == text


def test_write_scene_and_benchmark_on_two_scenes(tmp_path):
    """write_scene -> read_pre_trajectory, and RR_cal.benchmark(..., yoho_sign='YOHO_O_MW') as it is, on two synthetic scenes: scene A
    has one false registration, which the pairwise result fails and the multiway result repairs; in scene B a strict prune
    disconnects the last fragment, whose pairs keep their pairwise estimates"""
    from yoho_amd.estimator import write_pre_log
    from yoho_amd.run_dataset import result_dir
    cfg = types.SimpleNamespace(output_cache_fn=str(tmp_path / "cache"), RR_dist_threshold=0.2)
    scenes = {"A": make_scene(str(tmp_path / "data" / "sceneA"), "synthmw/sceneA", 0),
              "B": make_scene(str(tmp_path / "data" / "sceneB"), "synthmw/sceneB", 1, false_pair=None, split=0.08)}
    datasets = {"wholesetname": "synthmw"}
    calls = []
    out = {}
    for key, (ds, pairs, pre) in scenes.items():
        datasets[key] = ds
        os.makedirs(result_dir(cfg, ds, "YOHO_O", 1000))
        write_pre_log(os.path.join(result_dir(cfg, ds, "YOHO_O", 1000), "pre.log"), 5, [(a, b, t) for (a, b), t in zip(pairs, pre)])
        assert MW.write_gt_info(ds, edges=host_edges(calls)) is not None
        kw = {"prune": 0.9} if key == "B" else {}
        out[key] = MW.write_scene(cfg, ds, edges=host_edges(calls), **kw)
    assert calls == [(5, 10, 0.05)] * 4
    # scene A: the false pair is pruned, every fragment reached, pre.log holds the implied transform of every pair in pair_ids order
    ds, pairs, pre = scenes["A"]
    ed, res = out["A"]
    bad = pairs.tolist().index([1, 3])
    assert res["pruned"].tolist() == [e == bad for e in range(10)] and res["reached"].all() and ed["npairs"][bad] >= 10
    keys, traj = RR_cal.read_pre_trajectory(os.path.join(result_dir(cfg, ds, "YOHO_O_MW", 1000), "pre.log"))
    assert [(k[0], k[1]) for k in keys] == ds.pair_ids and (keys[:, 2] == "5").all()
    assert np.array_equal(traj, MW.implied_transforms(res["poses"], pairs))                  # repr round trip: to the last bit
    pk, ptraj = RR_cal.read_trajectory(os.path.join(result_dir(cfg, ds, "YOHO_O_MW", 1000), "poses.log"))
    assert pk.tolist() == [[str(f), str(f), "5"] for f in range(5)] and np.abs(ptraj - res["poses"]).max() < 1e-12 and np.array_equal(ptraj[0], np.eye(4))
    gk, gt = RR_cal.read_trajectory(ds.gt_dir)
    assert RR.rot_error_deg(gt[bad][:3, :3], pre[bad][:3, :3]) > 39 and RR.rot_error_deg(gt[bad][:3, :3], traj[bad][:3, :3]) < 0.5
    # scene B: fragment 4 is cut off; its pairs keep the pairwise estimate, the others are implied
    ds, pairs, pre = scenes["B"]
    ed, res = out["B"]
    into4 = pairs[:, 1] == 4
    assert np.array_equal(res["pruned"], into4) and res["reached"].tolist() == [True] * 4 + [False]
    keys, traj = RR_cal.read_pre_trajectory(os.path.join(result_dir(cfg, ds, "YOHO_O_MW", 1000), "pre.log"))
    assert [(k[0], k[1]) for k in keys] == ds.pair_ids
    assert np.array_equal(traj[into4], pre[into4]) and np.array_equal(traj[~into4], MW.implied_transforms(res["poses"], pairs[~into4]))
    assert "nan" in open(os.path.join(result_dir(cfg, ds, "YOHO_O_MW", 1000), "poses.log")).read()
    # the benchmark, unchanged, on both signs
    rec_mw, flags_mw, _ = RR_cal.benchmark(cfg, datasets, 1000, yoho_sign="YOHO_O_MW")
    rec_pw, flags_pw, _ = RR_cal.benchmark(cfg, datasets, 1000, yoho_sign="YOHO_O")
    print(f"registration recall: pairwise {rec_pw:.3f}, multiway {rec_mw:.3f}")
    assert rec_mw == 1.0 and rec_pw == (5.0 / 6.0 + 1.0) / 2.0          # six non-consecutive pairs per scene, one of them false in scene A
    assert flags_pw["synthmw/sceneA"][bad] == 1 and flags_mw["synthmw/sceneA"][bad] == 0
    assert os.path.exists(os.path.join(cfg.output_cache_fn, "Testset", "synthmw", "Eval_results", "YOHO_O_MW_RR", "1000iters", "result.txt"))
