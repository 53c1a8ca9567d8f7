"""CPU tests of the verification entries (include/yoho_verify.h): the library builds and exports exactly their symbols, the numpy
restatement of their contracts (tests/verify_ref.py) follows the header's rules on hand-made inputs, and the pair that motivated the
entries behaves as described: the vote's winner is a decoy, the top 8 by count alone are all decoys, and with
near-duplicates suppressed the truncated cost picks the true hypothesis."""
import os
import re
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import refine_ref as RR  # noqa: E402
import verify_ref as VR  # noqa: E402

f32, f64 = np.float32, np.float64
I34 = VR.IDENTITY


def test_library_exports_verify_header_symbols():
    """include/yoho_verify.h declares exactly hip.VERIFY_SYMBOLS, the library exports them, the list shares nothing with the other
    five, the one limit of the header is the binding's, and nothing of it leaked into the older headers"""
    import ctypes as C
    from yoho_amd import build, hip
    assert os.path.exists(build.build(verbose=False))
    lib = hip.load_library()
    hdr = open(os.path.join(REPO, "include", "yoho_verify.h")).read()
    fns = sorted(set(re.findall(r"\b(yoho_[a-zA-Z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert fns == ["yoho_eval_transforms", "yoho_verify_hypotheses"]
    for f in fns:
        assert hasattr(lib, f), f"libyoho_hip.so does not export {f}"
    assert set(fns) == set(hip.VERIFY_SYMBOLS) and len(hip.VERIFY_SYMBOLS) == 2
    assert not set(hip.VERIFY_SYMBOLS) & set(hip.SYMBOLS + hip.KNN_SYMBOLS + hip.TRAINSET_SYMBOLS + hip.REFINE_SYMBOLS + hip.PLANE_SYMBOLS)
    for f, nargs in (("yoho_eval_transforms", 12), ("yoho_verify_hypotheses", 20)):
        assert getattr(lib, f).restype is C.c_int and len(getattr(lib, f).argtypes) == nargs
    assert '#include "yoho_refine.h"' in hdr and re.findall(r"#define\s+(\w+)", hdr) == ["YOHO_VERIFY_H", "YOHO_VERIFY_MAX_K"]
    assert int(re.search(r"#define\s+YOHO_VERIFY_MAX_K\s+(\d+)", hdr).group(1)) == hip.VERIFY_MAX_K == 64
    for older in ("yoho_hip.h", "yoho_knn.h", "yoho_trainset.h", "yoho_refine.h", "yoho_plane.h"):
        txt = open(os.path.join(REPO, "include", older)).read()
        assert not any(f in txt for f in fns), older
    assert build.EXTRA["verify.hip"] == ["-ffp-contract=off"] and "verify.hip" in build.SOURCES


def test_verify_kernels_use_no_scratch(tmp_path):
    """csrc/verify.hip compiled for gfx950 with the flags of the build: the compiler's resource report names the four kernels, none
    with scratch (a spill)"""
    from yoho_amd import build
    cmd = [build._hipcc()] + build.FLAGS + build.EXTRA["verify.hip"] + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                                                                       os.path.join(build.CSRC, "verify.hip"), "-o", str(tmp_path / "verify.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r"\bVGPRs: (\d+)", r.stderr)]
    assert len(names) == len(scratch) == len(vgprs) == 4, names
    for k in ("vf_select_kernel", "vf_eval_kernel", "vf_sum_kernel", "vf_pick_kernel"):
        assert sum(k in n for n in names) == 1, (k, names)
    print("verify.hip: " + ", ".join(f"{re.search(r'vf_[a-z]+_kernel', n).group(0)} {v} VGPRs" for n, v in zip(names, vgprs)))
    assert scratch == [0, 0, 0, 0], dict(zip(names, scratch))


def _rows(n, rs):
    """n well separated transforms (no two within 0.1 of each other in every entry)"""
    return np.stack([np.concatenate([RR.rot_axis_angle(rs.randn(3), 10.0 + 300.0 * rs.rand()), 5.0 * rs.randn(3, 1)], axis=1) for _ in range(n)])


def test_selection_rules():
    rs = np.random.RandomState(0)
    T = _rows(8, rs)
    # equal counts take the lower position; min_count; Kc < K
    counts = np.array([2, 5, 5, 1, 5, 0, 3, 2], np.int32)
    assert VR.top_ref(T, None, counts, 8) == [1, 2, 4, 6, 0, 7, 3]                # count 0 is never alive: min_count >= 1
    assert VR.top_ref(T, None, counts, 3) == [1, 2, 4]
    assert VR.top_ref(T, None, counts, 8, min_count=3) == [1, 2, 4, 6]
    assert VR.top_ref(T, None, counts, 8, min_count=6) == []
    # positions stand for T[order[h]], and top holds positions
    order = np.array([7, 6, 5, 4, 3, 2, 1, 0], np.int64)
    assert VR.top_ref(T, order, counts, 2) == [1, 2] and np.array_equal(VR.rows_of(T, order, 8)[1], T[6])
    # suppression: rows 1, 2 and 4 are one cluster (entries 2^-8 apart), row 6 sits exactly distinct_tol away in one entry: '<' keeps it
    Tc = T.copy()
    Tc[2] = Tc[1] + 2.0 ** -8
    Tc[4] = Tc[1] - 2.0 ** -8
    Tc[6] = Tc[1]
    Tc[6, 0, 3] = Tc[1, 0, 3] + 0.125
    assert abs(Tc[6, 0, 3] - Tc[1, 0, 3]) == 0.125
    assert VR.top_ref(Tc, None, counts, 8, distinct_tol=0.125) == [1, 6, 0, 7, 3]
    assert VR.top_ref(Tc, None, counts, 8, distinct_tol=0.126) == [1, 0, 7, 3]
    assert VR.top_ref(Tc, None, counts, 8, distinct_tol=0.0) == [1, 2, 4, 6, 0, 7, 3]
    # a NaN entry: the row is not suppressed by its twin, and taken itself it suppresses nothing - not even its twin
    Tn = Tc.copy()
    Tn[2, 1, 1] = np.nan
    assert VR.top_ref(Tn, None, counts, 8, distinct_tol=0.126) == [1, 2, 0, 7, 3]
    Tn = Tc.copy()
    Tn[1, 1, 1] = np.nan
    assert VR.top_ref(Tn, None, counts, 8, distinct_tol=0.126) == [1, 2, 0, 7, 3]      # 2 suppresses 4 and 6 (0.121 away) in its turn


def test_evaluation_and_pick_rules():
    rs = np.random.RandomState(1)
    tgt = rs.rand(300, 3).astype(f32)
    src = tgt[:257].copy()                                                            # two blocks of THE SUM, the second with one element
    far = I34.copy()
    far[:, 3] = 100.0
    nanrow = I34.copy()
    nanrow[1, 1] = np.nan
    T = np.stack([far, I34, nanrow, I34])
    npairs, rmse, cost = VR.eval_ref(src, tgt, T, 0.05)
    g2 = f64(RR.gate2_of(0.05))
    # a row without a pair: rmse +inf, cost = Ns x gate2 BY THE SUM (which the plain product is not obliged to equal)
    assert npairs[0] == 0 and rmse[0] == np.inf and cost[0] == RR.tree_sum(np.full((257,), g2)) and abs(cost[0] - 257 * g2) <= 1e-13
    assert npairs[1] == 257 and rmse[1] == 0.0 and cost[1] == 0.0
    # the NaN entry reaches the y coordinate of every query: all unpaired
    assert npairs[2] == 0 and rmse[2] == np.inf and cost[2] == cost[0]
    # the pick: equal costs keep the earlier row; rows behind Kc hold the fill values
    counts = np.array([4, 3, 2, 1], np.int32)
    r = VR.verify_ref(src, tgt, T, None, counts, 6, 0.05)
    assert r["Kc"] == 4 and r["top"].tolist() == [0, 1, 2, 3, -1, -1] and r["npairs"].tolist() == [0, 257, 0, 257, -1, -1]
    assert r["cost"][1] == r["cost"][3] and r["best"] == 1 and r["info"].tolist() == [4, 1, 1, 3]
    assert r["rmse"].tolist()[4:] == [-1.0, -1.0] and r["cost"].tolist()[4:] == [-1.0, -1.0] and r["T_out"].tobytes() == T[1].tobytes()
    r = VR.verify_ref(src, tgt, T, np.array([2, 0, 3, 1], np.int64), counts, 2, 0.05)    # positions 0, 1 = rows 2, 0: both cost the same
    assert r["best"] == 0 and r["info"].tolist() == [2, 0, 0, 4] and r["T_out"].tobytes() == T[2].tobytes()      # the NaN is copied, too
    # nothing alive, and H = 0
    for cnt, Tx in ((np.zeros((4,), np.int32), T), (np.zeros((0,), np.int32), np.zeros((0, 3, 4)))):
        r = VR.verify_ref(src, tgt, Tx, None, cnt, 3, 0.05)
        assert r["Kc"] == 0 and r["info"].tolist() == [0, -1, -1, 0] and np.array_equal(r["T_out"], I34)
        assert r["top"].tolist() == [-1] * 3 and r["npairs"].tolist() == [-1] * 3 and r["rmse"].tolist() == [-1.0] * 3 and r["cost"].tolist() == [-1.0] * 3
    # K = 1 is one iteration of the ICP reference, bit for bit
    c = RR.icp_case(n=1500, seed=0, overlap=0.6)
    n, e, _, _, _ = RR.icp_step(c["src"], c["tgt"], c["T0"], c["max_dist"])
    npairs, rmse, _ = VR.eval_ref(c["src"], c["tgt"], c["T0"][None], c["max_dist"])
    assert npairs[0] == n and rmse[0].tobytes() == f64(e).tobytes()


def test_decoy_pair_conditions():
    """seeds 0-3: the vote's winner is a decoy; K = 8 with suppression holds both clusters and the truncated cost picks the true one,
    at least 0.5 below the vote winner's; K = 8 by count alone never leaves the decoy cluster"""
    for seed in range(4):
        c = VR.decoy_case(seed)
        gt = c["T_gt"][:, :3]
        assert c["src"].shape == c["tgt"].shape == (900, 3) and c["counts"].shape == (200,)
        win = int(np.argmax(c["counts"]))                                             # the vote's strict '>': the first maximum
        e_vote = RR.rot_error_deg(gt, c["T"][c["order"][win]][:, :3])
        r = VR.verify_ref(c["src"], c["tgt"], c["T"], c["order"], c["counts"], 8, c["max_dist"], distinct_tol=0.1)
        e_pick = RR.rot_error_deg(gt, r["T_out"][:, :3])
        plain = VR.verify_ref(c["src"], c["tgt"], c["T"], c["order"], c["counts"], 8, c["max_dist"], distinct_tol=0.0)
        e_plain = RR.rot_error_deg(gt, plain["T_out"][:, :3])
        print(f"seed {seed}: vote winner {c['counts'][win]} inliers, {e_vote:.1f} deg off; suppressed top 8: Kc {r['Kc']}, counts {c['counts'][r['top'][:r['Kc']]].tolist()}, "
              f"pairs {r['npairs'][:r['Kc']].tolist()}, cost {np.round(r['cost'][:r['Kc']], 3).tolist()}, pick {e_pick:.2f} deg off; "
              f"by count alone: counts {c['counts'][plain['top']].tolist()}, pick {e_plain:.1f} deg off")
        assert e_vote > 50.0 and r["top"][0] == win
        assert 4 <= r["Kc"] <= 8 and e_pick < 1.0 and r["cost"][r["best"]] <= r["cost"][0] - 0.5
        assert plain["Kc"] == 8 and e_plain > 50.0
