"""CPU tests of the k-nearest-neighbour search: the contract (tests/knn_ref.py) against the reference's own answers
(tests/golden/knn.npz, written by tools/gen_golden_knn.py), the fixture against a fresh run of the reference where its tree exists,
and the symbols of include/yoho_knn.h (the two invariants tests/test_abi.py / tests/test_gpu_abi.py keep for include/yoho_hip.h)."""
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import knn_ref as KR  # noqa: E402

TIE_CAP = 0.01           # share of rows that may be left out of an index comparison against the reference (torch.topk's tie order is open)


def knn_header_functions():
    txt = open(os.path.join(REPO, "include", "yoho_knn.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(yoho_[a-zA-Z0-9_]+)\s*\(", txt)))


@pytest.mark.parametrize("case", KR.FIXTURE_CASES, ids=lambda c: KR.case_name(*c))
def test_knn_ref_equals_reference_fixture(gold, case):
    """the stable argsort of the oracle's distances IS the reference's torch.topk(-dist, k): indices on every row without a tie
    among the reference's own distances (and at most 1 % of the rows have one), SquareL2 distances bit for bit, L2 to 1 ulp
    (the torch-CPU sqrt deviation of DESIGN section 6)"""
    g = gold("knn.npz")
    D, ns, nt, k, dt, seed = case
    name = KR.case_name(*case)
    assert name in set(g["cases"].tolist())
    assert g[name + "_params"].tolist() == [D, ns, nt, k, int(dt == "SquareL2"), seed]
    assert g[name + "_shape_dists"].tolist() == [ns, 1, k]
    assert g[name + "_shape_call_d"].tolist() == [1, k, 1, ns] and g[name + "_shape_call_idx"].tolist() == [1, k, ns]
    src, tgt = KR.fixture_inputs(D, ns, nt, seed)
    idx, dist = KR.knn_ref(src, tgt, k, dt == "SquareL2")
    ridx, rdist = g[name + "_idx"].astype(np.int64), g[name + "_dist"]
    assert ridx.shape == (ns, k) and rdist.shape == (ns, k)
    # ties: among the reference's k distances, and among the oracle's k + 1 (the k-th against the first one left out)
    ties = np.union1d(KR.tie_rows(rdist, k), KR.tie_rows(KR.knn_ref_more(src, tgt, k, dt == "SquareL2")[1], k))
    print(f"{name}: {len(ties)} of {ns} rows with a tie among the first k + 1 distances")
    assert len(ties) <= TIE_CAP * ns
    keep = np.setdiff1d(np.arange(ns), ties)
    assert np.array_equal(idx[keep], ridx[keep])
    ulps = KR.ulp_diff(dist, rdist)
    print(f"{name}: distances within {ulps} ulp of the reference's")
    assert ulps <= (0 if dt == "SquareL2" else 1)
    assert (np.diff(dist, axis=1) >= 0).all() and all(len(set(r)) == k for r in idx.tolist())


def test_fixture_regenerates_from_the_reference(gold):
    """where the reference tree exists (the build machine), tools/gen_golden_knn.py gives tests/golden/knn.npz again, array for array"""
    import gen_golden_knn as G
    if not G.reference_available():
        pytest.skip("the reference tree is not on this machine")
    fresh, g = G.generate(), gold("knn.npz")
    assert sorted(fresh) == sorted(g.files)
    for key in fresh:
        a, b = np.asarray(fresh[key]), g[key]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), key


def test_tie_rows_and_ref_order():
    """the helper itself: tie_rows looks at k + 1 columns, knn_ref puts the lower index first among equal distances"""
    d = np.array([[0., 1., 2., 2.], [0., 1., 1., 2.], [0., 0., 1., 2.], [0., 1., 2., 3.]], np.float32)
    assert KR.tie_rows(d, 2).tolist() == [1, 2] and KR.tie_rows(d, 3).tolist() == [0, 1, 2] and KR.tie_rows(d[:, :1], 1).tolist() == []
    tgt = np.ones((40, 32), np.float32)
    tgt[[30, 7, 19]] = 0.5
    idx, dist = KR.knn_ref(np.zeros((2, 32), np.float32), tgt, 4, False)
    assert idx.tolist() == [[7, 19, 30, 0]] * 2 and dist[0, 0] == dist[0, 2] < dist[0, 3]


def test_library_exports_knn_header_symbols():
    """include/yoho_knn.h: every function it declares is exported, the set is hip.KNN_SYMBOLS and shares nothing with hip.SYMBOLS (the
    list tests/test_abi.py pins to include/yoho_hip.h), and the header's limit is the binding's"""
    import ctypes as C
    from yoho_amd import build, hip
    lib_path = build.build(verbose=False)
    assert os.path.exists(lib_path)
    lib = hip.load_library()
    fns = knn_header_functions()
    assert fns == ["yoho_knn_search"]
    for f in fns:
        assert hasattr(lib, f), f"libyoho_hip.so does not export {f}"
    assert set(fns) == set(hip.KNN_SYMBOLS) and not set(hip.KNN_SYMBOLS) & set(hip.SYMBOLS)
    assert lib.yoho_knn_search.restype is C.c_int and len(lib.yoho_knn_search.argtypes) == 11
    hdr = open(os.path.join(REPO, "include", "yoho_knn.h")).read()
    assert int(re.search(r"#define\s+YOHO_KNN_MAX\s+(\d+)", hdr).group(1)) == hip.KNN_MAX == 16
    # and nothing of it leaked into the pinned header
    assert "yoho_knn" not in open(os.path.join(REPO, "include", "yoho_hip.h")).read()
