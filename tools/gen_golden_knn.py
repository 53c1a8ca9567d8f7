"""Generate tests/golden/knn.npz: the reference's own k-nearest-neighbour answers (utils/knn_search.py find_knn_gpu and the k >= 2
branch of __call__) on seeded inputs, computed on CPU tensors.

    python tools/gen_golden_knn.py            # rewrites tests/golden/knn.npz

The reference module is loaded by path at generation time only (the tree oracle/gen_golden.py reads, or $YOHO_REFERENCE); nothing of
it is copied.  The fixture holds no inputs: tests/knn_ref.py:fixture_inputs rebuilds them from the seeds with the project's generators.
Per case (tests/knn_ref.py:FIXTURE_CASES) it stores find_knn_gpu's indices as int32 (N,k), its distances (N,k) f32 with the shape the
reference returned them in (N,1,k), and the shapes of KNN(k)(target, source), whose contents the generator checks to be the same
neighbours transposed.  tests/test_knn_cpu.py regenerates and compares wherever the reference tree exists."""
import importlib.util
import os
import sys
import warnings

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "knn.npz")
for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import knn_ref as KR  # noqa: E402


def reference_root():
    root = os.environ.get("YOHO_REFERENCE")
    if not root:
        from gen_golden import REF          # oracle/gen_golden.py: where the other generators read the reference
        root = REF
    return root


def reference_available():
    return os.path.isfile(os.path.join(reference_root(), "utils", "knn_search.py"))


def load_reference_module():
    spec = importlib.util.spec_from_file_location("_ref_knn_search", os.path.join(reference_root(), "utils", "knn_search.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def generate():
    ref = load_reference_module()
    out = {"cases": np.array([KR.case_name(*c) for c in KR.FIXTURE_CASES])}
    for case in KR.FIXTURE_CASES:
        D, ns, nt, k, dt, seed = case
        name = KR.case_name(*case)
        src, tgt = KR.fixture_inputs(D, ns, nt, seed)
        m = ref.knn_module.KNN(k)
        dists, inds = m.find_knn_gpu(torch.from_numpy(src), torch.from_numpy(tgt), dist_type=dt)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")           # the reference's d.T on a 3-D tensor (utils/knn_search.py:162)
            cd, ci = m(torch.from_numpy(np.ascontiguousarray(tgt.T))[None], torch.from_numpy(np.ascontiguousarray(src.T))[None], dist_type=dt)
        assert tuple(dists.shape) == (ns, 1, k) and tuple(inds.shape) == (ns, k), (dists.shape, inds.shape)
        # __call__ hands find_knn_gpu transposed VIEWS, whose torch.sum runs in another order than a contiguous row's: the same
        # neighbours, distances a few ulps away (the mirror copies its inputs contiguous and has the contiguous order)
        assert torch.equal(ci[0].T, inds) and KR.ulp_diff(cd[0, :, 0, :].T.numpy(), dists[:, 0, :].numpy()) <= 4, name
        out[name + "_params"] = np.array([D, ns, nt, k, int(dt == "SquareL2"), seed], np.int64)
        out[name + "_idx"] = inds.numpy().astype(np.int32)
        out[name + "_dist"] = dists.numpy()[:, 0, :].astype(np.float32)
        out[name + "_shape_dists"] = np.array(dists.shape, np.int64)
        out[name + "_shape_call_d"] = np.array(cd.shape, np.int64)
        out[name + "_shape_call_idx"] = np.array(ci.shape, np.int64)
    return out


if __name__ == "__main__":
    arrays = generate()
    np.savez_compressed(GOLD, **arrays)
    print("wrote", os.path.relpath(GOLD, REPO), os.path.getsize(GOLD), "bytes,", len(KR.FIXTURE_CASES), "cases")
