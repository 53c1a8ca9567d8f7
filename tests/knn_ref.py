"""The k-nearest-neighbour contract on the CPU (helper of tests/test_knn_cpu.py and tests/test_gpu_knn.py, not a conftest).

`knn_ref` is the order yoho_knn_search promises: the fp32 distances of oracle.yoho_oracle.pdist_l2 (torch-CPU summation order, 'L2'
= sqrt(D2 + 1e-7) correctly rounded), every row sorted ascending by (distance as returned, target index) - a stable argsort.  It gives
the reference's torch.topk(-dist, k) wherever the k + 1 smallest distances of a row are distinct; `tie_rows` names the other rows."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "oracle"))
import yoho_oracle as orc  # noqa: E402


def knn_ref(src, tgt, k, squared, chunk=250):
    """-> (idx (Ns,k) int64, dist (Ns,k) f32); the distance matrix is built `chunk` rows at a time, as oracle.find_nn does"""
    src, tgt = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(tgt, np.float32)
    idx = np.empty((src.shape[0], k), np.int64)
    dist = np.empty((src.shape[0], k), np.float32)
    for s in range(0, src.shape[0], chunk):
        d = orc.pdist_l2(src[s:s + chunk], tgt, squared=squared)
        o = np.argsort(d, axis=1, kind="stable")[:, :k]
        idx[s:s + chunk] = o
        dist[s:s + chunk] = np.take_along_axis(d, o, axis=1)
    return idx, dist


def knn_ref_more(src, tgt, k, squared):
    """knn_ref with one more column where the targets allow it: what tie_rows wants"""
    return knn_ref(src, tgt, min(k + 1, tgt.shape[0]), squared)


def tie_rows(dist_sorted, k):
    """rows whose first k + 1 distances (ascending; fewer columns are taken as they are) contain an equal pair"""
    d = np.asarray(dist_sorted)[:, :k + 1]
    if d.shape[1] < 2:
        return np.zeros((0,), np.int64)
    return np.nonzero((d[:, 1:] == d[:, :-1]).any(axis=1))[0]


def ulp_diff(a, b):
    """largest distance in units of the last place between two non-negative fp32 arrays"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()) if a.size else 0


def fixture_inputs(D, ns, nt, seed):
    """the seeded inputs of tests/golden/knn.npz (tools/gen_golden_knn.py): descriptor-like rows (the group mean of unit features, what
    the matcher searches) for D = 32, uniform points in the unit cube for D = 3"""
    from yoho_amd import synth, weights
    if D == 32:
        return (np.ascontiguousarray(np.mean(synth.unit_features(ns, seed=seed, name="knn_src"), -1), np.float32),
                np.ascontiguousarray(np.mean(synth.unit_features(nt, seed=seed, name="knn_tgt"), -1), np.float32))
    return (weights.hash_uniform(seed, "knn_src3", ns * 3).reshape(ns, 3), weights.hash_uniform(seed, "knn_tgt3", nt * 3).reshape(nt, 3))


# the cases of tests/golden/knn.npz: (D, Ns, Nt, k, dist_type, seed)
FIXTURE_CASES = [(32, 600, 700, k, dt, 11) for k in (2, 8, 16) for dt in ("L2", "SquareL2")] + [(3, 500, 900, 8, "L2", 12), (3, 500, 900, 8, "SquareL2", 12)]


def case_name(D, ns, nt, k, dt, seed):
    return f"d{D}_{ns}x{nt}_k{k}_{dt}"
