"""Every caller of rfgrid.h's one walk over the distinct buckets, and both key policies of disk.hip's one set of thinning rounds, on
the GPU (-m gpu) on the two inputs at which a walk goes wrong: tests/test_gpu_disk.py's 100 rows whose 27 cells mostly share a bucket,
and its 600 rows beyond the grid's 2^20-cell clamp.  Everything compared is an integer: plain equality, no tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cluster_ref as CL  # noqa: E402
import disk_ref as DR  # noqa: E402
import salient_ref as SR  # noqa: E402
from test_gpu_clean import R_FAR, slots27  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def ctx(hip):
    return hip.Context()


@pytest.fixture(scope="module")
def clouds():
    """[(name, pts, radius, neighbours_ref)]; the inputs are asserted to be the ones that go wrong: at least 10 of the 100 rows meet a
    neighbour twice on a walk that does not skip repeated slots, the clamped rows have at most 8 / 18 distinct slots of 27"""
    rs = np.random.RandomState(41)
    pts = (rs.rand(100, 3) * 0.3 + 0.375).astype(f32)
    s = slots27(pts, 0.1, 100)
    nb = CL.neighbours_ref(pts, 0.1)
    twice = np.array([any((s[i] == s[j, 13]).sum() >= 2 for j in nb[i][0]) for i in range(100)])
    assert twice.sum() >= 10
    far = (rs.rand(600, 3) * 0.004).astype(f32)
    far[:200] += f32(4000.0)
    far[200:400] -= f32(4000.0)
    far[400:450, 0] += f32(4000.0)                                                                 # clamped on one axis only
    distinct = np.array([len(set(row)) for row in slots27(far, R_FAR, 600).tolist()])
    assert distinct[:400].max() <= 8 and distinct[400:450].max() <= 18
    return [("shared buckets", pts, 0.1, nb), ("beyond the clamp", far, R_FAR, CL.neighbours_ref(far, R_FAR))]


def test_every_walk_counts_the_same_neighbours(ctx, clouds):
    """count of yoho_knn_within (skip_same_row), yoho_dbscan, yoho_estimate_normals and yoho_iss_saliency: the last two count the row
    itself, the first two do not (every row of both clouds is finite), and each equals cluster_ref.neighbours_ref"""
    for name, pts, r, nb in clouds:
        p = cu(pts)
        want = np.array([len(j) for j, _ in nb], np.int32)
        assert np.isfinite(pts).all() and want.max() >= 3, name
        knn = ctx.knn_within(p, p, r, 1, skip_same_row=True, want_idx=False, want_d2=False)[2].cpu().numpy()
        listed = ctx.knn_within(p, p, r, 9, skip_same_row=True)[2].cpu().numpy()                  # the kernel with the insertion chain in the functor
        db = ctx.dbscan(p, r, 4)["count"].cpu().numpy()
        nrm = ctx.estimate_normals(p, r, 3)[1].cpu().numpy()
        iss = ctx.iss_saliency(p, r)[1].cpu().numpy()
        for what, got in (("knn_within", knn + 1), ("knn_within, k = 9", listed + 1), ("dbscan", db + 1), ("estimate_normals", nrm), ("iss_saliency", iss)):
            assert got.dtype == np.int32 and np.array_equal(got, want + 1), (name, what, np.nonzero(got != want + 1)[0][:8])


def test_both_key_policies_run_the_same_rounds(ctx, clouds):
    """yoho_disk_sample_prio with a random and with a constant priority, one round per call, equals salient_ref.disk_prio_rounds_ref
    state by state, and in one call its last state and n_out; with the constant priority the bytes are yoho_disk_sample's"""
    for name, pts, r, _ in clouds:
        p = cu(pts)
        n = len(pts)
        for seed in (0, 1):
            for kind, prio in (("random", np.random.RandomState(7 + seed).rand(n).astype(f32)), ("constant", np.full((n,), 0.25, f32))):
                st = SR.disk_prio_rounds_ref(pts, r, prio, seed)
                assert (st[-1] != 0).all() and 2 <= len(st) - 1 <= DR.MAX_ROUNDS, (name, kind)
                pr = cu(prio)
                got, n_out = ctx.disk_sample_prio(p, r, pr, seed=seed, rounds=DR.MAX_ROUNDS)
                assert got.cpu().numpy().tobytes() == st[-1].tobytes() and n_out.cpu().numpy().tobytes() == DR.n_out_of(st).tobytes(), (name, kind, seed)
                state = None
                for k in range(1, len(st)):
                    state, n1 = ctx.disk_sample_prio(p, r, pr, seed=seed, rounds=1, state=state)
                    assert state.cpu().numpy().tobytes() == st[k].tobytes(), (name, kind, seed, k)
                    assert n1.tolist() == [int((st[k] == 1).sum()), 1, int((st[k] == 0).sum())], (name, kind, seed, k)
                if kind == "constant":
                    hashed, n_h = ctx.disk_sample(p, r, seed=seed, rounds=DR.MAX_ROUNDS)
                    assert hashed.cpu().numpy().tobytes() == got.cpu().numpy().tobytes() and n_h.tolist() == n_out.tolist(), (name, seed)
                    state = None
                    for k in range(1, len(st)):
                        state, _ = ctx.disk_sample(p, r, seed=seed, rounds=1, state=state)
                        assert state.cpu().numpy().tobytes() == st[k].tobytes(), (name, "hashed", seed, k)
