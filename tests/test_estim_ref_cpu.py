"""The estimators' high-precision reference (oracle/estim_ref.py) and its fixture (tests/golden/estim_edges.npz), on the CPU:
the reference against the LAPACK path of the oracle and the golden vectors of the reference's own run, the exact vote against
numpy, and the fixture against a fresh run of its generator, family conditions included."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import estim_ref as er  # noqa: E402
import gen_golden_estim as gen  # noqa: E402
import yoho_oracle as orc  # noqa: E402


def have_mpmath():
    try:
        import mpmath  # noqa: F401
        return True
    except ImportError:
        return False


needs_mpmath = pytest.mark.skipif(not have_mpmath(), reason="mpmath is not installed: the 80-digit reference cannot be re-run here")


@pytest.fixture(scope="module")
def edges(gold):
    return gold("estim_edges.npz")


@needs_mpmath
def test_kabsch_ref_vs_lapack_on_nominal():
    fams = gen.kabsch_families()
    for name in (n for n in fams if n.startswith("nominal/")):
        a0, a1, _ = fams[name]
        for i in range(a0.shape[0]):
            r = er.kabsch_ref(a0[i], a1[i])
            To, _ = orc.threepps2tran(a0[i], a1[i], proper=True)
            assert r["cls"] == "rank2"
            assert np.max(np.abs(r["R"] - To[:, :3])) < 1e-13 and np.max(np.abs(r["t"] - To[:, 3])) < 1e-13, (name, i)
            # the optimum really is one: the objective of the reference's own R is f_min, and LAPACK's R is not below it
            fmin = er.Fraction(r["f_min"][0]) + er.Fraction(r["f_min"][1])
            assert abs(float(er.objective(r["R"], a0[i], a1[i]) - fmin)) < 1e-14 * r["N"]
            assert float(er.objective(To[:, :3], a0[i], a1[i]) - fmin) > -1e-14 * r["N"]


@needs_mpmath
def test_kabsch_ref_vs_golden_reference_run(gold):
    """tests/golden/kabsch.npz holds the reference's own Threepps2Tran outputs: no determinant fix, so its reflections are
    the proper rotation times the mirror in the plane of the k1 triangle"""
    g = gold("kabsch.npz")
    nrefl = 0
    for i in range(g["k0"].shape[0]):
        r = er.kabsch_ref(g["k0"][i], g["k1"][i])
        R = r["R"]
        if np.linalg.det(g["T"][i][:, :3]) < 0:
            x = g["k1"][i] - g["k1"][i].mean(axis=0)
            n = np.cross(x[1] - x[0], x[2] - x[0])
            n /= np.linalg.norm(n)
            R = R @ (np.eye(3) - 2.0 * np.outer(n, n))
            nrefl += 1
        else:
            assert np.max(np.abs(r["t"] - g["T"][i][:, 3])) < 1e-12, i
        assert np.max(np.abs(R - g["T"][i][:, :3])) < 1e-12, i
    assert 0 < nrefl < g["k0"].shape[0]


def test_rank_classes_are_exact():
    a = np.array([[0.1, 0.2, 0.3], [1.1, 0.25, 0.3], [0.4, 0.9, 0.7]])
    b = np.array([[0.5, 0.5, 0.5], [0.75, 0.5, 0.5], [1.25, 0.5, 0.5]])            # collinear as numbers
    p = np.repeat(np.array([[0.1, 0.7, 0.3]]), 3, axis=0)                           # (p + p + p) / 3 = p as numbers, not in float64
    assert er.rank_class(a, a[[1, 2, 0]]) == "rank2"
    assert er.rank_class(a, b) == "rank1" and er.rank_class(b, a) == "rank1" and er.rank_class(a[[0, 0, 1]], a[[0, 0, 1]]) == "rank1"
    assert er.rank_class(a, p) == "rank0" and er.rank_class(p, p) == "rank0"


def test_vote_exact_vs_numpy(edges):
    fams = gen.vote_families()
    f = fams["dyadic"]
    v = er.vote_exact(f["k0"], f["k1"], f["T"], f["d"])
    ref = np.array([[orc.inlier_count(f["k0"][:M], f["k1"][:M], T, f["d"]) for M in (1, 64, 1500)] for T in f["T"]])
    got = np.stack([v["inl"][:, :M].sum(axis=1) for M in (1, 64, 1500)], axis=1)
    assert np.array_equal(got, ref)                                                  # no rounding on this grid: equal, ties included
    f = fams["random"]
    v = er.vote_exact(f["k0"], f["k1"], f["T"], f["d"])
    s_np = np.stack([np.sum(np.square(f["k0"] - orc.transform_points(f["k1"], T)), axis=-1) for T in f["T"]])
    differ = (s_np < v["d2"]) != v["inl"]
    assert not (differ & v["sure"]).any()                                            # equal up to unsure decisions
    assert np.max(np.abs(s_np - v["s"]) / v["b"]) < 0.5                              # numpy stays inside the ambiguity bound
    for h in range(f["T"].shape[0]):
        lo = int((v["inl"][h] & v["sure"][h]).sum())
        assert lo <= orc.inlier_count(f["k0"], f["k1"], f["T"][h], f["d"]) <= lo + int((~v["sure"][h]).sum())
    assert np.array_equal(np.packbits(v["inl"], axis=1), edges["vote__random__inl"])


def test_family_conditions(edges):
    """what the generator promises, read back from the file: rank classes, the s1 / s2 cap, e_np, no unsure decision where none
    is allowed, the on-threshold share"""
    kab = gen.kabsch_families()
    assert list(edges["kab_names"]) == list(kab)
    for name, (a0, a1, cls) in kab.items():
        k = gen.key(name)
        assert str(edges[f"kab__{k}__sha"]) == gen.sha(a0) + gen.sha(a1), name
        assert str(edges[f"kab__{k}__cls"]) == cls
        assert {er.rank_class(a0[i], a1[i]) for i in range(a0.shape[0])} == {cls}, name          # exactly so, not nearly
        if cls == "rank2":
            s = edges[f"kab__{k}__s"]
            assert np.all(s[:, 1] > 0) and np.max(s[:, 0] / s[:, 1]) <= gen.S12_CAP, name
            e_np = float(edges[f"kab__{k}__e_np"])
            assert np.isfinite(e_np) and e_np > 0, name
        elif cls == "rank1":
            assert np.all(edges[f"kab__{k}__s"][:, 0] > 0) and np.all(edges[f"kab__{k}__s"][:, 1] == 0), name
    assert kab["repeat3"][0].shape[0] == 512
    votes = gen.vote_families()
    assert list(edges["vote_names"]) == list(votes)
    for name, f in votes.items():
        k = gen.key(name)
        assert str(edges[f"vote__{k}__sha"]) == gen.sha(f["k0"]) + gen.sha(f["k1"]) + gen.sha(f["T"]), name
        n_unsure = int(edges[f"vote__{k}__unsure_n"])
        if name == "random":
            assert n_unsure * 100000 <= f["T"].shape[0] * gen.VOTE_M
        else:
            assert n_unsure == 0, name
            assert (f["kind"] == 0).sum() >= 0.05 * gen.VOTE_M if name == "dyadic" else (f["kind"] != 0).sum() >= 0.05 * gen.VOTE_M
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "estim_edges.npz")) < 300 * 1024


@needs_mpmath
def test_fixture_is_what_the_generator_makes(edges):
    fresh = gen.generate(verbose=False)
    assert sorted(fresh) == sorted(edges.files)
    for key in edges.files:
        a, b = np.asarray(fresh[key]), edges[key]
        assert a.dtype == b.dtype and a.shape == b.shape, key
        if key.endswith("__e_np"):
            # a measurement of this machine's LAPACK, not a reference value: its last bits follow the BLAS kernels of the CPU it
            # ran on.  The same quantity measured twice must agree in size.
            assert 0.5 <= float(a) / float(b) <= 2.0, (key, float(a), float(b))
        elif a.dtype.kind == "f":
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), key           # bit for bit
        else:
            assert np.array_equal(a, b), key
