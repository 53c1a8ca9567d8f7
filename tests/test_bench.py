"""bench.py's own contract: the plain line (headline only, exactly --steps timed steps) and --dump-outputs (what the timed path
returned for its last pair).  The CPU test writes a fabricated result; the GPU test runs the plain command and recomputes its last pair."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench():
    sys.path.insert(0, REPO)
    import bench
    return bench


def test_dump_outputs_names_dtypes_and_seeded_sample(tmp_path):
    from yoho_amd.pipeline import PairResult
    bench = _bench()
    g = torch.Generator().manual_seed(0)
    eqv, inv = torch.randn(900, 32, 60, generator=g), torch.randn(900, 32, generator=g)
    r = PairResult()
    r.trans, r.best_h, r.best_count, r.matches = np.arange(12.0).reshape(3, 4), 4, 17, 120
    r.eqv = ({"eqv": eqv[:600], "inv_np": inv[:600]}, {"eqv": eqv[600:], "inv_np": inv[600:]})
    r.match = torch.randint(0, 300, (120, 2), generator=g)
    r.dr_index = r.quat = r.trans_pre = None
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), r)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) == sorted(
        n + ".npy" for n in ("trans", "registration", "eqv0_rows", "eqv0_sample", "inv0", "eqv1_rows", "eqv1_sample", "inv1", "match"))
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
    assert np.array_equal(np.load(tmp_path / "a" / "registration.npy"), [4, 17, 120])
    assert np.array_equal(np.load(tmp_path / "a" / "match.npy"), r.match.numpy())
    for i, (lo, n) in enumerate(((0, 600), (600, 300))):
        rows = np.load(tmp_path / "a" / f"eqv{i}_rows.npy").astype(np.int64)
        assert len(rows) == min(n, bench.DUMP_EQV_ROWS) and len(set(rows.tolist())) == len(rows) and rows.max() < n
        assert np.array_equal(np.load(tmp_path / "a" / f"eqv{i}_sample.npy"), eqv[lo:lo + n].numpy()[rows])
        assert np.array_equal(np.load(tmp_path / "a" / f"inv{i}.npy"), inv[lo:lo + n].numpy())


@pytest.mark.gpu
def test_plain_bench_times_its_steps_and_dumps_the_last_pair(tmp_path, hip, sd1, sd2):
    """`bench.py --steps 3 --warmup 1 --dump-outputs DIR`: one timed region of exactly 3 steps, the headline keys and none of the
    --full legs; the dumped arrays are the last timed pair's - the rank-0 pair with the vote order of the last step's seed, recomputed
    here through the staged entries bit for bit"""
    from yoho_amd import pipeline, synth
    out = tmp_path / "out"
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    d = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert all(k in d for k in HEADLINE) and d["higher_is_better"] is True and d["unit"] == "keypoints/s"
    assert d["steps"] == 3 and d["ms_per_step_repeats"]["n"] == 1 and d["ms_per_step"] > 0
    assert abs(d["value"] - 2 * 5000 * 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"]
    assert not {"roofline", "sustained", "yohoc", "fgemm8", "fcgf", "dataset", "cpu_baseline"} & set(d)
    ctx = hip.Context()
    ctx.load_partI(sd1)
    ctx.load_partII(sd2)
    pr = synth.make_pair(5000, seed=10)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    r = pipeline.run_pair(ctx, cu(pr["feat0"]), cu(pr["feat1"]), cu(pr["keys0"]), cu(pr["keys1"]), inlier_dist=0.09, max_iter=1000,
                          order_rng=np.random.RandomState(1000 + 3 - 1))
    got = lambda n: np.load(out / (n + ".npy"))
    assert np.array_equal(got("trans"), r.trans)
    assert np.array_equal(got("registration"), [r.best_h, r.best_count, r.matches])
    for i in range(2):
        rows = torch.from_numpy(got(f"eqv{i}_rows").astype(np.int64)).cuda()
        assert np.array_equal(got(f"eqv{i}_sample"), r.eqv[i]["eqv"][rows].cpu().numpy())
        assert np.array_equal(got(f"inv{i}"), r.eqv[i]["inv_np"].cpu().numpy())
