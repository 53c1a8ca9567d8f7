"""Generate tests/golden/trainset.npz: the reference's own YOHO_Trainset.py (trainset_create.PCA_keys_sample / trainset / valset and
utils.utils.random_rotation_matrix) run on the synthetic set of tests/trainset_fixture.py, on CPU tensors.

    python tools/gen_golden_trainset.py [--out FILE]        # rewrites tests/golden/trainset.npz (or writes FILE)

The reference modules are loaded by path at generation time only (the tree oracle/gen_golden.py reads, or $YOHO_REFERENCE); nothing
of them is copied.  They need the import shims oracle/gen_golden.py uses (np.int, .cuda() -> identity, a stub tensorboardX / open3d)
plus stubs for `utils.misc` and `fcgf_model` (MinkowskiEngine): FCGF_Group_Feature_Extractor is the one stage that cannot run here,
so Rotated_Features are written from seeds (tests/trainset_fixture.py) with rotations drawn by the reference's
random_rotation_matrix() under a seeded np.random.RandomState (its generator is otherwise unseedable).  The shims change this
process for good: run it as a program (tests/test_trainset_cpu.py starts it as a child process).

The fixture holds no inputs.  Stored: the PCA-filtered key rows and the correspondence list of every pair; every fragment's 5
rotations; per pair the 5 x 5 true_idx / deltaR / R; per training batch the drawn (pps, Index_i, Index_j), true_idx, deltaR, R,
keys0 / keys1 and synth.tensor_digest of feats0 / feats1; train_pcp / val_pcp; per validation item true_idx, R, keys and digests;
four random_rotation_matrix() results for RandomState(0..3).
Conditions the generator asserts, so that no last bit decides a stored answer: no keypoint pair has an f64 distance within 1e-5
relative of 0.02; for every stored rotation the best and second-best compute_R_diff over the 60 group elements are more than 1e-6
degrees apart; scene 'edge' has one pair of 10..31 correspondences and one of fewer than 10."""
import importlib.util
import os
import pickle
import random
import sys
import tempfile
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "trainset.npz")
for p in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import trainset_fixture as TF  # noqa: E402
from yoho_amd import synth  # noqa: E402


def reference_root():
    root = os.environ.get("YOHO_REFERENCE")
    if not root:
        from gen_golden import REF          # oracle/gen_golden.py: where the other generators read the reference
        root = REF
    return root


def reference_available():
    return os.path.isfile(os.path.join(reference_root(), "YOHO_Trainset.py"))


def load_reference():
    """-> (YOHO_Trainset module, utils.utils module, utils.r_eval module) of the reference"""
    root = reference_root()
    np.int = int
    np.float = float
    torch.Tensor.cuda = lambda self, *a, **k: self
    sys.modules["tensorboardX"] = types.SimpleNamespace(SummaryWriter=object)
    sys.modules["open3d"] = types.ModuleType("open3d")
    misc = types.ModuleType("utils.misc")
    misc.extract_features = None                       # the backbone stage is not run
    sys.modules["utils.misc"] = misc
    fm = types.ModuleType("fcgf_model")
    fm.load_model = None
    sys.modules["fcgf_model"] = fm
    sys.argv = ["x"]
    sys.path.insert(0, root)
    spec = importlib.util.spec_from_file_location("_ref_YOHO_Trainset", os.path.join(root, "YOHO_Trainset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import utils.utils as ref_utils
    import utils.r_eval as ref_r_eval
    return mod, ref_utils, ref_r_eval


def seeded_rotation(ref_utils, seed):
    """the reference's random_rotation_matrix() with its `np.random.RandomState()` replaced by RandomState(seed) for the call"""
    orig = np.random.RandomState
    np.random.RandomState = lambda *a, **k: orig(seed)
    try:
        return ref_utils.random_rotation_matrix()
    finally:
        np.random.RandomState = orig


def assert_group_margin(ref_r_eval, Rgroup, Rs, what):
    for R in np.asarray(Rs, np.float64).reshape(-1, 3, 3):
        d = np.sort([ref_r_eval.compute_R_diff(Rgroup[g], R) for g in range(Rgroup.shape[0])])
        assert d[1] - d[0] > 1e-6, (what, d[:2])


def generate():
    ref, ref_utils, ref_r_eval = load_reference()
    ts = TF.build_dataset()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        ts.write_inputs(f"{tmp}/origin")
        tc = object.__new__(ref.trainset_create)
        tc.dataset_name = TF.NAME
        tc.origin_data_dir = f"{tmp}/origin"
        tc.datasets = ts.datasets()
        tc.output_dir = f"{tmp}/out"
        tc.Rgroup = np.load(os.path.join(reference_root(), "group_related", "Rotation.npy"))
        tc.valscenes = tc.datasets["valscenes"]

        # -- filtered keys and correspondences
        tc.PCA_keys_sample()
        npairs = {}
        for scene, d in ts.scenes.items():
            for k, pc_id in enumerate(d.pc_ids):
                ok = ts.ok_index(scene, pc_id)
                assert np.array_equal(np.load(f"{tc.output_dir}/Filtered_Keys/{d.name}/{pc_id}_index.npy"), d.key_idx[k][ok])
                assert np.array_equal(np.load(f"{tc.output_dir}/Filtered_Keys/{d.name}/{pc_id}_coor.npy"), d.get_kps(pc_id)[ok])
                out[f"{scene}_{pc_id}_ok"] = ok.astype(np.int32)
            for p0, p1 in d.pair_ids:
                pairs = np.load(f"{tc.output_dir}/Pairs_0.03/{d.name}/{p0}-{p1}.npy")
                k0, k1 = d.get_kps(p0)[ts.ok_index(scene, p0)], d.get_kps(p1)[ts.ok_index(scene, p1)]
                dist = np.linalg.norm(k0[:, None, :] - k1[None, :, :], axis=-1)
                margin = np.abs(dist - 0.02).min() / 0.02
                assert margin > 1e-5, (scene, p0, p1, margin)
                print(f"{scene} {p0}-{p1}: {len(k0)} x {len(k1)} filtered keys, {len(pairs)} correspondences, closest distance {margin:.1e} relative from 0.02")
                out[f"{scene}_{p0}-{p1}_pairs"] = pairs.astype(np.int32)
                npairs[(scene, p0, p1)] = len(pairs)
        assert 10 <= npairs[("edge", "0", "1")] < 32 and npairs[("edge", "0", "2")] < 10, npairs

        # -- rotated features: seeds + the reference's rotations
        Rs_of = {}
        for no, (scene, pc_id) in enumerate(ts.fragments()):
            Rs_of[(scene, pc_id)] = np.stack([seeded_rotation(ref_utils, 100 + 5 * no + r) for r in range(5)])
            out[f"{scene}_{pc_id}_Rs"] = Rs_of[(scene, pc_id)]
        ts.write_rotated_features(tc.output_dir, lambda scene, pc_id: Rs_of[(scene, pc_id)])
        out["rrm"] = np.stack([seeded_rotation(ref_utils, s) for s in range(4)])
        assert_group_margin(ref_r_eval, tc.Rgroup, out["rrm"], "rrm")

        # -- the 5 x 5 labels of every pair, by the reference's own R2DR_id / DeltaR
        for scene, d in ts.scenes.items():
            for p0, p1 in d.pair_ids:
                R_gt = d.get_transform(p0, p1)[0:3, 0:3]
                Rs, idx, dR = [], [], []
                for R_i in Rs_of[(scene, p0)]:
                    for R_j in Rs_of[(scene, p1)]:
                        R = R_j @ R_gt.T @ R_i.T
                        Rs.append(R)
                        idx.append(tc.R2DR_id(R))
                        dR.append(tc.DeltaR(R, idx[-1]))
                assert_group_margin(ref_r_eval, tc.Rgroup, Rs, (scene, p0, p1))
                out[f"{scene}_{p0}-{p1}_R"] = np.stack(Rs).reshape(5, 5, 3, 3)
                out[f"{scene}_{p0}-{p1}_true_idx"] = np.array(idx, np.int64).reshape(5, 5)
                out[f"{scene}_{p0}-{p1}_deltaR"] = np.stack(dR).reshape(5, 5, 4)

        # -- trainset(), with the draws recorded
        log = []
        orig_choice, orig_shuffle = np.random.choice, np.random.shuffle

        def choice(*a, **k):
            r = orig_choice(*a, **k)
            log.append(("c", np.array(r)))
            return r

        def shuffle(x):
            orig_shuffle(x)
            log.append(("s", np.array(x[:32])))
        np.random.seed(TF.SEED_NP)
        random.seed(TF.SEED_PY)
        np.random.choice, np.random.shuffle = choice, shuffle
        try:
            tc.trainset()
        finally:
            np.random.choice, np.random.shuffle = orig_choice, orig_shuffle
        with open(f"{tc.output_dir}/Train_val_list/train_pcp.pkl", "rb") as f:
            pcp = pickle.load(f)
        with open(f"{tc.output_dir}/Train_val_list/train.pkl", "rb") as f:
            assert pickle.load(f) == list(range(len(pcp)))
        assert len(pcp) == 10 * sum(1 for (s, _, _), n in npairs.items() if s not in TF.VALSCENES and n >= 10) == 40
        out["train_pcp_name"] = np.array([t[0] for t in pcp])
        out["train_pcp_pc0"] = np.array([t[1] for t in pcp])
        out["train_pcp_pc1"] = np.array([t[2] for t in pcp])
        out["train_pcp_i"] = np.array([t[3] for t in pcp], np.int64)
        cols = {k: [] for k in ("pps", "Ii", "Ij", "true_idx", "deltaR", "R", "keys0", "keys1", "dig0", "dig1")}
        pos = 0
        for b, (name, p0, p1, i) in enumerate(pcp):
            scene = name.split("/")[-1]
            if i == 0 and npairs[(scene, p0, p1)] < 32:
                assert log[pos][0] == "s"                # the shuffle of the repeat branch
                pos += 1
            (ks, sh), (k1, Ii), (k2, Ij) = log[pos:pos + 3]
            assert (ks, k1, k2) == ("s", "c", "c")
            pos += 3
            item = torch.load(f"{tc.output_dir}/Train_val_list/trainset/{b}.pth", weights_only=False)
            pps = out[f"{scene}_{p0}-{p1}_pairs"][sh]
            d = ts.scenes[scene]
            assert np.array_equal(item["keys0"].numpy(), d.get_kps(p0)[pps[:, 0]].astype(np.float32))
            assert np.array_equal(item["true_idx"].numpy(), out[f"{scene}_{p0}-{p1}_true_idx"][Ii, Ij])
            assert item["feats0"].dtype == torch.float32 and tuple(item["feats0"].shape) == (32, 32, 60)
            cols["pps"].append(pps.astype(np.int32)); cols["Ii"].append(Ii.astype(np.int8)); cols["Ij"].append(Ij.astype(np.int8))
            for k in ("true_idx", "deltaR", "R", "keys0", "keys1"):
                cols[k].append(item[k].numpy())
            cols["dig0"].append(synth.tensor_digest(item["feats0"].numpy()))
            cols["dig1"].append(synth.tensor_digest(item["feats1"].numpy()))
        assert pos == len(log)
        for k, v in cols.items():
            out["train_" + k] = np.stack(v)
        assert out["train_true_idx"].dtype == np.int64 and out["train_deltaR"].dtype == np.float32 and out["train_keys0"].dtype == np.float32

        # -- valset(), on the streams as trainset() left them (the order of the reference's __main__)
        tc.valset()
        with open(f"{tc.output_dir}/Train_val_list/val_pcp.pkl", "rb") as f:
            vp = pickle.load(f)
        with open(f"{tc.output_dir}/Train_val_list/val.pkl", "rb") as f:
            assert pickle.load(f) == list(range(len(vp)))
        assert 0 < len(vp) == sum(n for (s, _, _), n in npairs.items() if s in TF.VALSCENES) < 5000
        out["val_pcp_name"] = np.array([t[0] for t in vp])
        out["val_pcp_pc0"] = np.array([t[1] for t in vp])
        out["val_pcp_pc1"] = np.array([t[2] for t in vp])
        out["val_pcp_idx"] = np.array([[int(x) for x in t[3:]] for t in vp], np.int64)          # Ri, Rj, pt0, pt1
        cols = {k: [] for k in ("true_idx", "R", "keys0", "keys1", "dig0", "dig1")}
        for i in range(len(vp)):
            item = torch.load(f"{tc.output_dir}/Train_val_list/valset/{i}.pth", weights_only=False)
            assert sorted(item) == ["R", "feats0", "feats1", "keys0", "keys1", "true_idx"] and isinstance(item["keys0"], np.ndarray)
            cols["true_idx"].append(item["true_idx"].numpy()); cols["R"].append(item["R"].numpy())
            cols["keys0"].append(item["keys0"]); cols["keys1"].append(item["keys1"])
            cols["dig0"].append(synth.tensor_digest(item["feats0"].numpy()))
            cols["dig1"].append(synth.tensor_digest(item["feats1"].numpy()))
        for k, v in cols.items():
            out["val_" + k] = np.stack(v)
        assert out["val_keys0"].dtype == np.float64 and out["val_true_idx"].shape == (len(vp), 1)
        assert_group_margin(ref_r_eval, tc.Rgroup, out["val_R"], "val")
    return out


if __name__ == "__main__":
    dst = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLD
    arrays = generate()
    np.savez_compressed(dst, **arrays)
    print("wrote", dst, os.path.getsize(dst), "bytes,", len(arrays), "arrays")
