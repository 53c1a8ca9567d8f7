"""The synthetic training set behind tests/golden/trainset.npz, rebuilt from seeds by the generator (tools/gen_golden_trainset.py,
which runs the reference's YOHO_Trainset.py on it) and by the CPU and GPU tests of yoho_amd.YOHO_Trainset.

Three scenes, duck types of utils/dataset.py:ThrDMatchPartDataset as the training-set driver uses it (name, root, pc_ids, pair_ids,
get_pc / get_kps / get_key_dir / get_transform):

    trainA   3 fragments, 3 pairs of ~100 correspondences                      (training)
    valA     2 fragments, 1 pair                                               (validation: in 'valscenes')
    edge     3 fragments: pair 0-1 has 10..31 correspondences (the `< 32` repeat branch), pair 0-2 fewer than 10 (skipped)

A fragment's 300 keypoints are a base shared by the scene + noise (the reference pairs keypoints WITHOUT the ground truth,
YOHO_Trainset.py:57-61, so corresponding keys are close in their own frames); they sit at scattered rows of a 400-point cloud.
pca_0.3 keeps about 70 % of them.  Everything comes from weights.hash_uniform / synth._gauss, i.e. the same bits on any machine.
The rotated feature blocks (5, kn, 32, 60) are hashed noise; their 5 rotations are the reference's random_rotation_matrix() drawn by
the generator and stored in the fixture."""
import os
import pickle
from collections import OrderedDict

import numpy as np
import torch

from yoho_amd import synth
from yoho_amd.weights import hash_uniform

NAME = "synth_train"
SEED = 2024
K = 300                 # keypoints per fragment
NPC = 400               # points per fragment cloud
VALSCENES = ["valA"]
# scene -> (fragments, pairs, {fragment: how many of its keys follow the scene's base; the others lie 5 m away})
SPEC = OrderedDict([
    ("trainA", (3, [("0", "1"), ("0", "2"), ("1", "2")], {})),
    ("valA", (2, [("0", "1")], {})),
    ("edge", (3, [("0", "1"), ("0", "2")], {1: 80, 2: 18})),
])
SEED_NP, SEED_PY = 11, 13       # np.random.seed / random.seed once, before trainset(); valset() follows on the same streams, as in run()


class Fragments:
    def __init__(self, scene, pcs, key_idx, pcas, pair_ids, gts):
        self.scene = scene
        self.name = f"{NAME}/{scene}"
        self.root = None                                 # set by TrainSet.write_inputs
        self.pcs, self.key_idx, self.pcas, self.gts = pcs, key_idx, pcas, gts
        self.pc_ids = [str(k) for k in range(len(pcs))]
        self.pair_ids = list(pair_ids)

    def get_pc(self, pc_id):
        return self.pcs[int(pc_id)]

    def get_kps(self, pc_id):
        return self.pcs[int(pc_id)][self.key_idx[int(pc_id)]]

    def get_key_dir(self, pc_id):
        return f"{self.root}/Keypoints/cloud_bin_{pc_id}Keypoints.txt"

    def get_transform(self, id0, id1):
        return self.gts[(id0, id1)]


def _rotation34(seed, name):
    """a (3,4) float32 ground truth as ThrDMatchPartDataset.parse_gt_fn returns it"""
    q = synth._gauss(seed, name, 4, np.float64)
    q = q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    T = np.zeros((3, 4), np.float64)
    T[:, :3] = synth.quat_to_mat64(q)
    T[:, 3] = hash_uniform(seed, name + "/t", 3)
    return T.astype(np.float32)


class TrainSet:
    def __init__(self):
        self.scenes = OrderedDict()
        for scene, (nfrag, pairs, near) in SPEC.items():
            base = hash_uniform(SEED, f"{scene}/base", 3 * K).astype(np.float64).reshape(K, 3)
            pcs, kidx, pcas = [], [], []
            for k in range(nfrag):
                keys = base + 0.008 * synth._gauss(SEED, f"{scene}/{k}/noise", 3 * K, np.float64).reshape(K, 3)
                if k in near:
                    keys[near[k]:] += 5.0
                pc = hash_uniform(SEED, f"{scene}/{k}/pc", 3 * NPC).astype(np.float64).reshape(NPC, 3) + 2.0
                idx = (7 * np.arange(K) + 3) % NPC       # distinct rows: 7 and 400 are coprime
                pc[idx] = keys
                pcs.append(pc)
                kidx.append(idx.astype(np.int64))
                pcas.append(0.1 * hash_uniform(SEED, f"{scene}/{k}/pca", 3 * K).astype(np.float64).reshape(K, 3))
            gts = {p: _rotation34(SEED, f"{scene}/{p[0]}-{p[1]}/gt") for p in pairs}
            self.scenes[scene] = Fragments(scene, pcs, kidx, pcas, pairs, gts)

    def datasets(self):
        """the dict utils/dataset.py:get_dataset_name returns for a training set"""
        d = OrderedDict([("wholesetname", NAME), ("valscenes", list(VALSCENES))])
        d.update(self.scenes)
        return d

    def write_inputs(self, root):
        """what PCA_keys_sample reads from disk: Keypoints/cloud_bin_{k}Keypoints.txt (rows of the cloud) and pca_0.3/{k}.npy"""
        for scene, d in self.scenes.items():
            d.root = f"{root}/{NAME}/{scene}"
            os.makedirs(f"{d.root}/Keypoints", exist_ok=True)
            os.makedirs(f"{d.root}/pca_0.3", exist_ok=True)
            for k, pc_id in enumerate(d.pc_ids):
                np.savetxt(d.get_key_dir(pc_id), d.key_idx[k])
                np.save(f"{d.root}/pca_0.3/{pc_id}.npy", d.pcas[k])
        return self

    def ok_index(self, scene, pc_id):
        """rows of the fragment's keypoints that pass the PCA filter (YOHO_Trainset.py:46)"""
        return np.arange(K)[self.scenes[scene].pcas[int(pc_id)][:, 0] > 0.03]

    def fragments(self):
        """(scene, pc_id) in the order the driver visits them"""
        return [(scene, pc_id) for scene, d in self.scenes.items() for pc_id in d.pc_ids]

    def rotated_features(self, scene, pc_id):
        """the fragment's (5, kn, 32, 60) f32 block: hashed noise in [-0.5, 0.5)"""
        kn = len(self.ok_index(scene, pc_id))
        return (hash_uniform(SEED, f"{scene}/{pc_id}/rot", 5 * kn * 32 * 60) - np.float32(0.5)).astype(np.float32).reshape(5, kn, 32, 60)

    def write_rotated_features(self, output_dir, Rs_of):
        """Rotated_Features/{name}/{id}_feats.npz + {id}_Rs.npy as PC_random_rot_feat leaves them; Rs_of(scene, pc_id) -> (5,3,3) f64"""
        for scene, pc_id in self.fragments():
            d = f"{output_dir}/Rotated_Features/{self.scenes[scene].name}"
            os.makedirs(d, exist_ok=True)
            Rs = np.asarray(Rs_of(scene, pc_id), np.float64)
            np.save(f"{d}/{pc_id}_Rs.npy", Rs)
            np.savez(f"{d}/{pc_id}_feats.npz", Rs=Rs, feats=self.rotated_features(scene, pc_id))


def build_dataset():
    return TrainSet()


# ---- the generated Train_val_list files against the fixture (CPU and GPU tests) ---------------------------------------------------

def check_train_items(out_dir, g):
    nb = len(g["train_pcp_i"])
    for b in range(nb):
        item = torch.load(f"{out_dir}/Train_val_list/trainset/{b}.pth", weights_only=False)
        assert sorted(item) == ["R", "deltaR", "feats0", "feats1", "keys0", "keys1", "true_idx"]
        assert item["true_idx"].dtype == torch.int64 and np.array_equal(item["true_idx"].numpy(), g["train_true_idx"][b]), b
        for k in ("keys0", "keys1"):
            assert item[k].dtype == torch.float32 and np.array_equal(item[k].numpy(), g["train_" + k][b]), (b, k)
        for k in ("deltaR", "R"):
            assert item[k].dtype == torch.float32 and item[k].shape == g["train_" + k][b].shape
            assert np.abs(item[k].numpy() - g["train_" + k][b]).max() <= 1e-6, (b, k)
        for k, dk in (("feats0", "dig0"), ("feats1", "dig1")):
            assert item[k].dtype == torch.float32 and tuple(item[k].shape) == (32, 32, 60)
            assert np.array_equal(synth.tensor_digest(item[k].numpy()), g["train_" + dk][b]), (b, k)      # rows are copied: exact
    assert not os.path.exists(f"{out_dir}/Train_val_list/trainset/{nb}.pth")


def check_val_items(out_dir, g):
    vp = pickle.load(open(f"{out_dir}/Train_val_list/val_pcp.pkl", "rb"))
    nv = len(g["val_pcp_idx"])
    assert len(vp) == nv and pickle.load(open(f"{out_dir}/Train_val_list/val.pkl", "rb")) == list(range(nv))
    assert [t[:3] for t in vp] == list(zip(g["val_pcp_name"].tolist(), g["val_pcp_pc0"].tolist(), g["val_pcp_pc1"].tolist()))
    assert np.array_equal(np.array([[int(x) for x in t[3:]] for t in vp]), g["val_pcp_idx"])
    for i in range(nv):
        item = torch.load(f"{out_dir}/Train_val_list/valset/{i}.pth", weights_only=False)
        assert sorted(item) == ["R", "feats0", "feats1", "keys0", "keys1", "true_idx"]
        assert item["true_idx"].dtype == torch.int64 and np.array_equal(item["true_idx"].numpy(), g["val_true_idx"][i]), i
        for k in ("keys0", "keys1"):                              # the reference's quirk: numpy f64 rows
            assert isinstance(item[k], np.ndarray) and item[k].dtype == np.float64 and np.array_equal(item[k], g["val_" + k][i])
        assert item["R"].dtype == torch.float32 and np.abs(item["R"].numpy() - g["val_R"][i]).max() <= 1e-6
        for k, dk in (("feats0", "dig0"), ("feats1", "dig1")):
            assert item[k].dtype == torch.float32 and tuple(item[k].shape) == (32, 60)
            assert np.array_equal(synth.tensor_digest(item[k].numpy()), g["val_" + dk][i]), (i, k)
    assert not os.path.exists(f"{out_dir}/Train_val_list/valset/{nv}.pth")
