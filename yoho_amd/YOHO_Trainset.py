"""Drop-in for YOHO_Trainset.py: "generate the training set for PartI and PartII" from fragment clouds, gt.log and pca_0.3.

    trainset_create(cfg).run()          # = the reference's __main__: PCA_keys_sample, PC_random_rot_feat, trainset, valset

writes, under ``output_dir``, the reference's layout in the reference's file formats

    Filtered_Keys/{scene}/{id}_coor.npy, {id}_index.npy       keypoints that pass the PCA filter (coordinates, rows of the cloud)
    Pairs_0.03/{scene}/{a}-{b}.npy                            (M,2) int64 correspondences between two fragments' filtered keys
    Rotated_Features/{scene}/{id}_feats.npz (Rs, feats), {id}_Rs.npy      5 random rotations, (5,kn,32,60) f32 group features
    Train_val_list/trainset/{i}.pth, valset/{i}.pth, train.pkl, train_pcp.pkl, val.pkl, val_pcp.pkl

with the reference's skip-if-exists rules, so a set half made by the reference is continued here and either side's output feeds
either side's trainer (yoho_amd.train reads exactly these files).  The thresholds 0.03 (PCA) and 0.02 (pairs), 5 random rotations,
10 batches of 32 per pair and 5000 validation items are the reference's constants.

Where the work goes: correspondences are yoho_radius_pairs (Context.radius_pairs: no (N0,N1) matrix); the 5 x 60 backbone passes
of a fragment are testset_create's pipeline (fcgf_extractor.rotated_passes + yoho_group_gather, two lanes, a loader and a writer
thread); a fragment's feature block is uploaded once per scene (yoho_amd.store's budget) and the rows of all 10 batches of a pair
are cut by one yoho_trainset_gather call per side; the labels (25 rotations per pair x 60 group elements) are host f64.

np.random / random are consumed exactly as the reference consumes them, so a seeded run reproduces the reference's batches:
per pair the `< 32` repeat + shuffle, per batch shuffle(pps_all), choice x 2; valset two choice(size=1) per correspondence (drawn
here as one choice(size=2n): the same stream), random.shuffle, the first 5000.

The reference's quirks are kept:
  * correspondences are searched WITHOUT applying the ground truth (:57-61): fragments are expected in one frame;
  * keys0 / keys1 of an item index the UNFILTERED dataset.get_kps with indices of the filtered keys (:198-212, :279-282);
  * valset's R = R_j @ R_i.T leaves the ground truth out (:285); val items carry numpy f64 keys (:292-293).
Deviations, stated:
  * trainset() returns at once when the set is complete - train_pcp.pkl is the whole list the pair files imply, train.pkl numbers
    it and every item exists - and valset() keeps an item that exists; the reference (its check at :170 is commented out) redraws and
    rewrites all of them on every run.  A set interrupted between scenes is not complete and is made again from the first pair;
  * group features take the nearest down-sampled point in f32 coordinates (yoho_group_gather, as YOHO_testset.py:92), the
    reference's open3d KD-tree in f64.

``cfg`` needs ``model`` (FCGF checkpoint path or dict; only read when a fragment's features are missing) and ``voxel_size``;
optional ``datasetname`` ('3dmatch_train'), ``output_dir`` / ``origin_dir`` (defaults './data/YOHO_FCGF', './data/origin_data', :26-28),
``datasets`` (a prebuilt dict incl. 'valscenes', otherwise ``get_dataset_name(datasetname, origin_dir)``) and ``rot_seed`` (the random
rotations become reproducible; unseeded like the reference by default).
"""
import os
import pickle
import queue
import random
import threading

import numpy as np
import torch

from . import hip, store
from .dataset import get_dataset_name
from .utils import make_non_exists_dir, random_rotation_matrix, quaternion_from_matrix, group_R_diff
from .YOHO_testset import group_features

N_ROT = 5             # random rotations per fragment
N_BATCH = 10          # batches per pair
BATCH = 32            # correspondences per batch
N_VAL = 5000          # validation items


def read_pickle(fn):
    with open(fn, 'rb') as f:
        return pickle.load(f)


def save_pickle(data, fn):
    make_non_exists_dir(os.path.dirname(fn))
    with open(fn, 'wb') as f:
        pickle.dump(data, f)


class _Writer:
    """one thread that runs queued jobs (event to wait for, function that writes files) in order; at most `depth` wait"""

    def __init__(self, name, depth=2):
        self.q = queue.Queue(maxsize=depth)
        self.errors = []
        self.t = threading.Thread(target=self._loop, name=name, daemon=True)
        self.t.start()

    def _loop(self):
        while True:
            job = self.q.get()
            if job is None:
                return
            done, fn = job
            try:
                if not self.errors:
                    if done is not None:
                        done.synchronize()
                    fn()
            except BaseException as e:
                self.errors.append(e)

    def put(self, done, fn):
        self.q.put((done, fn))

    def close(self):
        self.q.put(None)
        self.t.join()
        if self.errors:
            raise self.errors[0]


class trainset_create():
    def __init__(self, config, ctx=None):
        self.config = config
        self.dataset_name = getattr(config, 'datasetname', '3dmatch_train')
        self.origin_data_dir = getattr(config, 'origin_dir', './data/origin_data')
        self.output_dir = getattr(config, 'output_dir', './data/YOHO_FCGF')
        self.datasets = getattr(config, 'datasets', None) or get_dataset_name(self.dataset_name, self.origin_data_dir)
        self.valscenes = self.datasets['valscenes']
        self.ctx = ctx if ctx is not None else hip.get_context()
        self.Rgroup = self.ctx.tables.R64
        self.rot_seed = getattr(config, 'rot_seed', None)
        self.lanes = max(1, min(2, int(os.environ.get("YOHO_FCGF_LANES", "2"))))      # backbone lanes, as testset_create
        self._fcgf = None
        self.stats = {}

    def _scenes(self, training_only=False):
        """[(key, dataset)] of the scenes, without the two entries of the dict that are not scenes"""
        return [(name, d) for name, d in self.datasets.items()
                if name not in ('wholesetname', 'valscenes') and not (training_only and name in self.valscenes)]

    def _pairs_file(self, dataset, pc0, pc1):
        return f'{self.output_dir}/Pairs_0.03/{dataset.name}/{pc0}-{pc1}.npy'

    # ---- keypoints and correspondences ----------------------------------------------------------------------------------------
    def PCA_keys_sample(self):
        """:32-62.  Per fragment: the keypoints whose first pca_0.3 value exceeds 0.03, as coordinates ({id}_coor.npy) and as rows of the
        cloud ({id}_index.npy).  Per pair: the (M,2) list of filtered keys closer than 0.02 (rows of the two _coor files), without the
        ground truth applied - yoho_radius_pairs on the f32 coordinates, a fragment's keys uploaded once per scene."""
        for _, dataset in self._scenes():
            keys_dir = f'{self.output_dir}/Filtered_Keys/{dataset.name}'
            make_non_exists_dir(keys_dir)
            make_non_exists_dir(os.path.dirname(self._pairs_file(dataset, 0, 0)))
            for pc_id in dataset.pc_ids:
                if os.path.exists(f'{keys_dir}/{pc_id}_index.npy'):
                    continue
                rows_in_cloud = np.loadtxt(dataset.get_key_dir(pc_id)).astype(int)
                keep = np.flatnonzero(np.load(f'{dataset.root}/pca_0.3/{pc_id}.npy')[:, 0] > 0.03)
                np.save(f'{keys_dir}/{pc_id}_coor.npy', dataset.get_kps(pc_id)[keep])
                np.save(f'{keys_dir}/{pc_id}_index.npy', rows_in_cloud[keep])
            on_device = {}

            def keys_of(pc_id):
                if pc_id not in on_device:
                    on_device[pc_id] = torch.from_numpy(np.load(f'{keys_dir}/{pc_id}_coor.npy').astype(np.float32).reshape(-1, 3)).cuda()
                return on_device[pc_id]

            for pc0, pc1 in dataset.pair_ids:
                if not os.path.exists(self._pairs_file(dataset, pc0, pc1)):
                    np.save(self._pairs_file(dataset, pc0, pc1), self.ctx.radius_pairs(keys_of(pc0), keys_of(pc1), 0.02).cpu().numpy())

    # ---- rotated group features ----------------------------------------------------------------------------------------------
    def _use_args(self, args):
        """the reference hands its argparse namespace (model, voxel_size) to the feature methods; here it is the constructor's cfg,
        which a namespace given to a method replaces"""
        if args is not None and args is not self.config:
            self.config, self._fcgf = args, None

    @property
    def fcgf(self):
        """the backbone, loaded when the first fragment without features is met"""
        if self._fcgf is None:
            from .fcgf_feat import fcgf_extractor
            self._fcgf = fcgf_extractor(self.config.model, ctx=self.ctx)
            if self.lanes > 1:
                self._fcgf.lane_context()
        return self._fcgf

    def fragment_group_features(self, pc, keys, join=True):
        """pc (N,3), keys (K,3) f64 -> (K,32,60) f32 cuda, all 60 group elements: the routine testset_create runs (YOHO_testset.group_features)"""
        return group_features(self.fcgf, self.Rgroup, self.lanes, self.config.voxel_size, pc, keys, join)

    def FCGF_Group_Feature_Extractor(self, args, Point, Keys_index):
        """:65-109: Point (N,3) f64, Keys_index rows of it -> (kn,32,60) f32 numpy.  `args` as the reference's (None: the constructor's cfg)"""
        self._use_args(args)
        Point = np.asarray(Point, dtype=np.float64)
        return self.fragment_group_features(Point, Point[Keys_index]).cpu().numpy()

    def PC_random_rot_feat(self, args=None):
        """:112-137.  Per fragment 5 random rotations; the rotated cloud PC @ R.T is formed on the host in f64 as the reference forms it
        (the voxel decisions are those of its two roundings) and uploaded per rotation.  The next fragment is read ahead by a loader
        thread, the finished (5,kn,32,60) block leaves through a page-locked buffer and a writer thread."""
        import time
        self._use_args(args)
        jobs = []
        for _, dataset in self._scenes():
            save_dir = f'{self.output_dir}/Rotated_Features/{dataset.name}'
            make_non_exists_dir(save_dir)
            jobs += [(dataset, pc_id, save_dir) for pc_id in dataset.pc_ids if not os.path.exists(f'{save_dir}/{pc_id}_feats.npz')]
        self.stats['rot_feat'] = {"fragments": len(jobs), "seconds": 0.0, "lanes": self.lanes}
        if not jobs:
            return
        t_start = time.perf_counter()
        loaded = queue.Queue(maxsize=2)
        errors = []
        stop = threading.Event()

        def loader():
            try:
                for no, (dataset, pc_id, save_dir) in enumerate(jobs):
                    if stop.is_set():
                        break
                    cloud = np.asarray(dataset.get_pc(pc_id), dtype=np.float64)
                    key_rows = np.load(f'{self.output_dir}/Filtered_Keys/{dataset.name}/{pc_id}_index.npy')
                    loaded.put((cloud, key_rows, save_dir, pc_id, no))
            except BaseException as e:
                errors.append(e)
            loaded.put(None)

        tl = threading.Thread(target=loader, name="trainset-loader", daemon=True)
        tl.start()
        writer = _Writer("trainset-feat-writer")
        copy_stream = self.fcgf.stream_beside_lanes(self.lanes)
        ended = False
        try:
            while True:
                item = loaded.get()
                ended = item is None
                if ended or errors or writer.errors:
                    break
                cloud, key_rows, save_dir, pc_id, no = item
                Rs = np.stack([random_rotation_matrix(None if self.rot_seed is None else self.rot_seed + N_ROT * no + r) for r in range(N_ROT)])
                host = torch.empty((N_ROT, key_rows.shape[0], 32, 60), dtype=torch.float32, pin_memory=True)
                for r in range(N_ROT):
                    turned = cloud @ Rs[r].T
                    out = self.fragment_group_features(turned, turned[key_rows], join=copy_stream)
                    with torch.cuda.stream(copy_stream):
                        host[r].copy_(out, non_blocking=True)
                    del out
                done = torch.cuda.Event()
                done.record(copy_stream)

                def write(host=host, Rs=Rs, save_dir=save_dir, pc_id=pc_id):
                    np.save(f'{save_dir}/{pc_id}_Rs.npy', Rs)
                    tmp = f'{save_dir}/{pc_id}_feats.{os.getpid()}.tmp.npz'      # the skip test looks at the .npz: it must never be seen half written
                    np.savez(tmp, Rs=Rs, feats=host.numpy())
                    os.replace(tmp, f'{save_dir}/{pc_id}_feats.npz')
                writer.put(done, write)
        finally:
            stop.set()
            try:
                writer.close()
            finally:
                if not ended:
                    while loaded.get() is not None:
                        pass
                tl.join()
        torch.cuda.synchronize()
        if errors:
            raise errors[0]
        self.stats['rot_feat']["seconds"] = time.perf_counter() - t_start

    # ---- labels ------------------------------------------------------------------------------------------------------------------
    def R2DR_ids(self, Rs):
        """:140-148 for a stack (n,3,3): the group element with the smallest compute_R_diff; the first minimum wins (the reference's
        strict `<` from 180), f64"""
        diff = group_R_diff(self.Rgroup, Rs)
        best = np.argmin(diff, axis=1)
        best[diff[np.arange(len(best)), best] >= 180] = 0
        return best

    def R2DR_id(self, R):
        return int(self.R2DR_ids(np.asarray(R)[None])[0])

    def DeltaR(self, R, index):
        """:151-155: the residual of R over group element `index` (R = residual @ Rgroup[index]) as a quaternion"""
        return quaternion_from_matrix(R @ self.Rgroup[index].T)

    def pair_labels(self, Rs0, Rs1, R_gt):
        """:178-194 -> R (5,5,3,3), true_idx (5,5), deltaR (5,5,4) for every (rotation i of pc0, rotation j of pc1):
        R = R_j @ R_gt.T @ R_i.T takes pc0 turned by R_i to pc1 turned by R_j"""
        R = np.stack([R_j @ R_gt.T @ R_i.T for R_i in Rs0 for R_j in Rs1])
        idx = self.R2DR_ids(R)
        dR = np.stack([self.DeltaR(r, i) for r, i in zip(R, idx)])
        n0, n1 = len(Rs0), len(Rs1)
        return R.reshape(n0, n1, 3, 3), idx.reshape(n0, n1), dR.reshape(n0, n1, 4)

    # ---- feature blocks on the device ------------------------------------------------------------------------------------------
    def _block(self, name, pc_id):
        """(Rs (5,3,3), feats (5,kn,32,60) f32 cuda) of Rotated_Features/{name}/{pc_id}_feats.npz: read and uploaded once while
        yoho_amd.store keeps it"""
        feats, rest = store.load_npz(f'{self.output_dir}/Rotated_Features/{name}/{pc_id}_feats.npz', 'feats')
        return rest['Rs'], feats

    def _gather_to_host(self, feats_d, rot, key, stream):
        """rows feats_d[rot, key] -> page-locked (B,32,60), complete when `stream` has run"""
        out = self.ctx.trainset_gather(feats_d, rot, key)
        host = torch.empty(out.shape, dtype=torch.float32, pin_memory=True)
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            host.copy_(out, non_blocking=True)
        out.record_stream(stream)
        return host

    # ---- batches ---------------------------------------------------------------------------------------------------------------------
    def _expected_train_list(self):
        """train_pcp.pkl as a finished trainset() leaves it, from the pair lists alone (nothing random decides it): 10 entries for every
        pair of a training scene with at least 10 correspondences, in the driver's order; None while a pair list is missing"""
        want = []
        for _, dataset in self._scenes(training_only=True):
            for pc0, pc1 in dataset.pair_ids:
                fn = self._pairs_file(dataset, pc0, pc1)
                if not os.path.exists(fn):
                    return None
                if np.load(fn).shape[0] >= 10:
                    want += [(dataset.name, pc0, pc1, i) for i in range(N_BATCH)]
        return want

    def _trainset_complete(self, item_dir):
        """the lists are rewritten after every scene, so their existence says nothing: the set is complete when train_pcp.pkl is the
        whole expected list, train.pkl numbers it and every item is on disk.  A set interrupted between scenes (here or in the
        reference) is not, and is made again from the first pair - the random stream has no other place to resume from."""
        lists = [f'{self.output_dir}/Train_val_list/train.pkl', f'{self.output_dir}/Train_val_list/train_pcp.pkl']
        want = self._expected_train_list()
        if want is None or not all(os.path.exists(fn) for fn in lists):
            return False
        if [tuple(t) for t in read_pickle(lists[1])] != want or list(read_pickle(lists[0])) != list(range(len(want))):
            return False
        return all(os.path.exists(f'{item_dir}/{i}.pth') for i in range(len(want)))

    def trainset(self):
        """:158-248.  Per pair of a training scene with at least 10 correspondences: 10 batches of 32 correspondences, each row with
        its own random rotation of either fragment and the labels of that combination."""
        item_dir = f'{self.output_dir}/Train_val_list/trainset'
        make_non_exists_dir(item_dir)
        if self._trainset_complete(item_dir):
            return
        copy_stream = torch.cuda.Stream() if torch.cuda.is_available() else None
        writer = _Writer("trainset-batch-writer", depth=4)
        listed = []                                                 # (scene, pc0, pc1, batch of the pair); its length numbers the next item
        rotations = np.arange(N_ROT).astype(int)
        try:
            for _, dataset in self._scenes(training_only=True):
                for pc0, pc1 in dataset.pair_ids:
                    corr = np.load(self._pairs_file(dataset, pc0, pc1))       # (M,2) rows of the filtered keys
                    M = corr.shape[0]
                    if M < 10:                                      # the reference reads the features first; nothing random happens before this
                        continue
                    Rs0, feats0 = self._block(dataset.name, pc0)
                    Rs1, feats1 = self._block(dataset.name, pc1)
                    R, true_idx, deltaR = self.pair_labels(Rs0, Rs1, dataset.get_transform(pc0, pc1)[0:3, 0:3])
                    kps0, kps1 = dataset.get_kps(pc0), dataset.get_kps(pc1)      # the quirk: unfiltered keypoints, filtered rows
                    # the random stream, call for call as the reference: fewer than 32 -> repeated to at least 32 and shuffled once;
                    # then per batch a shuffle (its first 32 are the batch) and a rotation per row for either fragment
                    order = np.arange(M)
                    if M < BATCH:
                        order = np.repeat(order, BATCH // M + 1)
                        np.random.shuffle(order)
                    rows, ri, rj = [], [], []
                    for _ in range(N_BATCH):
                        np.random.shuffle(order)
                        rows.append(corr[order[:BATCH]])
                        ri.append(np.random.choice(rotations, size=BATCH, replace=True))
                        rj.append(np.random.choice(rotations, size=BATCH, replace=True))
                    rows, ri, rj = np.stack(rows), np.stack(ri), np.stack(rj)      # (10,32,2), (10,32), (10,32)
                    # the feature rows of all 10 batches in one call per side
                    host0 = self._gather_to_host(feats0, ri.reshape(-1), rows[:, :, 0].reshape(-1), copy_stream)
                    host1 = self._gather_to_host(feats1, rj.reshape(-1), rows[:, :, 1].reshape(-1), copy_stream)
                    done = None
                    if copy_stream is not None:
                        done = torch.cuda.Event()
                        done.record(copy_stream)
                    items = []
                    for b in range(N_BATCH):
                        items.append((f'{item_dir}/{len(listed)}.pth', {
                            'keys0': torch.from_numpy(kps0[rows[b, :, 0]].astype(np.float32)),
                            'keys1': torch.from_numpy(kps1[rows[b, :, 1]].astype(np.float32)),
                            'R': torch.from_numpy(R[ri[b], rj[b]].astype(np.float32)),
                            'true_idx': torch.from_numpy(true_idx[ri[b], rj[b]].astype(int)),
                            'deltaR': torch.from_numpy(deltaR[ri[b], rj[b]].astype(np.float32))}))
                        listed.append((dataset.name, pc0, pc1, b))

                    def write(items=items, host0=host0, host1=host1):
                        for b, (fn, item) in enumerate(items):
                            item = dict(feats0=host0[b * BATCH:(b + 1) * BATCH].clone(),       # rows of pc0's block, of pc1's block
                                        feats1=host1[b * BATCH:(b + 1) * BATCH].clone(), **item)
                            torch.save(item, fn, _use_new_zipfile_serialization=False)
                    writer.put(done, write)
                # as the reference: the lists are rewritten after every training scene
                save_pickle(list(range(len(listed))), f'{self.output_dir}/Train_val_list/train.pkl')
                save_pickle(list(listed), f'{self.output_dir}/Train_val_list/train_pcp.pkl')
        finally:
            writer.close()

    def valset(self):
        """:252-297.  One item per correspondence of the validation scenes' pairs (the first 5000 of a shuffle), each with a random
        rotation of either fragment; val_pcp.pkl, once written, fixes them."""
        item_dir = f'{self.output_dir}/Train_val_list/valset'
        make_non_exists_dir(item_dir)
        list_fn = f'{self.output_dir}/Train_val_list/val_pcp.pkl'
        if os.path.exists(list_fn):
            chosen = read_pickle(list_fn)
        else:
            chosen = []
            for scene in self.valscenes:
                dataset = self.datasets[scene]
                for pc0, pc1 in dataset.pair_ids:
                    corr = np.load(self._pairs_file(dataset, pc0, pc1))
                    # the rotations of correspondence k are draws 2k and 2k + 1 of the stream (two choice(size=1) per k in the reference)
                    draws = np.random.choice(np.arange(N_ROT).astype(int), size=2 * corr.shape[0], replace=True)
                    chosen += [(dataset.name, pc0, pc1, draws[2 * k], draws[2 * k + 1], corr[k, 0], corr[k, 1]) for k in range(corr.shape[0])]
            random.shuffle(chosen)
            chosen = chosen[:N_VAL]
            save_pickle(list(range(len(chosen))), f'{self.output_dir}/Train_val_list/val.pkl')
            save_pickle(chosen, list_fn)

        copy_stream = torch.cuda.Stream() if torch.cuda.is_available() else None
        groups = {}                                                 # the missing items of one fragment pair share two gathers
        for i, (name, pc0, pc1, ri, rj, row0, row1) in enumerate(chosen):
            if not os.path.exists(f'{item_dir}/{i}.pth'):
                groups.setdefault((name, pc0, pc1), []).append((i, int(ri), int(rj), int(row0), int(row1)))
        if not groups:
            return
        writer = _Writer("trainset-val-writer", depth=4)
        try:
            for (name, pc0, pc1), members in groups.items():
                Rs0, feats0 = self._block(name, pc0)
                Rs1, feats1 = self._block(name, pc1)
                dataset = self.datasets[name.rsplit('/', 1)[-1]]      # the dict is keyed by the scene, a dataset's name is 'set/scene'
                kps0, kps1 = dataset.get_kps(pc0), dataset.get_kps(pc1)
                ids, ri, rj, row0, row1 = (np.array(c) for c in zip(*members))
                R = np.stack([Rs1[j] @ Rs0[i].T for i, j in zip(ri, rj)])      # the quirk: no ground truth in it
                true_idx = self.R2DR_ids(R)
                host0 = self._gather_to_host(feats0, ri, row0, copy_stream)
                host1 = self._gather_to_host(feats1, rj, row1, copy_stream)
                done = None
                if copy_stream is not None:
                    done = torch.cuda.Event()
                    done.record(copy_stream)
                items = [(f'{item_dir}/{ids[n]}.pth', {
                    'keys0': kps0[row0[n]],                          # the quirk: numpy f64 rows
                    'keys1': kps1[row1[n]],
                    'R': torch.from_numpy(R[n].astype(np.float32)),
                    'true_idx': torch.from_numpy(np.array([true_idx[n]]))}) for n in range(len(members))]

                def write(items=items, host0=host0, host1=host1):
                    for n, (fn, item) in enumerate(items):
                        item = dict(feats0=host0[n].clone(), feats1=host1[n].clone(), **item)      # (32,60) each
                        torch.save(item, fn, _use_new_zipfile_serialization=False)
                writer.put(done, write)
        finally:
            writer.close()

    def run(self):
        """the reference's __main__ (:319-323)"""
        self.PCA_keys_sample()
        self.PC_random_rot_feat()
        self.trainset()
        self.valset()


if __name__ == "__main__":
    import argparse
    parser = argparse.ArgumentParser()
    parser.add_argument('-m', '--model', default='./model/Backbone/best_val_checkpoint.pth', type=str, help='FCGF checkpoint')
    parser.add_argument('--datasetname', default='3dmatch_train', type=str, help='trainset name')
    parser.add_argument('--voxel_size', default=0.025, type=float, help='voxel size to preprocess point cloud')
    parser.add_argument('--output_dir', default='./data/YOHO_FCGF', type=str)
    parser.add_argument('--origin_dir', default='./data/origin_data', type=str)
    parser.add_argument('--rot_seed', default=None, type=int, help='make the random rotations reproducible (unseeded as the reference by default)')
    trainset_create(parser.parse_args()).run()
