"""Drop-in for YOHO_testset.py: "PC*60 rotations -> FCGF backbone -> FCGF group feature for PC keypoints".

    testset_create(cfg).batch_feature_extraction()

writes ``{output_dir}/Testset/{dataset}/{scene}/FCGF_Input_Group_feature/{pc_id}.npy`` ((K,32,60) f32, group axis in the
order of Rotation.npy) for every fragment of every scene, exactly the files tests/extractor.py:46-49 reads.

Reference flow (YOHO_testset.py:20-166), kept step for step: rotate the fragment by R_g (f64), voxelise (first point of
every voxel, :39-49), run the backbone (:143-147), rotate the keypoints by R_g and take, for each, the feature row of its
nearest down-sampled point (:153-159, KNN(1), type-promoted f64 'L2' distance).  Here the fragment is uploaded once and
all 60 group elements run on the device (yoho_fcgf_voxelize / yoho_fcgf_forward / yoho_group_gather); there is no
DataLoader batching (the reference's batch of 4 clouds only amortises MinkowskiEngine launches).

``cfg`` needs ``model`` (FCGF checkpoint path or dict), ``voxel_size``, ``dataset``; optional ``output_dir`` /
``origin_dir`` (defaults './data/YOHO_FCGF', './data/origin_data' as the reference, :61-62) and ``datasets`` (a prebuilt
{scene: dataset} dict, otherwise ``get_dataset_name(dataset, origin_dir)``).
"""
import os
import queue
import threading

import numpy as np
import torch

from . import hip
from .dataset import get_dataset_name
from .fcgf_feat import fcgf_extractor
from .utils import make_non_exists_dir


def group_features(fcgf, Rgroup, lanes, voxel_size, pc, keys, join=True):
    """pc (N,3), keys (K,3) f64 -> (K,32,60) f32 cuda tensor (one fragment, all 60 group elements) on the backbone `fcgf` (an fcgf_extractor) with
    the group `Rgroup` (60,3,3) over `lanes` backbone lanes; shared by testset_create and YOHO_Trainset.trainset_create.  Complete on the stream `join`:
    True (the default) - the caller's current stream; a torch stream (Feature_extracting: its copy stream) - that stream, with
    the caller's stream NOT made to wait for the lanes, so that the next fragment's first pass can be queued under this
    fragment's last one."""
    def prepare(pc_d):                                           # on lane 0's stream, before the first pass
        k_d = torch.from_numpy(np.ascontiguousarray(np.asarray(keys, dtype=np.float64))).cuda()
        out = torch.empty((k_d.shape[0], 32, 60), dtype=torch.float32, device="cuda")

        def transfer(ctx, res, g0, Rs):
            # rotated copies (pc @ R_g^T, :143) are never materialised: rotation, voxelisation and 'dspcd0' (the down-sampled
            # points, .float(), :92) come out of one pass over the cloud (fcgf_extractor.extract_rotated_batch)
            for j, (sel, feat, pts) in enumerate(res):
                ctx.group_gather(k_d, pts, feat, g0 + j, out)    # keys @ R_g^T, f64 NN, feature row -> out[:, :, g]
        return transfer, (pc_d, k_d, out)

    nb = 15                                                      # rotated copies per backbone pass (split further by voxel count)
    passes = [(g0, [Rgroup[g] for g in range(g0, g0 + nb)]) for g0 in range(0, 60, nb)]
    done, (pc_d, k_d, out) = fcgf.rotated_passes(pc, passes, voxel_size, fcgf.lanes(lanes), prepare, draw_ahead=False)
    st = torch.cuda.current_stream() if join is True else join
    for e in done:
        st.wait_event(e)
    for x in (pc_d, k_d, out):                                   # released once `st` has run past the lanes' last use
        x.record_stream(st)
    return out


class testset_create():
    def __init__(self, config, ctx=None):
        self.config = config
        self.dataset_name = self.config.dataset
        self.output_dir = getattr(config, 'output_dir', './data/YOHO_FCGF')
        self.origin_dir = getattr(config, 'origin_dir', './data/origin_data')
        self.datasets = getattr(config, 'datasets', None) or get_dataset_name(self.dataset_name, self.origin_dir)
        self.ctx = ctx if ctx is not None else hip.get_context()
        self.Rgroup = self.ctx.tables.R64
        self.fcgf = fcgf_extractor(self.config.model, ctx=self.ctx)
        # backbone passes alternate over two lanes (fcgf_extractor.lanes: stream + library context = workspace), as in yoho_extractor:
        # a pass's voxelisation and maps are queued while the previous pass's convolutions run (YOHO_FCGF_LANES=1: everything on the
        # caller's stream).
        # Across fragments the host never waits for the device: the result goes to a page-locked buffer by an asynchronous copy and
        # is written by a writer thread while the next fragments run; the next fragment's files are read ahead by a loader thread.
        self.lanes = max(1, min(2, int(os.environ.get("YOHO_FCGF_LANES", "2"))))
        self.stats = {}
        if self.lanes > 1:
            self.fcgf.lane_context()                                 # the second lane's weights are resident from here on, like the first one's

    def fragment_group_features(self, pc, keys, join=True):
        """pc (N,3), keys (K,3) f64 -> (K,32,60) f32 cuda tensor (one fragment, all 60 group elements): group_features on this object's
        backbone, tables, lanes and voxel size"""
        return group_features(self.fcgf, self.Rgroup, self.lanes, self.config.voxel_size, pc, keys, join)

    def Feature_extracting(self):
        import time
        jobs = []
        for scene, dataset in self.datasets.items():
            if scene == 'wholesetname':
                continue
            save_dir = f'{self.output_dir}/Testset/{self.dataset_name}/{scene}/FCGF_Input_Group_feature'
            make_non_exists_dir(save_dir)
            jobs += [(dataset, pc_id, f'{save_dir}/{pc_id}.npy') for pc_id in dataset.pc_ids]
        t_start = time.perf_counter()
        depth = 2                                                    # fragments read ahead / results waiting for the writer
        loaded = queue.Queue(maxsize=depth)
        towrite = queue.Queue(maxsize=depth)
        errors = []
        stop = threading.Event()                                     # set when the main loop ends: the loader reads no further fragment

        def loader():
            try:
                for dataset, pc_id, fn in jobs:
                    if stop.is_set():
                        break
                    loaded.put((dataset.get_pc(pc_id), dataset.get_kps(pc_id), fn))
            except BaseException as e:                               # handed to the main thread
                errors.append(e)
            loaded.put(None)

        def writer():
            while True:
                item = towrite.get()
                if item is None:
                    return
                host, done, fn = item
                try:
                    done.synchronize()
                    np.save(fn, host.numpy())
                except BaseException as e:
                    errors.append(e)

        tl = threading.Thread(target=loader, name="testset-loader", daemon=True)
        tw = threading.Thread(target=writer, name="testset-writer", daemon=True)
        tl.start(); tw.start()
        copy_stream = self.fcgf.stream_beside_lanes(self.lanes)
        n = 0
        ended = False                                                # the loader's sentinel has been taken
        try:
            while True:
                item = loaded.get()
                ended = item is None
                if ended or errors:
                    break
                pc, kps, fn = item
                out = self.fragment_group_features(pc, kps, join=copy_stream)
                host = torch.empty(out.shape, dtype=out.dtype, pin_memory=True)
                with torch.cuda.stream(copy_stream):
                    host.copy_(out, non_blocking=True)
                    done = torch.cuda.Event()
                    done.record(copy_stream)
                del out
                towrite.put((host, done, fn))                        # blocks while `depth` results are still waiting: bounds the pinned bytes
                n += 1
        finally:
            stop.set()
            towrite.put(None)
            tw.join()
            if not ended:                                            # stopped early: let the loader run out of its bounded queue
                while loaded.get() is not None:
                    pass
            tl.join()
        torch.cuda.synchronize()
        if errors:
            raise errors[0]
        self.stats = {"fragments": n, "seconds": time.perf_counter() - t_start, "lanes": self.lanes}

    def batch_feature_extraction(self):
        self.Feature_extracting()
