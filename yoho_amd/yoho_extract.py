"""Drop-in for simple_yoho/yoho_extract.py: one-cloud API  pc -> (kpts, inv, eqv).

    extractor = yoho_extractor(fcgf_ckpt, yoho_ckpt, fcgf=my_backbone)
    kpts, feat_inv, feat_eqv = extractor.run(pc, voxel_size=0.025, nkpts=5000)

The FCGF sparse-conv backbone (simple_yoho/fcgf_feat.py on MinkowskiEngine) is ``yoho_amd.fcgf_feat.fcgf_extractor``
(csrc/sparse.hip, csrc/spmaps.hip, csrc/spconv.hip), built from ``fcgf_ckpt`` as the reference does (:20); any object with ``run(pc, voxel_size) ->
(ds_points (n,3), unit-norm feats (n,32))`` can be passed as ``fcgf`` instead.  The 60-fold NN feature transfer and
the PartI group conv run on the HIP library too.

Differences from the reference (all deliberate):
  * no argparse at import time (simple_yoho/yoho_extract.py:11-13 breaks under pytest / other argv);
  * the NN result is unpacked as (dists, inds) - the reference names them the other way round
    (:37) and would index the features with distances;
  * any number of keypoints works (no "avoid B == 1" last-batch merge needed, :55-58).
"""
import os
import threading

import numpy as np
import torch

from . import hip
from . import keypoints as KP
from . import weights as W
from .fcgf_feat import fcgf_extractor
from .utils import transform_points


# Page-locked result tensors are handed out only while the pinned bytes still ALIVE in the caller's hands stay under this budget
# (YOHO_PIN_OUTPUT_BYTES, default 2 GiB; 0 = always pageable, as the reference returns them).  A caller that streams fragments
# (describe, consume, drop) keeps the fast copy; one that keeps the descriptors of a whole scene or test set - 38 MB per fragment,
# the testset and cache writers do - gets ordinary pageable tensors once the budget is used up instead of pinning GBs of host RAM
# that torch's caching host allocator never gives back to the OS.
PIN_OUTPUT_BYTES = int(os.environ.get("YOHO_PIN_OUTPUT_BYTES", str(2 << 30)))
_pinned_alive = [0]
_pinned_lock = threading.Lock()


def _unpin(nbytes):
    with _pinned_lock:
        _pinned_alive[0] -= nbytes


def _to_host(*tensors):
    """device tensors -> CPU tensors, as the reference API returns them (simple_yoho/yoho_extract.py:72-77), through page-locked memory
    while the budget above allows: a pageable 38 MB copy of the descriptors took 2.5 ms of a 48 ms fragment, the same copy into a pinned
    tensor 0.8 ms.  The pinned blocks come from torch's caching host allocator (no hipHostMalloc per call after the first); every call
    gets tensors of its own."""
    import weakref
    need = sum(t.numel() * t.element_size() for t in tensors)
    with _pinned_lock:                                 # reserve the whole call's bytes or none (several extractor threads share the budget)
        pin = need > 0 and _pinned_alive[0] + need <= PIN_OUTPUT_BYTES
        if pin:
            _pinned_alive[0] += need
    outs = [torch.empty(t.shape, dtype=t.dtype, pin_memory=pin) for t in tensors]
    for o, t in zip(outs, tensors):
        o.copy_(t, non_blocking=pin)
        if pin:
            # released when the page-locked STORAGE dies, not the tensor object: out.numpy(), a view or a slice keep the storage (and
            # the pinned pages) alive after the tensor the caller was handed is gone
            weakref.finalize(o.untyped_storage(), _unpin, o.numel() * o.element_size())
    torch.cuda.current_stream().synchronize()
    return tuple(outs)


KEYPOINT_MODES = ("random", "fps", "disk")


class yoho_extractor():
    def __init__(self, fcgf_ckpt='model/Backbone/best_val_checkpoint.pth', yoho_ckpt='model/PartI_train/model_best.pth',
                 fcgf=None, so3_dir=None, keypoints="random", keypoint_voxel=None, keypoint_clean=None, keypoint_radius=None, keypoint_seed=0, keypoint_saliency=None):
        """keypoints: "random" - the reference's np.random.permutation(len(pc))[0:nkpts] on numpy's global generator -, or "fps" -
        farthest-point sampling on the device (yoho_amd.keypoints.select) over the first point of every voxel of
        keypoint_voxel (None: the voxel_size of the call), from candidate 0: no draw from any generator, keypoints in pick order, a
        smaller nkpts a prefix of a larger one.  keypoint_clean ("fps" only): a dict of yoho_amd.clean.statistical's keyword arguments -
        the candidates that filter drops are never picked (yoho_amd.keypoints.select's `clean`); None: no filter.
        "disk": exact Poisson-disk thinning of the same candidates at keypoint_radius (required, and refused in the other modes) with
        priority seed keypoint_seed (yoho_amd.keypoints.select_disk): no two keypoints closer than the radius, every
        candidate within the radius of one, in about a dozen parallel rounds instead of nkpts dependent picks; the number of
        keypoints follows from the radius (keypoints.disk_radius calibrates it for a dataset) and nkpts only caps it;
        keypoint_clean is accepted as in "fps".  keypoint_saliency ("disk" only, refused in the other modes): a dict of
        yoho_amd.keypoints.select_salient's keyword arguments ({}: its defaults) - the thinning runs in the order of the ISS saliency
        instead of the hash, distinctive points first; None: select_disk, as before."""
        if keypoints not in KEYPOINT_MODES:
            raise ValueError(f"yoho_extractor: keypoints must be one of {KEYPOINT_MODES}, got {keypoints!r}")
        if keypoint_clean is not None and keypoints not in ("fps", "disk"):
            raise ValueError(f"yoho_extractor: keypoint_clean filters the candidates of keypoints=\"fps\" and \"disk\"; keypoints={keypoints!r} draws from the whole cloud")
        if keypoints == "disk" and not (keypoint_radius is not None and float(keypoint_radius) > 0 and np.isfinite(float(keypoint_radius))):
            raise ValueError(f"yoho_extractor: keypoints=\"disk\" needs a finite keypoint_radius > 0, got {keypoint_radius!r}")
        if keypoints != "disk" and keypoint_radius is not None:
            raise ValueError(f"yoho_extractor: keypoint_radius is the radius of keypoints=\"disk\"; keypoints={keypoints!r} takes none")
        keypoint_saliency = KP.check_saliency("yoho_extractor", "keypoint_saliency", keypoint_saliency)
        if keypoint_saliency is not None and keypoints != "disk":
            raise ValueError(f"yoho_extractor: keypoint_saliency orders the thinning of keypoints=\"disk\"; keypoints={keypoints!r} takes none")
        self.keypoint_saliency = keypoint_saliency
        self.keypoints = keypoints
        self.keypoint_radius = None if keypoint_radius is None else float(keypoint_radius)
        self.keypoint_seed = int(keypoint_seed)
        self.keypoint_clean = None if keypoint_clean is None else dict(keypoint_clean)
        self.keypoint_voxel = keypoint_voxel
        self.ctx = hip.get_context(so3_dir=so3_dir)
        self.grs = self.ctx.tables.R64
        self.fcgf_ckpt = fcgf_ckpt
        if fcgf is None and fcgf_ckpt is not None:
            fcgf = fcgf_extractor(fcgf_ckpt, ctx=self.ctx)
        self.fcgf = fcgf
        self.yoho_ckpt = yoho_ckpt
        self._load_model()
        self.bs = 500
        # rotated copies of the cloud per backbone pass (split further by voxel count): one number, or a list
        # "9,17,17,17" (the first pass's voxelisation and maps are the only ones nothing hides - a smaller first pass exposes less)
        rb = [int(v) for v in os.environ.get("YOHO_ROT_BATCH", "15").split(",")]
        self.rot_batch = rb[0] if len(rb) == 1 else rb
        self.overlap_keypoint_draw = os.environ.get("YOHO_OVERLAP_DRAW", "1") != "0"   # keypoint permutation drawn while the first backbone pass runs
        # backbone passes alternate between two lanes (fcgf_extractor.lanes: stream + library context = workspace): a pass's
        # voxelisation, coordinate and kernel maps - atomics and scans with host round trips for the level sizes - are queued while
        # the previous pass's convolutions still run on the other lane (YOHO_FCGF_LANES=1: one lane, as up to round 5)
        self.lanes = max(1, min(2, int(os.environ.get("YOHO_FCGF_LANES", "2"))))
        self._tail = None                          # run_many's (lanes it was picked beside, library context, stream)
        self._side_stream = None
        if self.lanes > 1 and hasattr(self.fcgf, "lane_context"):
            self.fcgf.lane_context()               # the second lane's weights are resident from here on, like the first one's

    def _load_model(self):
        sd = self.yoho_ckpt if isinstance(self.yoho_ckpt, dict) else W.load_checkpoint(self.yoho_ckpt)[0]
        self._sd = W.to_numpy_state_dict(sd)
        W.check_state_dict(self._sd, W.PARTI_SPEC, strict=False)
        self.ctx.load_partI(self._sd, owner=self)

    def _partI(self, kpts_f):
        if self.ctx.partI_owner is not self:          # another network object loaded its checkpoint into the shared context
            self.ctx.load_partI(self._sd, owner=self)
        return self.ctx.partI_forward(kpts_f.contiguous(), want_inv=True)

    def _feature_transfer_xyz(self, query, source, source_f):
        """NN in xyz (fp32, 'SquareL2') and feature row transfer (simple_yoho/yoho_extract.py:33-39)."""
        q = torch.from_numpy(np.asarray(query).astype(np.float32)).cuda().contiguous()
        s = (source if isinstance(source, torch.Tensor) else torch.from_numpy(np.asarray(source))).to(device="cuda", dtype=torch.float32).contiguous()
        f = (source_f if isinstance(source_f, torch.Tensor) else torch.from_numpy(np.asarray(source_f))).to(device="cuda", dtype=torch.float32)
        dist, idx = self.ctx.nn_search(q, s, want_dist=False, squared=True)
        return f[idx]

    def _select(self, ctx, pc_d, voxel_size, nkpts):
        """the device selection of keypoints="fps" / "disk" on the current stream -> cloud indices (k) int64 on the device"""
        voxel = voxel_size if self.keypoint_voxel is None else self.keypoint_voxel
        if self.keypoints == "disk" and self.keypoint_saliency is not None:
            return KP.select_salient(ctx, pc_d, self.keypoint_radius, nkpts=nkpts, voxel=voxel, seed=self.keypoint_seed, clean=self.keypoint_clean,
                                     **self.keypoint_saliency)[0]
        if self.keypoints == "disk":
            return KP.select_disk(ctx, pc_d, self.keypoint_radius, nkpts=nkpts, voxel=voxel, seed=self.keypoint_seed, clean=self.keypoint_clean)[0]
        return KP.select(ctx, pc_d, nkpts, voxel=voxel, clean=self.keypoint_clean)[0]

    def _pass_starts(self, G):
        """first group element of every backbone pass, and G"""
        rb = self.rot_batch
        sizes = list(rb) if isinstance(rb, (list, tuple)) else [int(rb)] * ((G + int(rb) - 1) // int(rb))
        starts = [0]
        for n in sizes:
            if starts[-1] >= G:
                break
            starts.append(min(G, starts[-1] + max(1, int(n))))
        while starts[-1] < G:                      # a list that does not cover the group: its last size repeats
            starts.append(min(G, starts[-1] + max(1, int(sizes[-1]))))
        return starts

    def _queue_passes(self, pc, voxel_size, nkpts):
        """Queue a fragment's backbone passes and NN feature transfers on the lanes (fcgf_extractor.rotated_passes); returns without
        joining them: dict(kpts, kpts_f (K,32,60) cuda - complete once `done` has run -, done = one event per lane, keep = tensors
        that must outlive `done`, main = lane 0's stream).  The keypoint draw sits off the critical path: the reference's
        np.random.permutation(len(pc))[0:nkpts] on the global generator costs 5 ms of host time for 300 k points, and nothing on the
        device depends on it until the first NN transfer - it is taken after one backbone pass per lane has been queued
        (YOHO_OVERLAP_DRAW=0: before the first pass).  It is the only draw in this method, so the generator is consumed exactly as
        in the reference (same keypoints for the same seed).
        keypoints="fps" / "disk": the selection is queued on lane 0 BEFORE the first pass (draw_ahead off): its one host read, the voxel count,
        then waits for the upload alone and never for a backbone pass, and its k launches are in front of everything that needs
        them.  The indices stay on the device (kpts = None, kidx_d): _results reads them back with the descriptors."""
        fps = self.keypoints in ("fps", "disk")    # a selection on the device
        lanes = self.fcgf.lanes(self.lanes)

        def prepare(pc_d):                         # on lane 0's stream
            if fps:
                kidx_d = self._select(lanes[0][0], pc_d, voxel_size, nkpts)
                kpts = None
            else:
                kpts_index = np.random.permutation(len(pc))[0:nkpts]
                kidx_d = torch.from_numpy(kpts_index.astype(np.int64)).cuda()
                kpts = pc[kpts_index]
            kpts_f = torch.empty((kidx_d.shape[0], 32, 60), dtype=torch.float32, device="cuda")

            def transfer(ctx, res, g0, Rs):        # kpts_f[:, :, g0 + j] = F_j[nn(R_j keypoints, down-sampled points of copy j)]
                ctx.group_transfer_batch(pc_d, kidx_d, list(Rs), [ds for _, _, ds in res], [f.contiguous() for _, f, _ in res], g0, kpts_f)
            return transfer, {"kpts": kpts, "pc": pc, "kidx_d": kidx_d, "kpts_f": kpts_f, "keep": (pc_d, kidx_d)}

        starts = self._pass_starts(self.grs.shape[0])
        passes = [(i0, [self.grs[i] for i in range(i0, i1)]) for i0, i1 in zip(starts[:-1], starts[1:])]
        self._side_stream = lanes[1][1] if len(lanes) > 1 else None       # the second lane's stream of the last call, for inspection
        done, q = self.fcgf.rotated_passes(pc, passes, voxel_size, lanes, prepare, draw_ahead=self.overlap_keypoint_draw and not fps)
        return dict(q, done=done, main=lanes[0][1])

    @staticmethod
    def _results(q, out):
        """(kpts, inv, eqv) of a queued fragment on the current stream, which has waited for q["done"]: the device selection's indices
        come to the host in the same copy as the descriptors"""
        if q["kpts"] is not None:
            return (q["kpts"],) + _to_host(out["inv"], out["eqv"])
        inv, eqv, kidx = _to_host(out["inv"], out["eqv"], q["kidx_d"])
        return (q["pc"][kidx.numpy()], inv, eqv)

    def _extract_features_overlapped(self, pc, voxel_size, nkpts):
        q = self._queue_passes(pc, voxel_size, nkpts)
        cur, main = torch.cuda.current_stream(), q["main"]
        with torch.cuda.stream(main):
            for e in q["done"]:
                main.wait_event(e)                 # PartI reads every column of kpts_f
            self._last_group_feats = q["kpts_f"]   # (n,32,60) group features, kept for inspection
            out = self._partI(q["kpts_f"])
            res = self._results(q, out)            # (waits for lane 0)
        if main is not cur:
            cur.wait_stream(main)                  # what the caller queues next sees a finished call, as on one stream
        return res

    def run_many(self, pcs, voxel_size=0.025, nkpts=5000):
        """run() over an iterable of clouds, streamed: yields (kpts, feat_inv, feat_eqv) per cloud, in order, the same values
        run() returns for the same clouds and generator state.  The descriptor pass and the result copy of fragment f run on a tail
        lane (its own stream and library context, driven by a helper thread) while the backbone lanes already work on fragment f + 1,
        so that what a single run() call leaves exposed - the first pass's voxelisation and maps, PartI, the copy of 38 MB of results -
        is hidden behind convolutions (`bench.py` fcgf leg: ms_per_fragment_streamed).  Fragment f is yielded once f + 1 has been
        queued, and f + 1 is handed to the tail only when the caller asks for the next result, after f + 2 has been queued: at most
        three fragments are in flight, each with its cloud (N,3) f64 and group features (K,32,60) f32 on the device - 7 + 38 MB at
        300 k points and 5000 keypoints - and the one on the tail with its PartI output (another 38 MB) and pinned result copy."""
        if not hasattr(self.fcgf, "rotated_passes") or self.lanes < 2:
            for pc in pcs:
                yield self.run(pc, voxel_size=voxel_size, nkpts=nkpts)
            return
        lanes = self.fcgf.lanes(self.lanes)
        if self._tail is None or self._tail[0] is not lanes:
            self._tail = (lanes, hip.get_context(self.ctx.device, self.ctx.tables.dir, lane=2),
                          self.fcgf.stream_beside_lanes(self.lanes, [torch.cuda.current_stream()]))
        _, tctx, tst = self._tail

        def finish(q):                             # on the helper thread
            with torch.cuda.stream(tst):
                for e in q["done"]:
                    tst.wait_event(e)
                if tctx.partI_owner is not self:
                    tctx.load_partI(self._sd, owner=self)
                out = tctx.partI_forward(q["kpts_f"], want_inv=True)        # (its range check waits for the tail stream only)
                return self._results(q, out)       # (waits for the tail stream: the fragment is complete)

        queued = []                                # fragments queued on the lanes and not yet yielded, oldest first

        def take(fut):                             # the result of the oldest fragment (on this, the yielding, thread)
            res = fut.result()
            self._last_group_feats = queued.pop(0)["kpts_f"]
            return res

        # finish(f) - PartI, its range check, the result copy: mostly waiting for the device - runs on a helper thread while this
        # one queues the passes of f + 1 (the keypoint draws stay on this thread, in order)
        from concurrent.futures import ThreadPoolExecutor
        pool = ThreadPoolExecutor(max_workers=1)
        try:
            fut = None
            for pc in pcs:
                queued.append(self._queue_passes(pc, voxel_size, nkpts))
                if fut is not None:
                    yield take(fut)
                fut = pool.submit(finish, queued[-2]) if len(queued) > 1 else None
            if fut is not None:
                yield take(fut)
            if queued:
                yield take(pool.submit(finish, queued[0]))
        finally:
            pool.shutdown(wait=True)
            for q in queued:                       # left early (an error, or the caller stopped iterating): queued lanes still use the
                for e in q["done"]:                # fragment's tensors - wait for them before this frame lets go of them (a finished
                    e.synchronize()                # fragment's events have long completed: no cost on the normal path)

    def extract_features(self, pc, voxel_size, nkpts=5000):
        if self.fcgf is None:
            raise NotImplementedError("no FCGF backbone: pass fcgf_ckpt=<FCGF checkpoint> or fcgf=<object with run(pc, voxel_size)>")
        if hasattr(self.fcgf, "rotated_passes"):
            return self._extract_features_overlapped(pc, voxel_size, nkpts)
        # a backbone with run() only: the reference's host loop
        if self.keypoints in ("fps", "disk"):
            pc_d = torch.from_numpy(np.ascontiguousarray(np.asarray(pc, dtype=np.float64))).cuda()
            kpts_index = self._select(self.ctx, pc_d, voxel_size, nkpts).cpu().numpy()
        else:
            kpts_index = np.random.permutation(len(pc))[0:nkpts]
        kpts = pc[kpts_index]
        kpts_f = torch.empty((kpts.shape[0], 32, 60), dtype=torch.float32, device="cuda")
        for i in range(self.grs.shape[0]):
            kptsi = transform_points(kpts.copy(), self.grs[i])
            pci = transform_points(pc.copy(), self.grs[i])
            pci_ds, pci_f = self.fcgf.run(pci, voxel_size)
            kpts_f[:, :, i] = self._feature_transfer_xyz(kptsi, pci_ds, pci_f)
        self._last_group_feats = kpts_f
        out = self._partI(kpts_f)
        # output: n*32; n*32*60 (cpu tensors, as the reference)
        return (kpts,) + _to_host(out["inv"], out["eqv"])

    def run(self, pc, voxel_size=0.025, nkpts=5000):
        kpts, feat_inv, feat_eqv = self.extract_features(pc, voxel_size, nkpts=nkpts)
        return kpts, feat_inv, feat_eqv
