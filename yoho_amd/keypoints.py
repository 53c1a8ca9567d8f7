"""Spread keypoints: exact farthest-point sampling on the device (include/yoho_keypoints.h).

The reference draws its 5000 keypoints uniformly over the scan points (simple_yoho/yoho_extract.py, utils/dataset.py get_kps), or reads
`Keypoints/*.txt` that another tool prepared.  A uniform draw follows the scan's density; farthest-point sampling covers the surface:

    kidx, dist2 = keypoints.select(ctx, pc_d, 5000, voxel=0.025)      # cloud indices in pick order, on the device
    keypoints.write_keypoints(dataset)                                # Keypoints/*.txt + Keypoints_PC/*.npy for an own dataset
    yoho_extractor(..., keypoints="fps")                              # the one-cloud API with spread keypoints
    keypoints.select(ctx, pc_d, 5000, voxel=0.025, clean={})          # strays filtered out of the candidates first (yoho_amd.clean)

Every pick is a prefix of every longer selection from the same start, so nkpts only cuts the list.  Nothing here draws from a random
generator.
"""
import os

import numpy as np
import torch

from . import hip
from .utils import make_non_exists_dir


def candidates(ctx, pc_d, voxel):
    """pc_d (n,3) f64 on the device -> (sel (c) int64 ascending cloud indices, pts (c,3) f32): the points the selection runs over.
    With a voxel size the first point of every voxel (fcgf_voxelize: what the backbone keeps of the cloud, one read of the count);
    voxel=None: every point."""
    if pc_d.dim() != 2 or pc_d.shape[1] != 3:
        raise ValueError("candidates: pc_d (n,3)")
    if voxel is None:
        sel = torch.arange(pc_d.shape[0], dtype=torch.int64, device=pc_d.device)
    else:
        if not float(voxel) > 0:
            raise ValueError(f"candidates: voxel={voxel!r} must be > 0 or None")
        sel = ctx.fcgf_voxelize(pc_d, float(voxel))[0].contiguous()
    return sel, ctx.rotate_select(pc_d, None, sel)


def clean_candidates(ctx, sel, pts, voxel, clean):
    """the candidates that yoho_amd.clean.statistical keeps: clean is a dict of its keyword arguments, max_dist defaulting to 4 voxels
    (it has to be given when voxel is None) -> (sel, pts) of the kept candidates, in their order.  An optional "method" key names
    another filter of yoho_amd.clean.METHODS, "cluster" (yoho_amd.cluster.keep_large: eps defaults to 4 voxels) or "radius"; the
    other keys are then that filter's arguments."""
    from . import clean as CL
    kw = dict(clean)
    method, key = CL.method_of(kw)
    kw.pop("method", None)
    if kw.get(key) is None:
        if voxel is None:
            raise ValueError(f"select: clean needs {key} when there is no voxel to take it from")
        kw[key] = 4.0 * float(voxel)
    kept = CL.METHODS[method](ctx, pts, **kw)["sel"]
    return sel[kept], pts[kept].contiguous()


def select(ctx, pc_d, nkpts, voxel=None, start=0, clean=None):
    """k = min(nkpts, candidates) spread keypoints of pc_d (n,3) f64 on the device -> (kidx (k) int64 cloud indices in pick order,
    dist2 (k) f32), device tensors: farthest-point sampling (Context.fps) over candidates(ctx, pc_d, voxel), from candidate `start`.
    clean: None, or a dict of yoho_amd.clean.statistical's keyword arguments ({}: its defaults) - farthest-point sampling seeks out
    whatever lies far from everything, a stray first of all, so the candidates go through the outlier filter before the selection
    (one more host read); `start` then counts the kept candidates.  {"method": "cluster", "min_size": 100} filters by cluster size
    instead (clean_candidates): strays that come in clumps pass the statistical filter."""
    sel, pts = candidates(ctx, pc_d, voxel)
    if clean is not None:
        sel, pts = clean_candidates(ctx, sel, pts, voxel, clean)
    k = max(0, min(int(nkpts), sel.shape[0]))
    idx, dist2 = ctx.fps(pts, k, start=start)
    return sel[idx], dist2


def coverage_radius(ctx, pts_f32, keys_f32):
    """the largest distance from a point of pts (n,3) f32 to its nearest key (k,3) f32, device tensors -> float: the radius the keys
    leave uncovered, the figure a keypoint selection is judged by (one host read)"""
    d2, _ = ctx.nn_search(pts_f32.contiguous(), keys_f32.contiguous(), want_dist=True, squared=True)
    return float(np.sqrt(np.float64(d2.max().item())))


def _select_host(ctx, pc, nkpts, voxel, clean=None):
    pc_d = torch.from_numpy(np.ascontiguousarray(np.asarray(pc, dtype=np.float64))).cuda()
    return select(ctx, pc_d, nkpts, voxel=voxel, clean=clean)[0].cpu().numpy()


def write_keypoints(dataset, nkpts=5000, voxel=0.025, ctx=None, overwrite=False, selector=None, clean=None):
    """Spread keypoints for every cloud of an EvalDataset that has no `Keypoints/cloud_bin_{k}Keypoints.txt` yet (overwrite=True: for
    every cloud): the index file, np.savetxt of the cloud indices in pick order, and `Keypoints_PC/cloud_bin_{k}Keypoints.npy`,
    pc[indices] - the two files ThrDMatchPartDataset.get_kps reads, in its formats, so that it never reaches its random draw.  A cloud
    whose index file exists is left alone.  selector(pc, nkpts, voxel) -> indices replaces the device selection (tests).
    clean: select's; a selector is then called as selector(pc, nkpts, voxel, clean=clean).
    -> the ids of the clouds written."""
    if selector is None:
        ctx = hip.get_context() if ctx is None else ctx
        selector = lambda pc, n, v, clean=None: _select_host(ctx, pc, n, v, clean)      # noqa: E731
    written = []
    for cid in dataset.get_cloud_ids():
        k = int(cid)
        if os.path.exists(dataset.kps_fn[k]) and not overwrite:
            continue
        pc = dataset.get_pc(cid)
        picked = selector(pc, nkpts, voxel) if clean is None else selector(pc, nkpts, voxel, clean=clean)
        key_idxs = np.asarray(picked, dtype=np.int64).reshape(-1)
        make_non_exists_dir(os.path.dirname(dataset.kps_fn[k]))
        np.savetxt(dataset.kps_fn[k], key_idxs)
        make_non_exists_dir(os.path.dirname(dataset.kps_pc_fn[k]))
        np.save(dataset.kps_pc_fn[k], pc[key_idxs])
        written.append(cid)
    return written
