"""Spread keypoints: exact farthest-point sampling on the device (include/yoho_keypoints.h).

The reference draws its 5000 keypoints uniformly over the scan points (simple_yoho/yoho_extract.py, utils/dataset.py get_kps), or reads
`Keypoints/*.txt` that another tool prepared.  A uniform draw follows the scan's density; farthest-point sampling covers the surface:

    kidx, dist2 = keypoints.select(ctx, pc_d, 5000, voxel=0.025)      # cloud indices in pick order, on the device
    keypoints.write_keypoints(dataset)                                # Keypoints/*.txt + Keypoints_PC/*.npy for an own dataset
    yoho_extractor(..., keypoints="fps")                              # the one-cloud API with spread keypoints
    keypoints.select(ctx, pc_d, 5000, voxel=0.025, clean={})          # strays filtered out of the candidates first (yoho_amd.clean)

Every pick is a prefix of every longer selection from the same start, so nkpts only cuts the list.  Nothing here draws from a random
generator.

Farthest-point sampling is a chain of nkpts dependent picks.  Exact Poisson-disk thinning (include/yoho_disk.h) gives the
same kind of coverage in about a dozen parallel rounds; the count then follows from a radius instead of being asked for:

    kidx, info = keypoints.select_disk(ctx, pc_d, 0.074, voxel=0.025) # no two closer than 0.074, every candidate within 0.074 of one
    r, rows, info = keypoints.disk_radius(ctx, pts, 5000, r0=0.1)     # once per dataset: the radius that keeps about 5000
    yoho_extractor(..., keypoints="disk", keypoint_radius=0.074)
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


def disk_key(i, seed=0):
    """the priority of include/yoho_disk.h: mix32(uint32(i) ^ seed) of an integer tensor -> int64 in [0, 2^32)"""
    m = 0xFFFFFFFF
    x = (i.to(torch.int64) ^ (int(seed) & m)) & m
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & m
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & m
    return x ^ (x >> 16)


def _thin(ctx, pts, radius, seed, what):
    """Context.disk_sample over pts to the end -> (rows kept, in ascending key order; info).  One call and one host read of its
    counts; while rows are undecided, resumed calls - every round decides at least the undecided row of lowest key, so
    ceil(N / rounds) + 1 calls always suffice and one more is an error, not another turn of a loop."""
    N = pts.shape[0]
    if N == 0:
        raise ValueError(f"{what}: no candidates")
    state, n = ctx.disk_sample(pts, radius, seed=seed)
    kept, ran, open_ = (int(v) for v in n.tolist())
    if ran < 1 and open_ > 0:
        raise RuntimeError(f"{what}: {open_} rows undecided after a call that ran no round")
    calls, rounds = 1, ran
    bound = -(-N // max(ran, 1)) + 1                       # an unfinished call ran all of its rounds: `ran` is the rounds per call
    while open_ > 0:
        if calls >= bound:
            raise RuntimeError(f"{what}: {open_} of {N} rows still undecided after {calls} calls of {ran} rounds")
        state, n = ctx.disk_sample(pts, radius, seed=seed, state=state)
        kept, r, open_ = (int(v) for v in n.tolist())
        calls, rounds = calls + 1, rounds + r
    # the kept rows in key order without another host read (torch.nonzero would be one): the others sort behind every key, and the
    # keys are distinct, so any sort gives the one order
    key = torch.where(state == 1, disk_key(torch.arange(N, device=state.device), seed), torch.full((), 1 << 32, dtype=torch.int64, device=state.device))
    rows = torch.argsort(key)[:kept]
    return rows, {"radius": float(radius), "kept": kept, "rounds": rounds, "calls": calls, "capped": False}


def select_disk(ctx, pc_d, radius, nkpts=None, voxel=None, seed=0, clean=None):
    """Spread keypoints of pc_d (n,3) f64 on the device in one pass -> (kidx int64 cloud indices, info): exact Poisson-disk thinning
    (Context.disk_sample) over candidates(ctx, pc_d, voxel), through clean_candidates when `clean` is a dict (select's).
    No two keypoints are closer than radius and every candidate has a keypoint within radius of it: the coverage farthest-point
    sampling gives at the same count to within a few per cent, without its chain of dependent picks.  The number of keypoints
    follows from the radius (about radius^-2 on a surface; disk_radius calibrates it).  kidx is in ascending order of the priority
    key(row) = mix32(row ^ seed) of the candidate rows.  nkpts: a cap - with fewer kept rows it changes nothing; with more, the first
    nkpts in that order are returned, info["capped"] is True and the coverage bound NO LONGER HOLDS (the rows cut off leave holes of
    up to 2 radius).  info: radius, kept (before the cap), rounds, calls, capped.  One host read per call of the entry: one on a
    scan with the default rounds."""
    sel, pts = candidates(ctx, pc_d, voxel)
    if clean is not None:
        sel, pts = clean_candidates(ctx, sel, pts, voxel, clean)
    rows, info = _thin(ctx, pts, radius, seed, "select_disk")
    if nkpts is not None and int(nkpts) < rows.shape[0]:
        rows = rows[:max(0, int(nkpts))]
        info["capped"] = True
    return sel[rows], info


def disk_radius(ctx, pts, nkpts, r0, steps=6, seed=0):
    """A radius at which thinning pts (m,3) f32 on the device keeps close to, and not more than, nkpts rows -> (radius, rows, info) of
    the tested radius with the largest count <= nkpts (rows: the kept rows of pts in key order; (None, None, None) when every
    tested radius kept more).  The count goes about as radius^-2, so from the probe r0 the radius is updated as
    r <- r * sqrt(count / nkpts), at most `steps` times, stopping on an exact hit or a radius that repeats.  Every step is a full
    thinning with its host read: this calibrates a radius for a dataset (one representative cloud, a few calls), it is not a
    per-fragment step - fragments are then thinned at the radius it found."""
    nkpts = int(nkpts)
    if nkpts < 1 or not float(r0) > 0:
        raise ValueError(f"disk_radius: nkpts={nkpts!r} must be >= 1 and r0={r0!r} > 0")
    best, tried, r = (None, None, None), set(), float(np.float32(r0))
    for _ in range(max(1, int(steps))):
        if r in tried:
            break
        tried.add(r)
        rows, info = _thin(ctx, pts, r, seed, "disk_radius")
        if info["kept"] <= nkpts and (best[0] is None or info["kept"] > best[2]["kept"]):
            best = (r, rows, info)
        if info["kept"] == nkpts:
            break
        r = float(np.float32(r * np.sqrt(info["kept"] / nkpts)))
    return best


def coverage_radius(ctx, pts_f32, keys_f32):
    """the largest distance from a point of pts (n,3) f32 to its nearest key (k,3) f32, device tensors -> float: the radius the keys
    leave uncovered, the figure a keypoint selection is judged by (one host read)"""
    d2, _ = ctx.nn_search(pts_f32.contiguous(), keys_f32.contiguous(), want_dist=True, squared=True)
    return float(np.sqrt(np.float64(d2.max().item())))


def _select_host(ctx, pc, nkpts, voxel, clean=None):
    pc_d = torch.from_numpy(np.ascontiguousarray(np.asarray(pc, dtype=np.float64))).cuda()
    return select(ctx, pc_d, nkpts, voxel=voxel, clean=clean)[0].cpu().numpy()


def _select_disk_host(ctx, pc, nkpts, voxel, radius, seed, clean=None):
    pc_d = torch.from_numpy(np.ascontiguousarray(np.asarray(pc, dtype=np.float64))).cuda()
    return select_disk(ctx, pc_d, radius, nkpts=nkpts, voxel=voxel, seed=seed, clean=clean)[0].cpu().numpy()


METHODS = ("fps", "disk")


def write_keypoints(dataset, nkpts=5000, voxel=0.025, ctx=None, overwrite=False, selector=None, clean=None, method="fps", radius=None, seed=0):
    """Spread keypoints for every cloud of an EvalDataset that has no `Keypoints/cloud_bin_{k}Keypoints.txt` yet (overwrite=True: for
    every cloud): the index file, np.savetxt of the cloud indices in pick order, and `Keypoints_PC/cloud_bin_{k}Keypoints.npy`,
    pc[indices] - the two files ThrDMatchPartDataset.get_kps reads, in its formats, so that it never reaches its random draw.  A cloud
    whose index file exists is left alone.  selector(pc, nkpts, voxel) -> indices replaces the device selection (tests).
    clean: select's; a selector is then called as selector(pc, nkpts, voxel, clean=clean).
    method: "fps" (select), or "disk" - select_disk at `radius` (required then, refused otherwise) with priority seed `seed`, nkpts
    its cap, the indices in key order; it replaces the default selector only, a selector passed in is called as before.
    -> the ids of the clouds written."""
    if method not in METHODS:
        raise ValueError(f"write_keypoints: method must be one of {METHODS}, got {method!r}")
    if (method == "disk") != (radius is not None):
        raise ValueError(f"write_keypoints: method=\"disk\" needs a radius, and only it takes one (method={method!r}, radius={radius!r})")
    if selector is None:
        ctx = hip.get_context() if ctx is None else ctx
        if method == "disk":
            selector = lambda pc, n, v, clean=None: _select_disk_host(ctx, pc, n, v, radius, seed, clean)      # noqa: E731
        else:
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
