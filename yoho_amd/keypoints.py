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

Evenly spread keypoints of an indoor scan lie mostly on walls and floors, where a descriptor says "a plane".  select_salient thins in
the order of the ISS saliency (include/yoho_salient.h) instead of a hash: non-maximum suppression that goes on to fill
the gaps:

    kidx, info = keypoints.select_salient(ctx, pc_d, 0.074, voxel=0.025)   # distinctive points first, the rest as select_disk
    yoho_extractor(..., keypoints="disk", keypoint_radius=0.074, keypoint_saliency={})
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


def prio_ord(prio):
    """ord of include/yoho_salient.h on an f32 tensor -> int64 in [0, 2^32): the bits, all flipped under a set sign bit, the sign bit
    set otherwise; every NaN 0"""
    m = 0xFFFFFFFF
    b = prio.contiguous().view(torch.int32).to(torch.int64) & m
    o = torch.where((b >> 31) != 0, ~b & m, b | 0x80000000)
    return torch.where(torch.isnan(prio), torch.zeros_like(o), o)


def prio_key(prio, seed=0):
    """key64 of include/yoho_salient.h of rows 0 .. N-1 with priorities prio (N) f32 -> (N) int64 holding key64 - 2^63: the order of
    the signed values is the order of the keys"""
    hi = ~prio_ord(prio) & 0xFFFFFFFF
    return ((hi - (1 << 31)) << 32) | disk_key(torch.arange(prio.shape[0], device=prio.device), seed)


def _key_order(state, kept, key):
    """the rows with state 1 in ascending order of key (distinct int64) without another host read (torch.nonzero would be one): one
    stable sort by the key, one that moves the other rows behind"""
    order = torch.argsort(key, stable=True)
    return order[torch.argsort((state[order] != 1).to(torch.uint8), stable=True)][:kept]


def _thin(ctx, pts, radius, seed, what, prio=None, state0=None):
    """Context.disk_sample over pts to the end -> (rows kept, in ascending key order; info).  One call and one host read of its
    counts; while rows are undecided, resumed calls - every round decides at least the undecided row of lowest key, so
    ceil(N / rounds) + 1 calls always suffice and one more is an error, not another turn of a loop.
    prio (N) f32 and / or state0 (N) uint8 (left as it is): Context.disk_sample_prio instead - the order of key64
    (include/yoho_salient.h; prio=None: a constant, the hashed order) from the start state0, whose rows set to 2 are masked out."""
    N = pts.shape[0]
    if N == 0:
        raise ValueError(f"{what}: no candidates")
    if prio is None and state0 is None:
        step = lambda state: ctx.disk_sample(pts, radius, seed=seed) if state is None else ctx.disk_sample(pts, radius, seed=seed, state=state)      # noqa: E731
    else:
        if prio is None:
            prio = torch.zeros((N,), dtype=torch.float32, device=pts.device)
        step = lambda state: ctx.disk_sample_prio(pts, radius, prio, seed=seed, state=state)      # noqa: E731
    state, n = step(None if state0 is None else state0.clone())
    kept, ran, open_ = (int(v) for v in n.tolist())
    if ran < 1 and open_ > 0:
        raise RuntimeError(f"{what}: {open_} rows undecided after a call that ran no round")
    calls, rounds = 1, ran
    bound = -(-N // max(ran, 1)) + 1                       # an unfinished call ran all of its rounds: `ran` is the rounds per call
    while open_ > 0:
        if calls >= bound:
            raise RuntimeError(f"{what}: {open_} of {N} rows still undecided after {calls} calls of {ran} rounds")
        state, n = step(state)
        kept, r, open_ = (int(v) for v in n.tolist())
        calls, rounds = calls + 1, rounds + r
    if prio is None:
        # the kept rows in key order without another host read (torch.nonzero would be one): the others sort behind every key, and the
        # keys are distinct, so any sort gives the one order
        key = torch.where(state == 1, disk_key(torch.arange(N, device=state.device), seed), torch.full((), 1 << 32, dtype=torch.int64, device=state.device))
        rows = torch.argsort(key)[:kept]
    else:
        rows = _key_order(state, kept, prio_key(prio, seed))
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


SALIENT_MODES = ("greedy", "nms")
SALIENT_DEFAULT_TIERS = 2                   # rank classes of the response by default: the largest tested number that ends inside one call of 16 rounds (profiles/salient.md)


def tier_classes(prio, tiers):
    """prio (N) f32 with NaN for the ineligible rows -> (N) f32: the rank class tiers - 1 - floor(tiers * descending rank / eligible) of
    an eligible row (the highest responses in class tiers - 1; equal responses ranked in row order), NaN elsewhere.  On the device,
    without a host read."""
    N = prio.shape[0]
    elig = ~torch.isnan(prio)
    order = torch.argsort(torch.where(elig, prio, torch.full_like(prio, float("-inf"))), descending=True, stable=True)
    # the ineligible rows may tie with an eligible -inf: the second stable sort puts every eligible row in front, in the order it has
    order = order[torch.argsort((~elig[order]).to(torch.uint8), stable=True)]
    rank = torch.empty((N,), dtype=torch.int64, device=prio.device)
    rank[order] = torch.arange(N, dtype=torch.int64, device=prio.device)
    cls = (int(tiers) - 1) - (int(tiers) * rank) // elig.sum().clamp(min=1)
    return torch.where(elig, cls.to(torch.float32), torch.full_like(prio, float("nan")))


def select_salient(ctx, pc_d, radius, salient_radius=None, mode="greedy", fill=True, tiers="default", min_nbrs=5, gamma21=0.975,
                   gamma32=0.975, nkpts=None, voxel=None, seed=0, clean=None):
    """Salient keypoints of pc_d (n,3) f64 on the device -> (kidx int64 cloud indices, info): Poisson-disk thinning at `radius` in the
    order of the ISS saliency (Context.iss_saliency at salient_radius, by default 2 radius) over select_disk's
    candidates, through clean_candidates when `clean` is a dict.  A row is eligible where its neighbourhood has min_nbrs points and
    eigenvalues l2 < gamma21 l3, l1 < gamma32 l2; its response is l1.
    mode "greedy": thinning to the end, the highest response first - non-maximum suppression that goes on to fill the gaps.  fill=True:
    the ineligible rows follow in hashed order, so select_disk's coverage bound holds for every candidate; fill=False: they are
    masked out (state 2) and the bound holds among the eligible rows only.
    mode "nms": ONE round from a start state that masks the ineligible rows, the rows it keeps - classical ISS, the eligible strict
    local maxima inside `radius`, no fill.
    tiers=k: the response is replaced by its rank class k - 1 - floor(k * descending rank / eligible) (tier_classes); rows of one
    class fall in hashed order, which shortens the chains of dependent decisions a smooth response builds.  "default":
    SALIENT_DEFAULT_TIERS for "greedy", and None - the response itself - for "nms", whose single round builds no chain.
    kidx is in ascending key64 order (include/yoho_salient.h); nkpts caps it as in select_disk, with the same loss of the bound.
    info: select_disk's, and eligible, mode, tiers."""
    if mode not in SALIENT_MODES:
        raise ValueError(f"select_salient: mode must be one of {SALIENT_MODES}, got {mode!r}")
    if isinstance(tiers, str):
        if tiers != "default":
            raise ValueError(f"select_salient: tiers={tiers!r} must be None, \"default\" or in [1, 2^24]")
        tiers = SALIENT_DEFAULT_TIERS if mode == "greedy" else None
    if tiers is not None and not 1 <= int(tiers) <= 1 << 24:
        raise ValueError(f"select_salient: tiers={tiers!r} must be None, \"default\" or in [1, 2^24]")
    sel, pts = candidates(ctx, pc_d, voxel)
    if clean is not None:
        sel, pts = clean_candidates(ctx, sel, pts, voxel, clean)
    if pts.shape[0] == 0:
        raise ValueError("select_salient: no candidates")
    prio = ctx.iss_saliency(pts, 2.0 * float(radius) if salient_radius is None else float(salient_radius), min_nbrs=min_nbrs, gamma21=gamma21,
                            gamma32=gamma32)[0]
    elig = ~torch.isnan(prio)
    n_elig = elig.sum()
    if tiers is not None:
        prio = tier_classes(prio, tiers)
    masked = torch.where(elig, 0, 2).to(torch.uint8)
    if mode == "nms":
        state, n = ctx.disk_sample_prio(pts, radius, prio, seed=seed, rounds=1, state=masked)
        kept = int(n.tolist()[0])
        rows = _key_order(state, kept, prio_key(prio, seed))
        info = {"radius": float(radius), "kept": kept, "rounds": 1, "calls": 1, "capped": False}
    else:
        rows, info = _thin(ctx, pts, radius, seed, "select_salient", prio=prio, state0=None if fill else masked)
    info.update(eligible=int(n_elig.item()), mode=mode, tiers=None if tiers is None else int(tiers))      # read behind the thinning's own host read
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


def _select_salient_host(ctx, pc, nkpts, voxel, radius, seed, saliency, clean=None):
    pc_d = torch.from_numpy(np.ascontiguousarray(np.asarray(pc, dtype=np.float64))).cuda()
    return select_salient(ctx, pc_d, radius, nkpts=nkpts, voxel=voxel, seed=seed, clean=clean, **saliency)[0].cpu().numpy()


def check_saliency(what, name, saliency):
    """saliency: None, or a dict of select_salient's keyword arguments other than those the caller sets itself -> a copy"""
    if saliency is None:
        return None
    allowed = ("salient_radius", "mode", "fill", "tiers", "min_nbrs", "gamma21", "gamma32")
    if not isinstance(saliency, dict) or set(saliency) - set(allowed):
        raise ValueError(f"{what}: {name} must be None or a dict with keys among {allowed}, got {saliency!r}")
    return dict(saliency)


METHODS = ("fps", "disk")


def write_keypoints(dataset, nkpts=5000, voxel=0.025, ctx=None, overwrite=False, selector=None, clean=None, method="fps", radius=None, seed=0, saliency=None):
    """Spread keypoints for every cloud of an EvalDataset that has no `Keypoints/cloud_bin_{k}Keypoints.txt` yet (overwrite=True: for
    every cloud): the index file, np.savetxt of the cloud indices in pick order, and `Keypoints_PC/cloud_bin_{k}Keypoints.npy`,
    pc[indices] - the two files ThrDMatchPartDataset.get_kps reads, in its formats, so that it never reaches its random draw.  A cloud
    whose index file exists is left alone.  selector(pc, nkpts, voxel) -> indices replaces the device selection (tests).
    clean: select's; a selector is then called as selector(pc, nkpts, voxel, clean=clean).
    method: "fps" (select), or "disk" - select_disk at `radius` (required then, refused otherwise) with priority seed `seed`, nkpts
    its cap, the indices in key order; it replaces the default selector only, a selector passed in is called as before.
    saliency (method "disk" only, refused otherwise): a dict of select_salient's keyword arguments ({}: its defaults) - the thinning
    runs in the order of the ISS saliency instead of the hash; None: select_disk, as before.
    -> the ids of the clouds written."""
    if method not in METHODS:
        raise ValueError(f"write_keypoints: method must be one of {METHODS}, got {method!r}")
    if (method == "disk") != (radius is not None):
        raise ValueError(f"write_keypoints: method=\"disk\" needs a radius, and only it takes one (method={method!r}, radius={radius!r})")
    saliency = check_saliency("write_keypoints", "saliency", saliency)
    if saliency is not None and method != "disk":
        raise ValueError(f"write_keypoints: saliency orders the thinning of method=\"disk\"; method={method!r} takes none")
    if selector is None:
        ctx = hip.get_context() if ctx is None else ctx
        if method == "disk" and saliency is not None:
            selector = lambda pc, n, v, clean=None: _select_salient_host(ctx, pc, n, v, radius, seed, saliency, clean)      # noqa: E731
        elif method == "disk":
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
