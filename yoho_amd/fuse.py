"""A registered scene fused into one cloud (include/yoho_fuse.h): the fragments of a scene under their poses, reduced to
one mean point per voxel with the number of points and of distinct fragments behind it, and the files that carry the result.

    fuse_clouds(ctx, clouds_d, poses, voxel)         the device pass (Context.fuse_clouds) on a list of fragments
    fuse_registered(ctx, clouds_d, result, voxel)    the same on multiway.register_scene's result; unreached fragments (NaN poses) drop out
    write_ply / read_ply                             binary little-endian PLY with plain numpy
    write_scene_cloud(cfg, dataset)                  poses.log (multiway.write_scene) + the dataset's clouds -> scene.ply beside the log
    clean_fused(ctx, out, clean)                     the fused rows an outlier filter keeps (yoho_amd.clean)
"""
import os

import numpy as np

from . import RR_cal
from .multiway import _scene_clouds, as_4x4

f32, f64 = np.float32, np.float64
_PLY_FIELDS = (("x", "<f4", "float"), ("y", "<f4", "float"), ("z", "<f4", "float"), ("nx", "<f4", "float"), ("ny", "<f4", "float"), ("nz", "<f4", "float"),
               ("count", "<i4", "int"), ("nfrag", "<i4", "int"))


# ---- the device pass -----------------------------------------------------------------------------------------------------------------------
def fuse_clouds(ctx, clouds_d, poses, voxel, min_count=1, min_frags=1, normals=None):
    """clouds_d: the K fragments as (n_k,3) device tensors (f32, or anything .to(float32) takes), each in its own frame; poses (K,4,4) or
    (K,3,4): fragment k into the scene frame (a NaN pose removes its fragment); normals: None or K (n_k,3) tensors ->
    dict(pts (M,3) f32, normals (M,3) f32 or None, count (M) int32, nfrag (M) int32: device tensors, the kept voxels in ascending key;
    row_of: K int32 device tensors, the row of every input point's voxel or -1; M).  One concatenation, Context.fuse_clouds' two
    calls and its one read of M."""
    import torch
    K = len(clouds_d)
    T34 = np.ascontiguousarray(as_4x4(poses)[:, :3, :], dtype=f64)
    if T34.shape[0] != K or (normals is not None and len(normals) != K):
        raise ValueError("fuse_clouds: one pose (and one array of normals) per fragment")
    as32 = lambda c: c if c.dtype == torch.float32 and c.is_contiguous() else c.to(torch.float32).contiguous()      # noqa: E731
    clouds = [as32(c) for c in clouds_d]
    soff = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int64)
    src = clouds[0] if K == 1 else torch.cat(clouds, dim=0)
    nrm = None
    if normals is not None:
        ns = [as32(n) for n in normals]
        nrm = ns[0] if K == 1 else torch.cat(ns, dim=0)
    out = ctx.fuse_clouds(src, soff, torch.from_numpy(T34).to(src.device), voxel, min_count, min_frags, nrm=nrm)
    out["row_of"] = [out["row_of"][int(soff[k]):int(soff[k + 1])] for k in range(K)]
    return out


def fuse_registered(ctx, clouds_d, result, voxel, min_count=1, min_frags=1, normals=None):
    """fuse_clouds under the poses of multiway.register_scene - its (edges, result) pair or the result dict alone, as it is: the
    fragments the kept edges did not reach have NaN poses and contribute nothing"""
    res = result[1] if isinstance(result, tuple) else result
    return fuse_clouds(ctx, clouds_d, res["poses"], voxel, min_count, min_frags, normals)


# ---- files -------------------------------------------------------------------------------------------------------------------------------
def _ply_layout(has_normals, has_count, has_nfrag):
    use = [True, True, True, has_normals, has_normals, has_normals, has_count, has_nfrag]
    return [fld for fld, on in zip(_PLY_FIELDS, use) if on]


def write_ply(path, pts, normals=None, count=None, nfrag=None):
    """pts (M,3), normals (M,3) or None, count / nfrag (M) or None -> a binary little-endian PLY: vertex properties x y z (float), then
    nx ny nz (float), count (int), nfrag (int) for what is given.  Plain numpy; what it writes depends on the arrays alone."""
    pts = np.asarray(pts, f32).reshape(-1, 3)
    M = pts.shape[0]
    fields = _ply_layout(normals is not None, count is not None, nfrag is not None)
    rec = np.zeros((M,), dtype=np.dtype([(name, code) for name, code, _ in fields]))
    rec["x"], rec["y"], rec["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
    if normals is not None:
        normals = np.asarray(normals, f32).reshape(M, 3)
        rec["nx"], rec["ny"], rec["nz"] = normals[:, 0], normals[:, 1], normals[:, 2]
    if count is not None:
        rec["count"] = np.asarray(count).reshape(M)
    if nfrag is not None:
        rec["nfrag"] = np.asarray(nfrag).reshape(M)
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % M
    header += "".join("property %s %s\n" % (kind, name) for name, _, kind in fields) + "end_header\n"
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(rec.tobytes())


def read_ply(path):
    """a file of write_ply -> dict(pts (M,3) f32, normals (M,3) f32 or None, count (M) int32 or None, nfrag (M) int32 or None)"""
    with open(path, "rb") as fh:
        raw = fh.read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: not a binary little-endian PLY")
    M, props = None, []
    for ln in lines[2:]:
        tok = ln.split()
        if tok[0] == "element":
            if tok[1] != "vertex" or M is not None:
                raise ValueError(f"{path}: only a vertex element is read")
            M = int(tok[2])
        elif tok[0] == "property":
            props.append((tok[2], tok[1]))
    known = {name: (code, kind) for name, code, kind in _PLY_FIELDS}
    if M is None or any(name not in known or known[name][1] != kind for name, kind in props):
        raise ValueError(f"{path}: properties {props} are not write_ply's")
    rec = np.frombuffer(raw, dtype=np.dtype([(name, known[name][0]) for name, _ in props]), count=M, offset=end)
    if len(raw) != end + rec.nbytes:
        raise ValueError(f"{path}: {len(raw) - end} bytes of data for {M} vertices")
    names = [name for name, _ in props]
    col = lambda *ks: np.ascontiguousarray(np.stack([rec[k] for k in ks], axis=1)) if M else np.zeros((0, len(ks)), f32)      # noqa: E731
    return {"pts": col("x", "y", "z"), "normals": col("nx", "ny", "nz") if "nx" in names else None,
            "count": np.ascontiguousarray(rec["count"]) if "count" in names else None,
            "nfrag": np.ascontiguousarray(rec["nfrag"]) if "nfrag" in names else None}


def filter_rows(out, sel):
    """the rows `sel` (ascending indices) of a fused result: pts, normals, count and nfrag together; M follows; row_of, which names rows
    of the unfiltered result, does not travel"""
    kept = {k: (None if out.get(k) is None else out[k][sel]) for k in ("pts", "normals", "count", "nfrag")}
    kept["M"] = int(kept["pts"].shape[0])
    return kept


def clean_fused(ctx, out, clean):
    """the fused result (host arrays) without the rows yoho_amd.clean.statistical drops from its points.  clean: a dict of that function's
    keyword arguments; max_dist has to be among them (a fused cloud's spacing is its voxel's: 4 voxels is the usual choice).  An
    optional "method" key names another filter of yoho_amd.clean.METHODS ("cluster": yoho_amd.cluster.keep_large, with its eps); the
    other keys are then that filter's arguments."""
    import torch
    from . import clean as CL
    from . import hip
    ctx = hip.get_context() if ctx is None else ctx
    pts = torch.from_numpy(np.ascontiguousarray(out["pts"], dtype=f32)).cuda()
    kw = dict(clean)
    method = CL.method_of(kw)[0]
    kw.pop("method", None)
    return filter_rows(out, CL.METHODS[method](ctx, pts, **kw)["sel"].cpu().numpy())


def _device_fuse(ctx):
    import torch
    from . import hip
    ctx = hip.get_context() if ctx is None else ctx

    def fuse(clouds, poses, voxel, min_count, min_frags):
        out = fuse_clouds(ctx, [torch.from_numpy(np.ascontiguousarray(c, dtype=f32)).cuda() for c in clouds], poses, voxel, min_count, min_frags)
        return {k: (None if out[k] is None else out[k].cpu().numpy()) for k in ("pts", "normals", "count", "nfrag")}
    return fuse


def write_scene_cloud(cfg, dataset, yoho_sign='YOHO_O_MW', voxel=0.025, min_frags=1, fuse=None, max_iter=1000, min_count=1, ctx=None, clean=None,
                      cleaner=None):
    """The fused cloud of one scene.  Reads result_dir(cfg, dataset, yoho_sign, max_iter)/poses.log (what multiway.write_scene left: one
    pose per fragment, nan for an unreached one) and the dataset's clouds, fuses them and writes scene.ply beside the log: the mean point
    of every voxel that >= min_count points of >= min_frags fragments fed, with both counts.
    fuse(clouds, poses, voxel, min_count, min_frags) -> dict(pts, normals or None, count, nfrag), on host arrays, replaces the device
    pass (tests).  clean: None, or a dict of yoho_amd.clean.statistical's keyword arguments (max_dist defaults to 4 voxels) - or, with
    "method": "cluster", of yoho_amd.cluster.keep_large's (eps defaults to 4 voxels; the key travels on to the cleaner) -: the fused
    rows that filter drops - strays that min_frags cannot reach where one fragment alone saw a region - are left out of the file, with
    their normals, count and nfrag; cleaner(out, clean) -> dict replaces clean_fused (tests).  -> (path, the dict written)"""
    from .run_dataset import result_dir
    out_dir = result_dir(cfg, dataset, yoho_sign, max_iter)
    _, poses = RR_cal.read_trajectory(os.path.join(out_dir, 'poses.log'))
    clouds = _scene_clouds(dataset)
    if poses.shape[0] != len(clouds):
        raise ValueError(f"write_scene_cloud: poses.log holds {poses.shape[0]} poses, the dataset {len(clouds)} clouds")
    fuse = _device_fuse(ctx) if fuse is None else fuse
    out = fuse(clouds, poses, voxel, min_count, min_frags)
    if clean is not None:
        from . import clean as CL
        kw = dict(clean)
        key = CL.method_of(kw)[1]
        if kw.get(key) is None:
            kw[key] = 4.0 * float(voxel)
        out = cleaner(out, kw) if cleaner is not None else clean_fused(ctx, out, kw)
    path = os.path.join(out_dir, 'scene.ply')
    write_ply(path, out["pts"], out.get("normals"), out["count"], out["nfrag"])
    return path, out
