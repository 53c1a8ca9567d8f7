"""Outlier filters for a scan on the device (include/yoho_clean.h).

A scan carries strays - mixed pixels at depth edges, reflections, dust - and the stages behind it take every point for surface:
farthest-point sampling seeks the strays out, normal estimation averages them in, and the fused scene's min_frags only cleans where
two fragments overlap.  The two filters every point-cloud library has, on the exact k-NN inside a radius (Context.knn_within):

    statistical(ctx, pts, k=16, std_ratio=2.0, max_dist=0.1)      mean distance to the k nearest inside max_dist, keep <= mean + 2 sigma
    radius(ctx, pts, 0.05, 8)                                     keep the points with >= 8 others inside 0.05
    sel, kept = clean_cloud(ctx, pc_d, max_dist=0.1)              either of them on an (n,3) f64 cloud
    clean_cloud(ctx, pc_d, method="cluster", eps=0.1, min_size=100)   strays that come in clumps: yoho_amd.cluster.keep_large

Opt-in consumers: keypoints.select(..., clean={...}), yoho_extractor(..., keypoint_clean={...}), fuse.write_scene_cloud(..., clean={...}).
"""
import torch

from . import cluster


def _result(keep, mean_dist, stats, **more):
    sel = torch.nonzero(keep, as_tuple=False).reshape(-1)      # the one host read: the number of kept points
    return dict(keep=keep, sel=sel, mean_dist=mean_dist, stats=stats, **more)


def statistical(ctx, pts_f32, k=16, std_ratio=2.0, max_dist=None, min_found=1):
    """statistical outlier removal of pts_f32 (N,3) f32 on the device -> dict(keep (N) bool, sel ascending int64 indices of the kept
    points, mean_dist (N) f64, stats (4) f64 = (n_valid, mu, sigma, thr), count (N) int32), device tensors.  mean_dist: the mean
    distance to the min(k, count) nearest other points strictly inside max_dist, NaN for a point with fewer than min_found of them -
    an isolated point is an outlier by definition; kept: mean_dist <= mu + std_ratio * sigma over the valid points
    (Context.statistical_outliers).  max_dist bounds the search and has to be given: a few point spacings, so that a surface point
    finds its k neighbours and a stray does not."""
    if max_dist is None:
        raise ValueError("statistical: max_dist has to be given (a few point spacings)")
    if pts_f32.shape[0] == 0:
        raise ValueError("statistical: an empty cloud")
    r = ctx.statistical_outliers(pts_f32, max_dist, k=k, min_found=min_found, std_ratio=std_ratio)
    return _result(r["keep"].bool(), r["mean_dist"], r["stats"], count=r["count"])


def radius(ctx, pts_f32, radius, min_nbrs):
    """radius outlier removal of pts_f32 (N,3) f32 on the device: kept are the points with at least min_nbrs OTHER points strictly
    inside `radius` -> statistical's keys, mean_dist and stats None (a count-only Context.knn_within: no list is formed)."""
    if pts_f32.shape[0] == 0:
        raise ValueError("radius: an empty cloud")
    count = ctx.knn_within(pts_f32, pts_f32, radius, 1, skip_same_row=True, want_idx=False, want_d2=False)[2]
    return _result(count >= int(min_nbrs), None, None, count=count)


METHODS = {"statistical": statistical, "radius": radius, "cluster": cluster.keep_large}
# the argument that carries a method's radius: what the consumers default to 4 voxels
RADIUS_KEY = {"statistical": "max_dist", "radius": "radius", "cluster": "eps"}


def method_of(clean):
    """a consumer's clean dict -> (method, its radius argument's name): the optional "method" key, "statistical" when absent"""
    method = clean.get("method", "statistical")
    if method not in METHODS:
        raise ValueError(f"clean: method must be one of {sorted(METHODS)}, got {method!r}")
    return method, RADIUS_KEY[method]


def clean_cloud(ctx, pc_d, method="statistical", **kw):
    """pc_d (n,3) f64 on the device -> (sel ascending int64 indices of the kept points, pc_d[sel]); the filter runs on the cloud rounded
    to f32, kw are the method's arguments"""
    if method not in METHODS:
        raise ValueError(f"clean_cloud: method must be one of {sorted(METHODS)}, got {method!r}")
    if pc_d.dim() != 2 or pc_d.shape[1] != 3:
        raise ValueError("clean_cloud: pc_d (n,3)")
    sel = METHODS[method](ctx, pc_d.to(torch.float32).contiguous(), **kw)["sel"]
    return sel, pc_d[sel]
