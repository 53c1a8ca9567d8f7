"""Density clusters of a scan on the device (include/yoho_cluster.h).

The outlier filters of yoho_amd.clean remove isolated strays.  Strays that come in clumps - a person walking through the scan, a
reflection patch, the blob a misplaced fragment leaves in a fused scene - have plenty of close neighbours each and pass both of
them; farthest-point sampling then gives every clump a keypoint.  The third cleaning primitive every point-cloud library has, on
exact DBSCAN labels (Context.dbscan):

    dbscan(ctx, pts, 0.04, min_pts=4)                         labels, count, core, sizes, n = (clusters, core rows, noise rows)
    components(ctx, pts, 0.04)                                min_pts = 1: Euclidean cluster extraction
    keep_large(ctx, pts, 0.04, min_size=100)                  keep the points of clusters of >= 100 members
    keep_large(ctx, pts, 0.04, largest=1)                     keep the largest cluster
    sel, kept = clean.clean_cloud(ctx, pc_d, method="cluster", eps=0.04, min_size=100)

Opt-in consumers: keypoints.select(..., clean={"method": "cluster", ...}), fuse.write_scene_cloud(..., clean={"method": "cluster", ...}).
"""
import torch


def dbscan(ctx, pts_f32, eps, min_pts=4):
    """exact DBSCAN of pts_f32 (N,3) f32 on the device -> dict(labels (N) int32 cluster id or -1, count (N) int32, core (N) uint8,
    sizes (N) int32, n (3) int32), device tensors (Context.dbscan).  eps: a few point spacings."""
    if pts_f32.shape[0] == 0:
        raise ValueError("dbscan: an empty cloud")
    return ctx.dbscan(pts_f32, eps, min_pts=min_pts)


def components(ctx, pts_f32, radius):
    """the connected components of the graph that joins points closer than `radius`: dbscan with min_pts = 1, every finite point core"""
    return dbscan(ctx, pts_f32, radius, min_pts=1)


def keep_large(ctx, pts_f32, eps, min_pts=4, min_size=None, largest=None):
    """the points of the large clusters of pts_f32 (N,3) f32 -> clean.statistical's keys (keep (N) bool, sel ascending int64 indices of
    the kept points - the one host read -, mean_dist and stats None) plus labels, sizes, n of dbscan.  Exactly one of
    min_size: keep = label >= 0 and sizes[label] >= min_size;
    largest:  keep = label among the `largest` clusters with the most members, ties going to the lower id."""
    from .clean import _result
    if (min_size is None) == (largest is None):
        raise ValueError("keep_large: exactly one of min_size and largest has to be given")
    if int(min_size if largest is None else largest) < 1:
        raise ValueError("keep_large: min_size / largest must be at least 1")
    r = dbscan(ctx, pts_f32, eps, min_pts=min_pts)
    labels, sizes = r["labels"], r["sizes"]
    if largest is None:
        big = sizes >= int(min_size)
    else:
        order = torch.sort(sizes, descending=True, stable=True)[1]      # ties: the lower id first
        big = torch.zeros_like(sizes, dtype=torch.bool)
        big[order[:int(largest)]] = True
        big &= sizes > 0                                                 # fewer clusters than asked for
    keep = (labels >= 0) & big[labels.clamp(min=0).long()]
    return _result(keep, None, None, labels=labels, sizes=sizes, n=r["n"])
