"""Refinement behind the global estimators: the winner's [R|t] refitted on its inlier matches (iterated Kabsch) and, where the
clouds are at hand, polished by a few iterations of gated ICP, point-to-point or point-to-plane - all on the device
(include/yoho_refine.h, include/yoho_plane.h), chained through device memory: the transform an estimator left on the device goes in, one host read at the end
brings everything back.  Not a mirror of a reference file: the reference stops at the estimator's transform."""
import numpy as np
import torch

from . import hip


def refine_pair(ctx, keys0, keys1, matches, T, inlier_dist, iters=4, clouds=None, max_dist=None, icp_iters=30, tol=0.0, icp="point", normal_radius=None):
    """keys0 / keys1 (K,3) f64 cuda keypoints of fragment 0 / 1, matches (M,2) int64 cuda rows into them (matches=None: keys0 / keys1
    are the matched keypoints themselves, row by row), T (3,4) f64 mapping fragment 1 onto fragment 0 - a device tensor (no host
    read in front) or a host array.  Refit: Context.refit_matches with `iters` iterations.  clouds = (cloud0, cloud1), (N,3) f32
    cuda, adds Context.icp_refine of cloud1 onto cloud0 inside max_dist, started from the refit's transform; icp="plane" runs
    Context.icp_plane instead, on cloud0's normals from Context.estimate_normals inside normal_radius (None: max_dist) - icp_rmse is then
    the point-to-plane rms.
    -> dict(trans (3,4) f64 host: the refined transform, trans_refit, refit_counts (iters + 1, -1 = not reached), refit_best,
    refit_evaluated, inliers (the count of trans_refit, never below counts[0] = T's own) and, with clouds, trans_icp, icp_npairs,
    icp_rmse (icp_iters; -1 = not made), icp_iters, icp_reason (one of hip.ICP_REASONS), icp_mode ("point" / "plane"))"""
    if icp not in ("point", "plane"):
        raise ValueError(f"refine_pair: icp must be 'point' or 'plane', got {icp!r}")
    if clouds is not None and (max_dist is None or not max_dist > 0):
        raise ValueError("refine_pair: clouds need a max_dist > 0")
    dev = keys0.device
    if matches is not None:
        keys0, keys1 = keys0[matches[:, 0]].contiguous(), keys1[matches[:, 1]].contiguous()
    Td = T if isinstance(T, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(T, dtype=np.float64)[:3, :4])).to(dev)
    Td = Td.reshape(3, 4).contiguous()
    T_fit, counts, info = ctx.refit_matches(keys0, keys1, Td, inlier_dist, iters)
    parts = [T_fit.reshape(-1), counts.to(torch.float64), info.to(torch.float64)]
    if clouds is not None:
        if icp == "plane":
            normals, _ = ctx.estimate_normals(clouds[0], max_dist if normal_radius is None else normal_radius)
            T_icp, npairs, rmse, iinfo = ctx.icp_plane(clouds[1], clouds[0], normals, T_fit, max_dist, icp_iters, tol)
        else:
            T_icp, npairs, rmse, iinfo = ctx.icp_refine(clouds[1], clouds[0], T_fit, max_dist, icp_iters, tol)
        parts += [T_icp.reshape(-1), npairs.to(torch.float64), rmse, iinfo.to(torch.float64)]
    host = torch.cat(parts).cpu().numpy()                  # the one host read
    n = counts.shape[0]
    out = {"trans_refit": host[:12].reshape(3, 4).copy(), "refit_counts": host[12:12 + n].astype(np.int32),
           "refit_best": int(host[12 + n]), "refit_evaluated": int(host[13 + n])}
    out["inliers"] = int(out["refit_counts"][out["refit_best"]])
    out["trans"] = out["trans_refit"]
    if clouds is not None:
        h = host[14 + n:]
        k = npairs.shape[0]
        out.update(trans_icp=h[:12].reshape(3, 4).copy(), icp_npairs=h[12:12 + k].astype(np.int32), icp_rmse=h[12 + k:12 + 2 * k].copy(),
                   icp_iters=int(h[12 + 2 * k]), icp_reason=hip.ICP_REASONS[int(h[13 + 2 * k])], icp_mode=icp)
        out["trans"] = out["trans_icp"]
    return out
