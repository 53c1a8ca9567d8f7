"""Registration from the match list alone: the compatibility graph of the matches, its second-order scores, a hypothesis per cluster of
mutually consistent matches (include/yoho_consist.h), then the entries that already choose among hypotheses and polish one -
the vote's counts, the verification on the clouds, the refit - all on the device, chained through device memory, one host read at the
end.  Needs no PartII weights and no coarse rotation index (dr_index): a context with nothing loaded will do, which is the point - every
other estimator of the package turns PartII's per-match rotation into its hypotheses.  Not a mirror of a reference file."""
import numpy as np
import torch

from . import hip


def empty_result(K, refit_iters=4):
    """register_matches' dict for a pair without a match: no row taken (Kc = 0, row = -1), trans = trans_refit = [I|0], every per-row array
    what the entries write behind Kc (seeds -1, sizes / counts 0), the verification's figures as for rows never evaluated, the refit's as
    yoho_refit_matches gives them at M = 0 (counts[0] = 0, -1 for the iterates not reached)"""
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    out = {"Kc": 0, "seeds": np.full((K,), -1, np.int32), "sizes": np.zeros((K,), np.int32), "counts": np.zeros((K,), np.int32),
           "top": None, "npairs": None, "rmse": None, "cost": None, "best": None, "fitness": None, "row": -1,
           "trans": eye, "trans_refit": eye.copy(), "refit_counts": np.array([0] + [-1] * int(refit_iters), np.int32), "refit_best": 0, "inliers": 0}
    if K > 1:
        out.update(top=np.full((K,), -1, np.int32), npairs=np.full((K,), -1, np.int32), rmse=np.full((K,), -1.0), cost=np.full((K,), -1.0), best=-1, fitness=0.0)
    return out


def register_matches(ctx, keys0, keys1, match, tol, K=8, min_len=0.0, inlier_dist=None, refit_iters=4, clouds=None, max_dist=None):
    """keys0 / keys1 (N,3) f64 cuda keypoints of fragment 0 / 1, match (M,2) int64 cuda rows into them (match=None: keys0 / keys1 are the
    matched keypoints themselves, row by row), M <= hip.CONSIST_MAX_M; an empty match list gives empty_result(K) and runs nothing.  Needs no
    PartII weights and no dr_index.
      graph       Context.consistency_graph(tol, min_len): two matches are compatible when they keep their distance within tol
      scores      Context.sc2_scores
      hypotheses  Context.consensus_hypotheses: K rows (1 .. hip.CONSIST_MAX_K), Kc of them taken
      vote        Context.o_score over the K rows in row order at inlier_dist (None: tol); rows behind Kc count 0
      choice      K = 1: row 0 if it has a count.  K > 1: Context.verify_hypotheses over the rows with a count - on clouds = (cloud0, cloud1), (N,3) f32
                  cuda, when given, on the whole keypoint sets otherwise (all of keys1 onto all of keys0, cast to f32, not the matched rows alone), as
                  pipeline.run_pair does -
                  inside max_dist (None: inlier_dist): the row with the smallest truncated cost
      refit       Context.refit_matches from the chosen device row, refit_iters iterations
    -> dict(trans (3,4) f64 host: the chosen row ([I|0] when no row qualifies), trans_refit, refit_counts, refit_best, inliers (the count
    of trans_refit), row (the chosen row, -1 when none), Kc, seeds / sizes / counts (K), and for K > 1 top, npairs, rmse, cost (K; -1
    behind the rows evaluated), best, fitness - None for K = 1), fetched in one host read."""
    K = int(K)
    if not 1 <= K <= hip.CONSIST_MAX_K:
        raise ValueError(f"register_matches: K must be in [1, {hip.CONSIST_MAX_K}], got {K}")
    d = float(tol if inlier_dist is None else inlier_dist)
    if match is not None and match.shape[0] == 0:
        return empty_result(K, refit_iters)                            # a shape, not a device value: no match, no hypothesis
    # k0 / k1: the matched rows, what the graph, the vote and the refit see; keys0 / keys1 stay the whole keypoint sets for the verification
    k0, k1 = (keys0, keys1) if match is None else (keys0[match[:, 0]], keys1[match[:, 1]])
    k0, k1 = k0.contiguous(), k1.contiguous()
    bits, _ = ctx.consistency_graph(k0, k1, tol, min_len)
    s2 = ctx.sc2_scores(bits)
    T, seeds, sizes, info = ctx.consensus_hypotheses(k0, k1, bits, s2, K)
    _, counts = ctx.o_score(k0, k1, T, None, K, d)
    counts = torch.where(torch.arange(K, device=counts.device, dtype=torch.int32) < info[0], counts, torch.zeros_like(counts))      # [I|0] rows are no hypotheses
    parts = [info.to(torch.float64), seeds.to(torch.float64), sizes.to(torch.float64), counts.to(torch.float64)]
    if K == 1:
        chosen = torch.where(counts[0] > 0, T[0], torch.eye(3, 4, dtype=torch.float64, device=T.device)).contiguous()
    else:
        src, tgt = (clouds[1], clouds[0]) if clouds is not None else (keys1.to(torch.float32).contiguous(), keys0.to(torch.float32).contiguous())
        chosen, top, npairs, rmse, cost, vinfo = ctx.verify_hypotheses(src, tgt, T, counts, K, d if max_dist is None else max_dist)
        parts += [top.to(torch.float64), npairs.to(torch.float64), rmse, cost, vinfo.to(torch.float64)]
    T_fit, rcounts, rinfo = ctx.refit_matches(k0, k1, chosen, d, refit_iters)
    parts += [chosen.reshape(-1), T_fit.reshape(-1), rcounts.to(torch.float64), rinfo.to(torch.float64)]
    host = torch.cat(parts).cpu().numpy()                  # the one host read
    cut = lambda n: (host[:n], host[n:])
    h, host = cut(2)
    out = {"Kc": int(h[0])}
    for name in ("seeds", "sizes", "counts"):
        h, host = cut(K)
        out[name] = h.astype(np.int32)
    out.update(top=None, npairs=None, rmse=None, cost=None, best=None, fitness=None)
    if K == 1:
        out["row"] = 0 if out["counts"][0] > 0 else -1
    else:
        for name in ("top", "npairs"):
            h, host = cut(K)
            out[name] = h.astype(np.int32)
        for name in ("rmse", "cost"):
            h, host = cut(K)
            out[name] = h.copy()
        h, host = cut(4)
        best = out["best"] = int(h[1])
        out["row"] = int(h[2])
        out["fitness"] = float(out["npairs"][best]) / src.shape[0] if best >= 0 else 0.0
    h, host = cut(12)
    out["trans"] = h.reshape(3, 4).copy()
    h, host = cut(12)
    out["trans_refit"] = h.reshape(3, 4).copy()
    h, host = cut(rcounts.shape[0])
    out["refit_counts"] = h.astype(np.int32)
    out["refit_best"] = int(host[0])
    out["inliers"] = int(out["refit_counts"][out["refit_best"]])
    return out
