/* Verification of the estimator's hypotheses on the clouds: what a user runs between the YOHO-O vote and the refinement entries
 * 
 *
 *   yoho_eval_transforms     K transforms evaluated on two clouds in one pass: pairs inside a gate, rmse, truncated cost
 *   yoho_verify_hypotheses   the best few DISTINCT hypotheses of a vote, evaluated like that, the cheapest handed on
 *
 * The vote (yoho_o_score) counts inliers among a few thousand sparse matches and commits to the first strict maximum; the refinement
 * entries (yoho_refine.h, yoho_plane.h) then polish that one transform.  These two entries look at the dense geometry first, and give
 * a caller without ground truth a fitness figure for any transform.  A header of their own beside yoho_refine.h and yoho_plane.h, whose
 * symbol sets are pinned by their tests; tests/test_verify_cpu.py and tests/test_gpu_verify.py keep the same invariants for this one.
 * The conventions, YOHO_REFINE_MAX_POINTS, a transform T (3 x 4 row-major f64 [R|t], src = fragment 1 onto tgt = fragment 0) and THE
 * SUM are yoho_refine.h's: device pointers, contiguous row-major, asynchronous on `stream`, YOHO_E* codes, yoho_last_error() naming the
 * entry; float arrays 4-byte aligned (rows of 12 bytes), double / int64 arrays 8-byte, int32 arrays 4-byte.  Neither entry mirrors a
 * file of the reference: tests/verify_ref.py restates both in numpy.  Every result depends on nothing but the arguments (not on
 * yoho_set_nn_grid / yoho_set_nn_prefilter, the workspace contents or the call count); a workspace request refused under
 * YOHO_WS_LIMIT_MB returns YOHO_ENOMEM and leaves the context usable; no entry reads anything back to the host or uses a float atomic.
 */
#ifndef YOHO_VERIFY_H
#define YOHO_VERIFY_H

#include "yoho_refine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define YOHO_VERIFY_MAX_K 64               /* largest number of transforms evaluated by one call */

/* the K transforms T (K,3,4) f64 evaluated on src (Ns,3) f32 and tgt (Nt,3) f32.  For every row k, from T[k] = [R|t]:
 *   q_e = (float)(((r0 sx + r1 sy) + r2 sz) + t) per coordinate for every source point e, in f64, each operation rounded, none fused
 *   (yoho_icp_refine's arithmetic); point e is PAIRED iff yoho_nn_within(q, tgt, max_dist) gives it a partner, d2_e that answer's d2.
 *   npairs[k] = n, the number of paired points;
 *   rmse[k]   = sqrt(SUM(paired ? (double)d2_e : +0.0) / n), +inf when n = 0;
 *   cost[k]   = SUM(paired ? (double)d2_e : (double)gate2), gate2 = max_dist * max_dist rounded to f32: the truncated (MSAC) cost - a
 *               point without a partner costs what a partner at the gate would, so more pairs AND closer pairs both lower it.
 * Both sums are THE SUM over e = 0 .. Ns - 1 in the source's own index order: rmse and cost are bits.  A non-finite entry of T[k] makes
 * the queries it reaches NaN or infinite and leaves them unpaired; nothing else is special-cased.  1 <= K <= YOHO_VERIFY_MAX_K;
 * 1 <= Ns, Nt <= YOHO_REFINE_MAX_POINTS; max_dist finite and > 0.  The grid over tgt is built once per call, whatever K is: for K = 1
 * npairs[0], rmse[0] are yoho_icp_refine(iters = 1)'s npairs[0], rmse[0] bit for bit. */
int yoho_eval_transforms(yoho_ctx* ctx, const float* src, int Ns, const float* tgt, int Nt, const double* T, int K, float max_dist, int32_t* npairs,
                         double* rmse, double* cost, void* stream);

/* the vote's best few distinct hypotheses, verified on the clouds.  Position h < H stands for the hypothesis T[order ? order[h] : h]
 * with counts[h] inliers: yoho_o_score's own addressing (order (H) int64 or NULL, every order[h] a row of T) and its counts output.
 *   SELECTION.  Position h is alive iff counts[h] >= min_count.  Up to K times: take the alive position with the largest count, the
 *   smallest h among equal counts (the vote's strict '>': with distinct_tol = 0 top[0] is yoho_o_score's best_h whenever its
 *   best_count >= min_count), record it in top[i] and kill it; if distinct_tol > 0 also kill every alive h' all of whose 12 entries
 *   differ from the taken hypothesis' by less than distinct_tol in absolute value (a NaN difference is not less: it kills nothing).  A
 *   cluster of n inlier matches produces n near-identical hypotheses of one count; without the suppression they fill the list.
 *   Kc <= K is the number taken; rows i >= Kc hold top = -1, npairs = -1, rmse = cost = -1.0.
 *   EVALUATION.  Rows i < Kc: npairs[i], rmse[i], cost[i] are yoho_eval_transforms' for the hypothesis of top[i], bit for bit.
 *   PICK.  best = 0; for i = 1 .. Kc - 1 in order best = i if cost[i] < cost[best] (equal costs keep the earlier row).  T_out (3 x 4
 *   f64) = the hypothesis of top[best], copied byte for byte; info (4) int32 = {Kc, best, top[best], counts[top[best]]}.  Kc = 0 (no
 *   position alive; H = 0 is valid, T / order / counts may then be NULL): T_out = [I | 0], as the reference returns eye(4), info =
 *   {0, -1, -1, 0}.
 * T_out is a device 3 x 4: it chains into yoho_refit_matches / yoho_icp_refine / yoho_icp_plane without a host read.  Kc stays on
 * the device: K rows are launched and the ones behind Kc return at once.  1 <= K <= YOHO_VERIFY_MAX_K; min_count >= 1; distinct_tol
 * finite and >= 0; 0 <= H <= YOHO_REFINE_MAX_POINTS; Ns, Nt, max_dist as above.  Sized for the few thousand hypotheses of a pair:
 * the selection is one workgroup, K sweeps over the H positions, which is right up to the limit but not tuned for H near 2^20. */
int yoho_verify_hypotheses(yoho_ctx* ctx, const float* src, int Ns, const float* tgt, int Nt, const double* T, const int64_t* order,
                           const int32_t* counts, int H, int K, int min_count, double distinct_tol, float max_dist, double* T_out, int32_t* top,
                           int32_t* npairs, double* rmse, double* cost, int32_t* info, void* stream);

#ifdef __cplusplus
}
#endif

#endif
