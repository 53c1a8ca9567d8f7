/* Refinement entries of libyoho_hip.so: what a user runs behind the global estimators (yoho_o_score / yoho_c_ransac) to polish their
 * 3 x 4 transform on the device
 *
 *   yoho_nn_within          exact nearest neighbour inside a radius (a cell-sorted grid; the correspondence step of ICP)
 *   yoho_refit_matches      iterated proper-rotation Kabsch on the inlier matches of a transform
 *   yoho_icp_refine         gated point-to-point ICP on two clouds
 *
 * None of them mirrors a file of the reference: they are this library's own contracts, restated in numpy by tests/refine_ref.py.
 * The entries live in a header of their own beside yoho_hip.h, yoho_knn.h and yoho_trainset.h (whose symbol sets are pinned entry by
 * entry by their tests); tests/test_refine_cpu.py and tests/test_gpu_refine.py keep the same invariants for this one.  The
 * conventions of yoho_hip.h hold: device pointers, contiguous row-major, asynchronous on `stream`, YOHO_E* codes, yoho_last_error()
 * naming the entry.  float arrays 4-byte aligned (rows of 12 bytes, as yoho_nn_search with D = 3), double / int64 arrays 8-byte,
 * int32 arrays 4-byte.  Every result depends on nothing but the arguments: not on yoho_set_nn_grid / yoho_set_nn_prefilter, the
 * workspace contents or the call count; a workspace request refused under YOHO_WS_LIMIT_MB returns YOHO_ENOMEM and leaves the
 * context usable.  No entry reads anything back to the host.
 *
 * A transform T is 3 x 4 row-major f64, [R|t], and maps fragment 1 (k1, src) onto fragment 0 (k0, tgt): k0 ~ R k1 + t.
 *
 * THE SUM.  Every f64 sum over matches or points below is taken in one fixed order, so that results are bits, not approximations:
 * element e (a match, or a source point; an element outside the selected set contributes +0.0) belongs to block e / 256 and run
 * (e % 256) / 64; the 64 values of a run are added by halving - value l takes (value l) + (value l + 32) for l < 32, then with l + 16, 8, 4, 2, 1 -, the four
 * runs of a block in ascending order ((r0 + r1) + r2) + r3, a ragged tail padded with +0.0, and the blocks in ascending order onto
 * the first block's sum.
 *
 * THE KABSCH STEP over a set S of pairs (a_e on fragment 0's side, b_e on fragment 1's), n = |S| >= 3:
 *   c0 = SUM(a) / n, c1 = SUM(b) / n per coordinate, H[i][j] = SUM (b_i - c1_i)(a_j - c0_j) (second pass, each factor and the product
 *   rounded, no fma), H = U S V^T, R = V diag(1, 1, det(V U^T)) U^T, t_i = c0_i - ((R_i0 c1_0 + R_i1 c1_1) + R_i2 c1_2).
 * The decomposition is a one-sided Jacobi iteration in f64 (R is orthogonal with det +1 to f64 rounding; a planar set, s3 = 0, is
 * solved like any other).  The set has RANK BELOW 2 - the centred points of either side collinear or coincident, which leaves the
 * rotation open - when the singular values of H satisfy s1 = 0 or s2 <= 1e-13 s1; then no transform is formed.
 */
#ifndef YOHO_REFINE_H
#define YOHO_REFINE_H

#include "yoho_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define YOHO_REFINE_MAX_POINTS (1 << 22)   /* largest Nq / Nt / Ns / M */
#define YOHO_REFIT_MAX_ITERS 32
#define YOHO_ICP_MAX_ITERS 64

/* yoho_icp_refine's info[1] */
#define YOHO_ICP_ITERS 0        /* `iters` iterations were made */
#define YOHO_ICP_CONVERGED 1    /* max |T_{i+1} - T_i| <= tol: T_{i+1} was accepted */
#define YOHO_ICP_FEW_PAIRS 2    /* fewer than 3 pairs inside the gate: T_i was kept */
#define YOHO_ICP_RANK 3         /* the pairs have rank below 2: T_i was kept */

/* for every row of q (Nq,3) f32 the nearest row of tgt (Nt,3) f32 strictly inside max_dist.  With gate2 = max_dist * max_dist rounded
 * to f32, the candidates of row i are the j with d2 = ((qx - tx)^2 + (qy - ty)^2) + (qz - tz)^2 < gate2, every operation rounded to f32 and
 * none fused (yoho_nn_search's D = 3 'SquareL2' arithmetic, bit for bit); idx[i] is the candidate with the smallest pair (d2, j) and
 * d2[i] its d2 (d2 may be NULL).  Without a candidate idx[i] = -1 and d2[i] = +inf: a d2 equal to the gate is out, a NaN or
 * infinite query gets -1, a NaN target is nobody's neighbour.  In other words yoho_nn_search(D = 3, YOHO_DIST_SQUARE_L2)'s answer, kept
 * iff its distance is below the gate.  Nq = 0 is valid and launches nothing (q, idx may then be NULL); Nt >= 1; max_dist finite
 * and > 0; Nq, Nt <= YOHO_REFINE_MAX_POINTS.  Cost: a counting sort of tgt into cells of side max_dist (1 + 2^-10) per call, then one
 * lane per query over the 27 cells around it: sized for radii of a few point spacings, correct (not fast) for a gate that holds the
 * whole cloud. */
int yoho_nn_within(yoho_ctx* ctx, const float* q, int Nq, const float* tgt, int Nt, float max_dist, int64_t* idx, float* d2, void* stream);

/* iterated Kabsch on the inlier matches: k0, k1 (M,3) f64 matched keypoints as yoho_o_score takes them, T_in a DEVICE 3 x 4 (the
 * winners of yoho_o_score / yoho_c_ransac chain into it without a host read).  T_0 = T_in; for i = 0 .. iters:
 *   S_i = { m : |k0[m] - (R_i k1[m] + t_i)|^2 < inlier_dist * inlier_dist } with yoho_o_score's own predicate, so counts[0] is the count
 *   yoho_o_score gives T_in, bit for bit; counts[i] = |S_i|;  T_{i+1} = THE KABSCH STEP over S_i (a = k0, b = k1).
 * The iteration ends behind counts[i] when i = iters, when i >= 1 and S_i = S_{i-1} as sets (a fixed point: every later iterate would
 * repeat), when |S_i| < 3, or when S_i has rank below 2.  counts (iters + 1) int32: -1 for the iterates not reached.  T_out (3 x 4
 * f64) = the iterate with the largest count, the earliest among equal counts (the vote's strict '>'), so the result never holds
 * fewer inliers than T_in.  info (2) int32 = {index of that iterate, number of iterates evaluated}.  0 <= iters <=
 * YOHO_REFIT_MAX_ITERS; 0 <= M <= YOHO_REFINE_MAX_POINTS (M = 0: k0 / k1 may be NULL, counts[0] = 0, T_out = T_in); inlier_dist
 * finite and >= 0.  T_out may be T_in.  Sized for the few thousand matches of a pair: the per-block partial sums are added by one
 * thread per component, which is right up to the limit but not tuned for M near 2^20. */
int yoho_refit_matches(yoho_ctx* ctx, const double* k0, const double* k1, int M, const double* T_in, double inlier_dist, int iters,
                       double* T_out, int32_t* counts, int32_t* info, void* stream);

/* gated point-to-point ICP of src (Ns,3) f32 onto tgt (Nt,3) f32 from the device 3 x 4 T_in.  T_0 = T_in; iteration i < iters:
 *   q_e = (float)(((r0 sx + r1 sy) + r2 sz) + t) per coordinate for every source point e, in f64, each operation rounded, none fused;
 *   the pairs are yoho_nn_within(q, tgt, max_dist): npairs[i] their number n, rmse[i] = sqrt(SUM((double)d2) / n) (+inf when n = 0);
 *   T_{i+1} = THE KABSCH STEP over the pairs with a = (double)tgt[j_e], b = (double)src[e] - the UNTRANSFORMED source, so the iterates
 *   do not accumulate drift.
 * Stop rules, looked at in this order: n < 3 (T_i is kept, YOHO_ICP_FEW_PAIRS); rank below 2 (T_i is kept, YOHO_ICP_RANK); the largest
 * |T_{i+1} - T_i| over the 12 entries <= tol (T_{i+1} is accepted, YOHO_ICP_CONVERGED; a negative tol never stops); i + 1 = iters
 * (YOHO_ICP_ITERS).  T_out = the last accepted transform, info (2) int32 = {iterations made, reason}; npairs (iters) int32 / rmse
 * (iters) f64 hold -1 / -1.0 for the iterations not made.  0 <= iters <= YOHO_ICP_MAX_ITERS (0: T_out = T_in, info = {0,
 * YOHO_ICP_ITERS}; npairs / rmse may then be NULL); 1 <= Ns, Nt <= YOHO_REFINE_MAX_POINTS; max_dist finite and > 0; tol not NaN.
 * The grid over tgt is built once per call; all iterations are queued at once and the ones behind a stop return at once. */
int yoho_icp_refine(yoho_ctx* ctx, const float* src, int Ns, const float* tgt, int Nt, const double* T_in, float max_dist, int iters,
                    double tol, double* T_out, int32_t* npairs, double* rmse, int32_t* info, void* stream);

#ifdef __cplusplus
}
#endif

#endif
