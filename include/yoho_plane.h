/* Surface normals and point-to-plane ICP: the refinement that has no sampling floor
 *
 *   yoho_estimate_normals   per point: neighbours inside a radius, f64 covariance, the eigenvector of its smallest eigenvalue
 *   yoho_icp_plane          gated point-to-plane ICP on two clouds, the target with normals
 *
 * A header of their own beside yoho_refine.h, whose symbol set is pinned by its tests; tests/test_plane_cpu.py and
 * tests/test_gpu_plane.py keep the same invariants for this one.  The conventions, YOHO_REFINE_MAX_POINTS, YOHO_ICP_MAX_ITERS, the
 * four YOHO_ICP_* reason codes, a transform T (3 x 4 row-major f64 [R|t], src onto tgt) and THE SUM are yoho_refine.h's.  Neither
 * entry mirrors a file of the reference: tests/plane_ref.py restates both in numpy.  Every result depends on nothing but the
 * arguments (not on yoho_set_nn_grid / yoho_set_nn_prefilter, the workspace contents or the call count); a workspace request refused
 * under YOHO_WS_LIMIT_MB returns YOHO_ENOMEM and leaves the context usable; no entry reads anything back to the host or uses a float
 * atomic.
 */
#ifndef YOHO_PLANE_H
#define YOHO_PLANE_H

#include "yoho_refine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* normals of pts (N,3) f32 from the neighbours inside `radius`.  The neighbours of point i are the j, i itself included, with
 * d2 = ((dx^2 + dy^2) + dz^2) < gate2 = radius * radius rounded to f32 - yoho_nn_within's arithmetic, f32, nothing fused; count[i]
 * (int32) is their number, exact.  A point with a NaN or infinite coordinate has count 0 and is nobody's neighbour.
 *   Covariance, f64, one pass about the point itself: d = (double)p_j - (double)p_i, S1 = sum d, S2 = sum d d^T, C = S2 - S1 S1^T / n.
 *   The neighbours are added in the order of the grid walk: deterministic (results repeat bit for bit from call to call) but not
 *   part of the contract, so a reference is met by a tolerance, not by bits.
 *   normals[i] (f32) = the unit eigenvector of the smallest eigenvalue l1 <= l2 <= l3 of C (an f64 Jacobi iteration), rounded to
 *   f32; curv[i] = (float)(l1 / (l1 + l2 + l3)) (curv may be NULL).  Orientation: with v = (vx, vy, vz), n . (v - p_i) >= 0, the
 *   product ((nx (vx - px) + ny (vy - py)) + nz (vz - pz)) taken in f64 on the f64 eigenvector; when it is exactly 0, the first non-zero
 *   component of n is positive.
 *   Invalid: count[i] < min_nbrs, or l3 = 0 (not > 0), or l2 <= 1e-12 l3 (collinear neighbours leave the normal open).  Then
 *   normals[i] = (0, 0, 0) and curv[i] = -1.
 * 1 <= N <= YOHO_REFINE_MAX_POINTS; radius finite and > 0; min_nbrs >= 3; v finite.  Cost: yoho_nn_within's counting sort of pts
 * into cells of side radius (1 + 2^-10), then one lane per point over the 27 cells around it. */
int yoho_estimate_normals(yoho_ctx* ctx, const float* pts, int N, float radius, int min_nbrs, float vx, float vy, float vz, float* normals,
                          int32_t* count, float* curv, void* stream);

/* gated point-to-plane ICP of src (Ns,3) f32 onto tgt (Nt,3) f32 with tgt_normals (Nt,3) f32 (yoho_estimate_normals', or the
 * caller's), from the device 3 x 4 T_in.  T_0 = T_in; iteration i < iters, from T_i = [R|t]:
 *   x_e = ((r0 sx + r1 sy) + r2 sz) + t per coordinate for every source point e, in f64, each operation rounded, none fused;
 *   q_e = (float)x_e; j_e = yoho_nn_within(q, tgt, max_dist)'s answer.  The pair is KEPT iff j_e >= 0 and n = (double)tgt_normals[j_e]
 *   is finite and not (0, 0, 0); npairs[i] = their number n_kept.
 *   First pass: c = SUM(x) / n_kept per coordinate over the kept pairs (THE SUM over e; c = 0 without a pair).
 *   Second pass, nothing fused: u = x - c, p = (double)tgt[j], r = ((nx (x_x - p_x)) + ny (x_y - p_y)) + nz (x_z - p_z),
 *   a = u x n with every component formed as u_y n_z - u_z n_y, J = (a_x, a_y, a_z, n_x, n_y, n_z); the 28 sums by THE SUM:
 *   A_kl = SUM J_k J_l (k <= l), b_k = SUM J_k r, E = SUM r r.  rmse[i] = sqrt(E / n_kept), +inf at 0 pairs: the point-to-plane rms
 *   in front of the step.
 *   A z = -b by an unpivoted Cholesky decomposition in that order of the variables, f64, z = (w, v).  The system has RANK BELOW 6 when
 *   a pivot d_k = A_kk - sum_m L_km^2 is not > 1e-13 A_kk (a single exact plane: A_kk = 0 for three variables).
 *   dR = exp([w]x) (Rodrigues, a series for small |w|), R' = dR R, t' = ((dR (t - c)) + c) + v; no re-orthonormalisation.
 * Stop rules, looked at in this order: n_kept < 6 (T_i is kept, YOHO_ICP_FEW_PAIRS); rank below 6 (T_i is kept, YOHO_ICP_RANK); the
 * largest |T_{i+1} - T_i| over the 12 entries <= tol (T_{i+1} is accepted, YOHO_ICP_CONVERGED; a negative tol never stops);
 * i + 1 = iters (YOHO_ICP_ITERS).  T_out, info (2) int32 = {iterations made, reason}, npairs (iters) int32 / rmse (iters) f64 with
 * -1 / -1.0 for the iterations not made: as yoho_icp_refine.  0 <= iters <= YOHO_ICP_MAX_ITERS (0: T_out = T_in, info = {0,
 * YOHO_ICP_ITERS}; npairs / rmse may then be NULL); 1 <= Ns, Nt <= YOHO_REFINE_MAX_POINTS; max_dist finite and > 0; tol not NaN.
 * The grid over tgt is built once per call; all iterations are queued at once and the ones behind a stop return at once. */
int yoho_icp_plane(yoho_ctx* ctx, const float* src, int Ns, const float* tgt, int Nt, const float* tgt_normals, const double* T_in,
                   float max_dist, int iters, double tol, double* T_out, int32_t* npairs, double* rmse, int32_t* info, void* stream);

#ifdef __cplusplus
}
#endif

#endif
