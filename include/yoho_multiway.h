/* Multiway registration, the device half: the information matrix of registered pairs on the dense clouds
 *
 *   yoho_edge_information    K source fragments against ONE target fragment in one pass over one grid: per edge the pairs inside a
 *                            gate, their rmse and the 6 x 6 information matrix of the Redwood protocol
 *
 * Everything else the library registers is a pair.  A scene of F fragments is a graph: its edges are the registered pairs, and the
 * weight of an edge - in the pose-graph solve of yoho_amd/multiway.py as much as in the benchmark's own criterion
 * er' info er / info[0,0] <= 0.2^2 (RR_cal.computeTransformationErr) - is the information matrix of its overlap.  This entry produces
 * it; the solve has 6 F unknowns and stays on the host.  A header of its own beside yoho_verify.h, whose symbol set is pinned by its
 * tests; tests/test_multiway_cpu.py and tests/test_gpu_multiway.py keep the same invariants for this one.  The conventions,
 * YOHO_REFINE_MAX_POINTS, a transform T (3 x 4 row-major f64 [R|t], src = fragment 1 onto tgt = fragment 0) and THE SUM are
 * yoho_refine.h's: device pointers, contiguous row-major, asynchronous on `stream`, YOHO_E* codes, yoho_last_error() naming the entry;
 * float arrays 4-byte aligned (rows of 12 bytes), double arrays 8-byte, int32 arrays 4-byte.  The entry mirrors no file of the
 * reference: tests/multiway_ref.py restates it in numpy.  Every result depends on nothing but the arguments (not on yoho_set_nn_grid /
 * yoho_set_nn_prefilter, the workspace contents or the call count); a workspace request refused under YOHO_WS_LIMIT_MB returns
 * YOHO_ENOMEM and leaves the context usable; the entry reads nothing back to the host and uses no float atomic.
 */
#ifndef YOHO_MULTIWAY_H
#define YOHO_MULTIWAY_H

#include "yoho_refine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define YOHO_MULTIWAY_MAX_K 64                       /* sources (edges into one target) per call */
#define YOHO_MULTIWAY_MAX_SOURCE_POINTS (1 << 26)    /* largest soff[K] */

/* K edges into one target.  tgt (Nt,3) f32 is the target fragment (fragment 0 of every edge); src (S,3) f32 holds the K source
 * fragments one behind another, source k owning the rows soff[k] .. soff[k+1] - 1; T (K,3,4) f64 maps source k onto the target.
 *
 * soff (K + 1) int32 is a HOST array, read before the call returns (the caller may free it then): soff[0] = 0, strictly increasing -
 * every source has at least one point -, soff[k+1] - soff[k] <= YOHO_REFINE_MAX_POINTS, soff[K] = S <= YOHO_MULTIWAY_MAX_SOURCE_POINTS.
 * It is a host array because the launch shape and the map from workgroups to edges depend on it, and because that lets the entry
 * validate it exactly; it reaches the kernels by value, never through a copy from the caller's memory that could outlive the call.
 *
 * Row k, with n_k = soff[k+1] - soff[k] and the LOCAL index e = 0 .. n_k - 1 of source k's points:
 *   q_e = (float)(((r0 sx + r1 sy) + r2 sz) + t) per coordinate of src[soff[k] + e] under T[k], in f64, each operation rounded, none
 *   fused (yoho_icp_refine's arithmetic); point e is PAIRED iff yoho_nn_within(q, tgt, max_dist) gives it a partner j_e, d2_e that
 *   answer's d2 - yoho_eval_transforms' pairing exactly.
 *   npairs[k] = n, the number of paired points;
 *   rmse[k]   = sqrt(SUM(paired ? (double)d2_e : +0.0) / n), +inf when n = 0.
 * For any k these two are yoho_eval_transforms(src_k, tgt, T[k])'s npairs and rmse bit for bit.  With p = (double)tgt[j_e] ten more
 * sums are THE SUM over the local index e: s = SUM p (3) and Sxx, Sxy, Sxz, Syy, Syz, Szz = SUM of the rounded products px px,
 * px py, ...; block b of row k is the local elements 256 b .. 256 b + 255 whatever soff[k] is, and an unpaired element contributes
 * +0.0 to every sum.  A row therefore does not depend on where its source lies in src nor on the other rows.
 *   info[k] (6,6 row-major f64) = SUM G^T G with G = [I3 | -[p]x], the information matrix of Choi, Zhou, Koltun (CVPR 2015) in the
 *   variable order (translation, rotation) of RR_cal.computeTransformationErr and the Redwood .info files:
 *     [0:3,0:3] = n I
 *     [0:3,3:6] = ((0, s_z, -s_y), (-s_z, 0, s_x), (s_y, -s_x, 0)),  [3:6,0:3] its transpose
 *     [3:6,3:6] = ((Syy + Szz, -Sxy, -Sxz), (-Sxy, Sxx + Szz, -Syz), (-Sxz, -Syz, Sxx + Syy)), one rounded addition each.
 *   The entries are values: the sign of a zero is not part of the contract.  n = 0 gives the zero matrix.
 * A non-finite entry of T[k] makes the queries it reaches NaN or infinite and leaves them unpaired, as in yoho_eval_transforms.
 * 1 <= K <= YOHO_MULTIWAY_MAX_K; 1 <= Nt <= YOHO_REFINE_MAX_POINTS; max_dist finite and > 0.  The grid over tgt is built once per
 * call, whatever K is: a scene of F fragments builds F grids, not one per edge. */
int yoho_edge_information(yoho_ctx* ctx, const float* src, const int32_t* soff, int K, const float* tgt, int Nt, const double* T,
                          float max_dist, int32_t* npairs, double* rmse, double* info, void* stream);

#ifdef __cplusplus
}
#endif

#endif
