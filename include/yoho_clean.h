/* Clean scans on the device: the k nearest neighbours of a 3-D point inside a radius, and the outlier filter built on them
 *
 *   yoho_knn_within             per query: the number of targets inside a radius, exact, and the k nearest of them
 *   yoho_statistical_outliers   per point: the mean distance to its k nearest neighbours inside a radius; keep = below mean + ratio * sigma
 *
 * A header of their own beside yoho_refine.h and yoho_plane.h, whose symbol sets are pinned by their tests; tests/test_clean_cpu.py and
 * tests/test_gpu_clean.py keep the same invariants for this one.  The conventions, YOHO_REFINE_MAX_POINTS and THE SUM are
 * yoho_refine.h's: device pointers, contiguous row-major, asynchronous on `stream`, YOHO_E* codes, yoho_last_error() naming the entry;
 * float / int32 arrays 4-byte aligned, double / int64 arrays 8-byte.  Neither entry mirrors a file of the reference: tests/clean_ref.py
 * restates both in numpy.  Every result depends on nothing but the arguments (not on yoho_set_nn_grid / yoho_set_nn_prefilter, the
 * workspace contents or the call count); a workspace request refused under YOHO_WS_LIMIT_MB returns YOHO_ENOMEM and leaves the context
 * usable; no entry reads anything back to the host or uses a float atomic.
 */
#ifndef YOHO_CLEAN_H
#define YOHO_CLEAN_H

#include "yoho_refine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define YOHO_KNN3_MAX 32   /* largest k of both entries */

/* for every row of q (Nq,3) f32 the rows of tgt (Nt,3) f32 strictly inside max_dist.  The candidates of row i are yoho_nn_within's: the j
 * with d2 = ((dx^2 + dy^2) + dz^2) < gate2 = max_dist * max_dist rounded to f32, every operation rounded to f32 and none fused.  With
 * skip_same_row != 0, j = i is no candidate: meant for q == tgt, it needs Nq == Nt; the copies of a point at other rows stay candidates
 * at d2 = 0.
 *   count[i] (int32) = the number of candidates, exact and not capped at k.
 *   Row i of idx (Nq,k) int64 / d2 (Nq,k) f32 = the min(k, count[i]) candidates with the smallest pair (d2, j), ascending; the rest of
 *   the row is -1 / +inf.
 * A NaN or infinite query has count 0; a non-finite target is nobody's neighbour; a d2 equal to the gate is out.  Column 0 with
 * skip_same_row = 0 is yoho_nn_within's (idx, d2) bit for bit; a row whose k-th d2 is below the gate is, for k <= YOHO_KNN_MAX,
 * yoho_knn_search(D = 3, YOHO_DIST_SQUARE_L2)'s.
 * Any subset of idx, d2, count may be NULL, all three may not; with idx and d2 both NULL nothing but the count is formed.
 * 1 <= k <= YOHO_KNN3_MAX (k may exceed Nt); Nq = 0 is valid and launches nothing (no pointer is looked at then); Nt >= 1; Nq, Nt <=
 * YOHO_REFINE_MAX_POINTS; max_dist finite and > 0.  Cost: yoho_nn_within's counting sort of tgt into cells of side max_dist (1 + 2^-10),
 * then one lane per query over the distinct buckets of the 27 cells around it, the k best kept sorted in registers: sized for radii of
 * a few point spacings, correct (not fast) for a gate that holds the whole cloud. */
int yoho_knn_within(yoho_ctx* ctx, const float* q, int Nq, const float* tgt, int Nt, float max_dist, int k, int skip_same_row, int64_t* idx,
                    float* d2, int32_t* count, void* stream);

/* statistical outlier removal of pts (N,3) f32.  For point i, with yoho_knn_within(pts, pts, max_dist, k, skip_same_row = 1):
 *   count[i] its candidates, found_i = min(k, count[i]); the point is VALID iff found_i >= min_found (a point with a NaN or infinite
 *   coordinate has count 0: never valid).
 *   m_i = (the sum, from +0.0 in ascending (d2, j) order, of sqrt((double)d2) over the found_i nearest) / found_i, in f64;
 *   mean_dist[i] = m_i, NaN for an invalid point.
 *   n_valid = the number of valid points; mu = SUM(m) / n_valid; sigma = sqrt(SUM((m - mu)^2) / (n_valid - 1)), the difference and the
 *   square rounded, none fused: two passes of THE SUM over i, an invalid point contributing +0.0.  sigma = 0 for n_valid < 2; mu = 0 for
 *   n_valid = 0.  thr = mu + std_ratio * sigma, the product and the sum rounded.
 *   keep[i] (uint8) = 1 iff the point is valid and m_i <= thr, else 0; n_keep (int32, one) = their number.
 *   stats (4) f64 = {n_valid, mu, sigma, thr}.
 * A point with fewer than min_found neighbours inside the gate is an outlier by definition, whatever the others do.  mean_dist and count
 * may be NULL.  1 <= N <= YOHO_REFINE_MAX_POINTS; max_dist finite and > 0; 1 <= k <= YOHO_KNN3_MAX; min_found >= 1 (above k: nothing is
 * valid); std_ratio not NaN (0 and negative values are taken as they are).  The (N,k) lists are never written: one walk per point, two
 * more passes over N doubles. */
int yoho_statistical_outliers(yoho_ctx* ctx, const float* pts, int N, float max_dist, int k, int min_found, double std_ratio, double* mean_dist,
                              int32_t* count, uint8_t* keep, double* stats, int32_t* n_keep, void* stream);

#ifdef __cplusplus
}
#endif

#endif
