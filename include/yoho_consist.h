/* Geometric-consistency consensus: hypotheses from the match list alone
 *
 *   yoho_consistency_graph      which pairs of matches preserve their distance: a bit matrix and its row degrees
 *   yoho_sc2_scores             per match, the common compatible neighbours summed over its compatible pairs (second-order compatibility)
 *   yoho_consensus_hypotheses   greedy seeds by that score, one per cluster, each cluster's matches fitted by THE KABSCH STEP
 *
 * Every other transform of this library starts in PartII's per-match rotation (yoho_hyp_from_quat, yoho_c_ransac*); the entries behind
 * the vote (yoho_refine.h, yoho_plane.h, yoho_verify.h) polish or choose among those.  These three propose hypotheses from the matched
 * keypoints alone: inlier matches preserve their pairwise distances, outliers do so by chance only.  The output, (K,3,4) f64 on the
 * device, is what yoho_o_score, yoho_verify_hypotheses and the refinement entries take.  A header of their own beside the other five,
 * whose symbol sets are pinned by their tests; tests/test_consist_cpu.py and tests/test_gpu_consist.py keep the same invariants for
 * this one.  The conventions, a transform T (3 x 4 row-major f64 [R|t], k0 ~ R k1 + t), THE SUM and THE KABSCH STEP are
 * yoho_refine.h's: device pointers, contiguous row-major, asynchronous on `stream`, YOHO_E* codes, yoho_last_error() naming the entry;
 * double / uint64 arrays 8-byte aligned, int32 arrays 4-byte.  None of them mirrors a file of the reference: tests/consist_ref.py
 * restates all three in numpy.  Every result depends on nothing but the arguments (not on the workspace contents or the call count);
 * a workspace request refused under YOHO_WS_LIMIT_MB returns YOHO_ENOMEM and leaves the context usable; no entry reads anything back
 * to the host or uses a float atomic.  Graph and scores are integers and bits: exact, not approximations.
 *
 * W = (M + 63) / 64 is the number of 64-bit words of a row of the graph.
 */
#ifndef YOHO_CONSIST_H
#define YOHO_CONSIST_H

#include "yoho_refine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define YOHO_CONSIST_MAX_M (1 << 14)       /* largest number of matches */
#define YOHO_CONSIST_MAX_K 64              /* largest number of hypotheses; YOHO_VERIFY_MAX_K, so a result chains into the verification */

/* the compatibility graph of the matches k0, k1 (M,3) f64, matched keypoints as yoho_refit_matches takes them.  For i != j
 *   a = sqrt((dx dx + dy dy) + dz dz) over d = k0[i] - k0[j], b likewise over k1[i] - k1[j], every operation rounded to f64, none fused;
 *   C[i][j] = |a - b| < tol && a >= min_len && b >= min_len;   C[i][i] = 0.
 * A comparison with a NaN is false: a match with a NaN or infinite coordinate is compatible with nobody.  C IS SYMMETRIC BY
 * CONSTRUCTION: x - y = -(y - x) exactly in IEEE arithmetic and a square loses the sign, so (a, b) of (i, j) are (a, b) of (j, i) bit
 * for bit - the kernel computes both triangles and no pass mirrors one into the other.  f64 sqrt is correctly rounded on the device,
 * as yoho_icp_refine's rmse already assumes.  bits (M, W) uint64: bit j % 64 of word j / 64 of row i holds C[i][j]; the bits of the
 * last word at j >= M are 0.  deg (M) int32: the popcount of row i.  1 <= M <= YOHO_CONSIST_MAX_M; tol finite and > 0; min_len
 * finite and >= 0 (0 lets duplicated keypoints, a = b = 0, be compatible; any positive value keeps them out). */
int yoho_consistency_graph(yoho_ctx* ctx, const double* k0, const double* k1, int M, double tol, double min_len, uint64_t* bits, int32_t* deg,
                           void* stream);

/* second-order compatibility from a graph: with row_i the W words of bits,
 *   S[i][j] = C[i][j] ? popcount(row_i & row_j) : 0   (the matches compatible with both ends of a compatible pair),
 *   s2[i] = SUM_j S[i][j], int32: at most (M - 1)(M - 2) < 2^28 at the limit, so it cannot overflow and fits beside an index in a
 *   64-bit key.
 * Integers only: exact, and independent of any order.  S is never formed (at the limit it would take 1 GB): a row walks its own set
 * bits only, M deg W word operations in all.  bits is read as given: nothing is checked, the result is that of the given words, except that the bits
 * of a row's last word at j >= M (0 as yoho_consistency_graph leaves them) are ignored.  1 <= M <= YOHO_CONSIST_MAX_M. */
int yoho_sc2_scores(yoho_ctx* ctx, const uint64_t* bits, int M, int32_t* s2, void* stream);

/* up to K hypotheses from the graph, its scores and the matches.
 *   SEEDS.  Match i is alive iff s2[i] >= 1 (it sits in a triangle).  Up to K times: take the alive match with the largest s2, the
 *   smallest index among equals, record it in seeds[r], kill it and every alive j with C[seed][j] = 1 - one seed stands for one
 *   cluster, the role distinct_tol plays in yoho_verify_hypotheses.  Kc <= K rows are taken.
 *   SET of the seed s.  Smax = max_j S[s][j]; the members are s and every j with C[s][j] and 2 S[s][j] >= Smax: the matches that share at
 *   least half as many neighbours with the seed as its best partner does.  Integers only, no cap on the size.  sizes[r] = n, the number
 *   of members; n >= 2 (the seed and its best partner).
 *   FIT.  T_out[r] = THE KABSCH STEP over the set with a = k0, b = k1, the sums over m = 0 .. M - 1 in index order (THE SUM; a non-member
 *   contributes +0.0): the step yoho_refit_matches takes over an inlier set, the same device code.  When n < 3 (the seed's best partner
 *   shares neighbours with it that share few themselves) or the set has rank below 2, all 12 entries of the row are NaN and sizes[r] =
 *   -n: yoho_o_score counts 0 inliers for such a row and yoho_eval_transforms leaves all its points unpaired.
 *   ROWS BEHIND Kc.  seeds = -1, sizes = 0, T_out row = [I | 0].  info (2) int32 = {Kc, M}.  Kc stays on the device: K rows are launched
 *   and the ones behind Kc return at once.
 * T_out (K,3,4) f64, seeds (K), sizes (K) int32.  1 <= K <= YOHO_CONSIST_MAX_K; 1 <= M <= YOHO_CONSIST_MAX_M.  bits / s2 are meant to be
 * the outputs of the two entries above for the same k0, k1; nothing is checked: the result is that of the given graph and scores (a set
 * bit on the diagonal or an asymmetric graph is used as it stands, s2 only orders the seeds and decides who is alive). */
int yoho_consensus_hypotheses(yoho_ctx* ctx, const double* k0, const double* k1, int M, const uint64_t* bits, const int32_t* s2, int K, double* T_out,
                              int32_t* seeds, int32_t* sizes, int32_t* info, void* stream);

#ifdef __cplusplus
}
#endif

#endif
