/* Salient keypoints: ISS saliency of a 3-D cloud and Poisson-disk thinning in the order of a caller's priority
 *
 *   yoho_iss_saliency           per point: the eigenvalues of the covariance of its neighbourhood and the intrinsic-shape-signature
 *                               response - the smallest eigenvalue where the three are well apart, NaN elsewhere
 *   yoho_disk_sample_prio       yoho_disk_sample (yoho_disk.h) with the priority handed in: higher priority first, NaN last, equal
 *                               priorities in that entry's hashed order; its first round is non-maximum suppression
 *
 * A header of its own beside yoho_disk.h and yoho_plane.h, whose symbol sets are pinned by their tests; tests/test_salient_cpu.py and
 * tests/test_gpu_salient.py keep the same invariants for this one.  The conventions, YOHO_REFINE_MAX_POINTS and the codes are
 * yoho_refine.h's: device pointers, contiguous row-major, asynchronous on `stream`, YOHO_E* codes, yoho_last_error() naming the entry
 * and the argument; float / int32 arrays 4-byte aligned, double arrays 8-byte aligned.  The entries mirror no file of the reference:
 * tests/salient_ref.py restates them in numpy.  A result depends on nothing but the arguments (not on the schedule, the workspace
 * contents, the stream, yoho_set_nn_grid / yoho_set_nn_prefilter or the call count); a workspace request refused under
 * YOHO_WS_LIMIT_MB returns YOHO_ENOMEM and leaves the context usable; the entries read nothing back to the host, use no float atomic
 * and write every workspace byte before they read it.
 */
#ifndef YOHO_SALIENT_H
#define YOHO_SALIENT_H

#include "yoho_refine.h"

#define YOHO_SALIENT_MAX_ROUNDS 64

#ifdef __cplusplus
extern "C" {
#endif

/* ISS saliency of pts (N,3) f32 at `radius`.
 *   NEIGHBOURS.  yoho_estimate_normals' (yoho_plane.h): the j, i itself included, with d2 = ((dx^2 + dy^2) + dz^2) < gate2 =
 *   radius * radius rounded to f32, every operation rounded to f32 and none fused (yoho_nn_within's arithmetic); every bucket of the
 *   grid is walked once, so count is exact.  A row with a NaN or infinite coordinate has count 0 and is nobody's neighbour.
 *   COVARIANCE.  In f64, in one pass about the point itself: with d_j = p_j - p_i, n = count, S1 = SUM d_j, S2 = SUM d_j d_j^T,
 *   C = (S2 - S1 S1^T / n) / n.  The division by n makes the response comparable across densities.  The order of the sums is the
 *   grid walk's: the same from call to call, but not part of the contract - a reference is met within a bound, not bit for bit.
 *   count (N) int32      the neighbours of the row.
 *   eig (N,3) f64        the eigenvalues of C by an f64 Jacobi iteration, each clamped at 0 from below, ascending: l1 <= l2 <= l3;
 *                        (0, 0, 0) for a row with count 0.  May be NULL.
 *   prio (N) f32         a row is eligible iff count >= min_nbrs and l2 < gamma21 * l3 and l1 < gamma32 * l2, each product one
 *                        rounded f64 multiply on the clamped values; prio = (float) l1 for an eligible row and the quiet NaN
 *                        0x7fc00000 otherwise.  prio is a function of (eig[i], count[i], min_nbrs, gamma21, gamma32) alone, bit for
 *                        bit.  A row with l3 = 0 (copies of one point) or l2 = 0 (collinear neighbours) is never eligible.
 * 1 <= N <= YOHO_REFINE_MAX_POINTS; radius finite and > 0; min_nbrs >= 3; gamma21 and gamma32 finite and in (0, 1]; pts, count and
 * prio required.  Cost: yoho_estimate_normals' - the counting sort of pts into cells of side radius (1 + 2^-10) and one launch, one
 * lane per point. */
int yoho_iss_saliency(yoho_ctx* ctx, const float* pts, int N, float radius, int min_nbrs, double gamma21, double gamma32, int32_t* count,
                      double* eig, float* prio, void* stream);

/* Poisson-disk thinning of pts (N,3) f32 with radius `radius` in the order of prio (N) f32.  NEIGHBOURS, THE SET, ROUNDS, state,
 * n_out, the argument ranges (rounds up to YOHO_SALIENT_MAX_ROUNDS = YOHO_DISK_MAX_ROUNDS) and the launch structure are
 * yoho_disk_sample's (yoho_disk.h) with key64 in the place of key.  Two things differ.
 *   PRIORITY.  ord(p) is the monotone map of an f32 to uint32: take the bits; if the sign bit is set flip all bits, else set the sign
 *   bit; every NaN maps to 0, below -inf (-0.0 comes below +0.0).  With mix32 of yoho_disk.h,
 *       key64(i) = ((uint64) (~ord(prio[i])) << 32) | mix32((uint32) i ^ seed)
 *   and row j precedes row i iff key64(j) < key64(i): higher priority first, NaN last, equal priorities in the hashed order of
 *   yoho_disk.h.  mix32 is a bijection, so the keys of distinct rows are distinct.
 *       (i, seed, prio bits) -> key64:   (0, 0, 0x3f800000) -> 0x407fffff00000000      (1, 0, 0xbf800000) -> 0xbf800000688990c0
 *                                        (12345, 0, 0x7fc00000) -> 0xffffffff912efcf7  (2048, 12345, 0x00000000) -> 0x7fffffff72c087ec
 *   With a constant prio every output byte is yoho_disk_sample's: the state after every round and n_out.
 *   START.  resume = 0 starts as yoho_disk_sample does.  resume = 1 starts from the `state` handed in, whoever wrote it: a byte 0 is
 *   undecided, any other byte is decided and copied through; a row with a NaN or infinite coordinate handed in as 0 is set to 2.
 *   resume = 1 is both the resumption of an unfinished call and the caller's mask: rows handed in as 2 are never kept and never
 *   block anybody.
 * The first synchronous round from a fresh start is non-maximum suppression: a row is kept by round 1 iff no neighbour precedes it.
 * k rounds in one call and the same k rounds split over resumed calls leave the same bytes; every output is a function of the
 * arguments alone.  prio is required like every other pointer, and 4-byte aligned.  Cost: yoho_disk_sample's, and one 64-bit key per
 * row in the workspace, written by the init launch and loaded beside a neighbour's state. */
int yoho_disk_sample_prio(yoho_ctx* ctx, const float* pts, int N, float radius, const float* prio, uint32_t seed, int rounds, int resume,
                          uint8_t* state, int32_t* n_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
