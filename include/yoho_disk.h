/* Spread keypoints in one pass: exact Poisson-disk thinning of a 3-D cloud on the device
 *
 *   yoho_disk_sample            per point: kept or dropped, so that no two kept points are closer than the radius and every point
 *                               has a kept point within it - the maximal set a greedy pass in a fixed priority order keeps
 *
 * A header of its own beside yoho_keypoints.h and yoho_cluster.h, whose symbol sets are pinned by their tests; tests/test_disk_cpu.py
 * and tests/test_gpu_disk.py keep the same invariants for this one.  The conventions, YOHO_REFINE_MAX_POINTS and the codes are
 * yoho_refine.h's: device pointers, contiguous row-major, asynchronous on `stream`, YOHO_E* codes, yoho_last_error() naming the entry
 * and the argument; float / int32 arrays 4-byte aligned.  The entry mirrors no file of the reference: tests/disk_ref.py restates it in
 * numpy.  The result depends on nothing but the arguments (not on the schedule, the workspace contents, the stream,
 * yoho_set_nn_grid / yoho_set_nn_prefilter or the call count); a workspace request refused under YOHO_WS_LIMIT_MB returns YOHO_ENOMEM
 * and leaves the context usable; the entry reads nothing back to the host, uses no float atomic and writes every workspace byte before
 * it reads it.
 */
#ifndef YOHO_DISK_H
#define YOHO_DISK_H

#include "yoho_refine.h"

#define YOHO_DISK_MAX_ROUNDS 64

#ifdef __cplusplus
extern "C" {
#endif

/* Poisson-disk thinning of pts (N,3) f32 with radius `radius`.
 *   NEIGHBOURS.  The neighbours of row i are the candidates of yoho_knn_within(pts, pts, radius, skip_same_row = 1) (yoho_clean.h):
 *   the j != i with d2 = ((dx^2 + dy^2) + dz^2) < gate2 = radius * radius rounded to f32, every operation rounded to f32 and none
 *   fused.  The relation is symmetric in f32 (a difference and its negative round alike).  A d2 equal to the gate is out; the copies
 *   of a point at other rows are neighbours at d2 = 0.  A row with a NaN or infinite coordinate has no neighbour and is nobody's.
 *   PRIORITY.  key(i) = mix32((uint32) i ^ seed), all in uint32 arithmetic modulo 2^32:
 *       x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
 *   Every step is invertible, so mix32 is a bijection and the keys of distinct rows are distinct.
 *       (i, seed) -> key:   (0, 0) -> 0x00000000   (1, 0) -> 0x688990c0   (12345, 0) -> 0x912efcf7   (2048, 12345) -> 0x72c087ec
 *   THE SET.  K is the unique set with: i in K iff row i is finite and no neighbour j with key(j) < key(i) is in K - what a greedy
 *   pass over the finite rows in ascending key order keeps.  Two kept rows are never neighbours, and every finite row is kept or has
 *   a kept neighbour: the kept rows are at least `radius` apart and cover the finite rows with balls of that radius.
 *   ROUNDS.  state[i] (uint8) is 0 for a row not decided yet, 1 for a kept row, 2 for a dropped one.  resume = 0 starts from
 *   state[i] = 0 for a finite row and 2 for every other; resume = 1 starts from `state` as a previous call with the same pts, N,
 *   radius and seed left it.  A round is synchronous: every undecided row looks at the states of its neighbours of lower key AS THE
 *   PREVIOUS ROUND LEFT THEM, becomes 2 if one of them is 1, 1 if none of them is 0, and stays 0 otherwise; a decided row keeps its
 *   state.  The call runs rounds until no row is undecided or `rounds` of them have run.  The undecided row of lowest key is decided
 *   by every round, so ceil(N / rounds) calls always finish; a hashed priority on a scan needs 10 - 12 rounds.
 *   state (N) uint8      in (resume = 1) and out: the state after the last round that ran.
 *   n_out (3) int32      = {rows with state 1, rounds that ran in this call, rows with state 0}.
 * Every output is a function of (pts, N, radius, seed, rounds, and with resume = 1 the state handed in) alone, n_out[1] and the state
 * of an unfinished call included: k rounds in one call and the same k rounds split over resumed calls leave the same bytes.
 * 1 <= N <= YOHO_REFINE_MAX_POINTS; radius finite and > 0; 1 <= rounds <= YOHO_DISK_MAX_ROUNDS; resume 0 or 1; every pointer
 * required.  With resume = 1 a byte of `state` other than 0, 1, 2 is treated as decided and copied through.  Cost:
 * yoho_nn_within's counting sort of pts into cells of side radius (1 + 2^-10), then `rounds` launches that walk the undecided rows over the
 * 27 cells around it, of which those behind the last round that had work return at once, and a tail; the number of launches does
 * not depend on N.  Sized for radii of a few point spacings, correct (not fast) for a radius that holds the whole cloud. */
int yoho_disk_sample(yoho_ctx* ctx, const float* pts, int N, float radius, uint32_t seed, int rounds, int resume, uint8_t* state,
                     int32_t* n_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
