/* Keypoint selection on the device: exact farthest-point sampling
 *
 *   yoho_fps                k points of a cloud, each the one farthest from all picked before it
 *
 * The reference draws its keypoints uniformly over the scan points (simple_yoho/yoho_extract.py, np.random.permutation), so they
 * follow the scan's density; farthest-point sampling spreads them over the surface instead.  The entry lives in a header of its own
 * beside yoho_hip.h (whose symbol set is pinned entry by entry by tests/test_abi.py and tests/test_gpu_abi.py);
 * tests/test_keypoints_cpu.py and tests/test_gpu_keypoints.py keep the same two invariants for this one.  The conventions of
 * yoho_hip.h hold: device pointers, contiguous row-major, asynchronous on `stream`, no host read, YOHO_E* codes, yoho_last_error()
 * naming the entry.  It mirrors no file of the reference: tests/keypoints_ref.py restates it in numpy float32.
 */
#ifndef YOHO_KEYPOINTS_H
#define YOHO_KEYPOINTS_H

#include "yoho_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define YOHO_FPS_MAX_POINTS (1 << 22)   /* largest m */
#define YOHO_FPS_ONE_WG_MAX 16384       /* largest m of YOHO_FPS_ONE_WG: 1024 threads with 16 points each in registers */
#define YOHO_FPS_BLOCK_POINTS 1024      /* points one workgroup of YOHO_FPS_PER_PICK owns */
#define YOHO_FPS_AUTO 0                 /* YOHO_FPS_ONE_WG when m <= YOHO_FPS_ONE_WG_MAX, else YOHO_FPS_PER_PICK */
#define YOHO_FPS_ONE_WG 1               /* one launch of one 1024-thread workgroup runs all k picks */
#define YOHO_FPS_PER_PICK 2             /* any m: one launch per pick and a tail launch, no workgroup ever waits for another */

/* pts (m,3) f32, idx (k) int64, dist2 (k) f32 or NULL.
 *   PICKS.  idx[0] = start.  With D(i, j) = (dx dx + dy dy) + dz dz over d = pts[i] - pts[j] in fp32, every operation rounded and none
 *   fused - yoho_nn_search's D = 3 YOHO_DIST_SQUARE_L2 arithmetic, bit for bit - and the running minimum
 *     r_s(i) = min over t <= s of D(i, idx[t]),   r_s(i) = -1 once i is picked (a value below every real one),
 *   idx[s + 1] is the i with the largest r_s(i), the lowest such i among equals.  The k picks are therefore k distinct indices, in a
 *   cloud of duplicates too, and a numpy float32 restatement gives the same indices exactly.
 *   dist2[0] = +inf; dist2[s] = r_{s-1}(idx[s]), the pick's running minimum at the moment it was chosen: after s picks every point
 *   of the cloud lies within sqrt(dist2[s]) of a pick, and dist2[1:] does not increase.
 * The result depends on nothing but the arguments: not on `path`, the workspace contents, the call count or the stream.
 * 0 <= m <= YOHO_FPS_MAX_POINTS; 0 <= k <= m; 0 <= start < m when k > 0; path one of the three above, YOHO_FPS_ONE_WG only with
 * m <= YOHO_FPS_ONE_WG_MAX; pts / dist2 4-byte, idx 8-byte aligned.  k = 0 is valid and launches nothing.  A NaN or infinite
 * coordinate is outside what is pinned: the call still ends and still returns k distinct indices in [0, m).  YOHO_FPS_PER_PICK
 * takes 4 m + 48 ceil(m / YOHO_FPS_BLOCK_POINTS) bytes of the context workspace; a request refused under YOHO_WS_LIMIT_MB returns
 * YOHO_ENOMEM and leaves the context usable.  YOHO_FPS_ONE_WG takes none. */
int yoho_fps(yoho_ctx* ctx, const float* pts, int m, int k, int start, int path, int64_t* idx, float* dist2, void* stream);

#ifdef __cplusplus
}
#endif

#endif
