/* Training-set generation entries of libyoho_hip.so: what the reference's YOHO_Trainset.py does on the data path beside the
 * backbone passes
 *
 *   yoho_radius_pairs       trainset_create.PCA_keys_sample   YOHO_Trainset.py:57-61   (ground-truth correspondences of two key sets)
 *   yoho_trainset_gather    trainset_create.trainset          YOHO_Trainset.py:222-228 (rows of the rotated feature blocks -> batches)
 *
 * The entries live in a header of their own beside yoho_hip.h and yoho_knn.h (whose symbol sets are pinned entry by entry by
 * tests/test_abi.py, tests/test_gpu_abi.py and tests/test_knn_cpu.py); tests/test_trainset_cpu.py and tests/test_gpu_trainset.py
 * keep the same invariants for this one.  The conventions of yoho_hip.h hold: device pointers unless said otherwise, contiguous
 * row-major, asynchronous on `stream`, YOHO_E* codes, yoho_last_error() naming the entry.
 */
#ifndef YOHO_TRAINSET_H
#define YOHO_TRAINSET_H

#include "yoho_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define YOHO_RADIUS_MAX_POINTS (1 << 20)   /* largest Na / Nb of yoho_radius_pairs */

/* every pair (i, j) of a (Na,3) f32 and b (Nb,3) f32 closer than `radius`, in np.where's order (ascending i, then ascending j):
 *   dx = a_i.x - b_j.x (same for y, z), d2 = (dx*dx + dy*dy) + dz*dz, d = sqrtf(d2) correctly rounded, pair iff d < radius
 * all in f32 without contraction - the entry's own contract (tests/trainset_ref.py restates it in numpy).  It is the reference's
 * np.where(torch.norm(a[:,None]-b[None], dim=-1) < radius) wherever no distance is within a last bit of the radius (torch.norm's
 * summation order is not specified).  A NaN never pairs; radius <= 0 gives no pairs; a NaN radius is YOHO_EINVAL.
 * count: one device int64 that ALWAYS receives the full number M of pairs.  pairs (capacity,2) int64 receives the first
 * min(M, capacity) pairs of that order and nothing beyond them is written; pairs may be NULL with capacity = 0 (count only).
 * Na, Nb <= YOHO_RADIUS_MAX_POINTS; a count of 0 is valid (M = 0, a / b may then be NULL).  a, b 4-byte aligned (rows of 12 bytes,
 * as yoho_nn_search with D = 3), pairs and count 8-byte aligned.  The result depends on nothing but the arguments: not on the
 * workspace contents or the call count.  The workspace holds 12 bytes per row of a; a request refused under YOHO_WS_LIMIT_MB
 * returns YOHO_ENOMEM and leaves the context usable.  Sized for key sets of a few thousand points: the row offsets are scanned by one
 * workgroup (ceil(Na / 1024) rows per thread, serial), which is right up to the limit but not tuned for Na near it. */
int yoho_radius_pairs(yoho_ctx* ctx, const float* a, int Na, const float* b, int Nb, float radius, int64_t* pairs, int64_t capacity,
                      int64_t* count, void* stream);

/* out[b] = feats[rot[b], key[b]] for b < B: feats (nr,kn,32,60) f32 and out (B,32,60) f32 on the device, 16-byte aligned; rot_host,
 * key_host (B) int64 HOST arrays, read before the call returns (they travel in kernel arguments).  Rows of 7680 bytes are copied
 * unchanged.  An index outside [0, nr) / [0, kn) is YOHO_EINVAL naming the first bad one, and nothing is launched.  B = 0 is valid. */
int yoho_trainset_gather(yoho_ctx* ctx, const float* feats, int nr, int kn, const int64_t* rot_host, const int64_t* key_host, int B,
                         float* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
