/* The fused scene: poses and fragments into one cloud
 *
 *   yoho_fuse_clouds    K fragments under K poses into the voxel means of the scene: per voxel the mean point, the mean normal, the
 *                       number of points and the number of distinct FRAGMENTS that fed it, and per input point the voxel row it went to
 *
 * Multiway registration (yoho_multiway.h, yoho_amd/multiway.py) ends at F poses; what a scan of a room is for is one model of the room.
 * This entry is the step between: a sort of the points by voxel and a reduction per voxel.  The fragment count is what a multiway
 * result needs as a filter - a falsely placed fragment, or sensor noise, leaves voxels that only one fragment supports - and what a
 * unique / index_add of a tensor library cannot give; nor does that promise the same bytes twice, its sums being float atomics.  A header
 * of its own beside yoho_multiway.h, whose symbol set is pinned by its tests; tests/test_fuse_cpu.py and tests/test_gpu_fuse.py keep
 * the same invariants for this one.  The conventions, YOHO_REFINE_MAX_POINTS and a transform T (3 x 4 row-major f64 [R|t]) are
 * yoho_refine.h's: device pointers unless said otherwise, contiguous row-major, asynchronous on `stream`, YOHO_E* codes,
 * yoho_last_error() naming the entry; float and int32 arrays 4-byte aligned (rows of 12 bytes), double and int64 arrays 8-byte.  The
 * entry mirrors no file of the reference: tests/fuse_ref.py restates it in numpy.  Every result depends on nothing but the arguments
 * (not on the workspace contents, the call count or the stream); a workspace request refused under YOHO_WS_LIMIT_MB returns YOHO_ENOMEM
 * and leaves the context usable; the entry reads nothing back to the host and uses no float atomic.
 */
#ifndef YOHO_FUSE_H
#define YOHO_FUSE_H

#include "yoho_refine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define YOHO_FUSE_MAX_K 1024                 /* fragments per call */
#define YOHO_FUSE_MAX_POINTS (1 << 26)       /* largest soff[K] */

/* src (S,3) f32 holds the K fragments one behind another, fragment k owning the rows soff[k] .. soff[k+1] - 1, each in its own frame;
 * T (K,3,4) f64: T[k] maps fragment k into the scene frame; nrm (S,3) f32 or NULL: a normal per row of src, in the fragment's frame.
 *
 * soff (K + 1) int32 is a HOST array, read before the call returns (the caller may free it then), as in yoho_edge_information:
 * soff[0] = 0, strictly increasing - every fragment has at least one point -, soff[k+1] - soff[k] <= YOHO_REFINE_MAX_POINTS,
 * soff[K] = S <= YOHO_FUSE_MAX_POINTS, 1 <= K <= YOHO_FUSE_MAX_K.  It reaches the kernels by value, 64 fragments per launch; the
 * fragment number of every point is kept in the workspace.
 *
 * THE POINT.  Row e of src (the GLOBAL row) in fragment k becomes q_e = ((r0 sx + r1 sy) + r2 sz) + t per coordinate under T[k], in
 * f64, each operation rounded, none fused (yoho_icp_refine's arithmetic), and is KEPT in f64.  With inv = 1.0 / voxel in f64 its cell
 * is c = floor(q inv) per axis (the product rounded once).  The point is OUTSIDE iff some c is not inside [-(2^20 - 1), 2^20 - 1]; a
 * NaN or infinite coordinate fails that test, so a non-finite T[k] puts the whole fragment k outside (the poses of the fragments that
 * multiway.register_scene did not reach are NaN: they drop out here).  Outside points contribute to nothing.
 *
 * THE VOXELS.  key = (cz + 2^20) << 42 | (cy + 2^20) << 21 | (cx + 2^20); a voxel is the set of inside points with one key, and the
 * voxels are taken in ascending key.  Per voxel, over its points in ASCENDING GLOBAL ROW, one after another, every sum starting from
 * +0.0:
 *   count  the number of points;      nfrag  the number of distinct fragments among them;
 *   s      SUM q (three f64 sums);    m      with nrm: SUM n', n' = (r0 nx + r1 ny) + r2 nz under T[k] (rotated, not translated).
 * A voxel is KEPT iff count >= min_count and nfrag >= min_frags (both >= 1).  The kept voxels are numbered 0 .. M - 1 in key order.
 *
 * THE OUTPUTS.  n_out: one device int64 that ALWAYS receives M.  Row r < min(M, capacity) of
 *   pts (capacity,3) f32      (float)(s / count) per coordinate, the quotient in f64
 *   out_nrm (capacity,3) f32  or NULL: (float)(m / len) per coordinate with len = sqrt((mx mx + my my) + mz mz) in f64; three zeros when
 *                             len is 0 or not finite.  Needs nrm.
 *   count, nfrag (capacity) int32
 * and nothing at or beyond row min(M, capacity) is written (yoho_radius_pairs' convention): with capacity = 0 all four may be NULL and
 * the call only counts; with capacity > 0 pts, count and nfrag are required.
 *   row_of (S) int32 or NULL: the kept row of the voxel of point e; -1 for an outside point and for a point of a voxel that is not
 *                             kept.  It is written for every e whatever capacity is, and may be >= capacity: what a caller needs to
 *                             carry colours or labels over to the fused rows.
 * YOHO_EINVAL, naming the argument: voxel not finite or <= 0; soff as above; K outside [1, YOHO_FUSE_MAX_K]; min_count or min_frags
 * < 1; capacity < 0; out_nrm without nrm; a required pointer NULL.  The workspace holds about 40 bytes per point. */
int yoho_fuse_clouds(yoho_ctx* ctx, const float* src, const int32_t* soff, int K, const double* T, const float* nrm, double voxel,
                     int min_count, int min_frags, float* pts, float* out_nrm, int32_t* count, int32_t* nfrag, int32_t* row_of,
                     int64_t capacity, int64_t* n_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
