/* Cluster scans on the device: exact DBSCAN labels of a 3-D cloud
 *
 *   yoho_dbscan                 per point: the density cluster it belongs to, numbered deterministically, or noise
 *
 * A header of its own beside yoho_clean.h, whose symbol set is pinned by its tests; tests/test_cluster_cpu.py and
 * tests/test_gpu_cluster.py keep the same invariants for this one.  The conventions, YOHO_REFINE_MAX_POINTS and the codes are
 * yoho_refine.h's: device pointers, contiguous row-major, asynchronous on `stream`, YOHO_E* codes, yoho_last_error() naming the entry
 * and the argument; float / int32 arrays 4-byte aligned.  The entry mirrors no file of the reference: tests/cluster_ref.py restates it
 * in numpy.  The result depends on nothing but the arguments (not on the schedule, the workspace contents, the stream,
 * yoho_set_nn_grid / yoho_set_nn_prefilter or the call count); a workspace request refused under YOHO_WS_LIMIT_MB returns YOHO_ENOMEM
 * and leaves the context usable; the entry reads nothing back to the host, uses no float atomic and writes every workspace byte before
 * it reads it.
 */
#ifndef YOHO_CLUSTER_H
#define YOHO_CLUSTER_H

#include "yoho_refine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* DBSCAN of pts (N,3) f32 with radius eps and density min_pts.
 *   NEIGHBOURS.  The neighbours of row i are the candidates of yoho_knn_within(pts, pts, eps, skip_same_row = 1) (yoho_clean.h): the
 *   j != i with d2 = ((dx^2 + dy^2) + dz^2) < gate2 = eps * eps rounded to f32, every operation rounded to f32 and none fused.  The
 *   relation is symmetric in f32 (a difference and its negative round alike).  count[i] (int32) = their number, bit for bit that
 *   entry's count.  A row with a NaN or infinite coordinate has count 0, is nobody's neighbour and is never core.  A d2 equal to the
 *   gate is out; the copies of a point at other rows are neighbours at d2 = 0.
 *   CORE.  core[i] (uint8) = 1 iff the row is finite and count[i] + 1 >= min_pts: the point counts itself, as in Open3D and
 *   scikit-learn.  min_pts = 1 makes every finite point core, which gives plain Euclidean cluster extraction (connected components
 *   of the neighbour graph).
 *   CLUSTERS.  A cluster is a connected component of the graph whose vertices are the core rows and whose edges join core rows that
 *   are neighbours.
 *   BORDER.  A finite row that is not core and has at least one core neighbour joins the cluster of the core neighbour with the
 *   smallest pair (d2, j).  A border point never joins two clusters into one.  Every other row that is not core is noise.
 *   NUMBERING.  The clusters are numbered 0 .. C-1 in ascending order of their lowest core row.
 *   labels[i] (N) int32  = the cluster of row i, -1 for noise.
 *   sizes (N) int32      : sizes[c] = the members of cluster c, core and border, for c < C, and 0 for c >= C; every element is written.
 *   n_out (3) int32      = {C, the number of core rows, the number of noise rows}.
 * labels and n_out are required; count, core and sizes may be NULL.  1 <= N <= YOHO_REFINE_MAX_POINTS; eps finite and > 0;
 * min_pts >= 1 (a value above N is valid and makes every row noise).  Cost: yoho_nn_within's counting sort of pts into cells of side
 * eps (1 + 2^-10), then three walks over the distinct buckets of the 27 cells around a row - the count, one pass over the edges that
 * unites the trees of neighbouring core rows (the walk of the core rows), the nearest core neighbour of the rows that are not core -
 * and two passes over N integers; the number of launches does not depend on N.  Sized for radii of a few point spacings, correct
 * (not fast) for an eps that holds the whole cloud. */
int yoho_dbscan(yoho_ctx* ctx, const float* pts, int N, float eps, int min_pts, int32_t* labels, int32_t* count, uint8_t* core, int32_t* sizes,
                int32_t* n_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
