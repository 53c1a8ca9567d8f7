/* k-nearest-neighbour search of libyoho_hip.so: the k >= 2 branch of the reference's matcher
 *
 *   yoho_knn_search         modified_knn_matcher.find_knn_gpu   utils/knn_search.py:68-106,155-162
 *
 * The entry lives in a header of its own beside yoho_hip.h (whose symbol set is pinned entry by entry by tests/test_abi.py and
 * tests/test_gpu_abi.py); tests/test_knn_cpu.py and tests/test_gpu_knn.py keep the same two invariants for this one.  The conventions
 * of yoho_hip.h hold: device pointers, contiguous row-major, asynchronous on `stream`, YOHO_E* codes, yoho_last_error().
 */
#ifndef YOHO_KNN_H
#define YOHO_KNN_H

#include "yoho_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define YOHO_KNN_MAX 16   /* largest k */

/* for every row of src (Ns,D) the k rows of tgt (Nt,D) with the smallest distance: idx (Ns,k) int64 and dist (Ns,k) f32 (may be
 * NULL), each row sorted ascending by the pair (fp32 distance as returned, target index).  The distance is yoho_nn_search's, bit for
 * bit: YOHO_DIST_SQUARE_L2 sum_f (s_f - t_jf)^2, YOHO_DIST_L2 sqrt(that + 1e-7) correctly rounded - two targets whose ROUNDED
 * distances are equal tie (the lower index first) even when their squared distances differ.  This is torch.topk(-pdist, k) of the
 * reference wherever a row's k + 1 smallest distances are distinct (torch leaves the order of equal values open).
 * D = 32 (torch-CPU summation order) or 3; 1 <= k <= YOHO_KNN_MAX and k <= Nt (torch.topk refuses k > Nt too); pointers aligned as
 * for yoho_nn_search.  Ns = 0 is valid and launches nothing.  Rows with NaN / inf still get k distinct indices in [0, Nt); NaN
 * distances sort last (the reference sorts them first: such rows are outside what is pinned).  The result depends on nothing but
 * the arguments: not on yoho_set_nn_prefilter / yoho_set_nn_grid, the workspace contents or the call count. */
int yoho_knn_search(yoho_ctx* ctx, const float* src, int Ns, const float* tgt, int Nt, int D, int dist_type, int k,
                    int64_t* idx, float* dist, void* stream);

#ifdef __cplusplus
}
#endif

#endif
