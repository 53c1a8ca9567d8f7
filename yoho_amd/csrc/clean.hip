// k nearest neighbours inside a radius and the statistical outlier filter (include/yoho_clean.h).  Compiled with -ffp-contract=off like
// refine.hip (yoho_amd/build.py).  The cell-sorted grid comes from rfgrid.hip / rfgrid.h (THE GRID, THE QUERY's exactness argument),
// the fixed-order f64 sums from rffit.h (THE SUMS); both carry over unchanged.
//
//   cl_knn_kernel<CAP>     yoho_knn_within: one lane per query over the distinct buckets of the 27 cells around it; CAP = 0 counts only
//   cl_stat_kernel<CAP>    yoho_statistical_outliers: the same walk without the row itself, m_i, first-pass partial sums {n, SUM m}
//   cl_mean_kernel         one wave: n_valid, mu
//   cl_var_kernel          the partial sums of (m - mu)^2
//   cl_thr_kernel          one wave: sigma, thr
//   cl_keep_kernel         keep[i], n_keep
//
// THE WALK is rfgrid.h's rf_walk_each (THE DISTINCT BUCKETS): every bucket of the 27 cells around a query is walked once, so the count
// is exact, and the loop over the buckets is not unrolled, because the functor here holds the insertion chain below.
//
// THE LIST.  The k best are packed keys nn_key(d2 bits, j) (nnmath.h), kept sorted ascending in CAP registers; d2 >= +0, so the order of the
// integers is the contract's order of (d2, j) - matchf.hip's packing.  An empty place holds NN_KEY_EMPTY, all ones, above every key
// (a candidate's d2 is below the gate: finite, or below +inf).  A candidate is tested against the last place first; one that gets in
// replaces it and sinks through a chain of CAP - 1 compare-exchanges whose indices are all compile-time constants, so the list stays
// in registers (a register array indexed at run time goes to scratch).  k <= CAP: the list simply keeps CAP, the first k are the
// answer.  Three capacities, 8 / 16 / 32, chosen from k on the host.  The result does not depend on the order in which the
// candidates are met.
//
// THE FILTER never writes the (N, k) lists: a lane adds its own found_i square roots in list order.  m lives in the workspace (NaN for
// an invalid point), the two sums go through rf_block_sum / rf_slab_total, stats itself carries mu and thr from kernel to kernel, and
// n_keep is an integer atomic per block on a word that cl_mean_kernel has zeroed.  Every workspace byte is written (the grid build,
// cl_stat_kernel, the passes in order) before it is read; no float atomic anywhere.
//
// Registers (hipcc -O3, gfx950) and timings: tools/time_clean.py -> profiles/clean.md; no kernel of this file uses scratch.
#include "rfgrid.h"
#include "rffit.h"
#include "yoho_clean.h"
#include <cmath>

namespace yoho {

constexpr int CL_SLAB = 2;                     // doubles per slab row

template <int CAP>
__device__ __forceinline__ void cl_insert(u64 (&key)[CAP], u64 cand) {
    if (cand < key[CAP - 1]) {
        key[CAP - 1] = cand;
#pragma unroll
        for (int m = CAP - 1; m >= 1; --m) {
            const u64 a = key[m - 1], b = key[m];
            const bool swap = b < a;
            key[m - 1] = swap ? b : a;
            key[m] = swap ? a : b;
        }
    }
}

// the candidates of q among the grid's points, row `self` left out (-1: none): their number; CAP > 0: the CAP smallest keys, ascending
template <int CAP>
__device__ __forceinline__ int cl_walk(const RfGrid& g, const float (&q)[3], int self, u64 (&key)[CAP > 0 ? CAP : 1], unsigned (*slots)[256]) {
    if constexpr (CAP > 0) {
#pragma unroll
        for (int m = 0; m < CAP; ++m) key[m] = NN_KEY_EMPTY;
    }
    int n = 0;
    rf_walk_each(g, q, self, slots, [&](float d2, int j) {
        ++n;
        if constexpr (CAP > 0) cl_insert<CAP>(key, nn_key(__float_as_uint(d2), (unsigned)j));
    });
    return n;
}

template <int CAP>
__global__ __launch_bounds__(256) void cl_knn_kernel(RfGrid g, const float* __restrict__ q, int Nq, int k, int skip, int64_t* __restrict__ idx,
                                                     float* __restrict__ d2, int32_t* __restrict__ count) {
    __shared__ unsigned slots[27][256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Nq) return;                                                  // no barrier below
    float qq[3];
    rf_load_row(q, i, qq);
    u64 key[CAP > 0 ? CAP : 1];
    const int n = cl_walk<CAP>(g, qq, skip ? i : -1, key, slots);
    if (count) count[i] = n;
    if constexpr (CAP > 0) {
#pragma unroll
        for (int m = 0; m < CAP; ++m) {
            if (m < k) {
                const bool there = key[m] != NN_KEY_EMPTY;
                if (idx) idx[(size_t)i * k + m] = there ? (int64_t)nn_key_index(key[m]) : (int64_t)-1;
                if (d2) d2[(size_t)i * k + m] = there ? nn_key_dist(key[m]) : __builtin_inff();
            }
        }
    }
}

// first pass: mws[i] = m_i (NaN: invalid), slab row = {valid points, SUM m} of the block
template <int CAP>
__global__ __launch_bounds__(256) void cl_stat_kernel(RfGrid g, const float* __restrict__ pts, int N, int k, int min_found, double* __restrict__ mws,
                                                      double* __restrict__ mean_dist, int32_t* __restrict__ count, double* __restrict__ slab) {
    __shared__ unsigned slots[27][256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    double v[2] = {0.0, 0.0};
    if (i < N) {
        float qq[3];
        rf_load_row(pts, i, qq);
        u64 key[CAP];
        const int n = cl_walk<CAP>(g, qq, i, key, slots);
        const int found = n < k ? n : k;
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < CAP; ++m)
            if (m < found) s = __dadd_rn(s, sqrt((double)nn_key_dist(key[m])));
        const bool valid = found >= min_found;                            // min_found >= 1: a non-finite point, count 0, is never valid
        const double mi = valid ? s / (double)found : __builtin_nan("");
        mws[i] = mi;
        if (mean_dist) mean_dist[i] = mi;
        if (count) count[i] = n;
        if (valid) { v[0] = 1.0; v[1] = mi; }
    }
    rf_block_sum<2>(v, slab + (size_t)blockIdx.x * CL_SLAB);
}

// one wave: stats[0] = n_valid, stats[1] = mu; n_keep = 0 for cl_keep_kernel's atomics
__global__ __launch_bounds__(64) void cl_mean_kernel(const double* __restrict__ slab, int nblk, double* __restrict__ stats, int32_t* __restrict__ n_keep) {
    __shared__ double tot[2];
    rf_slab_total<2>(slab, nblk, CL_SLAB, tot);
    __syncthreads();
    if (threadIdx.x == 0) {
        stats[0] = tot[0];
        stats[1] = tot[0] > 0.0 ? tot[1] / tot[0] : 0.0;
        *n_keep = 0;
    }
}

// second pass: slab row = {SUM (m - mu)^2} of the block
__global__ __launch_bounds__(256) void cl_var_kernel(const double* __restrict__ mws, int N, const double* __restrict__ stats, double* __restrict__ slab) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    double v[1] = {0.0};
    if (i < N) {
        const double m = mws[i];
        if (m == m) { const double d = __dsub_rn(m, stats[1]); v[0] = __dmul_rn(d, d); }
    }
    rf_block_sum<1>(v, slab + (size_t)blockIdx.x * CL_SLAB);
}

// one wave: stats[2] = sigma, stats[3] = thr
__global__ __launch_bounds__(64) void cl_thr_kernel(const double* __restrict__ slab, int nblk, double std_ratio, double* __restrict__ stats) {
    __shared__ double tot[1];
    rf_slab_total<1>(slab, nblk, CL_SLAB, tot);
    __syncthreads();
    if (threadIdx.x == 0) {
        const double n = stats[0];
        const double sigma = n >= 2.0 ? sqrt(tot[0] / (n - 1.0)) : 0.0;
        stats[2] = sigma;
        stats[3] = __dadd_rn(stats[1], __dmul_rn(std_ratio, sigma));
    }
}

__global__ __launch_bounds__(256) void cl_keep_kernel(const double* __restrict__ mws, int N, const double* __restrict__ stats, uint8_t* __restrict__ keep,
                                                      int32_t* __restrict__ n_keep) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool kp = false;
    if (i < N) {
        kp = mws[i] <= stats[3];                                          // false for an invalid point's NaN, and for a NaN threshold
        keep[i] = kp ? 1 : 0;
    }
    const int n = __syncthreads_count(kp);
    if (threadIdx.x == 0 && n > 0) atomicAdd(n_keep, n);                  // an integer sum: the order of arrival does not show
}

static int cl_check_k(const char* fn, int k) { return rf_check_range(fn, "k", k, 1, RF_NAMED(YOHO_KNN3_MAX)); }

}  // namespace yoho

using namespace yoho;

extern "C" {

int yoho_knn_within(yoho_ctx* c, const float* q, int Nq, const float* tgt, int Nt, float max_dist, int k, int skip_same_row, int64_t* idx, float* d2,
                    int32_t* count, void* stream) {
    const char* fn = "yoho_knn_within";
    int rc;
    if ((rc = rf_check_sizes(fn, c, "Nq", Nq, 0, "Nt", Nt, 1)) || (rc = rf_check_limit(fn, RF_NAMED(YOHO_REFINE_MAX_POINTS), "Nq", Nq, "Nt", Nt)) ||
        (rc = rf_check_radius(fn, "max_dist", max_dist)) || (rc = cl_check_k(fn, k))) return rc;
    if (skip_same_row && Nq != Nt) { set_error("yoho_knn_within: skip_same_row needs Nq == Nt (Nq=%d, Nt=%d)", Nq, Nt); return YOHO_EINVAL; }
    if (Nq == 0) return 0;
    if ((rc = rf_check_pointers(fn, q && tgt))) return rc;
    if (!idx && !d2 && !count) { set_error("yoho_knn_within: idx, d2 and count are all NULL"); return YOHO_EINVAL; }
    YOHO_NEED_ALIGNED("yoho_knn_within", 3, q, tgt, d2, count);
    YOHO_NEED_ALIGNED("yoho_knn_within", 7, idx);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    RfGridWs w;
    if ((rc = bind_ws(c, s, [&](Arena& ar) { rf_grid_layout(ar, Nt, w); }))) return rc;
    RfGrid g;
    if ((rc = rf_build_grid(tgt, Nt, max_dist, w, g, s))) return rc;
    const dim3 grid((Nq + 255) / 256), block(256);
    const int skip = skip_same_row ? 1 : 0;
    if (!idx && !d2) hipLaunchKernelGGL(cl_knn_kernel<0>, grid, block, 0, s, g, q, Nq, k, skip, idx, d2, count);
    else if (k <= 8) hipLaunchKernelGGL(cl_knn_kernel<8>, grid, block, 0, s, g, q, Nq, k, skip, idx, d2, count);
    else if (k <= 16) hipLaunchKernelGGL(cl_knn_kernel<16>, grid, block, 0, s, g, q, Nq, k, skip, idx, d2, count);
    else hipLaunchKernelGGL(cl_knn_kernel<32>, grid, block, 0, s, g, q, Nq, k, skip, idx, d2, count);
    HIPCHK(hipGetLastError());
    return 0;
}

int yoho_statistical_outliers(yoho_ctx* c, const float* pts, int N, float max_dist, int k, int min_found, double std_ratio, double* mean_dist,
                              int32_t* count, uint8_t* keep, double* stats, int32_t* n_keep, void* stream) {
    const char* fn = "yoho_statistical_outliers";
    int rc;
    if ((rc = rf_check_cloud(fn, c, N, "max_dist", max_dist)) || (rc = cl_check_k(fn, k))) return rc;
    if (min_found < 1) { set_error("yoho_statistical_outliers: min_found=%d must be at least 1", min_found); return YOHO_EINVAL; }
    if (std::isnan(std_ratio)) { set_error("yoho_statistical_outliers: std_ratio is NaN"); return YOHO_EINVAL; }
    if ((rc = rf_check_pointers(fn, pts && keep && stats && n_keep))) return rc;
    YOHO_NEED_ALIGNED("yoho_statistical_outliers", 3, pts, count, n_keep);
    YOHO_NEED_ALIGNED("yoho_statistical_outliers", 7, mean_dist, stats);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int nblk = (N + 255) / 256;
    double *mws = nullptr, *slab = nullptr;
    RfGridWs w;
    if ((rc = bind_ws(c, s, [&](Arena& ar) {
            mws = ar.take<double>((size_t)N);
            slab = ar.take<double>((size_t)CL_SLAB * nblk);
            rf_grid_layout(ar, N, w);
        }))) return rc;
    RfGrid g;
    if ((rc = rf_build_grid(pts, N, max_dist, w, g, s))) return rc;
    const dim3 grid(nblk), block(256);
    if (k <= 8) hipLaunchKernelGGL(cl_stat_kernel<8>, grid, block, 0, s, g, pts, N, k, min_found, mws, mean_dist, count, slab);
    else if (k <= 16) hipLaunchKernelGGL(cl_stat_kernel<16>, grid, block, 0, s, g, pts, N, k, min_found, mws, mean_dist, count, slab);
    else hipLaunchKernelGGL(cl_stat_kernel<32>, grid, block, 0, s, g, pts, N, k, min_found, mws, mean_dist, count, slab);
    hipLaunchKernelGGL(cl_mean_kernel, dim3(1), dim3(64), 0, s, (const double*)slab, nblk, stats, n_keep);
    hipLaunchKernelGGL(cl_var_kernel, grid, block, 0, s, (const double*)mws, N, (const double*)stats, slab);
    hipLaunchKernelGGL(cl_thr_kernel, dim3(1), dim3(64), 0, s, (const double*)slab, nblk, std_ratio, stats);
    hipLaunchKernelGGL(cl_keep_kernel, grid, block, 0, s, (const double*)mws, N, (const double*)stats, keep, n_keep);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
