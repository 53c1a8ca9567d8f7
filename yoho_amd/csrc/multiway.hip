// The information matrix of K edges into one target (include/yoho_multiway.h).  Compiled with -ffp-contract=off like
// verify.hip (yoho_amd/build.py).  The cell-sorted grid and its walk come from rfgrid.hip / rfgrid.h, the fixed-order f64 sums and the
// rounded transform from rffit.h (THE SUMS, rf_apply); both carry over unchanged.
//
//   mw_eval_kernel   one lane per (edge, local element), sum_k ceil(n_k / 256) workgroups: transform + rf_walk + the 11 partial sums
//   mw_sum_kernel    one wave per edge: the edge's slab rows in block order -> npairs, rmse, the 36 entries
//
// THE EDGE TABLE.  soff is a host array; the entry validates it and hands the kernels a copy BY VALUE (MwEdges, 520 bytes of kernel
// arguments): the source offsets and the prefix of the workgroup counts.  Workgroups are aligned to edges - block b of edge k is
// the local elements 256 b .. 256 b + 255 -, so a row's sums do not depend on soff[k] or on its neighbours.  A workgroup finds its
// edge by bisection of the prefix with blockIdx.x: scalar loads of kernel arguments, a wave-uniform edge index, and through it scalar
// loads of the row's 12 doubles.  vf_eval_kernel's grid (ceil(Ns / 256), K) needs equal lengths; a scene's fragments are not.
//
// THE SUMS.  A lane contributes {1, d2, p (3), px px, px py, px pz, py py, py pz, pz pz} with p its partner widened to f64, or
// eleven +0.0 without a partner; rf_block_sum writes the block's sums to the slab row of the WORKGROUP (the global block index, so
// the rows of an edge are contiguous and in block order).  mw_sum_kernel adds an edge's rows, one thread per component
// (rf_slab_total, serial: the price of the stated order), and forms the matrix.  No float atomics, no grid-wide barrier; every
// workspace byte is written (the grid build, the evaluation) before it is read.
//
// Registers (hipcc -O3, gfx950) and timings are recorded in profiles/multiway.md; no kernel of this file uses scratch.
#include "rfgrid.h"
#include "rffit.h"
#include "yoho_multiway.h"
#include <cmath>

namespace yoho {

constexpr int MW_NV = 11;                 // {n, SUM d2, s (3), Sxx, Sxy, Sxz, Syy, Syz, Szz}
constexpr int MW_SLAB = 12;               // doubles per slab row (11 used)

struct MwEdges {
    int soff[YOHO_MULTIWAY_MAX_K + 1];    // first row of source k in src
    int bpre[YOHO_MULTIWAY_MAX_K + 1];    // first workgroup of edge k; bpre[K] workgroups in all
};

__global__ __launch_bounds__(256) void mw_eval_kernel(MwEdges ed, int K, RfGrid g, const float* __restrict__ src, const float* __restrict__ tgt,
                                                      const double* __restrict__ Trows, double* __restrict__ slab) {
    const int blk = blockIdx.x;
    int lo = 0, hi = K;                                               // bpre[lo] <= blk < bpre[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ed.bpre[mid] <= blk) lo = mid; else hi = mid;
    }
    const int k = lo;                                                 // wave-uniform: from blockIdx and kernel arguments alone
    const int s0 = ed.soff[k], n = ed.soff[k + 1] - s0;
    const double* __restrict__ T = Trows + 12 * (size_t)k;
    const int e = (blk - ed.bpre[k]) * 256 + threadIdx.x;             // the LOCAL index
    double v[MW_NV] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (e < n) {
        double x[3];
        rf_apply(T, src, s0 + e, x);
        const float q[3] = {(float)x[0], (float)x[1], (float)x[2]};
        float bd;
        int bi;
        rf_walk(g, q, bd, bi);
        if (bi != RF_NONE) {
            const double px = (double)tgt[3 * (size_t)bi], py = (double)tgt[3 * (size_t)bi + 1], pz = (double)tgt[3 * (size_t)bi + 2];
            v[0] = 1.0; v[1] = (double)bd;
            v[2] = px; v[3] = py; v[4] = pz;
            v[5] = __dmul_rn(px, px); v[6] = __dmul_rn(px, py); v[7] = __dmul_rn(px, pz);
            v[8] = __dmul_rn(py, py); v[9] = __dmul_rn(py, pz); v[10] = __dmul_rn(pz, pz);
        }
    }
    rf_block_sum<MW_NV>(v, slab + (size_t)blk * MW_SLAB);
}

// one wave per edge: the slab rows of the edge in block order, then the matrix
__global__ __launch_bounds__(64) void mw_sum_kernel(MwEdges ed, const double* __restrict__ slab, int32_t* __restrict__ npairs, double* __restrict__ rmse,
                                                    double* __restrict__ info) {
    const int k = blockIdx.x;
    __shared__ double tot[MW_NV];
    rf_slab_total<MW_NV>(slab + (size_t)ed.bpre[k] * MW_SLAB, ed.bpre[k + 1] - ed.bpre[k], MW_SLAB, tot);
    __syncthreads();
    const int t = threadIdx.x;
    if (t == 0) {
        const int n = (int)tot[0];
        npairs[k] = n;
        rmse[k] = n > 0 ? sqrt(tot[1] / (double)n) : __builtin_inf();
    }
    if (t < 36) {
        const int r = t / 6, c = t % 6;
        const double sx = tot[2], sy = tot[3], sz = tot[4];
        const double Sxx = tot[5], Sxy = tot[6], Sxz = tot[7], Syy = tot[8], Syz = tot[9], Szz = tot[10];
        double v;
        if (r < 3 && c < 3) v = r == c ? tot[0] : 0.0;
        else if (r >= 3 && c >= 3) {
            const int a = r - 3, b = c - 3;
            if (a == b) v = a == 0 ? __dadd_rn(Syy, Szz) : (a == 1 ? __dadd_rn(Sxx, Szz) : __dadd_rn(Sxx, Syy));
            else { const int m = a + b; v = -(m == 1 ? Sxy : (m == 2 ? Sxz : Syz)); }
        } else {
            // -[s]x in the upper right block, its transpose in the lower left: entry (a, b) of -[s]x with a the translation index
            const int a = r < 3 ? r : c, b = r < 3 ? c - 3 : r - 3;
            if (a == b) v = 0.0;
            else {
                const int o = 3 - a - b;                              // the third axis
                const double sv = o == 0 ? sx : (o == 1 ? sy : sz);
                v = (b == (a + 1) % 3) ? sv : -sv;                    // (0,1) = s_z, (1,2) = s_x, (2,0) = s_y; the others negated
            }
        }
        info[36 * (size_t)k + t] = v;
    }
}

}  // namespace yoho

using namespace yoho;

extern "C" {

int yoho_edge_information(yoho_ctx* c, const float* src, const int32_t* soff, int K, const float* tgt, int Nt, const double* T, float max_dist,
                          int32_t* npairs, double* rmse, double* info, void* stream) {
    const char* fn = "yoho_edge_information";
    int rc;
    if ((rc = rf_check_sizes(fn, c, "K", K, 1, "Nt", Nt, 1)) || (rc = rf_check_range(fn, "K", K, 1, RF_NAMED(YOHO_MULTIWAY_MAX_K))) ||
        (rc = rf_check_limit(fn, RF_NAMED(YOHO_REFINE_MAX_POINTS), "Nt", Nt)) || (rc = rf_check_radius(fn, "max_dist", max_dist)) ||
        (rc = rf_check_pointers(fn, src && soff && tgt && T && npairs && rmse && info))) return rc;
    if (soff[0] != 0) return RF_REFUSE("%s: soff[0]=%d must be 0", fn, (int)soff[0]);
    MwEdges ed;
    ed.soff[0] = 0;
    ed.bpre[0] = 0;
    for (int k = 0; k < K; ++k) {
        const long long n = (long long)soff[k + 1] - (long long)soff[k];
        if (n < 1) return RF_REFUSE("%s: soff[%d]=%d, soff[%d]=%d: soff must be strictly increasing (no empty source)", fn, k, (int)soff[k], k + 1, (int)soff[k + 1]);
        if (n > YOHO_REFINE_MAX_POINTS)
            return RF_REFUSE("%s: source %d has %lld points, more than YOHO_REFINE_MAX_POINTS = %d", fn, k, n, (int)YOHO_REFINE_MAX_POINTS);
        ed.soff[k + 1] = soff[k + 1];
        ed.bpre[k + 1] = ed.bpre[k] + (int)((n + 255) / 256);
    }
    if (soff[K] > YOHO_MULTIWAY_MAX_SOURCE_POINTS)
        return RF_REFUSE("%s: soff[K]=%d must not exceed YOHO_MULTIWAY_MAX_SOURCE_POINTS = %d", fn, (int)soff[K], (int)YOHO_MULTIWAY_MAX_SOURCE_POINTS);
    for (int k = K + 1; k <= YOHO_MULTIWAY_MAX_K; ++k) { ed.soff[k] = ed.soff[K]; ed.bpre[k] = ed.bpre[K]; }
    YOHO_NEED_ALIGNED("yoho_edge_information", 3, src, tgt, npairs);
    YOHO_NEED_ALIGNED("yoho_edge_information", 7, T, rmse, info);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int nblk = ed.bpre[K];
    double* slab = nullptr;
    RfGridWs w;
    if ((rc = bind_ws(c, s, [&](Arena& ar) {
            slab = ar.take<double>((size_t)MW_SLAB * nblk);
            rf_grid_layout(ar, Nt, w);
        }))) return rc;
    RfGrid g;
    if ((rc = rf_build_grid(tgt, Nt, max_dist, w, g, s))) return rc;
    hipLaunchKernelGGL(mw_eval_kernel, dim3(nblk), dim3(256), 0, s, ed, K, g, src, tgt, T, slab);
    hipLaunchKernelGGL(mw_sum_kernel, dim3(K), dim3(64), 0, s, ed, (const double*)slab, npairs, rmse, info);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
