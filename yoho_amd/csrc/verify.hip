// Verification of hypotheses on the clouds (include/yoho_verify.h).  Compiled with -ffp-contract=off like refine.hip
// (yoho_amd/build.py).  The cell-sorted grid and its walk come from rfgrid.hip / rfgrid.h (THE GRID, THE QUERY's exactness argument),
// the fixed-order f64 sums and the rounded transform from rffit.h (THE SUMS, rf_apply); both carry over unchanged.
//
//   vf_select_kernel   one workgroup: the best K distinct positions of a vote (greedy, with suppression), their rows gathered
//   vf_eval_kernel     grid (ceil(Ns / 256), K), one lane per (source point, row): transform + rf_walk + the three partial sums
//   vf_sum_kernel      one wave per row: the row's slabs in block order -> npairs, rmse, cost
//   vf_pick_kernel     one wave: the cheapest row -> T_out, info
//
// THE SELECTION.  K rounds of one sweep over the H positions, thread t owning the positions t, t + 256, ...: a sweep first applies the
// suppression of the hypothesis taken in the round before to the positions still alive, then offers the survivors to the maximum of
// the key (count << 32 | ~h) - the largest count, the smallest position among equal counts.  The maximum goes through a __shfl_xor
// butterfly and four LDS words; integer maxima do not depend on the order, no atomic decides anything.  alive[] lives in the
// workspace and every byte of it is only ever touched by its owning thread, so the barriers of the loop order LDS alone.  That is
// O(K H / 256) dependent steps: right up to the limit, sized for the few thousand hypotheses of a pair.  The taken rows are copied to
// Tsel (K,3,4), so the evaluation reads K contiguous rows whatever `order` says, and yoho_eval_transforms and yoho_verify_hypotheses
// share one evaluation kernel.
//
// THE EVALUATION.  blockIdx.y is the row: its 12 doubles are the same for the whole workgroup and reach the lanes through scalar
// loads.  Each lane transforms its source point with rf_icp_pair_kernel's expression (rf_apply), walks the 27 cells, and
// contributes {1, d2, d2} when it has a partner and {0, +0.0, gate2} when not; rf_block_sum writes the block's three sums to the slab
// row of (row, block).  No float atomics, no grid-wide barrier: vf_sum_kernel adds a row's slabs in block order, one thread per
// component (rf_slab_total) - serial, nblk dependent additions, which is the price of the stated order.  Kc, the number of
// rows selected, never leaves the device: K rows are launched and a workgroup whose row is >= Kc returns on a loaded word, which is
// wave-uniform (yoho_icp_refine's idiom for the iterations behind a stop).  Every workspace byte is written (vf_select_kernel, the
// grid build, the evaluation) before it is read.
//
// Registers (hipcc -O3, gfx950) and timings are recorded in profiles/verify.md; no kernel of this file uses scratch.
#include "rfgrid.h"
#include "rffit.h"
#include "yoho_verify.h"
#include <cmath>

namespace yoho {

constexpr int VF_SLAB = 4;                // doubles per slab row (3 used): {n, SUM d2, cost}

struct VfState {
    int Kc;                  // rows selected
    int pad;
};

// ---- selection ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vf_select_kernel(const double* __restrict__ T, const int64_t* __restrict__ order, const int32_t* __restrict__ counts,
                                                        int H, int K, int min_count, double tol, unsigned char* __restrict__ alive,
                                                        VfState* __restrict__ st, double* __restrict__ Tsel, int32_t* __restrict__ top,
                                                        int32_t* __restrict__ npairs, double* __restrict__ rmse, double* __restrict__ cost) {
    __shared__ u64 wkey[4];
    __shared__ double Tp[12];                                         // the hypothesis taken in the round before
    const int tid = threadIdx.x;
    for (int h = tid; h < H; h += 256) alive[h] = counts[h] >= min_count ? 1 : 0;
    int Kc = 0;
    for (int i = 0; i < K; ++i) {
        u64 best = 0ull;                                              // an alive position has count >= 1: its key is not 0
        for (int h = tid; h < H; h += 256) {
            if (!alive[h]) continue;
            if (i > 0 && tol > 0.0) {
                const double* row = T + 12 * (size_t)(order ? order[h] : (int64_t)h);
                bool close = true;
#pragma unroll
                for (int j = 0; j < 12; ++j) close = close && (fabs(__dsub_rn(row[j], Tp[j])) < tol);      // a NaN difference is not less
                if (close) { alive[h] = 0; continue; }
            }
            const u64 key = ((u64)(unsigned)counts[h] << 32) | (u64)(0xFFFFFFFFu - (unsigned)h);
            best = key > best ? key : best;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const u64 other = __shfl_xor(best, o);
            best = other > best ? other : best;
        }
        if ((tid & 63) == 0) wkey[tid >> 6] = best;
        __syncthreads();
        u64 b = wkey[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) b = wkey[w] > b ? wkey[w] : b;
        if (b == 0ull) break;                                         // nobody alive: the same word in every thread
        const int pos = (int)(0xFFFFFFFFu - (unsigned)(b & 0xFFFFFFFFull));
        __syncthreads();                                              // wkey and Tp have been read by everyone
        if (tid < 12) {
            const double v = T[12 * (size_t)(order ? order[pos] : (int64_t)pos) + tid];
            Tp[tid] = v;
            Tsel[12 * (size_t)i + tid] = v;
        }
        if (tid == (pos & 255)) alive[pos] = 0;                       // by its owner
        if (tid == 0) top[i] = pos;
        __syncthreads();
        ++Kc;
    }
    for (int i = Kc + tid; i < K; i += 256) { top[i] = -1; npairs[i] = -1; rmse[i] = -1.0; cost[i] = -1.0; }
    if (tid == 0) { st->Kc = Kc; st->pad = 0; }
}

// ---- evaluation ----------------------------------------------------------------------------------------------------------------------
// st == nullptr: every row is evaluated (yoho_eval_transforms)
__global__ __launch_bounds__(256) void vf_eval_kernel(const VfState* __restrict__ st, RfGrid g, const float* __restrict__ src, int Ns,
                                                      const double* __restrict__ Trows, int nblk, double* __restrict__ slab) {
    const int k = blockIdx.y;
    if (st && k >= st->Kc) return;                                    // wave-uniform: a loaded word
    const double* __restrict__ T = Trows + 12 * (size_t)k;
    const int e = blockIdx.x * 256 + threadIdx.x;
    double v[3] = {0.0, 0.0, 0.0};
    if (e < Ns) {
        double x[3];
        rf_apply(T, src, e, x);
        const float q[3] = {(float)x[0], (float)x[1], (float)x[2]};
        float bd;
        int bi;
        rf_walk(g, q, bd, bi);
        const bool paired = bi != RF_NONE;
        v[0] = paired ? 1.0 : 0.0;
        v[1] = paired ? (double)bd : 0.0;
        v[2] = paired ? (double)bd : (double)g.gate2;
    }
    rf_block_sum<3>(v, slab + ((size_t)k * nblk + blockIdx.x) * VF_SLAB);
}

// one wave per row: the slabs of the row in block order
__global__ __launch_bounds__(64) void vf_sum_kernel(const VfState* __restrict__ st, const double* __restrict__ slab, int nblk, int32_t* __restrict__ npairs,
                                                    double* __restrict__ rmse, double* __restrict__ cost) {
    const int k = blockIdx.x;
    if (st && k >= st->Kc) return;
    __shared__ double tot[3];
    rf_slab_total<3>(slab + (size_t)k * nblk * VF_SLAB, nblk, VF_SLAB, tot);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int n = (int)tot[0];
        npairs[k] = n;
        rmse[k] = n > 0 ? sqrt(tot[1] / (double)n) : __builtin_inf();
        cost[k] = tot[2];
    }
}

// one wave: the first row with the smallest cost
__global__ __launch_bounds__(64) void vf_pick_kernel(const VfState* __restrict__ st, const double* __restrict__ Tsel, const double* __restrict__ cost,
                                                     const int32_t* __restrict__ top, const int32_t* __restrict__ counts, double* __restrict__ T_out,
                                                     int32_t* __restrict__ info) {
    __shared__ int sbest;
    if (threadIdx.x == 0) {
        const int Kc = st->Kc;
        int best = -1;
        if (Kc > 0) {
            best = 0;
            for (int i = 1; i < Kc; ++i)
                if (cost[i] < cost[best]) best = i;
        }
        sbest = best;
        info[0] = Kc;
        info[1] = best;
        info[2] = best >= 0 ? top[best] : -1;
        info[3] = best >= 0 ? counts[top[best]] : 0;
    }
    __syncthreads();
    const int best = sbest, t = threadIdx.x;
    if (t < 12) T_out[t] = best >= 0 ? Tsel[12 * (size_t)best + t] : (t % 5 == 0 ? 1.0 : 0.0);       // [I | 0] without a hypothesis
}

}  // namespace yoho

using namespace yoho;

extern "C" {

int yoho_eval_transforms(yoho_ctx* c, const float* src, int Ns, const float* tgt, int Nt, const double* T, int K, float max_dist, int32_t* npairs,
                         double* rmse, double* cost, void* stream) {
    const char* fn = "yoho_eval_transforms";
    int rc;
    if ((rc = rf_check_clouds(fn, c, Ns, Nt)) || (rc = rf_check_range(fn, "K", K, 1, RF_NAMED(YOHO_VERIFY_MAX_K))) ||
        (rc = rf_check_radius(fn, "max_dist", max_dist)) || (rc = rf_check_pointers(fn, src && tgt && T && npairs && rmse && cost))) return rc;
    YOHO_NEED_ALIGNED("yoho_eval_transforms", 3, src, tgt, npairs);
    YOHO_NEED_ALIGNED("yoho_eval_transforms", 7, T, rmse, cost);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int nblk = (Ns + 255) / 256;
    double* slab = nullptr;
    RfGridWs w;
    if ((rc = bind_ws(c, s, [&](Arena& ar) {
            slab = ar.take<double>((size_t)VF_SLAB * nblk * K);
            rf_grid_layout(ar, Nt, w);
        }))) return rc;
    RfGrid g;
    if ((rc = rf_build_grid(tgt, Nt, max_dist, w, g, s))) return rc;
    hipLaunchKernelGGL(vf_eval_kernel, dim3(nblk, K), dim3(256), 0, s, (const VfState*)nullptr, g, src, Ns, T, nblk, slab);
    hipLaunchKernelGGL(vf_sum_kernel, dim3(K), dim3(64), 0, s, (const VfState*)nullptr, (const double*)slab, nblk, npairs, rmse, cost);
    HIPCHK(hipGetLastError());
    return 0;
}

int yoho_verify_hypotheses(yoho_ctx* c, const float* src, int Ns, const float* tgt, int Nt, const double* T, const int64_t* order, const int32_t* counts,
                           int H, int K, int min_count, double distinct_tol, float max_dist, double* T_out, int32_t* top, int32_t* npairs, double* rmse,
                           double* cost, int32_t* info, void* stream) {
    const char* fn = "yoho_verify_hypotheses";
    int rc;
    if ((rc = rf_check_clouds(fn, c, Ns, Nt)) || (rc = rf_check_range(fn, "K", K, 1, RF_NAMED(YOHO_VERIFY_MAX_K))) ||
        (rc = rf_check_radius(fn, "max_dist", max_dist)) || (rc = rf_check_range(fn, "H", H, 0, RF_NAMED(YOHO_REFINE_MAX_POINTS)))) return rc;
    if (min_count < 1) { set_error("yoho_verify_hypotheses: min_count=%d must be at least 1", min_count); return YOHO_EINVAL; }
    if (!(distinct_tol >= 0.0) || !std::isfinite(distinct_tol)) { set_error("yoho_verify_hypotheses: distinct_tol=%g must be finite and >= 0", distinct_tol); return YOHO_EINVAL; }
    if ((rc = rf_check_pointers(fn, src && tgt && T_out && top && npairs && rmse && cost && info && (H == 0 || (T && counts))))) return rc;
    YOHO_NEED_ALIGNED("yoho_verify_hypotheses", 3, src, tgt, counts, top, npairs, info);
    YOHO_NEED_ALIGNED("yoho_verify_hypotheses", 7, T, order, T_out, rmse, cost);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int nblk = (Ns + 255) / 256;
    VfState* st = nullptr;
    double *Tsel = nullptr, *slab = nullptr;
    unsigned char* alive = nullptr;
    RfGridWs w;
    if ((rc = bind_ws(c, s, [&](Arena& ar) {
            st = ar.take<VfState>(1);
            Tsel = ar.take<double>(12 * (size_t)K);
            alive = ar.take<unsigned char>((size_t)(H > 0 ? H : 1));
            slab = ar.take<double>((size_t)VF_SLAB * nblk * K);
            rf_grid_layout(ar, Nt, w);
        }))) return rc;
    hipLaunchKernelGGL(vf_select_kernel, dim3(1), dim3(256), 0, s, T, order, counts, H, K, min_count, distinct_tol, alive, st, Tsel, top, npairs, rmse, cost);
    HIPCHK(hipGetLastError());
    RfGrid g;
    if ((rc = rf_build_grid(tgt, Nt, max_dist, w, g, s))) return rc;
    hipLaunchKernelGGL(vf_eval_kernel, dim3(nblk, K), dim3(256), 0, s, (const VfState*)st, g, src, Ns, (const double*)Tsel, nblk, slab);
    hipLaunchKernelGGL(vf_sum_kernel, dim3(K), dim3(64), 0, s, (const VfState*)st, (const double*)slab, nblk, npairs, rmse, cost);
    hipLaunchKernelGGL(vf_pick_kernel, dim3(1), dim3(64), 0, s, (const VfState*)st, (const double*)Tsel, (const double*)cost, (const int32_t*)top, counts, T_out,
                       info);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
