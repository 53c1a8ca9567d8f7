// Refinement behind the global estimators (include/yoho_refine.h): nearest neighbour inside a radius, iterated Kabsch on the inlier
// matches, gated point-to-point ICP.  Compiled with -ffp-contract=off like estim.hip / match.hip / gridnn.hip (yoho_amd/build.py).
//
//   rf_within_kernel                                             yoho_nn_within: one lane per query over 27 cells
//   rf_icp_pair_kernel                                           ICP: transform + the same walk + gate + first-pass partial sums
//   rf_refit_mask_kernel                                         refit: estim.hip's inlier() + first-pass partial sums
//   rf_mean_kernel / rf_*_cov_kernel / rf_solve_kernel           the Kabsch step: centroids, centred products, Jacobi, stop word
// The cell-sorted grid over the target cloud is built by rfgrid.hip and walked through rfgrid.h (rf_walk: THE GRID and THE QUERY are
// described in rfgrid.hip); the sums and the pieces of the Kabsch step (rf_block_sum, rf_slab_total, rf_apply, rf_centroids,
// rf_centred_products, rf_rotation, rf_rigid_row: THE SUMS) are in rffit.h.  plane.hip, verify.hip and consist.hip share both.
//
// THE ITERATIONS.  All of them are queued at once.  rf_mean_kernel / rf_solve_kernel, one wave, keep the state of the call in device
// memory (RfState: the current transform, centroids, the stop word); a kernel that finds the stop word set returns at once - a
// wave-uniform branch on a loaded word.  Nothing is read back to the host.
//
// Registers (hipcc -O3, gfx950): rf_within_kernel 23 VGPRs, rf_icp_pair_kernel 38, the covariance passes 42, rf_refit_mask_kernel 46,
// rf_solve_kernel (one thread's Jacobi) 80; no scratch in any kernel of this file (.private_segment_fixed_size 0, no spills).
// Untuned at large sizes, for ICP as much as for the refit: rf_mean_kernel and rf_solve_kernel add the per-block slabs serially
// (rffit.h rf_slab_total), twice per iteration.  Timings: tools/time_refine.py -> profiles/refine.md.
#include "rfgrid.h"
#include "rffit.h"
#include "yoho_refine.h"
#include <cmath>

namespace yoho {

// ---- the query (rf_walk: rfgrid.h) -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rf_within_kernel(RfGrid g, const float* __restrict__ q, int Nq, int64_t* __restrict__ idx, float* __restrict__ d2) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Nq) return;
    const float qq[3] = {q[3 * (size_t)i], q[3 * (size_t)i + 1], q[3 * (size_t)i + 2]};
    float bd;
    int bi;
    rf_walk(g, qq, bd, bi);
    idx[i] = bi == RF_NONE ? -1 : bi;
    if (d2) d2[i] = bd;                                               // +inf without a candidate
}

// ---- the state of a call and the sums ------------------------------------------------------------------------------------------
struct RfState {
    double T[12];            // the current (last accepted) transform
    double c0[3], c1[3];     // centroids of the current set: fragment 0's side (k0 / tgt), fragment 1's side (k1 / src)
    int n;                   // size of the current set
    int stop;                // set once: every later kernel of the call returns
    int reason, done;        // ICP: stop reason, iterations made
    int best, best_count;    // refit: the iterate with the largest count so far
    int evaluated, pad;
};

__global__ void rf_init_kernel(RfState* __restrict__ st, const double* __restrict__ T_in, double* __restrict__ Tall, int32_t* __restrict__ ints, int nints,
                               double* __restrict__ dbls, int ndbls) {
    const int t = threadIdx.x;
    if (t < 12) { const double v = T_in[t]; st->T[t] = v; if (Tall) Tall[t] = v; }
    if (t < 3) { st->c0[t] = 0.0; st->c1[t] = 0.0; }
    if (t == 0) { st->n = 0; st->stop = 0; st->reason = 0; st->done = 0; st->best = 0; st->best_count = -1; st->evaluated = 0; st->pad = 0; }
    for (int k = t; k < nints; k += blockDim.x) ints[k] = -1;
    for (int k = t; k < ndbls; k += blockDim.x) dbls[k] = -1.0;
}

// ICP, first pass of iteration `it`: pair[e] = partner of source point e under the current transform (or -1), slab row =
// {n, SUM d2, SUM tgt (3), SUM src (3)} of the block
__global__ __launch_bounds__(256) void rf_icp_pair_kernel(const RfState* __restrict__ st, RfGrid g, const float* __restrict__ src, int Ns,
                                                          const float* __restrict__ tgt, int* __restrict__ pair, double* __restrict__ slab) {
    if (st->stop) return;                                             // wave-uniform: a loaded word
    const int e = blockIdx.x * 256 + threadIdx.x;
    const bool valid = e < Ns;
    double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (valid) {
        const double s0 = (double)src[3 * (size_t)e], s1 = (double)src[3 * (size_t)e + 1], s2 = (double)src[3 * (size_t)e + 2];
        double x[3];
        rf_apply(st->T, s0, s1, s2, x);
        const float q[3] = {(float)x[0], (float)x[1], (float)x[2]};
        float bd;
        int bi;
        rf_walk(g, q, bd, bi);
        pair[e] = bi == RF_NONE ? -1 : bi;
        if (bi != RF_NONE) {
            v[0] = 1.0; v[1] = (double)bd;
            v[2] = (double)tgt[3 * (size_t)bi]; v[3] = (double)tgt[3 * (size_t)bi + 1]; v[4] = (double)tgt[3 * (size_t)bi + 2];
            v[5] = s0; v[6] = s1; v[7] = s2;
        }
    }
    rf_block_sum<8>(v, slab + (size_t)blockIdx.x * RF_SLAB);
}

// refit, first pass of iterate `it`: mask[m] = inlier under Tcur, slab row = {n, matches whose flag differs from the iterate before,
// SUM k0 (3), SUM k1 (3)}
__global__ __launch_bounds__(256) void rf_refit_mask_kernel(const RfState* __restrict__ st, const double* __restrict__ Tcur, const double* __restrict__ k0,
                                                            const double* __restrict__ k1, int M, double d2thr, unsigned char* __restrict__ mask,
                                                            const unsigned char* __restrict__ mask_prev, double* __restrict__ slab) {
    if (st->stop) return;
    __shared__ double Ts[12];
    if (threadIdx.x < 12) Ts[threadIdx.x] = Tcur[threadIdx.x];
    __syncthreads();
    const int m = blockIdx.x * 256 + threadIdx.x;
    double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (m < M) {
        const double* a = k0 + 3 * (size_t)m;
        const double* b = k1 + 3 * (size_t)m;
        const bool in = inlier(Ts, a, b, d2thr);
        mask[m] = in ? 1 : 0;
        if (mask_prev && (mask_prev[m] != 0) != in) v[1] = 1.0;
        if (in) rf_pair_row(a, b, v);
    }
    rf_block_sum<8>(v, slab + (size_t)blockIdx.x * RF_SLAB);
}

// one wave: the slabs of a first pass in block order -> n, centroids; the per-iteration outputs; the stop rules that need no transform
// MODE 0 ICP (npairs / rmse), 1 refit (counts, best so far, fixed point, last iterate)
template <int MODE>
__global__ __launch_bounds__(64) void rf_mean_kernel(RfState* __restrict__ st, const double* __restrict__ slab, int nblk, int it, int iters,
                                                     int32_t* __restrict__ counts, double* __restrict__ rmse) {
    if (st->stop) return;
    __shared__ double tot[8];
    rf_slab_total<8>(slab, nblk, RF_SLAB, tot);
    __syncthreads();
    const int n = (int)tot[0];
    rf_centroids(tot, n, st->c0, st->c1);
    if (threadIdx.x == 0) {
        st->n = n;
        counts[it] = n;
        if (MODE == 0) {
            rmse[it] = n > 0 ? sqrt(tot[1] / (double)n) : __builtin_inf();
            st->done = it + 1;
            if (n < 3) { st->stop = 1; st->reason = YOHO_ICP_FEW_PAIRS; }
        } else {
            st->evaluated = it + 1;
            if (n > st->best_count) { st->best_count = n; st->best = it; }
            if (it == iters || n < 3 || (it > 0 && tot[1] == 0.0)) st->stop = 1;
        }
    }
}

// second pass: slab row = the nine centred products H[i][j] = SUM (b_i - c1_i)(a_j - c0_j) of the block
__global__ __launch_bounds__(256) void rf_icp_cov_kernel(const RfState* __restrict__ st, const float* __restrict__ src, int Ns, const float* __restrict__ tgt,
                                                         const int* __restrict__ pair, double* __restrict__ slab) {
    if (st->stop) return;
    const int e = blockIdx.x * 256 + threadIdx.x;
    double v[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int j = e < Ns ? pair[e] : -1;
    if (j >= 0) rf_centred_products(tgt + 3 * (size_t)j, src + 3 * (size_t)e, st->c0, st->c1, v);
    rf_block_sum<9>(v, slab + (size_t)blockIdx.x * RF_SLAB);
}

__global__ __launch_bounds__(256) void rf_refit_cov_kernel(const RfState* __restrict__ st, const double* __restrict__ k0, const double* __restrict__ k1, int M,
                                                           const unsigned char* __restrict__ mask, double* __restrict__ slab) {
    if (st->stop) return;
    const int m = blockIdx.x * 256 + threadIdx.x;
    double v[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (m < M && mask[m]) rf_centred_products(k0 + 3 * (size_t)m, k1 + 3 * (size_t)m, st->c0, st->c1, v);
    rf_block_sum<9>(v, slab + (size_t)blockIdx.x * RF_SLAB);
}

// one wave: the slabs of a second pass in block order -> H -> T_{i+1}, and the stop rules that need it
// MODE 0 ICP: Tnext = st->T (replaced when accepted); 1 refit: Tnext = the next row of the iterates
template <int MODE>
__global__ __launch_bounds__(64) void rf_solve_kernel(RfState* __restrict__ st, const double* __restrict__ slab, int nblk, int it, int iters, double tol,
                                                      double* __restrict__ Tnext) {
    if (st->stop) return;
    __shared__ double H[9];
    rf_slab_total<9>(slab, nblk, RF_SLAB, H);
    __syncthreads();
    if (threadIdx.x != 0) return;
    double R[9], T[12];
    if (!rf_rotation(H, R)) {
        st->stop = 1;
        if (MODE == 0) st->reason = YOHO_ICP_RANK;
        return;
    }
    rf_rigid_row(R, st->c0, st->c1, T);
    if (MODE == 0) {
        double delta = 0.0;
#pragma unroll
        for (int i = 0; i < 12; ++i) { delta = fmax(delta, fabs(__dsub_rn(T[i], st->T[i]))); st->T[i] = T[i]; }
        if (delta <= tol) { st->stop = 1; st->reason = YOHO_ICP_CONVERGED; }
        else if (it + 1 == iters) { st->stop = 1; st->reason = YOHO_ICP_ITERS; }
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) Tnext[i] = T[i];
    }
}

// MODE 0: T_out = the current transform, info = {iterations made, reason}; 1: T_out = the best iterate, info = {its index, evaluated}
template <int MODE>
__global__ void rf_finish_kernel(const RfState* __restrict__ st, const double* __restrict__ Tall, double* __restrict__ T_out, int32_t* __restrict__ info) {
    const int t = threadIdx.x;
    if (t < 12) T_out[t] = MODE == 0 ? st->T[t] : Tall[12 * (size_t)st->best + t];
    if (t == 0) { info[0] = MODE == 0 ? st->done : st->best; info[1] = MODE == 0 ? st->reason : st->evaluated; }
}

}  // namespace yoho

using namespace yoho;

extern "C" {

int yoho_nn_within(yoho_ctx* c, const float* q, int Nq, const float* tgt, int Nt, float max_dist, int64_t* idx, float* d2, void* stream) {
    const char* fn = "yoho_nn_within";
    int rc;
    if ((rc = rf_check_sizes(fn, c, "Nq", Nq, 0, "Nt", Nt, 1)) || (rc = rf_check_limit(fn, RF_NAMED(YOHO_REFINE_MAX_POINTS), "Nq", Nq, "Nt", Nt)) ||
        (rc = rf_check_radius(fn, "max_dist", max_dist))) return rc;
    if (Nq == 0) return 0;
    if ((rc = rf_check_pointers(fn, q && tgt && idx))) return rc;
    YOHO_NEED_ALIGNED("yoho_nn_within", 3, q, tgt, d2);
    YOHO_NEED_ALIGNED("yoho_nn_within", 7, idx);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    RfGridWs w;
    if ((rc = bind_ws(c, s, [&](Arena& ar) { rf_grid_layout(ar, Nt, w); }))) return rc;
    RfGrid g;
    if ((rc = rf_build_grid(tgt, Nt, max_dist, w, g, s))) return rc;
    hipLaunchKernelGGL(rf_within_kernel, dim3((Nq + 255) / 256), dim3(256), 0, s, g, q, Nq, idx, d2);
    HIPCHK(hipGetLastError());
    return 0;
}

int yoho_refit_matches(yoho_ctx* c, const double* k0, const double* k1, int M, const double* T_in, double inlier_dist, int iters, double* T_out,
                       int32_t* counts, int32_t* info, void* stream) {
    const char* fn = "yoho_refit_matches";
    int rc;
    if ((rc = rf_check_sizes(fn, c, "M", M, 0)) || (rc = rf_check_limit(fn, RF_NAMED(YOHO_REFINE_MAX_POINTS), "M", M)) ||
        (rc = rf_check_range(fn, "iters", iters, 0, RF_NAMED(YOHO_REFIT_MAX_ITERS)))) return rc;
    if (!(inlier_dist >= 0.0) || !std::isfinite(inlier_dist)) { set_error("yoho_refit_matches: inlier_dist=%g must be finite and >= 0", inlier_dist); return YOHO_EINVAL; }
    if ((rc = rf_check_pointers(fn, T_in && T_out && counts && info && (M == 0 || (k0 && k1))))) return rc;
    YOHO_NEED_ALIGNED("yoho_refit_matches", 7, k0, k1, T_in, T_out);
    YOHO_NEED_ALIGNED("yoho_refit_matches", 3, counts, info);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int nblk = (M + 255) / 256;
    RfState* st = nullptr;
    double *Tall = nullptr, *slab = nullptr;
    unsigned char* mask[2] = {nullptr, nullptr};
    if ((rc = bind_ws(c, s, [&](Arena& ar) {
            st = ar.take<RfState>(1);
            Tall = ar.take<double>(12 * (size_t)(iters + 1));
            slab = ar.take<double>((size_t)RF_SLAB * (nblk > 0 ? nblk : 1));
            mask[0] = ar.take<unsigned char>((size_t)M);
            mask[1] = ar.take<unsigned char>((size_t)M);
        }))) return rc;
    const double d2thr = inlier_dist * inlier_dist;                   // yoho_o_score's d * d
    hipLaunchKernelGGL(rf_init_kernel, dim3(1), dim3(64), 0, s, st, T_in, Tall, counts, iters + 1, (double*)nullptr, 0);
    HIPCHK(hipGetLastError());
    for (int it = 0; it <= iters; ++it) {
        if (nblk > 0)
            hipLaunchKernelGGL(rf_refit_mask_kernel, dim3(nblk), dim3(256), 0, s, (const RfState*)st, (const double*)(Tall + 12 * (size_t)it), k0, k1, M, d2thr,
                               mask[it & 1], (const unsigned char*)(it > 0 ? mask[(it - 1) & 1] : nullptr), slab);
        hipLaunchKernelGGL(rf_mean_kernel<1>, dim3(1), dim3(64), 0, s, st, (const double*)slab, nblk, it, iters, counts, (double*)nullptr);
        HIPCHK(hipGetLastError());
        if (it == iters || nblk == 0) break;
        hipLaunchKernelGGL(rf_refit_cov_kernel, dim3(nblk), dim3(256), 0, s, (const RfState*)st, k0, k1, M, (const unsigned char*)mask[it & 1], slab);
        hipLaunchKernelGGL(rf_solve_kernel<1>, dim3(1), dim3(64), 0, s, st, (const double*)slab, nblk, it, iters, 0.0, Tall + 12 * (size_t)(it + 1));
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(rf_finish_kernel<1>, dim3(1), dim3(64), 0, s, (const RfState*)st, (const double*)Tall, T_out, info);
    HIPCHK(hipGetLastError());
    return 0;
}

int yoho_icp_refine(yoho_ctx* c, const float* src, int Ns, const float* tgt, int Nt, const double* T_in, float max_dist, int iters, double tol,
                    double* T_out, int32_t* npairs, double* rmse, int32_t* info, void* stream) {
    const char* fn = "yoho_icp_refine";
    int rc;
    if ((rc = rf_check_icp(fn, c, Ns, Nt, iters, max_dist, tol)) ||
        (rc = rf_check_pointers(fn, src && tgt && T_in && T_out && info && (iters == 0 || (npairs && rmse))))) return rc;
    YOHO_NEED_ALIGNED("yoho_icp_refine", 3, src, tgt, npairs, info);
    YOHO_NEED_ALIGNED("yoho_icp_refine", 7, T_in, T_out, rmse);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int nblk = (Ns + 255) / 256;
    RfState* st = nullptr;
    double* slab = nullptr;
    int* pair = nullptr;
    RfGridWs w;
    if ((rc = bind_ws(c, s, [&](Arena& ar) {
            st = ar.take<RfState>(1);
            slab = ar.take<double>((size_t)RF_SLAB * nblk);
            pair = ar.take<int>((size_t)Ns);
            if (iters > 0) rf_grid_layout(ar, Nt, w);
        }))) return rc;
    hipLaunchKernelGGL(rf_init_kernel, dim3(1), dim3(64), 0, s, st, T_in, (double*)nullptr, npairs, iters, rmse, iters);
    HIPCHK(hipGetLastError());
    if (iters > 0) {
        RfGrid g;
        if ((rc = rf_build_grid(tgt, Nt, max_dist, w, g, s))) return rc;
        for (int it = 0; it < iters; ++it) {
            hipLaunchKernelGGL(rf_icp_pair_kernel, dim3(nblk), dim3(256), 0, s, (const RfState*)st, g, src, Ns, tgt, pair, slab);
            hipLaunchKernelGGL(rf_mean_kernel<0>, dim3(1), dim3(64), 0, s, st, (const double*)slab, nblk, it, iters, npairs, rmse);
            hipLaunchKernelGGL(rf_icp_cov_kernel, dim3(nblk), dim3(256), 0, s, (const RfState*)st, src, Ns, tgt, (const int*)pair, slab);
            hipLaunchKernelGGL(rf_solve_kernel<0>, dim3(1), dim3(64), 0, s, st, (const double*)slab, nblk, it, iters, tol, (double*)nullptr);
            HIPCHK(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(rf_finish_kernel<0>, dim3(1), dim3(64), 0, s, (const RfState*)st, (const double*)nullptr, T_out, info);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
