// Surface normals and point-to-plane ICP (include/yoho_plane.h).  Compiled with -ffp-contract=off like refine.hip (yoho_amd/build.py).
// The cell-sorted grid and its walks come from rfgrid.hip / rfgrid.h (THE GRID, THE QUERY's exactness argument), the fixed-order f64
// sums, the rounded transform and the Jacobi from rffit.h (THE SUMS, rf_apply, rf_eig3).
//
//   pl_normals_kernel      yoho_estimate_normals: one lane per point over the 27 cells around it, ten accumulators, a 3 x 3 Jacobi
//   pl_pair_kernel         ICP: transform + rf_walk + the normal test + first-pass partial sums {n, SUM x}
//   pl_mean_kernel         one wave: n_kept, the centroid c
//   pl_normeq_kernel       ICP: the 28 partial sums of the normal equations about c
//   pl_solve_kernel        one wave: rmse, the 6 x 6 Cholesky solve, exp([w]x), the update and the stop word
//
// THE NORMALS.  The grid is built over the points themselves with cell side radius (1 + 2^-10), so the 27 cells around a point hold
// every j with d2 < gate2 (rfgrid.hip (1) - (3), with the point as the query).  The count and the ten sums are rfgrid.h's rf_moments
// (THE DISTINCT BUCKETS: a count needs every bucket walked once), the eigenvectors rffit.h's rf_eig3; what is this file's is the
// choice of the normal, its sign and the curvature.
//
// THE ITERATIONS are queued at once, four launches each, with refine.hip's state machine: PlState lives in the workspace, a kernel
// that finds the stop word set returns at once - a wave-uniform branch on a loaded word.  x_e is recomputed by the second pass (the
// same rounded operations give the same bits) instead of being stored.  All four stop rules are looked at by pl_solve_kernel,
// because rmse[i] comes out of the second pass and is owed for an iteration that stops for want of pairs, too.  Every workspace
// byte is written (pl_init_kernel, the grid build, the passes in order) before it is read; no float atomic anywhere.
//
// Registers (hipcc -O3, gfx950) are recorded in profiles/plane_icp.md; no kernel of this file uses scratch.
#include "rfgrid.h"
#include "rffit.h"
#include "yoho_plane.h"
#include <cmath>

namespace yoho {

constexpr int PL_SLAB = 32;               // doubles per slab row (4 or 28 used)
constexpr int PL_NSUM = 28;               // 21 A_kl (k <= l, row by row), 6 b_k, E
constexpr int PL_MIN_PAIRS = 6;
constexpr double PL_PIVOT_TOL = 1e-13;
constexpr double PL_COLLINEAR_TOL = 1e-12;

// ---- normals -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pl_normals_kernel(RfGrid g, const float* __restrict__ pts, int N, int min_nbrs, float vx, float vy, float vz,
                                                         float* __restrict__ normals, int32_t* __restrict__ count, float* __restrict__ curv) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    float q[3];
    rf_load_row(pts, i, q);
    const double px = (double)q[0], py = (double)q[1], pz = (double)q[2];
    int n;
    double S1[3], S2[6];
    rf_moments(g, q, n, S1, S2);
    count[i] = n;
    float out[3] = {0.f, 0.f, 0.f}, cv = -1.f;
    if (n >= min_nbrs) {                                              // min_nbrs >= 3 > 0
        const double dn = (double)n;
        const double C[6] = {S2[0] - S1[0] * S1[0] / dn, S2[1] - S1[0] * S1[1] / dn, S2[2] - S1[0] * S1[2] / dn,
                             S2[3] - S1[1] * S1[1] / dn, S2[4] - S1[1] * S1[2] / dn, S2[5] - S1[2] * S1[2] / dn};      // not divided by n: the vectors are those of C / n
        double lam[3], V[9];
        rf_eig3<true>(C, lam, V);
        int i1 = 0;
        if (lam[1] < lam[i1]) i1 = 1;
        if (lam[2] < lam[i1]) i1 = 2;
        int i2 = (i1 + 1) % 3, i3 = (i1 + 2) % 3;
        if (lam[i3] < lam[i2]) { const int t = i2; i2 = i3; i3 = t; }
        const double l1 = lam[i1], l2 = lam[i2], l3 = lam[i3];
        if (l3 > 0.0 && l2 > PL_COLLINEAR_TOL * l3) {
            double nx = V[i1], ny = V[3 + i1], nz = V[6 + i1];
            const double len = sqrt(nx * nx + ny * ny + nz * nz);
            nx /= len; ny /= len; nz /= len;
            const double dot = (nx * ((double)vx - px) + ny * ((double)vy - py)) + nz * ((double)vz - pz);
            const double first = nx != 0.0 ? nx : (ny != 0.0 ? ny : nz);
            if (dot < 0.0 || (dot == 0.0 && first < 0.0)) { nx = -nx; ny = -ny; nz = -nz; }
            out[0] = (float)nx; out[1] = (float)ny; out[2] = (float)nz;
            cv = (float)(l1 / ((l1 + l2) + l3));
        }
    }
    normals[3 * (size_t)i] = out[0]; normals[3 * (size_t)i + 1] = out[1]; normals[3 * (size_t)i + 2] = out[2];
    if (curv) curv[i] = cv;
}

// ---- ICP: the state of a call ------------------------------------------------------------------------------------------------------------
struct PlState {
    double T[12];            // the current (last accepted) transform
    double c[3];             // centroid of the transformed source points of the kept pairs
    int n;                   // kept pairs of the current iteration
    int stop;                // set once: every later kernel of the call returns
    int reason, done;
};

__global__ void pl_init_kernel(PlState* __restrict__ st, const double* __restrict__ T_in, int32_t* __restrict__ ints, double* __restrict__ dbls, int iters) {
    const int t = threadIdx.x;
    if (t < 12) st->T[t] = T_in[t];
    if (t < 3) st->c[t] = 0.0;
    if (t == 0) { st->n = 0; st->stop = 0; st->reason = YOHO_ICP_ITERS; st->done = 0; }
    for (int k = t; k < iters; k += blockDim.x) { ints[k] = -1; dbls[k] = -1.0; }
}

// first pass: pair[e] = partner of source point e when the pair is kept (else -1), slab row = {n, SUM x (3)} of the block
__global__ __launch_bounds__(256) void pl_pair_kernel(const PlState* __restrict__ st, RfGrid g, const float* __restrict__ src, int Ns,
                                                      const float* __restrict__ nrm, int* __restrict__ pair, double* __restrict__ slab) {
    if (st->stop) return;                                             // wave-uniform: a loaded word
    const int e = blockIdx.x * 256 + threadIdx.x;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    if (e < Ns) {
        double x[3];
        rf_apply(st->T, src, e, x);
        const float q[3] = {(float)x[0], (float)x[1], (float)x[2]};
        float bd;
        int bi;
        rf_walk(g, q, bd, bi);
        int j = -1;
        if (bi != RF_NONE) {
            const float n0 = nrm[3 * (size_t)bi], n1 = nrm[3 * (size_t)bi + 1], n2 = nrm[3 * (size_t)bi + 2];
            const bool finite = fabsf(n0) < __builtin_inff() && fabsf(n1) < __builtin_inff() && fabsf(n2) < __builtin_inff();      // false for a NaN
            if (finite && (n0 != 0.f || n1 != 0.f || n2 != 0.f)) j = bi;
        }
        pair[e] = j;
        if (j >= 0) { v[0] = 1.0; v[1] = x[0]; v[2] = x[1]; v[3] = x[2]; }
    }
    rf_block_sum<4>(v, slab + (size_t)blockIdx.x * PL_SLAB);
}

// one wave: the slabs of the first pass in block order -> n_kept, c
__global__ __launch_bounds__(64) void pl_mean_kernel(PlState* __restrict__ st, const double* __restrict__ slab, int nblk, int it, int32_t* __restrict__ npairs) {
    if (st->stop) return;
    __shared__ double tot[4];
    rf_slab_total<4>(slab, nblk, PL_SLAB, tot);
    __syncthreads();
    const int n = (int)tot[0];
    if (threadIdx.x < 3) st->c[threadIdx.x] = n > 0 ? tot[1 + threadIdx.x] / (double)n : 0.0;
    if (threadIdx.x == 0) { st->n = n; npairs[it] = n; st->done = it + 1; }
}

// second pass: slab row = the 28 sums of the block
__global__ __launch_bounds__(256) void pl_normeq_kernel(const PlState* __restrict__ st, const float* __restrict__ src, int Ns, const float* __restrict__ tgt,
                                                        const float* __restrict__ nrm, const int* __restrict__ pair, double* __restrict__ slab) {
    if (st->stop) return;
    const int e = blockIdx.x * 256 + threadIdx.x;
    double v[PL_NSUM];
#pragma unroll
    for (int k = 0; k < PL_NSUM; ++k) v[k] = 0.0;
    const int j = e < Ns ? pair[e] : -1;
    if (j >= 0) {
        double x[3], J[6];
        rf_apply(st->T, src, e, x);
        const double ux = __dsub_rn(x[0], st->c[0]), uy = __dsub_rn(x[1], st->c[1]), uz = __dsub_rn(x[2], st->c[2]);
        const double nx = (double)nrm[3 * (size_t)j], ny = (double)nrm[3 * (size_t)j + 1], nz = (double)nrm[3 * (size_t)j + 2];
        const double r = __dadd_rn(__dadd_rn(__dmul_rn(nx, __dsub_rn(x[0], (double)tgt[3 * (size_t)j])), __dmul_rn(ny, __dsub_rn(x[1], (double)tgt[3 * (size_t)j + 1]))),
                                   __dmul_rn(nz, __dsub_rn(x[2], (double)tgt[3 * (size_t)j + 2])));
        J[0] = __dsub_rn(__dmul_rn(uy, nz), __dmul_rn(uz, ny));
        J[1] = __dsub_rn(__dmul_rn(uz, nx), __dmul_rn(ux, nz));
        J[2] = __dsub_rn(__dmul_rn(ux, ny), __dmul_rn(uy, nx));
        J[3] = nx; J[4] = ny; J[5] = nz;
        int m = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k)
#pragma unroll
            for (int l = k; l < 6; ++l) v[m++] = __dmul_rn(J[k], J[l]);
#pragma unroll
        for (int k = 0; k < 6; ++k) v[21 + k] = __dmul_rn(J[k], r);
        v[27] = __dmul_rn(r, r);
    }
    rf_block_sum<PL_NSUM>(v, slab + (size_t)blockIdx.x * PL_SLAB);
}

// A (upper triangle, row by row) z = -b by an unpivoted Cholesky decomposition; false: rank below 6 (or a NaN)
__device__ bool pl_solve6(const double* __restrict__ S, double (&z)[6]) {
    double A[6][6], L[6][6];
    int m = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int l = k; l < 6; ++l) { A[k][l] = S[m]; A[l][k] = S[m]; ++m; }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double d = A[k][k];
#pragma unroll
        for (int q = 0; q < k; ++q) d -= L[k][q] * L[k][q];
        if (!(d > PL_PIVOT_TOL * A[k][k])) return false;
        L[k][k] = sqrt(d);
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            double s = A[i][k];
#pragma unroll
            for (int q = 0; q < k; ++q) s -= L[i][q] * L[k][q];
            L[i][k] = s / L[k][k];
        }
    }
    double y[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double s = -S[21 + k];
#pragma unroll
        for (int q = 0; q < k; ++q) s -= L[k][q] * y[q];
        y[k] = s / L[k][k];
    }
#pragma unroll
    for (int k = 5; k >= 0; --k) {
        double s = y[k];
#pragma unroll
        for (int q = k + 1; q < 6; ++q) s -= L[q][k] * z[q];
        z[k] = s / L[k][k];
    }
    return true;
}

// dR = exp([w]x) = I + a K + b K^2, a = sin(th) / th, b = (1 - cos(th)) / th^2 = (sin(th / 2) / (th / 2))^2 / 2 (no cancellation);
// below th^2 = 1e-4 both by their series, whose first dropped terms are th^8 / 9! and th^8 / 10!
__device__ void pl_exp_so3(const double* w, double (&dR)[9]) {
    const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    double a, b;
    if (t2 < 1e-4) {
        a = 1.0 - t2 / 6.0 * (1.0 - t2 / 20.0 * (1.0 - t2 / 42.0));
        b = 0.5 - t2 / 24.0 * (1.0 - t2 / 30.0 * (1.0 - t2 / 56.0));
    } else {
        const double th = sqrt(t2), h = sin(0.5 * th) / (0.5 * th);
        a = sin(th) / th;
        b = 0.5 * h * h;
    }
    const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double k2 = w[i] * w[j] - (i == j ? t2 : 0.0);       // K^2 = w w^T - |w|^2 I
            dR[3 * i + j] = (i == j ? 1.0 : 0.0) + a * K[3 * i + j] + b * k2;
        }
}

// one wave: the slabs of the second pass in block order -> rmse, the solve, T_{i+1} and the four stop rules in their order
__global__ __launch_bounds__(64) void pl_solve_kernel(PlState* __restrict__ st, const double* __restrict__ slab, int nblk, int it, int iters, double tol,
                                                      double* __restrict__ rmse) {
    if (st->stop) return;
    __shared__ double S[PL_NSUM];
    rf_slab_total<PL_NSUM>(slab, nblk, PL_SLAB, S);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int n = st->n;
    rmse[it] = n > 0 ? sqrt(S[27] / (double)n) : __builtin_inf();
    if (n < PL_MIN_PAIRS) { st->stop = 1; st->reason = YOHO_ICP_FEW_PAIRS; return; }
    double z[6], dR[9], T[12];
    if (!pl_solve6(S, z)) { st->stop = 1; st->reason = YOHO_ICP_RANK; return; }
    pl_exp_so3(z, dR);
    const double d[3] = {st->T[3] - st->c[0], st->T[7] - st->c[1], st->T[11] - st->c[2]};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) T[4 * i + j] = (dR[3 * i] * st->T[j] + dR[3 * i + 1] * st->T[4 + j]) + dR[3 * i + 2] * st->T[8 + j];
        T[4 * i + 3] = ((((dR[3 * i] * d[0] + dR[3 * i + 1] * d[1]) + dR[3 * i + 2] * d[2])) + st->c[i]) + z[3 + i];
    }
    double delta = 0.0;
    bool nan = false;
#pragma unroll
    for (int i = 0; i < 12; ++i) { const double dd = fabs(T[i] - st->T[i]); nan = nan || !(dd == dd); delta = fmax(delta, dd); st->T[i] = T[i]; }
    if (!nan && delta <= tol) { st->stop = 1; st->reason = YOHO_ICP_CONVERGED; }
    else if (it + 1 == iters) { st->stop = 1; st->reason = YOHO_ICP_ITERS; }
}

__global__ void pl_finish_kernel(const PlState* __restrict__ st, double* __restrict__ T_out, int32_t* __restrict__ info) {
    const int t = threadIdx.x;
    if (t < 12) T_out[t] = st->T[t];
    if (t == 0) { info[0] = st->done; info[1] = st->reason; }
}

}  // namespace yoho

using namespace yoho;

extern "C" {

int yoho_estimate_normals(yoho_ctx* c, const float* pts, int N, float radius, int min_nbrs, float vx, float vy, float vz, float* normals, int32_t* count,
                          float* curv, void* stream) {
    const char* fn = "yoho_estimate_normals";
    int rc;
    if ((rc = rf_check_cloud(fn, c, N, "radius", radius))) return rc;
    if (min_nbrs < 3) { set_error("yoho_estimate_normals: min_nbrs=%d must be at least 3", min_nbrs); return YOHO_EINVAL; }
    if (!std::isfinite(vx) || !std::isfinite(vy) || !std::isfinite(vz)) {
        set_error("yoho_estimate_normals: viewpoint (%g, %g, %g) must be finite", (double)vx, (double)vy, (double)vz);
        return YOHO_EINVAL;
    }
    if ((rc = rf_check_pointers(fn, pts && normals && count))) return rc;
    YOHO_NEED_ALIGNED("yoho_estimate_normals", 3, pts, normals, count, curv);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    RfGridWs w;
    if ((rc = bind_ws(c, s, [&](Arena& ar) { rf_grid_layout(ar, N, w); }))) return rc;
    RfGrid g;
    if ((rc = rf_build_grid(pts, N, radius, w, g, s))) return rc;
    hipLaunchKernelGGL(pl_normals_kernel, dim3((N + 255) / 256), dim3(256), 0, s, g, pts, N, min_nbrs, vx, vy, vz, normals, count, curv);
    HIPCHK(hipGetLastError());
    return 0;
}

int yoho_icp_plane(yoho_ctx* c, const float* src, int Ns, const float* tgt, int Nt, const float* tgt_normals, const double* T_in, float max_dist, int iters,
                   double tol, double* T_out, int32_t* npairs, double* rmse, int32_t* info, void* stream) {
    const char* fn = "yoho_icp_plane";
    int rc;
    if ((rc = rf_check_icp(fn, c, Ns, Nt, iters, max_dist, tol)) ||
        (rc = rf_check_pointers(fn, src && tgt && tgt_normals && T_in && T_out && info && (iters == 0 || (npairs && rmse))))) return rc;
    YOHO_NEED_ALIGNED("yoho_icp_plane", 3, src, tgt, tgt_normals, npairs, info);
    YOHO_NEED_ALIGNED("yoho_icp_plane", 7, T_in, T_out, rmse);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int nblk = (Ns + 255) / 256;
    PlState* st = nullptr;
    double* slab = nullptr;
    int* pair = nullptr;
    RfGridWs w;
    if ((rc = bind_ws(c, s, [&](Arena& ar) {
            st = ar.take<PlState>(1);
            slab = ar.take<double>((size_t)PL_SLAB * nblk);
            pair = ar.take<int>((size_t)Ns);
            if (iters > 0) rf_grid_layout(ar, Nt, w);
        }))) return rc;
    hipLaunchKernelGGL(pl_init_kernel, dim3(1), dim3(64), 0, s, st, T_in, npairs, rmse, iters);
    HIPCHK(hipGetLastError());
    if (iters > 0) {
        RfGrid g;
        if ((rc = rf_build_grid(tgt, Nt, max_dist, w, g, s))) return rc;
        for (int it = 0; it < iters; ++it) {
            hipLaunchKernelGGL(pl_pair_kernel, dim3(nblk), dim3(256), 0, s, (const PlState*)st, g, src, Ns, tgt_normals, pair, slab);
            hipLaunchKernelGGL(pl_mean_kernel, dim3(1), dim3(64), 0, s, st, (const double*)slab, nblk, it, npairs);
            hipLaunchKernelGGL(pl_normeq_kernel, dim3(nblk), dim3(256), 0, s, (const PlState*)st, src, Ns, tgt, tgt_normals, (const int*)pair, slab);
            hipLaunchKernelGGL(pl_solve_kernel, dim3(1), dim3(64), 0, s, st, (const double*)slab, nblk, it, iters, tol, rmse);
            HIPCHK(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(pl_finish_kernel, dim3(1), dim3(64), 0, s, (const PlState*)st, T_out, info);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
