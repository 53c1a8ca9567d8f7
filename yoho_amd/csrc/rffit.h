// THE KABSCH STEP (include/yoho_refine.h) in pieces, shared by refine.hip, plane.hip, verify.hip and consist.hip: the fixed-order f64
// sums, the rounded transform of a point, centroids, centred products, the 3 x 3 solve, the [R | t] row; and the symmetric 3 x 3
// eigen-solve of plane.hip's normals and salient.hip's saliency (rf_eig3).  No grid here (rfgrid.h).
// Include from translation units compiled with -ffp-contract=off only.
//
// THE SUMS (the header's "THE SUM").  A pass writes the partial sums of its 256 elements to a slab at its block index (rf_block_sum):
// every lane's value through a __shfl_xor butterfly (offsets 32 .. 1: lane 0 ends with the halving tree, f64 addition being
// commutative), the four waves' results added in order by thread 0.  A one-wave kernel adds the slab rows in block order, one thread
// per component (rf_slab_total).  No float atomics, no grid-wide barrier: the kernel boundary is the synchronisation
// (cdna_hip_programming.md Guideline 12, slab-and-sum).  Two passes per Kabsch step - centroids first, centred products second -
// because one pass of raw products about a fixed origin cancels |centroid - origin|^2 / spread^2 of its bits, and the tolerance of
// tests/test_gpu_refine.py is a few ulps of numpy's own.  rf_slab_total is SERIAL, nblk dependent f64 additions per component - 79
// blocks at 20 000 points, 1172 at 300 000, 16 384 at the limit: the price of the stated order with the simplest kernels.  A two-level
// version (per-thread partial runs in block order, combined in order) keeps the order; this is the one place to write it.
#pragma once
#include "common.h"

namespace yoho {

constexpr int RF_SLAB = 16;          // doubles per slab row of a Kabsch pass (8 or 9 used)
constexpr double RF_RANK_TOL = 1e-13;

// ---- the sums ------------------------------------------------------------------------------------------------------------------
template <int NV>
__device__ __forceinline__ void rf_block_sum(double (&v)[NV], double* __restrict__ slab_row) {
    __shared__ double red[4][NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v[k] = __dadd_rn(v[k], __shfl_xor(v[k], o));
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) red[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const int k = threadIdx.x;
        slab_row[k] = __dadd_rn(__dadd_rn(__dadd_rn(red[0][k], red[1][k]), red[2][k]), red[3][k]);
    }
}

// out[k] = the rows' component k added in block order, by thread k < NV; `slab` is the first row (a row-strided caller passes its
// row's base), `out` the caller's __shared__ array, and the __syncthreads() behind it is the caller's too
template <int NV>
__device__ __forceinline__ void rf_slab_total(const double* __restrict__ slab, int nblk, int stride, double* out) {
    if (threadIdx.x < NV) {
        double s = 0.0;
        for (int b = 0; b < nblk; ++b) s = __dadd_rn(s, slab[(size_t)b * stride + threadIdx.x]);
        out[threadIdx.x] = s;
    }
}

// ---- the pieces of a step ------------------------------------------------------------------------------------------------------
// x = ((r0 s0 + r1 s1) + r2 s2) + t per coordinate under T = [R | t], every operation rounded: of a widened point, and of source point e
__device__ __forceinline__ void rf_apply(const double* __restrict__ T, double s0, double s1, double s2, double (&x)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
        x[i] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(T[4 * i], s0), __dmul_rn(T[4 * i + 1], s1)), __dmul_rn(T[4 * i + 2], s2)), T[4 * i + 3]);
}
__device__ __forceinline__ void rf_apply(const double* __restrict__ T, const float* __restrict__ src, int e, double (&x)[3]) {
    rf_apply(T, (double)src[3 * (size_t)e], (double)src[3 * (size_t)e + 1], (double)src[3 * (size_t)e + 2], x);
}

// the 8-value first-pass row of a pair of f64 points: {1, ., a (3), b (3)}; v[1] is the caller's
__device__ __forceinline__ void rf_pair_row(const double* a, const double* b, double (&v)[8]) {
    v[0] = 1.0; v[2] = a[0]; v[3] = a[1]; v[4] = a[2]; v[5] = b[0]; v[6] = b[1]; v[7] = b[2];
}

// threads 0 .. 2: the centroids from the totals {n, ., SUM a (3), SUM b (3)} of a first pass
__device__ __forceinline__ void rf_centroids(const double* tot, int n, double* c0, double* c1) {
    if (threadIdx.x < 3) {
        c0[threadIdx.x] = n > 0 ? tot[2 + threadIdx.x] / (double)n : 0.0;
        c1[threadIdx.x] = n > 0 ? tot[5 + threadIdx.x] / (double)n : 0.0;
    }
}

// the second-pass row of a pair: the nine centred products H[i][j] = (b_i - c1_i)(a_j - c0_j); E = float (ICP) or double (refit, consensus)
template <class E>
__device__ __forceinline__ void rf_centred_products(const E* a, const E* b, const double* c0, const double* c1, double (&v)[9]) {
    double a_[3], b_[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        a_[i] = __dsub_rn((double)a[i], c0[i]);
        b_[i] = __dsub_rn((double)b[i], c1[i]);
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) v[i] = __dmul_rn(b_[i / 3], a_[i % 3]);
}

// T = [R | c0 - R c1], every operation rounded
__device__ __forceinline__ void rf_rigid_row(const double* R, const double* c0, const double* c1, double* T) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        T[4 * i] = R[3 * i]; T[4 * i + 1] = R[3 * i + 1]; T[4 * i + 2] = R[3 * i + 2];
        T[4 * i + 3] = __dsub_rn(c0[i], __dadd_rn(__dadd_rn(__dmul_rn(R[3 * i], c1[0]), __dmul_rn(R[3 * i + 1], c1[1])), __dmul_rn(R[3 * i + 2], c1[2])));
    }
}

// ---- the 3 x 3 solve -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void rf_cross(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// x normalised, y orthogonalised against it and normalised; false when nothing of y is left
__device__ __forceinline__ bool rf_orthonormal2(double* x, double* y) {
    const double nx = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    x[0] /= nx; x[1] /= nx; x[2] /= nx;
    const double d = x[0] * y[0] + x[1] * y[1] + x[2] * y[2];
    y[0] -= d * x[0]; y[1] -= d * x[1]; y[2] -= d * x[2];
    const double ny = sqrt(y[0] * y[0] + y[1] * y[1] + y[2] * y[2]);
    if (!(ny > 0.5)) return false;
    y[0] /= ny; y[1] /= ny; y[2] /= ny;
    return true;
}

// H = U S V^T by one-sided Jacobi on the columns of H (estim.hip kabsch3's iteration, on a full-rank matrix): H V = U S.  The proper
// rotation R = V diag(1, 1, det(V U^T)) U^T is formed as v1 u1^T + v2 u2^T + (v1 x v2)(u1 x u2)^T: with u3 = det(U) (u1 x u2) and
// v3 = det(V) (v1 x v2) the two are the same matrix, and the third singular direction - all noise for a planar set - is never
// divided by its singular value.  false: rank below 2 (s1 = 0, s2 <= RF_RANK_TOL s1, or a NaN), R untouched.
__device__ inline bool rf_rotation(const double* H, double* R) {
    double A[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
#pragma unroll
    for (int i = 0; i < 9; ++i) A[i] = H[i];
    for (int sweep = 0; sweep < 30; ++sweep) {
        double offmax = 0.0;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double al = A[p] * A[p] + A[3 + p] * A[3 + p] + A[6 + p] * A[6 + p];
            const double be = A[q] * A[q] + A[3 + q] * A[3 + q] + A[6 + q] * A[6 + q];
            const double ga = A[p] * A[q] + A[3 + p] * A[3 + q] + A[6 + p] * A[6 + q];
            const double nab = sqrt(al * be);
            if (fabs(ga) > 1e-16 * nab) {                             // relative test only (kabsch3): the answer does not depend on the unit of length
                offmax = fmax(offmax, fabs(ga) / nab);
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const double ap = A[r * 3 + p], aq = A[r * 3 + q];
                    A[r * 3 + p] = cs * ap - sn * aq;
                    A[r * 3 + q] = sn * ap + cs * aq;
                    const double vp = V[r * 3 + p], vq = V[r * 3 + q];
                    V[r * 3 + p] = cs * vp - sn * vq;
                    V[r * 3 + q] = sn * vp + cs * vq;
                }
            }
        }
        if (offmax < 1e-15) break;
    }
    double sg[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) sg[j] = sqrt(A[j] * A[j] + A[3 + j] * A[3 + j] + A[6 + j] * A[6 + j]);
    int i1 = 0;
    if (sg[1] > sg[i1]) i1 = 1;
    if (sg[2] > sg[i1]) i1 = 2;
    int i2 = (i1 + 1) % 3, i3 = (i1 + 2) % 3;
    if (sg[i3] > sg[i2]) { const int t = i2; i2 = i3; i3 = t; }
    if (!(sg[i1] > 0.0) || !(sg[i2] > RF_RANK_TOL * sg[i1])) return false;
    double u1[3], u2[3], u3[3], v1[3], v2[3], v3[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) { u1[r] = A[r * 3 + i1] / sg[i1]; v1[r] = V[r * 3 + i1]; u2[r] = A[r * 3 + i2] / sg[i2]; v2[r] = V[r * 3 + i2]; }
    // the frames are made orthonormal to rounding whatever the sweeps left; a second column parallel to the first is rank 1 after all
    if (!rf_orthonormal2(u1, u2) || !rf_orthonormal2(v1, v2)) return false;
    rf_cross(u1, u2, u3);
    rf_cross(v1, v2, v3);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[i * 3 + j] = v1[i] * u1[j] + v2[i] * u2[j] + v3[i] * u3[j];
    return true;
}

// ---- the symmetric 3 x 3 eigen-solve -------------------------------------------------------------------------------------------
// symmetric 3 x 3 (a = {xx, xy, xz, yy, yz, zz}) -> eigenvalues lam[3] (unsorted) and, with VECTORS, eigenvectors as the columns of V
// (row-major; without, V is not touched and may be null: nine fewer live doubles and a dozen fewer multiplies a rotation): cyclic
// two-sided Jacobi.  A rotation is skipped once the off-diagonal entry is below 2^-58 of the two diagonal entries it couples: an
// absolute perturbation that small moves an eigenvalue by no more (Weyl) and turns an eigenvector by 2^-58 / (relative gap), far inside
// the bounds of tests/test_gpu_plane.py and tests/test_gpu_salient.py.
template <bool VECTORS>
__device__ inline void rf_eig3(const double (&a)[6], double (&lam)[3], double* V) {
    double A[3][3] = {{a[0], a[1], a[2]}, {a[1], a[3], a[4]}, {a[2], a[4], a[5]}};
    if constexpr (VECTORS) {
#pragma unroll
        for (int i = 0; i < 9; ++i) V[i] = (i % 4 == 0) ? 1.0 : 0.0;
    }
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2, r = 3 - p - q;
            const double apq = A[p][q];
            if (fabs(apq) > 0x1p-58 * (fabs(A[p][p]) + fabs(A[q][q]))) {
                rotated = true;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                A[p][p] -= t * apq;
                A[q][q] += t * apq;
                A[p][q] = A[q][p] = 0.0;
                const double arp = A[r][p], arq = A[r][q];
                A[r][p] = A[p][r] = cs * arp - sn * arq;
                A[r][q] = A[q][r] = sn * arp + cs * arq;
                if constexpr (VECTORS) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const double vp = V[k * 3 + p], vq = V[k * 3 + q];
                        V[k * 3 + p] = cs * vp - sn * vq;
                        V[k * 3 + q] = sn * vp + cs * vq;
                    }
                }
            }
        }
        if (!rotated) break;
    }
    lam[0] = A[0][0]; lam[1] = A[1][1]; lam[2] = A[2][2];
}

}  // namespace yoho
