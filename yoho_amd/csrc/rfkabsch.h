// THE KABSCH STEP's 3 x 3 part (include/yoho_refine.h), shared by refine.hip and consist.hip the way rfgrid.h shares the grid and the
// sums: H = U S V^T by one-sided Jacobi, the proper rotation, the rank test.  Where the step sits in an iteration is described in
// refine.hip.  Include from translation units compiled with -ffp-contract=off only.
#pragma once
#include "rfgrid.h"

namespace yoho {

constexpr int RF_SLAB = 16;          // doubles per slab row of a Kabsch pass (8 or 9 used)
constexpr double RF_RANK_TOL = 1e-13;

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

}  // namespace yoho
