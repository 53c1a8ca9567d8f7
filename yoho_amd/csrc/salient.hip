// ISS saliency and Poisson-disk thinning in the order of a caller's priority (include/yoho_salient.h).  Compiled with
// -ffp-contract=off like plane.hip and disk.hip (yoho_amd/build.py).  The cell-sorted grid comes from rfgrid.hip / rfgrid.h (THE GRID,
// THE QUERY's exactness argument) unchanged.
//
//   sl_saliency_kernel  yoho_iss_saliency: one lane per point over the 27 cells around it, ten accumulators, a 3 x 3 Jacobi for the
//                       eigenvalues alone, the eligibility rule
//
// THE SALIENCY.  The count and the ten sums are rfgrid.h's rf_moments (THE DISTINCT BUCKETS), as for the normals of plane.hip: every
// bucket is walked once and count is exact.  The eigenvalues are rffit.h's rf_eig3 without the eigenvectors: the response needs the
// eigenvalues only.  They are clamped at 0 (a rounded Jacobi can leave -1e-20 where the exact value is 0), sorted, and the
// eligibility is decided on the clamped values with one rounded multiply each, so prio can be recomputed bit for bit from eig and count.
//
// THE THINNING of yoho_disk_sample_prio is disk.hip's (THE ROUNDS, THE KEY there), reached through dkthin.h: this file has the entry's
// argument checks and nothing else of it.
//
// Registers (hipcc -O3, gfx950) and timings: tools/time_salient.py -> profiles/salient.md; the kernel of this file uses no scratch.
#include "rfgrid.h"
#include "rffit.h"
#include "dkthin.h"
#include "yoho_salient.h"
#include <cmath>

namespace yoho {

__global__ __launch_bounds__(256) void sl_saliency_kernel(RfGrid g, const float* __restrict__ pts, int N, int min_nbrs, double gamma21, double gamma32,
                                                          int32_t* __restrict__ count, double* __restrict__ eig, float* __restrict__ prio) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    float q[3];
    rf_load_row(pts, i, q);
    int n;
    double S1[3], S2[6];
    rf_moments(g, q, n, S1, S2);
    count[i] = n;
    double l1 = 0.0, l2 = 0.0, l3 = 0.0;
    if (n > 0) {
        const double dn = (double)n;
        const double C[6] = {(S2[0] - S1[0] * S1[0] / dn) / dn, (S2[1] - S1[0] * S1[1] / dn) / dn, (S2[2] - S1[0] * S1[2] / dn) / dn,
                             (S2[3] - S1[1] * S1[1] / dn) / dn, (S2[4] - S1[1] * S1[2] / dn) / dn, (S2[5] - S1[2] * S1[2] / dn) / dn};
        double lam[3];
        rf_eig3<false>(C, lam, nullptr);
#pragma unroll
        for (int k = 0; k < 3; ++k) lam[k] = lam[k] > 0.0 ? lam[k] : 0.0;          // the clamp: +0 for -0 and for a negative rounding residue
        l1 = fmin(fmin(lam[0], lam[1]), lam[2]);
        l3 = fmax(fmax(lam[0], lam[1]), lam[2]);
        l2 = fmax(fmin(lam[0], lam[1]), fmin(fmax(lam[0], lam[1]), lam[2]));      // the median of three
    }
    if (eig) { eig[3 * (size_t)i] = l1; eig[3 * (size_t)i + 1] = l2; eig[3 * (size_t)i + 2] = l3; }
    const bool eligible = n >= min_nbrs && l2 < gamma21 * l3 && l1 < gamma32 * l2;
    prio[i] = eligible ? (float)l1 : __int_as_float(0x7fc00000);
}

}  // namespace yoho

using namespace yoho;

extern "C" {

int yoho_iss_saliency(yoho_ctx* c, const float* pts, int N, float radius, int min_nbrs, double gamma21, double gamma32, int32_t* count, double* eig,
                      float* prio, void* stream) {
    const char* fn = "yoho_iss_saliency";
    int rc;
    if ((rc = rf_check_cloud(fn, c, N, "radius", radius))) return rc;
    if (min_nbrs < 3) return RF_REFUSE("%s: min_nbrs=%d must be at least 3", fn, min_nbrs);
    if (!(gamma21 > 0.0 && gamma21 <= 1.0)) return RF_REFUSE("%s: gamma21=%g must be finite and in (0, 1]", fn, gamma21);      // false for a NaN
    if (!(gamma32 > 0.0 && gamma32 <= 1.0)) return RF_REFUSE("%s: gamma32=%g must be finite and in (0, 1]", fn, gamma32);
    if (!pts) return RF_REFUSE("%s: bad argument (pts is NULL)", fn);
    if (!count) return RF_REFUSE("%s: bad argument (count is NULL)", fn);
    if (!prio) return RF_REFUSE("%s: bad argument (prio is NULL)", fn);
    YOHO_NEED_ALIGNED("yoho_iss_saliency", 3, pts, count, prio);
    YOHO_NEED_ALIGNED("yoho_iss_saliency", 7, eig);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    RfGridWs w;
    if ((rc = bind_ws(c, s, [&](Arena& ar) { rf_grid_layout(ar, N, w); }))) return rc;
    RfGrid g;
    if ((rc = rf_build_grid(pts, N, radius, w, g, s))) return rc;
    hipLaunchKernelGGL(sl_saliency_kernel, dim3((N + 255) / 256), dim3(256), 0, s, g, pts, N, min_nbrs, gamma21, gamma32, count, eig, prio);
    HIPCHK(hipGetLastError());
    return 0;
}

int yoho_disk_sample_prio(yoho_ctx* c, const float* pts, int N, float radius, const float* prio, uint32_t seed, int rounds, int resume, uint8_t* state,
                          int32_t* n_out, void* stream) {
    const char* fn = "yoho_disk_sample_prio";
    int rc;
    if ((rc = rf_check_cloud(fn, c, N, "radius", radius)) || (rc = rf_check_range(fn, "rounds", rounds, 1, RF_NAMED(YOHO_SALIENT_MAX_ROUNDS)))) return rc;
    if (resume != 0 && resume != 1) return RF_REFUSE("%s: resume=%d must be 0 or 1", fn, resume);
    if (!pts) return RF_REFUSE("%s: bad argument (pts is NULL)", fn);
    if (!prio) return RF_REFUSE("%s: bad argument (prio is NULL)", fn);
    if (!state) return RF_REFUSE("%s: bad argument (state is NULL)", fn);
    if (!n_out) return RF_REFUSE("%s: bad argument (n_out is NULL)", fn);
    YOHO_NEED_ALIGNED("yoho_disk_sample_prio", 3, pts, prio, n_out);
    return dk_thin(c, pts, N, radius, prio, (unsigned)seed, rounds, resume, state, n_out, (hipStream_t)stream);
}

}  // extern "C"
