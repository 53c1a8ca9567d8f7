// ISS saliency and Poisson-disk thinning in the order of a caller's priority (include/yoho_salient.h).  Compiled with
// -ffp-contract=off like plane.hip and disk.hip (yoho_amd/build.py).  The cell-sorted grid comes from rfgrid.hip / rfgrid.h (THE GRID,
// THE QUERY's exactness argument) unchanged.
//
//   sl_saliency_kernel  yoho_iss_saliency: one lane per point over the 27 cells around it, ten accumulators, a 3 x 3 Jacobi for the
//                       eigenvalues alone, the eligibility rule
//   sp_zero_kernel      one workgroup: the round counters cnt[0 .. YOHO_SALIENT_MAX_ROUNDS] and n_out[0] = 0
//   sp_init_kernel      one lane per row: key64[i]; resume = 0 writes state[i] = 0 (finite) or 2, resume = 1 turns a non-finite row
//                       handed in as 0 into 2; cnt[0] += the undecided rows of the block
//   sp_round_kernel     round r = 1 .. rounds, one launch each, eight lanes per row: src -> dst, cnt[r] += the rows the block leaves
//                       undecided; the launch returns at once when cnt[r - 1] == 0
//   sp_tail_kernel      the number of rounds that ran from cnt[], the final state into `state`, n_out
//
// RESTATED, NOT SHARED.  The walk over the 27 cells, the bucket de-duplication and the Jacobi iteration are plane.hip's
// (pl_normals_kernel, pl_eig3) and the round structure is disk.hip's (dk_*), written out again here as disk.hip wrote out the walk:
// the tests of plane.hip, disk.hip, clean.hip and cluster.hip pin their include lists and kernel censuses, so those files stay as
// they are.
//
// THE SALIENCY follows THE NORMALS of plane.hip: every row has work, so one lane per point keeps n, S1 (3) and S2 (6) in registers
// with no cross-lane sum, whose order would have to be fixed as well.  The 27 slots are computed first and a slot equal to an earlier
// one is skipped, so every bucket is walked once and count is exact.  The Jacobi leaves the eigenvector updates out (nine fewer
// live doubles and a dozen fewer multiplies a rotation): the response needs the eigenvalues only.  They are clamped at 0 (a rounded
// Jacobi can leave -1e-20 where the exact value is 0), sorted, and the eligibility is decided on the clamped values with one rounded
// multiply each, so prio can be recomputed bit for bit from eig and count.
//
// THE ROUNDS are disk.hip's: synchronous, round r reads the buffer round r - 1 wrote and writes the other one, every byte of it, so no
// lane ever reads a byte that another lane of the same launch writes.  The two buffers are the caller's `state` (A) and N bytes of the
// workspace (B).  What a launch reads - the other buffer, cnt[r - 1], the keys - was stored by EARLIER launches on the stream, which is
// the only visibility the hardware gives for free: the per-XCD L2s are not coherent with each other inside a launch, and the kernel
// boundary is the only synchronisation.  In place the final set would be the same (it is unique), the round count and every
// intermediate state would not.  SP_LANES = 8 lanes share a row, SP_BATCH = 8 candidates of a bucket are in flight at once, two
// ballots hand what the lanes found to the row's first lane.  A candidate met twice (two of the 27 cells sharing a bucket) changes
// neither "a preceding neighbour is kept" nor "none is undecided".
//   THE KEY of a neighbour is the new cost: key64 depends on prio[j], so it cannot be recomputed from the row index as disk.hip does.
//   sp_init_kernel writes key64 of every row into the workspace; in a batch the key and the state of every candidate that passes
//   the gate are loaded TOGETHER - two independent gathers behind the point loads, not a key load in front of the state load - and
//   compared afterwards.  A candidate outside the gate loads neither.  The keys are in row order; a copy in the grid's sorted order
//   beside pk[] would save the gather and is left out until profiles/salient.md says the key loads matter.
//
// No kernel waits for another lane or workgroup: no spin, no flag, no cooperative launch, no grid barrier.  Every workspace byte is
// written (the grid build, sp_zero_kernel, sp_init_kernel's keys, every byte of B by the first round) before it is read: with
// rounds >= 1 round 1 always has a launch, and it either writes all of B or, with cnt[0] == 0, no later launch reads B.  Registers
// (hipcc -O3, gfx950) and timings: tools/time_salient.py -> profiles/salient.md; no kernel of this file uses scratch.
#include "rfgrid.h"
#include "yoho_salient.h"
#include <cmath>

namespace yoho {

// ---- saliency ------------------------------------------------------------------------------------------------------------------------
// symmetric 3 x 3 (a = {xx, xy, xz, yy, yz, zz}) -> eigenvalues lam[3] (unsorted): plane.hip's cyclic two-sided Jacobi without the
// eigenvectors.  A rotation is skipped once the off-diagonal entry is below 2^-58 of the two diagonal entries it couples: an absolute
// perturbation of an eigenvalue that small is far inside the bound of tests/test_gpu_salient.py (Weyl).
__device__ void sl_eig3(const double (&a)[6], double (&lam)[3]) {
    double A[3][3] = {{a[0], a[1], a[2]}, {a[1], a[3], a[4]}, {a[2], a[4], a[5]}};
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
            }
        }
        if (!rotated) break;
    }
    lam[0] = A[0][0]; lam[1] = A[1][1]; lam[2] = A[2][2];
}

__global__ __launch_bounds__(256) void sl_saliency_kernel(RfGrid g, const float* __restrict__ pts, int N, int min_nbrs, double gamma21, double gamma32,
                                                          int32_t* __restrict__ count, double* __restrict__ eig, float* __restrict__ prio) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float q[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
    const double px = (double)q[0], py = (double)q[1], pz = (double)q[2];
    const int cx = rf_cell(px, g.inv_cell), cy = rf_cell(py, g.inv_cell), cz = rf_cell(pz, g.inv_cell);
    unsigned slot[27];
#pragma unroll
    for (int c = 0; c < 27; ++c) slot[c] = rf_slot(rf_clampi(cx + c % 3 - 1), rf_clampi(cy + (c / 3) % 3 - 1), rf_clampi(cz + c / 9 - 1), g.mask);
    int n = 0;
    double s1x = 0.0, s1y = 0.0, s1z = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
#pragma unroll
    for (int c = 0; c < 27; ++c) {
        bool seen = false;
#pragma unroll
        for (int k = 0; k < c; ++k) seen = seen || slot[k] == slot[c];
        if (seen) continue;                                           // a bucket is walked once
        const int p1 = g.start[slot[c] + 1];
        for (int p = g.start[slot[c]]; p < p1; ++p) {
            const float4 v = g.pk[p];
            const float b[3] = {v.x, v.y, v.z};
            if (dist2_f32<3>(q, b) < g.gate2) {                       // false for a NaN / inf on either side
                const double dx = (double)v.x - px, dy = (double)v.y - py, dz = (double)v.z - pz;
                ++n;
                s1x += dx; s1y += dy; s1z += dz;
                sxx += dx * dx; sxy += dx * dy; sxz += dx * dz;
                syy += dy * dy; syz += dy * dz; szz += dz * dz;
            }
        }
    }
    count[i] = n;
    double l1 = 0.0, l2 = 0.0, l3 = 0.0;
    if (n > 0) {
        const double dn = (double)n;
        const double C[6] = {(sxx - s1x * s1x / dn) / dn, (sxy - s1x * s1y / dn) / dn, (sxz - s1x * s1z / dn) / dn,
                             (syy - s1y * s1y / dn) / dn, (syz - s1y * s1z / dn) / dn, (szz - s1z * s1z / dn) / dn};
        double lam[3];
        sl_eig3(C, lam);
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

// ---- thinning ------------------------------------------------------------------------------------------------------------------------
constexpr int SP_COUNTERS = YOHO_SALIENT_MAX_ROUNDS + 1;   // cnt[r] = the rows undecided after round r, cnt[0] at entry
constexpr int SP_BATCH = 8;                                // candidates of a bucket a lane has in flight at once (THE ROUNDS)
constexpr int SP_LANES = 8;                                // lanes that share the 27 buckets around a row: a power of two, a divisor of 64
constexpr int SP_CELLS = (27 + SP_LANES - 1) / SP_LANES;   // buckets per lane
constexpr int SP_ROWS = 256 / SP_LANES;                    // rows per workgroup of sp_round_kernel

// include/yoho_salient.h PRIORITY
__device__ __forceinline__ u64 sp_key64(unsigned i, unsigned seed, float p) {
    unsigned x = i ^ seed;
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    const unsigned b = (unsigned)__float_as_int(p);
    const unsigned ord = p != p ? 0u : ((b & 0x80000000u) ? ~b : (b | 0x80000000u));
    return ((u64)(~ord) << 32) | (u64)x;
}

__global__ __launch_bounds__(128) void sp_zero_kernel(int* __restrict__ cnt, int32_t* __restrict__ n_out) {
    if (threadIdx.x < SP_COUNTERS) cnt[threadIdx.x] = 0;
    if (threadIdx.x == 0) n_out[0] = 0;
}

__global__ __launch_bounds__(256) void sp_init_kernel(const float* __restrict__ pts, const float* __restrict__ prio, int N, unsigned seed, int resume,
                                                      uint8_t* __restrict__ state, u64* __restrict__ key, int* __restrict__ cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool und = false;
    if (i < N) {
        key[i] = sp_key64((unsigned)i, seed, prio[i]);
        const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
        const bool finite = fabsf(x) < __builtin_inff() && fabsf(y) < __builtin_inff() && fabsf(z) < __builtin_inff();      // false for a NaN
        uint8_t s = finite ? 0 : 2;
        if (resume) {
            const uint8_t given = state[i];
            if (given != 0) s = given;                                  // decided by whoever wrote it: copied through
        }
        state[i] = s;
        und = s == 0;
    }
    const int n = __syncthreads_count(und);
    if (threadIdx.x == 0 && n > 0) atomicAdd(&cnt[0], n);
}

// round r: prev = cnt + r - 1 (the rows the round before left undecided), prev[1] this round's counter.  SP_LANES lanes per row
__global__ __launch_bounds__(256) void sp_round_kernel(RfGrid g, const float* __restrict__ pts, int N, const u64* __restrict__ key,
                                                       const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int* __restrict__ prev) {
    if (prev[0] == 0) return;                                             // uniform: the thinning is complete, dst is never read
    const int sub = threadIdx.x & (SP_LANES - 1);
    const int i = blockIdx.x * SP_ROWS + (threadIdx.x / SP_LANES);
    uint8_t s = 2;
    if (i < N) s = src[i];
    const bool walk = i < N && s == 0;                                    // a decided row costs this one byte and its copy
    bool open = false, dropped = false;                                   // a preceding neighbour undecided / kept, among this lane's buckets
    if (walk) {
        const float q[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
        const u64 ki = key[i];
        const int cx = rf_cell((double)q[0], g.inv_cell), cy = rf_cell((double)q[1], g.inv_cell), cz = rf_cell((double)q[2], g.inv_cell);
        int p0[SP_CELLS], p1[SP_CELLS];
#pragma unroll
        for (int k = 0; k < SP_CELLS; ++k) {                              // the ranges of the lane's buckets, all on their way at once
            const int c = sub + k * SP_LANES;
            p0[k] = p1[k] = 0;
            if (c < 27) {
                const unsigned sl = rf_slot(rf_clampi(cx + c % 3 - 1), rf_clampi(cy + (c / 3) % 3 - 1), rf_clampi(cz + c / 9 - 1), g.mask);
                p0[k] = g.start[sl];
                p1[k] = g.start[sl + 1];
            }
        }
#pragma unroll
        for (int k = 0; k < SP_CELLS; ++k) {
#pragma unroll 1
            for (int p = p0[k]; p < p1[k]; p += SP_BATCH) {               // SP_BATCH candidates at a time: their loads are in flight together
                float4 v[SP_BATCH];
#pragma unroll
                for (int u = 0; u < SP_BATCH; ++u) v[u] = g.pk[p + u < p1[k] ? p + u : p1[k] - 1];
                uint8_t sj[SP_BATCH];
                u64 kj[SP_BATCH];
#pragma unroll
                for (int u = 0; u < SP_BATCH; ++u) {
                    const float b[3] = {v[u].x, v[u].y, v[u].z};
                    const float d2 = dist2_f32<3>(q, b);
                    const int j = __float_as_int(v[u].w);
                    // false for a NaN / inf on either side; a slot behind the bucket's end repeats its last point.  The key and the
                    // state of a candidate inside the gate are two independent loads (THE KEY); j == i has kj == ki and counts nothing
                    const bool in = d2 < g.gate2;
                    kj[u] = in ? key[j] : ~0ull;
                    sj[u] = in ? src[j] : (uint8_t)2;
                }
#pragma unroll
                for (int u = 0; u < SP_BATCH; ++u) {
                    const bool before = kj[u] < ki;
                    dropped = dropped || (before && sj[u] == 1);
                    open = open || (before && sj[u] == 0);
                }
            }
        }
    }
    // what the row's lanes found, to its first lane: the SP_LANES bits of the row in the wave's ballots (every lane of the wave is here)
    const int first = (threadIdx.x & 63) & ~(SP_LANES - 1);
    const bool any_dropped = ((__ballot(dropped) >> first) & ((1ull << SP_LANES) - 1ull)) != 0ull;
    const bool any_open = ((__ballot(open) >> first) & ((1ull << SP_LANES) - 1ull)) != 0ull;
    bool und = false;
    if (i < N && sub == 0) {
        if (walk) s = any_dropped ? 2 : (any_open ? 0 : 1);
        dst[i] = s;
        und = s == 0;
    }
    const int n = __syncthreads_count(und);
    if (threadIdx.x == 0 && n > 0) atomicAdd(&prev[1], n);
}

// cnt[r] > 0 implies cnt[r - 1] > 0 (a round that does not run leaves its counter 0), so the rounds that ran are the r < rounds with
// cnt[r] > 0; the state they left is in B when their number is odd
__global__ __launch_bounds__(256) void sp_tail_kernel(int N, int rounds, const int* __restrict__ cnt, const uint8_t* __restrict__ B,
                                                      uint8_t* __restrict__ state, int32_t* __restrict__ n_out) {
    const int ran = __syncthreads_count((int)threadIdx.x < rounds && cnt[threadIdx.x] > 0);
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool kept = false;
    if (i < N) {
        uint8_t s;
        if (ran & 1) {
            s = B[i];
            state[i] = s;
        } else {
            s = state[i];
        }
        kept = s == 1;
    }
    const int n = __syncthreads_count(kept);
    if (threadIdx.x == 0) {
        if (n > 0) atomicAdd(&n_out[0], n);
        if (blockIdx.x == 0) { n_out[1] = ran; n_out[2] = cnt[ran]; }
    }
}

}  // namespace yoho

using namespace yoho;

extern "C" {

int yoho_iss_saliency(yoho_ctx* c, const float* pts, int N, float radius, int min_nbrs, double gamma21, double gamma32, int32_t* count, double* eig,
                      float* prio, void* stream) {
    const char* fn = "yoho_iss_saliency";
    int rc;
    if ((rc = rf_check_sizes(fn, c, "N", N, 1)) || (rc = rf_check_limit(fn, RF_NAMED(YOHO_REFINE_MAX_POINTS), "N", N)) ||
        (rc = rf_check_radius(fn, "radius", radius))) return rc;
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
    if ((rc = rf_check_sizes(fn, c, "N", N, 1)) || (rc = rf_check_limit(fn, RF_NAMED(YOHO_REFINE_MAX_POINTS), "N", N)) ||
        (rc = rf_check_radius(fn, "radius", radius)) || (rc = rf_check_range(fn, "rounds", rounds, 1, RF_NAMED(YOHO_SALIENT_MAX_ROUNDS)))) return rc;
    if (resume != 0 && resume != 1) return RF_REFUSE("%s: resume=%d must be 0 or 1", fn, resume);
    if (!pts) return RF_REFUSE("%s: bad argument (pts is NULL)", fn);
    if (!prio) return RF_REFUSE("%s: bad argument (prio is NULL)", fn);
    if (!state) return RF_REFUSE("%s: bad argument (state is NULL)", fn);
    if (!n_out) return RF_REFUSE("%s: bad argument (n_out is NULL)", fn);
    YOHO_NEED_ALIGNED("yoho_disk_sample_prio", 3, pts, prio, n_out);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    uint8_t* B = nullptr;
    int* cnt = nullptr;
    u64* key = nullptr;
    RfGridWs w;
    if ((rc = bind_ws(c, s, [&](Arena& ar) {
            B = ar.take<uint8_t>((size_t)N);
            cnt = ar.take<int>((size_t)SP_COUNTERS);
            key = ar.take<u64>((size_t)N);
            rf_grid_layout(ar, N, w);
        }))) return rc;
    RfGrid g;
    if ((rc = rf_build_grid(pts, N, radius, w, g, s))) return rc;
    const dim3 grid((N + 255) / 256), block(256);
    hipLaunchKernelGGL(sp_zero_kernel, dim3(1), dim3(128), 0, s, cnt, n_out);
    hipLaunchKernelGGL(sp_init_kernel, grid, block, 0, s, pts, prio, N, (unsigned)seed, resume, state, key, cnt);
    for (int r = 1; r <= rounds; ++r) {
        const uint8_t* src = (r & 1) ? state : B;
        uint8_t* dst = (r & 1) ? B : state;
        hipLaunchKernelGGL(sp_round_kernel, dim3((N + SP_ROWS - 1) / SP_ROWS), block, 0, s, g, pts, N, (const u64*)key, src, dst, cnt + (r - 1));
    }
    hipLaunchKernelGGL(sp_tail_kernel, grid, block, 0, s, N, rounds, (const int*)cnt, (const uint8_t*)B, state, n_out);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
