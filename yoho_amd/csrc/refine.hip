// Refinement behind the global estimators (include/yoho_refine.h): nearest neighbour inside a radius, iterated Kabsch on the inlier
// matches, gated point-to-point ICP.  Compiled with -ffp-contract=off like estim.hip / match.hip / gridnn.hip (yoho_amd/build.py).
//
//   rf_key / rf_hist / rf_scan / rf_scatter / rf_cells_kernel   the cell-sorted grid over the target cloud
//   rf_within_kernel                                             yoho_nn_within: one lane per query over 27 cells
//   rf_icp_pair_kernel                                           ICP: transform + the same walk + gate + first-pass partial sums
//   rf_refit_mask_kernel                                         refit: estim.hip's inlier() + first-pass partial sums
//   rf_mean_kernel / rf_*_cov_kernel / rf_solve_kernel           the Kabsch step: centroids, centred products, Jacobi, stop word
// The device-side pieces of the grid and of the sums (rf_cell, rf_slot, rf_walk, rf_block_sum) are in rfgrid.h, which plane.hip shares;
// the 3 x 3 part of the Kabsch step (rf_rotation) is in rfkabsch.h, which consist.hip shares.
//
// THE GRID.  gridnn.hip's grid (linked lists behind an open-addressing table, a wave and 125 probes per query, brute force for what it
// cannot settle) is built for queries that all have a partner nearby; in ICP half the cloud has none.  Here the targets are SORTED by
// cell: a point's cell (cx, cy, cz) = rf_cell of its coordinates - gridnn.hip's monotone clamped gn_cell - with cell side
// max_dist (1 + 2^-10), its bucket = a hash of the cell into a table of nslots >= 2 Nt slots.  The sort is a stable least-significant-
// digit counting sort of (bucket, original index) on 8-bit digits, two or three passes: rf_hist_kernel counts the digits of every
// 256-point block, rf_scan_kernel turns the [digit][block] counts into offsets (one workgroup, an exclusive scan), rf_scatter_kernel
// places every point at offset + (points of the same digit in front of it in its block), that rank from eight ballots and a
// popcount below the lane (estim.hip same_bucket_lanes, radius.hip's ranks) plus the counts of the waves in front.  No atomic
// decides a position (the LDS atomics of rf_hist_kernel only count), every pass is stable, so the points of a bucket end up
// contiguous in ascending original index: the build is deterministic.  rf_cells_kernel then finds every bucket's first sorted
// position by bisection and re-packs the points as float4 (x, y, z, original index), one 16-byte load per candidate.  Two cells that
// share a bucket share its range: a query then looks at points it did not need to, which costs time and changes nothing, because
// every point it looks at goes through the exact test below.  Every workspace byte is written by these kernels before it is read.
//
// THE QUERY.  One lane per query: the 27 cells around the query's own, for each the bucket's contiguous range, for each point
// d2 = dist2_f32<3> (nnmath.h, the brute-force kernels' arithmetic), kept when d2 < gate2 and (d2, index) is below the best so far.
// No second pass, no fallback.  The (d2, index) minimum does not depend on the order in which points are met, nor on a point
// being met twice (clamped neighbour cells, buckets shared by two of the 27), so the answer is the contract's if the 27 cells hold
// every candidate.  They do, whatever rounding does:
//   (1) rf_cell(x) = clamp(floor(fl(x inv)), +-(2^20 - 1)), inv = fl(1 / cell), in f64 on the exactly widened f32 coordinate.  One
//       rounding, floor and the clamp are all monotone, so rf_cell is monotone in x.  Let a query coordinate q and a target coordinate
//       t have rf_cell(t) >= rf_cell(q) + 2 and m = rf_cell(q) + 1, an integer strictly inside the clamp range.  Then fl(q inv) < m,
//       hence q inv < m (a product >= m rounds to >= m), and fl(t inv) >= m + 1, hence t inv >= (m + 1) - |m + 1| 2^-53 >= m + 1 - 2^-33.
//       So (t - q) inv > 1 - 2^-33 and, with inv <= (1 + 2^-53) / cell, t - q > cell (1 - 2^-32).  (Symmetric for q above t; a NaN
//       coordinate maps to the lowest cell and never passes the gate anyway.)
//   (2) cell = fl(max_dist (1 + 2^-10)) in f64 >= max_dist (1 + 2^-10)(1 - 2^-53), so |t - q| > max_dist (1 + 2^-11).
//   (3) d2 is a sum of three rounded squares of rounded differences, all >= 0, and an f32 sum of non-negative terms is >= each term:
//       d2 >= fl(fl(t - q)^2) >= (t - q)^2 (1 - 2^-24)^3 > max_dist^2 (1 + 2^-11) > fl(max_dist^2) = gate2 (an overflow gives
//       +inf or NaN, not below any gate).  So a target two or more cells away on any axis is not a candidate.
//       The relative bounds need normal numbers: for max_dist < 2^-60 the cell side is 2^-60 instead (a larger cell is always right),
//       which keeps (t - q)^2 > 2^-121 above every gate2 <= 2^-120 such a radius can have; max_dist^2 overflowing f32 makes gate2 +inf,
//       then every finite d2 is a candidate and every finite coordinate is in cell -1 or 0 of a cell side >= 1.8e19: inside the 27.
//
// THE SUMS (the header's "THE SUM").  A pass writes the partial sums of its 256 elements to a slab at its block index: every lane's
// value through a __shfl_xor butterfly (offsets 32 .. 1: lane 0 ends with the halving tree, f64 addition being commutative), the four
// waves' results added in order by thread 0.  A one-wave kernel adds the slabs in block order, one thread per component.  No float
// atomics, no grid-wide barrier: the kernel boundary is the synchronisation (cdna_hip_programming.md Guideline 12, slab-and-sum).
// Two passes per Kabsch step - centroids first, centred products second - because one pass of raw products about a fixed origin
// cancels |centroid - origin|^2 / spread^2 of its bits, and the tolerance of tests/test_gpu_refine.py is a few ulps of numpy's own.
//
// THE ITERATIONS.  All of them are queued at once.  rf_mean_kernel / rf_solve_kernel, one wave, keep the state of the call in device
// memory (RfState: the current transform, centroids, the stop word); a kernel that finds the stop word set returns at once - a
// wave-uniform branch on a loaded word.  Nothing is read back to the host.
//
// Registers (hipcc -O3, gfx950): rf_within_kernel 23 VGPRs, rf_icp_pair_kernel 38, the covariance passes 42, rf_refit_mask_kernel 46,
// rf_solve_kernel (one thread's Jacobi) 80; no scratch in any kernel of this file (.private_segment_fixed_size 0, no spills).
// Untuned at large sizes, for ICP as much as for the refit: rf_mean_kernel and rf_solve_kernel add the per-block slabs SERIALLY, one
// thread per component, nblk dependent f64 additions each, twice per iteration - 79 blocks at 20 000 points, 1172 at 300 000, 16 384 at
// the limit - and rf_scan_kernel is one workgroup scanning 256 nblk counts, two or three times per grid build.  That is the price of the
// stated summation order with the simplest kernels; a two-level version (per-thread partial runs in block order, combined in order) keeps
// the order and is the remedy if the 300 000-point timing asks for it.  Timings: tools/time_refine.py -> profiles/refine.md.
#include "rfgrid.h"
#include "rfkabsch.h"
#include "yoho_refine.h"
#include <cmath>

namespace yoho {

// ---- the sort ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rf_key_kernel(const float* __restrict__ pts, int n, double inv_cell, unsigned mask, unsigned* __restrict__ keys,
                                                     int* __restrict__ idx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* p = pts + 3 * (size_t)i;
    keys[i] = rf_slot(rf_cell((double)p[0], inv_cell), rf_cell((double)p[1], inv_cell), rf_cell((double)p[2], inv_cell), mask);
    idx[i] = i;
}

// hist[digit * nblk + block] = points of the block with that digit
__global__ __launch_bounds__(256) void rf_hist_kernel(const unsigned* __restrict__ keys, int n, int shift, int nblk, int* __restrict__ hist) {
    __shared__ int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255u], 1);          // counts only: the sum does not depend on the order of arrival
    __syncthreads();
    hist[(size_t)threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];
}

// exclusive scan of hist[0 .. total) in place, one workgroup (radius.hip radius_scan_kernel's shape)
__global__ __launch_bounds__(1024) void rf_scan_kernel(int* __restrict__ hist, int total) {
    __shared__ int part[1024];
    const int tid = threadIdx.x, per = (total + 1023) / 1024;
    const int lo = tid * per < total ? tid * per : total, hi = lo + per < total ? lo + per : total;
    int s = 0;
    for (int i = lo; i < hi; ++i) s += hist[i];
    part[tid] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - s;
    for (int i = lo; i < hi; ++i) { const int c = hist[i]; hist[i] = run; run += c; }
}

// the lanes of the wave that hold the same 8-bit digit (estim.hip same_bucket_lanes)
__device__ __forceinline__ u64 rf_same_digit(unsigned d, bool valid) {
    u64 same = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
        const bool on = (d >> bit) & 1u;
        const u64 bal = __ballot(on);
        same &= on ? bal : ~bal;
    }
    return valid ? same : 0ull;
}

__global__ __launch_bounds__(256) void rf_scatter_kernel(const unsigned* __restrict__ keys, const int* __restrict__ idx, int n, int shift, int nblk,
                                                         const int* __restrict__ offs, unsigned* __restrict__ keys_out, int* __restrict__ idx_out) {
    __shared__ int wcnt[4][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int k = threadIdx.x; k < 4 * 256; k += 256) (&wcnt[0][0])[k] = 0;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < n;
    const unsigned key = valid ? keys[i] : 0u;
    const unsigned d = (key >> shift) & 255u;
    const u64 same = rf_same_digit(d, valid);
    const u64 below = same & ((1ull << lane) - 1ull);
    if (valid && below == 0ull) wcnt[w][d] = __popcll(same);          // one writer per (wave, digit)
    __syncthreads();
    if (!valid) return;
    int pos = offs[(size_t)d * nblk + blockIdx.x] + __popcll(below);
    for (int k = 0; k < w; ++k) pos += wcnt[k][d];
    keys_out[pos] = key;                                              // pos < n: the offsets are the scan of the counts of these very keys
    idx_out[pos] = idx[i];
}

// start[s] = first sorted position whose bucket is >= s (s = 0 .. nslots; start[nslots] = n), pk[p] = the p-th sorted point
__global__ __launch_bounds__(256) void rf_cells_kernel(const unsigned* __restrict__ keys, const int* __restrict__ idx, const float* __restrict__ pts, int n,
                                                       unsigned nslots, int* __restrict__ start, float4* __restrict__ pk) {
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    if (g <= nslots) {
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (keys[mid] < g) lo = mid + 1; else hi = mid;
        }
        start[g] = lo;
    }
    if (g < (unsigned)n) {
        const int j = idx[g];
        const float* p = pts + 3 * (size_t)j;
        pk[g] = make_float4(p[0], p[1], p[2], __int_as_float(j));
    }
}

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
        float q[3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
            q[i] = (float)__dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(st->T[4 * i], s0), __dmul_rn(st->T[4 * i + 1], s1)), __dmul_rn(st->T[4 * i + 2], s2)),
                                    st->T[4 * i + 3]);
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
        if (in) { v[0] = 1.0; v[2] = a[0]; v[3] = a[1]; v[4] = a[2]; v[5] = b[0]; v[6] = b[1]; v[7] = b[2]; }
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
    if (threadIdx.x < 8) {
        double s = 0.0;
        for (int b = 0; b < nblk; ++b) s = __dadd_rn(s, slab[(size_t)b * RF_SLAB + threadIdx.x]);
        tot[threadIdx.x] = s;
    }
    __syncthreads();
    const int n = (int)tot[0];
    if (threadIdx.x < 3) {
        st->c0[threadIdx.x] = n > 0 ? tot[2 + threadIdx.x] / (double)n : 0.0;
        st->c1[threadIdx.x] = n > 0 ? tot[5 + threadIdx.x] / (double)n : 0.0;
    }
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
    if (j >= 0) {
        double a[3], b[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            a[i] = __dsub_rn((double)tgt[3 * (size_t)j + i], st->c0[i]);
            b[i] = __dsub_rn((double)src[3 * (size_t)e + i], st->c1[i]);
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) v[i] = __dmul_rn(b[i / 3], a[i % 3]);
    }
    rf_block_sum<9>(v, slab + (size_t)blockIdx.x * RF_SLAB);
}

__global__ __launch_bounds__(256) void rf_refit_cov_kernel(const RfState* __restrict__ st, const double* __restrict__ k0, const double* __restrict__ k1, int M,
                                                           const unsigned char* __restrict__ mask, double* __restrict__ slab) {
    if (st->stop) return;
    const int m = blockIdx.x * 256 + threadIdx.x;
    double v[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (m < M && mask[m]) {
        double a[3], b[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            a[i] = __dsub_rn(k0[3 * (size_t)m + i], st->c0[i]);
            b[i] = __dsub_rn(k1[3 * (size_t)m + i], st->c1[i]);
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) v[i] = __dmul_rn(b[i / 3], a[i % 3]);
    }
    rf_block_sum<9>(v, slab + (size_t)blockIdx.x * RF_SLAB);
}

// one wave: the slabs of a second pass in block order -> H -> T_{i+1}, and the stop rules that need it
// MODE 0 ICP: Tnext = st->T (replaced when accepted); 1 refit: Tnext = the next row of the iterates
template <int MODE>
__global__ __launch_bounds__(64) void rf_solve_kernel(RfState* __restrict__ st, const double* __restrict__ slab, int nblk, int it, int iters, double tol,
                                                      double* __restrict__ Tnext) {
    if (st->stop) return;
    __shared__ double H[9];
    if (threadIdx.x < 9) {
        double s = 0.0;
        for (int b = 0; b < nblk; ++b) s = __dadd_rn(s, slab[(size_t)b * RF_SLAB + threadIdx.x]);
        H[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double R[9], T[12];
    if (!rf_rotation(H, R)) {
        st->stop = 1;
        if (MODE == 0) st->reason = YOHO_ICP_RANK;
        return;
    }
    double delta = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        T[4 * i] = R[3 * i]; T[4 * i + 1] = R[3 * i + 1]; T[4 * i + 2] = R[3 * i + 2];
        T[4 * i + 3] = __dsub_rn(st->c0[i], __dadd_rn(__dadd_rn(__dmul_rn(R[3 * i], st->c1[0]), __dmul_rn(R[3 * i + 1], st->c1[1])), __dmul_rn(R[3 * i + 2], st->c1[2])));
    }
    if (MODE == 0) {
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

// ---- host side -------------------------------------------------------------------------------------------------------------------
void rf_grid_layout(Arena& ar, int Nt, RfGridWs& w) {
    w.bits = 8;
    while (w.bits < 23 && (1u << w.bits) < 2u * (unsigned)Nt) ++w.bits;
    w.nslots = 1u << w.bits;
    w.nblk = (Nt + 255) / 256;
    for (int k = 0; k < 2; ++k) { w.keys[k] = ar.take<unsigned>((size_t)Nt); w.idx[k] = ar.take<int>((size_t)Nt); }
    w.hist = ar.take<int>(256 * (size_t)w.nblk);
    w.start = ar.take<int>((size_t)w.nslots + 1);
    w.pk = ar.take<float4>((size_t)Nt);
}

int rf_build_grid(const float* tgt, int Nt, float max_dist, const RfGridWs& w, RfGrid& g, hipStream_t s) {
    double cell = (double)max_dist * (1.0 + 0x1p-10);
    if (cell < RF_MIN_CELL) cell = RF_MIN_CELL;
    g.inv_cell = 1.0 / cell;
    g.mask = w.nslots - 1;
    g.gate2 = max_dist * max_dist;                                    // f32, rounded once (-ffp-contract=off; host code anyway)
    g.start = w.start;
    g.pk = w.pk;
    const dim3 grid(w.nblk), block(256);
    hipLaunchKernelGGL(rf_key_kernel, grid, block, 0, s, tgt, Nt, g.inv_cell, g.mask, w.keys[0], w.idx[0]);
    HIPCHK(hipGetLastError());
    int cur = 0;
    for (int shift = 0; shift < w.bits; shift += 8) {
        hipLaunchKernelGGL(rf_hist_kernel, grid, block, 0, s, (const unsigned*)w.keys[cur], Nt, shift, w.nblk, w.hist);
        hipLaunchKernelGGL(rf_scan_kernel, dim3(1), dim3(1024), 0, s, w.hist, 256 * w.nblk);
        hipLaunchKernelGGL(rf_scatter_kernel, grid, block, 0, s, (const unsigned*)w.keys[cur], (const int*)w.idx[cur], Nt, shift, w.nblk, (const int*)w.hist,
                           w.keys[cur ^ 1], w.idx[cur ^ 1]);
        HIPCHK(hipGetLastError());
        cur ^= 1;
    }
    const unsigned work = w.nslots + 1 > (unsigned)Nt ? w.nslots + 1 : (unsigned)Nt;
    hipLaunchKernelGGL(rf_cells_kernel, dim3((work + 255) / 256), block, 0, s, (const unsigned*)w.keys[cur], (const int*)w.idx[cur], tgt, Nt, w.nslots, w.start,
                       w.pk);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace yoho

using namespace yoho;

extern "C" {

int yoho_nn_within(yoho_ctx* c, const float* q, int Nq, const float* tgt, int Nt, float max_dist, int64_t* idx, float* d2, void* stream) {
    if (!c || Nq < 0 || Nt < 1) { set_error("yoho_nn_within: bad argument (ctx %p, Nq=%d, Nt=%d)", (void*)c, Nq, Nt); return YOHO_EINVAL; }
    if (Nq > YOHO_REFINE_MAX_POINTS || Nt > YOHO_REFINE_MAX_POINTS) {
        set_error("yoho_nn_within: Nq=%d, Nt=%d must not exceed YOHO_REFINE_MAX_POINTS = %d", Nq, Nt, YOHO_REFINE_MAX_POINTS);
        return YOHO_EINVAL;
    }
    if (rf_bad_radius(max_dist)) { set_error("yoho_nn_within: max_dist=%g must be finite and > 0", (double)max_dist); return YOHO_EINVAL; }
    if (Nq == 0) return 0;
    if (!q || !tgt || !idx) { set_error("yoho_nn_within: bad argument (a required pointer is NULL)"); return YOHO_EINVAL; }
    YOHO_NEED_ALIGNED("yoho_nn_within", 3, q, tgt, d2);
    YOHO_NEED_ALIGNED("yoho_nn_within", 7, idx);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    int rc;
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
    if (!c || M < 0) { set_error("yoho_refit_matches: bad argument (ctx %p, M=%d)", (void*)c, M); return YOHO_EINVAL; }
    if (M > YOHO_REFINE_MAX_POINTS) { set_error("yoho_refit_matches: M=%d must not exceed YOHO_REFINE_MAX_POINTS = %d", M, YOHO_REFINE_MAX_POINTS); return YOHO_EINVAL; }
    if (iters < 0 || iters > YOHO_REFIT_MAX_ITERS) { set_error("yoho_refit_matches: iters=%d must be in [0, YOHO_REFIT_MAX_ITERS = %d]", iters, YOHO_REFIT_MAX_ITERS); return YOHO_EINVAL; }
    if (!(inlier_dist >= 0.0) || !std::isfinite(inlier_dist)) { set_error("yoho_refit_matches: inlier_dist=%g must be finite and >= 0", inlier_dist); return YOHO_EINVAL; }
    if (!T_in || !T_out || !counts || !info || (M > 0 && (!k0 || !k1))) { set_error("yoho_refit_matches: bad argument (a required pointer is NULL)"); return YOHO_EINVAL; }
    YOHO_NEED_ALIGNED("yoho_refit_matches", 7, k0, k1, T_in, T_out);
    YOHO_NEED_ALIGNED("yoho_refit_matches", 3, counts, info);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int nblk = (M + 255) / 256;
    int rc;
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
    if (!c || Ns < 1 || Nt < 1) { set_error("yoho_icp_refine: bad argument (ctx %p, Ns=%d, Nt=%d)", (void*)c, Ns, Nt); return YOHO_EINVAL; }
    if (Ns > YOHO_REFINE_MAX_POINTS || Nt > YOHO_REFINE_MAX_POINTS) {
        set_error("yoho_icp_refine: Ns=%d, Nt=%d must not exceed YOHO_REFINE_MAX_POINTS = %d", Ns, Nt, YOHO_REFINE_MAX_POINTS);
        return YOHO_EINVAL;
    }
    if (iters < 0 || iters > YOHO_ICP_MAX_ITERS) { set_error("yoho_icp_refine: iters=%d must be in [0, YOHO_ICP_MAX_ITERS = %d]", iters, YOHO_ICP_MAX_ITERS); return YOHO_EINVAL; }
    if (rf_bad_radius(max_dist)) { set_error("yoho_icp_refine: max_dist=%g must be finite and > 0", (double)max_dist); return YOHO_EINVAL; }
    if (std::isnan(tol)) { set_error("yoho_icp_refine: tol is NaN"); return YOHO_EINVAL; }
    if (!src || !tgt || !T_in || !T_out || !info || (iters > 0 && (!npairs || !rmse))) { set_error("yoho_icp_refine: bad argument (a required pointer is NULL)"); return YOHO_EINVAL; }
    YOHO_NEED_ALIGNED("yoho_icp_refine", 3, src, tgt, npairs, info);
    YOHO_NEED_ALIGNED("yoho_icp_refine", 7, T_in, T_out, rmse);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int nblk = (Ns + 255) / 256;
    int rc;
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
