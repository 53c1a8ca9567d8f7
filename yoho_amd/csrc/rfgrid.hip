// The cell-sorted grid over a target cloud: its build (rf_key / rf_hist / rf_scan / rf_scatter / rf_cells_kernel, rf_grid_layout,
// rf_build_grid).  What a query needs on the device (rf_cell, rf_slot, RfGrid, rf_walk) is inline in rfgrid.h.  Six files build the
// grid: refine.hip (yoho_nn_within, yoho_icp_refine), plane.hip (yoho_estimate_normals, yoho_icp_plane), verify.hip
// (yoho_eval_transforms, yoho_verify_hypotheses), multiway.hip (yoho_edge_information), clean.hip (yoho_knn_within,
// yoho_statistical_outliers) and cluster.hip (yoho_dbscan); refine, verify, multiway and plane.hip's ICP query it with rf_walk,
// plane.hip's normals, clean.hip and cluster.hip walk start / pk with loops of their own.  fuse.hip and consist.hip include rfgrid.h for the shared
// refusals only.  Compiled with -ffp-contract=off like every file that includes rfgrid.h (yoho_amd/build.py).  The digit passes at
// both sides of their size thresholds: tests/test_gpu_sizes.py.
//
// THE GRID.  gridnn.hip's grid (linked lists behind an open-addressing table, a wave and 125 probes per query, brute force for what it
// cannot settle) is built for queries that all have a partner nearby; in ICP half the cloud has none.  Here the targets are SORTED by
// cell: a point's cell (cx, cy, cz) = rf_cell of its coordinates - gridnn.hip's monotone clamped gn_cell - with cell side
// max_dist (1 + 2^-10), its bucket = a hash of the cell into a table of nslots >= 2 Nt slots.  The sort is a stable least-significant-
// digit counting sort of (bucket, original index) on 8-bit digits, two or three passes: rf_hist_kernel counts the digits of every
// 256-point block, rf_scan_kernel turns the [digit][block] counts into offsets (one workgroup, an exclusive scan), rf_scatter_kernel
// places every point at offset + (points of the same digit in front of it in its block), that rank from eight ballots and a
// popcount below the lane (common.h wave_same_value, radius.hip's ranks) plus the counts of the waves in front.  No atomic
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
// Untuned at large sizes: rf_scan_kernel is one workgroup scanning 256 nblk counts, two or three times per grid build.  No scratch in
// any kernel of this file.  Timings: tools/time_refine.py -> profiles/refine.md.
#include "rfgrid.h"

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
    const u64 same = wave_same_value<8>(d, valid);
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
