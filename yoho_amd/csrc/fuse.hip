// K fragments under K poses into the voxel means of a scene (include/yoho_fuse.h).  Compiled with -ffp-contract=off like
// multiway.hip (yoho_amd/build.py); the rounded transform is rffit.h's rf_apply, the refusals are rfgrid.h's.
//
//   fu_key_kernel        one lane per (fragment, local point): transform, cells, the contract's key (or OUTSIDE), the row, the fragment
//                        number; per workgroup the extent of its cells
//   fu_plan_kernel       one workgroup: the extent of the scene -> FuPlan: the bit width of every axis, which digit passes run and on
//                        which of the two buffers
//   fu_pack_kernel       the contract's key rewritten as the PACKED key (below)
//   fu_hist_kernel, fu_scatter_kernel     one stable counting-sort pass on an 8-bit digit, rfgrid.hip's: ranks from ballots
//   fu_tile_sum_kernel, fu_tile_scan_kernel     THE SCAN
//   fu_count_kernel      one lane per sorted position, the lane of a run's head walks the run until it knows: kept or not
//   fu_heads_kernel      the kept flags scanned into rows -> the head position of every kept row; M; row_of = -1 everywhere
//   fu_emit_kernel       one lane per kept row walks its run: the sums, the outputs of the row, row_of of every point of the run
//
// THE TABLE.  soff is a host array; the entry validates it and hands fu_key_kernel 64 fragments per launch BY VALUE (FuFrags, as
// multiway.hip's MwEdges): workgroups aligned to fragments, the fragment found by bisection with blockIdx.x, wave-uniform.  Later
// kernels know a point's fragment from frag[row] (16 bits, workspace).
//
// THE SORT.  The contract orders voxels by key = (cz + 2^20) << 42 | (cy + 2^20) << 21 | (cx + 2^20): 63 bits, of which a room uses
// about thirty - but not the LOW thirty, and cells on both sides of 0 differ in every bit of an axis.  So the sort runs on the packed
// key ((cz - lo_z) << (bx + by)) | ((cy - lo_y) << bx) | (cx - lo_x), lo the smallest cell of the axis and b the bits of its span:
// the same order, the same equalities, ceil(bits / 8) digit passes instead of eight.  OUTSIDE is 1 << (bx + by + bz), above every
// voxel, and costs a bit only when some point is outside.  The extent comes from the device (per-workgroup minima, reduced by one
// workgroup: integer minima, no atomics); the host queues all eight passes and the kernels of a pass the plan does not need return at
// once, each kernel reading from the plan which buffer holds its input.  A pass is rfgrid.hip's: digit counts per 256-point block
// (LDS atomics that only count), an exclusive scan of the [digit][block] table, every point placed at offset + its rank among the
// equal digits of its block, the rank from eight ballots.  No atomic decides a position and every pass is stable, so a voxel's points
// end up contiguous in ascending global row - the order the contract sums in.
//
// THE SCAN.  256 ceil(S / 256) counts per pass, 18 M at 60 fragments of 300 000 points: rf_scan_kernel's one workgroup is the wrong
// tool.  Here a scan is tiles of 2048: fu_tile_sum_kernel adds every tile, the tile sums are scanned the same way (two levels reach
// 2^33 elements), fu_tile_scan_kernel scans every tile from its carry.  Integer sums: exact in any order.  The kernel boundary is the
// synchronisation; no workgroup waits for another.
//
// THE WALK.  A position whose key differs from the one before it heads a run.  fu_count_kernel: the head's lane walks its run until both
// thresholds are met (fragment numbers never decrease along a run, so nfrag is the number of changes plus one) and writes the kept
// flag, 0 for every other position.  The flags are scanned into kept rows; fu_heads_kernel turns them into the list of head positions
// - so that the walk that sums has one lane per KEPT ROW, 64 runs per wave in flight, not one lane in a run's length - and writes M
// and row_of = -1 for every point.  fu_emit_kernel walks again: count, the fragment changes, the f64 sums one point after another from
// +0.0 with the pose reloaded only when the fragment changes, row_of of every point of the run, and the row's outputs when the row is
// below capacity.  Serial in the run length: the price of the stated order; a voxel of a fused room holds tens of points.  The head
// list lives where the digit counts did.  No float atomics, no host read; every workspace byte is written before it is read.
//
// No scratch in any kernel of this file.  Registers and timings: tools/time_fuse.py -> profiles/fuse.md.
#include "rfgrid.h"
#include "rffit.h"
#include "yoho_fuse.h"
#include <climits>
#include <cmath>

namespace yoho {

constexpr int FU_CHUNK = 64;                         // fragments per fu_key_kernel launch
constexpr int FU_TILE = 2048;                        // elements per workgroup of THE SCAN
constexpr int FU_PASSES = 8;
constexpr int FU_CELL_MAX = (1 << 20) - 1;
constexpr u64 FU_OUTSIDE = ~0ull;                    // in the contract's key; the packed key has FuPlan::outkey
constexpr int FU_EXT = 8;                            // ints per extent row: min cx, cy, cz, min -cx, -cy, -cz, min -(outside), unused

struct FuFrags {
    int soff[FU_CHUNK + 1];                          // first global row of fragment k of the chunk
    int bpre[FU_CHUNK + 1];                          // first workgroup of fragment k in the chunk's launch
};
struct FuPlan {
    int lo[3], bits[3];
    int nbits;                                       // bits a pass has to look at
    int final_buf;                                   // the buffer that holds the sorted points
    u64 outkey;
    int active[FU_PASSES], srcbuf[FU_PASSES];
};
struct FuSort {
    u64* keys[2];
    int* rows[2];
};

__device__ __forceinline__ int fu_wave_min(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(256) void fu_key_kernel(FuFrags fr, int K, int k0, int blk0, const float* __restrict__ src, const double* __restrict__ Trows,
                                                     double inv, u64* __restrict__ keys, int* __restrict__ rows, unsigned short* __restrict__ frag,
                                                     int* __restrict__ ext) {
    __shared__ int red[4][FU_EXT];
    const int blk = blockIdx.x;
    int lo = 0, hi = K;                                               // bpre[lo] <= blk < bpre[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (fr.bpre[mid] <= blk) lo = mid; else hi = mid;
    }
    const int k = lo;                                                 // wave-uniform: from blockIdx and kernel arguments alone
    const int s0 = fr.soff[k], n = fr.soff[k + 1] - s0;
    const double* __restrict__ T = Trows + 12 * (size_t)(k0 + k);
    const int e = (blk - fr.bpre[k]) * 256 + threadIdx.x;
    int r[7] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX, 0};
    if (e < n) {
        const int row = s0 + e;                                       // < soff[K] <= YOHO_FUSE_MAX_POINTS
        double x[3];
        rf_apply(T, src, row, x);
        const double cx = floor(__dmul_rn(x[0], inv)), cy = floor(__dmul_rn(x[1], inv)), cz = floor(__dmul_rn(x[2], inv));
        const double m = (double)FU_CELL_MAX;
        const bool inside = cx >= -m && cx <= m && cy >= -m && cy <= m && cz >= -m && cz <= m;      // false for a NaN
        u64 key = FU_OUTSIDE;
        if (inside) {
            const int ix = (int)cx, iy = (int)cy, iz = (int)cz;
            key = ((u64)(unsigned)(iz + (1 << 20)) << 42) | ((u64)(unsigned)(iy + (1 << 20)) << 21) | (u64)(unsigned)(ix + (1 << 20));
            r[0] = ix; r[1] = iy; r[2] = iz; r[3] = -ix; r[4] = -iy; r[5] = -iz;
        } else {
            r[6] = -1;
        }
        keys[row] = key;
        rows[row] = row;
        frag[row] = (unsigned short)(k0 + k);
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) r[j] = fu_wave_min(r[j]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < 7; ++j) red[threadIdx.x >> 6][j] = r[j];
    }
    __syncthreads();
    if (threadIdx.x < FU_EXT) {
        const int j = threadIdx.x;
        ext[(size_t)(blk0 + blk) * FU_EXT + j] = j < 7 ? min(min(red[0][j], red[1][j]), min(red[2][j], red[3][j])) : 0;
    }
}

__global__ __launch_bounds__(1024) void fu_plan_kernel(const int* __restrict__ ext, int nblk, FuPlan* __restrict__ plan) {
    __shared__ int red[16][FU_EXT];
    int r[7] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX, 0};
    for (int b = threadIdx.x; b < nblk; b += 1024) {
#pragma unroll
        for (int j = 0; j < 7; ++j) r[j] = min(r[j], ext[(size_t)b * FU_EXT + j]);
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) r[j] = fu_wave_min(r[j]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < 7; ++j) red[threadIdx.x >> 6][j] = r[j];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        int v = red[0][j];
        for (int w = 1; w < 16; ++w) v = min(v, red[w][j]);
        r[j] = v;
    }
    const bool any = r[0] != INT_MAX;                                 // some point is inside
    int total = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int span = any ? -r[3 + a] - r[a] : 0;                  // max - min <= 2^21 - 2
        const int b = span > 0 ? 32 - __clz(span) : 0;
        plan->lo[a] = any ? r[a] : 0;
        plan->bits[a] = b;
        total += b;
    }
    plan->outkey = 1ull << total;                                     // total <= 63
    const int nbits = total + (r[6] != 0 ? 1 : 0);
    plan->nbits = nbits;
    int cur = 0;
#pragma unroll
    for (int p = 0; p < FU_PASSES; ++p) {
        const int on = 8 * p < nbits ? 1 : 0;
        plan->active[p] = on;
        plan->srcbuf[p] = cur;
        cur ^= on;
    }
    plan->final_buf = cur;
}

__global__ __launch_bounds__(256) void fu_pack_kernel(u64* __restrict__ keys, int n, const FuPlan* __restrict__ plan) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 key = keys[i];
    u64 out = plan->outkey;
    if (key != FU_OUTSIDE) {
        const int bx = plan->bits[0], by = plan->bits[1];
        const u64 dx = (u64)(unsigned)((int)(key & 0x1FFFFFu) - (1 << 20) - plan->lo[0]);
        const u64 dy = (u64)(unsigned)((int)((key >> 21) & 0x1FFFFFu) - (1 << 20) - plan->lo[1]);
        const u64 dz = (u64)(unsigned)((int)((key >> 42) & 0x1FFFFFu) - (1 << 20) - plan->lo[2]);
        out = (dz << (bx + by)) | (dy << bx) | dx;
    }
    keys[i] = out;
}

// ---- one digit pass ------------------------------------------------------------------------------------------------------------
// hist[digit * nblk + block] = points of the block with that digit
__global__ __launch_bounds__(256) void fu_hist_kernel(FuSort so, const FuPlan* __restrict__ plan, int pass, int n, int nblk, int* __restrict__ hist) {
    if (!plan->active[pass]) return;
    __shared__ int h[256];
    const u64* __restrict__ keys = plan->srcbuf[pass] ? so.keys[1] : so.keys[0];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) atomicAdd(&h[(unsigned)(keys[i] >> (8 * pass)) & 255u], 1);      // counts only: the sum does not depend on the order of arrival
    __syncthreads();
    hist[(size_t)threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(256) void fu_scatter_kernel(FuSort so, const FuPlan* __restrict__ plan, int pass, int n, int nblk, const int* __restrict__ offs) {
    if (!plan->active[pass]) return;
    __shared__ int wcnt[4][256];
    const int sb = plan->srcbuf[pass];
    const u64* __restrict__ keys = sb ? so.keys[1] : so.keys[0];
    const int* __restrict__ rows = sb ? so.rows[1] : so.rows[0];
    u64* __restrict__ keys_out = sb ? so.keys[0] : so.keys[1];
    int* __restrict__ rows_out = sb ? so.rows[0] : so.rows[1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int k = threadIdx.x; k < 4 * 256; k += 256) (&wcnt[0][0])[k] = 0;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < n;
    const u64 key = valid ? keys[i] : 0ull;
    const unsigned d = (unsigned)(key >> (8 * pass)) & 255u;
    const u64 same = wave_same_value<8>(d, valid);
    const u64 below = same & ((1ull << lane) - 1ull);
    if (valid && below == 0ull) wcnt[w][d] = __popcll(same);          // one writer per (wave, digit)
    __syncthreads();
    if (!valid) return;
    int pos = offs[(size_t)d * nblk + blockIdx.x] + __popcll(below);
    for (int k = 0; k < w; ++k) pos += wcnt[k][d];
    keys_out[pos] = key;                                              // pos < n: the offsets are the scan of the counts of these very keys
    rows_out[pos] = rows[i];
}

// ---- the scan ------------------------------------------------------------------------------------------------------------------
// gate: NULL, or a device word that is 0 when the scan is not needed (the pass of a plan that skips it)
__global__ __launch_bounds__(256) void fu_tile_sum_kernel(const int* __restrict__ in, int n, int* __restrict__ sums, const int* __restrict__ gate) {
    if (gate && !*gate) return;
    __shared__ int red[4];
    const size_t base = (size_t)blockIdx.x * FU_TILE;
    int s = 0;
#pragma unroll
    for (int j = 0; j < FU_TILE / 256; ++j) {
        const size_t i = base + (size_t)j * 256 + threadIdx.x;
        if (i < (size_t)n) s += in[i];
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// out[i] = carry[tile] + the sum of the tile's elements in front of i; in == out is allowed (a thread reads its eight before it writes)
__global__ __launch_bounds__(256) void fu_tile_scan_kernel(const int* in, int n, const int* __restrict__ carry, int* out, const int* __restrict__ gate) {
    if (gate && !*gate) return;
    __shared__ int wtot[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const size_t base = (size_t)blockIdx.x * FU_TILE + (size_t)threadIdx.x * 8;
    int v[8];
    if (base + 8 <= (size_t)n) {
        const int4 a = *reinterpret_cast<const int4*>(in + base), b = *reinterpret_cast<const int4*>(in + base + 4);      // base % 8 == 0, arrays 256-byte aligned
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = base + j < (size_t)n ? in[base + j] : 0;
    }
    const int s = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    int x = s;                                                        // inclusive over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) wtot[w] = x;
    __syncthreads();
    int pre = (carry ? carry[blockIdx.x] : 0) + (x - s);
    for (int k = 0; k < w; ++k) pre += wtot[k];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (base + j < (size_t)n) out[base + j] = pre;
        pre += v[j];
    }
}

// ---- the walk ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fu_count_kernel(FuSort so, const FuPlan* __restrict__ plan, const unsigned short* __restrict__ frag, int n, int min_count,
                                                       int min_frags, int* __restrict__ flag) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int fb = plan->final_buf;
    const u64* __restrict__ keys = fb ? so.keys[1] : so.keys[0];
    const int* __restrict__ rows = fb ? so.rows[1] : so.rows[0];
    const u64 key = keys[p];
    int kept = 0;
    if (key != plan->outkey && (p == 0 || keys[p - 1] != key)) {
        int cnt = 0, nf = 0, last = -1;
        for (int j = p; j < n && keys[j] == key; ++j) {
            const int f = (int)frag[rows[j]];
            nf += f != last ? 1 : 0;
            last = f;
            ++cnt;
            if (cnt >= min_count && nf >= min_frags) { kept = 1; break; }
        }
    }
    flag[p] = kept;
}

// heads[r] = the sorted position that heads kept row r; row_of = -1 everywhere (fu_emit_kernel overwrites the points of kept voxels); M
__global__ __launch_bounds__(256) void fu_heads_kernel(FuSort so, const FuPlan* __restrict__ plan, int n, const int* __restrict__ flag, const int* __restrict__ krow,
                                                       int* __restrict__ heads, int32_t* __restrict__ row_of, long long* __restrict__ n_out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int kept = flag[p], r = krow[p];
    if (p == n - 1) *n_out = (long long)r + (long long)kept;
    if (kept) heads[r] = p;                                           // r <= p < n
    if (row_of) {
        const int* __restrict__ rows = plan->final_buf ? so.rows[1] : so.rows[0];
        row_of[rows[p]] = -1;
    }
}

// one lane per kept row: every lane of a wave walks a run, so a wave has 64 chains of loads in flight instead of one or two
template <bool NRM>
__global__ __launch_bounds__(256) void fu_emit_kernel(FuSort so, const FuPlan* __restrict__ plan, const unsigned short* __restrict__ frag, int n,
                                                      const float* __restrict__ src, const float* __restrict__ nrm, const double* __restrict__ Trows,
                                                      const int* __restrict__ flag, const int* __restrict__ krow, const int* __restrict__ heads,
                                                      float* __restrict__ pts, float* __restrict__ out_nrm, int32_t* __restrict__ count,
                                                      int32_t* __restrict__ nfrag, int32_t* __restrict__ row_of, long long capacity) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= krow[n - 1] + flag[n - 1]) return;                        // M: the grid is sized for the largest M there can be
    const bool emit = (long long)r < capacity;
    if (!emit && !row_of) return;
    const int fb = plan->final_buf;
    const u64* __restrict__ keys = fb ? so.keys[1] : so.keys[0];
    const int* __restrict__ rows = fb ? so.rows[1] : so.rows[0];
    const int p = heads[r];
    const u64 key = keys[p];
    int cnt = 0, nf = 0, last = -1;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, m0 = 0.0, m1 = 0.0, m2 = 0.0;
    double T[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = p; j < n && keys[j] == key; ++j) {
        const int row = rows[j];
        if (row_of) row_of[row] = r;
        if (!emit) continue;
        const int f = (int)frag[row];
        if (f != last) {
#pragma unroll
            for (int i = 0; i < 12; ++i) T[i] = Trows[12 * (size_t)f + i];
            ++nf;
            last = f;
        }
        ++cnt;
        double x[3];
        rf_apply(T, src, row, x);
        s0 = __dadd_rn(s0, x[0]); s1 = __dadd_rn(s1, x[1]); s2 = __dadd_rn(s2, x[2]);
        if (NRM) {
            const double a = (double)nrm[3 * (size_t)row], b = (double)nrm[3 * (size_t)row + 1], c = (double)nrm[3 * (size_t)row + 2];
            m0 = __dadd_rn(m0, __dadd_rn(__dadd_rn(__dmul_rn(T[0], a), __dmul_rn(T[1], b)), __dmul_rn(T[2], c)));
            m1 = __dadd_rn(m1, __dadd_rn(__dadd_rn(__dmul_rn(T[4], a), __dmul_rn(T[5], b)), __dmul_rn(T[6], c)));
            m2 = __dadd_rn(m2, __dadd_rn(__dadd_rn(__dmul_rn(T[8], a), __dmul_rn(T[9], b)), __dmul_rn(T[10], c)));
        }
    }
    if (!emit) return;
    const double c = (double)cnt;
    pts[3 * (size_t)r] = (float)(s0 / c);
    pts[3 * (size_t)r + 1] = (float)(s1 / c);
    pts[3 * (size_t)r + 2] = (float)(s2 / c);
    count[r] = cnt;
    nfrag[r] = nf;
    if (NRM) {
        const double len = sqrt(__dadd_rn(__dadd_rn(__dmul_rn(m0, m0), __dmul_rn(m1, m1)), __dmul_rn(m2, m2)));
        const bool ok = len > 0.0 && len < __builtin_inf();           // false for a NaN
        out_nrm[3 * (size_t)r] = ok ? (float)(m0 / len) : 0.f;
        out_nrm[3 * (size_t)r + 1] = ok ? (float)(m1 / len) : 0.f;
        out_nrm[3 * (size_t)r + 2] = ok ? (float)(m2 / len) : 0.f;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
struct FuScanWs {
    int levels;
    int n[2];
    int* sums[2];
};

static void fu_scan_layout(Arena& ar, size_t n, FuScanWs& w) {
    w.levels = 0;
    while (n > (size_t)FU_TILE && w.levels < 2) {
        n = (n + FU_TILE - 1) / FU_TILE;
        w.n[w.levels] = (int)n;
        w.sums[w.levels] = ar.take<int>(n);
        ++w.levels;
    }
}

// exclusive scan of in[0 .. n) into out (in == out allowed), n <= 2^33 / 2048 per level: two levels of tile sums at most
static void fu_scan(const int* in, int* out, int n, const FuScanWs& w, const int* gate, hipStream_t s) {
    const int* src = in;
    int cnt = n;
    for (int l = 0; l < w.levels; ++l) {
        hipLaunchKernelGGL(fu_tile_sum_kernel, dim3(w.n[l]), dim3(256), 0, s, src, cnt, w.sums[l], gate);
        src = w.sums[l];
        cnt = w.n[l];
    }
    for (int l = w.levels; l >= 0; --l) {
        const int* a = l == 0 ? in : w.sums[l - 1];
        int* o = l == 0 ? out : w.sums[l - 1];
        const int m = l == 0 ? n : w.n[l - 1];
        const int* carry = l == w.levels ? nullptr : w.sums[l];
        hipLaunchKernelGGL(fu_tile_scan_kernel, dim3((m + FU_TILE - 1) / FU_TILE), dim3(256), 0, s, a, m, carry, o, gate);
    }
}

}  // namespace yoho

using namespace yoho;

extern "C" {

int yoho_fuse_clouds(yoho_ctx* c, const float* src, const int32_t* soff, int K, const double* T, const float* nrm, double voxel, int min_count,
                     int min_frags, float* pts, float* out_nrm, int32_t* count, int32_t* nfrag, int32_t* row_of, int64_t capacity, int64_t* n_out,
                     void* stream) {
    const char* fn = "yoho_fuse_clouds";
    int rc;
    if ((rc = rf_check_sizes(fn, c, "K", K, 1)) || (rc = rf_check_range(fn, "K", K, 1, RF_NAMED(YOHO_FUSE_MAX_K)))) return rc;
    if (!(voxel > 0.0) || !std::isfinite(voxel)) return RF_REFUSE("%s: voxel=%g must be finite and > 0", fn, voxel);
    if (min_count < 1 || min_frags < 1) return RF_REFUSE("%s: min_count=%d, min_frags=%d must be >= 1", fn, min_count, min_frags);
    if (capacity < 0) return RF_REFUSE("%s: capacity=%lld must be >= 0", fn, (long long)capacity);
    if ((rc = rf_check_pointers(fn, src && soff && T && n_out && (capacity == 0 || (pts && count && nfrag))))) return rc;
    if (out_nrm && !nrm) return RF_REFUSE("%s: out_nrm needs nrm (the normals of the input points)", fn);
    if (soff[0] != 0) return RF_REFUSE("%s: soff[0]=%d must be 0", fn, (int)soff[0]);
    int nkey = 0;                                                     // workgroups of fu_key_kernel over all chunks
    for (int k = 0; k < K; ++k) {
        const long long n = (long long)soff[k + 1] - (long long)soff[k];
        if (n < 1) return RF_REFUSE("%s: soff[%d]=%d, soff[%d]=%d: soff must be strictly increasing (no empty fragment)", fn, k, (int)soff[k], k + 1, (int)soff[k + 1]);
        if (n > YOHO_REFINE_MAX_POINTS)
            return RF_REFUSE("%s: fragment %d has %lld points, more than YOHO_REFINE_MAX_POINTS = %d", fn, k, n, (int)YOHO_REFINE_MAX_POINTS);
        if (soff[k + 1] > YOHO_FUSE_MAX_POINTS)
            return RF_REFUSE("%s: soff[%d]=%d must not exceed YOHO_FUSE_MAX_POINTS = %d", fn, k + 1, (int)soff[k + 1], (int)YOHO_FUSE_MAX_POINTS);
        nkey += (int)((n + 255) / 256);
    }
    YOHO_NEED_ALIGNED("yoho_fuse_clouds", 3, src, nrm, pts, out_nrm, count, nfrag, row_of);
    YOHO_NEED_ALIGNED("yoho_fuse_clouds", 7, T, n_out);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int S = soff[K], nblk = (S + 255) / 256;
    FuSort so;
    unsigned short* frag = nullptr;
    int *ext = nullptr, *hist = nullptr, *flag = nullptr, *krow = nullptr;
    FuPlan* plan = nullptr;
    FuScanWs hs, fs;
    if ((rc = bind_ws(c, s, [&](Arena& ar) {
            for (int b = 0; b < 2; ++b) { so.keys[b] = ar.take<u64>((size_t)S); so.rows[b] = ar.take<int>((size_t)S); }
            frag = ar.take<unsigned short>((size_t)S);
            ext = ar.take<int>((size_t)FU_EXT * nkey);
            plan = ar.take<FuPlan>(1);
            hist = ar.take<int>(256 * (size_t)nblk);
            fu_scan_layout(ar, 256 * (size_t)nblk, hs);
            flag = ar.take<int>((size_t)S);
            krow = ar.take<int>((size_t)S);
            fu_scan_layout(ar, (size_t)S, fs);
        }))) return rc;
    const double inv = 1.0 / voxel;
    const dim3 block(256), grid(nblk);
    for (int k0 = 0, blk0 = 0; k0 < K; k0 += FU_CHUNK) {
        const int kc = K - k0 < FU_CHUNK ? K - k0 : FU_CHUNK;
        FuFrags fr;
        fr.soff[0] = soff[k0];
        fr.bpre[0] = 0;
        for (int k = 0; k < kc; ++k) {
            fr.soff[k + 1] = soff[k0 + k + 1];
            fr.bpre[k + 1] = fr.bpre[k] + (soff[k0 + k + 1] - soff[k0 + k] + 255) / 256;
        }
        for (int k = kc + 1; k <= FU_CHUNK; ++k) { fr.soff[k] = fr.soff[kc]; fr.bpre[k] = fr.bpre[kc]; }
        hipLaunchKernelGGL(fu_key_kernel, dim3(fr.bpre[kc]), block, 0, s, fr, kc, k0, blk0, src, T, inv, so.keys[0], so.rows[0], frag, ext);
        blk0 += fr.bpre[kc];
    }
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(fu_plan_kernel, dim3(1), dim3(1024), 0, s, (const int*)ext, nkey, plan);
    hipLaunchKernelGGL(fu_pack_kernel, grid, block, 0, s, so.keys[0], S, (const FuPlan*)plan);
    HIPCHK(hipGetLastError());
    for (int pass = 0; pass < FU_PASSES; ++pass) {
        hipLaunchKernelGGL(fu_hist_kernel, grid, block, 0, s, so, (const FuPlan*)plan, pass, S, nblk, hist);
        fu_scan(hist, hist, 256 * nblk, hs, &plan->active[pass], s);
        hipLaunchKernelGGL(fu_scatter_kernel, grid, block, 0, s, so, (const FuPlan*)plan, pass, S, nblk, (const int*)hist);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(fu_count_kernel, grid, block, 0, s, so, (const FuPlan*)plan, (const unsigned short*)frag, S, min_count, min_frags, flag);
    fu_scan(flag, krow, S, fs, nullptr, s);
    int* heads = hist;                                                // the digit counts are dead behind the last pass; 256 nblk >= S ints
    hipLaunchKernelGGL(fu_heads_kernel, grid, block, 0, s, so, (const FuPlan*)plan, S, (const int*)flag, (const int*)krow, heads, row_of, (long long*)n_out);
    if (capacity > 0 || row_of) {
        if (out_nrm)
            hipLaunchKernelGGL(fu_emit_kernel<true>, grid, block, 0, s, so, (const FuPlan*)plan, (const unsigned short*)frag, S, src, nrm, T, (const int*)flag,
                               (const int*)krow, (const int*)heads, pts, out_nrm, count, nfrag, row_of, (long long)capacity);
        else
            hipLaunchKernelGGL(fu_emit_kernel<false>, grid, block, 0, s, so, (const FuPlan*)plan, (const unsigned short*)frag, S, src, nrm, T, (const int*)flag,
                               (const int*)krow, (const int*)heads, pts, out_nrm, count, nfrag, row_of, (long long)capacity);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
