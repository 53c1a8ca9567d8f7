// FCGF backbone, integer side: everything that turns points or voxel rows into integer tables.  No floating-point work except the
// f64 voxel index of a point.  The sparse-tensor semantics are MinkowskiEngine 0.5.x's as listed in oracle/fcgf_oracle.py.
//
//   hash tables        open addressing, 64-bit packed voxel key -> row; a coarser level is built by inserting the quantised coordinates
//                      with atomicMin of the source row and compacting the first occurrences (count / scan / scatter), so its rows
//                      come out in the CPU coordinate manager's order.  The fall-back coordinate path of a pass (YOHO_FCGF_COORDS=hash,
//                      clouds too large for a bitmap, duplicate voxels) and the single-cloud voxelisation;
//   rank-ordered       the default coordinate path: a level IS its occupancy bitmap plus a prefix popcount (rk_*, layout in
//   bitmaps            rklayout.h), the next level its 2 x 2 x 2 OR-reduction;
//   voxelisation       fcgf_voxelize (one cloud, tables), fcgf_voxelize_batch (the rotated copies of one cloud: bitmaps, else tables),
//                      fcgf_rotate_select;
//   boxes, bitmaps     per-cloud bounding boxes of a pass and the level-0 occupancy bitmaps of the first convolution (hash path);
//   kernel maps        map[k][n] = input row at coord(n) + offset(k), -1 if the voxel is empty (output-stationary: a convolution needs
//                      no atomics and sums in kernel-index order): build_map (any lookup), build_map_sym (3^3 onto itself, half the
//                      probes), invert_map (transposed = strided with the roles exchanged);
//   row orders         parity classes for the transposed convolutions, 8^3-voxel cells for level 0 of the hash path.
// The launch_* entries at the end of each group are what the driver (sparse.hip) calls; declarations in sparse.h.
#include <algorithm>
#include <cmath>

#include "sparse.h"

namespace yoho {

__global__ void hash_clear_kernel(u64* keys, int* vals, unsigned cap) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i < cap) { keys[i] = HEMPTY; vals[i] = 0x7FFFFFFF; }
}

// floor(p / voxel) as an int with defined behaviour for huge or non-finite values (they land outside VOX_LIM)
__device__ __forceinline__ int voxel_index(double p, double voxel) {
    const double q = floor(p / voxel);
    return (q >= -1073741824.0 && q <= 1073741824.0) ? (int)q : 1073741824;
}
// one coordinate of R p in f64, fixed operation order
__device__ __forceinline__ double rot_coord(const double* R3, double p0, double p1, double p2) { return fma(p2, R3[2], fma(p1, R3[1], p0 * R3[0])); }
__device__ __forceinline__ void point_of(const CoordSrc& s, int i, double& p0, double& p1, double& p2) {
    const double q0 = s.pts[3 * (size_t)i], q1 = s.pts[3 * (size_t)i + 1], q2 = s.pts[3 * (size_t)i + 2];
    if (s.rot) { p0 = rot_coord(s.R, q0, q1, q2); p1 = rot_coord(s.R + 3, q0, q1, q2); p2 = rot_coord(s.R + 6, q0, q1, q2); }
    else { p0 = q0; p1 = q1; p2 = q2; }
}
__device__ __forceinline__ void voxel_of(const CoordSrc& s, int i, int& x, int& y, int& z, int& b) {
    if (s.pts) {
        double p0, p1, p2;
        point_of(s, i, p0, p1, p2);
        x = voxel_index(p0, s.voxel);
        y = voxel_index(p1, s.voxel);
        z = voxel_index(p2, s.voxel);
        b = 0;
        if (s.oor && (x < -VOX_LIM || x > VOX_LIM || y < -VOX_LIM || y > VOX_LIM || z < -VOX_LIM || z > VOX_LIM)) atomicOr(s.oor, 1);
    } else {
        const int4 c = reinterpret_cast<const int4*>(s.coords)[i];
        x = floor_to(c.x, s.ts); y = floor_to(c.y, s.ts); z = floor_to(c.z, s.ts); b = c.w;
    }
}

// slot value = smallest source row with that voxel
__global__ void hash_insert_min_kernel(CoordSrc src, int n, u64* keys, int* vals, unsigned mask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int x, y, z, b;
    voxel_of(src, i, x, y, z, b);
    const u64 key = pack_key(x, y, z, b);
    unsigned s = hslot(key, mask);
    for (;;) {
        const u64 old = atomicCAS(&keys[s], HEMPTY, key);
        if (old == HEMPTY || old == key) {
            atomicMin(&vals[s], i);
            if (old == key && src.dup) atomicOr(src.dup, 1);
            return;
        }
        s = (s + 1) & mask;
    }
}

// first occurrences in source order -> new rows (order = the CPU coordinate manager's).  Three phases: per-block counts,
// single-workgroup scan of the block counts, per-block ballot scan + scatter.
__device__ __forceinline__ bool is_first(const CoordSrc& src, int i, int n, const u64* keys, const int* vals, unsigned mask, int& x, int& y,
                                         int& z, int& b) {
    if (i >= n) return false;
    voxel_of(src, i, x, y, z, b);
    const int slot = hash_find_slot(keys, mask, pack_key(x, y, z, b));
    return vals[slot] == i;
}

__global__ __launch_bounds__(1024) void first_count_kernel(CoordSrc src, int n, const u64* keys, const int* vals, unsigned mask, int* bsum) {
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int x, y, z, b;
    const bool keep = is_first(src, blockIdx.x * 1024 + tid, n, keys, vals, mask, x, y, z, b);
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wsum[wv] = __popcll(m);
    __syncthreads();
    if (tid == 0) { int t = 0; for (int k = 0; k < 16; ++k) t += wsum[k]; bsum[blockIdx.x] = t; }
}

// exclusive scan of nb block counts in place, total -> *count
__global__ __launch_bounds__(1024) void block_scan_kernel(int* bsum, int nb, int* count) {
    __shared__ int sh[1024];
    __shared__ int carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < nb; b0 += 1024) {
        const int i = b0 + tid;
        const int v = i < nb ? bsum[i] : 0;
        sh[tid] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int t = tid >= o ? sh[tid - o] : 0;
            __syncthreads();
            sh[tid] += t;
            __syncthreads();
        }
        if (i < nb) bsum[i] = carry + sh[tid] - v;
        __syncthreads();
        if (tid == 0) carry += sh[1023];
        __syncthreads();
    }
    if (tid == 0) *count = carry;
}

// out_coords rows: ocs = 3 (x, y, z: the caller's voxelisation output) or 4 (x, y, z, cloud: internal coordinate maps)
__global__ __launch_bounds__(1024) void first_scatter_kernel(CoordSrc src, int n, const u64* keys, const int* vals, unsigned mask,
                                                             const int* bsum, int* out_coords, int ocs, int64_t* sel) {
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int i = blockIdx.x * 1024 + tid;
    int x = 0, y = 0, z = 0, b = 0;
    const bool keep = is_first(src, i, n, keys, vals, mask, x, y, z, b);
    const unsigned long long m = __ballot(keep);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wv] = __popcll(m);
    __syncthreads();
    int off = bsum[blockIdx.x];
    for (int k = 0; k < wv; ++k) off += wsum[k];
    if (keep) {
        const int r = off + before;
        out_coords[ocs * (size_t)r] = x; out_coords[ocs * (size_t)r + 1] = y; out_coords[ocs * (size_t)r + 2] = z;
        if (ocs == 4) out_coords[4 * (size_t)r + 3] = b;
        if (sel) sel[r] = i;
    }
}

int launch_first_compact(const CoordSrc& src, int n, const u64* keys, const int* vals, unsigned mask, int* bsum, int* out_coords, int ocs,
                         int64_t* sel, int* count, hipStream_t s) {
    const int nb = (n + 1023) / 1024;
    hipLaunchKernelGGL(first_count_kernel, dim3(nb), dim3(1024), 0, s, src, n, keys, vals, mask, bsum);
    hipLaunchKernelGGL(block_scan_kernel, dim3(1), dim3(1024), 0, s, bsum, nb, count);
    hipLaunchKernelGGL(first_scatter_kernel, dim3(nb), dim3(1024), 0, s, src, n, keys, vals, mask, bsum, out_coords, ocs, sel);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- rank-ordered occupancy bitmaps: the coordinate maps of all four levels without a hash table ------------------------------
// When every cloud of a pass fits a dense bitmap (it does for anything the backbone is used on: bounding boxes of a few hundred voxels
// per axis), a level's coordinate map IS its bitmap plus a prefix popcount: row(voxel) = rank[word] + popcount(bits below it).  The
// bitmap of level l + 1 is the 2 x 2 x 2 OR-reduction of level l's (coordinates are floored to the coarser stride,
// src/coordinate_map.hpp:58-76, and the bitmap origin is a multiple of 16, so flooring is a shift of the cell index); sizes, rows and
// coordinates of all levels come out of bit operations and scans over a few MB instead of four hash tables of up to 48 MB built with
// two atomics per voxel (8 ms per fragment with the lookups that followed).  The INTERNAL row order of every level becomes rank order.
// Ranks run over 32 (x) x 8 x 8 bricks of words, so rows that are close in space are close in memory - the job the cell sort did
// for level 0.  The order is free: a row's sum is taken in kernel-offset order whatever its number, level 0 is handed back in the
// caller's order (operm), so every output bit is what the hash-table path produces (YOHO_FCGF_COORDS=hash, and the automatic fall-back
// for clouds too large for a bitmap or inputs with duplicate voxels).
// level l -> l + 1: out cell (X, Y, Z) = OR of the in cells (2X .. 2X+1, 2Y .. 2Y+1, 2Z .. 2Z+1); one thread per output word
__global__ void rk_coarsen_kernel(const RkDesc* __restrict__ din, const RkDesc* __restrict__ dout, const unsigned* __restrict__ bin, unsigned* __restrict__ bout) {
    const RkDesc di = din[blockIdx.y], d = dout[blockIdx.y];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)d.wx * d.ny * d.nz) return;
    const int w = (int)(i % d.wx), Y = (int)((i / d.wx) % d.ny), Z = (int)(i / ((long long)d.wx * d.ny));
    unsigned a = 0u, b = 0u;
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int y = 2 * Y + dy, z = 2 * Z + dz;
            if (y < di.ny && z < di.nz) {
                const unsigned* row = bin + di.base + ((long long)z * di.ny + y) * di.wx;
                a |= row[2 * w];
                if (2 * w + 1 < di.wx) b |= row[2 * w + 1];
            }
        }
    auto squeeze = [](unsigned v) {                      // bit i of the result = bits 2i | 2i+1 of v
        v = (v | (v >> 1)) & 0x55555555u;
        v = (v | (v >> 1)) & 0x33333333u;
        v = (v | (v >> 2)) & 0x0F0F0F0Fu;
        v = (v | (v >> 4)) & 0x00FF00FFu;
        v = (v | (v >> 8)) & 0x0000FFFFu;
        return v;
    };
    bout[d.base + i] = squeeze(a) | (squeeze(b) << 16);
}

// the word of rank entry r (brick order) of cloud descriptor d, 0 for the padding of incomplete bricks
__device__ __forceinline__ unsigned rk_word_of(const RkDesc& d, const unsigned* __restrict__ bm, int r, int& w, int& Y, int& Z) {
    const int in = r & 63, br = r >> 6;
    w = br % d.wx;
    const int byz = br / d.wx;
    Y = (byz % d.nyb) * 8 + (in & 7);
    Z = (byz / d.nyb) * 8 + (in >> 3);
    return (Y < d.ny && Z < d.nz) ? bm[d.base + ((long long)Z * d.ny + Y) * d.wx + w] : 0u;
}

// popcounts of 1024 rank entries: exclusive prefix inside the block -> rank[], block total -> btot[]   (grid: blocks of the cloud, cloud)
__global__ __launch_bounds__(1024) void rk_count_kernel(const RkDesc* __restrict__ desc, const unsigned* __restrict__ bm, int* __restrict__ rank,
                                                         int* __restrict__ btot) {
    __shared__ int wsum[16];
    const RkDesc d = desc[blockIdx.y];
    if ((int)blockIdx.x * 1024 >= d.nrank) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r = blockIdx.x * 1024 + tid;
    int w, Y, Z;
    const int v = r < d.nrank ? __popc(rk_word_of(d, bm, r, w, Y, Z)) : 0;
    int sc = v;
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(sc, o); if (lane >= o) sc += t; }
    if (lane == 63) wsum[wv] = sc;
    __syncthreads();
    int off = 0;
    for (int k = 0; k < wv; ++k) off += wsum[k];
    if (r < d.nrank) rank[d.rbase + r] = off + sc - v;
    if (tid == 1023) btot[d.blk0 + blockIdx.x] = off + sc;
}

// finishes rank[] (adds the scanned block offsets) and writes the level's rows in rank order: coords[row] = (x, y, z, cloud)
__global__ __launch_bounds__(256) void rk_rows_kernel(const RkDesc* __restrict__ desc, const unsigned* __restrict__ bm, int* __restrict__ rank,
                                                      const int* __restrict__ bscan, int ts, int* __restrict__ coords) {
    const RkDesc d = desc[blockIdx.y];
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= d.nrank) return;
    int w, Y, Z;
    unsigned word = rk_word_of(d, bm, r, w, Y, Z);
    const int row0 = rank[d.rbase + r] + bscan[d.blk0 + (r >> 10)];
    rank[d.rbase + r] = row0;
    int k = 0;
    while (word) {
        const int bit = __ffs(word) - 1;
        word &= word - 1u;
        reinterpret_cast<int4*>(coords)[row0 + k] = make_int4(d.x0 + (w * 32 + bit) * ts, d.y0 + Y * ts, d.z0 + Z * ts, (int)blockIdx.y);
        ++k;
    }
}

// caller's level-0 row i -> internal row: operm[row] = i (the input voxels of a cloud are distinct, so every row has one writer)
__global__ void rk_operm_kernel(const int* __restrict__ c4, int n, const RkDesc* __restrict__ desc, const unsigned* __restrict__ bm,
                                const int* __restrict__ rank, int* __restrict__ operm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int4 c = reinterpret_cast<const int4*>(c4)[i];
    const int r = rk_lookup(desc[c.w], bm, rank, c.x, c.y, c.z, 0);
    if (r >= 0) operm[r] = i;
}

__global__ void rk_fill_kernel(const int* __restrict__ c4, int n, const RkDesc* __restrict__ desc, unsigned* __restrict__ bm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int4 c = reinterpret_cast<const int4*>(c4)[i];
    const RkDesc d = desc[c.w];
    const int bx = c.x - d.x0;
    atomicOr(bm + d.base + ((long long)(c.z - d.z0) * d.ny + (c.y - d.y0)) * d.wx + (bx >> 5), 1u << (bx & 31));
}

void launch_rk_fill(const int* c4, int n, const RkLevel& l0, hipStream_t s) {
    hipLaunchKernelGGL(rk_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, s, c4, n, l0.d, l0.bm);
}
void launch_rk_coarsen(const RkLevel& in, const RkLevel& out, int nb, hipStream_t s) {
    hipLaunchKernelGGL(rk_coarsen_kernel, dim3((unsigned)((out.maxw + 255) / 256), nb), dim3(256), 0, s, in.d, out.d, in.bm, out.bm);
}
void launch_rk_count(const RkLevel& l, int nb, int* total, hipStream_t s) {
    hipLaunchKernelGGL(rk_count_kernel, dim3((l.maxr + 1023) / 1024, nb), dim3(1024), 0, s, l.d, l.bm, l.rank, l.btot);
    hipLaunchKernelGGL(block_scan_kernel, dim3(1), dim3(1024), 0, s, l.btot, l.blocks, total);
}
void launch_rk_rows(const RkLevel& l, int nb, int ts, int* coords, hipStream_t s) {
    hipLaunchKernelGGL(rk_rows_kernel, dim3((l.maxr + 255) / 256, nb), dim3(256), 0, s, l.d, l.bm, l.rank, l.btot, ts, coords);
}
void launch_rk_operm(const int* c4, int n, const RkLevel& l0, int* operm, hipStream_t s) {
    hipLaunchKernelGGL(rk_operm_kernel, dim3((n + 255) / 256), dim3(256), 0, s, c4, n, l0.d, l0.bm, l0.rank, operm);
}

// ---- batched voxelisation: the rotated copies of ONE cloud, copy = blockIdx.y --------------------------------------------------
// Per copy the same stages as fcgf_voxelize (insert-min, count, scan, scatter), but one launch per stage for up to VOX_BATCH
// copies: 300 k points are ~1200 workgroups, far too few to cover the latency of the table atomics, and 7 launches per copy were
// 105 per backbone pass.  The rotations travel in the kernel arguments.  A copy's table / block sums / counters are slices of one
// allocation; the scatter also writes the rotated fp32 points of the selected rows (the reference's pcd[sel].float(): the very f64
// values the voxel index was taken from), so no second pass over `sel` is needed.
constexpr int VOX_BATCH = 16;
struct VoxBatch {
    const double* pts; int n; double voxel;
    double R[VOX_BATCH][9];
    u64* keys; int* vals; unsigned cap;          // copy b: keys + b * cap
    int* bsum; int nblk;                         // copy b: bsum + b * (nblk + 1)
    int* dcount;                                 // copy b: [2b] voxels, [2b + 1] out-of-range flag
    int* coords; int64_t* sel; float* pts_sel;   // copy b: + b * n rows (pts_sel may be null)
    // rank-ordered bitmaps instead of the tables (rk != null): copy b's bitmap descriptor rk[b0 + b], the first point of voxel row r in first[r]
    const RkDesc* rk; const unsigned* bm; const int* rank; int* first; int b0;
};
__device__ __forceinline__ void vox_point(const VoxBatch& a, int b, int i, double& p0, double& p1, double& p2) {
    const double q0 = a.pts[3 * (size_t)i], q1 = a.pts[3 * (size_t)i + 1], q2 = a.pts[3 * (size_t)i + 2];
    const double* R = a.R[b];
    p0 = rot_coord(R, q0, q1, q2); p1 = rot_coord(R + 3, q0, q1, q2); p2 = rot_coord(R + 6, q0, q1, q2);
}
__global__ void vox_clear_kernel(u64* keys, int* vals, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < total) { keys[i] = HEMPTY; vals[i] = 0x7FFFFFFF; }
}
__global__ void vox_insert_kernel(VoxBatch a) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= a.n) return;
    double p0, p1, p2;
    vox_point(a, b, i, p0, p1, p2);
    const int x = voxel_index(p0, a.voxel), y = voxel_index(p1, a.voxel), z = voxel_index(p2, a.voxel);
    if (x < -VOX_LIM || x > VOX_LIM || y < -VOX_LIM || y > VOX_LIM || z < -VOX_LIM || z > VOX_LIM) atomicOr(a.dcount + 2 * b + 1, 1);
    const u64 key = pack_key(x, y, z, 0);
    u64* keys = a.keys + (size_t)b * a.cap;
    int* vals = a.vals + (size_t)b * a.cap;
    const unsigned mask = a.cap - 1;
    unsigned s = hslot(key, mask);
    for (;;) {
        const u64 old = atomicCAS(&keys[s], HEMPTY, key);
        if (old == HEMPTY || old == key) { atomicMin(&vals[s], i); return; }
        s = (s + 1) & mask;
    }
}
__device__ __forceinline__ bool vox_is_first(const VoxBatch& a, int b, int i, int& x, int& y, int& z, double& p0, double& p1, double& p2) {
    if (i >= a.n) return false;
    vox_point(a, b, i, p0, p1, p2);
    x = voxel_index(p0, a.voxel); y = voxel_index(p1, a.voxel); z = voxel_index(p2, a.voxel);
    if (a.rk) {
        const int r = rk_lookup(a.rk[a.b0 + b], a.bm, a.rank, x, y, z, 0);
        return r >= 0 && a.first[r] == i;
    }
    const int slot = hash_find_slot(a.keys + (size_t)b * a.cap, a.cap - 1, pack_key(x, y, z, 0));
    return a.vals[(size_t)b * a.cap + slot] == i;
}
// rank mode, pass 1: the voxel of every (point, copy) sets its bit; a voxel outside its copy's bitmap raises a.dcount[2b + 1]
__global__ void vox_fill_kernel(VoxBatch a, unsigned* bm) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= a.n) return;
    double p0, p1, p2;
    vox_point(a, b, i, p0, p1, p2);
    const int x = voxel_index(p0, a.voxel), y = voxel_index(p1, a.voxel), z = voxel_index(p2, a.voxel);
    const RkDesc d = a.rk[a.b0 + b];
    const int X = x - d.x0, Y = y - d.y0, Z = z - d.z0;
    if (X < 0 || X >= d.wx * 32 || Y < 0 || Y >= d.ny || Z < 0 || Z >= d.nz || x < -VOX_LIM || x > VOX_LIM || y < -VOX_LIM || y > VOX_LIM ||
        z < -VOX_LIM || z > VOX_LIM) { atomicOr(a.dcount + 2 * b + 1, 1); return; }
    // (bound by the rate of device atomics, ~22 G/s: 0.2 ms for the 4.5 M points of a 15-copy pass.  Reading the word first and skipping
    // the atomic when the bit is there was measured: 3 x SLOWER - 0.60 ms - the read goes to memory and sees the bit too rarely)
    atomicOr(bm + d.base + ((long long)Z * d.ny + Y) * d.wx + (X >> 5), 1u << (X & 31));
}
// rank mode, pass 2 (ranks finished): first[row of the voxel] = smallest point index
__global__ void vox_first_kernel(VoxBatch a) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= a.n) return;
    double p0, p1, p2;
    vox_point(a, b, i, p0, p1, p2);
    const int r = rk_lookup(a.rk[a.b0 + b], a.bm, a.rank, voxel_index(p0, a.voxel), voxel_index(p1, a.voxel), voxel_index(p2, a.voxel), 0);
    if (r >= 0) atomicMin(a.first + r, i);                  // (a read-and-skip in front of it: 0.18 -> 0.55 ms, as in vox_fill_kernel)
}
// rank[] += scanned block offsets (rk_rows_kernel does this for the coordinate maps, where it also writes the rows)
__global__ void rk_finish_kernel(const RkDesc* __restrict__ desc, int* __restrict__ rank, const int* __restrict__ bscan) {
    const RkDesc d = desc[blockIdx.y];
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < d.nrank) rank[d.rbase + r] += bscan[d.blk0 + (r >> 10)];
}
// per-workgroup axis-aligned bounds of (n,3) f64 points -> part[block][6] = (min x, y, z, max x, y, z); the host combines the blocks
__global__ __launch_bounds__(256) void aabb_kernel(const double* __restrict__ pts, int n, double* __restrict__ part) {
    __shared__ double red[4][6];
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    bool bad = false;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double v = pts[3 * (size_t)i + a];
            bad |= !(v > -1e300 && v < 1e300);                 // NaN / inf: reported as an unbounded box, the caller falls back to the tables
            lo[a] = fmin(lo[a], v); hi[a] = fmax(hi[a], v);
        }
    if (bad) { lo[0] = -1e308; hi[0] = 1e308; }
#pragma unroll
    for (int a = 0; a < 3; ++a)
        for (int o = 32; o >= 1; o >>= 1) { lo[a] = fmin(lo[a], __shfl_xor(lo[a], o)); hi[a] = fmax(hi[a], __shfl_xor(hi[a], o)); }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { for (int a = 0; a < 3; ++a) { red[w][a] = lo[a]; red[w][3 + a] = hi[a]; } }
    __syncthreads();
    if (threadIdx.x < 6) {
        double v = red[0][threadIdx.x];
        for (int ww = 1; ww < 4; ++ww) v = threadIdx.x < 3 ? fmin(v, red[ww][threadIdx.x]) : fmax(v, red[ww][threadIdx.x]);
        part[blockIdx.x * 6 + threadIdx.x] = v;
    }
}
__global__ __launch_bounds__(1024) void vox_count_kernel(VoxBatch a) {
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y;
    int x, y, z; double p0, p1, p2;
    const bool keep = vox_is_first(a, b, blockIdx.x * 1024 + tid, x, y, z, p0, p1, p2);
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wsum[wv] = __popcll(m);
    __syncthreads();
    if (tid == 0) { int t = 0; for (int k = 0; k < 16; ++k) t += wsum[k]; a.bsum[(size_t)b * (a.nblk + 1) + blockIdx.x] = t; }
}
// one workgroup per copy: exclusive scan of its block counts in place, total -> dcount[2b]
__global__ __launch_bounds__(1024) void vox_scan_kernel(VoxBatch a) {
    __shared__ int sh[1024];
    __shared__ int carry;
    const int tid = threadIdx.x, b = blockIdx.x;
    int* bsum = a.bsum + (size_t)b * (a.nblk + 1);
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < a.nblk; b0 += 1024) {
        const int i = b0 + tid;
        const int v = i < a.nblk ? bsum[i] : 0;
        sh[tid] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int t = tid >= o ? sh[tid - o] : 0;
            __syncthreads();
            sh[tid] += t;
            __syncthreads();
        }
        if (i < a.nblk) bsum[i] = carry + sh[tid] - v;
        __syncthreads();
        if (tid == 0) carry += sh[1023];
        __syncthreads();
    }
    if (tid == 0) a.dcount[2 * b] = carry;
}
__global__ __launch_bounds__(1024) void vox_scatter_kernel(VoxBatch a) {
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y;
    const int i = blockIdx.x * 1024 + tid;
    int x = 0, y = 0, z = 0; double p0 = 0, p1 = 0, p2 = 0;
    const bool keep = vox_is_first(a, b, i, x, y, z, p0, p1, p2);
    const unsigned long long m = __ballot(keep);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wv] = __popcll(m);
    __syncthreads();
    int off = a.bsum[(size_t)b * (a.nblk + 1) + blockIdx.x];
    for (int k = 0; k < wv; ++k) off += wsum[k];
    if (keep) {
        const size_t r = (size_t)b * a.n + off + before;
        a.coords[3 * r] = x; a.coords[3 * r + 1] = y; a.coords[3 * r + 2] = z;
        a.sel[r] = i;
        if (a.pts_sel) { a.pts_sel[3 * r] = (float)p0; a.pts_sel[3 * r + 1] = (float)p1; a.pts_sel[3 * r + 2] = (float)p2; }
    }
}

// table value := row of the compacted map
__global__ void hash_set_rows_kernel(const int* coords, int n, const u64* keys, int* vals, unsigned mask) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int4 c = reinterpret_cast<const int4*>(coords)[r];
    const int slot = hash_find_slot(keys, mask, pack_key(c.x, c.y, c.z, c.w));
    vals[slot] = r;
}
void launch_hash_set_rows(const Level& L, hipStream_t s) {
    hipLaunchKernelGGL(hash_set_rows_kernel, dim3((L.n + 255) / 256), dim3(256), 0, s, L.coords, L.n, L.keys, L.vals, L.mask);
}

// map[k][n] = row of (coord(n) + sign * offset(k) * ts) in the table, -1 if absent; kernel index with x fastest.
// (rk != null: the looked-up level is a rank-ordered bitmap, `sh` = log2 of its stride; else its hash table.)
// Two cheap rejections before the hash probe: a coordinate that is not a multiple of the table's tensor stride ts_in
// cannot be in it (7 of 8 candidates of a transposed map, whose offsets live on the finer stride), and for a level-0
// table the occupancy bitmap (bm != null) answers "absent" for the two thirds of a 3^3 region that are empty.
__global__ void build_map_kernel(const int* out_coords, int nout, const u64* keys, const int* vals, unsigned mask, int ksize, int ts,
                                 int sign, int ts_in, const BmDesc* __restrict__ desc, const unsigned* __restrict__ bm, int* map,
                                 const RkDesc* __restrict__ rk = nullptr, const int* __restrict__ rkrank = nullptr, int sh = 0) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    if (n >= nout) return;
    const int h = ksize / 2;
    const int ox = (k % ksize - h) * ts * sign, oy = ((k / ksize) % ksize - h) * ts * sign, oz = (k / (ksize * ksize) - h) * ts * sign;
    const int4 c = reinterpret_cast<const int4*>(out_coords)[n];
    const int qx = c.x + ox, qy = c.y + oy, qz = c.z + oz;
    int row = -1;
    bool probe = ((qx | qy | qz) & (ts_in - 1)) == 0;                 // tensor strides are powers of two
    if (rk) {
        map[(size_t)k * nout + n] = probe ? rk_lookup(rk[c.w], bm, rkrank, qx, qy, qz, sh) : -1;
        return;
    }
    if (probe && bm) {
        const BmDesc d = desc[c.w];
        const int bx = qx - d.x0, by = qy - d.y0, bz = qz - d.z0;
        if (bx >= 0 && bx < d.wx * 32 && by >= 0 && by < d.ny && bz >= 0 && bz < d.nz)
            probe = (bm[d.base + ((long long)bz * d.ny + by) * d.wx + (bx >> 5)] >> (bx & 31)) & 1u;
    }
    if (probe) {
        const int slot = hash_find_slot(keys, mask, pack_key(qx, qy, qz, c.w));
        row = slot < 0 ? -1 : vals[slot];
    }
    map[(size_t)k * nout + n] = row;
}

// The 3^3 stride-1 map of a level onto itself is symmetric under the point reflection of the kernel: (k, in = i, out = o) is a
// pair iff (26 - k, in = o, out = i) is.  So only the offsets k < 13 are looked up; a hit also fills map[26 - k][i] = o (each
// (k', row) entry has one possible writer: the row at coord(row) + offset(k'), so the stores do not race), k = 13 is the identity,
// and the upper half is preset to -1 by the caller.  Halves the hash probes of the largest maps.
__global__ void build_map_sym_kernel(const int* out_coords, int nout, const u64* keys, const int* vals, unsigned mask, int ts,
                                     const BmDesc* __restrict__ desc, const unsigned* __restrict__ bm, int* map,
                                     const RkDesc* __restrict__ rk = nullptr, const int* __restrict__ rkrank = nullptr, int sh = 0) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;                                  // 0..13
    if (n >= nout) return;
    if (k == 13) { map[(size_t)13 * nout + n] = n; return; }
    const int ox = (k % 3 - 1) * ts, oy = ((k / 3) % 3 - 1) * ts, oz = (k / 9 - 1) * ts;
    const int4 c = reinterpret_cast<const int4*>(out_coords)[n];
    const int qx = c.x + ox, qy = c.y + oy, qz = c.z + oz;
    int row = -1;
    bool probe = true;
    if (rk) {
        row = rk_lookup(rk[c.w], bm, rkrank, qx, qy, qz, sh);
        map[(size_t)k * nout + n] = row;
        if (row >= 0) map[(size_t)(26 - k) * nout + row] = n;
        return;
    }
    if (bm) {
        const BmDesc d = desc[c.w];
        const int bx = qx - d.x0, by = qy - d.y0, bz = qz - d.z0;
        if (bx >= 0 && bx < d.wx * 32 && by >= 0 && by < d.ny && bz >= 0 && bz < d.nz)
            probe = (bm[d.base + ((long long)bz * d.ny + by) * d.wx + (bx >> 5)] >> (bx & 31)) & 1u;
    }
    if (probe) {
        const int slot = hash_find_slot(keys, mask, pack_key(qx, qy, qz, c.w));
        row = slot < 0 ? -1 : vals[slot];
    }
    map[(size_t)k * nout + n] = row;
    if (row >= 0) map[(size_t)(26 - k) * nout + row] = n;
}

// A transposed convolution's kernel map is the strided convolution's with input and output exchanged (MinkowskiEngine asks its
// manager for the same map with is_transpose, src/convolution_transpose_cpu.cpp:75-107): up[k][f] = c  iff  down[k][c] = f.
// `up` is preset to -1; every (k, f) has at most one coarse row c, so the stores do not race.
__global__ void invert_map_kernel(const int* __restrict__ down, int ncoarse, int nfine, int* __restrict__ up) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y;
    if (c >= ncoarse) return;
    const int f = down[(size_t)k * ncoarse + c];
    if (f >= 0) up[(size_t)k * nfine + f] = c;
}

// the one launch site of each map kernel: the lookup says which of the two coordinate paths the looked-up level lives on
void launch_build_map(const int* out_coords, int nout, const LevelLookup& in, int ksize, int ts, int sign, int ts_in, int* map, hipStream_t s) {
    if (nout == 0) return;
    hipLaunchKernelGGL(build_map_kernel, dim3((nout + 255) / 256, ksize * ksize * ksize), dim3(256), 0, s, out_coords, nout, in.keys, in.vals, in.mask, ksize,
                       ts, sign, ts_in, in.desc, in.bm, map, in.rk, in.rank, in.sh);
}
void launch_build_map_sym(const int* coords, int n, const LevelLookup& in, int ts, int* map, hipStream_t s) {
    hipLaunchKernelGGL(build_map_sym_kernel, dim3((n + 255) / 256, 14), dim3(256), 0, s, coords, n, in.keys, in.vals, in.mask, ts, in.desc, in.bm, map,
                       in.rk, in.rank, in.sh);
}
void launch_invert_map(const int* down, int ncoarse, int nfine, int* up, hipStream_t s) {
    hipLaunchKernelGGL(invert_map_kernel, dim3((ncoarse + 255) / 256, 27), dim3(256), 0, s, down, ncoarse, nfine, up);
}

// Rows of a level sorted by the parity class of their coordinates on the next coarser stride (8 classes, each padded with
// -1 to a multiple of 128 slots = one workgroup of the fine-level kernel).  A transposed convolution reaches a fine row
// from 1, 2, 4 or 8 of the 27 offsets - per axis: offset 0 if the coordinate is even on the coarse stride, +-1 if odd -
// and the set is the same for the whole class, so class-pure tiles skip the other offsets (sp_next_offset).  The order
// inside a class follows the atomics and does not matter: every row's sum is taken in kernel-offset order.  (PAR_PAD: sparse.h)
__device__ __forceinline__ int parity_class(int4 c, int sh) { return ((c.x >> sh) & 1) | (((c.y >> sh) & 1) << 1) | (((c.z >> sh) & 1) << 2); }

// A workgroup takes PAR_ROWS rows (eight per thread) and adds its class counts to the global counters once: with one row per
// thread the 8 atomics per workgroup on ONE cache line - 41 k of them on a 1.3 M-row level, serialised in the L2 - were most of
// the 60 us either kernel took (the same finding as bbox_kernel's).
constexpr int PAR_ROWS = 2048;
__global__ __launch_bounds__(256) void parity_count_kernel(const int* __restrict__ coords, int n, int sh, int* __restrict__ cnt) {
    __shared__ int lc[8];
    if (threadIdx.x < 8) lc[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PAR_ROWS / 256; ++u) {
        const int i = blockIdx.x * PAR_ROWS + u * 256 + threadIdx.x;
        if (i < n) atomicAdd(&lc[parity_class(reinterpret_cast<const int4*>(coords)[i], sh)], 1);
    }
    __syncthreads();
    if (threadIdx.x < 8 && lc[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], lc[threadIdx.x]);
}

// cnt[0..7]: class sizes, cnt[8..15]: cursors (zeroed); perm: n + 8 * PAR_PAD slots preset to -1
__global__ __launch_bounds__(256) void parity_scatter_kernel(const int* __restrict__ coords, int n, int sh, int* __restrict__ cnt,
                                                             int* __restrict__ perm) {
    __shared__ int lc[8], lbase[8];
    if (threadIdx.x < 8) lc[threadIdx.x] = 0;
    __syncthreads();
    int cls[PAR_ROWS / 256], pos[PAR_ROWS / 256];
#pragma unroll
    for (int u = 0; u < PAR_ROWS / 256; ++u) {
        const int i = blockIdx.x * PAR_ROWS + u * 256 + threadIdx.x;
        cls[u] = 0; pos[u] = 0;
        if (i < n) {
            cls[u] = parity_class(reinterpret_cast<const int4*>(coords)[i], sh);
            pos[u] = atomicAdd(&lc[cls[u]], 1);
        }
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        int base = 0;
        for (int c = 0; c < (int)threadIdx.x; ++c) base += (cnt[c] + PAR_PAD - 1) / PAR_PAD * PAR_PAD;
        lbase[threadIdx.x] = base + (lc[threadIdx.x] ? atomicAdd(&cnt[8 + threadIdx.x], lc[threadIdx.x]) : 0);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PAR_ROWS / 256; ++u) {
        const int i = blockIdx.x * PAR_ROWS + u * 256 + threadIdx.x;
        if (i < n) perm[lbase[cls[u]] + pos[u]] = i;
    }
}
void launch_parity_order(const int* coords, int n, int sh, int* cnt, int* perm, hipStream_t s) {
    hipLaunchKernelGGL(parity_count_kernel, dim3((n + PAR_ROWS - 1) / PAR_ROWS), dim3(256), 0, s, coords, n, sh, cnt);
    hipLaunchKernelGGL(parity_scatter_kernel, dim3((n + PAR_ROWS - 1) / PAR_ROWS), dim3(256), 0, s, coords, n, sh, cnt, perm);
}

// Level-0 rows grouped by the 8^3-voxel cell they lie in (cells in Morton order inside a cloud, 16 cells per axis with
// wrap-around): the rows a workgroup's 128 output rows gather are then mostly shared (a surface patch and its one-voxel
// halo) and hit in the L2 instead of each coming from the MALL / HBM, and the coarser levels - compacted in first-occurrence
// order - inherit the grouping.  Counting sort: cell histogram, scan (in-block + block totals), scatter; the order inside a
// cell follows the atomics and does not matter: a row's result does not depend on where the row sits, and the final kernel
// writes through the permutation, so the caller's row order is kept.
constexpr int CELL_SH = 3;                       // (CELL_PER_CLOUD = 16^3 and the threshold CELL_SORT_MIN_ROWS: sparse.h)
__device__ __forceinline__ int cell_of(int4 c) {
    auto spread = [](unsigned v) { v &= 15u; v = (v | (v << 4)) & 0x0C3u; v = (v | (v << 2)) & 0x249u; return v; };     // abcd -> a00b00c00d
    return c.w * CELL_PER_CLOUD + (int)(spread(c.x >> CELL_SH) | (spread(c.y >> CELL_SH) << 1) | (spread(c.z >> CELL_SH) << 2));
}

__global__ void cell_count_kernel(const int* __restrict__ coords, int n, int* __restrict__ cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) atomicAdd(&cnt[cell_of(reinterpret_cast<const int4*>(coords)[i])], 1);
}

// cnt[1024 b .. 1024 b + 1023] -> exclusive prefix inside the block, block total -> btot[b]
__global__ __launch_bounds__(1024) void cell_scan_kernel(int* __restrict__ cnt, int* __restrict__ btot) {
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int v = cnt[blockIdx.x * 1024 + tid];
    int s = v;
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(s, o); if (lane >= o) s += t; }
    if (lane == 63) wsum[wv] = s;
    __syncthreads();
    int off = 0;
    for (int k = 0; k < wv; ++k) off += wsum[k];
    cnt[blockIdx.x * 1024 + tid] = off + s - v;
    if (tid == 1023) btot[blockIdx.x] = off + s;
}

__global__ void cell_scatter_kernel(const int* __restrict__ coords, int n, const int* __restrict__ pre, const int* __restrict__ btot,
                                    int* __restrict__ cursor, int* __restrict__ perm, int* __restrict__ sorted) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int4 c = reinterpret_cast<const int4*>(coords)[i];
    const int cell = cell_of(c);
    const int r = btot[cell >> 10] + pre[cell] + atomicAdd(&cursor[cell], 1);
    perm[r] = i;
    reinterpret_cast<int4*>(sorted)[r] = c;
}
// cnt: 2 * nb * CELL_PER_CLOUD ints (histogram -> in-block prefix | cursors), btot: the scan blocks + 1
void launch_cell_sort(const int* coords, int n, int nb, int* cnt, int* btot, int* perm, int* sorted, hipStream_t s) {
    const int ncell = nb * CELL_PER_CLOUD, nblk = ncell / 1024;
    (void)hipMemsetAsync(cnt, 0, sizeof(int) * 2 * (size_t)ncell, s);
    hipLaunchKernelGGL(cell_count_kernel, dim3((n + 255) / 256), dim3(256), 0, s, coords, n, cnt);
    hipLaunchKernelGGL(cell_scan_kernel, dim3(nblk), dim3(1024), 0, s, cnt, btot);
    hipLaunchKernelGGL(block_scan_kernel, dim3(1), dim3(1024), 0, s, btot, nblk, btot + nblk);
    hipLaunchKernelGGL(cell_scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, s, coords, n, cnt, btot, cnt + ncell, perm, sorted);
}

// Bounding boxes of the clouds of a pass.  A workgroup scans a run of <= rows_per_wg rows of ONE cloud (the clouds' row ranges are in
// the kernel arguments; workgroup -> (cloud, run) by walking the clouds' run counts) and leaves its box in part[block] = (cloud, lo,
// hi); bbox_reduce_kernel combines the blocks.  No atomics here: the first version let a run straddle clouds and flushed a thread's
// box with six atomics at the boundary - 256 threads x 6 atomics on one cache line per boundary, serialised at ~50 ns each, were
// 75 of the kernel's 80 us on a 15-cloud pass (the row loop without them: 5 us).
// FROM3: the rows come from the caller's (n,3) matrix and the (n,4) rows with the cloud index are written on the way.
template <bool FROM3>
__global__ __launch_bounds__(256) void bbox_kernel(const int* __restrict__ coords, int rows_per_wg, int* __restrict__ part, CloudOff o, int nb,
                                                   int* __restrict__ c4) {
    __shared__ int red[4][6];
    int b = 0, base = 0;
    for (; b < nb; ++b) {
        const int runs = (o.off[b + 1] - o.off[b] + rows_per_wg - 1) / rows_per_wg;
        if ((int)blockIdx.x < base + runs) break;
        base += runs;
    }
    int* p = part + 7 * blockIdx.x;
    if (b == nb) { if (threadIdx.x == 0) p[0] = -1; return; }
    const int r0 = o.off[b] + ((int)blockIdx.x - base) * rows_per_wg, r1 = min(o.off[b + 1], r0 + rows_per_wg);
    int lo[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, hi[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
    for (int i = r0 + threadIdx.x; i < r1; i += 256) {
        int x, y, z;
        if constexpr (FROM3) {
            x = coords[3 * (size_t)i]; y = coords[3 * (size_t)i + 1]; z = coords[3 * (size_t)i + 2];
            reinterpret_cast<int4*>(c4)[i] = make_int4(x, y, z, b);
        } else {
            const int4 c = reinterpret_cast<const int4*>(coords)[i];
            x = c.x; y = c.y; z = c.z;
        }
        lo[0] = min(lo[0], x); lo[1] = min(lo[1], y); lo[2] = min(lo[2], z);
        hi[0] = max(hi[0], x); hi[1] = max(hi[1], y); hi[2] = max(hi[2], z);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
        for (int o2 = 32; o2 >= 1; o2 >>= 1) {
            lo[a] = min(lo[a], __shfl_xor(lo[a], o2));
            hi[a] = max(hi[a], __shfl_xor(hi[a], o2));
        }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[w][0] = lo[0]; red[w][1] = lo[1]; red[w][2] = lo[2]; red[w][3] = hi[0]; red[w][4] = hi[1]; red[w][5] = hi[2]; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int ww = 1; ww < 4; ++ww)
            for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], red[ww][a]); hi[a] = max(hi[a], red[ww][3 + a]); }
        p[0] = lo[0] <= hi[0] ? b : -1;
        p[1] = lo[0]; p[2] = lo[1]; p[3] = lo[2]; p[4] = hi[0]; p[5] = hi[1]; p[6] = hi[2];
    }
}

__global__ __launch_bounds__(1024) void bbox_reduce_kernel(const int* __restrict__ part, int nblocks, int nb, int* __restrict__ bb) {
    __shared__ int lb[64 * 6];
    for (int i = threadIdx.x; i < 64 * 6; i += 1024) lb[i] = (i % 6) < 3 ? 0x7FFFFFFF : (int)0x80000000;
    __syncthreads();
    for (int b = threadIdx.x; b < nblocks; b += 1024) {
        const int* p = part + 7 * b;
        const int cl = p[0];
        if (cl >= 0 && cl < 64) {
            atomicMin(&lb[cl * 6 + 0], p[1]); atomicMin(&lb[cl * 6 + 1], p[2]); atomicMin(&lb[cl * 6 + 2], p[3]);
            atomicMax(&lb[cl * 6 + 3], p[4]); atomicMax(&lb[cl * 6 + 4], p[5]); atomicMax(&lb[cl * 6 + 5], p[6]);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb * 6; i += 1024) bb[i] = lb[i];
}
// partial boxes of nblk runs (none: nothing is launched); from3: the caller's (n,3) rows, and the (n,4) rows are written to c4
void launch_bbox(const int* coords, bool from3, int rows_per_wg, int* part, const CloudOff& o, int nb, int* c4, int nblk, hipStream_t s) {
    if (nblk && from3) hipLaunchKernelGGL(bbox_kernel<true>, dim3(nblk), dim3(256), 0, s, coords, rows_per_wg, part, o, nb, c4);
    else if (nblk) hipLaunchKernelGGL(bbox_kernel<false>, dim3(nblk), dim3(256), 0, s, coords, rows_per_wg, part, o, nb, c4);
}
void launch_bbox_reduce(const int* part, int nblk, int nb, int* bb, hipStream_t s) {
    hipLaunchKernelGGL(bbox_reduce_kernel, dim3(1), dim3(1024), 0, s, part, nblk, nb, bb);
}

// Dense occupancy bitmap of the level-0 voxels of every cloud of a pass (bounding box + K/2 margin, x fastest, 32 voxels per
// word): the first convolution tests its K^3 neighbours with one cached word read each instead of a hash probe, and the
// level-0 kernel maps use it as a presence filter in front of the hash table.
__global__ void bitmap_fill_kernel(const int* __restrict__ coords, int n, const BmDesc* __restrict__ desc, unsigned* __restrict__ bm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int4 c = reinterpret_cast<const int4*>(coords)[i];
    const BmDesc d = desc[c.w];
    const int bx = c.x - d.x0;
    atomicOr(bm + d.base + ((long long)(c.z - d.z0) * d.ny + (c.y - d.y0)) * d.wx + (bx >> 5), 1u << (bx & 31));
}
void launch_bitmap_fill(const int* coords, int n, const BmDesc* desc, unsigned* bm, hipStream_t s) {
    hipLaunchKernelGGL(bitmap_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, s, coords, n, desc, bm);
}

int build_table(const CoordSrc& src, int n, Level& L, hipStream_t s) {
    const unsigned cap = L.mask + 1;
    hipLaunchKernelGGL(hash_clear_kernel, dim3((cap + 255) / 256), dim3(256), 0, s, L.keys, L.vals, cap);
    if (n > 0) hipLaunchKernelGGL(hash_insert_min_kernel, dim3((n + 255) / 256), dim3(256), 0, s, src, n, L.keys, L.vals, L.mask);
    HIPCHK(hipGetLastError());
    return 0;
}

// voxelisation (fcgf_feat.py:33-43): first point of every voxel in input order -> sel (ascending), integer coordinates
// the selected points, rotated like the voxelisation saw them, as fp32 (the reference's pcd[sel].float())
// m_dev (or null): the row count lives on the device (batched voxelisation: no host round trip between its stages)
__global__ void rotate_sel_kernel(CoordSrc src, const int64_t* __restrict__ sel, int m, float* __restrict__ out, const int* __restrict__ m_dev) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (m_dev ? *m_dev : m)) return;
    double p0, p1, p2;
    point_of(src, (int)sel[i], p0, p1, p2);
    out[3 * (size_t)i] = (float)p0; out[3 * (size_t)i + 1] = (float)p1; out[3 * (size_t)i + 2] = (float)p2;
}

int fcgf_rotate_select(const double* pts, const double* R_host, const int64_t* sel, int m, float* out, hipStream_t s) {
    if (m == 0) return 0;
    CoordSrc src{nullptr, pts, 1.0, 1, R_host ? 1 : 0, {0}};
    if (R_host) for (int i = 0; i < 9; ++i) src.R[i] = R_host[i];
    hipLaunchKernelGGL(rotate_sel_kernel, dim3((m + 255) / 256), dim3(256), 0, s, src, sel, m, out, (const int*)nullptr);
    HIPCHK(hipGetLastError());
    return 0;
}

// voxelisation (fcgf_feat.py:33-43): first point of every voxel in input order -> sel (ascending), integer coordinates.
// R_host (9 doubles, row major) or null: the points are rotated (p' = R p, f64) on the fly; pts_sel (n,3) f32 or null
// receives the rotated selected points.
int fcgf_voxelize(yoho_ctx* ctx, const double* pts, int n, const double* R_host, double voxel, int64_t* sel, int* coords, float* pts_sel,
                  int* count_host, hipStream_t s) {
    if (n == 0) { *count_host = 0; return 0; }
    int rc;
    const unsigned cap = table_cap(n);
    if ((rc = ensure_ws(ctx, (size_t)cap * 12 + (size_t)n / 256 + 8192, s))) return rc;
    Arena ar{(char*)ctx->ws.p, 0, ctx->ws.bytes};
    Level L;
    L.mask = cap - 1; L.keys = ar.take<u64>(cap); L.vals = ar.take<int>(cap);
    int* dcount = ar.take<int>(2);                       // [0] number of voxels, [1] out-of-range flag
    int* bsum = ar.take<int>((size_t)(n + 1023) / 1024 + 1);
    if (ar.over) return arena_overrun(ar, "fcgf_voxelize");
    HIPCHK(hipMemsetAsync(dcount, 0, 2 * sizeof(int), s));
    CoordSrc src{nullptr, pts, voxel, 1, R_host ? 1 : 0, {0}, dcount + 1};
    if (R_host) for (int i = 0; i < 9; ++i) src.R[i] = R_host[i];
    if ((rc = build_table(src, n, L, s))) return rc;
    if ((rc = launch_first_compact(src, n, L.keys, L.vals, L.mask, bsum, coords, 3, sel, dcount, s))) return rc;
    int hc[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(hc, dcount, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *count_host = hc[0];
    if (hc[1]) {
        *count_host = 0;
        set_error("voxelisation: a point's voxel index is outside +-%d (cloud extent / voxel size too large, or a non-finite point)", VOX_LIM);
        return YOHO_EINVAL;
    }
    if (pts_sel) return fcgf_rotate_select(pts, R_host, sel, *count_host, pts_sel, s);
    return 0;
}

// The argument block of copies b0 .. b0 + nbc - 1 of a batched voxelisation: `a` arrives with the arrays of ALL copies (tables, or
// bitmaps when rk != null) and leaves with this batch's rotations and slices.
static VoxBatch vox_batch(VoxBatch a, const double* R_host, int b0, int nbc) {
    for (int b = 0; b < nbc; ++b) for (int i = 0; i < 9; ++i) a.R[b][i] = R_host[9 * (size_t)(b0 + b) + i];
    if (a.keys) { a.keys += (size_t)b0 * a.cap; a.vals += (size_t)b0 * a.cap; }
    a.bsum += (size_t)b0 * (a.nblk + 1);
    a.dcount += 2 * (size_t)b0;
    a.coords += (size_t)b0 * a.n * 3; a.sel += (size_t)b0 * a.n;
    if (a.pts_sel) a.pts_sel += (size_t)b0 * a.n * 3;
    a.b0 = a.rk ? b0 : 0;
    return a;
}

// nb rotated copies of one cloud in one call: the stages of all copies are queued back to back (one hash table, block sums and
// counters per copy in the workspace) and the nb voxel counts come back with ONE read-back.  Outputs are laid out with n rows per
// copy: sel (nb, n), coords (nb, n, 3), pts_sel (nb, n, 3) or null; counts_host (nb).
// The batched voxelisation through rank-ordered bitmaps (RkDesc) instead of one hash table per copy: a copy's occupancy bitmap over a
// conservative box (the rotated corners of the cloud's bounds, two voxels of margin), ranks by prefix popcount, first[row] = smallest
// point index by one atomicMin per point into a dense array that stays in the L2 - the tables took a CAS and an atomicMin per point
// into 180 MB (4.5 M points of a 15-copy pass: 0.41 ms for the inserts alone).  The compaction in first-occurrence order is the table
// path's (vox_count / vox_scan / vox_scatter with the lookup swapped), so the outputs are the same rows in the same order.
// Returns 0 = done, < 0 = error, 1 = not applicable (a copy too large for a bitmap, non-finite points, indices near the key range):
// the caller runs the table path, which also owns the exact range check and its error message.
static int voxelize_batch_rank(yoho_ctx* ctx, const double* pts, int n, const double* R_host, int nb, double voxel, int64_t* sel, int* coords,
                               float* pts_sel, int* counts_host, hipStream_t s) {
    int rc;
    const int gblk = std::min(256, (n + 255) / 256);
    if ((rc = ensure_ws(ctx, 64 * 1024, s))) return rc;
    Arena ar0{(char*)ctx->ws.p, 0, ctx->ws.bytes};
    double* dpart = ar0.take<double>(6 * (size_t)gblk);    // per-workgroup partial bounds of the cloud
    if (ar0.over) return arena_overrun(ar0, "fcgf_voxelize_batch: bounds");
    phase_mark(ctx, 0, s);
    double hpart[256 * 6];
    hipLaunchKernelGGL(aabb_kernel, dim3(gblk), dim3(256), 0, s, pts, n, dpart);
    HIPCHK(hipMemcpyAsync(hpart, dpart, sizeof(double) * 6 * gblk, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (int g = 0; g < gblk; ++g)
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], hpart[6 * g + a]); hi[a] = std::max(hi[a], hpart[6 * g + 3 + a]); }
    for (int a = 0; a < 3; ++a) if (!(lo[a] > -1e290 && hi[a] < 1e290 && lo[a] <= hi[a])) return 1;
    RkDesc hd[64];
    RkRun run;
    int maxr = 1;
    for (int b = 0; b < nb; ++b) {
        const double* R = R_host + 9 * (size_t)b;
        double bl[3] = {1e300, 1e300, 1e300}, bh[3] = {-1e300, -1e300, -1e300};
        for (int c = 0; c < 8; ++c) {
            const double px = (c & 1) ? hi[0] : lo[0], py = (c & 2) ? hi[1] : lo[1], pz = (c & 4) ? hi[2] : lo[2];
            for (int a = 0; a < 3; ++a) {
                const double v = R[3 * a] * px + R[3 * a + 1] * py + R[3 * a + 2] * pz;
                bl[a] = std::min(bl[a], v); bh[a] = std::max(bh[a], v);
            }
        }
        long long vlo[3], dim[3];
        for (int a = 0; a < 3; ++a) {
            const double l = std::floor(bl[a] / voxel) - 2.0, h = std::floor(bh[a] / voxel) + 2.0;
            if (!(l > -(double)VOX_LIM && h < (double)VOX_LIM)) return 1;
            vlo[a] = (long long)l; dim[a] = (long long)h - (long long)l + 1;
        }
        if (!rk_layout(hd[b], run, (int)vlo[0], (int)vlo[1], (int)vlo[2], dim[0], dim[1], dim[2])) return 1;
        maxr = std::max(maxr, hd[b].nrank);
    }
    const long long words = run.words, ranks = run.ranks;
    const int blocks = run.blocks;
    const int nblk = (n + 1023) / 1024;
    const size_t need = (size_t)words * 4 + (size_t)ranks * 4 + (size_t)blocks * 4 + (size_t)nb * n * 4 + ((size_t)nblk + 1) * 4 * nb + sizeof(RkDesc) * 64 + 65536;
    if ((rc = ensure_ws(ctx, need, s))) { if (rc == YOHO_ENOMEM) clear_error(); return rc == YOHO_ENOMEM ? 1 : rc; }      // multi-GB ranks that cannot be had: the table path needs 12 bytes per point and copy
    Arena ar{(char*)ctx->ws.p, 0, ctx->ws.bytes};
    int* dcount = ar.take<int>(2 * (size_t)nb + 2);      // per copy: [0] number of voxels, [1] flag: a voxel outside the bitmap / the key range
    RkDesc* dd = reinterpret_cast<RkDesc*>(ar.take<char>(sizeof(RkDesc) * 64));
    unsigned* bm = ar.take<unsigned>((size_t)words + 2);
    int* rank = ar.take<int>((size_t)ranks + 1);
    int* btot = ar.take<int>((size_t)blocks + 2);
    int* first = ar.take<int>((size_t)nb * n);
    int* bsum = ar.take<int>(((size_t)nblk + 1) * nb);
    if (ar.over) return arena_overrun(ar, "fcgf_voxelize_batch: rank arrays");
    HIPCHK(hipMemcpyAsync(dd, hd, sizeof(RkDesc) * nb, hipMemcpyHostToDevice, s));      // hd lives until the synchronisation below
    HIPCHK(hipMemsetAsync(dcount, 0, sizeof(int) * (2 * nb + 2), s));
    HIPCHK(hipMemsetAsync(bm, 0, ((size_t)words + 2) * 4, s));
    HIPCHK(hipMemsetAsync(first, 0x7F, (size_t)nb * n * 4, s));
    const VoxBatch all{pts, n, voxel, {}, nullptr, nullptr, 0, bsum, nblk, dcount, coords, sel, pts_sel, dd, bm, rank, first, 0};
    auto batch = [&](int b0, int nbc) { return vox_batch(all, R_host, b0, nbc); };
    for (int b0 = 0; b0 < nb; b0 += VOX_BATCH) {
        const int nbc = std::min(VOX_BATCH, nb - b0);
        hipLaunchKernelGGL(vox_fill_kernel, dim3((n + 255) / 256, nbc), dim3(256), 0, s, batch(b0, nbc), bm);
    }
    hipLaunchKernelGGL(rk_count_kernel, dim3((maxr + 1023) / 1024, nb), dim3(1024), 0, s, dd, bm, rank, btot);
    hipLaunchKernelGGL(block_scan_kernel, dim3(1), dim3(1024), 0, s, btot, blocks, dcount + 2 * nb);
    hipLaunchKernelGGL(rk_finish_kernel, dim3((maxr + 255) / 256, nb), dim3(256), 0, s, dd, rank, btot);
    for (int b0 = 0; b0 < nb; b0 += VOX_BATCH) {
        const int nbc = std::min(VOX_BATCH, nb - b0);
        hipLaunchKernelGGL(vox_first_kernel, dim3((n + 255) / 256, nbc), dim3(256), 0, s, batch(b0, nbc));
    }
    for (int b0 = 0; b0 < nb; b0 += VOX_BATCH) {
        const int nbc = std::min(VOX_BATCH, nb - b0);
        const VoxBatch a = batch(b0, nbc);
        hipLaunchKernelGGL(vox_count_kernel, dim3(nblk, nbc), dim3(1024), 0, s, a);
        hipLaunchKernelGGL(vox_scan_kernel, dim3(nbc), dim3(1024), 0, s, a);
        hipLaunchKernelGGL(vox_scatter_kernel, dim3(nblk, nbc), dim3(1024), 0, s, a);
    }
    HIPCHK(hipGetLastError());
    phase_mark(ctx, -1, s);
    int hc[130];
    HIPCHK(hipMemcpyAsync(hc, dcount, sizeof(int) * 2 * nb, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int b = 0; b < nb; ++b) if (hc[2 * b + 1]) return 1;           // outside the box or the key range: the table path decides
    for (int b = 0; b < nb; ++b) counts_host[b] = hc[2 * b];
    return 0;
}

int fcgf_voxelize_batch(yoho_ctx* ctx, const double* pts, int n, const double* R_host, int nb, double voxel, int64_t* sel, int* coords,
                        float* pts_sel, int* counts_host, hipStream_t s) {
    if (nb < 1 || nb > 64) { set_error("fcgf_voxelize_batch: 1..64 copies per call"); return YOHO_EINVAL; }
    for (int b = 0; b < nb; ++b) counts_host[b] = 0;
    if (n == 0) return 0;
    int rc;
    if (!ctx->fcgf_hash_coords) {
        rc = voxelize_batch_rank(ctx, pts, n, R_host, nb, voxel, sel, coords, pts_sel, counts_host, s);
        if (rc <= 0) return rc;
    }
    const unsigned cap = table_cap(n);
    const int nblk = (n + 1023) / 1024;
    const size_t per = (size_t)cap * 12 + ((size_t)nblk + 1) * 4 + 1024;
    if ((rc = ensure_ws(ctx, per * nb + 8192, s))) return rc;
    Arena ar{(char*)ctx->ws.p, 0, ctx->ws.bytes};
    int* dcount = ar.take<int>(2 * (size_t)nb);          // per copy: [0] number of voxels, [1] out-of-range flag
    u64* keys = ar.take<u64>((size_t)cap * nb);
    int* vals = ar.take<int>((size_t)cap * nb);
    int* bsum = ar.take<int>(((size_t)nblk + 1) * nb);
    if (ar.over) return arena_overrun(ar, "fcgf_voxelize_batch: hash tables");
    phase_mark(ctx, 0, s);
    HIPCHK(hipMemsetAsync(dcount, 0, 2 * sizeof(int) * nb, s));
    {
        const size_t total = (size_t)cap * nb;
        hipLaunchKernelGGL(vox_clear_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, keys, vals, total);
    }
    // the stages of up to VOX_BATCH copies per launch (copy = blockIdx.y; the rotations travel in the kernel arguments)
    const VoxBatch all{pts, n, voxel, {}, keys, vals, cap, bsum, nblk, dcount, coords, sel, pts_sel, nullptr, nullptr, nullptr, nullptr, 0};
    for (int b0 = 0; b0 < nb; b0 += VOX_BATCH) {
        const int nbc = nb - b0 < VOX_BATCH ? nb - b0 : VOX_BATCH;
        const VoxBatch a = vox_batch(all, R_host, b0, nbc);
        hipLaunchKernelGGL(vox_insert_kernel, dim3((n + 255) / 256, nbc), dim3(256), 0, s, a);
        hipLaunchKernelGGL(vox_count_kernel, dim3(nblk, nbc), dim3(1024), 0, s, a);
        hipLaunchKernelGGL(vox_scan_kernel, dim3(nbc), dim3(1024), 0, s, a);
        hipLaunchKernelGGL(vox_scatter_kernel, dim3(nblk, nbc), dim3(1024), 0, s, a);
    }
    HIPCHK(hipGetLastError());
    phase_mark(ctx, -1, s);
    int hc[128];
    HIPCHK(hipMemcpyAsync(hc, dcount, 2 * sizeof(int) * nb, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int b = 0; b < nb; ++b) {
        if (hc[2 * b + 1]) {
            set_error("voxelisation: a point's voxel index is outside +-%d in rotated copy %d (cloud extent / voxel size too large, or a non-finite point)", VOX_LIM, b);
            return YOHO_EINVAL;
        }
        counts_host[b] = hc[2 * b];
    }
    return 0;
}

}  // namespace yoho