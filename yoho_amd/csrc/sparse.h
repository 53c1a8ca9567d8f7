// FCGF backbone, what its three translation units share:
//   spmaps.hip   points or voxel rows -> integer tables: hash tables, rank-ordered bitmaps, voxelisation, bounding boxes, kernel maps,
//                row orders;
//   spconv.hip   everything that multiplies: the sparse convolutions, the first-layer kernels, the heads, the row normalisation;
//   sparse.hip   the weights (FcgfNet) and the forward driver, which only takes workspace and calls the launch_* entries below.
// Here: the voxel key and its hash, the coordinate source of the table kernels, the lookups of the rank-ordered bitmaps (layout:
// rklayout.h), the argument blocks of the convolutions and the host entry points of the two kernel units.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"
#include "rklayout.h"

namespace yoho {

typedef unsigned long long u64;
constexpr u64 HEMPTY = ~0ull;

// 19 bits per axis (|voxel index| < 2^18) + 7 bits of cloud (batch) index
__device__ __forceinline__ u64 pack_key(int x, int y, int z, int b) {
    return ((u64)(unsigned)b << 57) | ((u64)(unsigned)((x + (1 << 18)) & 0x7FFFF) << 38) | ((u64)(unsigned)((y + (1 << 18)) & 0x7FFFF) << 19) |
           (u64)(unsigned)((z + (1 << 18)) & 0x7FFFF);
}
__device__ __forceinline__ unsigned hslot(u64 key, unsigned mask) { return (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 33) & mask; }
__device__ __forceinline__ int floor_to(int c, int ts) {            // floor(c / ts) * ts  (src/coordinate_map.hpp:58-76)
    if (ts <= 1) return c;
    int q = c / ts;
    if ((c % ts) != 0 && c < 0) --q;
    return q * ts;
}
__device__ __forceinline__ int hash_find_slot(const u64* keys, unsigned mask, u64 key) {
    unsigned s = hslot(key, mask);
    for (;;) {
        const u64 k = keys[s];
        if (k == key) return (int)s;
        if (k == HEMPTY) return -1;
        s = (s + 1) & mask;
    }
}

// voxel of point i: from integer coordinates (quantised to `ts`) or from f64 points (floor(p / voxel), fcgf_feat.py:34)
struct CoordSrc {
    const int* coords;       // (n,4) rows (x, y, z, cloud) or null
    const double* pts;       // (n,3) or null
    double voxel;
    int ts;
    int rot;                 // pts are rotated on the fly: p' = R p  (the 60 rotated copies of a fragment, YOHO_testset.py:143)
    double R[9];
    int* oor;                // optional device flag: raised when a point's voxel index does not fit the 19-bit key fields
    int* dup;                // optional device flag: raised by the table insert when a voxel arrives a second time
};
constexpr int VOX_LIM = (1 << 18) - 16;      // |voxel index| bound of pack_key, minus the reach of the coarsest kernel offsets

__device__ __forceinline__ long long rk_index(const RkDesc& d, int w, int Y, int Z) {
    return d.rbase + ((long long)((Z >> 3) * d.nyb + (Y >> 3)) * d.wx + w) * 64 + (Z & 7) * 8 + (Y & 7);
}
// row of the voxel at coordinate (qx, qy, qz) - a multiple of the level's stride 2^sh - or -1
__device__ __forceinline__ int rk_lookup(const RkDesc& d, const unsigned* __restrict__ bm, const int* __restrict__ rank, int qx, int qy, int qz, int sh) {
    const int X = (qx - d.x0) >> sh, Y = (qy - d.y0) >> sh, Z = (qz - d.z0) >> sh;
    if (X < 0 || X >= d.wx * 32 || Y < 0 || Y >= d.ny || Z < 0 || Z >= d.nz) return -1;
    const unsigned word = bm[d.base + ((long long)Z * d.ny + Y) * d.wx + (X >> 5)];
    const int bit = X & 31;
    if (!((word >> bit) & 1u)) return -1;
    return rank[rk_index(d, X >> 5, Y, Z)] + __popc(word & ((1u << bit) - 1u));
}

// row offsets of the concatenated clouds of a pass (row ranges off[0..nb]), in the kernel arguments: bbox_kernel<true> turns the (n,3)
// voxel rows into (n,4) rows with the cloud index
struct CloudOff { int off[65]; };

// one level of a pass: its rows and, on the hash path, its table
struct Level {
    int n = 0, ts = 1;
    int* coords = nullptr;
    u64* keys = nullptr;
    int* vals = nullptr;
    unsigned mask = 0;
};
// one level of the rank-ordered bitmaps: device arrays, and what the grids of its kernels need from the host descriptors
struct RkLevel {
    RkDesc* d = nullptr;     // [nb]
    unsigned* bm = nullptr;
    int* rank = nullptr;
    int* btot = nullptr;     // 1024-entry scan blocks
    int blocks = 0;
    long long maxw = 1;      // largest bitmap / rank array of one cloud
    int maxr = 1;
};
// how a kernel map finds the row of a voxel: the level's hash table, with the level-0 occupancy bitmap as an optional filter in front
// of it (desc, bm), or - rk != null - the level's rank-ordered bitmap (bm, rank, sh = log2 of its stride)
struct LevelLookup {
    const u64* keys; const int* vals; unsigned mask;
    const BmDesc* desc; const unsigned* bm;
    const RkDesc* rk; const int* rank; int sh;
};

constexpr int PAR_PAD = 128;                     // parity classes are padded to a multiple of this many slots (one fine-level workgroup)
constexpr int CELL_PER_CLOUD = 4096;
constexpr int CELL_SORT_MIN_ROWS = 1 << 18;      // measured: -0.2 ms on a 1.3 M-row pass (sort included), +0.06 ms on an 88 k-row pass
constexpr int SP_MAXK = 27;
constexpr int C1O_MAXK = 343;                    // the first-layer kernels hold up to 7^3 offsets

struct SpConvArgs {
    const float* in; int ldin, cin;
    const int* map;          // [K][nout] or null (K = 1, identity)
    int K, nout;
    const float* W;          // (K, cin, cout)
    const void* Wh;          // fp16x2 planes of W * 2^s in MFMA B-fragment order (null: fp32 MFMA path), see pack_w16
    float descale;           // 1 / (2^s * SP_ASCALE)
    int cout;
    float* out; int ldout, ocoff;
    const float* aff_s;      // per output channel affine (BN folded) or null
    const float* aff_t;      // shift / bias or null
    const float* res; int ldres, rcoff;    // residual added after the affine, or null
    int relu;
    const int* rowperm;      // fp16x2 kernels: tile slot -> output row (-1 = padding), or null (slot = row)
    int nslots;              // tile slots (= nout without a permutation)
    int debug;               // always 0.  The fine-level kernels still test it (once a timing switch): without the field and its two tests
                             // the compiler schedules spconv16w_kernel<1> differently (profiles/sparse_split.md), so it stays
    int norm;                // spconv16w_kernel<1>, cout == 32 only: rows /= |row| this many times in the epilogue (the feature head)
    const int* operm;        // with norm: output row -> caller's row (level-0 rows are kept in an internal order), or null
};
struct HeadsArgs {
    const float* in; int ldin;           // (n, ldin) rows; the first 32 NC1 columns are convolved
    int n;
    const void* W1; float descale1;      // pack_w16 planes, cout = 64
    const void* W2; float descale2;      // cout = 32
    const float* bias2;
    float* out;                          // (n, 32)
    int norm;
    const int* operm;                    // output row -> caller's row, or null
};
// the first convolution on the constant-one input: level-0 rows, their occupancy bitmaps (bm null: the level-0 hash table is probed),
// fp16 weight planes (null: fp32 weights W)
struct Conv1Args {
    const int* coords; int n;
    const BmDesc* desc; const unsigned* bm; long long bm_words;
    const u64* keys; unsigned mask;
    int ksize;
    const void* planes; float descale;
    const float* W; const float* aff_s; const float* aff_t;
    float* out;
};

inline unsigned table_cap(int n) {
    unsigned c = 64;
    while (c < 2u * (unsigned)(n > 0 ? n : 1)) c <<= 1;
    return c;
}

// The passes of the backbone size their workspace from estimates (fcgf_workspace_bytes, the voxelisations' formulas): how much they take
// depends on counts that come back in the middle of a pass, so they cannot measure first as bind_ws does.  Instead every group of takes
// is checked before the first launch that uses a pointer of the group.  An overrun is a defect of the estimate, not an exhausted
// device: YOHO_EINVAL, so that the recoveries that retry on YOHO_ENOMEM do not hide it.
inline int arena_overrun(const Arena& ar, const char* what) {
    set_error("internal: workspace estimate too small at %s: %zu > %zu", what, ar.off, ar.cap);
    return YOHO_EINVAL;
}

// ---- spmaps.hip.  The void entries only queue kernels on s: the stage that calls them checks hipGetLastError() once, behind its group
int build_table(const CoordSrc& src, int n, Level& L, hipStream_t s);
int launch_first_compact(const CoordSrc& src, int n, const u64* keys, const int* vals, unsigned mask, int* bsum, int* out_coords, int ocs,
                         int64_t* sel, int* count, hipStream_t s);
void launch_hash_set_rows(const Level& L, hipStream_t s);
void launch_bbox(const int* coords, bool from3, int rows_per_wg, int* part, const CloudOff& o, int nb, int* c4, int nblk, hipStream_t s);
void launch_bbox_reduce(const int* part, int nblk, int nb, int* bb, hipStream_t s);
void launch_rk_fill(const int* c4, int n, const RkLevel& l0, hipStream_t s);
void launch_rk_coarsen(const RkLevel& in, const RkLevel& out, int nb, hipStream_t s);
void launch_rk_count(const RkLevel& l, int nb, int* total, hipStream_t s);                      // in-block ranks, then the scan of the block totals
void launch_rk_rows(const RkLevel& l, int nb, int ts, int* coords, hipStream_t s);
void launch_rk_operm(const int* c4, int n, const RkLevel& l0, int* operm, hipStream_t s);
void launch_cell_sort(const int* coords, int n, int nb, int* cnt, int* btot, int* perm, int* sorted, hipStream_t s);
void launch_bitmap_fill(const int* coords, int n, const BmDesc* desc, unsigned* bm, hipStream_t s);
void launch_build_map(const int* out_coords, int nout, const LevelLookup& in, int ksize, int ts, int sign, int ts_in, int* map, hipStream_t s);
void launch_build_map_sym(const int* coords, int n, const LevelLookup& in, int ts, int* map, hipStream_t s);
void launch_invert_map(const int* down, int ncoarse, int nfine, int* up, hipStream_t s);
void launch_parity_order(const int* coords, int n, int sh, int* cnt, int* perm, hipStream_t s);

// ---- spconv.hip
int launch_spconv(const SpConvArgs& a, hipStream_t s);
void launch_conv1(const Conv1Args& a, int nCU, hipStream_t s);
void launch_heads_fused(const HeadsArgs& a, int nCU, hipStream_t s);
void launch_fill_ones(float* p, int n, hipStream_t s);
void launch_row_normalize(const float* in, int n, int c, float* out, int twice, const int* operm, hipStream_t s);

}  // namespace yoho
