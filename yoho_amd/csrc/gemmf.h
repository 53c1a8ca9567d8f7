// Shared by the irrep-GEMM kernels (gemmf.hip: fgemm_kernel, 256 x 256 tiles, one four-wave workgroup per CU; gemmf2.hip: fgemm2_kernel,
// 256 x 128 tiles, two workgroups per CU, fgemm3 / fgemm3c / fgemm3s, 256 x 256 tiles in eight waves, and the cone GEMMs cgemm_kernel / cgemmk_kernel):
// operand pack constants, launch arguments, the tile work map, the residual start and the coefficient epilogue - for the 32 x 32 x 16
// MFMA of the K16 loops and for the 16 x 16 x 32 MFMA of the large layers' K32 loops (fgemmk, fgemm2k, fgemm3k, cgemmk), whose product order is here.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "common.h"

namespace yoho {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef unsigned uintx4 __attribute__((ext_vector_type(4)));
typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

constexpr int FG_STAGE = 32768;               // bytes of one operand tile per K32 stage
constexpr int FG_LDS = 4 * FG_STAGE;          // 2 buffers x (A + B)

// irreps in launch order (heaviest first)
static const int FG_ORD_D[NIR_ORD] = {5, 4, 3, 3, 1};
static const int FG_ORD_R[NIR_ORD] = {4, 3, 1, 2, 0};
static const int FG_IR_BASE[5] = {0, 1, 10, 19, 35};
static const int FG_IR_D[5] = {1, 3, 3, 4, 5};

struct FGemmArgs {
    const char* A;        // weight planes, all irreps
    const char* B;        // activation planes, all irreps
    const float* bias;
    const float* res;     // fp32 coefficient slabs [tile32][60 q][cout8][h][kp32][4] or null (q-major: a workgroup owns one q)
    float* out;           // same layout
    long long a_off[NIR_ORD], b_off[NIR_ORD];
    int NT[NIR_ORD], MT[NIR_ORD], rot[NIR_ORD];
    int dim[NIR_ORD], qbase[NIR_ORD];     // dimension and first coefficient index of the t-th irrep in launch order
    int cin, cout, kppad, nT32;
    float descale;
    int* rflag;           // fp16 range flag: raised when an output coefficient will not fit the consumer's fp16 planes (x HF_ASCALE)
    const unsigned* amax; // gconv_mode 7 (fgemm3c): largest |value| of the B planes as a float bit pattern, left by their producer; null = fgemm3
    int* tix;             // fgemm3k's tile tickets: [0..7] next slot of XCD x, [8] finished workgroups (all 0 between launches), or null = one static tile per workgroup
    int tiles;            // with tix: tiles a workgroup takes before it retires (FGEMM_TILES_MAX at most)
};

template <int I, int N, typename Fn>
__device__ __forceinline__ void sfor(Fn&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        sfor<I + 1, N>(f);
    }
}

__device__ __forceinline__ floatx16 mfma_h(uintx4 a, uintx4 b, floatx16 c) {
    union { uintx4 u; halfx8 h; } ca, cb;
    ca.u = a; cb.u = b;
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(ca.h, cb.h, c, 0, 0, 0);
}

// uniform (SGPR) copy of a wave-uniform pointer
__device__ __forceinline__ const char* uniform_ptr(const char* p) {
    const unsigned long long v = reinterpret_cast<unsigned long long>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return reinterpret_cast<const char*>(((unsigned long long)hi << 32) | lo);
}

template <int MI, int NJ>
__device__ __forceinline__ void zero_acc(floatx16 (&acc)[MI][NJ]) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
}

// Work map, one workgroup per 256 x 256 tile.  Workgroup b runs on XCD b & 7.  A column tile (irrep t, ntile) and its MT[t] row tiles
// stay on one XCD (the B panel is then read from HBM once and served from that XCD's L2 to the other row tiles); the column tiles of
// every irrep are dealt round-robin over the XCDs so that all eight get the same mix of long and short K loops.  Returns false for a
// slot beyond the XCD's work.
__device__ __forceinline__ bool fg3_map(const FGemmArgs& a, int xcd, int slot, int& t, int& local, int& r) {
    int start = 0;
    for (int u = 0; u < NIR_ORD; ++u) {
        const int ru = (xcd + a.rot[u]) & 7;
        const int cnt = a.NT[u] > ru ? ((a.NT[u] - 1 - ru) / 8 + 1) * a.MT[u] : 0;
        if (slot < start + cnt) { t = u; local = slot - start; r = ru; return true; }
        start += cnt;
    }
    return false;
}

constexpr int FGEMM_TILES_MAX = 64;   // YOHO_FGEMM_TILES: 1 .. 64 tiles per fgemm3k workgroup
constexpr int FGEMM_TIX_INTS = 16;    // ints of one launch's ticket counters (FGemmArgs::tix: nine used)

// grid of the work maps: 8 x the longest XCD list, `per_tile` workgroups per 256 x 256 tile
inline int fgemm_grid(const FGemmArgs& a, int per_tile) {
    int tot = 0;
    for (int x = 0; x < 8; ++x) {
        int n = 0;
        for (int t = 0; t < NIR_ORD; ++t) {
            const int r = (x + a.rot[t]) & 7;
            if (a.NT[t] > r) n += ((a.NT[t] - 1 - r) / 8 + 1) * a.MT[t] * per_tile;
        }
        tot = n > tot ? n : tot;
    }
    return 8 * tot;
}

// YOHO_FGEMM_DEBUG experiments (launch_fgemm2 / launch_fgemm3).  F2_MIX is a work-map choice of fgemm2; the others change the stores of
// coef_epilogue and are compiled into the -DYOHO_EXPERIMENTS library only.  F2_K32 is no experiment: launch_fgemm sets it for the layers
// of fgemm_layer_k32 (the 16x16x32 kernels); the experiments build's YOHO_FGEMM_DEBUG=k16 leaves it off (the K16 loops, every blocking).
enum { F2_NOSTORE = 0x100, F2_MIX = 0x200, F2_ST_SC1 = 0x400, F2_ST_NT = 0x800, F2_SPARSE4 = 0x1000, F2_SPARSE16 = 0x2000, F2_K32 = 0x4000 };

// float offset of four channels from o (half = second four of their eight) at keypoint kp32 of a 32-keypoint tile in FGemmArgs::res / out
__device__ __forceinline__ size_t slab_off(int tile32, int q, int cout8, int o, int half, int kp32) {
    return (((((size_t)tile32 * G + q) * cout8 + (o >> 3)) * 2 + half) * TILE + kp32) * 4;
}

// The accumulators start from the residual (scaled by 1 / descale, a power of two): its loads are in flight together with the first
// DMA stages.  Added in the epilogue instead they are serialised behind the accumulators' registers (no room to prefetch) and cost a
// third of a millisecond per pass.
// Where a wave's MI x NJ MFMA tiles (32 x 32 each) lie: row0 = first of the irrep's (i, o) rows (the 32 rows of an MFMA tile share i: cout
// is a multiple of 32), kp0 = first keypoint of coefficient column jidx, d / qbase = dimension and first coefficient of the irrep.
// D[row][col]: lane (col = lane & 31, half = lane >> 5), reg e -> row = (e & 3) + 8 * (e >> 2) + 4 * half.
template <int MI, int NJ>
__device__ __forceinline__ void residual_start(floatx16 (&acc)[MI][NJ], int row0, int kp0, int jidx, int d, int qbase, const float* res, float descale,
                                               int cout, int nT32, int lane) {
    const float inv = 1.f / descale;
    const int half = lane >> 5, kp32 = lane & 31, cout8 = cout >> 3;
#pragma unroll
    for (int bi = 0; bi < NJ; ++bi) {
        const int tile32 = (kp0 >> 5) + bi;
#pragma unroll
        for (int ai = 0; ai < MI; ++ai) {
            const int rowb = row0 + ai * 32;
            const int iidx = rowb / cout, o0 = rowb - iidx * cout;
            const bool ok = tile32 < nT32 && iidx < d;
            const int q = qbase + iidx * d + jidx;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const size_t off = slab_off(tile32, q, cout8, o0 + q4 * 8 + half * 4, half, kp32);
                // branch-free, so that all loads go out back to back
                const floatx4 v = *reinterpret_cast<const floatx4*>(res + (ok ? off : 0)) * (ok ? inv : 0.f);
                acc[ai][bi][4 * q4 + 0] = v.x; acc[ai][bi][4 * q4 + 1] = v.y;
                acc[ai][bi][4 * q4 + 2] = v.z; acc[ai][bi][4 * q4 + 3] = v.w;
            }
        }
    }
}

// Coefficient epilogue: descale, sqrt(60) * bias on the trivial irrep (d = 1: coefficient 0 carries it), store, range word.  Columns
// past the last keypoint tile and rows past the irrep hold padding: they are skipped BEFORE they reach `top`, the largest |coefficient|
// written (bit pattern; inf / NaN order above) - the transform kernel that reads the coefficients multiplies by HF_ASCALE and converts to fp16.
template <int MI, int NJ>
__device__ __forceinline__ void coef_epilogue(const floatx16 (&acc)[MI][NJ], int row0, int kp0, int jidx, int d, int qbase, float* out, const float* bias,
                                              float descale, int cout, int nT32, int* rflag, int lane, int flags) {
    const int half = lane >> 5, kp32 = lane & 31, cout8 = cout >> 3;
    unsigned top = 0u;
#ifdef YOHO_EXPERIMENTS
    if ((flags & F2_SPARSE4) && (blockIdx.x >> 3) % 4 != 0) flags |= F2_NOSTORE;          // only every 4th / 16th workgroup stores
    if ((flags & F2_SPARSE16) && (blockIdx.x >> 3) % 16 != 0) flags |= F2_NOSTORE;
    const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(out, 0, 0x7FFFFFFF, 0x00020000);
#endif
#pragma unroll
    for (int bi = 0; bi < NJ; ++bi) {
        const int tile32 = (kp0 >> 5) + bi;
        if (tile32 >= nT32) continue;
#pragma unroll
        for (int ai = 0; ai < MI; ++ai) {
            const int rowb = row0 + ai * 32;
            const int iidx = rowb / cout, o0 = rowb - iidx * cout;
            if (iidx >= d) continue;
            const int q = qbase + iidx * d + jidx;
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int o = o0 + q4 * 8 + half * 4;
                floatx4 val;
                val.x = acc[ai][bi][4 * q4 + 0]; val.y = acc[ai][bi][4 * q4 + 1];
                val.z = acc[ai][bi][4 * q4 + 2]; val.w = acc[ai][bi][4 * q4 + 3];
                val *= descale;
                if (d == 1) val += *reinterpret_cast<const floatx4*>(bias + o) * 7.745966692414834f;
                const size_t off = slab_off(tile32, q, cout8, o, half, kp32);
#ifdef YOHO_EXPERIMENTS
                if (flags & F2_ST_SC1) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uintx4, val), orsrc, (int)(off * 4), 0, 16);
                else if (flags & F2_ST_NT) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(uintx4, val), orsrc, (int)(off * 4), 0, 2);
                else if (!(flags & F2_NOSTORE))
#endif
                *reinterpret_cast<floatx4*>(out + off) = val;
                top = max(max(top, __float_as_uint(val.x) & 0x7FFFFFFFu), __float_as_uint(val.y) & 0x7FFFFFFFu);
                top = max(max(top, __float_as_uint(val.z) & 0x7FFFFFFFu), __float_as_uint(val.w) & 0x7FFFFFFFu);
            }
        }
    }
    note_range_bits(rflag, top, FP16_MAX / HF_ASCALE);
}

// ---------------------------------------------------------------------------------------------------------------
// The same three products on v_mfma_f32_16x16x32_f16: ONE MFMA spans a whole K32 stage of the packs (lane l holds row / column l & 15,
// k-group l >> 4 of the stage's four).  Product order per accumulator and K32 stage, for every kernel that uses this shape:
//     lo.hi (A lo plane x B hi plane), hi.lo, hi.hi          - the order of the K16 loops, one MFMA per product and stage instead of two.
// A wave's MI x NJ MFMA tiles are 16 x 16: D[row][col]: lane (col = lane & 15, g = lane >> 4), reg e -> row = 4 * g + e.  The four
// registers of a lane are still four consecutive output channels (second four of their eight when g is odd), so a tile's stores are
// slab_off's 16 bytes per lane exactly as with the 32 x 32 shape; two 16-column tiles make one 32-keypoint slab tile.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ floatx4 mfma_h16(uintx4 a, uintx4 b, floatx4 c) {
    union { uintx4 u; halfx8 h; } ca, cb;
    ca.u = a; cb.u = b;
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(ca.h, cb.h, c, 0, 0, 0);
}

// which layers run on this shape, in every blocking alike (the blockings stay bit-identical to one another): the two large layers
// 256 -> 512 and 512 -> 256.  A layer with 32 output channels keeps the K16 loop (fgemm3s), so does a short K (cin < 256: down to one stage).
inline bool fgemm_layer_k32(const FGemmArgs& a) { return a.cin >= 256 && a.cin % 64 == 0 && a.cout >= 256; }

// THE product order: the 3 NJ MFMAs of one 16-row block of a stage - lo.hi on the row's NJ accumulators, then hi.lo, then hi.hi.  The order
// is pinned (left alone the scheduler puts dependent MFMAs back to back); extra(m) is issued behind MFMA m (fragment reads, DMA pieces).
template <int NJ, typename Extra>
__device__ __forceinline__ void row_products32(floatx4 (&accrow)[NJ], const uintx4& al, const uintx4& ah, const uintx4 (&bh)[NJ], const uintx4 (&bl)[NJ],
                                               Extra&& extra) {
    sfor<0, 3 * NJ>([&](auto mc) {
        constexpr int m = decltype(mc)::value, j = m % NJ, p = m / NJ;
        accrow[j] = mfma_h16(p == 0 ? al : ah, p == 1 ? bl[j] : bh[j], accrow[j]);
        __builtin_amdgcn_sched_barrier(0);       // a read hoisted above its MFMA would be caught by that MFMA's lgkmcnt(0)
        extra(mc);
        __builtin_amdgcn_sched_barrier(0);
    });
}

// One whole K32 stage of a wave's MI x NJ tiles, fragments read as they are needed (the reference blockings fgemm256 / fgemm128; the
// default blocking's pipelined loop is gemmf2.hip's step32).  pa / pb: the stage's A / B image in LDS with the lane's offset applied
// ((lane >> 4) * k-group stride + (first row + (lane & 15)) * 16); a 16-row block is 256 bytes, LOB = offset of B's lo plane (A's: 16 KiB).
template <int LOB, int MI, int NJ>
__device__ __forceinline__ void stage32_plain(floatx4 (&acc)[MI][NJ], const char* pa, const char* pb) {
    uintx4 bh[NJ], bl[NJ], al[2], ah[2];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        bh[j] = *reinterpret_cast<const uintx4*>(pb + j * 256);
        bl[j] = *reinterpret_cast<const uintx4*>(pb + LOB + j * 256);
    }
    al[0] = *reinterpret_cast<const uintx4*>(pa + 16384);
    ah[0] = *reinterpret_cast<const uintx4*>(pa);
    sfor<0, MI>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        if constexpr (i + 1 < MI) {
            al[(i + 1) & 1] = *reinterpret_cast<const uintx4*>(pa + 16384 + (i + 1) * 256);
            ah[(i + 1) & 1] = *reinterpret_cast<const uintx4*>(pa + (i + 1) * 256);
        }
        row_products32(acc[i], al[i & 1], ah[i & 1], bh, bl, [](auto) {});
    });
}

template <int MI, int NJ>
__device__ __forceinline__ void zero_acc(floatx4 (&acc)[MI][NJ]) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
}

// Two 16-column tiles (one 32-keypoint slab tile) trade rows before they are stored: v_permlane16_swap + v_permlane32_swap leave lane l
// with keypoint l & 31 and channels 4 * (l >> 5) .. + 3 of the first (x) / second (y) eight of the tiles' sixteen rows, so that a store is
// 1 KiB of consecutive addresses, as with the 32 x 32 shape (four separate 256-byte runs per store cost 0.07 ms per big launch).
// TO_SLAB: MFMA layout -> slab layout (stores); else the inverse (residual loads): each swap undoes itself, so the inverse is the other order.
template <bool TO_SLAB>
__device__ __forceinline__ void swap_rows16(floatx4& x, floatx4& y) {
    typedef unsigned uintx2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        uintx2 r = {__float_as_uint(x[e]), __float_as_uint(y[e])};
        if constexpr (TO_SLAB) {
            r = __builtin_amdgcn_permlane16_swap(r.x, r.y, false, false);
            r = __builtin_amdgcn_permlane32_swap(r.x, r.y, false, false);
        } else {
            r = __builtin_amdgcn_permlane32_swap(r.x, r.y, false, false);
            r = __builtin_amdgcn_permlane16_swap(r.x, r.y, false, false);
        }
        x[e] = __uint_as_float(r.x); y[e] = __uint_as_float(r.y);
    }
}

template <int MI, int NJ>
__device__ __forceinline__ void residual_start(floatx4 (&acc)[MI][NJ], int row0, int kp0, int jidx, int d, int qbase, const float* res, float descale,
                                               int cout, int nT32, int lane) {
    static_assert(NJ % 2 == 0, "pairs of 16-column tiles");
    const float inv = 1.f / descale;
    const int half = lane >> 5, kp32 = lane & 31, cout8 = cout >> 3;
#pragma unroll
    for (int bi = 0; bi < NJ; bi += 2) {
        const int tile32 = (kp0 >> 5) + (bi >> 1);
#pragma unroll
        for (int ai = 0; ai < MI; ++ai) {
            const int rowb = row0 + ai * 16;
            const int iidx = rowb / cout, o0 = rowb - iidx * cout;
            const bool ok = tile32 < nT32 && iidx < d;
            const int q = qbase + iidx * d + jidx;
            // branch-free, so that all loads go out back to back
            const size_t off0 = slab_off(tile32, q, cout8, o0 + half * 4, half, kp32), off1 = slab_off(tile32, q, cout8, o0 + 8 + half * 4, half, kp32);
            acc[ai][bi] = *reinterpret_cast<const floatx4*>(res + (ok ? off0 : 0)) * (ok ? inv : 0.f);
            acc[ai][bi + 1] = *reinterpret_cast<const floatx4*>(res + (ok ? off1 : 0)) * (ok ? inv : 0.f);
            swap_rows16<false>(acc[ai][bi], acc[ai][bi + 1]);
        }
    }
}

template <int MI, int NJ>
__device__ __forceinline__ void coef_epilogue(const floatx4 (&acc)[MI][NJ], int row0, int kp0, int jidx, int d, int qbase, float* out, const float* bias,
                                              float descale, int cout, int nT32, int* rflag, int lane, int flags) {
    static_assert(NJ % 2 == 0, "pairs of 16-column tiles");
    const int half = lane >> 5, kp32 = lane & 31, cout8 = cout >> 3;
    unsigned top = 0u;
#pragma unroll
    for (int bi = 0; bi < NJ; bi += 2) {
        const int tile32 = (kp0 >> 5) + (bi >> 1);
        if (tile32 >= nT32) continue;
#pragma unroll
        for (int ai = 0; ai < MI; ++ai) {
            const int rowb = row0 + ai * 16;
            const int iidx = rowb / cout, o0 = rowb - iidx * cout;
            if (iidx >= d) continue;
            const int q = qbase + iidx * d + jidx;
            floatx4 v[2] = {acc[ai][bi], acc[ai][bi + 1]};
            swap_rows16<true>(v[0], v[1]);
#pragma unroll
            for (int h8 = 0; h8 < 2; ++h8) {
                const int o = o0 + h8 * 8 + half * 4;
                floatx4 val = v[h8] * descale;
                if (d == 1) val += *reinterpret_cast<const floatx4*>(bias + o) * 7.745966692414834f;
#ifdef YOHO_EXPERIMENTS
                if (!(flags & F2_NOSTORE))
#endif
                *reinterpret_cast<floatx4*>(out + slab_off(tile32, q, cout8, o, half, kp32)) = val;
                top = max(max(top, __float_as_uint(val.x) & 0x7FFFFFFFu), __float_as_uint(val.y) & 0x7FFFFFFFu);
                top = max(max(top, __float_as_uint(val.z) & 0x7FFFFFFFu), __float_as_uint(val.w) & 0x7FFFFFFFu);
            }
        }
    }
    note_range_bits(rflag, top, FP16_MAX / HF_ASCALE);
}

void fgemm_fill_args(FGemmArgs& a, const Layer& L, const char* Bplanes, int kppad, int nT32, const float* res, float* out, int* rflag);
int launch_fgemm2(const FGemmArgs& a, int flags, hipStream_t s);
int launch_fgemm3(const FGemmArgs& a, int flags, hipStream_t s);
int fgemm2_init();

}  // namespace yoho
