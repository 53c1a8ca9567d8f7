// Shared by the irrep-GEMM kernels (gemmf.hip: fgemm_kernel, 256 x 256 tiles, one four-wave workgroup per CU; gemmf2.hip: fgemm2_kernel,
// 256 x 128 tiles, two workgroups per CU, fgemm3 / fgemm3c / fgemm3s, 256 x 256 tiles in eight waves, and the cone GEMM cgemm_kernel):
// operand pack constants, launch arguments, the tile work map, the residual start and the coefficient epilogue.
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
// coef_epilogue and are compiled into the -DYOHO_EXPERIMENTS library only.
enum { F2_NOSTORE = 0x100, F2_MIX = 0x200, F2_ST_SC1 = 0x400, F2_ST_NT = 0x800, F2_SPARSE4 = 0x1000, F2_SPARSE16 = 0x2000 };

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

void fgemm_fill_args(FGemmArgs& a, const Layer& L, const char* Bplanes, int kppad, int nT32, const float* res, float* out, int* rflag);
int launch_fgemm2(const FGemmArgs& a, int flags, hipStream_t s);
int launch_fgemm3(const FGemmArgs& a, int flags, hipStream_t s);
int fgemm2_init();

}  // namespace yoho
