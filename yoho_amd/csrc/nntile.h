// What the nearest-neighbour searches share beside the distance arithmetic and the packed key of nnmath.h (match.hip, matchf.hip,
// knn.hip, gridnn.hip): the (distance, index) minimum, the cut of the targets into segments, the (D, SQUARED) dispatch and the
// pieces of the 256-target LDS tile.  Like nnmath.h, only translation units built with -ffp-contract=off may include this
// (yoho_amd/build.py EXTRA).
#pragma once
#include <type_traits>
#include "nnmath.h"

namespace yoho {

// ---- the (distance, index) minimum: the smaller distance, on a tie the lower index.  A NaN distance never wins; a search that saw
// nothing but NaN keeps its initial index (0x7FFFFFFF in gridnn.hip, mapped to 0 there).
template <typename T>
__device__ __forceinline__ void nn_take_min(T& bd, int& bi, T d, int i) {
    if (d < bd || (d == bd && i < bi)) { bd = d; bi = i; }
}

// over the 64 lanes of a wave; every lane ends with the winner
template <typename T>
__device__ __forceinline__ void nn_wave_min(T& bd, int& bi) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const T od = __shfl_xor(bd, o);
        const int oi = __shfl_xor(bi, o);
        nn_take_min(bd, bi, od, oi);
    }
}

// over the 256 threads of a workgroup through rd / ri (256 entries each, in LDS): the winner is in rd[0] / ri[0] when this returns
template <typename T>
__device__ __forceinline__ void nn_block_min(T* rd, int* ri, T bd, int bi) {
    __syncthreads();                                          // the previous winner has been read
    rd[threadIdx.x] = bd; ri[threadIdx.x] = bi;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (threadIdx.x < o) nn_take_min(rd[threadIdx.x], ri[threadIdx.x], rd[threadIdx.x + o], ri[threadIdx.x + o]);
        __syncthreads();
    }
}

// ---- the cut of Nt targets into segments over blockIdx.y (nn32seg_kernel, knn_kernel; restated by tests/nn_ref.seg_len): a few
// workgroups per CU whatever Ns is, no segment below 64 targets, segments of a multiple of 16 rows (tiles start 16-byte aligned for
// every D).  rows = source rows per workgroup.  one_below_2p20: a single segment below 2^20 pairs (a single launch).
struct NnPlan { int segLen, nseg; };
inline NnPlan nn_segment_plan(int Ns, int Nt, int rows, int nCU, bool one_below_2p20) {
    const int rb = (Ns + rows - 1) / rows;
    int nseg = one_below_2p20 && (size_t)Ns * Nt < (1u << 20) ? 1 : (4 * nCU + rb - 1) / rb;
    const int maxseg = (Nt + 63) / 64;
    nseg = nseg < 1 ? 1 : (nseg > maxseg ? maxseg : nseg);
    int segLen = (Nt + nseg - 1) / nseg;
    segLen = (segLen + 15) / 16 * 16;
    return {segLen, (Nt + segLen - 1) / segLen};
}

// ---- f(integral_constant<int, D>, bool_constant<SQUARED>) for the descriptor widths the kernels are built for; false: D is neither
template <typename F>
inline bool nn_dispatch(int D, bool squared, F&& f) {
    auto both = [&](auto d) { if (squared) f(d, std::true_type{}); else f(d, std::false_type{}); };
    if (D == 32) both(std::integral_constant<int, 32>{});
    else if (D == 3) both(std::integral_constant<int, 3>{});
    else return false;
    return true;
}

// ---- the tile: NN_TT target rows in LDS at a stride of LD floats (LD = D, or D + 4 to spread the bank quads of knn_kernel's reads),
// 16 lanes interleaved over the targets of a source row, one or two source rows per thread (16 rows apart).
constexpr int NN_SPLIT = 16;    // lanes per source row: a thread visits the targets congruent to its lane mod 16
constexpr int NN_TT = 256;      // target rows per LDS tile; tiles start at the segment's start

// row `row` of src into registers, clamped to the last row (the surplus threads compute and are not stored)
template <int D>
__device__ __forceinline__ void nn_load_row(float (&a)[D], const float* __restrict__ src, int row, int Ns) {
    const int rc = row < Ns ? row : Ns - 1;
#pragma unroll
    for (int k = 0; k < D; ++k) a[k] = src[(size_t)rc * D + k];
}

// two rows at once, the loads interleaved.  (The rows are separate arrays on purpose: with one a[2][D] the compiler orders the operands of
// dist2_f32's sums differently and packs nn32seg_kernel's fp32 math into other instructions - profiles/nn_family_refactor.md.)
template <int D>
__device__ __forceinline__ void nn_load_row(float (&a0)[D], float (&a1)[D], const float* __restrict__ src, int row0, int row1, int Ns) {
    const int rc0 = row0 < Ns ? row0 : Ns - 1, rc1 = row1 < Ns ? row1 : Ns - 1;
#pragma unroll
    for (int k = 0; k < D; ++k) { a0[k] = src[(size_t)rc0 * D + k]; a1[k] = src[(size_t)rc1 * D + k]; }
}

// rows t0 .. t0 + nt of tgt into the tile, by all 256 threads between two barriers of the caller.  vec4: the caller's word that nt * D
// is a multiple of 4 and row t0 16-byte aligned (a multiple of 16 rows from the cloud's base); the padded tile needs it.
template <int D, int LD>
__device__ __forceinline__ void nn_stage_tile(float* tile, const float* __restrict__ tgt, int t0, int nt, bool vec4) {
    static_assert(LD == D || (D % 4 == 0 && LD % 4 == 0), "a padded tile is staged in float4");
    if (vec4) {
        const float4* g4 = reinterpret_cast<const float4*>(tgt + (size_t)t0 * D);
        float4* t4 = reinterpret_cast<float4*>(tile);
        if constexpr (LD == D) {
            for (int i = threadIdx.x; i < nt * D / 4; i += 256) t4[i] = g4[i];
        } else {
            for (int i = threadIdx.x; i < nt * (D / 4); i += 256) t4[(i / (D / 4)) * (LD / 4) + i % (D / 4)] = g4[i];
        }
    } else {
        for (int i = threadIdx.x; i < nt * D; i += 256) tile[i] = tgt[(size_t)t0 * D + i];
    }
}

// row t of the tile into registers (ds_read_b128 where D % 4 == 0)
template <int D, int LD>
__device__ __forceinline__ void nn_tile_row(float (&b)[D], const float* tile, int t) {
    const float* bp = tile + t * LD;
    if constexpr (D % 4 == 0) {
#pragma unroll
        for (int k = 0; k < D / 4; ++k) {
            const float4 v = reinterpret_cast<const float4*>(bp)[k];
            b[4 * k] = v.x; b[4 * k + 1] = v.y; b[4 * k + 2] = v.z; b[4 * k + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < D; ++k) b[k] = bp[k];
    }
}

// the winner among the NN_SPLIT partial minima that the lanes of row rr left in rd / ri
__device__ __forceinline__ void nn_row_winner(const float* rd, const int* ri, int rr, float& bd, int& bi) {
    bd = rd[rr * NN_SPLIT];
    bi = ri[rr * NN_SPLIT];
    for (int k = 1; k < NN_SPLIT; ++k) nn_take_min(bd, bi, rd[rr * NN_SPLIT + k], ri[rr * NN_SPLIT + k]);
}

}  // namespace yoho
