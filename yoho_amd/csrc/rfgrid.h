// The cell-sorted grid and the fixed-order f64 block sum of refine.hip, shared with plane.hip: the device-side pieces (rf_cell /
// rf_slot, RfGrid, rf_walk, rf_block_sum) are inline here, the grid build (rf_grid_layout / rf_build_grid and its kernels) stays in
// refine.hip, where THE GRID, THE QUERY and THE SUMS are described, and is declared below.  Include from translation units compiled
// with -ffp-contract=off only.
#pragma once
#include "common.h"
#include "nnmath.h"
#include <cmath>

namespace yoho {

typedef unsigned long long u64;
constexpr int RF_CLAMP = (1 << 20) - 1;
constexpr int RF_NONE = 0x7FFFFFFF;
constexpr double RF_MIN_CELL = 0x1p-60;

// gridnn.hip's gn_cell / gn_key / gn_slot
__device__ __forceinline__ int rf_cell(double x, double inv_cell) {
    double c = floor(x * inv_cell);
    c = fmin(fmax(c, -(double)RF_CLAMP), (double)RF_CLAMP);          // NaN -> -RF_CLAMP
    return (int)c;
}
__device__ __forceinline__ int rf_clampi(int c) { return c < -RF_CLAMP ? -RF_CLAMP : (c > RF_CLAMP ? RF_CLAMP : c); }
__device__ __forceinline__ unsigned rf_slot(int cx, int cy, int cz, unsigned mask) {
    const u64 key = ((u64)(unsigned)(cx + (1 << 20)) << 42) | ((u64)(unsigned)(cy + (1 << 20)) << 21) | (u64)(unsigned)(cz + (1 << 20));
    return (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 33) & mask;
}

struct RfGrid {
    const int* start;        // [nslots + 1] first sorted position of a bucket
    const float4* pk;        // [Nt] sorted points (x, y, z, original index)
    double inv_cell;
    unsigned mask;           // nslots - 1
    float gate2;
};

// ---- the query -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void rf_walk(const RfGrid& g, const float (&q)[3], float& bd, int& bi) {
    const int cx = rf_cell((double)q[0], g.inv_cell), cy = rf_cell((double)q[1], g.inv_cell), cz = rf_cell((double)q[2], g.inv_cell);
    bd = __builtin_inff();
    bi = RF_NONE;
    for (int c = 0; c < 27; ++c) {
        const unsigned s = rf_slot(rf_clampi(cx + c % 3 - 1), rf_clampi(cy + (c / 3) % 3 - 1), rf_clampi(cz + c / 9 - 1), g.mask);
        const int p1 = g.start[s + 1];
        for (int p = g.start[s]; p < p1; ++p) {
            const float4 v = g.pk[p];
            const float b[3] = {v.x, v.y, v.z};
            const float d2 = dist2_f32<3>(q, b);
            const int j = __float_as_int(v.w);
            if (d2 < g.gate2 && (d2 < bd || (d2 == bd && j < bi))) { bd = d2; bi = j; }
        }
    }
}

// ---- the sums ------------------------------------------------------------------------------------------------------------------
template <int NV>
__device__ __forceinline__ void rf_block_sum(double (&v)[NV], double* __restrict__ slab_row) {
    __shared__ double red[4][NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v[k] = __dadd_rn(v[k], __shfl_xor(v[k], o));
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) red[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const int k = threadIdx.x;
        slab_row[k] = __dadd_rn(__dadd_rn(__dadd_rn(red[0][k], red[1][k]), red[2][k]), red[3][k]);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
struct RfGridWs {
    unsigned nslots; int bits, nblk;
    unsigned* keys[2]; int* idx[2];
    int* hist; int* start; float4* pk;
};

// the grid's buffers as one run of takes inside the caller's arena layout; the build queues the sort on `s` (refine.hip)
void rf_grid_layout(Arena& ar, int Nt, RfGridWs& w);
int rf_build_grid(const float* tgt, int Nt, float max_dist, const RfGridWs& w, RfGrid& g, hipStream_t s);
inline bool rf_bad_radius(float r) { return !(r > 0.f) || !std::isfinite(r); }

}  // namespace yoho
