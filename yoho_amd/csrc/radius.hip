// Training-set generation (include/yoho_trainset.h): what the reference's YOHO_Trainset.py does beside the backbone passes.
//
//   radius_kernel<count / fill> + radius_scan_kernel   trainset_create.PCA_keys_sample   YOHO_Trainset.py:57-61
//   trainset_gather_kernel                              trainset_create.trainset          YOHO_Trainset.py:222-228
//
// yoho_radius_pairs: np.where(|a_i - b_j| < radius) in np.where's order without an (Na, Nb) matrix and without atomics deciding a
// position.  Three launches: the count instantiation writes how many pairs every row of `a` has, one workgroup scans the counts into
// 64-bit row offsets (and the total into `count`), the fill instantiation evaluates the SAME predicate (radius_pred, one function
// for both) and writes row i's pairs from offset[i] on.  In both a wave owns a row and walks the targets 64 at a time; the fill pass
// ranks the hits of a chunk with __ballot + popcount below the lane on top of a running row base, so j ascends within the row.
// `b` is staged through LDS in tiles of RP_TILE points, structure of arrays (48 KB), shared by the RP_WAVES rows of a workgroup.
// The predicate is f32 without contraction (this file is compiled with -ffp-contract=off, yoho_amd/build.py) and its square root is
// the correctly rounded one, obtained as knn.hip obtains it: the f64 square root of the f32 sum rounded to f32 (53 >= 2 * 24 + 2 bits).
// Only sums within 1e-6 relative of radius^2 pay for it: RadiusTest carries two bounds on d2 outside which the comparison of the
// rounded root is already decided (radius_test below has the argument).
#include "common.h"
#include "yoho_trainset.h"
#include <cmath>
#include <limits>

namespace yoho {

constexpr int RP_TILE = 4096;    // points of b per LDS tile
constexpr int RP_WAVES = 4;      // rows of a per workgroup, one per wave
constexpr int GATHER_ROWS = 512; // row indices per launch of trainset_gather_kernel (2 KB of kernel arguments)
constexpr int GATHER_V4 = 32 * 60 / 4;   // float4 per (32,60) row

struct RadiusTest {
    float radius;
    float lo;        // d2 <  lo: d < radius whatever the rounding of the root
    float hi;        // d2 >= hi: d >= radius whatever the rounding of the root
};

// With r2 = radius^2 in f64: lo = fl(r2 (1 - 1e-6)) <= r2 (1 - 9e-7), so d2 < lo has sqrt(d2) < radius (1 - 4e-7), below the f32
// neighbour of radius (radius (1 - 1.2e-7) at most), and rounding is monotone: the rounded root is < radius.  hi = fl(r2 (1 + 1e-6))
// >= r2 (1 + 9e-7) likewise gives a rounded root >= radius.  Where r2 leaves the normal f32 range the bounds are switched off
// (lo = -1: no sum is below it; hi = +inf: an infinite sum has an infinite root, never < radius) and every sum takes the exact path.
static RadiusTest radius_test(float radius) {
    RadiusTest t{radius, -1.f, std::numeric_limits<float>::infinity()};
    if (radius > 1e-15f && radius < 1e15f) {
        const double r2 = (double)radius * (double)radius;
        t.lo = (float)(r2 * (1.0 - 1e-6));
        t.hi = (float)(r2 * (1.0 + 1e-6));
    }
    return t;
}

// the contract of yoho_radius_pairs, used by the count and the fill pass alike
__device__ __forceinline__ bool radius_pred(float ax, float ay, float az, float bx, float by, float bz, const RadiusTest& t) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    if (d2 < t.lo) return true;
    if (d2 >= t.hi) return false;
    return (float)sqrt((double)d2) < t.radius;          // NaN: false
}

// FILL = false: rowcount[i] = pairs of row i.  FILL = true: row i's pairs to pairs[rowoff[i] ...], positions >= capacity dropped.
template <bool FILL>
__global__ __launch_bounds__(64 * RP_WAVES) void radius_kernel(const float* __restrict__ a, int Na, const float* __restrict__ b, int Nb, RadiusTest t,
                                                                int* __restrict__ rowcount, const int64_t* __restrict__ rowoff,
                                                                int64_t* __restrict__ pairs, int64_t capacity) {
    __shared__ float tile[3 * RP_TILE];
    const int lane = threadIdx.x & 63, row = blockIdx.x * RP_WAVES + (threadIdx.x >> 6);
    bool live = row < Na;                                // wave-uniform
    int64_t base = 0;
    if (FILL) {
        if (live) {
            base = rowoff[row];
            live = rowcount[row] != 0 && base < capacity;
        }
        if (!__syncthreads_or(live)) return;             // no row of this workgroup has a pair to write
    }
    const size_t ra = live ? (size_t)row * 3 : 0;
    const float ax = a[ra], ay = a[ra + 1], az = a[ra + 2];
    int cnt = 0;
    for (int t0 = 0; t0 < Nb; t0 += RP_TILE) {
        const int nt = Nb - t0 < RP_TILE ? Nb - t0 : RP_TILE;
        __syncthreads();
        for (int f = threadIdx.x; f < nt * 3; f += 64 * RP_WAVES) {
            const int p = f / 3;
            tile[(f - 3 * p) * RP_TILE + p] = b[(size_t)t0 * 3 + f];
        }
        __syncthreads();
        if (!live) continue;
        for (int j0 = 0; j0 < nt; j0 += 64) {
            const int j = j0 + lane;                     // < RP_TILE: j0 is a multiple of 64 below nt <= RP_TILE
            const bool hit = j < nt && radius_pred(ax, ay, az, tile[j], tile[RP_TILE + j], tile[2 * RP_TILE + j], t);
            if (FILL) {
                const unsigned long long mask = __ballot(hit);
                if (hit) {
                    const int64_t pos = base + __popcll(mask & ((1ull << lane) - 1ull));
                    if (pos < capacity) {
                        pairs[2 * pos] = row;
                        pairs[2 * pos + 1] = t0 + j;
                    }
                }
                base += __popcll(mask);
            } else {
                cnt += hit ? 1 : 0;
            }
        }
        if (FILL && base >= capacity) live = false;      // the rest of the row lies beyond the buffer
    }
    if (!FILL) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        if (lane == 0 && row < Na) rowcount[row] = cnt;
    }
}

// rowoff = exclusive scan of rowcount in 64 bits, *count = the total.  One workgroup: thread t sums rows [t per, (t + 1) per), the
// 1024 partial sums are scanned in LDS, the thread walks its rows again.
__global__ __launch_bounds__(1024) void radius_scan_kernel(const int* __restrict__ rowcount, int Na, int64_t* __restrict__ rowoff, int64_t* __restrict__ count) {
    __shared__ int64_t part[1024];
    const int tid = threadIdx.x, per = (Na + 1023) / 1024;
    const int lo = tid * per < Na ? tid * per : Na, hi = lo + per < Na ? lo + per : Na;
    int64_t s = 0;
    for (int i = lo; i < hi; ++i) s += rowcount[i];
    part[tid] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int64_t v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int64_t run = part[tid] - s;
    for (int i = lo; i < hi; ++i) { rowoff[i] = run; run += rowcount[i]; }
    if (tid == 1023) *count = part[1023];
}

struct GatherRows { int row[GATHER_ROWS]; };      // row[b] = rot[b] * kn + key[b]

// out row blockIdx.x = feats row g.row[blockIdx.x]: 480 16-byte loads / stores
__global__ __launch_bounds__(256) void trainset_gather_kernel(const float4* __restrict__ feats, GatherRows g, float4* __restrict__ out) {
    const float4* src = feats + (size_t)g.row[blockIdx.x] * GATHER_V4;
    float4* dst = out + (size_t)blockIdx.x * GATHER_V4;
    for (int v = threadIdx.x; v < GATHER_V4; v += 256) dst[v] = src[v];
}

}  // namespace yoho

using namespace yoho;

extern "C" {

int yoho_radius_pairs(yoho_ctx* c, const float* a, int Na, const float* b, int Nb, float radius, int64_t* pairs, int64_t capacity, int64_t* count,
                      void* stream) {
    if (!c || !count || Na < 0 || Nb < 0) {
        set_error("yoho_radius_pairs: bad argument (ctx %p, count %p, Na=%d, Nb=%d)", (void*)c, (void*)count, Na, Nb);
        return YOHO_EINVAL;
    }
    if (Na > YOHO_RADIUS_MAX_POINTS || Nb > YOHO_RADIUS_MAX_POINTS) {
        set_error("yoho_radius_pairs: Na=%d, Nb=%d must not exceed YOHO_RADIUS_MAX_POINTS = %d", Na, Nb, YOHO_RADIUS_MAX_POINTS);
        return YOHO_EINVAL;
    }
    if (std::isnan(radius)) { set_error("yoho_radius_pairs: radius is NaN"); return YOHO_EINVAL; }
    if (capacity < 0 || (!pairs && capacity > 0)) {
        set_error("yoho_radius_pairs: capacity=%lld with pairs %p (pairs may be NULL with capacity = 0 only)", (long long)capacity, (void*)pairs);
        return YOHO_EINVAL;
    }
    const bool empty = Na == 0 || Nb == 0 || !(radius > 0.f);
    if (!empty && (!a || !b)) { set_error("yoho_radius_pairs: bad argument (a required pointer is NULL)"); return YOHO_EINVAL; }
    YOHO_NEED_ALIGNED("yoho_radius_pairs", 3, a, b);
    YOHO_NEED_ALIGNED("yoho_radius_pairs", 7, pairs, count);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (empty) {
        HIPCHK(hipMemsetAsync(count, 0, sizeof(int64_t), s));
        return 0;
    }
    int rc;
    int64_t* rowoff = nullptr;
    int* rowcount = nullptr;
    if ((rc = bind_ws(c, s, [&](Arena& ar) { rowoff = ar.take<int64_t>((size_t)Na); rowcount = ar.take<int>((size_t)Na); }))) return rc;
    const RadiusTest t = radius_test(radius);
    const dim3 grid((Na + RP_WAVES - 1) / RP_WAVES), block(64 * RP_WAVES);
    hipLaunchKernelGGL((radius_kernel<false>), grid, block, 0, s, a, Na, b, Nb, t, rowcount, (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(radius_scan_kernel, dim3(1), dim3(1024), 0, s, (const int*)rowcount, Na, rowoff, count);
    HIPCHK(hipGetLastError());
    if (capacity > 0) {
        hipLaunchKernelGGL((radius_kernel<true>), grid, block, 0, s, a, Na, b, Nb, t, rowcount, (const int64_t*)rowoff, pairs, capacity);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

int yoho_trainset_gather(yoho_ctx* c, const float* feats, int nr, int kn, const int64_t* rot_host, const int64_t* key_host, int B, float* out,
                         void* stream) {
    if (!c || nr < 0 || kn < 0 || B < 0) {
        set_error("yoho_trainset_gather: bad argument (ctx %p, nr=%d, kn=%d, B=%d)", (void*)c, nr, kn, B);
        return YOHO_EINVAL;
    }
    if (B == 0) return 0;
    if (!feats || !rot_host || !key_host || !out) { set_error("yoho_trainset_gather: bad argument (a required pointer is NULL)"); return YOHO_EINVAL; }
    if ((int64_t)nr * kn > 0x7FFFFFFFll) { set_error("yoho_trainset_gather: nr=%d x kn=%d rows exceed 2^31 - 1", nr, kn); return YOHO_EINVAL; }
    YOHO_NEED_ALIGNED("yoho_trainset_gather", 15, feats, out);
    for (int i = 0; i < B; ++i) {
        if (rot_host[i] < 0 || rot_host[i] >= nr) {
            set_error("yoho_trainset_gather: rot[%d]=%lld is outside [0, nr=%d)", i, (long long)rot_host[i], nr);
            return YOHO_EINVAL;
        }
        if (key_host[i] < 0 || key_host[i] >= kn) {
            set_error("yoho_trainset_gather: key[%d]=%lld is outside [0, kn=%d)", i, (long long)key_host[i], kn);
            return YOHO_EINVAL;
        }
    }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    for (int b0 = 0; b0 < B; b0 += GATHER_ROWS) {
        const int nb = B - b0 < GATHER_ROWS ? B - b0 : GATHER_ROWS;
        GatherRows g;
        for (int i = 0; i < nb; ++i) g.row[i] = (int)(rot_host[b0 + i] * kn + key_host[b0 + i]);
        for (int i = nb; i < GATHER_ROWS; ++i) g.row[i] = 0;
        hipLaunchKernelGGL(trainset_gather_kernel, dim3(nb), dim3(256), 0, s, reinterpret_cast<const float4*>(feats), g,
                           reinterpret_cast<float4*>(out) + (size_t)b0 * GATHER_V4);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
