// Exact farthest-point sampling (include/yoho_keypoints.h).  Compiled with -ffp-contract=off like knn.hip
// (yoho_amd/build.py): the squared distance is dist2_f32<3> of nnmath.h, yoho_nn_search's D = 3 arithmetic.
//
//   fps_one_wg_kernel<P>   one 1024-thread workgroup, all k picks in one launch; thread t owns the points j * 1024 + t, j < P, their
//                          coordinates and running minima in 4 P registers (P = 16 at YOHO_FPS_ONE_WG_MAX: 64 of the 128 a thread of
//                          a 16-wave workgroup may hold); the smallest P in {1, 2, 4, 8, 16} that covers m is launched
//   fps_pick_kernel        grid ceil(m / YOHO_FPS_BLOCK_POINTS), one launch per pick: every workgroup reduces the previous launch's
//                          partial maxima to the new centre, updates the running minima of its own points and writes its own partial
//
// THE KEY.  A candidate is the 64-bit word (ord(r) << 32) | ~i: ord maps a float to an unsigned that orders like the float (r >= 0
// sets the sign bit, r < 0 flips every bit), so that one unsigned max is "largest running minimum, lowest index among equals" in a
// thread's own points, inside a wave, across waves and across workgroups alike, and the picked points' -1 sits below every real
// value.  A slot behind m is key 0, below every point.  The running minimum is updated as `d < r ? d : r`: a NaN distance leaves it
// alone, so it is never NaN, every key is ordered, and with k <= m an unpicked point (r >= 0) is always there to beat the picked.
//
// ONE WORKGROUP.  Per pick: each thread updates its P points against the centre and keeps its best (value, index, coordinates) in
// a float compare (ascending j is ascending index: a strict > keeps the lowest); a __shfl_xor butterfly takes the wave's maximum
// key; the lane that holds it writes the key and ITS point's coordinates into the wave's slot of LDS; one __syncthreads; every thread
// reads the 16 slots, takes their maximum and the coordinates beside it - the next centre, without a load from memory on the chain.
// The slots are double-buffered by pick parity, so that the one barrier suffices: a wave can write pick s + 2's slot only behind
// the barrier of pick s + 1, which every wave joins after its reads of pick s.
//
// ONE LAUNCH PER PICK.  Launch s reduces partial[(s - 1) & 1][0 .. nb) - every workgroup redundantly, 24 nb bytes from L2 -, so the
// centre is known to all of them without one workgroup waiting for another: the kernel boundary is the grid's only
// synchronisation.  A partial is the block's maximum key WITH its point's coordinates, so the centre needs no further load.  The
// launch then writes partial[s & 1][its block]: the other parity, because a workgroup may still be reading the previous partials.
// Launch 0 takes `start` and reads no running minimum (they are +inf), so every workspace byte is written before it is read.  The
// last pick needs no update: a tail launch of one workgroup reduces the last partials.  Workgroup 0 writes idx / dist2.
#include "common.h"
#include "nnmath.h"
#include "yoho_keypoints.h"
#include <cmath>

namespace yoho {

typedef unsigned long long fps_key;

constexpr int FPS_WG1 = 1024;                        // threads of the one-workgroup path
constexpr int FPS_WAVES1 = FPS_WG1 / 64;
constexpr int FPS_PMAX = YOHO_FPS_ONE_WG_MAX / FPS_WG1;
constexpr int FPS_WG2 = 256;                         // threads of a per-pick workgroup
constexpr int FPS_PP = YOHO_FPS_BLOCK_POINTS / FPS_WG2;
static_assert(FPS_PMAX * FPS_WG1 == YOHO_FPS_ONE_WG_MAX && FPS_PMAX == 16, "fps_one_wg_kernel is instantiated up to 16 points per thread");
static_assert(FPS_PP * FPS_WG2 == YOHO_FPS_BLOCK_POINTS, "a per-pick workgroup owns a whole number of points per thread");

__device__ __forceinline__ unsigned fps_ord(float r) {
    const unsigned b = __float_as_uint(r);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float fps_unord(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }
__device__ __forceinline__ fps_key fps_make(float r, unsigned i) { return ((fps_key)fps_ord(r) << 32) | (fps_key)(~i); }
__device__ __forceinline__ unsigned fps_index(fps_key k) { return ~(unsigned)k; }
__device__ __forceinline__ float fps_value(fps_key k) { return fps_unord((unsigned)(k >> 32)); }
__device__ __forceinline__ fps_key fps_max(fps_key a, fps_key b) { return a > b ? a : b; }

__device__ __forceinline__ fps_key fps_wave_max(fps_key v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fps_max(v, (fps_key)__shfl_xor((unsigned long long)v, o));
    return v;
}

__device__ __forceinline__ float fps_dist2(float px, float py, float pz, float cx, float cy, float cz) {
    const float a[3] = {px, py, pz}, b[3] = {cx, cy, cz};
    return dist2_f32<3>(a, b);
}

struct FpsSlot {
    fps_key key;
    float x, y, z, pad;
};

template <int P>
__global__ __launch_bounds__(FPS_WG1) void fps_one_wg_kernel(const float* __restrict__ pts, int m, int k, int start, int64_t* __restrict__ idx,
                                                              float* __restrict__ dist2) {
    __shared__ FpsSlot slot[2][FPS_WAVES1];
    const int t = threadIdx.x, wave = t >> 6;
    float x[P], y[P], z[P], r[P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int i = j * FPS_WG1 + t;
        const bool in = i < m;
        x[j] = in ? pts[3 * (size_t)i] : 0.f;
        y[j] = in ? pts[3 * (size_t)i + 1] : 0.f;
        z[j] = in ? pts[3 * (size_t)i + 2] : 0.f;
        r[j] = in ? INFINITY : -2.f;                 // a slot behind m: below the picked points' -1, and no distance lowers it further
    }
    unsigned c = (unsigned)start;
    float cx = pts[3 * (size_t)c], cy = pts[3 * (size_t)c + 1], cz = pts[3 * (size_t)c + 2];
    if (t == 0) {
        idx[0] = start;
        if (dist2) dist2[0] = INFINITY;
    }
    for (int s = 1; s < k; ++s) {
        float br = -3.f, bx = 0.f, by = 0.f, bz = 0.f;
        unsigned bi = 0;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const unsigned i = (unsigned)(j * FPS_WG1 + t);
            const float d = fps_dist2(x[j], y[j], z[j], cx, cy, cz);
            float v = d < r[j] ? d : r[j];
            v = i == c ? -1.f : v;
            r[j] = v;
            const bool up = v > br;
            br = up ? v : br; bi = up ? i : bi; bx = up ? x[j] : bx; by = up ? y[j] : by; bz = up ? z[j] : bz;
        }
        const fps_key mine = fps_make(br, bi);
        const fps_key top = fps_wave_max(mine);
        FpsSlot* sl = slot[s & 1];
        if (mine == top) {                           // one lane: the indices of a wave's lanes differ
            sl[wave].key = top; sl[wave].x = bx; sl[wave].y = by; sl[wave].z = bz;
        }
        __syncthreads();
        fps_key best = sl[0].key;
        int w = 0;
#pragma unroll
        for (int q = 1; q < FPS_WAVES1; ++q) {
            const fps_key kq = sl[q].key;
            const bool up = kq > best;
            best = up ? kq : best; w = up ? q : w;
        }
        c = fps_index(best);
        cx = sl[w].x; cy = sl[w].y; cz = sl[w].z;
        if (t == 0) {
            idx[s] = (int64_t)c;
            if (dist2) dist2[s] = fps_value(best);
        }
    }
}

// the maximum of a workgroup's keys and the coordinates that travel with it, in every thread: the first lane that holds the wave's
// maximum writes the wave's slot (`ws`, FPS_WG2 / 64 of them), every thread reads them all
__device__ __forceinline__ void fps_block_max(fps_key& v, float& x, float& y, float& z, FpsSlot* ws) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const fps_key top = fps_wave_max(v);
    if (lane == __ffsll((unsigned long long)__ballot(v == top)) - 1) {
        ws[wave].key = v; ws[wave].x = x; ws[wave].y = y; ws[wave].z = z;
    }
    __syncthreads();
    int w = 0;
    v = ws[0].key;
#pragma unroll
    for (int q = 1; q < FPS_WG2 / 64; ++q) {
        const fps_key kq = ws[q].key;
        const bool up = kq > v;
        v = up ? kq : v; w = up ? q : w;
    }
    x = ws[w].x; y = ws[w].y; z = ws[w].z;
}

// pick s: update = 1, grid nb - the centre from the previous partials (s = 0: `start`), this block's minima and partial;
//         update = 0, grid 1 - the tail: the centre alone
// A partial carries its point's coordinates beside the key, and a block's own points and minima are loaded before the partials are
// reduced: the launch has two dependent trips to memory (partials, then the stores), not four.
__global__ __launch_bounds__(FPS_WG2) void fps_pick_kernel(const float* __restrict__ pts, int m, int s, int start, int nb, const FpsSlot* __restrict__ prev,
                                                            FpsSlot* __restrict__ cur, float* __restrict__ rmin, int64_t* __restrict__ idx,
                                                            float* __restrict__ dist2, int update) {
    __shared__ FpsSlot ws[2][FPS_WG2 / 64];
    const int t = threadIdx.x;
    float px[FPS_PP], py[FPS_PP], pz[FPS_PP], old[FPS_PP];
    if (update) {
#pragma unroll
        for (int j = 0; j < FPS_PP; ++j) {
            const unsigned i = (unsigned)blockIdx.x * YOHO_FPS_BLOCK_POINTS + (unsigned)(j * FPS_WG2 + t);
            const bool in = i < (unsigned)m;
            px[j] = in ? pts[3 * (size_t)i] : 0.f;
            py[j] = in ? pts[3 * (size_t)i + 1] : 0.f;
            pz[j] = in ? pts[3 * (size_t)i + 2] : 0.f;
            old[j] = (in && s > 0) ? rmin[i] : INFINITY;
        }
    }
    unsigned c = (unsigned)start;
    float val = INFINITY, cx, cy, cz;
    if (s > 0) {
        fps_key v = 0;
        cx = cy = cz = 0.f;
        for (int j = t; j < nb; j += FPS_WG2) {
            const FpsSlot q = prev[j];
            const bool up = q.key > v;
            v = up ? q.key : v; cx = up ? q.x : cx; cy = up ? q.y : cy; cz = up ? q.z : cz;
        }
        fps_block_max(v, cx, cy, cz, ws[0]);
        c = fps_index(v);
        val = fps_value(v);
    } else {
        cx = pts[3 * (size_t)c]; cy = pts[3 * (size_t)c + 1]; cz = pts[3 * (size_t)c + 2];
    }
    if (blockIdx.x == 0 && t == 0) {
        idx[s] = (int64_t)c;
        if (dist2) dist2[s] = val;
    }
    if (!update) return;
    fps_key best = 0;
    float bx = 0.f, by = 0.f, bz = 0.f;
#pragma unroll
    for (int j = 0; j < FPS_PP; ++j) {
        const unsigned i = (unsigned)blockIdx.x * YOHO_FPS_BLOCK_POINTS + (unsigned)(j * FPS_WG2 + t);
        if (i < (unsigned)m) {
            const float d = fps_dist2(px[j], py[j], pz[j], cx, cy, cz);
            float v = d < old[j] ? d : old[j];
            v = i == c ? -1.f : v;
            rmin[i] = v;
            const fps_key kv = fps_make(v, i);
            const bool up = kv > best;
            best = up ? kv : best; bx = up ? px[j] : bx; by = up ? py[j] : by; bz = up ? pz[j] : bz;
        }
    }
    fps_block_max(best, bx, by, bz, ws[1]);
    if (t == 0) {
        FpsSlot o;
        o.key = best; o.x = bx; o.y = by; o.z = bz; o.pad = 0.f;
        cur[blockIdx.x] = o;
    }
}

template <int P>
static void fps_launch_one(hipStream_t s, const float* pts, int m, int k, int start, int64_t* idx, float* dist2) {
    hipLaunchKernelGGL(fps_one_wg_kernel<P>, dim3(1), dim3(FPS_WG1), 0, s, pts, m, k, start, idx, dist2);
}

}  // namespace yoho

using namespace yoho;

extern "C" {

int yoho_fps(yoho_ctx* c, const float* pts, int m, int k, int start, int path, int64_t* idx, float* dist2, void* stream) {
    if (!c || !pts || !idx) { set_error("yoho_fps: bad argument (ctx %p, pts %p, idx %p: a required pointer is NULL)", (void*)c, (const void*)pts, (void*)idx); return YOHO_EINVAL; }
    if (m < 0 || m > YOHO_FPS_MAX_POINTS) { set_error("yoho_fps: m=%d must be in [0, YOHO_FPS_MAX_POINTS = %d]", m, YOHO_FPS_MAX_POINTS); return YOHO_EINVAL; }
    if (k < 0 || k > m) { set_error("yoho_fps: k=%d must be in [0, m = %d]", k, m); return YOHO_EINVAL; }
    if (k > 0 && (start < 0 || start >= m)) { set_error("yoho_fps: start=%d must be in [0, m = %d)", start, m); return YOHO_EINVAL; }
    if (path != YOHO_FPS_AUTO && path != YOHO_FPS_ONE_WG && path != YOHO_FPS_PER_PICK) { set_error("yoho_fps: unknown path=%d", path); return YOHO_EINVAL; }
    if (path == YOHO_FPS_ONE_WG && m > YOHO_FPS_ONE_WG_MAX) {
        set_error("yoho_fps: YOHO_FPS_ONE_WG takes m <= YOHO_FPS_ONE_WG_MAX = %d, m=%d", YOHO_FPS_ONE_WG_MAX, m);
        return YOHO_EINVAL;
    }
    YOHO_NEED_ALIGNED("yoho_fps", 3, pts, dist2);
    YOHO_NEED_ALIGNED("yoho_fps", 7, idx);
    if (k == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (path == YOHO_FPS_AUTO) path = m <= YOHO_FPS_ONE_WG_MAX ? YOHO_FPS_ONE_WG : YOHO_FPS_PER_PICK;
    if (path == YOHO_FPS_ONE_WG) {
        const int per = (m + FPS_WG1 - 1) / FPS_WG1;
        if (per <= 1) fps_launch_one<1>(s, pts, m, k, start, idx, dist2);
        else if (per <= 2) fps_launch_one<2>(s, pts, m, k, start, idx, dist2);
        else if (per <= 4) fps_launch_one<4>(s, pts, m, k, start, idx, dist2);
        else if (per <= 8) fps_launch_one<8>(s, pts, m, k, start, idx, dist2);
        else fps_launch_one<16>(s, pts, m, k, start, idx, dist2);
        HIPCHK(hipGetLastError());
        return 0;
    }
    const int nb = (m + YOHO_FPS_BLOCK_POINTS - 1) / YOHO_FPS_BLOCK_POINTS;
    float* rmin = nullptr;
    FpsSlot* part = nullptr;
    int rc;
    if ((rc = bind_ws(c, s, [&](Arena& ar) {
            part = ar.take<FpsSlot>((size_t)2 * nb);
            rmin = ar.take<float>((size_t)m);
        }))) return rc;
    // all k launches are queued at once, as yoho_icp_refine queues its iterations: nothing is read back between them
    for (int p = 0; p + 1 < k; ++p)
        hipLaunchKernelGGL(fps_pick_kernel, dim3(nb), dim3(FPS_WG2), 0, s, pts, m, p, start, nb, (const FpsSlot*)(part + (size_t)((p + 1) & 1) * nb),
                           part + (size_t)(p & 1) * nb, rmin, idx, dist2, 1);
    hipLaunchKernelGGL(fps_pick_kernel, dim3(1), dim3(FPS_WG2), 0, s, pts, m, k - 1, start, nb, (const FpsSlot*)(part + (size_t)(k & 1) * nb),
                       part + (size_t)((k - 1) & 1) * nb, rmin, idx, dist2, 0);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
