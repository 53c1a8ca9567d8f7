// Exact 1-nearest-neighbour in 3-D through a uniform hash grid - the same answers as the brute-force kernels
// (match.hip nn32seg_kernel<3,*>, estim.hip gather_nn_kernel), for callers that know the scale of the cloud:
//
//   60-fold feature transfer   YOHO_testset.py:153-166 (f64, 'L2'), simple_yoho/yoho_extract.py:33-39 (f32, 'SquareL2')
//
// The target cloud there is one point per voxel and every query is a point of the same cloud, so the winner sits within
// a voxel diagonal.  The grid (cell = the hint given to yoho_set_nn_grid; open-addressing table over packed cell
// coordinates, a linked list of points per cell) turns 5000 x n distance evaluations into 5000 x 125 cell probes.
//
// Exactness does not depend on the hint: a wave evaluates, with the brute-force kernels' own arithmetic, every point in
// the 5^3 cells around the query's cell and takes the minimum of (distance, index) - the reference's first minimum.
// Every point outside that block is more than 2 cells away, so the result is final when the winner is closer than
// 2 cells (with a 1e-4 relative slack that dwarfs every rounding involved).  Queries that fail the test (no point
// nearby, hint too small) go to a list and are redone by brute force, one workgroup per query.
//
// Two sets of kernels use the grid: gn_* (one cloud, queries given; yoho_nn_search in 3-D and the f64 group gather) and gt_* (the copies
// of a backbone pass in one launch, copy = blockIdx.y, the query rotated and the feature row written in the kernel).  They differ in
// where the query comes from, which copy's table they address and where the winner goes; the insert (gn_insert), the 125-cell probe
// (gn_probe) and the fallback scan (gn_scan) are written once, on the (distance, index) minimum of nntile.h.
// Compiled with -ffp-contract=off like match.hip / estim.hip.
#include "common.h"
#include "nntile.h"

namespace yoho {

typedef unsigned long long u64;
constexpr u64 GN_EMPTY = ~0ull;
constexpr int GN_CLAMP = (1 << 20) - 1;

__device__ __forceinline__ int gn_cell(double x, double inv_cell) {
    double c = floor(x * inv_cell);                                   // monotone in x: |cell difference| >= 3 => distance > 2 cells
    c = fmin(fmax(c, -(double)GN_CLAMP), (double)GN_CLAMP);           // clamping keeps the map monotone (NaN -> -GN_CLAMP)
    return (int)c;
}
__device__ __forceinline__ int gn_clampi(int c) { return c < -GN_CLAMP ? -GN_CLAMP : (c > GN_CLAMP ? GN_CLAMP : c); }
__device__ __forceinline__ u64 gn_key(int cx, int cy, int cz) {
    return ((u64)(unsigned)(cx + (1 << 20)) << 42) | ((u64)(unsigned)(cy + (1 << 20)) << 21) | (u64)(unsigned)(cz + (1 << 20));
}
__device__ __forceinline__ unsigned gn_slot(u64 key, unsigned mask) { return (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 33) & mask; }

__global__ void gn_clear_kernel(u64* keys, int* head, unsigned cap, int* ucount) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i < cap) { keys[i] = GN_EMPTY; head[i] = -1; }
    if (i == 0) *ucount = 0;
}

// point i of pts into the table: claim the cell's slot, push i on the cell's list
__device__ __forceinline__ void gn_insert(const float* __restrict__ pts, int i, double inv_cell, u64* keys, int* head, int* next, unsigned mask) {
    const u64 key = gn_key(gn_cell((double)pts[3 * (size_t)i], inv_cell), gn_cell((double)pts[3 * (size_t)i + 1], inv_cell),
                           gn_cell((double)pts[3 * (size_t)i + 2], inv_cell));
    unsigned s = gn_slot(key, mask);
    for (;;) {
        const u64 old = atomicCAS(&keys[s], GN_EMPTY, key);
        if (old == GN_EMPTY || old == key) break;
        s = (s + 1) & mask;
    }
    next[i] = atomicExch(&head[s], i);             // list order is arbitrary; the query takes a (distance, index) minimum
}

__global__ void gn_build_kernel(const float* __restrict__ pts, int n, double inv_cell, u64* keys, int* head, int* next, unsigned mask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    gn_insert(pts, i, inv_cell, keys, head, next, mask);
}

// MODE 0: f32 'SquareL2' (distance = squared), 1: f32 'L2', 2: f64 'L2' on keys rotated by Rg (group gather)
template <int MODE> struct GnMetric;
template <> struct GnMetric<0> {
    typedef float dist_t;
    float q[3];
    __device__ void load(const void* src, int i, const GnMat3&) { const float* s = (const float*)src + 3 * (size_t)i; q[0] = s[0]; q[1] = s[1]; q[2] = s[2]; }
    __device__ double pos(int a) const { return (double)q[a]; }
    __device__ float eval(const float* p) const { return dist2_f32<3>(q, p); }
    __device__ static bool resolved(float d, double lim2) { return (double)d < lim2; }
};
template <> struct GnMetric<1> {
    typedef float dist_t;
    float q[3];
    __device__ void load(const void* src, int i, const GnMat3&) { const float* s = (const float*)src + 3 * (size_t)i; q[0] = s[0]; q[1] = s[1]; q[2] = s[2]; }
    __device__ double pos(int a) const { return (double)q[a]; }
    __device__ float eval(const float* p) const { return dist_of_f32(dist2_f32<3>(q, p)); }
    __device__ static bool resolved(float d, double lim2) { return (double)d * (double)d - 1e-7 < lim2; }
};
template <> struct GnMetric<2> {
    typedef double dist_t;
    double q[3];
    __device__ void load(const void* src, int i, const GnMat3& R) {
        const double* kk = (const double*)src + 3 * (size_t)i;
#pragma unroll
        for (int a = 0; a < 3; ++a) q[a] = rotate_key_f64(kk, R.m + 3 * a);
    }
    __device__ double pos(int a) const { return q[a]; }
    __device__ double eval(const float* p) const { return sqrt(__dadd_rn(dist2_key_f64(q, (double)p[0], (double)p[1], (double)p[2]), 1e-7)); }
    __device__ static bool resolved(double d, double lim2) { return d * d - 1e-7 < lim2; }
};

struct GnArgs {
    const void* src; int Ns;
    const float* tgt; int Nt;
    GnMat3 R;
    double inv_cell, lim2;          // lim2 = (2 cell)^2 (1 - 1e-4)
    const u64* keys; const int* head; const int* next; unsigned mask;
    int64_t* idx; float* dist;      // MODE 0/1 outputs
    double* part_d; int* part_i;    // MODE 2 outputs (one "slice" for gather_merge_kernel)
    int* ulist; int* ucount;
};

template <typename T> __device__ __forceinline__ T gn_inf();
template <> __device__ __forceinline__ float gn_inf<float>() { return __builtin_inff(); }
template <> __device__ __forceinline__ double gn_inf<double>() { return __builtin_inf(); }

template <int MODE>
__device__ __forceinline__ void gn_store(const GnArgs& a, int q, typename GnMetric<MODE>::dist_t d, int i) {
    if (MODE == 2) { a.part_d[q] = (double)d; a.part_i[q] = i; }
    else { a.idx[q] = i; if (a.dist) a.dist[q] = (float)d; }
}

// One wave: the (distance, index) minimum over every point in the 5^3 cells around the query, left in every lane.  bi = 0x7FFFFFFF: no
// point there (or all distances NaN).
template <int MODE>
__device__ __forceinline__ void gn_probe(const GnMetric<MODE>& m, double inv_cell, const u64* keys, const int* head, const int* next, unsigned mask,
                                         const float* tgt, int lane, typename GnMetric<MODE>::dist_t& bd, int& bi) {
    typedef typename GnMetric<MODE>::dist_t D;
    const int cx = gn_cell(m.pos(0), inv_cell), cy = gn_cell(m.pos(1), inv_cell), cz = gn_cell(m.pos(2), inv_cell);
    bd = gn_inf<D>();
    bi = 0x7FFFFFFF;
    for (int c = lane; c < 125; c += 64) {
        const u64 key = gn_key(gn_clampi(cx + c % 5 - 2), gn_clampi(cy + (c / 5) % 5 - 2), gn_clampi(cz + c / 25 - 2));
        unsigned s = gn_slot(key, mask);
        int i = -1;
        for (;;) {
            const u64 k = keys[s];
            if (k == key) { i = head[s]; break; }
            if (k == GN_EMPTY) break;
            s = (s + 1) & mask;
        }
        for (; i >= 0; i = next[i]) nn_take_min(bd, bi, m.eval(tgt + 3 * (size_t)i), i);
    }
    nn_wave_min(bd, bi);
}

// One workgroup: the brute-force (distance, index) minimum over all n points, left in rd[0] / ri[0] (256 entries each, in LDS).  All
// distances NaN (NaN query): index 0, the brute-force kernels' answer.
template <int MODE>
__device__ __forceinline__ void gn_scan(const GnMetric<MODE>& m, const float* tgt, int n, typename GnMetric<MODE>::dist_t* rd, int* ri) {
    typedef typename GnMetric<MODE>::dist_t D;
    D bd = gn_inf<D>();
    int bi = 0x7FFFFFFF;
    for (int i = threadIdx.x; i < n; i += 256) nn_take_min(bd, bi, m.eval(tgt + 3 * (size_t)i), i);
    nn_block_min(rd, ri, bd, bi);
}
__device__ __forceinline__ int gn_scan_index(const int* ri) { return ri[0] == 0x7FFFFFFF ? 0 : ri[0]; }

template <int MODE>
__global__ __launch_bounds__(256) void gn_query_kernel(GnArgs a) {
    typedef typename GnMetric<MODE>::dist_t D;
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= a.Ns) return;                                           // wave-uniform
    GnMetric<MODE> m;
    m.load(a.src, q, a.R);
    D bd;
    int bi;
    gn_probe<MODE>(m, a.inv_cell, a.keys, a.head, a.next, a.mask, a.tgt, lane, bd, bi);
    if (lane == 0) {
        if (bi != 0x7FFFFFFF && GnMetric<MODE>::resolved(bd, a.lim2)) gn_store<MODE>(a, q, bd, bi);
        else a.ulist[atomicAdd(a.ucount, 1)] = q;
    }
}

// brute force for the queries the grid could not settle: one workgroup per query, same arithmetic
template <int MODE>
__global__ __launch_bounds__(256) void gn_fallback_kernel(GnArgs a) {
    typedef typename GnMetric<MODE>::dist_t D;
    __shared__ D rd[256];
    __shared__ int ri[256];
    const int count = *a.ucount;
    for (int u = blockIdx.x; u < count; u += gridDim.x) {
        const int q = a.ulist[u];
        GnMetric<MODE> m;
        m.load(a.src, q, a.R);
        gn_scan<MODE>(m, a.tgt, a.Nt, rd, ri);
        if (threadIdx.x == 0) gn_store<MODE>(a, q, rd[0], gn_scan_index(ri));
    }
}

static unsigned grid_cells(int n) {           // power of two, at least twice the points
    unsigned cap = 1024;
    while (cap < 2u * (unsigned)n) cap <<= 1;
    return cap;
}

void grid_nn_layout(Arena& ar, int Ns, int Nt, GridWs& w) {
    w.cap = grid_cells(Nt);
    w.keys = ar.take<u64>(w.cap);
    w.head = ar.take<int>(w.cap);
    w.next = ar.take<int>((size_t)Nt);
    w.ulist = ar.take<int>((size_t)Ns);
    w.ucount = ar.take<int>(1);
}

template <int MODE>
static void gn_launch_search(const GnArgs& a, int nCU, hipStream_t s) {
    hipLaunchKernelGGL(gn_query_kernel<MODE>, dim3((a.Ns + 3) / 4), dim3(256), 0, s, a);
    hipLaunchKernelGGL(gn_fallback_kernel<MODE>, dim3(nCU > 0 ? nCU : 256), dim3(256), 0, s, a);
}

int launch_grid_nn(int mode, const void* src, int Ns, const GnMat3* R, const float* tgt, int Nt, double cell, const GridWs& w, int64_t* idx, float* dist,
                   double* part_d, int* part_i, int nCU, hipStream_t s) {
    const unsigned cap = w.cap;
    u64* keys = w.keys;
    int *head = w.head, *next = w.next;
    GnArgs a;
    a.ulist = w.ulist; a.ucount = w.ucount;
    a.src = src; a.Ns = Ns; a.tgt = tgt; a.Nt = Nt;
    if (R) a.R = *R; else for (int i = 0; i < 9; ++i) a.R.m[i] = i % 4 == 0 ? 1.0 : 0.0;
    a.inv_cell = 1.0 / cell; a.lim2 = 4.0 * cell * cell * (1.0 - 1e-4);
    a.keys = keys; a.head = head; a.next = next; a.mask = cap - 1;
    a.idx = idx; a.dist = dist; a.part_d = part_d; a.part_i = part_i;
    hipLaunchKernelGGL(gn_clear_kernel, dim3(cap / 256), dim3(256), 0, s, keys, head, cap, a.ucount);
    hipLaunchKernelGGL(gn_build_kernel, dim3((Nt + 255) / 256), dim3(256), 0, s, tgt, Nt, a.inv_cell, keys, head, next, a.mask);
    switch (mode) {
        case 0: gn_launch_search<0>(a, nCU, s); break;
        case 1: gn_launch_search<1>(a, nCU, s); break;
        default: gn_launch_search<2>(a, nCU, s); break;
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- the feature transfer of one backbone pass in four launches (copy = blockIdx.y) -------------------------------------------
// simple_yoho/yoho_extract.py:33-39 per rotated copy b: q = (R_b keypoint).float(), nearest down-sampled point of copy b in fp32
// 'SquareL2', out[k, :, g0 + b] = feat_b[nn].  Per copy that was rotate -> clear -> build -> query -> fallback -> scatter, six
// launches of 5-15 us on 5000 queries: 90 launches per 15-copy pass.  Here the copies share the launches; the query kernel rotates
// its keypoint itself (the rotate kernel's expression: f64 fma chain, then the cast) and writes the feature row as soon as it knows
// the winner.  Same arithmetic, same (distance, index) minimum: the same rows.
constexpr int GT_BATCH = 16;
struct GtBatch {
    const double* pts; const int64_t* kidx; int K, nb;
    double R[GT_BATCH][9];
    const float* ds[GT_BATCH]; const float* feat[GT_BATCH]; int m[GT_BATCH];
    double inv_cell, lim2;
    u64* keys; int* head; unsigned cap;          // copy b: + b * cap
    int* next; int mmax;                         // copy b: + b * mmax
    int* ulist; int* ucount;                     // copy b: ulist + b * K, ucount[b]
    int g0; float* out;
};

__global__ void gt_clear_kernel(u64* keys, int* head, size_t total, int* ucount, int nb) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < total) { keys[i] = GN_EMPTY; head[i] = -1; }
    if (i < (size_t)nb) ucount[i] = 0;
}

__global__ void gt_build_kernel(GtBatch a) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= a.m[b]) return;
    gn_insert(a.ds[b], i, a.inv_cell, a.keys + (size_t)b * a.cap, a.head + (size_t)b * a.cap, a.next + (size_t)b * a.mmax, a.cap - 1);
}

// the rotated keypoint as the rotate kernel (spmaps.hip rotate_sel_kernel / point_of) forms it: f64 fma chain per coordinate, then float
__device__ __forceinline__ void gt_query_point(const GtBatch& a, int b, int k, float (&q)[3]) {
    const size_t r = (size_t)a.kidx[k];
    const double p0 = a.pts[3 * r], p1 = a.pts[3 * r + 1], p2 = a.pts[3 * r + 2];
    const double* R = a.R[b];
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = (float)fma(p2, R[3 * c + 2], fma(p1, R[3 * c + 1], p0 * R[3 * c]));
}

// out[k, :, g] = feat[row, :] by the first 32 threads of the caller's wave / workgroup (group_scatter_kernel's clamp)
__device__ __forceinline__ void gt_scatter(const GtBatch& a, int b, int k, int row, int t) {
    row = row < 0 ? 0 : (row >= a.m[b] ? a.m[b] - 1 : row);
    if (t < F) a.out[((size_t)k * F + t) * G + a.g0 + b] = a.feat[b][(size_t)row * F + t];
}

__global__ __launch_bounds__(256) void gt_query_kernel(GtBatch a) {
    const int lane = threadIdx.x & 63, b = blockIdx.y;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= a.K) return;                                            // wave-uniform
    GnMetric<0> m;
    gt_query_point(a, b, k, m.q);
    float bd;
    int bi;
    gn_probe<0>(m, a.inv_cell, a.keys + (size_t)b * a.cap, a.head + (size_t)b * a.cap, a.next + (size_t)b * a.mmax, a.cap - 1, a.ds[b], lane, bd, bi);
    if (bi != 0x7FFFFFFF && GnMetric<0>::resolved(bd, a.lim2)) gt_scatter(a, b, k, bi, lane);       // every lane holds the winner
    else if (lane == 0) a.ulist[(size_t)b * a.K + atomicAdd(a.ucount + b, 1)] = k;
}

__global__ __launch_bounds__(256) void gt_fallback_kernel(GtBatch a) {
    __shared__ float rd[256];
    __shared__ int ri[256];
    const int b = blockIdx.y;
    const int count = a.ucount[b];
    for (int u = blockIdx.x; u < count; u += gridDim.x) {
        const int k = a.ulist[(size_t)b * a.K + u];
        GnMetric<0> m;
        gt_query_point(a, b, k, m.q);
        gn_scan<0>(m, a.ds[b], a.m[b], rd, ri);
        gt_scatter(a, b, k, gn_scan_index(ri), threadIdx.x);
    }
}

void grid_transfer_layout(Arena& ar, int K, int nb, int mmax, GridWs& w) {
    w.cap = grid_cells(mmax);
    w.keys = ar.take<u64>((size_t)w.cap * nb);
    w.head = ar.take<int>((size_t)w.cap * nb);
    w.next = ar.take<int>((size_t)mmax * nb);
    w.ulist = ar.take<int>((size_t)K * nb);
    w.ucount = ar.take<int>((size_t)nb);
}

// nb <= 64 copies (launched GT_BATCH at a time); w: bound by grid_transfer_layout(K, nb, max m)
int launch_grid_transfer_batch(const double* pts, const int64_t* kidx, int K, const double* R_host, int nb, const float* const* ds,
                               const float* const* feat, const int* m, int g0, float* out, double cell, const GridWs& w, int nCU, hipStream_t s) {
    int mmax = 1;
    for (int b = 0; b < nb; ++b) mmax = m[b] > mmax ? m[b] : mmax;
    const unsigned cap = w.cap;
    u64* keys = w.keys;
    int *head = w.head, *next = w.next, *ulist = w.ulist, *ucount = w.ucount;
    {
        const size_t total = (size_t)cap * nb;
        hipLaunchKernelGGL(gt_clear_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, keys, head, total, ucount, nb);
    }
    for (int b0 = 0; b0 < nb; b0 += GT_BATCH) {
        const int nbc = nb - b0 < GT_BATCH ? nb - b0 : GT_BATCH;
        GtBatch a;
        a.pts = pts; a.kidx = kidx; a.K = K; a.nb = nbc;
        for (int b = 0; b < GT_BATCH; ++b) {
            const int sb = b < nbc ? b0 + b : b0;
            for (int i = 0; i < 9; ++i) a.R[b][i] = R_host[9 * (size_t)sb + i];
            a.ds[b] = ds[sb]; a.feat[b] = feat[sb]; a.m[b] = m[sb];
        }
        a.inv_cell = 1.0 / cell; a.lim2 = 4.0 * cell * cell * (1.0 - 1e-4);
        a.keys = keys + (size_t)b0 * cap; a.head = head + (size_t)b0 * cap; a.cap = cap;
        a.next = next + (size_t)b0 * mmax; a.mmax = mmax;
        a.ulist = ulist + (size_t)b0 * K; a.ucount = ucount + b0;
        a.g0 = g0 + b0; a.out = out;
        hipLaunchKernelGGL(gt_build_kernel, dim3((mmax + 255) / 256, nbc), dim3(256), 0, s, a);
        hipLaunchKernelGGL(gt_query_kernel, dim3((K + 3) / 4, nbc), dim3(256), 0, s, a);
        hipLaunchKernelGGL(gt_fallback_kernel, dim3(nCU > 64 ? 64 : (nCU > 0 ? nCU : 64), nbc), dim3(256), 0, s, a);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace yoho
