// Exact k-nearest-neighbour search (1 <= k <= 16): the k >= 2 branch of the reference's matcher.
//
//   knn_kernel / knn_merge_kernel   modified_knn_matcher.find_knn_gpu   utils/knn_search.py:68-106,155-162
//
// For every source row the k target rows with the smallest pdist, ascending by (fp32 distance as returned, target index).  The
// distance is match.hip's, bit for bit (nnmath.h: dist2_f32 in torch's CPU summation order, 'L2' = sqrt(D2 + 1e-7) correctly
// rounded); this file is compiled with -ffp-contract=off like match.hip (yoho_amd/build.py).
//
// Shape: nn32seg_kernel's, from the same pieces (nntile.h) - a 256-row target tile in LDS, 16 lanes interleaved over the targets of a
// source row, two source rows per thread (a target read from LDS feeds two distances), the targets cut into segments over blockIdx.y
// for large problems (nn_segment_plan) - with the 16 lanes of a row ADJACENT in the wave (row group = threadIdx.x / 16, interleave =
// threadIdx.x % 16; the tile's rows are padded to 36 floats so that the 16 different rows one ds_read_b128 fetches fall into 16
// different bank quads).
//
// The selection.  A sorted list of k keys per THREAD was considered and dropped on paper: a thread that has seen t of its targets
// still inserts with probability k / t, a wave holds 128 (thread, row) lists, and one inserting lane makes the whole wave run the
// insertion - with 128 k / t >= 1 for every t a segment reaches (t <= 45 at 5000 x 5000), the wave would run it at every step.
// Here the 16 lanes of a row hold ONE sorted list between them: lane j keeps the j-th smallest key
//     key = nn_key(bits of the fp32 distance as returned, target index)          (distances >= +0: integer order = float order)
// so the list is always a top-16, whatever k is (no k buckets, one 64-bit register per row, nothing indexed dynamically: no scratch),
// and a row inserts ~ k (1 + ln(N / k)) times per segment IN ALL.  A step computes 16 distances of the row; the lanes whose sum is
// below the row's threshold T form their exact key, and the pending keys go in one by one: broadcast from the lowest pending lane,
// compare (c_j = key < e_j, monotone in j), shift through a one-lane shuffle:  e_j <- c_j ? (c_{j-1} ? e_{j-1} : key) : e_j.
// Insertions use exact keys only, so the list does not depend on the order in which keys arrive; T only has to let every key
// through that belongs into the top k:
//   * every target of an earlier step has a lower index than the candidates of this one, so a candidate enters only with a distance
//     STRICTLY below r = the k-th key's distance (T = "everything" while the row holds fewer than k keys);
//   * SquareL2: T = r.   L2: the candidate's fp32 sum s = fl(D2 + 1e-7) is compared, the f64 square root is taken only below T.
//     sqrt and its rounding are monotone, and s >= T = fl(fl(r r)(1 + 1e-6)) >= r^2 (1 + 8e-7) gives sqrt(s) >= r (1 + 3e-7) > r,
//     i.e. a rounded distance >= r: rejected rightly.  The test is on the SUM, so it holds at every magnitude - D2 = 1e-15 and
//     2e-15 both give s = 1e-7f, equal distance bits, a tie that the index decides (a relative test on D2 would call them clearly
//     different; nn32seg_kernel had one and now decides on the sums too: nn_closer, nnmath.h).  Sums in the band
//     [r^2, T) pay a square root for nothing; that is all.
//   * NaN sums are folded to the one quiet NaN 0x7FC00000 (above +inf in integer order: NaN sorts last), so the keys stay totally
//     ordered and a row of NaN / inf still gets k distinct in-range indices.
// A segment's 16 lanes write its k keys to the workspace [Ns][nseg][k]; knn_merge_kernel (16 lanes per row, the same insertion)
// writes idx / dist.  Keys are exact, so the result cannot depend on the segment count; with one segment the search kernel writes
// idx / dist itself.  No atomics.
#include "common.h"
#include "nntile.h"
#include "yoho_knn.h"

namespace yoho {

constexpr int KNN_G = NN_SPLIT;  // lanes per source row = length of the distributed list
constexpr int KNN_ROWS = 32;     // source rows per workgroup: 16 row groups x 2 rows per thread
static_assert(YOHO_KNN_MAX == KNN_G, "the list is one key per lane of a row group");

__device__ __forceinline__ unsigned long long knn_shfl64(unsigned long long v, int src) {
    const unsigned lo = __shfl((unsigned)v, src, KNN_G), hi = __shfl((unsigned)(v >> 32), src, KNN_G);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long knn_shfl_up64(unsigned long long v) {
    const unsigned lo = __shfl_up((unsigned)v, 1, KNN_G), hi = __shfl_up((unsigned)(v >> 32), 1, KNN_G);
    return ((unsigned long long)hi << 32) | lo;
}

// bits of a distance or sum, NaN folded to the one quiet NaN
__device__ __forceinline__ unsigned knn_bits(float x) {
    const unsigned u = __float_as_uint(x);
    return u > 0x7F800000u ? 0x7FC00000u : u;
}

// Insert the pending keys of every row group of the wave into the groups' lists (ent = this lane's entry).  Called by all 64 lanes.
__device__ __forceinline__ void knn_insert(unsigned long long& ent, unsigned long long key, bool pend, int sp, int lane) {
    unsigned mask = (unsigned)(__ballot(pend) >> (lane & 48)) & 0xFFFFu;         // the pending lanes of this lane's group
    while (__any(mask != 0)) {
        unsigned long long cand = knn_shfl64(key, mask ? __ffs(mask) - 1 : 0);
        if (!mask) cand = NN_KEY_EMPTY;                                          // this group is done: EMPTY is below no entry
        const bool c = cand < ent;
        const unsigned long long prev = knn_shfl_up64(ent);
        const int cprev = __shfl_up((int)c, 1, KNN_G);
        if (c) ent = (sp > 0 && cprev) ? prev : cand;
        mask &= mask - 1;
    }
}

// the threshold on a candidate's bits (squared distance, or the sum D2 + 1e-7) below which it may enter a list whose k-th key is kth
template <bool SQUARED>
__device__ __forceinline__ unsigned knn_threshold(unsigned long long ent, int k) {
    const unsigned r = __shfl(__float_as_uint(nn_key_dist(ent)), k - 1, KNN_G);
    if (SQUARED || r >= 0x7F800000u) return r;                                   // inf, NaN, or fewer than k keys so far (0xFFFFFFFF)
    const float rf = __uint_as_float(r);
    return __float_as_uint(__fmul_rn(__fmul_rn(rf, rf), 1.0f + 1e-6f));
}

// src (Ns,D), tgt (Nt,D) -> keys [Ns][gridDim.y][k] (segments) or, keys == nullptr (one segment), idx (Ns,k) int64 / dist (Ns,k) f32
template <int D, bool SQUARED>
__global__ __launch_bounds__(256) void knn_kernel(const float* __restrict__ src, int Ns, const float* __restrict__ tgt, int Nt, int k, int segLen,
                                                  unsigned long long* __restrict__ keys, int64_t* __restrict__ idx, float* __restrict__ dist) {
    constexpr int LD = D % 4 == 0 ? D + 4 : D;       // tile row stride in floats
    __shared__ __attribute__((aligned(16))) float tile[NN_TT * LD];
    const int sp = threadIdx.x % KNN_G, g = threadIdx.x / KNN_G, lane = threadIdx.x & 63;
    const int row0 = blockIdx.x * KNN_ROWS + g, row1 = row0 + KNN_ROWS / 2;
    float a0[D], a1[D];
    nn_load_row<D>(a0, a1, src, row0, row1, Ns);
    unsigned long long e0 = NN_KEY_EMPTY, e1 = NN_KEY_EMPTY;
    unsigned T0 = 0xFFFFFFFFu, T1 = 0xFFFFFFFFu;
    const int tlo = blockIdx.y * segLen;
    const int thi = tlo + segLen < Nt ? tlo + segLen : Nt;
    for (int t0 = tlo; t0 < thi; t0 += NN_TT) {
        const int nt = thi - t0 < NN_TT ? thi - t0 : NN_TT;
        __syncthreads();
        nn_stage_tile<D, LD>(tile, tgt, t0, nt, D % 4 == 0);                 // rows of D floats from a 16-byte aligned base
        __syncthreads();
        for (int tb = 0; tb < nt; tb += KNN_G) {
            const int tl = tb + sp;
            const bool valid = tl < nt;
            float b[D];
            nn_tile_row<D, LD>(b, tile, valid ? tl : 0);
            float d0 = dist2_f32<D>(a0, b), d1 = dist2_f32<D>(a1, b);
            if (!SQUARED) { d0 = __fadd_rn(d0, 1e-7f); d1 = __fadd_rn(d1, 1e-7f); }      // dist_of_f32's sum; its square root below
            const unsigned u0 = knn_bits(d0), u1 = knn_bits(d1);
            const bool p0 = valid && u0 < T0, p1 = valid && u1 < T1;
            if (__any(p0 || p1)) {
                const unsigned ti = (unsigned)(t0 + tl);
                unsigned long long k0 = NN_KEY_EMPTY, k1 = NN_KEY_EMPTY;
                if (p0) k0 = nn_key(SQUARED ? u0 : knn_bits((float)sqrt((double)__uint_as_float(u0))), ti);
                if (p1) k1 = nn_key(SQUARED ? u1 : knn_bits((float)sqrt((double)__uint_as_float(u1))), ti);
                knn_insert(e0, k0, p0, sp, lane);
                knn_insert(e1, k1, p1, sp, lane);
                T0 = knn_threshold<SQUARED>(e0, k);
                T1 = knn_threshold<SQUARED>(e1, k);
            }
        }
    }
    if (sp < k) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = h ? row1 : row0;
            const unsigned long long e = h ? e1 : e0;
            if (row >= Ns) continue;
            if (keys) {
                keys[((size_t)row * gridDim.y + blockIdx.y) * k + sp] = e;
            } else {
                idx[(size_t)row * k + sp] = (int64_t)nn_key_index(e);
                if (dist) dist[(size_t)row * k + sp] = nn_key_dist(e);
            }
        }
    }
}

// keys [Ns][n] (n = segments x k exact keys, EMPTY where a segment had fewer than k targets) -> idx (Ns,k), dist (Ns,k): 16 lanes per row
__global__ __launch_bounds__(256) void knn_merge_kernel(const unsigned long long* __restrict__ keys, int Ns, int n, int k, int64_t* __restrict__ idx,
                                                        float* __restrict__ dist) {
    const int sp = threadIdx.x % KNN_G, g = threadIdx.x / KNN_G, lane = threadIdx.x & 63;
    const int row = blockIdx.x * (256 / KNN_G) + g;
    const unsigned long long* p = keys + (size_t)(row < Ns ? row : Ns - 1) * n;
    unsigned long long e = NN_KEY_EMPTY, kth = NN_KEY_EMPTY;
    for (int tb = 0; tb < n; tb += KNN_G) {
        const unsigned long long key = tb + sp < n ? p[tb + sp] : NN_KEY_EMPTY;
        const bool pend = key < kth;
        if (__any(pend)) {
            knn_insert(e, key, pend, sp, lane);
            kth = knn_shfl64(e, k - 1);
        }
    }
    if (row < Ns && sp < k) {
        idx[(size_t)row * k + sp] = (int64_t)nn_key_index(e);
        if (dist) dist[(size_t)row * k + sp] = nn_key_dist(e);
    }
}

}  // namespace yoho

using namespace yoho;

extern "C" {

int yoho_knn_search(yoho_ctx* c, const float* src, int Ns, const float* tgt, int Nt, int D, int dist_type, int k, int64_t* idx, float* dist,
                    void* stream) {
    if (!c || Ns < 0 || Nt < 1) { set_error("yoho_knn_search: bad argument (ctx %p, Ns=%d, Nt=%d)", (void*)c, Ns, Nt); return YOHO_EINVAL; }
    if (k < 1 || k > YOHO_KNN_MAX || k > Nt) { set_error("yoho_knn_search: k=%d must be in [1, min(YOHO_KNN_MAX = %d, Nt = %d)]", k, YOHO_KNN_MAX, Nt); return YOHO_EINVAL; }
    if (D != 32 && D != 3) { set_error("yoho_knn_search: D must be 32 or 3 (got %d)", D); return YOHO_EINVAL; }
    const bool sq = dist_type == YOHO_DIST_SQUARE_L2;
    if (dist_type != YOHO_DIST_L2 && !sq) { set_error("yoho_knn_search: unknown dist_type %d", dist_type); return YOHO_EINVAL; }
    if (Ns == 0) return 0;
    if (!src || !tgt || !idx) { set_error("yoho_knn_search: bad argument (a required pointer is NULL)"); return YOHO_EINVAL; }
    YOHO_NEED_ALIGNED("yoho_knn_search", (D == 32 ? 15 : 3), src, tgt);
    YOHO_NEED_ALIGNED("yoho_knn_search", 7, idx);
    YOHO_NEED_ALIGNED("yoho_knn_search", 3, dist);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    // segments of the targets: one below 2^20 pairs (a single launch, as yoho_nn_search's one-row kernel), else a few workgroups per CU
    const NnPlan plan = nn_segment_plan(Ns, Nt, KNN_ROWS, c->nCU, true);
    const int nseg = plan.nseg;
    unsigned long long* keys = nullptr;
    if (nseg > 1) {
        int rc;
        if ((rc = bind_ws(c, s, [&](Arena& ar) { keys = ar.take<unsigned long long>((size_t)Ns * nseg * k); }))) return rc;
    }
    const dim3 grid((Ns + KNN_ROWS - 1) / KNN_ROWS, nseg);
    nn_dispatch(D, sq, [&](auto d, auto q) {           // D was checked above
        hipLaunchKernelGGL((knn_kernel<decltype(d)::value, decltype(q)::value>), grid, dim3(256), 0, s, src, Ns, tgt, Nt, k, plan.segLen, keys, idx, dist);
    });
    HIPCHK(hipGetLastError());
    if (nseg > 1) {
        hipLaunchKernelGGL(knn_merge_kernel, dim3((Ns + 256 / KNN_G - 1) / (256 / KNN_G)), dim3(256), 0, s, keys, Ns, nseg * k, k, idx, dist);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
