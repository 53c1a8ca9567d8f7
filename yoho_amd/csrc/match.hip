// Brute-force nearest neighbour, mutual matching and the coarse-rotation index.
//
//   nn32seg_kernel   modified_knn_matcher.pdist / find_nn_gpu   utils/knn_search.py:17-20,26-66
//   mutual kernels   matcher_dual.match                         tests/matcher.py:37-48
//   des2r_kernel     extractor_dr_index.Batch_Des2R_torch       tests/extractor.py:74-78
//
// The reference takes argmin of sqrt(sum((a-b)^2) + 1e-7) over an explicit difference (not the
// GEMM expansion); indices must be bit-exact, so the arithmetic below is written with explicit
// round-to-nearest intrinsics (no FMA contraction) in the summation order torch's CPU reduction
// uses for a contiguous 32-float row: 8 lane sums over x[l], x[8+l], x[16+l], x[24+l], lanes then
// added 0..7 in sequence (pinned by tests/golden/pdist.npz).  The first minimum wins.
// The tile, the packed key, the segment plan and the (distance, index) minimum are nntile.h's, shared with knn.hip and gridnn.hip.
// This file is compiled with -ffp-contract=off (yoho_amd/build.py).
#include "common.h"
#include "nntile.h"

namespace yoho {

// ---------------------------------------------------------------------------------------------------------------
// One kernel, R source rows per thread (thread -> row r = threadIdx.x % 16 (+ 16 per further row), target lane sp = threadIdx.x / 16):
//   R = 1, below 2^20 pairs: one segment, 16 rows per workgroup, idx / dist stored directly - one launch, no keys;
//   R = 2, large problems: the same arithmetic, blocked for the LDS return path and for load balance.
//   * a thread owns TWO source rows, so every target row read from LDS (8 x ds_read_b128) feeds two distance
//     evaluations (with one row the kernel is bound by the LDS return bandwidth, not by its packed fp32 math);
//   * the targets are cut into segments over blockIdx.y (nn_segment_plan) so that there are a few workgroups per CU whatever Ns
//     is; the per-segment winners meet in a packed key (nn_key) with atomicMin, and nn_unpack_kernel writes idx / dist.
// best holds the squared distance.  For the 'L2' form the reference compares sqrt(D2 + 1e-7) (first minimum): a later
// candidate wins only with a strictly smaller ROUNDED distance, which nn_closer (nnmath.h) decides on the sums D2 + 1e-7 -
// the correctly rounded sqrt (computed in f64) is evaluated only when the two sums are not proven 9e-7 apart.
// ---------------------------------------------------------------------------------------------------------------
// src (Ns,D) f32, tgt (Nt,D) f32 -> R = 2: keys (Ns), initialised by the caller;  R = 1: idx (Ns) int64, dist (Ns) f32 (optional)
template <int D, bool SQUARED, int R>
__global__ __launch_bounds__(256) void nn32seg_kernel(const float* __restrict__ src, int Ns, const float* __restrict__ tgt, int Nt,
                                                      unsigned long long* __restrict__ keys, int segLen, const int* __restrict__ run_if,
                                                      int64_t* __restrict__ idx, float* __restrict__ dist) {
    if constexpr (R == 2) {                          // fallback launch behind the MFMA pre-filter (matchf.hip): only if it declined.  Two rows
        if (run_if && !*run_if) return;              // only: one row runs where a dependent load in front of the kernel's own shows
    }
    __shared__ __attribute__((aligned(16))) float tile[NN_TT * D];
    __shared__ float rd[16 * R * NN_SPLIT];
    __shared__ int ri[16 * R * NN_SPLIT];
    const int r = threadIdx.x % 16, sp = threadIdx.x / 16;
    const int row0 = blockIdx.x * (16 * R) + r;
    float a0[D], a1[D];                              // a1, best1, bi1: the second row of a two-row thread
    if constexpr (R == 2) nn_load_row<D>(a0, a1, src, row0, row0 + 16, Ns);
    else nn_load_row<D>(a0, src, row0, Ns);
    float best0 = __builtin_inff(), best1 = __builtin_inff();
    int bi0 = 0, bi1 = 0;
    const int tlo = blockIdx.y * segLen;
    const int thi = tlo + segLen < Nt ? tlo + segLen : Nt;
    for (int t0 = tlo; t0 < thi; t0 += NN_TT) {
        const int nt = thi - t0 < NN_TT ? thi - t0 : NN_TT;
        __syncthreads();
        // t0 is a multiple of 16 rows.  One row per thread stages with scalar loads: the compiler keeps eight of them in flight where it
        // issues one float4 at a time, and a grid of a few dozen workgroups has nothing to hide that latency behind (profiles/nn_family_refactor.md)
        nn_stage_tile<D, D>(tile, tgt, t0, nt, R == 2 && (nt * D) % 4 == 0);
        __syncthreads();
        for (int t = sp; t < nt; t += NN_SPLIT) {
            float b[D];
            nn_tile_row<D, D>(b, tile, t);
            if constexpr (R == 2) {
                const float d0 = dist2_f32<D>(a0, b), d1 = dist2_f32<D>(a1, b);
                if (nn_closer<SQUARED>(d0, best0)) { best0 = d0; bi0 = t0 + t; }
                if (nn_closer<SQUARED>(d1, best1)) { best1 = d1; bi1 = t0 + t; }
            } else {
                const float d0 = dist2_f32<D>(a0, b);
                if (nn_closer<SQUARED>(d0, best0)) { best0 = d0; bi0 = t0 + t; }
            }
        }
    }
    if (!SQUARED) { best0 = dist_of_f32(best0); best1 = dist_of_f32(best1); }           // (best1 is dead code with one row)
    rd[r * NN_SPLIT + sp] = best0; ri[r * NN_SPLIT + sp] = bi0;
    if constexpr (R == 2) { rd[(r + 16) * NN_SPLIT + sp] = best1; ri[(r + 16) * NN_SPLIT + sp] = bi1; }
    __syncthreads();
    if (threadIdx.x < 16 * R) {
        const int rr = threadIdx.x, row = blockIdx.x * (16 * R) + rr;
        if (row < Ns && tlo < thi) {
            float bd;
            int bi;
            nn_row_winner(rd, ri, rr, bd, bi);
            if constexpr (R == 1) {
                idx[row] = bi;
                if (dist) dist[row] = bd;
            } else {
                atomicMin(keys + row, nn_key(__float_as_uint(bd), (unsigned)bi));
            }
        }
    }
}

__global__ __launch_bounds__(256) void nn_unpack_kernel(const unsigned long long* __restrict__ keys, int Ns, int64_t* __restrict__ idx,
                                                        float* __restrict__ dist) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Ns) return;
    const unsigned long long k = keys[i];
    idx[i] = (int64_t)nn_key_index(k);
    if (dist) dist[i] = nn_key_dist(k);
}

// the one launcher of the brute-force search (arguments: common.h); the callers take the one-row kernel below 2^20 pairs
int launch_nn32seg(const float* src, int Ns, const float* tgt, int Nt, int D, int dist_type, int nCU, unsigned long long* keys, bool init_keys,
                   const int* run_if, int64_t* idx, float* dist, hipStream_t s) {
    const bool sq = dist_type == YOHO_DIST_SQUARE_L2;
    if (dist_type != YOHO_DIST_L2 && !sq) { set_error("yoho_nn_search: unknown dist_type %d", dist_type); return YOHO_EINVAL; }
    if (D != 32 && D != 3) { set_error("yoho_nn_search: D must be 32 or 3 (got %d)", D); return YOHO_EINVAL; }
    const int rows = keys ? 32 : 16;
    const NnPlan plan = keys ? nn_segment_plan(Ns, Nt, rows, nCU, false) : NnPlan{Nt, 1};
    const dim3 grid((Ns + rows - 1) / rows, plan.nseg);
    if (keys && init_keys) HIPCHK(hipMemsetAsync(keys, 0xFF, sizeof(unsigned long long) * (size_t)Ns, s));      // NN_KEY_EMPTY
    nn_dispatch(D, sq, [&](auto d, auto q) {
        if (keys) hipLaunchKernelGGL((nn32seg_kernel<decltype(d)::value, decltype(q)::value, 2>), grid, dim3(256), 0, s, src, Ns, tgt, Nt, keys, plan.segLen, run_if, idx, dist);
        else hipLaunchKernelGGL((nn32seg_kernel<decltype(d)::value, decltype(q)::value, 1>), grid, dim3(256), 0, s, src, Ns, tgt, Nt, keys, plan.segLen, run_if, idx, dist);
    });
    HIPCHK(hipGetLastError());
    return 0;
}

int launch_nn_unpack(const unsigned long long* keys, int Ns, int64_t* idx, float* dist, hipStream_t s) {
    hipLaunchKernelGGL(nn_unpack_kernel, dim3((Ns + 255) / 256), dim3(256), 0, s, keys, Ns, idx, dist);
    HIPCHK(hipGetLastError());
    return 0;
}

// keep i with back[fwd[i]] == i, ascending i (tests/matcher.py:42-47).  Single workgroup scan.
// PACKED: fwd / back hold the packed keys (nn_key) of the segmented search.
template <bool PACKED>
__global__ __launch_bounds__(1024) void mutual_compact_kernel(const int64_t* __restrict__ fwd, const int64_t* __restrict__ back,
                                                              int Na, int64_t* __restrict__ pairs, int* __restrict__ M_out) {
    __shared__ int wsum[16];
    __shared__ int base;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < Na; i0 += 1024) {
        const int i = i0 + tid;
        bool keep = false;
        int64_t j = 0;
        if (i < Na) {
            j = PACKED ? (int64_t)nn_key_index((unsigned long long)fwd[i]) : fwd[i];
            const int64_t bk = PACKED ? (int64_t)nn_key_index((unsigned long long)back[j]) : back[j];
            keep = bk == (int64_t)i;
        }
        const unsigned long long m = __ballot(keep);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wv] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int k = 0; k < wv; ++k) off += wsum[k];
        if (keep) { pairs[2 * (size_t)(off + before)] = i; pairs[2 * (size_t)(off + before) + 1] = j; }
        __syncthreads();
        if (tid == 0) { int t = 0; for (int k = 0; k < 16; ++k) t += wsum[k]; base += t; }
        __syncthreads();
    }
    if (tid == 0) *M_out = base;
}

int launch_mutual_compact(const int64_t* fwd, const int64_t* back, int Na, int64_t* pairs, int* M_out, hipStream_t s, bool packed = false) {
    if (packed) hipLaunchKernelGGL(mutual_compact_kernel<true>, dim3(1), dim3(1024), 0, s, fwd, back, Na, pairs, M_out);
    else hipLaunchKernelGGL(mutual_compact_kernel<false>, dim3(1), dim3(1024), 0, s, fwd, back, Na, pairs, M_out);
    HIPCHK(hipGetLastError());
    return 0;
}

// cor[m, a] = sum_g sum_f d1[m, f, P[a, g]] * d2[m, f, g];  idx[m] = argmax_a (first maximum).
// One wave per match, two waves per workgroup, grid-stride over the matches.  The double sum is a gather of the 60 x 60 Gram
// matrix C = D1^T D2 (contraction over the 32 channels): cor[a] = sum_g C[P[a,g]][g].  C is computed on the fp32 MFMA
// (64 x v_mfma_f32_32x32x2_f32, exact fp32 products, fp32 accumulation).  The operands go from global memory straight into
// registers: lane (g' = lane & 31, half = lane >> 5) of step kk holds channel f = 2 kk + half of group elements g' and g' + 32
// (zero beyond 59), i.e. every load is two 128-byte runs per wave and all 64 of them are in flight at once.  C goes to a
// wave-private LDS tile (row stride 65: the gather's rows are a permutation, so stride 64 would put all lanes on one bank) and
// lane a < 60 adds its 60 entries in the order g = 0..59, the rows P[a][g] read as packed bytes (ctx->dPq, in LDS).
// Optional row indices address the descriptors in place.  (Round 3: the first version staged both descriptors in LDS - 33 KB per
// one-wave workgroup, i.e. one wave per SIMD - and read P with 60 dependent global loads per lane: 170-300 us per 3233 matches.)
typedef float floatx16m __attribute__((ext_vector_type(16)));
constexpr int D2R_C = 65;        // row stride of the Gram matrix
constexpr int D2R_W = 2;         // waves (matches in flight) per workgroup

__global__ __launch_bounds__(64 * D2R_W) void des2r_kernel(const float* __restrict__ e1, const int64_t* __restrict__ i1, const float* __restrict__ e2,
                                                          const int64_t* __restrict__ i2, int istride, const unsigned* __restrict__ Pq, int M,
                                                          int64_t* __restrict__ idx, float* __restrict__ cor) {
    __shared__ float Cls[D2R_W][G * D2R_C];
    __shared__ unsigned Pl[15 * 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < 15 * 64; i += 64 * D2R_W) Pl[i] = Pq[i];
    __syncthreads();
    float* Cl = Cls[w];
    const int li = lane & 31, lk = lane >> 5;
    const bool hi_ok = li + 32 < G;
    for (int m = blockIdx.x * D2R_W + w; m < M; m += gridDim.x * D2R_W) {
        const size_t r1 = i1 ? (size_t)i1[(size_t)m * istride] : (size_t)m, r2 = i2 ? (size_t)i2[(size_t)m * istride] : (size_t)m;
        const float* p1 = e1 + r1 * F * G + lk * G + li;
        const float* p2 = e2 + r2 * F * G + lk * G + li;
        float a0[16], a1[16], b0[16], b1[16];
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            a0[kk] = p1[2 * kk * G];
            b0[kk] = p2[2 * kk * G];
            a1[kk] = hi_ok ? p1[2 * kk * G + 32] : 0.f;
            b1[kk] = hi_ok ? p2[2 * kk * G + 32] : 0.f;
        }
        floatx16m acc[2][2];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[rb][cb][r] = 0.f;
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[kk], b0[kk], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[kk], b1[kk], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[kk], b0[kk], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[kk], b1[kk], acc[1][1], 0, 0, 0);
        }
        // D[row g'][col g]: lane (col = lane & 31, half = lane >> 5), reg r -> row = (r & 3) + 8 (r >> 2) + 4 half
#pragma unroll
        for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = 32 * rb + (r & 3) + 8 * (r >> 2) + 4 * lk;
                    if (row < G && (cb == 0 || hi_ok)) Cl[row * D2R_C + 32 * cb + li] = acc[rb][cb][r];
                }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        float sum = 0.f;
#pragma unroll
        for (int q = 0; q < 15; ++q) {
            const unsigned pw = Pl[q * 64 + lane];
#pragma unroll
            for (int j = 0; j < 4; ++j) sum += Cl[((pw >> (8 * j)) & 255u) * D2R_C + 4 * q + j];
        }
        if (cor && lane < G) cor[(size_t)m * G + lane] = sum;
        float bv = lane < G ? sum : -__builtin_inff();
        int bi = lane;
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) idx[m] = bi;
        __builtin_amdgcn_wave_barrier();             // the next match's tile overwrites Cl
    }
}

int launch_des2r(const float* e1, const int64_t* i1, const float* e2, const int64_t* i2, int istride, const unsigned* Pq, int M, int64_t* idx,
                 float* cor, hipStream_t s) {
    if (M <= 0) return 0;
    static const int ncu = [] { int d = 0, n = 256; (void)hipGetDevice(&d); (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d); return n; }();
    const int nwg = std::min((M + D2R_W - 1) / D2R_W, 4 * ncu);          // 35 KB of LDS per workgroup: four per CU
    hipLaunchKernelGGL(des2r_kernel, dim3(nwg), dim3(64 * D2R_W), 0, s, e1, i1, e2, i2, istride, Pq, M, idx, cor);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace yoho

using namespace yoho;

extern "C" {

int yoho_nn_search(yoho_ctx* c, const float* src, int Ns, const float* tgt, int Nt, int D, int dist_type, int64_t* idx, float* dist,
                   void* stream) {
    if (!c || !src || !tgt || !idx || Ns < 0 || Nt < 1) { set_error("yoho_nn_search: bad argument"); return YOHO_EINVAL; }
    if (Ns == 0) return 0;
    YOHO_NEED_ALIGNED("yoho_nn_search", (D == 32 ? 15 : 3), src, tgt);
    YOHO_NEED_ALIGNED("yoho_nn_search", 7, idx);
    YOHO_NEED_ALIGNED("yoho_nn_search", 3, dist);
    HIPCHK(hipSetDevice(c->device));
    if (D == 3 && c->nn_cell > 0.0 && (size_t)Ns * Nt >= (1u << 20) && (dist_type == YOHO_DIST_L2 || dist_type == YOHO_DIST_SQUARE_L2)) {
        int rc;
        GridWs w;
        if ((rc = bind_ws(c, (hipStream_t)stream, [&](Arena& ar) { grid_nn_layout(ar, Ns, Nt, w); }))) return rc;
        return launch_grid_nn(dist_type == YOHO_DIST_SQUARE_L2 ? 0 : 1, src, Ns, nullptr, tgt, Nt, c->nn_cell, w, idx, dist, nullptr, nullptr,
                              c->nCU, (hipStream_t)stream);
    }
    if ((D == 32 || D == 3) && (size_t)Ns * Nt >= (1u << 20) && (dist_type == YOHO_DIST_L2 || dist_type == YOHO_DIST_SQUARE_L2)) {
        int rc;
        unsigned long long* keys = nullptr;
        if ((rc = bind_ws(c, (hipStream_t)stream, [&](Arena& ar) { keys = ar.take<unsigned long long>((size_t)Ns); }))) return rc;
        if ((rc = launch_nn32seg(src, Ns, tgt, Nt, D, dist_type, c->nCU, keys, true, nullptr, nullptr, nullptr, (hipStream_t)stream))) return rc;
        return launch_nn_unpack(keys, Ns, idx, dist, (hipStream_t)stream);
    }
    return launch_nn32seg(src, Ns, tgt, Nt, D, dist_type, c->nCU, nullptr, false, nullptr, idx, dist, (hipStream_t)stream);
}

int yoho_mutual_nn(yoho_ctx* c, const float* a, int Na, const float* b, int Nb, int64_t* pairs, int* M_out, void* stream) {
    if (!c || !a || !b || !pairs || !M_out || Na < 1 || Nb < 1) { set_error("yoho_mutual_nn: bad argument"); return YOHO_EINVAL; }
    YOHO_NEED_ALIGNED("yoho_mutual_nn", 15, a, b, pairs);
    YOHO_NEED_ALIGNED("yoho_mutual_nn", 3, M_out);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((size_t)Na * Nb >= (1u << 20) && c->nn_prefilter) {
        // MFMA pre-filter + exact evaluation of the candidates (matchf.hip): the same packed keys as the segmented search below
        MfArgs p;
        if ((rc = bind_ws(c, s, [&](Arena& ar) { mutual_prefilter_layout(ar, Na, Nb, p); }))) return rc;
        if ((rc = launch_mutual_prefilter(p, a, b, c->nCU, s, c->env.nn_splits))) return rc;
        return launch_mutual_compact((const int64_t*)p.keysA, (const int64_t*)p.keysB, Na, pairs, M_out, s, true);
    }
    int64_t *fwd = nullptr, *back = nullptr;                    // nearest neighbour of every a row in b, of every b row in a
    if ((rc = bind_ws(c, s, [&](Arena& ar) { fwd = ar.take<int64_t>((size_t)Na); back = ar.take<int64_t>((size_t)Nb); }))) return rc;
    if ((size_t)Na * Nb >= (1u << 20)) {
        // segmented search: the workspace words are the packed keys, the compaction reads the index half
        if ((rc = launch_nn32seg(a, Na, b, Nb, 32, YOHO_DIST_L2, c->nCU, (unsigned long long*)fwd, true, nullptr, nullptr, nullptr, s))) return rc;
        if ((rc = launch_nn32seg(b, Nb, a, Na, 32, YOHO_DIST_L2, c->nCU, (unsigned long long*)back, true, nullptr, nullptr, nullptr, s))) return rc;
        return launch_mutual_compact(fwd, back, Na, pairs, M_out, s, true);
    }
    if ((rc = launch_nn32seg(a, Na, b, Nb, 32, YOHO_DIST_L2, c->nCU, nullptr, false, nullptr, fwd, nullptr, s))) return rc;     // NN of every a-row in b  (KNN(feats1, feats0))
    if ((rc = launch_nn32seg(b, Nb, a, Na, 32, YOHO_DIST_L2, c->nCU, nullptr, false, nullptr, back, nullptr, s))) return rc;    // NN of every b-row in a  (KNN(feats0, feats1))
    return launch_mutual_compact(fwd, back, Na, pairs, M_out, s);
}

int yoho_des2r(yoho_ctx* c, const float* d1, const float* d2, int M, int64_t* idx, float* cor, void* stream) {
    if (!c || !d1 || !d2 || !idx || M < 0) { set_error("yoho_des2r: bad argument"); return YOHO_EINVAL; }
    if (M == 0) return 0;
    YOHO_NEED_ALIGNED("yoho_des2r", 15, d1, d2);
    YOHO_NEED_ALIGNED("yoho_des2r", 7, idx);
    YOHO_NEED_ALIGNED("yoho_des2r", 3, cor);
    HIPCHK(hipSetDevice(c->device));
    return launch_des2r(d1, nullptr, d2, nullptr, 1, c->dPq, M, idx, cor, (hipStream_t)stream);
}

int yoho_des2r_indexed(yoho_ctx* c, const float* e1, const int64_t* i1, const float* e2, const int64_t* i2, int istride, int M,
                       int64_t* idx, float* cor, void* stream) {
    if (!c || !e1 || !e2 || !i1 || !i2 || !idx || M < 0 || istride < 1) { set_error("yoho_des2r_indexed: bad argument"); return YOHO_EINVAL; }
    if (M == 0) return 0;
    YOHO_NEED_ALIGNED("yoho_des2r_indexed", 15, e1, e2);
    YOHO_NEED_ALIGNED("yoho_des2r_indexed", 7, i1, i2, idx);
    YOHO_NEED_ALIGNED("yoho_des2r_indexed", 3, cor);
    HIPCHK(hipSetDevice(c->device));
    return launch_des2r(e1, i1, e2, i2, istride, c->dPq, M, idx, cor, (hipStream_t)stream);
}

}  // extern "C"
