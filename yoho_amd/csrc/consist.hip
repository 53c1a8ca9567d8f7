// Geometric-consistency consensus (include/yoho_consist.h).  Compiled with -ffp-contract=off like refine.hip / verify.hip
// (yoho_amd/build.py): the graph's distances are a stated order of rounded f64 operations, the fit is the Kabsch step of rffit.h as
// refine.hip's refit runs it, everything between them is integer.  rfgrid.h is here for the entries' refusals only: there is no grid.
//
//   cg_graph_kernel    grid (W, ceil(M / 256)): one thread per (row i, word w), the 64 partners of the word broadcast from LDS
//   cg_deg_kernel      one wave per row: popcount of its W words
//   cg_sc2_kernel      one workgroup per row i: its set bits compacted to a neighbour list in LDS, the rows of the list gathered
//   cs_seed_kernel     one workgroup: K greedy rounds of vf_select_kernel's (value << 32 | ~index) maximum, neighbours of a seed killed
//   cs_sval_kernel     grid (ceil(M / 256), K): S[seed][m] for the seed's neighbours, one wave per neighbour row, and the block's maximum
//   cs_sum1_kernel     grid (ceil(M / 256), K): Smax, the half-of-maximum rule -> member mask, first-pass partial sums
//   cs_mean_kernel / cs_cov_kernel / cs_solve_kernel   the Kabsch step (rffit.h) with a row per hypothesis
//
// THE GRAPH.  Thread (i, w) computes the 64 bits C[i][64 w .. 64 w + 63] and stores one word: both triangles are computed, the
// symmetry is IEEE's (the header), so no pass mirrors anything and no word has two writers.  The partners' six coordinates sit in LDS
// and every lane reads the same address in the same step (a broadcast, no bank conflict); the lane's own match stays in registers.  A
// partner behind M is loaded as NaN and is tested against M as well: the tail bits of the last word are 0.  2 M^2 f64 square roots
// in all - 2.1e7 at M = 3233, 5.4e8 at the limit.
//
// THE SCORES.  s2[i] = SUM over the set bits j of row i of popcount(row_i & row_j).  The dense form is M^2 W word operations whatever the
// graph holds; walking row i's set bits is M deg W, never more and about M / deg times fewer (27 x at M = 3233, deg 120).  The gather
// decides the memory traffic: a neighbour's row is W contiguous words, read by consecutive lanes (one 512-byte request per 64 words).
// The walk needs the neighbours as a list, or the lanes of a wave would have to agree on the next set bit word by word: thread t
// owns word t of row i (W <= 256), counts its bits, an exclusive scan of the counts over the workgroup (a __shfl_up scan per wave,
// four wave totals in LDS) gives the word's first slot, and the thread writes its bits' indices there as 16-bit numbers (M <= 2^14):
// the list is ascending and its length is the row's degree.  Row i itself - the broadcast operand - stays in LDS, 8 bytes per lane at
// consecutive addresses (conflict-free ds_read_b64).  Then
//   W <= 64 (ONE): a lane owns word l % Wp of slot l / Wp, Wp the power of two >= W: 64 / Wp neighbours per wave and step, its word of
//   row i in a register, one load + and + popcount per neighbour, unrolled four deep so that four gathers are in flight;
//   W > 64: a wave per neighbour, the lane's words l, l + 64, ... against LDS.
// The four waves take the list's entries round robin.  Per-lane int sums, a __shfl_xor butterfly, four words of LDS: integer sums do not
// depend on the order.  A hybrid with a dense path was not built: the dense form only wins when deg approaches M, where the two
// cost the same.  The tail bits of row i's last word are masked on load, so no index >= M is ever formed whatever `bits` holds.
//
// THE HYPOTHESES.  Kc, the number of seeds, never leaves the device: K rows are launched and a workgroup whose row is >= Kc returns on
// a loaded word (verify.hip's idiom).  S[seed][m] is recomputed for the seed's neighbours only (K deg W word operations), kept in
// the workspace as int32 (-1 for a non-neighbour), the block maxima beside it: the kernel boundary in front of cs_sum1_kernel makes
// Smax known to every workgroup without an atomic or a hand-off.  The member mask then drives the step's two passes - centroids,
// centred products - and one thread per row runs rf_rotation.  Every workspace byte is written before it is read.
//
// Registers (hipcc -O3, gfx950) and timings: profiles/consist.md; no kernel of this file uses scratch.
#include "rfgrid.h"
#include "rffit.h"
#include "yoho_consist.h"
#include <cmath>

namespace yoho {

struct CsState {
    int Kc;                  // seeds taken
    int pad;
};

struct CsRow {
    double c0[3], c1[3];     // centroids of the row's set
    int n;                   // its size
    int pad;
};

// the bits of the last word that stand for matches: all of them when M is a multiple of 64
__device__ __forceinline__ u64 cg_last_mask(int M) { return (M & 63) ? ((1ull << (M & 63)) - 1ull) : ~0ull; }

__device__ __forceinline__ double cg_len(const double* p, const double* q) {
    const double dx = __dsub_rn(p[0], q[0]), dy = __dsub_rn(p[1], q[1]), dz = __dsub_rn(p[2], q[2]);
    return sqrt(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
}

__device__ __forceinline__ int cg_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ int cg_wave_max(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const int u = __shfl_xor(v, o); v = u > v ? u : v; }
    return v;
}

// ---- the graph -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cg_graph_kernel(const double* __restrict__ k0, const double* __restrict__ k1, int M, int W, double tol, double min_len,
                                                       u64* __restrict__ bits) {
    __shared__ double pj[64][6];                                      // the word's partners: k0[j] (3), k1[j] (3)
    const int w = blockIdx.x, j0 = w * 64;
    for (int t = threadIdx.x; t < 64 * 6; t += 256) {
        const int j = j0 + t / 6, c = t % 6;
        pj[t / 6][c] = j < M ? (c < 3 ? k0[3 * (size_t)j + c] : k1[3 * (size_t)j + c - 3]) : __builtin_nan("");
    }
    __syncthreads();
    const int i = blockIdx.y * 256 + threadIdx.x;
    if (i >= M) return;
    const double a0[3] = {k0[3 * (size_t)i], k0[3 * (size_t)i + 1], k0[3 * (size_t)i + 2]};
    const double b0[3] = {k1[3 * (size_t)i], k1[3 * (size_t)i + 1], k1[3 * (size_t)i + 2]};
    u64 word = 0ull;
    for (int b = 0; b < 64; ++b) {
        const double a = cg_len(a0, &pj[b][0]), bb = cg_len(b0, &pj[b][3]);
        const bool c = fabs(__dsub_rn(a, bb)) < tol && a >= min_len && bb >= min_len && j0 + b != i && j0 + b < M;      // a NaN comparison is false
        word |= (u64)(c ? 1 : 0) << b;
    }
    bits[(size_t)i * W + w] = word;
}

__global__ __launch_bounds__(256) void cg_deg_kernel(const u64* __restrict__ bits, int M, int W, int32_t* __restrict__ deg) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= M) return;                                               // wave-uniform
    int c = 0;
    for (int w = lane; w < W; w += 64) c += __popcll(bits[(size_t)i * W + w]);
    c = cg_wave_sum(c);
    if (lane == 0) deg[i] = c;
}

// ---- the scores ------------------------------------------------------------------------------------------------------------------------
// dynamic LDS: the neighbour list, M 16-bit indices; wp_log2 (ONE only): log2 of the power of two >= W
template <bool ONE>
__global__ __launch_bounds__(256) void cg_sc2_kernel(const u64* __restrict__ bits, int M, int W, int wp_log2, int32_t* __restrict__ s2) {
    extern __shared__ unsigned short nbr[];
    __shared__ u64 rowi[256];
    __shared__ int wcnt[4], wtot[4];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    u64 mine = tid < W ? bits[(size_t)i * W + tid] : 0ull;
    if (tid == W - 1) mine &= cg_last_mask(M);
    rowi[tid] = mine;
    const int c = __popcll(mine);
    int inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(inc, o);
        if (lane >= o) inc += v;
    }
    if (lane == 63) wcnt[wv] = inc;
    __syncthreads();
    int pos = inc - c;
    for (int k = 0; k < wv; ++k) pos += wcnt[k];
    const int deg = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];           // <= M - 1 after the mask (the diagonal aside): the list fits
    for (u64 m = mine; m; m &= m - 1ull) nbr[pos++] = (unsigned short)(tid * 64 + __builtin_ctzll(m));
    __syncthreads();
    int acc = 0;
    if (ONE) {
        const int wl = lane & ((1 << wp_log2) - 1), slot = lane >> wp_log2, G = 64 >> wp_log2;
        const bool act = wl < W;
        const u64 ri = act ? rowi[wl] : 0ull;
        const int wc = act ? wl : 0;                                  // an idle lane re-reads word 0 against a zero operand
#pragma unroll 4
        for (int n = wv * G + slot; n < deg; n += 4 * G) acc += __popcll(ri & bits[(size_t)nbr[n] * W + wc]);
    } else {
        for (int n = wv; n < deg; n += 4) {
            const u64* __restrict__ rj = bits + (size_t)nbr[n] * W;
            for (int w = lane; w < W; w += 64) acc += __popcll(rowi[w] & rj[w]);
        }
    }
    acc = cg_wave_sum(acc);
    if (lane == 0) wtot[wv] = acc;
    __syncthreads();
    if (tid == 0) s2[i] = wtot[0] + wtot[1] + wtot[2] + wtot[3];
}

// ---- the seeds -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cs_seed_kernel(const u64* __restrict__ bits, const int32_t* __restrict__ s2, int M, int W, int K,
                                                      unsigned char* __restrict__ alive, CsState* __restrict__ st, double* __restrict__ T_out,
                                                      int32_t* __restrict__ seeds, int32_t* __restrict__ sizes, int32_t* __restrict__ info) {
    __shared__ u64 wkey[4];
    const int tid = threadIdx.x;
    for (int m = tid; m < M; m += 256) alive[m] = s2[m] >= 1 ? 1 : 0;
    int Kc = 0, prev = -1;
    for (int r = 0; r < K; ++r) {
        const u64* __restrict__ prow = prev >= 0 ? bits + (size_t)prev * W : nullptr;      // the seed of the round before kills its neighbours
        u64 best = 0ull;                                              // an alive match has s2 >= 1: its key is not 0
        for (int m = tid; m < M; m += 256) {
            if (!alive[m]) continue;
            if (prow && ((prow[m >> 6] >> (m & 63)) & 1ull)) { alive[m] = 0; continue; }
            const u64 key = ((u64)(unsigned)s2[m] << 32) | (u64)(0xFFFFFFFFu - (unsigned)m);
            best = key > best ? key : best;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const u64 other = __shfl_xor(best, o);
            best = other > best ? other : best;
        }
        if ((tid & 63) == 0) wkey[tid >> 6] = best;
        __syncthreads();
        u64 b = wkey[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) b = wkey[w] > b ? wkey[w] : b;
        if (b == 0ull) break;                                         // nobody alive: the same word in every thread
        const int pos = (int)(0xFFFFFFFFu - (unsigned)(b & 0xFFFFFFFFull));
        __syncthreads();                                              // wkey has been read by everyone
        if (tid == (pos & 255)) alive[pos] = 0;                       // by its owner
        if (tid == 0) seeds[r] = pos;
        prev = pos;
        ++Kc;
    }
    for (int r = Kc + tid; r < K; r += 256) { seeds[r] = -1; sizes[r] = 0; }
    for (int e = 12 * Kc + tid; e < 12 * K; e += 256) T_out[e] = (e % 12) % 5 == 0 ? 1.0 : 0.0;      // [I | 0] behind the rows taken
    if (tid == 0) { st->Kc = Kc; st->pad = 0; info[0] = Kc; info[1] = M; }
}

// ---- the sets --------------------------------------------------------------------------------------------------------------------------
// sval[r][m] = S[seed_r][m] for the seed's neighbours, -1 for everybody else; smaxblk[r][block] = the largest of the block
__global__ __launch_bounds__(256) void cs_sval_kernel(const CsState* __restrict__ st, const u64* __restrict__ bits, const int32_t* __restrict__ seeds, int M, int W,
                                                      int nblk, int32_t* __restrict__ sval, int32_t* __restrict__ smaxblk) {
    const int r = blockIdx.y;
    if (r >= st->Kc) return;                                          // wave-uniform: a loaded word
    __shared__ int wmax[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int m0 = blockIdx.x * 256 + wv * 64;                        // the wave's 64 matches are word m0 / 64 of the seed's row
    const u64* __restrict__ rs = bits + (size_t)seeds[r] * W;
    const u64 last = cg_last_mask(M);
    u64 word = 0ull;
    if (m0 < M) {
        word = rs[m0 >> 6];
        if ((m0 >> 6) == W - 1) word &= last;
    }
    word = ((u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(word >> 32)) << 32) | (u64)(unsigned)__builtin_amdgcn_readfirstlane((int)word);
    int mine = -1;
    for (u64 mw = word; mw; mw &= mw - 1ull) {                        // the same word in every lane: a uniform loop
        const int b = __builtin_ctzll(mw);
        const u64* __restrict__ rm = bits + (size_t)(m0 + b) * W;
        int a = 0;
        for (int w = lane; w < W; w += 64) a += __popcll((w == W - 1 ? rs[w] & last : rs[w]) & rm[w]);
        a = cg_wave_sum(a);
        if (lane == b) mine = a;
    }
    if (m0 + lane < M) sval[(size_t)r * M + m0 + lane] = mine;
    const int mx = cg_wave_max(mine);
    if (lane == 0) wmax[wv] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        int b = wmax[0];
        for (int k = 1; k < 4; ++k) b = wmax[k] > b ? wmax[k] : b;
        smaxblk[(size_t)r * nblk + blockIdx.x] = b;
    }
}

// the half-of-maximum rule -> mask[r][m], and the first pass of the Kabsch step: slab row = {n, 0, SUM k0 (3), SUM k1 (3)} of the block
__global__ __launch_bounds__(256) void cs_sum1_kernel(const CsState* __restrict__ st, const int32_t* __restrict__ seeds, const int32_t* __restrict__ sval,
                                                      const int32_t* __restrict__ smaxblk, const double* __restrict__ k0, const double* __restrict__ k1, int M,
                                                      int nblk, unsigned char* __restrict__ mask, double* __restrict__ slab) {
    const int r = blockIdx.y;
    if (r >= st->Kc) return;
    __shared__ int smax_s;
    if (threadIdx.x < 64) {                                           // nblk <= 64 at the limit: one word per lane
        const int mx = cg_wave_max((int)threadIdx.x < nblk ? smaxblk[(size_t)r * nblk + threadIdx.x] : -1);
        if (threadIdx.x == 0) smax_s = mx;
    }
    __syncthreads();
    const int smax = smax_s, s = seeds[r];
    const int m = blockIdx.x * 256 + threadIdx.x;
    double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (m < M) {
        const int sv = sval[(size_t)r * M + m];
        const bool in = m == s || (sv >= 0 && 2 * sv >= smax);
        mask[(size_t)r * M + m] = in ? 1 : 0;
        if (in) rf_pair_row(k0 + 3 * (size_t)m, k1 + 3 * (size_t)m, v);
    }
    rf_block_sum<8>(v, slab + ((size_t)r * nblk + blockIdx.x) * RF_SLAB);
}

// ---- the fit (the refit's rf_mean_kernel / rf_refit_cov_kernel / rf_solve_kernel of refine.hip with a row per hypothesis) -----------------
__global__ __launch_bounds__(64) void cs_mean_kernel(const CsState* __restrict__ st, const double* __restrict__ slab, int nblk, CsRow* __restrict__ rows,
                                                     int32_t* __restrict__ sizes) {
    const int r = blockIdx.x;
    if (r >= st->Kc) return;
    __shared__ double tot[8];
    rf_slab_total<8>(slab + (size_t)r * nblk * RF_SLAB, nblk, RF_SLAB, tot);
    __syncthreads();
    const int n = (int)tot[0];
    rf_centroids(tot, n, rows[r].c0, rows[r].c1);
    if (threadIdx.x == 0) { rows[r].n = n; rows[r].pad = 0; sizes[r] = n; }
}

__global__ __launch_bounds__(256) void cs_cov_kernel(const CsState* __restrict__ st, const CsRow* __restrict__ rows, const double* __restrict__ k0,
                                                     const double* __restrict__ k1, int M, int nblk, const unsigned char* __restrict__ mask,
                                                     double* __restrict__ slab) {
    const int r = blockIdx.y;
    if (r >= st->Kc) return;
    const int m = blockIdx.x * 256 + threadIdx.x;
    double v[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (m < M && mask[(size_t)r * M + m]) rf_centred_products(k0 + 3 * (size_t)m, k1 + 3 * (size_t)m, rows[r].c0, rows[r].c1, v);
    rf_block_sum<9>(v, slab + ((size_t)r * nblk + blockIdx.x) * RF_SLAB);
}

__global__ __launch_bounds__(64) void cs_solve_kernel(const CsState* __restrict__ st, const CsRow* __restrict__ rows, const double* __restrict__ slab, int nblk,
                                                      double* __restrict__ T_out, int32_t* __restrict__ sizes) {
    const int r = blockIdx.x;
    if (r >= st->Kc) return;
    __shared__ double H[9];
    rf_slab_total<9>(slab + (size_t)r * nblk * RF_SLAB, nblk, RF_SLAB, H);
    __syncthreads();
    if (threadIdx.x != 0) return;
    double* T = T_out + 12 * (size_t)r;
    const CsRow& cr = rows[r];
    double R[9];
    if (cr.n < 3 || !rf_rotation(H, R)) {
#pragma unroll
        for (int i = 0; i < 12; ++i) T[i] = __builtin_nan("");
        sizes[r] = -cr.n;
        return;
    }
    rf_rigid_row(R, cr.c0, cr.c1, T);
}

static int cg_check_m(const char* fn, yoho_ctx* c, int M) {
    const int rc = rf_check_sizes(fn, c, "M", M, 1);
    return rc ? rc : rf_check_limit(fn, RF_NAMED(YOHO_CONSIST_MAX_M), "M", M);
}

}  // namespace yoho

using namespace yoho;

extern "C" {

int yoho_consistency_graph(yoho_ctx* c, const double* k0, const double* k1, int M, double tol, double min_len, uint64_t* bits, int32_t* deg, void* stream) {
    const char* fn = "yoho_consistency_graph";
    int rc;
    if ((rc = cg_check_m(fn, c, M))) return rc;
    if (!(tol > 0.0) || !std::isfinite(tol)) { set_error("yoho_consistency_graph: tol=%g must be finite and > 0", tol); return YOHO_EINVAL; }
    if (!(min_len >= 0.0) || !std::isfinite(min_len)) { set_error("yoho_consistency_graph: min_len=%g must be finite and >= 0", min_len); return YOHO_EINVAL; }
    if ((rc = rf_check_pointers(fn, k0 && k1 && bits && deg))) return rc;
    YOHO_NEED_ALIGNED("yoho_consistency_graph", 7, k0, k1, bits);
    YOHO_NEED_ALIGNED("yoho_consistency_graph", 3, deg);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int W = (M + 63) / 64;
    hipLaunchKernelGGL(cg_graph_kernel, dim3(W, (M + 255) / 256), dim3(256), 0, s, k0, k1, M, W, tol, min_len, (u64*)bits);
    hipLaunchKernelGGL(cg_deg_kernel, dim3((M + 3) / 4), dim3(256), 0, s, (const u64*)bits, M, W, deg);
    HIPCHK(hipGetLastError());
    return 0;
}

int yoho_sc2_scores(yoho_ctx* c, const uint64_t* bits, int M, int32_t* s2, void* stream) {
    const char* fn = "yoho_sc2_scores";
    int rc;
    if ((rc = cg_check_m(fn, c, M)) ||
        (rc = rf_check_pointers(fn, bits && s2))) return rc;
    YOHO_NEED_ALIGNED("yoho_sc2_scores", 7, bits);
    YOHO_NEED_ALIGNED("yoho_sc2_scores", 3, s2);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int W = (M + 63) / 64;
    const size_t lds = (((size_t)M * sizeof(unsigned short)) + 15) & ~(size_t)15;
    if (W <= 64) {
        int wp_log2 = 0;
        while ((1 << wp_log2) < W) ++wp_log2;
        hipLaunchKernelGGL(cg_sc2_kernel<true>, dim3(M), dim3(256), lds, s, (const u64*)bits, M, W, wp_log2, s2);
    } else {
        hipLaunchKernelGGL(cg_sc2_kernel<false>, dim3(M), dim3(256), lds, s, (const u64*)bits, M, W, 6, s2);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

int yoho_consensus_hypotheses(yoho_ctx* c, const double* k0, const double* k1, int M, const uint64_t* bits, const int32_t* s2, int K, double* T_out,
                              int32_t* seeds, int32_t* sizes, int32_t* info, void* stream) {
    const char* fn = "yoho_consensus_hypotheses";
    int rc;
    if ((rc = cg_check_m(fn, c, M)) ||
        (rc = rf_check_range(fn, "K", K, 1, RF_NAMED(YOHO_CONSIST_MAX_K))) ||
        (rc = rf_check_pointers(fn, k0 && k1 && bits && s2 && T_out && seeds && sizes && info))) return rc;
    YOHO_NEED_ALIGNED("yoho_consensus_hypotheses", 7, k0, k1, bits, T_out);
    YOHO_NEED_ALIGNED("yoho_consensus_hypotheses", 3, s2, seeds, sizes, info);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int W = (M + 63) / 64, nblk = (M + 255) / 256;
    CsState* st = nullptr;
    CsRow* rows = nullptr;
    unsigned char *alive = nullptr, *mask = nullptr;
    int32_t *sval = nullptr, *smaxblk = nullptr;
    double* slab = nullptr;
    if ((rc = bind_ws(c, s, [&](Arena& ar) {
            st = ar.take<CsState>(1);
            rows = ar.take<CsRow>((size_t)K);
            alive = ar.take<unsigned char>((size_t)M);
            sval = ar.take<int32_t>((size_t)K * M);
            smaxblk = ar.take<int32_t>((size_t)K * nblk);
            mask = ar.take<unsigned char>((size_t)K * M);
            slab = ar.take<double>((size_t)RF_SLAB * nblk * K);
        }))) return rc;
    const u64* b = (const u64*)bits;
    hipLaunchKernelGGL(cs_seed_kernel, dim3(1), dim3(256), 0, s, b, s2, M, W, K, alive, st, T_out, seeds, sizes, info);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(cs_sval_kernel, dim3(nblk, K), dim3(256), 0, s, (const CsState*)st, b, (const int32_t*)seeds, M, W, nblk, sval, smaxblk);
    hipLaunchKernelGGL(cs_sum1_kernel, dim3(nblk, K), dim3(256), 0, s, (const CsState*)st, (const int32_t*)seeds, (const int32_t*)sval, (const int32_t*)smaxblk, k0, k1,
                       M, nblk, mask, slab);
    hipLaunchKernelGGL(cs_mean_kernel, dim3(K), dim3(64), 0, s, (const CsState*)st, (const double*)slab, nblk, rows, sizes);
    hipLaunchKernelGGL(cs_cov_kernel, dim3(nblk, K), dim3(256), 0, s, (const CsState*)st, (const CsRow*)rows, k0, k1, M, nblk, (const unsigned char*)mask, slab);
    hipLaunchKernelGGL(cs_solve_kernel, dim3(K), dim3(64), 0, s, (const CsState*)st, (const CsRow*)rows, (const double*)slab, nblk, T_out, sizes);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
