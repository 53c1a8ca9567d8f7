// Irrep GEMMs of the group-Fourier conv (see gemmf.hip for the algebra and the operand packs), second blocking:
// 256 x 128 output tile per workgroup, TWO workgroups per CU.
//
// Why.  With one 256 x 256 workgroup per CU (gemmf.hip) nothing overlaps a workgroup's epilogue: its four waves hold 256
// accumulator registers each, write 256 KiB of fp32 coefficients and only then can the CU start the next tile - a quarter
// of the kernel's time is spent draining stores with the matrix pipes idle.  Here a wave owns 128 x 64 outputs (128
// accumulator registers, at most 256 registers in all), a workgroup needs 72 KiB of LDS, and two workgroups share a CU:
// while one of them runs its prologue (first DMA stages, residual loads) or its epilogue (stores), the other one's K loop
// has the matrix pipes to itself.
//
// K loop.  Steps of K = 16 (one MFMA sub-step): a step is 16 KiB of the A tile (256 rows x 16 k x {hi, lo}) + 8 KiB of
// one 128-column half of the B tile, copied by LDS DMA straight from the packs into a ring of three 24 KiB buffers
// (the packs are unchanged: a half column tile is four 2 KiB runs of the 256-column pack).  In iteration s a wave issues
// its 24 MFMAs on the fragments of step s (registers), reads the 12 fragments of step s+1 from the ring and issues its
// six 1 KiB pieces of the DMA of step s+3; at the end `s_waitcnt vmcnt(6)` (the six pieces just issued stay in flight) and
// one barrier make step s+2 readable: the DMA runs two steps ahead of its consumers.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include "common.h"
#include "gemmf.h"

namespace yoho {

constexpr int F2_BUF = 24576;                 // fgemm2's ring buffer: A 16 KiB [plane 2][k-group 2][row 256][16 B] | B 8 KiB [plane 2][k-group 2][col 128][16 B]
constexpr int F2_LDS = 3 * F2_BUF;
constexpr int F3_BUF = 32768;                 // fgemm3's: the same A | B 16 KiB [plane 2][k-group 2][col 256][16 B]
constexpr int F3_LDS = 3 * F3_BUF;

struct Frags2 {
    uintx4 ah[4], al[4], bh[2], bl[2];
};

// fragment read R (0..11) of a step, in the order of use: A lo x4, B hi x2 (products lo.hi), A hi x4, B lo x2; LO = offset of B's lo plane
template <int LO, int R>
__device__ __forceinline__ void read_frag2(const char* pa, const char* pb, Frags2& f) {
    if constexpr (R < 4) f.al[R] = *reinterpret_cast<const uintx4*>(pa + 8192 + R * 512);
    else if constexpr (R < 6) f.bh[R - 4] = *reinterpret_cast<const uintx4*>(pb + (R - 4) * 512);
    else if constexpr (R < 10) f.ah[R - 6] = *reinterpret_cast<const uintx4*>(pa + (R - 6) * 512);
    else f.bl[R - 10] = *reinterpret_cast<const uintx4*>(pb + LO + (R - 10) * 512);
}
template <int LO>
__device__ __forceinline__ void read_frags2(const char* pa, const char* pb, Frags2& f) {
    sfor<0, 12>([&](auto rc) { read_frag2<LO, decltype(rc)::value>(pa, pb, f); });
}

// A wave's share of the LDS DMA of one K16 step, in pieces of 1 KiB.  srcA / srcB point at the step inside the packs (stage * 32 KiB +
// sub-step * 8 KiB, wave uniform).  fgemm2 (four waves, 24 KiB): six pieces; la / lb are the per-lane byte offsets inside the A and B parts.
struct Dma2 {
    static constexpr int NP = 6, LO = 4096;
    int la, lb, w;
    __device__ __forceinline__ Dma2(int w_, int lane) : la(w_ * 1024 + lane * 16), lb((w_ >> 1) * 4096 + (w_ & 1) * 1024 + lane * 16), w(w_) {}
    template <int U>
    __device__ __forceinline__ void piece(const char* srcA, const char* srcB, char* buf) const {
        if constexpr (U < 4) {
            constexpr int plane = U >> 1, kg = U & 1;                       // A: piece (plane, kg, 64-row block w)
            __builtin_amdgcn_global_load_lds((gptr_t)(srcA + plane * 16384 + kg * 4096 + la), (lptr_t)(buf + plane * 8192 + kg * 4096 + w * 1024), 16, 0, 0);
        } else {
            constexpr int plane = U - 4;                                    // B: piece (plane, kg = w >> 1, 64-column block w & 1)
            __builtin_amdgcn_global_load_lds((gptr_t)(srcB + plane * 16384 + lb), (lptr_t)(buf + 16384 + plane * 4096 + (w >> 1) * 2048 + (w & 1) * 1024), 16, 0, 0);
        }
    }
};
// the 256 x 256 tiles (eight waves, 32 KiB): four pieces, U = 0, 1: A plane U; U = 2, 3: B plane U - 2; the wave's (k-group w8 >> 2, 64-row /
// 64-column block w8 & 3) is folded into `la` (source, the same for the A and the B piece) and `ldst` (destination)
struct Dma3 {
    static constexpr int NP = 4, LO = 8192;
    int la, ldst;
    __device__ __forceinline__ Dma3(int w8, int lane) : la(w8 * 1024 + lane * 16), ldst(w8 * 1024) {}
    template <int U>
    __device__ __forceinline__ void piece(const char* srcA, const char* srcB, char* buf) const {
        constexpr int plane = U & 1;
        if constexpr (U < 2) __builtin_amdgcn_global_load_lds((gptr_t)(srcA + plane * 16384 + la), (lptr_t)(buf + plane * 8192 + ldst), 16, 0, 0);
        else __builtin_amdgcn_global_load_lds((gptr_t)(srcB + plane * 16384 + la), (lptr_t)(buf + 16384 + plane * 8192 + ldst), 16, 0, 0);
    }
};
template <typename Dma>
__device__ __forceinline__ void dma_step(const Dma& dm, const char* srcA, const char* srcB, char* buf) {
    sfor<0, Dma::NP>([&](auto uc) { dm.template piece<decltype(uc)::value>(srcA, srcB, buf); });
}

// One K16 step: 24 MFMAs on `f` (every accumulator gets lo.hi, hi.lo, hi.hi, 8 MFMAs apart); behind them, one per MFMA, the 12 fragment
// reads of the next step and (DMA) the wave's DMA pieces of the step three ahead: piece p rides behind MFMA 12 + p.
template <bool DMA, typename Dma>
__device__ __forceinline__ void step2(const Dma& dm, const Frags2& f, floatx16 (&acc)[4][2], const char* ra, const char* rb, Frags2& nf,
                                      const char* srcA, const char* srcB, char* dmabuf) {
    sfor<0, 8>([&](auto gc) {
        constexpr int g = decltype(gc)::value;
        acc[g >> 1][g & 1] = mfma_h(f.al[g >> 1], f.bh[g & 1], acc[g >> 1][g & 1]);
        read_frag2<Dma::LO, g>(ra, rb, nf);
        __builtin_amdgcn_sched_barrier(0);
    });
    sfor<0, 8>([&](auto gc) {
        constexpr int g = decltype(gc)::value;
        acc[g >> 1][g & 1] = mfma_h(f.ah[g >> 1], f.bl[g & 1], acc[g >> 1][g & 1]);
        if constexpr (g < 4) read_frag2<Dma::LO, 8 + g>(ra, rb, nf);
        else if constexpr (DMA) dm.template piece<g - 4>(srcA, srcB, dmabuf);
        __builtin_amdgcn_sched_barrier(0);
    });
    sfor<0, 8>([&](auto gc) {
        constexpr int g = decltype(gc)::value;
        acc[g >> 1][g & 1] = mfma_h(f.ah[g >> 1], f.bh[g & 1], acc[g >> 1][g & 1]);
        if constexpr (DMA && 4 + g < Dma::NP) dm.template piece<4 + g>(srcA, srcB, dmabuf);
        __builtin_amdgcn_sched_barrier(0);
    });
}

// Work map.  Workgroup b runs on XCD b & 7; a column tile (irrep t, ntile) and all its row tiles stay on one XCD (the B panel is
// read from HBM once and served from that XCD's L2), column tiles of an irrep are dealt round-robin over the XCDs (gemmf.hip).
// The two workgroups of a CU must NOT run in lockstep - if both reach their epilogue together nothing is gained over one large
// tile - so the slots of an XCD alternate between the d = 5 irrep (long K loops: 40000 of an XCD's 78000 steps for 256 -> 512)
// and the other four (shorter K loops, in launch order): co-resident workgroups then have different lengths and drift apart
// after the first round.  Returns false for a slot beyond the XCD's work.
__host__ __device__ inline bool fg2_map(const FGemmArgs& a, int xcd, int slot, bool contiguous, int& t, int& local, int& r) {
    int cnt[NIR_ORD], ru[NIR_ORD];
    for (int u = 0; u < NIR_ORD; ++u) {
        ru[u] = (xcd + a.rot[u]) & 7;
        cnt[u] = a.NT[u] > ru[u] ? ((a.NT[u] - 1 - ru[u]) / 8 + 1) * a.MT[u] * 2 : 0;
    }
    const int L = cnt[0], S = cnt[1] + cnt[2] + cnt[3] + cnt[4];
    int list, idx;                                   // list 0: the first irrep, list 1: the others, idx: position in that list
    if (contiguous) { list = slot < L ? 0 : 1; idx = slot < L ? slot : slot - L; }
    else {
        const int P = L < S ? L : S;
        if (slot < 2 * P) { list = slot & 1; idx = slot >> 1; }
        else { list = L > S ? 0 : 1; idx = P + (slot - 2 * P); }
    }
    if (list == 0) {
        if (idx >= L) return false;
        t = 0; local = idx; r = ru[0];
        return true;
    }
    for (int u = 1; u < NIR_ORD; ++u) {
        if (idx < cnt[u]) { t = u; local = idx; r = ru[u]; return true; }
        idx -= cnt[u];
    }
    return false;
}

// byte offset of K16 step ks inside a tile's pack: stage (ks >> 1) * 32 KiB + sub-step (ks & 1) * 8 KiB
__device__ __forceinline__ size_t step_off(int ks) { return (size_t)(ks >> 1) * FG_STAGE + (size_t)(ks & 1) * 8192; }

// ---------------------------------------------------------------------------------------------------------------
// The pipelined ring (fgemm2, fgemm3, fgemm3s).  Step s lives in buffer s % 3 of BUF bytes.  In iteration s a wave issues its MFMAs on
// the fragments of step s (registers), reads the fragments of step s + 1 from the ring and issues its INFLIGHT pieces of the DMA of
// step s + 3 into the buffer of step s; `s_waitcnt vmcnt(INFLIGHT)` (the pieces just issued stay in flight) and one barrier then make
// step s + 2 readable.  P: the fragments of step 0, read by the caller behind the prologue's barrier; step(dma, f, nf, ra, rb, srcA, srcB,
// dmabuf) is the kernel's step function (dma: std::bool_constant).
// ---------------------------------------------------------------------------------------------------------------
template <int BUF, typename Dma>
__device__ __forceinline__ void ring_prologue(int KT, Dma&& dma) {      // steps 0, 1, 2 into the three buffers
    dma(0, 0);
    dma(1, BUF);
    if (KT > 2) dma(2, 2 * BUF);
}

template <int BUF, int INFLIGHT, typename F, typename Step>
__device__ __forceinline__ void ring_pipelined(char* smem, const char* Ag, const char* Bg, int KT, int lane_a, int lane_b, F& P, Step&& step) {
    F Q;
    // Every wave must have step 0 in registers before ANY wave overwrites buffer 0 with step 3 (the first DMA of the loop below):
    // inside the loop the barrier at the end of step s - 1 orders the reads of step s before the DMA of step s + 3, but between
    // the prologue's barrier and the first step there was nothing - a wave delayed by a few hundred cycles (cold instruction
    // cache at the head of a launch) read step 3's rows in place of step 0's.  Found in round 3 by the depth-first schedule
    // (many short launches), whose outputs differed from the breadth-first pass in whole 32-keypoint wave tiles.
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    int cur = 0, nxt = BUF;                      // buffer of step s (already in registers: the target of the DMA of step s + 3), of step s + 1
    int s = 0;
    // step s on f, the fragments of step s + 1 into nf
    auto run = [&](auto dma, const F& f, F& nf) {
        if constexpr (decltype(dma)::value) {
            step(dma, f, nf, smem + nxt + lane_a, smem + nxt + lane_b, uniform_ptr(Ag + step_off(s + 3)), uniform_ptr(Bg + step_off(s + 3)), smem + cur);
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(INFLIGHT) : "memory");
        } else {
            step(dma, f, nf, smem + nxt + lane_a, smem + nxt + lane_b, nullptr, nullptr, nullptr);
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        cur = nxt; nxt = nxt == 2 * BUF ? 0 : nxt + BUF; ++s;
    };
    constexpr std::true_type dma;
    constexpr std::false_type nodma;
    // main loop: both steps of a pair still have a DMA to issue
    while (s + 4 < KT) {
        run(dma, P, Q);
        run(dma, Q, P);
    }
    // tail: the last four steps (two if KT == 2); only the first of them still has a DMA (step KT - 1) to issue
    if (KT >= 4) {
        run(dma, P, Q);
        run(nodma, Q, P);
    }
    run(nodma, P, Q);
    // last step: its "next" fragments are read from a buffer that holds valid (unused) data
    step(nodma, Q, P, smem + cur + lane_a, smem + cur + lane_b, nullptr, nullptr, nullptr);
}

// a wave whose 128 rows are all padding (cout = 32): keep its share of the DMA and the barriers going (the live waves meet at one
// barrier per step but the last)
template <int BUF, typename Dma>
__device__ __forceinline__ void ring_pipelined_idle(int KT, Dma&& dma) {
    __builtin_amdgcn_s_barrier();                              // the live waves' barrier behind their reads of step 0
    for (int s = 0; s + 1 < KT; ++s) {
        if (s + 3 < KT) dma(s + 3, (s % 3) * BUF);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
}

__global__ __launch_bounds__(256, 2) void fgemm2_kernel(FGemmArgs a, int flags) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    // two workgroups - the two 128-column halves - per (column tile, row tile), neighbours in their irrep's list: they stream the
    // same A stages at about the same time, so one of the two reads hits the XCD's L2
    int t = 0, local = 0, r = 0;
    if (!fg2_map(a, blockIdx.x & 7, blockIdx.x >> 3, (flags & F2_MIX) == 0, t, local, r)) return;
    const int d = a.dim[t];
    const int MT = a.MT[t], KS = d * a.cin / 32, KT = 2 * KS;
    const int nh = local & 1, pair = local >> 1;
    const int cg = pair / MT, mtile = pair - cg * MT;
    const int ntile = r + 8 * cg;
    const char* Ag = a.A + a.a_off[t] + (size_t)mtile * KS * FG_STAGE;
    const char* Bg = a.B + a.b_off[t] + (size_t)ntile * KS * FG_STAGE + nh * 2048;
    const int wm = w >> 1, wn = w & 1;
    const Dma2 dm(w, lane);
    const int lane_a = (lane >> 5) * 4096 + (wm * 128 + (lane & 31)) * 16;
    const int lane_b = 16384 + (lane >> 5) * 2048 + (wn * 64 + (lane & 31)) * 16;

    floatx16 acc[4][2];
    zero_acc(acc);
    auto dma = [&](int st, int buf) { dma_step(dm, Ag + step_off(st), Bg + step_off(st), smem + buf); };
    ring_prologue<F2_BUF>(KT, dma);
    const int row0 = mtile * 256 + wm * 128, colbase = ntile * 256 + nh * 128 + wn * 64;
    const bool rows_live = row0 < d * a.cout;       // else: all 128 rows of this wave are padding (cout = 32)
    const int jidx = colbase / a.kppad, kp0 = colbase - jidx * a.kppad, qbase = a.qbase[t];
    if ((flags & EPI_RES) && rows_live) residual_start(acc, row0, kp0, jidx, d, qbase, a.res, a.descale, a.cout, a.nT32, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (!rows_live) return ring_pipelined_idle<F2_BUF>(KT, dma);

    Frags2 P;
    read_frags2<Dma2::LO>(smem + lane_a, smem + lane_b, P);
    ring_pipelined<F2_BUF, 6>(smem, Ag, Bg, KT, lane_a, lane_b, P,
        [&](auto dmac, const Frags2& f, Frags2& nf, const char* ra, const char* rb, const char* srcA, const char* srcB, char* buf) {
            step2<decltype(dmac)::value>(dm, f, acc, ra, rb, nf, srcA, srcB, buf);
        });
    coef_epilogue(acc, row0, kp0, jidx, d, qbase, a.out, a.bias, a.descale, a.cout, a.nT32, a.rflag, lane, flags);
}

// ---------------------------------------------------------------------------------------------------------------
// fgemm3: the same K loop with the two 128-column halves of a 256 x 256 tile in ONE workgroup of eight waves (two per SIMD).
// The halves share the A stage in LDS, so the L2 -> LDS traffic and the fabric traffic are those of the 256 x 256 blocking
// (a step is 16 KiB of A + 16 KiB of B, ring of three 32 KiB buffers = 96 KiB), while every SIMD still has two waves.
// ---------------------------------------------------------------------------------------------------------------
// What fgemm3, fgemm3c and cgemm share: waves 0-3 own the left 128 columns of the tile, 4-7 the right; in a half, 2 (rows) x 2 (columns) waves
struct Wave3 {
    int wm, wn, nh, lane_a, lane_b;
    Dma3 dm;
    __device__ __forceinline__ Wave3(int w8, int lane) : wm((w8 & 3) >> 1), wn(w8 & 1), nh(w8 >> 2), dm(w8, lane) {
        lane_a = (lane >> 5) * 4096 + (wm * 128 + (lane & 31)) * 16;
        lane_b = 16384 + (lane >> 5) * 4096 + (nh * 128 + wn * 64 + (lane & 31)) * 16;
    }
};

__global__ __launch_bounds__(512, 2) void fgemm3_kernel(FGemmArgs a, int flags) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const Wave3 wv(__builtin_amdgcn_readfirstlane(tid >> 6), lane);
    int t = 0, local = 0, r = 0;
    if (!fg3_map(a, blockIdx.x & 7, blockIdx.x >> 3, t, local, r)) return;
    const int d = a.dim[t];
    const int MT = a.MT[t], KS = d * a.cin / 32, KT = 2 * KS;
    const int cg = local / MT, mtile = local - cg * MT;
    const int ntile = r + 8 * cg;
    const char* Ag = a.A + a.a_off[t] + (size_t)mtile * KS * FG_STAGE;
    const char* Bg = a.B + a.b_off[t] + (size_t)ntile * KS * FG_STAGE;

    floatx16 acc[4][2];
    zero_acc(acc);
    auto dma = [&](int st, int buf) { dma_step(wv.dm, Ag + step_off(st), Bg + step_off(st), smem + buf); };
    ring_prologue<F3_BUF>(KT, dma);
    const int row0 = mtile * 256 + wv.wm * 128, colbase = ntile * 256 + wv.nh * 128 + wv.wn * 64;
    const bool rows_live = row0 < d * a.cout;       // else: all 128 rows of this wave are padding (cout = 32)
    const int jidx = colbase / a.kppad, kp0 = colbase - jidx * a.kppad, qbase = a.qbase[t];
    if ((flags & EPI_RES) && rows_live) residual_start(acc, row0, kp0, jidx, d, qbase, a.res, a.descale, a.cout, a.nT32, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (!rows_live) return ring_pipelined_idle<F3_BUF>(KT, dma);

    Frags2 P;
    read_frags2<Dma3::LO>(smem + wv.lane_a, smem + wv.lane_b, P);
    ring_pipelined<F3_BUF, 4>(smem, Ag, Bg, KT, wv.lane_a, wv.lane_b, P,
        [&](auto dmac, const Frags2& f, Frags2& nf, const char* ra, const char* rb, const char* srcA, const char* srcB, char* buf) {
            step2<decltype(dmac)::value>(wv.dm, f, acc, ra, rb, nf, srcA, srcB, buf);
        });
    coef_epilogue(acc, row0, kp0, jidx, d, qbase, a.out, a.bias, a.descale, a.cout, a.nT32, a.rflag, lane, flags);
}

// ---------------------------------------------------------------------------------------------------------------
// fgemm3k: fgemm3 for the two large layers (gemmf.h: fgemm_layer_k32) - its tile, work map and wave arrangement with the three products
// on v_mfma_f32_16x16x32_f16 (gemmf.h: mfma_h16, row_products32 and the 16 x 16 accumulator mapping).  Same output tile per wave, same
// MFMA cycles and same LDS read bytes as fgemm3's K16 loop; the chip holds a higher clock under this shape (profiles/fgemm_mfma_shape.md:
// the A / B of the two loops; YOHO_FGEMM_DEBUG=k16 in the experiments build brings the K16 loop back for these layers).
//
// LDS: two buffers of one whole K32 stage (A 32 KiB | B 32 KiB, both in pack order [plane 2][k-group 4][row 256][16 B], so a stage is
// eight straight 1 KiB pieces per wave), 128 KiB, one workgroup per CU as fgemm3.
// Registers: 128 accumulators (floatx4 acc[8][4]), the stage's eight B fragments twice (current and next stage: 64), the two A fragments
// of a 16-row block twice (this block and the next: 16).
// K loop, stage s in buffer s & 1: block rows 0..6 (12 MFMAs each: lo.hi, hi.lo, hi.hi on the row's four accumulators, the next row's
// two A fragments read behind the second and third); then `vmcnt(0)` + ONE barrier: every wave has all of stage s in registers and stage s + 1
// (its DMA went out a whole stage ago) has landed; behind the barrier block row 7 with the ten fragment reads that open stage s + 1 and the
// wave's eight DMA pieces of stage s + 2 into the buffer just freed.
// ---------------------------------------------------------------------------------------------------------------
constexpr int F3K_BUF = 2 * FG_STAGE;
constexpr int F3K_LDS = 2 * F3K_BUF;

struct Dma3k {
    static constexpr int NP = 8;
    int la, ldst;
    __device__ __forceinline__ Dma3k(int w8, int lane) : la(w8 * 1024 + lane * 16), ldst(w8 * 1024) {}
    template <int U>
    __device__ __forceinline__ void piece(const char* srcA, const char* srcB, char* buf) const {
        constexpr int q = (U & 3) * 8192;                                 // U = 0..3: A, 4..7: B; 8 KiB (eight waves) per piece index
        if constexpr (U < 4) __builtin_amdgcn_global_load_lds((gptr_t)(srcA + q + la), (lptr_t)(buf + q + ldst), 16, 0, 0);
        else __builtin_amdgcn_global_load_lds((gptr_t)(srcB + q + la), (lptr_t)(buf + FG_STAGE + q + ldst), 16, 0, 0);
    }
};
struct FragsA32 { uintx4 al, ah; };            // one 16-row block of a stage
struct FragsB32 { uintx4 bh[4], bl[4]; };      // the wave's four 16-column blocks of a stage

// read R (0..9) of the fragments that open a stage: A lo of block row 0, B hi x4 (products lo.hi), A hi, B lo x4
template <int R>
__device__ __forceinline__ void read_open32(const char* pa, const char* pb, FragsA32& a0, FragsB32& b) {
    if constexpr (R == 0) a0.al = *reinterpret_cast<const uintx4*>(pa + 16384);
    else if constexpr (R < 5) b.bh[R - 1] = *reinterpret_cast<const uintx4*>(pb + (R - 1) * 256);
    else if constexpr (R == 5) a0.ah = *reinterpret_cast<const uintx4*>(pa);
    else b.bl[R - 6] = *reinterpret_cast<const uintx4*>(pb + 16384 + (R - 6) * 256);
}

// block rows 0..6 of a K32 stage on B fragments `b` and A fragments read from pa (block row 0 already in fa[0])
__device__ __forceinline__ void rows32(floatx4 (&acc)[8][4], FragsA32 (&fa)[2], const FragsB32& b, const char* pa) {
    sfor<0, 7>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        row_products32(acc[i], fa[i & 1].al, fa[i & 1].ah, b.bh, b.bl, [&](auto mc) {
            constexpr int m = decltype(mc)::value;
            // not behind MFMA 0: the compiler waits with lgkmcnt(0) only, and the row's first MFMA waits for its own fragments
            if constexpr (m == 1) fa[(i + 1) & 1].al = *reinterpret_cast<const uintx4*>(pa + 16384 + (i + 1) * 256);
            if constexpr (m == 2) fa[(i + 1) & 1].ah = *reinterpret_cast<const uintx4*>(pa + (i + 1) * 256);
        });
    });
}
// the stage's one wait and barrier: every wave has all of the stage in registers, the next stage has landed
__device__ __forceinline__ void stage_barrier32() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

// One K32 stage; npa / npb: the next stage in LDS, whose opening fragments go to fa[0] / nb; DMA: the wave's pieces of the stage two
// ahead go to dmabuf (this stage's buffer); pre() runs in front of the stage's wait (the ticket of the next tile is published there)
template <bool DMA, typename Pre>
__device__ __forceinline__ void step32(const Dma3k& dm, floatx4 (&acc)[8][4], FragsA32 (&fa)[2], const FragsB32& b, FragsB32& nb, const char* pa,
                                       const char* npa, const char* npb, const char* srcA, const char* srcB, char* dmabuf, Pre&& pre) {
    rows32(acc, fa, b, pa);
    pre();
    stage_barrier32();
    row_products32(acc[7], fa[1].al, fa[1].ah, b.bh, b.bl, [&](auto mc) {
        constexpr int m = decltype(mc)::value;
        if constexpr (m < 5) {                  // two per MFMA: the next stage's first MFMA waits for all ten
            read_open32<2 * m>(npa, npb, fa[0], nb);
            read_open32<2 * m + 1>(npa, npb, fa[0], nb);
        }
        if constexpr (DMA && m >= 4) dm.template piece<m - 4>(srcA, srcB, dmabuf);
    });
}

template <bool DMA>
__device__ __forceinline__ void step32(const Dma3k& dm, floatx4 (&acc)[8][4], FragsA32 (&fa)[2], const FragsB32& b, FragsB32& nb, const char* pa,
                                       const char* npa, const char* npb, const char* srcA, const char* srcB, char* dmabuf) {
    step32<DMA>(dm, acc, fa, b, nb, pa, npa, npb, srcA, srcB, dmabuf, [] {});
}

// The last stage of a tile.  Behind its barrier every wave holds the stage in registers and BOTH buffers are dead: nothing is read from
// them any more (there is no next stage to open), and when the workgroup has a next tile (`next`, wave uniform) that tile's stages 0 and 1
// go out here, behind block row 7's MFMAs - their latency then runs under this tile's epilogue instead of in front of the next K loop.
__device__ __forceinline__ void step32_last(const Dma3k& dm, floatx4 (&acc)[8][4], FragsA32 (&fa)[2], const FragsB32& b, const char* pa, bool next,
                                            const char* nsrcA, const char* nsrcB, char* smem) {
    rows32(acc, fa, b, pa);
    stage_barrier32();
    if (next) {
        row_products32(acc[7], fa[1].al, fa[1].ah, b.bh, b.bl, [&](auto mc) {
            constexpr int m = decltype(mc)::value;
            if constexpr (m < Dma3k::NP) {
                dm.template piece<m>(nsrcA, nsrcB, smem);
                dm.template piece<m>(nsrcA + FG_STAGE, nsrcB + FG_STAGE, smem + F3K_BUF);
            }
        });
    } else {
        row_products32(acc[7], fa[1].al, fa[1].ah, b.bh, b.bl, [](auto) {});
    }
}

// A tile of the work map as its workgroup's waves see it (all wave uniform: SGPRs)
struct Tile3k {
    const char *Ag, *Bg;
    int d, KS, row0, kp0, jidx, qbase;
};
__device__ __forceinline__ bool tile3k(const FGemmArgs& a, int xcd, int slot, int w8, Tile3k& T) {
    int t = 0, local = 0, r = 0;
    if (!fg3_map(a, xcd, slot, t, local, r)) return false;
    T.d = a.dim[t];
    const int MT = a.MT[t];
    T.KS = T.d * a.cin / 32;
    const int cg = local / MT, mtile = local - cg * MT;
    const int ntile = r + 8 * cg;
    T.Ag = a.A + a.a_off[t] + (size_t)mtile * T.KS * FG_STAGE;
    T.Bg = a.B + a.b_off[t] + (size_t)ntile * T.KS * FG_STAGE;
    const int wm = (w8 & 3) >> 1, wn = w8 & 1, nh = w8 >> 2;            // Wave3's arrangement
    T.row0 = mtile * 256 + wm * 128;
    const int colbase = ntile * 256 + nh * 128 + wn * 64;
    T.jidx = colbase / a.kppad; T.kp0 = colbase - T.jidx * a.kppad; T.qbase = a.qbase[t];
    return true;
}

// Threads 0..7 issue the draw, thread x on XCD x's counter; only the workgroup's own XCD adds 1, the others add 0.  With ONE thread on an
// address the compiler knows to be wave uniform it funnels the add through a lane of its own choice and broadcasts the answer with a
// readfirstlane behind vmcnt(0): a wait for the whole round trip at the head of the K loop.  Per-lane addresses keep the answer in the
// thread's register until it is used.
__device__ __forceinline__ int draw_ticket(int* tix, int tid, int xcd) {
    return tid < 8 ? __hip_atomic_fetch_add(tix + tid, tid == xcd ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
}

constexpr int F3K_TICKET = F3K_LDS;            // LDS byte offset of the ticket word
constexpr int F3K_LDS_ALL = F3K_LDS + 16;

// Tiles per workgroup.  With FGemmArgs::tix set a workgroup runs up to FGemmArgs::tiles tiles and then retires (a workgroup that stayed
// for the whole launch would leave the other stream's kernels nothing but launch boundaries to get a CU at).  The tiles are TAKEN, one
// by one and in the work map's order: tix[x] is XCD x's next slot, drawn with a relaxed fetch-add (draw_ticket) and passed to the other
// waves through the word behind the stage buffers.  The draw for the next tile goes out at the head of this tile's K loop and is
// published in front of the second-last stage's barrier (any wait the compiler puts in front of that LDS write is the stage's own
// vmcnt(0)), so at the last stage's barrier the next tile is known and its DMA starts there (step32_last): dispatch, DMA latency,
// residual loads and the drain of this tile's stores overlap instead of adding up.  The last workgroup out (tix[8] counts them) leaves
// the counters at zero for the next launch, as gft16x does.  tix == null: one tile, static slot blockIdx.x >> 3.
__global__ __launch_bounds__(512, 2) void fgemm3k_kernel(FGemmArgs a, int flags) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w8 = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int xcd = blockIdx.x & 7;
    int* tw = reinterpret_cast<int*>(smem + F3K_TICKET);
    int slot = blockIdx.x >> 3;
    if (a.tix) {
        const int tk = draw_ticket(a.tix, tid, xcd);
        if (tid == xcd) *tw = tk;
        __syncthreads();
        slot = __builtin_amdgcn_readfirstlane(*tw);
    }
    const Dma3k dm(w8, lane);
    const int lane_a = (lane >> 4) * 4096 + (((w8 & 3) >> 1) * 128 + (lane & 15)) * 16;
    const int lane_b = FG_STAGE + (lane >> 4) * 4096 + ((w8 >> 2) * 128 + (w8 & 1) * 64 + (lane & 15)) * 16;
    auto dma = [&](const Tile3k& U, int st, int buf) {
        const char* sa = uniform_ptr(U.Ag + (size_t)st * FG_STAGE);
        const char* sb = uniform_ptr(U.Bg + (size_t)st * FG_STAGE);
        sfor<0, Dma3k::NP>([&](auto uc) { dm.template piece<decltype(uc)::value>(sa, sb, smem + buf); });
    };
    Tile3k T;
    bool have = tile3k(a, xcd, slot, w8, T);
    if (have) {                                    // KS >= 8 and even (cin >= 256, cin % 64 == 0: fgemm_layer_k32)
        dma(T, 0, 0);
        dma(T, 1, F3K_BUF);
    }
    floatx4 acc[8][4];
    for (int left = a.tix ? a.tiles : 1; have;) {
        const bool draw = --left > 0;              // this workgroup may take another tile
        zero_acc(acc);
        const bool rows_live = T.row0 < T.d * a.cout;       // else: all 128 rows of this wave are padding (launch_fgemm3: only without tickets)
        if ((flags & EPI_RES) && rows_live) residual_start(acc, T.row0, T.kp0, T.jidx, T.d, T.qbase, a.res, a.descale, a.cout, a.nT32, lane);
        // a tile behind the first: this wait also drains the previous tile's stores, which were issued behind this tile's DMA (a counted
        // wait that leaves them to the first stage's vmcnt(0) was measured and gains nothing: profiles/fgemm_multitile.md)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (!rows_live) {
            // keep the wave's share of the DMA and the barriers going: one barrier per stage, as the live waves
            for (int s = 0; s < T.KS; ++s) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                if (s + 2 < T.KS) dma(T, s + 2, (s & 1) * F3K_BUF);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            return;
        }

        FragsA32 fa[2];
        FragsB32 P, Q;
        sfor<0, 10>([&](auto rc) { read_open32<decltype(rc)::value>(smem + lane_a, smem + lane_b, fa[0], P); });
        const int tk = draw ? draw_ticket(a.tix, tid, xcd) : 0;
        int s = 0, cur = 0;
        auto run = [&](auto dmac, const FragsB32& b, FragsB32& nb, auto&& pre) {
            const int nxt = cur ^ F3K_BUF;
            if constexpr (decltype(dmac)::value)
                step32<true>(dm, acc, fa, b, nb, smem + cur + lane_a, smem + nxt + lane_a, smem + nxt + lane_b, uniform_ptr(T.Ag + (size_t)(s + 2) * FG_STAGE),
                             uniform_ptr(T.Bg + (size_t)(s + 2) * FG_STAGE), smem + cur, pre);
            else    // the last two stages stage nothing of this tile
                step32<false>(dm, acc, fa, b, nb, smem + cur + lane_a, smem + nxt + lane_a, smem + nxt + lane_b, nullptr, nullptr, nullptr, pre);
            cur = nxt; ++s;
        };
        constexpr std::true_type dmay;
        constexpr std::false_type dman;
        auto nothing = [] {};
        while (s + 2 < T.KS) {
            run(dmay, P, Q, nothing);
            run(dmay, Q, P, nothing);
        }
        run(dman, P, Q, [&] { if (draw && tid == xcd) *tw = tk; });
        Tile3k N = T;
        const bool next = draw && tile3k(a, xcd, __builtin_amdgcn_readfirstlane(*tw), w8, N);
        step32_last(dm, acc, fa, Q, smem + cur + lane_a, next, uniform_ptr(N.Ag), uniform_ptr(N.Bg), smem);
        coef_epilogue(acc, T.row0, T.kp0, T.jidx, T.d, T.qbase, a.out, a.bias, a.descale, a.cout, a.nT32, a.rflag, lane, flags);
        T = N; have = next;
    }
    if (a.tix && tid == 0) {
        // Every ticket this workgroup drew has been answered (its value was used) before it reports; the last workgroup to report leaves the
        // counters at zero.  All of it relaxed: the counters are touched by nothing but agent-scope atomics, which are carried out at the
        // memory side in the order their answers imply, and they order no other data (the next launch starts behind this kernel's end).
        // An acquire / release report costs an L2 write-back and invalidate per retiring workgroup - measured: 0.05 - 0.2 ms per launch,
        // more than the loop saves (profiles/fgemm_multitile.md).
        const int done = __hip_atomic_fetch_add(a.tix + 8, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (done == (int)gridDim.x - 1) {
#pragma unroll
            for (int x = 0; x < 9; ++x) __hip_atomic_store(a.tix + x, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// fgemm2k: fgemm2's 256 x 128 tiles and work map for the layers of fgemm_layer_k32, so that the blockings stay bit-identical: the same
// products in the same order per accumulator as fgemm3k (row_products32), on a plain loop - two buffers of one K32 stage (A 32 KiB |
// the B half tile 16 KiB [plane 2][k-group 4][col 128][16 B]), 96 KiB: one workgroup per CU.  Per stage: the stage's products with the
// fragments read as they are needed, `vmcnt(0)` + one barrier (stage s + 1 has landed, stage s is read), the DMA of stage s + 2.
// ---------------------------------------------------------------------------------------------------------------
constexpr int F2K_BUF = FG_STAGE + FG_STAGE / 2;
constexpr int F2K_LDS = 2 * F2K_BUF;

__global__ __launch_bounds__(256, 1) void fgemm2k_kernel(FGemmArgs a, int flags) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    int t = 0, local = 0, r = 0;
    if (!fg2_map(a, blockIdx.x & 7, blockIdx.x >> 3, (flags & F2_MIX) == 0, t, local, r)) return;
    const int d = a.dim[t];
    const int MT = a.MT[t], KS = d * a.cin / 32;
    const int nh = local & 1, pair = local >> 1;
    const int cg = pair / MT, mtile = pair - cg * MT;
    const int ntile = r + 8 * cg;
    const char* Ag = a.A + a.a_off[t] + (size_t)mtile * KS * FG_STAGE;
    const char* Bg = a.B + a.b_off[t] + (size_t)ntile * KS * FG_STAGE + nh * 2048;
    const int wm = w >> 1, wn = w & 1;
    const int lane_a = (lane >> 4) * 4096 + (wm * 128 + (lane & 15)) * 16;
    const int lane_b = FG_STAGE + (lane >> 4) * 2048 + (wn * 64 + (lane & 15)) * 16;

    floatx4 acc[8][4];
    zero_acc(acc);
    // a wave's share of a stage: eight 1 KiB pieces of A, four of the B half (a (plane, k-group) unit of the half is a 2 KiB run of the pack)
    auto dma = [&](int st, int buf) {
        const char* sa = uniform_ptr(Ag + (size_t)st * FG_STAGE) + lane * 16;
        const char* sb = uniform_ptr(Bg + (size_t)st * FG_STAGE) + lane * 16;
#pragma unroll
        for (int k = 0; k < 8; ++k) __builtin_amdgcn_global_load_lds((gptr_t)(sa + (k * 4 + w) * 1024), (lptr_t)(smem + buf + (k * 4 + w) * 1024), 16, 0, 0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int pb = w * 4 + k, u = pb >> 1, part = pb & 1;
            __builtin_amdgcn_global_load_lds((gptr_t)(sb + u * 4096 + part * 1024), (lptr_t)(smem + buf + FG_STAGE + u * 2048 + part * 1024), 16, 0, 0);
        }
    };
    dma(0, 0);
    if (KS > 1) dma(1, F2K_BUF);
    const int row0 = mtile * 256 + wm * 128, colbase = ntile * 256 + nh * 128 + wn * 64;
    const bool rows_live = row0 < d * a.cout;       // else: all 128 rows of this wave are padding
    const int jidx = colbase / a.kppad, kp0 = colbase - jidx * a.kppad, qbase = a.qbase[t];
    if ((flags & EPI_RES) && rows_live) residual_start(acc, row0, kp0, jidx, d, qbase, a.res, a.descale, a.cout, a.nT32, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    for (int s = 0; s < KS; ++s) {
        const int cur = (s & 1) * F2K_BUF;
        if (rows_live) stage32_plain<FG_STAGE / 4>(acc, smem + cur + lane_a, smem + cur + lane_b);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (s + 2 < KS) dma(s + 2, cur);
    }
    if (rows_live) coef_epilogue(acc, row0, kp0, jidx, d, qbase, a.out, a.bias, a.descale, a.cout, a.nT32, a.rflag, lane, flags);
}

// ---------------------------------------------------------------------------------------------------------------
// fgemm3c (gconv_mode 7, "fgemm8"; round 5, opt-in): fgemm3 with the two CORRECTION products of the fp16 split on the fp8 matrix pipe.
// A product a * w is a_h w_h + a_h w_l + a_l w_h; the corrections are 2^-11 of the main term and survive e4m3 (3 mantissa bits: 2^-15
// of the sum; tools/fp8_correction_study.py: 1.5e-5 worst relative error of the descriptor against 1.4e-6 and a tolerance of 1e-4).
// v_mfma_scale_f32_32x32x64_f8f6f4 does K = 64 at twice the fp16 rate, and ONE such MFMA takes both corrections of TWO K16 steps by
// K-concatenation:  A' = [a_h(s0) | a_l(s0) | a_h(s1) | a_l(s1)],  B' = [w_l(s0) | w_h(s0) | w_l(s1) | w_h(s1)]  (32 fp8 per lane; the
// lane's eight values of a fragment keep their place, so A' and B' pair element by element exactly like the fp16 fragments do).
// Per K16 step: 8 fp16 MFMAs + 4 fp8 MFMAs of twice the length = 2 / 3 of fgemm3's matrix time, plus 16 v_cvt_scalef32_pk_fp8_f16
// (two values each) on the activation fragments; the weight operand's fp8 fragments are packed on the host (Layer::wpg8).  The K loop is the one tools/fp8_corr_probe.hip measured (1.23-1.32 x over
// the same loop with three fp16 products): fragments of the CURRENT step read at its head, DMA two steps ahead, no hand interleaving.
// Tile shape, operand packs, LDS image, work map, residual start and epilogue are fgemm3's; the sums differ from fgemm3's in the last
// bits by construction.
// ---------------------------------------------------------------------------------------------------------------
typedef int intx8 __attribute__((ext_vector_type(8)));
typedef short shortx2 __attribute__((ext_vector_type(2)));
typedef _Float16 halfx2 __attribute__((ext_vector_type(2)));
struct Frags8 {
    intx8 a[4], b[2];          // dwords [4 p .. 4 p + 1] = hi plane (A) / lo plane (B) of the pair's step p, [4 p + 2 .. 4 p + 3] = lo (A) / hi (B)
};
// fp8 conversion scales (the conversion DIVIDES by its scale operand; powers of two throughout).  Weights: max |What| * wscale is in
// [2^9, 2^10) (pack_fgemm_weights) -> / 4 puts the hi plane below 256 (e4m3 tops out at 448); their lo plane is 2^-11 of that.
// Activations: the producer of the planes left the largest magnitude it wrote in *amax (bit pattern of a non-negative float):
// 2^k with k = floor(log2(amax)) - 7 puts it into [128, 256).  Both correction products then carry 1 / (4 * 2^k * 2^-11), undone by
// the block scales of the MFMA (E8M0, 127 = 2^0).
struct C8Scales {
    float ah = 4.f, al = 4.f / 2048.f, bh = 1.f, bl = 1.f;
    int mfma_b = 127;
    C8Scales() = default;
    __device__ __forceinline__ explicit C8Scales(const unsigned* amax) {
        const unsigned amax_bits = __builtin_amdgcn_readfirstlane(*amax);
        int kexp = (int)(amax_bits >> 23) - 127 - 7;
        kexp = kexp < -60 ? -60 : (kexp > 9 ? 9 : kexp);
        bh = __uint_as_float((unsigned)(kexp + 127) << 23); bl = __uint_as_float((unsigned)(kexp - 11 + 127) << 23);
        mfma_b = 127 + kexp;
    }
};
struct Int2 { int x, y; };
// eight fp16 (one fragment) / scale -> eight fp8 e4m3 (two dwords)
__device__ __forceinline__ Int2 frag_to_fp8(uintx4 f, float scale) {
    union { unsigned u; halfx2 h; } p0, p1, p2, p3;
    p0.u = f[0]; p1.u = f[1]; p2.u = f[2]; p3.u = f[3];
    shortx2 r = {0, 0}, q = {0, 0};
    r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(r, p0.h, scale, false);
    r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(r, p1.h, scale, true);
    q = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(q, p2.h, scale, false);
    q = __builtin_amdgcn_cvt_scalef32_pk_fp8_f16(q, p3.h, scale, true);
    Int2 o;
    __builtin_memcpy(&o.x, &r, 4);
    __builtin_memcpy(&o.y, &q, 4);
    return o;
}

// the products of one K16 step of a pair (PAR = 0, 1) on its fragments: main product on the fp16 pipe, the fragments into half PAR of the
// fp8 operands, and behind the pair's second step the eight fp8 MFMAs that take both corrections of both steps
template <int PAR>
__device__ __forceinline__ void step3c(const Frags2& f, floatx16 (&acc)[4][2], Frags8& c8, const C8Scales& sc) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma_h(f.ah[i], f.bh[j], acc[i][j]);
    // the weight operand's fp8 fragments come ready-made: fgemm3c's weight pack (Layer::wpg8) carries, in the place of the lo plane, the
    // 16 bytes [e4m3(hi / 4) x 8 | e4m3(lo * 512) x 8] of every (row, k-group) unit - exactly this step's four dwords of A'
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) c8.a[i][4 * PAR + e] = (int)f.al[i][e];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const Int2 l = frag_to_fp8(f.bl[j], sc.bl), h = frag_to_fp8(f.bh[j], sc.bh);
        c8.b[j][4 * PAR] = l.x; c8.b[j][4 * PAR + 1] = l.y; c8.b[j][4 * PAR + 2] = h.x; c8.b[j][4 * PAR + 3] = h.y;
    }
    if constexpr (PAR == 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(c8.a[i], c8.b[j], acc[i][j], 0, 0, 0, 127 + 2 - 11, 0, sc.mfma_b);
    }
}

// The plain ring (fgemm3c, cgemm) behind a prologue that staged steps 0 and 1.  Step s lives in ring buffer s % 3.  At the head of step
// s: its DMA (issued two steps ago) has landed - the four pieces issued one step ago may stay in flight -, one barrier, then the DMA of
// step s + 2 goes into the buffer every wave finished reading BEFORE that barrier (step s - 1's), the twelve fragments of step s are read,
// and the products are issued: the two waves of a SIMD cover each other's fragment latency (tools/fp8_corr_probe.hip: this plain loop
// runs the three-product arithmetic as fast as fgemm3's hand-interleaved one).  Past the end the last step is staged again (into a
// buffer nobody reads any more): uniform counted waits.  bsrc(s) = B source of step s; FP8: corrections on the fp8 pipe (step3c).
template <bool FP8, typename BSrc>
__device__ __forceinline__ void ring_plain(floatx16 (&acc)[4][2], char* smem, const Wave3& wv, const char* Ag, BSrc&& bsrc, int KT, bool rows_live,
                                           const C8Scales& sc) {
    Frags8 c8;
    if constexpr (FP8) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) c8.a[i][e] = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 8; ++e) c8.b[j][e] = 0;
    }
    int cur = 0, stg = 2 * F3_BUF;                // buffer of step s, buffer the DMA of step s + 2 goes to
    int s = 0;
    auto stage = [&] {
        const int s2 = s + 2 < KT ? s + 2 : KT - 1;
        dma_step(wv.dm, uniform_ptr(Ag + step_off(s2)), uniform_ptr(bsrc(s2)), smem + stg);
    };
    auto rotate = [&] { stg = cur; cur = cur == 2 * F3_BUF ? 0 : cur + F3_BUF; ++s; };      // (s + 3) % 3 == s % 3
    auto one_step = [&](auto parity) {
        asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        stage();
        Frags2 f;
        read_frags2<Dma3::LO>(smem + cur + wv.lane_a, smem + cur + wv.lane_b, f);
        if constexpr (FP8) step3c<decltype(parity)::value>(f, acc, c8, sc);
        else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = mfma_h(f.al[i], f.bh[j], acc[i][j]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = mfma_h(f.ah[i], f.bl[j], acc[i][j]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = mfma_h(f.ah[i], f.bh[j], acc[i][j]);
        }
        rotate();
    };
    if (rows_live) {
        for (int it = 0; it < KT; it += 2) {     // KT is even
            one_step(std::integral_constant<int, 0>{});
            one_step(std::integral_constant<int, 1>{});
        }
    } else {
        // all 128 rows of this wave are padding: keep its share of the DMA and the barriers going
        for (int it = 0; it < KT; ++it) {
            asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            stage();
            rotate();
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the re-staged tail pieces must not land in the LDS of the next workgroup
}

__global__ __launch_bounds__(512, 2) void fgemm3c_kernel(FGemmArgs a, int flags) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const Wave3 wv(__builtin_amdgcn_readfirstlane(tid >> 6), lane);
    int t = 0, local = 0, r = 0;
    if (!fg3_map(a, blockIdx.x & 7, blockIdx.x >> 3, t, local, r)) return;
    const int d = a.dim[t];
    const int MT = a.MT[t], KS = d * a.cin / 32, KT = 2 * KS;
    const int cg = local / MT, mtile = local - cg * MT;
    const int ntile = r + 8 * cg;
    const char* Ag = a.A + a.a_off[t] + (size_t)mtile * KS * FG_STAGE;
    const char* Bg = a.B + a.b_off[t] + (size_t)ntile * KS * FG_STAGE;

    floatx16 acc[4][2];
    zero_acc(acc);
    const C8Scales sc(a.amax);
    dma_step(wv.dm, Ag, Bg, smem);
    dma_step(wv.dm, Ag + step_off(1), Bg + step_off(1), smem + F3_BUF);
    const int row0 = mtile * 256 + wv.wm * 128, colbase = ntile * 256 + wv.nh * 128 + wv.wn * 64;
    const bool rows_live = row0 < d * a.cout;       // else: all 128 rows of this wave are padding (cout = 32)
    const int jidx = colbase / a.kppad, kp0 = colbase - jidx * a.kppad, qbase = a.qbase[t];
    if ((flags & EPI_RES) && rows_live) residual_start(acc, row0, kp0, jidx, d, qbase, a.res, a.descale, a.cout, a.nT32, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    ring_plain<true>(acc, smem, wv, Ag, [&](int s) { return Bg + step_off(s); }, KT, rows_live, sc);
    if (rows_live) coef_epilogue(acc, row0, kp0, jidx, d, qbase, a.out, a.bias, a.descale, a.cout, a.nT32, a.rflag, lane, flags);
}

// ---------------------------------------------------------------------------------------------------------------
// cgemm (round 6): PartII's 13-element cone layer (utils/network.py:243-249,23-65 evaluated only where the g = 0 output needs it) as ONE
// implicit GEMM on fgemm3c's K loop:
//     y[o, (j, m)] = sum_k sum_c W[o, c, k] * act[c, N[n_j][k], m]        M = cout = 512, N = 13 output elements x matches, K = 13 taps x cin
// The "gather" of the 13-tap group convolution is a choice of B-operand STAGE BLOCK per (output element j, tap k): the producer
// (gft16_kernel<G16_INVG>) leaves the activated first-layer output as [column tile of 256 matches][cone slot][32-channel block] x 32 KiB in
// exactly the image an LDS stage wants, so a K step's B half is still one straight LDS-DMA copy - only its base moves with the tap
// (a.slot: slot of N[n_j][k], 169 bytes).  A = the layer's weights as a plain [cout][tap * cin + c] matrix in fgemm's A pack (hi plane +
// fp8 correction operand in place of the lo plane for FP8, hi + lo planes else).  Tile shape, LDS image, DMA, fragment reads and the
// products are fgemm3c's / fgemm3's (three fp16 products, or one fp16 product + the two corrections on the fp8 pipe); the epilogue
// applies bias, the next layer's BN + ReLU and writes fp16x2 planes in the layout cone1_kernel stages from
// ([tile16][c8][plane][60 slabs][16 matches][8 ch], slab n_j).  Replaces gconv16_kernel<7,4,2> in PartII modes 2 / 3 / 4 (fp16x2 products: on cgemmk_kernel's K32 stage loop, below): no tap-pair or
// unit padding (14 / 13 twice), both operands blocked through LDS.
// ---------------------------------------------------------------------------------------------------------------
struct CGemmArgs {
    const char* A;            // [mtile][tap * KSt + cb][32 KiB]
    const char* B;            // [column tile][slot][cb][32 KiB]
    const float* bias;
    const float* bn_s;
    const float* bn_t;
    char* out;                // cone1 planes
    int NTm, MT, KSt, ntap, nj, nslot, c8out, nT32, nTiles16;
    float descale;
    int* rflag;
    const unsigned* amax;     // FP8: largest |B plane value| (float bit pattern) left by the producer
    unsigned char slot[13 * 13];
    unsigned char outg[16];
};

__device__ __forceinline__ void cg_split_pair(float x0, float x1, unsigned& hi, unsigned& lo) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    f2 x;
    x.x = x0; x.y = x1;
    const halfx2 h = __builtin_convertvector(x, halfx2);
    const f2 r = x - __builtin_convertvector(h, f2);
    const halfx2 l = __builtin_convertvector(r, halfx2);
    __builtin_memcpy(&hi, &h, 4);
    __builtin_memcpy(&lo, &l, 4);
}

template <bool FP8>
__global__ __launch_bounds__(512, 2) void cgemm_kernel(CGemmArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int tapoff[16];
    const int tid = threadIdx.x, lane = tid & 63;
    const Wave3 wv(__builtin_amdgcn_readfirstlane(tid >> 6), lane);
    // work map: both row tiles of a column tile are neighbours on one XCD (the B panel is served from that XCD's L2 to the second one)
    const int xcd = blockIdx.x & 7, slot_ = blockIdx.x >> 3;
    const int ct = xcd + 8 * (slot_ / a.MT), mtile = slot_ % a.MT;
    if (ct >= a.nj * a.NTm) return;
    const int j = ct / a.NTm, mt = ct - j * a.NTm;
    const int SPT = 2 * a.KSt;                                           // K16 steps per tap
    const int KT = a.ntap * SPT;
    if (tid < 16) tapoff[tid] = tid < a.ntap ? (int)a.slot[j * 13 + tid] : 0;
    const char* Ag = a.A + (size_t)mtile * (KT / 2) * FG_STAGE;
    const char* Bt = a.B + (size_t)mt * a.nslot * a.KSt * FG_STAGE;      // this column tile's slots
    __syncthreads();
    auto bsrc = [&](int s) -> const char* {
        const int tap = s / SPT, within = s - tap * SPT;
        const int sl = __builtin_amdgcn_readfirstlane(tapoff[tap]);
        return Bt + (size_t)sl * a.KSt * FG_STAGE + step_off(within);
    };

    floatx16 acc[4][2];
    zero_acc(acc);
    C8Scales sc;
    if constexpr (FP8) sc = C8Scales(a.amax);
    dma_step(wv.dm, Ag, uniform_ptr(bsrc(0)), smem);
    dma_step(wv.dm, Ag + step_off(1), uniform_ptr(bsrc(1)), smem + F3_BUF);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    ring_plain<FP8>(acc, smem, wv, Ag, bsrc, KT, true, sc);            // cout % 256 == 0: no padding waves

    // ---- epilogue: D[row][col]: lane (col = lane & 31, half = lane >> 5), reg e -> row = (e & 3) + 8 * (e >> 2) + 4 * half.
    // v = acc * descale + bias; the next layer's BN + ReLU; x H2_ASCALE; hi / lo planes; 8 bytes (4 channels) per plane and lane
    const int half = lane >> 5, c32 = lane & 31;
    const int g = a.outg[j];
    unsigned top = 0u;
#pragma unroll
    for (int bi = 0; bi < 2; ++bi) {
        const int m = mt * 256 + wv.nh * 128 + wv.wn * 64 + bi * 32 + c32;     // match
        // columns past the last 32-match tile were never written by the inverse transform (stale or foreign bytes): skipped before
        // they reach the range word, as in fgemm3c
        if ((m >> 5) >= a.nT32 || (m >> 4) >= a.nTiles16) continue;
#pragma unroll
        for (int ai = 0; ai < 4; ++ai) {
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int o = mtile * 256 + wv.wm * 128 + ai * 32 + q4 * 8 + half * 4;
                const floatx4 b4 = *reinterpret_cast<const floatx4*>(a.bias + o);
                const floatx4 s4 = *reinterpret_cast<const floatx4*>(a.bn_s + o);
                const floatx4 t4 = *reinterpret_cast<const floatx4*>(a.bn_t + o);
                float y[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = acc[ai][bi][4 * q4 + e] * a.descale + b4[e];
                    y[e] = fmaxf(v * s4[e] + t4[e], 0.f) * H2_ASCALE;
                    top = max(top, __float_as_uint(y[e]) & 0x7FFFFFFFu);
                }
                unsigned h0, l0, h1, l1;
                cg_split_pair(y[0], y[1], h0, l0);
                cg_split_pair(y[2], y[3], h1, l1);
                char* dst = a.out + (((size_t)(m >> 4) * a.c8out + (o >> 3)) * 2) * 15360 + g * 256 + (m & 15) * 16 + half * 8;
                *reinterpret_cast<uint2*>(dst) = uint2{h0, h1};
                *reinterpret_cast<uint2*>(dst + 15360) = uint2{l0, l1};
            }
        }
    }
    note_range_bits(a.rflag, top, FP16_MAX);
}

// ---------------------------------------------------------------------------------------------------------------
// cgemmk: the fp16x2 cone GEMM (cgemm_kernel<false>'s work map, operand packs and sums) on fgemm3k's K32 stage loop: step32 with
// row_products32 on v_mfma_f32_16x16x32_f16, two whole-stage buffers (128 KiB), one barrier per stage, the DMA one stage ahead.  The
// packs are K32-stage blocks of 32 KiB already, so a stage is still eight straight 1 KiB pieces per wave; the B stage base is chosen per
// K32 stage: a tap is KSt = cin / 32 whole stages, so the tap's slot is constant within a stage (stage s: tap s / KSt, channel block
// s % KSt).  K = 13 taps x cin is the longest K loop of the project (104 stages for cin = 256).  The stages come in pairs (the two B
// fragment sets trade places): ntap * KSt must be even, launch_cgemm keeps the K16 kernel otherwise.
// Epilogue on the 16 x 16 accumulator mapping (gemmf.h): lane (col = lane & 15, g = lane >> 4), reg e -> row = 4 g + e: the four registers
// of a lane are four consecutive output channels (second four of their eight when g is odd) of ONE match, 8 bytes per plane, and a
// 16-column tile is one 16-match tile of cone1's planes; bias, BN + ReLU, H2_ASCALE, the hi / lo split and the range word as cgemm_kernel.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512, 2) void cgemmk_kernel(CGemmArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int tapoff[16];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w8 = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int xcd = blockIdx.x & 7, slot_ = blockIdx.x >> 3;                // cgemm_kernel's work map
    const int ct = xcd + 8 * (slot_ / a.MT), mtile = slot_ % a.MT;
    if (ct >= a.nj * a.NTm) return;
    const int j = ct / a.NTm, mt = ct - j * a.NTm;
    const int KS = a.ntap * a.KSt;                                       // K32 stages (even, launch_cgemm)
    if (tid < 16) tapoff[tid] = tid < a.ntap ? (int)a.slot[j * 13 + tid] : 0;
    const char* Ag = a.A + (size_t)mtile * KS * FG_STAGE;
    const char* Bt = a.B + (size_t)mt * a.nslot * a.KSt * FG_STAGE;      // this column tile's slots
    __syncthreads();
    auto bsrc = [&](int st) -> const char* {
        const int tap = st / a.KSt, cb = st - tap * a.KSt;
        const int sl = __builtin_amdgcn_readfirstlane(tapoff[tap]);
        return uniform_ptr(Bt + ((size_t)sl * a.KSt + cb) * FG_STAGE);
    };
    const int wm = (w8 & 3) >> 1, wn = w8 & 1, nh = w8 >> 2;            // Wave3's arrangement
    const Dma3k dm(w8, lane);
    const int lane_a = (lane >> 4) * 4096 + (wm * 128 + (lane & 15)) * 16;
    const int lane_b = FG_STAGE + (lane >> 4) * 4096 + (nh * 128 + wn * 64 + (lane & 15)) * 16;

    floatx4 acc[8][4];
    zero_acc(acc);
    auto dma = [&](int st, int buf) {
        const char* sa = uniform_ptr(Ag + (size_t)st * FG_STAGE);
        const char* sb = bsrc(st);
        sfor<0, Dma3k::NP>([&](auto uc) { dm.template piece<decltype(uc)::value>(sa, sb, smem + buf); });
    };
    dma(0, 0);
    dma(1, F3K_BUF);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    FragsA32 fa[2];
    FragsB32 P, Q;
    sfor<0, 10>([&](auto rc) { read_open32<decltype(rc)::value>(smem + lane_a, smem + lane_b, fa[0], P); });
    int s = 0, cur = 0;
    auto run = [&](auto dmac, const FragsB32& b, FragsB32& nb) {
        const int nxt = cur ^ F3K_BUF;
        if constexpr (decltype(dmac)::value)
            step32<true>(dm, acc, fa, b, nb, smem + cur + lane_a, smem + nxt + lane_a, smem + nxt + lane_b, uniform_ptr(Ag + (size_t)(s + 2) * FG_STAGE),
                         bsrc(s + 2), smem + cur);
        else    // the last two stages stage nothing; behind the last one the "next" fragments are read from the other buffer and never used
            step32<false>(dm, acc, fa, b, nb, smem + cur + lane_a, smem + nxt + lane_a, smem + nxt + lane_b, nullptr, nullptr, nullptr);
        cur = nxt; ++s;
    };
    constexpr std::true_type dmay;
    constexpr std::false_type dman;
    while (s + 2 < KS) {
        run(dmay, P, Q);
        run(dmay, Q, P);
    }
    run(dman, P, Q);
    run(dman, Q, P);

    // ---- epilogue: v = acc * descale + bias; the next layer's BN + ReLU; x H2_ASCALE; hi / lo planes; 8 bytes (4 channels) per plane and lane
    // (the lane is made opaque here: the store addresses derived from it must not be hoisted above the K loop, whose registers are full)
    int etid = threadIdx.x;
    asm volatile("" : "+v"(etid));
    const int g4 = (etid >> 4) & 3, c16 = etid & 15;
    const int g = a.outg[j];
    const int col0 = mt * 256 + nh * 128 + wn * 64;
    unsigned top = 0u;
#pragma unroll
    for (int ai = 0; ai < 8; ++ai) {
        const int o = mtile * 256 + wm * 128 + ai * 16 + g4 * 4;
        const floatx4 b4 = *reinterpret_cast<const floatx4*>(a.bias + o);
        const floatx4 s4 = *reinterpret_cast<const floatx4*>(a.bn_s + o);
        const floatx4 t4 = *reinterpret_cast<const floatx4*>(a.bn_t + o);
#pragma unroll
        for (int bi = 0; bi < 4; ++bi) {
            const int m0 = col0 + bi * 16;                                // first match of the 16-column tile (wave uniform)
            // columns past the last 32-match tile were never written by the inverse transform (stale or foreign bytes): skipped before
            // they reach the range word, as in cgemm_kernel
            if ((m0 >> 5) >= a.nT32 || (m0 >> 4) >= a.nTiles16) continue;
            float y[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = acc[ai][bi][e] * a.descale + b4[e];
                y[e] = fmaxf(v * s4[e] + t4[e], 0.f) * H2_ASCALE;
                top = max(top, __float_as_uint(y[e]) & 0x7FFFFFFFu);
            }
            unsigned h0, l0, h1, l1;
            cg_split_pair(y[0], y[1], h0, l0);
            cg_split_pair(y[2], y[3], h1, l1);
            char* dst = a.out + (((size_t)(m0 >> 4) * a.c8out + (o >> 3)) * 2) * 15360 + g * 256 + c16 * 16 + (g4 & 1) * 8;
            *reinterpret_cast<uint2*>(dst) = uint2{h0, h1};
            *reinterpret_cast<uint2*>(dst + 15360) = uint2{l0, l1};
        }
    }
    note_range_bits(a.rflag, top, FP16_MAX);
}

int cgemm_init() {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&cgemm_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, F3_LDS));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&cgemm_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, F3_LDS));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&cgemmk_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, F3K_LDS));
    return 0;
}

// the cone layer L (cin -> cout, 13 taps) on M matches: Bstages as launch_gft16_invg left them, out = cone1's input planes;
// slot[j * 13 + k] = cone slot of N[n_j][k], outg[j] = n_j; amax != null selects the fp8-correction kernel (needs L.wcg8)
int launch_cgemm(const Layer& L, const char* Bstages, int nslot, const unsigned char* slot, const unsigned char* outg, int nT32, int nTiles16,
                 char* out, hipStream_t s, int* rflag, const unsigned* amax) {
    const bool fp8 = amax != nullptr;
    if (!(fp8 ? L.wcg8 : L.wcg) || L.cin % 32 || L.cout % 256) { set_error("cgemm: needs the cone-GEMM weight pack, cin %% 32 == 0, cout %% 256 == 0"); return YOHO_EINVAL; }
    if (nT32 == 0) return 0;
    CGemmArgs a;
    a.A = reinterpret_cast<const char*>(fp8 ? L.wcg8 : L.wcg); a.B = Bstages; a.bias = L.bias; a.bn_s = L.bn_s; a.bn_t = L.bn_t; a.out = out;
    a.NTm = (nT32 + 7) / 8; a.MT = L.cout / 256; a.KSt = L.cin / 32; a.ntap = 13; a.nj = 13; a.nslot = nslot; a.c8out = L.cout / 8;
    a.nT32 = nT32; a.nTiles16 = nTiles16; a.descale = L.wcg_descale; a.rflag = rflag; a.amax = amax;
    std::memcpy(a.slot, slot, 169);
    std::memset(a.outg, 0, 16);
    std::memcpy(a.outg, outg, 13);
    const int CT = a.nj * a.NTm;
    const int grid = 8 * ((CT + 7) / 8) * a.MT;
    // the fp16x2 products run on the K32 stage loop (cgemmk_kernel; profiles/cone_gemm_k32.md); YOHO_FGEMM_DEBUG=k16 in the experiments
    // build brings the K16 loop back, as for fgemm3k.  The fp8 corrections keep their loop.
    const char* dbg = experiment_env("YOHO_FGEMM_DEBUG");
    const bool k32 = !fp8 && (a.ntap * a.KSt) % 2 == 0 && !(dbg && std::strstr(dbg, "k16"));
    if (fp8) hipLaunchKernelGGL(cgemm_kernel<true>, dim3(grid), dim3(512), F3_LDS, s, a);
    else if (k32) hipLaunchKernelGGL(cgemmk_kernel, dim3(grid), dim3(512), F3K_LDS, s, a);
    else hipLaunchKernelGGL(cgemm_kernel<false>, dim3(grid), dim3(512), F3_LDS, s, a);
    HIPCHK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// fgemm3s: fgemm3's staging and K loop for layers with 32 output channels (32 d <= 160 live rows of the 256-row A tile).  In
// fgemm3 the waves are arranged 2 (rows) x 4 (columns): the lower row half is padding, so half the waves - two of the four
// SIMDs - idle and the other two issue 24 MFMAs per step on 128 rows of which 32 d are real.  Here the eight waves split the
// 256 columns (32 each) and every wave holds the d live 32-row tiles: 3 d MFMAs per wave and step on all four SIMDs, the same
// products in the same order per accumulator (bit-identical coefficients).
// ---------------------------------------------------------------------------------------------------------------
struct Frags3s {
    uintx4 ah[5], al[5], bh, bl;
};

// fragment read R (0..11) of a step, in the order of use: A lo x5, B hi, A hi x5, B lo
template <int R>
__device__ __forceinline__ void read_frag3s(const char* pa, const char* pb, Frags3s& f) {
    if constexpr (R < 5) f.al[R] = *reinterpret_cast<const uintx4*>(pa + 8192 + R * 512);
    else if constexpr (R == 5) f.bh = *reinterpret_cast<const uintx4*>(pb);
    else if constexpr (R < 11) f.ah[R - 6] = *reinterpret_cast<const uintx4*>(pa + (R - 6) * 512);
    else f.bl = *reinterpret_cast<const uintx4*>(pb + 8192);
}

// One K16 step: 3 d MFMAs on `f` (lo.hi, hi.lo, hi.hi per accumulator, as fgemm3); behind them the 12 fragment reads of the next
// step (rows beyond 32 d are padding: read, never used) and the wave's four DMA pieces of the step three ahead.
template <bool DMA, int D>
__device__ __forceinline__ void step3s(const Frags3s& f, floatx16 (&acc)[5][1], const char* ra, const char* rb, Frags3s& nf,
                                       const char* srcA, const char* srcB, char* dmabuf, const Dma3& dm) {
    sfor<0, 5>([&](auto gc) {
        constexpr int g = decltype(gc)::value;
        if constexpr (g < D) acc[g][0] = mfma_h(f.al[g], f.bh, acc[g][0]);
        if constexpr (g < D) read_frag3s<g>(ra, rb, nf);
        if constexpr (g == 4) read_frag3s<5>(ra, rb, nf);
        __builtin_amdgcn_sched_barrier(0);
    });
    sfor<0, 5>([&](auto gc) {
        constexpr int g = decltype(gc)::value;
        if constexpr (g < D) acc[g][0] = mfma_h(f.ah[g], f.bl, acc[g][0]);
        if constexpr (g < D) read_frag3s<6 + g>(ra, rb, nf);
        if constexpr (g == 4) read_frag3s<11>(ra, rb, nf);
        __builtin_amdgcn_sched_barrier(0);
    });
    sfor<0, 5>([&](auto gc) {
        constexpr int g = decltype(gc)::value;
        if constexpr (g < D) acc[g][0] = mfma_h(f.ah[g], f.bh, acc[g][0]);
        if constexpr (DMA && g < 4) dm.template piece<g>(srcA, srcB, dmabuf);
        __builtin_amdgcn_sched_barrier(0);
    });
}

// K loop of fgemm3s for an irrep of dimension D (compile time: no branches around the MFMAs, no reads of padding rows)
template <int D>
__device__ __forceinline__ void fgemm3s_kloop(floatx16 (&acc)[5][1], char* smem, const char* Ag, const char* Bg, int KT, const Dma3& dm, int lane_a, int lane_b) {
    Frags3s P;
    sfor<0, 12>([&](auto rc) {
        constexpr int R = decltype(rc)::value;
        if constexpr (R == 5 || R == 11 || (R < 5 && R < D) || (R > 5 && R < 11 && R - 6 < D)) read_frag3s<R>(smem + lane_a, smem + lane_b, P);
    });
    ring_pipelined<F3_BUF, 4>(smem, Ag, Bg, KT, lane_a, lane_b, P,
        [&](auto dmac, const Frags3s& f, Frags3s& nf, const char* ra, const char* rb, const char* srcA, const char* srcB, char* buf) {
            step3s<decltype(dmac)::value, D>(f, acc, ra, rb, nf, srcA, srcB, buf, dm);
        });
}

__global__ __launch_bounds__(512, 2) void fgemm3s_kernel(FGemmArgs a, int flags) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w8 = __builtin_amdgcn_readfirstlane(tid >> 6);
    int t = 0, local = 0, r = 0;
    if (!fg3_map(a, blockIdx.x & 7, blockIdx.x >> 3, t, local, r)) return;
    const int d = a.dim[t];
    const int KS = d * a.cin / 32, KT = 2 * KS;                        // MT = 1: the tile holds all 32 d rows
    const int ntile = r + 8 * local;
    const char* Ag = a.A + a.a_off[t];
    const char* Bg = a.B + a.b_off[t] + (size_t)ntile * KS * FG_STAGE;
    const Dma3 dm(w8, lane);
    const int lane_a = (lane >> 5) * 4096 + (lane & 31) * 16;
    const int lane_b = 16384 + (lane >> 5) * 4096 + (w8 * 32 + (lane & 31)) * 16;

    floatx16 acc[5][1];
    zero_acc(acc);
    ring_prologue<F3_BUF>(KT, [&](int st, int buf) { dma_step(dm, uniform_ptr(Ag + step_off(st)), uniform_ptr(Bg + step_off(st)), smem + buf); });
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    switch (d) {
        case 1: fgemm3s_kloop<1>(acc, smem, Ag, Bg, KT, dm, lane_a, lane_b); break;
        case 3: fgemm3s_kloop<3>(acc, smem, Ag, Bg, KT, dm, lane_a, lane_b); break;
        case 4: fgemm3s_kloop<4>(acc, smem, Ag, Bg, KT, dm, lane_a, lane_b); break;
        default: fgemm3s_kloop<5>(acc, smem, Ag, Bg, KT, dm, lane_a, lane_b); break;
    }
    // 32 output channels (launch_fgemm3): row tile ai of the wave is coefficient row i = ai; the experiments build honours `nostore` alone here
    const int colbase = ntile * 256 + w8 * 32;
    const int jidx = colbase / a.kppad, kp0 = colbase - jidx * a.kppad;
    coef_epilogue(acc, 0, kp0, jidx, d, a.qbase[t], a.out, a.bias, a.descale, 32, a.nT32, a.rflag, lane, flags & F2_NOSTORE);
}

int fgemm3_init() {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&fgemm3_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, F3_LDS));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&fgemm3s_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, F3_LDS));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&fgemm3c_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, F3_LDS));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&fgemm3k_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, F3K_LDS_ALL));
    return 0;
}

int launch_fgemm3(const FGemmArgs& a, int flags, hipStream_t s) {
    if (const char* dbg = experiment_env("YOHO_FGEMM_DEBUG")) {
        if (std::strstr(dbg, "nostore")) flags |= F2_NOSTORE;
        if (std::strstr(dbg, "sc1")) flags |= F2_ST_SC1;            // round 6: the coefficient stores write-through ...
        if (std::strstr(dbg, "stnt")) flags |= F2_ST_NT;            // ... or non-temporal: produced once, consumed once by gft16x
    }
    const int tot = fgemm_grid(a, 1);
    // 32 output channels, no residual: all 32 d live rows in every wave (fgemm3s); YOHO_FGEMM_DEBUG=nosmall keeps fgemm3
    static const bool small_ok = [] { const char* e = experiment_env("YOHO_FGEMM_DEBUG"); return !(e && std::strstr(e, "nosmall")); }();
    if (small_ok && a.cout == 32 && !(flags & EPI_RES)) hipLaunchKernelGGL(fgemm3s_kernel, dim3(tot), dim3(512), F3_LDS, s, a, flags);
    else if (a.amax) hipLaunchKernelGGL(fgemm3c_kernel, dim3(tot), dim3(512), F3_LDS, s, a, flags);      // gconv_mode 7: corrections on the fp8 pipe
    else if (flags & F2_K32) {
        // several tiles per workgroup (fgemm3k_kernel): 8 x ceil(longest XCD list / R) workgroups draw their slots from a.tix.  Every wave of
        // such a workgroup must have live rows (cout % 256 == 0: the kernel's idle waves leave at their tile's end); R = 1 is the static map
        FGemmArgs k = a;
        if (const char* dbg = experiment_env("YOHO_FGEMM_DEBUG"))
            if (const char* e = std::strstr(dbg, "tiles=")) k.tiles = std::atoi(e + 6);
        k.tiles = k.tiles < 1 ? 1 : (k.tiles > FGEMM_TILES_MAX ? FGEMM_TILES_MAX : k.tiles);
        if (k.tiles == 1 || k.cout % 256) { k.tix = nullptr; k.tiles = 1; }
        // Workgroups per XCD: ceil(longest list / R) have room for every tile, but a workgroup takes its R tiles one after the other, so
        // with exactly that many the last ones dispatched walk the end of the list alone while the CUs around them have nothing left to
        // start (measured: + 8 % on 512 -> 256 at R = 4).  One spare workgroup per other CU of the XCD keeps every CU supplied as long as
        // tickets remain; a spare that finds none retires at once.
        // A list no longer than the XCD's CUs keeps the static map: every tile has a CU to itself, a second tile in a workgroup only waits.
        static const int cu_xcd = [] {
            int dev = 0, n = 0;
            return hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n >= 8 ? n / 8 : 32;
        }();
        if (tot / 8 <= cu_xcd) { k.tix = nullptr; k.tiles = 1; }
        const int need = (tot / 8 + k.tiles - 1) / k.tiles + cu_xcd - 1;
        const int grid = k.tix ? 8 * (need < tot / 8 ? need : tot / 8) : tot;
        hipLaunchKernelGGL(fgemm3k_kernel, dim3(grid), dim3(512), F3K_LDS_ALL, s, k, flags);
    }
    else hipLaunchKernelGGL(fgemm3_kernel, dim3(tot), dim3(512), F3_LDS, s, a, flags);
    HIPCHK(hipGetLastError());
    return 0;
}

int fgemm2_init() {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&fgemm2_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, F2_LDS));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&fgemm2k_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, F2K_LDS));
    return fgemm3_init();
}

int launch_fgemm2(const FGemmArgs& a, int flags, hipStream_t s) {
    if (const char* dbg = experiment_env("YOHO_FGEMM_DEBUG")) {          // kernel-timing experiments only (results are not valid with nostore)
        if (std::strstr(dbg, "nostore")) flags |= F2_NOSTORE;       // no coefficient stores at all (K loops alone)
        if (std::strstr(dbg, "mix")) flags |= F2_MIX;               // slots alternate between the d = 5 irrep and the others
        if (std::strstr(dbg, "sc1")) flags |= F2_ST_SC1;            // write-through stores that do not stay in the L2
        if (std::strstr(dbg, "nt")) flags |= F2_ST_NT;              // non-temporal stores
        if (std::strstr(dbg, "sparse4")) flags |= F2_SPARSE4;
        if (std::strstr(dbg, "sparse16")) flags |= F2_SPARSE16;
    }
    if (flags & F2_K32) hipLaunchKernelGGL(fgemm2k_kernel, dim3(fgemm_grid(a, 2)), dim3(256), F2K_LDS, s, a, flags);
    else hipLaunchKernelGGL(fgemm2_kernel, dim3(fgemm_grid(a, 2)), dim3(256), F2_LDS, s, a, flags);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace yoho
