// FCGF backbone, floating-point side: everything that multiplies.  A convolution is output-stationary over a kernel map (spmaps.hip):
// a 32-row tile gathers its input rows offset by offset and accumulates all output channels on the MFMA; BN, residual, ReLU and the
// channel concatenation (a column offset of a wider buffer) are the epilogue.  launch_spconv picks the kernel:
//
//   spconv16w_kernel<1|2|4>      default, fine levels (>= 1024 row tiles): fp16x2 split products (lo*hi + hi*lo + hi*hi on
//                                v_mfma_f32_32x32x16_f16, fp32 accumulation), four tiles per workgroup in lockstep, the weight
//                                fragments through a double-buffered LDS stage, the gathers through a raw buffer descriptor in a
//                                register ring; <1> also normalises the rows of the feature head in its epilogue;
//   spconv16s_kernel<2,2|1,3>    default, coarse levels: one tile per workgroup, the (offset, chunk) loop split over its four waves;
//   spconv_kernel<NCB, SPLIT>    YOHO_FCGF=f32: the same two decompositions on v_mfma_f32_32x32x2_f32, gathers from global memory;
//   spconv_small_kernel          fewer than 32 input channels, plain fp32.
// Tiles skip the kernel offsets none of their rows reaches (exact zeros: identical bits), which the parity-sorted row orders of the
// transposed convolutions make the common case.  The first convolution on the constant-one input needs no map (launch_conv1:
// conv1_mfma / conv1_bitmap over the level-0 occupancy bitmaps, conv1_ones over the hash table); heads_fused_kernel runs the
// decoder's two 1 x 1 heads and the normalisation in one launch; row_normalize_kernel is the staged normalisation.
#include <algorithm>

#include "sparse.h"

namespace yoho {

typedef float floatx16s __attribute__((ext_vector_type(16)));

// Offsets that no row of a tile reaches are skipped (their rows of the A operand are all zero: the skipped MFMAs would add
// exact zeros, so the sums are bit-identical).  The mask has one bit per kernel offset; iteration is in ascending order.
__device__ __forceinline__ int sp_next_offset(unsigned& mask) {
    const int k = __builtin_ctz(mask);
    mask &= mask - 1;
    return k;
}

// The ReLU of every epilogue: IEEE maximum (one v_maximum3_f32), which hands a NaN on.  Not fmaxf: that answers a NaN with 0, and a NaN
// is what an activation past the range of the fp16 planes (split_pair_sp) makes of the rows it reaches - it has to arrive at the caller.
// Every other value gets the bits fmaxf gave it (-0 -> +0 included).
__device__ __forceinline__ float sp_relu(float v) { return __builtin_elementwise_maximum(v, 0.f); }
// the same as a maximum with a floor picked outside the loop: 0, or -inf where the layer has no ReLU (the identity, NaN included) - no
// branch and no select per value in the fine-level epilogue
__device__ __forceinline__ float sp_floor(float v, float lo) { return __builtin_elementwise_maximum(v, lo); }

// NCB = 32-channel output blocks per wave.  SPLIT = false: every wave of the workgroup owns its own 32 output rows.
// SPLIT = true (coarse levels: few rows, many channels): the four waves share one 32-row tile and split the
// (kernel offset, channel chunk) loop four ways; the partial sums meet in LDS and are added in wave order.
// The input rows of the whole kernel region are looked up once (K <= 27 indices per row, kept in LDS); the gathered
// A values and the weight fragment of step i+1 are loaded while the MFMAs of step i issue (register ping-pong).
template <int NCB, bool SPLIT>
__global__ __launch_bounds__(256) void spconv_kernel(SpConvArgs a) {
    __shared__ int srcl[4][SP_MAXK * 32];
    __shared__ float red[SPLIT ? 3 * NCB * 16 * 64 : 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int li = lane & 31, h = lane >> 5;
    const int rbase = SPLIT ? blockIdx.x * 32 : (blockIdx.x * 4 + w) * 32;
    if (!SPLIT && rbase >= a.nout) return;
    const int cb0 = blockIdx.y * NCB;                      // this workgroup's first 32-channel output block
    const int row = rbase + li;
    const bool valid = row < a.nout;
    int* sl = srcl[w];
    for (int k = h; k < a.K; k += 2) sl[k * 32 + li] = valid ? (a.map ? a.map[(size_t)k * a.nout + row] : row) : -1;
    __builtin_amdgcn_wave_barrier();

    floatx16s acc[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[cb][r] = 0.f;
    const int nchunk = a.cin / 32;
    const int total = a.K * nchunk;
    const int it0 = SPLIT ? (total * w) / 4 : 0, it1 = SPLIT ? (total * (w + 1)) / 4 : total;

    auto issue = [&](int it, float (&av)[16], float (&bv)[16 * NCB]) {
        const int k = it / nchunk, cc = it - k * nchunk;
        const int src = sl[k * 32 + li];
        const float* ip = a.in + (size_t)(src < 0 ? 0 : src) * a.ldin + cc * 32 + h * 16;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (src >= 0) v = *reinterpret_cast<const float4*>(ip + 4 * q);
            av[4 * q] = v.x; av[4 * q + 1] = v.y; av[4 * q + 2] = v.z; av[4 * q + 3] = v.w;
        }
        const float* wp = a.W + ((size_t)k * a.cin + cc * 32 + h * 16) * a.cout + cb0 * 32 + li;
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) bv[kk * NCB + cb] = wp[(size_t)kk * a.cout + cb * 32];
    };
    auto mma = [&](const float (&av)[16], const float (&bv)[16 * NCB]) {
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kk], bv[kk * NCB + cb], acc[cb], 0, 0, 0);
    };
    float a0[16], a1[16], b0[16 * NCB], b1[16 * NCB];
    if (it0 < it1) issue(it0, a0, b0);
    for (int it = it0; it < it1; it += 2) {
        if (it + 1 < it1) issue(it + 1, a1, b1);
        mma(a0, b0);
        if (it + 1 < it1) {
            if (it + 2 < it1) issue(it + 2, a0, b0);
            mma(a1, b1);
        }
    }
    if (SPLIT) {
        if (w > 0) {
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[(((w - 1) * NCB + cb) * 16 + r) * 64 + lane] = acc[cb][r];
        }
        __syncthreads();
        if (w > 0) return;
#pragma unroll
        for (int ww = 0; ww < 3; ++ww)
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[cb][r] += red[((ww * NCB + cb) * 16 + r) * 64 + lane];
    }
    // D[i = row][j = channel]: lane (j = lane & 31, half = lane >> 5), reg r -> row = (r & 3) + 8 (r >> 2) + 4 half
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
        const int co = (cb0 + cb) * 32 + li;
        const float s = a.aff_s ? a.aff_s[co] : 1.f, t = a.aff_t ? a.aff_t[co] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int orow = rbase + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (orow < a.nout) {
                float v = acc[cb][r] * s + t;
                if (a.res) v += a.res[(size_t)orow * a.ldres + a.rcoff + co];
                if (a.relu) v = sp_relu(v);
                a.out[(size_t)orow * a.ldout + a.ocoff + co] = v;
            }
        }
    }
}

// fp16x2 split variant (same decomposition as spconv_kernel): every product as lo*hi + hi*lo + hi*hi on
// v_mfma_f32_32x32x16_f16 with fp32 accumulation (3 MFMAs at 16x the fp32-MFMA rate, error <= 3 * 2^-22 per product).
// The gathered fp32 rows are split in registers (x * 16 = hi + lo; activations must stay below 4094: from 4095 on hi is infinite, lo and the row's sums NaN); the weights are
// split once at load time and stored in B-fragment order
//     Wh[k][chunk32][K16 step 2][plane 2][cout block][lane = 32 kg + j][8]  =  W[k][32 chunk + 16 step + 8 kg + e][32 cb + j]
// so a fragment is one 16-byte load per lane.
typedef unsigned uintx4s __attribute__((ext_vector_type(4)));
typedef _Float16 halfx8s __attribute__((ext_vector_type(8)));
typedef _Float16 halfx2s __attribute__((ext_vector_type(2)));
typedef float floatx2s __attribute__((ext_vector_type(2)));
constexpr float SP_ASCALE = 16.f;

__device__ __forceinline__ floatx16s mfma_sp16(uintx4s a, uintx4s b, floatx16s c) {
    union { uintx4s u; halfx8s h; } ca, cb;
    ca.u = a; cb.u = b;
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(ca.h, cb.h, c, 0, 0, 0);
}
__device__ __forceinline__ void split_pair_sp(float x0, float x1, unsigned& hi, unsigned& lo) {
    floatx2s x;
    x.x = x0 * SP_ASCALE; x.y = x1 * SP_ASCALE;
    const halfx2s h = __builtin_convertvector(x, halfx2s);
    const floatx2s r = x - __builtin_convertvector(h, floatx2s);
    const halfx2s l = __builtin_convertvector(r, halfx2s);
    __builtin_memcpy(&hi, &h, 4);
    __builtin_memcpy(&lo, &l, 4);
}

// Gathered input rows are read through a raw buffer descriptor over [in, in + 2 GiB): a lane whose region cell is empty
// uses an out-of-range offset and gets zeros without a memory access and without a branch (branches around loads make
// the compiler drain vmcnt at every join, which serialises the load pipeline).
constexpr unsigned SP_OOB = 0x80000000u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t sp_rsrc(const float* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, 0x7FFFFFFF, 0x00020000);
}
__device__ __forceinline__ void sp_gather16(__amdgpu_buffer_rsrc_t rs, unsigned off, float (&av)[16]) {
    // K16 step s uses channels 32 cc + 16 s + 8 h + e: two 32-byte runs of this lane's input row (off points at 32 cc + 8 h)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uintx4s v = __builtin_amdgcn_raw_buffer_load_b128(rs, off, ((q >> 1) * 16 + (q & 1) * 4) * 4, 0);
        __builtin_memcpy(&av[4 * q], &v, 16);      // not v.x .. v.w: hipcc 7.2 then narrows the load to one dword and replicates it
    }
}

// Coarse levels (few rows, many channels): the four waves share one 32-row tile and split the (offset, chunk) loop four
// ways, each fetching its own weight fragments; the partial sums meet in LDS and are added in wave order.
template <int NCB, int ND>
__global__ __launch_bounds__(256) void spconv16s_kernel(SpConvArgs a) {
    __shared__ int srcl[4][SP_MAXK * 32];
    __shared__ float red[3 * NCB * 16 * 64];
    __shared__ int prow[32];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int li = lane & 31, h = lane >> 5;
    const int rbase = blockIdx.x * 32;
    const int cb0 = blockIdx.y * NCB;
    const int slot = rbase + li;
    int row = -1;
    if (slot < a.nslots) row = a.rowperm ? a.rowperm[slot] : slot;
    const bool valid = row >= 0;
    if (w == 0 && h == 0) prow[li] = row;
    int* sl = srcl[w];
    unsigned actl = 0u;                                                   // offsets reached by any row of the tile (every wave computes it)
    for (int k = h; k < a.K; k += 2) {
        const int v = valid ? (a.map ? a.map[(size_t)k * a.nout + row] : row) : -1;
        sl[k * 32 + li] = v;
        const unsigned long long b = __ballot(v >= 0);
        if ((unsigned)b) actl |= 1u << (k - h);
        if (b >> 32) actl |= 2u << (k - h);
    }
    const unsigned act = __builtin_amdgcn_readfirstlane(actl) | __builtin_amdgcn_readlane(actl, 32);
    __builtin_amdgcn_wave_barrier();

    floatx16s acc[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[cb][r] = 0.f;
    const int nchunk = a.cin / 32, ncbt = a.cout / 32;
    const int total = a.K * nchunk;
    const int it0 = (total * w) / 4, it1 = (total * (w + 1)) / 4;
    const uintx4s* Wh = reinterpret_cast<const uintx4s*>(a.Wh);

    // Loads are branch-free (empty cells: out-of-range buffer offset; steps past the end re-read the last one): the
    // compiler's vmcnt bookkeeping only keeps loads in flight across straight-line code.
    // this wave's steps: those of [it0, it1) whose offset is active, in ascending order (the fixed ranges keep the order
    // in which the partial sums meet independent of what the tile skips)
    int nit = 0, ik = 0, icc = 0, issued = 0;                            // wave-uniform position of the load pointer
    for (unsigned m = act; m;) {
        const int k = sp_next_offset(m);
        const int lo = max(it0, k * nchunk), hi = min(it1, (k + 1) * nchunk);
        if (hi > lo) {
            if (nit == 0) { ik = k; icc = lo - k * nchunk; }
            nit += hi - lo;
        }
    }
    auto next_active = [&](int k) { return __builtin_ctz(act & ~((2u << k) - 1u)); };
    const __amdgpu_buffer_rsrc_t rs = sp_rsrc(a.in);
    auto issue = [&](float (&av)[16], uintx4s (&bv)[4 * NCB]) {
        const int src = sl[ik * 32 + li];
        sp_gather16(rs, src < 0 ? SP_OOB : ((unsigned)src * (unsigned)a.ldin + icc * 32 + h * 8) * 4u, av);
        const uintx4s* wp = Wh + ((size_t)(ik * nchunk + icc) * 4 * ncbt + cb0) * 64 + lane;    // [it][step][plane][cb][lane]
#pragma unroll
        for (int sp = 0; sp < 4; ++sp)
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) bv[sp * NCB + cb] = wp[((size_t)sp * ncbt + cb) * 64];
        if (++issued < nit && ++icc == nchunk) { icc = 0; ik = next_active(ik); }
    };
    auto mma = [&](const float (&av)[16], const uintx4s (&bv)[4 * NCB]) {
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            uintx4s ah, al;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                unsigned hh, ll;
                split_pair_sp(av[8 * st + 2 * p], av[8 * st + 2 * p + 1], hh, ll);
                ah[p] = hh; al[p] = ll;
            }
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) acc[cb] = mfma_sp16(al, bv[(2 * st + 0) * NCB + cb], acc[cb]);
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) acc[cb] = mfma_sp16(ah, bv[(2 * st + 1) * NCB + cb], acc[cb]);
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) acc[cb] = mfma_sp16(ah, bv[(2 * st + 0) * NCB + cb], acc[cb]);
        }
    };
    // register ring: the loads of step i + ND - 1 are in flight behind the MFMAs of step i (the gathers come from the
    // MALL / a remote L2, 1-2 us away, and a coarse level has only a few waves per SIMD to hide that)
    if (nit > 0) {
        float av[ND][16];
        uintx4s bv[ND][4 * NCB];
#pragma unroll
        for (int j = 0; j < ND - 1; ++j) issue(av[j], bv[j]);
        const int nmain = (nit / ND) * ND;
        for (int it = 0; it < nmain; it += ND) {
#pragma unroll
            for (int j = 0; j < ND; ++j) {
                issue(av[(j + ND - 1) % ND], bv[(j + ND - 1) % ND]);
                mma(av[j], bv[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < ND - 1; ++j)
            if (nmain + j < nit) mma(av[j], bv[j]);              // already loaded by the ring
    }
    if (w > 0) {
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) red[(((w - 1) * NCB + cb) * 16 + r) * 64 + lane] = acc[cb][r];
    }
    __syncthreads();
    if (w > 0) return;
#pragma unroll
    for (int ww = 0; ww < 3; ++ww)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[cb][r] += red[((ww * NCB + cb) * 16 + r) * 64 + lane];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
        const int co = (cb0 + cb) * 32 + li;
        const float s = (a.aff_s ? a.aff_s[co] : 1.f) * a.descale, t = a.aff_t ? a.aff_t[co] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int orow = prow[(r & 3) + 8 * (r >> 2) + 4 * h];
            if (orow >= 0) {
                float v = acc[cb][r] * s + t;
                if (a.res) v += a.res[(size_t)orow * a.ldres + a.rcoff + co];
                if (a.relu) v = sp_relu(v);
                a.out[(size_t)orow * a.ldout + a.ocoff + co] = v;
            }
        }
    }
}

// Fine levels (many rows): the four waves of a workgroup own four 32-row tiles and walk the (offset, chunk) steps in
// lockstep, so the weight fragments of a step (4 NCB KiB) are shared: every thread fetches NCB 16-byte pieces two steps
// ahead, they go through a double-buffered LDS stage (one barrier per step) and each wave reads its fragments from
// there - the vector-memory pipe only carries the gathers (a quarter of the bytes of the per-wave weight loads).
// The gathered rows run NA - 1 steps ahead in a register ring.
template <int NCB, int NA>
__device__ __forceinline__ void spconv16w_body(const SpConvArgs& a) {
    // one LDS block: region rows of the four waves | double-buffered weight stage; the epilogue lays its output tiles over it
    constexpr int SRCL_INTS = 4 * SP_MAXK * 32, BST_FRAGS = 2 * 4 * NCB * 64, EPI_LD = 36;       // EPI_LD: padded row of 32 floats
    static_assert(SRCL_INTS * 4 + BST_FRAGS * 16 >= 4 * 32 * EPI_LD * 4, "epilogue tiles must fit");
    __shared__ __attribute__((aligned(16))) char smem[SRCL_INTS * 4 + BST_FRAGS * 16];
    __shared__ int prow[4][32];
    __shared__ unsigned actm;
    int (*srcl)[SP_MAXK * 32] = reinterpret_cast<int (*)[SP_MAXK * 32]>(smem);
    uintx4s (*bst)[4 * NCB * 64] = reinterpret_cast<uintx4s (*)[4 * NCB * 64]>(smem + SRCL_INTS * 4);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int li = lane & 31, h = lane >> 5;
    const int rbase = (blockIdx.x * 4 + w) * 32;
    const int cb0 = blockIdx.y * NCB;
    const int slot = rbase + li;
    int row = -1;
    if (slot < a.nslots) row = a.rowperm ? a.rowperm[slot] : slot;
    const bool valid = row >= 0;
    int* sl = srcl[w];
    if (tid == 0) actm = 0u;
    if (h == 0) prow[w][li] = row;
    __syncthreads();
    {
        // all map reads of the tile in flight at once (half h holds offsets h, h + 2, ...), then the LDS copies and the ballots
        constexpr int NV = (SP_MAXK + 1) / 2;
        int v[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int k = 2 * j + h;
            v[j] = (valid && k < a.K) ? (a.map ? a.map[(size_t)k * a.nout + row] : row) : -1;
        }
        unsigned m = 0u;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int k = 2 * j + h;
            if (k < SP_MAXK) sl[k * 32 + li] = v[j];
            const unsigned long long b = __ballot(v[j] >= 0);        // low half: offset 2 j, high half: 2 j + 1
            if ((unsigned)b) m |= 1u << (2 * j);
            if (b >> 32) m |= 2u << (2 * j);
        }
        if (m && li == 0) atomicOr(&actm, m);
    }
    __syncthreads();
    const unsigned act = __builtin_amdgcn_readfirstlane(actm);        // offsets reached by any of the workgroup's 128 rows
    if (act == 0u && __syncthreads_or(valid) == 0) return;            // padding only

    floatx16s acc[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[cb][r] = 0.f;
    const int nchunk = a.cin / 32, ncbt = a.cout / 32;
    const int total = __builtin_popcount(act) * nchunk;
    const uintx4s* Wh = reinterpret_cast<const uintx4s*>(a.Wh);

    if (total > 0 && !(a.debug & 1)) {
        // branch-free loads, see spconv16_kernel
        unsigned amask = act, bmask = act;                                    // wave-uniform load pointers
        int ak = sp_next_offset(amask), acc_ = 0, aissued = 0;
        int bk = sp_next_offset(bmask), bcc = 0, bissued = 0;
        const __amdgpu_buffer_rsrc_t rs = sp_rsrc(a.in);
        auto loadA = [&](float (&av)[16]) {
            const int src = sl[ak * 32 + li];
            sp_gather16(rs, src < 0 ? SP_OOB : ((unsigned)src * (unsigned)a.ldin + acc_ * 32 + h * 8) * 4u, av);
            if (++aissued < total && ++acc_ == nchunk) { acc_ = 0; ak = sp_next_offset(amask); }
        };
        // stage image = [step-plane 4][cb NCB][lane 64] fragments; piece j of this thread = image index j * 256 + tid
        auto loadB = [&](uintx4s (&br)[NCB]) {
            const int it = bk * nchunk + bcc;                                 // past the end: the last step again
#pragma unroll
            for (int j = 0; j < NCB; ++j) {
                const int idx = j * 256 + tid, sp = idx / (NCB * 64), within = idx - sp * (NCB * 64);
                br[j] = Wh[(((size_t)it * 4 + sp) * ncbt + cb0) * 64 + within];
            }
            if (++bissued < total && ++bcc == nchunk) { bcc = 0; bk = sp_next_offset(bmask); }
        };
        auto storeB = [&](int buf, const uintx4s (&br)[NCB]) {
#pragma unroll
            for (int j = 0; j < NCB; ++j) bst[buf][j * 256 + tid] = br[j];
        };
        auto mma = [&](const float (&av)[16], int buf) {
            const uintx4s* bl = &bst[buf][lane];
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                uintx4s ah, al, bh[NCB], bw[NCB];
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) { bh[cb] = bl[((2 * st + 0) * NCB + cb) * 64]; bw[cb] = bl[((2 * st + 1) * NCB + cb) * 64]; }
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    unsigned hh, ll;
                    split_pair_sp(av[8 * st + 2 * p], av[8 * st + 2 * p + 1], hh, ll);
                    ah[p] = hh; al[p] = ll;
                }
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) acc[cb] = mfma_sp16(al, bh[cb], acc[cb]);
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) acc[cb] = mfma_sp16(ah, bw[cb], acc[cb]);
#pragma unroll
                for (int cb = 0; cb < NCB; ++cb) acc[cb] = mfma_sp16(ah, bh[cb], acc[cb]);
            }
        };
        static_assert(NA % 2 == 0, "the stage parity of ring slot j is j & 1");
        float av[NA][16];
        uintx4s br[2][NCB];
        loadB(br[0]);
        loadB(br[1]);
#pragma unroll
        for (int j = 0; j < NA - 1; ++j) loadA(av[j]);
        storeB(0, br[0]);
        // step s: barrier (stage s & 1 complete, the other one free) -> weights of s + 1 into the free stage, fetch the
        // weights of s + 2 and the rows of s + NA - 1, MFMAs of s
        const int nmain = (total / NA) * NA;
        for (int it = 0; it < nmain; it += NA) {
#pragma unroll
            for (int j = 0; j < NA; ++j) {
                __syncthreads();
                storeB((j + 1) & 1, br[(j + 1) & 1]);
                loadB(br[j & 1]);
                loadA(av[(j + NA - 1) % NA]);
                mma(av[j], j & 1);
            }
        }
#pragma unroll
        for (int j = 0; j < NA - 1; ++j) {
            if (nmain + j < total) {                                          // uniform over the workgroup
                __syncthreads();
                storeB((j + 1) & 1, br[(j + 1) & 1]);
                loadB(br[j & 1]);
                mma(av[j], j & 1);
            }
        }
    }
    if (a.debug & 2) return;
    // Epilogue through LDS: the accumulator tile (a lane holds one channel of 16 rows) is turned into rows of 32 channels, so
    // that eight lanes move one row's 128 bytes with 16-byte accesses (residual read, affine, ReLU, store).
    __syncthreads();                                                      // every wave is done with the stage buffers
    float* et = reinterpret_cast<float*>(smem) + w * 32 * EPI_LD;
    const int er = lane >> 3, ep = lane & 7;                              // row within a group of eight, 4-channel piece
    const float relu_lo = a.relu ? 0.f : -__builtin_inff();
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
        if (cb) __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 16; ++r) et[((r & 3) + 8 * (r >> 2) + 4 * h) * EPI_LD + li] = acc[cb][r];
        __builtin_amdgcn_wave_barrier();
        const int co = (cb0 + cb) * 32 + 4 * ep;
        float4 sc = make_float4(a.descale, a.descale, a.descale, a.descale), sh = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.aff_s) { const float4 t = *reinterpret_cast<const float4*>(a.aff_s + co); sc.x *= t.x; sc.y *= t.y; sc.z *= t.z; sc.w *= t.w; }
        if (a.aff_t) sh = *reinterpret_cast<const float4*>(a.aff_t + co);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int orow = prow[w][8 * g + er];
            if (orow >= 0) {
                float4 v = *reinterpret_cast<const float4*>(et + (8 * g + er) * EPI_LD + 4 * ep);
                v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y; v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
                if (a.res) {
                    const float4 rr = *reinterpret_cast<const float4*>(a.res + (size_t)orow * a.ldres + a.rcoff + co);
                    v.x += rr.x; v.y += rr.y; v.z += rr.z; v.w += rr.w;
                }
                v.x = sp_floor(v.x, relu_lo); v.y = sp_floor(v.y, relu_lo); v.z = sp_floor(v.z, relu_lo); v.w = sp_floor(v.w, relu_lo);
                size_t drow = (size_t)orow;
                if constexpr (NCB == 1) {
                    if (a.norm) {
                        // the feature head: a row's 32 channels sit in the eight lanes of its group (4 each) - unit-normalise here
                        // (resunet.py:183-187, once more in fcgf_feat.py:48) instead of a pass of its own over the (n, 32) matrix
                        for (int pass = 0; pass < a.norm; ++pass) {
                            float ss = fmaf(v.x, v.x, v.y * v.y) + fmaf(v.z, v.z, v.w * v.w);      // explicit: the compiler's contraction must not differ between the two places this is written
                            ss += __shfl_xor(ss, 1); ss += __shfl_xor(ss, 2); ss += __shfl_xor(ss, 4);
                            const float nr = sqrtf(ss);
                            v.x /= nr; v.y /= nr; v.z /= nr; v.w /= nr;
                        }
                        if (a.operm) drow = (size_t)a.operm[orow];
                    }
                }
                *reinterpret_cast<float4*>(a.out + drow * a.ldout + a.ocoff + co) = v;
            }
        }
    }
}

// Ring depth and register budget per variant, measured on the 15-copy pass (NOTEBOOK 3.5, round 4: 8.61 -> 8.36 ms, same bits):
// with the gathers only one step ahead (ring 2) the 64-channel kernel fits 4 waves per SIMD (102 registers instead of 148 -> 3) and
// the 128-channel one 3 (156 instead of 204 -> 2), and the extra resident workgroup hides more than the deeper ring did; forcing the
// budget with the ring of 4 spills (9.36 ms), a ring of 6 at 3 waves is slower too (8.76), the 32-channel kernel does not care
// (ring 2 at 5 waves 8.60, ring 4 at 4 waves as it was)
constexpr int sp_ring(int ncb) { return ncb == 1 ? 4 : 2; }
constexpr int sp_wpe(int ncb) { return ncb == 4 ? 3 : 4; }
template <int NCB>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(sp_wpe(NCB), sp_wpe(NCB)))) void spconv16w_kernel(SpConvArgs a) {
    spconv16w_body<NCB, sp_ring(NCB)>(a);
}

// The decoder's two 1 x 1 heads in one kernel (resunet.py:181-187): f1 = relu(conv1_tr(x)) (32 NC1 -> 64 channels), out = final(f1) + bias
// (64 -> 32), rows /= |row| `norm` times, the caller's row order.  As two launches of spconv16w_kernel the 64-channel intermediate is
// written and read back once (2 x 336 MB of the 1.35 GB the two move per 1.3 M-voxel pass; both are HBM-bound).  Here it stays in LDS:
// the accumulator tile of the first head (a lane = one channel of 16 rows) is written as rows, and read back in the A-operand
// layout the gathers deliver (a lane = 8 + 8 channels of one row).  Both weight packs (24 + 8 KiB) stay in LDS for the life of the
// workgroup, which walks 128-row tiles with a stride of the grid.  The same products in the same order, the same epilogue
// expressions as the two launches: identical bits.
template <int NC1>
__global__ __launch_bounds__(256) void heads_fused_kernel(HeadsArgs a) {
    constexpr int W1F = NC1 * 4 * 2 * 64, W2F = 2 * 4 * 64, LD1 = 68, EPI_LD = 36;
    __shared__ uintx4s w1s[W1F];
    __shared__ uintx4s w2s[W2F];
    __shared__ __attribute__((aligned(16))) float tile[4][32 * LD1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int li = lane & 31, h = lane >> 5;
    for (int i = tid; i < W1F; i += 256) w1s[i] = reinterpret_cast<const uintx4s*>(a.W1)[i];
    for (int i = tid; i < W2F; i += 256) w2s[i] = reinterpret_cast<const uintx4s*>(a.W2)[i];
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rs = sp_rsrc(a.in);
    float* et = tile[w];
    const int er = lane >> 3, ep = lane & 7;
    const int ntiles = (a.n + 127) / 128;
    // the rows of the next tile are fetched while this one is multiplied (a wave's tile is a dependent chain gather -> MFMA -> LDS -> MFMA
    // -> store, and only eight waves share a CU)
    float avn[NC1][16];
    auto fetch = [&](int t) {
        const int row = t * 128 + w * 32 + li;
        const bool valid = t < ntiles && row < a.n;
#pragma unroll
        for (int cc = 0; cc < NC1; ++cc) sp_gather16(rs, valid ? ((unsigned)row * (unsigned)a.ldin + cc * 32 + h * 8) * 4u : SP_OOB, avn[cc]);
    };
    fetch(blockIdx.x);
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int rbase = t * 128 + w * 32;
        float av[NC1][16];
#pragma unroll
        for (int cc = 0; cc < NC1; ++cc)
#pragma unroll
            for (int e = 0; e < 16; ++e) av[cc][e] = avn[cc][e];
        fetch(t + gridDim.x);
        floatx16s acc1[2];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc1[cb][r] = 0.f;
#pragma unroll
        for (int cc = 0; cc < NC1; ++cc) {
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                uintx4s ah, al, bh[2], bw[2];
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) { bh[cb] = w1s[((cc * 4 + 2 * st + 0) * 2 + cb) * 64 + lane]; bw[cb] = w1s[((cc * 4 + 2 * st + 1) * 2 + cb) * 64 + lane]; }
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    unsigned hh, ll;
                    split_pair_sp(av[cc][8 * st + 2 * p], av[cc][8 * st + 2 * p + 1], hh, ll);
                    ah[p] = hh; al[p] = ll;
                }
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) acc1[cb] = mfma_sp16(al, bh[cb], acc1[cb]);
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) acc1[cb] = mfma_sp16(ah, bw[cb], acc1[cb]);
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) acc1[cb] = mfma_sp16(ah, bh[cb], acc1[cb]);
            }
        }
        // f1 = relu(acc * descale + 0) as the first launch's epilogue writes it, kept as rows of 64 channels
        {
            const float sc = a.descale1, sh = 0.f;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float v = acc1[cb][r];
                    v = v * sc + sh;
                    et[((r & 3) + 8 * (r >> 2) + 4 * h) * LD1 + cb * 32 + li] = sp_relu(v);
                }
        }
        __builtin_amdgcn_wave_barrier();
        floatx16s acc2;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[r] = 0.f;
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            float a2[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 v = *reinterpret_cast<const float4*>(et + li * LD1 + cc * 32 + h * 8 + (q >> 1) * 16 + (q & 1) * 4);
                a2[4 * q] = v.x; a2[4 * q + 1] = v.y; a2[4 * q + 2] = v.z; a2[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                uintx4s ah, al;
                const uintx4s bh = w2s[(cc * 4 + 2 * st + 0) * 64 + lane], bw = w2s[(cc * 4 + 2 * st + 1) * 64 + lane];
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    unsigned hh, ll;
                    split_pair_sp(a2[8 * st + 2 * p], a2[8 * st + 2 * p + 1], hh, ll);
                    ah[p] = hh; al[p] = ll;
                }
                acc2 = mfma_sp16(al, bh, acc2);
                acc2 = mfma_sp16(ah, bw, acc2);
                acc2 = mfma_sp16(ah, bh, acc2);
            }
        }
        __builtin_amdgcn_wave_barrier();                                  // every lane has read its row of f1
#pragma unroll
        for (int r = 0; r < 16; ++r) et[((r & 3) + 8 * (r >> 2) + 4 * h) * EPI_LD + li] = acc2[r];
        __builtin_amdgcn_wave_barrier();
        {
            const int co = 4 * ep;
            float4 sc = make_float4(a.descale2, a.descale2, a.descale2, a.descale2), sh = make_float4(0.f, 0.f, 0.f, 0.f);
            if (a.bias2) sh = *reinterpret_cast<const float4*>(a.bias2 + co);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int orow = rbase + 8 * g + er;
                if (orow < a.n) {
                    float4 v = *reinterpret_cast<const float4*>(et + (8 * g + er) * EPI_LD + 4 * ep);
                    v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y; v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
                    size_t drow = (size_t)orow;
                    if (a.norm) {
                        for (int pass = 0; pass < a.norm; ++pass) {
                            float ss = fmaf(v.x, v.x, v.y * v.y) + fmaf(v.z, v.z, v.w * v.w);      // as in spconv16w_body's epilogue
                            ss += __shfl_xor(ss, 1); ss += __shfl_xor(ss, 2); ss += __shfl_xor(ss, 4);
                            const float nr = sqrtf(ss);
                            v.x /= nr; v.y /= nr; v.z /= nr; v.w /= nr;
                        }
                        if (a.operm) drow = (size_t)a.operm[orow];
                    }
                    *reinterpret_cast<float4*>(a.out + drow * 32 + co) = v;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();                                  // the tile is written again by the next iteration
    }
}

// Cin < 32 (the first convolution: one input channel, 5^3 / 7^3 offsets): plain fp32, one thread per (row, channel)
__global__ __launch_bounds__(256) void spconv_small_kernel(SpConvArgs a) {
    const int co = threadIdx.x % a.cout, rl = threadIdx.x / a.cout;
    const int rows_per = 256 / a.cout;
    const int row = blockIdx.x * rows_per + rl;
    if (rl >= rows_per || row >= a.nout) return;
    float acc = 0.f;
    constexpr int UB = 7;                                  // offsets per batch: independent map / feature loads in flight
    for (int k0 = 0; k0 < a.K; k0 += UB) {
        int src[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) src[u] = (k0 + u < a.K) ? (a.map ? a.map[(size_t)(k0 + u) * a.nout + row] : row) : -1;
        for (int c = 0; c < a.cin; ++c) {
            float xv[UB], wv[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                xv[u] = src[u] >= 0 ? a.in[(size_t)src[u] * a.ldin + c] : 0.f;
                wv[u] = (k0 + u < a.K) ? a.W[((size_t)(k0 + u) * a.cin + c) * a.cout + co] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) acc = fmaf(xv[u], wv[u], acc);
        }
    }
    float v = acc * (a.aff_s ? a.aff_s[co] : 1.f) + (a.aff_t ? a.aff_t[co] : 0.f);
    if (a.res) v += a.res[(size_t)row * a.ldres + a.rcoff + co];
    if (a.relu) v = sp_relu(v);
    a.out[(size_t)row * a.ldout + a.ocoff + co] = v;
}

// First convolution with the constant-one input feature (simple_yoho/fcgf_feat.py:41, one input channel, 32 outputs):
//     out[n][co] = sum over the occupied voxels of the K^3 region of W[k][0][co]
// fused with the neighbourhood lookup: a half-wave owns one output row, its 32 lanes probe the hash table for 32 kernel
// offsets at a time (ballot), then every lane (= output channel) adds the weights of the occupied offsets in kernel-index
// order from an LDS copy of W.  No K^3 x N kernel map is written or read.
__global__ __launch_bounds__(256) void conv1_ones_kernel(const int* __restrict__ coords, int n, const u64* __restrict__ keys, unsigned mask,
                                                         int ksize, const float* __restrict__ W, const float* __restrict__ aff_s,
                                                         const float* __restrict__ aff_t, float* __restrict__ out) {
    __shared__ float Wl[C1O_MAXK * 32];
    const int kv = ksize * ksize * ksize, hk = ksize / 2;
    for (int i = threadIdx.x; i < kv * 32; i += 256) Wl[i] = W[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, l32 = lane & 31, hw = lane >> 5;
    const int row = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + hw;
    const bool valid = row < n;
    const int4 c = valid ? reinterpret_cast<const int4*>(coords)[row] : make_int4(0, 0, 0, 0);
    float acc = 0.f;
    for (int k0 = 0; k0 < kv; k0 += 32) {
        const int k = k0 + l32;
        bool present = false;
        if (valid && k < kv) {
            const int ox = k % ksize - hk, oy = (k / ksize) % ksize - hk, oz = k / (ksize * ksize) - hk;
            present = hash_find_slot(keys, mask, pack_key(c.x + ox, c.y + oy, c.z + oz, c.w)) >= 0;
        }
        const unsigned long long m64 = __ballot(present);
        unsigned m = hw ? (unsigned)(m64 >> 32) : (unsigned)m64;
        while (m) {
            const int j = __ffs(m) - 1;
            m &= m - 1;
            acc += Wl[(k0 + j) * 32 + l32];
        }
    }
    if (valid) out[(size_t)row * 32 + l32] = acc * (aff_s ? aff_s[l32] : 1.f) + (aff_t ? aff_t[l32] : 0.f);
}

// Persistent workgroups (the 44 KiB weight table is loaded into LDS once per workgroup, not once per 8 rows); a half-wave
// owns a row per round.  All ceil(K^3 / 32) bitmap words of a row are requested before the first one is used.
constexpr int C1B_NIT = (C1O_MAXK + 31) / 32;
__global__ __launch_bounds__(256) void conv1_bitmap_kernel(const int* __restrict__ coords, int n, const BmDesc* __restrict__ desc,
                                                           const unsigned* __restrict__ bm, int ksize, const float* __restrict__ W,
                                                           const float* __restrict__ aff_s, const float* __restrict__ aff_t,
                                                           float* __restrict__ out) {
    __shared__ float Wl[(C1O_MAXK + 1) * 32];
    __shared__ int koff[C1B_NIT * 32];                   // offset k -> dx | dy << 8 | dz << 16 (each 0 .. K-1), -1 past the end
    const int kv = ksize * ksize * ksize, hk = ksize / 2;
    for (int i = threadIdx.x; i < kv * 32; i += 256) Wl[i] = W[i];
    if (threadIdx.x < 32) Wl[C1O_MAXK * 32 + threadIdx.x] = 0.f;
    for (int k = threadIdx.x; k < C1B_NIT * 32; k += 256)
        koff[k] = k < kv ? (k % ksize) | (((k / ksize) % ksize) << 8) | ((k / (ksize * ksize)) << 16) : -1;
    __syncthreads();
    const int lane = threadIdx.x & 63, l32 = lane & 31, hw = lane >> 5;
    const int nit = (kv + 31) / 32;
    const float sc = aff_s ? aff_s[l32] : 1.f, sh = aff_t ? aff_t[l32] : 0.f;
    for (int pair = blockIdx.x * 4 + (threadIdx.x >> 6); pair * 2 < n; pair += gridDim.x * 4) {
        const int row = pair * 2 + hw;
        const bool valid = row < n;
        const int4 c = valid ? reinterpret_cast<const int4*>(coords)[row] : make_int4(0, 0, 0, 0);
        const BmDesc d = desc[c.w];
        const unsigned* bmc = bm + d.base;
        const int bx = c.x - d.x0 - hk, by = c.y - d.y0 - hk, bz = c.z - d.z0 - hk;      // >= 0 by construction of the margin
        unsigned word[C1B_NIT];
        int shift[C1B_NIT];
#pragma unroll
        for (int it = 0; it < C1B_NIT; ++it) {
            const int ko = koff[it * 32 + l32];
            const bool use = valid && ko >= 0 && it < nit;
            const int x = bx + (ko & 255), y = by + ((ko >> 8) & 255), z = bz + (ko >> 16);
            word[it] = bmc[use ? (z * d.ny + y) * d.wx + (x >> 5) : 0];                   // a cloud's bitmap has < 2^24 words
            shift[it] = use ? (x & 31) : 32;
        }
        float acc = 0.f;
#pragma unroll
        for (int it = 0; it < C1B_NIT; ++it) {
            const bool present = shift[it] < 32 && ((word[it] >> shift[it]) & 1u);
            const unsigned long long m64 = __ballot(present);
            unsigned m = hw ? (unsigned)(m64 >> 32) : (unsigned)m64;
            while (m) {                                      // ascending offsets: fixed summation order; 4 LDS reads in flight
                float wv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int row = m ? it * 32 + __ffs(m) - 1 : C1O_MAXK;                 // row C1O_MAXK of Wl is zero
                    m &= m - 1;
                    wv[u] = Wl[row * 32 + l32];
                }
                acc += wv[0]; acc += wv[1]; acc += wv[2]; acc += wv[3];
            }
        }
        if (valid) out[(size_t)row * 32 + l32] = acc * sc + sh;
    }
}

// The first convolution as a matrix product on the fp16 MFMA: out[row][32] = occ[row][K^3] * W[K^3][32] with the occupancy
// bits of the row's K^3 region as a 0 / 1 operand (exact in fp16) and the weights as fp16 hi + lo planes (W * 2^s = hi + lo,
// fp32 accumulation; |error| <= 2^-22 |w| per term).  The reduction axis is ordered (z, y, x) with x padded to 8: the eight
// x-neighbours of one (y, z) line are one lane's share of a 32x32x16 step, i.e. one unaligned 8-bit run of one bitmap row,
// so a step is two (y, z) lines (one per lane half) and K = 7 takes 25 steps of two MFMAs for 32 rows.  Persistent
// workgroups keep the weight planes (50 KiB for K = 7) in LDS; a wave's 2 x 25 bitmap words are requested before the first
// step.  Replaces the per-row bit scan of conv1_bitmap_kernel (1.3 ms -> see DESIGN 3.5 for 1.3 M rows).
constexpr int C1M_MAXSTEPS = 25;                                     // (7 * 7 + 1) / 2
__global__ __launch_bounds__(256) void conv1_mfma_kernel(const int* __restrict__ coords, int n, const BmDesc* __restrict__ desc,
                                                         const unsigned* __restrict__ bm, const unsigned* __restrict__ zero2, int ksize,
                                                         const uintx4s* __restrict__ planes, float descale, const float* __restrict__ aff_s, const float* __restrict__ aff_t,
                                                         float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uintx4s pl[C1M_MAXSTEPS * 2 * 64];
    const int nsteps = (ksize * ksize + 1) / 2, hk = ksize / 2;
    for (int i = threadIdx.x; i < nsteps * 128; i += 256) pl[i] = planes[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
    const unsigned runmask = (1u << ksize) - 1u;
    const float sc = (aff_s ? aff_s[li] : 1.f) * descale, sh = aff_t ? aff_t[li] : 0.f;
    const int ntiles = (n + 31) / 32;
    for (int tile = blockIdx.x * 4 + (threadIdx.x >> 6); tile < ntiles; tile += gridDim.x * 4) {
        const int row = tile * 32 + li;
        const bool valid = row < n;
        const int4 c = valid ? reinterpret_cast<const int4*>(coords)[row] : make_int4(0, 0, 0, 0);
        const BmDesc d = desc[c.w];
        const unsigned* bmc = bm + d.base;
        const int bx = c.x - d.x0 - hk, by = c.y - d.y0 - hk, bz = c.z - d.z0 - hk;      // >= 0 by construction of the margin
        const int wcol = bx >> 5, shift = bx & 31;
        // this lane's (y, z) lines: 2 s + h, s = 0 .. nsteps - 1
        unsigned w0[C1M_MAXSTEPS], w1[C1M_MAXSTEPS];
        {
            int dy = h, dz = 0;
#pragma unroll
            for (int st = 0; st < C1M_MAXSTEPS; ++st) {
                const bool use = valid && st < nsteps && dz < ksize;
                const unsigned* wp = use ? bmc + (((bz + dz) * d.ny + (by + dy)) * d.wx + wcol) : zero2;      // a cloud's bitmap has < 2^24 words
                w0[st] = wp[0];
                w1[st] = wp[1];                                                               // (two spare words behind the last bitmap)
                dy += 2;
                if (dy >= ksize) { dy -= ksize; ++dz; }
            }
        }
        floatx16s acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int st = 0; st < C1M_MAXSTEPS; ++st) {
            if (st < nsteps) {                                                                // uniform
                const unsigned run = (unsigned)((((unsigned long long)w1[st] << 32) | w0[st]) >> shift) & runmask;
                uintx4s af;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int b0 = __builtin_amdgcn_sbfe(run, 2 * j, 1), b1 = __builtin_amdgcn_sbfe(run, 2 * j + 1, 1);   // 0 / -1
                    af[j] = ((unsigned)b0 & 0x00003C00u) | ((unsigned)b1 & 0x3C000000u);                                   // 1.0 in fp16
                }
                acc = mfma_sp16(af, pl[(2 * st + 0) * 64 + lane], acc);
                acc = mfma_sp16(af, pl[(2 * st + 1) * 64 + lane], acc);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int orow = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (orow < n) out[(size_t)orow * 32 + li] = acc[r] * sc + sh;
        }
    }
}

int launch_spconv(const SpConvArgs& a_in, hipStream_t s) {
    if (a_in.nout == 0) return 0;
    SpConvArgs a = a_in;
    if (!a.Wh || !a.rowperm) { a.rowperm = nullptr; a.nslots = a.nout; }     // the permutation is an optimisation of the fp16x2 kernels
    if (a.norm && !(a.Wh && a.cout == 32 && a.cin % 32 == 0 && (a.nslots + 31) / 32 >= 1024)) {
        set_error("sparse conv: the fused row normalisation exists in the 32-channel fine-level kernel only"); return YOHO_EINVAL;
    }
    const bool vec_ok = a.ldout % 4 == 0 && a.ocoff % 4 == 0 && (!a.res || (a.ldres % 4 == 0 && a.rcoff % 4 == 0));      // 16-byte epilogue accesses
    if (a.cin % 32 == 0 && a.cout % 32 == 0 && a.cout <= 256 && a.ldin % 4 == 0 && a.K <= SP_MAXK && vec_ok) {
        // Two 32-channel output blocks per wave where possible (halves the gather traffic).  Levels with fewer than ~1024
        // (row tile, channel group) units run the split variant: one unit per workgroup, the K loop over its 4 waves.
        const int ncbt = a.cout / 32, rowtiles = (a.nslots + 31) / 32;
        const int ncb = (ncbt % 2 == 0 && (long long)rowtiles * (ncbt / 2) >= 1024) ? 2 : 1;
        const bool split = (long long)rowtiles * (ncbt / ncb) < 1024;
        const dim3 blk(256);
        if (split) {
            const dim3 grid(rowtiles, ncbt / ncb);
            if (a.Wh && ncb == 2) hipLaunchKernelGGL((spconv16s_kernel<2, 2>), grid, blk, 0, s, a);
            else if (a.Wh) hipLaunchKernelGGL((spconv16s_kernel<1, 3>), grid, blk, 0, s, a);
            else if (ncb == 2) hipLaunchKernelGGL((spconv_kernel<2, true>), grid, blk, 0, s, a);
            else hipLaunchKernelGGL((spconv_kernel<1, true>), grid, blk, 0, s, a);
        } else {
            const dim3 grid((a.nslots + 127) / 128, ncbt / ncb);
            // 128 output channels: all four channel blocks in one wave, so every row is gathered once instead of twice (the gathers'
            // lane requests are what bounds these kernels; measured -0.25 ms on a 1.3 M-voxel pass, no gain at 256 channels)
            if (a.Wh && ncb == 2 && ncbt == 4 && rowtiles >= 1024)
                hipLaunchKernelGGL((spconv16w_kernel<4>), dim3(grid.x, 1), blk, 0, s, a);
            else if (a.Wh && ncb == 2) hipLaunchKernelGGL((spconv16w_kernel<2>), grid, blk, 0, s, a);
            else if (a.Wh) hipLaunchKernelGGL((spconv16w_kernel<1>), grid, blk, 0, s, a);
            else if (ncb == 2) hipLaunchKernelGGL((spconv_kernel<2, false>), grid, blk, 0, s, a);
            else hipLaunchKernelGGL((spconv_kernel<1, false>), grid, blk, 0, s, a);
        }
    } else {
        if (a.cout > 256 || a.cout < 1) { set_error("sparse conv: unsupported channel count %d", a.cout); return YOHO_EINVAL; }
        const int rows_per = 256 / a.cout;
        hipLaunchKernelGGL(spconv_small_kernel, dim3((a.nout + rows_per - 1) / rows_per), dim3(256), 0, s, a);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

__global__ void fill_ones_kernel(float* p, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 1.f;
}
void launch_fill_ones(float* p, int n, hipStream_t s) {
    hipLaunchKernelGGL(fill_ones_kernel, dim3((n + 255) / 256), dim3(256), 0, s, p, n);
}

// rows /= |row| (resunet.py:183-187), then once more (fcgf_feat.py:48).  c <= 32: a half-wave per row (the xor tree over
// 32 lanes gives the same sum as the 64-lane tree with zeros in the upper half), 8 rows per wave; else one wave per row.
__global__ __launch_bounds__(256) void row_normalize_kernel(const float* in, int n, int c, float* out, int twice, const int* __restrict__ operm) {
    const int lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c == 32) {
        // eight lanes per row, four channels each, the sum of squares in the order of the fused epilogue of spconv16w_kernel<1>
        // (a pass large enough for that kernel normalises there): the same bits whichever of the two runs
        const int ep = lane & 7;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = (wave * 4 + i) * 8 + (lane >> 3);
            const bool ok = row < n;
            float4 v = ok ? *reinterpret_cast<const float4*>(in + (size_t)row * 32 + 4 * ep) : make_float4(1.f, 0.f, 0.f, 0.f);
            for (int pass = 0; pass < (twice ? 2 : 1); ++pass) {
                float ss = fmaf(v.x, v.x, v.y * v.y) + fmaf(v.z, v.z, v.w * v.w);      // explicit: the compiler's contraction must not differ between the two places this is written
                ss += __shfl_xor(ss, 1); ss += __shfl_xor(ss, 2); ss += __shfl_xor(ss, 4);
                const float nr = sqrtf(ss);
                v.x /= nr; v.y /= nr; v.z /= nr; v.w /= nr;
            }
            if (ok) *reinterpret_cast<float4*>(out + (size_t)(operm ? operm[row] : row) * 32 + 4 * ep) = v;
        }
        return;
    }
    if (c <= 32) {
        const int l32 = lane & 31;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = (wave * 4 + i) * 2 + (lane >> 5);
            const bool ok = row < n && l32 < c;
            float v = ok ? in[(size_t)row * c + l32] : 0.f;
            for (int pass = 0; pass < (twice ? 2 : 1); ++pass) {
                float s = v * v;
                for (int o = 16; o >= 1; o >>= 1) s += __shfl_xor(s, o);
                v = v / sqrtf(s);
            }
            if (ok) out[(size_t)(operm ? operm[row] : row) * c + l32] = v;
        }
        return;
    }
    const int row = wave;
    if (row >= n) return;
    float v = lane < c ? in[(size_t)row * c + lane] : 0.f;
    for (int pass = 0; pass < (twice ? 2 : 1); ++pass) {
        float s = v * v;
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
        v = v / sqrtf(s);
    }
    if (lane < c) out[(size_t)(operm ? operm[row] : row) * c + lane] = v;
}
void launch_row_normalize(const float* in, int n, int c, float* out, int twice, const int* operm, hipStream_t s) {
    hipLaunchKernelGGL(row_normalize_kernel, dim3(c == 32 ? (n + 127) / 128 : (c < 32 ? (n + 31) / 32 : (n + 3) / 4)), dim3(256), 0, s, in, n, c, out, twice, operm);
}

// the first convolution on the constant-one input: the MFMA product over the occupancy bitmaps where both exist, the bit scan over
// the bitmaps without weight planes, hash probes without bitmaps
void launch_conv1(const Conv1Args& a, int nCU, hipStream_t s) {
    const int wide = 3 * (nCU > 0 ? nCU : 256);                          // persistent workgroups
    if (a.bm && a.planes)
        hipLaunchKernelGGL(conv1_mfma_kernel, dim3(std::min((a.n + 127) / 128, wide)), dim3(256), 0, s, a.coords, a.n, a.desc, a.bm, a.bm + a.bm_words, a.ksize,
                           reinterpret_cast<const uintx4s*>(a.planes), a.descale, a.aff_s, a.aff_t, a.out);
    else if (a.bm)
        hipLaunchKernelGGL(conv1_bitmap_kernel, dim3(std::min((a.n + 7) / 8, wide)), dim3(256), 0, s, a.coords, a.n, a.desc, a.bm, a.ksize, a.W, a.aff_s, a.aff_t, a.out);
    else
        hipLaunchKernelGGL(conv1_ones_kernel, dim3((a.n + 7) / 8), dim3(256), 0, s, a.coords, a.n, a.keys, a.mask, a.ksize, a.W, a.aff_s, a.aff_t, a.out);
}
void launch_heads_fused(const HeadsArgs& a, int nCU, hipStream_t s) {
    hipLaunchKernelGGL((heads_fused_kernel<3>), dim3(std::min((a.n + 127) / 128, 2 * (nCU > 0 ? nCU : 256))), dim3(256), 0, s, a);
}

}  // namespace yoho
