// Exact Poisson-disk thinning of a 3-D cloud, in the order of a hashed key (include/yoho_disk.h) or of a caller's priority
// (include/yoho_salient.h's yoho_disk_sample_prio, DESIGN 3.22, whose entry is in salient.hip and comes here through dkthin.h).
// Compiled with -ffp-contract=off like clean.hip and cluster.hip (yoho_amd/build.py).  The cell-sorted grid comes from rfgrid.hip /
// rfgrid.h (THE GRID, THE QUERY's exactness argument) unchanged.
//
//   dk_zero_kernel      one workgroup: the round counters cnt[0 .. YOHO_DISK_MAX_ROUNDS] and n_out[0] = 0
//   dk_init_kernel<K>   one lane per row: a stored key is written; state[i] = 0 (finite) or 2 - with resume = 1 the hashed entry
//                       takes the state handed in as it is, the priority entry turns a non-finite row handed in as 0 into 2 -;
//                       cnt[0] += the undecided rows of the block
//   dk_round_kernel<K>  round r = 1 .. rounds, one launch each, eight lanes per row: src -> dst, cnt[r] += the rows the block leaves undecided;
//                       the launch returns at once when cnt[r - 1] == 0 (yoho_icp_refine's iterations do the same behind convergence)
//   dk_tail_kernel      the number of rounds that ran from cnt[], the final state into `state`, n_out
//   dk_thin             the host side of both entries: the arena, the grid build, the launches and the A/B alternation
//
// THE ROUNDS are synchronous, which is what makes the state of an unfinished call a function of the arguments: round r reads the
// buffer round r - 1 wrote and writes the other one, every byte of it (a decided row copies its byte), so no lane ever reads a byte
// that another lane of the same launch writes.  The two buffers are the caller's `state` (A) and N bytes of the workspace (B): odd
// rounds read A and write B, even rounds read B and write A; the tail copies B to A when the last round that ran was odd.  What a
// launch reads - the other buffer, cnt[r - 1] - was stored by EARLIER launches on the stream, which is the only visibility the
// hardware gives for free (the per-XCD L2s are not coherent with each other inside a launch; cluster.hip's THE UNION pays for that
// with agent-scope atomics, this file has no need to).  In place, a row would see some neighbours' new states and some old ones,
// as the schedule has it: the final set would be the same (it is unique), the round count and every intermediate state would not.
//
// THE WALK is rf_walk's plain loop over the 27 cells around a row with this file's test in the middle.  Two of the 27 cells may share a
// bucket, or be the same clamped cell, and a candidate is then met twice: "a preceding neighbour is kept" and "none is undecided"
// count nothing and do not notice, so rfgrid.h's de-duplicated slot list and its 27 KB of LDS are left out.
//
// THE KEY is a policy of the two templated kernels.  DkHashed: the key of a neighbour comes from its row index in pk[].w, there is no
// key array, and d2 < gate2 && key(j) < ki gates the state load.  DkStored: key64 depends on prio[j], so dk_init_kernel writes it for
// every row into the workspace; in a batch the key and the state of every candidate that passes the gate are loaded TOGETHER - two
// independent gathers behind the point loads, not a key load in front of the state load - and compared afterwards; a candidate
// outside the gate loads neither, and j == i has kj == ki and counts nothing.  The keys are in row order; a copy in the grid's sorted
// order beside pk[] would save the gather and is left out until profiles/salient.md says the key loads matter.
//   A round is bound by latency, not by work: from the third round on a few per cent of the rows are undecided, and the launch lasts
//   as long as ONE row's walk - with one lane per row a chain of some 300 dependent loads (a bucket's range, then point after point,
//   then the state of each neighbour), 0.15 ms a round whatever N (profiles/disk.md).  So DK_LANES = 8 lanes share a row: lane k
//   takes buckets k, k + 8, k + 16 (, k + 24), loads their ranges together, and walks each DK_BATCH = 8 candidates at a time - the
//   points of a batch are loaded together, then the states of those that pass the gate and the key test together (a slot behind
//   the bucket's end repeats its last point: harmless, see above).  The row's lanes sit side by side in one wave; two ballots hand
//   what they found to the row's first lane, which writes the byte.  There is no way out of the walk at the first kept neighbour:
//   it would put the loads back in a chain.  A decided row still costs one byte read (by its 8 lanes, one transaction) and its copy.
//
// No kernel waits for another lane or workgroup: no spin, no flag, no cooperative launch, no grid barrier; the only synchronisation
// is the kernel boundary (and __syncthreads_count for the one integer atomic a workgroup adds to its round's counter - an integer sum,
// whose order of arrival does not show).  Every workspace byte is written (the grid build, dk_zero_kernel, dk_init_kernel's stored keys, every byte of B by the
// first round) before it is read: with rounds >= 1 round 1 always has a launch, and it either writes all of B or, with cnt[0] == 0,
// no later launch reads B.  Registers (hipcc -O3, gfx950) and timings: tools/time_disk.py -> profiles/disk.md,
// tools/time_salient.py -> profiles/salient.md; no kernel of this file uses scratch.
#include "rfgrid.h"
#include "dkthin.h"
#include "yoho_disk.h"
#include "yoho_salient.h"
#include <cmath>

namespace yoho {

static_assert(YOHO_SALIENT_MAX_ROUNDS == YOHO_DISK_MAX_ROUNDS, "the two entries share dk_zero_kernel's and dk_tail_kernel's counters");
constexpr int DK_COUNTERS = YOHO_DISK_MAX_ROUNDS + 1;      // cnt[r] = the rows undecided after round r, cnt[0] at entry
constexpr int DK_BATCH = 8;                                // candidates of a bucket a lane has in flight at once (THE WALK)
constexpr int DK_LANES = 8;                                // lanes that share the 27 buckets around a row: a power of two, a divisor of 64
constexpr int DK_CELLS = (27 + DK_LANES - 1) / DK_LANES;   // buckets per lane
constexpr int DK_ROWS = 256 / DK_LANES;                    // rows per workgroup of dk_round_kernel

// the mixer of include/yoho_disk.h PRIORITY, the low half of include/yoho_salient.h's key64
__device__ __forceinline__ unsigned dk_key(unsigned i, unsigned seed) {
    unsigned x = i ^ seed;
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// ---- the key policies (THE KEY): a lower key precedes ------------------------------------------------------------------------------------
struct DkHashed {
    typedef unsigned Key;
    static constexpr bool STORED = false;
    unsigned seed;
    __device__ __forceinline__ Key of(int i) const { return dk_key((unsigned)i, seed); }
};
struct DkStored {
    typedef u64 Key;
    static constexpr bool STORED = true;
    u64* __restrict__ key;                                 // [N] in the workspace, written by dk_init_kernel
    const float* __restrict__ prio;
    unsigned seed;
    __device__ __forceinline__ Key of(int i) const { return key[i]; }
    // include/yoho_salient.h PRIORITY
    __device__ __forceinline__ void store(int i) const {
        const float p = prio[i];
        const unsigned b = (unsigned)__float_as_int(p);
        const unsigned ord = p != p ? 0u : ((b & 0x80000000u) ? ~b : (b | 0x80000000u));
        key[i] = ((u64)(~ord) << 32) | (u64)dk_key((unsigned)i, seed);
    }
};

__global__ __launch_bounds__(128) void dk_zero_kernel(int* __restrict__ cnt, int32_t* __restrict__ n_out) {
    if (threadIdx.x < DK_COUNTERS) cnt[threadIdx.x] = 0;
    if (threadIdx.x == 0) n_out[0] = 0;
}

template <class K>
__global__ __launch_bounds__(256) void dk_init_kernel(const float* __restrict__ pts, int N, K key, int resume, uint8_t* __restrict__ state,
                                                      int* __restrict__ cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool und = false;
    if (i < N) {
        if constexpr (K::STORED) key.store(i);
        uint8_t s = 0;
        if (resume) s = state[i];
        // the hashed entry takes a state handed in as it is; the priority entry looks at a row handed in as 0 again: a non-finite one becomes 2
        if (K::STORED ? s == 0 : !resume) {
            float q[3];
            rf_load_row(pts, i, q);
            s = rf_finite3(q[0], q[1], q[2]) ? 0 : 2;
            state[i] = s;
        }
        und = s == 0;
    }
    const int n = __syncthreads_count(und);
    if (threadIdx.x == 0 && n > 0) atomicAdd(&cnt[0], n);
}

// round r: prev = cnt + r - 1 (the rows the round before left undecided), prev[1] this round's counter.  DK_LANES lanes per row (THE WALK)
template <class K>
__global__ __launch_bounds__(256) void dk_round_kernel(RfGrid g, const float* __restrict__ pts, int N, const K key, const uint8_t* __restrict__ src,
                                                       uint8_t* __restrict__ dst, int* __restrict__ prev) {
    if (prev[0] == 0) return;                                             // uniform: the thinning is complete, dst is never read
    const int sub = threadIdx.x & (DK_LANES - 1);
    const int i = blockIdx.x * DK_ROWS + (threadIdx.x / DK_LANES);
    uint8_t s = 2;
    if (i < N) s = src[i];
    const bool walk = i < N && s == 0;                                    // a decided row costs this one byte and its copy
    bool open = false, dropped = false;                                   // a preceding neighbour undecided / kept, among this lane's buckets
    if (walk) {
        float q[3];
        rf_load_row(pts, i, q);
        const typename K::Key ki = key.of(i);
        const int cx = rf_cell((double)q[0], g.inv_cell), cy = rf_cell((double)q[1], g.inv_cell), cz = rf_cell((double)q[2], g.inv_cell);
        int p0[DK_CELLS], p1[DK_CELLS];
#pragma unroll
        for (int k = 0; k < DK_CELLS; ++k) {                              // the ranges of the lane's buckets, all on their way at once
            const int c = sub + k * DK_LANES;
            p0[k] = p1[k] = 0;
            if (c < 27) {
                const unsigned sl = rf_slot(rf_clampi(cx + c % 3 - 1), rf_clampi(cy + (c / 3) % 3 - 1), rf_clampi(cz + c / 9 - 1), g.mask);
                p0[k] = g.start[sl];
                p1[k] = g.start[sl + 1];
            }
        }
#pragma unroll
        for (int k = 0; k < DK_CELLS; ++k) {
#pragma unroll 1
            for (int p = p0[k]; p < p1[k]; p += DK_BATCH) {               // DK_BATCH candidates at a time: their loads are in flight together
                float4 v[DK_BATCH];
#pragma unroll
                for (int u = 0; u < DK_BATCH; ++u) v[u] = g.pk[p + u < p1[k] ? p + u : p1[k] - 1];
                uint8_t sj[DK_BATCH];
                typename K::Key kj[DK_BATCH];
#pragma unroll
                for (int u = 0; u < DK_BATCH; ++u) {
                    const float b[3] = {v[u].x, v[u].y, v[u].z};
                    const float d2 = dist2_f32<3>(q, b);
                    const int j = __float_as_int(v[u].w);
                    // false for a NaN / inf on either side; a slot behind the bucket's end repeats its last point (THE KEY)
                    const bool in = d2 < g.gate2;
                    if constexpr (K::STORED) {
                        kj[u] = in ? key.of(j) : ~(typename K::Key)0;
                        sj[u] = in ? src[j] : (uint8_t)2;
                    } else {
                        kj[u] = 0;                                        // the key test is in front of the load; false for j == i
                        sj[u] = in && key.of(j) < ki ? src[j] : (uint8_t)2;
                    }
                }
#pragma unroll
                for (int u = 0; u < DK_BATCH; ++u) {
                    const bool before = !K::STORED || kj[u] < ki;
                    dropped = dropped || (before && sj[u] == 1);
                    open = open || (before && sj[u] == 0);
                }
            }
        }
    }
    // what the row's lanes found, to its first lane: the DK_LANES bits of the row in the wave's ballots (every lane of the wave is here)
    const int first = (threadIdx.x & 63) & ~(DK_LANES - 1);
    const bool any_dropped = ((__ballot(dropped) >> first) & ((1ull << DK_LANES) - 1ull)) != 0ull;
    const bool any_open = ((__ballot(open) >> first) & ((1ull << DK_LANES) - 1ull)) != 0ull;
    bool und = false;
    if (i < N && sub == 0) {
        if (walk) s = any_dropped ? 2 : (any_open ? 0 : 1);
        dst[i] = s;
        und = s == 0;
    }
    const int n = __syncthreads_count(und);
    if (threadIdx.x == 0 && n > 0) atomicAdd(&prev[1], n);
}

// cnt[r] > 0 implies cnt[r - 1] > 0 (a round that does not run leaves its counter 0), so the rounds that ran are the r < rounds with
// cnt[r] > 0; the state they left is in B when their number is odd
__global__ __launch_bounds__(256) void dk_tail_kernel(int N, int rounds, const int* __restrict__ cnt, const uint8_t* __restrict__ B,
                                                      uint8_t* __restrict__ state, int32_t* __restrict__ n_out) {
    const int ran = __syncthreads_count((int)threadIdx.x < rounds && cnt[threadIdx.x] > 0);
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool kept = false;
    if (i < N) {
        uint8_t s;
        if (ran & 1) {
            s = B[i];
            state[i] = s;
        } else {
            s = state[i];
        }
        kept = s == 1;
    }
    const int n = __syncthreads_count(kept);
    if (threadIdx.x == 0) {
        if (n > 0) atomicAdd(&n_out[0], n);
        if (blockIdx.x == 0) { n_out[1] = ran; n_out[2] = cnt[ran]; }
    }
}

template <class K>
static void dk_launch(const K& key, const RfGrid& g, const float* pts, int N, int rounds, int resume, uint8_t* state, uint8_t* B, int* cnt, int32_t* n_out,
                      hipStream_t s) {
    const dim3 grid((N + 255) / 256), block(256);
    hipLaunchKernelGGL(dk_zero_kernel, dim3(1), dim3(128), 0, s, cnt, n_out);
    hipLaunchKernelGGL(dk_init_kernel<K>, grid, block, 0, s, pts, N, key, resume, state, cnt);
    for (int r = 1; r <= rounds; ++r) {                                   // odd rounds read A = state and write B, even rounds the other way
        const uint8_t* src = (r & 1) ? state : B;
        uint8_t* dst = (r & 1) ? B : state;
        hipLaunchKernelGGL(dk_round_kernel<K>, dim3((N + DK_ROWS - 1) / DK_ROWS), block, 0, s, g, pts, N, key, src, dst, cnt + (r - 1));
    }
    hipLaunchKernelGGL(dk_tail_kernel, grid, block, 0, s, N, rounds, (const int*)cnt, (const uint8_t*)B, state, n_out);
}

int dk_thin(yoho_ctx* c, const float* pts, int N, float radius, const float* prio, unsigned seed, int rounds, int resume, uint8_t* state,
            int32_t* n_out, hipStream_t s) {
    HIPCHK(hipSetDevice(c->device));
    int rc;
    uint8_t* B = nullptr;
    int* cnt = nullptr;
    u64* key = nullptr;
    RfGridWs w;
    if ((rc = bind_ws(c, s, [&](Arena& ar) {
            B = ar.take<uint8_t>((size_t)N);
            cnt = ar.take<int>((size_t)DK_COUNTERS);
            if (prio) key = ar.take<u64>((size_t)N);
            rf_grid_layout(ar, N, w);
        }))) return rc;
    RfGrid g;
    if ((rc = rf_build_grid(pts, N, radius, w, g, s))) return rc;
    if (prio) dk_launch(DkStored{key, prio, seed}, g, pts, N, rounds, resume, state, B, cnt, n_out, s);
    else dk_launch(DkHashed{seed}, g, pts, N, rounds, resume, state, B, cnt, n_out, s);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace yoho

using namespace yoho;

extern "C" {

int yoho_disk_sample(yoho_ctx* c, const float* pts, int N, float radius, uint32_t seed, int rounds, int resume, uint8_t* state, int32_t* n_out,
                     void* stream) {
    const char* fn = "yoho_disk_sample";
    int rc;
    if ((rc = rf_check_cloud(fn, c, N, "radius", radius)) || (rc = rf_check_range(fn, "rounds", rounds, 1, RF_NAMED(YOHO_DISK_MAX_ROUNDS)))) return rc;
    if (resume != 0 && resume != 1) return RF_REFUSE("%s: resume=%d must be 0 or 1", fn, resume);
    if (!pts) return RF_REFUSE("%s: bad argument (pts is NULL)", fn);
    if (!state) return RF_REFUSE("%s: bad argument (state is NULL)", fn);
    if (!n_out) return RF_REFUSE("%s: bad argument (n_out is NULL)", fn);
    YOHO_NEED_ALIGNED("yoho_disk_sample", 3, pts, n_out);
    return dk_thin(c, pts, N, radius, nullptr, (unsigned)seed, rounds, resume, state, n_out, (hipStream_t)stream);
}

}  // extern "C"
