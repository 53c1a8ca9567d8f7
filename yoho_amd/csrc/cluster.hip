// Exact DBSCAN labels of a 3-D cloud (include/yoho_cluster.h).  Compiled with -ffp-contract=off like clean.hip
// (yoho_amd/build.py).  The cell-sorted grid comes from rfgrid.hip / rfgrid.h (THE GRID, THE QUERY's exactness argument) unchanged.
//
//   cu_count_kernel     one lane per row: count, core, parent[i] = i, sizes[i] = 0
//   cu_union_kernel     one lane per core row i: every core neighbour j < i unites the two trees (the one pass over the edges)
//   cu_root_kernel      a later launch: root[i] = the root of a core row, of a border row's best core neighbour, or -1; the root marks
//                       as one ballot word per wave and one count per block
//   cu_scan_kernel      one workgroup: the exclusive scan of the block counts, n_out = {C, 0, 0}
//   cu_label_kernel     labels[i] = rank of root[i] among the roots in row order; sizes and n_out[1..2] by integer atomics
//
// THE WALK is rfgrid.h's rf_walk_each (THE DISTINCT BUCKETS), which hands every candidate (d2 < gate2, j != self) to a functor once:
// the three passes differ in the functor alone.
//
// THE UNION.  parent[] is a forest with parent[x] <= x, every row its own root after cu_count_kernel.  A lane of cu_union_kernel
// finds the roots of both ends of an edge and hooks the LARGER root under the smaller with a compare-and-swap that expects the larger
// root to be a root still, so the root of a tree is the lowest row of it, whatever the order of the hooks: the forest at the end of
// the launch has one tree per connected component and its root is the component's lowest core row - a function of the arguments
// alone.  A lane keeps the row its last edge left row i under, ri, and starts from there (an ancestor of i: as good as i), and
// an edge whose other end's path leads to ri is settled there (cu_edge): ri is an ancestor of both ends, root or not.  A find
// also halves the path it walks (parent[x]: p -> parent[p], a compare-and-swap that expects p), which moves a row
// under another of its ancestors and nothing else.
//   Visibility.  The per-XCD L2s are not coherent with each other and a CU's L1 is never refreshed by another CU's stores, so inside
//   that launch EVERY access to parent[] is an agent-scope atomic: a relaxed load that bypasses the L1, or a compare-and-swap.  A
//   value read may still be old.  An old value of parent[x] is x itself or an earlier parent: an ancestor of x in the forest of now
//   (a parent is only ever replaced by an ancestor of it, and only a root gets its first parent), so a find that follows old values
//   stays inside the tree and strictly descends in row number; if it stops at a row that is a root no longer, the hook's
//   compare-and-swap - which is decided where the word lives, not in a cache - fails and returns the row's parent of now, and the
//   lane goes on from THAT value.  Two lanes that hook the same root: one wins, the other continues likewise.  A hook never closes a
//   cycle (parent < child always), and a lane ends an edge only when both ends reached one row or its own hook went in: at the end
//   of the launch both ends of every edge are in one tree.
//   No waiting.  The only loops are the find, which strictly descends, and the retry after a failed swap, which means that
//   another lane made progress: no spin, no flag, no barrier across workgroups, no launch that depends on N.
//   Everything that reads parent[] as final (cu_root_kernel) does so in a later launch, with plain loads, and writes root[], not
//   parent[].
//
// Every workspace byte is written (the grid build, cu_count_kernel, cu_root_kernel - all four ballot words of every block -,
// cu_scan_kernel) before it is read; no float atomic; sizes and n_out[1..2] are integer sums, whose order of arrival does not
// show.  Registers (hipcc -O3, gfx950) and timings: tools/time_cluster.py -> profiles/cluster.md; no kernel of this file uses scratch.
#include "rfgrid.h"
#include "yoho_cluster.h"
#include <climits>
#include <cmath>

namespace yoho {

__global__ __launch_bounds__(256) void cu_count_kernel(RfGrid g, const float* __restrict__ pts, int N, int min_pts, int32_t* __restrict__ count,
                                                       uint8_t* __restrict__ core, uint8_t* __restrict__ cw, int* __restrict__ parent,
                                                       int32_t* __restrict__ sizes) {
    __shared__ unsigned slots[27][256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;                                                   // no barrier below
    float q[3];
    rf_load_row(pts, i, q);
    int n = 0;
    rf_walk_each(g, q, i, slots, [&](float, int) { ++n; });
    const uint8_t c = rf_finite3(q[0], q[1], q[2]) && n >= min_pts - 1 ? 1 : 0;     // count + 1 >= min_pts, min_pts >= 1
    if (count) count[i] = n;
    if (core) core[i] = c;
    cw[i] = c;
    parent[i] = i;
    if (sizes) sizes[i] = 0;
}

// ---- the union: agent-scope atomics on parent[] and nothing else (THE UNION) -------------------------------------------------------
__device__ __forceinline__ int cu_parent(const int* parent, int x) { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// compare-and-swap of parent[x]: the value found there, `expect` when the swap went in
__device__ __forceinline__ int cu_swap(int* parent, int x, int expect, int desired) {
    __hip_atomic_compare_exchange_strong(parent + x, &expect, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expect;
}
// a row that was a root when it was read, reached from x by parents only: strictly descending; halves the path on its way
__device__ __forceinline__ int cu_find(int* parent, int x) {
    for (;;) {
        const int p = cu_parent(parent, x);
        if (p == x) return x;
        const int gp = cu_parent(parent, p);
        if (gp != p) cu_swap(parent, x, p, gp);                           // p -> an ancestor of p; a failure changes nothing
        x = p;
    }
}
// unites the trees of a and b -> the root both hang under now (a row that was a root when it was last read)
__device__ __forceinline__ int cu_unite(int* parent, int a, int b) {
    for (;;) {
        a = cu_find(parent, a);
        b = cu_find(parent, b);
        if (a == b) return b;
        if (a < b) { const int t = a; a = b; b = t; }                     // a the larger root
        const int was = cu_swap(parent, a, a, b);
        if (was == a) return b;
        a = was;                                                          // another lane hooked a first: go on from where it hangs now
    }
}

// the edge {i, j}, ri an ancestor of i -> an ancestor of i that j hangs under too.  The path from j is followed down to ri and no
// further: where it meets ri the edge is settled without a look at parent[ri] - the word of a large tree's root, which every lane of
// the tree would otherwise load once per edge, millions of loads of one address (profiles/cluster.md: 2.1 -> 1.3 ms at 300 000 points)
__device__ __forceinline__ int cu_edge(int* parent, int ri, int j) {
    int x = j;
    if (x > ri) {
        int p = cu_parent(parent, x);
        for (;;) {
            if (p == ri) return ri;
            if (p == x) break;                                            // a root above ri
            if (p < ri) { x = p; break; }
            const int gp = cu_parent(parent, p);                          // p > ri: every word is loaded once
            if (gp != p) cu_swap(parent, x, p, gp);                       // halve the path, as cu_find does
            x = p;
            p = gp;
        }
    }
    return x == ri ? ri : cu_unite(parent, ri, x);                        // another tree, or ri is a root no longer
}

__global__ __launch_bounds__(256) void cu_union_kernel(RfGrid g, const float* __restrict__ pts, int N, const uint8_t* __restrict__ cw, int* parent) {
    __shared__ unsigned slots[27][256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N || !cw[i]) return;                                         // no barrier below
    float q[3];
    rf_load_row(pts, i, q);
    int ri = i;                                                           // an ancestor of i: where the last edge left it
    rf_walk_each(g, q, i, slots, [&](float, int j) {
        if (j < i && cw[j]) ri = cu_edge(parent, ri, j);                  // the edge {i, j} once, from its higher end
    });
}

// ---- the passes behind it: parent[] is final and read with plain loads ----------------------------------------------------------------
__device__ __forceinline__ int cu_root_of(const int* __restrict__ parent, int x) {
    for (;;) {
        const int p = parent[x];
        if (p == x) return x;
        x = p;
    }
}

// root[i]; bal[4 b + w] = the lanes of wave w of block b whose row is a root, blk[b] = their number in the block
__global__ __launch_bounds__(256) void cu_root_kernel(RfGrid g, const float* __restrict__ pts, int N, const uint8_t* __restrict__ cw,
                                                      const int* __restrict__ parent, int* __restrict__ root, u64* __restrict__ bal,
                                                      int* __restrict__ blk) {
    __shared__ unsigned slots[27][256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool is_root = false;
    if (i < N) {
        int r = -1;
        if (cw[i]) {
            r = cu_root_of(parent, i);
            is_root = r == i;
        } else {
            float q[3];
            rf_load_row(pts, i, q);
            u64 best = NN_KEY_EMPTY;
            rf_walk_each(g, q, i, slots, [&](float d2, int j) {
                const u64 key = nn_key(__float_as_uint(d2), (unsigned)j);       // d2 >= +0: the order of the integers is that of (d2, j)
                if (cw[j] && key < best) best = key;
            });
            if (best != NN_KEY_EMPTY) r = cu_root_of(parent, (int)nn_key_index(best));
        }
        root[i] = r;
    }
    const u64 m = __ballot(is_root);
    if ((threadIdx.x & 63) == 0) bal[4 * (size_t)blockIdx.x + (threadIdx.x >> 6)] = m;
    const int n = __syncthreads_count(is_root);
    if (threadIdx.x == 0) blk[blockIdx.x] = n;
}

// exclusive scan of blk[0 .. nblk) in place, one workgroup (rf_scan_kernel's shape); n_out = {the total, 0, 0}
__global__ __launch_bounds__(1024) void cu_scan_kernel(int* __restrict__ blk, int nblk, int32_t* __restrict__ n_out) {
    __shared__ int part[1024];
    const int tid = threadIdx.x, per = (nblk + 1023) / 1024;
    const int lo = tid * per < nblk ? tid * per : nblk, hi = lo + per < nblk ? lo + per : nblk;
    int s = 0;
    for (int i = lo; i < hi; ++i) s += blk[i];
    part[tid] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - s;
    for (int i = lo; i < hi; ++i) { const int c = blk[i]; blk[i] = run; run += c; }
    if (tid == 1023) { n_out[0] = part[1023]; n_out[1] = 0; n_out[2] = 0; }
}

__global__ __launch_bounds__(256) void cu_label_kernel(int N, const uint8_t* __restrict__ cw, const int* __restrict__ root, const u64* __restrict__ bal,
                                                       const int* __restrict__ blk, int32_t* __restrict__ labels, int32_t* __restrict__ sizes,
                                                       int32_t* __restrict__ n_out) {
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    int lab = -1;
    bool is_core = false;
    if (i < N) {
        const int r = root[i];
        if (r >= 0) {                                                     // the roots in front of r, in row order
            const size_t b = (size_t)(r >> 8);
            const int w = (r >> 6) & 3;
            lab = blk[b];
            for (int k = 0; k < w; ++k) lab += __popcll(bal[4 * b + k]);
            lab += __popcll(bal[4 * b + w] & ((1ull << (r & 63)) - 1ull));
        }
        labels[i] = lab;
        is_core = cw[i] != 0;
    }
    // one add per wave and cluster: the lanes of a wave mostly share a label
    bool todo = sizes != nullptr && lab >= 0;
    for (;;) {
        const u64 open = __ballot(todo);
        if (open == 0ull) break;
        const int leader = __ffsll((long long)open) - 1;
        const int l0 = __shfl(lab, leader);
        const bool same = todo && lab == l0;
        const u64 sm = __ballot(same);
        if (lane == leader) atomicAdd(&sizes[l0], __popcll(sm));          // an integer sum: the order of arrival does not show
        if (same) todo = false;
    }
    const int ncore = __syncthreads_count(is_core);
    const int nnoise = __syncthreads_count(i < N && lab < 0);
    if (threadIdx.x == 0) {
        if (ncore > 0) atomicAdd(&n_out[1], ncore);
        if (nnoise > 0) atomicAdd(&n_out[2], nnoise);
    }
}

}  // namespace yoho

using namespace yoho;

extern "C" {

int yoho_dbscan(yoho_ctx* c, const float* pts, int N, float eps, int min_pts, int32_t* labels, int32_t* count, uint8_t* core, int32_t* sizes,
                int32_t* n_out, void* stream) {
    const char* fn = "yoho_dbscan";
    int rc;
    if ((rc = rf_check_cloud(fn, c, N, "eps", eps)) || (rc = rf_check_range(fn, "min_pts", min_pts, 1, RF_NAMED(INT_MAX)))) return rc;
    if (!pts) return RF_REFUSE("%s: bad argument (pts is NULL)", fn);
    if (!labels) return RF_REFUSE("%s: bad argument (labels is NULL)", fn);
    if (!n_out) return RF_REFUSE("%s: bad argument (n_out is NULL)", fn);
    YOHO_NEED_ALIGNED("yoho_dbscan", 3, pts, labels, count, sizes, n_out);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const int nblk = (N + 255) / 256;
    int *parent = nullptr, *root = nullptr, *blk = nullptr;
    uint8_t* cw = nullptr;
    u64* bal = nullptr;
    RfGridWs w;
    if ((rc = bind_ws(c, s, [&](Arena& ar) {
            parent = ar.take<int>((size_t)N);
            root = ar.take<int>((size_t)N);
            cw = ar.take<uint8_t>((size_t)N);
            bal = ar.take<u64>(4 * (size_t)nblk);
            blk = ar.take<int>((size_t)nblk);
            rf_grid_layout(ar, N, w);
        }))) return rc;
    RfGrid g;
    if ((rc = rf_build_grid(pts, N, eps, w, g, s))) return rc;
    const dim3 grid(nblk), block(256);
    hipLaunchKernelGGL(cu_count_kernel, grid, block, 0, s, g, pts, N, min_pts, count, core, cw, parent, sizes);
    hipLaunchKernelGGL(cu_union_kernel, grid, block, 0, s, g, pts, N, (const uint8_t*)cw, parent);
    hipLaunchKernelGGL(cu_root_kernel, grid, block, 0, s, g, pts, N, (const uint8_t*)cw, (const int*)parent, root, bal, blk);
    hipLaunchKernelGGL(cu_scan_kernel, dim3(1), dim3(1024), 0, s, blk, nblk, n_out);
    hipLaunchKernelGGL(cu_label_kernel, grid, block, 0, s, N, (const uint8_t*)cw, (const int*)root, (const u64*)bal, (const int*)blk, labels, sizes, n_out);
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
