// The cell-sorted grid over a target cloud, as its users see it: the device-side pieces of a query inline, the workspace and the two
// host calls that build it (rfgrid.hip, where THE GRID and THE QUERY are described), and the refusals the entries of the family share.
// The sums, the Kabsch step and the 3 x 3 Jacobi are in rffit.h.  Include from translation units compiled with -ffp-contract=off only.
//
//   rf_cell / rf_slot, RfGrid     a coordinate's cell, a cell's bucket, the grid as a kernel argument
//   rf_load_row, rf_finite3       row i of an (N, 3) f32 cloud; "three coordinates finite" (false for a NaN)
//   rf_walk                       the nearest candidate inside the gate, ties to the lower row: refine, verify, multiway, fuse, pl_pair_kernel.
//                                 It may meet a point twice - clamped neighbour cells are the same cell, and two of the 27 can hash to one
//                                 bucket -, which a minimum does not notice and a count, a list or a sum does
//   rf_slots27                    THE DISTINCT BUCKETS: the 27 slots around a query in registers, handed one by one to a functor, a slot equal
//                                 to an earlier one replaced by RF_SEEN.  Every bucket is then walked once, every point of it goes through the exact f32 test, a point
//                                 lies in one bucket only: a count is exact
//   rf_walk_each                  f(d2, j) once per candidate (d2 < gate2, j != self): clean.hip's lists, cluster.hip's three passes.  The
//                                 marked slots are parked in LDS, one column per lane (27 648 bytes a workgroup of 256), and the buckets are
//                                 walked by a loop that is NOT unrolled: the functor may be a 31-step insertion chain, and 27 copies of it
//                                 would not fit the instruction cache.  A lane reads its own column only, so no barrier is needed
//   rf_moments                    the unrolled walk with the slots in registers: n, S1 (3) and S2 (6) of the offsets from the query in
//                                 f64, the row itself included - plane.hip's normals, salient.hip's saliency.  One lane per point: the ten
//                                 accumulators need no cross-lane sum, whose order would have to be fixed as well
#pragma once
#include "common.h"
#include "nnmath.h"
#include "yoho_refine.h"
#include <cmath>

namespace yoho {

typedef unsigned long long u64;
constexpr int RF_CLAMP = (1 << 20) - 1;
constexpr int RF_NONE = 0x7FFFFFFF;
constexpr double RF_MIN_CELL = 0x1p-60;

// gridnn.hip's gn_cell / gn_key / gn_slot
__device__ __forceinline__ int rf_cell(double x, double inv_cell) {
    double c = floor(x * inv_cell);
    c = fmin(fmax(c, -(double)RF_CLAMP), (double)RF_CLAMP);          // NaN -> -RF_CLAMP
    return (int)c;
}
__device__ __forceinline__ int rf_clampi(int c) { return c < -RF_CLAMP ? -RF_CLAMP : (c > RF_CLAMP ? RF_CLAMP : c); }
__device__ __forceinline__ unsigned rf_slot(int cx, int cy, int cz, unsigned mask) {
    const u64 key = ((u64)(unsigned)(cx + (1 << 20)) << 42) | ((u64)(unsigned)(cy + (1 << 20)) << 21) | (u64)(unsigned)(cz + (1 << 20));
    return (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 33) & mask;
}

struct RfGrid {
    const int* start;        // [nslots + 1] first sorted position of a bucket
    const float4* pk;        // [Nt] sorted points (x, y, z, original index)
    double inv_cell;
    unsigned mask;           // nslots - 1
    float gate2;
};

// ---- the query -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void rf_walk(const RfGrid& g, const float (&q)[3], float& bd, int& bi) {
    const int cx = rf_cell((double)q[0], g.inv_cell), cy = rf_cell((double)q[1], g.inv_cell), cz = rf_cell((double)q[2], g.inv_cell);
    bd = __builtin_inff();
    bi = RF_NONE;
    for (int c = 0; c < 27; ++c) {
        const unsigned s = rf_slot(rf_clampi(cx + c % 3 - 1), rf_clampi(cy + (c / 3) % 3 - 1), rf_clampi(cz + c / 9 - 1), g.mask);
        const int p1 = g.start[s + 1];
        for (int p = g.start[s]; p < p1; ++p) {
            const float4 v = g.pk[p];
            const float b[3] = {v.x, v.y, v.z};
            const float d2 = dist2_f32<3>(q, b);
            const int j = __float_as_int(v.w);
            if (d2 < g.gate2 && (d2 < bd || (d2 == bd && j < bi))) { bd = d2; bi = j; }
        }
    }
}

// ---- the distinct buckets (rf_slots27, rf_walk_each, rf_moments) ------------------------------------------------------------------------
constexpr unsigned RF_SEEN = 0xFFFFFFFFu;      // no slot: a slot is below 2^23

__device__ __forceinline__ void rf_load_row(const float* __restrict__ pts, int i, float (&q)[3]) {
    q[0] = pts[3 * (size_t)i];
    q[1] = pts[3 * (size_t)i + 1];
    q[2] = pts[3 * (size_t)i + 2];
}
__device__ __forceinline__ bool rf_finite3(float x, float y, float z) {      // false for a NaN
    return fabsf(x) < __builtin_inff() && fabsf(y) < __builtin_inff() && fabsf(z) < __builtin_inff();
}

// f(c, slot) for the 27 cells c around q in order, unrolled; a slot equal to an earlier one comes as RF_SEEN
template <typename F>
__device__ __forceinline__ void rf_slots27(const RfGrid& g, const float (&q)[3], F&& f) {
    const int cx = rf_cell((double)q[0], g.inv_cell), cy = rf_cell((double)q[1], g.inv_cell), cz = rf_cell((double)q[2], g.inv_cell);
    unsigned slot[27];
#pragma unroll
    for (int c = 0; c < 27; ++c) slot[c] = rf_slot(rf_clampi(cx + c % 3 - 1), rf_clampi(cy + (c / 3) % 3 - 1), rf_clampi(cz + c / 9 - 1), g.mask);
#pragma unroll
    for (int c = 0; c < 27; ++c) {
        bool seen = false;
#pragma unroll
        for (int k = 0; k < c; ++k) seen = seen || slot[k] == slot[c];
        f(c, seen ? RF_SEEN : slot[c]);                                   // a bucket is walked once
    }
}

// every candidate of q among the grid's points, row `self` left out (-1: none): f(d2, j), each once, in no promised order
template <typename F>
__device__ __forceinline__ void rf_walk_each(const RfGrid& g, const float (&q)[3], int self, unsigned (*slots)[256], F&& f) {
    rf_slots27(g, q, [&](int c, unsigned s) { slots[c][threadIdx.x] = s; });
#pragma unroll 1
    for (int c = 0; c < 27; ++c) {
        const unsigned s = slots[c][threadIdx.x];
        if (s == RF_SEEN) continue;
        const int p1 = g.start[s + 1];
        for (int p = g.start[s]; p < p1; ++p) {
            const float4 v = g.pk[p];
            const float b[3] = {v.x, v.y, v.z};
            const float d2 = dist2_f32<3>(q, b);
            const int j = __float_as_int(v.w);
            if (d2 < g.gate2 && j != self) f(d2, j);                      // false for a NaN / inf on either side
        }
    }
}

// the candidates of q, q's own row among them: their number, S1 = SUM d, S2 = SUM d d^T {xx, xy, xz, yy, yz, zz}, d = candidate - q in f64
__device__ __forceinline__ void rf_moments(const RfGrid& g, const float (&q)[3], int& n, double (&S1)[3], double (&S2)[6]) {
    const double px = (double)q[0], py = (double)q[1], pz = (double)q[2];
    n = 0;
    double s1x = 0.0, s1y = 0.0, s1z = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
    rf_slots27(g, q, [&](int, unsigned s) {
        if (s == RF_SEEN) return;
        const int p1 = g.start[s + 1];
        for (int p = g.start[s]; p < p1; ++p) {
            const float4 v = g.pk[p];
            const float b[3] = {v.x, v.y, v.z};
            if (dist2_f32<3>(q, b) < g.gate2) {                           // false for a NaN / inf on either side
                const double dx = (double)v.x - px, dy = (double)v.y - py, dz = (double)v.z - pz;
                ++n;
                s1x += dx; s1y += dy; s1z += dz;
                sxx += dx * dx; sxy += dx * dy; sxz += dx * dz;
                syy += dy * dy; syz += dy * dz; szz += dz * dz;
            }
        }
    });
    S1[0] = s1x; S1[1] = s1y; S1[2] = s1z;
    S2[0] = sxx; S2[1] = sxy; S2[2] = sxz; S2[3] = syy; S2[4] = syz; S2[5] = szz;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
struct RfGridWs {
    unsigned nslots; int bits, nblk;
    unsigned* keys[2]; int* idx[2];
    int* hist; int* start; float4* pk;
};

// the grid's buffers as one run of takes inside the caller's arena layout; the build queues the sort on `s` (rfgrid.hip)
void rf_grid_layout(Arena& ar, int Nt, RfGridWs& w);
int rf_build_grid(const float* tgt, int Nt, float max_dist, const RfGridWs& w, RfGrid& g, hipStream_t s);
inline bool rf_bad_radius(float r) { return !(r > 0.f) || !std::isfinite(r); }

// ---- the refusals the entries share: 0, or YOHO_EINVAL with the error set -----------------------------------------------------------
#define RF_NAMED(limit) #limit, limit          // a limit of the public headers with its name, for the message
#define RF_REFUSE(...) (set_error(__VA_ARGS__), YOHO_EINVAL)
// the context and one or two sizes (nb == nullptr: one) against their smallest values
inline int rf_check_sizes(const char* fn, const void* c, const char* na, int a, int amin, const char* nb = nullptr, int b = 0, int bmin = 0) {
    if (c && a >= amin && (!nb || b >= bmin)) return 0;
    return nb ? RF_REFUSE("%s: bad argument (ctx %p, %s=%d, %s=%d)", fn, c, na, a, nb, b) : RF_REFUSE("%s: bad argument (ctx %p, %s=%d)", fn, c, na, a);
}
// one or two sizes against a named limit
inline int rf_check_limit(const char* fn, const char* limit_name, int limit, const char* na, int a, const char* nb = nullptr, int b = 0) {
    if (a <= limit && (!nb || b <= limit)) return 0;
    return nb ? RF_REFUSE("%s: %s=%d, %s=%d must not exceed %s = %d", fn, na, a, nb, b, limit_name, limit)
              : RF_REFUSE("%s: %s=%d must not exceed %s = %d", fn, na, a, limit_name, limit);
}
// a count (iters, K, H) in [lo, a named maximum]
inline int rf_check_range(const char* fn, const char* name, int v, int lo, const char* max_name, int hi) {
    return v >= lo && v <= hi ? 0 : RF_REFUSE("%s: %s=%d must be in [%d, %s = %d]", fn, name, v, lo, max_name, hi);
}
inline int rf_check_radius(const char* fn, const char* name, float r) {
    return rf_bad_radius(r) ? RF_REFUSE("%s: %s=%g must be finite and > 0", fn, name, (double)r) : 0;
}
inline int rf_check_tol(const char* fn, double tol) { return std::isnan(tol) ? RF_REFUSE("%s: tol is NaN", fn) : 0; }
inline int rf_check_pointers(const char* fn, bool all_there) { return all_there ? 0 : RF_REFUSE("%s: bad argument (a required pointer is NULL)", fn); }
// one cloud of at least one point and the radius of its grid: what the entries over a single cloud refuse first, in that order
inline int rf_check_cloud(const char* fn, const void* c, int N, const char* radius_name, float radius) {
    int rc;
    if ((rc = rf_check_sizes(fn, c, "N", N, 1)) || (rc = rf_check_limit(fn, RF_NAMED(YOHO_REFINE_MAX_POINTS), "N", N))) return rc;
    return rf_check_radius(fn, radius_name, radius);
}
// a source and a target cloud of at least one point each
inline int rf_check_clouds(const char* fn, const void* c, int Ns, int Nt) {
    const int rc = rf_check_sizes(fn, c, "Ns", Ns, 1, "Nt", Nt, 1);
    return rc ? rc : rf_check_limit(fn, RF_NAMED(YOHO_REFINE_MAX_POINTS), "Ns", Ns, "Nt", Nt);
}
// what yoho_icp_refine and yoho_icp_plane refuse before they look at their pointers, in that order
inline int rf_check_icp(const char* fn, const void* c, int Ns, int Nt, int iters, float max_dist, double tol) {
    int rc;
    if ((rc = rf_check_clouds(fn, c, Ns, Nt)) || (rc = rf_check_range(fn, "iters", iters, 0, RF_NAMED(YOHO_ICP_MAX_ITERS))) ||
        (rc = rf_check_radius(fn, "max_dist", max_dist))) return rc;
    return rf_check_tol(fn, tol);
}

}  // namespace yoho
