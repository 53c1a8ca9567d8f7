// The cell-sorted grid over a target cloud, as its users see it: the device-side pieces of a query (rf_cell / rf_slot, RfGrid, rf_walk)
// inline, the workspace and the two host calls that build it (rfgrid.hip, where THE GRID and THE QUERY are described), and the
// refusals the entries of the family share.  The sums and the Kabsch step are in rffit.h.  Include from translation units compiled
// with -ffp-contract=off only.
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
