// Distance arithmetic shared by the brute-force and the grid nearest-neighbour kernels (match.hip, knn.hip, estim.hip,
// gridnn.hip; the tile, key and minimum they share: nntile.h): explicit round-to-nearest intrinsics in the summation order the reference's CPU reduction uses
// (pinned by tests/golden/pdist.npz); the translation units that include this are built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace yoho {

template <int D>
__device__ __forceinline__ float dist2_f32(const float* a, const float* b) {
    if constexpr (D == 32) {
        float l[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { const float d = __fsub_rn(a[k], b[k]); l[k] = __fmul_rn(d, d); }
#pragma unroll
        for (int blk = 1; blk < 4; ++blk)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float d = __fsub_rn(a[8 * blk + k], b[8 * blk + k]);
                l[k] = __fadd_rn(l[k], __fmul_rn(d, d));
            }
        float s = l[0];
#pragma unroll
        for (int k = 1; k < 8; ++k) s = __fadd_rn(s, l[k]);
        return s;
    } else {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const float d = __fsub_rn(a[k], b[k]);
            const float q = __fmul_rn(d, d);
            s = k == 0 ? q : __fadd_rn(s, q);
        }
        return s;
    }
}

// pdist 'L2': sqrt(D2 + 1e-7) as torch evaluates it on fp32 (utils/knn_search.py:17-20)
__device__ __forceinline__ float dist_of_f32(float d2) { return (float)sqrt((double)__fadd_rn(d2, 1e-7f)); }

// The first-minimum rule of the brute-force searches (nn32seg_kernel): does a LATER target with squared distance d2
// replace the best so far (squared distance `best`)?  SquareL2: d2 < best.  L2: only a strictly smaller ROUNDED distance does, and
// what decides are the sums s = fl(d2 + e), sb = fl(best + e), e = 1e-7f, that the square root is taken of, as in knn.hip - a
// relative test on d2 itself (these kernels had `d2 < best (1 - 1e-6)`) is wrong once d2 is small against e: D2 = 1e-9 and
// 1e-9 (1 - 8e-6) are far apart relatively and give the same distance bits.  Addition, square root and rounding are monotone, so
// d2 >= best cannot win.  Below that, the roots are skipped where the sums are PROVEN more than 9e-7 apart, by one fma on d2:
// with c = fl(1 - 1e-6) = 1 - 1.0133e-6, k = 1.1e-13 >= 9e-7 e and u = 2^-24,
//   d2 < t = fl(best c - k)  =>  t > 0 and d2 + e < (best c - k)(1 + u) + e <= (best + e)(1 - 9e-7)      [c (1 + u) <= 1 - 9e-7]
//   =>  s / sb <= (1 - 9e-7)(1 + u) / (1 - u) < 1 - 7.8e-7  =>  sqrt(s) < sqrt(sb)(1 - 3.9e-7)
//   =>  fl(sqrt(s)) <= sqrt(s)(1 + u) < sqrt(sb)(1 - u) <= fl(sqrt(sb)):  strictly smaller.
// Everything else below `best` pays the two f64 roots and their rounded values decide; for best <= 1.1e-13 that is every such d2
// (t <= 0).  The test costs what the old one did (an fma for a multiplication): in nn32seg_kernel some lane of a wave is below its
// best at almost every step, so whatever stands behind `d2 < best` is paid per step (forming both sums there: + 2 % at D = 3,
// profiles/nn_ties.md).  best = +inf (nothing seen yet) takes any finite d2; a NaN d2 never wins.
template <bool SQUARED>
__device__ __forceinline__ bool nn_closer(float d2, float best) {
    if (!(d2 < best)) return false;
    if (SQUARED) return true;
    if (d2 < fmaf(best, 1.0f - 1e-6f, -1.1e-13f)) return true;
    return dist_of_f32(d2) < dist_of_f32(best);
}

// The packed key of the searches (match.hip, matchf.hip, knn.hip, clean.hip): (bits of a distance >= +0) << 32 | index.  Distances are
// non-negative, so the order of the integers is the order of (distance, then lowest index) = the reference's first minimum; atomicMin and
// sorted lists work on the key alone.
constexpr unsigned long long NN_KEY_EMPTY = ~0ull;           // above every real key (indices are < 2^31); a memset of 0xFF bytes
__device__ __forceinline__ unsigned long long nn_key(unsigned dist_bits, unsigned index) { return ((unsigned long long)dist_bits << 32) | index; }
__device__ __forceinline__ float nn_key_dist(unsigned long long key) { return __uint_as_float((unsigned)(key >> 32)); }
__device__ __forceinline__ unsigned nn_key_index(unsigned long long key) { return (unsigned)(key & 0xFFFFFFFFull); }

// one coordinate of keys @ Rg^T in f64 (YOHO_testset.py:157) and the f64 squared distance to a widened f32 point
struct GnMat3 { double m[9]; };
__device__ __forceinline__ double rotate_key_f64(const double* kk, const double* row) {
    return fma(kk[2], row[2], fma(kk[1], row[1], kk[0] * row[0]));
}
__device__ __forceinline__ double dist2_key_f64(const double* kr, double px, double py, double pz) {
    const double d0 = __dsub_rn(kr[0], px), d1 = __dsub_rn(kr[1], py), d2 = __dsub_rn(kr[2], pz);
    return __dadd_rn(__dadd_rn(__dmul_rn(d0, d0), __dmul_rn(d1, d1)), __dmul_rn(d2, d2));
}

// inlier test of one match under one [R|t] (3x4 row-major): the vote of estim.hip and the refit of refine.hip (both built with
// -ffp-contract=off: only the explicit fma() fuses)
__device__ __forceinline__ bool inlier(const double* T, const double* a, const double* b, double d2thr) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double p = __dadd_rn(fma(b[2], T[i * 4 + 2], fma(b[1], T[i * 4 + 1], b[0] * T[i * 4])), T[i * 4 + 3]);
        const double e = __dsub_rn(a[i], p);
        const double q = __dmul_rn(e, e);
        s = i == 0 ? q : __dadd_rn(s, q);
    }
    return s < d2thr;
}

}  // namespace yoho
