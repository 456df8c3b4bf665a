// Any-hit rays (mcpt.h: any-hit rays): is anything in the way of a ray before distance tmax?  The one copy of the pair arithmetic
// (pair_ray) and of the word and bit indexing of a packed pair matrix, compiled for the host (any_hit_api.cpp: mcpt_pair_rays;
// tests/any_hit_sanitize_main.cpp) and for the GPU (any_hit.hip: k_any_pairs); tests/any_hit_ref.py restates them.  fp64, no contraction
// (-ffp-contract=off), every expression in the order mcpt.h writes it.  The launch interface of the two kernels is at the end.  The walk
// that answers a ray, and the argument that makes its early exit exact, are any_hit_walk.hpp's: device code, which only any_hit.hip
// includes (a header of its own because the engine headers it is built from do not compile for the host).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#ifndef MCPT_HD
#if defined(__HIPCC__)
#define MCPT_HD __host__ __device__ __forceinline__
#else
#define MCPT_HD inline
#endif
#endif

namespace mcpt {

// ---- the pair arithmetic ----------------------------------------------------------------------------------------------------------
// The ray of the pair (a, b) over the part [t0, t1] of the segment a -> b: d = b - a, o = a + t0 * d (a product, then a sum: two
// roundings per component), tmax = t1 - t0.  In the ray's own parameter b lies at 1 - t0, so (t0, t1) = (0, 1) asks for the open segment.
struct PairRay {
    double o[3], d[3], tmax;
};
MCPT_HD PairRay pair_ray(const double* a, const double* b, double t0, double t1)
{
    PairRay r;
    r.d[0] = b[0] - a[0];
    r.d[1] = b[1] - a[1];
    r.d[2] = b[2] - a[2];
    const double sx = t0 * r.d[0], sy = t0 * r.d[1], sz = t0 * r.d[2];
    r.o[0] = a[0] + sx;
    r.o[1] = a[1] + sy;
    r.o[2] = a[2] + sz;
    r.tmax = t1 - t0;
    return r;
}

// ---- the packed matrix ------------------------------------------------------------------------------------------------------------
// bits[i * W + (j >> 6)], bit j & 63, W = (nb + 63) / 64 words a row; the padding bits of a row's last word are 0.
constexpr int64_t kPairCountMax = 2147483647;           // rows, columns and words of a matrix
MCPT_HD int64_t pair_row_words(int64_t nb) { return (nb + 63) >> 6; }
MCPT_HD int64_t pair_word_index(int64_t i, int64_t W, int64_t j) { return i * W + (j >> 6); }
MCPT_HD uint64_t pair_bit(int64_t j) { return uint64_t(1) << (j & 63); }
// the bits of word w of a row of nb columns that are columns (the others are padding)
MCPT_HD uint64_t pair_word_mask(int64_t nb, int64_t w)
{
    const int64_t left = nb - (w << 6);
    return left >= 64 ? ~uint64_t(0) : (left <= 0 ? uint64_t(0) : (uint64_t(1) << left) - 1);
}
// na * W fits the word count (na, nb in 0 .. kPairCountMax: the product stays below 2^56)
MCPT_HD bool pair_words_ok(int64_t na, int64_t nb) { return na * pair_row_words(nb) <= kPairCountMax; }

// ---- launch interface (any_hit.hip) ----------------------------------------------------------------------------------------------
struct DScene;
struct DCounters;
// occluded[i] = 0 or 1 for rays6[i] with limit d_tmax[i] (d_tmax null: +inf); fast: any_lane_fast, else the definition.  n > 0.
void launch_any_rays(const DScene& S, bool fast, const double* d_rays6, const double* d_tmax, long long n, uint8_t* d_occluded, DCounters* ctr,
                     int cus, hipStream_t st);
// the na x nb matrix of pair_ray(a_i, b_j, t0, t1), one wave per word: all na * W words are written.  na, nb > 0.
void launch_any_pairs(const DScene& S, bool fast, const double* d_a3, long long na, const double* d_b3, long long nb, double t0, double t1,
                      unsigned long long* d_bits, DCounters* ctr, int cus, hipStream_t st);

}  // namespace mcpt
