// Which slots of a window a refill of the pool engine takes (trace_pool.hpp, sparse sources).
//
// A wave that refills looks at a window of W <= 128 consecutive source slots, next .. next + W - 1: lane i holds the flags of window
// offsets i and 64 + i, and two ballots give V0 (offsets 0 .. 63) and V1 (offsets 64 .. 127), a set bit for every slot that holds a ray.
// The n_have lanes that claimed a pool slot take the first min(n_valid, n_have) rays of the window in slot order: the ray of rank r goes
// to the claiming lane of rank r.  The window is consumed up to and including the last slot taken, or whole when every ray in it is
// taken (an empty window too): every slot below next + used is empty or taken, none is taken twice, and used >= 1 whenever W >= 1.
//
// The kernel evaluates the per-slot functions below in the lane that holds the slot's flag; refill_window() is the same arithmetic laid
// out over all 128 offsets.  Pure, and compiled by the host compiler too (tests/test_refill_window_cpu.py).  Masks hold no bit at or
// above W (the kernel does not look at a flag outside its window).
#pragma once

namespace mcpt {

#ifdef __HIPCC__
#define MCPT_RW_FN __host__ __device__ __forceinline__
#else
#define MCPT_RW_FN inline
#endif

enum { kRefillWindow = 128 };

// rays in the window
MCPT_RW_FN int refill_n_valid(unsigned long long V0, unsigned long long V1)
{
    return __builtin_popcountll(V0) + __builtin_popcountll(V1);
}

// rank among the window's rays of the slot at offset half * 64 + lane (meaningful where that slot holds one); below_in_half: the rays
// of the slot's own half at lower offsets (the kernel has it from mbcnt, the host from refill_below)
MCPT_RW_FN int refill_rank(unsigned long long V0, int half, int below_in_half)
{
    return (half ? __builtin_popcountll(V0) : 0) + below_in_half;
}
MCPT_RW_FN int refill_below(unsigned long long V, int lane)
{
    return __builtin_popcountll(V & ((1ull << lane) - 1ull));
}

// a ray of this rank is taken by the step; it is the last one taken
MCPT_RW_FN bool refill_taken(int rank, int n_have) { return rank < n_have; }
MCPT_RW_FN bool refill_last(int rank, int n_have) { return rank == n_have - 1; }

// Source slots the step consumes.  last0 / last1: ballots of refill_last over the rays of the two halves (at most one bit in both
// together; none when the window holds fewer than n_have rays).
MCPT_RW_FN int refill_used(unsigned long long last0, unsigned long long last1, int n_valid, int n_have, int W)
{
    if (n_valid <= n_have) return W;                         // every ray of the window is taken: the window is done, empty or not
    return last0 ? __builtin_ctzll(last0) + 1 : 64 + __builtin_ctzll(last1) + 1;   // (n_valid > n_have >= 1: the ray of rank n_have - 1 exists)
}

// Exact unsigned quotient n / d for 0 <= n < 2^31 by one multiplication and one shift: with l = ceil(log2 d) and
// m = floor(2^(31 + l) / d) + 1, m * d - 2^(31 + l) lies in (0, d] <= 2^l, so n * m / 2^(31 + l) exceeds n / d by less than 1 / d and
// its floor is floor(n / d).  d > 2^(l - 1) (or d = 1), so m <= 2^32 - 3: it fits 32 bits, and n * m < 2^63.
struct DivMagic { unsigned int mul; int shift; };
MCPT_RW_FN DivMagic div_magic(unsigned int d)      // 1 <= d < 2^31
{
    int l = 0;
    while ((1ull << l) < d) l++;
    DivMagic r;
    r.mul = (unsigned int)((1ull << (31 + l)) / d + 1ull);
    r.shift = 31 + l;
    return r;
}
MCPT_RW_FN unsigned int div_by_magic(unsigned int n, unsigned int mul, int shift)
{
    return (unsigned int)(((unsigned long long)n * mul) >> shift);
}

#ifndef __HIP_DEVICE_COMPILE__
// The whole window at once: off[r] = window offset of the ray of rank r, for r < *n_take = min(n_valid, n_have); returns used.
inline int refill_window(unsigned long long V0, unsigned long long V1, int n_have, int W, unsigned char off[64], int* n_take)
{
    const int n_valid = refill_n_valid(V0, V1);
    unsigned long long last[2] = {0ull, 0ull};
    const unsigned long long V[2] = {V0, V1};
    for (int half = 0; half < 2; half++)
        for (int lane = 0; lane < 64; lane++) {
            if (!((V[half] >> lane) & 1ull)) continue;
            const int rank = refill_rank(V0, half, refill_below(V[half], lane));
            if (refill_taken(rank, n_have)) off[rank] = (unsigned char)(half * 64 + lane);
            if (refill_last(rank, n_have)) last[half] |= 1ull << lane;
        }
    *n_take = n_valid < n_have ? n_valid : n_have;
    return refill_used(last[0], last[1], n_valid, n_have, W);
}
#endif

#undef MCPT_RW_FN

}  // namespace mcpt
