// Where a wave of the logic kernel puts its 64 vertices within its 64 output positions: those with a bounce ray first.
//
// Russian roulette ends 40 % of the vertices a pass shades, and nothing ever reads the bounce direction or (one light) the throughput of
// a vertex without a bounce ray.  Left in lane order, those vertices sit between the others, and every 128-byte line of these planes is
// written by this pass and read whole by the next one's shade round.  Ranked -- bounce rays first, in lane order; the others after them,
// in lane order -- the tail of every 64-position run holds none of those words: of the four lines a run has per plane, about one is
// never touched.  A position within a pass's output means nothing (every consumer goes through WfState::id), so the frame is the same.
// (Ranked over a block's 256 positions instead, the untouched share of those lines is larger, but the wave totals cost a barrier per
// shade round: the headline frame was 0.7 ms slower than with this form -- profiles/r05_bounce_first.txt.)
//
// Pure, and compiled by the host compiler too (tests/test_bounce_rank_cpu.py).
#pragma once

namespace mcpt {

#ifdef __HIPCC__
#define MCPT_RANK_FN __host__ __device__ __forceinline__
#else
#define MCPT_RANK_FN inline
#endif

// has: bit l set when lane l's vertex has a bounce ray (a lane that takes no part has a clear bit and, being above every lane that
// does, a rank above theirs).  Returns lane's rank: a permutation of 0 .. 63 over the 64 lanes.
MCPT_RANK_FN unsigned int bounce_first_rank(unsigned long long has, int lane)
{
    const unsigned long long below = (1ull << lane) - 1ull;
    if ((has >> lane) & 1ull) return (unsigned int)__builtin_popcountll(has & below);
    return (unsigned int)(__builtin_popcountll(has) + __builtin_popcountll(~has & below));
}

#undef MCPT_RANK_FN

}  // namespace mcpt
