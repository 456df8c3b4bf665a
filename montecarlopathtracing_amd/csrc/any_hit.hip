// Any-hit rays on the GPU (mcpt.h: any-hit rays; any_hit_walk.hpp: the rule and the walk; any_hit.hpp: the pair arithmetic): two kernels for gfx950 beside the
// unchanged closest-hit engines.  One ray per lane, start to finish; a lane that has its answer waits for the longest walk of its wave
// (no refill: DESIGN 6z).  fp64 at the leaves, no contraction (-ffp-contract=off).  wave64, blocks of 256.
//
// Stacks: kFastMaxDepth entries per lane in LDS, lane-interleaved (stack[i * 256]): 36 KB a block, four blocks a CU.  The reference-shaped
// instantiations (FAST = false) walk without a stack and hold no LDS.
// Counters: node steps, triangle tests and rays answered go to the DCounters the closest-hit entry points use.
#include <hip/hip_runtime.h>

#include "accel_build.hpp"
#include "any_hit.hpp"
#include "any_hit_walk.hpp"

namespace mcpt {

constexpr int kAnyBlock = 256;

// occluded[q] = the rule for ray q under its limit (tmax null: +inf).  Grid-stride over the rays.
template <bool FAST>
__global__ void __launch_bounds__(kAnyBlock) k_any_rays(DScene S, const double* __restrict__ rays6, const double* __restrict__ tmax, long long n,
                                                        uint8_t* __restrict__ occluded, DCounters* ctr)
{
    __shared__ int lds_stack[FAST ? kFastMaxDepth * kAnyBlock : 1];
    LaneStats ls;
    Work w = {0, 0};
    const long long step = (long long)gridDim.x * kAnyBlock;
    for (long long q = (long long)blockIdx.x * kAnyBlock + threadIdx.x; q < n; q += step) {
        Ray r;
        r.o = ld3(rays6 + q * 6); r.d = ld3(rays6 + q * 6 + 3);
        const double lim = tmax ? tmax[q] : __builtin_inf();
        const bool occ = FAST ? any_lane_fast(S, r, lim, w, lds_stack + threadIdx.x, kAnyBlock) : any_lane_reference(S, r, lim, w);
        occluded[q] = occ ? 1 : 0;
        ls.primary++;
    }
    ls.nodes = w.nodes; ls.tris = w.tris;
    flush_stats(ctr, ls);
}

// The na x nb matrix of pair_ray(a_i, b_j, t0, t1): one wave per word (i, w) of the packed matrix, grid-stride over the na * W words.
// Lane l forms the ray of column j = 64 w + l in registers -- the rays of a wave share their origin up to t0 * d, so their first node
// steps are coherent -- and the wave votes once, every lane taking part; columns past nb take no walk and vote 0, which is the padding.
template <bool FAST>
__global__ void __launch_bounds__(kAnyBlock) k_any_pairs(DScene S, const double* __restrict__ a3, long long na, const double* __restrict__ b3, long long nb,
                                                         double t0, double t1, unsigned long long* __restrict__ bits, DCounters* ctr)
{
    __shared__ int lds_stack[FAST ? kFastMaxDepth * kAnyBlock : 1];
    LaneStats ls;
    Work w = {0, 0};
    const int lane = threadIdx.x & 63;
    const long long W = pair_row_words(nb), words = na * W;
    const long long step = (long long)gridDim.x * (kAnyBlock / 64);
    for (long long q = (long long)blockIdx.x * (kAnyBlock / 64) + (threadIdx.x >> 6); q < words; q += step) {
        const long long i = q / W, j = ((q - i * W) << 6) + lane;
        bool occ = false;
        if (j < nb) {
            const double a[3] = {a3[i * 3], a3[i * 3 + 1], a3[i * 3 + 2]}, b[3] = {b3[j * 3], b3[j * 3 + 1], b3[j * 3 + 2]};
            const PairRay pr = pair_ray(a, b, t0, t1);
            Ray r;
            r.o = mk(pr.o[0], pr.o[1], pr.o[2]); r.d = mk(pr.d[0], pr.d[1], pr.d[2]);
            occ = FAST ? any_lane_fast(S, r, pr.tmax, w, lds_stack + threadIdx.x, kAnyBlock) : any_lane_reference(S, r, pr.tmax, w);
            ls.primary++;
        }
        const unsigned long long word = __ballot(occ);
        if (lane == 0) bits[q] = word;
    }
    ls.nodes = w.nodes; ls.tris = w.tris;
    flush_stats(ctr, ls);
}

// blocks of a grid-stride launch over `items` block-sized pieces of work: every piece its own block up to 32 blocks a CU (four are
// resident beside their stacks; the rest queue behind them and even out walks of different lengths)
static unsigned any_grid(long long items, int cus)
{
    const long long cap = (long long)(cus > 0 ? cus : 256) * 32;
    return (unsigned)(items < cap ? items : cap);
}

void launch_any_rays(const DScene& S, bool fast, const double* d_rays6, const double* d_tmax, long long n, uint8_t* d_occluded, DCounters* ctr,
                     int cus, hipStream_t st)
{
    if (n <= 0) return;
    const dim3 grid(any_grid((n + kAnyBlock - 1) / kAnyBlock, cus)), block(kAnyBlock);
    if (fast) hipLaunchKernelGGL(k_any_rays<true>, grid, block, 0, st, S, d_rays6, d_tmax, n, d_occluded, ctr);
    else hipLaunchKernelGGL(k_any_rays<false>, grid, block, 0, st, S, d_rays6, d_tmax, n, d_occluded, ctr);
}

void launch_any_pairs(const DScene& S, bool fast, const double* d_a3, long long na, const double* d_b3, long long nb, double t0, double t1,
                      unsigned long long* d_bits, DCounters* ctr, int cus, hipStream_t st)
{
    if (na <= 0 || nb <= 0) return;
    const long long words = na * pair_row_words(nb);
    const dim3 grid(any_grid((words + kAnyBlock / 64 - 1) / (kAnyBlock / 64), cus)), block(kAnyBlock);
    if (fast) hipLaunchKernelGGL(k_any_pairs<true>, grid, block, 0, st, S, d_a3, na, d_b3, nb, t0, t1, d_bits, ctr);
    else hipLaunchKernelGGL(k_any_pairs<false>, grid, block, 0, st, S, d_a3, na, d_b3, nb, t0, t1, d_bits, ctr);
}

}  // namespace mcpt
