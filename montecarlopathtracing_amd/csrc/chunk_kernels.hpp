// Device code the kernels of a call that answers a list chunk by chunk share: the kernel that draws a chunk's rays, the grid of a launch
// over a chunk, and the wave's read of one lane's value.  Included by the .hip files that use it (visibility.hip, occlusion.hip) and by
// nothing else: every other file's object is untouched by what is added here.
#pragma once
#include <hip/hip_runtime.h>

#include "query.hpp"
#include "visibility.hpp"

namespace mcpt {

static constexpr int kChunkBlock = 256;

// the blocks of a launch over n items at per_block items a block: at least one, at most cap
static inline unsigned grid_blocks(long long n, long long per_block, long long cap)
{
    const long long b = (n + per_block - 1) / per_block;
    return (unsigned)(b < cap ? (b > 0 ? b : 1) : cap);
}

// ---- rays: rays6[slot] = query_ray(KIND, ...) of every ray of the chunk, the query's own draw: one lane per ray, six fp64 stores.
// An item of the list is a position (sphere: 3 doubles) or a position and a normal (hemisphere: 6).
template <int KIND>
__global__ void __launch_bounds__(kChunkBlock) k_chunk_rays(RayChunk c, long long n)
{
    constexpr int kStride = KIND == MCPT_QUERY_KIND_SPHERE ? 3 : 6;
    const long long gid = (long long)blockIdx.x * kChunkBlock + threadIdx.x;
    if (gid >= n) return;
    const long long i = c.first + gid / c.spp;
    const int j = int(gid % c.spp);
    V3 o, d;
    query_ray(KIND, c.list + i * kStride, c.seed, c.ids ? c.ids[i] : (int)i, c.sample_base + j, o, d);
    double* r = c.rays6 + gid * 6;
    r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = d.x; r[4] = d.y; r[5] = d.z;
}

template <int KIND>
static inline void launch_chunk_rays(const RayChunk& c, hipStream_t st)
{
    const long long n = c.count * c.spp;
    hipLaunchKernelGGL(k_chunk_rays<KIND>, dim3(grid_blocks(n, kChunkBlock, 0x7fffffffll)), dim3(kChunkBlock), 0, st, c, n);
}

// the value lane `src` (the same for the whole wave) holds
__device__ __forceinline__ int wave_read(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ double wave_read(double v, int src)
{
    const long long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, src), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), src);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

}  // namespace mcpt
