// Ambient occlusion's kernels (mcpt.h: ambient occlusion): the rays of a chunk of entries -- the irradiance query's own draw (query.hpp:
// query_ray; chunk_kernels.hpp: k_chunk_rays), written into the visibility bake's workspace, which the unchanged closest-hit launch then
// answers --, the fold of those answers into every entry's occlusion, error, bent normal and hit counts, and, for a map, the scatter of
// a texel list's answers (its dilation is the lightmap's own kernel on one channel: lightmap.hip).  The arithmetic is occlusion.hpp's,
// the copy the host fold compiles.  fp64 throughout, no contraction (-ffp-contract=off).  Every sum is added in sample order; no
// atomics, no LDS: a result depends neither on the grid of the launch nor on the chunking nor on the device.
#include <hip/hip_runtime.h>

#include "chunk_kernels.hpp"
#include "dev_common.hpp"
#include "device_scene.hpp"
#include "occlusion.hpp"
#include "query.hpp"

namespace mcpt {

static constexpr int kOccBlock = 256;
static constexpr int kOccWaves = kOccBlock / 64;

// sample `slot` of the workspace as the fold reads it
__device__ __forceinline__ OccSample occ_load(const DScene& S, const OccChunk& c, long long slot)
{
    const double d[3] = {c.rays6[slot * 6 + 3], c.rays6[slot * 6 + 4], c.rays6[slot * 6 + 5]};
    const int leaf = c.leaf[slot];
    return occlusion_sample(c.falloff, c.max_distance, d, leaf >= 0, c.t[slot], leaf >= 0 ? S.tris[leaf].n : nullptr);
}

// entry P's answers from its sums
__device__ __forceinline__ void occ_store(const OccChunk& c, long long P, const OccSums& a, double* __restrict__ ao, double* __restrict__ err,
                                          double* __restrict__ bent3, int32_t* __restrict__ hits, int32_t* __restrict__ back)
{
    ao[P] = a.s1 / c.spp;
    if (err) err[P] = occlusion_stderr(a.s1, a.s2, c.spp);
    if (bent3) {
        const double nrm[3] = {c.list[P * 6 + 3], c.list[P * 6 + 4], c.list[P * 6 + 5]};
        double o[3];
        occlusion_bent(a.b, nrm, o);
        bent3[P * 3] = o[0]; bent3[P * 3 + 1] = o[1]; bent3[P * 3 + 2] = o[2];
    }
    if (hits) hits[P] = a.hits;
    if (back) back[P] = a.back;
}

// ---- fold: one wave per entry, waves striding over the chunk's entries.  The wave reads 64 samples a step, coalesced, each lane derives
// its own sample's value and weighted direction, and the 64 samples go round the wave by v_readlane in sample order: every lane adds
// them all, so the five sums are added in j order whatever the launch's shape.  The two counts are ballots.  A lane per entry that scans
// its own samples was measured and removed: 3.49 ms against 4.55 ms of fold in a 2048 x 2048 bake at 64 samples, but 13 %
// slower on the whole bake at 256 -- a chunk then holds too few entries to fill the device -- and a list of few entries would not fill it
// at all.
__global__ void __launch_bounds__(kOccBlock) k_occ_fold(DScene S, OccChunk c, double* __restrict__ ao, double* __restrict__ err, double* __restrict__ bent3,
                                                        int32_t* __restrict__ hits, int32_t* __restrict__ back)
{
    const int lane = threadIdx.x & 63;
    const long long nwaves = (long long)gridDim.x * kOccWaves;
    for (long long i = (long long)blockIdx.x * kOccWaves + (threadIdx.x >> 6); i < c.count; i += nwaves) {
        OccSums a;
        occlusion_clear(a);
        const long long slot0 = i * c.spp;
        for (int k0 = 0; k0 < c.spp; k0 += 64) {
            OccSample s;
            s.v = 0.0; s.dv[0] = 0.0; s.dv[1] = 0.0; s.dv[2] = 0.0; s.near = false; s.behind = false;
            const int m = c.spp - k0 < 64 ? c.spp - k0 : 64;
            if (lane < m) s = occ_load(S, c, slot0 + k0 + lane);
            a.hits += __popcll(__ballot(s.near));
            a.back += __popcll(__ballot(s.behind));
            for (int j = 0; j < m; j++) {
                OccSample r;
                r.v = wave_read(s.v, j);
                r.dv[0] = wave_read(s.dv[0], j); r.dv[1] = wave_read(s.dv[1], j); r.dv[2] = wave_read(s.dv[2], j);
                r.near = false; r.behind = false;       // (counted above)
                occlusion_add(a, r);
            }
        }
        if (lane == 0) occ_store(c, c.first + i, a, ao, err, bent3, hits, back);
    }
}

// ---- a map's scatter: the answers of list entry i go to texel T = texels[i].  One lane per entry.
__global__ void __launch_bounds__(kOccBlock) k_occ_scatter(const int32_t* __restrict__ texels, long long n, const double* __restrict__ ao_in,
                                                           const double* __restrict__ err_in, const double* __restrict__ bent_in,
                                                           const int32_t* __restrict__ hits_in, const int32_t* __restrict__ back_in, double* __restrict__ ao,
                                                           double* __restrict__ err, double* __restrict__ bent3, int32_t* __restrict__ hits,
                                                           int32_t* __restrict__ back)
{
    const long long i = (long long)blockIdx.x * kOccBlock + threadIdx.x;
    if (i >= n) return;
    const size_t T = (size_t)texels[i];
    ao[T] = ao_in[i];
    if (err) err[T] = err_in[i];
    if (bent3)
        for (int ch = 0; ch < 3; ch++) bent3[T * 3 + ch] = bent_in[i * 3 + ch];
    if (hits) hits[T] = hits_in[i];
    if (back) back[T] = back_in[i];
}

void launch_occlusion_rays(const OccChunk& c, hipStream_t st) { launch_chunk_rays<MCPT_QUERY_KIND_HEMISPHERE>(c, st); }

void launch_occlusion_fold(const DScene& S, const OccChunk& c, double* d_ao, double* d_stderr1, double* d_bent3, int32_t* d_hits, int32_t* d_back,
                           hipStream_t st)
{
    // (the fold's waves stride over the entries: a grid beyond a few waves per SIMD of the largest device gains nothing)
    hipLaunchKernelGGL(k_occ_fold, dim3(grid_blocks(c.count, kOccWaves, 1 << 16)), dim3(kOccBlock), 0, st, S, c, d_ao, d_stderr1, d_bent3, d_hits, d_back);
}

void launch_occlusion_scatter(const int32_t* d_texels, long long n_list, const double* ao, const double* err, const double* bent3, const int32_t* hits,
                              const int32_t* back, double* d_ao, double* d_err, double* d_bent3, int32_t* d_hits, int32_t* d_back, hipStream_t st)
{
    if (n_list <= 0) return;
    hipLaunchKernelGGL(k_occ_scatter, dim3(grid_blocks(n_list, kOccBlock, 0x7fffffffll)), dim3(kOccBlock), 0, st, d_texels, n_list, ao, err, bent3, hits, back,
                       d_ao, d_err, d_bent3, d_hits, d_back);
}

}  // namespace mcpt
