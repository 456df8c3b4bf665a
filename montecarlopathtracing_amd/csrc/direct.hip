// Direct light from a caller's own lights on the GPU (mcpt.h: direct light; direct.hpp: the arithmetic; any_hit_walk.hpp: the rule and the
// walk of a shadow ray): the first consumer of any_lane_fast, beside the unchanged any-hit kernels and closest-hit engines.  One
// receiver per lane, grid-stride; the lane loops over the lights and, inside a rectangle, over its samples, forms each shadow ray in
// registers, walks it and folds in the order mcpt.h writes: no atomics, no workspace, no cross-lane sum, so an answer depends neither on
// the grid nor on the device.  Every lane of a wave shoots at the same light at the same time (the light table is read with wave-uniform
// indices) from neighbouring receivers.  fp64, no contraction (-ffp-contract=off).  wave64, blocks of 256.
//
// Stacks: as any_hit.hip's -- kFastMaxDepth entries per lane in LDS, lane-interleaved: 36 KB a block, four blocks a CU; FAST = false walks
// without a stack and holds no LDS.  Counters: node steps, triangle tests and shadow rays walked (rays_primary) go to the DCounters the
// closest-hit entry points use.
#include <hip/hip_runtime.h>

#include "accel_build.hpp"
#include "any_hit_walk.hpp"
#include "direct.hpp"

namespace mcpt {

constexpr int kDirectBlock = 256;

// xi1, xi2 of sample k of light l for the entry with id `id`: words 0 and 1 of the light's block at MCPT_DIRECT_RNG_DEPTH
__device__ __forceinline__ void direct_uniforms(unsigned long long seed, int id, int k, int l, double& xi1, double& xi2)
{
    RngKey key; key.k0 = (uint32_t)seed; key.k1 = (uint32_t)(seed >> 32); key.pixel = (uint32_t)id; key.sample = (uint32_t)k;
    double u2, u3;
    uniform4(key, MCPT_DIRECT_RNG_DEPTH, (uint32_t)l, xi1, xi2, u2, u3);
}

// entry i of the call: its position, its n^ and its id
__device__ __forceinline__ int direct_entry(const DirectCall& c, long long i, double* a, double* nh)
{
    const double* q = c.q6 + i * 6;
    a[0] = q[0]; a[1] = q[1]; a[2] = q[2];
    const double b[3] = {q[3], q[4], q[5]};
    direct_normal(b, nh);
    return c.ids ? c.ids[i] : (int)i;
}

template <bool FAST>
__global__ void __launch_bounds__(kDirectBlock) k_direct(DScene S, DirectCall c, double* __restrict__ irr, double* __restrict__ err,
                                                         double* __restrict__ per_light, double* __restrict__ vis, DCounters* ctr)
{
    __shared__ int lds_stack[FAST ? kFastMaxDepth * kDirectBlock : 1];
    LaneStats ls;
    Work w = {0, 0};
    const long long step = (long long)gridDim.x * kDirectBlock;
    for (long long i = (long long)blockIdx.x * kDirectBlock + threadIdx.x; i < c.n; i += step) {
        double a[3], nh[3];
        const int id = direct_entry(c, i, a, nh);
        DirectFold f;
        f.begin();
        for (int l = 0; l < c.nl; l++) {
            const DirectLight& D = c.lights[l];
            const int slots = direct_light_slots(D.type, c.spp);
            f.light_begin();
            for (int j = 0; j < slots; j++) {
                double xi1 = 0.0, xi2 = 0.0;
                if (D.type == MCPT_LIGHT_RECT) direct_uniforms(c.seed, id, c.sample_base + j, l, xi1, xi2);
                const DirectSlot s = direct_slot(D, a, nh, c.bias, xi1, xi2);
                bool occ = false;
                if (s.g > 0.0) {
                    Ray r;
                    r.o = mk(s.o[0], s.o[1], s.o[2]); r.d = mk(s.d[0], s.d[1], s.d[2]);
                    occ = FAST ? any_lane_fast(S, r, s.tmax, w, lds_stack + threadIdx.x, kDirectBlock) : any_lane_reference(S, r, s.tmax, w);
                    ls.primary++;
                }
                f.add(D, s.g, occ);
            }
            f.light_end(D, c.spp);
            if (per_light) {
                double* o = per_light + (i * c.nl + l) * 3;
                o[0] = f.El[0]; o[1] = f.El[1]; o[2] = f.El[2];
            }
            if (vis) vis[i * c.nl + l] = f.vis;
        }
        irr[i * 3] = f.E[0]; irr[i * 3 + 1] = f.E[1]; irr[i * 3 + 2] = f.E[2];
        if (err) { err[i * 3] = sqrt(f.V[0]); err[i * 3 + 1] = sqrt(f.V[1]); err[i * 3 + 2] = sqrt(f.V[2]); }
    }
    ls.nodes = w.nodes; ls.tris = w.tris;
    flush_stats(ctr, ls);
}

// The seam: the slots of every entry as k_direct forms them, written out.  One lane per entry; slot (l, j) of entry i sits at i * R + the
// slots of the lights before l + j.
__global__ void __launch_bounds__(kDirectBlock) k_direct_rays(DirectCall c, long long R, double* __restrict__ rays6, double* __restrict__ tmax,
                                                              double* __restrict__ g)
{
    const long long i = (long long)blockIdx.x * kDirectBlock + threadIdx.x;
    if (i >= c.n) return;
    double a[3], nh[3];
    const int id = direct_entry(c, i, a, nh);
    long long at = i * R;
    for (int l = 0; l < c.nl; l++) {
        const DirectLight& D = c.lights[l];
        const int slots = direct_light_slots(D.type, c.spp);
        for (int j = 0; j < slots; j++, at++) {
            double xi1 = 0.0, xi2 = 0.0;
            if (D.type == MCPT_LIGHT_RECT) direct_uniforms(c.seed, id, c.sample_base + j, l, xi1, xi2);
            const DirectSlot s = direct_slot(D, a, nh, c.bias, xi1, xi2);
            double* o = rays6 + at * 6;
            o[0] = s.o[0]; o[1] = s.o[1]; o[2] = s.o[2]; o[3] = s.d[0]; o[4] = s.d[1]; o[5] = s.d[2];
            tmax[at] = s.tmax;
            g[at] = s.g;
        }
    }
}

// ---- a map's scatter: `width` doubles of list entry i go to texel T = texels[i], unchanged (the lightmap's own scatter turns a mean
// radiance into irradiance by a factor pi, which has no place here).  One lane per double.
__global__ void __launch_bounds__(kDirectBlock) k_direct_scatter(const int32_t* __restrict__ texels, long long items, int width, const double* __restrict__ in,
                                                                 double* __restrict__ out)
{
    const long long q = (long long)blockIdx.x * kDirectBlock + threadIdx.x;
    if (q >= items) return;
    const long long i = q / width, c = q - i * width;
    out[(size_t)texels[i] * (size_t)width + (size_t)c] = in[q];
}

// blocks of a grid-stride launch over `items` block-sized pieces of work (any_hit.hip: any_grid): every piece its own block up to 32
// blocks a CU
static unsigned direct_grid(long long items, int cus)
{
    const long long cap = (long long)(cus > 0 ? cus : 256) * 32;
    return (unsigned)(items < cap ? items : cap);
}

void launch_direct(const DScene& S, bool fast, const DirectCall& c, double* d_irradiance3, double* d_stderr3, double* d_per_light3, double* d_visibility,
                   DCounters* ctr, int cus, hipStream_t st)
{
    if (c.n <= 0) return;
    const dim3 grid(direct_grid((c.n + kDirectBlock - 1) / kDirectBlock, cus)), block(kDirectBlock);
    if (fast) hipLaunchKernelGGL(k_direct<true>, grid, block, 0, st, S, c, d_irradiance3, d_stderr3, d_per_light3, d_visibility, ctr);
    else hipLaunchKernelGGL(k_direct<false>, grid, block, 0, st, S, c, d_irradiance3, d_stderr3, d_per_light3, d_visibility, ctr);
}

void launch_direct_rays(const DirectCall& c, long long R, double* d_rays6, double* d_tmax, double* d_g, hipStream_t st)
{
    if (c.n <= 0 || R <= 0) return;
    hipLaunchKernelGGL(k_direct_rays, dim3((unsigned)((c.n + kDirectBlock - 1) / kDirectBlock)), dim3(kDirectBlock), 0, st, c, R, d_rays6, d_tmax, d_g);
}

void launch_direct_scatter(const int32_t* d_texels, long long n_list, int width, const double* d_in, double* d_out, hipStream_t st)
{
    const long long items = n_list * width;
    if (items <= 0 || !d_out) return;
    hipLaunchKernelGGL(k_direct_scatter, dim3((unsigned)((items + kDirectBlock - 1) / kDirectBlock)), dim3(kDirectBlock), 0, st, d_texels, items, width, d_in,
                       d_out);
}

}  // namespace mcpt
