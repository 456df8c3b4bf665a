// Lenses (mcpt_device_set_lens): a camera ray per sample.  The image-plane points, the mcpt_camera_rays seam, the megakernel and
// mcpt_sample_radiance forms that trace their own camera ray per lane, the wavefront's camera pass (the camera as a vertex -1 whose bounce
// ray the unchanged trace kernels trace) and the folds of the per-sample route.  -ffp-contract=off (Makefile).
#include <hip/hip_runtime.h>

#include "camera.hpp"
#include "dev_common.hpp"
#include "kernels.hpp"
#include "shade_common.hpp"
#include "shade_path.hpp"
#include "vertex.hpp"
#include "wavefront.hpp"

namespace mcpt {

// pos(i,j) with the bits k_primary_dirs forms: pos(i,0) = start - pdy*i, pos(i,j+1) = pos(i,j) + pdx; one thread walks one row
__global__ void k_primary_pos(DCamera cam, double* __restrict__ pos_out)
{
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= cam.height) return;
    const V3 pdx = ld3(cam.pdx);
    V3 pos = ld3(cam.start_point) - ld3(cam.pdy) * (double)row;
    double* out = pos_out + (size_t)row * cam.width * 3;
    for (int j = 0; j < cam.width; j++) {
        out[j * 3] = pos.x; out[j * 3 + 1] = pos.y; out[j * 3 + 2] = pos.z;
        pos = pos + pdx;
    }
}

__global__ void __launch_bounds__(256) k_camera_rays(DLens lens, unsigned long long seed, const int32_t* __restrict__ pix, const int32_t* __restrict__ ks,
                                                     long long n, double* __restrict__ rays6)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n) return;
    V3 o, d;
    camera_ray(lens, seed, pix[gid], ks[gid], o, d);
    double* r = rays6 + gid * 6;
    r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = d.x; r[4] = d.y; r[5] = d.z;
}

// The megakernel with a lens: one lane per camera sample traces its own camera ray (reference-shaped walk) and shades the path from its
// hit, as k_shade_samples does from the pixel's shared one.  Lane (slot, k) -> rad[(slot*spp + k)*3], flags[slot*spp + k].  ENV: an active
// environment (a camera ray that misses gives Le of its direction).  PICK: the pick mode (1: MCPT_LIGHTS_ONE, 2: MCPT_LIGHTS_TREE).
template <bool ENV, int PICK>
__global__ void __launch_bounds__(256) k_shade_samples_lens(DScene S, DLens lens, unsigned long long seed, const int32_t* __restrict__ pixels,
                                                            int first_slot, long long n_samples, int spp, int sample_base, double* __restrict__ rad,
                                                            uint8_t* __restrict__ flags, DCounters* ctr)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    LaneStats ls;
    if (gid < n_samples) {
        const int slot = first_slot + (int)(gid / spp);
        const int k = sample_base + (int)(gid % spp);
        const int pix = pixels ? pixels[slot] : slot;
        Ray r;
        camera_ray(lens, seed, pix, k, r.o, r.d);
        Hit h; Work w = {0, 0};
        const bool ok = trace_closest(S, r, h, w);
        ls.nodes = w.nodes; ls.tris = w.tris; ls.primary = 1; ls.samples = 1;
        double out[3] = {0, 0, 0};
        if (ok) {
            RngKey key; key.k0 = (uint32_t)seed; key.k1 = (uint32_t)(seed >> 32); key.pixel = (uint32_t)pix; key.sample = (uint32_t)k;
            shade_path<ENV, PICK>(S, key, r.d, h, out, ls);
        } else if (ENV) env_camera_miss(S, r.d, out);
        rad[gid * 3] = out[0]; rad[gid * 3 + 1] = out[1]; rad[gid * 3 + 2] = out[2];
        flags[gid] = ok ? 1 : 0;
    }
    flush_stats(ctr, ls);
}

// mcpt_sample_radiance with a lens: arbitrary (pixel, k) pairs
template <bool ENV, int PICK>
__global__ void __launch_bounds__(256) k_sample_radiance_lens(DScene S, DLens lens, unsigned long long seed, const int32_t* __restrict__ pix,
                                                              const int32_t* __restrict__ ks, long long n, double* __restrict__ rgb, DCounters* ctr)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    LaneStats ls;
    if (gid < n) {
        Ray r;
        camera_ray(lens, seed, pix[gid], ks[gid], r.o, r.d);
        Hit h; Work w = {0, 0};
        double out[3] = {0, 0, 0};
        ls.primary = 1; ls.samples = 1;
        if (trace_closest(S, r, h, w)) {
            RngKey key; key.k0 = (uint32_t)seed; key.k1 = (uint32_t)(seed >> 32); key.pixel = (uint32_t)pix[gid]; key.sample = (uint32_t)ks[gid];
            shade_path<ENV, PICK>(S, key, r.d, h, out, ls);
        } else if (ENV) env_camera_miss(S, r.d, out);
        ls.nodes += w.nodes; ls.tris += w.tris;
        rgb[gid * 3] = out[0]; rgb[gid * 3 + 1] = out[1]; rgb[gid * 3 + 2] = out[2];
    }
    flush_stats(ctr, ls);
}

// The camera as vertex -1 of every sample of the chunk: path position j = chunk-local sample id (slot - first_slot) * spp + k, no
// compaction.  Its bounce ray is the camera ray, left from the lens point itself (MCPT_BT_NO_OFFSET; type TRANSMISSION, so that an emitter
// it reaches is not taken for a diffuse bounce's), and it has no shadow rays.  T = 1 and L = 0 are implied: the logic pass of depth 0
// reads neither (wavefront_logic.hip), so 60 bytes per sample are written, not 108.  The queue words are cleared for the trace launch that
// follows, as a logic pass does.
__global__ void __launch_bounds__(256) k_camera_pass(DLens lens, WfArgs a, long long n)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0) {
        a.counts->n_next = (unsigned int)n;
        if (a.queue) { a.queue->head = 0ull; a.queue->slow_count = 0u; a.queue->redo_all = 0u; }
    }
    if (j >= n) return;
    const long long cap = a.cap;
    const int slot = a.first_slot + (int)(j / a.spp);
    const int k = a.sample_base + (int)(j % a.spp);
    const int pix = a.pixels ? a.pixels[slot] : slot;
    V3 o, d;
    camera_ray(lens, a.seed, pix, k, o, d);
    a.out.id[j] = (int32_t)j;
    stc(a.out.p, cap, j, o);
    stc(a.out.bdir, cap, j, d);
    a.out.btype[j] = RT_TRANSMISSION | MCPT_BT_NO_OFFSET;
    for (int l = 0; l < a.nl; l++) a.out.expect[(long long)l * cap + j] = -2;
}

// k_fold_samples / k_fold_progressive for the per-sample route.  A camera ray that missed gives radiance +0.0, which leaves the fold and
// the moments as they are, so a pixel none of whose rays of the pass hit is not read at all: it keeps +0.0 and zero moments from its first
// pass on -- what the per-pixel route writes for a missed pixel.  PROG: the pixel's count of hit samples continues (one
// lane per pixel writes it: c == 0), hit[pix] = count > 0.  One lane per (slot, channel).  ENV: a camera ray that missed has radiance Le
// of its direction, so every pixel folds all its samples into the image and both moments, whether or not any of them hit.
template <bool PROG, bool ENV>
__global__ void k_fold_lens(const double* __restrict__ rad, const uint8_t* __restrict__ flags, const int32_t* __restrict__ pixels, int first_slot,
                            int n_slots, int n, int k0, int N, double* __restrict__ img, double* __restrict__ mom, uint8_t* __restrict__ hit,
                            int32_t* __restrict__ hitcnt)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)n_slots * 3) return;
    const int s = (int)(gid / 3), c = (int)(gid % 3);
    const int slot = first_slot + s;
    const int pix = pixels ? pixels[slot] : slot;
    const double* src = rad + (size_t)s * n * 3 + c;
    const uint8_t* f = flags + (size_t)s * n;
    int h = 0;
    for (int k = 0; k < n; k++) h += f[k];
    const size_t i = (size_t)pix * 3 + c;
    if (!PROG) {
        float acc = 0.0f;
        if (h > 0 || ENV)
            for (int k = 0; k < n; k++) acc = (float)((double)acc + src[(size_t)k * 3] / n);
        img[i] = (double)acc;
        return;
    }
    if (c == 0) {
        const int total = (k0 > 0 ? hitcnt[pix] : 0) + h;
        hitcnt[pix] = total;
        hit[pix] = total > 0 ? 1 : 0;
    }
    double* m = mom + (size_t)pix * 6 + c;
    if (h == 0 && !ENV) {                            // nothing to add: the image and the moments stay (+0.0 from the first pass on)
        if (k0 == 0) { img[i] = 0.0; m[0] = 0.0; m[3] = 0.0; }
        return;
    }
    float acc = k0 > 0 ? (float)img[i] : 0.0f;
    double s1 = k0 > 0 ? m[0] : 0.0, s2 = k0 > 0 ? m[3] : 0.0;
    for (int k = 0; k < n; k++) {
        const double x = src[(size_t)k * 3];
        acc = (float)((double)acc + x / N);
        s1 += x;
        s2 += x * x;
    }
    img[i] = (double)acc;
    m[0] = s1; m[3] = s2;
}

// k_fold_progressive (kernels.hip: keep the two in step) for a piece of a motion frame (mcpt.h: motion blur; the per-pixel route).  The pieces of one pixel are rendered on
// different geometries and cameras, so its primary ray may hit in one and miss in another: a missed piece brings samples of +0.0 -- which
// leave the fold and the moments as they are -- or, ENV, of Le(the piece's primary direction), folded and summed like any other sample.
// hit[pix]: the primary ray hit in some piece so far.  One lane per (slot, channel).
template <bool ENV>
__global__ void k_fold_motion(const double* __restrict__ rad, const int32_t* __restrict__ pixels, const PrimaryHit* __restrict__ hits, int first_slot,
                              int n_slots, int n, int k0, int N, double* __restrict__ img, double* __restrict__ mom, uint8_t* __restrict__ hit, DEnv env,
                              const double* __restrict__ dirs)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)n_slots * 3) return;
    const int s = (int)(gid / 3), c = (int)(gid % 3);
    const int slot = first_slot + s;
    const int pix = pixels ? pixels[slot] : slot;
    const bool h = hits[slot].leaf >= 0;
    if (c == 0) hit[pix] = (uint8_t)((k0 > 0 ? hit[pix] : 0) | (h ? 1 : 0));
    const size_t i = (size_t)pix * 3 + c;
    double* m = mom + (size_t)pix * 6 + c;
    double le = 0.0;
    if (!h) {
        if (ENV) {
            const V3 e = env_eval(env, ld3(dirs + (size_t)pix * 3));
            le = c == 0 ? e.x : (c == 1 ? e.y : e.z);
        } else {
            if (k0 == 0) { img[i] = 0.0; m[0] = 0.0; m[3] = 0.0; }
            return;
        }
    }
    const double* src = rad + (size_t)s * n * 3 + c;
    float acc = k0 > 0 ? (float)img[i] : 0.0f;
    double s1 = k0 > 0 ? m[0] : 0.0, s2 = k0 > 0 ? m[3] : 0.0;
    for (int k = 0; k < n; k++) {
        const double x = h ? src[(size_t)k * 3] : le;
        acc = (float)((double)acc + x / N);
        s1 += x;
        s2 += x * x;
    }
    img[i] = (double)acc;
    m[0] = s1; m[3] = s2;
}

// ------------------------------------------------------------------------------------------------ launchers
static inline unsigned blocks_of(long long n, int block) { return (unsigned)((n + block - 1) / block); }

void launch_primary_pos(const DCamera& cam, double* d_pos, hipStream_t st)
{
    hipLaunchKernelGGL(k_primary_pos, dim3(blocks_of(cam.height, 64)), dim3(64), 0, st, cam, d_pos);
}
void launch_camera_rays(const DLens& lens, unsigned long long seed, const int32_t* d_pix, const int32_t* d_k, long long n, double* d_rays6, hipStream_t st)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_camera_rays, dim3(blocks_of(n, 256)), dim3(256), 0, st, lens, seed, d_pix, d_k, n, d_rays6);
}
void launch_shade_samples_lens(const DScene& S, const DLens& lens, unsigned long long seed, const int32_t* d_pixels, int first_slot, int n_slots, int spp,
                               int sample_base, double* d_rad, uint8_t* d_flags, DCounters* ctr, hipStream_t st)
{
    const long long n = (long long)n_slots * spp;
    if (n <= 0) return;
    const dim3 grid(blocks_of(n, 256));
    with_path_variant(S, [&](auto env, auto pick) {
        hipLaunchKernelGGL((k_shade_samples_lens<env(), pick()>), grid, dim3(256), 0, st, S, lens, seed, d_pixels, first_slot, n, spp, sample_base, d_rad, d_flags, ctr);
    });
}
void launch_sample_radiance_lens(const DScene& S, const DLens& lens, unsigned long long seed, const int32_t* d_pix, const int32_t* d_k, long long n,
                                 double* d_rgb, DCounters* ctr, hipStream_t st)
{
    if (n <= 0) return;
    const dim3 grid(blocks_of(n, 256));
    with_path_variant(S, [&](auto env, auto pick) {
        hipLaunchKernelGGL((k_sample_radiance_lens<env(), pick()>), grid, dim3(256), 0, st, S, lens, seed, d_pix, d_k, n, d_rgb, ctr);
    });
}
void launch_camera_pass(const DLens& lens, const WfArgs& a, long long n_samples, hipStream_t st)
{
    hipLaunchKernelGGL(k_camera_pass, dim3(blocks_of(n_samples > 0 ? n_samples : 1, 256)), dim3(256), 0, st, lens, a, n_samples);
}
void launch_fold_lens(const double* d_rad, const uint8_t* d_flags, const int32_t* d_pixels, int first_slot, int n_slots, int n, int k0, int N,
                      double* d_img, double* d_mom, uint8_t* d_hit, int32_t* d_hitcnt, bool env, hipStream_t st)
{
    if (n_slots <= 0) return;
    const dim3 grid(blocks_of((long long)n_slots * 3, 256));
    if (env) {
        if (d_mom) hipLaunchKernelGGL((k_fold_lens<true, true>), grid, dim3(256), 0, st, d_rad, d_flags, d_pixels, first_slot, n_slots, n, k0, N, d_img, d_mom, d_hit, d_hitcnt);
        else hipLaunchKernelGGL((k_fold_lens<false, true>), grid, dim3(256), 0, st, d_rad, d_flags, d_pixels, first_slot, n_slots, n, k0, N, d_img, d_mom, d_hit, d_hitcnt);
        return;
    }
    if (d_mom) hipLaunchKernelGGL((k_fold_lens<true, false>), grid, dim3(256), 0, st, d_rad, d_flags, d_pixels, first_slot, n_slots, n, k0, N, d_img, d_mom, d_hit, d_hitcnt);
    else hipLaunchKernelGGL((k_fold_lens<false, false>), grid, dim3(256), 0, st, d_rad, d_flags, d_pixels, first_slot, n_slots, n, k0, N, d_img, d_mom, d_hit, d_hitcnt);
}

void launch_fold_motion(const double* d_rad, const int32_t* d_pixels, const PrimaryHit* d_hits, int first_slot, int n_slots, int n, int k0, int N,
                        double* d_img, double* d_mom, uint8_t* d_hit, const DEnv& env, const double* d_dirs, hipStream_t st)
{
    if (n_slots <= 0) return;
    const dim3 grid(blocks_of((long long)n_slots * 3, 256));
    if (env_on(env)) hipLaunchKernelGGL(k_fold_motion<true>, grid, dim3(256), 0, st, d_rad, d_pixels, d_hits, first_slot, n_slots, n, k0, N, d_img, d_mom, d_hit, env, d_dirs);
    else hipLaunchKernelGGL(k_fold_motion<false>, grid, dim3(256), 0, st, d_rad, d_pixels, d_hits, first_slot, n_slots, n, k0, N, d_img, d_mom, d_hit, env, d_dirs);
}

}  // namespace mcpt
