// Sample AOVs (mcpt.h: mcpt_progressive_sample_aovs): the guides of the denoiser averaged over each pixel's camera samples, so that they
// show what the frame shows under a lens -- antialiased silhouettes, the blur of what is out of focus.  Three stages per chunk of whole
// pixels: the camera rays of samples 0 .. G-1 (camera_ray, the frame's own), the closest-hit launch (launch_trace_closest_leaf), the fold.
// Rays are laid out sample-major (j = k * n + i), so the fold's lanes read consecutive records for a fixed k.  fp64, no contraction
// (-ffp-contract=off), one lane forms one pixel in k order: no atomics, the same bits on any grid.
#include <hip/hip_runtime.h>

#include "camera.hpp"
#include "denoise.hpp"
#include "dev_common.hpp"
#include "shade_common.hpp"
#include "vertex.hpp"

namespace mcpt {

__global__ void __launch_bounds__(256) k_guide_rays(DLens lens, unsigned long long seed, const int32_t* __restrict__ pixels, int first, int n, int G,
                                                    double* __restrict__ rays6)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (long long)n * G) return;
    const int k = (int)(j / n), i = (int)(j % n);
    V3 o, d;
    camera_ray(lens, seed, pixels[first + i], k, o, d);
    double* r = rays6 + j * 6;
    r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = d.x; r[4] = d.y; r[5] = d.z;
}

// A sample is a miss, an emitter hit (material.light >= 0) or a surface hit; a surface hit adds t, vertex_surface's kd and the closest hit's
// normal (hit_normal: findGarCor's quotients, the pn of mcpt_trace_closest, so the fold is checkable against the fp64 oracle bit for bit)
// divided by its length (a zero normal adds 0).  depth, albedo, normal = the sums / ns (0 when ns == 0).  The guide record: n^ = normal / |normal|,
// t = depth, m = max((ns / G) * albedo, 0.01), filtered = ns > 0 and ne == 0.
__global__ void __launch_bounds__(256) k_guide_fold(DScene S, const int32_t* __restrict__ pixels, int first, int n, int G, const int32_t* __restrict__ leaf,
                                                    const double* __restrict__ t, const double* __restrict__ p, int32_t* __restrict__ counts,
                                                    double* __restrict__ depth, double* __restrict__ normal, double* __restrict__ albedo,
                                                    SampleGuide* __restrict__ guide)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int pix = pixels[first + i];
    int ns = 0, ne = 0, nm = 0;
    double st = 0.0;
    V3 sn = mk(0, 0, 0), sk = mk(0, 0, 0);
    for (int k = 0; k < G; k++) {
        const long long j = (long long)k * n + i;
        const int lf = leaf[j];
        if (lf < 0) { nm++; continue; }
        const DMaterial* m = S.materials + S.tris[lf].material;
        if (m->light >= 0) { ne++; continue; }
        ns++;
        V3 pn, kd;
        Hit h;
        h.leaf = lf; h.t = t[j]; h.p = ld3(p + j * 3);
        vertex_surface(S, lf, h.p, m, pn, kd);
        pn = hit_normal(S, h);
        const double len = sqrt((pn.x * pn.x + pn.y * pn.y) + pn.z * pn.z);
        st += t[j];
        sk.x += kd.x; sk.y += kd.y; sk.z += kd.z;
        sn.x += len > 0.0 ? pn.x / len : 0.0;
        sn.y += len > 0.0 ? pn.y / len : 0.0;
        sn.z += len > 0.0 ? pn.z / len : 0.0;
    }
    const double d = (double)ns;
    const double dep = ns > 0 ? st / d : 0.0;
    const double a[3] = {ns > 0 ? sk.x / d : 0.0, ns > 0 ? sk.y / d : 0.0, ns > 0 ? sk.z / d : 0.0};
    const double nr[3] = {ns > 0 ? sn.x / d : 0.0, ns > 0 ? sn.y / d : 0.0, ns > 0 ? sn.z / d : 0.0};
    counts[(size_t)pix * 3] = ns; counts[(size_t)pix * 3 + 1] = ne; counts[(size_t)pix * 3 + 2] = nm;
    depth[pix] = dep;
    for (int c = 0; c < 3; c++) { normal[(size_t)pix * 3 + c] = nr[c]; albedo[(size_t)pix * 3 + c] = a[c]; }
    SampleGuide g;
    const double len = sqrt((nr[0] * nr[0] + nr[1] * nr[1]) + nr[2] * nr[2]);
    const double cov = d / (double)G;
    for (int c = 0; c < 3; c++) {
        g.n[c] = len > 0.0 ? nr[c] / len : 0.0;
        const double m = cov * a[c];
        g.m[c] = m > 0.01 ? m : 0.01;
    }
    g.t = dep;
    g.filtered = ns > 0 && ne == 0 ? 1 : 0;
    g.pad = 0;
    guide[pix] = g;
}

static inline unsigned blocks_of(long long n, int block) { return (unsigned)((n + block - 1) / block); }

void launch_guide_rays(const DLens& lens, unsigned long long seed, const int32_t* d_pixels, int first, int n, int G, double* d_rays6, hipStream_t st)
{
    if (n <= 0 || G <= 0) return;
    hipLaunchKernelGGL(k_guide_rays, dim3(blocks_of((long long)n * G, 256)), dim3(256), 0, st, lens, seed, d_pixels, first, n, G, d_rays6);
}

void launch_guide_fold(const DScene& S, const int32_t* d_pixels, int first, int n, int G, const int32_t* d_leaf, const double* d_t, const double* d_p,
                       int32_t* d_counts, double* d_depth, double* d_normal, double* d_albedo, SampleGuide* d_guide, hipStream_t st)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_guide_fold, dim3(blocks_of(n, 256)), dim3(256), 0, st, S, d_pixels, first, n, G, d_leaf, d_t, d_p, d_counts, d_depth, d_normal,
                       d_albedo, d_guide);
}

}  // namespace mcpt
