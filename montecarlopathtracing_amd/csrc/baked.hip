// Baked frames' kernels (mcpt.h: baked frames): the lightmap's lookup by chart coordinate, the camera rays of a chunk of pixels, the shading
// of closest hits under a baked source -- an irradiance volume or a lightmap -- and the fold of a pixel's samples.  The rays are answered
// by the unchanged closest-hit launch (kernels.hip: launch_trace_closest_leaf) between the kernels here.  The arithmetic is baked.hpp's,
// volume.hpp's and visibility.hpp's, the copies the host forms compile; the surface is vertex_surface's and hit_normal's, what shading and
// mcpt_trace_closest form.  fp64 throughout, no contraction (-ffp-contract=off).  Every output is one lane's, every sum in a fixed order;
// no atomics, no LDS: a result depends neither on the grid of the launch nor on the chunking nor on the device.
#include <hip/hip_runtime.h>

#include "baked.hpp"
#include "baked_surface.hpp"
#include "camera.hpp"
#include "dev_common.hpp"
#include "env.hpp"
#include "shade_common.hpp"
#include "vertex.hpp"

namespace mcpt {

static constexpr int kBakedBlock = 256;

// the source kinds as the shading kernels are instantiated: one lookup each, so that none carries another's registers
enum { kSrcVolume = 0, kSrcVolumeVisible = 1, kSrcLightmap = 2 };

// ---- lookup: one lane per chart coordinate, all three channels from the four texels around it
__global__ void __launch_bounds__(kBakedBlock) k_lightmap_irradiance(int W, int H, const double* __restrict__ irr, const int32_t* __restrict__ owner,
                                                                     const double* __restrict__ uv2, long long n, double* __restrict__ e3,
                                                                     int32_t* __restrict__ taps)
{
    const long long i = (long long)blockIdx.x * kBakedBlock + threadIdx.x;
    if (i >= n) return;
    double E[3];
    const int c = baked_lightmap_lookup(W, H, irr, owner, uv2[i * 2], uv2[i * 2 + 1], E);
    for (int k = 0; k < 3; k++) e3[i * 3 + k] = E[k];
    if (taps) taps[i] = c;
}

// ---- camera rays: one lane per ray of the chunk, sample-major, six fp64 stores
__global__ void __launch_bounds__(kBakedBlock) k_baked_camera_rays(DLens lens, unsigned long long seed, int first, int n, int G, double* __restrict__ rays6)
{
    const long long j = (long long)blockIdx.x * kBakedBlock + threadIdx.x;
    if (j >= (long long)n * G) return;
    const int k = (int)(j / n), i = (int)(j % n);
    V3 o, d;
    camera_ray(lens, seed, first + i, k, o, d);
    double* r = rays6 + j * 6;
    r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = d.x; r[4] = d.y; r[5] = d.z;
}

// What one sample shows.  Everything but L, kind and face stays +0.0 / 0 unless the sample is a surface hit.
struct BakedSample {
    double L[3], q[6], uv[2], kd[3], E[3];
    int kind, face, lit;
};

// One ray d with its closest hit (lf < 0: none) under source B (mcpt.h: baked frames, "baked radiance").
template <int SRC>
__device__ __forceinline__ void baked_sample(const DScene& S, const BakedSource& B, int flags, const V3& d, int lf, double t, const V3& p, BakedSample& r)
{
    for (int c = 0; c < 3; c++) { r.L[c] = 0.0; r.kd[c] = 0.0; r.E[c] = 0.0; }
    for (int c = 0; c < 6; c++) r.q[c] = 0.0;
    r.uv[0] = r.uv[1] = 0.0;
    r.kind = MCPT_BAKED_MISS; r.face = -1; r.lit = 0;
    if (lf < 0) {
        if (env_on(S.env)) {
            const V3 le = env_eval(S.env, d);
            r.L[0] = le.x; r.L[1] = le.y; r.L[2] = le.z;
        }
        return;
    }
    const DTri* tr = S.tris + lf;
    const DMaterial* m = S.materials + tr->material;
    r.face = tr->face;
    if (m->light >= 0) {
        const double* rad = S.lights[m->light].radiance;
        r.kind = MCPT_BAKED_EMITTER;
        r.L[0] = rad[0]; r.L[1] = rad[1]; r.L[2] = rad[2];
        return;
    }
    r.kind = MCPT_BAKED_SURFACE;
    V3 pn, kd;
    vertex_surface(S, lf, p, m, pn, kd);
    Hit h;
    h.leaf = lf; h.t = t; h.p = p;
    pn = hit_normal(S, h);
    double n[3] = {pn.x, pn.y, pn.z};
    baked_normal_rule(tr, d, flags, n);
    r.kd[0] = kd.x; r.kd[1] = kd.y; r.kd[2] = kd.z;
    r.q[0] = p.x; r.q[1] = p.y; r.q[2] = p.z;
    for (int c = 0; c < 3; c++) r.q[3 + c] = n[c];
    if constexpr (SRC == kSrcLightmap) {
        const V3 g = barycentric(ld3(tr->v1), ld3(tr->v2), ld3(tr->v3), p);
        double uv[6];
        if (B.uv6) {
            const double* c6 = B.uv6 + (size_t)tr->face * 6;
            for (int c = 0; c < 6; c++) uv[c] = c6[c];
        } else {
            const DTriShade& s = S.shade[lf];
            uv[0] = s.vt1[0]; uv[1] = s.vt1[1]; uv[2] = s.vt2[0]; uv[3] = s.vt2[1]; uv[4] = s.vt3[0]; uv[5] = s.vt3[1];
        }
        baked_chart_uv(uv, g.x, g.y, g.z, r.uv);
        r.lit = baked_lightmap_lookup(B.width, B.height, B.irr, B.owner, r.uv[0], r.uv[1], r.E);
    } else {
        int32_t P[8];
        double w[8], AY[MCPT_SH_N];
        if constexpr (SRC == kSrcVolumeVisible) r.lit = visibility_corners(B.grid, B.vis, B.moments, B.valid, r.q, P, w);
        else r.lit = volume_corners(B.grid, B.valid, r.q, P, w);
        volume_lobe9(r.q + 3, AY);
        volume_eval(B.sh27, P, w, AY, r.lit > 0, (B.grid.flags & MCPT_VOLUME_CLAMP_ZERO) != 0, r.E);
    }
    baked_surface_radiance(r.kd, r.E, (flags & MCPT_BAKED_LIGHTING_ONLY) != 0, r.L);
}

// ---- shade: one lane per ray; neighbouring lanes are neighbouring rays (of one sample index in a frame), whose hits mostly share
// triangles, probes and texels
template <int SRC>
__global__ void __launch_bounds__(kBakedBlock) k_baked_shade(DScene S, BakedSource B, int flags, const double* __restrict__ rays6,
                                                             const int32_t* __restrict__ leaf, const double* __restrict__ t,
                                                             const double* __restrict__ p, long long n, BakedOut o)
{
    const long long i = (long long)blockIdx.x * kBakedBlock + threadIdx.x;
    if (i >= n) return;
    const int lf = leaf[i];
    BakedSample r;
    baked_sample<SRC>(S, B, flags, ld3(rays6 + i * 6 + 3), lf, lf >= 0 ? t[i] : 0.0, lf >= 0 ? ld3(p + i * 3) : mk(0, 0, 0), r);
    if (o.radiance3) for (int c = 0; c < 3; c++) o.radiance3[i * 3 + c] = r.L[c];
    if (o.kind) o.kind[i] = r.kind;
    if (o.face) o.face[i] = r.face;
    if (o.q6) for (int c = 0; c < 6; c++) o.q6[i * 6 + c] = r.q[c];
    if (o.uv2) { o.uv2[i * 2] = r.uv[0]; o.uv2[i * 2 + 1] = r.uv[1]; }
    if (o.kd3) for (int c = 0; c < 3; c++) o.kd3[i * 3 + c] = r.kd[c];
    if (o.e3) for (int c = 0; c < 3; c++) o.e3[i * 3 + c] = r.E[c];
    if (o.lit) o.lit[i] = r.lit;
}

// ---- fold: one lane per pixel of the chunk, its G samples in k order (consecutive lanes read consecutive records for a fixed k).  One lane
// per pixel that also shades its G samples in a loop (no per-sample records at all) needs 142 to 256 registers, one to three waves per
// SIMD, and measured 17 % slower under a visible volume at G = 16 and within 2 % elsewhere; it was removed.
__global__ void __launch_bounds__(kBakedBlock) k_baked_fold(int first, int n, int G, const double* __restrict__ rad3, const int32_t* __restrict__ kind,
                                                            const int32_t* __restrict__ lit, double* __restrict__ img, int32_t* __restrict__ counts3,
                                                            int32_t* __restrict__ litcount)
{
    const int i = blockIdx.x * kBakedBlock + threadIdx.x;
    if (i >= n) return;
    double s[3] = {0.0, 0.0, 0.0};
    int ns = 0, ne = 0, nm = 0, nlit = 0;
    for (int k = 0; k < G; k++) {
        const long long j = (long long)k * n + i;
        const int kd = kind[j];
        for (int c = 0; c < 3; c++) s[c] += rad3[j * 3 + c];
        ns += kd == MCPT_BAKED_SURFACE ? 1 : 0;
        ne += kd == MCPT_BAKED_EMITTER ? 1 : 0;
        nm += kd == MCPT_BAKED_MISS ? 1 : 0;
        nlit += kd == MCPT_BAKED_SURFACE && lit[j] > 0 ? 1 : 0;
    }
    const size_t pix = (size_t)(first + i);
    for (int c = 0; c < 3; c++) img[pix * 3 + c] = s[c] / (double)G;
    if (counts3) { counts3[pix * 3] = ns; counts3[pix * 3 + 1] = ne; counts3[pix * 3 + 2] = nm; }
    if (litcount) litcount[pix] = nlit;
}

static inline unsigned blocks_of(long long n) { return (unsigned)((n + kBakedBlock - 1) / kBakedBlock); }
static inline int source_kind(const BakedSource& B) { return B.kind == MCPT_BAKED_LIGHTMAP ? kSrcLightmap : (B.visible ? kSrcVolumeVisible : kSrcVolume); }

void launch_lightmap_irradiance(int W, int H, const double* d_irr, const int32_t* d_owner, const double* d_uv2, int64_t n, double* d_e3, int32_t* d_taps,
                                hipStream_t st)
{
    hipLaunchKernelGGL(k_lightmap_irradiance, dim3(blocks_of((long long)n)), dim3(kBakedBlock), 0, st, W, H, d_irr, d_owner, d_uv2, (long long)n, d_e3, d_taps);
}

void launch_baked_camera_rays(const DLens& lens, unsigned long long seed, const BakedChunk& c, double* d_rays6, hipStream_t st)
{
    hipLaunchKernelGGL(k_baked_camera_rays, dim3(blocks_of((long long)c.n * c.G)), dim3(kBakedBlock), 0, st, lens, seed, c.first, c.n, c.G, d_rays6);
}

void launch_baked_shade(const DScene& S, const BakedSource& B, int flags, const double* d_rays6, const int32_t* d_leaf, const double* d_t,
                        const double* d_p, long long n, const BakedOut& o, hipStream_t st)
{
    const dim3 grid(blocks_of(n)), block(kBakedBlock);
    switch (source_kind(B)) {
    case kSrcLightmap: hipLaunchKernelGGL(k_baked_shade<kSrcLightmap>, grid, block, 0, st, S, B, flags, d_rays6, d_leaf, d_t, d_p, n, o); break;
    case kSrcVolumeVisible: hipLaunchKernelGGL(k_baked_shade<kSrcVolumeVisible>, grid, block, 0, st, S, B, flags, d_rays6, d_leaf, d_t, d_p, n, o); break;
    default: hipLaunchKernelGGL(k_baked_shade<kSrcVolume>, grid, block, 0, st, S, B, flags, d_rays6, d_leaf, d_t, d_p, n, o); break;
    }
}

void launch_baked_fold(const BakedChunk& c, const double* d_rad3, const int32_t* d_kind, const int32_t* d_lit, double* d_img, int32_t* d_counts3,
                       int32_t* d_litcount, hipStream_t st)
{
    hipLaunchKernelGGL(k_baked_fold, dim3(blocks_of(c.n)), dim3(kBakedBlock), 0, st, c.first, c.n, c.G, d_rad3, d_kind, d_lit, d_img, d_counts3, d_litcount);
}

}  // namespace mcpt
