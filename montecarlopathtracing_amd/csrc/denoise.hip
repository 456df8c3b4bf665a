// First-hit AOVs and the edge-avoiding a-trous denoiser of progressive frames (the spatial filter of SVGF: Dammertz et al. 2010,
// Schied et al. 2017).  The filter is stated exactly in mcpt.h (mcpt_progressive_denoise); tests/denoise_ref.py restates it in numpy.
// fp64 throughout, no contraction (-ffp-contract=off), every sum in a fixed order: one lane forms one output, so the result depends
// neither on the grid nor on the device.
#include <hip/hip_runtime.h>

#include "dev_common.hpp"
#include "denoise.hpp"
#include "shade_common.hpp"
#include "vertex.hpp"

namespace mcpt {

// ---- AOVs: one lane per owned pixel.  The albedo at the hit is vertex_surface's (what shading sees), the normal the closest hit's
// (hit_normal: the pn of mcpt_trace_closest, the oracle's bits), both formed only where shading forms a surface: on a hit of a
// non-emitting material.  A miss: material -1, everything else 0; an emitter: its material and depth, normal and
// albedo 0.  The guide record of a surface pixel carries the normal divided by its length (0 for a zero normal).
__global__ void __launch_bounds__(256) k_primary_aov(DScene S, const int32_t* __restrict__ pixels, int n, const PrimaryHit* __restrict__ hits,
                                                     int32_t* __restrict__ mat, double* __restrict__ depth, double* __restrict__ normal,
                                                     double* __restrict__ albedo, DenoiseGuide* __restrict__ guide)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int pix = pixels[i];
    const PrimaryHit ph = hits[i];
    int32_t material = -1;
    double t = 0.0;
    V3 pn = mk(0, 0, 0), kd = mk(0, 0, 0);
    bool surface = false;
    if (ph.leaf >= 0) {
        material = S.tris[ph.leaf].material;
        t = ph.t;
        const DMaterial* m = S.materials + material;
        if (m->light < 0) {
            Hit h;
            h.leaf = ph.leaf; h.t = ph.t; h.p = mk(ph.p[0], ph.p[1], ph.p[2]);
            vertex_surface(S, ph.leaf, h.p, m, pn, kd);
            pn = hit_normal(S, h);
            surface = true;
        }
    }
    mat[pix] = material;
    depth[pix] = t;
    normal[(size_t)pix * 3] = pn.x; normal[(size_t)pix * 3 + 1] = pn.y; normal[(size_t)pix * 3 + 2] = pn.z;
    albedo[(size_t)pix * 3] = kd.x; albedo[(size_t)pix * 3 + 1] = kd.y; albedo[(size_t)pix * 3 + 2] = kd.z;
    DenoiseGuide g;
    const double len = sqrt((pn.x * pn.x + pn.y * pn.y) + pn.z * pn.z);
    g.n[0] = len > 0.0 ? pn.x / len : 0.0;
    g.n[1] = len > 0.0 ? pn.y / len : 0.0;
    g.n[2] = len > 0.0 ? pn.z / len : 0.0;
    g.t = t;
    g.material = surface ? material : -1;
    g.pad[0] = g.pad[1] = g.pad[2] = 0;
    guide[pix] = g;
}

__device__ __forceinline__ double luminance(double e0, double e1, double e2) { return (0.2126 * e0 + 0.7152 * e1) + 0.0722 * e2; }
__device__ __forceinline__ double demod_albedo(double a) { return a > 0.01 ? a : 0.01; }   // max(albedo, 0.01)

// ---- prepare: one lane per owned pixel.  The estimate is mcpt_progressive_image's (the float fold at k == N, else the fp64 mean), the
// squared standard error its progressive_se2 (0 below two samples).  A surface pixel, when the filter iterates, is demodulated into
// buf: e = c / a, v = sum_c (w_c^2 se2_c / a_c^2) in channel order.  Every other owned pixel -- and every one when there are no
// iterations -- is the output now, as the estimate.  SAMPLES (mcpt_progressive_denoise_guided): the guide is the sample AOVs' record, a
// filtered pixel is demodulated by its m = max(cov * albedo, 0.01) and `albedo` is not read.
template <bool SAMPLES> struct GuideOf { using type = DenoiseGuide; };
template <> struct GuideOf<true> { using type = SampleGuide; };
__device__ __forceinline__ bool filtered(const DenoiseGuide& g) { return g.material >= 0; }
__device__ __forceinline__ bool filtered(const SampleGuide& g) { return g.filtered != 0; }

template <bool SAMPLES>
__global__ void __launch_bounds__(256) k_denoise_prepare(const int32_t* __restrict__ pixels, long long n, const double* __restrict__ img,
                                                         const double* __restrict__ mom, int done, const int32_t* __restrict__ cnt, int N,
                                                         const double* __restrict__ albedo,
                                                         const typename GuideOf<SAMPLES>::type* __restrict__ guide, int iterations,
                                                         DenoisePix* __restrict__ buf, double* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int pix = pixels ? pixels[i] : (int)i;
    const int k = cnt ? cnt[pix] : done;
    const double* m = mom + (size_t)pix * 6;
    double c[3];
    for (int ch = 0; ch < 3; ch++) c[ch] = k == N ? img[(size_t)pix * 3 + ch] : (k > 0 ? m[ch] / k : 0.0);
    if (iterations == 0 || !filtered(guide[pix])) {
        for (int ch = 0; ch < 3; ch++) out[(size_t)pix * 3 + ch] = c[ch];
        return;
    }
    const double w[3] = {0.2126, 0.7152, 0.0722};
    DenoisePix r;
    double v = 0.0;
    for (int ch = 0; ch < 3; ch++) {
        double a;
        if constexpr (SAMPLES) a = guide[pix].m[ch];
        else a = demod_albedo(albedo[(size_t)pix * 3 + ch]);
        const double se2 = k >= 2 ? progressive_se2(m[ch], m[3 + ch], k) : 0.0;
        r.e[ch] = c[ch] / a;
        v += ((w[ch] * w[ch]) * se2) / (a * a);
    }
    r.v = v;
    buf[pix] = r;
}

// ---- one a-trous iteration at step s, one lane per pixel of the frame in 16 x 16 tiles (four wave64s: 16 x 4 pixels each).
// Only surface pixels work.  g = the 3 x 3 binomial average of v over the same-material surface pixels of the window (normalised by
// the weights used); then 25 taps q = p + s (dx, dy), row-major, of the same material inside the frame:
//     w = h[dx] h[dy] * N * exp(-D - L),   N = max(0, n_p . n_q)^128 (1 at the centre),
//     D = |t_q - t_p| / (sigma_z t_p s max(|dx|, |dy|)) (0 at the centre),   L = |lum(e_q) - lum(e_p)| / (sigma_l sqrt(g) + 1e-10),
//     e' = sum w e_q / sum w,   v' = sum w^2 v_q / (sum w)^2.
// The last iteration writes max(albedo, 0.01) * e' to out instead of dst.
// SAMPLES: a window entry or tap counts when it is a filtered pixel inside the frame, whatever its material, and the weight is
//     w = h[dx] h[dy] * N * exp((-D - L) - A),   A = ((|m_q0 - m_p0| + |m_q1 - m_p1|) + |m_q2 - m_p2|) / sigma_a (0 at the centre);
// the last iteration writes m * e'.
template <bool SAMPLES>
__global__ void __launch_bounds__(256) k_denoise_atrous(int width, int height, int s, const typename GuideOf<SAMPLES>::type* __restrict__ guide,
                                                        const DenoisePix* __restrict__ src, DenoisePix* __restrict__ dst, double sigma_l,
                                                        double sigma_z, const double* __restrict__ albedo, double* __restrict__ out, double sigma_a)
{
    const int x = blockIdx.x * 16 + threadIdx.x, y = blockIdx.y * 16 + threadIdx.y;
    if (x >= width || y >= height) return;
    const size_t pix = (size_t)y * width + x;
    using Guide = typename GuideOf<SAMPLES>::type;
    const Guide gp = guide[pix];
    if (!filtered(gp)) return;
    const double k3[3] = {0.25, 0.5, 0.25};
    double sv = 0.0, sk = 0.0;
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= height) continue;
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= width) continue;
            const size_t q = (size_t)qy * width + qx;
            if constexpr (SAMPLES) { if (guide[q].filtered == 0) continue; }
            else { if (guide[q].material != gp.material) continue; }
            const double kw = k3[dx + 1] * k3[dy + 1];
            sv += kw * src[q].v;
            sk += kw;
        }
    }
    const double g = sv / sk;
    const DenoisePix cp = src[pix];
    const double lp = luminance(cp.e[0], cp.e[1], cp.e[2]);
    const double lden = sigma_l * sqrt(g) + 1e-10;
    const double h5[5] = {1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16};
    double sw = 0.0, se[3] = {0.0, 0.0, 0.0}, svv = 0.0;
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + s * dy;
        if (qy < 0 || qy >= height) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + s * dx;
            if (qx < 0 || qx >= width) continue;
            const size_t q = (size_t)qy * width + qx;
            const Guide gq = guide[q];
            if constexpr (SAMPLES) { if (gq.filtered == 0) continue; }
            else { if (gq.material != gp.material) continue; }
            const DenoisePix cq = src[q];
            double nw = 1.0, dz = 0.0, da = 0.0;
            if (dx != 0 || dy != 0) {
                const double d = (gp.n[0] * gq.n[0] + gp.n[1] * gq.n[1]) + gp.n[2] * gq.n[2];
                nw = d > 0.0 ? d : 0.0;
                for (int j = 0; j < 7; j++) nw = nw * nw;
                const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
                dz = fabs(gq.t - gp.t) / (((sigma_z * gp.t) * (double)s) * (double)(ax > ay ? ax : ay));
                if constexpr (SAMPLES) da = ((fabs(gq.m[0] - gp.m[0]) + fabs(gq.m[1] - gp.m[1])) + fabs(gq.m[2] - gp.m[2])) / sigma_a;
            }
            const double lq = luminance(cq.e[0], cq.e[1], cq.e[2]);
            const double dl = fabs(lq - lp) / lden;
            double w;
            if constexpr (SAMPLES) w = ((h5[dx + 2] * h5[dy + 2]) * nw) * exp((-dz - dl) - da);
            else w = ((h5[dx + 2] * h5[dy + 2]) * nw) * exp(-dz - dl);
            sw += w;
            for (int ch = 0; ch < 3; ch++) se[ch] += w * cq.e[ch];
            svv += (w * w) * cq.v;
        }
    }
    if (out) {
        for (int ch = 0; ch < 3; ch++) {
            if constexpr (SAMPLES) out[pix * 3 + ch] = gp.m[ch] * (se[ch] / sw);
            else out[pix * 3 + ch] = demod_albedo(albedo[pix * 3 + ch]) * (se[ch] / sw);
        }
        return;
    }
    DenoisePix r;
    for (int ch = 0; ch < 3; ch++) r.e[ch] = se[ch] / sw;
    r.v = svv / (sw * sw);
    dst[pix] = r;
}

static inline unsigned blocks_of(long long n, int block) { return (unsigned)((n + block - 1) / block); }

void launch_primary_aov(const DScene& S, const int32_t* d_pixels, int n_pixels, const PrimaryHit* d_hits, int32_t* d_mat, double* d_depth,
                        double* d_normal, double* d_albedo, DenoiseGuide* d_guide, hipStream_t st)
{
    if (n_pixels <= 0) return;
    hipLaunchKernelGGL(k_primary_aov, dim3(blocks_of(n_pixels, 256)), dim3(256), 0, st, S, d_pixels, n_pixels, d_hits, d_mat, d_depth, d_normal,
                       d_albedo, d_guide);
}

void launch_denoise(const int32_t* d_pixels, long long n_pixels, int width, int height, const double* d_img, const double* d_mom, int done,
                    const int32_t* d_cnt, int N, const double* d_albedo, const DenoiseGuide* d_guide, int iterations, double sigma_l,
                    double sigma_z, DenoisePix* d_buf0, DenoisePix* d_buf1, double* d_out, hipStream_t st)
{
    if (n_pixels <= 0) return;
    hipLaunchKernelGGL(k_denoise_prepare<false>, dim3(blocks_of(n_pixels, 256)), dim3(256), 0, st, d_pixels, n_pixels, d_img, d_mom, done, d_cnt, N,
                       d_albedo, d_guide, iterations, d_buf0, d_out);
    const dim3 grid(blocks_of(width, 16), blocks_of(height, 16));
    DenoisePix* buf[2] = {d_buf0, d_buf1};
    for (int i = 0; i < iterations; i++) {
        const bool last = i + 1 == iterations;
        hipLaunchKernelGGL(k_denoise_atrous<false>, grid, dim3(16, 16), 0, st, width, height, 1 << i, d_guide, buf[i & 1], buf[(i + 1) & 1], sigma_l,
                           sigma_z, d_albedo, last ? d_out : nullptr, 0.0);
    }
}

void launch_denoise_guided(const int32_t* d_pixels, long long n_pixels, int width, int height, const double* d_img, const double* d_mom, int done,
                           const int32_t* d_cnt, int N, const SampleGuide* d_guide, int iterations, double sigma_l, double sigma_z, double sigma_a,
                           DenoisePix* d_buf0, DenoisePix* d_buf1, double* d_out, hipStream_t st)
{
    if (n_pixels <= 0) return;
    const double* no_albedo = nullptr;
    hipLaunchKernelGGL(k_denoise_prepare<true>, dim3(blocks_of(n_pixels, 256)), dim3(256), 0, st, d_pixels, n_pixels, d_img, d_mom, done, d_cnt, N,
                       no_albedo, d_guide, iterations, d_buf0, d_out);
    const dim3 grid(blocks_of(width, 16), blocks_of(height, 16));
    DenoisePix* buf[2] = {d_buf0, d_buf1};
    for (int i = 0; i < iterations; i++) {
        const bool last = i + 1 == iterations;
        hipLaunchKernelGGL(k_denoise_atrous<true>, grid, dim3(16, 16), 0, st, width, height, 1 << i, d_guide, buf[i & 1], buf[(i + 1) & 1], sigma_l,
                           sigma_z, no_albedo, last ? d_out : nullptr, sigma_a);
    }
}

}  // namespace mcpt
