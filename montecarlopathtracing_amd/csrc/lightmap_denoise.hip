// The lightmap denoiser's kernels (mcpt.h: mcpt_lightmap_denoise): an edge-avoiding a-trous filter of an irradiance map in UV space.  A
// frame's filter (denoise.hip) is guided by depth, normal and material; a texel has none of these, and its neighbours in the map need not
// be its neighbours in the world, so the guides are the world position, the normal and the world footprint of every covered texel,
// derived from the chart and the device's current vertices exactly as the baker derives a texel's query (lightmap.hip: k_lm_texels).
// The filter is stated exactly in mcpt.h; tests/lightmap_denoise_ref.py restates it in numpy.  fp64 throughout, no contraction
// (-ffp-contract=off), every sum in a fixed order: one lane forms one output, so the result depends neither on the grid nor on the device.
// No atomics.
#include <hip/hip_runtime.h>

#include "lightmap_denoise.hpp"

namespace mcpt {

static constexpr int kLmdBlock = 256;

// ---- guides: one lane per texel, from the raster's owner[] and slot_of_face[].  Position and normal are k_lm_texels' expressions, so a
// covered texel's (p, n) are its q6 of mcpt_lightmap_texels bit for bit; the record keeps n divided by its length (0 for a zero normal)
// and h, the world length of a texel's side: sqrt(world area of the face / (chart area of the face * W * H)), both areas doubled.
__global__ void __launch_bounds__(kLmdBlock) k_lmd_guide(const DTri* __restrict__ tris, const DTriShade* __restrict__ shade,
                                                         const double* __restrict__ uv6, int W, int H, const int32_t* __restrict__ owner,
                                                         const int32_t* __restrict__ slot_of_face, LightmapGuide* __restrict__ guide)
{
    const int i = blockIdx.x * kLmdBlock + threadIdx.x;
    if (i >= W * H) return;
    LightmapGuide g;
    for (int c = 0; c < 3; c++) g.p[c] = g.n[c] = 0.0;
    g.h = 0.0;
    g.covered = 0;
    g.pad = 0;
    const int f = owner[i];
    if (f >= 0) {
        const int k = slot_of_face[f];
        const DTri& tr = tris[k];
        const DTriShade& s = shade[k];
        double uv[6], e[3], wt[3];
        if (uv6) {
            const double* c = uv6 + (size_t)f * 6;
            for (int j = 0; j < 6; j++) uv[j] = c[j];
        } else {
            uv[0] = s.vt1[0]; uv[1] = s.vt1[1]; uv[2] = s.vt2[0]; uv[3] = s.vt2[1]; uv[4] = s.vt3[0]; uv[5] = s.vt3[1];
        }
        const double area2 = lightmap_area2(uv);
        lightmap_edges(uv, lightmap_centre(i % W, W), lightmap_centre(i / W, H), e);
        for (int c = 0; c < 3; c++) wt[c] = e[c] / area2;
        double nrm[3];
        for (int c = 0; c < 3; c++) {
            g.p[c] = (tr.v1[c] * wt[0] + tr.v2[c] * wt[1]) + tr.v3[c] * wt[2];
            nrm[c] = (s.vn1[c] * wt[0] + s.vn2[c] * wt[1]) + s.vn3[c] * wt[2];
        }
        if (!lightmap_normal_ok(nrm))
            for (int c = 0; c < 3; c++) nrm[c] = tr.n[c];
        const double len = sqrt((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]);
        for (int c = 0; c < 3; c++) g.n[c] = len > 0.0 ? nrm[c] / len : 0.0;
        const double e1[3] = {tr.v2[0] - tr.v1[0], tr.v2[1] - tr.v1[1], tr.v2[2] - tr.v1[2]};
        const double e2[3] = {tr.v3[0] - tr.v1[0], tr.v3[1] - tr.v1[1], tr.v3[2] - tr.v1[2]};
        const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
        const double A2 = sqrt((cx * cx + cy * cy) + cz * cz);
        g.h = sqrt(A2 / (fabs(area2) * (double(W) * double(H))));
        g.covered = 1;
    }
    guide[i] = g;
}

__device__ __forceinline__ double lmd_luminance(double e0, double e1, double e2) { return (0.2126 * e0 + 0.7152 * e1) + 0.0722 * e2; }

// ---- prepare: one lane per texel.  A covered texel's e is its irradiance and v = sum_c (w_c w_c)(se_c se_c) in channel order; there is
// nothing to demodulate, an irradiance carries no albedo.  Without iterations the output is written here: e where covered, +0.0 elsewhere.
// Each lane reads its own texel's inputs before it writes that texel, and nothing else writes `out` before the last iteration, so `out`
// may be `irr`.  A texel that is not covered is never read.
__global__ void __launch_bounds__(kLmdBlock) k_lmd_prepare(const LightmapGuide* __restrict__ guide, int n, const double* irr, const double* __restrict__ err,
                                                           int iterations, LightmapPix* __restrict__ buf, double* out)
{
    const int i = blockIdx.x * kLmdBlock + threadIdx.x;
    if (i >= n) return;
    const bool covered = guide[i].covered != 0;
    LightmapPix r;
    r.e[0] = r.e[1] = r.e[2] = 0.0;
    r.v = 0.0;
    if (covered) {
        const double w[3] = {0.2126, 0.7152, 0.0722};
        double v = 0.0;
        for (int ch = 0; ch < 3; ch++) {
            const double se = err[(size_t)i * 3 + ch];
            r.e[ch] = irr[(size_t)i * 3 + ch];
            v += (w[ch] * w[ch]) * (se * se);
        }
        r.v = v;
    }
    if (iterations == 0) {
        for (int ch = 0; ch < 3; ch++) out[(size_t)i * 3 + ch] = r.e[ch];
        return;
    }
    if (covered) buf[i] = r;
}

// ---- one a-trous iteration at step s, one lane per texel of the map in 16 x 16 tiles (four wave64s: 16 x 4 texels each), in the shape
// of k_denoise_atrous.  Only covered texels work; on the last iteration the others write +0.0 and leave.  g = the 3 x 3 binomial average
// of v over the covered texels of the window (normalised by the weights used); then 25 taps q = p + s (dx, dy), row-major, covered and
// inside the map:
//     w = h5[dx] h5[dy] * N * exp(-D - L),   N = max(0, n_p . n_q)^128 (1 at the centre),
//     D = max(0, |p_q - p_p| / ((h_p s) len(dx, dy)) - 1) / sigma_p (0 at the centre),   L = |lum(e_q) - lum(e_p)| / (sigma_l sqrt(g) + 1e-10),
//     e' = sum w e_q / sum w,   v' = sum w^2 v_q / (sum w)^2.
// D is the excess of the world distance over what a continuous isotropic chart gives at that tap: 0 inside a well-behaved chart, enormous
// across an atlas seam.  A tap's guide and its (e, v) are both addressed by q alone: the two loads are issued together, ahead of the
// test of the covered flag (an uncovered texel's (e, v) record is whatever the buffer held and is dropped unread).
__global__ void __launch_bounds__(256) k_lmd_atrous(int width, int height, int s, const LightmapGuide* __restrict__ guide,
                                                    const LightmapPix* __restrict__ src, LightmapPix* __restrict__ dst, double sigma_l, double sigma_p,
                                                    double* __restrict__ out)
{
    const int x = blockIdx.x * 16 + threadIdx.x, y = blockIdx.y * 16 + threadIdx.y;
    if (x >= width || y >= height) return;
    const size_t pix = (size_t)y * width + x;
    const LightmapGuide gp = guide[pix];
    if (!gp.covered) {
        if (out)
            for (int ch = 0; ch < 3; ch++) out[pix * 3 + ch] = 0.0;
        return;
    }
    const double k3[3] = {0.25, 0.5, 0.25};
    double sv = 0.0, sk = 0.0;
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= height) continue;
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= width) continue;
            const size_t q = (size_t)qy * width + qx;
            const int cov = guide[q].covered;
            const double vq = src[q].v;
            if (!cov) continue;
            const double kw = k3[dx + 1] * k3[dy + 1];
            sv += kw * vq;
            sk += kw;
        }
    }
    const double g = sv / sk;
    const LightmapPix cp = src[pix];
    const double lp = lmd_luminance(cp.e[0], cp.e[1], cp.e[2]);
    const double lden = sigma_l * sqrt(g) + 1e-10;
    const double hs = gp.h * (double)s;
    const double h5[5] = {1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16};
    double sw = 0.0, se[3] = {0.0, 0.0, 0.0}, svv = 0.0;
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + s * dy;
        if (qy < 0 || qy >= height) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + s * dx;
            if (qx < 0 || qx >= width) continue;
            const size_t q = (size_t)qy * width + qx;
            const LightmapGuide gq = guide[q];
            const LightmapPix cq = src[q];
            if (!gq.covered) continue;
            double nw = 1.0, dd = 0.0;
            if (dx != 0 || dy != 0) {
                const double d = (gp.n[0] * gq.n[0] + gp.n[1] * gq.n[1]) + gp.n[2] * gq.n[2];
                nw = d > 0.0 ? d : 0.0;
                for (int j = 0; j < 7; j++) nw = nw * nw;
                const double rx = gq.p[0] - gp.p[0], ry = gq.p[1] - gp.p[1], rz = gq.p[2] - gp.p[2];
                const double dist = sqrt((rx * rx + ry * ry) + rz * rz);
                const double t = dist / (hs * sqrt((double)(dx * dx + dy * dy))) - 1.0;
                dd = (t > 0.0 ? t : 0.0) / sigma_p;
            }
            const double lq = lmd_luminance(cq.e[0], cq.e[1], cq.e[2]);
            const double dl = fabs(lq - lp) / lden;
            const double w = ((h5[dx + 2] * h5[dy + 2]) * nw) * exp(-dd - dl);
            sw += w;
            for (int ch = 0; ch < 3; ch++) se[ch] += w * cq.e[ch];
            svv += (w * w) * cq.v;
        }
    }
    if (out) {
        for (int ch = 0; ch < 3; ch++) out[pix * 3 + ch] = se[ch] / sw;
        return;
    }
    LightmapPix r;
    for (int ch = 0; ch < 3; ch++) r.e[ch] = se[ch] / sw;
    r.v = svv / (sw * sw);
    dst[pix] = r;
}

void launch_lightmap_denoise(const DScene& S, const double* d_uv6, int W, int H, const LightmapWork& w, const double* d_irr, const double* d_err,
                             int iterations, double sigma_l, double sigma_p, LightmapGuide* d_guide, LightmapPix* d_buf0, LightmapPix* d_buf1,
                             double* d_out, hipStream_t st)
{
    const int n = W * H;
    const unsigned blocks = (unsigned)lightmap_blocks((long long)n);
    hipLaunchKernelGGL(k_lmd_guide, dim3(blocks), dim3(kLmdBlock), 0, st, S.tris, S.shade, d_uv6, W, H, w.owner, w.slot_of_face, d_guide);
    hipLaunchKernelGGL(k_lmd_prepare, dim3(blocks), dim3(kLmdBlock), 0, st, d_guide, n, d_irr, d_err, iterations, d_buf0, d_out);
    const dim3 grid((unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16));
    LightmapPix* buf[2] = {d_buf0, d_buf1};
    for (int i = 0; i < iterations; i++) {
        const bool last = i + 1 == iterations;
        hipLaunchKernelGGL(k_lmd_atrous, grid, dim3(16, 16), 0, st, W, H, 1 << i, d_guide, buf[i & 1], buf[(i + 1) & 1], sigma_l, sigma_p,
                           last ? d_out : nullptr);
    }
}

}  // namespace mcpt
