// Probe visibility's kernels (mcpt.h: probe visibility): the rays of a chunk of probes -- the probe query's own draw (query.hpp:
// query_ray, in chunk_kernels.hpp's k_chunk_rays), written into a workspace the unchanged closest-hit launch then answers --, the fold
// of those answers into every probe's octahedral depth moments and hit counts, and the irradiance volume's lookup with a factor per
// corner.  The arithmetic is visibility.hpp's, the copy the host forms compile.  fp64 throughout, no contraction (-ffp-contract=off).
// Every sum is one lane's, in sample order; no atomics, no LDS: a result depends neither on the grid of the launch nor on the chunking
// nor on the device.
#include <hip/hip_runtime.h>

#include "chunk_kernels.hpp"
#include "dev_common.hpp"
#include "device_scene.hpp"
#include "query.hpp"
#include "visibility.hpp"

namespace mcpt {

static constexpr int kVisBlock = 256;
static constexpr int kVisWaves = kVisBlock / 64;

// ---- fold: one wave per probe, a lane per bin (NB = 1: R <= 8) or per four bins (NB = 4: lane l holds bins l, l + 64, l + 128, l + 192).
// The wave reads 64 samples a step, each lane derives its sample's bin and depth, and the 64 (bin, depth) pairs go round the wave in
// sample order: the lane that holds the bin adds.  So a bin's sums are one lane's, added in j order.  Hits and back-face hits are
// counted by ballot.  A lane per (probe, bin) that scans all the probe's samples itself derives every sample's bin R * R times over and
// measured 6.4 times slower (3.47 ms against 0.54 ms for 64^3 probes of 64 samples at R = 8: DESIGN 6r); it was removed.
template <int NB>
__global__ void __launch_bounds__(kVisBlock) k_vis_fold(DScene S, RayChunk c, int R, double max_distance, double max_back_fraction, double* __restrict__ moments,
                                                        int32_t* __restrict__ hits, int32_t* __restrict__ back, uint8_t* __restrict__ valid)
{
    const int lane = threadIdx.x & 63;
    const long long nwaves = (long long)gridDim.x * kVisWaves;
    const int bins = R * R;
    for (long long i = (long long)blockIdx.x * kVisWaves + (threadIdx.x >> 6); i < c.count; i += nwaves) {
        double s1[NB], s2[NB];
        int cnt[NB];
        for (int s = 0; s < NB; s++) { s1[s] = 0.0; s2[s] = 0.0; cnt[s] = 0; }
        int nhit = 0, nback = 0;
        const long long slot0 = i * c.spp;
        for (long long k0 = 0; k0 < c.spp; k0 += 64) {
            const long long k = k0 + lane;
            int b = -1;
            double r = 0.0;
            bool hit = false, behind = false;
            if (k < c.spp) {
                const long long q = slot0 + k;
                const double d[3] = {c.rays6[q * 6 + 3], c.rays6[q * 6 + 4], c.rays6[q * 6 + 5]};
                const int leaf = c.leaf[q];
                hit = leaf >= 0;
                if (hit) behind = visibility_back(d, S.tris[leaf].n);
                r = visibility_depth(hit, c.t[q], max_distance);
                b = visibility_bin(d[0], d[1], d[2], R);
            }
            nhit += __popcll(__ballot(hit));
            nback += __popcll(__ballot(behind));
            const int m = c.spp - k0 < 64 ? int(c.spp - k0) : 64;
            for (int j = 0; j < m; j++) {
                const int bj = wave_read(b, j);
                const double rj = wave_read(r, j);
                const bool mine = (bj & 63) == lane;
#pragma unroll
                for (int s = 0; s < NB; s++)
                    if (mine && (bj >> 6) == s) { cnt[s] += 1; s1[s] += rj; s2[s] += rj * rj; }
            }
        }
        const long long P = c.first + i;
#pragma unroll
        for (int s = 0; s < NB; s++) {
            const int bin = s * 64 + lane;
            if (bin < bins) {
                double* o = moments + (P * bins + bin) * 2;
                o[0] = cnt[s] > 0 ? s1[s] / double(cnt[s]) : -1.0;
                o[1] = cnt[s] > 0 ? s2[s] / double(cnt[s]) : 0.0;
            }
        }
        if (lane == 0) {
            if (hits) hits[P] = nhit;
            if (back) back[P] = nback;
            if (valid) valid[P] = double(nback) <= max_back_fraction * double(c.spp) ? 1 : 0;
        }
    }
}

// ---- lookup: k_vol_irradiance (volume.hip) with a factor per corner: one lane per receiver, 16 more bytes read per corner
__global__ void __launch_bounds__(kVisBlock) k_vol_irradiance_visible(mcpt_volume_grid g, mcpt_volume_visibility vp, const double* __restrict__ sh27,
                                                                      const double* __restrict__ moments, const uint8_t* __restrict__ valid,
                                                                      const double* __restrict__ q6, long long n, double* __restrict__ e3,
                                                                      int32_t* __restrict__ corners)
{
    const long long r = (long long)blockIdx.x * kVisBlock + threadIdx.x;
    if (r >= n) return;
    const double* qr = q6 + r * 6;
    const double q[6] = {qr[0], qr[1], qr[2], qr[3], qr[4], qr[5]};
    int32_t P[8];
    double w[8], AY[MCPT_SH_N], E[3];
    const int c = visibility_corners(g, vp, moments, valid, q, P, w);
    volume_lobe9(q + 3, AY);
    volume_eval(sh27, P, w, AY, c > 0, (g.flags & MCPT_VOLUME_CLAMP_ZERO) != 0, E);
    for (int k = 0; k < 3; k++) e3[r * 3 + k] = E[k];
    if (corners) corners[r] = c;
}

void launch_visibility_rays(const RayChunk& c, hipStream_t st) { launch_chunk_rays<MCPT_QUERY_KIND_SPHERE>(c, st); }

void launch_visibility_fold(const DScene& S, const RayChunk& c, const mcpt_visibility_params& vp, double* d_moments, int32_t* d_hits, int32_t* d_back,
                            uint8_t* d_valid, hipStream_t st)
{
    // (the fold's waves stride over the probes: a grid beyond a few waves per SIMD of the largest device gains nothing)
    const dim3 grid(grid_blocks(c.count, kVisWaves, 1 << 16));
    if (vp.res <= 8)
        hipLaunchKernelGGL(k_vis_fold<1>, grid, dim3(kVisBlock), 0, st, S, c, vp.res, vp.max_distance, vp.max_back_fraction, d_moments, d_hits, d_back, d_valid);
    else
        hipLaunchKernelGGL(k_vis_fold<4>, grid, dim3(kVisBlock), 0, st, S, c, vp.res, vp.max_distance, vp.max_back_fraction, d_moments, d_hits, d_back, d_valid);
}

void launch_volume_irradiance_visible(const mcpt_volume_grid& g, const mcpt_volume_visibility& vp, const double* d_sh27, const double* d_moments,
                                      const uint8_t* d_valid, const double* d_q6, int64_t n, double* d_e3, int32_t* d_corners, hipStream_t st)
{
    hipLaunchKernelGGL(k_vol_irradiance_visible, dim3((unsigned)(((long long)n + kVisBlock - 1) / kVisBlock)), dim3(kVisBlock), 0, st, g, vp, d_sh27, d_moments,
                       d_valid, d_q6, (long long)n, d_e3, d_corners);
}

}  // namespace mcpt
