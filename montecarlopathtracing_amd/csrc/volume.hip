// The irradiance volume's kernels (mcpt.h: irradiance volumes): the positions of a probe grid, which the unchanged probe query then
// answers, and the lookup of a list of receivers between the probes.  The arithmetic is volume.hpp's, the copy the host forms compile.
// fp64 throughout, no contraction (-ffp-contract=off), every sum in a fixed order: one lane forms one output, so the result depends
// neither on the grid of the launch nor on the device.  No atomics, no LDS.
#include <hip/hip_runtime.h>

#include "volume.hpp"

namespace mcpt {

static constexpr int kVolBlock = 256;

// ---- points: one lane per probe, three fp64 stores
__global__ void __launch_bounds__(kVolBlock) k_vol_points(mcpt_volume_grid g, long long n, double* __restrict__ p3)
{
    const long long P = (long long)blockIdx.x * kVolBlock + threadIdx.x;
    if (P >= n) return;
    const long long row = P / g.nx;
    const int ix = int(P - row * g.nx), iy = int(row % g.ny), iz = int(row / g.ny);
    p3[P * 3 + 0] = volume_coord(g, 0, ix);
    p3[P * 3 + 1] = volume_coord(g, 1, iy);
    p3[P * 3 + 2] = volume_coord(g, 2, iz);
}

// ---- lookup: one lane per receiver, all three channels from the eight probes around it (a lane per (receiver, channel) repeats the
// index arithmetic and the basis three times and measured a third slower: DESIGN 6q).  Neighbouring lanes are neighbouring receivers,
// whose corners are mostly the same probes: the gather is served by the caches.
__global__ void __launch_bounds__(kVolBlock) k_vol_irradiance(mcpt_volume_grid g, const double* __restrict__ sh27, const uint8_t* __restrict__ valid,
                                                              const double* __restrict__ q6, long long n, double* __restrict__ e3,
                                                              int32_t* __restrict__ corners)
{
    const long long r = (long long)blockIdx.x * kVolBlock + threadIdx.x;
    if (r >= n) return;
    const double* q = q6 + r * 6;
    const double x[3] = {q[0], q[1], q[2]}, b[3] = {q[3], q[4], q[5]};
    int32_t P[8];
    double w[8], AY[MCPT_SH_N], E[3];
    const int c = volume_corners(g, valid, x, P, w);
    volume_lobe9(b, AY);
    volume_eval(sh27, P, w, AY, c > 0, (g.flags & MCPT_VOLUME_CLAMP_ZERO) != 0, E);
    for (int k = 0; k < 3; k++) e3[r * 3 + k] = E[k];
    if (corners) corners[r] = c;
}

void launch_volume_points(const mcpt_volume_grid& g, double* d_p3, hipStream_t st)
{
    const long long n = volume_probes(g);
    hipLaunchKernelGGL(k_vol_points, dim3((unsigned)((n + kVolBlock - 1) / kVolBlock)), dim3(kVolBlock), 0, st, g, n, d_p3);
}

void launch_volume_irradiance(const mcpt_volume_grid& g, const double* d_sh27, const uint8_t* d_valid, const double* d_q6, int64_t n, double* d_e3,
                              int32_t* d_corners, hipStream_t st)
{
    hipLaunchKernelGGL(k_vol_irradiance, dim3((unsigned)(((long long)n + kVolBlock - 1) / kVolBlock)), dim3(kVolBlock), 0, st, g, d_sh27, d_valid, d_q6,
                       (long long)n, d_e3, d_corners);
}

}  // namespace mcpt
