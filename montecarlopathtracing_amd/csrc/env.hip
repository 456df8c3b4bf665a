// The environment light's test seams (mcpt_environment_eval / mcpt_environment_sample): env.hpp's device functions on caller-given
// directions and (pixel, sample) keys.
#include <hip/hip_runtime.h>

#include "env.hpp"
#include "kernels.hpp"

namespace mcpt {

__global__ void __launch_bounds__(256) k_env_eval(DEnv E, const double* __restrict__ dirs, long long n, double* __restrict__ rgb)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3 le = env_eval(E, ld3(dirs + i * 3));
    rgb[i * 3] = le.x; rgb[i * 3 + 1] = le.y; rgb[i * 3 + 2] = le.z;
}

// out7[i] = direction xyz, pdf, radiance rgb of the block-(nl + 2) draw of vertex `depth` of camera sample (pix[i], k[i])
__global__ void __launch_bounds__(256) k_env_sample(DEnv E, unsigned long long seed, const int32_t* __restrict__ pix, const int32_t* __restrict__ ks,
                                                    int depth, int nl, long long n, double* __restrict__ out7)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    RngKey key; key.k0 = (uint32_t)seed; key.k1 = (uint32_t)(seed >> 32); key.pixel = (uint32_t)pix[i]; key.sample = (uint32_t)ks[i];
    V3 d, le;
    double pdf;
    env_sample(E, key, (uint32_t)depth, (uint32_t)nl, d, pdf, le);
    double* o = out7 + i * 7;
    o[0] = d.x; o[1] = d.y; o[2] = d.z; o[3] = pdf; o[4] = le.x; o[5] = le.y; o[6] = le.z;
}

void launch_env_eval(const DEnv& E, const double* d_dirs, long long n, double* d_rgb, hipStream_t st)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_env_eval, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, E, d_dirs, n, d_rgb);
}

void launch_env_sample(const DEnv& E, unsigned long long seed, const int32_t* d_pix, const int32_t* d_k, int depth, int nl, long long n, double* d_out7,
                       hipStream_t st)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_env_sample, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, E, seed, d_pix, d_k, depth, nl, n, d_out7);
}

}  // namespace mcpt
