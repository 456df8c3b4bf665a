// Baked specular's kernels (mcpt.h: baked specular): the reflection volume's lookup by position, direction and exponent, the specular
// pass that follows a baked shading launch -- it forms the sample's normal again (baked_surface.hpp: what the diffuse lookup took), the
// mirror direction and the lookup, and adds ks * R to the sample's radiance -- and the count of a pixel's specular samples.  The
// arithmetic is reflection_volume.hpp's and baked_specular.hpp's, the copies the host form compiles.  fp64 throughout, no contraction
// (-ffp-contract=off).  Every output is one lane's, every sum in a fixed order; no atomics, no LDS: a result depends neither on the grid of
// the launch nor on the chunking nor on the device.
#include <hip/hip_runtime.h>

#include "baked_specular.hpp"
#include "baked_surface.hpp"
#include "dev_common.hpp"

namespace mcpt {

static constexpr int kSpecBlock = 256;

// ---- lookup: one lane per receiver
template <bool VISIBLE>
__global__ void __launch_bounds__(kSpecBlock) k_reflection_volume_lookup(ReflVolume V, const double* __restrict__ q6, const double* __restrict__ d3,
                                                                         const double* __restrict__ x, long long m, double* __restrict__ out3,
                                                                         int32_t* __restrict__ corners)
{
    const long long i = (long long)blockIdx.x * kSpecBlock + threadIdx.x;
    if (i >= m) return;
    double q[6], d[3], v[3];
    for (int c = 0; c < 6; c++) q[c] = q6[i * 6 + c];
    for (int c = 0; c < 3; c++) d[c] = d3[i * 3 + c];
    const int n = reflection_volume_lookup<VISIBLE>(V, q, d, x[i], v);
    for (int c = 0; c < 3; c++) out3[i * 3 + c] = v[c];
    if (corners) corners[i] = n;
}

// ---- specular: one lane per ray, after k_baked_shade of the same rays; neighbouring lanes are neighbouring rays, whose hits mostly share
// triangles and probes and whose mirror directions mostly share texels
template <bool VISIBLE>
__global__ void __launch_bounds__(kSpecBlock) k_baked_specular(DScene S, ReflVolume V, int flags, const double* __restrict__ rays6,
                                                               const int32_t* __restrict__ leaf, const double* __restrict__ t,
                                                               const double* __restrict__ p, long long n, double* radiance3, BakedSpecOut o)
{
    const long long i = (long long)blockIdx.x * kSpecBlock + threadIdx.x;
    if (i >= n) return;
    double R[3] = {0.0, 0.0, 0.0}, ks[3] = {0.0, 0.0, 0.0}, r[3] = {0.0, 0.0, 0.0}, Ns = 0.0;
    int slit = 0;
    bool spec = false;
    const int lf = leaf[i];
    if (lf >= 0) {
        const DTri* tr = S.tris + lf;
        const DMaterial* m = S.materials + tr->material;
        if (m->light < 0 && (m->ks[0] != 0.0 || m->ks[1] != 0.0 || m->ks[2] != 0.0)) {
            const V3 d = ld3(rays6 + i * 6 + 3), hp = ld3(p + i * 3);
            double q[6] = {hp.x, hp.y, hp.z, 0.0, 0.0, 0.0};
            baked_normal(S, tr, lf, t[i], hp, d, flags, q + 3);
            const double dd[3] = {d.x, d.y, d.z};
            double rr[3];
            if (baked_mirror(dd, q + 3, rr)) {
                spec = true;
                Ns = m->Ns;
                for (int c = 0; c < 3; c++) { ks[c] = m->ks[c]; r[c] = rr[c]; }
                slit = reflection_volume_lookup<VISIBLE>(V, q, rr, baked_exponent(Ns), R);
            }
        }
    }
    if (spec && radiance3) {
        const bool lighting_only = (flags & MCPT_BAKED_LIGHTING_ONLY) != 0;
        for (int c = 0; c < 3; c++) radiance3[i * 3 + c] = radiance3[i * 3 + c] + (lighting_only ? R[c] : ks[c] * R[c]);
    }
    if (o.spec3) for (int c = 0; c < 3; c++) o.spec3[i * 3 + c] = R[c];
    if (o.ks3) for (int c = 0; c < 3; c++) o.ks3[i * 3 + c] = ks[c];
    if (o.r3) for (int c = 0; c < 3; c++) o.r3[i * 3 + c] = r[c];
    if (o.ns) o.ns[i] = Ns;
    if (o.slit) o.slit[i] = slit;
}

// ---- count: one lane per pixel of the chunk, its G samples in k order
__global__ void __launch_bounds__(kSpecBlock) k_baked_specular_count(int first, int n, int G, const int32_t* __restrict__ slit, int32_t* __restrict__ count)
{
    const int i = blockIdx.x * kSpecBlock + threadIdx.x;
    if (i >= n) return;
    int s = 0;
    for (int k = 0; k < G; k++) s += slit[(long long)k * n + i] > 0 ? 1 : 0;
    count[(size_t)(first + i)] = s;
}

static inline unsigned spec_blocks(long long n) { return (unsigned)((n + kSpecBlock - 1) / kSpecBlock); }

void launch_reflection_volume_lookup(const ReflVolume& V, const double* d_q6, const double* d_d3, const double* d_x, int64_t m, double* d_out3,
                                     int32_t* d_corners, hipStream_t st)
{
    const dim3 grid(spec_blocks((long long)m)), block(kSpecBlock);
    if (V.visible) hipLaunchKernelGGL(k_reflection_volume_lookup<true>, grid, block, 0, st, V, d_q6, d_d3, d_x, (long long)m, d_out3, d_corners);
    else hipLaunchKernelGGL(k_reflection_volume_lookup<false>, grid, block, 0, st, V, d_q6, d_d3, d_x, (long long)m, d_out3, d_corners);
}

void launch_baked_specular(const DScene& S, const ReflVolume& V, int flags, const double* d_rays6, const int32_t* d_leaf, const double* d_t,
                           const double* d_p, long long n, double* d_radiance3, const BakedSpecOut& o, hipStream_t st)
{
    const dim3 grid(spec_blocks(n)), block(kSpecBlock);
    if (V.visible) hipLaunchKernelGGL(k_baked_specular<true>, grid, block, 0, st, S, V, flags, d_rays6, d_leaf, d_t, d_p, n, d_radiance3, o);
    else hipLaunchKernelGGL(k_baked_specular<false>, grid, block, 0, st, S, V, flags, d_rays6, d_leaf, d_t, d_p, n, d_radiance3, o);
}

void launch_baked_specular_count(const BakedChunk& c, const int32_t* d_slit, int32_t* d_count, hipStream_t st)
{
    hipLaunchKernelGGL(k_baked_specular_count, dim3(spec_blocks(c.n)), dim3(kSpecBlock), 0, st, c.first, c.n, c.G, d_slit, d_count);
}

}  // namespace mcpt
