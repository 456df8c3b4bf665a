// Radiance queries (mcpt_query_radiance): the source pass that puts a caller's rays where the camera pass puts the lens's, the megakernel
// form, the fold into per-query mean, standard error and hit count, and the mcpt_query_rays seam; for a list of light probes
// (mcpt_query_sh) the same pass and megakernel form over the sphere draw, and the fold into spherical-harmonic coefficients.
// -ffp-contract=off (Makefile).
#include <hip/hip_runtime.h>

#include "dev_common.hpp"
#include "kernels.hpp"
#include "path_variant.hpp"
#include "query.hpp"
#include "shade_common.hpp"
#include "sh_math.hpp"
#include "shade_path.hpp"
#include "vertex.hpp"
#include "wavefront.hpp"

namespace mcpt {

__global__ void __launch_bounds__(256) k_query_rays(DQuery q, unsigned long long seed, const int32_t* __restrict__ ids, const int32_t* __restrict__ ks,
                                                    long long n, double* __restrict__ rays6)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n) return;
    V3 o, d;
    query_ray(q.kind, q.q6 + gid * query_stride(q.kind), seed, ids ? ids[gid] : (int)gid, ks[gid], o, d);
    double* r = rays6 + gid * 6;
    r[0] = o.x; r[1] = o.y; r[2] = o.z; r[3] = d.x; r[4] = d.y; r[5] = d.z;
}

// k_shade_samples_lens (camera.hip) with the query's ray for the camera's: one lane per (slot, j) traces it (reference-shaped walk) and
// shades the path from its hit.  Lane (slot, j) -> rad[(s*spp + j)*3], flags[s*spp + j], s = the slot within the chunk.
template <bool ENV, int PICK>
__global__ void __launch_bounds__(256) k_query_samples(DScene S, DQuery q, unsigned long long seed, const int32_t* __restrict__ ids, int first_slot,
                                                       long long n_samples, int spp, int sample_base, double* __restrict__ rad,
                                                       uint8_t* __restrict__ flags, DCounters* ctr)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    LaneStats ls;
    if (gid < n_samples) {
        const int slot = first_slot + (int)(gid / spp);
        const int k = sample_base + (int)(gid % spp);
        const int id = ids ? ids[slot] : slot;
        Ray r;
        query_ray(q.kind, q.q6 + (size_t)slot * query_stride(q.kind), seed, id, k, r.o, r.d);
        Hit h; Work w = {0, 0};
        const bool ok = trace_closest(S, r, h, w);
        ls.nodes = w.nodes; ls.tris = w.tris; ls.primary = 1; ls.samples = 1;
        double out[3] = {0, 0, 0};
        if (ok) {
            RngKey key; key.k0 = (uint32_t)seed; key.k1 = (uint32_t)(seed >> 32); key.pixel = (uint32_t)id; key.sample = (uint32_t)k;
            shade_path<ENV, PICK>(S, key, r.d, h, out, ls);
        } else if (ENV) env_camera_miss(S, r.d, out);
        rad[gid * 3] = out[0]; rad[gid * 3 + 1] = out[1]; rad[gid * 3 + 2] = out[2];
        flags[gid] = ok ? 1 : 0;
    }
    flush_stats(ctr, ls);
}

// k_camera_pass (camera.hip) for a query list: path position j = chunk-local sample id (slot - first_slot) * spp + k, no compaction.  The
// bounce ray of vertex -1 is the query's ray, left from its origin itself (MCPT_BT_NO_OFFSET; type TRANSMISSION, so that an emitter it
// reaches is not taken for a diffuse bounce's), and it has no shadow rays.  The queue words are cleared for the trace launch that follows.
// KIND: the list's kind as a constant, so that a ray list's pass carries none of the hemisphere draw: the kernel streams 60 bytes per
// sample, and with both kinds behind a run-time branch it held 59 VGPRs and 40 bytes of scratch and took 3.5 ms for the 236 M samples of
// a 1280 x 720, 256-sample chunk, against 2.3 ms with 30 VGPRs and none (the camera pass: 2.6 ms).
template <int KIND>
__global__ void __launch_bounds__(256) k_query_pass(DQuery q, WfArgs a, long long n)
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
    const int id = a.pixels ? a.pixels[slot] : slot;
    V3 o, d;
    query_ray(KIND, q.q6 + (size_t)slot * query_stride(KIND), a.seed, id, k, o, d);
    a.out.id[j] = (int32_t)j;
    stc(a.out.p, cap, j, o);
    stc(a.out.bdir, cap, j, d);
    a.out.btype[j] = RT_TRANSMISSION | MCPT_BT_NO_OFFSET;
    for (int l = 0; l < a.nl; l++) a.out.expect[(long long)l * cap + j] = -2;
}

// One lane per (slot, channel), k_fold_lens's layout and loops (camera.hip): the slot's hit flags first, then its n samples in k order, no
// atomics -- s1 += x, s2 += x * x -- and the mean and the standard error as k_progressive_image (kernels.hip) forms them from the same
// moments.  A ray that missed has radiance +0.0 in rad (ENV: Le of its direction), so it is summed like any other; a slot none of whose
// rays hit is not read at all without an environment: its sums are +0.0.  hits[slot]: the samples whose ray hit (one lane per slot
// writes it: c == 0).
template <bool ENV>
__global__ void __launch_bounds__(256) k_query_fold(DQuery q, const double* __restrict__ rad, const uint8_t* __restrict__ flags, int first_slot,
                                                    int n_slots, int n)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)n_slots * 3) return;
    const int s = (int)(gid / 3), c = (int)(gid % 3);
    const double* src = rad + (size_t)s * n * 3 + c;
    const uint8_t* f = flags + (size_t)s * n;
    int h = 0;
    for (int k = 0; k < n; k++) h += f[k];
    double s1 = 0.0, s2 = 0.0;
    if (h > 0 || ENV)
        for (int k = 0; k < n; k++) {
            const double x = src[(size_t)k * 3];
            s1 += x;
            s2 += x * x;
        }
    const size_t i = (size_t)(first_slot + s) * 3 + c;
    q.mean3[i] = s1 / n;
    if (q.stderr3) q.stderr3[i] = n >= 2 ? sqrt(progressive_se2(s1, s2, n)) : 0.0;
    if (c == 0 && q.hits) q.hits[first_slot + s] = h;
}

// The fold of a probe list (mcpt_query_sh): k_query_fold's lanes and walk -- one lane per (slot, channel), the slot's hit flags, then its
// n samples in k order, no atomics -- with every sample weighted by the nine basis functions of its own direction: v = x * Y_i(d_k),
// s1[i] += v, s2[i] += v * v.  The path state's direction is gone by now, so d_k is drawn again from the key (query_ray: bitwise the
// direction the sample's ray was given).  The three lanes of a slot repeat that draw; a lane per slot would not, but holds 54
// accumulators and reads 24-byte pieces a sample stride apart, and a lane per (slot, coefficient) repeats it nine times.  q.mean3 and
// q.stderr3 are [n][9][3] here.  A slot none of whose rays hit is not read without an environment: x = +0.0 throughout, so is every sum.
template <bool ENV>
__global__ void __launch_bounds__(256) k_query_fold_sh(DQuery q, unsigned long long seed, const int32_t* __restrict__ ids, const double* __restrict__ rad,
                                                       const uint8_t* __restrict__ flags, int first_slot, int n_slots, int n, int sample_base)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)n_slots * 3) return;
    const int s = (int)(gid / 3), c = (int)(gid % 3);
    const double* src = rad + (size_t)s * n * 3 + c;
    const uint8_t* f = flags + (size_t)s * n;
    int h = 0;
    for (int k = 0; k < n; k++) h += f[k];
    double s1[MCPT_SH_N], s2[MCPT_SH_N];
#pragma unroll
    for (int i = 0; i < MCPT_SH_N; i++) { s1[i] = 0.0; s2[i] = 0.0; }
    const int slot = first_slot + s;
    if (h > 0 || ENV) {
        const int id = ids ? ids[slot] : slot;
        const double* p = q.q6 + (size_t)slot * 3;
        for (int k = 0; k < n; k++) {
            const double x = src[(size_t)k * 3];
            V3 o, d;
            query_ray(MCPT_QUERY_KIND_SPHERE, p, seed, id, sample_base + k, o, d);
            double Y[MCPT_SH_N];
            sh_basis9(d.x, d.y, d.z, Y);
#pragma unroll
            for (int i = 0; i < MCPT_SH_N; i++) {
                const double v = x * Y[i];
                s1[i] += v;
                s2[i] += v * v;
            }
        }
    }
    const size_t o27 = (size_t)slot * (MCPT_SH_N * 3) + c;
#pragma unroll
    for (int i = 0; i < MCPT_SH_N; i++) {
        q.mean3[o27 + i * 3] = 12.566370614359172 * (s1[i] / n);
        if (q.stderr3) q.stderr3[o27 + i * 3] = n >= 2 ? 12.566370614359172 * sqrt(progressive_se2(s1[i], s2[i], n)) : 0.0;
    }
    if (c == 0 && q.hits) q.hits[slot] = h;
}

// ------------------------------------------------------------------------------------------------ launchers
static inline unsigned blocks_of(long long n, int block) { return (unsigned)((n + block - 1) / block); }

void launch_query_rays(const DQuery& q, unsigned long long seed, const int32_t* d_ids, const int32_t* d_k, long long n, double* d_rays6, hipStream_t st)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_query_rays, dim3(blocks_of(n, 256)), dim3(256), 0, st, q, seed, d_ids, d_k, n, d_rays6);
}
void launch_query_samples(const DScene& S, const DQuery& q, unsigned long long seed, const int32_t* d_ids, int first_slot, int n_slots, int spp,
                          int sample_base, double* d_rad, uint8_t* d_flags, DCounters* ctr, hipStream_t st)
{
    const long long n = (long long)n_slots * spp;
    if (n <= 0) return;
    const dim3 grid(blocks_of(n, 256));
    with_path_variant(S, [&](auto env, auto pick) {
        hipLaunchKernelGGL((k_query_samples<env(), pick()>), grid, dim3(256), 0, st, S, q, seed, d_ids, first_slot, n, spp, sample_base, d_rad, d_flags, ctr);
    });
}
void launch_query_pass(const DQuery& q, const WfArgs& a, long long n_samples, hipStream_t st)
{
    const dim3 grid(blocks_of(n_samples > 0 ? n_samples : 1, 256));
    if (q.kind == MCPT_QUERY_KIND_RAY) hipLaunchKernelGGL(k_query_pass<MCPT_QUERY_KIND_RAY>, grid, dim3(256), 0, st, q, a, n_samples);
    else if (q.kind == MCPT_QUERY_KIND_SPHERE) hipLaunchKernelGGL(k_query_pass<MCPT_QUERY_KIND_SPHERE>, grid, dim3(256), 0, st, q, a, n_samples);
    else hipLaunchKernelGGL(k_query_pass<MCPT_QUERY_KIND_HEMISPHERE>, grid, dim3(256), 0, st, q, a, n_samples);
}
void launch_query_fold(const DQuery& q, const double* d_rad, const uint8_t* d_flags, int first_slot, int n_slots, int n, bool env, hipStream_t st)
{
    if (n_slots <= 0) return;
    const dim3 grid(blocks_of((long long)n_slots * 3, 256));
    if (env) hipLaunchKernelGGL(k_query_fold<true>, grid, dim3(256), 0, st, q, d_rad, d_flags, first_slot, n_slots, n);
    else hipLaunchKernelGGL(k_query_fold<false>, grid, dim3(256), 0, st, q, d_rad, d_flags, first_slot, n_slots, n);
}
void launch_query_fold_sh(const DQuery& q, unsigned long long seed, const int32_t* d_ids, const double* d_rad, const uint8_t* d_flags, int first_slot,
                          int n_slots, int n, int sample_base, bool env, hipStream_t st)
{
    if (n_slots <= 0) return;
    const dim3 grid(blocks_of((long long)n_slots * 3, 256));
    if (env) hipLaunchKernelGGL(k_query_fold_sh<true>, grid, dim3(256), 0, st, q, seed, d_ids, d_rad, d_flags, first_slot, n_slots, n, sample_base);
    else hipLaunchKernelGGL(k_query_fold_sh<false>, grid, dim3(256), 0, st, q, seed, d_ids, d_rad, d_flags, first_slot, n_slots, n, sample_base);
}

}  // namespace mcpt
