// Reflection probes' kernels (mcpt.h: reflection probes): the rays of a chunk of texels -- a jittered point of the texel's square, decoded --
// written with their ids into a workspace the unchanged query call then answers (query_api.cpp: query_device), the fold of those answers
// per texel, the prefilter that convolves a probe's map with Phong lobes, and the lookup in the chain of filtered maps.  The arithmetic is
// reflection.hpp's, the copy the host forms compile.  fp64 throughout, no contraction (-ffp-contract=off).  Every output is one lane's,
// every sum in a fixed order; no atomics: a result depends neither on the grid of the launch nor on the chunking nor on the device.
#include <hip/hip_runtime.h>

#include "camera.hpp"
#include "dev_common.hpp"
#include "reflection.hpp"

namespace mcpt {

static constexpr int kReflBlock = 256;
// The prefilter stages the source in tiles of as many records as a workgroup has lanes: every lane writes one record of seven doubles
// (direction, solid angle, radiance) in a slot of eight, so that a record is read in 16-byte pieces: 16 384 bytes of LDS a workgroup.
// tests/test_gpu_reflection.py names the tile.  A lane takes kReflGroup records at a time (reflection_accumulate).
static constexpr int kReflTile = kReflBlock;
static constexpr int kReflRecord = 8;
static constexpr int kReflGroup = 4;

// the ray and the id of entry e of the call (mcpt.h: reflection probes, "ray of an entry")
__device__ __forceinline__ void reflection_ray(const ReflChunk& c, long long e, double* ray6, int32_t& id)
{
    const long long texels = (long long)c.R * c.R, per_probe = texels * c.S;
    const long long i = e / per_probe, rest = e % per_probe;
    const int b = (int)(rest / c.S);
    const long long base = c.id_base ? (long long)c.id_base[i] : i * per_probe;
    id = (int32_t)(base + rest);                            // rest = b * S + j
    RngKey key; key.k0 = (uint32_t)c.seed; key.k1 = (uint32_t)(c.seed >> 32); key.pixel = (uint32_t)id; key.sample = (uint32_t)c.sample_base;
    double u0, u1, u2, u3;
    uniform4(key, MCPT_LENS_RNG_DEPTH, 0u, u0, u1, u2, u3);
    const int x = b % c.R, y = b / c.R;
    reflection_decode((double(x) + u0) / double(c.R), (double(y) + u1) / double(c.R), ray6 + 3);
    const double* p = c.p3 + i * 3;
    ray6[0] = p[0]; ray6[1] = p[1]; ray6[2] = p[2];
}

// ---- rays: one lane per ray, six fp64 stores and the id
__global__ void __launch_bounds__(kReflBlock) k_reflection_rays(ReflChunk c, const long long* __restrict__ entries, long long m)
{
    const long long g = (long long)blockIdx.x * kReflBlock + threadIdx.x;
    if (g >= m) return;
    double r[6];
    int32_t id;
    reflection_ray(c, entries ? entries[g] : c.first_texel * c.S + g, r, id);
    for (int k = 0; k < 6; k++) c.rays6[g * 6 + k] = r[k];
    c.ids[g] = id;
}

// ---- fold: one lane per texel of the chunk, its S samples in j order with the query's own expressions (query.hip: k_query_fold)
__global__ void __launch_bounds__(kReflBlock) k_reflection_fold(ReflChunk c, double* __restrict__ radiance, double* __restrict__ err, int32_t* __restrict__ hits)
{
    const long long t = (long long)blockIdx.x * kReflBlock + threadIdx.x;
    if (t >= c.texels) return;
    const int S = c.S;
    double s1[3] = {0.0, 0.0, 0.0}, s2[3] = {0.0, 0.0, 0.0};
    int nhit = 0;
    for (int j = 0; j < S; j++) {
        const long long g = t * S + j;
        for (int ch = 0; ch < 3; ch++) {
            const double x = c.mean3[g * 3 + ch];
            s1[ch] += x;
            s2[ch] += x * x;
        }
        nhit += c.hits[g];
    }
    const long long T = c.first_texel + t;
    for (int ch = 0; ch < 3; ch++) {
        radiance[T * 3 + ch] = s1[ch] / S;
        if (err) err[T * 3 + ch] = S >= 2 ? sqrt(progressive_se2(s1[ch], s2[ch], S)) : 0.0;
    }
    if (hits) hits[T] = nhit;
}

// The levels of a chain as the prefilter's grid sees them: workgroups first_block[l] .. first_block[l + 1] - 1 of a probe work on level l.
struct ReflLevels {
    int R, num_levels, source_texels, chain_texels;
    int res[kReflectionMaxLevels], ns[kReflectionMaxLevels], first_texel[kReflectionMaxLevels], first_block[kReflectionMaxLevels + 1];
};

// N consecutive records of the tile into one lane's sums.  All N records are read first, in whole: left to itself the compiler sinks
// the reads of the solid angle and the radiance into the branch on the cosine, one LDS round trip each with a wait of its own, four in
// a row per record, and that wait is where the time went; the empty asm statement pins a value read to this point at the
// cost of no instruction.  The N lobes are raised together: the squaring loop is a chain of dependent multiplications under scalar
// branches (ns is the workgroup's), and N independent chains share every branch and fill one another's latency.  The terms are added
// one record after the other, in ascending order, and a record whose cosine is not positive leaves the sums as they were -- mcpt.h's
// arithmetic, bit for bit.
template <int N>
__device__ __forceinline__ void reflection_accumulate(const double* __restrict__ rec, const double* r, int ns, double& W, double* A)
{
    double e[N * kReflRecord];
#pragma unroll
    for (int f = 0; f < N * kReflRecord; f++) e[f] = rec[f];                 // (a record's eighth slot comes along: 16-byte reads)
#pragma unroll
    for (int f = 0; f < N * kReflRecord; f++) asm volatile("" : "+v"(e[f]));
    double c[N], p[N], b[N];
#pragma unroll
    for (int j = 0; j < N; j++) {
        c[j] = (r[0] * e[j * kReflRecord] + r[1] * e[j * kReflRecord + 1]) + r[2] * e[j * kReflRecord + 2];
        p[j] = 1.0;
        b[j] = c[j];
    }
    for (int n = ns; n > 0;) {                              // reflection_ipow, N at a time
        const bool odd = (n & 1) != 0;
        n >>= 1;
        if (odd) {
#pragma unroll
            for (int j = 0; j < N; j++) p[j] = p[j] * b[j];
        }
        if (n) {
#pragma unroll
            for (int j = 0; j < N; j++) b[j] = b[j] * b[j];
        }
    }
#pragma unroll
    for (int j = 0; j < N; j++) {
        const bool on = c[j] > 0.0;
        const double g = e[j * kReflRecord + 3] * p[j];
        W = on ? W + g : W;
        A[0] = on ? A[0] + g * e[j * kReflRecord + 4] : A[0];
        A[1] = on ? A[1] + g * e[j * kReflRecord + 5] : A[1];
        A[2] = on ? A[2] + g * e[j * kReflRecord + 6] : A[2];
    }
}

// ---- prefilter: one lane per output texel, a workgroup within one (probe, level); blockIdx.y is the probe.  The source goes through LDS
// tile by tile: lane k of the workgroup forms the record of source texel tile + k -- its direction and solid angle from the texel's
// index, its radiance from the map -- and then every lane of a wave reads the same record at the same time, a broadcast.  ns is the
// workgroup's, so the squaring loop is uniform; a lane's sums run over the source in ascending order, tile after tile.  The record holds
// L, not the product of solid angle and L: mcpt.h multiplies the lobe into the solid angle first, and the bits follow that order.
__global__ void __launch_bounds__(kReflBlock) k_reflection_prefilter(ReflLevels lv, const double* __restrict__ radiance, double* __restrict__ chain)
{
    __shared__ __attribute__((aligned(16))) double rec[kReflTile * kReflRecord];
    int l = 0;
    while (l + 1 < lv.num_levels && (int)blockIdx.x >= lv.first_block[l + 1]) l++;
    const int Ro = lv.res[l], ns = lv.ns[l], outs = Ro * Ro;
    const int o = ((int)blockIdx.x - lv.first_block[l]) * kReflBlock + (int)threadIdx.x;
    const bool live = o < outs;
    double r[3] = {0.0, 0.0, 0.0}, w;
    if (live) reflection_texel(Ro, o, r, w);
    const double* L = radiance + (size_t)blockIdx.y * (size_t)lv.source_texels * 3;
    double W = 0.0, A[3] = {0.0, 0.0, 0.0};
    for (int tile = 0; tile < lv.source_texels; tile += kReflTile) {
        const int b = tile + (int)threadIdx.x;
        __syncthreads();                                    // the tile before this one has been read
        if (b < lv.source_texels) {
            double* e = rec + threadIdx.x * kReflRecord;
            reflection_texel(lv.R, b, e, e[3]);
            e[4] = L[(size_t)b * 3]; e[5] = L[(size_t)b * 3 + 1]; e[6] = L[(size_t)b * 3 + 2]; e[7] = 0.0;
        }
        __syncthreads();
        const int count = lv.source_texels - tile < kReflTile ? lv.source_texels - tile : kReflTile;
        if (live) {
            int k = 0;
            for (; k + kReflGroup <= count; k += kReflGroup) reflection_accumulate<kReflGroup>(rec + k * kReflRecord, r, ns, W, A);
            for (; k < count; k++) reflection_accumulate<1>(rec + k * kReflRecord, r, ns, W, A);
        }
    }
    if (live) {
        double* out = chain + ((size_t)blockIdx.y * (size_t)lv.chain_texels + (size_t)lv.first_texel[l] + (size_t)o) * 3;
        for (int ch = 0; ch < 3; ch++) out[ch] = W > 0.0 ? A[ch] / W : 0.0;
    }
}

// ---- lookup: one lane per receiver
__global__ void __launch_bounds__(kReflBlock) k_reflection_lookup(mcpt_reflection_chain c, int chain_texels, const double* __restrict__ chain, long long n,
                                                                  const int32_t* __restrict__ probe, const double* __restrict__ d3,
                                                                  const double* __restrict__ x, long long m, double* __restrict__ out3)
{
    const long long q = (long long)blockIdx.x * kReflBlock + threadIdx.x;
    if (q >= m) return;
    const long long P = probe[q];
    double v[3] = {0.0, 0.0, 0.0};
    if (P >= 0 && P < n) {
        const double d[3] = {d3[q * 3], d3[q * 3 + 1], d3[q * 3 + 2]};
        reflection_lookup(c, chain + (size_t)P * (size_t)chain_texels * 3, d, x[q], v);
    }
    for (int ch = 0; ch < 3; ch++) out3[q * 3 + ch] = v[ch];
}

static inline unsigned refl_blocks(long long n) { return (unsigned)((n + kReflBlock - 1) / kReflBlock); }

void launch_reflection_rays(const ReflChunk& c, const long long* d_entries, long long m, hipStream_t st)
{
    hipLaunchKernelGGL(k_reflection_rays, dim3(refl_blocks(m)), dim3(kReflBlock), 0, st, c, d_entries, m);
}

void launch_reflection_fold(const ReflChunk& c, double* d_radiance, double* d_stderr, int32_t* d_hits, hipStream_t st)
{
    hipLaunchKernelGGL(k_reflection_fold, dim3(refl_blocks(c.texels)), dim3(kReflBlock), 0, st, c, d_radiance, d_stderr, d_hits);
}

void launch_reflection_prefilter(const mcpt_reflection_chain& c, const double* d_radiance, int64_t n, double* d_chain, hipStream_t st)
{
    ReflLevels lv{};
    lv.R = c.res; lv.num_levels = c.num_levels; lv.source_texels = c.res * c.res;
    int texel = 0, block = 0;
    for (int l = 0; l < c.num_levels; l++) {
        lv.res[l] = c.level_res[l]; lv.ns[l] = c.level_ns[l];
        lv.first_texel[l] = texel; lv.first_block[l] = block;
        texel += c.level_res[l] * c.level_res[l];
        block += (int)refl_blocks((long long)c.level_res[l] * c.level_res[l]);
    }
    lv.first_block[c.num_levels] = block;
    lv.chain_texels = texel;
    // (blockIdx.y holds at most 65 535 probes a launch)
    for (int64_t first = 0; first < n; first += 65535) {
        const int64_t count = n - first < 65535 ? n - first : 65535;
        hipLaunchKernelGGL(k_reflection_prefilter, dim3((unsigned)block, (unsigned)count), dim3(kReflBlock), 0, st, lv,
                           d_radiance + (size_t)first * (size_t)lv.source_texels * 3, d_chain + (size_t)first * (size_t)texel * 3);
    }
}

void launch_reflection_lookup(const mcpt_reflection_chain& c, const double* d_chain, int64_t n, const int32_t* d_probe, const double* d_d3, const double* d_x,
                              int64_t m, double* d_out3, hipStream_t st)
{
    hipLaunchKernelGGL(k_reflection_lookup, dim3(refl_blocks((long long)m)), dim3(kReflBlock), 0, st, c, reflection_chain_texels(c), d_chain, (long long)n,
                       d_probe, d_d3, d_x, (long long)m, d_out3);
}

}  // namespace mcpt
