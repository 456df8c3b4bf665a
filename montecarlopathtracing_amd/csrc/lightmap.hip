// The lightmap baker's own kernels (mcpt.h: lightmaps): the chart rasteriser, the compaction of the covered texels with their positions
// and normals, the scatter of a hemisphere query's answers into the map and the dilation of the gutters.  The path tracing in between is
// mcpt_query_radiance's, unchanged.  The arithmetic is lightmap.hpp's, shared with mcpt_lightmap_raster_host; tests/lightmap_ref.py
// restates it in numpy.  Ownership is an integer minimum and the list an order-preserving compaction: each has one correct output, so
// nothing here depends on the grid or on the order in which waves run.
#include <hip/hip_runtime.h>

#include "lightmap.hpp"

namespace mcpt {

static constexpr int kLmBlock = 256;
static constexpr unsigned kLmMaxBlocks = 2048;             // grids that stride: 8 blocks per CU
static constexpr int kLmBigBox = 4096;                     // a texel box above this many texels is left to the whole grid (k_lm_raster_big)

static inline unsigned blocks_of(long long n) { return (unsigned)((n + kLmBlock - 1) / kLmBlock); }
int lightmap_blocks(long long n) { return (int)blocks_of(n); }

// the chart of triangle slot k: the caller's, by .obj face, or the face's own vt
__device__ __forceinline__ void lm_chart(const DTri* __restrict__ tris, const DTriShade* __restrict__ shade, const double* __restrict__ uv6, int k,
                                         double* uv)
{
    if (uv6) {
        const double* c = uv6 + (size_t)tris[k].face * 6;
        for (int i = 0; i < 6; i++) uv[i] = c[i];
    } else {
        const DTriShade& s = shade[k];
        uv[0] = s.vt1[0]; uv[1] = s.vt1[1]; uv[2] = s.vt2[0]; uv[3] = s.vt2[1]; uv[4] = s.vt3[0]; uv[5] = s.vt3[1];
    }
}

// texel i of the box (x0, y0, width bw) against the chart: the face claims it when it covers the centre
__device__ __forceinline__ void lm_claim(const double* uv, double area2, int face, int x0, int y0, unsigned bw, unsigned i, int W, int H,
                                         int32_t* __restrict__ owner)
{
    const int x = x0 + (int)(i % bw), y = y0 + (int)(i / bw);
    double e[3];
    lightmap_edges(uv, lightmap_centre(x, W), lightmap_centre(y, H), e);
    if (!lightmap_covers(area2, e)) return;
    int32_t* o = owner + ((size_t)y * W + x);
    if (*o > face) atomicMin(o, face);                      // (a stale read only costs an atomic that changes nothing)
}

// ---- step 1, one wave per triangle slot: the slot's texel box is spread over the 64 lanes.  A teapot's triangles cover less than a texel
// and a floor quad the whole map: a box above kLmBigBox texels goes to a list the next kernel spreads over the whole grid.  The wave also
// notes where its face sits (slot_of_face), which step 2 needs to find a texel's owner among the triangles in leaf order.
__global__ void __launch_bounds__(kLmBlock) k_lm_raster(const DTri* __restrict__ tris, const DTriShade* __restrict__ shade, int t,
                                                        const double* __restrict__ uv6, int W, int H, int32_t* __restrict__ owner,
                                                        int32_t* __restrict__ slot_of_face, int32_t* __restrict__ big, unsigned int* __restrict__ n_big)
{
    const int lane = threadIdx.x & 63;
    const int waves = (int)gridDim.x * (kLmBlock / 64);
    for (int k = (int)blockIdx.x * (kLmBlock / 64) + (threadIdx.x >> 6); k < t; k += waves) {
        const int face = tris[k].face;
        if (lane == 0) slot_of_face[face] = k;
        double uv[6];
        lm_chart(tris, shade, uv6, k, uv);
        const double area2 = lightmap_area2(uv);
        if (!lightmap_area_ok(area2) || !lightmap_normal_ok(tris[k].n)) continue;
        int x0, x1, y0, y1;
        if (!lightmap_box(uv, W, H, x0, x1, y0, y1)) continue;
        const unsigned bw = (unsigned)(x1 - x0 + 1), cnt = bw * (unsigned)(y1 - y0 + 1);       // at most 2^28
        if (cnt > (unsigned)kLmBigBox) {
            if (lane == 0) big[atomicAdd(n_big, 1u)] = k;
            continue;
        }
        for (unsigned i = lane; i < cnt; i += 64) lm_claim(uv, area2, face, x0, y0, bw, i, W, H, owner);
    }
}

// ... and the large boxes, one after the other, each over every lane of the grid
__global__ void __launch_bounds__(kLmBlock) k_lm_raster_big(const DTri* __restrict__ tris, const DTriShade* __restrict__ shade,
                                                            const double* __restrict__ uv6, int W, int H, int32_t* __restrict__ owner,
                                                            const int32_t* __restrict__ big, const unsigned int* __restrict__ n_big)
{
    const unsigned stride = gridDim.x * kLmBlock, first = blockIdx.x * kLmBlock + threadIdx.x;
    const unsigned n = *n_big;
    for (unsigned j = 0; j < n; j++) {
        const int k = big[j];
        double uv[6];
        lm_chart(tris, shade, uv6, k, uv);
        const double area2 = lightmap_area2(uv);
        int x0, x1, y0, y1;
        lightmap_box(uv, W, H, x0, x1, y0, y1);
        const unsigned bw = (unsigned)(x1 - x0 + 1), cnt = bw * (unsigned)(y1 - y0 + 1);
        const int face = tris[k].face;
        for (unsigned i = first; i < cnt; i += stride) lm_claim(uv, area2, face, x0, y0, bw, i, W, H, owner);
    }
}

// ---- step 2, the compaction of the covered texels in ascending order: the three kernels of the adaptive frames' pixel list
// (kernels.hip: k_adaptive_select).  select: one lane per texel; a texel nobody claimed gets its -1; each wave stores the __ballot of
// `covered` and the block its count.  scan: one workgroup turns the block counts into exclusive offsets and the total.  texels: a covered
// lane's list position is its block's offset, the popcounts of the waves before it in the block and the set bits of its wave's mask
// below it; there it writes the texel and its query.
__global__ void __launch_bounds__(kLmBlock) k_lm_select(int32_t* __restrict__ owner, int n, unsigned long long* __restrict__ masks,
                                                        int32_t* __restrict__ block_counts)
{
    __shared__ int wave_count[4];
    const int i = blockIdx.x * kLmBlock + threadIdx.x;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    bool covered = false;
    if (i < n) {
        covered = owner[i] != kLightmapUnowned;
        if (!covered) owner[i] = -1;
    }
    const unsigned long long mask = __ballot(covered);
    if (lane == 0) {
        masks[(size_t)blockIdx.x * 4 + w] = mask;
        wave_count[w] = __popcll(mask);
    }
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = ((wave_count[0] + wave_count[1]) + wave_count[2]) + wave_count[3];
}

// Exclusive scan of n block counts into offsets, in chunks of 256 with a running carry; *total = the sum.  One workgroup of 256.
// (k_adaptive_scan's algorithm, kept here so that the frame kernels' file and its objects stay as they are.)
__global__ void __launch_bounds__(kLmBlock) k_lm_scan(const int32_t* __restrict__ counts, int n, int32_t* __restrict__ offsets, int32_t* __restrict__ total)
{
    __shared__ int wave_sum[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int carry = 0;
    for (int base = 0; base < n; base += kLmBlock) {
        const int i = base + threadIdx.x;
        const int v = i < n ? counts[i] : 0;
        int x = v;                                              // inclusive scan within the wave
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) wave_sum[w] = x;
        __syncthreads();
        int before = carry;
        for (int j = 0; j < w; j++) before += wave_sum[j];
        if (i < n) offsets[i] = before + x - v;
        carry += ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
        __syncthreads();                                        // wave_sum is rewritten by the next chunk
    }
    if (threadIdx.x == 0) *total = carry;
}

// the blend of a face's three corner values by the weights of a texel's centre, per component, in the order mcpt.h writes it
__device__ __forceinline__ double lm_blend(double a, double b, double c, const double* w) { return (a * w[0] + b * w[1]) + c * w[2]; }

__global__ void __launch_bounds__(kLmBlock) k_lm_texels(const DTri* __restrict__ tris, const DTriShade* __restrict__ shade, const double* __restrict__ uv6,
                                                        int W, int H, const int32_t* __restrict__ owner, const int32_t* __restrict__ slot_of_face,
                                                        const unsigned long long* __restrict__ masks, const int32_t* __restrict__ offsets,
                                                        int32_t* __restrict__ texels, double* __restrict__ q6)
{
    const int i = blockIdx.x * kLmBlock + threadIdx.x;
    if (i >= W * H) return;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long* bm = masks + (size_t)blockIdx.x * 4;
    const unsigned long long mask = bm[w];
    if (!((mask >> lane) & 1ull)) return;
    int pos = offsets[blockIdx.x];
    for (int j = 0; j < w; j++) pos += __popcll(bm[j]);
    pos += (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)mask, 0u));
    if (texels) texels[pos] = i;
    if (!q6) return;
    const int k = slot_of_face[owner[i]];
    double uv[6], e[3], wt[3];
    lm_chart(tris, shade, uv6, k, uv);
    const double area2 = lightmap_area2(uv);
    lightmap_edges(uv, lightmap_centre(i % W, W), lightmap_centre(i / W, H), e);
    for (int c = 0; c < 3; c++) wt[c] = e[c] / area2;
    const DTri& tr = tris[k];
    const DTriShade& s = shade[k];
    double* q = q6 + (size_t)pos * 6;
    double nrm[3];
    for (int c = 0; c < 3; c++) {
        q[c] = lm_blend(tr.v1[c], tr.v2[c], tr.v3[c], wt);
        nrm[c] = lm_blend(s.vn1[c], s.vn2[c], s.vn3[c], wt);
    }
    const bool own = lightmap_normal_ok(nrm);                 // a blended normal of length zero, NaN or infinity: the face's
    for (int c = 0; c < 3; c++) q[3 + c] = own ? nrm[c] : tr.n[c];
}

// ---- step 4: the query's answers go to their texels, times pi (the full-precision constant: a mean of cosine-weighted radiance is an
// irradiance over pi).  One lane per (list entry, channel).
__global__ void __launch_bounds__(kLmBlock) k_lm_scatter(const int32_t* __restrict__ texels, long long n3, const double* __restrict__ mean,
                                                         const double* __restrict__ err_in, const int32_t* __restrict__ hits_in, double* __restrict__ irr,
                                                         double* __restrict__ err, int32_t* __restrict__ hits)
{
    const long long j = (long long)blockIdx.x * kLmBlock + threadIdx.x;
    if (j >= n3) return;
    const long long i = j / 3;
    const int c = (int)(j % 3);
    const size_t T = (size_t)texels[i];
    irr[T * 3 + c] = 3.141592653589793 * mean[j];
    if (err) err[T * 3 + c] = 3.141592653589793 * err_in[j];
    if (hits && c == 0) hits[T] = hits_in[i];
}

// ---- step 5, one round: a texel that is not valid (owner -1) takes the mean of its valid neighbours of the round before, summed in
// row-major order, and becomes valid with owner -1 - round; every other texel is copied.  Input and output are different buffers.
// CH channels a texel: 3 (irradiance) or 1 (an occlusion map).
template <int CH>
__global__ void __launch_bounds__(kLmBlock) k_lm_dilate(const double* __restrict__ irr_in, const int32_t* __restrict__ owner_in, int W, int H, int round,
                                                        double* __restrict__ irr_out, int32_t* __restrict__ owner_out)
{
    const int i = blockIdx.x * kLmBlock + threadIdx.x;
    if (i >= W * H) return;
    const int o = owner_in[i];
    double s[CH];
    for (int ch = 0; ch < CH; ch++) s[ch] = irr_in[(size_t)i * CH + ch];
    int out = o;
    if (o == -1) {
        const int x = i % W, y = i / W;
        double a[CH];
        for (int ch = 0; ch < CH; ch++) a[ch] = 0.0;
        int c = 0;
        for (int dy = -1; dy <= 1; dy++) {
            for (int dx = -1; dx <= 1; dx++) {
                const int xx = x + dx, yy = y + dy;
                if (xx < 0 || xx >= W || yy < 0 || yy >= H) continue;
                const size_t j = (size_t)yy * W + xx;
                if (owner_in[j] == -1) continue;                // (the texel itself among them)
                for (int ch = 0; ch < CH; ch++) a[ch] += irr_in[j * CH + ch];
                c++;
            }
        }
        if (c > 0) {
            for (int ch = 0; ch < CH; ch++) s[ch] = a[ch] / double(c);
            out = -1 - round;
        }
    }
    for (int ch = 0; ch < CH; ch++) irr_out[(size_t)i * CH + ch] = s[ch];
    owner_out[i] = out;
}

void launch_lightmap_raster(const DScene& S, const double* d_uv6, int W, int H, const LightmapWork& w, hipStream_t st)
{
    const int n = W * H;
    (void)hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(w.owner), kLightmapUnowned, size_t(n), st);
    (void)hipMemsetAsync(w.n_big, 0, sizeof(unsigned int), st);
    if (S.t > 0) {
        const unsigned want = blocks_of((long long)S.t * 64);
        hipLaunchKernelGGL(k_lm_raster, dim3(want < kLmMaxBlocks ? want : kLmMaxBlocks), dim3(kLmBlock), 0, st, S.tris, S.shade, S.t, d_uv6, W, H, w.owner,
                           w.slot_of_face, w.big, w.n_big);
        hipLaunchKernelGGL(k_lm_raster_big, dim3(kLmMaxBlocks), dim3(kLmBlock), 0, st, S.tris, S.shade, d_uv6, W, H, w.owner, w.big, w.n_big);
    }
    const int blocks = lightmap_blocks(n);
    hipLaunchKernelGGL(k_lm_select, dim3(blocks), dim3(kLmBlock), 0, st, w.owner, n, w.masks, w.block_counts);
    hipLaunchKernelGGL(k_lm_scan, dim3(1), dim3(kLmBlock), 0, st, w.block_counts, blocks, w.block_offsets, w.total);
}

void launch_lightmap_texels(const DScene& S, const double* d_uv6, int W, int H, const LightmapWork& w, int32_t* d_texels, double* d_q6, hipStream_t st)
{
    hipLaunchKernelGGL(k_lm_texels, dim3(lightmap_blocks((long long)W * H)), dim3(kLmBlock), 0, st, S.tris, S.shade, d_uv6, W, H, w.owner, w.slot_of_face,
                       w.masks, w.block_offsets, d_texels, d_q6);
}

void launch_lightmap_scatter(const int32_t* d_texels, long long n_list, const double* d_mean, const double* d_stderr, const int32_t* d_hits_in,
                             double* d_irr, double* d_err, int32_t* d_hits, hipStream_t st)
{
    if (n_list <= 0) return;
    hipLaunchKernelGGL(k_lm_scatter, dim3(blocks_of(n_list * 3)), dim3(kLmBlock), 0, st, d_texels, n_list * 3, d_mean, d_stderr, d_hits_in, d_irr, d_err,
                       d_hits);
}

void launch_lightmap_dilate(const double* d_in, const int32_t* d_owner_in, int W, int H, int round, double* d_out, int32_t* d_owner_out, int channels,
                            hipStream_t st)
{
    const dim3 grid(lightmap_blocks((long long)W * H));
    if (channels == 3)
        hipLaunchKernelGGL(k_lm_dilate<3>, grid, dim3(kLmBlock), 0, st, d_in, d_owner_in, W, H, round, d_out, d_owner_out);
    else
        hipLaunchKernelGGL(k_lm_dilate<1>, grid, dim3(kLmBlock), 0, st, d_in, d_owner_in, W, H, round, d_out, d_owner_out);
}

}  // namespace mcpt
