// Hand-written HIP kernels for gfx950 (MI355X): the reference's per-pixel integrator loop
// generateImg -> ray_intersect/bvh_intersect -> shade -> nextRay (MTPC/pathTracing.cpp), in fp64 with the
// reference's operation order.  Built with -ffp-contract=off: a fused multiply-add would change the last
// bit of the hit tests and with it the closest-hit triangle.
//
// No MFMA: this is per-lane tree walking and branching, not a contraction.  wave64 throughout.
#include <hip/hip_runtime.h>

#include "accel_build.hpp"
#include "dev_common.hpp"
#include "kernels.hpp"
#include "shade_common.hpp"
#include "shade_path.hpp"
#include "trace_persistent.hpp"
#include "trace_pool.hpp"

namespace mcpt {

// ------------------------------------------------------------------------------------------------ kernels
// mcpt_trace_closest with the reference-shaped walk: one lane per ray.  LEAF: face receives the leaf index, not the .obj face (the
// caller shades at the hit: launch_trace_closest_leaf), and no normal is formed.
template <bool LEAF>
__global__ void __launch_bounds__(256) k_trace_closest_reference(DScene S, const double* __restrict__ rays, long long n,
                                                       int32_t* __restrict__ face, double* __restrict__ t_out,
                                                       double* __restrict__ p_out, double* __restrict__ pn_out, DCounters* ctr)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    LaneStats ls;
    if (gid < n) {
        Ray r;
        r.o = ld3(rays + gid * 6); r.d = ld3(rays + gid * 6 + 3);
        Hit h; Work w = {0, 0};
        const bool ok = trace_closest(S, r, h, w);
        ls.nodes = w.nodes; ls.tris = w.tris; ls.primary = 1;
        V3 pn = mk(0, 0, 0);
        if (ok && !LEAF) pn = hit_normal(S, h);
        if (face) face[gid] = ok ? (LEAF ? h.leaf : S.tris[h.leaf].face) : -1;
        if (t_out) t_out[gid] = ok ? h.t : 0.0;
        if (p_out) { p_out[gid * 3] = h.p.x; p_out[gid * 3 + 1] = h.p.y; p_out[gid * 3 + 2] = h.p.z; }
        if (pn_out) { pn_out[gid * 3] = pn.x; pn_out[gid * 3 + 1] = pn.y; pn_out[gid * 3 + 2] = pn.z; }
    }
    flush_stats(ctr, ls);
}

// ---- persistent fast walk over a plain ray array (mcpt_trace_closest) and over the primary rays
struct ArrayRaySource {
    static constexpr bool kWantsPoint = true;
    static constexpr bool kSparse = false;          // every slot holds a ray
    const double* rays; long long n;
    int32_t* leaf_out; double* t_out; double* p_out;     // leaf_out receives the LEAF index; k_finish_hits turns it into a face
    __device__ __forceinline__ long long total() const { return n; }
    __device__ __forceinline__ bool fetch(long long q, Ray& r) const
    {
        r.o = ld3(rays + q * 6); r.d = ld3(rays + q * 6 + 3);
#ifdef MCPT_DBG_INVALID        /* debugging builds: a pseudo-random quarter of the slots holds no ray */
        return ((((unsigned int)q * 2654435761u) >> 7) & 3u) != 0u;
#else
        return true;
#endif
    }
    __device__ __forceinline__ void store(long long q, bool ok, const Hit& h) const
    {
        leaf_out[q] = ok ? h.leaf : -1;
        t_out[q] = ok ? h.t : 0.0;
        p_out[q * 3] = h.p.x; p_out[q * 3 + 1] = h.p.y; p_out[q * 3 + 2] = h.p.z;
    }
};

struct PrimaryRaySource {
    static constexpr bool kWantsPoint = true;
    static constexpr bool kSparse = false;
    const double* dirs; const int32_t* pixels; int n_pixels; double eye[3]; PrimaryHit* hits;
    __device__ __forceinline__ long long total() const { return n_pixels; }
    __device__ __forceinline__ bool fetch(long long q, Ray& r) const
    {
        const int pix = pixels ? pixels[q] : (int)q;
        r.o = ld3(eye); r.d = ld3(dirs + (size_t)pix * 3);
        return true;
    }
    __device__ __forceinline__ void store(long long q, bool ok, const Hit& h) const
    {
        PrimaryHit ph;
        ph.leaf = ok ? h.leaf : -1; ph.surf = 0; ph.t = h.t; ph.p[0] = h.p.x; ph.p[1] = h.p.y; ph.p[2] = h.p.z;
        hits[q] = ph;
    }
};

template <class Src, int STACK, int WAVES>
__global__ void __launch_bounds__(256, WAVES) k_trace_persistent(DScene S, Src src, TraceQueue* queue, long long* slow_list, unsigned int slow_cap,
                                                                long long chunk, DCounters* ctr)
{
    __shared__ int lds_stack[STACK * 256];
    __shared__ double lds_rays[4 * MCPT_RAYBUF_BYTES / 8];
    LaneStats ls;
    Work w = {0, 0};
    trace_persistent(S, src, queue, slow_list, slow_cap, chunk, lds_stack + threadIdx.x, 256, lds_rays + (threadIdx.x >> 6) * (MCPT_RAYBUF_BYTES / 8), w, S.fast.stack_cap < STACK ? S.fast.stack_cap : STACK);
    ls.nodes = w.nodes; ls.tris = w.tris;
    { const unsigned long long tw = wave_sum(w.pre_wrong); if ((threadIdx.x & 63) == 0 && tw && ctr) atomicAdd(&ctr->pre_wrong, tw); }
    flush_stats(ctr, ls);
}

template <class Src, int NW, int KT, int SCAP>
__global__ void __launch_bounds__(NW * 64, 1) k_trace_pool(DScene S, Src src, TraceQueue* queue, long long* slow_list, unsigned int slow_cap,
                                                          long long chunk, DCounters* ctr)
{
    __shared__ PoolLds<NW, KT, SCAP> L;
    LaneStats ls;
    Work w = {0, 0};
    trace_pool<Src, NW, KT, SCAP>(S, src, queue, slow_list, slow_cap, chunk, L, w, reinterpret_cast<int*>(slow_list + slow_cap));
    ls.nodes = w.nodes; ls.tris = w.tris;
    { const unsigned long long tw = wave_sum(w.pre_wrong); if ((threadIdx.x & 63) == 0 && tw && ctr) atomicAdd(&ctr->pre_wrong, tw); }
    flush_stats(ctr, ls);
}

template <class Src>
__global__ void __launch_bounds__(256) k_trace_slow(DScene S, Src src, const TraceQueue* queue, const long long* slow_list, unsigned int slow_cap,
                                                    DCounters* ctr)
{
    __shared__ int lds_stack[MCPT_FAST_STACK * 256];
    LaneStats ls;
    Work w = {0, 0};
    trace_slow_list(S, src, queue, slow_list, slow_cap, w, lds_stack + threadIdx.x);
    ls.nodes = w.nodes; ls.tris = w.tris;
    flush_stats(ctr, ls);
}

// leaf index -> .obj face index, interpolated normal of the accepted hit
__global__ void k_finish_hits(DScene S, long long n, int32_t* __restrict__ face, const double* __restrict__ p, double* __restrict__ pn_out, DCounters* ctr)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    LaneStats ls;
    if (gid < n) {
        ls.primary = 1;
        const int leaf = face[gid];
        V3 pn = mk(0, 0, 0);
        if (leaf >= 0) {
            Hit h; h.leaf = leaf; h.t = 0; h.p = ld3(p + gid * 3);
            pn = hit_normal(S, h);
            face[gid] = S.tris[leaf].face;
        }
        if (pn_out) { pn_out[gid * 3] = pn.x; pn_out[gid * 3 + 1] = pn.y; pn_out[gid * 3 + 2] = pn.z; }
    }
    flush_stats(ctr, ls);
}

// Pixel positions: pos(i,0) = start - pdy*i, pos(i,j+1) = pos(i,j) + pdx -- a running sum along each row
// (pathTracing.cpp:297,326), so one thread walks one row.  Writes the normalised primary direction.
__global__ void k_primary_dirs(DCamera cam, double* __restrict__ dirs)
{
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= cam.height) return;
    const V3 eye = ld3(cam.eye), pdx = ld3(cam.pdx);
    V3 pos = ld3(cam.start_point) - ld3(cam.pdy) * (double)row;
    double* out = dirs + (size_t)row * cam.width * 3;
    for (int j = 0; j < cam.width; j++) {
        const V3 d = normalized(pos - eye);
        out[j * 3] = d.x; out[j * 3 + 1] = d.y; out[j * 3 + 2] = d.z;
        pos = pos + pdx;
    }
}

// One lane per owned pixel: the primary ray is the same for every sample of a pixel (no jitter,
// pathTracing.cpp:306-308), so it is traced once.
__global__ void __launch_bounds__(256) k_primary_hits_reference(DScene S, const double* __restrict__ dirs, const int32_t* __restrict__ pixels,
                                                      int n_pixels, PrimaryHit* __restrict__ hits, DCounters* ctr)
{
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    LaneStats ls;
    if (gid < n_pixels) {
        const int pix = pixels ? pixels[gid] : gid;
        Ray r;
        r.o = ld3(S.cam.eye); r.d = ld3(dirs + (size_t)pix * 3);
        Hit h; Work w = {0, 0};
        const bool ok = trace_closest(S, r, h, w);
        ls.nodes = w.nodes; ls.tris = w.tris; ls.primary = 1;
        PrimaryHit ph;
        ph.leaf = ok ? h.leaf : -1; ph.surf = 0; ph.t = h.t; ph.p[0] = h.p.x; ph.p[1] = h.p.y; ph.p[2] = h.p.z;
        hits[gid] = ph;
    }
    flush_stats(ctr, ls);
}

// One lane per camera sample.  Samples of one pixel are consecutive lanes, so a wave starts from one shared
// primary hit (coherent first vertex and shadow rays).  Radiance goes to rad[(slot*spp + k)*3]; lane k of a slot renders camera
// sample sample_base + k (a whole frame: 0).  ENV: S.env is active (a pixel whose primary ray missed is folded from Le, not from rad).
// PICK: the pick mode of S.pick, 0 (none), 1 (MCPT_LIGHTS_ONE) or 2 (MCPT_LIGHTS_TREE): shade_path.hpp.
template <bool ENV, int PICK>
__global__ void __launch_bounds__(256) k_shade_samples(DScene S, unsigned long long seed, const double* __restrict__ dirs,
                                                       const int32_t* __restrict__ pixels, const PrimaryHit* __restrict__ hits,
                                                       int first_slot, long long n_samples, int spp, int sample_base, double* __restrict__ rad, DCounters* ctr)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    LaneStats ls;
    if (gid < n_samples) {
        const int slot = first_slot + (int)(gid / spp);
        const int k = (int)(gid % spp);
        const int pix = pixels ? pixels[slot] : slot;
        const PrimaryHit ph = hits[slot];
        ls.samples = 1;
        double r[3] = {0, 0, 0};
        if (ph.leaf >= 0) {
            RngKey key; key.k0 = (uint32_t)seed; key.k1 = (uint32_t)(seed >> 32); key.pixel = (uint32_t)pix; key.sample = (uint32_t)(sample_base + k);
            Hit h; h.leaf = ph.leaf; h.t = ph.t; h.p = mk(ph.p[0], ph.p[1], ph.p[2]);
            shade_path<ENV, PICK>(S, key, ld3(dirs + (size_t)pix * 3), h, r, ls);
        }
        rad[gid * 3] = r[0]; rad[gid * 3 + 1] = r[1]; rad[gid * 3 + 2] = r[2];
    }
    flush_stats(ctr, ls);
}

// mcpt_sample_radiance: arbitrary (pixel, k) pairs, primary ray traced per sample.
template <bool ENV, int PICK>
__global__ void __launch_bounds__(256) k_sample_radiance(DScene S, unsigned long long seed, const double* __restrict__ dirs,
                                                         const int32_t* __restrict__ pix, const int32_t* __restrict__ ks, long long n,
                                                         double* __restrict__ rgb, DCounters* ctr)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    LaneStats ls;
    if (gid < n) {
        Ray r; r.o = ld3(S.cam.eye); r.d = ld3(dirs + (size_t)pix[gid] * 3);
        Hit h; Work w = {0, 0};
        double out[3] = {0, 0, 0};
        ls.primary = 1; ls.samples = 1;
        if (trace_closest(S, r, h, w)) {
            RngKey key; key.k0 = (uint32_t)seed; key.k1 = (uint32_t)(seed >> 32); key.pixel = (uint32_t)pix[gid]; key.sample = (uint32_t)ks[gid];
            shade_path<ENV, PICK>(S, key, r.d, h, out, ls);
        } else if (ENV) env_camera_miss(S, r.d, out);
        ls.nodes += w.nodes; ls.tris += w.tris;
        rgb[gid * 3] = out[0]; rgb[gid * 3 + 1] = out[1]; rgb[gid * 3 + 2] = out[2];
    }
    flush_stats(ctr, ls);
}

// mcpt_light_pick: the light MCPT_LIGHTS_ONE picks at vertex `depth` of camera samples (pix[i], ks[i])
__global__ void __launch_bounds__(256) k_light_pick(DLightPick pick, int nl, unsigned long long seed, const int32_t* __restrict__ pix, const int32_t* __restrict__ ks,
                                                    int depth, long long n, int32_t* __restrict__ light)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n) return;
    RngKey key; key.k0 = (uint32_t)seed; key.k1 = (uint32_t)(seed >> 32); key.pixel = (uint32_t)pix[gid]; key.sample = (uint32_t)ks[gid];
    double inv_p;
    light[gid] = light_pick(pick, key, (uint32_t)depth, (uint32_t)nl, inv_p);
}

// mcpt_light_pick_at: the light MCPT_LIGHTS_TREE picks at the vertices (p[i], pn[i]) at `depth` of camera samples (pix[i], ks[i]), and its probability
__global__ void __launch_bounds__(256) k_light_pick_at(DLightPick pick, int nl, unsigned long long seed, const int32_t* __restrict__ pix, const int32_t* __restrict__ ks,
                                                       int depth, const double* __restrict__ p, const double* __restrict__ pn, long long n,
                                                       int32_t* __restrict__ light, double* __restrict__ pdf)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n) return;
    RngKey key; key.k0 = (uint32_t)seed; key.k1 = (uint32_t)(seed >> 32); key.pixel = (uint32_t)pix[gid]; key.sample = (uint32_t)ks[gid];
    double q;
    light[gid] = light_pick_at(pick, key, (uint32_t)depth, (uint32_t)nl, ld3(p + gid * 3), ld3(pn + gid * 3), q);
    pdf[gid] = q;
}

// Per pixel: acc(float) += radiance/N for k = 0..N-1 in order (pathTracing.cpp:301,316-318 with D3), widened
// to double for image::img (sceneManagement.h:221).  One lane per (pixel, channel).  ENV: a pixel whose primary ray missed folds
// Le(primary direction) for each of its samples, through the same float fold.
template <bool ENV>
__global__ void k_fold_samples(const double* __restrict__ rad, const int32_t* __restrict__ pixels, const PrimaryHit* __restrict__ hits,
                               int first_slot, int n_slots, int spp, double* __restrict__ img, DEnv env, const double* __restrict__ dirs)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)n_slots * 3) return;
    const int s = (int)(gid / 3), c = (int)(gid % 3);
    const double* src = rad + (size_t)s * spp * 3 + c;
    const int slot = first_slot + s;
    float acc = 0.0f;
    if (hits[slot].leaf >= 0)            // a primary miss adds nothing (pathTracing.cpp:311)
        for (int k = 0; k < spp; k++) acc = (float)((double)acc + src[(size_t)k * 3] / spp);
    else if (ENV) {                      // ... but the environment's radiance
        const V3 le = env_eval(env, ld3(dirs + (size_t)(pixels ? pixels[slot] : slot) * 3));
        const double x = c == 0 ? le.x : (c == 1 ? le.y : le.z);
        for (int k = 0; k < spp; k++) acc = (float)((double)acc + x / spp);
    }
    const int pix = pixels ? pixels[slot] : slot;
    img[(size_t)pix * 3 + c] = (double)acc;
}

// ---- progressive frames (mcpt_progressive_*): samples [k0, k0 + n) of a frame of N per pass
// The fold of k_fold_samples continued from where the previous pass left it: acc starts from the float the fp64 image holds (exactly a
// float), so once every pass is in, img is k_fold_samples' frame bit for bit whatever the pass boundaries were.  Beside it the pixel's
// first and second moments of the radiance, in fp64 in k order: mom[pix][0][c] = sum x, mom[pix][1][c] = sum x*x (no contraction:
// the library is built with -ffp-contract=off).  hit[pix] records whether the pixel's primary ray hit (k_noise_reduce counts only those).
// One lane per (slot, channel).  ENV: a missed pixel's image continues the fold of Le(primary direction), its first moment the sum.
// (A pixel is hit or missed for the whole frame here.  The pieces of a motion frame, where that changes from step to step, fold through
// k_fold_motion in camera.hip: the same fold and moments, a change to either belongs in both.)
template <bool ENV>
__global__ void k_fold_progressive(const double* __restrict__ rad, const int32_t* __restrict__ pixels, const PrimaryHit* __restrict__ hits,
                                   int first_slot, int n_slots, int n, int k0, int N, double* __restrict__ img, double* __restrict__ mom,
                                   uint8_t* __restrict__ hit, DEnv env, const double* __restrict__ dirs)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)n_slots * 3) return;
    const int s = (int)(gid / 3), c = (int)(gid % 3);
    const int slot = first_slot + s;
    const int pix = pixels ? pixels[slot] : slot;
    const bool h = hits[slot].leaf >= 0;
    if (c == 0) hit[pix] = h ? 1 : 0;
    if (!h) {                                               // a primary miss adds nothing (pathTracing.cpp:311); its moments stay 0
        if (ENV) {                                          // every sample of the pixel is Le(primary direction): the image holds the whole
            const V3 le = env_eval(env, ld3(dirs + (size_t)pix * 3));      // frame's fold from the first pass on (mcpt_progressive_image shows it
            const double x = c == 0 ? le.x : (c == 1 ? le.y : le.z);      // for a missed pixel at any count); the first moment sums the samples
            double* m = mom + (size_t)pix * 6 + c;                          // so far, the second stays 0 (standard error 0)
            float acc = 0.0f;
            for (int k = 0; k < N; k++) acc = (float)((double)acc + x / N);
            double s1 = k0 > 0 ? m[0] : 0.0;
            for (int k = 0; k < n; k++) s1 += x;
            img[(size_t)pix * 3 + c] = (double)acc;
            m[0] = s1; m[3] = 0.0;
        } else img[(size_t)pix * 3 + c] = 0.0;
        return;
    }
    const double* src = rad + (size_t)s * n * 3 + c;
    double* m = mom + (size_t)pix * 6 + c;
    float acc = k0 > 0 ? (float)img[(size_t)pix * 3 + c] : 0.0f;
    double s1 = k0 > 0 ? m[0] : 0.0, s2 = k0 > 0 ? m[3] : 0.0;
    for (int k = 0; k < n; k++) {
        const double x = src[(size_t)k * 3];
        acc = (float)((double)acc + x / N);
        s1 += x;
        s2 += x * x;
    }
    img[(size_t)pix * 3 + c] = (double)acc;
    m[0] = s1; m[3] = s2;
}

// Frame summary (k_noise_reduce + k_noise_final): over the owned hit pixels, sum se2 and sum mean^2 of every channel and the pixel count.
// Deterministic and independent of the device: the pixel list is cut into `ranges` contiguous ranges (a number fixed by the pixel count,
// not by the grid), block r reduces range r -- thread t takes the range's pixels t, t + 256, ... in order, the waves reduce with a fixed
// __shfl_xor butterfly, wave 0 adds the four wave sums in order -- and one block adds the ranges' partials the same way.  No atomics.
__device__ __forceinline__ double wave_sum_fixed(double v)
{
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ void block_sum3(double v[3], double* out)
{
    __shared__ double part[4][3];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = 0; i < 3; i++) v[i] = wave_sum_fixed(v[i]);
    if (lane == 0) for (int i = 0; i < 3; i++) part[w][i] = v[i];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 0; i < 3; i++) out[i] = ((part[0][i] + part[1][i]) + part[2][i]) + part[3][i];
}
// PER_PIXEL (adaptive frames): every pixel with its own sample count cnt[pix] instead of `done`.
template <bool PER_PIXEL>
__global__ void __launch_bounds__(256) k_noise_reduce(const int32_t* __restrict__ pixels, long long n_pixels, long long per_range,
                                                      const double* __restrict__ mom, const uint8_t* __restrict__ hit, int done,
                                                      const int32_t* __restrict__ cnt, double* __restrict__ partials)
{
    const long long lo = (long long)blockIdx.x * per_range;
    const long long hi = lo + per_range < n_pixels ? lo + per_range : n_pixels;
    double v[3] = {0.0, 0.0, 0.0};
    for (long long i = lo + threadIdx.x; i < hi; i += 256) {
        const int pix = pixels ? pixels[i] : (int)i;
        if (!hit[pix]) continue;
        const double* m = mom + (size_t)pix * 6;
        const int k = PER_PIXEL ? cnt[pix] : done;
        for (int c = 0; c < 3; c++) {
            const double mean = m[c] / k;
            v[0] += progressive_se2(m[c], m[3 + c], k);
            v[1] += mean * mean;
        }
        v[2] += 1.0;
    }
    block_sum3(v, partials + (size_t)blockIdx.x * 3);
}
__global__ void __launch_bounds__(256) k_noise_final(const double* __restrict__ partials, int ranges, double* __restrict__ out)
{
    double v[3] = {0.0, 0.0, 0.0};
    for (int r = threadIdx.x; r < ranges; r += 256)
        for (int i = 0; i < 3; i++) v[i] += partials[(size_t)r * 3 + i];
    block_sum3(v, out);
    if (threadIdx.x == 0) out[3] = 0.0;
}

// Current estimate and (est_err != null) the standard error of every owned pixel after `done` of N samples.  done == N: the float fold
// itself (the frame mcpt_render computes); done < N: the fp64 mean s1 / done, which is not the float fold.  Error: sqrt(se2), 0 for
// done < 2.  One lane per (owned pixel, channel); other pixels are not touched.  PER_PIXEL (adaptive frames): the pixel's own count
// cnt[pix] in place of `done`.
// (one lane per (owned pixel, channel): a pixel whose primary ray missed shows its image -- under an environment, the whole frame's fold)
__global__ void k_missed_image(const int32_t* __restrict__ pixels, long long n_pixels, const uint8_t* __restrict__ hit, const double* __restrict__ img,
                               double* __restrict__ est)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n_pixels * 3) return;
    const int pix = pixels ? pixels[gid / 3] : (int)(gid / 3);
    const size_t i = (size_t)pix * 3 + (int)(gid % 3);
    if (!hit[pix]) est[i] = img[i];
}

template <bool PER_PIXEL>
__global__ void k_progressive_image(const int32_t* __restrict__ pixels, long long n_pixels, const double* __restrict__ img,
                                    const double* __restrict__ mom, int done, const int32_t* __restrict__ cnt, int N, double* __restrict__ est,
                                    double* __restrict__ est_err)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n_pixels * 3) return;
    const int c = (int)(gid % 3);
    const int pix = pixels ? pixels[gid / 3] : (int)(gid / 3);
    const size_t i = (size_t)pix * 3 + c;
    const double* m = mom + (size_t)pix * 6 + c;
    const int k = PER_PIXEL ? cnt[pix] : done;
    if (est) est[i] = k == N ? img[i] : (k > 0 ? m[0] / k : 0.0);
    if (est_err) est_err[i] = k >= 2 ? sqrt(progressive_se2(m[0], m[3], k)) : 0.0;
}

// ---- adaptive frames: which pixels of the active list continue after a pass of k samples, and the next list (order kept)
// Three kernels, no atomics.  select: one lane per list entry, 256-lane blocks of four waves; each wave stores the __ballot of its keep
// flags (masks[wave]) and the block stores its count; every listed pixel's count becomes k.  scan: one workgroup turns the block counts
// into exclusive offsets and writes the total.  scatter: a kept lane's position is its block's offset, the popcounts of the waves before
// it in the block and the set bits of its wave's mask below it (v_mbcnt).  An order-preserving compaction has one correct output, so the
// list is deterministic.  The rule (mcpt.h, mcpt_progressive_create_adaptive) reads the pixel's own moments only; fp64, no contraction
// (-ffp-contract=off), channels summed in order 0, 1, 2.
__global__ void __launch_bounds__(256) k_adaptive_select(const int32_t* __restrict__ list, int n, const double* __restrict__ mom,
                                                         const uint8_t* __restrict__ hit, int k, int min_spp, double rel2, double abs2,
                                                         int32_t* __restrict__ cnt, unsigned long long* __restrict__ masks,
                                                         int32_t* __restrict__ block_counts)
{
    __shared__ int wave_count[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    bool keep = false;
    if (i < n) {
        const int pix = list[i];
        cnt[pix] = k;
        if (hit[pix]) {
            keep = k < min_spp;
            if (!keep) {
                const double* m = mom + (size_t)pix * 6;
                double se2 = 0.0, m2 = 0.0;
                for (int c = 0; c < 3; c++) {
                    const double mean = m[c] / k;
                    se2 += progressive_se2(m[c], m[3 + c], k);
                    m2 += mean * mean;
                }
                keep = !(se2 < rel2 * m2 + abs2);
            }
        }
    }
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) {
        masks[(size_t)blockIdx.x * 4 + w] = mask;
        wave_count[w] = __popcll(mask);
    }
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = ((wave_count[0] + wave_count[1]) + wave_count[2]) + wave_count[3];
}

// Exclusive scan of n block counts into offsets, in chunks of 256 with a running carry; *total = the sum.  One workgroup of 256.
__global__ void __launch_bounds__(256) k_adaptive_scan(const int32_t* __restrict__ counts, int n, int32_t* __restrict__ offsets,
                                                       int32_t* __restrict__ total)
{
    __shared__ int wave_sum[4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int carry = 0;
    for (int base = 0; base < n; base += 256) {
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

__global__ void __launch_bounds__(256) k_adaptive_scatter(const int32_t* __restrict__ list, int n, const unsigned long long* __restrict__ masks,
                                                          const int32_t* __restrict__ offsets, int32_t* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long* bm = masks + (size_t)blockIdx.x * 4;
    const unsigned long long mask = bm[w];
    if (!((mask >> lane) & 1ull)) return;
    int pos = offsets[blockIdx.x];
    for (int j = 0; j < w; j++) pos += __popcll(bm[j]);
    pos += (int)__builtin_amdgcn_mbcnt_hi((unsigned int)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)mask, 0u));
    out[pos] = list[i];
}

// End-of-frame exchange of the multi-GPU entry (multi_device.cpp): a rank's pixels leave its frame as one compact buffer
// (pack, on the rank's GPU) and are put at their frame positions on GPU 0 (unpack).  One lane per (pixel, channel).
__global__ void k_pack_pixels(const double* __restrict__ frame, const int32_t* __restrict__ pixels, long long n3, double* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n3) out[i] = frame[(size_t)pixels[i / 3] * 3 + (i % 3)];
}
__global__ void k_unpack_pixels(const double* __restrict__ in, const int32_t* __restrict__ pixels, long long n3, double* __restrict__ frame)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n3) frame[(size_t)pixels[i / 3] * 3 + (i % 3)] = in[i];
}

// ------------------------------------------------------------------------------------------------ launchers
static inline unsigned blocks_for(long long n, int block) { return (unsigned)((n + block - 1) / block); }

template <class Src>
static void launch_persistent(const DScene& S, const Src& src, long long total, TraceQueue* queue, long long* slow_list, unsigned int slow_cap,
                              DCounters* ctr, hipStream_t st, int grid, int grid_short, const LaunchCfg& cfg)
{
    const bool shallow = S.fast.stack_limit <= kFastShortStack;
    const int resident = shallow ? grid_short : grid;
    const long long blocks_needed = (total + 255) / 256;
    const int g = (int)(blocks_needed < resident ? blocks_needed : resident);
    (void)hipMemsetAsync(queue, 0, sizeof(TraceQueue), st);
    if (cfg.trace_pool && total < (1ll << 32)) {        // (the pool engine keeps a ray's slot number in 32 bits)
        const long long per_block = cfg.trace_block_rays * (MCPT_POOL_WAVES / 4);
        const long long nb = (total + per_block - 1) / per_block;
        const int gp = (int)(nb < cfg.cus ? nb : cfg.cus);
        long long c = total / ((long long)gp * MCPT_POOL_WAVES * 4);
        c = (c / 64) * 64; c = c < cfg.min_chunk ? cfg.min_chunk : (c > cfg.max_chunk ? cfg.max_chunk : c);
        hipLaunchKernelGGL((k_trace_pool<Src, MCPT_POOL_WAVES, MCPT_POOL_KT, MCPT_POOL_STACK>), dim3(gp), dim3(MCPT_POOL_WAVES * 64), 0, st, S, src, queue, slow_list, slow_cap, c, ctr);
    } else if (shallow) hipLaunchKernelGGL((k_trace_persistent<Src, kFastShortStack, 4>), dim3(g), dim3(256), 0, st, S, src, queue, slow_list, slow_cap, persistent_chunk(total, g), ctr);
    else hipLaunchKernelGGL((k_trace_persistent<Src, MCPT_FAST_STACK, 3>), dim3(g), dim3(256), 0, st, S, src, queue, slow_list, slow_cap, persistent_chunk(total, g), ctr);
    hipLaunchKernelGGL(k_trace_slow<Src>, dim3(256), dim3(256), 0, st, S, src, queue, slow_list, slow_cap, ctr);
}

bool pool_engine_available_closest()
{
    int a = 0, b = 0;
    const hipError_t e1 = hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &a, reinterpret_cast<const void*>(k_trace_pool<ArrayRaySource, MCPT_POOL_WAVES, MCPT_POOL_KT, MCPT_POOL_STACK>), MCPT_POOL_WAVES * 64, 0);
    const hipError_t e2 = hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &b, reinterpret_cast<const void*>(k_trace_pool<PrimaryRaySource, MCPT_POOL_WAVES, MCPT_POOL_KT, MCPT_POOL_STACK>), MCPT_POOL_WAVES * 64, 0);
    if (e1 != hipSuccess || e2 != hipSuccess) (void)hipGetLastError();
    return e1 == hipSuccess && e2 == hipSuccess && a >= 1 && b >= 1;
}

void init_launch_cfg_closest(LaunchCfg& cfg)
{
    cfg.array_grid = persistent_grid(reinterpret_cast<const void*>(k_trace_persistent<ArrayRaySource, MCPT_FAST_STACK, 3>), cfg.cus);
    cfg.primary_grid = persistent_grid(reinterpret_cast<const void*>(k_trace_persistent<PrimaryRaySource, MCPT_FAST_STACK, 3>), cfg.cus);
    cfg.array_grid_short = persistent_grid(reinterpret_cast<const void*>(k_trace_persistent<ArrayRaySource, kFastShortStack, 4>), cfg.cus);
    cfg.primary_grid_short = persistent_grid(reinterpret_cast<const void*>(k_trace_persistent<PrimaryRaySource, kFastShortStack, 4>), cfg.cus);
}

// d_face, d_t, d_p must be non-null device buffers (the C-ABI layer always allocates them); d_pn may be null
void launch_trace_closest(const DScene& S, bool fast, const double* d_rays, long long n, int32_t* d_face, double* d_t, double* d_p,
                          double* d_pn, DCounters* ctr, TraceQueue* queue, long long* slow_list, unsigned int slow_cap, hipStream_t st,
                          const LaunchCfg& cfg)
{
    if (n <= 0) return;
    if (!fast) {
        hipLaunchKernelGGL(k_trace_closest_reference<false>, dim3(blocks_for(n, 256)), dim3(256), 0, st, S, d_rays, n, d_face, d_t, d_p, d_pn, ctr);
        return;
    }
    ArrayRaySource src; src.rays = d_rays; src.n = n; src.leaf_out = d_face; src.t_out = d_t; src.p_out = d_p;
    launch_persistent(S, src, n, queue, slow_list, slow_cap, ctr, st, cfg.array_grid, cfg.array_grid_short, cfg);
    hipLaunchKernelGGL(k_finish_hits, dim3(blocks_for(n, 256)), dim3(256), 0, st, S, n, d_face, d_p, d_pn, ctr);
}
// The same launch, handing back the leaf of every hit (-1: a miss) instead of its .obj face: what vertex_surface needs.  The walks, and so
// t and p, are launch_trace_closest's; only the last step (leaf -> face, the hit's normal) is left out.
void launch_trace_closest_leaf(const DScene& S, bool fast, const double* d_rays, long long n, int32_t* d_leaf, double* d_t, double* d_p,
                               DCounters* ctr, TraceQueue* queue, long long* slow_list, unsigned int slow_cap, hipStream_t st, const LaunchCfg& cfg)
{
    if (n <= 0) return;
    if (!fast) {
        hipLaunchKernelGGL(k_trace_closest_reference<true>, dim3(blocks_for(n, 256)), dim3(256), 0, st, S, d_rays, n, d_leaf, d_t, d_p, (double*)nullptr, ctr);
        return;
    }
    ArrayRaySource src; src.rays = d_rays; src.n = n; src.leaf_out = d_leaf; src.t_out = d_t; src.p_out = d_p;
    launch_persistent(S, src, n, queue, slow_list, slow_cap, ctr, st, cfg.array_grid, cfg.array_grid_short, cfg);
}
void launch_pack_pixels(const double* d_frame, const int32_t* d_pixels, long long n_pixels, double* d_out, hipStream_t st)
{
    if (n_pixels <= 0) return;
    hipLaunchKernelGGL(k_pack_pixels, dim3(blocks_for(n_pixels * 3, 256)), dim3(256), 0, st, d_frame, d_pixels, n_pixels * 3, d_out);
}
void launch_unpack_pixels(const double* d_in, const int32_t* d_pixels, long long n_pixels, double* d_frame, hipStream_t st)
{
    if (n_pixels <= 0) return;
    hipLaunchKernelGGL(k_unpack_pixels, dim3(blocks_for(n_pixels * 3, 256)), dim3(256), 0, st, d_in, d_pixels, n_pixels * 3, d_frame);
}
void launch_primary_dirs(const DCamera& cam, double* d_dirs, hipStream_t st)
{
    hipLaunchKernelGGL(k_primary_dirs, dim3(blocks_for(cam.height, 64)), dim3(64), 0, st, cam, d_dirs);
}
void launch_primary_hits(const DScene& S, bool fast, const double* d_dirs, const int32_t* d_pixels, int n_pixels, PrimaryHit* d_hits,
                         DCounters* ctr, TraceQueue* queue, long long* slow_list, unsigned int slow_cap, hipStream_t st, const LaunchCfg& cfg)
{
    if (n_pixels <= 0) return;
    if (!fast) {
        hipLaunchKernelGGL(k_primary_hits_reference, dim3(blocks_for(n_pixels, 256)), dim3(256), 0, st, S, d_dirs, d_pixels, n_pixels, d_hits, ctr);
        return;
    }
    PrimaryRaySource src; src.dirs = d_dirs; src.pixels = d_pixels; src.n_pixels = n_pixels; src.hits = d_hits;
    src.eye[0] = S.cam.eye[0]; src.eye[1] = S.cam.eye[1]; src.eye[2] = S.cam.eye[2];
    launch_persistent(S, src, n_pixels, queue, slow_list, slow_cap, ctr, st, cfg.primary_grid, cfg.primary_grid_short, cfg);
}
void launch_shade_samples(const DScene& S, unsigned long long seed, const double* d_dirs, const int32_t* d_pixels,
                          const PrimaryHit* d_hits, int first_slot, int n_slots, int spp, int sample_base, double* d_rad, DCounters* ctr, hipStream_t st)
{
    const long long n = (long long)n_slots * spp;
    if (n <= 0) return;
    const dim3 grid(blocks_for(n, 256));
    with_path_variant(S, [&](auto env, auto pick) {
        hipLaunchKernelGGL((k_shade_samples<env(), pick()>), grid, dim3(256), 0, st, S, seed, d_dirs, d_pixels, d_hits, first_slot, n, spp, sample_base, d_rad, ctr);
    });
}
void launch_sample_radiance(const DScene& S, unsigned long long seed, const double* d_dirs, const int32_t* d_pix, const int32_t* d_k,
                            long long n, double* d_rgb, DCounters* ctr, hipStream_t st)
{
    if (n <= 0) return;
    const dim3 grid(blocks_for(n, 256));
    with_path_variant(S, [&](auto env, auto pick) {
        hipLaunchKernelGGL((k_sample_radiance<env(), pick()>), grid, dim3(256), 0, st, S, seed, d_dirs, d_pix, d_k, n, d_rgb, ctr);
    });
}
void launch_light_pick(const DScene& S, unsigned long long seed, const int32_t* d_pix, const int32_t* d_k, int depth, long long n, int32_t* d_light, hipStream_t st)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_light_pick, dim3(blocks_for(n, 256)), dim3(256), 0, st, S.pick, S.num_lights, seed, d_pix, d_k, depth, n, d_light);
}
void launch_light_pick_at(const DScene& S, unsigned long long seed, const int32_t* d_pix, const int32_t* d_k, int depth, const double* d_p, const double* d_pn,
                          long long n, int32_t* d_light, double* d_pdf, hipStream_t st)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_light_pick_at, dim3(blocks_for(n, 256)), dim3(256), 0, st, S.pick, S.num_lights, seed, d_pix, d_k, depth, d_p, d_pn, n, d_light, d_pdf);
}
void launch_fold_samples(const double* d_rad, const int32_t* d_pixels, const PrimaryHit* d_hits, int first_slot, int n_slots, int spp,
                         double* d_img, const DEnv& env, const double* d_dirs, hipStream_t st)
{
    if (n_slots <= 0) return;
    if (env_on(env)) hipLaunchKernelGGL(k_fold_samples<true>, dim3(blocks_for((long long)n_slots * 3, 256)), dim3(256), 0, st, d_rad, d_pixels, d_hits, first_slot, n_slots, spp, d_img, env, d_dirs);
    else hipLaunchKernelGGL(k_fold_samples<false>, dim3(blocks_for((long long)n_slots * 3, 256)), dim3(256), 0, st, d_rad, d_pixels, d_hits, first_slot, n_slots, spp, d_img, env, d_dirs);
}

void launch_fold_progressive(const double* d_rad, const int32_t* d_pixels, const PrimaryHit* d_hits, int first_slot, int n_slots, int n, int k0, int N,
                             double* d_img, double* d_mom, uint8_t* d_hit, const DEnv& env, const double* d_dirs, hipStream_t st)
{
    if (n_slots <= 0) return;
    if (env_on(env))
        hipLaunchKernelGGL(k_fold_progressive<true>, dim3(blocks_for((long long)n_slots * 3, 256)), dim3(256), 0, st, d_rad, d_pixels, d_hits, first_slot, n_slots, n,
                           k0, N, d_img, d_mom, d_hit, env, d_dirs);
    else
        hipLaunchKernelGGL(k_fold_progressive<false>, dim3(blocks_for((long long)n_slots * 3, 256)), dim3(256), 0, st, d_rad, d_pixels, d_hits, first_slot, n_slots, n,
                           k0, N, d_img, d_mom, d_hit, env, d_dirs);
}
int noise_ranges(long long n_pixels) { return (int)std::min<long long>(kNoiseRanges, std::max<long long>(1, (n_pixels + 255) / 256)); }
void launch_noise_reduce(const int32_t* d_pixels, long long n_pixels, const double* d_mom, const uint8_t* d_hit, int done, const int32_t* d_cnt,
                         double* d_partials, double* d_out, hipStream_t st)
{
    const int ranges = noise_ranges(n_pixels);
    const long long per_range = (n_pixels + ranges - 1) / ranges;
    if (d_cnt) hipLaunchKernelGGL(k_noise_reduce<true>, dim3(ranges), dim3(256), 0, st, d_pixels, n_pixels, per_range, d_mom, d_hit, done, d_cnt, d_partials);
    else hipLaunchKernelGGL(k_noise_reduce<false>, dim3(ranges), dim3(256), 0, st, d_pixels, n_pixels, per_range, d_mom, d_hit, done, d_cnt, d_partials);
    hipLaunchKernelGGL(k_noise_final, dim3(1), dim3(256), 0, st, d_partials, ranges, d_out);
}
void launch_progressive_image(const int32_t* d_pixels, long long n_pixels, const double* d_img, const double* d_mom, int done, const int32_t* d_cnt,
                              int N, double* d_est, double* d_err, const uint8_t* d_missed_hit, hipStream_t st)
{
    if (n_pixels <= 0) return;
    const dim3 grid(blocks_for(n_pixels * 3, 256));
    if (d_cnt) hipLaunchKernelGGL(k_progressive_image<true>, grid, dim3(256), 0, st, d_pixels, n_pixels, d_img, d_mom, done, d_cnt, N, d_est, d_err);
    else hipLaunchKernelGGL(k_progressive_image<false>, grid, dim3(256), 0, st, d_pixels, n_pixels, d_img, d_mom, done, d_cnt, N, d_est, d_err);
    if (d_missed_hit && d_est) hipLaunchKernelGGL(k_missed_image, grid, dim3(256), 0, st, d_pixels, n_pixels, d_missed_hit, d_img, d_est);
}
int adaptive_blocks(int n) { return (n + 255) / 256; }
void launch_adaptive_select(const int32_t* d_list, int n, const double* d_mom, const uint8_t* d_hit, int k, int min_spp, double rel2, double abs2,
                            int32_t* d_cnt, unsigned long long* d_masks, int32_t* d_block_counts, int32_t* d_block_offsets, int32_t* d_total,
                            int32_t* d_out, hipStream_t st)
{
    const int blocks = adaptive_blocks(n);
    if (blocks == 0) { (void)hipMemsetAsync(d_total, 0, sizeof(int32_t), st); return; }
    hipLaunchKernelGGL(k_adaptive_select, dim3(blocks), dim3(256), 0, st, d_list, n, d_mom, d_hit, k, min_spp, rel2, abs2, d_cnt, d_masks, d_block_counts);
    hipLaunchKernelGGL(k_adaptive_scan, dim3(1), dim3(256), 0, st, d_block_counts, blocks, d_block_offsets, d_total);
    hipLaunchKernelGGL(k_adaptive_scatter, dim3(blocks), dim3(256), 0, st, d_list, n, d_masks, d_block_offsets, d_out);
}

}  // namespace mcpt
