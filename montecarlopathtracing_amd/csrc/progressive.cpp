// C ABI, progressive frames (include/mcpt.h: mcpt_progressive_*): a frame of N samples per pixel in passes, its noise estimate, adaptive
// frames that stop each pixel on its own error, first-hit AOVs, sample AOVs, the denoiser in both its forms and the frame's picture.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "denoise.hpp"
#include "handles.hpp"

using namespace mcpt;

// a device buffer of at least 8 bytes, unless b holds one already; alloc_zeroed: cleared as well
template <class T>
static hipError_t alloc_once(DevBuf<T>& b, size_t bytes) { return b ? hipSuccess : b.alloc_bytes(std::max<size_t>(bytes, 8)); }
template <class T>
static hipError_t alloc_zeroed(DevBuf<T>& b, size_t bytes)
{
    const hipError_t e = alloc_once(b, bytes);
    return e == hipSuccess ? hipMemset(b.get(), 0, std::max<size_t>(bytes, 8)) : e;
}

// ------------------------------------------------------------------------------------------------ progressive frames
// A frame of N samples per pixel rendered in passes of consecutive sample ranges.  Every (pixel, sample) owns its RNG key, so a pass
// of samples [k0, k1) computes the same radiance as the one-shot frame does for them, and k_fold_progressive continues the frame's float
// fold where the last pass left it: at done == N the image is mcpt_render's frame bit for bit.
struct mcpt_progressive {
    mcpt_device* d = nullptr;          // holds a reference (mcpt_device::refs)
    mcpt_render_params p{};            // p.spp = N
    int done = 0;
    bool broken = false;               // a step failed half-way: the image and the moments hold part of a pass
    DevBuf<int32_t> pixels; int64_t n_pixels = 0;      // the owned pixels of (rank, world)
    DevBuf<double> img;                // W*H*3: the float fold of samples [0, done) (pixels not owned stay 0)
    DevBuf<double> mom;                // W*H*2*3: sum x, sum x*x per channel
    DevBuf<uint8_t> hit;               // W*H: the pixel's primary ray hit
    DevBuf<double> partials;           // noise_ranges() x 3
    DevBuf<double> sums;               // 4 doubles: sum se2, sum mean^2, hit pixels, 0
    HostBuf<double> h_sums;            // pinned copy of sums (the pass's one 32-byte read-back)
    std::vector<int32_t> owned;        // host copy of `pixels`
    // adaptive frames (mcpt_progressive_create_adaptive): the active list, double-buffered -- a pass renders active[cur][0..n_active) and
    // the selection writes the pixels that continue to active[cur ^ 1]
    bool adaptive = false;
    double rel2 = 0.0, abs2 = 0.0;     // rel_target^2, abs_target^2
    int min_spp = 0;
    DevBuf<int32_t> active[2];
    int cur = 0;
    int64_t n_active = 0;
    DevBuf<int32_t> cnt;               // W*H: the samples each pixel holds (written for the listed pixels after every pass)
    DevBuf<unsigned long long> masks;  // 4 * adaptive_blocks(n_pixels): the keep ballots of the selection
    DevBuf<int32_t> block_counts, block_offsets;   // adaptive_blocks(n_pixels) each
    DevBuf<int32_t> total;             // the next list's length
    HostBuf<int32_t> h_total;          // pinned copy of total (the pass's 4-byte read-back)
    // first-hit AOVs (W*H[*3], owned pixels written; computed on the first mcpt_progressive_aovs / _denoise call: they do not depend on
    // the samples) and the guide record the denoiser's taps read
    bool aov_ready = false;
    DevBuf<int32_t> aov_mat; DevBuf<double> aov_depth, aov_normal, aov_albedo;
    DevBuf<DenoiseGuide> guide;
    DevBuf<DenoisePix> dn_buf[2];      // the denoiser's ping-pong buffers (W*H each), allocated on its first call
    mcpt_lens lens{};                  // the device's lens when the handle was created
    std::shared_ptr<const EnvData> env;   // ... and its environment (null: none)
    DevBuf<int32_t> hitcnt;            // W*H, under an active lens: the samples so far whose camera ray hit (hit = hitcnt > 0)
    // sample AOVs (mcpt_progressive_sample_aovs: W*H[*3], owned pixels written) of guide_G camera samples per pixel (0: none yet) and the
    // guide record mcpt_progressive_denoise_guided's taps read; made again when a call asks for another G
    int guide_G = 0;
    DevBuf<int32_t> saov_counts; DevBuf<double> saov_depth, saov_normal, saov_albedo;
    DevBuf<SampleGuide> sguide;
    bool motion = false;               // created on a device with a motion (which stays while the handle lives): passes are cut at its steps
    DevBuf<double> disp_frame;         // W*H*3: the frame mcpt_progressive_display maps (allocated on its first call)
};

extern "C" {

void mcpt_progressive_free(mcpt_progressive* h)
{
    if (!h) return;
    (void)hipSetDevice(h->d->ordinal);
    (void)hipStreamSynchronize(h->d->stream.get());
    mcpt_device* d = h->d;
    delete h;                          // its buffers go before the device reference
    mcpt_device_free(d);
}

// ap == null: a uniform frame; otherwise an adaptive one (arguments checked by the caller)
static int progressive_create(mcpt_device* d, const mcpt_render_params* p, const mcpt_adaptive_params* ap, mcpt_progressive** out)
{
    if (p->flags & (MCPT_RENDER_PIPELINE | MCPT_RENDER_KEEP_STATS))
        return fail(MCPT_ERR_ARG, "a progressive frame takes neither MCPT_RENDER_PIPELINE nor MCPT_RENDER_KEEP_STATS");
    if (const int rc = geometry_gate(d)) return rc;
    if (d->motion && ap) return fail(MCPT_ERR_ARG, "the device holds a motion: adaptive frames under a motion are not supported");
    if (d->motion && d->motion->shutter.steps > p->spp) return fail(MCPT_ERR_ARG, "the shutter has more steps than the frame has samples per pixel");
    std::vector<int32_t> v;
    if (const int rc = owned_pixels(d->width, d->height, p, v)) return rc;
    HIP_TRY(hipSetDevice(d->ordinal));
    const size_t px = size_t(d->width) * d->height;
    std::unique_ptr<mcpt_progressive, void (*)(mcpt_progressive*)> h(new mcpt_progressive, mcpt_progressive_free);
    h->d = d; d->refs.fetch_add(1);
    h->p = *p;
    h->lens = d->lens;
    h->env = d->env;
    h->motion = d->motion != nullptr;
    h->n_pixels = int64_t(v.size());
    HIP_TRY(h->pixels.upload(v));
    HIP_TRY(alloc_zeroed(h->img, px * 3 * sizeof(double)));
    HIP_TRY(alloc_zeroed(h->mom, px * 6 * sizeof(double)));
    HIP_TRY(alloc_zeroed(h->hit, px));
    if (lens_active(h->lens)) HIP_TRY(alloc_zeroed(h->hitcnt, px * sizeof(int32_t)));
    HIP_TRY(alloc_zeroed(h->partials, size_t(kNoiseRanges) * 3 * sizeof(double)));
    HIP_TRY(alloc_zeroed(h->sums, 4 * sizeof(double)));
    HIP_TRY(h->h_sums.alloc(4));
    if (ap) {
        const size_t blocks = size_t(adaptive_blocks(int(v.size())));
        HIP_TRY(alloc_zeroed(h->active[0], v.size() * sizeof(int32_t)));
        HIP_TRY(alloc_zeroed(h->active[1], v.size() * sizeof(int32_t)));
        HIP_TRY(alloc_zeroed(h->cnt, px * sizeof(int32_t)));
        HIP_TRY(alloc_zeroed(h->masks, blocks * 4 * sizeof(unsigned long long)));
        HIP_TRY(alloc_zeroed(h->block_counts, blocks * sizeof(int32_t)));
        HIP_TRY(alloc_zeroed(h->block_offsets, blocks * sizeof(int32_t)));
        HIP_TRY(alloc_zeroed(h->total, sizeof(int32_t)));
        HIP_TRY(h->h_total.alloc(1));
        if (!v.empty()) HIP_TRY(hipMemcpy(h->active[0].get(), h->pixels.get(), v.size() * sizeof(int32_t), hipMemcpyDeviceToDevice));
        h->adaptive = true;
        h->rel2 = ap->rel_target * ap->rel_target;
        h->abs2 = ap->abs_target * ap->abs_target;
        h->min_spp = std::min(ap->min_spp, p->spp);
        h->n_active = h->n_pixels;
    }
    h->owned = std::move(v);
    *out = h.release();
    return MCPT_OK;
}

int mcpt_progressive_create(mcpt_device* d, const mcpt_render_params* p, mcpt_progressive** out)
{
    if (!out || !p) return fail(MCPT_ERR_ARG, "null argument");
    *out = nullptr;
    if (const int rc = require_device()) return rc;
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    if (p->spp <= 0) return fail(MCPT_ERR_ARG, "spp must be positive");
    return progressive_create(d, p, nullptr, out);
}

int mcpt_progressive_create_adaptive(mcpt_device* d, const mcpt_render_params* p, const mcpt_adaptive_params* ap, mcpt_progressive** out)
{
    if (!out || !p || !ap) return fail(MCPT_ERR_ARG, "null argument");
    *out = nullptr;
    if (!(std::isfinite(ap->rel_target) && ap->rel_target >= 0.0 && std::isfinite(ap->abs_target) && ap->abs_target >= 0.0))
        return fail(MCPT_ERR_ARG, "rel_target and abs_target must be finite and >= 0");
    if (ap->min_spp < 2) return fail(MCPT_ERR_ARG, "min_spp must be >= 2 (a standard error needs two samples)");
    if (p->spp <= 0) return fail(MCPT_ERR_ARG, "spp must be positive");
    if (const int rc = require_device()) return rc;
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    return progressive_create(d, p, ap, out);
}

int mcpt_progressive_step(mcpt_progressive* h, int32_t n, mcpt_stats* stats)
{
    if (!h || n <= 0) return fail(MCPT_ERR_ARG, "bad argument");
    if (h->done >= h->p.spp) return fail(MCPT_ERR_ARG, "the progressive frame is complete");
    if (h->broken) return fail(MCPT_ERR_ARG, "an earlier step of this progressive frame failed");
    if (h->adaptive && h->n_active == 0) return fail(MCPT_ERR_ARG, "the adaptive frame is complete: no pixel is active");
    mcpt_device* d = h->d;
    HIP_TRY(hipSetDevice(d->ordinal));
    if (stats) std::memset(stats, 0, sizeof *stats);
    mcpt_render_params q = h->p;
    q.spp = std::min(n, h->p.spp - h->done);
    const PixelList L = h->adaptive ? PixelList{h->active[h->cur].get(), h->n_active} : PixelList{h->pixels.get(), h->n_pixels};
    const size_t ev_used0 = d->ev_used;
    int slot_used = -1;
    // one sample range on the device's geometry and camera -- or, under a motion, one per step of the shutter the pass touches
    const auto pass = [&](int k0, int n, mcpt_stats* out) {
        mcpt_render_params piece = q;
        piece.spp = n;
        const SampleRange r{k0, n, h->p.spp, h->mom.get(), h->hit.get(), &h->lens, h->hitcnt.get(), h->env.get(), h->motion};
        return render_device_impl(d, r, L, &piece, h->img.get(), out, d->stream.get(), slot_used);
    };
    int rc;
    if (h->motion)
        rc = motion_passes(d, h->done, q.spp, h->p.spp, d->stream.get(), [&](int k0, int n) {
            mcpt_stats piece{};
            const int prc = pass(k0, n, stats ? &piece : nullptr);
            if (prc == MCPT_OK && stats) add_piece(*stats, piece);
            return prc;
        });
    else rc = pass(h->done, q.spp, stats);
    if (rc == MCPT_OK && h->adaptive) {
        // which pixels continue: decided on the device; the host reads back the new list's length only
        launch_adaptive_select(L.pixels, int(L.n), h->mom.get(), h->hit.get(), h->done + q.spp, h->min_spp, h->rel2, h->abs2, h->cnt.get(), h->masks.get(),
                               h->block_counts.get(), h->block_offsets.get(), h->total.get(), h->active[h->cur ^ 1].get(), d->stream.get());
        hipError_t le = hipGetLastError();
        if (le == hipSuccess) le = hipMemcpyAsync(h->h_total.get(), h->total.get(), sizeof(int32_t), hipMemcpyDeviceToHost, d->stream.get());
        if (le != hipSuccess) rc = fail(MCPT_ERR_HIP, hipGetErrorString(le));
    }
    const hipError_t e = hipStreamSynchronize(d->stream.get());
    if (rc == MCPT_OK && e != hipSuccess) rc = fail(MCPT_ERR_HIP, hipGetErrorString(e));
    if (rc != MCPT_OK) { d->ev_used = ev_used0; h->broken = true; return rc; }
    h->done += q.spp;
    if (h->adaptive) { h->n_active = h->h_total[0]; h->cur ^= 1; }
    return MCPT_OK;
}

int64_t mcpt_progressive_active(const mcpt_progressive* h)
{
    if (!h) return fail(MCPT_ERR_ARG, "null handle");
    if (h->done >= h->p.spp) return 0;
    return h->adaptive ? h->n_active : h->n_pixels;
}

int64_t mcpt_progressive_active_pixels(mcpt_progressive* h, int32_t* pixels)
{
    const int64_t n = mcpt_progressive_active(h);
    if (n <= 0 || !pixels) return n;
    if (!h->adaptive) { std::memcpy(pixels, h->owned.data(), size_t(n) * sizeof(int32_t)); return n; }
    HIP_TRY(hipSetDevice(h->d->ordinal));
    HIP_TRY(hipMemcpy(pixels, h->active[h->cur].get(), size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost));
    return n;
}

int mcpt_progressive_sample_counts(mcpt_progressive* h, int32_t* counts)
{
    if (!h || !counts) return fail(MCPT_ERR_ARG, "null argument");
    if (!h->adaptive) {
        for (int32_t pix : h->owned) counts[pix] = h->done;
        return MCPT_OK;
    }
    HIP_TRY(hipSetDevice(h->d->ordinal));
    std::vector<int32_t> all(size_t(h->d->width) * h->d->height);
    HIP_TRY(hipMemcpy(all.data(), h->cnt.get(), all.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int32_t pix : h->owned) counts[pix] = all[size_t(pix)];
    return MCPT_OK;
}

int mcpt_progressive_done(const mcpt_progressive* h) { return h ? h->done : fail(MCPT_ERR_ARG, "null handle"); }

int mcpt_progressive_noise(mcpt_progressive* h, mcpt_noise* o)
{
    if (!h || !o) return fail(MCPT_ERR_ARG, "null argument");
    std::memset(o, 0, sizeof *o);
    o->done = h->done; o->spp = h->p.spp;
    if (h->done < 2) { o->rel_error = o->abs_rms = INFINITY; return MCPT_OK; }     // no variance estimate from fewer than two samples
    HIP_TRY(hipSetDevice(h->d->ordinal));
    hipStream_t st = h->d->stream.get();
    launch_noise_reduce(h->pixels.get(), h->n_pixels, h->mom.get(), h->hit.get(), h->done, h->cnt.get(), h->partials.get(), h->sums.get(), st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->h_sums.get(), h->sums.get(), 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    o->sum_se2 = h->h_sums[0]; o->sum_mean2 = h->h_sums[1]; o->pixels = int64_t(h->h_sums[2]);
    o->rel_error = o->sum_mean2 > 0 ? std::sqrt(o->sum_se2 / o->sum_mean2) : (o->sum_se2 > 0 ? INFINITY : 0.0);
    o->abs_rms = o->pixels > 0 ? std::sqrt(o->sum_se2 / (3.0 * double(o->pixels))) : 0.0;
    return MCPT_OK;
}

int mcpt_progressive_image_device(mcpt_progressive* h, double* d_img, double* d_stderr, void* stream)
{
    if (!h || (!d_img && !d_stderr)) return fail(MCPT_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(h->d->ordinal));
    // (the per-pixel route under an environment: a missed pixel's image already is the frame's fold of Le)
    // (... unless the handle renders a motion: its missed pixels see another sky in every step and show their mean like any other)
    const bool sky = h->env && env_on(h->env->denv) && !lens_active(h->lens) && !h->motion;
    launch_progressive_image(h->pixels.get(), h->n_pixels, h->img.get(), h->mom.get(), h->done, h->cnt.get(), h->p.spp, d_img, d_stderr,
                             sky ? h->hit.get() : nullptr, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return MCPT_OK;
}

int mcpt_progressive_image(mcpt_progressive* h, double* img, double* stderr_img)
{
    if (!h || (!img && !stderr_img)) return fail(MCPT_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(h->d->ordinal));
    // pixels this rank does not own keep the caller's values
    Staging S(h->d->stream.get());
    const size_t words = size_t(h->d->width) * h->d->height * 3;
    double *d_est = nullptr, *d_err = nullptr;
    if (const int rc = S.inout(img, words, "the image", d_est)) return rc;
    if (const int rc = S.inout(stderr_img, words, "the standard errors", d_err)) return rc;
    return S.finish(mcpt_progressive_image_device(h, d_est, d_err, h->d->stream.get()));
}

// First-hit AOVs of the owned pixels: the primary hits of the owned list traced again on the device's stream and closest-hit workspace
// (launch_primary_hits, as a render call traces them), then k_primary_aov.  Once per handle.
static int ensure_aovs(mcpt_progressive* h)
{
    if (h->aov_ready) return MCPT_OK;
    mcpt_device* d = h->d;
    hipStream_t st = d->stream.get();
    int rc = ensure_dirs(d, st);
    if (rc) return rc;
    const size_t px = size_t(d->width) * d->height;
    DevBuf<PrimaryHit> hits;
    hipError_t e = alloc_once(hits, size_t(h->n_pixels) * sizeof(PrimaryHit));
    if (e == hipSuccess) e = alloc_once(h->aov_mat, px * sizeof(int32_t));
    if (e == hipSuccess) e = alloc_once(h->aov_depth, px * sizeof(double));
    if (e == hipSuccess) e = alloc_once(h->aov_normal, px * 3 * sizeof(double));
    if (e == hipSuccess) e = alloc_once(h->aov_albedo, px * 3 * sizeof(double));
    if (e == hipSuccess) e = alloc_once(h->guide, px * sizeof(DenoiseGuide));
    // pixels not owned: material -1 everywhere in the guide (all bits set), so that no tap reads them
    if (e == hipSuccess) e = hipMemsetAsync(h->guide.get(), 0xff, px * sizeof(DenoiseGuide), st);
    if (e == hipSuccess) {
        launch_primary_hits(d->ds, d->trace_mode == MCPT_TRACE_FAST, d->dirs.get(), h->pixels.get(), int(h->n_pixels), hits.get(), d->aux_ctr.get(), d->aux_queue.get(),
                            d->aux_slow_list.get(), d->slow_cap, st, d->cfg);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        launch_primary_aov(d->ds, h->pixels.get(), int(h->n_pixels), hits.get(), h->aov_mat.get(), h->aov_depth.get(), h->aov_normal.get(), h->aov_albedo.get(), h->guide.get(), st);
        e = hipGetLastError();
    }
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(MCPT_ERR_HIP, std::string("first-hit AOVs: ") + hipGetErrorString(e));
    h->aov_ready = true;
    return MCPT_OK;
}

int mcpt_progressive_aovs(mcpt_progressive* h, int32_t* material, double* depth, double* normal, double* albedo)
{
    if (!h) return fail(MCPT_ERR_ARG, "null handle");
    if (h->motion) return fail(MCPT_ERR_ARG, "the frame renders a motion: first-hit AOVs under a motion are not supported");
    HIP_TRY(hipSetDevice(h->d->ordinal));
    int rc = ensure_aovs(h);
    if (rc) return rc;
    const size_t px = size_t(h->d->width) * h->d->height;
    // the device arrays whole, then the owned pixels into the caller's (pixels not owned keep the caller's values)
    auto fetch = [&](const void* src, void* dst, size_t per_pixel) -> int {
        if (!dst) return MCPT_OK;
        std::vector<uint8_t> all(px * per_pixel);
        HIP_TRY(hipMemcpy(all.data(), src, all.size(), hipMemcpyDeviceToHost));
        for (int32_t pix : h->owned) std::memcpy(static_cast<uint8_t*>(dst) + size_t(pix) * per_pixel, all.data() + size_t(pix) * per_pixel, per_pixel);
        return MCPT_OK;
    };
    if ((rc = fetch(h->aov_mat.get(), material, sizeof(int32_t)))) return rc;
    if ((rc = fetch(h->aov_depth.get(), depth, sizeof(double)))) return rc;
    if ((rc = fetch(h->aov_normal.get(), normal, 3 * sizeof(double)))) return rc;
    return fetch(h->aov_albedo.get(), albedo, 3 * sizeof(double));
}

static int denoise_args(const mcpt_progressive* h, const mcpt_denoise_params* dp, int& iterations, double& sigma_l, double& sigma_z)
{
    if (!h) return fail(MCPT_ERR_ARG, "null handle");
    if (h->motion) return fail(MCPT_ERR_ARG, "the frame renders a motion: denoising under a motion is not supported");
    const mcpt_denoise_params z{};
    const mcpt_denoise_params& q = dp ? *dp : z;
    if (q.reserved != 0) return fail(MCPT_ERR_ARG, "mcpt_denoise_params.reserved must be 0");
    if (q.iterations < 0 || q.iterations > MCPT_DENOISE_MAX_ITERATIONS) return fail(MCPT_ERR_ARG, "denoise iterations outside 0..10");
    if (!(std::isfinite(q.sigma_l) && q.sigma_l >= 0.0 && std::isfinite(q.sigma_z) && q.sigma_z >= 0.0))
        return fail(MCPT_ERR_ARG, "denoise sigmas must be finite and >= 0 (0: the default)");
    if (h->done < 2) return fail(MCPT_ERR_ARG, "denoising needs a variance estimate: at least two samples done");
    const bool defaults = q.iterations == 0 && q.sigma_l == 0.0 && q.sigma_z == 0.0;     // a zero struct: the defaults
    iterations = defaults ? MCPT_DENOISE_ITERATIONS : q.iterations;
    sigma_l = q.sigma_l > 0.0 ? q.sigma_l : MCPT_DENOISE_SIGMA_L;
    sigma_z = q.sigma_z > 0.0 ? q.sigma_z : MCPT_DENOISE_SIGMA_Z;
    return MCPT_OK;
}

int mcpt_progressive_denoise_device(mcpt_progressive* h, const mcpt_denoise_params* dp, double* d_img, void* stream)
{
    int iterations = 0;
    double sigma_l = 0.0, sigma_z = 0.0;
    int rc = denoise_args(h, dp, iterations, sigma_l, sigma_z);
    if (rc) return rc;
    if (!d_img) return fail(MCPT_ERR_ARG, "null image");
    HIP_TRY(hipSetDevice(h->d->ordinal));
    if ((rc = ensure_aovs(h))) return rc;
    const size_t px = size_t(h->d->width) * h->d->height;
    for (auto& b : h->dn_buf)
        if (!b) HIP_TRY(b.alloc(px));
    launch_denoise(h->pixels.get(), h->n_pixels, h->d->width, h->d->height, h->img.get(), h->mom.get(), h->done, h->cnt.get(), h->p.spp, h->aov_albedo.get(), h->guide.get(),
                   iterations, sigma_l, sigma_z, h->dn_buf[0].get(), h->dn_buf[1].get(), d_img, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return MCPT_OK;
}

int mcpt_progressive_denoise(mcpt_progressive* h, const mcpt_denoise_params* dp, double* img)
{
    int iterations = 0;
    double sigma_l = 0.0, sigma_z = 0.0;
    int rc = denoise_args(h, dp, iterations, sigma_l, sigma_z);
    if (rc) return rc;
    if (!img) return fail(MCPT_ERR_ARG, "null image");
    HIP_TRY(hipSetDevice(h->d->ordinal));
    // pixels this rank does not own keep the caller's values
    Staging S(h->d->stream.get());
    double* d_out = nullptr;
    if ((rc = S.inout(img, size_t(h->d->width) * h->d->height * 3, "the image", d_out))) return rc;
    return S.finish(mcpt_progressive_denoise_device(h, dp, d_out, h->d->stream.get()));
}

// ---- sample AOVs and the filter they guide (mcpt.h: mcpt_progressive_sample_aovs, mcpt_progressive_denoise_guided)
static constexpr long long kGuideChunkRays = 1ll << 20;

// samples: the caller's G (0: the default) -> G, or MCPT_ERR_ARG
static int guide_samples(const mcpt_progressive* h, int32_t samples, int& G)
{
    if (samples < 0 || samples > h->p.spp) return fail(MCPT_ERR_ARG, "guide samples outside 0..spp");
    G = samples > 0 ? samples : std::min<int>(h->p.spp, MCPT_GUIDE_SAMPLES);
    return MCPT_OK;
}

// The sample AOVs of G camera samples per owned pixel, in chunks of whole pixels of at most 2^20 rays: the frame's own camera rays
// (launch_guide_rays), their closest hits on the device's stream and closest-hit workspace, the fold.  Kept per G.
static int ensure_sample_aovs(mcpt_progressive* h, int G)
{
    if (h->guide_G == G) return MCPT_OK;
    mcpt_device* d = h->d;
    hipStream_t st = d->stream.get();
    if (const int rc = ensure_pos(d, st)) return rc;
    const size_t px = size_t(d->width) * d->height;
    const int per_chunk = int(std::max<long long>(1, std::min<long long>(kGuideChunkRays / G, std::max<int64_t>(h->n_pixels, 1))));
    const size_t rays = size_t(per_chunk) * size_t(G);
    h->guide_G = 0;                                   // what the buffers hold is overwritten from here on
    DevBuf<double> rays6, t, p;
    DevBuf<int32_t> leaf;
    hipError_t e = alloc_once(rays6, rays * 6 * sizeof(double));
    if (e == hipSuccess) e = alloc_once(t, rays * sizeof(double));
    if (e == hipSuccess) e = alloc_once(p, rays * 3 * sizeof(double));
    if (e == hipSuccess) e = alloc_once(leaf, rays * sizeof(int32_t));
    if (e == hipSuccess) e = alloc_once(h->saov_counts, px * 3 * sizeof(int32_t));
    if (e == hipSuccess) e = alloc_once(h->saov_depth, px * sizeof(double));
    if (e == hipSuccess) e = alloc_once(h->saov_normal, px * 3 * sizeof(double));
    if (e == hipSuccess) e = alloc_once(h->saov_albedo, px * 3 * sizeof(double));
    if (e == hipSuccess) e = alloc_once(h->sguide, px * sizeof(SampleGuide));
    // pixels not owned: filtered == 0 in the guide, so that no tap reads them
    if (e == hipSuccess) e = hipMemsetAsync(h->sguide.get(), 0, px * sizeof(SampleGuide), st);
    const DLens lens = lens_for(d, h->lens);
    for (int64_t first = 0; first < h->n_pixels && e == hipSuccess; first += per_chunk) {
        const int n = int(std::min<int64_t>(per_chunk, h->n_pixels - first));
        launch_guide_rays(lens, h->p.seed, h->pixels.get(), int(first), n, G, rays6.get(), st);
        trace_leaf(d, rays6.get(), (long long)n * G, leaf.get(), t.get(), p.get(), st);
        launch_guide_fold(d->ds, h->pixels.get(), int(first), n, G, leaf.get(), t.get(), p.get(), h->saov_counts.get(), h->saov_depth.get(),
                          h->saov_normal.get(), h->saov_albedo.get(), h->sguide.get(), st);
        e = hipGetLastError();
    }
    const hipError_t es = hipStreamSynchronize(st);   // the chunk buffers go with this call
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(MCPT_ERR_HIP, std::string("sample AOVs: ") + hipGetErrorString(e));
    h->guide_G = G;
    return MCPT_OK;
}

int mcpt_progressive_sample_aovs(mcpt_progressive* h, int32_t samples, int32_t* counts3, double* depth, double* normal, double* albedo)
{
    if (!h) return fail(MCPT_ERR_ARG, "null handle");
    if (h->motion) return fail(MCPT_ERR_ARG, "the frame renders a motion: sample AOVs under a motion are not supported");
    int G = 0;
    int rc = guide_samples(h, samples, G);
    if (rc) return rc;
    if ((rc = geometry_gate(h->d))) return rc;
    HIP_TRY(hipSetDevice(h->d->ordinal));
    if ((rc = ensure_sample_aovs(h, G))) return rc;
    const size_t px = size_t(h->d->width) * h->d->height;
    // the device arrays whole, then the owned pixels into the caller's (pixels not owned keep the caller's values)
    auto fetch = [&](const void* src, void* dst, size_t per_pixel) -> int {
        if (!dst) return MCPT_OK;
        std::vector<uint8_t> all(px * per_pixel);
        HIP_TRY(hipMemcpy(all.data(), src, all.size(), hipMemcpyDeviceToHost));
        for (int32_t pix : h->owned) std::memcpy(static_cast<uint8_t*>(dst) + size_t(pix) * per_pixel, all.data() + size_t(pix) * per_pixel, per_pixel);
        return MCPT_OK;
    };
    if ((rc = fetch(h->saov_counts.get(), counts3, 3 * sizeof(int32_t)))) return rc;
    if ((rc = fetch(h->saov_depth.get(), depth, sizeof(double)))) return rc;
    if ((rc = fetch(h->saov_normal.get(), normal, 3 * sizeof(double)))) return rc;
    return fetch(h->saov_albedo.get(), albedo, 3 * sizeof(double));
}

static int guided_args(const mcpt_progressive* h, const mcpt_denoise_params* dp, const mcpt_guide_params* gp, int& iterations, double& sigma_l,
                       double& sigma_z, int& G, double& sigma_a)
{
    if (!h) return fail(MCPT_ERR_ARG, "null handle");
    const mcpt_guide_params z{};
    const mcpt_guide_params& q = gp ? *gp : z;
    if (q.reserved != 0) return fail(MCPT_ERR_ARG, "mcpt_guide_params.reserved must be 0");
    if (!(std::isfinite(q.sigma_a) && q.sigma_a >= 0.0)) return fail(MCPT_ERR_ARG, "sigma_a must be finite and >= 0 (0: the default)");
    if (const int rc = guide_samples(h, q.samples, G)) return rc;
    sigma_a = q.sigma_a > 0.0 ? q.sigma_a : MCPT_DENOISE_SIGMA_A;
    return denoise_args(h, dp, iterations, sigma_l, sigma_z);
}

int mcpt_progressive_denoise_guided_device(mcpt_progressive* h, const mcpt_denoise_params* dp, const mcpt_guide_params* gp, double* d_img, void* stream)
{
    int iterations = 0, G = 0;
    double sigma_l = 0.0, sigma_z = 0.0, sigma_a = 0.0;
    int rc = guided_args(h, dp, gp, iterations, sigma_l, sigma_z, G, sigma_a);
    if (rc) return rc;
    if (!d_img) return fail(MCPT_ERR_ARG, "null image");
    if ((rc = geometry_gate(h->d))) return rc;
    HIP_TRY(hipSetDevice(h->d->ordinal));
    if ((rc = ensure_sample_aovs(h, G))) return rc;
    const size_t px = size_t(h->d->width) * h->d->height;
    for (auto& b : h->dn_buf)
        if (!b) HIP_TRY(b.alloc(px));
    launch_denoise_guided(h->pixels.get(), h->n_pixels, h->d->width, h->d->height, h->img.get(), h->mom.get(), h->done, h->cnt.get(), h->p.spp, h->sguide.get(),
                          iterations, sigma_l, sigma_z, sigma_a, h->dn_buf[0].get(), h->dn_buf[1].get(), d_img, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return MCPT_OK;
}

int mcpt_progressive_denoise_guided(mcpt_progressive* h, const mcpt_denoise_params* dp, const mcpt_guide_params* gp, double* img)
{
    int iterations = 0, G = 0;
    double sigma_l = 0.0, sigma_z = 0.0, sigma_a = 0.0;
    int rc = guided_args(h, dp, gp, iterations, sigma_l, sigma_z, G, sigma_a);
    if (rc) return rc;
    if (!img) return fail(MCPT_ERR_ARG, "null image");
    HIP_TRY(hipSetDevice(h->d->ordinal));
    // pixels this rank does not own keep the caller's values
    Staging S(h->d->stream.get());
    double* d_out = nullptr;
    if ((rc = S.inout(img, size_t(h->d->width) * h->d->height * 3, "the image", d_out))) return rc;
    return S.finish(mcpt_progressive_denoise_guided_device(h, dp, gp, d_out, h->d->stream.get()));
}

// ---- the picture of the frame (mcpt.h: display transform): the source frame into the handle's scratch, then histogram and map over the
// owned pixels -- the whole frame when the handle owns all of it
int mcpt_progressive_display_device(mcpt_progressive* h, int32_t source, const mcpt_display_params* p, uint8_t* d_rgb8, mcpt_display_info* info,
                                    void* stream)
{
    if (const int rc = display_check(p)) return rc;
    if (!h || !d_rgb8) return fail(MCPT_ERR_ARG, "null argument");
    if (source != MCPT_DISPLAY_ESTIMATE && source != MCPT_DISPLAY_DENOISED && source != MCPT_DISPLAY_DENOISED_GUIDED)
        return fail(MCPT_ERR_ARG, "unknown display source");
    mcpt_device* d = h->d;
    HIP_TRY(hipSetDevice(d->ordinal));
    const size_t px = size_t(d->width) * d->height;
    if (!h->disp_frame) {
        // cleared on the caller's stream, ahead of the kernels that write it (pixels not owned are never read)
        HIP_TRY(alloc_once(h->disp_frame, px * 3 * sizeof(double)));
        HIP_TRY(hipMemsetAsync(h->disp_frame.get(), 0, px * 3 * sizeof(double), static_cast<hipStream_t>(stream)));
    }
    double* frame = h->disp_frame.get();
    int rc;
    if (source == MCPT_DISPLAY_ESTIMATE) rc = mcpt_progressive_image_device(h, frame, nullptr, stream);
    else if (source == MCPT_DISPLAY_DENOISED) rc = mcpt_progressive_denoise_device(h, nullptr, frame, stream);
    else rc = mcpt_progressive_denoise_guided_device(h, nullptr, nullptr, frame, stream);
    if (rc) return rc;
    const bool whole = h->n_pixels == int64_t(px);
    return display_frame_device(d, frame, whole ? nullptr : h->pixels.get(), h->n_pixels, p, d_rgb8, info, static_cast<hipStream_t>(stream));
}

int mcpt_progressive_display(mcpt_progressive* h, int32_t source, const mcpt_display_params* p, uint8_t* rgb8, mcpt_display_info* info)
{
    if (const int rc = display_check(p)) return rc;
    if (!h || !rgb8) return fail(MCPT_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(h->d->ordinal));
    // pixels this rank does not own keep the caller's bytes
    const size_t bytes = size_t(h->d->width) * h->d->height * ((p && (p->flags & MCPT_DISPLAY_RGBA)) ? 4 : 3);
    Staging S(h->d->stream.get());
    uint8_t* d_out = nullptr;
    if (const int rc = S.inout(rgb8, bytes, "the picture", d_out)) return rc;
    return S.finish(mcpt_progressive_display_device(h, source, p, d_out, info, h->d->stream.get()));
}

int mcpt_progressive_next_pass(int32_t spp, int32_t done, double remaining_s, double s_per_sample)
{
    if (spp <= 0 || done < 0 || done >= spp) return 0;
    if (done == 0) return std::min(spp, 8);                  // the first pass: no rate measured yet, and a frame needs one pass
    const int n = std::min(spp - done, done);               // each later pass doubles the samples done
    if (std::isinf(remaining_s) && remaining_s > 0) return n;     // no time budget
    if (!(remaining_s > 0)) return 0;                        // the budget is spent
    if (!(s_per_sample > 0)) return n;                        // no rate to go by
    const double cap = std::floor(remaining_s / s_per_sample);
    return cap < 1.0 ? 0 : int(std::min<double>(n, cap));
}

}  // extern "C"
