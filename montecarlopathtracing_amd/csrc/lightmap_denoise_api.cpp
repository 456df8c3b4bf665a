// C ABI, the lightmap denoiser (include/mcpt.h: mcpt_lightmap_denoise*): the chart is rasterised as a bake rasterises it (lightmap.hip,
// unchanged), every covered texel gets its guides, the irradiance map goes through the a-trous iterations (lightmap_denoise.hip) and the
// result through the baker's dilation.  Everything runs map-wide on the GPU: the host never needs the number of covered texels, so the
// device form enqueues and returns.  The workspace lives in the device beside the baker's and shares its event.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <string>

#include "handles.hpp"
#include "lightmap_denoise.hpp"

using namespace mcpt;

// what both forms refuse without looking at the device or the chart, in mcpt.h's order
static int params_check(const mcpt_lightmap_denoise_params* p, const void* irradiance3, const void* stderr3, const void* out3)
{
    if (!p) return fail(MCPT_ERR_ARG, "null lightmap denoise parameters");
    if (const int rc = lightmap_size_check(p->width, p->height)) return rc;
    if (p->iterations < 0 || p->iterations > MCPT_LIGHTMAP_DENOISE_MAX_ITERATIONS) return fail(MCPT_ERR_ARG, "iterations must be in 0 .. 10");
    if (p->dilate < 0 || p->dilate > kLightmapMaxDilate) return fail(MCPT_ERR_ARG, "dilate must be in 0 .. 64");
    if (!(p->sigma_l >= 0.0) || !std::isfinite(p->sigma_l)) return fail(MCPT_ERR_ARG, "sigma_l must be finite and >= 0");
    if (!(p->sigma_p >= 0.0) || !std::isfinite(p->sigma_p)) return fail(MCPT_ERR_ARG, "sigma_p must be finite and >= 0");
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(MCPT_ERR_ARG, "mcpt_lightmap_denoise_params.reserved must be 0");
    if (!irradiance3) return fail(MCPT_ERR_ARG, "null irradiance map");
    if (!stderr3) return fail(MCPT_ERR_ARG, "null stderr map");
    if (!out3) return fail(MCPT_ERR_ARG, "null output map");
    return MCPT_OK;
}

// (a map too large for the memory that is left is MCPT_ERR_NOMEM, and the device stays usable)
static const char* const kWork = "the lightmap denoiser's workspace";

// The whole call on st, after the refusals; device pointers throughout.  Nothing here waits for st.
static int denoise_device(mcpt_device* d, const double* d_uv6, const mcpt_lightmap_denoise_params& p, const double* d_irr, const double* d_err,
                          double* d_out, int32_t* d_owner, hipStream_t st)
{
    if (const int rc = lightmap_device_gate(d)) return rc;
    const int W = p.width, H = p.height, R = p.dilate, K = p.iterations;
    const size_t n = size_t(W) * H;
    const double sigma_l = p.sigma_l > 0.0 ? p.sigma_l : MCPT_LIGHTMAP_DENOISE_SIGMA_L;
    const double sigma_p = p.sigma_p > 0.0 ? p.sigma_p : MCPT_LIGHTMAP_DENOISE_SIGMA_P;
    LightmapWork w{};
    Lease l;
    if (const int rc = lightmap_ensure_work(d, W, H, w, st, l)) return rc;
    mcpt_device::Lightmap& m = *d->lm;
    if (const int rc = grow(m.dn_guide, n * sizeof(LightmapGuide), kWork)) return rc;
    if (K > 0) {
        if (const int rc = grow(m.dn_buf[0], n * sizeof(LightmapPix), kWork)) return rc;
        if (const int rc = grow(m.dn_buf[1], n * sizeof(LightmapPix), kWork)) return rc;
    }
    if (R > 0) {
        if (const int rc = grow(m.owner[1], n, kWork)) return rc;
        if (const int rc = grow(m.irr, n * 3, kWork)) return rc;
    }
    launch_lightmap_raster(d->ds, d_uv6, W, H, w, st);
    HIP_TRY(hipGetLastError());
    // the dilation's rounds alternate between the caller's frame and the baker's own: the filter writes where R rounds end in the caller's
    double* const frame[2] = {d_out, m.irr.get()};
    int at = R & 1;
    launch_lightmap_denoise(d->ds, d_uv6, W, H, w, d_irr, d_err, K, sigma_l, sigma_p, reinterpret_cast<LightmapGuide*>(m.dn_guide.get()),
                            reinterpret_cast<LightmapPix*>(m.dn_buf[0].get()), reinterpret_cast<LightmapPix*>(m.dn_buf[1].get()), frame[at], st);
    HIP_TRY(hipGetLastError());
    int32_t* const own[2] = {m.owner[0].get(), m.owner[1].get()};
    lightmap_dilate_rounds(frame, own, W, H, R, 3, at, st);
    HIP_TRY(hipGetLastError());
    if (d_owner) HIP_TRY(hipMemcpyAsync(d_owner, own[R & 1], n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    return l.end(MCPT_OK);
}

extern "C" {

int mcpt_lightmap_denoise_device(mcpt_device* d, const double* d_uv6, const mcpt_lightmap_denoise_params* p, const double* d_irradiance3,
                                 const double* d_stderr3, double* d_out3, int32_t* d_owner, void* stream)
{
    if (const int rc = params_check(p, d_irradiance3, d_stderr3, d_out3)) return rc;
    return denoise_device(d, d_uv6, *p, d_irradiance3, d_stderr3, d_out3, d_owner, static_cast<hipStream_t>(stream));
}

int mcpt_lightmap_denoise(mcpt_device* d, const double* uv6, const mcpt_lightmap_denoise_params* p, const double* irradiance3, const double* stderr3,
                          double* out3, int32_t* owner)
{
    if (const int rc = params_check(p, irradiance3, stderr3, out3)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (uv6)
        if (const int rc = lightmap_chart_check(uv6, d->ds.t)) return rc;
    const size_t n = size_t(p->width) * p->height;
    Staging S(d->stream.get());
    const double *d_uv = nullptr, *d_irr = nullptr, *d_err = nullptr;    // (a null chart stays null: the scene's own vt)
    double* d_out = nullptr;
    int32_t* d_owner = nullptr;
    if (const int rc = S.in(uv6, size_t(d->ds.t) * 6, "the chart", d_uv)) return rc;
    if (const int rc = S.in(irradiance3, n * 3, "the irradiance map", d_irr)) return rc;
    if (const int rc = S.in(stderr3, n * 3, "the standard error map", d_err)) return rc;
    if (const int rc = S.out(out3, n * 3, "the denoised map", d_out)) return rc;
    if (const int rc = S.out(owner, n, "the owner map", d_owner)) return rc;
    return S.finish(denoise_device(d, d_uv, *p, d_irr, d_err, d_out, d_owner, d->stream.get()));
}

}  // extern "C"
