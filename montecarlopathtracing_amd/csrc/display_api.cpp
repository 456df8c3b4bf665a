// C ABI, display transform (include/mcpt.h: mcpt_display_*): a linear fp64 frame becomes 8-bit pixels -- on the GPU where the frame lies
// (display.hip), or on the CPU for frames that end on the host (mcpt_display_host: the same header's arithmetic, display_math.hpp).
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "display.hpp"
#include "handles.hpp"

using namespace mcpt;

int display_check(const mcpt_display_params* p)
{
    if (!p) return MCPT_OK;
    if (p->reserved != 0) return fail(MCPT_ERR_ARG, "mcpt_display_params.reserved must be 0");
    if (p->curve != MCPT_CURVE_CLAMP && p->curve != MCPT_CURVE_REINHARD && p->curve != MCPT_CURVE_FILMIC)
        return fail(MCPT_ERR_ARG, "unknown display curve");
    if (p->transfer != MCPT_TRANSFER_LINEAR && p->transfer != MCPT_TRANSFER_SRGB) return fail(MCPT_ERR_ARG, "unknown display transfer");
    if (p->flags & ~MCPT_DISPLAY_RGBA) return fail(MCPT_ERR_ARG, "unknown display flag");
    for (const double v : {p->exposure, p->auto_key, p->percentile, p->white})
        if (!(std::isfinite(v) && v >= 0.0)) return fail(MCPT_ERR_ARG, "display exposure, auto_key, percentile and white must be finite and >= 0");
    if (p->percentile > 1.0) return fail(MCPT_ERR_ARG, "display percentile outside [0, 1]");
    return MCPT_OK;
}

// The parameters q (checked) become the map m and the report info; take(slots) fills the histogram and is called only when q needs it.
template <class Take>
static int display_resolve(const mcpt_display_params& q, Take&& take, DisplayMap& m, mcpt_display_info& info)
{
    info = mcpt_display_info{};
    double e = q.exposure > 0.0 ? q.exposure : 1.0;
    const bool reinhard = q.curve == MCPT_CURVE_REINHARD;
    if (q.auto_key > 0.0 || (reinhard && q.white == 0.0)) {
        int64_t slots[MCPT_DISPLAY_SLOTS];
        if (const int rc = take(slots)) return rc;
        if (const int rc = mcpt_display_exposure(slots, q.percentile, &info.log_average, &info.l_percentile)) return rc;
        info.skipped = slots[0];
        for (int s = 1; s < MCPT_DISPLAY_SLOTS; s++) info.counted += slots[s];
        if (q.auto_key > 0.0 && info.log_average > 0.0) e = e * (q.auto_key / info.log_average);
    }
    double w = q.white;
    if (reinhard && w == 0.0) {
        w = e * info.l_percentile;
        w = w > 1.0 ? w : 1.0;                              // max(1, e * l_percentile); 1 when nothing was counted
    }
    info.exposure = e;
    info.white = w;
    m.e = e; m.ww = w * w; m.curve = q.curve; m.transfer = q.transfer;
    return MCPT_OK;
}

// the histogram's slots on the device and their pinned copy, made on the device's first display call
static int ensure_slots(mcpt_device* d)
{
    if (!d->disp_slots) HIP_TRY(d->disp_slots.alloc(MCPT_DISPLAY_SLOTS));
    if (!d->h_disp_slots) HIP_TRY(d->h_disp_slots.alloc(MCPT_DISPLAY_SLOTS));
    return MCPT_OK;
}

int display_histogram_device(mcpt_device* d, const double* d_img, const int32_t* d_pixels, int64_t n, int64_t* slots, hipStream_t st)
{
    if (const int rc = ensure_slots(d)) return rc;
    HIP_TRY(hipMemsetAsync(d->disp_slots.get(), 0, MCPT_DISPLAY_SLOTS * sizeof(unsigned long long), st));
    launch_display_histogram(d_img, d_pixels, n, d->disp_slots.get(), st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(d->h_disp_slots.get(), d->disp_slots.get(), MCPT_DISPLAY_SLOTS * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::memcpy(slots, d->h_disp_slots.get(), MCPT_DISPLAY_SLOTS * sizeof(int64_t));
    return MCPT_OK;
}

int display_frame_device(mcpt_device* d, const double* d_img, const int32_t* d_pixels, int64_t n, const mcpt_display_params* p, uint8_t* d_out,
                         mcpt_display_info* info, hipStream_t st)
{
    const mcpt_display_params q = p ? *p : mcpt_display_params{};
    DisplayMap m{};
    mcpt_display_info rep{};
    if (const int rc = display_resolve(q, [&](int64_t* slots) { return display_histogram_device(d, d_img, d_pixels, n, slots, st); }, m, rep)) return rc;
    launch_display_map(d_img, d_pixels, n, m, (q.flags & MCPT_DISPLAY_RGBA) != 0, d_out, st);
    HIP_TRY(hipGetLastError());
    if (info) *info = rep;
    return MCPT_OK;
}

extern "C" {

int mcpt_display_exposure(const int64_t* slots, double percentile, double* log_average, double* l_percentile)
{
    if (!slots || !log_average || !l_percentile) return fail(MCPT_ERR_ARG, "null argument");
    if (!(percentile >= 0.0 && percentile <= 1.0)) return fail(MCPT_ERR_ARG, "display percentile outside [0, 1]");
    for (int s = 0; s < MCPT_DISPLAY_SLOTS; s++)
        if (slots[s] < 0) return fail(MCPT_ERR_ARG, "negative histogram count");
    const double p = percentile > 0.0 ? percentile : 0.99;
    // slot s counts at bin: the under slot at bin 0, the over slot at bin 383
    const auto bin_of = [](int s) { return s == 1 ? 0 : (s == MCPT_DISPLAY_SLOTS - 1 ? MCPT_DISPLAY_BINS - 1 : s - 2); };
    int64_t counted = 0;
    double sum = 0.0;
    for (int s = 1; s < MCPT_DISPLAY_SLOTS; s++) {
        if (slots[s] == 0) continue;
        const int b = bin_of(s);
        const double centre = std::ldexp(1.0 + (double(b & 7) + 0.5) / 8.0, (b >> 3) - 24);
        sum += double(slots[s]) * std::log2(centre);
        counted += slots[s];
    }
    *log_average = *l_percentile = 0.0;
    if (counted == 0) return MCPT_OK;
    *log_average = std::exp2(sum / double(counted));
    const double target = std::ceil(p * double(counted));
    int64_t running = 0;
    for (int s = 1; s < MCPT_DISPLAY_SLOTS; s++) {
        running += slots[s];
        if (slots[s] != 0 && double(running) >= target) {
            const int b = bin_of(s);
            *l_percentile = std::ldexp(1.0 + (double(b & 7) + 1.0) / 8.0, (b >> 3) - 24);
            break;
        }
    }
    return MCPT_OK;
}

int mcpt_display_host(const double* img, int64_t n_pixels, const mcpt_display_params* p, uint8_t* out, mcpt_display_info* info)
{
    if (const int rc = display_check(p)) return rc;
    if (n_pixels < 0 || (n_pixels > 0 && (!img || !out))) return fail(MCPT_ERR_ARG, "bad argument");
    const mcpt_display_params q = p ? *p : mcpt_display_params{};
    DisplayMap m{};
    mcpt_display_info rep{};
    const auto take = [&](int64_t* slots) {
        std::memset(slots, 0, MCPT_DISPLAY_SLOTS * sizeof(int64_t));
        for (int64_t i = 0; i < n_pixels; i++) slots[display_slot(display_luminance(img[3 * i], img[3 * i + 1], img[3 * i + 2]))]++;
        return MCPT_OK;
    };
    if (const int rc = display_resolve(q, take, m, rep)) return rc;
    const int bytes = (q.flags & MCPT_DISPLAY_RGBA) ? 4 : 3;
    for (int64_t i = 0; i < n_pixels; i++) {
        uint8_t* dst = out + i * bytes;
        display_pixel(m, img + 3 * i, dst);
        if (bytes == 4) dst[3] = 255;
    }
    if (info) *info = rep;
    return MCPT_OK;
}

int mcpt_display_histogram_device(mcpt_device* d, const double* d_img, int64_t n_pixels, int64_t* slots, void* stream)
{
    if (!d || !slots || n_pixels < 0 || (n_pixels > 0 && !d_img)) return fail(MCPT_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(d->ordinal));
    return display_histogram_device(d, d_img, nullptr, n_pixels, slots, static_cast<hipStream_t>(stream));
}

int mcpt_display_histogram(mcpt_device* d, const double* img, int64_t n_pixels, int64_t* slots)
{
    if (!d || !slots || n_pixels < 0 || (n_pixels > 0 && !img)) return fail(MCPT_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(d->ordinal));
    Staging S(d->stream.get());
    const double* d_img = nullptr;
    if (const int rc = S.in(img, size_t(n_pixels) * 3, "the frame", d_img)) return rc;
    return display_histogram_device(d, d_img, nullptr, n_pixels, slots, d->stream.get());            // (returns with the stream idle)
}

int mcpt_display_device(mcpt_device* d, const double* d_img, int64_t n_pixels, const mcpt_display_params* p, uint8_t* d_out, mcpt_display_info* info,
                        void* stream)
{
    if (const int rc = display_check(p)) return rc;
    if (!d || n_pixels < 0 || (n_pixels > 0 && (!d_img || !d_out))) return fail(MCPT_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(d->ordinal));
    return display_frame_device(d, d_img, nullptr, n_pixels, p, d_out, info, static_cast<hipStream_t>(stream));
}

int mcpt_display(mcpt_device* d, const double* img, int64_t n_pixels, const mcpt_display_params* p, uint8_t* out, mcpt_display_info* info)
{
    if (const int rc = display_check(p)) return rc;
    if (!d || n_pixels < 0 || (n_pixels > 0 && (!img || !out))) return fail(MCPT_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(d->ordinal));
    const size_t bytes = size_t(n_pixels) * ((p && (p->flags & MCPT_DISPLAY_RGBA)) ? 4 : 3);
    Staging S(d->stream.get());
    const double* d_img = nullptr;
    uint8_t* d_out = nullptr;
    if (const int rc = S.in(img, size_t(n_pixels) * 3, "the frame", d_img)) return rc;
    if (const int rc = S.out(out, bytes, "the picture", d_out)) return rc;
    return S.finish(display_frame_device(d, d_img, nullptr, n_pixels, p, d_out, info, d->stream.get()));
}

}  // extern "C"
