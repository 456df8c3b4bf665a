// C ABI, light sampling (include/mcpt.h: mcpt_device_set_light_sampling ... mcpt_light_pick): validation, the pick table in fp64, its
// upload and the test seam.  The kernels that use it are in vertex.hpp (light_pick, light_sample_one).
#include <cmath>
#include <cstring>
#include <vector>

#include "handles.hpp"

using namespace mcpt;

int light_sampling_check(const mcpt_light_sampling* ls)
{
    if (!ls) return MCPT_OK;
    if (ls->mode != MCPT_LIGHTS_ALL && ls->mode != MCPT_LIGHTS_ONE) return fail(MCPT_ERR_ARG, "mcpt_light_sampling.mode must be MCPT_LIGHTS_ALL or MCPT_LIGHTS_ONE");
    if (ls->num_weights < 0 || (ls->num_weights > 0) != (ls->weights != nullptr)) return fail(MCPT_ERR_ARG, "mcpt_light_sampling: num_weights and weights must go together");
    return MCPT_OK;
}

// The table of mcpt.h from the lights' radiances and areas (or the caller's weights), sequential sums left to right.  false: a weight
// is negative or not finite, or the caller's weights are all zero.
static bool pick_table(const std::vector<LightRec>& lights, const double* areas, const double* weights, std::vector<double>& cdf, std::vector<double>& pdf, int& last)
{
    const size_t n = lights.size();
    std::vector<double> w(n);
    if (weights) {
        for (size_t l = 0; l < n; l++) {
            if (!std::isfinite(weights[l]) || !(weights[l] >= 0.0)) return false;
            w[l] = weights[l];
        }
    } else {
        bool any = false;
        for (size_t l = 0; l < n; l++) {
            const Vec3& r = lights[l].radiance;
            const double lum = (0.2126 * r.x + 0.7152 * r.y) + 0.0722 * r.z;
            w[l] = lum * (areas ? areas[l] : lights[l].total_area);
            if (!std::isfinite(w[l]) || !(w[l] >= 0.0)) w[l] = 0.0;
            any = any || w[l] > 0.0;
        }
        if (!any) std::fill(w.begin(), w.end(), 1.0);
    }
    cdf.resize(n); pdf.resize(n);
    double run = 0.0;
    last = -1;
    for (size_t l = 0; l < n; l++) {
        run += w[l];
        cdf[l] = run;
        if (w[l] > 0.0) last = int(l);
    }
    if (last < 0 || !std::isfinite(run)) return false;
    for (size_t l = 0; l < n; l++) pdf[l] = w[l] / run;
    return true;
}

// d's table from its state (the caller's weights, or the lights' current areas: null = the scene's), copied into the device's two arrays
// (allocated by the first call: their size is the scene's light count); nothing in flight reads it
static int pick_upload(mcpt_device* d, LightPickData& k, const double* areas)
{
    const std::vector<LightRec>& lights = d->scene->s.lights;
    int last = -1;
    if (!pick_table(lights, areas, k.own_weights ? k.weights.data() : nullptr, k.cdf, k.pdf, last)) return fail(MCPT_ERR_ARG, "light weights: negative, not finite or all zero");
    std::vector<double> inv(k.pdf.size());
    for (size_t l = 0; l < inv.size(); l++) inv[l] = k.pdf[l] > 0.0 ? 1.0 / k.pdf[l] : 0.0;
    if (!k.d_cdf) { HIP_TRY(k.d_cdf.alloc(k.cdf.size())); HIP_TRY(k.d_inv.alloc(inv.size())); }
    HIP_TRY(hipMemcpy(k.d_cdf.get(), k.cdf.data(), k.cdf.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(k.d_inv.get(), inv.data(), inv.size() * sizeof(double), hipMemcpyHostToDevice));
    k.dpick = DLightPick{};
    if (k.mode == MCPT_LIGHTS_ONE && lights.size() >= 2) {          // (none or one light: the mode changes nothing)
        k.dpick.cdf = k.d_cdf.get(); k.dpick.inv_pdf = k.d_inv.get(); k.dpick.Z = k.cdf.back(); k.dpick.last = last;
    }
    return MCPT_OK;
}

// what mcpt_device_set_light_sampling refuses about ls on a scene of nl lights, beyond light_sampling_check: the count and the weights
int light_weights_check(const mcpt_light_sampling* ls, size_t nl)
{
    if (!ls || ls->num_weights == 0) return MCPT_OK;
    if (size_t(ls->num_weights) != nl) return fail(MCPT_ERR_ARG, "mcpt_light_sampling.num_weights must be the scene's light count");
    bool any = false;
    for (int32_t l = 0; l < ls->num_weights; l++) {
        if (!std::isfinite(ls->weights[l]) || !(ls->weights[l] >= 0.0)) return fail(MCPT_ERR_ARG, "light weights: negative, not finite or all zero");
        any = any || ls->weights[l] > 0.0;
    }
    return any ? MCPT_OK : fail(MCPT_ERR_ARG, "light weights: negative, not finite or all zero");
}

int light_pick_refresh(mcpt_device* d, const double* areas)
{
    if (!d->pick || d->pick->own_weights) return MCPT_OK;
    if (const int rc = pick_upload(d, *d->pick, areas)) return rc;
    d->ds.pick = d->pick->dpick;
    return MCPT_OK;
}

extern "C" {

int mcpt_scene_light_pick_table(const mcpt_scene* h, const double* weights, double* cdf, double* pdf)
{
    if (!h || !cdf || !pdf) return fail(MCPT_ERR_ARG, "null argument");
    if (h->s.lights.empty()) return fail(MCPT_ERR_ARG, "the scene has no lights");
    std::vector<double> c, p;
    int last = -1;
    if (!pick_table(h->s.lights, nullptr, weights, c, p, last)) return fail(MCPT_ERR_ARG, "light weights: negative, not finite or all zero");
    std::memcpy(cdf, c.data(), c.size() * sizeof(double));
    std::memcpy(pdf, p.data(), p.size() * sizeof(double));
    return MCPT_OK;
}

int mcpt_device_set_light_sampling(mcpt_device* d, const mcpt_light_sampling* ls)
{
    if (int rc = light_sampling_check(ls)) return rc;
    if (const int rc = require_device()) return rc;
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    const size_t nl = d->scene->s.lights.size();
    if (const int rc = light_weights_check(ls, nl)) return rc;
    if (const int rc = motion_home(d)) return rc;              // (the default weights are key 0's areas)
    HIP_TRY(hipSetDevice(d->ordinal));
    std::shared_ptr<LightPickData> k;
    if (ls && ls->mode != MCPT_LIGHTS_ALL) {
        k = std::make_shared<LightPickData>();
        k->mode = ls->mode;
        k->own_weights = ls->num_weights > 0;
        if (k->own_weights) k->weights.assign(ls->weights, ls->weights + ls->num_weights);
        if (nl > 0) {
            std::vector<double> areas;
            if (d->upd && !k->own_weights) {                       // an updated device: the areas its light records hold now
                std::vector<DLight> cur(nl);
                HIP_TRY(hipDeviceSynchronize());
                HIP_TRY(hipMemcpy(cur.data(), d->lights.get(), nl * sizeof(DLight), hipMemcpyDeviceToHost));
                for (const DLight& l : cur) areas.push_back(l.total_area);
            }
            if (const int rc = pick_upload(d, *k, areas.empty() ? nullptr : areas.data())) return rc;
        }
    }
    HIP_TRY(hipDeviceSynchronize());           // (frames in flight may still read the table being replaced)
    d->pick = k;
    d->ds.pick = k ? k->dpick : DLightPick{};
    return MCPT_OK;
}

int mcpt_device_get_light_sampling(const mcpt_device* d, int32_t* mode, double* pdf)
{
    if (const int rc = require_device()) return rc;
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    if (mode) *mode = d->pick ? d->pick->mode : MCPT_LIGHTS_ALL;
    if (pdf) {
        const size_t nl = d->scene->s.lights.size();
        if (d->pick && d->pick->pdf.size() == nl) std::memcpy(pdf, d->pick->pdf.data(), nl * sizeof(double));
        else for (size_t l = 0; l < nl; l++) pdf[l] = 1.0;      // MCPT_LIGHTS_ALL: every light, every vertex
    }
    return MCPT_OK;
}

int mcpt_light_pick(mcpt_device* d, uint64_t seed, const int32_t* pix, const int32_t* k, int32_t depth, int64_t n, int32_t* light, double* pdf)
{
    if (!pix || !k || !light || !pdf || n < 0 || depth < 0 || depth >= MCPT_MAX_DEPTH) return fail(MCPT_ERR_ARG, "bad argument");
    if (const int rc = require_device()) return rc;
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    if (!pick_on(d->ds.pick)) return fail(MCPT_ERR_ARG, "the device does not pick lights (MCPT_LIGHTS_ALL, or a scene of fewer than two lights)");
    if (n == 0) return MCPT_OK;
    HIP_TRY(hipSetDevice(d->ordinal));
    DevBuf<int32_t> d_pix, d_k, d_light;
    HIP_TRY(d_pix.alloc(size_t(n)));
    HIP_TRY(d_k.alloc(size_t(n)));
    HIP_TRY(d_light.alloc(size_t(n)));
    HIP_TRY(hipMemcpy(d_pix.get(), pix, size_t(n) * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_k.get(), k, size_t(n) * 4, hipMemcpyHostToDevice));
    launch_light_pick(d->ds, seed, d_pix.get(), d_k.get(), depth, n, d_light.get(), d->stream.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(d->stream.get()));
    HIP_TRY(hipMemcpy(light, d_light.get(), size_t(n) * 4, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; i++) pdf[i] = d->pick->pdf[size_t(light[i])];
    return MCPT_OK;
}

}  // extern "C"
