// C ABI, irradiance volumes (include/mcpt.h: mcpt_volume_*, mcpt_bake_volume*): a regular grid of light probes and the lookup between
// them.  A bake writes the grid's positions on the GPU (volume.hip) and hands them to mcpt_query_sh's call (query_api.cpp: query_device,
// unchanged), so chunking, engines and statistics are the probe query's own.  The lookup takes coefficient arrays, not a bake; its
// arithmetic is volume.hpp's, compiled here for the host forms and in volume.hip for the GPU.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstring>
#include <string>

#include "handles.hpp"
#include "volume.hpp"

using namespace mcpt;

// what every call refuses of a grid, in the struct's field order
int volume_grid_check(const mcpt_volume_grid* g)
{
    if (!g) return fail(MCPT_ERR_ARG, "null volume grid");
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(g->origin[a])) return fail(MCPT_ERR_ARG, "a volume grid's origin must be finite");
    for (int a = 0; a < 3; a++)
        if (!(std::isfinite(g->spacing[a]) && g->spacing[a] > 0.0)) return fail(MCPT_ERR_ARG, "a volume grid's spacing must be finite and > 0 on every axis");
    if (g->nx < 1 || g->ny < 1 || g->nz < 1) return fail(MCPT_ERR_ARG, "a volume grid needs at least one probe on every axis");
    if (volume_probes(*g) > kInt32Max) return fail(MCPT_ERR_ARG, "a volume grid holds at most 2^31 - 1 probes");
    if (g->flags != 0 && g->flags != MCPT_VOLUME_CLAMP_ZERO) return fail(MCPT_ERR_ARG, "unknown volume flag (0 or MCPT_VOLUME_CLAMP_ZERO)");
    for (int i = 0; i < 4; i++)
        if (g->reserved[i] != 0) return fail(MCPT_ERR_ARG, "mcpt_volume_grid.reserved must be 0");
    return MCPT_OK;
}

// what every form of the lookup refuses without looking at the arrays
static int lookup_check(const mcpt_volume_grid* g, const void* sh27, const void* q6, int64_t n, const void* e3)
{
    if (const int rc = volume_grid_check(g)) return rc;
    if (const int rc = count_check(n, "receivers")) return rc;
    if (n > 0 && (!sh27 || !q6 || !e3)) return fail(MCPT_ERR_ARG, "null coefficients, receiver list or irradiance");
    return MCPT_OK;
}

// ... and what the host-pointer forms refuse of the arrays themselves
int volume_arrays_check(const mcpt_volume_grid& g, const double* sh27, const double* q6, int64_t n)
{
    const int64_t coefficients = volume_probes(g) * (MCPT_SH_N * 3);
    for (int64_t i = 0; i < coefficients; i++)
        if (!std::isfinite(sh27[i])) return fail(MCPT_ERR_ARG, "probe " + std::to_string(i / (MCPT_SH_N * 3)) + ": coefficient that is not finite");
    for (int64_t i = 0; i < n; i++) {
        const double* q = q6 + i * 6;
        for (int c = 0; c < 6; c++)
            if (!std::isfinite(q[c])) return fail(MCPT_ERR_ARG, "receiver " + std::to_string(i) + ": component that is not finite");
        const double l = std::sqrt((q[3] * q[3] + q[4] * q[4]) + q[5] * q[5]);
        if (!(std::isfinite(l) && l > 0.0)) return fail(MCPT_ERR_ARG, "receiver " + std::to_string(i) + ": the normal must have a non-zero finite length");
    }
    return MCPT_OK;
}

int volume_points_device(mcpt_device* d, const mcpt_volume_grid& g, hipStream_t st, Lease& l)
{
    if (const int rc = lease(d->vol, st, l)) return rc;    // the bake before this one has read its points
    if (const int rc = grow(d->vol->p3, size_t(volume_probes(g)) * 3, "the volume's probe positions")) return rc;
    launch_volume_points(g, d->vol->p3.get(), st);
    return launch_result();
}

// The bake on st, after the refusals; device pointers throughout.  Nothing here waits for st but the query itself, as mcpt_query_sh_device does.
static int bake_device(mcpt_device* d, const mcpt_volume_grid& g, const mcpt_sh_params& p, double* d_sh, double* d_err, int32_t* d_hits, mcpt_stats* stats,
                       hipStream_t st)
{
    if (const int rc = device_gate(d)) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    Lease l;
    if (const int rc = volume_points_device(d, g, st, l)) return rc;
    return l.end(query_device(d, DQuery{d->vol->p3.get(), MCPT_QUERY_KIND_SPHERE, d_sh, d_err, d_hits}, nullptr, volume_probes(g), p.spp, p.sample_base,
                              p.seed, p.flags, stats, st));
}

// the lookup on st, after the refusals: it allocates nothing and never waits
static int lookup_device(mcpt_device* d, const mcpt_volume_grid& g, const double* d_sh, const uint8_t* d_valid, const double* d_q6, int64_t n, double* d_e3,
                         int32_t* d_corners, hipStream_t st)
{
    if (const int rc = device_gate(d)) return rc;
    if (n == 0) return MCPT_OK;
    launch_volume_irradiance(g, d_sh, d_valid, d_q6, n, d_e3, d_corners, st);
    return launch_result();
}

extern "C" {

int mcpt_volume_points(const mcpt_volume_grid* g, double* p3)
{
    if (const int rc = volume_grid_check(g)) return rc;
    if (!p3) return fail(MCPT_ERR_ARG, "null positions");
    int64_t P = 0;
    for (int iz = 0; iz < g->nz; iz++)
        for (int iy = 0; iy < g->ny; iy++)
            for (int ix = 0; ix < g->nx; ix++, P++) {
                p3[P * 3 + 0] = volume_coord(*g, 0, ix);
                p3[P * 3 + 1] = volume_coord(*g, 1, iy);
                p3[P * 3 + 2] = volume_coord(*g, 2, iz);
            }
    return MCPT_OK;
}

int mcpt_bake_volume_device(mcpt_device* d, const mcpt_volume_grid* g, const mcpt_sh_params* p, double* d_sh27, double* d_stderr27, int32_t* d_hits,
                            mcpt_stats* stats, void* stream)
{
    if (!g || !p) return fail(MCPT_ERR_ARG, "null volume grid or probe parameters");
    if (const int rc = volume_grid_check(g)) return rc;
    if (const int rc = sh_params_check(p, volume_probes(*g), g, d_sh27)) return rc;
    return bake_device(d, *g, *p, d_sh27, d_stderr27, d_hits, stats, static_cast<hipStream_t>(stream));
}

int mcpt_bake_volume(mcpt_device* d, const mcpt_volume_grid* g, const mcpt_sh_params* p, double* sh27, double* stderr27, int32_t* hits, mcpt_stats* stats)
{
    if (!g || !p) return fail(MCPT_ERR_ARG, "null volume grid or probe parameters");
    if (const int rc = volume_grid_check(g)) return rc;
    if (const int rc = sh_params_check(p, volume_probes(*g), g, sh27)) return rc;
    if (const int rc = device_gate(d)) return rc;
    const size_t n = size_t(volume_probes(*g));
    Staging S(d->stream.get());
    double *d_sh = nullptr, *d_err = nullptr;
    int32_t* d_hits = nullptr;
    if (const int rc = S.out(sh27, n * MCPT_SH_N * 3, "the volume's coefficients", d_sh)) return rc;
    if (const int rc = S.out(stderr27, n * MCPT_SH_N * 3, "the volume's standard errors", d_err)) return rc;
    if (const int rc = S.out(hits, n, "the volume's hits", d_hits)) return rc;
    return S.finish(bake_device(d, *g, *p, d_sh, d_err, d_hits, stats, d->stream.get()));
}

int mcpt_volume_irradiance_host(const mcpt_volume_grid* g, const double* sh27, const uint8_t* valid, const double* q6, int64_t n, double* e3,
                                int32_t* corners)
{
    if (const int rc = lookup_check(g, sh27, q6, n, e3)) return rc;
    if (n == 0) return MCPT_OK;
    if (const int rc = volume_arrays_check(*g, sh27, q6, n)) return rc;
    const bool clamp = (g->flags & MCPT_VOLUME_CLAMP_ZERO) != 0;
    for (int64_t r = 0; r < n; r++) {
        int32_t P[8];
        double w[8], AY[MCPT_SH_N];
        const int c = volume_corners(*g, valid, q6 + r * 6, P, w);
        volume_lobe9(q6 + r * 6 + 3, AY);
        volume_eval(sh27, P, w, AY, c > 0, clamp, e3 + r * 3);
        if (corners) corners[r] = c;
    }
    return MCPT_OK;
}

int mcpt_volume_irradiance_device(mcpt_device* d, const mcpt_volume_grid* g, const double* d_sh27, const uint8_t* d_valid, const double* d_q6, int64_t n,
                                  double* d_e3, int32_t* d_corners, void* stream)
{
    if (const int rc = lookup_check(g, d_sh27, d_q6, n, d_e3)) return rc;
    return lookup_device(d, *g, d_sh27, d_valid, d_q6, n, d_e3, d_corners, static_cast<hipStream_t>(stream));
}

int mcpt_volume_irradiance(mcpt_device* d, const mcpt_volume_grid* g, const double* sh27, const uint8_t* valid, const double* q6, int64_t n, double* e3,
                           int32_t* corners)
{
    if (const int rc = lookup_check(g, sh27, q6, n, e3)) return rc;
    if (n > 0)
        if (const int rc = volume_arrays_check(*g, sh27, q6, n)) return rc;
    if (const int rc = device_gate(d)) return rc;
    if (n == 0) return MCPT_OK;
    const size_t probes = size_t(volume_probes(*g)), sn = size_t(n);
    Staging S(d->stream.get());
    const double *d_sh = nullptr, *d_q = nullptr;
    const uint8_t* d_valid = nullptr;
    double* d_e = nullptr;
    int32_t* d_corners = nullptr;
    if (const int rc = S.in(sh27, probes * MCPT_SH_N * 3, "the volume's coefficients", d_sh)) return rc;
    if (const int rc = S.in(q6, sn * 6, "the receiver list", d_q)) return rc;
    if (const int rc = S.in(valid, probes, "the volume's mask", d_valid)) return rc;
    if (const int rc = S.out(e3, sn * 3, "the receivers' irradiance", d_e)) return rc;
    if (const int rc = S.out(corners, sn, "the receivers' corners", d_corners)) return rc;
    return S.finish(lookup_device(d, *g, d_sh, d_valid, d_q, n, d_e, d_corners, d->stream.get()));
}

}  // extern "C"
