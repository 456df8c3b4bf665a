// C ABI, any-hit rays (include/mcpt.h: mcpt_trace_any*, mcpt_pair_rays, mcpt_trace_any_pairs*): is anything in the way of a ray before its
// limit, for a list of rays and for the matrix of point pairs of two lists, answered by a walk of its own that stops at the first blocker
// (any_hit.hip) beside the unchanged closest-hit engines.  The pair arithmetic and the matrix indexing are any_hit.hpp's, compiled here for
// mcpt_pair_rays.  No workspace is kept between calls: there is no lease.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstring>

#include "any_hit.hpp"
#include "handles.hpp"

using namespace mcpt;

// what the ray calls refuse: the count, then the two required arrays
static int rays_check(int64_t n, const void* rays6, const void* occluded)
{
    if (const int rc = count_check(n, "rays")) return rc;
    if (n > 0 && (!rays6 || !occluded)) return fail(MCPT_ERR_ARG, "null rays or occluded");
    return MCPT_OK;
}

// what the pair calls refuse: the parameters (flags and reserved, then the interval), the counts, the matrix's words, then the arrays.  out, out2: what
// the call writes when there is a pair at all (out2 only where the call has a second output)
static int pairs_check(const mcpt_pair_params* p, const void* a3, int64_t na, const void* b3, int64_t nb, const void* out, const void* out2, bool two)
{
    if (!p) return fail(MCPT_ERR_ARG, "null pair parameters");
    if (p->flags != 0) return fail(MCPT_ERR_ARG, "mcpt_pair_params.flags must be 0");
    if (p->reserved != 0) return fail(MCPT_ERR_ARG, "mcpt_pair_params.reserved must be 0");
    if (!(std::isfinite(p->t0) && std::isfinite(p->t1) && 0.0 <= p->t0 && p->t0 < p->t1)) return fail(MCPT_ERR_ARG, "t0 and t1 must be finite with 0 <= t0 < t1");
    if (const int rc = count_check(na, "first points")) return rc;
    if (const int rc = count_check(nb, "second points")) return rc;
    if (!pair_words_ok(na, nb)) return fail(MCPT_ERR_ARG, "the matrix must not exceed 2^31 - 1 words");
    if ((na > 0 && !a3) || (nb > 0 && !b3)) return fail(MCPT_ERR_ARG, "null point list");
    if (na > 0 && nb > 0 && (!out || (two && !out2))) return fail(MCPT_ERR_ARG, "null output");
    return MCPT_OK;
}

// what every call on a device does after its refusals, as mcpt_trace_closest_device: key 0 of a motion, a geometry that stands
static int any_gate(mcpt_device* d)
{
    if (const int rc = device_gate(d)) return rc;
    if (const int rc = motion_home(d)) return rc;
    return geometry_gate(d);
}

static bool fast_walk(const mcpt_device* d) { return d->trace_mode == MCPT_TRACE_FAST && d->ds.fast.enabled != 0; }

extern "C" {

int mcpt_trace_any_device(mcpt_device* d, const double* d_rays6, const double* d_tmax, int64_t n, uint8_t* d_occluded, void* stream)
{
    if (const int rc = rays_check(n, d_rays6, d_occluded)) return rc;
    if (const int rc = any_gate(d)) return rc;
    if (n == 0) return MCPT_OK;
    launch_any_rays(d->ds, fast_walk(d), d_rays6, d_tmax, n, d_occluded, d->aux_ctr.get(), d->cfg.cus, static_cast<hipStream_t>(stream));
    return launch_result();
}

int mcpt_trace_any(mcpt_device* d, const double* rays6, const double* tmax, int64_t n, uint8_t* occluded, mcpt_stats* stats)
{
    if (const int rc = rays_check(n, rays6, occluded)) return rc;
    if (const int rc = any_gate(d)) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n == 0) return MCPT_OK;
    const size_t sn = size_t(n);
    Staging S(d->stream.get());
    const double *d_rays = nullptr, *d_tmax = nullptr;
    uint8_t* d_occ = nullptr;
    if (const int rc = S.in(rays6, sn * 6, "the rays", d_rays)) return rc;
    if (const int rc = S.in(tmax, sn, "the rays' limits", d_tmax)) return rc;
    if (const int rc = S.out(occluded, sn, "the rays' answers", d_occ)) return rc;
    return host_form(d, S, n, stats, [&](hipStream_t st) {
        launch_any_rays(d->ds, fast_walk(d), d_rays, d_tmax, n, d_occ, d->aux_ctr.get(), d->cfg.cus, st);
    });
}

int mcpt_pair_rays(const double* a3, int64_t na, const double* b3, int64_t nb, const mcpt_pair_params* p, double* rays6, double* tmax)
{
    if (const int rc = pairs_check(p, a3, na, b3, nb, rays6, tmax, true)) return rc;
    if (na == 0 || nb == 0) return MCPT_OK;
    for (int64_t i = 0; i < na; i++)
        for (int64_t j = 0; j < nb; j++) {
            const PairRay r = pair_ray(a3 + i * 3, b3 + j * 3, p->t0, p->t1);
            double* o = rays6 + (i * nb + j) * 6;
            o[0] = r.o[0]; o[1] = r.o[1]; o[2] = r.o[2]; o[3] = r.d[0]; o[4] = r.d[1]; o[5] = r.d[2];
        }
    *tmax = p->t1 - p->t0;
    return MCPT_OK;
}

int mcpt_trace_any_pairs_device(mcpt_device* d, const double* d_a3, int64_t na, const double* d_b3, int64_t nb, const mcpt_pair_params* p,
                                uint64_t* d_bits, void* stream)
{
    if (const int rc = pairs_check(p, d_a3, na, d_b3, nb, d_bits, nullptr, false)) return rc;
    if (const int rc = any_gate(d)) return rc;
    if (na == 0 || nb == 0) return MCPT_OK;
    launch_any_pairs(d->ds, fast_walk(d), d_a3, na, d_b3, nb, p->t0, p->t1, reinterpret_cast<unsigned long long*>(d_bits), d->aux_ctr.get(), d->cfg.cus,
                     static_cast<hipStream_t>(stream));
    return launch_result();
}

int mcpt_trace_any_pairs(mcpt_device* d, const double* a3, int64_t na, const double* b3, int64_t nb, const mcpt_pair_params* p, uint64_t* bits,
                         mcpt_stats* stats)
{
    if (const int rc = pairs_check(p, a3, na, b3, nb, bits, nullptr, false)) return rc;
    if (const int rc = any_gate(d)) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (na == 0 || nb == 0) return MCPT_OK;
    Staging S(d->stream.get());
    const double *d_a = nullptr, *d_b = nullptr;
    uint64_t* d_bits = nullptr;
    if (const int rc = S.in(a3, size_t(na) * 3, "the first points", d_a)) return rc;
    if (const int rc = S.in(b3, size_t(nb) * 3, "the second points", d_b)) return rc;
    if (const int rc = S.out(bits, size_t(na * pair_row_words(nb)), "the pair matrix", d_bits)) return rc;
    return host_form(d, S, na * nb, stats, [&](hipStream_t st) {
        launch_any_pairs(d->ds, fast_walk(d), d_a, na, d_b, nb, p->t0, p->t1, reinterpret_cast<unsigned long long*>(d_bits), d->aux_ctr.get(), d->cfg.cus, st);
    });
}

}  // extern "C"
