// What the calls that answer a list by closest hits, chunk by chunk, share on the host (hit_work.hpp).
#include "hit_work.hpp"

#include <string>

#include "handles.hpp"

using namespace mcpt;

int hit_work_grow(HitWork& w, int64_t rays, int64_t cap_rays, const char* noun, bool own_rays)
{
    const std::string the = std::string("the ") + noun;
    if (rays > cap_rays) return fail(MCPT_ERR_NOMEM, the + " workspace of " + std::to_string(rays) + " rays cannot be allocated");
    const size_t sr = size_t(rays);
    if (own_rays)
        if (const int rc = grow(w.rays6, sr * 6, (the + " rays").c_str())) return rc;
    if (const int rc = grow(w.t, sr, (the + " rays' distances").c_str())) return rc;
    if (const int rc = grow(w.p, sr * 3, (the + " rays' hit points").c_str())) return rc;
    return grow(w.leaf, sr, (the + " rays' hits").c_str());
}

void trace_leaf(mcpt_device* d, const double* d_rays6, long long n, int32_t* d_leaf, double* d_t, double* d_p, hipStream_t st)
{
    launch_trace_closest_leaf(d->ds, d->trace_mode == MCPT_TRACE_FAST, d_rays6, n, d_leaf, d_t, d_p, d->aux_ctr.get(), d->aux_queue.get(),
                              d->aux_slow_list.get(), d->slow_cap, st, d->cfg);
}

int chunk_stats(mcpt_stats* stats, int64_t n, int64_t rays_per_item, int chunks, hipStream_t st)
{
    if (!stats) return MCPT_OK;
    HIP_TRY(hipStreamSynchronize(st));
    stats->rays_primary = stats->samples = uint64_t(n) * uint64_t(rays_per_item);
    stats->launches = chunks;
    return MCPT_OK;
}
