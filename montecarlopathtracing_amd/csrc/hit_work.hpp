// What the calls that answer a list by closest hits, chunk by chunk, share on the host (hit_work.cpp): the workspace of a chunk's rays and
// hits, the one spelling of the closest-hit launch, and the loop over the chunks with its way out.  Visibility bakes, occlusion queries
// and the baked radiance and frame calls are that loop around their own launches.  Host only: no .hip file includes it.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "chunks.hpp"
#include "staging.hpp"

// the rays of a chunk and their closest hits, kept by the device between calls and grown to the largest chunk so far
struct HitWork {
    mcpt::DevBuf<double> rays6, t, p;               // [rays][6], [rays], [rays][3]
    mcpt::DevBuf<int32_t> leaf;                     // [rays]
};

#pragma GCC visibility push(hidden)

// w holds chunks of `rays` rays afterwards (rays6 only when own_rays: the rays are then the call's own, not the caller's).  More than
// cap_rays: MCPT_ERR_NOMEM, "the <noun> workspace of <rays> rays cannot be allocated".
int hit_work_grow(HitWork& w, int64_t rays, int64_t cap_rays, const char* noun, bool own_rays);

// the closest hits of rays6[0 .. n) on st under d's trace mode and engine (kernels.hip: launch_trace_closest_leaf): the leaf (-1: a
// miss), the distance and the hit point of every ray
void trace_leaf(mcpt_device* d, const double* d_rays6, long long n, int32_t* d_leaf, double* d_t, double* d_p, hipStream_t st);

// the way out of a chunk loop that went well: when the caller asks for statistics, st is waited for and they are n * rays_per_item rays
// in `chunks` launches
int chunk_stats(mcpt_stats* stats, int64_t n, int64_t rays_per_item, int chunks, hipStream_t st);

// A list of n items in chunks of per_chunk on st, under the lease l of the workspace: body(first, count) enqueues a chunk and returns
// launch_result().  The lease ends behind the last chunk enqueued, whatever came of it; a failure leaves `stats` as it was.
template <class Body>
int chunk_run(int64_t n, int64_t per_chunk, int64_t rays_per_item, Lease& l, mcpt_stats* stats, hipStream_t st, Body body)
{
    int chunks = 0;
    if (const int rc = l.end(mcpt::chunk_walk(n, per_chunk, chunks, body))) return rc;
    return chunk_stats(stats, n, rays_per_item, chunks, st);
}

// The host form of a trace call (mcpt_trace_closest, mcpt_trace_any, mcpt_trace_any_pairs) around its launch on the device's own stream:
// the auxiliary counters cleared and the first event recorded (host_form_begin hands the stream back), launch(st), then the second event,
// S.finish and, where asked for, the statistics of one launch (host_form_end).  answered: what rays_primary reports; kNotReported: it is
// left as it was.
constexpr int64_t kNotReported = -1;
int host_form_begin(mcpt_device* d, hipStream_t& st);
int host_form_end(mcpt_device* d, Staging& S, int64_t answered, mcpt_stats* stats);
template <class Launch>
int host_form(mcpt_device* d, Staging& S, int64_t answered, mcpt_stats* stats, Launch launch)
{
    hipStream_t st = nullptr;
    if (const int rc = host_form_begin(d, st)) return rc;
    launch(st);
    return host_form_end(d, S, answered, stats);
}

#pragma GCC visibility pop
