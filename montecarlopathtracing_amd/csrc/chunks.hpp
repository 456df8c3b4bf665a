// How a call that works through a workspace of rays cuts its list of items (probes, texels, pixels, rays) into chunks.  Host only, and
// free of HIP: the arithmetic is tested on its own (tests/chunks_sanitize_main.cpp).
#pragma once
#include <cstdint>

namespace mcpt {

// the workspace of a call whose parameters leave workspace_rays at 0, in rays (mcpt.h states it per family, in bytes)
constexpr int64_t kDefaultWorkspaceRays = int64_t(1) << 22;

// The items per chunk of a list of n items of rays_per_item rays each under a budget of workspace_rays rays (0: the default): as many
// whole items as the budget holds, at least one, at most n.
// Bounds: 0 <= workspace_rays <= 2^62, 1 <= rays_per_item <= 2^62, 1 <= n <= 2^62 (an empty list is the callers' to return from).
// Nothing here multiplies, so nothing overflows.  The callers form chunk_plan(..) * rays_per_item, the rays of a full chunk: at most
// max(budget, rays_per_item) <= 2^62 (a single item may exceed the budget).  The callers' own limits are far below: rays_per_item
// <= 2^31 - 1 everywhere, and n * rays_per_item <= 2^31 - 1 for the reflection bake.
inline int64_t chunk_plan(int64_t workspace_rays, int64_t rays_per_item, int64_t n)
{
    const int64_t budget = workspace_rays > 0 ? workspace_rays : kDefaultWorkspaceRays;
    const int64_t per_chunk = budget / rays_per_item;
    return per_chunk < 1 ? 1 : (per_chunk > n ? n : per_chunk);
}

// the items of the chunk that starts at item `first` (0 <= first < n): per_chunk, or what is left of the list
inline int64_t chunk_count(int64_t per_chunk, int64_t n, int64_t first)
{
    return n - first < per_chunk ? n - first : per_chunk;
}

// The callers' loop: body(first, count) for every chunk of a list of n items in order, until the list is done or body returns non-zero,
// which is returned (else 0).  chunks = the calls of body.  first < n <= 2^62 before every step, so first + per_chunk does not overflow.
template <class Body>
int chunk_walk(int64_t n, int64_t per_chunk, int& chunks, Body body)
{
    int rc = 0;
    chunks = 0;
    for (int64_t first = 0; first < n && rc == 0; first += per_chunk, chunks++) rc = body(first, chunk_count(per_chunk, n, first));
    return rc;
}

}  // namespace mcpt
