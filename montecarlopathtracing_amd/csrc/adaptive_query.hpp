// Adaptive radiance queries (mcpt.h: adaptive queries): what a query call that stops every query on its own error keeps between its passes,
// and the launch interface of its kernels (adaptive_query.hip).  A pass renders the active queries as a compact list of their own through
// the unchanged source pass, engines and megakernel form; only the fold differs -- it continues the moments of the caller's positions.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace mcpt {

// Where a pass of an adaptive query call folds (SampleRange::moments, handles.hpp), all on the device.  Slot s of the pass is entry s of
// the active list; its sums live at the caller's position sel[s].
struct QueryMoments {
    double* mom;                // [n][2][3]: s1_c, s2_c of every position of the caller's list, added in k order from +0.0
    int32_t* hitcnt;            // [n]: the samples so far whose ray hit
    const int32_t* sel;         // [active]: the active list, positions into the caller's list, ascending
};

// sel[i] = i for the n positions of a call's first pass
void launch_aq_iota(int32_t* d_sel, long long n, hipStream_t st);
// The compact list of a pass, one lane per active query: cq6[i] = q6[sel[i]] (6 doubles), cids[i] = ids ? ids[sel[i]] : sel[i].
void launch_aq_gather(const double* d_q6, const int32_t* d_ids, const int32_t* d_sel, long long n_active, double* d_cq6, int32_t* d_cids,
                      hipStream_t st);
// The accumulating fold of a pass's chunk: k_query_fold's lanes and walk over rad / flags (n samples per slot, slots first_slot ..
// first_slot + n_slots - 1 of the active list), from and back into m.mom and m.hitcnt at position m.sel[first_slot + s].
void launch_query_fold_moments(const QueryMoments& m, const double* d_rad, const uint8_t* d_flags, int first_slot, int n_slots, int n, bool env,
                               hipStream_t st);
// The answers of all n queries from their moments and counts, k_query_fold's expressions; d_stderr3, d_hits and d_counts may be null.
void launch_aq_finish(const double* d_mom, const int32_t* d_hitcnt, const int32_t* d_cnt, long long n, double* d_mean3, double* d_stderr3,
                      int32_t* d_hits, int32_t* d_counts, hipStream_t st);
// The counts map of an adaptive lightmap: d_map[d_texels[i]] = d_cnt[i] for the n_list entries; the caller has cleared the map.
void launch_aq_scatter_counts(const int32_t* d_texels, long long n_list, const int32_t* d_cnt, int32_t* d_map, hipStream_t st);

}  // namespace mcpt
