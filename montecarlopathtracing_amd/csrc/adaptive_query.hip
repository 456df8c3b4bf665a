// Adaptive radiance queries (mcpt_query_radiance_adaptive, mcpt_bake_lightmap_adaptive): the kernels around the unchanged query pass.
// Before a pass the active queries are gathered into a compact list (k_aq_gather), which the source pass, the engines and the megakernel
// form render as any list; the pass's fold continues every active query's moments at its position in the caller's list
// (k_query_fold_moments); k_adaptive_select / scan / scatter (kernels.hip, unchanged) decide over list positions which queries go on; and
// after the last pass k_aq_finish forms the answers of all queries.  -ffp-contract=off (Makefile).
#include <hip/hip_runtime.h>

#include "adaptive_query.hpp"
#include "dev_common.hpp"

namespace mcpt {

__global__ void __launch_bounds__(256) k_aq_iota(int32_t* __restrict__ sel, long long n)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sel[i] = (int32_t)i;
}

// One lane per active query: 48 bytes of q6 and 4 of id written per query and pass, against the 60 bytes per sample of the source pass
// that reads them.
__global__ void __launch_bounds__(256) k_aq_gather(const double* __restrict__ q6, const int32_t* __restrict__ ids, const int32_t* __restrict__ sel,
                                                   long long n_active, double* __restrict__ cq6, int32_t* __restrict__ cids)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_active) return;
    const int pos = sel[i];
    const double* src = q6 + (size_t)pos * 6;
    double* dst = cq6 + (size_t)i * 6;
#pragma unroll
    for (int c = 0; c < 6; c++) dst[c] = src[c];
    cids[i] = ids ? ids[pos] : pos;
}

// k_query_fold (query.hip) between two stored sums: one lane per (slot, channel), the slot's hit flags first, then its n samples in k
// order, no atomics -- s1 += x, s2 += x * x -- starting from the s1, s2 and hit count the passes before left at the query's position in
// the caller's list, sel[first_slot + s], and stored back there.  A stored fp64 sum reloaded is the same sum, so after the pass that ends
// at count c the sums are those of k_query_fold over the c samples at once.  A slot none of whose rays hit in this pass is not read
// without an environment: its samples are +0.0 and leave both sums as they are.
template <bool ENV>
__global__ void __launch_bounds__(256) k_query_fold_moments(const double* __restrict__ rad, const uint8_t* __restrict__ flags,
                                                            const int32_t* __restrict__ sel, int first_slot, int n_slots, int n,
                                                            double* __restrict__ mom, int32_t* __restrict__ hitcnt)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long long)n_slots * 3) return;
    const int s = (int)(gid / 3), c = (int)(gid % 3);
    const double* src = rad + (size_t)s * n * 3 + c;
    const uint8_t* f = flags + (size_t)s * n;
    int h = 0;
    for (int k = 0; k < n; k++) h += f[k];
    const int pos = sel[first_slot + s];
    double* m = mom + (size_t)pos * 6 + c;
    if (h > 0 || ENV) {
        double s1 = m[0], s2 = m[3];
        for (int k = 0; k < n; k++) {
            const double x = src[(size_t)k * 3];
            s1 += x;
            s2 += x * x;
        }
        m[0] = s1; m[3] = s2;
    }
    if (c == 0 && h > 0) hitcnt[pos] += h;
}

// One lane per (query, channel) over the whole of the caller's list: mean, standard error, hits and count from the moments and the
// query's own count, as k_query_fold forms them from a one-shot call's.
__global__ void __launch_bounds__(256) k_aq_finish(const double* __restrict__ mom, const int32_t* __restrict__ hitcnt, const int32_t* __restrict__ cnt,
                                                   long long n, double* __restrict__ mean3, double* __restrict__ stderr3, int32_t* __restrict__ hits,
                                                   int32_t* __restrict__ counts)
{
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n * 3) return;
    const long long i = gid / 3;
    const int c = (int)(gid % 3);
    const int k = cnt[i];
    const double s1 = mom[(size_t)i * 6 + c], s2 = mom[(size_t)i * 6 + 3 + c];
    mean3[gid] = s1 / k;
    if (stderr3) stderr3[gid] = k >= 2 ? sqrt(progressive_se2(s1, s2, k)) : 0.0;
    if (c == 0) {
        if (hits) hits[i] = hitcnt[i];
        if (counts) counts[i] = k;
    }
}

__global__ void __launch_bounds__(256) k_aq_scatter_counts(const int32_t* __restrict__ texels, long long n_list, const int32_t* __restrict__ cnt,
                                                           int32_t* __restrict__ map)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_list) map[texels[i]] = cnt[i];
}

// ------------------------------------------------------------------------------------------------ launchers
static inline unsigned blocks_of(long long n, int block) { return (unsigned)((n + block - 1) / block); }

void launch_aq_iota(int32_t* d_sel, long long n, hipStream_t st)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_aq_iota, dim3(blocks_of(n, 256)), dim3(256), 0, st, d_sel, n);
}
void launch_aq_gather(const double* d_q6, const int32_t* d_ids, const int32_t* d_sel, long long n_active, double* d_cq6, int32_t* d_cids, hipStream_t st)
{
    if (n_active <= 0) return;
    hipLaunchKernelGGL(k_aq_gather, dim3(blocks_of(n_active, 256)), dim3(256), 0, st, d_q6, d_ids, d_sel, n_active, d_cq6, d_cids);
}
void launch_query_fold_moments(const QueryMoments& m, const double* d_rad, const uint8_t* d_flags, int first_slot, int n_slots, int n, bool env,
                               hipStream_t st)
{
    if (n_slots <= 0) return;
    const dim3 grid(blocks_of((long long)n_slots * 3, 256));
    if (env) hipLaunchKernelGGL(k_query_fold_moments<true>, grid, dim3(256), 0, st, d_rad, d_flags, m.sel, first_slot, n_slots, n, m.mom, m.hitcnt);
    else hipLaunchKernelGGL(k_query_fold_moments<false>, grid, dim3(256), 0, st, d_rad, d_flags, m.sel, first_slot, n_slots, n, m.mom, m.hitcnt);
}
void launch_aq_finish(const double* d_mom, const int32_t* d_hitcnt, const int32_t* d_cnt, long long n, double* d_mean3, double* d_stderr3,
                      int32_t* d_hits, int32_t* d_counts, hipStream_t st)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_aq_finish, dim3(blocks_of(n * 3, 256)), dim3(256), 0, st, d_mom, d_hitcnt, d_cnt, n, d_mean3, d_stderr3, d_hits, d_counts);
}
void launch_aq_scatter_counts(const int32_t* d_texels, long long n_list, const int32_t* d_cnt, int32_t* d_map, hipStream_t st)
{
    if (n_list <= 0) return;
    hipLaunchKernelGGL(k_aq_scatter_counts, dim3(blocks_of(n_list, 256)), dim3(256), 0, st, d_texels, n_list, d_cnt, d_map);
}

}  // namespace mcpt
