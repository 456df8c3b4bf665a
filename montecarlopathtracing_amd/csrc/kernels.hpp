// Launch interface between the C-ABI layer (the host files handles.hpp lists) and the HIP kernels (kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include "device_scene.hpp"
#include "path_variant.hpp"

namespace mcpt {

#define MCPT_MAX_DEPTH_DEV 64      /* == MCPT_MAX_DEPTH in mcpt.h (D6) */

struct PrimaryHit {                 // closest hit of a pixel's (sample-independent) primary ray
    int32_t leaf;
    int32_t surf;                   // wavefront frames: the pixel's PrimarySurface within its chunk (wavefront.hpp), set by k_primary_surface; else 0
    double t;
    double p[3];
};

struct TraceQueue;

// Resident grid sizes and tuning knobs of the persistent kernels, per GPU: filled once by init_launch_cfg() while that device is
// current (mcpt_device_create), carried by the mcpt_device -- nothing about a launch is process-wide, so one process can drive
// several GPUs from several threads.
struct LaunchCfg {
    int cus = 0;
    // k_wf_logic<true> / <false> and k_wf_finish, one entry per path variant (path_variant.hpp: variant_index(env, pick)) -- every
    // instantiation has its own occupancy, so fewer waves of one may be resident than of another
    unsigned logic_first[kPathVariants] = {}, logic_rest[kPathVariants] = {};
    int finish_grid[kPathVariants] = {};
    int trace_grid = 0, trace_grid_short = 0;       // k_wf_trace (deep / short stack)
    int array_grid = 0, primary_grid = 0;           // k_trace_persistent<ArrayRaySource> / <PrimaryRaySource>, deep stack
    int array_grid_short = 0, primary_grid_short = 0;   // ... short stack
    long long trace_block_rays = 2048;              // MCPT_TRACE_BLOCK_RAYS: a block of k_wf_trace is started per this many rays
    int min_chunk = 256, max_chunk = 2048;          // MCPT_TRACE_MIN_CHUNK / MAX_CHUNK: ray slots per queue claim
    int trace_pool = 0;                             // the pool engine (rays resident in LDS: k_wf_trace_pool, k_trace_pool) instead of the voting engine
    int finish_pool = 0;                            // the finishing pass in its pool form (k_wf_finish_pool: paths resident with their rays)
};
bool pool_engine_available();                      // wavefront.hip: the current device can hold a workgroup of the pool engine
bool pool_engine_available_closest();              // kernels.hip: ... of its closest-hit forms
size_t pool_spill_bytes(int cus);                  // wavefront.hip: bytes the pool engine wants behind a launch's deferred-ray list (stack entries beyond its LDS part)
void init_launch_cfg(LaunchCfg& cfg, unsigned forced_logic_grid, long long trace_block_rays, int min_chunk, int max_chunk);   // wavefront.hip (calls init_launch_cfg_closest of kernels.hip)
void init_launch_cfg_closest(LaunchCfg& cfg);
void launch_trace_closest(const DScene& S, bool fast, const double* d_rays, long long n, int32_t* d_face, double* d_t, double* d_p,
                          double* d_pn, DCounters* ctr, TraceQueue* queue, long long* slow_list, unsigned int slow_cap, hipStream_t st,
                          const LaunchCfg& cfg);
// ... with the leaf of every hit in d_leaf (-1: a miss) instead of the .obj face, and no normal: the same walks, t and p
void launch_trace_closest_leaf(const DScene& S, bool fast, const double* d_rays, long long n, int32_t* d_leaf, double* d_t, double* d_p,
                               DCounters* ctr, TraceQueue* queue, long long* slow_list, unsigned int slow_cap, hipStream_t st, const LaunchCfg& cfg);
void launch_pack_pixels(const double* d_frame, const int32_t* d_pixels, long long n_pixels, double* d_out, hipStream_t st);
void launch_unpack_pixels(const double* d_in, const int32_t* d_pixels, long long n_pixels, double* d_frame, hipStream_t st);
void launch_primary_dirs(const DCamera& cam, double* d_dirs, hipStream_t st);
void launch_primary_hits(const DScene& S, bool fast, const double* d_dirs, const int32_t* d_pixels, int n_pixels, PrimaryHit* d_hits,
                         DCounters* ctr, TraceQueue* queue, long long* slow_list, unsigned int slow_cap, hipStream_t st, const LaunchCfg& cfg);
void launch_shade_samples(const DScene& S, unsigned long long seed, const double* d_dirs, const int32_t* d_pixels,
                          const PrimaryHit* d_hits, int first_slot, int n_slots, int spp, int sample_base, double* d_rad, DCounters* ctr, hipStream_t st);
void launch_sample_radiance(const DScene& S, unsigned long long seed, const double* d_dirs, const int32_t* d_pix, const int32_t* d_k,
                            long long n, double* d_rgb, DCounters* ctr, hipStream_t st);
// env (active: env_on): a pixel whose primary ray missed folds Le(d_dirs[pixel]) for each sample
void launch_fold_samples(const double* d_rad, const int32_t* d_pixels, const PrimaryHit* d_hits, int first_slot, int n_slots, int spp,
                         double* d_img, const DEnv& env, const double* d_dirs, hipStream_t st);
// ---- lenses (camera.hip).  d_pos: the W*H image-plane points of the camera (DLens::pos).  d_flags[slot * spp + k] (chunk-local): 1 when
// the camera ray of that sample hit something.
void launch_primary_pos(const DCamera& cam, double* d_pos, hipStream_t st);
void launch_camera_rays(const DLens& lens, unsigned long long seed, const int32_t* d_pix, const int32_t* d_k, long long n, double* d_rays6, hipStream_t st);
void launch_shade_samples_lens(const DScene& S, const DLens& lens, unsigned long long seed, const int32_t* d_pixels, int first_slot, int n_slots, int spp,
                               int sample_base, double* d_rad, uint8_t* d_flags, DCounters* ctr, hipStream_t st);
void launch_sample_radiance_lens(const DScene& S, const DLens& lens, unsigned long long seed, const int32_t* d_pix, const int32_t* d_k, long long n,
                                 double* d_rgb, DCounters* ctr, hipStream_t st);
// the folds of k_fold_samples / k_fold_progressive for the per-sample route (a camera ray that missed has radiance 0: it adds nothing);
// progressive: d_hitcnt[pix] += the hits of the pass, d_hit[pix] = d_hitcnt[pix] > 0
// (env active: a camera ray that missed has radiance Le, and every sample is folded)
void launch_fold_lens(const double* d_rad, const uint8_t* d_flags, const int32_t* d_pixels, int first_slot, int n_slots, int n, int k0, int N,
                      double* d_img, double* d_mom, uint8_t* d_hit, int32_t* d_hitcnt, bool env, hipStream_t st);
// ---- radiance queries (query.hip)
// the megakernel form of a query list: lane (slot, j) -> d_rad[(s*spp + j)*3], d_flags[s*spp + j], s = the slot within the chunk
void launch_query_samples(const DScene& S, const DQuery& q, unsigned long long seed, const int32_t* d_ids, int first_slot, int n_slots, int spp,
                          int sample_base, double* d_rad, uint8_t* d_flags, DCounters* ctr, hipStream_t st);
// the fold of a chunk's n samples per slot into q's outputs at slots first_slot .. first_slot + n_slots; env: a missed ray's radiance is
// Le of its direction (else +0.0)
void launch_query_fold(const DQuery& q, const double* d_rad, const uint8_t* d_flags, int first_slot, int n_slots, int n, bool env, hipStream_t st);
// the same for a probe list (q.kind == MCPT_QUERY_KIND_SPHERE): every sample times the nine basis functions of its own direction, drawn
// again from (seed, d_ids[slot] or slot, sample_base + j); q.mean3 and q.stderr3 are [n][9][3]
void launch_query_fold_sh(const DQuery& q, unsigned long long seed, const int32_t* d_ids, const double* d_rad, const uint8_t* d_flags, int first_slot,
                          int n_slots, int n, int sample_base, bool env, hipStream_t st);
// test seam: the ray of sample d_k[i] of query i
void launch_query_rays(const DQuery& q, unsigned long long seed, const int32_t* d_ids, const int32_t* d_k, long long n, double* d_rays6, hipStream_t st);
// launch_fold_progressive for a piece of a motion frame (camera.hip): a pixel's primary ray may hit in one piece and miss in another, so a
// missed piece's samples (0, or Le under an environment) continue the fold and the moments; d_hit[pix] = hit in some piece so far
void launch_fold_motion(const double* d_rad, const int32_t* d_pixels, const PrimaryHit* d_hits, int first_slot, int n_slots, int n, int k0, int N,
                        double* d_img, double* d_mom, uint8_t* d_hit, const DEnv& env, const double* d_dirs, hipStream_t st);
// ---- the environment's test seams (env.hip): rgb[n*3] = Le(dirs[i]); out7[n*7] = direction, pdf, radiance of the block-(nl + 2) draw
void launch_env_eval(const DEnv& E, const double* d_dirs, long long n, double* d_rgb, hipStream_t st);
void launch_env_sample(const DEnv& E, unsigned long long seed, const int32_t* d_pix, const int32_t* d_k, int depth, int nl, long long n, double* d_out7,
                       hipStream_t st);
// MCPT_LIGHTS_ONE's test seam (kernels.hip): d_light[i] = the light S.pick draws at vertex `depth` of camera sample (pix[i], k[i])
void launch_light_pick(const DScene& S, unsigned long long seed, const int32_t* d_pix, const int32_t* d_k, int depth, long long n, int32_t* d_light, hipStream_t st);
// MCPT_LIGHTS_TREE's test seam: the light S.pick's tree gives the vertex (p[i], pn[i]) at `depth` of camera sample (pix[i], k[i]), and its probability
void launch_light_pick_at(const DScene& S, unsigned long long seed, const int32_t* d_pix, const int32_t* d_k, int depth, const double* d_p, const double* d_pn,
                          long long n, int32_t* d_light, double* d_pdf, hipStream_t st);
// progressive frames: fold of samples [k0, k0 + n) of a frame of N into d_img, moments into d_mom ([W*H][2][3]), primary hit flags into d_hit
void launch_fold_progressive(const double* d_rad, const int32_t* d_pixels, const PrimaryHit* d_hits, int first_slot, int n_slots, int n, int k0, int N,
                             double* d_img, double* d_mom, uint8_t* d_hit, const DEnv& env, const double* d_dirs, hipStream_t st);
// frame summary after `done` samples (done >= 2): d_out[0..3] = sum se2, sum mean^2, hit pixels, 0; d_partials holds noise_ranges() x 3 doubles
constexpr int kNoiseRanges = 1024;
int noise_ranges(long long n_pixels);
// d_cnt == null: every pixel holds `done` samples; otherwise pixel p holds d_cnt[p] (adaptive frames)
void launch_noise_reduce(const int32_t* d_pixels, long long n_pixels, const double* d_mom, const uint8_t* d_hit, int done, const int32_t* d_cnt,
                         double* d_partials, double* d_out, hipStream_t st);
// d_missed_hit (the per-pixel route under an environment, else null): a pixel with d_missed_hit[pix] == 0 shows d_img -- the whole frame's
// fold of Le, the same at every count
void launch_progressive_image(const int32_t* d_pixels, long long n_pixels, const double* d_img, const double* d_mom, int done, const int32_t* d_cnt,
                              int N, double* d_est, double* d_err, const uint8_t* d_missed_hit, hipStream_t st);
// adaptive frames: after a pass of k samples over d_list[0..n), d_cnt[p] = k for every listed p, and the pixels that continue go to d_out
// in list order, their number to *d_total.  d_masks holds 4 * adaptive_blocks(n) words, d_block_counts / d_block_offsets adaptive_blocks(n).
int adaptive_blocks(int n);
void launch_adaptive_select(const int32_t* d_list, int n, const double* d_mom, const uint8_t* d_hit, int k, int min_spp, double rel2, double abs2,
                            int32_t* d_cnt, unsigned long long* d_masks, int32_t* d_block_counts, int32_t* d_block_offsets, int32_t* d_total,
                            int32_t* d_out, hipStream_t st);

}  // namespace mcpt
