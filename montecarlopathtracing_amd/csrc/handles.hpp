// The C API's scene and device handles and the few host steps more than one of its files needs.  Host only: no .hip file includes it.
//   capi.cpp          error state, version, device count, the HIP runtime check
//   scene_api.cpp     scene handles, the tile partition, the trace engine of a scene, the shared culling hierarchy
//   device.cpp        device creation stage by stage, hierarchy queries, closest hit
//   render.cpp        lenses, the integrator (megakernel and wavefront), mcpt_render*, statistics, (pixel, sample) queries
//   query_api.cpp     radiance queries: the integrator behind a caller's rays, surface points and light probes
//   sh_api.cpp        light probes on the host: the spherical-harmonic basis, radiance and irradiance from a probe's coefficients
//   progressive.cpp   progressive frames, AOVs, the denoiser
//   light_sampling.cpp  MCPT_LIGHTS_ONE and MCPT_LIGHTS_TREE: the pick table, the light tree, their upload, the picks' test seams
//   motion.cpp        a device's motion: the shutter's steps between two keyframes, the return to key 0
//   display_api.cpp   the display transform: histogram, exposure, the map to 8-bit pixels on the GPU and on the host
//   lightmap_api.cpp  lightmap baking: a UV chart's coverage, its texel list, the hemisphere query of that list, scatter and dilation
//   adaptive_query_api.cpp  adaptive queries: the query call in passes, every query stopping on its own error estimate
//   lightmap_denoise_api.cpp  the lightmap denoiser: a chart-aware a-trous filter of an irradiance map, then the baker's dilation
//   volume_api.cpp    irradiance volumes: a probe grid's points, its bake through the probe query, the lookup between its probes
//   visibility_api.cpp  probe visibility: the octahedral bin, the depth-moment bake of a probe list or grid, the visibility-weighted lookup
//   occlusion_api.cpp  ambient occlusion: the hemisphere rays of a point list folded into occlusion and bent normals, and that query as a map
//   any_hit_api.cpp   any-hit rays: is anything in the way of a ray before its limit, for a ray list and for the matrix of two point lists' pairs
//   direct_api.cpp    direct light from a caller's own point, spot, directional and rectangle lights: a fused shadow-ray query, and that query as a map
//   baked_api.cpp     baked frames: the lightmap's lookup by chart coordinate, baked radiance along a caller's rays, frames lit by a bake
//   reflection_api.cpp  reflection probes: an octahedral radiance map per probe through the ray query, its Phong prefilter, the chain's lookup
//   render_scene.cpp  output writers, checkpoints, render_scene
//   staging.cpp       what the query family's files share (staging.hpp): the device gate, the allocation mapping, a host-pointer call's
//                     device copies, the lease of a per-device workspace; chunks.hpp: how a workspace budget cuts a list into chunks
//   hit_work.cpp      what the closest-hit chunk loops share (hit_work.hpp): the workspace of a chunk's rays and hits, the closest-hit
//                     launch, the loop and its statistics (visibility, occlusion, baked radiance and frames); the host form of a trace
//                     call around its launch (mcpt_trace_closest, mcpt_trace_any, mcpt_trace_any_pairs)
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstdint>
#include <functional>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "accel_build.hpp"
#include "adaptive_query.hpp"
#include "hip_owned.hpp"
#include "hit_work.hpp"
#include "kernels.hpp"
#include "knobs.hpp"
#include "scene.hpp"
#include "staging.hpp"
#include "stats.hpp"
#include "wavefront.hpp"

static_assert(MCPT_MAX_DEPTH_DEV == MCPT_MAX_DEPTH, "the kernels' path depth (kernels.hpp) is the C API's (mcpt.h)");

struct mcpt_scene {
    mcpt::Scene s;
    // The fast walk's culling hierarchy depends on the scene and the leaf order only: built once, shared by every device
    // created from this scene (one SAH build for the 8 GPUs of a node, not 8).
    mutable std::atomic<int> devices_created{0};      // mcpt_scene_set_resolution is refused once a device holds the camera
    // Shared ownership: the caller's handle and every device created from the scene hold one reference each; the scene goes with the
    // last of mcpt_scene_free / mcpt_device_free, in whichever order they come (a device keeps using the handle: the shared culling
    // hierarchy, the counter above).
    mutable std::atomic<int> refs{1};
    mutable std::mutex fast_mu;
    mutable std::shared_ptr<const mcpt::FastBvh> fast_cached;
    mutable std::vector<int32_t> fast_order;
    mutable int fast_leaf = 0;
    mutable double fast_ct = 0;
};

// start/stop events around a launch or a frame
using EventPair = std::pair<mcpt::Event, mcpt::Event>;

namespace mcpt {
// An environment as a device holds it (environment.cpp): the caller's texels and the sampling tables, on the GPU.  Shared: a progressive
// handle keeps the one it was created under alive after the device's is replaced.  denv is all zero when the map is inactive (Z == 0).
struct EnvData {
    int32_t W = 0, H = 0;
    double scale = 1.0, Z = 0.0;
    std::vector<float> rgb;                 // the caller's texels (the checkpoint identity mixes them in)
    DevBuf<float> d_rgb;
    DevBuf<double> d_c, d_marg, d_cond;
    DEnv denv{};
};
// A device's light sampling when it is not MCPT_LIGHTS_ALL (light_sampling.cpp): the pick table on the host and on the GPU.  dpick is all
// zero when the mode changes nothing (a scene of fewer than two lights).
struct LightPickData {
    int32_t mode = MCPT_LIGHTS_ALL;
    bool own_weights = false;               // the caller's weights; else luminance x area, made again when an update moves an emitter
    std::vector<double> weights;            // the caller's
    std::vector<double> cdf, pdf;           // the table (the checkpoint identity mixes pdf in)
    DevBuf<double> d_cdf, d_inv;
    std::vector<DLightNode> nodes;          // MCPT_LIGHTS_TREE: the tree as uploaded (the checkpoint identity mixes its bytes in)
    DevBuf<DLightNode> d_nodes;
    DLightPick dpick{};
};
}  // namespace mcpt

struct mcpt_device {
    int ordinal = 0;
    mcpt::Knobs knobs;                     // the environment as it was when this device was created (knobs.hpp)
    mcpt::DScene ds{};
    mcpt::Stream stream;                   // library stream for the host-pointer entry points
    // scene arrays
    mcpt::DevBuf<mcpt::DNode> nodes; mcpt::DevBuf<mcpt::DTri> tris; mcpt::DevBuf<mcpt::DTriShade> shade; mcpt::DevBuf<mcpt::DMaterial> materials;
    mcpt::DevBuf<mcpt::DLight> lights; mcpt::DevBuf<mcpt::DLightTri> light_tris; mcpt::DevBuf<double> light_cdf; mcpt::DevBuf<uint8_t> texels;
    mcpt::DevBuf<mcpt::DTri> fast_tris; mcpt::DevBuf<mcpt::CwNode> cw_nodes; mcpt::DevBuf<mcpt::DTriPre> fast_pre;
    mcpt_fast_info fast_info{};     // what mcpt_device_fast_hierarchy reports (node and triangle slot counts, builder, clusters, depth, stack need)
    int trace_mode = MCPT_TRACE_FAST;
    mcpt::DevBuf<int32_t> d_order;         // leaf -> .obj face (device build keeps it for read-back)
    mcpt_bvh_info bi{};
    // frame state
    int width = 0, height = 0;
    mcpt::DevBuf<double> dirs;             // W*H*3 primary directions
    bool dirs_ready = false;
    mcpt_lens lens{};                      // mcpt_device_set_lens (all zero: the reference's pinhole)
    mcpt::DevBuf<double> pos;              // W*H*3 image-plane points pos(i,j), made on the first frame under an active lens
    std::shared_ptr<const mcpt::EnvData> env;   // mcpt_device_set_environment (null: none); ds.env is its denv
    std::shared_ptr<mcpt::LightPickData> pick;  // mcpt_device_set_light_sampling (null: MCPT_LIGHTS_ALL); ds.pick is its dpick
    // render workspace
    mcpt::DevBuf<int32_t> pixels; int64_t n_pixels = 0; int part_key[4] = {-1, -1, -1, -1};
    mcpt::Event ev[4];
    mcpt::Stream look_stream;              // the host's looks at a path count travel here, so that they wait for the logic pass that wrote
    mcpt::Event look_ev;                   // the count and for nothing enqueued after it (the finishing kernel above all)
    mcpt::HostBuf<unsigned int> h_look;    // pinned host word the looks land in (never a pageable stack address: an async copy into
                                           // pageable memory goes through the runtime's pin-on-the-fly / staging paths)
    const mcpt_scene* scene = nullptr;     // the handle this device was created from (devices_created is given back in mcpt_device_free)
    // closest-hit and test entry points (mcpt_trace_closest*, mcpt_sample_radiance) have counters, queue words and a deferred-ray
    // list of their own: a frame in flight on another stream keeps using its frame slot's
    mcpt::DevBuf<mcpt::DCounters> aux_ctr; mcpt::DevBuf<mcpt::TraceQueue> aux_queue; mcpt::DevBuf<long long> aux_slow_list;
    size_t sample_budget_bytes = size_t(4) << 30;   // megakernel path: radiance staging buffer per chunk
    size_t wf_budget_bytes = 0;                     // path state + rays per frame slot; 0 = a share of the free HBM (MCPT_WORKSPACE_GB overrides)
    size_t wf_auto_budget = 0;                      // that share, asked for once (hipMemGetInfo costs a few hundred microseconds)
    // Everything a frame in flight owns.  Two slots: with MCPT_RENDER_PIPELINE consecutive frames alternate between them, so the
    // latency-bound tail of one frame (the finishing kernel's last long paths, the fold) overlaps the head of the next on another stream.
    struct FrameSlot {
        mcpt::DevBuf<mcpt::PrimaryHit> hits;
        mcpt::DevBuf<double> rad;                       // sized in bytes (a lens adds a hit flag per sample)
        mcpt::DevBuf<char> wf_ws;
        mcpt::DevBuf<int32_t> hit_slots;
        mcpt::DevBuf<mcpt::PrimarySurface> surf;        // first-vertex record per hit pixel of the chunk
        mcpt::DevBuf<uint8_t> cam_hit;                  // per-sample route of a lens: did the sample's camera ray hit (per chunk sample)
        mcpt::DevBuf<unsigned int> alive_base;          // shaded pixels before each group of 64 hit slots
        mcpt::DevBuf<mcpt::WfCounts> wf_counts;         // MCPT_WF_COUNT_SLOTS slots
        mcpt::DevBuf<mcpt::TraceQueue> queue;           // persistent trace kernels: chunk queue head + deferred-ray list
        mcpt::DevBuf<long long> slow_list;
        mcpt::DevBuf<char> path_area;                   // records and exact-walk stacks of the pool form of the finishing pass (finish_pool_bytes)
        mcpt::DevBuf<mcpt::DCounters> ctr;
        mcpt::Event done;                               // recorded after the slot's last kernel of a frame
        bool used = false;
        bool keeping = false;                           // ctr holds kept statistics of earlier frames (must not be cleared)
    } slot[2];
    int next_slot = 0;
    bool pipelined = false;                         // set by the first MCPT_RENDER_PIPELINE frame (sizes the workspace budget)
    // statistics kept on the device side until mcpt_device_collect_stats (MCPT_RENDER_KEEP_STATS)
    std::vector<EventPair> ev_pool;                 // start/stop pairs around trace launches
    size_t ev_used = 0;
    std::vector<EventPair> frame_ev;                // start/stop of every kept frame
    size_t frame_ev_used = 0;
    uint64_t kept_samples = 0, kept_primary = 0; int kept_launches = 0;
    unsigned int slow_cap = 1u << 20;
    mcpt::LaunchCfg cfg;                            // this GPU's resident grids and knobs
    long long finish_threshold = 500000;            // paths left at which the finishing pass takes over (MCPT_FINISH_PATHS; sweep: flat from 2e5 to 1e6)
    // Shared ownership, as a device holds its scene: the caller's handle and every progressive frame created on the device hold one
    // reference each; the device goes with the last of mcpt_device_free / mcpt_progressive_free.
    std::atomic<int> refs{1};
    // The camera the device renders from (create_dscene takes the scene's; mcpt_device_set_camera replaces it) and what geometry updates
    // need (update.cpp).  `upd` is made by the first mcpt_device_update_vertices: a device that is never updated holds none of it.
    mcpt::Vec3 cam_eye, cam_look_at, cam_up;
    double cam_fovy = 0;
    int32_t build_mode = MCPT_BUILD_HOST;
    struct Update {
        mcpt::DevBuf<double> v9, vn9, vt6, nrm3;        // the faces in .obj order: 216 B per face with the materials
        mcpt::DevBuf<int32_t> mat;
        mcpt::DevBuf<int32_t> leaf_of_face, slots, old_order, moved;
        // of the current culling hierarchy, made by the first refit of it and dropped by a rebuild:
        mcpt::DevBuf<int32_t> tri_faces;                // triangle slot -> .obj face
        mcpt::DevBuf<int32_t> sched;                    // the nodes grouped by depth
        std::vector<int> level_first;                   // level l = sched[level_first[l] .. level_first[l + 1])
        mcpt::DevBuf<double> node_box;                  // the nodes' exact boxes, 48 B per node
        std::vector<double> light_v;                    // the emitter faces' vertices the light tables were last made from
        mcpt::DevBuf<int32_t> light_faces;              // the emitter faces, light by light in material face order
        mcpt::DevBuf<double> light_buf;                 // their vertices, gathered on the GPU
        int n_light_faces = 0;
        double cost = -1;                               // the hierarchy's cost figure after the last update (< 0: not computed yet)
        float morton_lo[3], morton_span[3];
    };
    std::unique_ptr<Update> upd;
    // A motion (motion.cpp, mcpt_device_set_motion): key 0 is what the device held when it was set.  While a motion frame renders, and
    // until the next call that is not one, the geometry is a step's (away); the camera is back at key 0 whenever a frame or pass returns.
    struct Motion {
        mcpt_shutter shutter{};
        bool has_geometry = false, has_camera = false;
        mcpt::DevBuf<double> v0, v1;                    // both keyframes in the staging layout, 72 B per face each (has_geometry)
        mcpt_camera_key c0{}, c1{};                     // the cameras of key 0 and key 1
        mcpt::DCamera cam0{};                           // key 0's camera as the kernels read it
        bool away = false;                              // the geometry is step at_step's, not key 0's
        int at_step = -1;
        double cost0 = -1;                              // the culling hierarchy's cost figure at key 0
        mcpt_motion_info info{};                        // of the last motion frame or pass
        // what a one-shot motion frame folds through (a progressive handle has its own): moments, hit flags, hit counts under a lens
        mcpt::DevBuf<double> mom; mcpt::DevBuf<uint8_t> hit; mcpt::DevBuf<int32_t> hitcnt;
    };
    std::unique_ptr<Motion> motion;
    bool geometry_failed = false;                   // an update failed midway: nothing is traced or rendered until one succeeds
    // display transform (display_api.cpp): the luminance histogram's slots and their pinned copy, made on the first call that takes one
    mcpt::DevBuf<unsigned long long> disp_slots; mcpt::HostBuf<int64_t> h_disp_slots;
    // The seven workspaces below are kept between calls; a call holds one through its `done` event, by staging.hpp's lease.
    // lightmap baking (lightmap_api.cpp): what a bake keeps between its kernels, made by the first one and grown to the largest map so far
    struct Lightmap {
        mcpt::DevBuf<int32_t> owner[2], slot_of_face, big, block_counts, block_offsets, total;
        mcpt::DevBuf<unsigned int> n_big;
        mcpt::DevBuf<unsigned long long> masks;
        mcpt::DevBuf<int32_t> texels, hits;             // the covered texels' list and the query's answers, by list entry
        mcpt::DevBuf<int32_t> counts;                   // an adaptive bake: the queries' own sample counts, by list entry
        mcpt::DevBuf<double> q6, mean, err;
        mcpt::DevBuf<double> irr;                       // the dilation's second frame
        // an occlusion map (occlusion_api.cpp) shares the raster, the list, irr and `done` with the bakes and keeps its query's answers
        // by list entry, 48 bytes per covered texel: ao [c], stderr [c], bent [c][3]; hits [c], back [c]
        mcpt::DevBuf<double> occ;
        mcpt::DevBuf<int32_t> occ_cnt;
        // a direct-light map (direct_api.cpp) does the same and keeps, by list entry, irradiance [c][3], stderr [c][3], irradiance by
        // light [c][nl][3] and visibility by light [c][nl]: 48 + 32 nl bytes per covered texel
        mcpt::DevBuf<double> direct;
        mcpt::HostBuf<int32_t> h_total;                 // pinned word the covered count lands in
        mcpt::Event done;
        // the denoiser (lightmap_denoise_api.cpp) shares owner[], irr and `done` with the bakes and keeps, per texel of the largest map it
        // has seen, a 64-byte guide record and two 32-byte (e, v) records: 128 bytes
        mcpt::DevBuf<char> dn_guide, dn_buf[2];
    };
    std::unique_ptr<Lightmap> lm;
    // adaptive queries (adaptive_query_api.cpp): what a call keeps between its passes, made by the first one and grown to the longest
    // list so far
    struct AdaptiveQuery {
        mcpt::DevBuf<double> mom;                       // [n][2][3] the queries' moments, by position in the caller's list
        mcpt::DevBuf<int32_t> hitcnt, cnt;              // [n] hit counts and sample counts
        mcpt::DevBuf<int32_t> sel[2];                   // the active list (positions, ascending) and the next one
        mcpt::DevBuf<uint8_t> ones;                     // [n] the selection's hit bytes: a query has no miss rule
        mcpt::DevBuf<double> cq6;                       // the compact list of a pass
        mcpt::DevBuf<int32_t> cids;
        mcpt::DevBuf<unsigned long long> masks;
        mcpt::DevBuf<int32_t> block_counts, block_offsets, total;
        mcpt::HostBuf<int32_t> h_total;                 // pinned word the next list's length lands in
        mcpt::Event done;
    };
    std::unique_ptr<AdaptiveQuery> aq;
    // irradiance volumes (volume_api.cpp: volume_points_device, shared with the visibility grid bake): the positions of the grid a bake
    // answers, made by the first bake and grown to the largest grid so far
    struct Volume {
        mcpt::DevBuf<double> p3;                        // [nprobes][3]
        mcpt::Event done;
    };
    std::unique_ptr<Volume> vol;
    // probe visibility (visibility_api.cpp): the rays of a chunk of probes and their closest hits, made by the first bake and grown to the
    // largest chunk so far (hit_work.hpp), 84 bytes per ray; an occlusion query (occlusion_api.cpp) draws its rays into the same workspace
    // under the same lease
    struct Visibility : HitWork {
        mcpt::Event done;
    };
    std::unique_ptr<Visibility> vis;
    // baked frames (baked_api.cpp): the rays of a chunk and their closest hits (hit_work.hpp) and the chunk's shaded samples, made by the
    // first call and grown to the largest chunk so far, 116 bytes per ray
    struct Baked : HitWork {
        mcpt::DevBuf<double> rad;                       // [rays][3]
        mcpt::DevBuf<int32_t> kind, lit;                // [rays]
        mcpt::DevBuf<int32_t> slit;                     // [rays] a specular frame's lookups: 4 bytes per ray more, grown by those calls alone
        mcpt::Event done;
    };
    std::unique_ptr<Baked> baked;
    // reflection probes (reflection_api.cpp): the rays of a chunk of texels with their ids, and the query's answers to them, made by the
    // first bake and grown to the largest chunk so far, 80 bytes per ray
    struct Reflection {
        mcpt::DevBuf<double> rays6, mean;               // [rays][6], [rays][3]
        mcpt::DevBuf<int32_t> ids, hits;                // [rays]
        mcpt::Event done;
    };
    std::unique_ptr<Reflection> refl;
    // direct light (direct_api.cpp): the light table of a call (direct.hpp: DirectLight, 160 bytes a light) in a pinned copy, which the
    // caller's lights are turned into before the call returns, and the device copy the kernels read, grown to the longest table so far
    struct Direct {
        mcpt::HostBuf<char> h_lights;
        mcpt::DevBuf<char> lights;
        mcpt::Event done;
    };
    std::unique_ptr<Direct> direct;
};

// The helpers below are the library's own: none of them is exported from libmcpt.so.
#pragma GCC visibility push(hidden)

// ---- capi.cpp
int runtime_gate();                                 // what mcpt_device_create asks before it touches a device
// MCPT_ERR_NO_DEVICE unless a HIP device is visible (libmcpt has no CPU fallback); *visible: how many are
int require_device(int* visible = nullptr);

// ---- scene_api.cpp
void scene_release(const mcpt_scene* s);            // drops one reference to s
int trace_engine_for(long long t, const mcpt::Knobs& k);
// the culling hierarchy of h for the leaf order `order`, built on the first request and shared by every device of the scene
std::shared_ptr<const mcpt::FastBvh> shared_fast_bvh(const mcpt_scene* h, const std::vector<int32_t>& order, const mcpt::Knobs& k);
// p's tile partition (tiles of tile_w x tile_h, default 32 x 8, dealt over world ranks); MCPT_ERR_ARG when the rank is outside the world
struct TileShape { int tw, th, rank, world; };
int tile_shape(const mcpt_render_params* p, TileShape& t);
// the pixels (y * W + x, in scan order) that p's rank owns in a W x H frame; MCPT_ERR_ARG as tile_shape
int owned_pixels(int W, int H, const mcpt_render_params* p, std::vector<int32_t>& out);

// the host's SAH hierarchy over `faces` in leaf order `order`, private to the caller (MCPT_UPDATE_REBUILD: the scene's cache stays as it is)
std::shared_ptr<const mcpt::FastBvh> private_fast_bvh(const std::vector<mcpt::FaceRec>& faces, const std::vector<int32_t>& order, const mcpt::Knobs& k);

// ---- device.cpp
// MCPT_ERR_ARG while the device's last geometry update has failed midway
int geometry_gate(const mcpt_device* d);
// The fast walk's culling hierarchy of d's reference structures with d's builder: fills d->cw_nodes, d->fast_tris and d->fast_info.
// coords_ok / lo / hi: the vetting and the bounds of the coordinates; host_bvh: the host builder's tree (asked for by the host modes only).
int build_culling_hierarchy(mcpt_device* d, bool coords_ok, const double lo[3], const double hi[3],
                            const std::function<std::shared_ptr<const mcpt::FastBvh>()>& host_bvh, bool talk, double* absmax);
int create_pre_test(mcpt_device* d, double absmax);
inline bool fast_walk_enabled(const mcpt_fast_info& fi, bool coords_ok, double absmax)
{
    return coords_ok && fi.max_depth < mcpt::kFastMaxDepth && fi.cw_stack_need < mcpt::kFastMaxDepth && absmax >= 1e-15 && absmax <= 1e15;
}

// ---- update.cpp
int wait_for_frames(mcpt_device* d);                // nothing of the device is in flight afterwards
int stage_faces(mcpt_device* d);                    // the faces in .obj order become resident (d->upd), once
// MCPT_UPDATE_REFIT to the vertices d_v (device pointer, [t][9]) without the entry point's checks: the caller has waited for the frames
int refit_geometry(mcpt_device* d, const double* d_v, mcpt_update_info* info);
int camera_check(const double eye[3], const double look_at[3], const double up[3], double fovy);    // MCPT_ERR_ARG: not a camera
void camera_apply(mcpt_device* d, const double eye[3], const double look_at[3], const double up[3], double fovy);   // (checked, nothing in flight)

// ---- motion.cpp
int shutter_check(const mcpt_shutter* s);
// The geometry back at key 0 (one refit) when a motion frame has left it at a step: called by every entry point that is not a motion frame
// before it reads the device.  A device without a motion: nothing.
int motion_home(mcpt_device* d);
void motion_clear(mcpt_device* d);                  // drops the motion as it stands (the caller replaces what it left)
// Samples [k0, k0 + n) of an N-sample frame under d's motion, cut at the shutter's step boundaries: for every piece the device goes to the
// piece's step (blend, refit, camera) once st and the device's frames are idle, then run(first sample, count) renders it on st.  Returns
// with st idle, the camera at key 0 and d->motion->info describing the pieces.
int motion_passes(mcpt_device* d, int k0, int n, int N, hipStream_t st, const std::function<int(int, int)>& run);

// ---- environment.cpp
int env_check(const mcpt_environment* e);
int env_make(const mcpt_environment* e, std::shared_ptr<mcpt::EnvData>& out);   // tables + upload on the current device (e valid)

// ---- light_sampling.cpp
int light_sampling_check(const mcpt_light_sampling* ls);
int light_weights_check(const mcpt_light_sampling* ls, size_t num_lights);   // the weights' count and values (MCPT_ERR_ARG)
// the emitters have moved (areas[num_lights], the device's light records as they are now; d->upd->light_v, their vertices): default weights
// are made again, and so is the light tree of MCPT_LIGHTS_TREE
int light_pick_refresh(mcpt_device* d, const double* areas);

// ---- display_api.cpp
int display_check(const mcpt_display_params* p);    // MCPT_ERR_ARG: not display parameters (null: the defaults)
// The picture of pixels d_pixels[0 .. n) (null: pixels 0 .. n) of the frame d_img under p (checked), 3 or 4 bytes per pixel at each pixel's
// own place in d_out, on st: the histogram over the same pixels when p needs one (st is then waited for), and the map.
int display_frame_device(mcpt_device* d, const double* d_img, const int32_t* d_pixels, int64_t n, const mcpt_display_params* p, uint8_t* d_out,
                         mcpt_display_info* info, hipStream_t st);
int display_histogram_device(mcpt_device* d, const double* d_img, const int32_t* d_pixels, int64_t n, int64_t* slots, hipStream_t st);

// ---- query_api.cpp
// what every query call refuses of its sample range and count, and of its flags (MCPT_ERR_ARG)
int range_check(int32_t spp, int32_t sample_base, int64_t n);
int flags_check(int32_t flags);
// The query call itself, after the refusals: q's list, of q.kind, as the sample source of a render call on `stream` (device pointers
// throughout; d_ids null: entry i has id i).  stats (may be null) is cleared first; n == 0 launches nothing.
int query_device(mcpt_device* d, const mcpt::DQuery& q, const int32_t* d_ids, int64_t n, int32_t spp, int32_t sample_base, uint64_t seed, int32_t flags,
                 mcpt_stats* stats, void* stream);

// the refusals of mcpt_query_radiance's two forms, shared with the adaptive call (adaptive_query_api.cpp): the parameters, and the list itself
int query_params_check(const mcpt_query_params* p, int64_t n, const void* q6, const void* mean3);
int query_list_check(const double* q6, const int32_t* ids, int64_t n, int32_t kind);
// the refusals of mcpt_query_sh's two forms, shared with the volume bake (volume_api.cpp)
int sh_params_check(const mcpt_sh_params* p, int64_t n, const void* p3, const void* sh27);
// what the host-pointer forms refuse of a probe list itself, shared with the visibility bake (visibility_api.cpp)
int probe_list_check(const double* p3, const int32_t* ids, int64_t n);

// ---- volume_api.cpp (shared with visibility_api.cpp)
int volume_grid_check(const mcpt_volume_grid* g);   // what every call refuses of a grid, in the struct's field order
// what the host-pointer forms of a lookup refuse of the coefficients and the receivers themselves
int volume_arrays_check(const mcpt_volume_grid& g, const double* sh27, const double* q6, int64_t n);
// The grid's positions into the volume's own list (d->vol->p3) on st, for the bake that answers them: the list is the caller's until l ends
int volume_points_device(mcpt_device* d, const mcpt_volume_grid& g, hipStream_t st, Lease& l);

// ---- visibility_api.cpp (shared with baked_api.cpp)
int volume_visibility_check(const mcpt_volume_visibility* v);   // what every visibility-weighted lookup refuses of its knobs, in the struct's field order

// ---- reflection_api.cpp (shared with baked_specular_api.cpp)
int reflection_chain_check(const mcpt_reflection_chain* c);    // what every call refuses of a chain, in the struct's field order
int reflection_finite_check(const double* a, size_t count, const char* what);   // MCPT_ERR_ARG: a value of a[0 .. count) that is not finite

// ---- baked_api.cpp (shared with baked_specular_api.cpp)
namespace mcpt { struct BakedSpecular; }
int baked_source_check(const mcpt_baked_source* s);  // what every baked call refuses of its source, in the header's order
int baked_radiance_args_check(const void* rays6, int64_t n, int32_t flags, const mcpt_baked_outputs* o);
int baked_frame_args_check(const mcpt_baked_frame_params* p, const void* img);
// the device copies of a host-pointer source among the call's: `dev` is s with the device's pointers
int baked_source_upload(const mcpt_device* d, const mcpt_baked_source& s, Staging& S, mcpt_baked_source& dev);
// the baked radiance call and the baked frame on `st` after the refusals and the gate (device pointers throughout); spec null: the plain calls
int baked_radiance_device(mcpt_device* d, const mcpt_baked_source& s, const double* d_rays6, int64_t n, int32_t flags, const mcpt_baked_outputs& o,
                          const mcpt::BakedSpecular* spec, mcpt_stats* stats, hipStream_t st);
int baked_frame_device(mcpt_device* d, const mcpt_baked_source& s, const mcpt_baked_frame_params& fp, double* d_img, int32_t* d_counts3, int32_t* d_lit,
                       const mcpt::BakedSpecular* spec, mcpt_stats* stats, hipStream_t st);

// ---- lightmap_api.cpp
namespace mcpt { struct LightmapWork; }
int lightmap_size_check(int32_t width, int32_t height);             // MCPT_ERR_ARG: a size outside 1 .. 16384
int lightmap_chart_check(const double* uv6, int64_t num_faces);     // MCPT_ERR_ARG: a chart component that is not finite
// what every lightmap call on a device does before it reads the device's triangles: the device itself, key 0 of a motion, a geometry that stands
int lightmap_device_gate(mcpt_device* d);
// the baker's workspace of a W x H map on d (d->lm) for a call on st, once the bake or denoise before this one has left it
int lightmap_ensure_work(mcpt_device* d, int W, int H, mcpt::LightmapWork& w, hipStream_t st, Lease& l);
// step 1 on st and the number of covered texels, which the host waits for: 4 bytes back
int lightmap_raster_device(mcpt_device* d, const double* d_uv6, int W, int H, const mcpt::LightmapWork& w, hipStream_t st, int32_t& covered);
// Rounds 1 .. R of the dilation of a W x H map of `channels` doubles a texel on st: round r reads frame[at] and own[(r - 1) & 1] and writes
// the other frame and own[r & 1].  at: the frame round 1 reads, then the one round R wrote.
void lightmap_dilate_rounds(double* const frame[2], int32_t* const own[2], int W, int H, int R, int channels, int& at, hipStream_t st);
// A map the caller clears before the texel list is answered into it, and its size; a null map is skipped.
struct MapClear { void* map; size_t bytes; };
// The spine every map bake shares, after its refusals, on st: the gate, the baker's workspace, the raster and the covered count, the clear
// of d_map (channels doubles a texel) and of clears[0 .. n_clears), the covered texels' list, answer(texels, q6, covered, frame_at) -- which
// answers the list (stats are its to fill) and scatters into frame_at --, `dilate` rounds and the owner map (d_owner may be null).
using MapAnswer = std::function<int(const int32_t* texels, const double* q6, int32_t covered, double* frame_at)>;
int map_bake(mcpt_device* d, const double* d_uv6, int W, int H, int dilate, int channels, double* d_map, const MapClear* clears, int n_clears,
             int32_t* d_owner, mcpt_stats* stats, hipStream_t st, const MapAnswer& answer);

// ---- adaptive_query_api.cpp
// what the adaptive calls refuse of their adaptive parameters (MCPT_ERR_ARG)
int adaptive_params_check(const mcpt_adaptive_params* ap);
// The adaptive query call after the refusals, device pointers throughout: q's list in passes on `stream`, d_counts (may be null) the
// queries' own counts.  stats (may be null) is cleared first; n == 0 launches nothing.
int adaptive_query_device(mcpt_device* d, const mcpt::DQuery& q, const int32_t* d_ids, int64_t n, int32_t spp, int32_t sample_base, uint64_t seed,
                          int32_t flags, const mcpt_adaptive_params& ap, int32_t* d_counts, mcpt_stats* stats, void* stream);

// ---- render.cpp
inline bool lens_active(const mcpt_lens& l) { return l.flags != 0 || l.aperture > 0.0; }
int lens_check(const mcpt_lens* l);
int ensure_dirs(mcpt_device* d, hipStream_t st);    // the primary directions, made on first use
int ensure_pos(mcpt_device* d, hipStream_t st);     // the image-plane points camera_ray starts from (d->pos), made on first use
mcpt::DLens lens_for(const mcpt_device* d, const mcpt_lens& l);   // lens l on d's camera as the kernels read it (after ensure_pos)

// Which camera samples of every owned pixel a render call covers and where they are folded.  A frame: samples [0, N) through
// k_fold_samples (mom == null).  A progressive pass (mcpt_progressive_step): samples [k0, k0 + n) of a frame of N through
// k_fold_progressive, which continues the image's fold and the moments in mom.  n is the layout stride of the pass (WfArgs::spp):
// chunks are sized from it.
struct SampleRange {
    int k0, n, N;
    double* mom;
    uint8_t* hit;
    const mcpt_lens* lens;      // the lens of the call (the device's, or the one a progressive handle took); null: the pinhole
    int32_t* hitcnt;            // progressive passes under an active lens: per pixel, the samples whose camera ray hit
    const mcpt::EnvData* env;   // the environment of the call (the device's, or the one a progressive handle took); null: none
    bool motion = false;        // a piece of a motion frame (mom != null): a pixel's primary ray may hit in one step and miss in another
    // A radiance query (query_api.cpp): the call's slots are the entries of this list, not pixels -- sample k of slot s traces the list's
    // ray through the per-sample route and is folded into the list's own outputs (d_img, mom, hit, lens and hitcnt are not read; the
    // PixelList holds the ids, or null for the slot itself).  Null: a frame or a pass.
    const mcpt::DQuery* query = nullptr;
    // A pass of an adaptive query call (adaptive_query_api.cpp; host side, the pointers are the device's): `query` is the compact list of
    // the active queries and answers nothing itself -- the fold continues the moments and hit counts of the caller's positions
    // (k_query_fold_moments).  Null: a query call folds into its own outputs.
    const mcpt::QueryMoments* moments = nullptr;
};

// The pixels a render call covers, on the device: the partition's owned list (mcpt_render*, uniform progressive passes) or an adaptive
// frame's active list.  Slot s of the call renders pixel pixels[s].
struct PixelList {
    const int32_t* pixels;
    int64_t n;
};

int render_device_impl(mcpt_device* d, const SampleRange& r, const PixelList& L, const mcpt_render_params* p, double* d_img, mcpt_stats* stats,
                       hipStream_t st, int& slot_used);

#pragma GCC visibility pop
