/*
 * mcpt.h -- C ABI of libmcpt.so, the MI355X-native (gfx950 / HIP) replacement for the hot path of
 * Arieys/MonteCarloPathTracing:  render_scene -> generateImg -> ray_intersect/bvh_intersect -> shade.
 *
 * The reference has no FFI or plugin interface; its boundary is three free C++ functions.  Each entry
 * point below names the reference function it replaces (paths relative to the reference checkout):
 *
 *   mcpt_render_scene      <->  bool render_scene(std::string path, std::string filename, int N)   MTPC/MTPC.cpp:35-68
 *   mcpt_scene_load        <->  scene_data::read_scene + sort(compare) + BVH::BVH                 MTPC/MTPC.cpp:38-45,
 *                                                     MTPC/sceneManagement.cpp:264-274, MTPC/BVH.cpp:37-85
 *   mcpt_render[_device]   <->  void generateImg(scene_data&, BVH&, image&, int)                  MTPC/pathTracing.cpp:274-331
 *   mcpt_trace_closest[_device] <-> bool ray_intersect(Ray, scene_data&, BVH&, intersection&)      MTPC/pathTracing.cpp:382-390
 *   mcpt_quantize_rgb8 + mcpt_write_png <-> imshow(double*, W, H, filename, N) + svpng()           MTPC/MTPC.cpp:10-33, MTPC/svpng.inc:77
 *
 * Plain pointers and sizes only; the caller owns every buffer, the library owns the opaque handles.
 * All compute entry points run hand-written HIP kernels on an MI355X; there is NO CPU fallback: without a
 * HIP device they return MCPT_ERR_NO_DEVICE.  Functions return 0 on success or a negative MCPT_ERR_* code;
 * mcpt_last_error() gives the message for the calling thread.
 *
 * Semantics are the reference's (fp64 arithmetic in the reference's operation order, no FMA contraction)
 * with the documented seams D1..D8 of DESIGN.md (counter-based RNG instead of time(NULL) engines, stable
 * Morton sort, serial sample accumulation, CRLF stripping, no virtual-child aliasing, depth cap, texture
 * clamp, Ns/Ni defaults).
 *
 * Device pointers.  Every d_* argument (and every device pointer in a struct a _device form takes) need only be aligned to its element
 * type: 8 bytes for doubles, 4 for int32, 1 for bytes -- what a sub-allocator hands out.  The library reads exactly the documented extent
 * of each input and writes no input.  It writes exactly the documented extent of each output, in every word of it unless the entry says
 * otherwise (pixels a partition does not own, for instance), and nothing before or after it.  No answer depends on what an output held
 * before the call.  Where wider accesses are faster (the display map's four pixels per lane) the launcher takes them only when the
 * pointers allow it and a slower path otherwise; an entry point that truly needed more would refuse with MCPT_ERR_ARG and say so in its
 * block below, never misbehave silently.  tests/test_gpu_extents.py holds every device-pointer entry point to this, with each buffer
 * inside a larger allocation between two bands of a fill byte.
 */
#ifndef MCPT_H
#define MCPT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCPT_VERSION 105

#define MCPT_OK             0
#define MCPT_ERR_IO        -1   /* a scene/texture/output file could not be opened */
#define MCPT_ERR_PARSE     -2   /* malformed scene (face before usemtl, index out of range, light without material ...) */
#define MCPT_ERR_ARG       -3   /* bad argument */
#define MCPT_ERR_NO_DEVICE -4   /* no HIP device / ordinal out of range */
#define MCPT_ERR_HIP       -5   /* a HIP runtime call failed */
#define MCPT_ERR_NOMEM     -6

#define MCPT_MAX_DEPTH 64       /* shade() recursion cap (D6) */

typedef struct mcpt_scene  mcpt_scene;    /* host: scene_data + Morton-sorted faces + implicit BVH */
typedef struct mcpt_device mcpt_device;   /* one GPU's resident copy of a scene (SoA/record arrays in HBM) */

/* MTPC/BVH.h:29 (t, Nv, Nr, Nc, Lc, Lv, Level) */
typedef struct { int32_t t, Lc, Lv, Nc, Nv, Nr, Level; } mcpt_bvh_info;

typedef struct {
    int32_t num_faces, num_materials, num_lights, width, height;
    double eye[3], look_at[3], up[3], fovy;          /* MTPC/sceneManagement.h:150-156 */
    mcpt_bvh_info bvh;
} mcpt_scene_info;

typedef struct {
    uint64_t rays_primary, rays_shadow, rays_bounce; /* closest-hit queries actually traced */
    uint64_t node_visits, tri_tests;                 /* box tests / triangle tests executed */
    uint64_t shade_calls, samples;
    uint64_t shadow_skipped;                         /* shadow rays the reference traces although it never uses their answer
                                                        (light behind the surface, pathTracing.cpp:217); not traced here */
    uint64_t dom_rays, dom_node_visits, dom_tri_tests; /* the share of the above done inside the dominant kernel (k_wf_trace):
                                                        numerator of its roofline */
    double   ms_trace, ms_total;                     /* device time of the dominant kernel / whole call (HIP events) */
    int32_t  launches;                               /* launches of the dominant kernel */
    int32_t  max_depth;
} mcpt_stats;

typedef struct {
    int32_t  spp;            /* N_ray_per_pixel */
    uint64_t seed;           /* RNG seam key (D1) */
    /* pixel ownership: the frame is cut into tile_w x tile_h tiles; tile (tx, ty) belongs to rank
     * (tx + shift*ty) mod world, shift = first integer >= world/2 coprime with world (round-robin along a row, every
     * row starting on another rank).  world<=1 renders everything.  tile_w/h <= 0 -> 32 x 8. */
    int32_t  rank, world, tile_w, tile_h;
    int32_t  flags;          /* MCPT_RENDER_* */
} mcpt_render_params;

#define MCPT_RENDER_DEFAULT      0
#define MCPT_RENDER_MEGAKERNEL   2   /* one lane per camera sample, whole path in one kernel, reference-shaped walk
                                       (the first implementation; kept for A/B runs).  Default: wavefront pipeline. */
/* A renderer that produces a SEQUENCE of frames (mcpt_render_device only):
 *   MCPT_RENDER_KEEP_STATS  the frame's statistics stay on the device (counters accumulate, event pairs are recorded, nothing is
 *                           read back) until mcpt_device_collect_stats: the call returns without waiting for the frame.
 *   MCPT_RENDER_PIPELINE    consecutive frames use the device's two frame slots (path state, radiance, counters) in turn.  Called
 *                           on alternating streams, the latency-bound tail of frame i (the last long paths, the fold) then overlaps
 *                           the head of frame i+1.  The caller gives every frame in flight its own d_img. */
#define MCPT_RENDER_KEEP_STATS   4
#define MCPT_RENDER_PIPELINE     8

/* ---- general ---- */
int         mcpt_version(void);
const char* mcpt_last_error(void);
int         mcpt_device_count(void);                        /* number of HIP devices (0 without a GPU) */
const char* mcpt_build_id(void);                            /* 16 hex digits: hash of the sources this library was compiled from */
/* Which HIP runtime this process runs on (since 105).  libmcpt.so's kernels are built by one hipcc; the libamdhip64.so they run on is
 * whichever the process loaded first under that soname (a Python process that imported torch has the wheel's bundled copy).  The first
 * mcpt_device_create / mcpt_multi_create compares hipRuntimeGetVersion() with the HIP_VERSION the library was compiled against and
 * returns MCPT_ERR_HIP, naming both and the runtime's file, when major.minor differ -- unless mcpt_allow_runtime_mismatch(1) was called
 * (or MCPT_ALLOW_RUNTIME_MISMATCH=1 is set), which turns the refusal into one line on stderr.
 *   mcpt_hip_runtime_info : versions encoded as HIP_VERSION (major * 10^7 + minor * 10^5 + patch); path = the file the runtime was loaded from
 *   mcpt_hip_runtime_check: the comparison itself, a pure function (0 = compatible; msg receives the refusal's text) */
/* Every environment variable the library reads (since 105), one per line: "NAME | default | meaning".  The environment is parsed when a
 * device (or multi-device) handle is created and kept in the handle -- never inside a launch -- so two handles created under different
 * settings keep them; INTEGRATION.md section 7 is this table. */
const char* mcpt_knobs_describe(void);
int         mcpt_hip_runtime_info(int32_t* compiled, int32_t* runtime, char* path, int64_t cap);
int         mcpt_hip_runtime_check(int32_t compiled, int32_t runtime, const char* runtime_path, char* msg, int64_t cap);
void        mcpt_allow_runtime_mismatch(int32_t allow);

/* ---- scene (host) ---- */
/* Reads <path><filename>.obj/.mtl/.camera exactly like read_scene; textures named by map_Kd are looked up
 * relative to <path> first, then the cwd (reference: cwd only). */
int  mcpt_scene_load(const char* path, const char* filename, mcpt_scene** out);
/* The same with opt-in departures from the reference's reader; load_flags = 0 is mcpt_scene_load.
 * The reference's read_obj (MTPC/sceneManagement.cpp:76-189) takes the 2nd index of a face corner as the normal and the
 * 3rd as the texture coordinate, reads triangles only, ignores mtllib, and its Morton domain is the fixed cube [-1,4]^3
 * (MTPC/morton code.h:6-7). */
#define MCPT_LOAD_STANDARD_OBJ   1   /* corners v, v/vt, v//vn, v/vt/vn as the OBJ format defines them; relative (negative)
                                        indices; polygons fan-triangulated; any run of blanks separates fields; a corner
                                        without vn gets the face normal, without vt (0,0) */
#define MCPT_LOAD_MTLLIB         2   /* read the .mtl files named by the .obj's mtllib lines (next to the .obj);
                                        <filename>.mtl only when it names none */
#define MCPT_LOAD_MORTON_BOUNDS  4   /* Morton keys on the scene's bounding box (changes the leaf order, i.e. which of two
                                        equidistant triangles wins a tie; everything else is unchanged) */
int  mcpt_scene_load_ex(const char* path, const char* filename, int32_t load_flags, mcpt_scene** out);
/* Lifetime: a device (or mcpt_multi) created from a scene shares ownership of it -- the scene's memory goes with the last of
 * mcpt_scene_free and the mcpt_device_free / mcpt_multi_free of everything created from it, in any order.  After mcpt_scene_free the
 * caller's handle must not be passed to the library again. */
void mcpt_scene_free(mcpt_scene*);
/* The same scene_data from arrays instead of files (generated scenes: the 10 M-triangle stress scene would be ~1 GB of
 * .obj text).  Faces are given in the order the .obj would list them; Face::norm, Morton keys, per-material face
 * lists and light tables are derived exactly as read_obj / shade do. */
typedef struct {
    int64_t num_faces;
    const double*  v;               /* [num_faces][9]  v1 v2 v3 */
    const double*  vn;              /* [num_faces][9]  vn1 vn2 vn3 */
    const double*  vt;              /* [num_faces][6]  vt1 vt2 vt3, may be NULL (zeros) */
    const int32_t* material;        /* [num_faces] */
    int32_t num_materials;
    const double*  material_rec;    /* [num_materials][8]  Kd xyz, Ks xyz, Ns, Ni */
    const char* const* material_names;   /* may be NULL */
    int32_t num_lights;
    const int32_t* light_material;  /* [num_lights] material that emits (".camera" mtlname lines, in order) */
    const double*  light_radiance;  /* [num_lights][3] */
    double eye[3], look_at[3], up[3], fovy;
    int32_t width, height;
} mcpt_scene_desc;
#define MCPT_SCENE_DEFER_BUILD 1    /* leave Morton sort + BVH to the GPU (mcpt_device_create then builds on the device) */
int  mcpt_scene_create(const mcpt_scene_desc*, int32_t flags, mcpt_scene** out);
int  mcpt_scene_set_resolution(mcpt_scene*, int32_t width, int32_t height);   /* overrides .camera width/height */
int  mcpt_scene_get_info(const mcpt_scene*, mcpt_scene_info* out);
/* faces in .obj order: 27 doubles each = v1 v2 v3 vn1 vn2 vn3 (xyz) vt1 vt2 vt3 (uv) norm; any pointer may be NULL */
int  mcpt_scene_get_faces(const mcpt_scene*, double* geom27, int32_t* material, uint32_t* morton);
int  mcpt_scene_get_leaf_order(const mcpt_scene*, int32_t* leaf_to_face);     /* sorted (leaf) index -> .obj index */
/* Nr nodes in the reference's compact level order; box6 = max_x,max_y,max_z,min_x,min_y,min_z (sceneManagement.h:165-171) */
int  mcpt_scene_get_bvh_nodes(const mcpt_scene*, double* box6, int32_t* level, int32_t* leaf_face);
int  mcpt_scene_find_index(const mcpt_scene*, int32_t i, int32_t l);          /* BVH::findIndex, MTPC/BVH.cpp:99-104 */
/* rec8 = kd xyz, ks xyz, Ns, Ni; flags4 = has_map, map_width, map_height, light index or -1 */
int  mcpt_scene_get_material(const mcpt_scene*, int32_t m, char name[64], double rec8[8], int32_t flags4[4]);
int  mcpt_scene_get_light(const mcpt_scene*, int32_t i, char name[64], double radiance[3], int32_t* material, double* total_area);
uint32_t mcpt_morton_code(float x, float y, float z);                         /* getMortonCode, MTPC/morton code.cpp:22-32 */

/* Diagnostic: builds the fast closest-hit hierarchy (accel_build.cpp) on the host and reports its shape.
 * leaf_order[num_faces] (may be NULL) = reference leaf index held by every slot of its triangle list;
 * nesting_ok = 1 when every stored child box contains everything below it (what the culling argument needs). */
int  mcpt_scene_fast_bvh_stats(const mcpt_scene*, int32_t* n_nodes, int32_t* max_depth, int32_t* leaf_order, int32_t* nesting_ok);

/* ---- device ---- */
int  mcpt_device_create(const mcpt_scene*, int32_t device_ordinal, mcpt_device** out);
/* Where sort(scene.f, compare) + BVH::BVH (MTPC/MTPC.cpp:44-45) run: on the host (bvh_build.cpp) or on the GPU
 * (build_kernels.hip: Morton kernel, stable radix sort of (key, face), leaf records, one union kernel per level).
 * Both give bit-identical arrays; mcpt_device_get_* read the device's copy back for that comparison. */
#define MCPT_BUILD_HOST   0
#define MCPT_BUILD_DEVICE 1
/* MCPT_BUILD_DEVICE plus most of the fast walk's culling hierarchy built on the GPU: triangles sorted by a 63-bit Morton code on
 * the scene's bounds, every four consecutive ones under one compressed node (each triangle with its own box); only the tree over
 * those clusters (a quarter of the primitives) is built by the host's SAH builder.  2 s instead of 4 for a 10 M-triangle scene,
 * 1.3-1.5x the node visits per ray; results are identical (the hierarchy only culls). */
#define MCPT_BUILD_DEVICE_FAST 2
/* MCPT_BUILD_DEVICE with the culling hierarchy grown on the GPU at close to the quality of the host's SAH build: parallel
 * locally-ordered clustering (each cluster merges with the neighbour in Morton order that gives the smallest joint surface area) up to
 * subtrees of 4096 triangles, of bounded height and bounded box area, each collapsed on the GPU into compressed 4-wide nodes with
 * leaves of up to four triangles; the host's SAH builder only sees the clusters' boxes (3 272 for 10 M triangles).  0.8 s instead of
 * 2.1 for a 10 M-triangle scene, 7-12 % more walk time than on the host's tree; results are identical (the hierarchy only culls). */
#define MCPT_BUILD_DEVICE_SAH 3
int  mcpt_device_create_ex(const mcpt_scene*, int32_t device_ordinal, int32_t build_mode, mcpt_device** out);
int  mcpt_device_get_bvh_nodes(mcpt_device*, double* box6 /* Nr*6, may be NULL */, int32_t* leaf_face /* Nr, may be NULL */);
int  mcpt_device_get_leaf_order(mcpt_device*, int32_t* leaf_to_face);
/* Read-only view of the culling hierarchy the fast walk of a device walks (tests check its structure).  Two-call pattern: with
 * nodes and tri_faces NULL only *info is filled.  nodes[n_nodes] = the raw 64-byte compressed 4-wide records as the device holds
 * them (root = 0; per axis plane = p + q * 2^e, q in 0..255; child >= 0: node, MCPT_FAST_EMPTY: none, else a leaf
 * -1 - ((first << 4) | (count - 1)) over tri_faces[first .. first+count)); tri_faces[n_tris] = .obj face of each triangle slot. */
#define MCPT_FAST_BUILT_HOST        0   /* host SAH builder (MCPT_BUILD_HOST, MCPT_BUILD_DEVICE) */
#define MCPT_FAST_BUILT_DEVICE_FAST 1   /* MCPT_BUILD_DEVICE_FAST: Morton clusters on the GPU */
#define MCPT_FAST_BUILT_DEVICE_PLOC 2   /* MCPT_BUILD_DEVICE_SAH: clusters grown by PLOC on the GPU */
#define MCPT_FAST_BUILT_PLOC_FELL_BACK 3 /* MCPT_BUILD_DEVICE_SAH that left too many clusters: built as MCPT_BUILD_DEVICE_FAST */
typedef struct {
    int32_t n_nodes, n_tris;
    int32_t enabled;            /* 0: the fast walk is off on this device (coordinates or stack need out of range) */
    int32_t cw_stack_need;      /* worst-case walk stack entries the builder recorded */
    int32_t max_depth;          /* inner levels the builder recorded */
    int32_t builder;            /* MCPT_FAST_BUILT_* */
    int32_t clusters;           /* MCPT_FAST_BUILT_DEVICE_PLOC: clusters grown on the GPU; otherwise 0 */
    int32_t reserved;
} mcpt_fast_info;
int  mcpt_device_fast_hierarchy(const mcpt_device*, mcpt_fast_info* info, void* nodes, int32_t* tri_faces);
void mcpt_device_free(mcpt_device*);
/* Which walk the closest-hit queries use.  Both return identical results (tests/test_gpu_parity.py).
 *   MCPT_TRACE_FAST (default): SAH hierarchy over the reference's leaf boxes, conservative culling, distance pruning,
 *                              the reference's own fp64 leaf-box / triangle tests on every candidate;
 *   MCPT_TRACE_REFERENCE     : the reference's implicit Morton tree in the reference's visiting order
 *                              (bvh_intersect, MTPC/pathTracing.cpp:334-374), no pruning. */
#define MCPT_TRACE_FAST      0
#define MCPT_TRACE_REFERENCE 1
int  mcpt_device_set_trace_mode(mcpt_device*, int32_t mode);
/* Which closest-hit engine MCPT_TRACE_FAST runs (same tests on the same triangles, identical results): the voting engine (one ray per
 * lane in registers, csrc/trace_persistent.hpp) or the pool engine (the rays of a workgroup resident in LDS, csrc/trace_pool.hpp).  The
 * library picks by scene size -- the pool engine where the hierarchy stays in the caches and the walk is bound by instruction issue
 * (at most MCPT_POOL_MAX_TRIS triangles, default 131072) -- unless the environment says MCPT_TRACE_ENGINE=vote or =pool.
 * Returns what a device created for this scene now would use. */
#define MCPT_ENGINE_VOTE 0
#define MCPT_ENGINE_POOL 1
int  mcpt_scene_trace_engine(const mcpt_scene*);

/* ---- closest hit (ray_intersect) ---- */
/* rays: n x 6 doubles (origin xyz, direction xyz).  face[n] = .obj face index or -1, t[n], p[n*3], pn[n*3];
 * any output of the host-pointer form may be NULL.  It stages through HBM; the _device form takes device pointers
 * (d_pn may be NULL, the others are required) and a hipStream_t (NULL = default stream) and is asynchronous. */
int  mcpt_trace_closest(mcpt_device*, const double* rays, int64_t n, int32_t* face, double* t, double* p, double* pn, mcpt_stats* stats);
int  mcpt_trace_closest_device(mcpt_device*, const double* d_rays, int64_t n, int32_t* d_face, double* d_t, double* d_p, double* d_pn, void* stream);

/* ---- integrator (generateImg) ---- */
/* img: H*W*3 doubles, index (row*W + col)*3 + c (image::getIndex, sceneManagement.h:232-234).  Pixels this
 * rank does not own are left untouched.  stats may be NULL. */
int  mcpt_render(mcpt_device*, const mcpt_render_params*, double* img, mcpt_stats* stats);
int  mcpt_render_device(mcpt_device*, const mcpt_render_params*, double* d_img, mcpt_stats* stats, void* stream);
/* statistics of all MCPT_RENDER_KEEP_STATS frames since the last call (waits for them; counts summed, ms_trace = sum over
 * k_wf_trace launches, ms_total = sum of the frames' own durations -- pipelined frames overlap) */
int  mcpt_device_collect_stats(mcpt_device*, mcpt_stats* stats);
/* radiance of single camera samples: pix[n] = row*W+col, k[n] = sample index -> rgb[n*3] (test seam, host pointers) */
int  mcpt_sample_radiance(mcpt_device*, uint64_t seed, const int32_t* pix, const int32_t* k, int64_t n, double* rgb);
/* number of pixels owned by (rank, world) under the tile partition, and their indices (row*W+col, ascending) */
int64_t mcpt_owned_pixels(const mcpt_scene*, const mcpt_render_params*, int32_t* pixels /* may be NULL */);

/* ---- progressive frames (since the progressive-rendering change; no reference counterpart) ---- */
/* A frame of N = params->spp samples per pixel rendered in passes: mcpt_progressive_step(h, n) renders samples [done, min(done + n, N)) of
 * every pixel the handle owns (params->rank / world / tile_w / tile_h as mcpt_render; MCPT_RENDER_MEGAKERNEL honoured; MCPT_RENDER_PIPELINE
 * and MCPT_RENDER_KEEP_STATS refused with MCPT_ERR_ARG).  Every (pixel, sample) owns its RNG key and the passes continue the frame's
 * sequential float fold, so at done == N the image is mcpt_render's frame bit for bit, whatever the pass sizes were.  Beside the fold the
 * handle keeps, per pixel and channel, sum x and sum x^2 of the sample radiance in fp64 (k order).
 *   step   : n <= 0, or a step after done == N, returns MCPT_ERR_ARG; synchronous (the pass is finished when it returns).
 *   image  : host H*W*3 doubles; pixels the handle does not own keep the caller's values.  img = the current estimate: at done == N the
 *            float-folded frame itself, at done < N the fp64 mean sum_x / done (NOT the float fold, which is only complete at N; the two
 *            differ in the last float bits).  stderr_img (may be NULL; img may be NULL if stderr_img is not) = the standard error of that
 *            mean, sqrt(s^2 / done) with s^2 the unbiased sample variance (clamped at 0), per channel; 0 while done < 2.
 *            _device: the same into device buffers on `stream`, asynchronous.
 *   noise  : over the owned pixels whose primary ray hit, after `done` samples: sum_se2 = sum over pixels and channels of stderr^2,
 *            sum_mean2 = sum of mean^2, pixels = their number; rel_error = sqrt(sum_se2 / sum_mean2) (a relative RMS standard error),
 *            abs_rms = sqrt(sum_se2 / (3 pixels)).  Deterministic: the same bits on any MI355X and for any pass sizes that reach `done`.
 *            done < 2: rel_error = abs_rms = +inf and the sums 0.
 *   next_pass : the schedule render_scene uses (a pure function).  The first pass is min(N, 8); each later one doubles the samples done,
 *            min(N - done, done).  remaining_s = +inf: no time budget; otherwise a later pass is capped at floor(remaining_s / s_per_sample)
 *            (seconds per sample per pixel of the last pass), and 0 -- stop -- is returned when that cap is < 1 or remaining_s <= 0.  Also 0
 *            when done >= N.
 * A handle shares ownership of its device (as a device does of its scene): the device goes with the last of mcpt_device_free and the
 * mcpt_progressive_free of the handles created on it.  Without a HIP device create returns MCPT_ERR_NO_DEVICE. */
typedef struct mcpt_progressive mcpt_progressive;
typedef struct {
    int32_t done, spp;
    int64_t pixels;
    double rel_error, abs_rms, sum_se2, sum_mean2;
} mcpt_noise;
int  mcpt_progressive_create(mcpt_device*, const mcpt_render_params*, mcpt_progressive** out);
int  mcpt_progressive_step(mcpt_progressive*, int32_t n, mcpt_stats* stats /* may be NULL */);
int  mcpt_progressive_done(const mcpt_progressive*);
int  mcpt_progressive_noise(mcpt_progressive*, mcpt_noise* out);
int  mcpt_progressive_image(mcpt_progressive*, double* img, double* stderr_img);
int  mcpt_progressive_image_device(mcpt_progressive*, double* d_img, double* d_stderr, void* stream);
int  mcpt_progressive_next_pass(int32_t spp, int32_t done, double remaining_s, double s_per_sample);
void mcpt_progressive_free(mcpt_progressive*);

/* ---- adaptive frames (since the adaptive-sampling change): a progressive frame whose pixels stop on their own error estimate ---- */
/* mcpt_progressive_create_adaptive makes a progressive handle (step / done / noise / image / free as above) that keeps an active pixel
 * list, initially the owned list.  step(n) renders samples [done, min(done + n, N)) of the active pixels only, then decides on the GPU,
 * from each pixel's own moments, which of them continue; the list stays in ascending pixel order.  With k = done after the step, pixel p
 * stops when
 *     its primary ray missed (its value is +0.0 for any sample count), or
 *     k >= min_spp  and  se2 < rel2 * m2 + abs2,   where, in fp64 without contraction,
 *         rel2 = rel_target * rel_target,  abs2 = abs_target * abs_target,
 *         se2 = ((se2_0 + se2_1) + se2_2),  m2 = ((m_0 * m_0 + m_1 * m_1) + m_2 * m_2),
 *         m_c = s1_c / k,  se2_c = v_c / k with v_c = max((s2_c - s1_c * s1_c / k) / (k - 1), 0)   (the squared standard error above).
 * Pixels only ever leave the list, so all active pixels share the count `done` and a pixel that stopped at k holds exactly the uniform
 * frame's samples [0, k): its estimate and error are those of a uniform handle at done == k, bit for bit, and a pixel that reaches N
 * holds the one-shot frame's value.  With rel_target = abs_target = 0 only misses stop, and the frame is mcpt_render's bit for bit.
 * Stopping on the pixel's own variance estimate biases the estimate slightly (a pixel whose first samples happen to agree stops early);
 * targets of 0 remove the bias.  noise and image use every pixel's own count n_p: the estimate is the float fold at n_p == N, else
 * s1 / n_p; the error sqrt(se2(n_p)); noise sums over the owned hit pixels as above, each with its own n_p (done reports the last pass
 * boundary).  min_spp must be >= 2 (a value above N is taken as N), the targets finite and >= 0; MCPT_RENDER_PIPELINE and
 * MCPT_RENDER_KEEP_STATS are refused.  A step once the active list is empty, or at done == N, returns MCPT_ERR_ARG.
 *   active         : the pixels the next step renders; 0 when the frame is complete (an empty list, or done == N).
 *   active_pixels  : writes those pixels, ascending, to `pixels` (may be NULL) and returns their number (< 0: MCPT_ERR_*).
 *   sample_counts  : W*H int32: the samples each owned pixel holds (other entries are left as they are).
 * On a uniform handle (mcpt_progressive_create) active is the owned count until done == N, active_pixels the owned list, and every owned
 * pixel's count is done. */
typedef struct {
    double  rel_target, abs_target;
    int32_t min_spp;
    int32_t reserved;
} mcpt_adaptive_params;
int     mcpt_progressive_create_adaptive(mcpt_device*, const mcpt_render_params*, const mcpt_adaptive_params*, mcpt_progressive** out);
int64_t mcpt_progressive_active(const mcpt_progressive*);
int64_t mcpt_progressive_active_pixels(mcpt_progressive*, int32_t* pixels);
int     mcpt_progressive_sample_counts(mcpt_progressive*, int32_t* counts);

/* ---- first-hit AOVs and the denoiser (since the denoising change): a better image from a progressive frame's estimate ---- */
/* mcpt_progressive_aovs: auxiliary outputs of every owned pixel's primary hit, W*H int32 / doubles (normal, albedo: W*H*3), each pointer
 * may be NULL; other pixels are left as they are.  They do not depend on the samples: computed once, on the handle's first aovs or denoise
 * call (the primary rays of the owned pixels traced on the device's stream), kept with the handle and freed with it.
 *   material : the material of the hit triangle, -1 for a miss.
 *   depth    : the hit's ray parameter t (the primary direction is a unit vector); 0 on a miss.
 *   normal   : the interpolated normal of the hit, the barycentric blend of the vertex normals exactly as the closest hit forms it (the pn
 *              of mcpt_trace_closest: findGarCor's three quotients; shading's own blend multiplies by a reciprocal and may differ from it
 *              in the last bit), not normalised; 0 on a miss and on an emitter.
 *   albedo   : the diffuse colour Kd exactly as shading forms it, the texel / 255 (the .mtl's map_Kd) included; 0 on a miss and an emitter.
 * mcpt_progressive_denoise: an edge-avoiding a-trous wavelet filter (the spatial filter of SVGF) of the estimate, guided by the AOVs and
 * the per-pixel variance.  Host: W*H*3 doubles, pixels not owned keep the caller's values; _device: into a device buffer on `stream`,
 * asynchronous.  It works on uniform, adaptive and partitioned (rank / world) handles, reads the handle's state and never writes it.
 * THE DENOISED IMAGE IS BIASED: it trades variance for a bias towards the neighbours' values; the estimate and stderr of
 * mcpt_progressive_image are unchanged and stay unbiased.  Returns MCPT_ERR_ARG for done < 2, iterations outside 0..10, a sigma that is
 * negative or not finite, a non-zero reserved field.  params == NULL or all fields 0: the defaults.  Otherwise iterations is K as given
 * (0: no filtering) and a sigma of 0 is its default.  The filter, in fp64 without contraction, every sum in the order written:
 *   inputs   : per owned pixel p the estimate c_p (mcpt_progressive_image), the squared standard error se2_c of every channel from the
 *              moments (as mcpt_progressive_image, with the pixel's own count on an adaptive handle; 0 below two samples), the AOVs.
 *   surface  : p is a surface pixel when it is owned, material_p >= 0 and the material is not an emitter.  Every other pixel (not owned,
 *              miss, emitter) is output bit for bit as the estimate and is never a neighbour.
 *   demodulate: a_c = max(albedo_c, 0.01), e_c = c_c / a_c; lum(e) = (0.2126 e_0 + 0.7152 e_1) + 0.0722 e_2;
 *              v_p = sum_c ((w_c * w_c) * se2_c) / (a_c * a_c), w = (0.2126, 0.7152, 0.0722), channels in order.
 *   n^_p     : the normal AOV divided by its length sqrt((n_x n_x + n_y n_y) + n_z n_z); a zero normal stays 0.
 *   iteration i = 0 .. K-1, step s = 2^i, from (e, v) to (e', v'):
 *     g_p  = sum k_q v_q / sum k_q over the 3 x 3 window q = p + (dx, dy), dx, dy in -1..1 row-major, q inside the frame, a surface
 *            pixel with material_q == material_p; k_q = b[dx] b[dy], b = (1/4, 1/2, 1/4).
 *     taps : q = p + s (dx, dy) for dy, dx in -2..2, row-major; a tap counts when q is inside the frame, a surface pixel and
 *            material_q == material_p.
 *     w_pq = ((h[dx] h[dy]) N_pq) exp(-D_pq - L_pq),   h = (1/16, 1/4, 3/8, 1/4, 1/16),
 *            N_pq = max(0, (n^_p.x n^_q.x + n^_p.y n^_q.y) + n^_p.z n^_q.z)^128 by seven squarings, 1 at the centre tap,
 *            D_pq = |t_q - t_p| / (((sigma_z t_p) s) max(|dx|, |dy|)), 0 at the centre tap,
 *            L_pq = |lum(e_q) - lum(e_p)| / (sigma_l sqrt(g_p) + 1e-10).
 *     e'_p = (sum w_pq e_q) / sum w_pq per channel,  v'_p = (sum (w_pq w_pq) v_q) / (sum w_pq * sum w_pq).
 *   output   : a_c e_c after K iterations; K = 0: the estimate itself, bit for bit.
 * Defaults: K = MCPT_DENOISE_ITERATIONS, sigma_l = MCPT_DENOISE_SIGMA_L, sigma_z = MCPT_DENOISE_SIGMA_Z.  Every output is one GPU lane's
 * fixed-order sum: the same bits on any MI355X, on every call, for any pass schedule that reaches the same state. */
#define MCPT_DENOISE_ITERATIONS      5
#define MCPT_DENOISE_MAX_ITERATIONS  10
#define MCPT_DENOISE_SIGMA_L         2.0
#define MCPT_DENOISE_SIGMA_Z         0.05
typedef struct {
    int32_t iterations;         /* K (0 with both sigmas 0: the defaults) */
    int32_t reserved;           /* must be 0 */
    double  sigma_l, sigma_z;   /* 0 = the default */
} mcpt_denoise_params;
int mcpt_progressive_aovs(mcpt_progressive*, int32_t* material, double* depth, double* normal, double* albedo);
int mcpt_progressive_denoise(mcpt_progressive*, const mcpt_denoise_params*, double* img);
int mcpt_progressive_denoise_device(mcpt_progressive*, const mcpt_denoise_params*, double* d_img, void* stream);

/* ---- sample AOVs and the filter they guide (since the guided-denoising change): guides averaged over each pixel's camera samples ---- */
/* Under an active lens the first-hit AOVs above show a picture the frame does not: one hard surface per pixel where the frame mixes two at
 * an antialiased silhouette, razor-sharp edges inside the blur of what is out of focus, a miss where most of a pixel's samples hit.
 * mcpt_progressive_sample_aovs: for G camera samples per owned pixel (samples = G, 1 <= G <= the handle's spp; 0: min(spp,
 * MCPT_GUIDE_SAMPLES)) sample k = 0 .. G-1 gets the frame's own camera ray of (pixel, k) -- the handle's lens and seed, what mcpt_camera_rays
 * returns -- traced for its closest hit on the device's current walk and engine.  A sample is a MISS, an EMITTER hit (the hit material is a
 * light) or a SURFACE hit; a surface hit contributes its t, the diffuse colour kd and the normal pn of the first-hit AOVs, pn divided
 * by its length sqrt((x x + y y) + z z) (a zero normal contributes 0).  Per pixel, summed in k order in fp64 without contraction by one GPU
 * lane (no atomics):
 *   counts : 3 int32 per pixel, ns (surface), ne (emitter), nm (miss); ns + ne + nm = G.
 *   depth  : sum t / ns;   albedo : sum kd / ns per channel;   normal : sum pn^ / ns per component, not renormalised.  All 0 when ns == 0.
 * W*H*3 int32 / W*H / W*H*3 / W*H*3 doubles, each pointer may be NULL; pixels not owned keep the caller's values.  Kept with the handle per
 * G: a call with another G computes them again.  They depend on the lens, the seed and G, not on the samples rendered.  Without an active
 * lens the G rays of a pixel coincide and the AOVs are the first-hit ones (counts (G,0,0), (0,G,0) or (0,0,G)).
 * mcpt_progressive_denoise_guided: the filter of mcpt_progressive_denoise guided by them.  The first struct is that call's, with its rules
 * and defaults; mcpt_guide_params adds G and sigma_a (NULL or all 0: the defaults).  MCPT_ERR_ARG: samples outside 0..spp, reserved != 0,
 * sigma_a negative or not finite, whatever mcpt_progressive_denoise refuses (done < 2 among it), a handle under a motion (both calls).
 * Biased like that filter; reads the handle and never writes what the other calls return.  In fp64 without contraction, sums in the
 * order written:
 *   filtered : p is a FILTERED pixel when it is owned, ns_p > 0 and ne_p == 0.  Every other owned pixel is output bit for bit as the
 *              estimate and is never a neighbour; pixels not owned are not written.
 *   demodulate: cov = ns / G; m_c = max(cov * albedo_c, 0.01); e_c = c_c / m_c; v_p = sum_c ((w_c * w_c) * se2_c) / (m_c * m_c); c, se2,
 *              w and lum as in mcpt_progressive_denoise.
 *   n^_p     : the normal AOV divided by its length sqrt((n_x n_x + n_y n_y) + n_z n_z); a zero normal stays 0.  t_p: the depth AOV.
 *   iteration i = 0 .. K-1, step s = 2^i: g_p, the taps, h, b, N_pq, D_pq, L_pq, e'_p and v'_p as in mcpt_progressive_denoise, except
 *     that a window entry or tap counts when q is inside the frame and a filtered pixel (no material is compared), and
 *     w_pq = ((h[dx] h[dy]) N_pq) exp((-D_pq - L_pq) - A_pq),
 *     A_pq = ((|m_q0 - m_p0| + |m_q1 - m_p1|) + |m_q2 - m_p2|) / sigma_a, 0 at the centre tap.
 *   output   : m_c e_c after K iterations; K = 0: the estimate itself, bit for bit.
 * Defaults: G = min(spp, MCPT_GUIDE_SAMPLES), sigma_a = MCPT_DENOISE_SIGMA_A.  The same bits on any MI355X, on every call, for any pass
 * schedule that reaches the same state, under every trace engine. */
#define MCPT_GUIDE_SAMPLES     16
#define MCPT_DENOISE_SIGMA_A   0.2
typedef struct { int32_t samples, reserved; double sigma_a; } mcpt_guide_params;   /* 0 = default; reserved must be 0 */
int mcpt_progressive_sample_aovs(mcpt_progressive*, int32_t samples, int32_t* counts3, double* depth, double* normal, double* albedo);
int mcpt_progressive_denoise_guided(mcpt_progressive*, const mcpt_denoise_params*, const mcpt_guide_params*, double* img);
int mcpt_progressive_denoise_guided_device(mcpt_progressive*, const mcpt_denoise_params*, const mcpt_guide_params*, double* d_img, void* stream);

/* ---- camera lens (since the lens change; the reference has a pinhole and one primary ray per pixel) ---- */
/* The reference traces one primary ray per pixel, through the pixel's corner, and gives it to all N samples (pathTracing.cpp:297-308), so
 * every frame is aliased and nothing is out of focus.  A lens set on a device gives every camera sample (pixel, k) a camera ray of its own.
 *   uniforms : u0..u3 = words 0..3 of the Philox block with counter (pixel, k, 0xFFFF << 16 | 0, 'MCPT') and key = seed, each (w + 0.5) * 2^-32
 *              (the RNG seam of the path vertices at a depth no vertex has: uniform(seed, pixel, k, depth 0xFFFF, slot 0..3)).
 *   q        : pos(i,j), the reference's running-sum corner of pixel (i,j) (start_point - pdy*i, then + pdx once per column, the bits of the
 *              primary rays).  With MCPT_LENS_JITTER q = (pos(i,j) + pdx*u0) - pdy*u1: a uniform point of the pixel square whose top-left
 *              corner is the reference's point -- so a jittered image sits half a pixel right of and below the reference's corner-sampled one.
 *   pinhole  : aperture == 0: origin eye, direction normalize(q - eye).  Without jitter this is the reference's primary ray, bit for bit.
 *   thin lens: aperture > 0, l = |look_at - eye|, F = focus_distance (F <= 0: l).  Focal point f = eye + (q - eye) * (F / l); lens point
 *              o = (eye + x^ * (r cos phi)) + y^ * (r sin phi), r = aperture * sqrt(u2), phi = (2 pi) * u3 with the full-precision pi;
 *              x^ = screen_x_dir, y^ = the normalised up (the basis of the reference's image plane, pathTracing.cpp:285-288, not necessarily
 *              orthogonal to the view); the ray leaves o with direction normalize(f - o).  In focus is the reference's image plane scaled
 *              about the eye until it passes through the point at distance F along the eye -> look_at axis.
 *   shading  : unchanged.  The first vertex is shaded at depth 0 under the same rules and keys (a camera ray that reaches an emitter returns
 *              the light's radiance unweighted); a camera ray that misses gives a sample of radiance 0.  fp64, no contraction.
 * A lens is ACTIVE when it has a flag or aperture > 0.  Then mcpt_render*, MCPT_RENDER_MEGAKERNEL / PIPELINE / KEEP_STATS, partitions,
 * mcpt_sample_radiance, mcpt_multi_* and progressive / adaptive handles trace a camera ray per sample, and rays_primary counts those rays.
 * A progressive handle takes the device's lens when it is created (a later set_lens leaves it as it is).  Per pixel the handle counts the
 * samples whose camera ray hit something; "the pixel's primary ray missed" (noise sums, the adaptive rule's immediate stop, the zero pixels
 * of the fold) then means: that count is 0.  With a pinhole the count is 0 or `done`, which is the rule above.  The first-hit calls
 * (mcpt_progressive_aovs, mcpt_progressive_denoise) keep the guides of the pixel's unjittered pinhole ray and their pass-through rule; guides
 * that follow the lens are the sample AOVs above (mcpt_progressive_sample_aovs, mcpt_progressive_denoise_guided).
 * MCPT_LENS_PER_SAMPLE alone traces a camera ray per sample although all rays of a pixel coincide: the same frame, bit for bit, through the
 * per-sample route (an A/B and test seam).  Errors (MCPT_ERR_ARG): unknown flag bits, reserved != 0, aperture negative or not finite,
 * focus_distance not finite.  With a NULL device and valid arguments: MCPT_ERR_NO_DEVICE without a GPU, as the other entry points. */
#define MCPT_LENS_JITTER      1   /* uniform over the pixel square (antialiasing) */
#define MCPT_LENS_PER_SAMPLE  2   /* trace a camera ray per sample even when all of a pixel's rays coincide (A/B and test seam) */
typedef struct { int32_t flags; int32_t reserved; double aperture; double focus_distance; } mcpt_lens;
int mcpt_device_set_lens(mcpt_device*, const mcpt_lens*);   /* NULL = the reference pinhole */
int mcpt_device_get_lens(const mcpt_device*, mcpt_lens*);
/* test seam: the camera rays of samples (pix[i], k[i]) under the device's lens (active or not) -> rays6[n*6] = origin xyz, direction xyz */
int mcpt_camera_rays(mcpt_device*, uint64_t seed, const int32_t* pix, const int32_t* k, int64_t n, double* rays6);

/* ---- environment light (since the environment change; the reference lights a scene with its emissive triangles only) ---- */
/* An ENVIRONMENT is a latitude-longitude RGB radiance map of W x H texels (W, H >= 1), top row first, every texel finite and >= 0; scale > 0
 * multiplies the radiance.  A 1x1 map is a constant sky.  Without one, a ray that leaves the scene brings 0, as in the reference.
 *   frame: world +Y is up.  Row i covers cos(theta) in [c[i+1], c[i]], c[i] = cos(pi i / H) in fp64 on the host, c[0] = 1, c[H] = -1;
 *     column j covers phi in [2 pi j / W, 2 pi (j+1) / W); a direction is (sin(theta) cos(phi), cos(theta), sin(theta) sin(phi)).
 *   lookup Le(d), nearest texel: phi = atan2(d.z, d.x) (+ 2 pi if negative), j = min(W-1, floor((phi * W) / (2 pi))); i = the row with
 *     c[i+1] < y <= c[i] (the last row also takes y = -1), y = d.y clamped to [-1, 1], found by binary search in c; Le(d) = scale * texel(i, j).
 *   sampling tables (host, fp64): w_ij = lum_ij * omega_ij, lum = (0.2126 r + 0.7152 g) + 0.0722 b, omega_ij = ((c[i] - c[i+1]) * 2 pi) / W;
 *     per row the running sums of w_ij left to right (the conditional CDF), over the rows the running sums of each row's last entry (the
 *     marginal CDF); Z = the marginal's last entry.  Z == 0: the environment is INACTIVE and everything is as without one.
 *   a draw from uniforms u0..u3: row i = first i with u0 * Z < marg[i], column j = first j with u1 * rowsum_i < cond[i][j] (binary
 *     searches); cos(theta) = c[i] + (c[i+1] - c[i]) * u2, sin(theta) = sqrt(max(0, 1 - cos^2)), phi = (2 pi (j + u3)) / W;
 *     pdf = lum_ij / Z per unit solid angle (constant over the texel: no Jacobian).  A 1x1 map draws uniformly over the sphere.
 *   light sample at a vertex p with normal pn and diffuse colour kd, after the scene's lights, from Philox block nl + 2 of the vertex's
 *     depth (nl = the scene's lights; every other draw is unchanged): direction d, k = d . pn; !(k > 0): no shadow ray.  Otherwise a shadow
 *     ray from p + 0.01 d along d that must leave the scene, contributing c = (kd * Le) * (((k / |pn|) / pi) / pdf) per channel.
 *   rays that leave the scene: a camera ray brings Le(d), unweighted; a SPECULAR or TRANSMISSION bounce ray adds T' * Le(d), T' = T * w / 0.6
 *     the throughput the next vertex would have had; a DIFFUSE bounce ray adds nothing (light sampling covers the diffuse lobe, as for
 *     emitters, pathTracing.cpp:247-261).  A pixel whose primary ray missed folds Le(primary direction) for each of its N samples through
 *     the frame's float fold; it keeps a standard error of 0 and stays out of the noise sums and an adaptive frame's active list.
 * Every pipeline (wavefront, MCPT_RENDER_MEGAKERNEL, lenses, partitions, progressive and adaptive handles) renders the same frame under it.
 * A progressive handle takes the device's environment when it is created.  AOVs and the denoiser treat a missed pixel as before. */
typedef struct { int32_t width, height; const float* rgb; double scale; int32_t flags, reserved; } mcpt_environment;
/* NULL clears it; the device copies the texels.  MCPT_ERR_ARG: a size < 1, a texel that is NaN, inf or < 0, scale not finite or <= 0, flags or
 * reserved != 0. */
int mcpt_device_set_environment(mcpt_device*, const mcpt_environment*);
/* width = height = 0 when there is none; Z = 0 when it is inactive.  Any pointer may be NULL. */
int mcpt_device_get_environment(const mcpt_device*, int32_t* width, int32_t* height, double* scale, double* Z);
/* test seams: rgb[n*3] = Le(dirs[i]) under the device's environment; the draw of vertex `depth` of camera samples (pix[i], k[i]) ->
 * dirs[n*3], pdf[n], rgb[n*3] (the radiance of the drawn texel).  MCPT_ERR_ARG without an active environment.  A copy that cannot be
 * allocated: MCPT_ERR_NOMEM, and the device stays usable. */
int mcpt_environment_eval(mcpt_device*, const double* dirs, int64_t n, double* rgb);
int mcpt_environment_sample(mcpt_device*, uint64_t seed, const int32_t* pix, const int32_t* k, int32_t depth, int64_t n, double* dirs, double* pdf,
                            double* rgb);
/* a PFM file (the format mcpt_write_pfm writes; 'PF' colour only) -> its size and, when rgb is not NULL, w*h*3 floats top row first (cap:
 * floats rgb holds; too few: MCPT_ERR_ARG).  MCPT_ERR_IO: no file; MCPT_ERR_PARSE: not a colour PFM. */
int mcpt_read_pfm(const char* file, int32_t* width, int32_t* height, float* rgb, int64_t cap);

/* ---- light sampling: one shadow ray per vertex from a weighted light pick (no reference counterpart) ---- */
/* MCPT_VERSION stays 105 with this block, as it did with the environment, update and motion blocks: a binder detects these entry points by
 * symbol (dlsym of mcpt_device_set_light_sampling), not by the version number. */
/* MCPT_LIGHTS_ALL, the default and the reference's loop: every vertex samples every light of the scene, one shadow ray each.
 * MCPT_LIGHTS_ONE: every vertex picks ONE light l with probability p_l, samples it as MCPT_LIGHTS_ALL samples light l (the same Philox
 * block l, area range and visibility rule; no light before it to inherit a material from) and scales the contribution by 1 / p_l.  The
 * bounce draws do not depend on the lights, so the paths -- geometry, throughput, emitter hits -- are the same in both modes, sample for
 * sample; only the direct light at the vertices differs, with the same expectation.  An active environment keeps its own shadow ray.
 *   table (host, fp64): weights w_l >= 0; cdf[l] = the running sum w_0 + ... + w_l, left to right; Z = cdf[nl-1]; pdf[l] = w_l / Z; the
 *     kernels scale by the quotient 1.0 / pdf[l], formed on the host.  Default weights: w_l = lum(radiance_l) * total_area_l,
 *     lum = (0.2126 r + 0.7152 g) + 0.0722 b; if every one of them is 0 (or not finite), w_l = 1.  A device whose emitters an update moves
 *     makes its default weights again from the new areas.
 *   the caller's weights: one per light of the scene, finite and >= 0, not all 0 (else MCPT_ERR_ARG).  A light of weight 0 is never
 *     picked: the estimator then leaves that light's direct light out, and keeping it unbiased is the caller's business.
 *   pick at vertex `depth` of a camera sample: u = slot 0 of Philox block nl + 3 of that depth (nl = the scene's lights; the lights use
 *     blocks 0..nl-1, the bounce nl and nl+1, the environment nl+2: every other draw keeps its value); x = u * Z; l = the smallest l with
 *     x < cdf[l], by binary search, clamped to the last light of non-zero weight.
 * A scene with no light or one light renders the same bits in both modes.  The setting is device state: every frame, progressive or
 * adaptive pass, motion frame and (pixel, sample) query that follows uses it (a progressive frame should not see it change between its
 * passes).  The megakernel counts a picked light behind the surface as shadow_skipped and traces no ray for it. */
/* MCPT_LIGHTS_TREE: as MCPT_LIGHTS_ONE -- one light per vertex, the same draw (slot 0 of block nl + 3), the same sample of the picked light,
 * scaled by 1 / p -- but the probability depends on the vertex (p, pn): a binary tree over the lights is descended from the root, and at
 * every node the two children are weighed by distance and horizon.
 *   tree (host, fp64): a leaf per light, its box the exact min / max of the light's triangle vertices, its weight the table's w_l (the same
 *     defaults, the same caller's weights, the same refusals).  Inner nodes top-down: the node's lights are ordered by box centre
 *     (lo + hi) * 0.5 along the widest axis of those centres' bounds (the lowest axis among equals), ties by light index; the first
 *     ceil(n / 2) go left.  An inner node's box is the union of its children's, its weight W_left + W_right.  Nodes are numbered in
 *     preorder (root 0, the left subtree right after its parent).  Record, 64 bytes: double lo[3], hi[3], w; int32 left, right (inner
 *     node: the children's indices; leaf: both ~light).  A device whose emitters an update or a motion step moves makes the tree again.
 *   importance of a node seen from (p, pn), with c = (lo + hi) * 0.5, h = (hi - lo) * 0.5:  0 if s = (c - p) . pn + h . |pn| is below
 *     -1e-9 * (|pn.x| + |pn.y| + |pn.z|) * (|p|inf + |c|inf + |h|inf) (the whole box lies below the vertex's horizon), else
 *     W / max(1, |c - p|^2, |h|^2).  Only + - * / and comparisons, sums left to right: host and device give the same bits.
 *   descent: at a node with children L, R: both importances 0 -> their weights stand in; I_R == 0 -> left, I_L == 0 -> right, with
 *     probability 1; else pL = I_L / (I_L + I_R), u < pL ? (left, u = u / pL, pdf *= pL) : (right, u = (u - pL) / (1 - pL), pdf *= 1 - pL).
 *     At the leaf the contribution is scaled by 1.0 / pdf.  A light of weight 0 is never picked; a light that can contribute has s above
 *     the margin at every ancestor, hence a positive probability: the estimator is unbiased as MCPT_LIGHTS_ONE's is.
 * A scene of fewer than two lights holds no tree and renders the MCPT_LIGHTS_ALL bits.  Under MCPT_LIGHTS_TREE mcpt_device_get_light_sampling
 * reports the ROOT's distribution w_l / Z (the table's); the per-vertex probabilities come from mcpt_scene_light_tree_pdf (host) and
 * mcpt_light_pick_at (device), and mcpt_light_pick, which has no vertex, is refused (MCPT_ERR_ARG). */
#define MCPT_LIGHTS_ALL 0
#define MCPT_LIGHTS_ONE 1
#define MCPT_LIGHTS_TREE 2
typedef struct { int32_t mode, num_weights; const double* weights; } mcpt_light_sampling;   /* num_weights 0 / weights NULL: the default weights */
/* NULL means MCPT_LIGHTS_ALL.  mode: MCPT_LIGHTS_ALL, MCPT_LIGHTS_ONE or MCPT_LIGHTS_TREE.  MCPT_ERR_ARG: an unknown mode, num_weights != 0 that is not the scene's light count, bad weights. */
int mcpt_device_set_light_sampling(mcpt_device*, const mcpt_light_sampling*);
/* *mode and pdf[num_lights] (each may be NULL): the table's probabilities; 1 for every light under MCPT_LIGHTS_ALL; under MCPT_LIGHTS_TREE
 * the root's distribution w_l / Z -- what a vertex really uses comes from mcpt_scene_light_tree_pdf and mcpt_light_pick_at */
int mcpt_device_get_light_sampling(const mcpt_device*, int32_t* mode, double* pdf);
/* host only (no GPU needed): the table of the scene's lights under `weights` (NULL: the default weights) -> cdf[num_lights], pdf[num_lights].
 * MCPT_ERR_ARG: a scene without lights, bad weights. */
int mcpt_scene_light_pick_table(const mcpt_scene*, const double* weights_or_null, double* cdf, double* pdf);
/* test seam: the pick at vertex `depth` of camera samples (pix[i], k[i]) -> light[n], pdf[n].  MCPT_ERR_ARG unless the device picks
 * (MCPT_LIGHTS_ONE on a scene of two or more lights).  A copy that cannot be allocated: MCPT_ERR_NOMEM, and the device stays usable. */
int mcpt_light_pick(mcpt_device*, uint64_t seed, const int32_t* pix, const int32_t* k, int32_t depth, int64_t n, int32_t* light, double* pdf);
/* host only (no GPU needed): the light tree of the scene under `weights` (NULL: the default weights), exactly as a device uploads it ->
 * *n_nodes (2 * num_lights - 1) and, unless NULL, nodes[*n_nodes] 64-byte records.  MCPT_ERR_ARG: fewer than two lights, bad weights. */
int mcpt_scene_light_tree(const mcpt_scene*, const double* weights_or_null, int32_t* n_nodes, void* nodes);
/* host only: the probability of every light at n vertices p[n][3] with normals pn[n][3] -> pdf[n][num_lights]; the host walks the same
 * tree with the same arithmetic as the device.  MCPT_ERR_ARG as above. */
int mcpt_scene_light_tree_pdf(const mcpt_scene*, const double* weights_or_null, const double* p, const double* pn, int64_t n, double* pdf);
/* test seam: the light the path kernels pick at the vertex (p[i], pn[i]) at `depth` of camera sample (pix[i], k[i]), and its probability
 * -> light[n], pdf[n].  MCPT_ERR_ARG unless the device picks by tree (MCPT_LIGHTS_TREE on a scene of two or more lights).  A copy that
 * cannot be allocated: MCPT_ERR_NOMEM, and the device stays usable. */
int mcpt_light_pick_at(mcpt_device*, uint64_t seed, const int32_t* pix, const int32_t* k, int32_t depth, const double* p, const double* pn, int64_t n,
                       int32_t* light, double* pdf);

/* ---- integrator over several GPUs of one node (no reference counterpart: generateImg is single-process OpenMP) ---- */
/* The frame is cut into tiles dealt to the GPUs exactly as mcpt_render_params.rank/world describe (rank r = devices[r]); the scene
 * is resident on every GPU; one host thread per GPU renders its tiles; at the end of the frame every rank's pixels travel as one
 * compact buffer into devices[0]'s HBM and are put at their frame positions there.  Every (pixel, sample) owns its RNG key, so the
 * frame is bit-identical for any number of GPUs (and to mcpt_render).  An ordinal may appear more than once in devices[] (several
 * ranks sharing a GPU: how the exchange is tested on a one-GPU box; MCPT_GATHER_PEER only). */
typedef struct mcpt_multi mcpt_multi;
#define MCPT_GATHER_PEER 0   /* hipMemcpyPeerAsync into devices[0] (over xGMI between the GPUs of a node) */
#define MCPT_GATHER_RCCL 1   /* ncclSend / ncclRecv in one group (librccl.so is loaded at mcpt_multi_create); distinct ordinals only */
/* devices == NULL or num_devices <= 0: every visible GPU.  build_mode as mcpt_device_create_ex (MCPT_BUILD_HOST needs a host build). */
int  mcpt_multi_create(const mcpt_scene*, const int32_t* devices, int32_t num_devices, int32_t build_mode, int32_t gather, mcpt_multi** out);
int  mcpt_multi_num_devices(const mcpt_multi*);
/* generateImg on all the GPUs: img = H*W*3 doubles on the host (every pixel is written); params->rank/world are ignored.
 * stats (may be NULL): counts summed over the GPUs, ms_total = slowest GPU + exchange, ms_trace = slowest GPU's. */
int  mcpt_multi_render(mcpt_multi*, const mcpt_render_params*, double* img, mcpt_stats* stats);
/* the same, leaving the frame in devices[0]'s HBM: *d_img (owned by the handle, valid until the next call) */
int  mcpt_multi_render_device(mcpt_multi*, const mcpt_render_params*, double** d_img, mcpt_stats* stats);
/* With MCPT_RENDER_KEEP_STATS in params->flags the GPUs keep their statistics (stats is left zero; nothing is read back inside the
 * frame); mcpt_multi_collect_stats sums what has gathered since the last call over the GPUs (ms_trace / ms_total: the slowest GPU's). */
int  mcpt_multi_collect_stats(mcpt_multi*, mcpt_stats* stats);
/* How the last frame's time divides (HIP events on each GPU's own stream): render_ms[num_devices] = each rank's render;
 * *gather_ms = from devices[0]'s own render being done to the last rank's pixels being in place in its HBM; *comm_ranks = the
 * number of ranks the RCCL communicator reports (0 with MCPT_GATHER_PEER).  Any pointer may be NULL. */
int  mcpt_multi_last_timing(const mcpt_multi*, double* render_ms, double* gather_ms, int32_t* comm_ranks);
void mcpt_multi_free(mcpt_multi*);
int  mcpt_multi_set_lens(mcpt_multi*, const mcpt_lens*);     /* every device of the group (NULL: the pinhole) */
int  mcpt_multi_set_environment(mcpt_multi*, const mcpt_environment*);   /* every device of the group (NULL: none) */
int  mcpt_multi_set_light_sampling(mcpt_multi*, const mcpt_light_sampling*);   /* every device of the group (NULL: MCPT_LIGHTS_ALL); a refused argument changes no device */

/* ---- one process per GPU (since 105; no reference counterpart) ---- */
/* The same exchange between the PROCESSES of a launch: every rank is a process that drives one GPU through mcpt_device_* (params->rank /
 * world = its place in the launch), and at the end of a frame the ranks' pixels travel over an RCCL communicator into rank 0's frame.
 * Rank 0 asks mcpt_comm_unique_id for RCCL's 128-byte id and hands it to the other ranks by whatever channel the launcher offers
 * (montecarlopathtracing_amd/procs.py: a file keyed by the launcher's process id); every rank then calls mcpt_comm_create.  No torch in
 * the process: the ranks run on the HIP runtime libmcpt.so was compiled against (see mcpt_hip_runtime_check) and /opt/rocm's librccl.
 *   mcpt_comm_gather_frame: d_frame = this rank's frame on its GPU (H*W*3 doubles, only its own pixels written); on return rank 0's holds
 *                           every pixel.  tile_w / tile_h of params select the partition; stream = the stream the frame was rendered on.
 *   mcpt_comm_allreduce   : v[n <= 64] on the host, summed (op 0) or maximised (op 1) over the ranks in place; n = 0: a barrier. */
typedef struct mcpt_comm mcpt_comm;
int  mcpt_comm_unique_id(uint8_t* id, int64_t cap /* >= 128 */);          /* returns the number of bytes written (128) or an error */
int  mcpt_comm_create(int32_t device_ordinal, int32_t rank, int32_t world, const uint8_t* id, int64_t id_bytes, mcpt_comm** out);
int  mcpt_comm_size(const mcpt_comm*);                                     /* ranks the RCCL communicator reports */
int  mcpt_comm_gather_frame(mcpt_comm*, const mcpt_scene*, const mcpt_render_params*, double* d_frame, void* stream);
int  mcpt_comm_allreduce(mcpt_comm*, double* v, int32_t n, int32_t op);
void mcpt_comm_free(mcpt_comm*);

/* ---- output (imshow + svpng) ---- */
int  mcpt_quantize_rgb8(const double* img, int64_t n, uint8_t* rgb8);        /* (unsigned char)clamp(v*255,0,255) */
int  mcpt_write_png(const char* file, const uint8_t* rgb8, int32_t width, int32_t height);
int64_t mcpt_png_encode(const uint8_t* rgb8, int32_t width, int32_t height, uint8_t* out, int64_t cap);

/* Output beyond svpng.  mcpt_png_encode_deflate / mcpt_write_png_deflate: the same 8-bit RGB picture as a
 * compressed PNG (per-row filter choice + deflate).  mcpt_write_pfm: img = double[h*w*3] as generateImg leaves it, written as
 * a little-endian fp32 Portable Float Map (bottom row first), no clamp.  Checkpoints: the fp64 frame plus the finished ones
 * of `parts` tile partitions (mcpt_render_params.rank/world = part/parts); load returns MCPT_ERR_IO when there is no file
 * and MCPT_ERR_PARSE when the file belongs to another frame (size, spp, seed, parts or scene differ). */
int64_t mcpt_png_encode_deflate(const uint8_t* rgb8, int32_t width, int32_t height, uint8_t* out, int64_t cap);
int  mcpt_write_png_deflate(const char* file, const uint8_t* rgb8, int32_t width, int32_t height);
int  mcpt_write_pfm(const char* file, const double* img, int32_t width, int32_t height);
int  mcpt_checkpoint_save(const char* file, const mcpt_scene* scene, const double* img, int32_t spp, uint64_t seed, int32_t parts, const uint8_t* done);
int  mcpt_checkpoint_load(const char* file, const mcpt_scene* scene, double* img, int32_t spp, uint64_t seed, int32_t parts, uint8_t* done);

/* Texture input (what the reference gets from cv::imread, MTPC/sceneManagement.h:137): decodes a baseline or progressive
 * JFIF file into an 8-bit BGR raster (rows x cols x 3).  With bgr == NULL only the size is returned. */
int  mcpt_decode_jpeg(const char* file, int32_t* width, int32_t* height, uint8_t* bgr, int64_t cap);

/* ---- whole program (render_scene) ---- */
/* Reads <path><filename>.*, renders with N samples per pixel on GPU 0 (or the GPUs named by the options) and writes
 * "../result/<filename>-SPP<N>.png" relative to the cwd, like the reference. */
int  mcpt_render_scene(const char* path, const char* filename, int32_t spp);
#define MCPT_OUT_PNG_DEFLATE  1      /* the .png is deflate-compressed (same pixels; the reference's svpng stores them raw) */
#define MCPT_OUT_PFM          2      /* also write <prefix>-SPP<N>.pfm: the linear fp32 radiance before imshow's clamp */
#define MCPT_OUT_ERROR_PFM    4      /* also write <prefix>-SPP<N>.err.pfm: the per-pixel standard error (mcpt_progressive_image) as fp32 */
#define MCPT_OUT_SPP_PFM      8      /* also write <prefix>-SPP<N>.spp.pfm: the samples each pixel holds (mcpt_progressive_sample_counts) */
#define MCPT_OUT_DENOISED    16      /* also write <prefix>-SPP<N>.denoised.png (and .denoised.pfm with MCPT_OUT_PFM): mcpt_progressive_denoise
                                        with the defaults; needs N >= 2 */
#define MCPT_OUT_AOV_PFM     32      /* also write <prefix>-SPP<N>.albedo.pfm, .normal.pfm, .depth.pfm and .material.pfm (mcpt_progressive_aovs;
                                        depth and material -- as a float, -1 for a miss -- in all three channels) as fp32 */
#define MCPT_OUT_DENOISED_SAMPLES 64  /* also write <prefix>-SPP<N>.denoised-samples.png (and .denoised-samples.pfm with MCPT_OUT_PFM):
                                        mcpt_progressive_denoise_guided with all defaults; needs N >= 2 */
#define MCPT_OUT_SAMPLE_AOV_PFM  128  /* also write <prefix>-SPP<N>.s-albedo.pfm, .s-normal.pfm, .s-depth.pfm (in all three channels) and
                                        .coverage.pfm (ns/G, ne/G, nm/G): mcpt_progressive_sample_aovs with the default G, as fp32 */
typedef struct {
    uint64_t seed;
    int32_t  device;            /* HIP ordinal */
    int32_t  width, height;     /* >0 overrides the .camera resolution */
    int32_t  quiet;             /* suppress the reference-style progress prints */
    const char* output_prefix;  /* NULL -> "../result/<filename>"; file = <prefix>-SPP<N>.png */
    /* since MCPT_VERSION 101 (all zero = the reference's behaviour): */
    int32_t  load_flags;        /* MCPT_LOAD_* */
    int32_t  output_flags;      /* MCPT_OUT_* */
    const char* checkpoint;     /* a file: the frame is rendered in checkpoint_parts tile partitions, the fp64 frame is saved
                                   after each, and a run that finds a matching file resumes after the partitions it holds */
    int32_t  checkpoint_parts;  /* 0 -> 8 */
    int32_t  reserved;
    /* since MCPT_VERSION 102: the frame on several GPUs of the node (mcpt_multi_*); all zero = one GPU (`device`) */
    int32_t  num_devices;       /* > 0: devices[0..num_devices); -1: every visible GPU */
    int32_t  gather;            /* MCPT_GATHER_* */
    const int32_t* devices;     /* NULL with num_devices > 0: ordinals 0..num_devices-1 */
    /* since the progressive-rendering change (mcpt_render_scene_opts only).  When noise_target > 0, time_budget_s > 0 or MCPT_OUT_ERROR_PFM
     * is set, the frame is rendered progressively (mcpt_progressive_*, the passes of mcpt_progressive_next_pass): it stops after the
     * first pass whose rel_error <= noise_target, or when the time budget (seconds, counted from the first pass) allows no further pass,
     * or at N.  A frame stopped at k < N samples is written as <prefix>-SPP<k>.png (the estimate of mcpt_progressive_image); at N it is
     * the plain call's frame, byte for byte.  With a checkpoint or num_devices != 0 these return MCPT_ERR_ARG.  MCPT_OUT_DENOISED and
     * MCPT_OUT_AOV_PFM (since the denoising change) also make the frame progressive, under the same conditions; the plain .png stays
     * byte for byte what it is without them.  So do MCPT_OUT_DENOISED_SAMPLES and MCPT_OUT_SAMPLE_AOV_PFM (since the guided-denoising
     * change), with the same refusals; MCPT_OUT_DENOISED keeps writing the first-hit-guided frame, lens or not. */
    double   noise_target;      /* 0 = none */
    double   time_budget_s;     /* 0 = none */
    /* since the adaptive-sampling change (mcpt_render_scene_opts only).  adaptive_min_spp > 0: an adaptive frame
     * (mcpt_progressive_create_adaptive with rel_target = noise_target, abs_target, min_spp = adaptive_min_spp).  Its first pass is
     * min(N, adaptive_min_spp) samples, later ones follow mcpt_progressive_next_pass's doubling; it stops when no pixel is active, at N, or
     * on the time budget -- the seconds per sample of the last pass scaled by (next active count / last active count); the fixed cost of a
     * pass is not modelled.  The PNG is named after the largest count any pixel reached.  With a checkpoint or num_devices != 0:
     * MCPT_ERR_ARG. */
    int32_t  adaptive_min_spp;  /* 0 = off */
    int32_t  reserved2;
    double   abs_target;        /* adaptive frames: the absolute term of the stopping rule */
} mcpt_render_scene_options;
/* The struct has grown with MCPT_VERSION and carries no size field.  mcpt_render_scene_ex -- the only entry point through version
 * 102 -- reads the struct as it stood at 102, i.e. every field above: what a caller sets through it (load_flags, checkpoint,
 * num_devices ...) is honoured, never silently dropped; a caller compiled against a 100 / 101 header must pass a zero-extended
 * struct of this size.  mcpt_render_scene_opts (since 103) takes sizeof(mcpt_render_scene_options) as the caller's header defines
 * it and reads exactly that many bytes: the entry point for any field added after 102, and the safe one for older headers. */
int  mcpt_render_scene_ex(const char* path, const char* filename, int32_t spp, const mcpt_render_scene_options*, mcpt_stats* stats);
int  mcpt_render_scene_opts(const char* path, const char* filename, int32_t spp, const mcpt_render_scene_options*, int64_t options_bytes, mcpt_stats* stats);
/* mcpt_render_scene_opts under a lens (NULL: the pinhole, = mcpt_render_scene_opts), on the device or on every GPU of the options.  An invalid
 * lens is refused before anything is read or written.  A checkpoint's frame identity includes the lens when it is active: a lens frame never
 * resumes from a pinhole frame's checkpoint nor the reverse, and a pinhole frame's identity is what it was before lenses existed. */
int  mcpt_render_scene_lens(const char* path, const char* filename, int32_t spp, const mcpt_render_scene_options*, int64_t options_bytes,
                            const mcpt_lens*, mcpt_stats* stats);
/* mcpt_render_scene_lens under an environment light: environment_pfm (NULL: none, = mcpt_render_scene_lens) is a colour PFM read with
 * mcpt_read_pfm, environment_scale its mcpt_environment.scale; on the device or on every GPU of the options.  A map that cannot be read
 * (MCPT_ERR_IO / MCPT_ERR_PARSE) or is invalid (MCPT_ERR_ARG) is refused before anything else is read or written.  A checkpoint's frame
 * identity includes the environment when it is active (its size, scale and texels): such a frame never resumes from a checkpoint of a frame
 * without it nor the reverse, and a frame without one (or with an inactive one) keeps the identity it had before environments existed. */
int  mcpt_render_scene_env(const char* path, const char* filename, int32_t spp, const mcpt_render_scene_options*, int64_t options_bytes,
                           const mcpt_lens*, const char* environment_pfm, double environment_scale, mcpt_stats* stats);
/* mcpt_render_scene_env under a light sampling (NULL: MCPT_LIGHTS_ALL, = mcpt_render_scene_env), set on the device or on every GPU of the
 * options; an invalid one is refused (MCPT_ERR_ARG) before anything is read or written, a weight count that is not the scene's light
 * count once the scene is read.  A checkpoint's frame identity includes the mode and the table's probabilities when the device picks
 * (MCPT_LIGHTS_ONE or MCPT_LIGHTS_TREE on a scene of two or more lights; under MCPT_LIGHTS_TREE the tree's node bytes too): such a frame never resumes from a checkpoint written under another setting, and a
 * frame that does not pick keeps the identity it had before. */
int  mcpt_render_scene_lights(const char* path, const char* filename, int32_t spp, const mcpt_render_scene_options*, int64_t options_bytes,
                              const mcpt_lens*, const char* environment_pfm, double environment_scale, const mcpt_light_sampling*,
                              mcpt_stats* stats);

/* ---- geometry and camera updates (since the update change): a second frame of a scene in which something moved, without a new scene ---- */
/* mcpt_device_update_vertices replaces the positions of every face on a live device: v = [num_faces][9] doubles (v1 v2 v3 of every face,
 * .obj order).  Only positions change: face count, materials, vn, vt, the lights' materials and radiances and the resolution stay;
 * Face::norm is derived again as the loader derives it.  After the call the device behaves, in every observable result (closest hits,
 * frames, mcpt_sample_radiance, AOVs, mcpt_device_get_bvh_nodes, mcpt_device_get_leaf_order), exactly as a device created with the same
 * build mode from a mcpt_scene_create of the same description with v in place of the old vertices; only the work counters (node_visits,
 * tri_tests, dom_*) may differ after a refit.  The reference's structures (Morton keys, sort, leaf records, level unions) are built again
 * on the GPU; the key domain is the fixed cube, or for a scene loaded with MCPT_LOAD_MORTON_BOUNDS the bounds of the new vertices.
 *   MCPT_UPDATE_REFIT   : the culling hierarchy keeps its topology (child references, triangle slots); every box is recomputed bottom up
 *                         from the new triangles and quantised again with the builders' rule, the smallest grid exponent that fits.
 *                         The culling hierarchy only culls, so the frame is that of a fresh build bit for bit, at more or fewer visits.
 *   MCPT_UPDATE_REBUILD : the hierarchy is built again by the builder the device was created with.
 * The pre-test records and the light tables (areas, CDFs, the area of lights[0]) follow.  The scene handle is not touched: the device owns
 * the geometry and camera it changes.  The call is synchronous: it waits for every frame of the device in flight (they finish on the old
 * geometry) and returns when the device holds the new one.  MCPT_ERR_ARG while a progressive or adaptive handle of the device is alive.
 * Coordinates are vetted as at creation: NaN, infinities or magnitudes outside [1e-150, 1e150] switch the fast walk off
 * (fast_enabled = 0, the reference-shaped walk answers); coming back into range switches it on again.  A failure midway leaves the device
 * refusing to trace or render (MCPT_ERR_ARG, "geometry update failed") until an update succeeds.  The first update makes the faces
 * resident in .obj order (216 bytes per face) and the first refit of a hierarchy its schedule and exact boxes (52 bytes per node).
 * cost_before / cost_after: sum over the non-empty child slots of (area of the slot's stored box x (1 for a node, the triangle count for a
 * leaf)) / the area of the root's box (the union of node 0's stored child boxes), from the decoded planes: the figure to watch to decide
 * when refits have degraded the hierarchy enough to rebuild.
 * _device: v is a device pointer; `stream` (may be NULL) is waited for before v is read.  mcpt_device_get_vertices: what the device holds.
 * mcpt_device_set_camera replaces the camera (width and height stay) for every later frame; the same refusal while a progressive handle
 * lives.  mcpt_multi_*: the same on every device of the group in turn (info: of devices[0]); the first failure is returned.
 * On a device that holds a motion (mcpt_device_set_motion, below) both calls define a new key 0 and CLEAR the motion. */
#define MCPT_UPDATE_REFIT    0   /* keep the culling hierarchy's topology, recompute its boxes on the GPU */
#define MCPT_UPDATE_REBUILD  1   /* build the culling hierarchy again with the builder the device was created with */
typedef struct {
    int32_t mode;            /* what was done: MCPT_UPDATE_* */
    int32_t fast_enabled;    /* mcpt_fast_info.enabled after the update */
    int32_t leaves_moved;    /* faces whose reference leaf index changed */
    int32_t reserved;
    double  ms_reference;    /* staging, Morton keys, sort, leaf records, level unions */
    double  ms_hierarchy;    /* refit or rebuild, triangle gather, pre-test records */
    double  ms_tables;       /* light triangles, areas, CDFs */
    double  ms_total;
    double  cost_before, cost_after;
} mcpt_update_info;
int mcpt_device_update_vertices(mcpt_device*, const double* v, int32_t mode, mcpt_update_info* info /* may be NULL */);
int mcpt_device_update_vertices_device(mcpt_device*, const double* d_v, int32_t mode, mcpt_update_info* info, void* stream);
int mcpt_device_get_vertices(mcpt_device*, double* v);
int mcpt_device_set_camera(mcpt_device*, const double eye[3], const double look_at[3], const double up[3], double fovy);
int mcpt_device_get_camera(const mcpt_device*, double eye[3], double look_at[3], double up[3], double* fovy);
int mcpt_multi_update_vertices(mcpt_multi*, const double* v, int32_t mode, mcpt_update_info* info /* of devices[0]; may be NULL */);
int mcpt_multi_set_camera(mcpt_multi*, const double eye[3], const double look_at[3], const double up[3], double fovy);

/* ---- motion blur (since the motion change): a frame that integrates over the time the shutter is open, between two keyframes of a device ---- */
/* A device may hold a MOTION.  Key 0 is the geometry and camera the device holds when the motion is set.  Key 1 is the caller's: v_end =
 * [num_faces][9] doubles in .obj order as mcpt_device_update_vertices takes them (NULL: the geometry does not move) and an end camera
 * (NULL: the camera does not move).  The shutter {open, close, steps} has 0 <= open <= close <= 1, steps = K >= 1, reserved = 0.
 *   time   : step j of K is rendered at u_j = open + (close - open) * ((j + 0.5) / K), fp64 without contraction, as written
 *            (mcpt_shutter_time).
 *   blend  : every coordinate (the vertices; eye, look_at, up, fovy) is x(u) = (1 - u) * x0 + u * x1, fp64 without contraction -- and x0
 *            itself, not its rounded blend, where x0 == x1: a coordinate that does not move keeps its bits at every u, so a motion whose key 1
 *            equals key 0 renders the static frame.  For finite keys u = 0 gives key 0 and u = 1 key 1 exactly.  Face::norm is derived from
 *            the blended vertices as the loader derives it; vn, vt, materials and radiances stay, as for an update.  The camera at u_j is
 *            what mcpt_device_set_camera makes of the blended values; a blended camera it would refuse fails the frame with MCPT_ERR_ARG.
 *   samples: sample k of an N-sample frame belongs to step j = (k * K) / N in 64-bit integer arithmetic (mcpt_shutter_step): the steps are
 *            contiguous, non-empty sample ranges in ascending order.  K <= N is required at render time (MCPT_ERR_ARG).
 *   THE FRAME: sample k of pixel p is the radiance mcpt_sample_radiance(seed, p, k) returns on a device created (same build mode, lens,
 *            environment) from a scene whose vertices are V(u_j) and whose camera is C(u_j); the frame is the ordered float fold of these
 *            (D3) exactly as for a static frame.  Primary hits, light tables, the Morton order and the vetting of the coordinates follow per
 *            step, because each step is an MCPT_UPDATE_REFIT of the blended vertices on key 0's topology: the boxes of step j come from
 *            V(u_j) alone, so neither the order of the steps nor what was rendered before can matter.
 * mcpt_render / mcpt_render_device on a device with a motion render that frame (MCPT_RENDER_MEGAKERNEL and partitions honoured; the call
 * returns when the frame is finished: the steps are joined by synchronous updates).  So does a uniform progressive handle created on such a
 * device: a step(n) that crosses step boundaries is split at them, the float fold and the moments carry across, primary hits are traced
 * again per step; at done == N the image is the one-shot shutter frame bit for bit, and noise / image keep the same bits for any pass
 * sizes.  A pixel counts as hit when its primary ray hit in any step so far; the moments take every sample (a missed one as 0, or as the
 * environment's radiance), so the standard error includes the variation over time, and before done == N every pixel shows sum x / done.
 * The steps are contiguous sample ranges, so BEFORE done == N A PROGRESSIVE FRAME HOLDS THE EARLIEST PART OF THE SHUTTER ONLY: image, stderr
 * and noise at done < N describe the steps rendered so far -- a preview of the first (done K) / N of the shutter, not a noisier picture of
 * the whole of it.  A caller that stops on a noise target inside a motion frame gets that partial shutter (mcpt_render_scene_motion refuses
 * to).
 * Everything that is not a motion frame -- mcpt_trace_closest*, mcpt_sample_radiance, mcpt_camera_rays, mcpt_device_get_vertices,
 * _get_camera, _get_bvh_nodes, _get_leaf_order, _fast_hierarchy -- sees key 0, bit for bit what it saw before the motion was set: the
 * camera returns to key 0 at the end of every frame or pass, the geometry before the next such call (one refit), so a run of motion frames
 * does not pay for it between frames.  THE FIRST SUCH CALL AFTER A MOTION FRAME THEREFORE COSTS A REFIT (mcpt_update_info.ms_total of the
 * scene: under a millisecond on the small scenes, 35 ms at 10 M triangles), waits for the device's frames in flight and writes the device's
 * geometry arrays -- the read-backs mcpt_device_get_vertices, _get_bvh_nodes, _get_leaf_order and _fast_hierarchy (whose handle is const
 * for what it reports, not for this) included; so do mcpt_device_set_motion*, _clear_motion, _set_camera and _update_vertices*, the last
 * so that its cost_before and leaves_moved compare with key 0 and not with a step.  mcpt_device_get_camera, _get_motion and _motion_info
 * never do.
 * mcpt_device_update_vertices and mcpt_device_set_camera define a new key 0 and CLEAR the motion -- once they have succeeded: a call that
 * is refused, or an update that fails midway, leaves the motion in place.  mcpt_device_set_motion* and
 * mcpt_device_clear_motion are refused (MCPT_ERR_ARG) while a progressive handle of the device lives, like an update.
 * Refused with MCPT_ERR_ARG on a device with a motion: mcpt_progressive_create_adaptive, MCPT_RENDER_PIPELINE, mcpt_progressive_aovs /
 * _denoise on a handle created under the motion, and in mcpt_render_scene_motion a checkpoint or several GPUs (a mcpt_multi group has no
 * motion).  Invalid shutters are MCPT_ERR_ARG before MCPT_ERR_NO_DEVICE, as for the lens.
 * Memory: both keyframes stay resident in the staging layout when the geometry moves, 72 bytes per face per keyframe on top of the 216 per
 * face the first update makes resident; a one-shot motion frame keeps 49 bytes per pixel of moments (53 under an active lens).
 * _device: d_v_end is a device pointer; `stream` (may be NULL) is waited for before it is read.
 * mcpt_device_get_motion: shutter->steps = 0 when the device holds none; *has_geometry / *has_camera say which of the two moves;
 * camera_end receives key 1's camera (the device's own when it does not move).  Any pointer may be NULL.
 * mcpt_device_motion_info: of the last motion frame or progressive pass -- the steps it ran, the milliseconds spent in their updates (the
 * return to key 0 is not in it) and the largest cost_after of a step / the cost at key 0 (mcpt_update_info; 0 when no geometry moved). */
typedef struct { double open, close; int32_t steps, reserved; } mcpt_shutter;
typedef struct { double eye[3], look_at[3], up[3], fovy; } mcpt_camera_key;
typedef struct { int32_t steps_run, reserved; double ms_updates, max_cost_ratio; } mcpt_motion_info;
int mcpt_device_set_motion(mcpt_device*, const double* v_end, const mcpt_camera_key* camera_end, const mcpt_shutter*);
int mcpt_device_set_motion_device(mcpt_device*, const double* d_v_end, const mcpt_camera_key* camera_end, const mcpt_shutter*, void* stream);
int mcpt_device_clear_motion(mcpt_device*);
int mcpt_device_get_motion(const mcpt_device*, mcpt_shutter* shutter, int32_t* has_geometry, int32_t* has_camera, mcpt_camera_key* camera_end);
int mcpt_device_motion_info(const mcpt_device*, mcpt_motion_info* out);
/* pure functions, usable without a GPU: u_j (NaN for an invalid shutter or j outside [0, steps)) and the step of sample k (-1 for
 * spp < 1, steps outside [1, spp] or k outside [0, spp)) */
double  mcpt_shutter_time(double open, double close, int32_t steps, int32_t j);
int32_t mcpt_shutter_step(int32_t spp, int32_t steps, int32_t k);
/* mcpt_render_scene_env with a motion: end_obj (NULL: the geometry does not move) is the path of an .obj file read with the scene's load
 * flags, whose faces -- same count, same per-face materials, otherwise MCPT_ERR_PARSE before anything is written -- give key 1's vertices;
 * end_camera (NULL: the camera does not move) the path of a .camera file whose eye, look_at, up and fovy give key 1's camera (its resolution
 * and lights are ignored).  shutter == NULL: mcpt_render_scene_env.  With a checkpoint or num_devices != 0: MCPT_ERR_ARG.  MCPT_OUT_ERROR_PFM
 * renders the frame through a uniform progressive handle under the motion, all N samples of it.  noise_target and time_budget_s are
 * refused with MCPT_ERR_ARG: a frame stopped at k < N would hold the first part of the shutter only.  So are adaptive frames,
 * MCPT_OUT_DENOISED and MCPT_OUT_AOV_PFM. */
int  mcpt_render_scene_motion(const char* path, const char* filename, int32_t spp, const mcpt_render_scene_options*, int64_t options_bytes,
                              const mcpt_lens*, const char* environment_pfm, double environment_scale, const char* end_obj,
                              const char* end_camera, const mcpt_shutter*, mcpt_stats* stats);

/* ---- display transform (since the display change): a linear fp64 frame becomes 8-bit pixels, on the GPU ---- */
/* Off by default: without display parameters every byte the library writes is mcpt_quantize_rgb8's.  A frame is n_pixels x 3 doubles,
 * the picture n_pixels x 3 bytes (x 4 with MCPT_DISPLAY_RGBA: alpha 255).  Everything is fp64 without contraction, in the order written.
 *   HISTOGRAM of the luminance Y = (0.2126 r + 0.7152 g) + 0.0722 b of the raw frame, MCPT_DISPLAY_SLOTS int64 counts.  With `bits` the 64
 *            bits of Y, b = (((bits >> 52) - 1023 + 24) * 8) + ((bits >> 49) & 7): MCPT_DISPLAY_BINS bins over 2^-24 .. 2^24, 8 per stop,
 *            taken from the exponent and the top three mantissa bits -- never from a logarithm, so no rounding moves a pixel across an edge
 *            and the counts are exact on every device.  slot 0: skipped pixels (Y not finite or Y <= 0, NaN included); slot 1: b < 0
 *            (denormals included); slots 2 .. 385: bins 0 .. 383; slot 386: b > 383.
 *   EXPOSURE from the slots (mcpt_display_exposure, host only): counted = the sum of slots 1 .. 386;
 *            log_average = exp2(sum n_b log2(centre_b) / counted), summed in slot order, centre_b = ldexp(1 + ((b & 7) + 0.5) / 8, (b >> 3) - 24),
 *            the under slot counted at bin 0's centre and the over slot at bin 383's;
 *            l_percentile = the upper edge ldexp(1 + ((b & 7) + 1) / 8, (b >> 3) - 24) of the first bin at which the running count (the
 *            under slot first) reaches ceil(p counted); p == 0 is 0.99.  counted == 0: both are 0.
 *   PARAMETERS  e = exposure (0: 1.0); with auto_key > 0 and log_average > 0, e = e * (auto_key / log_average).  REINHARD's white
 *            w = white, or max(1, e * l_percentile) when white == 0 (1 when nothing was counted).  The histogram is taken only when
 *            auto_key > 0 or REINHARD is asked with white == 0; otherwise info reports log_average = l_percentile = counted = skipped = 0.
 *   MAP      per pixel and channel c, with IEEE division:
 *            x = e * c;  x = x > 0 ? x : 0 (NaN and negatives: 0);  x = x < 2^64 ? x : 2^64;
 *            MCPT_CURVE_CLAMP    y = x
 *            MCPT_CURVE_REINHARD Yx = (0.2126 x_r + 0.7152 x_g) + 0.0722 x_b;  y_c = x_c * ((1 + Yx / (w * w)) / (1 + Yx)), 0 when Yx == 0
 *            MCPT_CURVE_FILMIC   y = (x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14)
 *            y = y < 1 ? y : 1;
 *            MCPT_TRANSFER_LINEAR  the byte is y * 255 truncated, as mcpt_quantize_rgb8 truncates
 *            MCPT_TRANSFER_SRGB    y = y <= 0.0031308 ? 12.92 * y : 1.055 * pow(y, 1 / 2.4) - 0.055;  the byte is floor(y * 255 + 0.5)
 *            (pow is the one step in which two math libraries may differ by an ulp: a byte may then differ where y * 255 + 0.5 is within
 *            that ulp of an integer).
 * NULL or all-zero parameters give mcpt_quantize_rgb8's bytes bit for bit.  MCPT_ERR_ARG: reserved != 0, an unknown curve, transfer or
 * flag, a negative or non-finite exposure, auto_key, percentile or white, a percentile above 1.
 * _device forms take device pointers and enqueue on `stream`; a call that takes the histogram waits for the stream (the slots come back
 * to the host: 3 KB).  The device map writes four pixels per lane with 4-byte (RGBA: 16-byte) stores when d_out is aligned to that and
 * d_img to 16 bytes, and single bytes otherwise: the bytes are the same.  mcpt_display_host is the same arithmetic on the CPU, usable
 * without a GPU: it is what mcpt_render_scene_display writes its pictures through.
 * mcpt_progressive_display: the picture of a progressive handle's estimate (MCPT_DISPLAY_ESTIMATE: mcpt_progressive_image), of its denoised
 * frame (_DENOISED: mcpt_progressive_denoise) or of the sample-guided one (_DENOISED_GUIDED: mcpt_progressive_denoise_guided), the filters
 * with all defaults and their own refusals.  Histogram and map run over the handle's owned pixels only: the bytes of every other pixel of
 * rgb8 (W x H x 3 or 4 bytes) stay as they are.  The frame never leaves the GPU; the handle keeps one fp64 scratch frame from the first
 * call on.  The handle's image, moments and counts are not changed.
 * mcpt_render_scene_display: mcpt_render_scene_lights whose .png, .denoised.png and .denoised-samples.png go through the display (each
 * picture with its own histogram); the PFMs stay linear.  display == NULL: mcpt_render_scene_lights, byte for byte.  MCPT_DISPLAY_RGBA is
 * refused there (the PNGs are RGB). */
#define MCPT_DISPLAY_BINS   384
#define MCPT_DISPLAY_SLOTS  387
#define MCPT_CURVE_CLAMP      0
#define MCPT_CURVE_REINHARD   1
#define MCPT_CURVE_FILMIC     2
#define MCPT_TRANSFER_LINEAR  0
#define MCPT_TRANSFER_SRGB    1
#define MCPT_DISPLAY_RGBA     1   /* flags: four bytes per pixel, alpha 255 */
#define MCPT_DISPLAY_ESTIMATE         0
#define MCPT_DISPLAY_DENOISED         1
#define MCPT_DISPLAY_DENOISED_GUIDED  2
typedef struct { double exposure;    /* 0: 1.0; with auto_key > 0 a compensation factor */
                 double auto_key;    /* > 0: exposure *= auto_key / log_average (0.18 is the usual key) */
                 double percentile;  /* 0: 0.99 */
                 double white;       /* REINHARD's w; 0: max(1, exposure * l_percentile) */
                 int32_t curve, transfer, flags, reserved; } mcpt_display_params;
typedef struct { double exposure, white, log_average, l_percentile; int64_t counted, skipped; } mcpt_display_info;
int mcpt_display_histogram_device(mcpt_device*, const double* d_img, int64_t n_pixels, int64_t slots[MCPT_DISPLAY_SLOTS], void* stream);
int mcpt_display_histogram(mcpt_device*, const double* img, int64_t n_pixels, int64_t slots[MCPT_DISPLAY_SLOTS]);
int mcpt_display_exposure(const int64_t slots[MCPT_DISPLAY_SLOTS], double percentile, double* log_average, double* l_percentile);
int mcpt_display_device(mcpt_device*, const double* d_img, int64_t n_pixels, const mcpt_display_params*, uint8_t* d_out,
                        mcpt_display_info* info /* may be NULL */, void* stream);
int mcpt_display(mcpt_device*, const double* img, int64_t n_pixels, const mcpt_display_params*, uint8_t* out, mcpt_display_info* info);
int mcpt_display_host(const double* img, int64_t n_pixels, const mcpt_display_params*, uint8_t* out, mcpt_display_info* info);
int mcpt_progressive_display(mcpt_progressive*, int32_t source, const mcpt_display_params*, uint8_t* rgb8, mcpt_display_info* info);
int mcpt_progressive_display_device(mcpt_progressive*, int32_t source, const mcpt_display_params*, uint8_t* d_rgb8, mcpt_display_info* info,
                                    void* stream);
int mcpt_render_scene_display(const char* path, const char* filename, int32_t spp, const mcpt_render_scene_options*, int64_t options_bytes,
                              const mcpt_lens*, const char* environment_pfm, double environment_scale, const mcpt_light_sampling*,
                              const mcpt_display_params* display, mcpt_stats* stats);

/* ---- radiance queries (since the query change; the reference reaches its path tracer through the scene's camera only) ---- */
/* A QUERY LIST gives the path tracer n rays, or n surface points, of the caller's: light probes and lightmaps, reflection probes, a
 * projection the .camera file cannot express, the radiance along a few rays.  Every query gets spp path samples and its answer is their
 * mean, the standard error of that mean and the number of samples whose ray hit anything.  MCPT_VERSION stays 105: detect the block by
 * symbol.  fp64, no contraction, sums in the order written.
 *   keys     : query i has id ids[i], or i when ids == NULL; ids are >= 0.  Its sample j = 0 .. spp-1 is sample index k = sample_base + j,
 *              and the path of (i, k) uses the RNG key (seed, pixel = id, sample = k) -- the key of camera sample (pixel, k).  Nothing else of
 *              a frame enters: the scene's width, height and camera and the device's lens do not affect a query.  A query whose rays are
 *              a frame's camera rays and whose ids are their pixels computes that frame's samples, bit for bit.
 *   MCPT_QUERY_RAY        : q = origin o, direction d.  Every sample traces the ray (o, d) as given, from o itself (the camera rays'
 *              convention, no offset).  d must have unit length: the host-pointer form refuses a component that is not finite and
 *              | |d|^2 - 1 | > 1e-9, |d|^2 = (dx dx + dy dy) + dz dz; the device form does not look.
 *   MCPT_QUERY_HEMISPHERE : q = position a, normal b of any non-zero finite length.  n^ = b / sqrt((bx bx + by by) + bz bz); e = the
 *              coordinate axis on which |n^| is smallest, the lowest axis among equals; t = normalize(cross(e, n^)), s = cross(n^, t),
 *              cross(p, q) = (py qz - qy pz, qx pz - px qz, px qy - qx py); u0, u1 = words 0 and 1 of the camera-uniform block
 *              uniform(seed, id, k, depth 0xFFFF, slot 0..3) the lens draws from (a query has no lens: nothing collides);
 *              r = sqrt(u0), phi = (2 pi) * u1 with the full-precision pi, z = sqrt(max(0, 1 - u0));
 *              d = normalize((t * (r cos phi) + s * (r sin phi)) + n^ * z), o = a + d * 0.01 (the shadow rays' offset).
 *              d is cosine-weighted about n^, so the mean is the cosine-weighted mean of the incoming radiance: THE IRRADIANCE IS
 *              pi TIMES THE MEAN (and its standard error pi times the standard error).
 *   shading  : the ray is a camera ray of the per-sample route (camera lens above).  Its first hit is shaded at depth 0 under the unchanged
 *              rules and draws; a ray that reaches an emitter returns the light's radiance unweighted; a ray that leaves the scene gives
 *              +0.0, or Le(d) under an active environment.  Environment, light sampling and trace mode are the device's.  A device that
 *              holds a motion answers from key 0, as every call that is not a frame.
 *   fold     : per query and channel, in k order: s1 += x, s2 += x * x; mean = s1 / spp; stderr = 0 when spp < 2, else
 *              sqrt(max((s2 - s1 * s1 / spp) / (spp - 1), 0) / spp) -- the expressions of a progressive frame's estimate and error.
 *              hits[i] = the samples of query i whose ray hit anything.  mean3 is required; stderr3 and hits may be NULL.
 *   stats    : rays_primary = samples = n * spp; the other counters as for a frame under a lens.
 *   flags    : 0, the wavefront pipeline, or MCPT_RENDER_MEGAKERNEL.
 * Errors (MCPT_ERR_ARG, before MCPT_ERR_NO_DEVICE): spp < 1, sample_base < 0, sample_base + spp > 2^31 - 1, n < 0 or n > 2^31 - 1, an
 * unknown kind or flag, reserved != 0, NULL q6 or mean3 with n > 0 and, in the host-pointer forms, a negative id, a component that is not
 * finite, a direction that is not unit, a normal of length zero or not finite.  n == 0: MCPT_OK, nothing is launched.
 * The host-pointer form is synchronous.  The device form (device pointers throughout) enqueues on `stream` and returns without waiting
 * when stats == NULL.  Both use the device's frame slot 0 and first wait for the device's frames still in flight (MCPT_RENDER_PIPELINE /
 * KEEP_STATS).  Queries are allowed while progressive handles of the device live: they touch none of a handle's state.
 * Not covered: the multi-device group, render_scene, sample counts given per query by the caller.  Queries that stop on their own error
 * estimate are the adaptive queries' block below.  The radiance of the whole sphere about a point, for any normal afterwards, is a light
 * probe's (below), not a kind of this call. */
#define MCPT_QUERY_RAY        0   /* q = origin xyz, direction xyz */
#define MCPT_QUERY_HEMISPHERE 1   /* q = position xyz, normal xyz  */
typedef struct { int32_t spp, sample_base; uint64_t seed; int32_t kind, flags, reserved[2]; } mcpt_query_params;
int mcpt_query_radiance(mcpt_device*, const double* q6, const int32_t* ids, int64_t n, const mcpt_query_params*,
                        double* mean3, double* stderr3, int32_t* hits, mcpt_stats*);
int mcpt_query_radiance_device(mcpt_device*, const double* d_q6, const int32_t* d_ids, int64_t n, const mcpt_query_params*,
                               double* d_mean3, double* d_stderr3, int32_t* d_hits, mcpt_stats*, void* stream);
/* test seam: the ray of sample k[i] of query i -> rays6[n*6] = origin xyz, direction xyz (k[i] >= 0) */
int mcpt_query_rays(mcpt_device*, const double* q6, const int32_t* ids, int64_t n, uint64_t seed, int32_t kind,
                    const int32_t* k, double* rays6);

/* ---- light probes (since the probe change; MCPT_VERSION stays 105: detect the block by symbol) ---- */
/* A LIGHT PROBE is a point in free space that stores the incoming radiance of the whole sphere about it as nine real spherical-harmonic
 * coefficients (bands 0..2) per colour channel; a receiver then looks up diffuse lighting for any normal without tracing again.
 * mcpt_query_sh is mcpt_query_radiance over a list of n positions p3[n*3] with a third source draw and a fold of its own; keys, shading,
 * sample ranges, flags, statistics (rays_primary = samples = n * spp), concurrency and the motion rule are that call's, word for word.
 * fp64, no contraction, sums in the order written.
 *   draw     : u0, u1 = words 0 and 1 of the camera-uniform block uniform(seed, id, k, depth 0xFFFF, slot 0..3), the hemisphere kind's;
 *              z = 1.0 - 2.0 * u0, r = sqrt(max(0, 1.0 - z * z)), phi = 6.283185307179586 * u1,
 *              d = normalize((r cos phi, r sin phi, z)) in world axes, o = p: the probe point itself, no offset (MCPT_QUERY_RAY's
 *              convention).  A PROBE IS MEANT TO SIT IN FREE SPACE; a caller who puts one on a surface lifts it off first.
 *              The draw is an internal third kind: mcpt_query_radiance and mcpt_query_rays refuse kind 2 as before.
 *   basis    : for a unit direction (x, y, z), in this index order and operation order:
 *                Y0 = 0.28209479177387814
 *                Y1 = 0.4886025119029199 * y      Y2 = 0.4886025119029199 * z      Y3 = 0.4886025119029199 * x
 *                Y4 = 1.0925484305920792 * (x * y)    Y5 = 1.0925484305920792 * (y * z)
 *                Y6 = 0.31539156525252005 * (3.0 * (z * z) - 1.0)
 *                Y7 = 1.0925484305920792 * (x * z)    Y8 = 0.5462742152960396 * (x * x - y * y)
 *              (1/(2 sqrt(pi)), sqrt(3/(4 pi)), sqrt(15/(4 pi)), sqrt(5/(16 pi)), sqrt(15/(16 pi)): orthonormal over the sphere)
 *   fold     : per probe s, coefficient i and channel c, in k order, with x_k the sample's radiance (a missed ray: +0.0, or Le(d) under an
 *              environment, summed like any other) and d_k bitwise the direction its ray was given:
 *              v = x_k[c] * Y_i(d_k), s1 += v, s2 += v * v;
 *              sh[s][i][c] = 12.566370614359172 * (s1 / spp)                                          (4 pi: 1 / the draw's density)
 *              err[s][i][c] = 0 when spp < 2, else 12.566370614359172 * sqrt(max((s2 - s1 * s1 / spp) / (spp - 1), 0) / spp)
 *              hits[s] = the samples of probe s whose ray hit anything.  sh27 [n][9][3] is required; stderr27 and hits may be NULL.
 *   use      : mcpt_sh_radiance: L(d) = sum_i sh[i] * Y_i(d), in index order from 0.0.  mcpt_sh_irradiance, probe i with normal i of any
 *              non-zero finite length: n^ = n / sqrt((nx nx + ny ny) + nz nz), E_c = sum_i (A_l(i) * Y_i(n^)) * sh[i][c] in index
 *              order from 0.0, A0 = 3.141592653589793 (i = 0), A1 = 2.0943951023931953 (i = 1..3), A2 = 0.7853981633974483 (i = 4..8):
 *              the order-2 approximation of the irradiance mcpt_query_radiance's hemisphere kind estimates for one normal.
 * Errors (MCPT_ERR_ARG, before MCPT_ERR_NO_DEVICE), in mcpt_query_radiance's order: NULL parameters, spp < 1, sample_base < 0,
 * sample_base + spp > 2^31 - 1, n < 0 or n > 2^31 - 1, a flag other than 0 or MCPT_RENDER_MEGAKERNEL, reserved != 0, NULL p3 or sh27 with
 * n > 0 and, in the host-pointer forms, a negative id or a position that is not finite.  n == 0: MCPT_OK, nothing is launched.  The device
 * form takes device pointers throughout (p3 as n*3 device doubles), enqueues on `stream` and returns without waiting when stats == NULL.
 * The host helpers need no device; they refuse a NULL pointer, n < 0, a component that is not finite and, mcpt_sh_irradiance, a normal of
 * zero, underflowing or overflowing length.
 * Not covered: the multi-device group, render_scene, interpolation between the probes of a grid (that is the irradiance volumes' block
 * below), bands above 2, adaptive stopping. */
typedef struct { int32_t spp, sample_base; uint64_t seed; int32_t flags, reserved[3]; } mcpt_sh_params;
int mcpt_query_sh(mcpt_device*, const double* p3, const int32_t* ids, int64_t n, const mcpt_sh_params*,
                  double* sh27, double* stderr27, int32_t* hits, mcpt_stats*);
int mcpt_query_sh_device(mcpt_device*, const double* d_p3, const int32_t* d_ids, int64_t n, const mcpt_sh_params*,
                         double* d_sh27, double* d_stderr27, int32_t* d_hits, mcpt_stats*, void* stream);
/* test seam: the ray of sample k[i] of probe i -> rays6[n*6] = origin xyz, direction xyz (k[i] >= 0) */
int mcpt_query_sh_rays(mcpt_device*, const double* p3, const int32_t* ids, int64_t n, uint64_t seed, const int32_t* k, double* rays6);
int mcpt_sh_basis(const double* d3, int64_t n, double* y9);                                     /* y9[n*9] = Y_0..8(d_i) */
int mcpt_sh_radiance(const double* sh27, const double* d3, int64_t n, double* rgb3);           /* probe i along direction i */
int mcpt_sh_irradiance(const double* sh27, const double* n3, int64_t n, double* e3);           /* probe i under normal i */

/* ---- lightmaps (since the lightmap change; MCPT_VERSION stays 105: detect the block by symbol) ---- */
/* A LIGHTMAP is the irradiance at the surface points a UV chart maps its texels to.  The baker rasterises the chart, lists the covered
 * texels with their positions and normals, asks mcpt_query_radiance's hemisphere kind for that list and puts the answers back: A LIGHTMAP
 * IS, BIT FOR BIT, THE HEMISPHERE QUERY OF ITS OWN TEXEL LIST.  fp64, no contraction, IEEE division, every expression in the order written.
 *   chart    : uv6[num_faces][6] = (au, av, bu, bv, cu, cv) of every face in .obj order; NULL: the scene's own vt1 vt2 vt3 (all zero in a
 *              scene created without vt: nothing is covered, which is not an error).  The map is width x height texels, each size in
 *              1 .. 16384.  Texel (x, y) has index T = y * width + x and centre pu = (x + 0.5) / width, pv = (y + 0.5) / height; row 0 is
 *              the row nearest v = 0: no flip, no wrap.  UVs outside [0, 1] are allowed; only texels of the map count.
 *   coverage : for face f with chart corners a, b, c and a centre p
 *                area2 = (bu - au) * (cv - av) - (bv - av) * (cu - au)
 *                e_a   = (bu - pu) * (cv - pv) - (bv - pv) * (cu - pu)
 *                e_b   = (cu - pu) * (av - pv) - (cv - pv) * (au - pu)
 *                e_c   = (au - pu) * (bv - pv) - (av - pv) * (bu - pu)
 *              f COVERS the texel when area2 > 0 and e_a, e_b, e_c >= 0, or area2 < 0 and all three <= 0.  A face is skipped altogether
 *              when area2 is 0 or not finite, or when its geometric normal n (Face::norm) has a length that is zero or not finite:
 *              (nx nx + ny ny) + nz nz is 0, NaN or infinite.  owner[T] = the LOWEST .obj face index that covers T, or -1.  A centre
 *              exactly on a shared edge or vertex is claimed by every face that touches it and the lowest wins: there is no top-left rule,
 *              and the answer does not depend on how the work is spread.  Only the texels of a face's box are tested against it: those
 *              whose centre lies between the smallest and the largest of its three u and of its three v, and one texel more on every side
 *              (in exact arithmetic no centre outside the corners' box passes the three inequalities; a sliver thinner than fp64's
 *              rounding does not get texels outside it from rounding either).
 *   list     : the covered texels in ascending T.  For entry i with texel T and owner f:
 *                w_a = e_a / area2, w_b = e_b / area2, w_c = e_c / area2;
 *                position = (v1 * w_a + v2 * w_b) + v3 * w_c per component, from the device's current vertices (after
 *                mcpt_device_update_vertices the updated ones; under a motion key 0's);
 *                normal = the same blend of vn1, vn2, vn3 -- Face::norm instead when its squared length (x x + y y) + z z is 0 or not finite;
 *                q6[i] = (position, normal), texels[i] = T.
 *              The id of a texel's query is T, so its samples depend neither on which other texels are covered nor on the list's order.
 *   bake     : mcpt_query_radiance_device over (q6, ids = texels) with kind MCPT_QUERY_HEMISPHERE and the caller's spp, sample_base, seed
 *              and flags (0 or MCPT_RENDER_MEGAKERNEL); environment, light sampling, trace mode and engine are the device's.  Chunking,
 *              statistics (rays_primary = samples = covered texels * spp), concurrency and the motion rule are that call's, word for word.
 *   scatter  : irradiance3[T] = 3.141592653589793 * mean, stderr3[T] = 3.141592653589793 * stderr, hits[T] = the query's hit count.
 *              Every texel that is not covered gets +0.0, +0.0 and 0.
 *   dilation : dilate = R rounds, 0 .. 64, on irradiance3 only.  A texel is VALID before round 1 when it is covered.  In round r = 1 .. R
 *              every texel not valid after round r - 1 looks at its 8 neighbours (y + dy, x + dx), dy and dx in -1 .. 1, row-major, inside
 *              the map; if c >= 1 of them were valid after round r - 1, its irradiance becomes s / c per channel, s = 0.0 plus their values
 *              of round r - 1 in that order, it becomes valid and its owner becomes -1 - r: a filled texel reads -2, -3, ..., -1 was
 *              never filled and >= 0 is a face.  stderr3 and hits of filled texels stay 0.  Every round reads the frame of the round
 *              before and writes another, so the result does not depend on scheduling.
 * mcpt_lightmap_raster_host is the coverage rule alone for a caller's chart, on the CPU: no device, no scene, hence never the skip by a
 * face's normal.  mcpt_lightmap_texels is coverage and list on the device; it returns the number of covered texels (< 0: MCPT_ERR_*);
 * owner[W*H], texels[cap] and q6[cap*6] may each be NULL; more covered texels than cap while a list is asked for: MCPT_ERR_ARG.
 * mcpt_bake_lightmap is all five steps: irradiance3[W*H*3] is required, stderr3[W*H*3], hits[W*H] and owner[W*H] may be NULL.  The host
 * form is synchronous.  The _device form takes device pointers throughout (d_uv6 as num_faces * 6 device doubles) and enqueues on `stream`;
 * IT WAITS ONCE FOR THE STREAM, for the number of covered texels (4 bytes come back to the host, as the display histogram's slots do),
 * and otherwise returns without waiting when stats == NULL.  No texel covered: MCPT_OK, no query is launched, the maps are all zero and
 * owner all -1.  A device keeps the baker's workspace from its first bake on (about 4 bytes per texel of the largest map so far, up to 104 per
 * covered texel, 8 per face, and with dilation 28 more per texel); a bake first waits for the device's previous bake.
 * Errors (MCPT_ERR_ARG, before MCPT_ERR_NO_DEVICE, in this order): NULL parameters, a size outside 1 .. 16384, spp < 1, sample_base < 0,
 * sample_base + spp > 2^31 - 1, a flag other than 0 or MCPT_RENDER_MEGAKERNEL, dilate outside 0 .. 64, reserved != 0, NULL irradiance3;
 * mcpt_lightmap_texels: a size outside 1 .. 16384, cap < 0; mcpt_lightmap_raster_host: num_faces < 0, a size outside 1 .. 16384, NULL uv6
 * or owner.  In the host-pointer forms a chart component that is not finite is MCPT_ERR_ARG as well -- on a device, after the missing
 * device and the NULL device, because the chart's length is the device's face count.  The device form does not look: a face whose area2
 * is not finite is skipped.
 * Not covered: UV unwrapping and packing; supersampling or conservative coverage (a sliver that contains no texel centre gets no texel:
 * dilation is the remedy); rejecting texels whose point lies inside other geometry; directional or SH lightmaps; the multi-device group
 * and render_scene.  (The ambient occlusion block's map counts, per texel, the rays that met a face from behind: that finds the
 * texels inside other geometry.)  The use of a lightmap in shading is the baked frames' block's, below.  Texels that stop on their own error
 * estimate are mcpt_bake_lightmap_adaptive's (adaptive queries, below). */
typedef struct { int32_t width, height, spp, sample_base; uint64_t seed;
                 int32_t flags, dilate, reserved[2]; } mcpt_lightmap_params;
int     mcpt_lightmap_raster_host(const double* uv6, int64_t num_faces, int32_t width, int32_t height, int32_t* owner);
int64_t mcpt_lightmap_texels(mcpt_device*, const double* uv6, int32_t width, int32_t height,
                             int32_t* owner, int32_t* texels, double* q6, int64_t cap);
int mcpt_bake_lightmap(mcpt_device*, const double* uv6, const mcpt_lightmap_params*,
                       double* irradiance3, double* stderr3, int32_t* hits, int32_t* owner, mcpt_stats*);
int mcpt_bake_lightmap_device(mcpt_device*, const double* d_uv6, const mcpt_lightmap_params*,
                              double* d_irradiance3, double* d_stderr3, int32_t* d_hits, int32_t* d_owner,
                              mcpt_stats*, void* stream);

/* ---- adaptive queries and lightmaps (since the adaptive-query change; MCPT_VERSION stays 105: detect the block by symbol) ---- */
/* AN ADAPTIVE QUERY CALL is mcpt_query_radiance in passes: every query stops on its own error estimate, as a pixel of an adaptive frame
 * does, and the active list is compacted on the GPU without atomics.  It takes a list, a mcpt_query_params -- whose spp is now the LARGEST
 * count a query may get -- and a mcpt_adaptive_params (rel_target, abs_target, min_spp, as for frames).  Keys, kinds (MCPT_QUERY_RAY and
 * MCPT_QUERY_HEMISPHERE), shading, flags, environment, light sampling, trace mode and the motion rule are mcpt_query_radiance's.
 *   passes   : boundaries b_0 = min(min_spp, spp), b_{j+1} = min(2 * b_j, spp), computed in 64 bits; the last boundary is spp.  A min_spp
 *              above spp is taken as spp: one pass, the one-shot call.  Pass j renders samples [sample_base + b_{j-1}, sample_base + b_j)
 *              of the active queries only, with b_{-1} = 0.  Queries only leave the list, so all active queries share the count.
 *              mcpt_query_pass_boundaries writes the boundaries of (spp >= 1, min_spp >= 2) to bounds[cap] (may be NULL) and returns
 *              their number; more boundaries than cap while a list is asked for, or cap < 0: MCPT_ERR_ARG.  Host only, no device.
 *   stopping : after the pass that ends at k = b_j < spp, query i stops when
 *                  se2 < rel2 * m2 + abs2
 *              with se2, m2, rel2 and abs2 exactly as in mcpt_progressive_create_adaptive's text above: fp64 without contraction, the
 *              channels summed in order 0, 1, 2, from query i's own s1_c and s2_c, the fold's sums, added in k order.  k >= min_spp holds
 *              at every boundary by construction.  THERE IS NO MISS RULE: a query has no pixel whose value is known to be +0.0 for every
 *              count, and under an environment a missed ray carries Le(d).  A query whose samples are all +0.0 has se2 = m2 = 0, so it
 *              stops only when abs_target > 0 (with abs_target = 0 it runs to spp).  A query that is still active at spp keeps count spp.
 *   answers  : with c_i the count of query i: mean = s1 / c_i; stderr = sqrt(se2_c(c_i)), and 0 when c_i < 2; hits = the number of those
 *              c_i samples whose ray hit; counts[i] = c_i -- mcpt_query_radiance's fold expressions.  Hence
 *              QUERY i OF AN ADAPTIVE CALL IS, BIT FOR BIT, QUERY i OF mcpt_query_radiance WITH spp = counts[i], the same id, seed and
 *              sample_base.  With both targets 0 every count is spp and the whole call is the one-shot call, bit for bit.  The sums
 *              continue across passes exactly: they start from +0.0 and add every sample of a pass in k order, and a stored fp64 sum
 *              reloaded is the same sum.  Stopping on a query's own variance estimate biases its estimate slightly, as for a frame.
 *              mean3 is required; stderr3, hits and counts may be NULL.
 *   stats    : rays_primary = samples = the sum of counts, added up over the passes; the other counters likewise, ms_trace and ms_total
 *              the passes' sums.
 * Errors (MCPT_ERR_ARG, before MCPT_ERR_NO_DEVICE): first mcpt_query_radiance's own, in its order (the host-pointer form's look at the
 * list included); then NULL adaptive parameters, targets that are not finite or are negative, min_spp < 2, reserved != 0.  n == 0:
 * MCPT_OK, nothing is launched.
 * The host-pointer form is synchronous.  The _device form takes device pointers throughout and enqueues on `stream`; AFTER EVERY PASS BUT
 * THE LAST IT WAITS FOR THE STREAM, for the length of the next list (4 bytes come back to the host through a pinned word, as an adaptive
 * frame's step and the baker's texel count do), and stops early when that list is empty; after the last pass it enqueues the finishing
 * kernel and returns without waiting when stats == NULL.  Both forms use the device's frame slot 0 and first wait for the device's frames
 * in flight; live progressive handles are untouched.  A device keeps the call's workspace from its first adaptive call on (117 bytes per
 * query of the longest list so far); a call first waits for the device's previous adaptive call.
 * AN ADAPTIVE LIGHTMAP IS, BIT FOR BIT, THE ADAPTIVE HEMISPHERE QUERY OF ITS OWN TEXEL LIST (ids = the texel indices), scattered as a
 * lightmap's: coverage, list, scatter, dilation, refusals and waiting are mcpt_bake_lightmap's with the adaptive call in the query's place
 * (so the _device form waits for the texel count and then as above); the adaptive parameters are refused after the lightmap's own.
 * counts[T] (W*H, may be NULL) is the texel's count, and 0 where the texel is not covered or was only dilated.  The targets apply to the
 * query's mean, which is the irradiance over pi: rel_target does not care about the scale, ABS_TARGET DOES -- an absolute error e of the
 * irradiance is abs_target = e / pi.
 * Not covered: adaptive light probes, sample counts given per query by the caller, a caller-chosen pass schedule, the multi-device group,
 * render_scene. */
int mcpt_query_pass_boundaries(int32_t spp, int32_t min_spp, int32_t* bounds, int32_t cap);
int mcpt_query_radiance_adaptive(mcpt_device*, const double* q6, const int32_t* ids, int64_t n, const mcpt_query_params*,
                                 const mcpt_adaptive_params*, double* mean3, double* stderr3, int32_t* hits, int32_t* counts, mcpt_stats*);
int mcpt_query_radiance_adaptive_device(mcpt_device*, const double* d_q6, const int32_t* d_ids, int64_t n, const mcpt_query_params*,
                                        const mcpt_adaptive_params*, double* d_mean3, double* d_stderr3, int32_t* d_hits, int32_t* d_counts,
                                        mcpt_stats*, void* stream);
int mcpt_bake_lightmap_adaptive(mcpt_device*, const double* uv6, const mcpt_lightmap_params*, const mcpt_adaptive_params*,
                                double* irradiance3, double* stderr3, int32_t* hits, int32_t* owner, int32_t* counts, mcpt_stats*);
int mcpt_bake_lightmap_adaptive_device(mcpt_device*, const double* d_uv6, const mcpt_lightmap_params*, const mcpt_adaptive_params*,
                                       double* d_irradiance3, double* d_stderr3, int32_t* d_hits, int32_t* d_owner, int32_t* d_counts,
                                       mcpt_stats*, void* stream);

/* ---- lightmap denoising (since the lightmap-denoise change; MCPT_VERSION stays 105: detect the block by symbol) ---- */
/* mcpt_lightmap_denoise: an edge-avoiding a-trous wavelet filter of an irradiance map in UV space, guided by the world position, the
 * normal and the world footprint of every covered texel and by the map's own standard error.  A frame's filter (mcpt_progressive_denoise)
 * cannot be pointed at a lightmap: neighbours in the map need not be neighbours in the world, there is no depth, material or albedo, and
 * gutter texels carry no data.  The call takes maps, not a bake, so it serves mcpt_bake_lightmap, mcpt_bake_lightmap_adaptive and maps
 * the caller has accumulated: irradiance3[W*H*3] and stderr3[W*H*3] as a bake writes them, out3[W*H*3], owner[W*H] (may be NULL).  out3 may
 * be the same buffer as irradiance3: every input is read before anything is written.  BAKE WITH dilate = 0 AND LET THIS CALL DILATE: it
 * dilates after it filters, and never reads a texel that is not covered.
 * THE DENOISED MAP IS BIASED: it trades variance for a bias towards the neighbours' values.  A MAP WHOSE stderr3 IS 0 COMES BACK
 * ESSENTIALLY UNFILTERED (the luminance stop is closed: only taps of exactly the same luminance count) -- a bake with spp = 1 is such a map.
 * The struct carries the map's size, so there is no all-zero-means-defaults rule: iterations is K as given, 0 .. 10 (0: no filtering), a
 * sigma of 0 is its default, dilate = R rounds, 0 .. 64.  The filter, in fp64 without contraction, every sum in the order written:
 *   coverage : mcpt_bake_lightmap's step 1 on the same chart (uv6 as there; NULL: the scene's own vt) gives owner[T].  T is COVERED when
 *              owner[T] >= 0.  Only covered texels are read from irradiance3 and stderr3: anything may stand at the others, NaN and the
 *              results of an earlier dilation included.
 *   guides   : of a covered texel T with owner f.  Position p and normal n are the q6 of T's entry of mcpt_lightmap_texels, bit for bit.
 *              n^ = n divided by its length sqrt((n_x n_x + n_y n_y) + n_z n_z); a zero normal stays 0.  The footprint h is the world
 *              length of a texel's side on f: e1 = v2 - v1, e2 = v3 - v1 from the device's current vertices,
 *              c = e1 x e2 = (e1_y e2_z - e1_z e2_y, e1_z e2_x - e1_x e2_z, e1_x e2_y - e1_y e2_x), A2 = sqrt((c_x c_x + c_y c_y) + c_z c_z),
 *              h = sqrt(A2 / (|area2_f| * (double(W) * double(H)))), area2_f the chart's of coverage.
 *   input    : e = irradiance3[T]; lum(e) = (0.2126 e_0 + 0.7152 e_1) + 0.0722 e_2; v = sum_c (w_c * w_c) * (se_c * se_c) from 0.0,
 *              se = stderr3[T], w = (0.2126, 0.7152, 0.0722), channels in order.  There is no demodulation: irradiance carries no albedo.
 *   iteration i = 0 .. K-1, step s = 2^i, from (e, v) to (e', v'):
 *     g_p  = sum k_q v_q / sum k_q over the 3 x 3 window q = p + (dx, dy), dx, dy in -1..1 row-major, q inside the map and covered;
 *            k_q = b[dx] b[dy], b = (1/4, 1/2, 1/4).
 *     taps : q = p + s (dx, dy) for dy, dx in -2..2, row-major; a tap counts when q is inside the map and covered.
 *     w_pq = ((h[dx] h[dy]) N_pq) exp(-D_pq - L_pq),   h = (1/16, 1/4, 3/8, 1/4, 1/16),
 *            N_pq = max(0, (n^_p.x n^_q.x + n^_p.y n^_q.y) + n^_p.z n^_q.z)^128 by seven squarings, 1 at the centre tap,
 *            L_pq = |lum(e_q) - lum(e_p)| / (sigma_l sqrt(g_p) + 1e-10),
 *            D_pq = max(0, t_pq) / sigma_p (t_pq > 0 ? t_pq : 0: a NaN counts as 0), 0 at the centre tap,
 *            t_pq = r_pq / ((h_p s) len) - 1, r_pq = sqrt((x x + y y) + z z) of (x, y, z) = p_q - p_p, len = sqrt(double(dx dx + dy dy)).
 *            D is the excess of the world distance over what a continuous, isotropic chart gives at that tap: 0 inside a well-behaved
 *            chart, growing with stretch, enormous across an atlas seam -- which is what keeps unrelated charts apart.
 *     e'_p = (sum w_pq e_q) / sum w_pq per channel,  v'_p = (sum (w_pq w_pq) v_q) / (sum w_pq * sum w_pq).
 *   output   : a covered texel gets e after K iterations (K = 0: its input, bit for bit), every other texel +0.0.  Then R rounds of
 *              mcpt_bake_lightmap's dilation run on out3, word for word: valid means covered, filled texels read -1 - r in owner.
 * Defaults: MCPT_LIGHTMAP_DENOISE_ITERATIONS for the Python face (the C struct's K is taken as given), sigma_l =
 * MCPT_LIGHTMAP_DENOISE_SIGMA_L, sigma_p = MCPT_LIGHTMAP_DENOISE_SIGMA_P.  Every output is one GPU lane's fixed-order sum: the same bits
 * on any MI355X, on every call.
 * The host form is synchronous.  The _device form takes device pointers throughout, enqueues on `stream` and DOES NOT WAIT FOR ANYTHING
 * it enqueues: it runs map-wide and needs no texel count back.  Like a bake, a call first waits for the event behind the device's previous
 * bake or denoise, and it keeps its workspace in the device: about 128 bytes per texel of the largest map so far (a 64-byte guide record
 * and two 32-byte (e, v) records), beside the baker's 4 bytes per texel and 8 per face, and with dilation 28 more per texel.  A map for
 * which that cannot be allocated returns MCPT_ERR_NOMEM and leaves the device usable.
 * Errors (MCPT_ERR_ARG, before MCPT_ERR_NO_DEVICE, in this order): NULL parameters, a size outside 1 .. 16384, iterations outside 0 .. 10,
 * dilate outside 0 .. 64, a sigma that is negative or not finite, reserved != 0, NULL irradiance3, stderr3 or out3.  In the host form a
 * chart component that is not finite is refused where mcpt_bake_lightmap refuses it; the call meets a motion as a bake does.
 * Not covered: stitching across seams (filtering between charts that are adjacent in the world but apart in the atlas); temporal or
 * multi-bake accumulation; a denoise option inside mcpt_bake_lightmap*; SH or directional lightmaps; the multi-device group and
 * render_scene; the use of a lightmap in shading. */
#define MCPT_LIGHTMAP_DENOISE_ITERATIONS      5
#define MCPT_LIGHTMAP_DENOISE_MAX_ITERATIONS  10
#define MCPT_LIGHTMAP_DENOISE_SIGMA_L         2.0
#define MCPT_LIGHTMAP_DENOISE_SIGMA_P         1.0
typedef struct { int32_t width, height, iterations, dilate;
                 double sigma_l, sigma_p;          /* 0 = the default */
                 int32_t reserved[2]; } mcpt_lightmap_denoise_params;
int mcpt_lightmap_denoise(mcpt_device*, const double* uv6, const mcpt_lightmap_denoise_params*,
                          const double* irradiance3, const double* stderr3, double* out3, int32_t* owner);
int mcpt_lightmap_denoise_device(mcpt_device*, const double* d_uv6, const mcpt_lightmap_denoise_params*,
                                 const double* d_irradiance3, const double* d_stderr3, double* d_out3, int32_t* d_owner,
                                 void* stream);

/* ---- irradiance volumes (since the volume change; MCPT_VERSION stays 105: detect the block by symbol) ---- */
/* AN IRRADIANCE VOLUME is a regular grid of light probes and a lookup that answers "the irradiance at this point for this normal" by
 * blending the eight probes around the point trilinearly and evaluating the blend as mcpt_sh_irradiance evaluates one probe.  It lights
 * moving objects and surfaces without a chart, and it is a cheap stand-in for a lightmap.  fp64, no contraction, IEEE division, every
 * sum in the order written.
 *   grid     : nx * ny * nz probes.  Probe (ix, iy, iz) has index P = (iz * ny + iy) * nx + ix and, on axis a, the coordinate
 *              origin[a] + double(i_a) * spacing[a].  A valid grid: origin finite; spacing finite and > 0 on every axis, also where the
 *              count is 1; every count >= 1 and nx * ny * nz <= 2^31 - 1 (in 64 bits); flags 0 or MCPT_VOLUME_CLAMP_ZERO; reserved 0.
 *              mcpt_volume_points writes the positions, p3[nprobes * 3], on the host: no device.
 *   bake     : A BAKE IS, BIT FOR BIT, mcpt_query_sh OVER mcpt_volume_points OF THE GRID WITH ids == NULL: the RNG key id of probe P is
 *              P; sh27 [nprobes][9][3] is required, stderr27 and hits [nprobes] may be NULL; stats->rays_primary = samples = nprobes *
 *              spp.  The positions are written on the GPU into a list the device keeps (24 bytes per probe of the largest grid so far);
 *              keys, shading, sample ranges, flags, chunking, concurrency and the motion rule are mcpt_query_sh's, word for word.
 *   lookup   : receiver r is q6[r] = position x, normal b of any non-zero finite length -- the hemisphere query's list format, so
 *              mcpt_lightmap_texels' q6 goes in unchanged.  Per axis a with n probes:
 *                g = (x_a - origin_a) / spacing_a, g = g > 0.0 ? g : 0.0, g = g < double(n - 1) ? g : double(n - 1): a point outside
 *                the grid takes the border's value;
 *                n == 1: i0 = i1 = 0, f = 0.0;   n >= 2: i0 = min(int(floor(g)), n - 2), i1 = i0 + 1, f = g - double(i0) (1.0 on the
 *                far border); then THE SNAP: f = 0.0 when x_a == origin_a + double(i0) * spacing_a, else f = 1.0 when x_a == origin_a +
 *                double(i1) * spacing_a -- a coordinate that is a probe's own, bit for bit, belongs to that probe alone (g does not
 *                give a probe's index back exactly unless origin and spacing are dyadic: (0.1 + 0.3 - 0.1) / 0.3 is 1 + 2^-52);
 *                w0 = 1.0 - f, w1 = f.
 *              Corner j = dz * 4 + dy * 2 + dx, j = 0 .. 7, is probe P_j = (i_dz * ny + i_dy) * nx + i_dx with weight
 *              w_j = (wx_dx * wy_dy) * wz_dz.
 *   mask     : valid is NULL or one byte per probe.  With a mask, w_j = 0.0 where valid[P_j] == 0; W = sum_j w_j in j order from 0.0;
 *              W > 0: w_j = w_j / W; otherwise every output of the receiver is +0.0.  Without a mask nothing is divided.
 *              corners[r] (may be NULL) = the number of j with w_j > 0 after masking.
 *   value    : c[i][ch] = sum_j w_j * sh[P_j][i][ch] in j order from 0.0; n^ and A_l as in mcpt_sh_irradiance;
 *              E_ch = sum_i (A_l(i) * Y_i(n^)) * c[i][ch] in i order from 0.0; under MCPT_VOLUME_CLAMP_ZERO, last,
 *              E_ch = E_ch > 0.0 ? E_ch : 0.0 (order-2 ringing can go negative).  Hence A RECEIVER EXACTLY ON PROBE P GETS
 *              mcpt_sh_irradiance(sh[P], b), BIT FOR BIT, with or without a mask that keeps P: weights of exactly 1 and 0 give exact
 *              sums when the coefficients are finite.  Every output is one lane's fixed-order sum: the same bits on the host and on the GPU.
 * The lookup takes coefficient arrays, not a bake: accumulated, edited or loaded volumes go through it.  mcpt_volume_irradiance_host runs
 * on the CPU and needs no device.  The host-pointer forms are synchronous and copy in and out around the device form.  The _device forms
 * take device pointers throughout and enqueue on `stream`: the bake returns without waiting when stats == NULL, after first waiting for
 * the event behind the device's previous bake; the lookup never waits and allocates nothing.
 * Errors (MCPT_ERR_ARG, before MCPT_ERR_NO_DEVICE, in this order): a NULL grid or NULL parameters; an invalid grid, in the field order
 * above; the bake: mcpt_query_sh's refusals in its order; the lookup: n < 0 or n > 2^31 - 1, then NULL sh27, q6 or e3 with n > 0.  The
 * host-pointer forms of the lookup also refuse a coefficient or a position that is not finite and a normal mcpt_sh_irradiance would
 * refuse; THE DEVICE FORM DOES NOT LOOK, and its result for such input is unspecified (it still reads no probe outside the grid).
 * n == 0: MCPT_OK, nothing is launched.  A probe list or a copy that cannot be allocated: MCPT_ERR_NOMEM, and the device stays usable.
 * Not covered: a standard error of the lookup (the coefficients of one probe share their samples: a sum of squares would be wrong);
 * finding invalid probes and visibility-weighted interpolation here (both are the probe visibility block's below: its bake fills the
 * mask, its lookup weighs every corner by what the probe sees); radiance (glossy) lookup and returning the blended coefficients; adaptive probes; the multi-device group and render_scene.  Lighting a
 * frame from the volume is the baked frames' block's, below. */
#define MCPT_VOLUME_CLAMP_ZERO 1   /* E_c = max(E_c, 0.0): order-2 ringing can go negative */
typedef struct { double origin[3], spacing[3]; int32_t nx, ny, nz, flags; int32_t reserved[4]; } mcpt_volume_grid;
int mcpt_volume_points(const mcpt_volume_grid*, double* p3);
int mcpt_bake_volume(mcpt_device*, const mcpt_volume_grid*, const mcpt_sh_params*,
                     double* sh27, double* stderr27, int32_t* hits, mcpt_stats*);
int mcpt_bake_volume_device(mcpt_device*, const mcpt_volume_grid*, const mcpt_sh_params*,
                            double* d_sh27, double* d_stderr27, int32_t* d_hits, mcpt_stats*, void* stream);
int mcpt_volume_irradiance_host(const mcpt_volume_grid*, const double* sh27, const uint8_t* valid,
                                const double* q6, int64_t n, double* e3, int32_t* corners);
int mcpt_volume_irradiance(mcpt_device*, const mcpt_volume_grid*, const double* sh27, const uint8_t* valid,
                           const double* q6, int64_t n, double* e3, int32_t* corners);
int mcpt_volume_irradiance_device(mcpt_device*, const mcpt_volume_grid*, const double* d_sh27, const uint8_t* d_valid,
                                  const double* d_q6, int64_t n, double* d_e3, int32_t* d_corners, void* stream);

/* ---- probe visibility (since the visibility change; MCPT_VERSION stays 105: detect the block by symbol) ---- */
/* PROBE VISIBILITY is what a probe sees of its surroundings: per probe an R x R octahedral map of the mean and mean square of the distance
 * to the nearest surface, and the number of its rays that hit a surface from behind.  The second finds the probes that sit inside
 * geometry (the mask of the irradiance volumes' lookup); the first lets a lookup take away the weight of a probe that cannot see the
 * receiver, so that light no longer leaks through walls.  fp64, no contraction, IEEE division, every expression and sum in the order
 * written.
 *   bin      : mcpt_visibility_bin, bin[i] of direction d3[i] = (x, y, z) in a map of res = R in 1 .. 16 (host, no device):
 *                l = (|x| + |y|) + |z|, u = x / l, v = y / l;
 *                z < 0.0: (u, v) = ((1.0 - |v|) * (u >= 0.0 ? 1.0 : -1.0), (1.0 - |u|) * (v >= 0.0 ? 1.0 : -1.0)), from the old u and v;
 *                bx = int(floor((u * 0.5 + 0.5) * double(R))) clamped to 0 .. R - 1, by likewise from v; bin = by * R + bx.
 *              The helper refuses a direction that is not finite or whose l is 0 or overflows; the kernels put such a direction into
 *              bin 0 and never outside the table.
 *   rays     : sample j of probe i is the ray mcpt_query_sh gives it: the sphere draw of (seed, ids[i] or i, sample_base + j) from the
 *              point itself.  A PROBE'S VISIBILITY RAYS ARE ITS RADIANCE RAYS, BIT FOR BIT, for the same seed, id and sample range.
 *   trace    : the closest hit mcpt_trace_closest_device answers (the device's trace mode and engine, key 0 of a motion, a geometry
 *              that stands), through the same walks; the rays are drawn on the GPU into a workspace the device keeps.
 *   fold     : per probe, in j order, with d the ray's direction, t the hit's distance and n the hit triangle's stored face normal
 *              (mcpt_scene_get_faces: geom27[24..26]):
 *                hit = the ray hit anything; hits += hit; back += hit && ((d.x n.x + d.y n.y) + d.z n.z) > 0.0;
 *                r = hit ? (t < max_distance ? t : max_distance) : max_distance;
 *                b = bin(d, R); c[b] += 1, s1[b] += r, s2[b] += r * r.
 *              The stored normal is normalize(cross(v1 - v2, v3 - v1)) of the face's vertices, the library's rule everywhere: `back`
 *              means what it says in a scene whose faces wind so that this normal points into free space.  A scene wound the other way
 *              (cornell-box is) reports every hit as a back-face hit: its caller takes the mask from hits - back instead.
 *   outputs  : moments[i][b] = (s1 / c, s2 / c), [n][R * R][2]; a bin with c == 0 holds (-1.0, 0.0): "no data".  hits[i], back[i];
 *              valid[i] = double(back) <= max_back_fraction * double(spp) ? 1 : 0.  moments is required; hits, back and valid may be NULL.
 *              stats->rays_primary = samples = n * spp, launches = the number of chunks; the other fields are 0.
 *   chunks   : the call works in chunks of whole probes: at most workspace_rays rays and at least one probe each; 0 selects 4 194 304
 *              rays.  The workspace holds 84 bytes per ray of the largest chunk so far.  THE RESULT DOES NOT DEPEND ON THE CHUNKING:
 *              every sum belongs to one probe and is added in j order.
 *   grid form: A VOLUME VISIBILITY BAKE IS, BIT FOR BIT, mcpt_query_visibility OVER mcpt_volume_points OF THE GRID WITH ids == NULL;
 *              the points are written on the GPU into the volume's own list.
 *   lookup   : mcpt_volume_irradiance with one factor per corner.  P_j and the trilinear w_j are that call's, the snap included.
 *              valid == NULL is a mask of ones; w_j = 0.0 where valid[P_j] == 0.  With n^ the receiver's unit normal (b / sqrt((bx bx
 *              + by by) + bz bz)), x' = x + n^ * normal_bias per component, (vx, vy, vz) = x' - c_j with c_j the probe's position,
 *              dist = sqrt((vx vx + vy vy) + vz vz):
 *                dist == 0.0: f = 1.0.  Otherwise b = bin(v / dist, R), (mu, m2) = moments[P_j][b];
 *                mu < 0.0: f = 1.0.  Otherwise dc = dist < max_distance ? dist : max_distance;
 *                dc <= mu: f = 1.0.  Otherwise var = m2 - mu * mu, var = var > 0.0 ? var : 0.0, delta = dc - mu,
 *                ch = var / (var + delta * delta), f = (ch * ch) * ch                                    (Chebyshev's bound, cubed);
 *                last, f = f > min_visibility ? f : min_visibility.
 *              w_j = w_j * f_j; W = sum_j w_j in j order from 0.0; W > 0: w_j = w_j / W, otherwise every output of the receiver is
 *              +0.0 and corners[r] = 0.  The value and the clamp are mcpt_volume_irradiance's; corners[r] = the number of w_j > 0.
 *              Hence (a) WITH EVERY FACTOR 1 (moments all (-1, 0)) THE CALL IS mcpt_volume_irradiance UNDER THE SAME MASK (all ones
 *              where NULL), BIT FOR BIT, and (b) with normal_bias == 0 A RECEIVER EXACTLY ON A VALID PROBE P GETS
 *              mcpt_sh_irradiance(sh[P], b), BIT FOR BIT.  mcpt_volume_irradiance_visible_host runs on the CPU and needs no device.
 * The host-pointer forms are synchronous and copy in and out around the device forms.  The _device forms take device pointers throughout
 * and enqueue on `stream`.  The bakes return without waiting when stats == NULL, after first waiting for the event behind the device's
 * previous visibility bake (and, the grid form, its previous volume bake); they use the counters and queue words of
 * mcpt_trace_closest_device and, like it, must not overlap another closest-hit call of the same device on another stream.  The lookup
 * never waits and allocates nothing; IT DOES NOT LOOK AT ITS ARRAYS and reads no probe or bin outside its tables.
 * Errors (MCPT_ERR_ARG, before MCPT_ERR_NO_DEVICE, in this order).  The bakes: NULL parameters (the grid form: a NULL grid or NULL
 * parameters, then an invalid grid in its field order); spp < 1; sample_base < 0; sample_base + spp > 2^31 - 1; res outside 1 .. 16;
 * max_distance not finite or <= 0; max_back_fraction not finite or outside [0, 1]; workspace_rays < 0; reserved0 or reserved != 0;
 * n < 0 or n > 2^31 - 1; NULL p3 or moments with n > 0; the host-pointer list form: a negative id or a position that is not finite.
 * The lookups: the grid's errors; a NULL mcpt_volume_visibility; res outside 1 .. 16; flags != 0; max_distance not finite or <= 0;
 * normal_bias not finite or < 0; min_visibility not finite or outside [0, 1]; reserved != 0; n < 0 or n > 2^31 - 1; NULL sh27, moments,
 * q6 or e3 with n > 0; the host-pointer forms: mcpt_volume_irradiance's array checks, then a moment that is neither finite with a mean
 * >= 0 nor exactly (-1.0, 0.0).  mcpt_visibility_bin: n < 0, NULL d3 or bin with n > 0, res outside 1 .. 16, then the directions.
 * n == 0: MCPT_OK, nothing is launched.  A workspace or a copy that cannot be allocated: MCPT_ERR_NOMEM, and the device stays usable.
 * Not covered: the normal-facing "wrap" weight and the weight crush of DDGI; a view bias; relocating probes; filtered (lobe-blended)
 * depth maps; fp32 or fp16 moment storage; a ray source inside the engines (the rays go through a workspace); the multi-device group
 * and render_scene. */
typedef struct { int32_t spp, sample_base; uint64_t seed; int32_t res, reserved0;
                 double max_distance, max_back_fraction; int64_t workspace_rays; int32_t reserved[2]; } mcpt_visibility_params;
typedef struct { int32_t res, flags; double max_distance, normal_bias, min_visibility; int32_t reserved[4]; } mcpt_volume_visibility;
int mcpt_visibility_bin(const double* d3, int64_t n, int32_t res, int32_t* bin);
int mcpt_query_visibility(mcpt_device*, const double* p3, const int32_t* ids, int64_t n, const mcpt_visibility_params*,
                          double* moments, int32_t* hits, int32_t* back, uint8_t* valid, mcpt_stats*);
int mcpt_query_visibility_device(mcpt_device*, const double* d_p3, const int32_t* d_ids, int64_t n, const mcpt_visibility_params*,
                                 double* d_moments, int32_t* d_hits, int32_t* d_back, uint8_t* d_valid, mcpt_stats*, void* stream);
int mcpt_bake_volume_visibility(mcpt_device*, const mcpt_volume_grid*, const mcpt_visibility_params*,
                                double* moments, int32_t* hits, int32_t* back, uint8_t* valid, mcpt_stats*);
int mcpt_bake_volume_visibility_device(mcpt_device*, const mcpt_volume_grid*, const mcpt_visibility_params*,
                                       double* d_moments, int32_t* d_hits, int32_t* d_back, uint8_t* d_valid, mcpt_stats*, void* stream);
int mcpt_volume_irradiance_visible_host(const mcpt_volume_grid*, const double* sh27, const double* moments, const uint8_t* valid,
                                        const mcpt_volume_visibility*, const double* q6, int64_t n, double* e3, int32_t* corners);
int mcpt_volume_irradiance_visible(mcpt_device*, const mcpt_volume_grid*, const double* sh27, const double* moments, const uint8_t* valid,
                                   const mcpt_volume_visibility*, const double* q6, int64_t n, double* e3, int32_t* corners);
int mcpt_volume_irradiance_visible_device(mcpt_device*, const mcpt_volume_grid*, const double* d_sh27, const double* d_moments,
                                          const uint8_t* d_valid, const mcpt_volume_visibility*, const double* d_q6, int64_t n,
                                          double* d_e3, int32_t* d_corners, void* stream);

/* ---- baked frames (since the baked-frame change; MCPT_VERSION stays 105: detect the block by symbol) ---- */
/* A BAKED FRAME shows what a bake holds: every camera ray is traced for its closest hit and the surface there is lit by the irradiance a
 * lightmap or an irradiance volume stores, L = kd * E / pi -- global illumination from one ray per camera sample.  Three layers, each a
 * test seam of the next: the lightmap's lookup by chart coordinate, the baked radiance along a caller's rays, the frame.  fp64, no
 * contraction, IEEE division, every expression and sum in the order written; every output is one lane's fixed-order sum: the same bits on
 * the host and on the GPU, whatever the launch shape and the chunking.
 *   lightmap lookup : mcpt_lightmap_irradiance*, the counterpart of mcpt_volume_irradiance*.  A map of width x height texels (each in
 *              1 .. 16384), irradiance3[W * H * 3], owner[W * H] or NULL, as mcpt_bake_lightmap writes them: texel x has its centre at
 *              (x + 0.5) / W, row 0 is the row nearest v = 0, no flip, no wrap.  For chart coordinate uv2[i] = (u, v), per axis (u with W,
 *              v with H):
 *                s = u * double(W) - 0.5; s = s > 0.0 ? s : 0.0; s = s < double(W - 1) ? s : double(W - 1)  -- THE CLAMP IS IN DOUBLE,
 *                before any conversion to int: a coordinate of 1e300 takes the border's texel, a NaN lands on texel 0;
 *                W == 1: i0 = i1 = 0, f = 0.0;   W >= 2: i0 = min(int(floor(s)), W - 2), i1 = i0 + 1, f = s - double(i0);
 *                w0 = 1.0 - f, w1 = f.
 *              Tap j = dy * 2 + dx, j = 0 .. 3, is texel T_j = y_dy * W + x_dx with weight w_j = wx_dx * wy_dy.  With an owner map,
 *              w_j = 0.0 where owner[T_j] == -1 (never covered, never filled by dilation); S = sum_j w_j in j order from 0.0; S > 0:
 *              w_j = w_j / S; otherwise E = +0.0 and taps = 0.  With owner == NULL nothing is divided.
 *              E_c = sum_j w_j * irradiance3[T_j][c] in j order from 0.0; taps[i] (may be NULL) = the number of j with w_j > 0.  Hence a
 *              coordinate whose s comes out a whole number on both axes gets that texel's value, bit for bit (finite maps).
 *   source   : mcpt_baked_source names what lights the surfaces.  MCPT_BAKED_VOLUME: grid, sh27 and valid (may be NULL) as
 *              mcpt_volume_irradiance takes them; with moments != NULL also visibility, and the lookup is
 *              mcpt_volume_irradiance_visible's.  MCPT_BAKED_LIGHTMAP: width, height, irradiance3 and owner (may be NULL) as above, and
 *              the chart uv6[num_faces][6] in .obj order, NULL: the faces' own vt -- exactly as mcpt_bake_lightmap reads a chart.  The
 *              fields of the other kind are not read.  In the host-pointer calls every pointer is a host pointer, in the _device calls a
 *              device pointer (grid and visibility are always host structs).
 *   baked radiance : mcpt_baked_radiance*, rays6[n][6] = origin, direction as mcpt_trace_closest takes them, answered by its walks (the
 *              device's trace mode and engine, its current geometry, key 0 of a motion).  With d the ray's direction and p the hit:
 *                kind = MCPT_BAKED_MISS (0), MCPT_BAKED_EMITTER (1: the hit material is a light) or MCPT_BAKED_SURFACE (2);
 *                MISS    : L = Le(d) as mcpt_environment_eval gives it when the device has an active environment, else +0.0;
 *                EMITTER : L = the light's radiance (what a camera sample that hits an emitter shows);
 *                SURFACE : kd = the diffuse colour shading forms there, texel included (mcpt_progressive_aovs' albedo); n = pn of
 *                          mcpt_trace_closest, replaced by the face's stored normal when (nx nx + ny ny) + nz nz is 0 or not finite;
 *                          under MCPT_BAKED_FACE_VIEWER n = -n when ((dx nx + dy ny) + dz nz) > 0.0.
 *                          Volume: E, lit = the lookup's e3 and corners at q6 = (p, n).
 *                          Lightmap: g = the barycentrics of p as mcpt_trace_closest forms them for pn (the quotient form);
 *                          (au .. cv) = the chart row of the hit face; u = (au * g.x + bu * g.y) + cu * g.z, v likewise;
 *                          E, lit = the lightmap lookup's e3 and taps at (u, v).
 *                          L_c = (kd_c * E_c) / 3.141592653589793; under MCPT_BAKED_LIGHTING_ONLY L_c = E_c / 3.141592653589793.
 *              mcpt_baked_outputs, every pointer may be NULL: radiance3[n][3], kind[n], face[n] (the .obj index, -1: a miss), q6[n][6]
 *              (p and the n that went into the lookup), uv2[n][2] (+0.0 under a volume), kd3[n][3], e3[n][3], lit[n].  For a ray that
 *              is not a surface hit everything but radiance3, kind and face is +0.0 or 0.  Glass and mirrors show kd * E / pi like any
 *              other surface here; mcpt_baked_radiance_specular (baked specular, below) adds their ks * R.  stats: rays_primary = samples = n, launches = the number of chunks (of at most 4 194 304 rays).
 *   frame    : mcpt_render_baked*.  For every pixel of the device's frame, sample k = 0 .. samples - 1 is the frame's own camera ray of
 *              (pixel, k): mcpt_camera_rays of (seed, pixel, k) under the device's lens, shaded as above under `flags`.
 *              img[pixel][c] = s / double(samples), s = 0.0 + L_0 + ... in k order: mcpt_render's layout, so mcpt_display_device takes
 *              it as it is.  counts3[pixel] (may be NULL) = (surface, emitter, miss) samples; lit[pixel] (may be NULL) = the surface
 *              samples whose lookup had lit > 0.  The call works in chunks of whole pixels of at most workspace_rays rays (0: 4 194 304)
 *              and at least one pixel; stats: rays_primary = samples = pixels * samples, launches = the number of chunks.
 * mcpt_lightmap_irradiance_host runs on the CPU and needs no device.  The host-pointer forms are synchronous and copy in and out around
 * the _device forms.  The _device forms take device pointers throughout and enqueue on `stream`.  mcpt_baked_radiance_device and
 * mcpt_render_baked_device keep a workspace on the device (116 bytes per ray of the largest chunk so far), first wait for the event behind
 * the device's previous baked call, and return without waiting when stats == NULL (the first frame of a device also makes the lens's
 * image-plane points and waits for them); they use the counters and queue words of mcpt_trace_closest_device and, like it, must not
 * overlap another closest-hit call of the same device on another stream.  The lightmap lookup never waits and allocates nothing.
 * Errors (MCPT_ERR_ARG, before MCPT_ERR_NO_DEVICE, in this order).  The lightmap lookup: a size outside 1 .. 16384; n < 0 or n > 2^31 - 1;
 * NULL irradiance3, uv2 or e3 with n > 0; the host-pointer forms: a coordinate that is not finite.  A source: NULL; kind neither
 * MCPT_BAKED_VOLUME nor MCPT_BAKED_LIGHTMAP; flags != 0; reserved != 0; a volume: the grid's errors (NULL first), NULL sh27, and with
 * moments a NULL visibility and then its errors in mcpt_volume_irradiance_visible's order; a lightmap: a size outside 1 .. 16384, NULL
 * irradiance3.  mcpt_baked_radiance*: the source; a flag other than MCPT_BAKED_FACE_VIEWER | MCPT_BAKED_LIGHTING_ONLY; n < 0 or
 * n > 2^31 - 1; NULL rays6 with n > 0; NULL outputs; outputs' reserved != 0.  mcpt_render_baked*: the source; NULL parameters; samples
 * outside 1 .. 65536; a flag other than the two above; workspace_rays < 0; reserved != 0; NULL img.  In the
 * host-pointer forms a chart component that is not finite is MCPT_ERR_ARG as well -- after the missing device and the NULL device, because
 * the chart's length is the device's face count.  THE DEVICE FORMS DO NOT LOOK AT THEIR ARRAYS and read no texel or probe outside their
 * tables.  n == 0: MCPT_OK, nothing is launched.  A workspace or a copy that cannot be allocated: MCPT_ERR_NOMEM, and the device stays usable.
 * Not covered: direct light or shadows added on top of the bake; glass transport (refraction); standard errors of a baked frame;
 * mip-mapping or anisotropic filtering of the map; chart-aware taps beyond the owner rule; partitions, the multi-device group and
 * render_scene; a baked source inside the progressive handles. */
#define MCPT_BAKED_VOLUME    1
#define MCPT_BAKED_LIGHTMAP  2
#define MCPT_BAKED_MISS      0
#define MCPT_BAKED_EMITTER   1
#define MCPT_BAKED_SURFACE   2
#define MCPT_BAKED_FACE_VIEWER    1   /* the shading normal faces the ray's origin */
#define MCPT_BAKED_LIGHTING_ONLY  2   /* L = E / pi: the lighting without the surface's colour */
typedef struct { int32_t kind, flags;
                 const mcpt_volume_grid* grid; const double* sh27; const uint8_t* valid;
                 const double* moments; const mcpt_volume_visibility* visibility;
                 const double* uv6; int32_t width, height; const double* irradiance3; const int32_t* owner;
                 int64_t reserved[4]; } mcpt_baked_source;
typedef struct { double* radiance3; int32_t* kind; int32_t* face; double* q6; double* uv2; double* kd3; double* e3; int32_t* lit;
                 int64_t reserved[2]; } mcpt_baked_outputs;
typedef struct { int32_t samples, flags; uint64_t seed; int64_t workspace_rays; int32_t reserved[2]; } mcpt_baked_frame_params;
int mcpt_lightmap_irradiance_host(int32_t width, int32_t height, const double* irradiance3, const int32_t* owner,
                                  const double* uv2, int64_t n, double* e3, int32_t* taps);
int mcpt_lightmap_irradiance(mcpt_device*, int32_t width, int32_t height, const double* irradiance3, const int32_t* owner,
                             const double* uv2, int64_t n, double* e3, int32_t* taps);
int mcpt_lightmap_irradiance_device(mcpt_device*, int32_t width, int32_t height, const double* d_irradiance3, const int32_t* d_owner,
                                    const double* d_uv2, int64_t n, double* d_e3, int32_t* d_taps, void* stream);
int mcpt_baked_radiance(mcpt_device*, const mcpt_baked_source*, const double* rays6, int64_t n, int32_t flags,
                        const mcpt_baked_outputs*, mcpt_stats*);
int mcpt_baked_radiance_device(mcpt_device*, const mcpt_baked_source*, const double* d_rays6, int64_t n, int32_t flags,
                               const mcpt_baked_outputs*, mcpt_stats*, void* stream);
int mcpt_render_baked(mcpt_device*, const mcpt_baked_source*, const mcpt_baked_frame_params*,
                      double* img, int32_t* counts3, int32_t* lit, mcpt_stats*);
int mcpt_render_baked_device(mcpt_device*, const mcpt_baked_source*, const mcpt_baked_frame_params*,
                             double* d_img, int32_t* d_counts3, int32_t* d_lit, mcpt_stats*, void* stream);

/* ---- reflection probes (since the reflection-probe change; MCPT_VERSION stays 105: detect the block by symbol) ---- */
/* A REFLECTION PROBE is a point in free space that holds an R x R octahedral map of the radiance arriving there.  A CHAIN is 1 to 8 maps
 * filtered from it with Phong lobes cos^ns of chosen integer exponents -- the lobe RT_SPECULAR draws from, which is radially symmetric
 * about the mirror direction, so the filtered map is exactly what a glossy surface of that exponent sees; there is no split-sum
 * approximation.  A LOOKUP answers "the radiance from direction d for a lobe of exponent x".  fp64, no contraction, IEEE division, every
 * expression and sum in the order written; every output is one lane's fixed-order sum: the same bits on the host and on the GPU, whatever
 * the launch shape and the chunking.
 *   encode   : direction (x, y, z) of any non-zero finite length -> (s, t) in [0, 1]^2, mcpt_visibility_bin's map continued:
 *                l = (|x| + |y|) + |z|, u = x / l, v = y / l;
 *                z < 0.0: (u, v) = ((1.0 - |v|) * (u >= 0.0 ? 1.0 : -1.0), (1.0 - |u|) * (v >= 0.0 ? 1.0 : -1.0)), from the old u and v;
 *                s = u * 0.5 + 0.5, t = v * 0.5 + 0.5.
 *   decode   : (s, t) -> d: u = 2.0 * s - 1.0, v = 2.0 * t - 1.0, z = (1.0 - |u|) - |v|; z < 0.0: the same fold of (u, v);
 *                d = (u, v, z) / sqrt((u u + v v) + z z).
 *   texels   : texel b = y * R + x has its centre at ((x + 0.5) / R, (y + 0.5) / R); d_b = decode(centre);
 *                w_b = ((2.0 / R) * (2.0 / R)) / (n2 * sqrt(n2)), n2 = (u u + v v) + z z of the centre's folded, unnormalised (u, v, z): the
 *                midpoint-rule solid angle du dv / |p|^3.  mcpt_reflection_texels(res, d3, w) gives both for res in 1 .. 256 (host, no
 *                device; either pointer may be NULL).  mcpt_visibility_bin(d_b, R) == b for R in 1 .. 16.
 *   wrap     : a tap (x, y) with x, y in -1 .. R: (1) if x < 0 or x >= R: x = x < 0 ? -1 - x : 2R - 1 - x and y = R - 1 - y; (2) then the
 *                same test on y, with x = R - 1 - x.  All four edges of the square are seams of the lower hemisphere, all four corners
 *                the direction (0, 0, -1).
 *   ipow     : ipow(c, n), integer n >= 0, by binary squaring: r = 1.0, b = c; while n > 0: if n & 1: r = r * b; n >>= 1; if n: b = b * b.
 *                There is no pow.
 *   bake     : mcpt_bake_reflection*, n probes p3[n][3], S = spp samples per texel.  Sample j of texel b of probe i is entry
 *                e = (i * R * R + b) * S + j.  Its RNG id is id_base[i] + b * S + j (id_base == NULL: i * R * R * S) and its sample index
 *                k = sample_base for every entry; u0, u1 = words 0 and 1 of the camera-uniform block uniform(seed, id, k, depth 0xFFFF,
 *                slot 0..3), which MCPT_QUERY_HEMISPHERE draws from and MCPT_QUERY_RAY does not: nothing collides;
 *                d = decode((x + u0) / R, (y + u1) / R), o = p_i itself, no offset (a probe sits in free space).
 *                A BAKE IS, BIT FOR BIT, mcpt_query_radiance_device OVER THESE RAYS -- kind MCPT_QUERY_RAY, spp = 1, ids = the entries' ids,
 *                the same sample_base, seed and flags -- FOLDED PER TEXEL in j order with the query's own expressions: s1 += x,
 *                s2 += x * x, radiance = s1 / S, stderr = 0 when S < 2, else sqrt(max((s2 - s1 * s1 / S) / (S - 1), 0) / S); hits[b] = the
 *                samples whose ray hit anything.  (An id per sample keeps the paths of a texel's samples independent; a ray-kind query
 *                with spp > 1 would retrace one ray.)  Environment, light sampling, trace mode, motion (key 0) and concurrency are the
 *                query's rules, word for word.  radiance [n][R * R][3] is required; stderr [n][R * R][3] and hits [n][R * R] may be NULL.
 *                stats: rays_primary = samples = n * R * R * S; the other counters are the queries', summed over the chunks.
 *   chunks   : the bake works in chunks of whole texels: at most workspace_rays rays and at least one texel each; 0 selects 4 194 304
 *                rays.  The workspace holds 80 bytes per ray of the largest chunk so far.  THE RESULT DOES NOT DEPEND ON THE CHUNKING.
 *   test seam: mcpt_reflection_rays gives rays6[m][6] and ids[m] of the listed entries entry[m] (host pointers), made by the bake's own
 *                device function.
 *   chain    : mcpt_reflection_chain: res = the source map's R; num_levels in 1 .. 8; level_res[l] in 1 .. 256; level_ns[l] in
 *                0 .. 65535, strictly descending; unused slots 0.  Storage chain[n][T][3], T = sum of level_res[l]^2; level l starts at
 *                texel sum_{m < l} level_res[m]^2.
 *   prefilter: mcpt_reflection_prefilter*.  For output texel o of level l with centre direction r and ns = level_ns[l], over the source
 *                texels b in ascending order: c = (r.x d_b.x + r.y d_b.y) + r.z d_b.z; a texel with c > 0.0 contributes
 *                g = w_b * ipow(c, ns), W += g, A_ch += g * L_b[ch]; the others contribute nothing.  out = W > 0.0 ? A / W : +0.0.
 *                W == 0 happens: a 1 x 1 source lies in the upper hemisphere, and cos^65535 underflows between coarse texels.
 *   lookup   : mcpt_reflection_lookup*.  Receiver q has a probe index probe[q], a direction d3[q] of any non-zero finite length and an
 *                exponent x[q], finite and >= 0.  With wt(a) = 1.0 / sqrt(a + 1.0): one level, or x >= ns[0]: level 0 alone;
 *                x <= ns[L - 1]: the last level alone; otherwise l with ns[l] >= x > ns[l + 1],
 *                a = (wt(x) - wt(ns[l])) / (wt(ns[l + 1]) - wt(ns[l])); a == 0.0: level l alone, otherwise
 *                value = (1.0 - a) * v_l + a * v_{l+1} per channel.  Hence AN x EQUAL TO A LEVEL'S EXPONENT READS THAT LEVEL ALONE.
 *                Inside a level of size R: (s, t) = encode(d), a = s * R - 0.5, b = t * R - 0.5, each clamped to [-1, R - 0.5] IN DOUBLE
 *                before any conversion to int (a = a > -1.0 ? a : -1.0, then a = a < R - 0.5 ? a : R - 0.5: a NaN takes -1).  A direction
 *                a caller may give has a in [-0.5, R - 0.5] already: half a texel beyond a border the tap across the seam weighs as
 *                much as the border's own, at all four borders alike, which is what makes the lookup continuous across the seams.
 *                x0 = floor(a), fx = a - x0, y0 and fy likewise; the taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) go
 *                through the wrap; v = ((w00 m00 + w10 m10) + w01 m01) + w11 m11 with w00 = (1 - fx)(1 - fy), w10 = fx (1 - fy),
 *                w01 = (1 - fx) fy, w11 = fx fy.  In the device form a probe[q] outside 0 .. n - 1 gives +0.0.
 * mcpt_reflection_texels, mcpt_reflection_prefilter_host and mcpt_reflection_lookup_host run on the CPU and need no device.  The
 * host-pointer forms are synchronous and copy in and out around the _device forms.  The _device forms take device pointers throughout
 * (parameters and chain are always host structs) and enqueue on `stream`.  mcpt_bake_reflection_device first waits for the event behind
 * the device's previous reflection bake and returns without waiting when stats == NULL; otherwise it is a query call: it uses the
 * device's frame slot 0 and first waits for the device's frames in flight.  The prefilter and the lookup never wait and allocate
 * nothing; THEY DO NOT LOOK AT THEIR ARRAYS and read nothing outside their tables.
 * Errors (MCPT_ERR_ARG, before MCPT_ERR_NO_DEVICE, in this order).  The bake and mcpt_reflection_rays: NULL parameters; spp < 1;
 * sample_base < 0; res outside 1 .. 256; a flag other than 0 or MCPT_RENDER_MEGAKERNEL; workspace_rays < 0; reserved != 0; n < 0;
 * n * R * R * S > 2^31 - 1; the bake: NULL p3 or radiance with n > 0; the seam: m outside 0 .. 2^31 - 1, a NULL array with m > 0, an
 * entry outside 0 .. n * R * R * S - 1; the host-pointer forms: a position that is not finite, a negative id_base[i],
 * id_base[i] + R * R * S - 1 > 2^31 - 1 (the device form cannot look at id_base: its caller keeps every id within 0 .. 2^31 - 1).
 * A chain: NULL; res outside 1 .. 256; num_levels outside 1 .. 8; a level_res outside 1 .. 256 or an unused slot != 0; a level_ns
 * outside 0 .. 65535, not strictly descending, or an unused slot != 0; reserved != 0.  The prefilter: the chain; n < 0 or n > 2^31 - 1;
 * NULL radiance or chain with n > 0; the host-pointer forms: a radiance that is not finite.  The lookup: the chain; n, then m, outside
 * 0 .. 2^31 - 1; a NULL array with m > 0; the host-pointer forms: a chain value that is not finite, then per receiver a direction
 * that is zero, not finite or whose l overflows, a probe index outside 0 .. n - 1, an x that is not finite or < 0.
 * mcpt_reflection_texels: res outside 1 .. 256.  n == 0 (the lookup: m == 0): MCPT_OK, nothing is launched.  A workspace or a copy
 * that cannot be allocated: MCPT_ERR_NOMEM, and the device stays usable.
 * Not covered: parallax correction; nearest-probe choice and irregular probe sets; GGX or other lobes, and real-valued level exponents;
 * fp32 or fp16 storage; adaptive stopping; the multi-device group and render_scene.  (A specular term in baked frames and choosing or
 * blending probes by position stood here; the baked specular block below adds both, for probes on a volume grid.) */
typedef struct { int32_t spp, sample_base; uint64_t seed; int32_t res, flags; int64_t workspace_rays; int32_t reserved[4]; } mcpt_reflection_params;
typedef struct { int32_t res, num_levels; int32_t level_res[8], level_ns[8]; int32_t reserved[4]; } mcpt_reflection_chain;
int mcpt_reflection_texels(int32_t res, double* d3, double* w);
int mcpt_bake_reflection(mcpt_device*, const double* p3, const int32_t* id_base, int64_t n, const mcpt_reflection_params*,
                         double* radiance, double* stderr3, int32_t* hits, mcpt_stats*);
int mcpt_bake_reflection_device(mcpt_device*, const double* d_p3, const int32_t* d_id_base, int64_t n, const mcpt_reflection_params*,
                                double* d_radiance, double* d_stderr3, int32_t* d_hits, mcpt_stats*, void* stream);
int mcpt_reflection_rays(mcpt_device*, const double* p3, const int32_t* id_base, int64_t n, const mcpt_reflection_params*,
                         const int64_t* entry, int64_t m, double* rays6, int32_t* ids);
int mcpt_reflection_prefilter_host(const mcpt_reflection_chain*, const double* radiance, int64_t n, double* chain);
int mcpt_reflection_prefilter(mcpt_device*, const mcpt_reflection_chain*, const double* radiance, int64_t n, double* chain);
int mcpt_reflection_prefilter_device(mcpt_device*, const mcpt_reflection_chain*, const double* d_radiance, int64_t n, double* d_chain,
                                     void* stream);
int mcpt_reflection_lookup_host(const mcpt_reflection_chain*, const double* chain, int64_t n, const int32_t* probe, const double* d3,
                                const double* x, int64_t m, double* out3);
int mcpt_reflection_lookup(mcpt_device*, const mcpt_reflection_chain*, const double* chain, int64_t n, const int32_t* probe,
                           const double* d3, const double* x, int64_t m, double* out3);
int mcpt_reflection_lookup_device(mcpt_device*, const mcpt_reflection_chain*, const double* d_chain, int64_t n, const int32_t* d_probe,
                                  const double* d_d3, const double* d_x, int64_t m, double* d_out3, void* stream);

/* ---- baked specular (since the baked-specular change; MCPT_VERSION stays 105: detect the block by symbol) ---- */
/* A REFLECTION VOLUME is a chain of reflection probes on every probe of an mcpt_volume_grid; it is looked up by position with the corners
 * and weights of the irradiance volume, and BAKED SPECULAR adds what it holds along the mirror direction to the surface samples of baked
 * radiance and baked frames: L = kd * E / pi + ks * R(reflect(d, n), Ns).  Three layers, each a test seam of the next: the reflection
 * volume's lookup, the baked radiance with a specular term, the frame.  fp64, no contraction, IEEE division, every expression and sum in
 * the order written; every output is one lane's fixed-order sum: the same bits on the host and on the GPU, whatever the launch shape and
 * the chunking.
 *   reflection volume lookup : mcpt_reflection_volume_lookup*.  grid as mcpt_volume_irradiance takes it (its flags are not read), a chain
 *              description as mcpt_reflection_lookup takes it, chain[nprobes][T][3] with the probes' rows in mcpt_volume_points' order,
 *              valid[nprobes] or NULL, moments (with visibility) or NULL.  Receiver i has q6[i] = (position, normal), a direction d3[i] of
 *              any non-zero finite length and an exponent x[i], finite and >= 0.
 *                P_j, w_j, j = 0 .. 7 = the corners and weights mcpt_volume_irradiance forms at q6[i] -- the snap, the mask and its
 *                renormalisation -- and with moments != NULL those of mcpt_volume_irradiance_visible, normal_bias included;
 *                v_j = mcpt_reflection_lookup's value for the chain of probe P_j, direction d3[i] and exponent x[i];
 *                out_c = sum_j w_j * v_j,c in j order from 0.0, where a corner with w_j == 0.0 contributes nothing and is not read;
 *                corners[i] (may be NULL) = the number of j with w_j > 0; with none out = +0.0.
 *              Hence a receiver on a probe reads that probe's mcpt_reflection_lookup, bit for bit.  (The level or levels of x, the blend
 *              factor a and each level's four wrapped taps and weights depend on d3[i] and x[i] alone: they are formed once per receiver
 *              and serve all eight corners; v_j is mcpt_reflection_lookup's expression tap by tap, with (1.0 - a) formed once.)
 *   specular source : mcpt_baked_specular: flags 0 (pad is not read); grid, chain, chain_data, valid (may be NULL), moments (may be NULL)
 *              and visibility (with moments) as above.  In the host-pointer calls chain_data, valid and moments are host pointers, in the
 *              _device calls device pointers (grid, chain and visibility are always host structs).
 *   baked radiance : mcpt_baked_radiance_specular*.  The rays, the closest hit, kind, face, q6, uv2, kd3, e3 and lit are
 *              mcpt_baked_radiance's under the same source and flags, bit for bit; D = its radiance.  For a SURFACE hit whose material
 *              has a ks component != 0.0, with d the ray's direction and n = q6[3..5] -- the normal that went into the diffuse lookup,
 *              after the fallback to the face's normal and after MCPT_BAKED_FACE_VIEWER:
 *                dn = (dx nx + dy ny) + dz nz;  nn = (nx nx + ny ny) + nz nz;
 *                r_c = d_c * nn - n_c * (2.0 * dn)   -- the mirror direction scaled by |n|^2: no division, the same for n and -n;
 *                l = (|rx| + |ry|) + |rz|; unless l > 0.0 and l is finite there is no specular term;
 *                x = Ns >= 0.0 ? Ns : 0.0;   R, slit = the reflection volume lookup's out and corners at (q6, r, x);
 *                L_c = D_c + ks_c * R_c; under MCPT_BAKED_LIGHTING_ONLY L_c = D_c + R_c.
 *              Everywhere else L = D.  Materials with Ni > 1 (glass) are treated by their ks like any other.
 *              mcpt_baked_specular_outputs (may be NULL, and so may every pointer of it): spec3[n][3] = R, ks3[n][3], r3[n][3], ns[n] =
 *              the material's Ns, slit[n]; +0.0 or 0 for every ray without a specular term.  stats and chunks: mcpt_baked_radiance's.
 *   frame    : mcpt_render_baked_specular*: mcpt_render_baked with every sample shaded as above; img, counts3 and lit as there;
 *              slit[pixel] (may be NULL) = the samples whose specular lookup had slit > 0.
 * mcpt_reflection_volume_lookup_host runs on the CPU and needs no device.  The host-pointer forms are synchronous and copy in and out
 * around the _device forms.  The _device forms take device pointers throughout and enqueue on `stream`.
 * mcpt_baked_radiance_specular_device and mcpt_render_baked_specular_device keep a workspace on the device (the baked calls' own: 116
 * bytes per ray of the largest chunk so far, 120 for a frame that asks for slit), first wait for the event behind the device's previous
 * baked call, and return without waiting when stats == NULL (the first frame of a device also makes the lens's image-plane points and
 * waits for them); they use the counters and queue words of mcpt_trace_closest_device and, like it, must not overlap another closest-hit
 * call of the same device on another stream.  The reflection volume lookup never waits and allocates nothing.
 * Errors (MCPT_ERR_ARG, before MCPT_ERR_NO_DEVICE, in this order).  The lookup: the grid's errors (NULL first); the chain's errors in
 * mcpt_reflection_lookup's order; with moments a NULL visibility and then its errors; m < 0 or m > 2^31 - 1; NULL chain, q6, d3, x or
 * out3 with m > 0; the host-pointer forms: a chain value that is not finite, then per receiver a component of q6 that is not finite, a
 * normal of zero or non-finite length, a direction that is zero, not finite or whose l overflows, an x that is not finite or < 0.
 * The baked calls: the diffuse source's errors as in the plain calls; the specular source: NULL; flags != 0; reserved != 0; the grid's
 * errors (NULL first); the chain's errors; NULL chain_data; with moments a NULL visibility and then its errors; then the call's own
 * errors as in the plain calls (mcpt_baked_radiance*: flags, n, NULL rays6, NULL outputs, outputs' reserved; mcpt_render_baked*: NULL
 * parameters, samples, flags, workspace_rays, reserved, NULL img); last mcpt_baked_specular_outputs' reserved != 0.  A chart component
 * that is not finite: as in the plain calls.  THE DEVICE FORMS DO NOT LOOK AT THEIR ARRAYS and read no texel, bin or probe outside their
 * tables.  n == 0 (the lookup: m == 0): MCPT_OK, nothing is launched.  A workspace or a copy that cannot be allocated: MCPT_ERR_NOMEM,
 * and the device stays usable.
 * Not covered: parallax correction; refraction and glass transport; nearest-probe choice and irregular probe sets; weighting the two
 * lobes by the path tracer's lobe-pick probability; a specular source inside the progressive handles; partitions, the multi-device group
 * and render_scene. */
typedef struct { int32_t flags, pad;
                 const mcpt_volume_grid* grid; const mcpt_reflection_chain* chain; const double* chain_data;
                 const uint8_t* valid; const double* moments; const mcpt_volume_visibility* visibility;
                 int64_t reserved[4]; } mcpt_baked_specular;
typedef struct { double* spec3; double* ks3; double* r3; double* ns; int32_t* slit; int64_t reserved[2]; } mcpt_baked_specular_outputs;
int mcpt_reflection_volume_lookup_host(const mcpt_volume_grid*, const mcpt_reflection_chain*, const double* chain, const uint8_t* valid,
                                       const double* moments, const mcpt_volume_visibility*, const double* q6, const double* d3,
                                       const double* x, int64_t m, double* out3, int32_t* corners);
int mcpt_reflection_volume_lookup(mcpt_device*, const mcpt_volume_grid*, const mcpt_reflection_chain*, const double* chain,
                                  const uint8_t* valid, const double* moments, const mcpt_volume_visibility*, const double* q6,
                                  const double* d3, const double* x, int64_t m, double* out3, int32_t* corners);
int mcpt_reflection_volume_lookup_device(mcpt_device*, const mcpt_volume_grid*, const mcpt_reflection_chain*, const double* d_chain,
                                         const uint8_t* d_valid, const double* d_moments, const mcpt_volume_visibility*,
                                         const double* d_q6, const double* d_d3, const double* d_x, int64_t m, double* d_out3,
                                         int32_t* d_corners, void* stream);
int mcpt_baked_radiance_specular(mcpt_device*, const mcpt_baked_source*, const mcpt_baked_specular*, const double* rays6, int64_t n,
                                 int32_t flags, const mcpt_baked_outputs*, const mcpt_baked_specular_outputs*, mcpt_stats*);
int mcpt_baked_radiance_specular_device(mcpt_device*, const mcpt_baked_source*, const mcpt_baked_specular*, const double* d_rays6,
                                        int64_t n, int32_t flags, const mcpt_baked_outputs*, const mcpt_baked_specular_outputs*,
                                        mcpt_stats*, void* stream);
int mcpt_render_baked_specular(mcpt_device*, const mcpt_baked_source*, const mcpt_baked_specular*, const mcpt_baked_frame_params*,
                               double* img, int32_t* counts3, int32_t* lit, int32_t* slit, mcpt_stats*);
int mcpt_render_baked_specular_device(mcpt_device*, const mcpt_baked_source*, const mcpt_baked_specular*,
                                      const mcpt_baked_frame_params*, double* d_img, int32_t* d_counts3, int32_t* d_lit,
                                      int32_t* d_slit, mcpt_stats*, void* stream);

/* ---- ambient occlusion (since the occlusion change; MCPT_VERSION stays 105: detect the block by symbol) ---- */
/* AMBIENT OCCLUSION is the share of a surface point's cosine-weighted hemisphere that nothing nearby closes, and the BENT NORMAL the mean
 * open direction.  A query takes a list of surface points, traces the irradiance query's own rays for their closest hit and folds
 * distances instead of radiance: no shading at all.  A map is that query over a lightmap's texel list.  The bent normal and ao repair
 * a coarse irradiance volume at contacts (E_volume(bent) * ao); the back-face count tells the texels whose point lies inside other
 * geometry.  fp64, no contraction, IEEE division, every expression and sum in the order written.
 *   list     : n entries, q6 = (position a, normal b of any non-zero finite length), ids[i] or i: MCPT_QUERY_HEMISPHERE's list and keys.
 *   rays     : sample j of entry i is the ray mcpt_query_radiance's hemisphere kind gives it: the draw of (seed, id, sample_base + j), from
 *              0.01 off the point.  AN ENTRY'S OCCLUSION RAYS ARE ITS IRRADIANCE RAYS, BIT FOR BIT, for the same seed, id and sample range;
 *              mcpt_query_rays with MCPT_QUERY_HEMISPHERE is the test seam.
 *   trace    : the closest hit mcpt_trace_closest_device answers (the device's trace mode and engine, key 0 of a motion, a geometry that
 *              stands), through the same walks; the rays are drawn on the GPU into the workspace the visibility bakes keep.
 *   fold     : per entry, in j order, with d the ray's direction, t the hit's distance (measured from the ray's origin, 0.01 off the
 *              point) and n the hit triangle's stored face normal (mcpt_scene_get_faces: geom27[24..26]):
 *                hit = the ray hit anything; near = hit && t < max_distance; x = t / max_distance;
 *                v = 1.0 when not near, otherwise 0.0 (MCPT_OCCLUSION_HARD), x (_LINEAR) or x * x (_SQUARE);
 *                s1 += v; s2 += v * v; bx += d.x * v, by += d.y * v, bz += d.z * v;
 *                hits += near; back += near && ((d.x n.x + d.y n.y) + d.z n.z) > 0.0.
 *              The stored normal is normalize(cross(v1 - v2, v3 - v1)) of the face's vertices, the library's rule everywhere: `back`
 *              means what it says in a scene whose faces wind so that this normal points into free space.  A scene wound the other way
 *              (cornell-box is) reports every near hit as a back-face hit: its caller reads hits - back instead.
 *   outputs  : ao[i] = s1 / spp; stderr1[i] = 0 when spp < 2, else sqrt(max((s2 - s1 * s1 / spp) / (spp - 1), 0) / spp), the radiance
 *              query's expression; bent3[i] = (bx, by, bz) / l with l = sqrt((bx bx + by by) + bz bz) when l is finite and > 0, otherwise
 *              the hemisphere rule's n^ = b / sqrt((bx bx + by by) + bz bz) of the entry's own normal b; hits[i], back[i].  ao [n] is
 *              required; stderr1 [n], bent3 [n][3], hits [n] and back [n] may be NULL.
 *              stats->rays_primary = samples = n * spp, launches = the number of chunks; the other fields are 0.
 *   chunks   : the call works in chunks of whole entries: at most workspace_rays rays and at least one entry each; 0 selects 4 194 304
 *              rays.  The workspace is the visibility bakes' own, 84 bytes per ray of the largest chunk so far.  THE RESULT DOES NOT
 *              DEPEND ON THE CHUNKING: every sum belongs to one entry and is added in j order.
 *   host fold: mcpt_occlusion_fold_host is the fold alone, on the CPU and without a device, over rays the caller traced: rays6 [n * spp][6]
 *              (origin, direction; the origin is not read), hit [n * spp] (non-zero: the ray hit), t [n * spp], n3 [n * spp][3] the hit
 *              faces' normals (read for near samples only); sample j of entry i sits at i * spp + j.  It does not look at the values.
 *   map      : mcpt_bake_occlusion_lightmap takes everything but the fold from the lightmap baker: the chart, coverage, texel list and
 *              owner of mcpt_lightmap_texels for a width x height map, unchanged.  AN OCCLUSION MAP IS, BIT FOR BIT, mcpt_query_occlusion
 *              OVER mcpt_lightmap_texels' LIST WITH ids = texels.  scatter: ao[T], stderr1[T], bent3[T], hits[T], back[T] = the answers
 *              of the entry of texel T; every texel that is not covered gets +0.0 and 0.  dilation: `dilate` rounds, 0 .. 64, of the
 *              lightmap's rule on ao alone -- the same neighbour order, s / c from s = 0.0, owner = -1 - r; stderr1, bent3, hits and back
 *              of filled texels stay 0.  ao [W*H] is required; stderr1 [W*H], bent3 [W*H*3], hits, back and owner [W*H] may be NULL.
 *              stats are the query's over the covered texels.  No texel covered: MCPT_OK, no query is launched.
 * The host-pointer forms are synchronous and copy in and out around the device forms.  The _device forms take device pointers throughout
 * and enqueue on `stream`.  The query returns without waiting when stats == NULL, after first waiting for the event behind the device's
 * previous visibility or occlusion call; it uses the counters and queue words of mcpt_trace_closest_device and, like it, must not
 * overlap another closest-hit call of the same device on another stream.  THE MAP'S DEVICE FORM WAITS ONCE FOR THE STREAM, for the number
 * of covered texels, as mcpt_bake_lightmap_device does, and first waits for the device's previous bake; besides the baker's raster and
 * list it keeps 48 bytes per covered texel and, with dilation, 12 per texel.  Calls are allowed while progressive handles of the device
 * live: they touch none of a handle's state.
 * Errors (MCPT_ERR_ARG, before MCPT_ERR_NO_DEVICE, in this order): NULL parameters; spp < 1; sample_base < 0; sample_base + spp > 2^31 - 1;
 * an unknown falloff; flags != 0; max_distance not finite or <= 0; workspace_rays < 0; reserved != 0; n < 0 or n > 2^31 - 1; NULL q6 or
 * ao with n > 0; mcpt_query_occlusion: the list checks of the hemisphere kind (a negative id, a component that is not finite, a normal of
 * length zero or not finite); mcpt_occlusion_fold_host: NULL rays6, hit, t or n3 with n > 0.  The map: a NULL mcpt_occlusion_map; a size
 * outside 1 .. 16384; dilate outside 0 .. 64; its reserved != 0; then the parameters' errors as above; NULL ao; in the host-pointer form
 * a chart component that is not finite, after the missing device, as in mcpt_bake_lightmap.  n == 0: MCPT_OK, nothing is launched.  A
 * workspace or a copy that cannot be allocated: MCPT_ERR_NOMEM, and the device stays usable.
 * Not covered: adaptive occlusion queries; denoising occlusion maps; occlusion as an input of mcpt_render_baked; two-sided or
 * per-material occlusion; a ray source inside the trace engines (the rays go through a workspace); detecting a scene's winding; the
 * multi-device group (mcpt_multi_*) and render_scene. */
#define MCPT_OCCLUSION_HARD   0   /* a near hit closes its direction */
#define MCPT_OCCLUSION_LINEAR 1   /* ... leaves t / max_distance of it open */
#define MCPT_OCCLUSION_SQUARE 2   /* ... leaves (t / max_distance)^2 of it open */
typedef struct { int32_t spp, sample_base; uint64_t seed; int32_t falloff, flags; double max_distance;
                 int64_t workspace_rays; int32_t reserved[2]; } mcpt_occlusion_params;          /* 48 bytes */
typedef struct { int32_t width, height, dilate, reserved; } mcpt_occlusion_map;                  /* 16 bytes */
int mcpt_query_occlusion(mcpt_device*, const double* q6, const int32_t* ids, int64_t n, const mcpt_occlusion_params*,
                         double* ao, double* stderr1, double* bent3, int32_t* hits, int32_t* back, mcpt_stats*);
int mcpt_query_occlusion_device(mcpt_device*, const double* d_q6, const int32_t* d_ids, int64_t n, const mcpt_occlusion_params*,
                                double* d_ao, double* d_stderr1, double* d_bent3, int32_t* d_hits, int32_t* d_back, mcpt_stats*,
                                void* stream);
int mcpt_occlusion_fold_host(const double* q6, const double* rays6, const int32_t* hit, const double* t, const double* n3, int64_t n,
                             const mcpt_occlusion_params*, double* ao, double* stderr1, double* bent3, int32_t* hits, int32_t* back);
int mcpt_bake_occlusion_lightmap(mcpt_device*, const double* uv6, const mcpt_occlusion_map*, const mcpt_occlusion_params*,
                                 double* ao, double* stderr1, double* bent3, int32_t* hits, int32_t* back, int32_t* owner, mcpt_stats*);
int mcpt_bake_occlusion_lightmap_device(mcpt_device*, const double* d_uv6, const mcpt_occlusion_map*, const mcpt_occlusion_params*,
                                        double* d_ao, double* d_stderr1, double* d_bent3, int32_t* d_hits, int32_t* d_back,
                                        int32_t* d_owner, mcpt_stats*, void* stream);

/* ---- any-hit rays (since the any-hit change; MCPT_VERSION stays 105: detect the block by symbol) ---- */
/* IS ANYTHING IN THE WAY OF A RAY BEFORE DISTANCE tmax?  The third question of a ray interface beside "what is the closest hit" and "what
 * radiance comes along it": line of sight between two points, coverage and form-factor matrices, shadow masks for a caller's own lights.
 * A walk of its own answers it: it stops at the first blocker, writes one byte per ray or one bit per point pair, and the rays of a pair
 * matrix are formed in registers and never exist in memory.  The closest-hit engines and the integrator are untouched.
 *   THE RULE : RAY i WITH LIMIT tmax[i] IS OCCLUDED IFF mcpt_trace_closest OF THE SAME RAY, ON THE SAME DEVICE STATE, ANSWERS face >= 0 AND
 *              t < tmax[i].  The comparison is the IEEE one: a NaN limit is never occluded; tmax <= 0 is never occluded; tmax = +inf asks
 *              "does the ray hit anything".  t is in the ray's own parameter: for an un-normalised direction, multiples of d.  Every
 *              answer is held to this rule exactly; nothing has a tolerance.  (The closest hit is the smallest accepted t_k and every
 *              accepted t_k is > 0, so the rule asks whether SOME leaf passes the reference's own box test, its triangle test and
 *              0 < t_k < tmax: no order between candidates is involved, and the first such leaf ends the walk.)
 *   state    : what mcpt_trace_closest_device sees: the device's trace mode (MCPT_TRACE_REFERENCE answers by the closest-hit walk of the
 *              reference shape and the comparison), key 0 of a motion, a geometry that stands after updates.
 *   rays     : mcpt_trace_any: rays6 [n][6] = origin, direction as mcpt_trace_closest takes them; tmax [n], or NULL for +inf throughout;
 *              occluded [n] receives 0 or 1.
 *   pairs    : for points a_i (a3 [na][3]) and b_j (b3 [nb][3]) and 0 <= t0 < t1, the ray of the pair (i, j) is, per component,
 *                d = b - a;  o = a + t0 * d (a product, then a sum: two roundings);  tmax = t1 - t0 (one value for all pairs),
 *              and THE PAIR IS OCCLUDED IFF THAT RAY WITH THAT LIMIT IS, for every pair, a == b included (a zero direction gets whatever
 *              the closest hit says for it).  In the ray's parameter b lies at 1 - t0: (t0, t1) = (0, 1) asks for the open segment; a caller
 *              whose points lie on surfaces passes, for example, t0 = 1e-4, t1 = 1 - 1e-4, so that neither point's own surface blocks.
 *              mcpt_pair_rays writes these rays on the host, without a device -- rays6 [na*nb][6], pair (i, j) at i * nb + j, and the one
 *              limit to *tmax --: A MATRIX IS, BIT FOR BIT, mcpt_trace_any OVER mcpt_pair_rays' RAYS WITH THAT LIMIT.
 *   matrix   : W = (nb + 63) / 64 words of 64 bits a row: pair (i, j) is bit j & 63 of bits[i * W + (j >> 6)], set means occluded.  The
 *              padding bits of a row's last word are 0.  Every one of the na * W words is written.
 *   stats    : the host-pointer forms fill rays_primary = the rays or pairs answered, node_visits, tri_tests, launches = 1 and ms_trace
 *              (= ms_total) from events around the launch; the other fields are 0.
 * The host-pointer forms are synchronous and copy in and out around the device forms.  The _device forms take device pointers throughout,
 * enqueue on `stream` and return without waiting; they keep no workspace.  They add to the counters of mcpt_trace_closest_device and, like
 * it, MUST NOT OVERLAP ANOTHER CLOSEST-HIT OR ANY-HIT CALL OF THE SAME DEVICE ON ANOTHER STREAM.  Calls are allowed while progressive
 * handles of the device live: they touch none of a handle's state.  (Their pointer parameters are spelled dev_*, not d_*: the extents of
 * these two calls are held by tests/test_gpu_any_hit.py, not by the table of tests/test_gpu_extents.py, which lists the d_* entry points.)
 * Errors (MCPT_ERR_ARG, before MCPT_ERR_NO_DEVICE, in this order).  The ray calls: n < 0 or n > 2^31 - 1; NULL rays6 or occluded with n > 0.
 * The pair calls: NULL parameters; flags != 0; reserved != 0; t0 or t1 not finite, or not 0 <= t0 < t1; na or nb < 0 or > 2^31 - 1;
 * na * W > 2^31 - 1; a NULL point list with a non-zero count; a NULL output (bits; rays6 or tmax) when na and nb are both non-zero.
 * n == 0 (na == 0 or nb == 0): MCPT_OK, nothing is launched and nothing is written.  A copy that cannot be allocated: MCPT_ERR_NOMEM,
 * and the device stays usable.
 * Not covered: the integrator's shadow rays, the occlusion query and the visibility bakes stay on their closest-hit walks; a tmin other
 * than through t0 (an interval (tmin, tmax) does not follow from one closest hit); any-hit in the pool or voting engines and refilling
 * lanes that finish early; which triangle blocked, or how many; alpha-tested or per-material blockers; matrices of more than 2^31 - 1
 * words (the caller cuts them); the multi-device group (mcpt_multi_*) and render_scene. */
typedef struct { double t0, t1; int32_t flags, reserved; } mcpt_pair_params;                     /* 24 bytes; flags == 0 */
int mcpt_trace_any(mcpt_device*, const double* rays6, const double* tmax, int64_t n, uint8_t* occluded, mcpt_stats*);
int mcpt_trace_any_device(mcpt_device*, const double* dev_rays6, const double* dev_tmax, int64_t n, uint8_t* dev_occluded, void* stream);
int mcpt_pair_rays(const double* a3, int64_t na, const double* b3, int64_t nb, const mcpt_pair_params*, double* rays6, double* tmax);
int mcpt_trace_any_pairs(mcpt_device*, const double* a3, int64_t na, const double* b3, int64_t nb, const mcpt_pair_params*,
                         uint64_t* bits, mcpt_stats*);
int mcpt_trace_any_pairs_device(mcpt_device*, const double* dev_a3, int64_t na, const double* dev_b3, int64_t nb,
                                const mcpt_pair_params*, uint64_t* dev_bits, void* stream);

/* ---- direct light (since the direct-light change; MCPT_VERSION stays 105: detect the block by symbol) ---- */
/* THE IRRADIANCE THAT A CALLER'S OWN LIGHTS SEND TO A LIST OF SURFACE POINTS, past the scene's geometry: point, spot, directional (sun)
 * and rectangle lights that are not modelled as emitting triangles.  One fused kernel forms every shadow ray in registers, walks it with
 * the any-hit walk and folds irradiance, its standard error, irradiance by light and a shadow mask by light per receiver; no ray exists in
 * memory.  A map is that query over a lightmap's texel list.  The closest-hit engines, the integrator and the any-hit kernels are
 * untouched.  fp64, no contraction, IEEE division and sqrt, every expression and sum in the order written; only + - * / and sqrt enter.
 *   THE RULE : A DIRECT-LIGHT ANSWER IS, BIT FOR BIT, mcpt_direct_fold_host OVER mcpt_trace_any'S ANSWERS TO THE RAYS AND LIMITS THAT
 *              mcpt_direct_rays (the test seam) WRITES FOR THE SAME LIST, LIGHTS AND PARAMETERS, on the same device state.
 *   receiver : entry i of q6 = (position a, normal b of any non-zero finite length), ids[i] or i: MCPT_QUERY_HEMISPHERE's list, ids and
 *              refusals; n^ = b / sqrt((bx bx + by by) + bz bz), that kind's n^.
 *   toward y : for a point y (a light's position, or a sample on a rectangle): L = y - a; r2 = (Lx Lx + Ly Ly) + Lz Lz; the slot is
 *              SKIPPED unless r2 is finite and > 0; r = sqrt(r2); w = L / r per component; cr = (n^x wx + n^y wy) + n^z wz; SKIPPED unless
 *              cr > 0.
 *   ray      : o = a + w * bias per component (a product, then a sum), d = w, tmax = r - bias.  THE SLOT IS OCCLUDED EXACTLY WHEN
 *              mcpt_trace_any'S RULE SAYS SO FOR THAT RAY AND LIMIT: tmax <= 0, a light within bias of the receiver, is never occluded.
 *   POINT    : SKIPPED when range > 0 && r > range; g = cr / r2.  color is the intensity (irradiance at distance 1, facing the light).
 *   SPOT     : POINT's rule, then s^ = direction / sqrt((dx dx + dy dy) + dz dz); cs = -((s^x wx + s^y wy) + s^z wz);
 *              x = (cs - cos_outer) / (cos_inner - cos_outer); SKIPPED unless x > 0; x = min(x, 1.0); f = (x * x) * (3.0 - 2.0 * x);
 *              g = (cr / r2) * f.
 *   DIRECTIONAL: direction is the way the light travels: w = -s^; cr as above, SKIPPED unless cr > 0; o = a + w * bias, d = w,
 *              tmax = +inf; g = cr.  color is the irradiance on a surface facing the light.
 *   RECT     : corner position, edges u, v; color is the emitted radiance; the light emits toward N = cross(u, v) =
 *              (uy vz - vy uz, vx uz - ux vz, ux vy - vx uy), the library's cross.  A = sqrt((Nx Nx + Ny Ny) + Nz Nz); N^ = N / A.  Sample j
 *              has index k = sample_base + j; xi1, xi2 are words 0 and 1 of the Philox block of (seed, pixel = id, sample = k) at depth
 *              0xFFFE, block l for light index l (a depth no path vertex and no camera draw has; a word w is (w + 0.5) * 2^-32);
 *              y = (position + u * xi1) + v * xi2; cl = -((N^x wx + N^y wy) + N^z wz), with MCPT_LIGHT_TWO_SIDED cl = fabs(cl); SKIPPED
 *              unless cl > 0; g = ((cr * cl) / r2) * A.
 *   g        : last, under every type: THE SLOT IS SKIPPED UNLESS g > 0 (a quotient that underflowed to zero, a NaN out of an overflow),
 *              so that a slot is skipped exactly when its g is +0.0 and the fold can tell from g alone.
 *   slots    : lights in order; a delta light (POINT, SPOT, DIRECTIONAL) has 1 slot, evaluated once whatever spp is, a RECT spp slots in
 *              j order; R = mcpt_direct_slots is their sum; slot s of entry i sits at i * R + s.  mcpt_direct_rays writes, per slot, the
 *              ray (rays6 [n*R][6]: o, d), tmax [n*R] and g [n*R]; for a skipped slot o = a, d = 0, tmax = 0, g = +0.0.  It runs on the
 *              device, through the same functions as the query (csrc/direct.hpp).
 *   fold     : per entry, for l = 0 .. nl - 1 in order: a slot's value is x[c] = color[c] * g when it was not skipped and its ray is not
 *              occluded, else +0.0; traced_l = the slots of light l not skipped (g > 0), lit_l = those of them not occluded.  Delta light:
 *              E_l = x, se2_l = 0.  RECT: s1 += x; s2 += x * x over j from +0.0; E_l = s1 / spp; se2_l = 0 when spp < 2, else
 *              max((s2 - s1 * s1 / spp) / (spp - 1), 0) / spp, the radiance query's expression.  E += E_l; V += se2_l per channel, both
 *              from +0.0.  irradiance3[i] = E; stderr3[i] = sqrt(V); per_light3[i][l] = E_l; visibility[i][l] = traced_l ?
 *              (double)lit_l / (double)traced_l : +0.0.  irradiance3 [n][3] is required; stderr3 [n][3], per_light3 [n][nl][3] and
 *              visibility [n][nl] may be NULL.  nl == 0: every output that is asked for is written with +0.0.
 *              mcpt_direct_fold_host is this fold alone, on the CPU and without a device, over g [n*R] and occluded [n*R] (non-zero:
 *              occluded); it reads `traced` from g > 0 and does not otherwise look at the values.
 *   lights   : a HOST array in every form, like the parameter structs.  The device turns it into a table of its own (a pinned copy and a
 *              device copy it keeps between calls, 160 bytes a light) before the call returns: THE CALLER MAY FREE OR OVERWRITE lights AS
 *              SOON AS A _device CALL HAS RETURNED.  A call first waits for the event behind the device's previous direct-light call.
 *   map      : mcpt_bake_direct_lightmap takes everything but the fold from the lightmap baker: the chart, coverage, texel list and owner of
 *              mcpt_lightmap_texels for a width x height map, unchanged.  A DIRECT LIGHTMAP IS, BIT FOR BIT, mcpt_query_direct OVER
 *              mcpt_lightmap_texels' LIST WITH ids = texels.  scatter: the four answers of the entry of texel T go to irradiance3[T],
 *              stderr3[T], per_light3[T], visibility[T] as they are (irradiance needs no factor pi here); every texel that is not covered
 *              gets +0.0.  dilation: `dilate` rounds, 0 .. 64, of the lightmap's rule on irradiance3 alone; stderr3, per_light3 and
 *              visibility of filled texels stay 0.  irradiance3 [W*H*3] is required; stderr3 [W*H*3], per_light3 [W*H*nl*3], visibility
 *              [W*H*nl] and owner [W*H] may be NULL.  stats are the query's over the covered texels.  No texel covered: MCPT_OK, no query
 *              is launched.
 *   state    : what mcpt_trace_any_device sees: the device's trace mode (MCPT_TRACE_REFERENCE answers every ray by the definition), key 0
 *              of a motion, a geometry that stands after updates.
 *   stats    : rays_primary = the shadow rays walked, that is, the slots not skipped; node_visits, tri_tests, launches = 1 and ms_trace
 *              (= ms_total) from events around the launch; the other fields are 0.
 * The host-pointer forms are synchronous and copy in and out around the device forms.  The _device forms take device pointers throughout
 * but for the lights and the structs, and enqueue on `stream`; the query returns without waiting, THE MAP'S DEVICE FORM WAITS ONCE FOR THE
 * STREAM, for the number of covered texels, as mcpt_bake_lightmap_device does (and again when stats are asked for), and first waits for
 * the device's previous bake; besides the baker's raster and list it keeps 48 + 32 nl bytes per covered texel and, with dilation, 28 per
 * texel.  They add to the counters of mcpt_trace_closest_device and, like it, MUST NOT OVERLAP ANOTHER CLOSEST-HIT OR ANY-HIT CALL OF THE
 * SAME DEVICE ON ANOTHER STREAM.  Calls are allowed while progressive handles of the device live: they touch none of a handle's state.
 * (The pointer parameters are spelled dev_*, not d_*, as the any-hit block's: tests/test_gpu_direct.py holds these calls' extents.)
 * Errors (MCPT_ERR_ARG, before MCPT_ERR_NO_DEVICE, in this order): NULL parameters; spp < 1; sample_base < 0; sample_base + spp > 2^31 - 1;
 * bias not finite or < 0; flags != 0; reserved != 0; nl < 0 or nl > 4096 (the Philox block field has 16 bits); NULL lights with nl > 0;
 * then per light, in index order, looking only at the fields its type reads (POINT: position, color, range; SPOT: those, direction and
 * the cosines; DIRECTIONAL: direction, color; RECT: position, u, v, color; flags and type of every light): an unknown type; a flag other
 * than MCPT_LIGHT_TWO_SIDED, or that flag on a light that is not a RECT; a component that is not finite; a direction of zero or
 * non-finite length; a cross(u, v) of zero or non-finite length; cosines not within -1 <= cos_outer < cos_inner <= 1; range < 0; then
 * n < 0 or n > 2^31 - 1; n * R > 2^31 - 1; NULL q6 or irradiance3 with n > 0 (mcpt_direct_rays: NULL q6, or NULL rays6, tmax or g with
 * n * R > 0; mcpt_direct_fold_host: NULL irradiance3, or NULL g or occluded with n * R > 0); the host-pointer forms: the list checks of
 * the hemisphere kind (a negative id, a component that is not finite, a normal of length zero or not finite).  mcpt_direct_slots: spp < 1,
 * then the lights' errors; it returns R >= 0 or the negative error code.  The map: a NULL mcpt_direct_map; a size outside 1 .. 16384;
 * dilate outside 0 .. 64; its reserved != 0; then the parameters' and lights' errors as above; NULL irradiance3; in the host-pointer form
 * a chart component that is not finite, after the missing device, as in mcpt_bake_lightmap; covered * R > 2^31 - 1, once the raster has
 * counted the covered texels.  n == 0: MCPT_OK, nothing is launched and nothing is written.  A table, a workspace or a copy that cannot
 * be allocated: MCPT_ERR_NOMEM, and the device stays usable.
 * Not covered: light from these lights after its first bounce (nothing here enters the integrator); textured, IES or sphere lights;
 * stratified rectangle samples; adaptive sampling, and denoising the map; these lights in mcpt_render_baked (the caller adds the map to
 * an indirect bake: irradiance is linear); any-hit in the engines and refill of lanes that finish early; the multi-device group
 * (mcpt_multi_*) and render_scene. */
#define MCPT_LIGHT_POINT       0
#define MCPT_LIGHT_SPOT        1
#define MCPT_LIGHT_DIRECTIONAL 2
#define MCPT_LIGHT_RECT        3
#define MCPT_LIGHT_TWO_SIDED   1   /* flags; RECT only */
typedef struct { int32_t type, flags; double position[3], direction[3], u[3], v[3], color[3];
                 double cos_inner, cos_outer, range; } mcpt_direct_light;                         /* 152 bytes */
typedef struct { int32_t spp, sample_base; uint64_t seed; double bias; int32_t flags, reserved[3]; } mcpt_direct_params;   /* 40 bytes; flags == 0 */
typedef struct { int32_t width, height, dilate, reserved; } mcpt_direct_map;                      /* 16 bytes */
int mcpt_query_direct(mcpt_device*, const double* q6, const int32_t* ids, int64_t n, const mcpt_direct_light* lights, int32_t nl,
                      const mcpt_direct_params*, double* irradiance3, double* stderr3, double* per_light3, double* visibility, mcpt_stats*);
int mcpt_query_direct_device(mcpt_device*, const double* dev_q6, const int32_t* dev_ids, int64_t n, const mcpt_direct_light* lights,
                             int32_t nl, const mcpt_direct_params*, double* dev_irradiance3, double* dev_stderr3, double* dev_per_light3,
                             double* dev_visibility, void* stream);
int64_t mcpt_direct_slots(const mcpt_direct_light* lights, int32_t nl, int32_t spp);             /* R: slots per entry; < 0: MCPT_ERR_* */
int mcpt_direct_rays(mcpt_device*, const double* q6, const int32_t* ids, int64_t n, const mcpt_direct_light* lights, int32_t nl,
                     const mcpt_direct_params*, double* rays6, double* tmax, double* g);          /* test seam: [n*R][6], [n*R], [n*R] */
int mcpt_direct_fold_host(const mcpt_direct_light* lights, int32_t nl, const mcpt_direct_params*, const double* g, const uint8_t* occluded,
                          int64_t n, double* irradiance3, double* stderr3, double* per_light3, double* visibility);   /* no device */
int mcpt_bake_direct_lightmap(mcpt_device*, const double* uv6, const mcpt_direct_map*, const mcpt_direct_light* lights, int32_t nl,
                              const mcpt_direct_params*, double* irradiance3, double* stderr3, double* per_light3, double* visibility,
                              int32_t* owner, mcpt_stats*);
int mcpt_bake_direct_lightmap_device(mcpt_device*, const double* dev_uv6, const mcpt_direct_map*, const mcpt_direct_light* lights, int32_t nl,
                                     const mcpt_direct_params*, double* dev_irradiance3, double* dev_stderr3, double* dev_per_light3,
                                     double* dev_visibility, int32_t* dev_owner, mcpt_stats*, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MCPT_H */
