/*
 * mcpt_oracle.h -- CPU restatement of Arieys/MonteCarloPathTracing's hot path.
 *
 * THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Only tests/, __graft_entry__.smoke()
 * and bench.py's cpu_baseline leg may load it.  The product path (libmcpt.so) never
 * links, loads or calls anything in oracle/.
 *
 * Every function cites the reference file:line it follows (paths relative to the
 * reference checkout, e.g. MTPC/pathTracing.cpp:137).  All arithmetic is IEEE fp64
 * in the reference's own operation order, compiled with -ffp-contract=off.
 *
 * Pinning status (see DESIGN.md "Oracle"; tests/test_oracle_pins.py, tests/pins_common.py):
 *   - Morton keys      : pinned bit-exactly against the reference's own "morton code.cpp"
 *                        compiled from where it lies (oracle/_ref/libref_morton.so).
 *   - PNG bytes        : pinned byte-exactly against the reference's svpng.inc (oracle/_ref).
 *   - camera model, loader, Morton order/BVH, primary closest hit: pinned PIXEL-EXACTLY by the
 *     RNG-independent pixels of the reference's published renders (a primary hit on an emitter is
 *     (255,255,255) whatever the RNG did): 4 922 / 4 922 pixels of cornell-box in six renders, with
 *     only 4 other saturated pixels in cornell-box-SPP25.png; 45 266 / 45 266 of veach-mis.
 *   - traversal + shading as a whole: (a) the work they do equals, figure for figure, what SURVEY.md
 *     3.5 measured on an instrumented build of the reference itself (rays per sample by kind, shade
 *     calls, box tests per ray to 4 digits: 264.26 vs 264.2 on veach-mis, triangle tests per ray),
 *     once the walk aliases virtual children like the reference (Q7) and the leaves are ordered as
 *     libstdc++'s unstable std::sort leaves them (std_sort_order.cpp); (b) the pictures agree with
 *     the published renders of the matching revision at MONTE-CARLO PRECISION: per-16x16-block
 *     z-scores at native resolution and the published SPP are standard normal (cornell-box SPP 25:
 *     mean -0.02, rms 0.99; whole-picture brightness within 0.05 %; veach-mis SPP 10 and 100).
 *   - bitwise values of traversal / shading: the reference TUs need glm, OpenCV and Eigen headers
 *     that this image lacks (no stand-ins are written) and the reference ships no tests or golden
 *     vectors, so beyond the above: PARITY UNPINNED.
 *
 * Documented deviations from the reference (all needed for reproducibility / to avoid UB):
 *   D1  RNG seam: the four time(NULL)-seeded static engines (pathTracing.cpp:5,32,68,169)
 *       are replaced by a counter-based Philox4x32-10 keyed (seed; pixel, sample, depth, slot).
 *   D2  stable sort of faces by Morton key (MTPC.cpp:44 uses unstable std::sort).
 *   D3  samples of a pixel are accumulated serially in k order (pathTracing.cpp:303-319 is
 *       an unordered OpenMP/mutex accumulation).
 *   D4  '\r' is stripped from every input line (the shipped scenes are CRLF).
 *   D5  virtual right children are skipped instead of aliased (pathTracing.cpp:368-371 /
 *       BVH.cpp:99-104); ORC_TRACE_ALIAS reproduces the aliasing for even t.
 *   D6  recursion depth of shade() is capped at ORC_MAX_DEPTH (reference: unbounded).
 *   D7  texture row/col are clamped to the raster (reference: possible 1-past read).
 *   D8  Ns/Ni default to 1 when absent from the .mtl (reference: uninitialised).
 *
 * Extension (not in the reference): the environment light of include/mcpt.h, restated from that header's text (orc_scene_set_environment
 * below); pinned by tests/test_env_cpu.py (tables and draws against tests/env_ref.py, closed forms) and held against the GPU by
 * tests/test_gpu_env_oracle.py.  Without an environment every answer and every count is what it was before.
 * Extension (not in the reference): the light pick of include/mcpt.h (MCPT_LIGHTS_ONE, MCPT_LIGHTS_TREE), restated from that header's
 * text and tests/light_pick_ref.py / tests/light_tree_ref.py (orc_scene_set_light_pick below); pinned by
 * tests/test_light_pick_oracle_cpu.py and held against the GPU by tests/test_gpu_light_pick_oracle.py.  Without a pick (the default)
 * every answer and every count is what it was before.
 * Extension (not in the reference): the camera lens of include/mcpt.h (MCPT_LENS_JITTER, MCPT_LENS_PER_SAMPLE, the thin lens), restated from
 * that header's "camera lens" paragraph (orc_scene_set_lens below); pinned by tests/test_lens_oracle_cpu.py (the rays against
 * tests/lens_ref.py, the per-sample route against the pinhole's, the frame against the fold of its samples) and held against the GPU by
 * tests/test_gpu_lens_oracle.py.  Without a lens (the default) every answer and every count is what it was before.
 * Extension (not in the reference): a ray-keyed entry to the integrator (orc_ray_radiance below), for the radiance queries of include/mcpt.h,
 * whose rays no camera sends: the caller's ray as given, shaded at depth 0 under the key (seed, id, k).  It adds no arithmetic -- it calls what
 * orc_sample_radiance calls -- and is pinned by tests/test_query_oracle_cpu.py (the camera's rays keyed by pixel give orc_sample_radiance bit
 * for bit, under every lens, sky and pick) and held against the GPU by tests/test_gpu_query_oracle.py.  No other function changed with it.
 */
#ifndef MCPT_ORACLE_H
#define MCPT_ORACLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORC_MAX_DEPTH 64
#define ORC_PI 3.1415926          /* MTPC/pathTracing.h:11 */
#define ORC_P_RR 0.6              /* MTPC/pathTracing.cpp:237 */

typedef struct orc_scene orc_scene;

typedef struct {
    int t, Lc, Lv, Nc, Nv, Nr, Level;    /* MTPC/BVH.cpp:46-52 */
} orc_bvh_info;

typedef struct {
    uint64_t rays_primary, rays_shadow, rays_bounce;
    uint64_t box_tests, tri_tests, shade_calls, samples;
    int max_depth;
    uint64_t rays_on_surface;   /* bounce rays that start on the surface itself: refraction / total reflection (pathTracing.cpp:102,109) */
    /* the environment (extension; all 0 without one).  env_shadow is also counted in rays_shadow. */
    uint64_t env_shadow, env_shadow_clear;                  /* environment shadow rays traced; those that hit nothing */
    uint64_t env_escape_specular, env_escape_transmission;  /* SPECULAR / TRANSMISSION bounce rays that left the scene */
    uint64_t camera_miss;                                   /* camera samples whose primary ray left the scene */
} orc_stats;

/* ---- RNG seam (D1) ---- */
void     orc_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
double   orc_uniform(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t depth, uint32_t slot);

/* ---- Morton key: MTPC/morton code.cpp:3-32 ---- */
uint32_t orc_morton_code(float x, float y, float z);

/* ---- scene: MTPC/sceneManagement.cpp:17-274, MTPC/MTPC.cpp:44, MTPC/BVH.cpp:37-132 ---- */
/* prefix = path+filename without extension; texture_dir = where map_Kd rasters are looked up
 * ("<texture_dir>/<map_Kd>.ppm", binary P6 holding the decoded RGB raster). */
orc_scene* orc_scene_load(const char* prefix, const char* texture_dir, char* err, int errlen);
void       orc_scene_free(orc_scene*);
void       orc_scene_set_resolution(orc_scene*, int width, int height);
/* which walk (ORC_TRACE_*, below) orc_render / orc_sample_radiance use for their rays; default ORC_TRACE_REAL_ONLY.
 * ORC_TRACE_ALIAS gives the same picture with the reference's own node-visit counts (Q7). */
void       orc_scene_set_walk_mode(orc_scene*, int mode);
/* D2: rebuild the BVH with another order of the faces that share a Morton key.  0 on success. */
#define ORC_ORDER_STABLE    0   /* .obj order among equal keys (default) */
#define ORC_ORDER_LIBSTDCXX 1   /* the order std::sort (MTPC/MTPC.cpp:44) leaves in a g++/libstdc++ build (std_sort_order.cpp) */
int        orc_scene_set_leaf_order(orc_scene*, int which);

int  orc_num_faces(const orc_scene*);
int  orc_num_materials(const orc_scene*);
int  orc_num_lights(const orc_scene*);
void orc_get_camera(const orc_scene*, double cam[10], int wh[2]); /* eye,lookat,up,fovy */
/* faces in .obj order: 9 v, 9 vn, 6 vt, 3 norm = 27 doubles per face */
void orc_get_faces(const orc_scene*, double* geom27, int32_t* material, uint32_t* morton);
/* sorted (leaf) order -> original .obj face index */
void orc_get_leaf_order(const orc_scene*, int32_t* leaf_to_face);
void orc_get_bvh_info(const orc_scene*, orc_bvh_info*);
/* Nr nodes, compact level order; box layout = max_x,max_y,max_z,min_x,min_y,min_z (sceneManagement.h:165-171) */
void orc_get_bvh_nodes(const orc_scene*, double* box6, int32_t* level, int32_t* leaf_face);
int  orc_find_index(const orc_scene*, int i, int l);              /* MTPC/BVH.cpp:99-104 */
/* material record: kd3 ks3 Ns Ni (8 doubles), flags: has_map, map_w, map_h, light_index(-1 if none) */
void orc_get_material(const orc_scene*, int m, char name[64], double rec8[8], int32_t flags4[4]);
void orc_get_light(const orc_scene*, int i, char name[64], double radiance[3], int32_t* material, double* total_area);

/* ---- closest hit: MTPC/pathTracing.cpp:334-390 ---- */
#define ORC_TRACE_REAL_ONLY 0
#define ORC_TRACE_ALIAS     1   /* reproduce the virtual-child aliasing (even t only) */
#define ORC_TRACE_FLAT      2   /* brute force over all leaves: own box + triangle test, no tree */
/* rays: n x 6 (origin, direction).  face = original .obj index or -1; p,pn = n x 3 */
void orc_trace_closest(const orc_scene*, const double* rays, int64_t n, int mode,
                       int32_t* face, double* t, double* p, double* pn, orc_stats* st);

/* ---- integrator: MTPC/pathTracing.cpp:137-331 ---- */
/* radiance of one camera sample (pixel index = row*W+col, sample k) */
void orc_sample_radiance(const orc_scene*, uint64_t seed, int row, int col, int k, double rgb[3], orc_stats* st);
/* primary ray for a pixel, exactly as generateImg builds it (incl. the running-sum position) */
void orc_primary_ray(const orc_scene*, int row, int col, double ray6[6]);
/* rows [row0,row1) x all columns, (row1-row0)*W x 6 doubles */
void orc_primary_rays(const orc_scene*, int row0, int row1, double* rays6);
/* render rows [row0,row1) x cols [col0,col1) into img (full H*W*3 layout, doubles; other pixels untouched).
 * faithful_cost!=0 re-traces the primary ray and rebuilds light CDFs per call like the reference
 * (same result, reference-like cost; used for the CPU baseline).  nthreads<=0 -> OpenMP default. */
void orc_render(const orc_scene*, int spp, uint64_t seed, int row0, int row1, int col0, int col1,
                int faithful_cost, int nthreads, double* img, orc_stats* st);

/* rows 0, stride, 2*stride, ... only (bounded CPU-baseline sample); OpenMP over the sampled rows */
void orc_render_strided(const orc_scene*, int spp, uint64_t seed, int row_stride, int faithful_cost, int nthreads,
                        int unused, double* img, orc_stats* st);
/* the reference's own parallel structure (one pixel at a time, min(spp, 8) threads over its samples, fork/join per pixel:
 * MTPC/pathTracing.cpp:300-320), faithful cost, on the pixels (k * row_stride, m * col_stride): the reference-style timing */
void orc_render_reference_style(const orc_scene*, int spp, uint64_t seed, int row_stride, int col_stride, double* img, orc_stats* st);

/* ---- environment light (extension, not in the reference): include/mcpt.h "environment light", restated from its text ----
 * rgb = W x H x 3 floats, top row first; the fp64 tables are built in the header's operation order (row borders through the C library's
 * cos; pi = 3.141592653589793 there, in phi and in the light sample's "/ pi" -- not ORC_PI).  Returns Z.  Z == 0 (an all-black map, or
 * rgb NULL) leaves the scene WITHOUT an environment, as the header's "inactive"; -1: bad arguments (the previous environment is kept).
 * With one, orc_sample_radiance and orc_render (either cost) follow the header: a light sample from slots 4(nl+2)..4(nl+2)+3 after the
 * lights' loop, escapes of SPECULAR and TRANSMISSION bounce rays, camera misses (a missed pixel folds Le / spp for every sample).
 * orc_render_strided and orc_render_reference_style IGNORE the environment: they render as without one (the CPU baseline). */
double orc_scene_set_environment(orc_scene*, const float* rgb, int W, int H, double scale);
/* Le(dirs[i]) -> rgb[n*3]; the draw of vertex `depth` of camera samples (pix[i] = row*W+col, k[i]) -> dirs[n*3], pdf[n], rgb[n*3] (the drawn
 * texel's radiance): the functions the paths use.  0, or -1 without an active environment. */
int orc_env_eval(const orc_scene*, const double* dirs, int64_t n, double* rgb);
int orc_env_sample(const orc_scene*, uint64_t seed, const int32_t* pix, const int32_t* k, int depth, int64_t n, double* dirs, double* pdf,
                   double* rgb);

/* ---- light pick (extension, not in the reference): include/mcpt.h "light sampling" ----
 * mode 0 (the default): every light at every vertex, the reference's loop.  mode 1 (MCPT_LIGHTS_ONE): one light per vertex from the
 * table cdf[n], inv_pdf[n] (1.0 / pdf, 0 for a light of weight 0), last (the last light of non-zero weight), Z (the weights' sum) --
 * tests/light_pick_ref.PickRef.  mode 2 (MCPT_LIGHTS_TREE): one light per vertex by the descent of the n_nodes = 2 nl - 1 64-byte nodes of
 * tests/light_tree_ref.TreeRef (lo[3], hi[3], w as doubles, left, right as int32; a leaf holds ~light in both).  The arrays are copied; the
 * oracle builds neither (tests hold both to the library's own, bit for bit).  Arguments a mode does not use may be NULL / 0.  In modes 1
 * and 2 orc_sample_radiance and orc_render shade a vertex with ONE light l in place of the loop: u = slot 0 of Philox block nl + 3 at the
 * vertex's depth; mode 1 the smallest l <= last with u * Z < cdf[l]; mode 2 the descent at the vertex's own (p, pn); the loop's body for
 * that light alone -- its draws from block l, no light before it to inherit a material from, one shadow ray -- and its term times 1 / p_l.
 * The environment's sample and the bounce are untouched (the paths are mode 0's).  orc_render_strided / _reference_style are for scenes
 * without a pick.  0, or -1 on bad arguments (the previous setting is kept). */
int orc_scene_set_light_pick(orc_scene*, int mode, const double* cdf, const double* inv_pdf, int n, int last, double Z,
                             const void* nodes, int n_nodes);
/* FOR THE TESTS' POWER CHECKS ONLY: makes the picking modes answer wrongly -- 1: the factor 1 / p is applied at depth 0 only, 2: the picked
 * light's four draws come from block 0.  0 (what every orc_scene_set_light_pick leaves) is right.  0, or -1 without a pick. */
int orc_scene_set_light_pick_wrong(orc_scene*, int wrong);
/* the pick alone, at vertex `depth` of camera samples (pix[i], k[i]): out_l[n] the light, out_inv[n] the factor shade() scales by, out_pdf[n]
 * the probability (mode 2: the descent's own, the factor is 1.0 / it; mode 1: 1.0 / the factor -- the table holds no probabilities).  p, pn (n x 3):
 * the vertices, mode 2 only.  out_pdf / out_inv may be NULL.  0, or -1 without a pick. */
int orc_light_pick(const orc_scene*, uint64_t seed, const int32_t* pix, const int32_t* k, int depth, const double* p, const double* pn,
                   int64_t n, int32_t* out_l, double* out_pdf, double* out_inv);

/* ---- camera lens (extension, not in the reference): include/mcpt.h "camera lens", restated from its text ----
 * flags: MCPT_LENS_JITTER (1) | MCPT_LENS_PER_SAMPLE (2); aperture >= 0; focus_distance (<= 0: |look_at - eye|).  All zero: the pinhole, and
 * every answer and count is the reference's.  A lens is ACTIVE when it has a flag or aperture > 0; then orc_sample_radiance and orc_render
 * (either cost) give every camera sample (pixel, k) a camera ray of its own -- u0..u3 = orc_uniform(seed, pixel, k, depth 0xFFFF, slot 0..3),
 * q = the running-sum corner, jittered as (q + pdx*u0) - pdy*u1, the pinhole's or the thin lens's ray in the header's operation order, phi with
 * pi = 3.141592653589793 (not ORC_PI) -- trace it (rays_primary counts each one), shade from THAT sample's hit with wo = -d of THAT sample; a
 * sample that misses is 0, or Le(its own d) under an environment (camera_miss counts it), and the frame folds every sample, missed ones
 * included, by the same float accumulation in k order.  MCPT_LENS_PER_SAMPLE alone: the pinhole's answers bit for bit, through this route.
 * orc_render_strided and orc_render_reference_style IGNORE the lens, as they ignore the environment: the pixel's pinhole ray (the CPU
 * baseline).  0, or -1 on what the header calls MCPT_ERR_ARG (unknown flag bits, aperture negative or not finite, focus_distance not
 * finite): the previous lens is kept. */
int orc_scene_set_lens(orc_scene*, int flags, double aperture, double focus_distance);
/* the camera rays of samples (pix[i] = row*W+col, k[i]) under the scene's lens, active or not -> rays6[n*6] = origin xyz, direction xyz.
 * 0, or -1 for a pixel outside the frame or a negative k (nothing is written). */
int orc_camera_rays(const orc_scene*, uint64_t seed, const int32_t* pix, const int32_t* k, int64_t n, double* rays6);
/* FOR THE TESTS' POWER CHECKS ONLY: makes the lens route answer wrongly -- 1: the first vertex is shaded with wo of the pixel's unjittered
 * pinhole ray, 2: a missed sample under an environment takes Le of the pixel's pinhole direction.  0 (what every orc_scene_set_lens leaves) is
 * right.  0, or -1 without an active lens. */
int orc_scene_set_lens_wrong(orc_scene*, int wrong);

/* ---- ray-keyed entry (extension, not in the reference): include/mcpt.h "radiance queries", its "keys" and "shading" paragraphs ----
 * Sample i traces rays6[i] (origin xyz, unit direction xyz) as given -- from its origin, no offset, under the scene's walk mode -- and shades
 * the hit at depth 0 with wo = -d under the RNG key (seed, pixel = ids[i], or i when ids == NULL, sample = k[i]); a miss is +0.0, or Le(d)
 * under an environment (camera_miss counts it).  The scene's environment and light pick apply; its lens, camera and resolution do not.  It is
 * the integrator orc_sample_radiance runs, entered by ray: on the rays of orc_camera_rays with ids = the pixels it gives that function's
 * answers and counts bit for bit, under any lens.  rgb[n*3]; hit[i] (may be NULL): whether the ray hit anything; on_surface[i] (may be
 * NULL): whether the path traced a bounce ray that starts on the surface it leaves (rays_on_surface); st (may be NULL): summed over the
 * samples (max_depth: the largest).  Samples run on OpenMP threads; every answer is its own.
 * wrong -- FOR THE TESTS' POWER CHECKS ONLY: 0 is right; 1: the ray leaves o + d * 0.01 instead of o; 2: the pixel word of the key is the list
 * position instead of the id.  Nothing of it stays in the scene. */
void orc_ray_radiance(const orc_scene*, uint64_t seed, const int32_t* ids, const int32_t* k, const double* rays6, int64_t n, int wrong,
                      double* rgb, uint8_t* hit, uint8_t* on_surface, orc_stats* st);

/* ---- output: MTPC/MTPC.cpp:10-33, MTPC/svpng.inc:77-107 ---- */
void orc_quantize(const double* img, int64_t n, uint8_t* rgb8);
/* returns number of bytes written into out (capacity cap), or -1 */
int64_t orc_png_encode(const uint8_t* rgb8, int w, int h, uint8_t* out, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif
