// Records of a scene as they sit in HBM.  Traversal touches one node or one triangle per lane per step,
// each lane somewhere else in the tree, so the unit of access is a whole record that fills exactly one or two
// 64-byte memory segments (array-of-records per node / per triangle, SoA across kinds of data: boxes, hit-test
// geometry, shading attributes, materials, light tables and textures live in separate arrays so that a step
// only pulls the bytes it needs).
#pragma once
#include <cstddef>
#include <cstdint>

// Per-lane traversal stack entries of the deep-stack trace kernels, in LDS (36 KB per block of 256 lanes).  The one definition: the kernels
// size their stacks by it and the builder (accel_build.hpp: kFastMaxDepth) keeps every hierarchy below it: 35 = 3 x 11 levels of the
// device-built 4-wide tree (16.7 M triangles) + slack.
#ifndef MCPT_FAST_STACK
#define MCPT_FAST_STACK 36
#endif

namespace mcpt {

// One real BVH node, compact level order (index = BVH::findIndex).  48 bytes of box padded to one 64-B segment.
struct alignas(64) DNode {
    double mn[3];
    double mx[3];
    double pad[2];
};

// Hit-test geometry of leaf k (Morton order): 96 bytes used by intersect(Ray,Face) + ids.  128 B = 2 segments.
struct alignas(128) DTri {
    double v1[3], v2[3], v3[3];
    double n[3];               // Face::norm
    int32_t material;
    int32_t face;              // .obj index
    int32_t leaf;              // k, the reference's leaf (Morton-order) index: tie-break key and index into shade[]
    int32_t pad[5];
};

// Shading attributes of leaf k, read once per accepted closest hit.
struct alignas(128) DTriShade {
    double vn1[3], vn2[3], vn3[3];
    double vt1[2], vt2[2], vt3[2];
    double pad;
};

// Fast structure: one inner node = both children's boxes + their references, 128 B = one fetch per step.
// child >= 0: inner node; child < 0: leaf, -1-child = (first << 4) | (count-1) into the permuted triangle array.
struct alignas(128) FastNode {
    double lo[2][3];
    double hi[2][3];
    int32_t child[2];
    int32_t pad[6];
};

// Compressed 4-wide node, 64 B = one memory segment = four 16-B loads per lane per step (the walk is bound by L1 line
// throughput, not by ALU or HBM): child boxes quantised to 8 bits per plane on a per-node grid
//     plane = p[axis] + q * 2^e[axis],   q in 0..255, rounded outward at build time,
// so the decoded box contains the child's fp64 box.  Only used to CULL; candidates are decided by the reference's
// own fp64 tests.  child >= 0: node index; child < 0: leaf, -1-child = (first << 4) | (count-1); MCPT_FAST_EMPTY: none.
struct alignas(64) CwNode {
    float p[3];
    int8_t e[3];
    uint8_t nchild;
    uint32_t qlo[3];           // [axis]: byte c = child c
    uint32_t qhi[3];
    int32_t child[4];
    uint32_t pad[2];
};

// fp32 companion of a fast-leaf triangle slot, 48 B = three 16-B loads: what the conservative pre-test of the triangle phase
// reads (trace_fast.hpp: tri_pre_reject).  v0 = fl32(v1), e1 = fl32(v2 - v1), e2 = fl32(v3 - v1) (differences formed in fp64);
// a1 >= |e1.x| + |e1.y| + |e1.z|, a2 likewise (rounded up).  a1 = +inf switches the pre-test off for this triangle (an edge so
// short against the scene's extent, or a sliver so thin, that the error bounds of the test would not cover the reference's own
// fp64 rounding: build_kernels.hip: k_build_pre).  Only ever used to SKIP the exact test of a triangle that cannot pass it.
struct alignas(16) DTriPre {
    float v0[3], a1;
    float e1[3], a2;
    float e2[3], pad;
};
static_assert(sizeof(DTriPre) == 48, "three 16-byte loads");

struct DFast {
    const CwNode* cw;          // compressed wide hierarchy (root = 0)
    const FastNode* nodes;
    const DTri* tris;          // DTri records permuted into fast-leaf order (leaf field = reference leaf index)
    const DTriPre* pre;        // same order: fp32 records of the pre-test
    double absmax;             // largest |coordinate| in the scene
    int32_t enabled;           // 0: scene has coordinates outside [1e-150,1e150] -> reference-shaped walk only
    int32_t stack_limit;       // per-lane stack entries of the trace engine that walks it: picks the short-stack or the deep-stack kernels
    int32_t stack_cap;         // entries of that stack the engine may use (= stack_limit; tests shrink it to force the overflow hand-over)
};

struct alignas(16) DMaterial {
    double kd[3], ks[3];
    double Ns, Ni;
    int32_t has_map, map_w, map_h, light;
    int64_t tex_offset;        // byte offset into the texel pool (BGR rows)
    int64_t pad;
};

// One triangle of an emitter, in the order of Material::f (the order shade() walks the area CDF in).
struct alignas(16) DLightTri {
    double v1[3], v2[3], v3[3];
    double vn1[3], vn2[3], vn3[3];
};

struct alignas(16) DLight {
    double radiance[3];
    double total_area;
    int32_t material, ntri, first, cdf_sorted;   // first = offset into light_tris / light_cdf
};

struct DCamera {                                   // generateImg's frame, pathTracing.cpp:276-294
    double eye[3], start_point[3], pdx[3], pdy[3];
    int32_t width, height;
};

// What a kernel needs of the lens: the device's camera frame and the lens itself, formed on the host (render.cpp: lens_for); camera.hpp: camera_ray.
struct DLens {
    const double* pos;          // [W*H][3] pos(i,j): the reference's running-sum corner of every pixel (k_primary_pos)
    double eye[3], pdx[3], pdy[3];
    double xhat[3], yhat[3];    // screen_x_dir and the normalised up: the basis of the reference's image plane
    double aperture;            // lens radius; 0 = pinhole
    double focus_scale;         // F / l (F <= 0 given: 1)
    int32_t flags, pad;
};

// A query list on the device and where its fold goes (mcpt_query_radiance; query.hpp: query_ray): entry i of q6 is query i, slot i of the
// call; its id is the call's slot list's, or i.  A probe list (mcpt_query_sh; kind 2, internal) holds positions alone, 3 doubles per entry,
// and its fold writes nine coefficients per channel.
#define MCPT_QUERY_KIND_SPHERE 2
struct DQuery {
    const double* q6;           // [n][6] origin + direction (MCPT_QUERY_RAY), or position + normal (MCPT_QUERY_HEMISPHERE); a probe list: [n][3]
    int kind;
    double* mean3;              // [n][3]; a probe list: [n][9][3]
    double* stderr3;            // [n][3] or null; a probe list: [n][9][3] or null
    int32_t* hits;              // [n] or null
};

// The environment light of a frame (env.hpp; tables built by environment.cpp).  All zero: none -- or an inactive one, Z == 0 -- and the
// kernels are the instantiations without it.
struct DEnv {
    const float* rgb;           // [H][W][3] texels, top row first
    const double* c;            // [H + 1] row borders: c[i] = cos(pi i / H), c[0] = 1, c[H] = -1
    const double* marg;         // [H] marginal CDF over rows: running sums of the rows' weights, marg[H-1] = Z
    const double* cond;         // [H][W] per row: running sums of w_ij = lum_ij * omega_ij
    int32_t W, H;
    double scale, Z;
};

struct DLightNode;

// The light pick of MCPT_LIGHTS_ONE (vertex.hpp: light_pick; the table is built on the host by light_sampling.cpp).  All zero: every light
// at every vertex, and the kernels are the instantiations without it.
struct DLightPick {
    const double* cdf;          // [num_lights] running sums of the lights' weights, left to right
    const double* inv_pdf;      // [num_lights] 1 / p_l as the host formed it (a light of weight 0: 0, never read)
    double Z;                   // cdf[num_lights - 1]
    int32_t last, pad;          // the last light of non-zero weight
    const DLightNode* nodes;      // MCPT_LIGHTS_TREE: the light tree, root = 0 (null: the table alone picks, MCPT_LIGHTS_ONE)
};

// One node of the light tree of MCPT_LIGHTS_TREE, one 64-byte segment (built by light_sampling.cpp, walked by vertex.hpp: light_pick_at).
// A leaf is one light of the scene: its box the exact min / max of its DLightTri vertices, its weight the pick table's w_l.  An inner node:
// the exact union of its children's boxes, w = w_left + w_right.
struct alignas(64) DLightNode {
    double lo[3], hi[3];        // the box
    double w;
    int32_t left, right;        // inner node: its children's indices (> 0); leaf: both ~light (< 0)
};
static_assert(sizeof(DLightNode) == 64 && offsetof(DLightNode, hi) == 24 && offsetof(DLightNode, w) == 48 && offsetof(DLightNode, left) == 56 &&
              offsetof(DLightNode, right) == 60, "six fp64 planes, the weight, two 32-bit references: one 64-byte segment");

struct DScene {
    const DNode* nodes;
    const DTri* tris;
    const DTriShade* shade;
    const DMaterial* materials;
    const DLight* lights;
    const DLightTri* light_tris;
    const double* light_cdf;
    const uint8_t* texels;
    DFast fast;
    int32_t t, Lv, Level, Nr, num_lights, num_materials;
    double area0;                                  // range of the frozen static u1 (Q1)
    DCamera cam;
    DEnv env;                                      // rgb == null: no (active) environment
    DLightPick pick;                               // cdf == null: MCPT_LIGHTS_ALL (or a scene of fewer than two lights); nodes: MCPT_LIGHTS_TREE
};

#if defined(__HIPCC__)
__host__ __device__
#endif
inline bool env_on(const DEnv& e) { return e.rgb != nullptr; }
#if defined(__HIPCC__)
__host__ __device__
#endif
inline bool pick_on(const DLightPick& p) { return p.cdf != nullptr; }
#if defined(__HIPCC__)
__host__ __device__
#endif
inline bool tree_on(const DLightPick& p) { return p.nodes != nullptr; }
// the kernels' compile-time pick mode of a scene: 0 (MCPT_LIGHTS_ALL), 1 (MCPT_LIGHTS_ONE), 2 (MCPT_LIGHTS_TREE)
inline int pick_mode(const DLightPick& p) { return tree_on(p) ? 2 : (pick_on(p) ? 1 : 0); }

// ---- device-side counters and diagnostic words.  The kernels add to them by name; stats.cpp turns them into mcpt_stats and the MCPT_PRINT_DIAG
// text.  The layout is fixed (680 bytes of 64-bit words, asserted below): mcpt_device_collect_stats sums two of them word by word.

// MCPT_TRACE_DIAG builds: what the waves of the persistent trace engine did, word by word (a wave counts in Work::diag, k_wf_trace adds that to
// DCounters::diag).  Phases: 0 inner, 1 pre-test, 2 exact; stages of the wave's time: 0 refill, then the phases.
enum TraceDiagWord {
    TD_ITERS = 0,           // + 2 * phase: iterations of the phase
    TD_LANES = 1,           // + 2 * phase: lanes that waited for it
    TD_IDLE_LANES = 6,
    TD_CYCLES = 8,          // + stage: wave cycles
    TD_WORDS = 12
};
// MCPT_PRE_CHECK builds: what the pre-test saw of the first triangle it should not have rejected (the wave that turns `claimed` from 0 to 1 writes it)
struct PreCheckRecord {
    unsigned long long claimed;
    double seen[8];                                          // tri_pre_reject's margins: beta, gamma, alpha, behind, beyond, clear; t32, |det|
    double t_k, leader, limit_f, margin, eta4, slot, count;
    double o[3], d[3];                                       // the ray
    unsigned long long spare[2];
};
// MCPT_POOL_DEBUG builds: the refill account of the pool engine's trace launches (trace_pool.hpp)
struct PoolDebug {
    unsigned long long used, ok, refills, retired, slots, launches, tickets, started;
    unsigned long long class_steps[4], class_lanes[4], class_want[4];
    unsigned long long sleeps, missed;
    unsigned long long spare[2];
};
// MCPT_POOL_DEBUG builds: the pool scheduler's account per class (node, leaf, exact, result, shade), of the finishing pass and of the trace launches
struct PoolAccount {
    unsigned long long steps[5], lanes[5];                   // steps per class, lanes that claimed
    unsigned long long sleeps, missed;                       // ... steps that claimed nothing
    unsigned long long cycles[5];                            // wave cycles per class
    unsigned long long overhead, life, waves;                // cycles voting / claiming / sleeping, wave lifetimes, waves
    unsigned long long spare[4];
};
// What a trace engine's Work::dbg points to.  The two debug builds share the first 24 words: a library is compiled with at most one of them.
struct DebugWords {
    union { PreCheckRecord pre; PoolDebug pool; };
    PoolAccount account;
};
#if defined(MCPT_PRE_CHECK) && defined(MCPT_POOL_DEBUG)
#error "MCPT_PRE_CHECK and MCPT_POOL_DEBUG share DebugWords: build one or the other (chk is the first alone, diag the second with MCPT_TRACE_DIAG)"
#endif

struct DCounters {
    unsigned long long rays_primary, rays_shadow, rays_bounce, node_visits, tri_tests, shade_calls, samples, max_depth;
    unsigned long long shadow_skipped;   // shadow rays the reference traces although their result is never used (light behind the surface)
    unsigned long long trace_rays, trace_nodes, trace_tris;   // work done inside the dominant kernel (k_wf_trace) only
    unsigned long long trace_exact;                           // ... triangles of those that survived the pre-test (exact fp64 tests)
    DebugWords dbg;
    unsigned long long diag[TD_WORDS];
    unsigned long long deferred_rays;                         // rays k_wf_trace handed to the exact walk
    unsigned long long finish_steps, finish_life, finish_trace;   // finishing kernel: longest wave in steps, in ticks alive, in ticks inside the ray walks (maxima)
    unsigned long long logic_cycles[3], logic_waves;          // logic kernel, later passes: cycles in resolve / compaction / shade, waves
    unsigned long long pre_wrong;                             // pre-test self-check: rejected triangles that are candidates by the exact test (must stay 0)
    unsigned long long kernarg_differ, kernarg_checked;       // MCPT_PRE_CHECK: trace launches whose kernarg WfArgs differ / that were checked
    unsigned long long spare;
};
// The layout, word by word: the debug words at byte 104, the pool account at 296, the diagnostics at 488.  Recorded profiles and both sides of
// the host / kernel boundary rely on it; a member that moves fails here, not on the GPU.
#define MCPT_WORD(member, base, index) static_assert(offsetof(DCounters, member) == (base) + 8 * (index), #member)
static_assert(sizeof(DCounters) == 680 && sizeof(DCounters) % sizeof(unsigned long long) == 0 && alignof(DCounters) == alignof(unsigned long long),
              "85 64-bit words and nothing else: summed word by word");
static_assert(sizeof(PreCheckRecord) == 192 && sizeof(PoolDebug) == 192 && sizeof(PoolAccount) == 192, "24 words each");
MCPT_WORD(dbg, 104, 0); MCPT_WORD(dbg.account, 296, 0); MCPT_WORD(diag, 488, 0);
MCPT_WORD(dbg.pre.claimed, 104, 0); MCPT_WORD(dbg.pre.seen, 104, 1); MCPT_WORD(dbg.pre.t_k, 104, 9); MCPT_WORD(dbg.pre.leader, 104, 10);
MCPT_WORD(dbg.pre.limit_f, 104, 11); MCPT_WORD(dbg.pre.margin, 104, 12); MCPT_WORD(dbg.pre.eta4, 104, 13); MCPT_WORD(dbg.pre.slot, 104, 14);
MCPT_WORD(dbg.pre.count, 104, 15); MCPT_WORD(dbg.pre.o, 104, 16); MCPT_WORD(dbg.pre.d, 104, 19);
MCPT_WORD(dbg.pool.used, 104, 0); MCPT_WORD(dbg.pool.ok, 104, 1); MCPT_WORD(dbg.pool.refills, 104, 2); MCPT_WORD(dbg.pool.retired, 104, 3);
MCPT_WORD(dbg.pool.slots, 104, 4); MCPT_WORD(dbg.pool.launches, 104, 5); MCPT_WORD(dbg.pool.tickets, 104, 6); MCPT_WORD(dbg.pool.started, 104, 7);
MCPT_WORD(dbg.pool.class_steps, 104, 8); MCPT_WORD(dbg.pool.class_lanes, 104, 12); MCPT_WORD(dbg.pool.class_want, 104, 16);
MCPT_WORD(dbg.pool.sleeps, 104, 20); MCPT_WORD(dbg.pool.missed, 104, 21);
MCPT_WORD(dbg.account.steps, 296, 0); MCPT_WORD(dbg.account.lanes, 296, 5); MCPT_WORD(dbg.account.sleeps, 296, 10); MCPT_WORD(dbg.account.missed, 296, 11);
MCPT_WORD(dbg.account.cycles, 296, 12); MCPT_WORD(dbg.account.overhead, 296, 17); MCPT_WORD(dbg.account.life, 296, 18); MCPT_WORD(dbg.account.waves, 296, 19);
MCPT_WORD(deferred_rays, 488, 12); MCPT_WORD(finish_steps, 488, 13); MCPT_WORD(finish_life, 488, 14); MCPT_WORD(finish_trace, 488, 15);
MCPT_WORD(logic_cycles, 488, 16); MCPT_WORD(logic_waves, 488, 19); MCPT_WORD(pre_wrong, 488, 20); MCPT_WORD(kernarg_differ, 488, 21);
MCPT_WORD(kernarg_checked, 488, 22); MCPT_WORD(spare, 488, 23);
#undef MCPT_WORD

}  // namespace mcpt
