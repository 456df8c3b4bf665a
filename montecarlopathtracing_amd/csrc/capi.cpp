// C ABI of libmcpt.so (include/mcpt.h): host scene handles, device residency, and the launch sequences that
// stand in for ray_intersect / generateImg / imshow / render_scene of the reference.
#include <hip/hip_runtime_api.h>
#include <hip/hip_version.h>
#include <dlfcn.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <functional>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "accel_build.hpp"
#include "build_kernels.hpp"
#include "denoise.hpp"
#include "hip_owned.hpp"
#include "jpeg_decoder.hpp"
#include "kernels.hpp"
#include "knobs.hpp"
#include "scene.hpp"
#include "wavefront.hpp"

using namespace mcpt;

namespace {
thread_local std::string g_error;
}  // namespace

// the calling thread's error message, for every translation unit of the library (hip_owned.hpp: fail, HIP_TRY)
namespace mcpt { int set_error(int code, const std::string& msg) { g_error = msg; return code; } }

// a device buffer of at least 8 bytes, unless b holds one already; alloc_zeroed: cleared as well
template <class T>
static hipError_t alloc_once(DevBuf<T>& b, size_t bytes) { return b ? hipSuccess : b.alloc_bytes(std::max<size_t>(bytes, 8)); }
template <class T>
static hipError_t alloc_zeroed(DevBuf<T>& b, size_t bytes)
{
    const hipError_t e = alloc_once(b, bytes);
    return e == hipSuccess ? hipMemset(b.get(), 0, std::max<size_t>(bytes, 8)) : e;
}

struct mcpt_scene {
    Scene s;
    // The fast walk's culling hierarchy depends on the scene and the leaf order only: built once, shared by every device
    // created from this scene (one SAH build for the 8 GPUs of a node, not 8).
    mutable std::atomic<int> devices_created{0};      // mcpt_scene_set_resolution is refused once a device holds the camera
    // Shared ownership: the caller's handle and every device created from the scene hold one reference each; the scene goes with the
    // last of mcpt_scene_free / mcpt_device_free, in whichever order they come (a device keeps using the handle: the shared culling
    // hierarchy, the counter above).
    mutable std::atomic<int> refs{1};
    mutable std::mutex fast_mu;
    mutable std::shared_ptr<const FastBvh> fast_cached;
    mutable std::vector<int32_t> fast_order;
    mutable int fast_leaf = 0;
    mutable double fast_ct = 0;
};

// The hierarchy is always built for the deep stack (the better tree); MCPT_FAST_STACK_LIMIT builds it for a shallower one (A/B runs).
static int stack_limit_for(const Knobs& k) { return k.fast_stack_limit ? k.fast_stack_limit : kFastMaxDepth; }
static FastBuildOpts build_opts_for(const Knobs& k)
{
    FastBuildOpts o;
    if (k.fast_leaf) o.max_leaf = std::max(1, std::min(kFastMaxLeaf, k.fast_leaf));
    if (k.fast_ct > 0) o.cost_tri = k.fast_ct;
    o.serial = k.build_serial != 0; o.talk = k.print_diag != 0;
    return o;
}

// (built with the knobs of the device creation that asks first; a later one with other builder knobs rebuilds)
static std::shared_ptr<const FastBvh> shared_fast_bvh(const mcpt_scene* h, const std::vector<int32_t>& order, const Knobs& k)
{
    std::lock_guard<std::mutex> lock(h->fast_mu);
    const int limit = stack_limit_for(k);
    const FastBuildOpts o = build_opts_for(k);
    if (!h->fast_cached || h->fast_order != order || h->fast_cached->stack_limit != limit || h->fast_leaf != o.max_leaf || h->fast_ct != o.cost_tri) {
        auto fb = std::make_shared<FastBvh>();
        build_fast_bvh(h->s.faces, order.data(), int(h->s.faces.size()), *fb, limit, o);
        h->fast_cached = fb;
        h->fast_order = order;
        h->fast_leaf = o.max_leaf; h->fast_ct = o.cost_tri;
    }
    return h->fast_cached;
}

// start/stop events around a launch or a frame; next_pair: the next unused pair of a pool, created on first use
using EventPair = std::pair<Event, Event>;
static int next_pair(std::vector<EventPair>& pool, size_t& used, EventPair*& out)
{
    if (used == pool.size()) {
        EventPair q;
        HIP_TRY(create(q.first, hipEventCreate));
        HIP_TRY(create(q.second, hipEventCreate));
        pool.push_back(std::move(q));
    }
    out = &pool[used++];
    return MCPT_OK;
}

struct mcpt_device {
    int ordinal = 0;
    Knobs knobs;                           // the environment as it was when this device was created (knobs.hpp)
    DScene ds{};
    Stream stream;                         // library stream for the host-pointer entry points
    // scene arrays
    DevBuf<DNode> nodes; DevBuf<DTri> tris; DevBuf<DTriShade> shade; DevBuf<DMaterial> materials;
    DevBuf<DLight> lights; DevBuf<DLightTri> light_tris; DevBuf<double> light_cdf; DevBuf<uint8_t> texels;
    DevBuf<DTri> fast_tris; DevBuf<CwNode> cw_nodes; DevBuf<DTriPre> fast_pre;
    mcpt_fast_info fast_info{};     // what mcpt_device_fast_hierarchy reports (node and triangle slot counts, builder, clusters, depth, stack need)
    int trace_mode = MCPT_TRACE_FAST;
    DevBuf<int32_t> d_order;               // leaf -> .obj face (device build keeps it for read-back)
    mcpt_bvh_info bi{};
    // frame state
    int width = 0, height = 0;
    DevBuf<double> dirs;                   // W*H*3 primary directions
    bool dirs_ready = false;
    mcpt_lens lens{};                      // mcpt_device_set_lens (all zero: the reference's pinhole)
    DevBuf<double> pos;                    // W*H*3 image-plane points pos(i,j), made on the first frame under an active lens
    // render workspace
    DevBuf<int32_t> pixels; int64_t n_pixels = 0; int part_key[4] = {-1, -1, -1, -1};
    Event ev[4];
    Stream look_stream;                    // the host's looks at a path count travel here, so that they wait for the logic pass that wrote
    Event look_ev;                         // the count and for nothing enqueued after it (the finishing kernel above all)
    HostBuf<unsigned int> h_look;          // pinned host word the looks land in (never a pageable stack address: an async copy into
                                           // pageable memory goes through the runtime's pin-on-the-fly / staging paths)
    const mcpt_scene* scene = nullptr;     // the handle this device was created from (devices_created is given back in mcpt_device_free)
    // closest-hit and test entry points (mcpt_trace_closest*, mcpt_sample_radiance) have counters, queue words and a deferred-ray
    // list of their own: a frame in flight on another stream keeps using its frame slot's
    DevBuf<DCounters> aux_ctr; DevBuf<TraceQueue> aux_queue; DevBuf<long long> aux_slow_list;
    size_t sample_budget_bytes = size_t(4) << 30;   // megakernel path: radiance staging buffer per chunk
    size_t wf_budget_bytes = 0;                     // path state + rays per frame slot; 0 = a share of the free HBM (MCPT_WORKSPACE_GB overrides)
    size_t wf_auto_budget = 0;                      // that share, asked for once (hipMemGetInfo costs a few hundred microseconds)
    // Everything a frame in flight owns.  Two slots: with MCPT_RENDER_PIPELINE consecutive frames alternate between them, so the
    // latency-bound tail of one frame (the finishing kernel's last long paths, the fold) overlaps the head of the next on another stream.
    struct FrameSlot {
        DevBuf<PrimaryHit> hits;
        DevBuf<double> rad;                             // sized in bytes (a lens adds a hit flag per sample)
        DevBuf<char> wf_ws;
        DevBuf<int32_t> hit_slots;
        DevBuf<PrimarySurface> surf;                    // first-vertex record per hit pixel of the chunk
        DevBuf<uint8_t> cam_hit;                        // per-sample route of a lens: did the sample's camera ray hit (per chunk sample)
        DevBuf<unsigned int> alive_base;                // shaded pixels before each group of 64 hit slots
        DevBuf<WfCounts> wf_counts;                     // MCPT_WF_COUNT_SLOTS slots
        DevBuf<TraceQueue> queue;                       // persistent trace kernels: chunk queue head + deferred-ray list
        DevBuf<long long> slow_list;
        DevBuf<char> path_area;                         // records and exact-walk stacks of the pool form of the finishing pass (finish_pool_bytes)
        DevBuf<DCounters> ctr;
        Event done;                                     // recorded after the slot's last kernel of a frame
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
    LaunchCfg cfg;                                  // this GPU's resident grids and knobs
    long long finish_threshold = 500000;            // paths left at which the finishing pass takes over (MCPT_FINISH_PATHS; sweep: flat from 2e5 to 1e6)
    // Shared ownership, as a device holds its scene: the caller's handle and every progressive frame created on the device hold one
    // reference each; the device goes with the last of mcpt_device_free / mcpt_progressive_free.
    std::atomic<int> refs{1};
};

extern "C" {

int mcpt_version(void) { return MCPT_VERSION; }
const char* mcpt_last_error(void) { return g_error.c_str(); }

const char* mcpt_knobs_describe(void) { return knobs_table(); }

int mcpt_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ------------------------------------------------------------------------------------------------ which HIP runtime is this?
// libmcpt.so's code objects are built by one hipcc; the libamdhip64.so they run on is whichever the process loaded first under that
// soname (a Python process that imported torch has the wheel's bundled runtime, not /opt/rocm's).  Kernels built by a newer compiler on
// an older runtime are the likeliest cause of the abort DESIGN 8a records, and nothing used to notice: now the first device creation
// compares the two versions and refuses when major.minor differ, unless the caller has said it knows (mcpt_allow_runtime_mismatch).
static std::atomic<int> g_allow_runtime_mismatch{0};

void mcpt_allow_runtime_mismatch(int32_t allow) { g_allow_runtime_mismatch.store(allow ? 1 : 0); }

// Pure comparison (CPU unit test): 0 when a library compiled against HIP `compiled` may run on runtime `runtime` (both encoded as
// HIP_VERSION: major * 10^7 + minor * 10^5 + patch), else MCPT_ERR_HIP with a message naming both and the runtime's file.
int mcpt_hip_runtime_check(int32_t compiled, int32_t runtime, const char* runtime_path, char* msg, int64_t cap)
{
    const int cmaj = compiled / 10000000, cmin = compiled / 100000 % 100, rmaj = runtime / 10000000, rmin = runtime / 100000 % 100;
    const bool ok = compiled > 0 && runtime > 0 && cmaj == rmaj && cmin == rmin;
    if (msg && cap > 0) {
        if (ok) msg[0] = 0;
        else
            std::snprintf(msg, size_t(cap),
                          "libmcpt.so was compiled against HIP %d.%d (%d) but this process runs on HIP runtime %d.%d (%d) loaded from %s: "
                          "another libamdhip64.so was loaded first (a Python process that imported torch has the wheel's).  Load libmcpt.so "
                          "before it, or call mcpt_allow_runtime_mismatch(1) / set MCPT_ALLOW_RUNTIME_MISMATCH=1 to run anyway",
                          cmaj, cmin, compiled, rmaj, rmin, runtime, (runtime_path && runtime_path[0]) ? runtime_path : "(unknown)");
    }
    return ok ? MCPT_OK : MCPT_ERR_HIP;
}

int mcpt_hip_runtime_info(int32_t* compiled, int32_t* runtime, char* path, int64_t cap)
{
    if (compiled) *compiled = HIP_VERSION;
    int rv = 0;
    if (hipRuntimeGetVersion(&rv) != hipSuccess) { (void)hipGetLastError(); rv = 0; }
    if (runtime) *runtime = rv;
    if (path && cap > 0) {
        path[0] = 0;
        Dl_info info;
        if (dladdr(reinterpret_cast<const void*>(static_cast<hipError_t (*)(int*)>(&hipRuntimeGetVersion)), &info) && info.dli_fname) std::snprintf(path, size_t(cap), "%s", info.dli_fname);
    }
    return MCPT_OK;
}

// what mcpt_device_create / mcpt_multi_create ask before they touch a device
static int runtime_gate()
{
    int32_t compiled = 0, runtime = 0;
    char path[512], msg[1024];
    mcpt_hip_runtime_info(&compiled, &runtime, path, sizeof path);
    if (mcpt_hip_runtime_check(compiled, runtime, path, msg, sizeof msg) == MCPT_OK) return MCPT_OK;
    if (g_allow_runtime_mismatch.load() || read_knobs().allow_runtime_mismatch) {
        static std::atomic<int> told{0};
        if (!told.exchange(1)) std::fprintf(stderr, "libmcpt: %s -- running anyway, as asked\n", msg);
        return MCPT_OK;
    }
    return fail(MCPT_ERR_HIP, msg);
}

// ------------------------------------------------------------------------------------------------ scene
int mcpt_scene_load(const char* path, const char* filename, mcpt_scene** out) { return mcpt_scene_load_ex(path, filename, 0, out); }

int mcpt_scene_load_ex(const char* path, const char* filename, int32_t load_flags, mcpt_scene** out)
{
    if (!path || !filename || !out) return fail(MCPT_ERR_ARG, "null argument");
    *out = nullptr;
    if (load_flags & ~(MCPT_LOAD_STANDARD_OBJ | MCPT_LOAD_MTLLIB | MCPT_LOAD_MORTON_BOUNDS)) return fail(MCPT_ERR_ARG, "unknown load flag");
    std::unique_ptr<mcpt_scene> h(new mcpt_scene);
    std::string err;
    int rc = load_scene_files(path, filename, load_flags, h->s, err);
    if (rc) return fail(rc, err);
    rc = build_accel(h->s, err);
    if (rc) return fail(rc, err);
    *out = h.release();
    return MCPT_OK;
}
static void scene_release(const mcpt_scene* s) { if (s && s->refs.fetch_sub(1) == 1) delete s; }
void mcpt_scene_free(mcpt_scene* s) { scene_release(s); }

int mcpt_scene_create(const mcpt_scene_desc* dsc, int32_t flags, mcpt_scene** out)
{
    if (!dsc || !out) return fail(MCPT_ERR_ARG, "null argument");
    *out = nullptr;
    if (dsc->num_faces <= 0 || dsc->num_faces > 0x3fffffff || !dsc->v || !dsc->vn || !dsc->material || dsc->num_materials <= 0 ||
        !dsc->material_rec || dsc->num_lights < 0 || (dsc->num_lights && (!dsc->light_material || !dsc->light_radiance)))
        return fail(MCPT_ERR_ARG, "incomplete scene description");
    std::unique_ptr<mcpt_scene> h(new mcpt_scene);
    Scene& s = h->s;
    s.materials.resize(size_t(dsc->num_materials));
    for (int m = 0; m < dsc->num_materials; m++) {
        MaterialRec& r = s.materials[m];
        const double* q = dsc->material_rec + size_t(m) * 8;
        r.name = (dsc->material_names && dsc->material_names[m]) ? dsc->material_names[m] : ("material" + std::to_string(m));
        r.kd = Vec3{q[0], q[1], q[2]}; r.ks = Vec3{q[3], q[4], q[5]}; r.Ns = q[6]; r.Ni = q[7];
    }
    const int64_t t = dsc->num_faces;
    s.faces.resize(size_t(t));
    for (int64_t i = 0; i < t; i++) {
        FaceRec& f = s.faces[size_t(i)];
        const int m = dsc->material[i];
        if (m < 0 || m >= dsc->num_materials) return fail(MCPT_ERR_PARSE, "face material index out of range");
        for (int c = 0; c < 3; c++) {
            f.v[c] = Vec3{dsc->v[i * 9 + c * 3], dsc->v[i * 9 + c * 3 + 1], dsc->v[i * 9 + c * 3 + 2]};
            f.vn[c] = Vec3{dsc->vn[i * 9 + c * 3], dsc->vn[i * 9 + c * 3 + 1], dsc->vn[i * 9 + c * 3 + 2]};
            f.vt[c][0] = dsc->vt ? dsc->vt[i * 6 + c * 2] : 0.0; f.vt[c][1] = dsc->vt ? dsc->vt[i * 6 + c * 2 + 1] : 0.0;
        }
        f.material = m;
        f.nrm = normalized(cross(f.v[0] - f.v[1], f.v[2] - f.v[0]));              // Face::calNorm
        const Vec3 center = (f.v[0] + f.v[1] + f.v[2]) / 3;
        f.morton = morton_code(float(center.x), float(center.y), float(center.z));
        s.materials[m].faces.push_back(int32_t(i));
    }
    s.lights.resize(size_t(dsc->num_lights));
    for (int l = 0; l < dsc->num_lights; l++) {
        LightRec& r = s.lights[l];
        r.material = dsc->light_material[l];
        if (r.material < 0 || r.material >= dsc->num_materials) return fail(MCPT_ERR_PARSE, "light material index out of range");
        r.name = s.materials[r.material].name;
        r.radiance = Vec3{dsc->light_radiance[l * 3], dsc->light_radiance[l * 3 + 1], dsc->light_radiance[l * 3 + 2]};
    }
    s.eye = Vec3{dsc->eye[0], dsc->eye[1], dsc->eye[2]}; s.look_at = Vec3{dsc->look_at[0], dsc->look_at[1], dsc->look_at[2]};
    s.up = Vec3{dsc->up[0], dsc->up[1], dsc->up[2]}; s.fovy = dsc->fovy; s.width = dsc->width; s.height = dsc->height;
    std::string err;
    int rc = finish_scene(s, "scene description", err);
    if (rc) return fail(rc, err);
    s.bi = bvh_shape(int(t));
    if (!(flags & MCPT_SCENE_DEFER_BUILD)) {
        rc = build_accel(s, err);
        if (rc) return fail(rc, err);
    }
    *out = h.release();
    return MCPT_OK;
}

int mcpt_scene_set_resolution(mcpt_scene* s, int32_t w, int32_t h)
{
    if (!s || w <= 0 || h <= 0) return fail(MCPT_ERR_ARG, "bad resolution");
    // a device caches the camera frame, the primary directions and its frame size when it is created; changing the resolution
    // under it would make callers size their frame buffers for another picture than the device writes
    if (s->devices_created.load() > 0 && (w != s->s.width || h != s->s.height))
        return fail(MCPT_ERR_ARG, "the resolution cannot change after a device has been created from the scene");
    s->s.width = w; s->s.height = h;
    return MCPT_OK;
}

int mcpt_scene_get_info(const mcpt_scene* h, mcpt_scene_info* o)
{
    if (!h || !o) return fail(MCPT_ERR_ARG, "null argument");
    const Scene& s = h->s;
    o->num_faces = int32_t(s.faces.size()); o->num_materials = int32_t(s.materials.size()); o->num_lights = int32_t(s.lights.size());
    o->width = s.width; o->height = s.height;
    o->eye[0] = s.eye.x; o->eye[1] = s.eye.y; o->eye[2] = s.eye.z;
    o->look_at[0] = s.look_at.x; o->look_at[1] = s.look_at.y; o->look_at[2] = s.look_at.z;
    o->up[0] = s.up.x; o->up[1] = s.up.y; o->up[2] = s.up.z;
    o->fovy = s.fovy; o->bvh = s.bi;
    return MCPT_OK;
}

int mcpt_scene_get_faces(const mcpt_scene* h, double* g, int32_t* material, uint32_t* morton)
{
    if (!h) return fail(MCPT_ERR_ARG, "null scene");
    const Scene& s = h->s;
    for (size_t i = 0; i < s.faces.size(); i++) {
        const FaceRec& f = s.faces[i];
        if (g) {
            double* o = g + i * 27;
            for (int c = 0; c < 3; c++) { o[c * 3] = f.v[c].x; o[c * 3 + 1] = f.v[c].y; o[c * 3 + 2] = f.v[c].z; }
            for (int c = 0; c < 3; c++) { o[9 + c * 3] = f.vn[c].x; o[9 + c * 3 + 1] = f.vn[c].y; o[9 + c * 3 + 2] = f.vn[c].z; }
            for (int c = 0; c < 3; c++) { o[18 + c * 2] = f.vt[c][0]; o[18 + c * 2 + 1] = f.vt[c][1]; }
            o[24] = f.nrm.x; o[25] = f.nrm.y; o[26] = f.nrm.z;
        }
        if (material) material[i] = f.material;
        if (morton) morton[i] = f.morton;
    }
    return MCPT_OK;
}

int mcpt_scene_get_leaf_order(const mcpt_scene* h, int32_t* o)
{
    if (!h || !o) return fail(MCPT_ERR_ARG, "null argument");
    if (!h->s.accel_built) return fail(MCPT_ERR_ARG, "scene has no host build (MCPT_SCENE_DEFER_BUILD): read the device's copy");
    std::copy(h->s.order.begin(), h->s.order.end(), o);
    return MCPT_OK;
}

int mcpt_scene_get_bvh_nodes(const mcpt_scene* h, double* box6, int32_t* level, int32_t* leaf_face)
{
    if (!h) return fail(MCPT_ERR_ARG, "null scene");
    const Scene& s = h->s;
    if (!s.accel_built) return fail(MCPT_ERR_ARG, "scene has no host build (MCPT_SCENE_DEFER_BUILD): read the device's copy");
    for (int i = 0; i < s.bi.Nr; i++) {
        const NodeBox& b = s.nodes[i];
        if (box6) { double* o = box6 + size_t(i) * 6; o[0] = b.max_x; o[1] = b.max_y; o[2] = b.max_z; o[3] = b.min_x; o[4] = b.min_y; o[5] = b.min_z; }
        if (level) level[i] = s.node_level[i];
        if (leaf_face) leaf_face[i] = s.node_leaf[i] >= 0 ? s.order[s.node_leaf[i]] : -1;
    }
    return MCPT_OK;
}

int mcpt_scene_find_index(const mcpt_scene* h, int32_t i, int32_t l) { return h ? find_index(h->s.bi, i, l) : -1; }

int mcpt_scene_get_material(const mcpt_scene* h, int32_t m, char name[64], double r[8], int32_t fl[4])
{
    if (!h || m < 0 || m >= int(h->s.materials.size())) return fail(MCPT_ERR_ARG, "material index");
    const MaterialRec& mt = h->s.materials[m];
    if (name) { std::memset(name, 0, 64); std::strncpy(name, mt.name.c_str(), 63); }
    if (r) { r[0] = mt.kd.x; r[1] = mt.kd.y; r[2] = mt.kd.z; r[3] = mt.ks.x; r[4] = mt.ks.y; r[5] = mt.ks.z; r[6] = mt.Ns; r[7] = mt.Ni; }
    if (fl) { fl[0] = mt.has_map; fl[1] = mt.map_w; fl[2] = mt.map_h; fl[3] = mt.light; }
    return MCPT_OK;
}

int mcpt_scene_get_light(const mcpt_scene* h, int32_t i, char name[64], double rad[3], int32_t* material, double* area)
{
    if (!h || i < 0 || i >= int(h->s.lights.size())) return fail(MCPT_ERR_ARG, "light index");
    const LightRec& l = h->s.lights[i];
    if (name) { std::memset(name, 0, 64); std::strncpy(name, l.name.c_str(), 63); }
    if (rad) { rad[0] = l.radiance.x; rad[1] = l.radiance.y; rad[2] = l.radiance.z; }
    if (material) *material = l.material;
    if (area) *area = l.total_area;
    return MCPT_OK;
}

uint32_t mcpt_morton_code(float x, float y, float z) { return morton_code(x, y, z); }

// Engine of the fast walk for a scene of t triangles (include/mcpt.h: mcpt_scene_trace_engine).  Measured on MI355X, frame times pool /
// vote: cornell-box (15 k triangles) 82.0 / 92.3 ms, veach-mis 147.5 / 160.7, one eighth of a cornell-box frame 13.9 / 15.3; the 204 k
// triangle interior 253 / 250, 10 M triangles 56.3 / 52.8: where the walk waits for memory, the pool engine's longer chain of dependent
// LDS and memory round trips per step costs what its fuller lanes save, or more.
static int trace_engine_for(long long t, const Knobs& k)
{
    if (k.trace_engine == 1) return (mcpt_device_count() > 0 && !pool_engine_available()) ? MCPT_ENGINE_VOTE : MCPT_ENGINE_POOL;
    if (k.trace_engine == 0) return MCPT_ENGINE_VOTE;
    if (t > k.pool_max_tris) return MCPT_ENGINE_VOTE;
    // (a device that cannot hold the pool engine's workgroup -- 1024 threads, 159 KB of LDS -- runs the voting engine; without a device
    // the answer is the policy's)
    if (mcpt_device_count() > 0 && !pool_engine_available()) {
        static std::atomic<int> told{0};
        if (!told.exchange(1)) std::fprintf(stderr, "libmcpt: this device cannot hold the pool engine's workgroup; the voting engine runs instead\n");
        return MCPT_ENGINE_VOTE;
    }
    return MCPT_ENGINE_POOL;
}

int mcpt_scene_trace_engine(const mcpt_scene* h)
{
    if (!h) return fail(MCPT_ERR_ARG, "null argument");
    return trace_engine_for((long long)h->s.faces.size(), read_knobs());      // (what a device created now would use)
}

int mcpt_scene_fast_bvh_stats(const mcpt_scene* h, int32_t* n_nodes, int32_t* max_depth, int32_t* leaf_order, int32_t* nesting_ok)
{
    if (!h) return fail(MCPT_ERR_ARG, "null scene");
    FastBvh fb;
    if (!h->s.accel_built) return fail(MCPT_ERR_ARG, "scene was created without a host build");
    { const Knobs k = read_knobs(); build_fast_bvh(h->s.faces, h->s.order.data(), h->s.bi.t, fb, stack_limit_for(k), build_opts_for(k)); }
    if (n_nodes) *n_nodes = int32_t(fb.nodes.size());
    if (max_depth) *max_depth = fb.max_depth;
    if (leaf_order) std::copy(fb.leaf_tris.begin(), fb.leaf_tris.end(), leaf_order);
    if (nesting_ok) {
        // every child box must contain what hangs below it: inner children by their own child boxes, leaves by the
        // reference's leaf boxes of their triangles
        const Scene& s = h->s;
        const int leaf0 = find_index(s.bi, (1 << s.bi.Level) - 1, s.bi.Level);
        bool ok = true;
        for (const FastNode& nd : fb.nodes)
            for (int c = 0; c < 2; c++) {
                const int32_t ref = nd.child[c];
                if (ref == kFastEmpty) continue;
                auto inside = [&](const double lo[3], const double hi[3]) {
                    for (int a = 0; a < 3; a++) if (lo[a] < nd.lo[c][a] || hi[a] > nd.hi[c][a]) ok = false;
                };
                if (ref >= 0) { inside(fb.nodes[ref].lo[0], fb.nodes[ref].hi[0]); if (fb.nodes[ref].child[1] != kFastEmpty) inside(fb.nodes[ref].lo[1], fb.nodes[ref].hi[1]); }
                else {
                    const int r = -1 - ref, first = r >> 4, count = (r & 7) + 1;
                    for (int i = 0; i < count; i++) {
                        const NodeBox& b = s.nodes[leaf0 + fb.leaf_tris[first + i]];
                        const double lo[3] = {b.min_x, b.min_y, b.min_z}, hi[3] = {b.max_x, b.max_y, b.max_z};
                        inside(lo, hi);
                    }
                }
            }
        // compressed nodes: every decoded child box must contain the fp64 box of what it refers to
        {
            std::vector<std::array<double, 6>> cwbox(fb.cw.size());     // fp64 box of each CwNode (union of its children's true boxes)
            std::vector<int> bin_of(fb.cw.size(), -1);
            // recompute true boxes bottom-up through the binary tree: box of a FastNode child is stored in its parent
            std::function<void(int, int, const double*, const double*)> walk;   // (cw node, unused, lo, hi)
            auto leaf_box = [&](int32_t ref, double lo[3], double hi[3]) {
                const int r = -1 - ref, first = r >> 4, count = (r & 7) + 1;
                for (int a = 0; a < 3; a++) { lo[a] = 1e300; hi[a] = -1e300; }
                for (int i = 0; i < count; i++) {
                    const NodeBox& b = s.nodes[leaf0 + fb.leaf_tris[first + i]];
                    const double l[3] = {b.min_x, b.min_y, b.min_z}, h2[3] = {b.max_x, b.max_y, b.max_z};
                    for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], l[a]); hi[a] = std::max(hi[a], h2[a]); }
                }
            };
            std::function<void(int, double*, double*)> true_box = [&](int n, double* lo, double* hi) {
                for (int a = 0; a < 3; a++) { lo[a] = 1e300; hi[a] = -1e300; }
                const CwNode& nd = fb.cw[n];
                for (int c = 0; c < 4; c++) {
                    if (nd.child[c] == kFastEmpty) continue;
                    double cl[3], ch[3];
                    if (nd.child[c] >= 0) true_box(nd.child[c], cl, ch); else leaf_box(nd.child[c], cl, ch);
                    for (int a = 0; a < 3; a++) {
                        const double sc = std::ldexp(1.0, nd.e[a]);
                        const double dl = double(nd.p[a]) + double((nd.qlo[a] >> (8 * c)) & 255u) * sc;
                        const double dh = double(nd.p[a]) + double((nd.qhi[a] >> (8 * c)) & 255u) * sc;
                        if (dl > cl[a] || dh < ch[a]) ok = false;
                        lo[a] = std::min(lo[a], cl[a]); hi[a] = std::max(hi[a], ch[a]);
                    }
                }
            };
            double lo[3], hi[3];
            if (!fb.cw.empty()) true_box(0, lo, hi);
            // every triangle slot must be reachable exactly once
            std::vector<int> seen(fb.leaf_tris.size(), 0);
            for (const CwNode& nd : fb.cw)
                for (int c = 0; c < 4; c++)
                    if (nd.child[c] < 0 && nd.child[c] != kFastEmpty) {
                        const int r = -1 - nd.child[c], first = r >> 4, count = (r & 7) + 1;
                        for (int i = 0; i < count; i++) seen[first + i]++;
                    }
            for (int v : seen) if (v != 1) ok = false;
            if (fb.cw_stack_need >= kFastMaxDepth) ok = false;
        }
        *nesting_ok = ok ? 1 : 0;
    }
    return MCPT_OK;
}

// ------------------------------------------------------------------------------------------------ partition
static void tile_shape(const mcpt_render_params* p, int& tw, int& th, int& rank, int& world)
{
    tw = (p && p->tile_w > 0) ? p->tile_w : 32;
    th = (p && p->tile_h > 0) ? p->tile_h : 8;
    world = (p && p->world > 1) ? p->world : 1;
    rank = (p && world > 1) ? p->rank : 0;
}

// Tile (tx, ty) belongs to rank (tx + shift*ty) mod world, shift = the first integer >= world/2 that is coprime with
// world: consecutive tiles of a row go round-robin over the ranks and every tile row starts on a different rank, so no
// rank ends up with a fixed set of image columns (a plain "tile index mod world" does when the row length is a multiple
// of world -- 1280/32 = 40 tiles per row with 8 ranks -- and the empty sides of a frame then unbalance the ranks).
static int tile_shift(int world)
{
    auto gcd = [](int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; };
    for (int s = std::max(1, world / 2); s < world; s++) if (gcd(s, world) == 1) return s;
    return 1;
}

static void owned_pixel_list(int W, int H, int tw, int th, int rank, int world, std::vector<int32_t>& out)
{
    out.clear();
    const int shift = tile_shift(world);
    for (int y = 0; y < H; y++) {
        const int ty = y / th;
        for (int x = 0; x < W; x++) {
            const int tx = x / tw;
            if ((tx + shift * ty) % world == rank) out.push_back(y * W + x);
        }
    }
}

int64_t mcpt_owned_pixels(const mcpt_scene* h, const mcpt_render_params* p, int32_t* pixels)
{
    if (!h) return fail(MCPT_ERR_ARG, "null scene");
    int tw, th, rank, world;
    tile_shape(p, tw, th, rank, world);
    if (rank < 0 || rank >= world) return fail(MCPT_ERR_ARG, "rank outside world");
    std::vector<int32_t> v;
    owned_pixel_list(h->s.width, h->s.height, tw, th, rank, world, v);
    if (pixels) std::copy(v.begin(), v.end(), pixels);
    return int64_t(v.size());
}

// ------------------------------------------------------------------------------------------------ device
void mcpt_device_free(mcpt_device* d)
{
    if (!d || d->refs.fetch_sub(1) != 1) return;
    (void)hipSetDevice(d->ordinal);
    (void)hipDeviceSynchronize();          // frames of a sequence may still be in flight on the caller's streams
    if (d->scene) { d->scene->devices_created.fetch_sub(1); scene_release(d->scene); }
    delete d;                              // (its buffers, events and streams with it)
}

int mcpt_device_create(const mcpt_scene* h, int32_t ordinal, mcpt_device** out)
{
    return mcpt_device_create_ex(h, ordinal, (h && !h->s.accel_built) ? MCPT_BUILD_DEVICE : MCPT_BUILD_HOST, out);
}

// ------------------------------------------------------------------------------------------------ device creation, stage by stage
// Each stage writes into d and returns an MCPT_* code.  Whatever it allocates is in a d-> field by the time it returns, so the
// caller's mcpt_device_free releases it when a later stage fails; temporaries are freed where they are made.

// MCPT_PRINT_DIAG on a large scene: how far device creation has come, and when
struct CreateClock {
    bool talk; std::chrono::steady_clock::time_point t0;
    void lap(const char* what) const { if (talk) std::fprintf(stderr, "device create: %s at %.2f s\n", what, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()); }
};
static void put3(double* o, const Vec3& v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }

// The reference's structures in HBM -- uploaded from the host build (MCPT_BUILD_HOST) or built on the GPU (the other modes) -- and
// the leaf order (leaf -> .obj face) either way
static int create_reference(mcpt_device* d, const Scene& s, int32_t build_mode, const CreateClock& clock, std::vector<int32_t>& order)
{
    const mcpt_bvh_info& bi = d->bi;
    const int t = bi.t;
    if (build_mode == MCPT_BUILD_HOST) {
        std::vector<DNode> nodes(bi.Nr);             // (records filled in place: the vectors zero them first)
        for (int i = 0; i < bi.Nr; i++) {
            const NodeBox& b = s.nodes[i];
            DNode& n = nodes[i];
            n.mn[0] = b.min_x; n.mn[1] = b.min_y; n.mn[2] = b.min_z; n.mx[0] = b.max_x; n.mx[1] = b.max_y; n.mx[2] = b.max_z;
        }
        std::vector<DTri> tris(t);
        std::vector<DTriShade> shade(t);
        for (int k = 0; k < t; k++) {
            const FaceRec& f = s.faces[s.order[k]];
            DTri& q = tris[k];
            DTriShade& a = shade[k];
            double *v[3] = {q.v1, q.v2, q.v3}, *vn[3] = {a.vn1, a.vn2, a.vn3}, *vt[3] = {a.vt1, a.vt2, a.vt3};
            for (int c = 0; c < 3; c++) { put3(v[c], f.v[c]); put3(vn[c], f.vn[c]); vt[c][0] = f.vt[c][0]; vt[c][1] = f.vt[c][1]; }
            put3(q.n, f.nrm);
            q.material = f.material; q.face = s.order[k]; q.leaf = k;
        }
        order = s.order;
        HIP_TRY(d->nodes.upload(nodes));
        HIP_TRY(d->tris.upload(tris));
        HIP_TRY(d->shade.upload(shade));
        HIP_TRY(d->d_order.upload(order));
    } else {
        // faces in .obj order -> HBM, then Morton keys, stable sort, leaf records and the level-by-level union on the GPU
        // (no zero fill: 2.2 GB at 10 M triangles, every element is written below)
        std::vector<double, default_init_alloc<double>> v9(size_t(t) * 9), vn9(size_t(t) * 9), vt6(size_t(t) * 6), nrm3(size_t(t) * 3);
        std::vector<int32_t, default_init_alloc<int32_t>> mat(static_cast<size_t>(t));
        parallel_pieces(t, [&](long long ib, long long ie) {
        for (long long i = ib; i < ie; i++) {
            const FaceRec& f = s.faces[size_t(i)];
            for (int c = 0; c < 3; c++) {
                put3(&v9[size_t(i) * 9 + c * 3], f.v[c]); put3(&vn9[size_t(i) * 9 + c * 3], f.vn[c]);
                vt6[size_t(i) * 6 + c * 2] = f.vt[c][0]; vt6[size_t(i) * 6 + c * 2 + 1] = f.vt[c][1];
            }
            put3(&nrm3[size_t(i) * 3], f.nrm);
            mat[size_t(i)] = f.material;
        }
        });
        clock.lap("faces staged");
        DevBuf<double> d_v9, d_vn9, d_vt6, d_nrm3;
        DevBuf<int32_t> d_mat;
        HIP_TRY(d_v9.upload(v9));
        HIP_TRY(d_vn9.upload(vn9));
        HIP_TRY(d_vt6.upload(vt6));
        HIP_TRY(d_nrm3.upload(nrm3));
        HIP_TRY(d_mat.upload(mat));
        hipError_t e = d->nodes.alloc(size_t(bi.Nr));
        if (e == hipSuccess) e = d->tris.alloc(size_t(t));
        if (e == hipSuccess) e = d->shade.alloc(size_t(t));
        if (e == hipSuccess) e = d->d_order.alloc(size_t(t));
        if (e == hipSuccess) {
            BuildInputs in{d_v9.get(), d_vn9.get(), d_vt6.get(), d_nrm3.get(), d_mat.get(), t, {s.morton_lo[0], s.morton_lo[1], s.morton_lo[2]},
                           {s.morton_span[0], s.morton_span[1], s.morton_span[2]}};
            e = device_build_reference(in, bi, d->nodes.get(), d->tris.get(), d->shade.get(), d->d_order.get(), d->stream.get());
        }
        order.resize(t);
        if (e == hipSuccess) e = hipMemcpy(order.data(), d->d_order.get(), size_t(t) * sizeof(int32_t), hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail(MCPT_ERR_HIP, std::string("device build: ") + hipGetErrorString(e));
    }
    clock.lap("reference structures in HBM");
    return MCPT_OK;
}

// materials and their texels, lights, light triangles and their CDF
static int create_materials_and_lights(mcpt_device* d, const Scene& s)
{
    std::vector<uint8_t> texels;
    std::vector<DMaterial> mats(s.materials.size());
    for (size_t i = 0; i < s.materials.size(); i++) {
        const MaterialRec& m = s.materials[i];
        DMaterial& dm = mats[i];
        put3(dm.kd, m.kd); put3(dm.ks, m.ks);
        dm.Ns = m.Ns; dm.Ni = m.Ni; dm.has_map = m.has_map; dm.map_w = m.map_w; dm.map_h = m.map_h; dm.light = m.light;
        dm.tex_offset = int64_t(texels.size());
        texels.insert(texels.end(), m.bgr.begin(), m.bgr.end());
    }
    std::vector<DLight> lights(s.lights.size());
    std::vector<DLightTri> ltris;
    std::vector<double> lcdf;
    for (size_t i = 0; i < s.lights.size(); i++) {
        const LightRec& l = s.lights[i];
        const MaterialRec& m = s.materials[l.material];
        DLight& dl = lights[i];
        put3(dl.radiance, l.radiance);
        dl.total_area = l.total_area; dl.material = l.material; dl.ntri = int32_t(m.faces.size());
        dl.first = int32_t(ltris.size()); dl.cdf_sorted = l.cdf_sorted ? 1 : 0;
        for (size_t j = 0; j < m.faces.size(); j++) {
            const FaceRec& f = s.faces[m.faces[j]];
            DLightTri q{};
            double *v[3] = {q.v1, q.v2, q.v3}, *vn[3] = {q.vn1, q.vn2, q.vn3};
            for (int c = 0; c < 3; c++) { put3(v[c], f.v[c]); put3(vn[c], f.vn[c]); }
            ltris.push_back(q);
            lcdf.push_back(l.cdf[j]);
        }
    }
    HIP_TRY(d->materials.upload(mats));
    HIP_TRY(d->lights.upload(lights));
    HIP_TRY(d->light_tris.upload(ltris));
    HIP_TRY(d->light_cdf.upload(lcdf));
    HIP_TRY(d->texels.upload(texels));
    return MCPT_OK;
}

// The whole hierarchy from the n_lower nodes a GPU builder left in d_lower.  n_top == 1: they are the whole tree.  Otherwise they
// are a forest of n_top clusters: the host's SAH tree over the clusters' boxes goes in front of them, and d_lower goes.
// roots[c] = lower node of cluster c's root, < 0: the cluster is one leaf and this is its reference; null: cluster c's root is
// lower node c.  lower_need / lower_depth = stack entries / inner levels a walk below a cluster root may take.
static int stitch_clusters(mcpt_device* d, DevBuf<CwNode> d_lower, int n_lower, int n_top, const std::vector<double>& top_boxes, const int32_t* roots,
                           int lower_need, int lower_depth)
{
    mcpt_fast_info& fi = d->fast_info;
    if (n_top == 1) {                        // small scene: the GPU's tree is the whole tree
        d->cw_nodes = std::move(d_lower);
        fi.n_nodes = n_lower; fi.max_depth = lower_depth; fi.cw_stack_need = lower_need;
        return MCPT_OK;
    }
    FastBvh up;
    build_fast_upper(top_boxes.data(), n_top, lower_need, up);
    const int n_up = int(up.cw.size());
    for (CwNode& nd : up.cw)
        for (int c = 0; c < 4; c++)
            if (nd.child[c] < 0 && nd.child[c] != kFastEmpty) {            // cluster -> its root node, or its triangles if it is one leaf
                const int cluster = -1 - nd.child[c];
                const int32_t r = roots ? roots[cluster] : cluster;
                nd.child[c] = r >= 0 ? n_up + r : r;
            }
    hipError_t e = d->cw_nodes.alloc(size_t(n_up + n_lower));
    CwNode* const cw = d->cw_nodes.get();
    if (e == hipSuccess) e = hipMemcpy(cw, up.cw.data(), size_t(n_up) * sizeof(CwNode), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpyAsync(cw + n_up, d_lower.get(), size_t(n_lower) * sizeof(CwNode), hipMemcpyDeviceToDevice, d->stream.get());
    if (e == hipSuccess) e = device_offset_children(cw + n_up, n_lower, n_up, d->stream.get());
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream.get());
    if (e != hipSuccess) return fail(MCPT_ERR_HIP, std::string("device build of the fast hierarchy: ") + hipGetErrorString(e));
    fi.n_nodes = int32_t(n_up + n_lower); fi.max_depth = up.max_depth + lower_depth;
    fi.cw_stack_need = up.cw_stack_need;     // includes lower_need
    return MCPT_OK;
}

// MCPT_BUILD_DEVICE_FAST / MCPT_BUILD_DEVICE_SAH: the lower part of the hierarchy built on the GPU in place over the leaf-ordered
// triangles, the host's tree over its clusters.  PLOC (MCPT_BUILD_DEVICE_SAH) that leaves too many clusters falls back to Morton.
static int build_hierarchy_on_device(mcpt_device* d, const double lo[3], const double hi[3], bool ploc, const CreateClock& clock, double* absmax)
{
    const Knobs& K = d->knobs;
    const int t = d->bi.t;
    d->fast_info.n_tris = t;
    DevBuf<CwNode> d_lower;
    int n_lower = 0, n_top = 0;
    std::vector<double> top_boxes;
    if (ploc) {
        // clusters grown by locally-ordered clustering on the GPU (build_kernels.hip: device_build_ploc), the host's SAH tree over them;
        // how tall a cluster may grow: what the walk's stack leaves once the tree over the expected number of clusters has its levels
        int height = K.ploc_height;
        if (!height) {
            const long long est = std::max<long long>(1, 2ll * t / K.ploc_cluster);
            int lv = 1;
            while ((1ll << lv) < est) lv++;
            height = std::max(6, std::min(20, 35 - 5 - lv));
        }
        std::vector<int32_t> top_roots;
        int lower_need = 0, rounds = 0;
        const hipError_t e = device_build_ploc(d->tris.get(), t, lo, hi, K.ploc_cluster, height, K.ploc_radius, K.ploc_leaf ? K.ploc_leaf : kFastDefaultLeaf,
                                               K.ploc_area > 0 ? 1.0 / K.ploc_area : 0.0, K.ploc_ct, K.ploc_cl, K.ploc_budget, d_lower, d->fast_tris, &n_lower,
                                               &n_top, &top_boxes, &top_roots, &lower_need, absmax, &rounds, d->stream.get());
        if (e != hipErrorNotSupported) {
            if (e != hipSuccess) return fail(MCPT_ERR_HIP, std::string("device build of the fast hierarchy (clustering): ") + hipGetErrorString(e));
            clock.lap("clusters on the GPU");
            if (clock.talk) std::fprintf(stderr, "device create: %d clusters in %d rounds, %d nodes below them, stack need below a cluster root %d\n", n_top, rounds, n_lower, lower_need);
            d->fast_info.builder = MCPT_FAST_BUILT_DEVICE_PLOC;
            d->fast_info.clusters = n_top;
            return stitch_clusters(d, std::move(d_lower), n_lower, n_top, top_boxes, top_roots.data(), lower_need, lower_need);
        }
    }
    // Clusters of Morton-consecutive triangles on the GPU (by default one compressed node over four single-triangle leaves:
    // every triangle keeps its own quantised box), a SAH tree over the clusters' boxes on the host.  Sweep on MI355X
    // (MCPT_CLUSTER_LEAF x MCPT_CLUSTER_LEVELS, ms per frame synthetic 10 M SPP 16 / cornell-box): 1x1 87 / 143, 1x2 93 / 161,
    // 1x3 103 / 182, 2x1 116 / 177, 4x2 163 / 238; the host's full SAH tree: 56 / 110.
    int levels = 0;
    const hipError_t e = device_build_fast(d->tris.get(), t, lo, hi, K.cluster_leaf, K.cluster_levels, d_lower, d->fast_tris, &n_lower, &levels, &n_top, &top_boxes,
                                           absmax, d->stream.get());
    if (e != hipSuccess) return fail(MCPT_ERR_HIP, std::string("device build of the fast hierarchy: ") + hipGetErrorString(e));
    d->fast_info.builder = ploc ? MCPT_FAST_BUILT_PLOC_FELL_BACK : MCPT_FAST_BUILT_DEVICE_FAST;
    return stitch_clusters(d, std::move(d_lower), n_lower, n_top, top_boxes, nullptr, 3 * levels, levels);   // three siblings pushed per level on the way down
}

// The fast walk's culling hierarchy: fills d->cw_nodes, d->fast_tris and d->fast_info; *absmax = largest |coordinate| of the scene
static int create_hierarchy(mcpt_device* d, const mcpt_scene* h, int32_t build_mode, const std::vector<int32_t>& order, const CreateClock& clock, double* absmax)
{
    // one pass over the faces: the scene's bounds, which the GPU builders sort on (a NaN coordinate passes neither comparison), and
    // whether every coordinate is zero or within [1e-150, 1e150], as the fast walk needs (NaN and infinities are not)
    bool coords_ok = true;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (const FaceRec& f : h->s.faces)
        for (int c = 0; c < 3; c++) {
            const double q[3] = {f.v[c].x, f.v[c].y, f.v[c].z};
            for (int a = 0; a < 3; a++) {
                const double m = std::fabs(q[a]);
                if (!(m == 0.0 || (m >= 1e-150 && m <= 1e150))) coords_ok = false;
                if (q[a] < lo[a]) lo[a] = q[a];
                if (q[a] > hi[a]) hi[a] = q[a];
            }
        }
    mcpt_fast_info& fi = d->fast_info;
    if (build_mode == MCPT_BUILD_DEVICE_FAST || build_mode == MCPT_BUILD_DEVICE_SAH) {
        if (const int rc = build_hierarchy_on_device(d, lo, hi, build_mode == MCPT_BUILD_DEVICE_SAH, clock, absmax)) return rc;
    } else {
        // the SAH hierarchy built on the host from the leaf order (accel_build.cpp, shared by every device of the scene), its
        // permuted triangle copy gathered on the GPU
        const std::shared_ptr<const FastBvh> fb = shared_fast_bvh(h, order, d->knobs);
        clock.lap("culling hierarchy on the host");
        DevBuf<int32_t> d_slots;
        HIP_TRY(d->cw_nodes.upload(fb->cw));
        HIP_TRY(d_slots.upload(fb->leaf_tris));
        hipError_t e = d->fast_tris.alloc(fb->leaf_tris.size());
        if (e == hipSuccess) e = device_gather_tris(d->tris.get(), d_slots.get(), int(fb->leaf_tris.size()), d->fast_tris.get(), d->stream.get());
        if (e == hipSuccess) e = hipStreamSynchronize(d->stream.get());
        if (e != hipSuccess) return fail(MCPT_ERR_HIP, std::string("fast triangle gather: ") + hipGetErrorString(e));
        fi.builder = MCPT_FAST_BUILT_HOST;
        fi.n_nodes = int32_t(fb->cw.size()); fi.n_tris = int32_t(fb->leaf_tris.size());
        fi.max_depth = fb->max_depth; fi.cw_stack_need = fb->cw_stack_need;
        *absmax = fb->scene_absmax;
    }
    fi.enabled = (coords_ok && fi.max_depth < kFastMaxDepth && fi.cw_stack_need < kFastMaxDepth && *absmax >= 1e-15 && *absmax <= 1e15) ? 1 : 0;
    return MCPT_OK;
}

// The pre-test pays where the walk is bound by instruction issue, i.e. where nodes and triangles come out of L1 / L2 / the 256-MB
// Infinity Cache (cornell-box: 7.38 -> 7.25 ms per k_wf_trace launch; veach-mis and the 204 k-triangle interior alike).  On the
// 10 M-triangle scene the walk waits for memory, and a second dependent fetch per leaf (48-B record, then the 128-B record of a
// survivor) costs more than the skipped arithmetic saves: 6.90 vs 6.44 ms per launch.  So: records only for scenes of at most
// MCPT_PRE_TEST_MAX_TRIS triangles (default 2^20: ~200 B per triangle of nodes, records and triangles stay cache-resident).
static int create_pre_test(mcpt_device* d, double absmax)
{
    if (d->bi.t > d->knobs.pre_test_max_tris) return MCPT_OK;
    // fp32 records of the triangle phase's pre-test, one per slot of the fast triangle array
    const int n_slots = d->fast_info.n_tris;
    // (four records of padding: the pre-test reads its triangles in rounds of up to four slots, used or not)
    hipError_t e = d->fast_pre.alloc(size_t(n_slots) + 4);
    if (e == hipSuccess) e = hipMemsetAsync(d->fast_pre.get() + n_slots, 0, 4 * sizeof(DTriPre), d->stream.get());
    if (e == hipSuccess) e = device_build_pre(d->fast_tris.get(), n_slots, absmax, d->fast_pre.get(), d->stream.get());
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream.get());
    if (e != hipSuccess) return fail(MCPT_ERR_HIP, std::string("pre-test records: ") + hipGetErrorString(e));
    return MCPT_OK;
}

// engine choice, frame slots, auxiliary buffers of the closest-hit entry points, finishing threshold and workspace budget
static int create_workspaces(mcpt_device* d, const Scene& s)
{
    const Knobs& K = d->knobs;
    if (K.slow_list) d->slow_cap = unsigned(K.slow_list);   // tests shrink it to force the overflow path
    init_launch_cfg(d->cfg, K.logic_grid, K.trace_block_rays, K.trace_min_chunk, K.trace_max_chunk);
    d->cfg.trace_pool = trace_engine_for(d->bi.t, K) == MCPT_ENGINE_POOL ? 1 : 0;
    // the pool engine keeps the stack entries of a ray beyond those it has in LDS in an area behind the deferred-ray list of the launch
    const size_t spill_bytes = d->cfg.trace_pool ? pool_spill_bytes(d->cfg.cus) : 0;
    // ... and finishes a frame's last paths in path mode (MCPT_FINISH_ENGINE=lane: the one-lane-per-path kernel, for A/B runs)
    d->cfg.finish_pool = K.finish_engine == 0 ? 0 : d->cfg.trace_pool;
    const size_t path_bytes = d->cfg.finish_pool ? finish_pool_bytes(d->cfg.cus, int(s.lights.size())) : 0;     // (0: a path's rays do not fit a lane's slots)
    if (!path_bytes) d->cfg.finish_pool = 0;
    for (auto& f : d->slot) {
        if (path_bytes) HIP_TRY(f.path_area.alloc(path_bytes));
        HIP_TRY(f.ctr.alloc(1));
        HIP_TRY(hipMemset(f.ctr.get(), 0, sizeof(DCounters)));
        HIP_TRY(f.wf_counts.alloc(MCPT_WF_COUNT_SLOTS));
        HIP_TRY(f.queue.alloc(1));
        HIP_TRY(f.slow_list.alloc_bytes(size_t(d->slow_cap) * sizeof(long long) + spill_bytes));     // (the pool engine's spill area behind the list)
        HIP_TRY(create(f.done, hipEventCreateWithFlags, hipEventDisableTiming));
    }
    HIP_TRY(d->aux_ctr.alloc(1));
    HIP_TRY(hipMemset(d->aux_ctr.get(), 0, sizeof(DCounters)));
    HIP_TRY(d->aux_queue.alloc(1));
    HIP_TRY(d->aux_slow_list.alloc_bytes(size_t(d->slow_cap) * sizeof(long long) + spill_bytes));
    // paths left at which the finishing pass takes over: the pool form holds the wavefront kernels' pace further up (sweep on one eighth of
    // the headline frame, ms: 250 k 14.2, 500 k 13.3, 1 M 13.1, 2 M 13.0, 4 M 13.5, 8 M 14.8; whole frame 81.0 / 80.3 at 500 k / 2 M), the
    // one-lane-per-path form is flat from 2e5 to 1e6
    d->finish_threshold = K.finish_paths >= 0 ? K.finish_paths : path_bytes ? 1500000 : 500000;
    if (K.workspace_gb > 0) d->wf_budget_bytes = size_t(K.workspace_gb * double(size_t(1) << 30));
    return MCPT_OK;
}

// the kernels' view of the scene (DScene), the camera and the primary directions' buffer
static int create_dscene(mcpt_device* d, const Scene& s, double absmax)
{
    const Knobs& K = d->knobs;
    const mcpt_bvh_info& bi = d->bi;
    DScene& S = d->ds;
    S.nodes = d->nodes.get(); S.tris = d->tris.get(); S.shade = d->shade.get(); S.materials = d->materials.get(); S.lights = d->lights.get();
    S.light_tris = d->light_tris.get(); S.light_cdf = d->light_cdf.get(); S.texels = d->texels.get();
    S.t = bi.t; S.Lv = bi.Lv; S.Level = bi.Level; S.Nr = bi.Nr;
    S.num_lights = int32_t(s.lights.size()); S.num_materials = int32_t(s.materials.size());
    S.area0 = s.area0;
    S.fast.cw = d->cw_nodes.get(); S.fast.nodes = nullptr; S.fast.tris = d->fast_tris.get(); S.fast.pre = d->fast_pre.get(); S.fast.absmax = absmax;
    S.fast.enabled = d->fast_info.enabled;
    // Which shape of the trace engine walks it (wavefront.hip): by default the short-stack one at 4 waves per SIMD -- the hierarchy may
    // need up to kFastMaxDepth - 1 entries in the worst case, but a ray that would push past entry 27 is simply handed to the one-lane
    // walk (deep stack), and on every scene measured none does (10 M triangles: 0 of 1.5e8 rays).  MCPT_SHORT_KERNEL=0: the deep-stack
    // engine at 3 waves per SIMD.
    S.fast.stack_limit = K.short_kernel ? kFastShortStack : kFastMaxDepth;
    S.fast.stack_cap = S.fast.stack_limit;
    if (K.test_stack_cap >= 4 && K.test_stack_cap < S.fast.stack_cap) S.fast.stack_cap = K.test_stack_cap;
    // (any prefix of the node array may be mirrored; the host builder puts the top of the tree there)
    S.fast.cached = int32_t(std::min<size_t>(size_t(d->fast_info.n_nodes), size_t(kFastTopNodes)));
    if (K.node_cache >= 0 && K.node_cache < S.fast.cached) S.fast.cached = K.node_cache;
    const CameraFrame cf = camera_frame(s);
    put3(S.cam.eye, cf.eye); put3(S.cam.start_point, cf.start_point); put3(S.cam.pdx, cf.screen_pdx); put3(S.cam.pdy, cf.screen_pdy);
    S.cam.width = s.width; S.cam.height = s.height;
    d->width = s.width; d->height = s.height;
    HIP_TRY(d->dirs.alloc(size_t(s.width) * s.height * 3));
    return MCPT_OK;
}

int mcpt_device_create_ex(const mcpt_scene* h, int32_t ordinal, int32_t build_mode, mcpt_device** out)
{
    if (!h || !out) return fail(MCPT_ERR_ARG, "null argument");
    *out = nullptr;
    if (build_mode != MCPT_BUILD_HOST && build_mode != MCPT_BUILD_DEVICE && build_mode != MCPT_BUILD_DEVICE_FAST && build_mode != MCPT_BUILD_DEVICE_SAH)
        return fail(MCPT_ERR_ARG, "bad build mode");
    const Scene& s = h->s;
    if (build_mode == MCPT_BUILD_HOST && !s.accel_built) return fail(MCPT_ERR_ARG, "scene has no host build; use MCPT_BUILD_DEVICE");
    int ndev = mcpt_device_count();
    if (ndev <= 0) return fail(MCPT_ERR_NO_DEVICE, "no HIP device available (libmcpt has no CPU fallback)");
    if (const int gate = runtime_gate()) return gate;          // kernels of one hipcc on another release's runtime: refused
    if (ordinal < 0 || ordinal >= ndev) return fail(MCPT_ERR_NO_DEVICE, "device ordinal out of range");
    HIP_TRY(hipSetDevice(ordinal));
    std::unique_ptr<mcpt_device, void (*)(mcpt_device*)> d(new mcpt_device, mcpt_device_free);
    d->ordinal = ordinal;
    d->knobs = read_knobs();
    HIP_TRY(create(d->stream, hipStreamCreateWithFlags, hipStreamNonBlocking));
    for (auto& e : d->ev) HIP_TRY(create(e, hipEventCreate));
    HIP_TRY(create(d->look_stream, hipStreamCreateWithFlags, hipStreamNonBlocking));
    HIP_TRY(create(d->look_ev, hipEventCreateWithFlags, hipEventDisableTiming));
    HIP_TRY(d->h_look.alloc_bytes(64));

    const int t = int(s.faces.size());
    d->bi = bvh_shape(t);
    const CreateClock clock{d->knobs.print_diag && t >= (1 << 17), std::chrono::steady_clock::now()};
    std::vector<int32_t> order;                     // leaf -> .obj face
    double absmax = 0;                              // largest |coordinate| of the scene, as the hierarchy's builder found it
    int rc;
    if ((rc = create_reference(d.get(), s, build_mode, clock, order)) || (rc = create_materials_and_lights(d.get(), s)) ||
        (rc = create_hierarchy(d.get(), h, build_mode, order, clock, &absmax)) || (rc = create_pre_test(d.get(), absmax)))
        return rc;
    clock.lap("culling hierarchy in HBM");
    if ((rc = create_workspaces(d.get(), s)) || (rc = create_dscene(d.get(), s, absmax))) return rc;
    h->devices_created.fetch_add(1);
    h->refs.fetch_add(1);
    d->scene = h;
    *out = d.release();
    return MCPT_OK;
}

// what the device holds, read back (parity of the device build against the host build)
int mcpt_device_get_bvh_nodes(mcpt_device* d, double* box6, int32_t* leaf_face)
{
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    HIP_TRY(hipSetDevice(d->ordinal));
    const mcpt_bvh_info& bi = d->bi;
    if (box6) {
        std::vector<DNode> nodes(bi.Nr);
        HIP_TRY(hipMemcpy(nodes.data(), d->nodes.get(), size_t(bi.Nr) * sizeof(DNode), hipMemcpyDeviceToHost));
        for (int i = 0; i < bi.Nr; i++) {
            double* o = box6 + size_t(i) * 6;
            o[0] = nodes[i].mx[0]; o[1] = nodes[i].mx[1]; o[2] = nodes[i].mx[2]; o[3] = nodes[i].mn[0]; o[4] = nodes[i].mn[1]; o[5] = nodes[i].mn[2];
        }
    }
    if (leaf_face) {
        std::vector<int32_t> order(bi.t);
        HIP_TRY(hipMemcpy(order.data(), d->d_order.get(), size_t(bi.t) * sizeof(int32_t), hipMemcpyDeviceToHost));
        const int leaf0 = find_index(bi, (1 << bi.Level) - 1, bi.Level);
        for (int i = 0; i < bi.Nr; i++) leaf_face[i] = (i >= leaf0 && i < leaf0 + bi.t) ? order[i - leaf0] : -1;
    }
    return MCPT_OK;
}

int mcpt_device_get_leaf_order(mcpt_device* d, int32_t* leaf_to_face)
{
    if (!d || !leaf_to_face) return fail(MCPT_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(d->ordinal));
    HIP_TRY(hipMemcpy(leaf_to_face, d->d_order.get(), size_t(d->bi.t) * sizeof(int32_t), hipMemcpyDeviceToHost));
    return MCPT_OK;
}

int mcpt_device_fast_hierarchy(const mcpt_device* d, mcpt_fast_info* info, void* nodes, int32_t* tri_faces)
{
    static_assert(sizeof(CwNode) == 64, "mcpt.h documents 64-byte node records");
    if (!d || !info) return fail(MCPT_ERR_ARG, "null argument");
    *info = d->fast_info;
    if (!nodes && !tri_faces) return MCPT_OK;
    HIP_TRY(hipSetDevice(d->ordinal));
    const size_t n_nodes = size_t(d->fast_info.n_nodes), n_tris = size_t(d->fast_info.n_tris);
    if (nodes && n_nodes) HIP_TRY(hipMemcpy(nodes, d->cw_nodes.get(), n_nodes * sizeof(CwNode), hipMemcpyDeviceToHost));
    if (tri_faces && n_tris) {
        std::vector<DTri> tris(n_tris);
        HIP_TRY(hipMemcpy(tris.data(), d->fast_tris.get(), n_tris * sizeof(DTri), hipMemcpyDeviceToHost));
        for (size_t k = 0; k < tris.size(); k++) tri_faces[k] = tris[k].face;
    }
    return MCPT_OK;
}

int mcpt_device_set_trace_mode(mcpt_device* d, int32_t mode)
{
    if (!d || (mode != MCPT_TRACE_FAST && mode != MCPT_TRACE_REFERENCE)) return fail(MCPT_ERR_ARG, "bad trace mode");
    d->trace_mode = mode;
    return MCPT_OK;
}

static int ensure_dirs(mcpt_device* d, hipStream_t st)
{
    if (!d->dirs_ready) {
        launch_primary_dirs(d->ds.cam, d->dirs.get(), st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
        d->dirs_ready = true;
    }
    return MCPT_OK;
}

// ---- lenses (mcpt.h: camera lens)
static bool lens_active(const mcpt_lens& l) { return l.flags != 0 || l.aperture > 0.0; }
static int lens_check(const mcpt_lens* l)
{
    if (!l) return MCPT_OK;
    if (l->flags & ~(MCPT_LENS_JITTER | MCPT_LENS_PER_SAMPLE)) return fail(MCPT_ERR_ARG, "unknown lens flag");
    if (l->reserved != 0) return fail(MCPT_ERR_ARG, "mcpt_lens.reserved must be 0");
    if (!(std::isfinite(l->aperture) && l->aperture >= 0.0)) return fail(MCPT_ERR_ARG, "the aperture must be finite and >= 0");
    if (!std::isfinite(l->focus_distance)) return fail(MCPT_ERR_ARG, "the focus distance must be finite");
    return MCPT_OK;
}
static int ensure_pos(mcpt_device* d, hipStream_t st)
{
    if (!d->pos) {
        HIP_TRY(d->pos.alloc_bytes(std::max<size_t>(size_t(d->width) * d->height * 3 * sizeof(double), 8)));
        launch_primary_pos(d->ds.cam, d->pos.get(), st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
    }
    return MCPT_OK;
}
// what the kernels need of a lens: the device's camera frame (capi: create_dscene), x^ = screen_x_dir and y^ = the normalised up as
// camera_frame forms them, F / l
static DLens lens_for(const mcpt_device* d, const mcpt_lens& l)
{
    DLens c{};
    const Scene& s = d->scene->s;
    const Vec3 up = normalized(s.up), dir = s.look_at - s.eye;
    const Vec3 x = normalized(cross(dir, up));
    const double len = norm(dir);
    const double F = l.focus_distance > 0.0 ? l.focus_distance : len;
    c.pos = d->pos.get();
    for (int i = 0; i < 3; i++) { c.eye[i] = d->ds.cam.eye[i]; c.pdx[i] = d->ds.cam.pdx[i]; c.pdy[i] = d->ds.cam.pdy[i]; }
    c.xhat[0] = x.x; c.xhat[1] = x.y; c.xhat[2] = x.z;
    c.yhat[0] = up.x; c.yhat[1] = up.y; c.yhat[2] = up.z;
    c.aperture = l.aperture;
    c.focus_scale = F / len;
    c.flags = l.flags;
    return c;
}

static void counters_to_stats(const DCounters& c, mcpt_stats* s, bool print_diag)
{
    s->rays_primary = c.rays_primary; s->rays_shadow = c.rays_shadow; s->rays_bounce = c.rays_bounce;
    s->node_visits = c.node_visits; s->tri_tests = c.tri_tests; s->shade_calls = c.shade_calls; s->samples = c.samples;
    s->shadow_skipped = c.shadow_skipped;
    s->dom_rays = c.trace_rays; s->dom_node_visits = c.trace_nodes; s->dom_tri_tests = c.trace_tris;
    if (print_diag) {
        const double tot = double(c.pad[8] + c.pad[9] + c.pad[10] + c.pad[11]);
        const double iters = double(c.pad[0] + c.pad[2] + c.pad[4]);
        auto per = [](unsigned long long a, unsigned long long b) { return b ? double(a) / double(b) : 0.0; };
        std::fprintf(stderr, "trace diag: inner iters %llu lanes %.1f/64 | pre-test iters %llu lanes %.1f/64 | exact iters %llu lanes %.1f/64 | idle lanes/iter %.1f | "
                             "wave time: refill %.1f%% inner %.1f%% pre-test %.1f%% exact %.1f%% | cycles per iter: inner %.0f pre-test %.0f exact %.0f\n",
                     c.pad[0], per(c.pad[1], c.pad[0]), c.pad[2], per(c.pad[3], c.pad[2]), c.pad[4], per(c.pad[5], c.pad[4]), iters ? double(c.pad[6]) / iters : 0.0,
                     tot ? 100.0 * c.pad[8] / tot : 0.0, tot ? 100.0 * c.pad[9] / tot : 0.0, tot ? 100.0 * c.pad[10] / tot : 0.0, tot ? 100.0 * c.pad[11] / tot : 0.0,
                     per(c.pad[9], c.pad[0]), per(c.pad[10], c.pad[2]), per(c.pad[11], c.pad[4]));
        std::fprintf(stderr, "k_wf_trace: %llu rays, %.3f nodes, %.3f triangles visited, %.3f exact tests per ray (%.1f %% of the visited triangles survive the pre-test)\n",
                     c.trace_rays, per(c.trace_nodes, c.trace_rays), per(c.trace_tris, c.trace_rays), per(c.trace_exact, c.trace_rays), 100.0 * per(c.trace_exact, c.trace_tris));
        std::fprintf(stderr, "rays deferred to the exact walk by k_wf_trace: %llu of %llu\n", c.pad[12], c.trace_rays);
#ifdef MCPT_POOL_DEBUG
        if (c.pp[19]) {
            static const char* nm[5] = {"node", "leaf", "exact", "result", "shade"};
            const double life = double(c.pp[18]);
            for (int i = 0; i < 5; i++)
                std::fprintf(stderr, "pool %-6s: %10llu steps, %5.1f lanes per step, %7.0f cycles per step, %5.1f %% of wave time\n", nm[i], c.pp[i],
                             c.pp[i] ? double(c.pp[5 + i]) / c.pp[i] : 0.0, c.pp[i] ? double(c.pp[12 + i]) / c.pp[i] : 0.0, life ? 100.0 * c.pp[12 + i] / life : 0.0);
            std::fprintf(stderr, "pool: %llu waves, %.0f cycles per wave, vote + claim + sleep %.1f %% of wave time, %llu sleeps, %llu steps that claimed nothing\n", c.pp[19],
                         life / c.pp[19], life ? 100.0 * c.pp[17] / life : 0.0, c.pp[10], c.pp[11]);
        }
        for (int i = 0; i < 4; i++) std::fprintf(stderr, "pool class %d: %llu steps, %.1f lanes per step (%.1f could before the claim)\n", i, c.dbg[8 + i], c.dbg[8 + i] ? double(c.dbg[12 + i]) / c.dbg[8 + i] : 0.0, c.dbg[8 + i] ? double(c.dbg[16 + i]) / c.dbg[8 + i] : 0.0);
        std::fprintf(stderr, "pool: %llu sleeps, %llu steps that claimed nothing\n", c.dbg[20], c.dbg[21]);
        std::fprintf(stderr, "pool debug: %llu launches, %llu slots in all, %llu consumed in %llu refill steps, %llu rays among them, %llu started, %llu slots retired, %llu tickets\n", c.dbg[5], c.dbg[4], c.dbg[0], c.dbg[2], c.dbg[1], c.dbg[7], c.dbg[3], c.dbg[6]);
#endif
        if (c.pad[20]) {
            std::fprintf(stderr, "PRE-TEST SELF-CHECK: %llu rejected triangles are candidates by the exact test\n", c.pad[20]);
            double g[24]; std::memcpy(g, c.dbg, sizeof g);
            std::fprintf(stderr, "  first: margins beta %.6g gamma %.6g alpha %.6g behind %.6g beyond %.6g clear %.6g | t32 %.9g |det| %.6g | t_k %.17g leader %.17g limit_f %.9g margin %.6g eta4 %.6g slot %.0f of %.0f\n"
                                 "  ray o %.17g %.17g %.17g d %.17g %.17g %.17g\n",
                         g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], g[9], g[10], g[11], g[12], g[13], g[14], g[15], g[16], g[17], g[18], g[19], g[20], g[21]);
        }
#ifdef MCPT_PRE_CHECK
        std::fprintf(stderr, "KERNARG CHECK: %llu of %llu trace launches read another WfArgs through the kernarg segment\n", c.pad[21], c.pad[22]);
#endif
        if (c.pad[13]) std::fprintf(stderr, "finish diag: longest wave %llu steps, %.0f us alive, %.0f us of it in the ray walks (100 MHz ticks; maxima over waves and launches)\n",
                                    c.pad[13], double(c.pad[14]) / 100.0, double(c.pad[15]) / 100.0);
        const double lt = double(c.pad[16] + c.pad[17] + c.pad[18]);
        std::fprintf(stderr, "logic diag: resolve %.1f%% compaction %.1f%% shade %.1f%% | cycles per wave: %.0f / %.0f / %.0f (waves %llu)\n",
                     lt ? 100.0 * c.pad[16] / lt : 0.0, lt ? 100.0 * c.pad[17] / lt : 0.0, lt ? 100.0 * c.pad[18] / lt : 0.0,
                     c.pad[19] ? double(c.pad[16]) / c.pad[19] : 0.0, c.pad[19] ? double(c.pad[17]) / c.pad[19] : 0.0, c.pad[19] ? double(c.pad[18]) / c.pad[19] : 0.0, c.pad[19]);
    }
}

// ------------------------------------------------------------------------------------------------ closest hit
int mcpt_trace_closest_device(mcpt_device* d, const double* d_rays, int64_t n, int32_t* d_face, double* d_t, double* d_p,
                              double* d_pn, void* stream)
{
    if (!d || (n > 0 && !d_rays) || n < 0) return fail(MCPT_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(d->ordinal));
    if (!d_face || !d_t || !d_p) return fail(MCPT_ERR_ARG, "d_face, d_t and d_p are required by the device form");
    launch_trace_closest(d->ds, d->trace_mode == MCPT_TRACE_FAST, d_rays, n, d_face, d_t, d_p, d_pn, d->aux_ctr.get(), d->aux_queue.get(), d->aux_slow_list.get(), d->slow_cap,
                         static_cast<hipStream_t>(stream), d->cfg);
    HIP_TRY(hipGetLastError());
    return MCPT_OK;
}

int mcpt_trace_closest(mcpt_device* d, const double* rays, int64_t n, int32_t* face, double* t, double* p, double* pn, mcpt_stats* stats)
{
    if (!d || (n > 0 && !rays) || n < 0) return fail(MCPT_ERR_ARG, "bad argument");
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n == 0) return MCPT_OK;
    HIP_TRY(hipSetDevice(d->ordinal));
    DevBuf<double> d_rays, d_t, d_p, d_pn;
    DevBuf<int32_t> d_face;
    HIP_TRY(d_rays.alloc(size_t(n) * 6));
    HIP_TRY(d_face.alloc(size_t(n)));
    HIP_TRY(d_t.alloc(size_t(n)));
    HIP_TRY(d_p.alloc(size_t(n) * 3));
    HIP_TRY(d_pn.alloc(size_t(n) * 3));
    hipStream_t st = d->stream.get();
    // host buffers are pageable: blocking copies (the runtime stages them), ordered around the kernels by stream synchronisation
    HIP_TRY(hipMemcpy(d_rays.get(), rays, size_t(n) * 6 * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(d->aux_ctr.get(), 0, sizeof(DCounters), st));
    HIP_TRY(hipEventRecord(d->ev[0].get(), st));
    launch_trace_closest(d->ds, d->trace_mode == MCPT_TRACE_FAST, d_rays.get(), n, d_face.get(), d_t.get(), d_p.get(), d_pn.get(), d->aux_ctr.get(),
                         d->aux_queue.get(), d->aux_slow_list.get(), d->slow_cap, st, d->cfg);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(d->ev[1].get(), st));
    HIP_TRY(hipStreamSynchronize(st));
    if (face) HIP_TRY(hipMemcpy(face, d_face.get(), size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (t) HIP_TRY(hipMemcpy(t, d_t.get(), size_t(n) * sizeof(double), hipMemcpyDeviceToHost));
    if (p) HIP_TRY(hipMemcpy(p, d_p.get(), size_t(n) * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (pn) HIP_TRY(hipMemcpy(pn, d_pn.get(), size_t(n) * 3 * sizeof(double), hipMemcpyDeviceToHost));
    DCounters c{};
    HIP_TRY(hipMemcpy(&c, d->aux_ctr.get(), sizeof c, hipMemcpyDeviceToHost));
    if (stats) {
        counters_to_stats(c, stats, d->knobs.print_diag != 0);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, d->ev[0].get(), d->ev[1].get());
        stats->ms_trace = ms; stats->ms_total = ms; stats->launches = 1;
    }
    return MCPT_OK;
}

// ------------------------------------------------------------------------------------------------ integrator
static int prepare_partition(mcpt_device* d, const mcpt_render_params* p, hipStream_t st)
{
    int tw, th, rank, world;
    tile_shape(p, tw, th, rank, world);
    if (rank < 0 || rank >= world) return fail(MCPT_ERR_ARG, "rank outside world");
    const int key[4] = {tw, th, rank, world};
    if (std::memcmp(key, d->part_key, sizeof key) == 0 && d->pixels) return MCPT_OK;
    std::vector<int32_t> v;
    owned_pixel_list(d->width, d->height, tw, th, rank, world, v);
    if (d->pixels) HIP_TRY(hipDeviceSynchronize());       // a frame of the previous partition may still be in flight (MCPT_RENDER_KEEP_STATS / PIPELINE)
    HIP_TRY(d->pixels.upload(v));                          // (blocking copy: v is pageable)
    d->n_pixels = int64_t(v.size());
    std::memcpy(d->part_key, key, sizeof key);
    return MCPT_OK;
}

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
};

// The pixels a render call covers, on the device: the partition's owned list (mcpt_render*, uniform progressive passes) or an adaptive
// frame's active list.  Slot s of the call renders pixel pixels[s].
struct PixelList {
    const int32_t* pixels;
    int64_t n;
};

static void fold_range(mcpt_device::FrameSlot& f, const SampleRange& r, const PixelList& L, int first, int n_slots, double* d_img, bool lensed, hipStream_t st)
{
    if (lensed) launch_fold_lens(f.rad.get(), f.cam_hit.get(), L.pixels, first, n_slots, r.n, r.k0, r.N, d_img, r.mom, r.hit, r.hitcnt, st);
    else if (r.mom) launch_fold_progressive(f.rad.get(), L.pixels, f.hits.get(), first, n_slots, r.n, r.k0, r.N, d_img, r.mom, r.hit, st);
    else launch_fold_samples(f.rad.get(), L.pixels, f.hits.get(), first, n_slots, r.n, d_img, st);
}

// megakernel path: one lane per camera sample, the whole path in one kernel (kept for A/B runs and as a second
// implementation the wavefront path is checked against)
static int render_megakernel(mcpt_device* d, mcpt_device::FrameSlot& f, const SampleRange& r, const PixelList& L, const mcpt_render_params* p,
                             double* d_img, bool timed, const DLens* lens, hipStream_t st, double& ms_trace, int& launches)
{
    const int64_t npx = L.n;
    const int spp = r.n;
    const size_t per_pixel = size_t(spp) * 3 * sizeof(double) + (lens ? size_t(spp) : 0);   // (+ the hit flag of every sample under a lens)
    int64_t chunk = int64_t(std::max<size_t>(d->sample_budget_bytes / per_pixel, 64));
    chunk = std::min<int64_t>(chunk, npx);
    HIP_TRY(f.rad.grow_bytes(size_t(chunk) * per_pixel));
    if (lens) HIP_TRY(f.cam_hit.grow(size_t(chunk * spp)));
    for (int64_t first = 0; first < npx; first += chunk) {
        const int n_slots = int(std::min<int64_t>(chunk, npx - first));
        if (timed) HIP_TRY(hipEventRecord(d->ev[2].get(), st));
        if (lens) launch_shade_samples_lens(d->ds, *lens, p->seed, L.pixels, int(first), n_slots, spp, r.k0, f.rad.get(), f.cam_hit.get(), f.ctr.get(), st);
        else launch_shade_samples(d->ds, p->seed, d->dirs.get(), L.pixels, f.hits.get(), int(first), n_slots, spp, r.k0, f.rad.get(), f.ctr.get(), st);
        HIP_TRY(hipGetLastError());
        if (timed) {
            HIP_TRY(hipEventRecord(d->ev[3].get(), st));
            HIP_TRY(hipEventSynchronize(d->ev[3].get()));
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, d->ev[2].get(), d->ev[3].get()));
            ms_trace += ms;
        }
        launches++;
        fold_range(f, r, L, int(first), n_slots, d_img, lens != nullptr, st);
        HIP_TRY(hipGetLastError());
    }
    return MCPT_OK;
}

// wavefront path (wavefront.hpp): per chunk, lockstep iterations of logic + trace over compacted path state in HBM.
// timed: event pairs around the trace launches, summed here (one stream synchronisation at the end); keep: the pairs are recorded
// and left in d->ev_pool for mcpt_device_collect_stats -- the frame ends without the host waiting for it.
// lens (non-null: an active lens): the per-sample route -- per chunk a camera pass (the camera as vertex -1 of every sample) and a trace
// launch of its rays, then the logic passes from depth 0 on, every vertex in the path state (WfArgs::hits == null)
static int render_wavefront(mcpt_device* d, mcpt_device::FrameSlot& f, const SampleRange& r, const PixelList& L, const mcpt_render_params* p,
                            double* d_img, bool timed, bool keep, const DLens* lens, hipStream_t st, double& ms_trace, int& launches)
{
    const int64_t npx = L.n;
    const int spp = r.n;
    const int nl = d->ds.num_lights;
    const bool fast = d->trace_mode == MCPT_TRACE_FAST;
    const size_t bpp = wf_bytes_per_path(nl);
    // chunk: as many pixels as the workspace budget holds paths for (every pixel may hit)
    const size_t overhead = 64 * 1024;
    // Fewer, larger chunks are cheaper (every chunk ends in a tail of small launches): by default a frame slot may use half of
    // the HBM that is free (a third when two frames are pipelined), which holds a whole 1280x720 SPP-256 frame (83 GB) on a
    // 288-GB device.
    size_t budget = d->wf_budget_bytes;
    if (!budget) {
        if (!d->wf_auto_budget) {
            size_t free_b = 0, total_b = 0;
            HIP_TRY(hipMemGetInfo(&free_b, &total_b));
            size_t mine = 0;
            for (const auto& q : d->slot) mine += q.wf_ws.bytes() + q.rad.bytes();
            d->wf_auto_budget = std::max<size_t>((free_b + mine) / (d->pipelined ? 3 : 2), size_t(1) << 30);
        }
        budget = d->wf_auto_budget;
    }
    int64_t cap = int64_t((budget - overhead) / (bpp + 24 + (lens ? 1 : 0)));      // + 24 B radiance per sample (+ its hit flag under a lens)
    cap = std::min<int64_t>(cap, npx * int64_t(spp));
    cap = std::min<int64_t>(cap, (int64_t(1) << 31) - 4096);                 // 32-bit compaction counter / sample ids
    int64_t chunk_slots = std::max<int64_t>(cap / spp, 1);
    chunk_slots = std::min<int64_t>(chunk_slots, npx);
    cap = chunk_slots * spp;
    const size_t ws_need = size_t(cap) * bpp + overhead;
    HIP_TRY(f.wf_ws.grow_bytes(ws_need));
    HIP_TRY(f.rad.grow_bytes(size_t(cap) * 3 * sizeof(double)));
    if (lens) {
        HIP_TRY(f.cam_hit.grow(size_t(cap)));
    } else {
        HIP_TRY(f.hit_slots.grow(size_t(chunk_slots)));
        HIP_TRY(f.surf.grow(size_t(chunk_slots)));
        HIP_TRY(f.alive_base.grow(size_t(chunk_slots / 64 + 2)));
    }
    int rc = MCPT_OK;
    WfArgs a{};
    WfState A, B;
    if (!wf_carve(f.wf_ws.get(), f.wf_ws.bytes(), cap, nl, A, B, a.rays)) return fail(MCPT_ERR_NOMEM, "wavefront workspace too small");
    a.cap = cap; a.nl = nl; a.spp = spp; a.sample_base = r.k0; a.seed = p->seed; a.pixels = L.pixels; a.hit_slots = f.hit_slots.get(); a.surf = f.surf.get(); a.alive_base = f.alive_base.get();
    a.hits = f.hits.get(); a.dirs = d->dirs.get(); a.rad = f.rad.get(); a.counts = f.wf_counts.get(); a.ctr = f.ctr.get(); a.tris = d->tris.get();
    a.materials = d->materials.get(); a.queue = fast ? f.queue.get() : nullptr;
    a.finish_below = fast ? unsigned(std::min<long long>(std::max<long long>(d->finish_threshold, 0), 1ll << 30)) : 0u;
    if (lens) { a.hits = nullptr; a.cam_hit = f.cam_hit.get(); }
    // Iterations are enqueued without waiting for their counts: every kernel reads its input count from the device slot the
    // previous one wrote.  The host looks at a count only every few iterations (to stop, and to size the next grids).
    const size_t ev_first = d->ev_used;
    const int kSyncEvery = 4;
    for (int64_t first = 0; first < npx; first += chunk_slots) {
        const int n_slots = int(std::min<int64_t>(chunk_slots, npx - first));
        HIP_TRY(hipMemsetAsync(f.wf_counts.get(), 0, sizeof(WfCounts) * MCPT_WF_COUNT_SLOTS, st));
        long long n_upper = (long long)n_slots * spp;        // upper bound of the live paths, refined at every look
        double n_grid = double(n_upper);                     // grid-sizing estimate between looks (kernels stride, any grid is correct)
        a.first_slot = int(first);
        a.in = A; a.out = B;
        a.counts_in = &f.wf_counts[0];
        if (lens) {
            // the camera as vertex -1: its state into a.out, the count into slot 0, its rays traced as a bounce (depth -1: from a.out.p)
            WfArgs ac = a;
            ac.depth = -1; ac.counts = &f.wf_counts[0]; ac.count_mul = 1u; ac.finish_below = 0u;
            launch_camera_pass(*lens, ac, n_upper, st);
            HIP_TRY(hipGetLastError());
            ac.nl = 0;          // the trace launch sees the bounce slot only (l == nl): no empty shadow-ray slots to walk past
            EventPair* pr = nullptr;
            if (timed || keep) { if ((rc = next_pair(d->ev_pool, d->ev_used, pr))) return rc; HIP_TRY(hipEventRecord(pr->first.get(), st)); }
            launch_wf_trace(d->ds, ac, n_upper, fast, f.queue.get(), f.slow_list.get(), d->slow_cap, st, d->cfg);
            HIP_TRY(hipGetLastError());
            if (timed || keep) HIP_TRY(hipEventRecord(pr->second.get(), st));
            launches++;
            std::swap(a.in, a.out);
        } else {
            launch_hit_slots(f.hits.get(), int(first), n_slots, f.hit_slots.get(), &f.wf_counts[0].n_next, st);
            HIP_TRY(hipGetLastError());
            launch_primary_surface(d->ds, a, f.surf.get(), f.alive_base.get(), &f.wf_counts[0].pad[2], n_slots, st);      // what the samples of a pixel share at their first vertex
            HIP_TRY(hipGetLastError());
        }
        for (int depth = 0; depth < MCPT_MAX_DEPTH && n_upper > 0; depth++) {
            a.depth = depth;
            a.counts_in = &f.wf_counts[depth]; a.count_mul = depth == 0 && !lens ? unsigned(spp) : 1u;
            a.counts = &f.wf_counts[depth + 1];
            const long long n_launch = std::max<long long>(1, (long long)n_grid);
            // the per-sample route's depth 0 resolves the camera rays: nothing went to the finishing kernel before it, and its pool form
            // (which reads a pixel's PrimaryHit at depth 0) does not adopt its paths
            const bool cam0 = lens && depth == 0;
            char* const area = cam0 ? nullptr : f.path_area.get();
            if (cam0) { WfArgs al = a; al.finish_below = 0u; launch_wf_logic(d->ds, al, n_launch, false, st, d->cfg); }
            else launch_wf_logic(d->ds, a, n_launch, depth == 0, st, d->cfg);
            HIP_TRY(hipGetLastError());
            // The host looks at this pass's count every few iterations, and at every iteration once the hand-over to the finishing
            // kernel is near.  The look waits for this logic pass only (event + side stream): when it finds the hand-over, the
            // finishing kernel is launched and the call returns while it runs -- the next frame's head can overlap it.
            const bool look = (depth + 1) % kSyncEvery == 0 || (a.finish_below && n_grid * 0.6 <= 6.0 * double(a.finish_below));
            if (look) {
                HIP_TRY(hipEventRecord(d->look_ev.get(), st));
                HIP_TRY(hipStreamWaitEvent(d->look_stream.get(), d->look_ev.get(), 0));
                HIP_TRY(hipMemcpyAsync(d->h_look.get(), &f.wf_counts[depth + 1].n_next, sizeof(unsigned int), hipMemcpyDeviceToHost, d->look_stream.get()));
                HIP_TRY(hipStreamSynchronize(d->look_stream.get()));
                const unsigned int n_now = d->h_look[0];
                if (n_now <= a.finish_below) {
                    if (n_now > 0) { launch_wf_finish(d->ds, a, (long long)n_now, st, d->cfg, area, f.slow_list.get(), d->slow_cap); HIP_TRY(hipGetLastError()); }
                    n_upper = 0;
                    break;
                }
                n_upper = n_now;
                n_grid = double(n_now);
            } else if (a.finish_below) {
                // few paths left (decided on the device from this pass's count): one lane per path runs them to the end
                launch_wf_finish(d->ds, a, std::min<long long>(n_launch, (long long)a.finish_below), st, d->cfg, area, f.slow_list.get(), d->slow_cap);
                HIP_TRY(hipGetLastError());
            }
            const long long n_trace = look ? (long long)n_grid : n_launch;
            EventPair* pr = nullptr;
            if (timed || keep) { if ((rc = next_pair(d->ev_pool, d->ev_used, pr))) return rc; HIP_TRY(hipEventRecord(pr->first.get(), st)); }
            launch_wf_trace(d->ds, a, n_trace, fast, f.queue.get(), f.slow_list.get(), d->slow_cap, st, d->cfg);
            HIP_TRY(hipGetLastError());
            if (timed || keep) HIP_TRY(hipEventRecord(pr->second.get(), st));
            launches++;
            std::swap(a.in, a.out);
            if (!look) n_grid *= 0.75;   // paths die at >= 40 % per bounce (Russian roulette 0.6)
        }
        // paths still alive at the depth cap cannot exist: logic(MAX_DEPTH-1) emits no bounce ray; a last logic pass resolves them
        if (n_upper > 0) {
            a.depth = MCPT_MAX_DEPTH;
            a.counts_in = &f.wf_counts[MCPT_MAX_DEPTH]; a.count_mul = 1u; a.counts = &f.wf_counts[MCPT_MAX_DEPTH + 1];
            launch_wf_logic(d->ds, a, n_upper, false, st, d->cfg);
            HIP_TRY(hipGetLastError());
        }
        fold_range(f, r, L, int(first), n_slots, d_img, lens != nullptr, st);
        HIP_TRY(hipGetLastError());
    }
    if (timed && !keep) {
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t i = ev_first; i < d->ev_used; i++) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, d->ev_pool[i].first.get(), d->ev_pool[i].second.get()));
            ms_trace += ms;
        }
        d->ev_used = ev_first;
    }
    return MCPT_OK;
}

static int render_device_impl(mcpt_device* d, const SampleRange& r, const PixelList& L, const mcpt_render_params* p, double* d_img, mcpt_stats* stats,
                              hipStream_t st, int& slot_used);

int mcpt_render_device(mcpt_device* d, const mcpt_render_params* p, double* d_img, mcpt_stats* stats, void* stream)
{
    if (!d || !p || !d_img || p->spp <= 0) return fail(MCPT_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(d->ordinal));
    if (stats) std::memset(stats, 0, sizeof *stats);
    // a frame that fails half-way must not leave half-recorded event pairs behind: mcpt_device_collect_stats would trip over them
    const size_t ev_used0 = d->ev_used, frame_ev_used0 = d->frame_ev_used;
    int slot_used = -1;
    const SampleRange whole{0, p->spp, p->spp, nullptr, nullptr, &d->lens, nullptr};
    int rc = prepare_partition(d, p, static_cast<hipStream_t>(stream));
    if (rc == MCPT_OK) rc = render_device_impl(d, whole, PixelList{d->pixels.get(), d->n_pixels}, p, d_img, stats, static_cast<hipStream_t>(stream), slot_used);
    if (rc != MCPT_OK) {
        d->ev_used = ev_used0; d->frame_ev_used = frame_ev_used0;
        if (slot_used >= 0) d->slot[slot_used].keeping = false;      // its counters hold part of a frame: cleared by the next one
    }
    return rc;
}

static int render_device_impl(mcpt_device* d, const SampleRange& r, const PixelList& L, const mcpt_render_params* p, double* d_img, mcpt_stats* stats,
                              hipStream_t st, int& slot_used)
{
    const bool keep = (p->flags & MCPT_RENDER_KEEP_STATS) != 0 && !(p->flags & MCPT_RENDER_MEGAKERNEL);
    const bool timed = stats != nullptr && !keep;
    // frame slot: consecutive pipelined frames alternate; a slot's previous frame (possibly on another stream) must be over
    if ((p->flags & MCPT_RENDER_PIPELINE) && !d->pipelined) {
        HIP_TRY(hipDeviceSynchronize());
        d->pipelined = true; d->wf_auto_budget = 0;                  // the budget now has to hold two frames
        for (auto& q : d->slot) q.wf_ws.reset();
    }
    const int si = (p->flags & MCPT_RENDER_PIPELINE) ? (d->next_slot ^= 1) : 0;
    slot_used = si;
    mcpt_device::FrameSlot& f = d->slot[si];
    if (f.used) HIP_TRY(hipStreamWaitEvent(st, f.done.get(), 0));
    int rc = ensure_dirs(d, st);
    if (rc) return rc;
    const bool lensed = r.lens && lens_active(*r.lens);
    if (lensed && (rc = ensure_pos(d, st))) return rc;
    const DLens dl = lensed ? lens_for(d, *r.lens) : DLens{};
    const int64_t npx = L.n;
    if (npx == 0) return MCPT_OK;
    const uint64_t primary_rays = uint64_t(npx) * (lensed ? uint64_t(r.n) : 1u);
    HIP_TRY(f.hits.grow(size_t(npx)));
    if (!keep || !f.keeping) HIP_TRY(hipMemsetAsync(f.ctr.get(), 0, sizeof(DCounters), st));    // kept statistics accumulate until they are collected
    f.keeping = keep;
    EventPair* fe = nullptr;
    if (keep) {
        if ((rc = next_pair(d->frame_ev, d->frame_ev_used, fe))) return rc;
        HIP_TRY(hipEventRecord(fe->first.get(), st));
    } else HIP_TRY(hipEventRecord(d->ev[0].get(), st));
    if (!lensed) {          // (a lens traces its camera rays per sample, in the render path)
        launch_primary_hits(d->ds, d->trace_mode == MCPT_TRACE_FAST, d->dirs.get(), L.pixels, int(npx), f.hits.get(), f.ctr.get(), f.queue.get(), f.slow_list.get(), d->slow_cap, st, d->cfg);
        HIP_TRY(hipGetLastError());
    }
    double ms_trace = 0;
    int launches = 0;
    if (p->flags & MCPT_RENDER_MEGAKERNEL) rc = render_megakernel(d, f, r, L, p, d_img, timed, lensed ? &dl : nullptr, st, ms_trace, launches);
    else rc = render_wavefront(d, f, r, L, p, d_img, timed, keep, lensed ? &dl : nullptr, st, ms_trace, launches);
    if (rc) return rc;
    if (keep) {
        HIP_TRY(hipEventRecord(fe->second.get(), st));
        d->kept_samples += uint64_t(npx) * uint64_t(r.n); d->kept_primary += primary_rays; d->kept_launches += launches;
    } else HIP_TRY(hipEventRecord(d->ev[1].get(), st));
    HIP_TRY(hipEventRecord(f.done.get(), st));
    f.used = true;
    if (timed) {
        DCounters c{};
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipMemcpy(&c, f.ctr.get(), sizeof c, hipMemcpyDeviceToHost));
        counters_to_stats(c, stats, d->knobs.print_diag != 0);
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, d->ev[0].get(), d->ev[1].get()));
        stats->ms_total = ms; stats->ms_trace = ms_trace; stats->launches = launches;
        stats->samples = uint64_t(npx) * uint64_t(r.n);         // camera samples covered (a primary miss is a finished sample)
        stats->rays_primary = primary_rays;
    }
    return MCPT_OK;
}

// Statistics of every MCPT_RENDER_KEEP_STATS frame since the last call: waits for those frames, sums the device counters of both
// frame slots, the event pairs around every k_wf_trace launch (ms_trace) and around every frame (ms_total = sum of frame times;
// pipelined frames overlap, so this can exceed the wall time), then starts over.
int mcpt_device_collect_stats(mcpt_device* d, mcpt_stats* stats)
{
    if (!d || !stats) return fail(MCPT_ERR_ARG, "null argument");
    std::memset(stats, 0, sizeof *stats);
    HIP_TRY(hipSetDevice(d->ordinal));
    HIP_TRY(hipDeviceSynchronize());
    DCounters sum{};
    for (auto& f : d->slot) {
        DCounters c{};
        HIP_TRY(hipMemcpy(&c, f.ctr.get(), sizeof c, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemset(f.ctr.get(), 0, sizeof(DCounters)));
        unsigned long long* a = reinterpret_cast<unsigned long long*>(&sum);
        const unsigned long long* b = reinterpret_cast<const unsigned long long*>(&c);
        for (size_t i = 0; i < sizeof(DCounters) / sizeof(unsigned long long); i++) a[i] += b[i];
        sum.max_depth = std::max(sum.max_depth - c.max_depth, c.max_depth);      // a maximum, not a sum
    }
    counters_to_stats(sum, stats, d->knobs.print_diag != 0);
    // the bookkeeping starts over whatever the queries say: a pair that cannot be read is left out and reported
    hipError_t bad = hipSuccess;
    for (size_t i = 0; i < d->ev_used; i++) {
        float ms = 0;
        const hipError_t e = hipEventElapsedTime(&ms, d->ev_pool[i].first.get(), d->ev_pool[i].second.get());
        if (e == hipSuccess) stats->ms_trace += ms; else bad = e;
    }
    for (size_t i = 0; i < d->frame_ev_used; i++) {
        float ms = 0;
        const hipError_t e = hipEventElapsedTime(&ms, d->frame_ev[i].first.get(), d->frame_ev[i].second.get());
        if (e == hipSuccess) stats->ms_total += ms; else bad = e;
    }
    stats->launches = d->kept_launches; stats->samples = d->kept_samples; stats->rays_primary = d->kept_primary;
    d->ev_used = 0; d->frame_ev_used = 0; d->kept_launches = 0; d->kept_samples = 0; d->kept_primary = 0;
    for (auto& f : d->slot) f.keeping = false;
    if (bad != hipSuccess) { (void)hipGetLastError(); return fail(MCPT_ERR_HIP, std::string("an event pair of a kept frame could not be read: ") + hipGetErrorString(bad)); }
    return MCPT_OK;
}

int mcpt_render(mcpt_device* d, const mcpt_render_params* p, double* img, mcpt_stats* stats)
{
    if (!d || !p || !img) return fail(MCPT_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(d->ordinal));
    const size_t bytes = size_t(d->width) * d->height * 3 * sizeof(double);
    DevBuf<double> d_img;
    HIP_TRY(d_img.alloc_bytes(bytes));
    // The caller's frame is pageable host memory: blocking copies on either side of the frame, which itself is ordered on d->stream.
    hipError_t e = hipMemcpy(d_img.get(), img, bytes, hipMemcpyHostToDevice);   // untouched pixels keep the caller's values
    int rc = e == hipSuccess ? mcpt_render_device(d, p, d_img.get(), stats, d->stream.get()) : fail(MCPT_ERR_HIP, hipGetErrorString(e));
    // also on failure: nothing of this frame may still be running when d_img goes
    e = hipStreamSynchronize(d->stream.get());
    if (rc == MCPT_OK && e == hipSuccess) e = hipMemcpy(img, d_img.get(), bytes, hipMemcpyDeviceToHost);
    if (rc == MCPT_OK && e != hipSuccess) rc = fail(MCPT_ERR_HIP, hipGetErrorString(e));
    return rc;
}

int mcpt_sample_radiance(mcpt_device* d, uint64_t seed, const int32_t* pix, const int32_t* k, int64_t n, double* rgb)
{
    if (!d || !pix || !k || !rgb || n < 0) return fail(MCPT_ERR_ARG, "bad argument");
    if (n == 0) return MCPT_OK;
    for (int64_t i = 0; i < n; i++)
        if (pix[i] < 0 || pix[i] >= d->width * d->height) return fail(MCPT_ERR_ARG, "pixel index out of range");
    HIP_TRY(hipSetDevice(d->ordinal));
    int rc = ensure_dirs(d, d->stream.get());
    if (rc) return rc;
    hipStream_t st = d->stream.get();
    DevBuf<int32_t> d_pix, d_k;
    DevBuf<double> d_rgb;
    hipError_t e = d_pix.alloc(size_t(n));
    if (e == hipSuccess) e = d_k.alloc(size_t(n));
    if (e == hipSuccess) e = d_rgb.alloc(size_t(n) * 3);
    if (e == hipSuccess) e = hipMemcpy(d_pix.get(), pix, size_t(n) * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_k.get(), k, size_t(n) * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        if (lens_active(d->lens)) {
            if ((rc = ensure_pos(d, st))) return rc;
            launch_sample_radiance_lens(d->ds, lens_for(d, d->lens), seed, d_pix.get(), d_k.get(), n, d_rgb.get(), d->aux_ctr.get(), st);
        } else launch_sample_radiance(d->ds, seed, d->dirs.get(), d_pix.get(), d_k.get(), n, d_rgb.get(), d->aux_ctr.get(), st);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpy(rgb, d_rgb.get(), size_t(n) * 24, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(MCPT_ERR_HIP, hipGetErrorString(e));
    return MCPT_OK;
}

int mcpt_device_set_lens(mcpt_device* d, const mcpt_lens* l)
{
    if (int rc = lens_check(l)) return rc;
    if (mcpt_device_count() <= 0) return fail(MCPT_ERR_NO_DEVICE, "no HIP device available (libmcpt has no CPU fallback)");
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    d->lens = l ? *l : mcpt_lens{};
    return MCPT_OK;
}

int mcpt_device_get_lens(const mcpt_device* d, mcpt_lens* out)
{
    if (!out) return fail(MCPT_ERR_ARG, "null argument");
    if (mcpt_device_count() <= 0) return fail(MCPT_ERR_NO_DEVICE, "no HIP device available (libmcpt has no CPU fallback)");
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    *out = d->lens;
    return MCPT_OK;
}

int mcpt_camera_rays(mcpt_device* d, uint64_t seed, const int32_t* pix, const int32_t* k, int64_t n, double* rays6)
{
    if (!pix || !k || !rays6 || n < 0) return fail(MCPT_ERR_ARG, "bad argument");
    if (mcpt_device_count() <= 0) return fail(MCPT_ERR_NO_DEVICE, "no HIP device available (libmcpt has no CPU fallback)");
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    if (n == 0) return MCPT_OK;
    for (int64_t i = 0; i < n; i++)
        if (pix[i] < 0 || pix[i] >= d->width * d->height) return fail(MCPT_ERR_ARG, "pixel index out of range");
    HIP_TRY(hipSetDevice(d->ordinal));
    int rc = ensure_pos(d, d->stream.get());
    if (rc) return rc;
    DevBuf<int32_t> d_pix, d_k;
    DevBuf<double> d_rays;
    hipError_t e = d_pix.alloc(size_t(n));
    if (e == hipSuccess) e = d_k.alloc(size_t(n));
    if (e == hipSuccess) e = d_rays.alloc(size_t(n) * 6);
    if (e == hipSuccess) e = hipMemcpy(d_pix.get(), pix, size_t(n) * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_k.get(), k, size_t(n) * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        launch_camera_rays(lens_for(d, d->lens), seed, d_pix.get(), d_k.get(), n, d_rays.get(), d->stream.get());
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream.get());
    if (e == hipSuccess) e = hipMemcpy(rays6, d_rays.get(), size_t(n) * 48, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(MCPT_ERR_HIP, hipGetErrorString(e));
    return MCPT_OK;
}

// ------------------------------------------------------------------------------------------------ progressive frames
// A frame of N samples per pixel rendered in passes of consecutive sample ranges.  Every (pixel, sample) owns its RNG key, so a pass
// of samples [k0, k1) computes the same radiance as the one-shot frame does for them, and k_fold_progressive continues the frame's float
// fold where the last pass left it: at done == N the image is mcpt_render's frame bit for bit.
struct mcpt_progressive {
    mcpt_device* d = nullptr;          // holds a reference (mcpt_device::refs)
    mcpt_render_params p{};            // p.spp = N
    int done = 0;
    bool broken = false;               // a step failed half-way: the image and the moments hold part of a pass
    DevBuf<int32_t> pixels; int64_t n_pixels = 0;      // the owned pixels of (rank, world)
    DevBuf<double> img;                // W*H*3: the float fold of samples [0, done) (pixels not owned stay 0)
    DevBuf<double> mom;                // W*H*2*3: sum x, sum x*x per channel
    DevBuf<uint8_t> hit;               // W*H: the pixel's primary ray hit
    DevBuf<double> partials;           // noise_ranges() x 3
    DevBuf<double> sums;               // 4 doubles: sum se2, sum mean^2, hit pixels, 0
    HostBuf<double> h_sums;            // pinned copy of sums (the pass's one 32-byte read-back)
    std::vector<int32_t> owned;        // host copy of `pixels`
    // adaptive frames (mcpt_progressive_create_adaptive): the active list, double-buffered -- a pass renders active[cur][0..n_active) and
    // the selection writes the pixels that continue to active[cur ^ 1]
    bool adaptive = false;
    double rel2 = 0.0, abs2 = 0.0;     // rel_target^2, abs_target^2
    int min_spp = 0;
    DevBuf<int32_t> active[2];
    int cur = 0;
    int64_t n_active = 0;
    DevBuf<int32_t> cnt;               // W*H: the samples each pixel holds (written for the listed pixels after every pass)
    DevBuf<unsigned long long> masks;  // 4 * adaptive_blocks(n_pixels): the keep ballots of the selection
    DevBuf<int32_t> block_counts, block_offsets;   // adaptive_blocks(n_pixels) each
    DevBuf<int32_t> total;             // the next list's length
    HostBuf<int32_t> h_total;          // pinned copy of total (the pass's 4-byte read-back)
    // first-hit AOVs (W*H[*3], owned pixels written; computed on the first mcpt_progressive_aovs / _denoise call: they do not depend on
    // the samples) and the guide record the denoiser's taps read
    bool aov_ready = false;
    DevBuf<int32_t> aov_mat; DevBuf<double> aov_depth, aov_normal, aov_albedo;
    DevBuf<DenoiseGuide> guide;
    DevBuf<DenoisePix> dn_buf[2];      // the denoiser's ping-pong buffers (W*H each), allocated on its first call
    mcpt_lens lens{};                  // the device's lens when the handle was created
    DevBuf<int32_t> hitcnt;            // W*H, under an active lens: the samples so far whose camera ray hit (hit = hitcnt > 0)
};

void mcpt_progressive_free(mcpt_progressive* h)
{
    if (!h) return;
    (void)hipSetDevice(h->d->ordinal);
    (void)hipStreamSynchronize(h->d->stream.get());
    mcpt_device* d = h->d;
    delete h;                          // its buffers go before the device reference
    mcpt_device_free(d);
}

// ap == null: a uniform frame; otherwise an adaptive one (arguments checked by the caller)
static int progressive_create(mcpt_device* d, const mcpt_render_params* p, const mcpt_adaptive_params* ap, mcpt_progressive** out)
{
    if (p->flags & (MCPT_RENDER_PIPELINE | MCPT_RENDER_KEEP_STATS))
        return fail(MCPT_ERR_ARG, "a progressive frame takes neither MCPT_RENDER_PIPELINE nor MCPT_RENDER_KEEP_STATS");
    int tw, th, rank, world;
    tile_shape(p, tw, th, rank, world);
    if (rank < 0 || rank >= world) return fail(MCPT_ERR_ARG, "rank outside world");
    HIP_TRY(hipSetDevice(d->ordinal));
    std::vector<int32_t> v;
    owned_pixel_list(d->width, d->height, tw, th, rank, world, v);
    const size_t px = size_t(d->width) * d->height;
    std::unique_ptr<mcpt_progressive, void (*)(mcpt_progressive*)> h(new mcpt_progressive, mcpt_progressive_free);
    h->d = d; d->refs.fetch_add(1);
    h->p = *p;
    h->lens = d->lens;
    h->n_pixels = int64_t(v.size());
    HIP_TRY(h->pixels.upload(v));
    HIP_TRY(alloc_zeroed(h->img, px * 3 * sizeof(double)));
    HIP_TRY(alloc_zeroed(h->mom, px * 6 * sizeof(double)));
    HIP_TRY(alloc_zeroed(h->hit, px));
    if (lens_active(h->lens)) HIP_TRY(alloc_zeroed(h->hitcnt, px * sizeof(int32_t)));
    HIP_TRY(alloc_zeroed(h->partials, size_t(kNoiseRanges) * 3 * sizeof(double)));
    HIP_TRY(alloc_zeroed(h->sums, 4 * sizeof(double)));
    HIP_TRY(h->h_sums.alloc(4));
    if (ap) {
        const size_t blocks = size_t(adaptive_blocks(int(v.size())));
        HIP_TRY(alloc_zeroed(h->active[0], v.size() * sizeof(int32_t)));
        HIP_TRY(alloc_zeroed(h->active[1], v.size() * sizeof(int32_t)));
        HIP_TRY(alloc_zeroed(h->cnt, px * sizeof(int32_t)));
        HIP_TRY(alloc_zeroed(h->masks, blocks * 4 * sizeof(unsigned long long)));
        HIP_TRY(alloc_zeroed(h->block_counts, blocks * sizeof(int32_t)));
        HIP_TRY(alloc_zeroed(h->block_offsets, blocks * sizeof(int32_t)));
        HIP_TRY(alloc_zeroed(h->total, sizeof(int32_t)));
        HIP_TRY(h->h_total.alloc(1));
        if (!v.empty()) HIP_TRY(hipMemcpy(h->active[0].get(), h->pixels.get(), v.size() * sizeof(int32_t), hipMemcpyDeviceToDevice));
        h->adaptive = true;
        h->rel2 = ap->rel_target * ap->rel_target;
        h->abs2 = ap->abs_target * ap->abs_target;
        h->min_spp = std::min(ap->min_spp, p->spp);
        h->n_active = h->n_pixels;
    }
    h->owned = std::move(v);
    *out = h.release();
    return MCPT_OK;
}

int mcpt_progressive_create(mcpt_device* d, const mcpt_render_params* p, mcpt_progressive** out)
{
    if (!out || !p) return fail(MCPT_ERR_ARG, "null argument");
    *out = nullptr;
    if (mcpt_device_count() <= 0) return fail(MCPT_ERR_NO_DEVICE, "no HIP device available (libmcpt has no CPU fallback)");
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    if (p->spp <= 0) return fail(MCPT_ERR_ARG, "spp must be positive");
    return progressive_create(d, p, nullptr, out);
}

int mcpt_progressive_create_adaptive(mcpt_device* d, const mcpt_render_params* p, const mcpt_adaptive_params* ap, mcpt_progressive** out)
{
    if (!out || !p || !ap) return fail(MCPT_ERR_ARG, "null argument");
    *out = nullptr;
    if (!(std::isfinite(ap->rel_target) && ap->rel_target >= 0.0 && std::isfinite(ap->abs_target) && ap->abs_target >= 0.0))
        return fail(MCPT_ERR_ARG, "rel_target and abs_target must be finite and >= 0");
    if (ap->min_spp < 2) return fail(MCPT_ERR_ARG, "min_spp must be >= 2 (a standard error needs two samples)");
    if (p->spp <= 0) return fail(MCPT_ERR_ARG, "spp must be positive");
    if (mcpt_device_count() <= 0) return fail(MCPT_ERR_NO_DEVICE, "no HIP device available (libmcpt has no CPU fallback)");
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    return progressive_create(d, p, ap, out);
}

int mcpt_progressive_step(mcpt_progressive* h, int32_t n, mcpt_stats* stats)
{
    if (!h || n <= 0) return fail(MCPT_ERR_ARG, "bad argument");
    if (h->done >= h->p.spp) return fail(MCPT_ERR_ARG, "the progressive frame is complete");
    if (h->broken) return fail(MCPT_ERR_ARG, "an earlier step of this progressive frame failed");
    if (h->adaptive && h->n_active == 0) return fail(MCPT_ERR_ARG, "the adaptive frame is complete: no pixel is active");
    mcpt_device* d = h->d;
    HIP_TRY(hipSetDevice(d->ordinal));
    if (stats) std::memset(stats, 0, sizeof *stats);
    mcpt_render_params q = h->p;
    q.spp = std::min(n, h->p.spp - h->done);
    const SampleRange r{h->done, q.spp, h->p.spp, h->mom.get(), h->hit.get(), &h->lens, h->hitcnt.get()};
    const PixelList L = h->adaptive ? PixelList{h->active[h->cur].get(), h->n_active} : PixelList{h->pixels.get(), h->n_pixels};
    const size_t ev_used0 = d->ev_used;
    int slot_used = -1;
    int rc = render_device_impl(d, r, L, &q, h->img.get(), stats, d->stream.get(), slot_used);
    if (rc == MCPT_OK && h->adaptive) {
        // which pixels continue: decided on the device; the host reads back the new list's length only
        launch_adaptive_select(L.pixels, int(L.n), h->mom.get(), h->hit.get(), h->done + q.spp, h->min_spp, h->rel2, h->abs2, h->cnt.get(), h->masks.get(),
                               h->block_counts.get(), h->block_offsets.get(), h->total.get(), h->active[h->cur ^ 1].get(), d->stream.get());
        hipError_t le = hipGetLastError();
        if (le == hipSuccess) le = hipMemcpyAsync(h->h_total.get(), h->total.get(), sizeof(int32_t), hipMemcpyDeviceToHost, d->stream.get());
        if (le != hipSuccess) rc = fail(MCPT_ERR_HIP, hipGetErrorString(le));
    }
    const hipError_t e = hipStreamSynchronize(d->stream.get());
    if (rc == MCPT_OK && e != hipSuccess) rc = fail(MCPT_ERR_HIP, hipGetErrorString(e));
    if (rc != MCPT_OK) { d->ev_used = ev_used0; h->broken = true; return rc; }
    h->done += q.spp;
    if (h->adaptive) { h->n_active = h->h_total[0]; h->cur ^= 1; }
    return MCPT_OK;
}

int64_t mcpt_progressive_active(const mcpt_progressive* h)
{
    if (!h) return fail(MCPT_ERR_ARG, "null handle");
    if (h->done >= h->p.spp) return 0;
    return h->adaptive ? h->n_active : h->n_pixels;
}

int64_t mcpt_progressive_active_pixels(mcpt_progressive* h, int32_t* pixels)
{
    const int64_t n = mcpt_progressive_active(h);
    if (n <= 0 || !pixels) return n;
    if (!h->adaptive) { std::memcpy(pixels, h->owned.data(), size_t(n) * sizeof(int32_t)); return n; }
    HIP_TRY(hipSetDevice(h->d->ordinal));
    HIP_TRY(hipMemcpy(pixels, h->active[h->cur].get(), size_t(n) * sizeof(int32_t), hipMemcpyDeviceToHost));
    return n;
}

int mcpt_progressive_sample_counts(mcpt_progressive* h, int32_t* counts)
{
    if (!h || !counts) return fail(MCPT_ERR_ARG, "null argument");
    if (!h->adaptive) {
        for (int32_t pix : h->owned) counts[pix] = h->done;
        return MCPT_OK;
    }
    HIP_TRY(hipSetDevice(h->d->ordinal));
    std::vector<int32_t> all(size_t(h->d->width) * h->d->height);
    HIP_TRY(hipMemcpy(all.data(), h->cnt.get(), all.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int32_t pix : h->owned) counts[pix] = all[size_t(pix)];
    return MCPT_OK;
}

int mcpt_progressive_done(const mcpt_progressive* h) { return h ? h->done : fail(MCPT_ERR_ARG, "null handle"); }

int mcpt_progressive_noise(mcpt_progressive* h, mcpt_noise* o)
{
    if (!h || !o) return fail(MCPT_ERR_ARG, "null argument");
    std::memset(o, 0, sizeof *o);
    o->done = h->done; o->spp = h->p.spp;
    if (h->done < 2) { o->rel_error = o->abs_rms = INFINITY; return MCPT_OK; }     // no variance estimate from fewer than two samples
    HIP_TRY(hipSetDevice(h->d->ordinal));
    hipStream_t st = h->d->stream.get();
    launch_noise_reduce(h->pixels.get(), h->n_pixels, h->mom.get(), h->hit.get(), h->done, h->cnt.get(), h->partials.get(), h->sums.get(), st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->h_sums.get(), h->sums.get(), 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    o->sum_se2 = h->h_sums[0]; o->sum_mean2 = h->h_sums[1]; o->pixels = int64_t(h->h_sums[2]);
    o->rel_error = o->sum_mean2 > 0 ? std::sqrt(o->sum_se2 / o->sum_mean2) : (o->sum_se2 > 0 ? INFINITY : 0.0);
    o->abs_rms = o->pixels > 0 ? std::sqrt(o->sum_se2 / (3.0 * double(o->pixels))) : 0.0;
    return MCPT_OK;
}

int mcpt_progressive_image_device(mcpt_progressive* h, double* d_img, double* d_stderr, void* stream)
{
    if (!h || (!d_img && !d_stderr)) return fail(MCPT_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(h->d->ordinal));
    launch_progressive_image(h->pixels.get(), h->n_pixels, h->img.get(), h->mom.get(), h->done, h->cnt.get(), h->p.spp, d_img, d_stderr, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return MCPT_OK;
}

int mcpt_progressive_image(mcpt_progressive* h, double* img, double* stderr_img)
{
    if (!h || (!img && !stderr_img)) return fail(MCPT_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(h->d->ordinal));
    const size_t bytes = size_t(h->d->width) * h->d->height * 3 * sizeof(double);
    DevBuf<double> d_est, d_err;
    // pageable host buffers: blocking copies either side; pixels this rank does not own keep the caller's values
    hipError_t e = hipSuccess;
    if (img) { e = d_est.alloc_bytes(bytes); if (e == hipSuccess) e = hipMemcpy(d_est.get(), img, bytes, hipMemcpyHostToDevice); }
    if (e == hipSuccess && stderr_img) { e = d_err.alloc_bytes(bytes); if (e == hipSuccess) e = hipMemcpy(d_err.get(), stderr_img, bytes, hipMemcpyHostToDevice); }
    int rc = e == hipSuccess ? mcpt_progressive_image_device(h, d_est.get(), d_err.get(), h->d->stream.get()) : fail(MCPT_ERR_HIP, hipGetErrorString(e));
    e = hipStreamSynchronize(h->d->stream.get());
    if (rc == MCPT_OK && e == hipSuccess && img) e = hipMemcpy(img, d_est.get(), bytes, hipMemcpyDeviceToHost);
    if (rc == MCPT_OK && e == hipSuccess && stderr_img) e = hipMemcpy(stderr_img, d_err.get(), bytes, hipMemcpyDeviceToHost);
    if (rc == MCPT_OK && e != hipSuccess) rc = fail(MCPT_ERR_HIP, hipGetErrorString(e));
    return rc;
}

// First-hit AOVs of the owned pixels: the primary hits of the owned list traced again on the device's stream and closest-hit workspace
// (launch_primary_hits, as a render call traces them), then k_primary_aov.  Once per handle.
static int ensure_aovs(mcpt_progressive* h)
{
    if (h->aov_ready) return MCPT_OK;
    mcpt_device* d = h->d;
    hipStream_t st = d->stream.get();
    int rc = ensure_dirs(d, st);
    if (rc) return rc;
    const size_t px = size_t(d->width) * d->height;
    DevBuf<PrimaryHit> hits;
    hipError_t e = alloc_once(hits, size_t(h->n_pixels) * sizeof(PrimaryHit));
    if (e == hipSuccess) e = alloc_once(h->aov_mat, px * sizeof(int32_t));
    if (e == hipSuccess) e = alloc_once(h->aov_depth, px * sizeof(double));
    if (e == hipSuccess) e = alloc_once(h->aov_normal, px * 3 * sizeof(double));
    if (e == hipSuccess) e = alloc_once(h->aov_albedo, px * 3 * sizeof(double));
    if (e == hipSuccess) e = alloc_once(h->guide, px * sizeof(DenoiseGuide));
    // pixels not owned: material -1 everywhere in the guide (all bits set), so that no tap reads them
    if (e == hipSuccess) e = hipMemsetAsync(h->guide.get(), 0xff, px * sizeof(DenoiseGuide), st);
    if (e == hipSuccess) {
        launch_primary_hits(d->ds, d->trace_mode == MCPT_TRACE_FAST, d->dirs.get(), h->pixels.get(), int(h->n_pixels), hits.get(), d->aux_ctr.get(), d->aux_queue.get(),
                            d->aux_slow_list.get(), d->slow_cap, st, d->cfg);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        launch_primary_aov(d->ds, h->pixels.get(), int(h->n_pixels), hits.get(), h->aov_mat.get(), h->aov_depth.get(), h->aov_normal.get(), h->aov_albedo.get(), h->guide.get(), st);
        e = hipGetLastError();
    }
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(MCPT_ERR_HIP, std::string("first-hit AOVs: ") + hipGetErrorString(e));
    h->aov_ready = true;
    return MCPT_OK;
}

int mcpt_progressive_aovs(mcpt_progressive* h, int32_t* material, double* depth, double* normal, double* albedo)
{
    if (!h) return fail(MCPT_ERR_ARG, "null handle");
    HIP_TRY(hipSetDevice(h->d->ordinal));
    int rc = ensure_aovs(h);
    if (rc) return rc;
    const size_t px = size_t(h->d->width) * h->d->height;
    // the device arrays whole, then the owned pixels into the caller's (pixels not owned keep the caller's values)
    auto fetch = [&](const void* src, void* dst, size_t per_pixel) -> int {
        if (!dst) return MCPT_OK;
        std::vector<uint8_t> all(px * per_pixel);
        HIP_TRY(hipMemcpy(all.data(), src, all.size(), hipMemcpyDeviceToHost));
        for (int32_t pix : h->owned) std::memcpy(static_cast<uint8_t*>(dst) + size_t(pix) * per_pixel, all.data() + size_t(pix) * per_pixel, per_pixel);
        return MCPT_OK;
    };
    if ((rc = fetch(h->aov_mat.get(), material, sizeof(int32_t)))) return rc;
    if ((rc = fetch(h->aov_depth.get(), depth, sizeof(double)))) return rc;
    if ((rc = fetch(h->aov_normal.get(), normal, 3 * sizeof(double)))) return rc;
    return fetch(h->aov_albedo.get(), albedo, 3 * sizeof(double));
}

static int denoise_args(const mcpt_progressive* h, const mcpt_denoise_params* dp, int& iterations, double& sigma_l, double& sigma_z)
{
    if (!h) return fail(MCPT_ERR_ARG, "null handle");
    const mcpt_denoise_params z{};
    const mcpt_denoise_params& q = dp ? *dp : z;
    if (q.reserved != 0) return fail(MCPT_ERR_ARG, "mcpt_denoise_params.reserved must be 0");
    if (q.iterations < 0 || q.iterations > MCPT_DENOISE_MAX_ITERATIONS) return fail(MCPT_ERR_ARG, "denoise iterations outside 0..10");
    if (!(std::isfinite(q.sigma_l) && q.sigma_l >= 0.0 && std::isfinite(q.sigma_z) && q.sigma_z >= 0.0))
        return fail(MCPT_ERR_ARG, "denoise sigmas must be finite and >= 0 (0: the default)");
    if (h->done < 2) return fail(MCPT_ERR_ARG, "denoising needs a variance estimate: at least two samples done");
    const bool defaults = q.iterations == 0 && q.sigma_l == 0.0 && q.sigma_z == 0.0;     // a zero struct: the defaults
    iterations = defaults ? MCPT_DENOISE_ITERATIONS : q.iterations;
    sigma_l = q.sigma_l > 0.0 ? q.sigma_l : MCPT_DENOISE_SIGMA_L;
    sigma_z = q.sigma_z > 0.0 ? q.sigma_z : MCPT_DENOISE_SIGMA_Z;
    return MCPT_OK;
}

int mcpt_progressive_denoise_device(mcpt_progressive* h, const mcpt_denoise_params* dp, double* d_img, void* stream)
{
    int iterations = 0;
    double sigma_l = 0.0, sigma_z = 0.0;
    int rc = denoise_args(h, dp, iterations, sigma_l, sigma_z);
    if (rc) return rc;
    if (!d_img) return fail(MCPT_ERR_ARG, "null image");
    HIP_TRY(hipSetDevice(h->d->ordinal));
    if ((rc = ensure_aovs(h))) return rc;
    const size_t px = size_t(h->d->width) * h->d->height;
    for (auto& b : h->dn_buf)
        if (!b) HIP_TRY(b.alloc(px));
    launch_denoise(h->pixels.get(), h->n_pixels, h->d->width, h->d->height, h->img.get(), h->mom.get(), h->done, h->cnt.get(), h->p.spp, h->aov_albedo.get(), h->guide.get(),
                   iterations, sigma_l, sigma_z, h->dn_buf[0].get(), h->dn_buf[1].get(), d_img, static_cast<hipStream_t>(stream));
    HIP_TRY(hipGetLastError());
    return MCPT_OK;
}

int mcpt_progressive_denoise(mcpt_progressive* h, const mcpt_denoise_params* dp, double* img)
{
    int iterations = 0;
    double sigma_l = 0.0, sigma_z = 0.0;
    int rc = denoise_args(h, dp, iterations, sigma_l, sigma_z);
    if (rc) return rc;
    if (!img) return fail(MCPT_ERR_ARG, "null image");
    HIP_TRY(hipSetDevice(h->d->ordinal));
    const size_t bytes = size_t(h->d->width) * h->d->height * 3 * sizeof(double);
    DevBuf<double> d_out;
    // pageable host buffer: blocking copies either side; pixels this rank does not own keep the caller's values
    hipError_t e = d_out.alloc_bytes(bytes);
    if (e == hipSuccess) e = hipMemcpy(d_out.get(), img, bytes, hipMemcpyHostToDevice);
    rc = e == hipSuccess ? mcpt_progressive_denoise_device(h, dp, d_out.get(), h->d->stream.get()) : fail(MCPT_ERR_HIP, hipGetErrorString(e));
    e = hipStreamSynchronize(h->d->stream.get());
    if (rc == MCPT_OK && e == hipSuccess) e = hipMemcpy(img, d_out.get(), bytes, hipMemcpyDeviceToHost);
    if (rc == MCPT_OK && e != hipSuccess) rc = fail(MCPT_ERR_HIP, hipGetErrorString(e));
    return rc;
}

int mcpt_progressive_next_pass(int32_t spp, int32_t done, double remaining_s, double s_per_sample)
{
    if (spp <= 0 || done < 0 || done >= spp) return 0;
    if (done == 0) return std::min(spp, 8);                  // the first pass: no rate measured yet, and a frame needs one pass
    const int n = std::min(spp - done, done);               // each later pass doubles the samples done
    if (std::isinf(remaining_s) && remaining_s > 0) return n;     // no time budget
    if (!(remaining_s > 0)) return 0;                        // the budget is spent
    if (!(s_per_sample > 0)) return n;                        // no rate to go by
    const double cap = std::floor(remaining_s / s_per_sample);
    return cap < 1.0 ? 0 : int(std::min<double>(n, cap));
}

// ------------------------------------------------------------------------------------------------ output
int mcpt_quantize_rgb8(const double* img, int64_t n, uint8_t* rgb8)
{
    if (!img || !rgb8 || n < 0) return fail(MCPT_ERR_ARG, "bad argument");
    for (int64_t i = 0; i < n; i++) {
        double v = img[i] * 255;                  // imshow, MTPC.cpp:26-28: (unsigned char)glm::clamp(v*255, 0.0, 255.0)
        v = std::max(v, 0.0);
        v = std::min(v, 255.0);
        rgb8[i] = static_cast<uint8_t>(v);
    }
    return MCPT_OK;
}

int64_t mcpt_png_encode(const uint8_t* rgb8, int32_t w, int32_t h, uint8_t* out, int64_t cap)
{
    if (!rgb8 || !out) return fail(MCPT_ERR_ARG, "null argument");
    const int64_t n = png_encode(rgb8, w, h, out, cap);
    if (n < 0) return fail(MCPT_ERR_ARG, "png: bad size or buffer too small");
    return n;
}

int mcpt_write_png(const char* file, const uint8_t* rgb8, int32_t w, int32_t h)
{
    if (!file || !rgb8 || w <= 0 || h <= 0) return fail(MCPT_ERR_ARG, "bad argument");
    const int64_t cap = 8 + 25 + 12 + 2 + int64_t(h) * (int64_t(w) * 3 + 6) + 4 + 12 + 16;
    std::vector<uint8_t> buf(static_cast<size_t>(cap));
    const int64_t n = png_encode(rgb8, w, h, buf.data(), cap);
    if (n < 0) return fail(MCPT_ERR_ARG, "png: width too large for one stored block per row");
    FILE* fp = std::fopen(file, "wb");
    if (!fp) return fail(MCPT_ERR_IO, std::string("cannot open ") + file);
    const bool ok = std::fwrite(buf.data(), 1, size_t(n), fp) == size_t(n);
    std::fclose(fp);                              // the reference never closes it (truncated veach-mis PNGs)
    return ok ? MCPT_OK : fail(MCPT_ERR_IO, std::string("short write to ") + file);
}

int64_t mcpt_png_encode_deflate(const uint8_t* rgb8, int32_t w, int32_t h, uint8_t* out, int64_t cap)
{
    if (!rgb8 || w <= 0 || h <= 0) { fail(MCPT_ERR_ARG, "bad argument"); return MCPT_ERR_ARG; }
    const int64_t n = png_encode_deflate(rgb8, w, h, out, cap);
    if (n < 0) { fail(MCPT_ERR_ARG, "png: buffer too small"); return MCPT_ERR_ARG; }
    return n;
}

int mcpt_write_png_deflate(const char* file, const uint8_t* rgb8, int32_t w, int32_t h)
{
    if (!file || !rgb8 || w <= 0 || h <= 0) return fail(MCPT_ERR_ARG, "bad argument");
    const int64_t need = png_encode_deflate(rgb8, w, h, nullptr, 0);
    std::vector<uint8_t> buf(static_cast<size_t>(need));
    const int64_t n = png_encode_deflate(rgb8, w, h, buf.data(), need);
    if (n != need) return fail(MCPT_ERR_ARG, "png: encoder size mismatch");
    FILE* fp = std::fopen(file, "wb");
    if (!fp) return fail(MCPT_ERR_IO, std::string("cannot open ") + file);
    const bool ok = std::fwrite(buf.data(), 1, size_t(n), fp) == size_t(n);
    return (std::fclose(fp) == 0 && ok) ? MCPT_OK : fail(MCPT_ERR_IO, std::string("short write to ") + file);
}

int mcpt_write_pfm(const char* file, const double* img, int32_t w, int32_t h)
{
    if (!file || !img || w <= 0 || h <= 0) return fail(MCPT_ERR_ARG, "bad argument");
    std::string err;
    const int rc = write_pfm(file, img, w, h, err);
    return rc ? fail(rc, err) : MCPT_OK;
}

// Identity of the frame a checkpoint belongs to: FNV-1a over everything the picture depends on besides spp / seed / parts
// (which the file header carries): geometry, normals, texture coordinates and material of every face in leaf order, material
// records and texels, lights, camera, resolution, Morton domain.  Version 2 of the tag (version 1 hashed three counts).
static uint64_t scene_tag(const Scene& s)
{
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void* p, size_t n) { const unsigned char* b = static_cast<const unsigned char*>(p); for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; } };
    auto mixd = [&](double v) { mix(&v, sizeof v); };
    auto mixi = [&](int64_t v) { mix(&v, sizeof v); };
    mixi(2); mixi(int64_t(s.faces.size())); mixi(int64_t(s.materials.size())); mixi(int64_t(s.lights.size()));
    for (const FaceRec& f : s.faces) {
        for (int c = 0; c < 3; c++) { mixd(f.v[c].x); mixd(f.v[c].y); mixd(f.v[c].z); mixd(f.vn[c].x); mixd(f.vn[c].y); mixd(f.vn[c].z); mixd(f.vt[c][0]); mixd(f.vt[c][1]); }
        mixi(f.material); mixi(f.morton);
    }
    for (const MaterialRec& m : s.materials) {
        mixd(m.kd.x); mixd(m.kd.y); mixd(m.kd.z); mixd(m.ks.x); mixd(m.ks.y); mixd(m.ks.z); mixd(m.Ns); mixd(m.Ni);
        mixi(m.has_map); mixi(m.map_w); mixi(m.map_h);
        if (!m.bgr.empty()) mix(m.bgr.data(), m.bgr.size());
    }
    for (const LightRec& l : s.lights) { mixi(l.material); mixd(l.radiance.x); mixd(l.radiance.y); mixd(l.radiance.z); }
    for (const Vec3* v : {&s.eye, &s.look_at, &s.up}) { mixd(v->x); mixd(v->y); mixd(v->z); }
    mixd(s.fovy); mixi(s.width); mixi(s.height);
    for (int a = 0; a < 3; a++) { mixd(s.morton_lo[a]); mixd(s.morton_span[a]); }
    return h;
}

// The identity of a frame rendered under a lens: the scene's tag with the lens mixed in -- only when the lens is active, so that a pinhole
// frame keeps its tag (and existing checkpoint files stay valid) and the two never resume from each other's files.
static uint64_t frame_tag(const Scene& s, const mcpt_lens* l)
{
    uint64_t h = scene_tag(s);
    if (!l || !lens_active(*l)) return h;
    auto mix = [&](const void* p, size_t n) { const unsigned char* b = static_cast<const unsigned char*>(p); for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; } };
    const char tag[] = "lens";
    const int64_t flags = l->flags;
    const double focus = l->focus_distance > 0.0 ? l->focus_distance : 0.0;     // (every F <= 0 is the same lens)
    mix(tag, 4); mix(&flags, sizeof flags); mix(&l->aperture, sizeof(double)); mix(&focus, sizeof focus);
    return h;
}

int mcpt_checkpoint_save(const char* file, const mcpt_scene* h, const double* img, int32_t spp, uint64_t seed, int32_t parts, const uint8_t* done)
{
    if (!file || !h || !img || !done || spp <= 0 || parts <= 0 || parts > 65536) return fail(MCPT_ERR_ARG, "bad argument");
    std::string err;
    const int rc = checkpoint_save(file, img, h->s.width, h->s.height, spp, seed, scene_tag(h->s), parts, done, err);
    return rc ? fail(rc, err) : MCPT_OK;
}

int mcpt_checkpoint_load(const char* file, const mcpt_scene* h, double* img, int32_t spp, uint64_t seed, int32_t parts, uint8_t* done)
{
    if (!file || !h || !img || !done || spp <= 0 || parts <= 0 || parts > 65536) return fail(MCPT_ERR_ARG, "bad argument");
    std::string err;
    const int rc = checkpoint_load(file, img, h->s.width, h->s.height, spp, seed, scene_tag(h->s), parts, done, err);
    return rc ? fail(rc, err) : MCPT_OK;
}

int mcpt_decode_jpeg(const char* file, int32_t* width, int32_t* height, uint8_t* bgr, int64_t cap)
{
    if (!file || !width || !height) return fail(MCPT_ERR_ARG, "null argument");
    int w = 0, h = 0;
    std::vector<uint8_t> px;
    std::string err;
    if (!decode_jpeg_file(file, w, h, px, err)) return fail(MCPT_ERR_IO, err);
    *width = w; *height = h;
    if (bgr) {
        if (cap < int64_t(px.size())) return fail(MCPT_ERR_ARG, "buffer too small");
        std::memcpy(bgr, px.data(), px.size());
    }
    return MCPT_OK;
}

// ------------------------------------------------------------------------------------------------ render_scene
// The options struct grew with the library version (100: seed .. output_prefix; 101: .. reserved; 102: .. devices) and carries no size
// of its own.  mcpt_render_scene_ex was the only entry point through version 102 and reads the struct as it stood then -- every field
// of it: a caller that sets load_flags, a checkpoint or num_devices through it gets what it asked for, not a silently different
// render -- so a caller compiled against a 100 / 101 header must hand over a zero-extended struct of that size.  Fields added after
// 102 are reached through mcpt_render_scene_opts only, which takes the caller's sizeof and reads exactly that many bytes.
// render_scene's progressive frame: passes of mcpt_progressive_next_pass's schedule until the relative error reaches o.noise_target (checked
// after every pass), the time budget runs out (measured from the first pass on, the rate of the last pass deciding the next one's size) or
// every sample is in.  Without a time budget the pass boundaries depend on nothing but N, so the stopping point is reproducible.
// An adaptive frame (o.adaptive_min_spp > 0): the first pass is min(N, adaptive_min_spp), the frame ends when no pixel is active, and the
// time budget scales the last pass's seconds per sample by the share of pixels the next pass renders (the fixed cost of a pass is not
// modelled).  counts (may be null) receives the samples of every pixel; denoised (may be null) mcpt_progressive_denoise's image with the
// defaults; aovs (may be null) the AOV images, every one as W*H*3 doubles (albedo, normal, depth, material: the scalars in all channels).
struct SceneAovs { std::vector<double> albedo, normal, depth, material; };
static int render_scene_progressive(mcpt_device* dev, const mcpt_render_params& rp, const mcpt_render_scene_options& o, bool talk, std::vector<double>& img,
                                    std::vector<double>* err, std::vector<int32_t>* counts, std::vector<double>* denoised, SceneAovs* aovs,
                                    int& rendered, mcpt_stats& local)
{
    using clk = std::chrono::steady_clock;
    const bool adaptive = o.adaptive_min_spp > 0;
    mcpt_progressive* pr = nullptr;
    mcpt_adaptive_params ap{o.noise_target, o.abs_target, o.adaptive_min_spp, 0};
    int rc = adaptive ? mcpt_progressive_create_adaptive(dev, &rp, &ap, &pr) : mcpt_progressive_create(dev, &rp, &pr);
    if (rc) return rc;
    const auto t0 = clk::now();
    double rate = 0.0;
    mcpt_noise nz{};
    nz.rel_error = INFINITY;
    bool measured = false;
    for (;;) {
        const double remaining = o.time_budget_s > 0 ? o.time_budget_s - std::chrono::duration<double>(clk::now() - t0).count() : INFINITY;
        int n = mcpt_progressive_next_pass(rp.spp, pr->done, remaining, rate);
        if (adaptive && pr->done == 0) n = std::min(rp.spp, o.adaptive_min_spp);
        if (n <= 0 || (adaptive && mcpt_progressive_active(pr) == 0)) break;
        const auto ts = clk::now();
        const int64_t listed = mcpt_progressive_active(pr);
        mcpt_stats one{};
        if ((rc = mcpt_progressive_step(pr, n, &one))) break;
        rate = std::chrono::duration<double>(clk::now() - ts).count() / n;
        if (adaptive) rate = listed > 0 ? rate * double(mcpt_progressive_active(pr)) / double(listed) : 0.0;
        local.rays_primary += one.rays_primary; local.rays_shadow += one.rays_shadow; local.rays_bounce += one.rays_bounce;
        local.node_visits += one.node_visits; local.tri_tests += one.tri_tests; local.shade_calls += one.shade_calls;
        local.samples += one.samples; local.shadow_skipped += one.shadow_skipped; local.ms_trace += one.ms_trace;
        local.ms_total += one.ms_total; local.launches += one.launches;
        local.max_depth = std::max(local.max_depth, one.max_depth);
        measured = false;
        if (o.noise_target > 0 && !adaptive) {
            if ((rc = mcpt_progressive_noise(pr, &nz))) break;
            measured = true;
            if (nz.rel_error <= o.noise_target) break;
        }
    }
    if (rc == MCPT_OK && talk && !measured) rc = mcpt_progressive_noise(pr, &nz);
    if (rc == MCPT_OK) {
        rendered = pr->done;
        if (err) err->assign(img.size(), 0.0);
        rc = mcpt_progressive_image(pr, img.data(), err ? err->data() : nullptr);
    }
    if (rc == MCPT_OK && counts) {
        counts->assign(img.size() / 3, 0);
        rc = mcpt_progressive_sample_counts(pr, counts->data());
    }
    if (rc == MCPT_OK && denoised) {
        denoised->assign(img.size(), 0.0);
        rc = mcpt_progressive_denoise(pr, nullptr, denoised->data());
    }
    if (rc == MCPT_OK && aovs) {
        const size_t px = img.size() / 3;
        std::vector<int32_t> mat(px, -1);
        std::vector<double> depth(px, 0.0);
        aovs->albedo.assign(img.size(), 0.0);
        aovs->normal.assign(img.size(), 0.0);
        rc = mcpt_progressive_aovs(pr, mat.data(), depth.data(), aovs->normal.data(), aovs->albedo.data());
        aovs->depth.resize(img.size());
        aovs->material.resize(img.size());
        for (size_t i = 0; i < px; i++)
            for (size_t c = 0; c < 3; c++) { aovs->depth[3 * i + c] = depth[i]; aovs->material[3 * i + c] = double(mat[i]); }
    }
    if (rc == MCPT_OK && talk) std::printf("progressive: %d of %d samples per pixel, relative error %.4g\n", pr->done, rp.spp, nz.rel_error);
    mcpt_progressive_free(pr);
    return rc;
}

static constexpr int64_t kOptionsBytesV102 = int64_t(offsetof(mcpt_render_scene_options, devices) + sizeof(const int32_t*));
int mcpt_render_scene_ex(const char* path, const char* filename, int32_t spp, const mcpt_render_scene_options* opt, mcpt_stats* stats)
{
    return mcpt_render_scene_opts(path, filename, spp, opt, opt ? kOptionsBytesV102 : 0, stats);
}

int mcpt_render_scene_opts(const char* path, const char* filename, int32_t spp, const mcpt_render_scene_options* opt, int64_t opt_bytes, mcpt_stats* stats)
{
    return mcpt_render_scene_lens(path, filename, spp, opt, opt_bytes, nullptr, stats);
}

int mcpt_render_scene_lens(const char* path, const char* filename, int32_t spp, const mcpt_render_scene_options* opt, int64_t opt_bytes,
                           const mcpt_lens* lens, mcpt_stats* stats)
{
    if (!path || !filename || spp <= 0 || opt_bytes < 0 || (opt_bytes > 0 && !opt)) return fail(MCPT_ERR_ARG, "bad argument");
    if (int lrc = lens_check(lens)) return lrc;
    mcpt_render_scene_options o{};
    if (opt) std::memcpy(&o, opt, std::min<size_t>(size_t(opt_bytes), sizeof o));
    const bool talk = !o.quiet;
    // a noise target, a time budget or the error image: the frame goes through a progressive handle (one GPU, no checkpoint)
    const bool adaptive = o.adaptive_min_spp > 0;
    const bool progressive = o.noise_target > 0 || o.time_budget_s > 0 || (o.output_flags & (MCPT_OUT_ERROR_PFM | MCPT_OUT_DENOISED | MCPT_OUT_AOV_PFM)) ||
                             adaptive;
    if (o.noise_target < 0 || o.time_budget_s < 0 || std::isnan(o.noise_target) || std::isnan(o.time_budget_s))
        return fail(MCPT_ERR_ARG, "noise_target and time_budget_s must be >= 0");
    if (o.adaptive_min_spp < 0 || o.adaptive_min_spp == 1 || (adaptive && (!(std::isfinite(o.abs_target) && o.abs_target >= 0.0) || std::isinf(o.noise_target))))
        return fail(MCPT_ERR_ARG, "adaptive_min_spp must be 0 or >= 2, the targets finite and >= 0");
    if (progressive && (o.checkpoint || o.num_devices != 0))
        return fail(MCPT_ERR_ARG, "a noise target, a time budget, an adaptive frame, MCPT_OUT_ERROR_PFM, MCPT_OUT_DENOISED or MCPT_OUT_AOV_PFM renders "
                                  "on one GPU without a checkpoint");
    if ((o.output_flags & MCPT_OUT_DENOISED) && spp < 2) return fail(MCPT_ERR_ARG, "MCPT_OUT_DENOISED needs N >= 2 (a variance estimate)");
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    mcpt_scene* sc = nullptr;
    int rc = mcpt_scene_load_ex(path, filename, o.load_flags, &sc);
    if (rc) return rc;
    if (o.width > 0 && o.height > 0) mcpt_scene_set_resolution(sc, o.width, o.height);
    const Scene& s = sc->s;
    if (talk) {
        std::printf("%s%s.obj\nnumber of materials = %zu\nnumber of vertices = %zu\nnumber of faces = %zu\n", path, filename,
                    s.materials.size(), s.v.size(), s.faces.size());
        std::printf("Total real = %d\nBuild BVH success\n", s.bi.Nr);
    }
    mcpt_device* dev = nullptr;
    mcpt_multi* multi = nullptr;
    const bool many = o.num_devices > 0 || o.num_devices == -1;
    if (many) rc = mcpt_multi_create(sc, o.num_devices > 0 ? o.devices : nullptr, o.num_devices > 0 ? o.num_devices : 0, MCPT_BUILD_HOST, o.gather, &multi);
    else rc = mcpt_device_create(sc, o.device, &dev);
    if (rc == MCPT_OK && lens) rc = many ? mcpt_multi_set_lens(multi, lens) : mcpt_device_set_lens(dev, lens);
    if (rc) { if (dev) mcpt_device_free(dev); if (multi) mcpt_multi_free(multi); mcpt_scene_free(sc); return rc; }
    if (talk && many) std::printf("rendering on %d GPUs\n", mcpt_multi_num_devices(multi));
    if (many && o.checkpoint) {
        mcpt_multi_free(multi); mcpt_scene_free(sc);
        return fail(MCPT_ERR_ARG, "a checkpointed frame is rendered partition by partition on one GPU: leave num_devices at 0");
    }
    const auto t1 = clk::now();
    if (talk) std::printf("Phase 1(read scene + bvh build) time cost = %.3f ms\n", std::chrono::duration<double, std::milli>(t1 - t0).count());
    std::vector<double> img(size_t(s.width) * s.height * 3, 0.0);
    mcpt_render_params rp{};
    rp.spp = spp; rp.seed = o.seed; rp.world = 1;
    mcpt_stats local{};
    int rendered = spp;                                  // samples per pixel the written frame holds
    std::vector<double> err_img;
    std::vector<int32_t> counts;                         // adaptive frames: the samples of every pixel
    std::vector<double> denoised;
    SceneAovs aovs;
    if (progressive) {
        rc = render_scene_progressive(dev, rp, o, talk, img, (o.output_flags & MCPT_OUT_ERROR_PFM) ? &err_img : nullptr, adaptive ? &counts : nullptr,
                                      (o.output_flags & MCPT_OUT_DENOISED) ? &denoised : nullptr, (o.output_flags & MCPT_OUT_AOV_PFM) ? &aovs : nullptr,
                                      rendered, local);
    } else if (!o.checkpoint) {
        rc = many ? mcpt_multi_render(multi, &rp, img.data(), &local) : mcpt_render(dev, &rp, img.data(), &local);
    } else {
        // the frame in `parts` tile partitions, saved after each; partitions a matching checkpoint already holds are skipped
        const int parts = o.checkpoint_parts > 0 ? o.checkpoint_parts : 8;
        std::vector<uint8_t> done(size_t(parts), 0);
        const uint64_t tag = frame_tag(s, lens);
        std::string cerr;
        const int lrc = checkpoint_load(o.checkpoint, img.data(), s.width, s.height, spp, o.seed, tag, parts, done.data(), cerr);
        if (lrc != MCPT_OK) { std::fill(img.begin(), img.end(), 0.0); std::fill(done.begin(), done.end(), uint8_t(0)); }
        if (talk && lrc == MCPT_OK) {
            int have = 0;
            for (uint8_t v : done) have += v ? 1 : 0;
            std::printf("resuming from %s: %d of %d partitions done\n", o.checkpoint, have, parts);
        }
        rp.world = parts;
        for (int part = 0; part < parts && rc == MCPT_OK; part++) {
            if (done[size_t(part)]) continue;
            rp.rank = part;
            mcpt_stats one{};
            rc = mcpt_render(dev, &rp, img.data(), &one);
            if (rc != MCPT_OK) break;
            local.rays_primary += one.rays_primary; local.rays_shadow += one.rays_shadow; local.rays_bounce += one.rays_bounce;
            local.node_visits += one.node_visits; local.tri_tests += one.tri_tests; local.shade_calls += one.shade_calls;
            local.samples += one.samples; local.shadow_skipped += one.shadow_skipped; local.ms_trace += one.ms_trace;
            local.ms_total += one.ms_total; local.launches += one.launches;
            local.max_depth = std::max(local.max_depth, one.max_depth);
            done[size_t(part)] = 1;
            rc = checkpoint_save(o.checkpoint, img.data(), s.width, s.height, spp, o.seed, tag, parts, done.data(), cerr);
            if (rc) rc = fail(rc, cerr);
        }
    }
    const auto t2 = clk::now();
    if (rc == MCPT_OK) {
        if (talk) std::printf("Phase 2(ray tracing) = %.3f ms\n", std::chrono::duration<double, std::milli>(t2 - t1).count());
        std::vector<uint8_t> rgb(img.size());
        mcpt_quantize_rgb8(img.data(), int64_t(img.size()), rgb.data());
        const std::string prefix = o.output_prefix ? std::string(o.output_prefix) : std::string("../result/") + filename;
        const std::string stem = prefix + "-SPP" + std::to_string(rendered);            // imshow, MTPC.cpp:17-20 (a progressive frame stopped early: its own count)
        rc = (o.output_flags & MCPT_OUT_PNG_DEFLATE) ? mcpt_write_png_deflate((stem + ".png").c_str(), rgb.data(), s.width, s.height)
                                                      : mcpt_write_png((stem + ".png").c_str(), rgb.data(), s.width, s.height);
        if (rc == MCPT_OK && (o.output_flags & MCPT_OUT_PFM)) rc = mcpt_write_pfm((stem + ".pfm").c_str(), img.data(), s.width, s.height);
        if (rc == MCPT_OK && !err_img.empty()) rc = mcpt_write_pfm((stem + ".err.pfm").c_str(), err_img.data(), s.width, s.height);
        if (rc == MCPT_OK && (o.output_flags & MCPT_OUT_SPP_PFM)) {
            // the sample-count map, the count in every channel: `rendered` everywhere unless the frame was adaptive
            std::vector<double> spp_img(img.size(), double(rendered));
            for (size_t i = 0; i < counts.size(); i++) spp_img[3 * i] = spp_img[3 * i + 1] = spp_img[3 * i + 2] = double(counts[i]);
            rc = mcpt_write_pfm((stem + ".spp.pfm").c_str(), spp_img.data(), s.width, s.height);
        }
        if (rc == MCPT_OK && !denoised.empty()) {
            mcpt_quantize_rgb8(denoised.data(), int64_t(denoised.size()), rgb.data());
            const std::string dn = stem + ".denoised";
            rc = (o.output_flags & MCPT_OUT_PNG_DEFLATE) ? mcpt_write_png_deflate((dn + ".png").c_str(), rgb.data(), s.width, s.height)
                                                          : mcpt_write_png((dn + ".png").c_str(), rgb.data(), s.width, s.height);
            if (rc == MCPT_OK && (o.output_flags & MCPT_OUT_PFM)) rc = mcpt_write_pfm((dn + ".pfm").c_str(), denoised.data(), s.width, s.height);
        }
        if (rc == MCPT_OK && (o.output_flags & MCPT_OUT_AOV_PFM)) {
            const std::pair<const char*, const std::vector<double>*> files[] = {
                {".albedo.pfm", &aovs.albedo}, {".normal.pfm", &aovs.normal}, {".depth.pfm", &aovs.depth}, {".material.pfm", &aovs.material}};
            for (const auto& f : files)
                if (rc == MCPT_OK) rc = mcpt_write_pfm((stem + f.first).c_str(), f.second->data(), s.width, s.height);
        }
    }
    if (stats) *stats = local;
    if (dev) mcpt_device_free(dev);
    if (multi) mcpt_multi_free(multi);
    mcpt_scene_free(sc);
    return rc;
}

int mcpt_render_scene(const char* path, const char* filename, int32_t spp)
{
    return mcpt_render_scene_ex(path, filename, spp, nullptr, nullptr);
}

}  // extern "C"
