// C ABI, scene handles (include/mcpt.h: mcpt_scene_*): load or describe a scene, read back its host build; the fast walk's culling
// hierarchy the devices of a scene share; which trace engine a scene gets; the tile partition of a frame over ranks.
#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "handles.hpp"

using namespace mcpt;

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
std::shared_ptr<const FastBvh> shared_fast_bvh(const mcpt_scene* h, const std::vector<int32_t>& order, const Knobs& k)
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

std::shared_ptr<const FastBvh> private_fast_bvh(const std::vector<FaceRec>& faces, const std::vector<int32_t>& order, const Knobs& k)
{
    auto fb = std::make_shared<FastBvh>();
    build_fast_bvh(faces, order.data(), int(faces.size()), *fb, stack_limit_for(k), build_opts_for(k));
    return fb;
}

void scene_release(const mcpt_scene* s) { if (s && s->refs.fetch_sub(1) == 1) delete s; }

// Engine of the fast walk for a scene of t triangles (include/mcpt.h: mcpt_scene_trace_engine).  Measured on MI355X, frame times pool /
// vote: cornell-box (15 k triangles) 82.0 / 92.3 ms, veach-mis 147.5 / 160.7, one eighth of a cornell-box frame 13.9 / 15.3; the 204 k
// triangle interior 253 / 250, 10 M triangles 56.3 / 52.8: where the walk waits for memory, the pool engine's longer chain of dependent
// LDS and memory round trips per step costs what its fuller lanes save, or more.
int trace_engine_for(long long t, const Knobs& k)
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

// ------------------------------------------------------------------------------------------------ partition
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

int tile_shape(const mcpt_render_params* p, TileShape& t)
{
    t.tw = (p && p->tile_w > 0) ? p->tile_w : 32;
    t.th = (p && p->tile_h > 0) ? p->tile_h : 8;
    t.world = (p && p->world > 1) ? p->world : 1;
    t.rank = (p && t.world > 1) ? p->rank : 0;
    if (t.rank < 0 || t.rank >= t.world) return fail(MCPT_ERR_ARG, "rank outside world");
    return MCPT_OK;
}

int owned_pixels(int W, int H, const mcpt_render_params* p, std::vector<int32_t>& out)
{
    TileShape t;
    if (const int rc = tile_shape(p, t)) return rc;
    out.clear();
    const int shift = tile_shift(t.world);
    for (int y = 0; y < H; y++) {
        const int ty = y / t.th;
        for (int x = 0; x < W; x++) {
            const int tx = x / t.tw;
            if ((tx + shift * ty) % t.world == t.rank) out.push_back(y * W + x);
        }
    }
    return MCPT_OK;
}

extern "C" {

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

int64_t mcpt_owned_pixels(const mcpt_scene* h, const mcpt_render_params* p, int32_t* pixels)
{
    if (!h) return fail(MCPT_ERR_ARG, "null scene");
    std::vector<int32_t> v;
    if (const int rc = owned_pixels(h->s.width, h->s.height, p, v)) return rc;
    if (pixels) std::copy(v.begin(), v.end(), pixels);
    return int64_t(v.size());
}

}  // extern "C"
