// C ABI, a device's geometry and camera changed in place (include/mcpt.h: mcpt_device_update_vertices, mcpt_device_set_camera): the stages
// of device creation again on new vertex positions -- the reference's structures rebuilt on the GPU, the culling hierarchy refitted
// (topology kept, boxes recomputed bottom up: build_kernels.hip) or rebuilt with the device's own builder, the pre-test records, the light
// tables -- into the arrays the trace kernels already read.  The scene handle is never written: the device owns what it changes.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "build_kernels.hpp"
#include "handles.hpp"

using namespace mcpt;

namespace {

using Update = mcpt_device::Update;

double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// the emitter faces' vertices, light by light in material face order (the order of DLightTri)
void light_vertices(const Scene& s, const double* v, std::vector<double>& out)
{
    out.clear();
    for (const LightRec& l : s.lights)
        for (int32_t f : s.materials[l.material].faces) out.insert(out.end(), v + size_t(f) * 9, v + size_t(f) * 9 + 9);
}

}  // namespace

// First update: the faces in .obj order become resident (device creation frees its staging copy, and a host-built device never had one)
int stage_faces(mcpt_device* d)
{
    if (d->upd) return MCPT_OK;
    const Scene& s = d->scene->s;
    const int t = d->bi.t;
    std::unique_ptr<Update> u(new Update);
    std::vector<double, default_init_alloc<double>> v9(size_t(t) * 9), vn9(size_t(t) * 9), vt6(size_t(t) * 6);
    std::vector<int32_t, default_init_alloc<int32_t>> mat(static_cast<size_t>(t));
    parallel_pieces(t, [&](long long ib, long long ie) {
        for (long long i = ib; i < ie; i++) {
            const FaceRec& f = s.faces[size_t(i)];
            for (int c = 0; c < 3; c++) {
                const double q[3] = {f.v[c].x, f.v[c].y, f.v[c].z}, n[3] = {f.vn[c].x, f.vn[c].y, f.vn[c].z};
                for (int a = 0; a < 3; a++) { v9[size_t(i) * 9 + c * 3 + a] = q[a]; vn9[size_t(i) * 9 + c * 3 + a] = n[a]; }
                vt6[size_t(i) * 6 + c * 2] = f.vt[c][0]; vt6[size_t(i) * 6 + c * 2 + 1] = f.vt[c][1];
            }
            mat[size_t(i)] = f.material;
        }
    });
    HIP_TRY(u->v9.upload(v9));
    HIP_TRY(u->vn9.upload(vn9));
    HIP_TRY(u->vt6.upload(vt6));
    HIP_TRY(u->nrm3.alloc(size_t(t) * 3));
    HIP_TRY(u->mat.upload(mat));
    HIP_TRY(u->leaf_of_face.alloc(size_t(t)));
    HIP_TRY(u->old_order.alloc(size_t(t)));
    HIP_TRY(u->moved.alloc(1));
    for (int a = 0; a < 3; a++) { u->morton_lo[a] = s.morton_lo[a]; u->morton_span[a] = s.morton_span[a]; }
    light_vertices(s, v9.data(), u->light_v);
    std::vector<int32_t> lf;
    for (const LightRec& l : s.lights) lf.insert(lf.end(), s.materials[l.material].faces.begin(), s.materials[l.material].faces.end());
    u->n_light_faces = int(lf.size());
    HIP_TRY(u->light_faces.upload(lf));
    HIP_TRY(u->light_buf.alloc(lf.size() * 9));
    d->upd = std::move(u);
    return MCPT_OK;
}

namespace {

// The refit's bottom-up schedule, once per hierarchy: the nodes in breadth-first order from the root are grouped by depth, and a child is
// one level below its parent.  With it the slot -> face table and the side array of exact boxes.
int make_schedule(mcpt_device* d)
{
    Update& u = *d->upd;
    const int n = d->fast_info.n_nodes, n_tris = d->fast_info.n_tris;
    std::vector<CwNode> nodes(static_cast<size_t>(n));
    if (n) HIP_TRY(hipMemcpy(nodes.data(), d->cw_nodes.get(), size_t(n) * sizeof(CwNode), hipMemcpyDeviceToHost));
    std::vector<int32_t> sched, depth(static_cast<size_t>(n), -1);
    std::vector<int> level_first;
    sched.reserve(size_t(n));
    if (n) { sched.push_back(0); depth[0] = 0; }
    for (size_t head = 0; head < sched.size(); head++) {
        const int32_t i = sched[head];
        if (depth[size_t(i)] == int(level_first.size())) level_first.push_back(int(head));
        for (int c = 0; c < 4; c++) {
            const int32_t r = nodes[size_t(i)].child[c];
            if (r >= 0 && r < n && depth[size_t(r)] < 0) { depth[size_t(r)] = depth[size_t(i)] + 1; sched.push_back(r); }
        }
    }
    level_first.push_back(int(sched.size()));
    // (into the device's record only once everything is there: a refit takes the presence of tri_faces for the presence of all of it)
    DevBuf<int32_t> d_sched, tri_faces, slots;
    DevBuf<double> node_box;
    HIP_TRY(d_sched.upload(sched));
    HIP_TRY(node_box.alloc(size_t(n) * 6));
    HIP_TRY(tri_faces.alloc(size_t(n_tris)));
    HIP_TRY(slots.alloc(size_t(n_tris)));
    HIP_TRY(device_tri_faces(d->fast_tris.get(), n_tris, tri_faces.get(), d->stream.get()));
    HIP_TRY(hipStreamSynchronize(d->stream.get()));
    u.sched = std::move(d_sched); u.node_box = std::move(node_box); u.slots = std::move(slots); u.level_first = std::move(level_first);
    u.tri_faces = std::move(tri_faces);
    return MCPT_OK;
}

// cost = sum over the non-empty child slots of (stored box's area x (1 for a node, triangle count for a leaf)) / the root's area, the
// root's box being the union of node 0's stored child boxes
int hierarchy_cost(mcpt_device* d, double* cost)
{
    *cost = 0;
    const int n = d->fast_info.n_nodes;
    if (n <= 0) return MCPT_OK;
    double sum = 0;
    HIP_TRY(device_cost_sum(d->cw_nodes.get(), n, &sum, d->stream.get()));
    CwNode root;
    HIP_TRY(hipMemcpy(&root, d->cw_nodes.get(), sizeof root, hipMemcpyDeviceToHost));
    double ext[3];
    for (int a = 0; a < 3; a++) {
        double lo = INFINITY, hi = -INFINITY;
        const double p = double(root.p[a]), sc = std::ldexp(1.0, int(root.e[a]));
        for (int c = 0; c < 4; c++) {
            if (root.child[c] == kFastEmpty) continue;
            lo = std::min(lo, p + double((root.qlo[a] >> (8 * c)) & 255u) * sc);
            hi = std::max(hi, p + double((root.qhi[a] >> (8 * c)) & 255u) * sc);
        }
        ext[a] = hi - lo;
    }
    const double area = ext[0] * ext[1] + ext[1] * ext[2] + ext[2] * ext[0];
    *cost = sum / area;
    return MCPT_OK;
}

// total_area, the running-sum cdf and cdf_sorted of every light as finish_scene makes them, the light triangles' new vertices, area0.
// The emitter faces' vertices are gathered on the GPU and only they come to the host; the serial running sum keeps finish_scene's bits.
int update_lights(mcpt_device* d)
{
    const Scene& s = d->scene->s;
    Update& u = *d->upd;
    if (s.lights.empty() || u.n_light_faces == 0) return MCPT_OK;
    std::vector<double> lv(size_t(u.n_light_faces) * 9);
    HIP_TRY(device_gather_faces(u.v9.get(), d->bi.t, u.light_faces.get(), u.n_light_faces, u.light_buf.get(), d->stream.get()));
    HIP_TRY(hipStreamSynchronize(d->stream.get()));
    HIP_TRY(hipMemcpy(lv.data(), u.light_buf.get(), lv.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (lv.size() == u.light_v.size() && std::memcmp(lv.data(), u.light_v.data(), lv.size() * sizeof(double)) == 0) return MCPT_OK;   // no emitter face moved
    size_t at = 0;                                  // lv runs light by light in material face order, as the loop below does
    std::vector<DLight> lights(s.lights.size());
    std::vector<DLightTri> ltris;
    std::vector<double> lcdf;
    for (size_t i = 0; i < s.lights.size(); i++) {
        const LightRec& l = s.lights[i];
        const MaterialRec& m = s.materials[l.material];
        DLight& dl = lights[i];
        dl.radiance[0] = l.radiance.x; dl.radiance[1] = l.radiance.y; dl.radiance[2] = l.radiance.z;
        dl.material = l.material; dl.ntri = int32_t(m.faces.size()); dl.first = int32_t(ltris.size());
        double total = 0;
        bool sorted = true;
        for (size_t j = 0; j < m.faces.size(); j++) {
            const FaceRec& old = s.faces[m.faces[j]];
            const double* p = lv.data() + at;
            at += 9;
            FaceRec f{};
            for (int c = 0; c < 3; c++) f.v[c] = Vec3{p[c * 3], p[c * 3 + 1], p[c * 3 + 2]};
            DLightTri q{};
            double *qv[3] = {q.v1, q.v2, q.v3}, *qn[3] = {q.vn1, q.vn2, q.vn3};
            for (int c = 0; c < 3; c++) {
                qv[c][0] = f.v[c].x; qv[c][1] = f.v[c].y; qv[c][2] = f.v[c].z;
                qn[c][0] = old.vn[c].x; qn[c][1] = old.vn[c].y; qn[c][2] = old.vn[c].z;
            }
            ltris.push_back(q);
            total += face_area(f);
            lcdf.push_back(total);
            if (!(total == total) || (j && !(lcdf[lcdf.size() - 1] >= lcdf[lcdf.size() - 2]))) sorted = false;
        }
        dl.total_area = total; dl.cdf_sorted = sorted ? 1 : 0;
    }
    HIP_TRY(hipMemcpy(d->lights.get(), lights.data(), lights.size() * sizeof(DLight), hipMemcpyHostToDevice));
    if (!ltris.empty()) {
        HIP_TRY(hipMemcpy(d->light_tris.get(), ltris.data(), ltris.size() * sizeof(DLightTri), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d->light_cdf.get(), lcdf.data(), lcdf.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    d->ds.area0 = lights[0].total_area;
    u.light_v.swap(lv);
    if (d->pick) {                                  // MCPT_LIGHTS_ONE with default weights: luminance x the new areas
        std::vector<double> areas;
        for (const DLight& l : lights) areas.push_back(l.total_area);
        if (const int rc = light_pick_refresh(d, areas.data())) return rc;
    }
    return MCPT_OK;
}

// Everything after the argument checks: d_v = the new vertices in HBM (the staging array itself when the host form has uploaded them)
int update_geometry(mcpt_device* d, const double* d_v, int32_t mode, mcpt_update_info* info, std::chrono::steady_clock::time_point t0)
{
    const Scene& s = d->scene->s;
    const int t = d->bi.t;
    hipStream_t st = d->stream.get();
    Update& u = *d->upd;
    mcpt_update_info out{};
    out.mode = mode;
    if (u.cost < 0) { if (const int rc = hierarchy_cost(d, &u.cost)) return rc; }       // (once: every later update leaves its cost_after here)
    out.cost_before = u.cost;

    d->geometry_failed = true;                      // from here on the arrays are between two geometries
    // ---- staging and the reference's structures
    if (d_v != u.v9.get()) HIP_TRY(hipMemcpyAsync(u.v9.get(), d_v, size_t(t) * 9 * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIP_TRY(device_face_normals(u.v9.get(), t, u.nrm3.get(), st));
    bool coords_ok = true;
    double lo[3], hi[3];
    HIP_TRY(device_vet_bounds(u.v9.get(), t, &coords_ok, lo, hi, st));
    if (s.morton_bounds)                            // the key domain follows the new vertices, as the loader derives it
        for (int a = 0; a < 3; a++) {
            u.morton_lo[a] = float(lo[a]);
            const float span = float(hi[a]) - u.morton_lo[a];
            u.morton_span[a] = span > 0.0f ? span : 1.0f;
        }
    HIP_TRY(hipMemcpyAsync(u.old_order.get(), d->d_order.get(), size_t(t) * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    const BuildInputs in{u.v9.get(), u.vn9.get(), u.vt6.get(), u.nrm3.get(), u.mat.get(), t, {u.morton_lo[0], u.morton_lo[1], u.morton_lo[2]},
                         {u.morton_span[0], u.morton_span[1], u.morton_span[2]}};
    HIP_TRY(device_build_reference(in, d->bi, d->nodes.get(), d->tris.get(), d->shade.get(), d->d_order.get(), st));
    HIP_TRY(device_count_differing(u.old_order.get(), d->d_order.get(), t, u.moved.get(), st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(&out.leaves_moved, u.moved.get(), sizeof(int32_t), hipMemcpyDeviceToHost));
    out.ms_reference = ms_since(t0);

    // ---- the culling hierarchy and the pre-test records
    mcpt_fast_info& fi = d->fast_info;
    double absmax = 0;
    if (mode == MCPT_UPDATE_REFIT) {
        if (!u.tri_faces) { if (const int rc = make_schedule(d)) return rc; }
        HIP_TRY(device_refit_slots(d->d_order.get(), t, u.tri_faces.get(), fi.n_tris, u.leaf_of_face.get(), u.slots.get(), st));
        HIP_TRY(device_gather_tris(d->tris.get(), u.slots.get(), fi.n_tris, d->fast_tris.get(), st));
        HIP_TRY(device_refit_levels(d->cw_nodes.get(), fi.n_nodes, u.sched.get(), u.level_first.data(), int(u.level_first.size()) - 1, d->fast_tris.get(), fi.n_tris,
                                    u.node_box.get(), st));
        HIP_TRY(device_tris_absmax(d->fast_tris.get(), fi.n_tris, &absmax, st));
        fi.enabled = fast_walk_enabled(fi, coords_ok, absmax) ? 1 : 0;       // (max_depth and cw_stack_need are the topology's)
        if (d->fast_pre) {
            HIP_TRY(device_build_pre(d->fast_tris.get(), fi.n_tris, absmax, d->fast_pre.get(), st));
            HIP_TRY(hipStreamSynchronize(st));
        }
    } else {
        u.tri_faces.reset(); u.sched.reset(); u.node_box.reset(); u.slots.reset(); u.level_first.clear();     // they describe the hierarchy that goes
        hipError_t copy_err = hipSuccess;
        const auto host_bvh = [&]() -> std::shared_ptr<const FastBvh> {
            // the host's SAH builder on a copy of the faces that is the device's own (the scene's cached hierarchy is another geometry's):
            // the one place where every vertex comes back to the host
            std::vector<double, default_init_alloc<double>> hv(size_t(t) * 9);
            std::vector<int32_t> order(static_cast<size_t>(t));
            copy_err = hipMemcpy(hv.data(), u.v9.get(), hv.size() * sizeof(double), hipMemcpyDeviceToHost);
            if (copy_err == hipSuccess) copy_err = hipMemcpy(order.data(), d->d_order.get(), size_t(t) * sizeof(int32_t), hipMemcpyDeviceToHost);
            if (copy_err != hipSuccess) return nullptr;
            std::vector<FaceRec> faces(static_cast<size_t>(t));
            for (size_t i = 0; i < size_t(t); i++)
                for (int c = 0; c < 3; c++) faces[i].v[c] = Vec3{hv[i * 9 + c * 3], hv[i * 9 + c * 3 + 1], hv[i * 9 + c * 3 + 2]};
            return private_fast_bvh(faces, order, d->knobs);
        };
        if (const int rc = build_culling_hierarchy(d, coords_ok, lo, hi, host_bvh, false, &absmax)) return rc;
        d->fast_pre.reset();
        if (const int rc = create_pre_test(d, absmax)) return rc;
    }
    DScene& S = d->ds;
    S.fast.cw = d->cw_nodes.get(); S.fast.tris = d->fast_tris.get(); S.fast.pre = d->fast_pre.get();
    S.fast.absmax = absmax; S.fast.enabled = fi.enabled;
    out.ms_hierarchy = ms_since(t0) - out.ms_reference;

    // ---- light tables
    if (const int rc = update_lights(d)) return rc;
    out.ms_tables = ms_since(t0) - out.ms_reference - out.ms_hierarchy;
    if (const int rc = hierarchy_cost(d, &out.cost_after)) return rc;
    u.cost = out.cost_after;
    d->geometry_failed = false;
    out.fast_enabled = fi.enabled;
    out.ms_total = ms_since(t0);
    if (info) *info = out;
    return MCPT_OK;
}

}  // namespace

// nothing of the device is in flight afterwards: both frame slots (a pipelined frame ends on the old geometry), the library's streams
int wait_for_frames(mcpt_device* d)
{
    HIP_TRY(hipSetDevice(d->ordinal));
    for (auto& f : d->slot) if (f.done) HIP_TRY(hipEventSynchronize(f.done.get()));
    HIP_TRY(hipStreamSynchronize(d->stream.get()));
    HIP_TRY(hipStreamSynchronize(d->look_stream.get()));
    return MCPT_OK;
}

int refit_geometry(mcpt_device* d, const double* d_v, mcpt_update_info* info)
{
    return update_geometry(d, d_v, MCPT_UPDATE_REFIT, info, std::chrono::steady_clock::now());
}

// a camera the frame cannot be formed from is refused, not rendered as NaN
int camera_check(const double eye[3], const double look_at[3], const double up[3], double fovy)
{
    const Vec3 e{eye[0], eye[1], eye[2]}, l{look_at[0], look_at[1], look_at[2]}, w{up[0], up[1], up[2]};
    const Vec3 dir = l - e, side = cross(dir, w);
    const double all = e.x + e.y + e.z + l.x + l.y + l.z + w.x + w.y + w.z + fovy;
    if (!std::isfinite(all) || !(fovy > 0.0 && fovy < 180.0) || !(norm(dir) > 0.0) || !(norm(w) > 0.0) || !(norm(side) > 0.0))
        return fail(MCPT_ERR_ARG, "camera: finite numbers, 0 < fovy < 180, eye != look_at and up not along the view direction");
    return MCPT_OK;
}

void camera_apply(mcpt_device* d, const double eye[3], const double look_at[3], const double up[3], double fovy)
{
    Scene c;                                        // camera_frame reads the camera and the frame size
    c.eye = Vec3{eye[0], eye[1], eye[2]}; c.look_at = Vec3{look_at[0], look_at[1], look_at[2]}; c.up = Vec3{up[0], up[1], up[2]};
    c.fovy = fovy; c.width = d->width; c.height = d->height;
    const CameraFrame cf = camera_frame(c);
    DCamera& cam = d->ds.cam;
    const Vec3 src[4] = {cf.eye, cf.start_point, cf.screen_pdx, cf.screen_pdy};
    double* dst[4] = {cam.eye, cam.start_point, cam.pdx, cam.pdy};
    for (int i = 0; i < 4; i++) { dst[i][0] = src[i].x; dst[i][1] = src[i].y; dst[i][2] = src[i].z; }
    d->cam_eye = c.eye; d->cam_look_at = c.look_at; d->cam_up = c.up; d->cam_fovy = fovy;
    d->dirs_ready = false;
    d->pos.reset();
}

namespace {

// what both forms check before anything is touched
int update_checks(mcpt_device* d, const double* v, int32_t mode)
{
    if (!d || !v) return fail(MCPT_ERR_ARG, "null argument");
    if (mode != MCPT_UPDATE_REFIT && mode != MCPT_UPDATE_REBUILD) return fail(MCPT_ERR_ARG, "unknown update mode");
    if (const int rc = require_device()) return rc;
    if (d->refs.load() > 1) return fail(MCPT_ERR_ARG, "a progressive frame of the device is alive: it is defined over one geometry and camera");
    if (const int rc = wait_for_frames(d)) return rc;
    if (const int rc = stage_faces(d)) return rc;
    if (const int rc = motion_home(d)) return rc;   // new vertices are a new key 0: the update's info compares with the old one
    return MCPT_OK;
}

}  // namespace

extern "C" {

int mcpt_device_update_vertices_device(mcpt_device* d, const double* d_v, int32_t mode, mcpt_update_info* info, void* stream)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (const int rc = update_checks(d, d_v, mode)) return rc;
    if (stream) HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
    const int rc = update_geometry(d, d_v, mode, info, t0);
    if (rc == MCPT_OK) motion_clear(d);             // the update has succeeded: a new key 0
    return rc;
}

// an upload into the staging array, then the device form
int mcpt_device_update_vertices(mcpt_device* d, const double* v, int32_t mode, mcpt_update_info* info)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (const int rc = update_checks(d, v, mode)) return rc;
    d->geometry_failed = true;                      // (the staging array is what mcpt_device_get_vertices reports)
    HIP_TRY(hipMemcpy(d->upd->v9.get(), v, size_t(d->bi.t) * 9 * sizeof(double), hipMemcpyHostToDevice));
    const int rc = update_geometry(d, d->upd->v9.get(), mode, info, t0);
    if (rc == MCPT_OK) motion_clear(d);             // the update has succeeded: a new key 0
    return rc;
}

int mcpt_device_get_vertices(mcpt_device* d, double* v)
{
    if (!d || !v) return fail(MCPT_ERR_ARG, "null argument");
    if (const int rc = require_device()) return rc;
    if (const int rc = motion_home(d)) return rc;
    const size_t t = size_t(d->bi.t);
    if (d->upd) {
        HIP_TRY(hipSetDevice(d->ordinal));
        HIP_TRY(hipMemcpy(v, d->upd->v9.get(), t * 9 * sizeof(double), hipMemcpyDeviceToHost));
        return MCPT_OK;
    }
    const Scene& s = d->scene->s;
    for (size_t i = 0; i < t; i++)
        for (int c = 0; c < 3; c++) { v[i * 9 + c * 3] = s.faces[i].v[c].x; v[i * 9 + c * 3 + 1] = s.faces[i].v[c].y; v[i * 9 + c * 3 + 2] = s.faces[i].v[c].z; }
    return MCPT_OK;
}

int mcpt_device_set_camera(mcpt_device* d, const double eye[3], const double look_at[3], const double up[3], double fovy)
{
    if (!d || !eye || !look_at || !up) return fail(MCPT_ERR_ARG, "null argument");
    if (const int rc = require_device()) return rc;
    if (d->refs.load() > 1) return fail(MCPT_ERR_ARG, "a progressive frame of the device is alive: it is defined over one geometry and camera");
    if (const int rc = camera_check(eye, look_at, up, fovy)) return rc;
    if (const int rc = wait_for_frames(d)) return rc;       // a frame in flight still reads the primary directions
    if (const int rc = motion_home(d)) return rc;           // a new camera is a new key 0: the geometry returns to the old one's first
    motion_clear(d);
    camera_apply(d, eye, look_at, up, fovy);
    return MCPT_OK;
}

int mcpt_device_get_camera(const mcpt_device* d, double eye[3], double look_at[3], double up[3], double* fovy)
{
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    if (const int rc = require_device()) return rc;
    const Vec3 src[3] = {d->cam_eye, d->cam_look_at, d->cam_up};
    double* dst[3] = {eye, look_at, up};
    for (int i = 0; i < 3; i++) if (dst[i]) { dst[i][0] = src[i].x; dst[i][1] = src[i].y; dst[i][2] = src[i].z; }
    if (fovy) *fovy = d->cam_fovy;
    return MCPT_OK;
}

}  // extern "C"
