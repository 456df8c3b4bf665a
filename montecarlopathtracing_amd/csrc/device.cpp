// C ABI, device handles (include/mcpt.h: mcpt_device_*): a scene made resident on one GPU, stage by stage -- the reference's
// structures, materials and lights, the fast walk's culling hierarchy and its pre-test records, the workspaces -- what the device holds,
// read back, and the closest-hit queries of ray_intersect.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "build_kernels.hpp"
#include "handles.hpp"

using namespace mcpt;

int geometry_gate(const mcpt_device* d)
{
    return d->geometry_failed ? fail(MCPT_ERR_ARG, "geometry update failed: the device renders again after an update that succeeds") : MCPT_OK;
}

extern "C" {

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

}  // extern "C"

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
int build_culling_hierarchy(mcpt_device* d, bool coords_ok, const double lo[3], const double hi[3],
                            const std::function<std::shared_ptr<const FastBvh>()>& host_bvh, bool talk, double* absmax)
{
    const CreateClock clock{talk, std::chrono::steady_clock::now()};
    const int32_t build_mode = d->build_mode;
    mcpt_fast_info& fi = d->fast_info;
    if (build_mode == MCPT_BUILD_DEVICE_FAST || build_mode == MCPT_BUILD_DEVICE_SAH) {
        if (const int rc = build_hierarchy_on_device(d, lo, hi, build_mode == MCPT_BUILD_DEVICE_SAH, clock, absmax)) return rc;
    } else {
        // the SAH hierarchy built on the host from the leaf order (accel_build.cpp, shared by every device of the scene), its
        // permuted triangle copy gathered on the GPU
        const std::shared_ptr<const FastBvh> fb = host_bvh();
        if (!fb) return fail(MCPT_ERR_HIP, "culling hierarchy on the host: the faces could not be read");
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
    fi.enabled = fast_walk_enabled(fi, coords_ok, *absmax) ? 1 : 0;
    return MCPT_OK;
}

// ... of the scene the device is created from
static int create_hierarchy(mcpt_device* d, const mcpt_scene* h, const std::vector<int32_t>& order, const CreateClock& clock, double* absmax)
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
    return build_culling_hierarchy(d, coords_ok, lo, hi, [&]() { return shared_fast_bvh(h, order, d->knobs); }, clock.talk, absmax);
}

// The pre-test pays where the walk is bound by instruction issue, i.e. where nodes and triangles come out of L1 / L2 / the 256-MB
// Infinity Cache (cornell-box: 7.38 -> 7.25 ms per k_wf_trace launch; veach-mis and the 204 k-triangle interior alike).  On the
// 10 M-triangle scene the walk waits for memory, and a second dependent fetch per leaf (48-B record, then the 128-B record of a
// survivor) costs more than the skipped arithmetic saves: 6.90 vs 6.44 ms per launch.  So: records only for scenes of at most
// MCPT_PRE_TEST_MAX_TRIS triangles (default 2^20: ~200 B per triangle of nodes, records and triangles stay cache-resident).
int create_pre_test(mcpt_device* d, double absmax)
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
    d->cam_eye = s.eye; d->cam_look_at = s.look_at; d->cam_up = s.up; d->cam_fovy = s.fovy;
    const CameraFrame cf = camera_frame(s);
    put3(S.cam.eye, cf.eye); put3(S.cam.start_point, cf.start_point); put3(S.cam.pdx, cf.screen_pdx); put3(S.cam.pdy, cf.screen_pdy);
    S.cam.width = s.width; S.cam.height = s.height;
    d->width = s.width; d->height = s.height;
    HIP_TRY(d->dirs.alloc(size_t(s.width) * s.height * 3));
    return MCPT_OK;
}

extern "C" {

int mcpt_device_create_ex(const mcpt_scene* h, int32_t ordinal, int32_t build_mode, mcpt_device** out)
{
    if (!h || !out) return fail(MCPT_ERR_ARG, "null argument");
    *out = nullptr;
    if (build_mode != MCPT_BUILD_HOST && build_mode != MCPT_BUILD_DEVICE && build_mode != MCPT_BUILD_DEVICE_FAST && build_mode != MCPT_BUILD_DEVICE_SAH)
        return fail(MCPT_ERR_ARG, "bad build mode");
    const Scene& s = h->s;
    if (build_mode == MCPT_BUILD_HOST && !s.accel_built) return fail(MCPT_ERR_ARG, "scene has no host build; use MCPT_BUILD_DEVICE");
    int ndev = 0;
    if (const int rc = require_device(&ndev)) return rc;
    if (const int gate = runtime_gate()) return gate;          // kernels of one hipcc on another release's runtime: refused
    if (ordinal < 0 || ordinal >= ndev) return fail(MCPT_ERR_NO_DEVICE, "device ordinal out of range");
    HIP_TRY(hipSetDevice(ordinal));
    std::unique_ptr<mcpt_device, void (*)(mcpt_device*)> d(new mcpt_device, mcpt_device_free);
    d->ordinal = ordinal;
    d->build_mode = build_mode;
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
        (rc = create_hierarchy(d.get(), h, order, clock, &absmax)) || (rc = create_pre_test(d.get(), absmax)))
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
    if (const int rc = motion_home(d)) return rc;
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
    if (const int rc = motion_home(d)) return rc;
    HIP_TRY(hipMemcpy(leaf_to_face, d->d_order.get(), size_t(d->bi.t) * sizeof(int32_t), hipMemcpyDeviceToHost));
    return MCPT_OK;
}

int mcpt_device_fast_hierarchy(const mcpt_device* d, mcpt_fast_info* info, void* nodes, int32_t* tri_faces)
{
    static_assert(sizeof(CwNode) == 64, "mcpt.h documents 64-byte node records");
    if (!d || !info) return fail(MCPT_ERR_ARG, "null argument");
    if (const int rc = motion_home(const_cast<mcpt_device*>(d))) return rc;     // (the view is read-only; a motion frame's step is not what it shows)
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

// ------------------------------------------------------------------------------------------------ closest hit
int mcpt_trace_closest_device(mcpt_device* d, const double* d_rays, int64_t n, int32_t* d_face, double* d_t, double* d_p,
                              double* d_pn, void* stream)
{
    if (!d || (n > 0 && !d_rays) || n < 0) return fail(MCPT_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(d->ordinal));
    if (!d_face || !d_t || !d_p) return fail(MCPT_ERR_ARG, "d_face, d_t and d_p are required by the device form");
    if (const int rc = motion_home(d)) return rc;
    if (const int rc = geometry_gate(d)) return rc;
    launch_trace_closest(d->ds, d->trace_mode == MCPT_TRACE_FAST, d_rays, n, d_face, d_t, d_p, d_pn, d->aux_ctr.get(), d->aux_queue.get(), d->aux_slow_list.get(), d->slow_cap,
                         static_cast<hipStream_t>(stream), d->cfg);
    HIP_TRY(hipGetLastError());
    return MCPT_OK;
}

int mcpt_trace_closest(mcpt_device* d, const double* rays, int64_t n, int32_t* face, double* t, double* p, double* pn, mcpt_stats* stats)
{
    if (!d || (n > 0 && !rays) || n < 0) return fail(MCPT_ERR_ARG, "bad argument");
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (const int rc = motion_home(d)) return rc;
    if (const int rc = geometry_gate(d)) return rc;
    if (n == 0) return MCPT_OK;
    HIP_TRY(hipSetDevice(d->ordinal));
    const size_t sn = size_t(n);
    Staging S(d->stream.get());
    const double* d_rays = nullptr;
    int32_t* d_face = nullptr;
    double *d_t = nullptr, *d_p = nullptr, *d_pn = nullptr;
    // the launch requires d_face, d_t and d_p, so an absent one still gets room; d_pn may be null
    if (const int rc = S.in(rays, sn * 6, "the rays", d_rays)) return rc;
    if (const int rc = S.out(face, sn, "the rays' faces", d_face, Staging::kRoom)) return rc;
    if (const int rc = S.out(t, sn, "the rays' distances", d_t, Staging::kRoom)) return rc;
    if (const int rc = S.out(p, sn * 3, "the rays' hit points", d_p, Staging::kRoom)) return rc;
    if (const int rc = S.out(pn, sn * 3, "the rays' normals", d_pn)) return rc;
    return host_form(d, S, kNotReported, stats, [&](hipStream_t st) {
        launch_trace_closest(d->ds, d->trace_mode == MCPT_TRACE_FAST, d_rays, n, d_face, d_t, d_p, d_pn, d->aux_ctr.get(), d->aux_queue.get(),
                             d->aux_slow_list.get(), d->slow_cap, st, d->cfg);
    });
}

}  // extern "C"
