// C ABI, light sampling (include/mcpt.h: mcpt_device_set_light_sampling ... mcpt_light_pick_at): validation, the pick table and the light
// tree in fp64, their upload and the test seams.  The kernels that use them are in vertex.hpp (light_pick, light_pick_at, light_sample_one).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "handles.hpp"
#include "light_tree.hpp"

using namespace mcpt;

int light_sampling_check(const mcpt_light_sampling* ls)
{
    if (!ls) return MCPT_OK;
    if (ls->mode != MCPT_LIGHTS_ALL && ls->mode != MCPT_LIGHTS_ONE && ls->mode != MCPT_LIGHTS_TREE)
        return fail(MCPT_ERR_ARG, "mcpt_light_sampling.mode must be MCPT_LIGHTS_ALL, MCPT_LIGHTS_ONE or MCPT_LIGHTS_TREE");
    if (ls->num_weights < 0 || (ls->num_weights > 0) != (ls->weights != nullptr)) return fail(MCPT_ERR_ARG, "mcpt_light_sampling: num_weights and weights must go together");
    return MCPT_OK;
}

// The table of mcpt.h from the lights' radiances and areas (or the caller's weights), sequential sums left to right.  false: a weight
// is negative or not finite, or the caller's weights are all zero.
static bool pick_table(const std::vector<LightRec>& lights, const double* areas, const double* weights, std::vector<double>& cdf, std::vector<double>& pdf, int& last,
                       std::vector<double>* w_out = nullptr)
{
    const size_t n = lights.size();
    std::vector<double> w(n);
    if (weights) {
        for (size_t l = 0; l < n; l++) {
            if (!std::isfinite(weights[l]) || !(weights[l] >= 0.0)) return false;
            w[l] = weights[l];
        }
    } else {
        bool any = false;
        for (size_t l = 0; l < n; l++) {
            const Vec3& r = lights[l].radiance;
            const double lum = (0.2126 * r.x + 0.7152 * r.y) + 0.0722 * r.z;
            w[l] = lum * (areas ? areas[l] : lights[l].total_area);
            if (!std::isfinite(w[l]) || !(w[l] >= 0.0)) w[l] = 0.0;
            any = any || w[l] > 0.0;
        }
        if (!any) std::fill(w.begin(), w.end(), 1.0);
    }
    cdf.resize(n); pdf.resize(n);
    double run = 0.0;
    last = -1;
    for (size_t l = 0; l < n; l++) {
        run += w[l];
        cdf[l] = run;
        if (w[l] > 0.0) last = int(l);
    }
    if (last < 0 || !std::isfinite(run)) return false;
    for (size_t l = 0; l < n; l++) pdf[l] = w[l] / run;
    if (w_out) w_out->swap(w);
    return true;
}

// ---- the light tree of MCPT_LIGHTS_TREE
// box[l] = lo.xyz, hi.xyz: the exact min / max of the vertices of light l's triangles.  light_v: the emitter faces' vertices, light by light
// in material face order (an updated device's: mcpt_device::Update::light_v), or null for the scene's own.
static void light_boxes(const Scene& s, const double* light_v, std::vector<double>& box)
{
    box.assign(s.lights.size() * 6, 0.0);
    size_t at = 0;
    for (size_t l = 0; l < s.lights.size(); l++) {
        double* b = box.data() + l * 6;
        for (int a = 0; a < 3; a++) { b[a] = INFINITY; b[3 + a] = -INFINITY; }
        for (int32_t f : s.materials[s.lights[l].material].faces)
            for (int c = 0; c < 3; c++) {
                double q[3];
                if (light_v) { for (int a = 0; a < 3; a++) q[a] = light_v[at + size_t(c) * 3 + a]; }
                else { const Vec3& v = s.faces[size_t(f)].v[c]; q[0] = v.x; q[1] = v.y; q[2] = v.z; }
                for (int a = 0; a < 3; a++) { if (q[a] < b[a]) b[a] = q[a]; if (q[a] > b[3 + a]) b[3 + a] = q[a]; }
                if (c == 2) at += 9;
            }
    }
}

// Top-down, nodes in preorder (root 0, a node's left subtree right behind it): the lights of a node are split at the median of their box
// centres along the widest axis of those centres' bounds (the lowest axis among equals); ties are broken by light index; the left side
// gets the larger half.  The depth is ceil(log2 nl).
static int tree_node(const std::vector<double>& box, const std::vector<double>& w, std::vector<int>& idx, size_t b, size_t e, std::vector<DLightNode>& nodes)
{
    const int me = int(nodes.size());
    nodes.emplace_back();
    if (e - b == 1) {
        const int l = idx[b];
        DLightNode n{};
        for (int a = 0; a < 3; a++) { n.lo[a] = box[size_t(l) * 6 + a]; n.hi[a] = box[size_t(l) * 6 + 3 + a]; }
        n.w = w[size_t(l)]; n.left = n.right = ~l;
        nodes[size_t(me)] = n;
        return me;
    }
    auto centre = [&](int l, int a) { return (box[size_t(l) * 6 + a] + box[size_t(l) * 6 + 3 + a]) * 0.5; };
    int axis = 0;
    double widest = -1.0;
    for (int a = 0; a < 3; a++) {
        double lo = INFINITY, hi = -INFINITY;
        for (size_t i = b; i < e; i++) { const double c = centre(idx[i], a); if (c < lo) lo = c; if (c > hi) hi = c; }
        if (hi - lo > widest) { widest = hi - lo; axis = a; }
    }
    std::sort(idx.begin() + long(b), idx.begin() + long(e), [&](int x, int y) { const double cx = centre(x, axis), cy = centre(y, axis); return cx < cy || (cx == cy && x < y); });
    const size_t mid = b + (e - b + 1) / 2;
    const int left = tree_node(box, w, idx, b, mid, nodes), right = tree_node(box, w, idx, mid, e, nodes);
    DLightNode n{};
    const DLightNode &L = nodes[size_t(left)], &R = nodes[size_t(right)];
    for (int a = 0; a < 3; a++) { n.lo[a] = L.lo[a] < R.lo[a] ? L.lo[a] : R.lo[a]; n.hi[a] = L.hi[a] > R.hi[a] ? L.hi[a] : R.hi[a]; }
    n.w = L.w + R.w; n.left = left; n.right = right;
    nodes[size_t(me)] = n;
    return me;
}

static void tree_build(const std::vector<double>& box, const std::vector<double>& w, std::vector<DLightNode>& nodes)
{
    nodes.clear();
    std::vector<int> idx(w.size());
    for (size_t l = 0; l < idx.size(); l++) idx[l] = int(l);
    nodes.reserve(2 * w.size());
    tree_node(box, w, idx, 0, idx.size(), nodes);
}

// the probability of every light at the vertex (p, pn): the products light_pick_at forms on its way down, for every leaf
static void tree_pdf(const std::vector<DLightNode>& nodes, const double* p, const double* pn, double* pdf)
{
    std::vector<std::pair<int, double>> todo{{0, 1.0}};
    while (!todo.empty()) {
        const auto [n, q] = todo.back();
        todo.pop_back();
        const DLightNode& nd = nodes[size_t(n)];
        if (nd.left < 0) { pdf[~nd.left] = q; continue; }
        const double pL = light_tree_left(nodes[size_t(nd.left)], nodes[size_t(nd.right)], p[0], p[1], p[2], pn[0], pn[1], pn[2]);
        if (pL >= 1.0) { todo.push_back({nd.left, q}); todo.push_back({nd.right, 0.0}); }
        else { todo.push_back({nd.left, q * pL}); todo.push_back({nd.right, q * (1.0 - pL)}); }
    }
}

// d's table from its state (the caller's weights, or the lights' current areas: null = the scene's), copied into the device's two arrays
// (allocated by the first call: their size is the scene's light count); nothing in flight reads it
static int pick_upload(mcpt_device* d, LightPickData& k, const double* areas)
{
    const std::vector<LightRec>& lights = d->scene->s.lights;
    int last = -1;
    std::vector<double> w;
    if (!pick_table(lights, areas, k.own_weights ? k.weights.data() : nullptr, k.cdf, k.pdf, last, &w)) return fail(MCPT_ERR_ARG, "light weights: negative, not finite or all zero");
    std::vector<double> inv(k.pdf.size());
    for (size_t l = 0; l < inv.size(); l++) inv[l] = k.pdf[l] > 0.0 ? 1.0 / k.pdf[l] : 0.0;
    if (!k.d_cdf) { HIP_TRY(k.d_cdf.alloc(k.cdf.size())); HIP_TRY(k.d_inv.alloc(inv.size())); }
    HIP_TRY(hipMemcpy(k.d_cdf.get(), k.cdf.data(), k.cdf.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(k.d_inv.get(), inv.data(), inv.size() * sizeof(double), hipMemcpyHostToDevice));
    k.dpick = DLightPick{};
    k.nodes.clear();
    if (k.mode != MCPT_LIGHTS_ALL && lights.size() >= 2) {          // (none or one light: the mode changes nothing)
        k.dpick.cdf = k.d_cdf.get(); k.dpick.inv_pdf = k.d_inv.get(); k.dpick.Z = k.cdf.back(); k.dpick.last = last;
        if (k.mode == MCPT_LIGHTS_TREE) {                           // boxes from the light triangles as they are now
            std::vector<double> box;
            light_boxes(d->scene->s, d->upd ? d->upd->light_v.data() : nullptr, box);
            tree_build(box, w, k.nodes);
            if (!k.d_nodes) HIP_TRY(k.d_nodes.alloc(k.nodes.size()));
            HIP_TRY(hipMemcpy(k.d_nodes.get(), k.nodes.data(), k.nodes.size() * sizeof(DLightNode), hipMemcpyHostToDevice));
            k.dpick.nodes = k.d_nodes.get();
        }
    }
    return MCPT_OK;
}

// what mcpt_device_set_light_sampling refuses about ls on a scene of nl lights, beyond light_sampling_check: the count and the weights
int light_weights_check(const mcpt_light_sampling* ls, size_t nl)
{
    if (!ls || ls->num_weights == 0) return MCPT_OK;
    if (size_t(ls->num_weights) != nl) return fail(MCPT_ERR_ARG, "mcpt_light_sampling.num_weights must be the scene's light count");
    bool any = false;
    for (int32_t l = 0; l < ls->num_weights; l++) {
        if (!std::isfinite(ls->weights[l]) || !(ls->weights[l] >= 0.0)) return fail(MCPT_ERR_ARG, "light weights: negative, not finite or all zero");
        any = any || ls->weights[l] > 0.0;
    }
    return any ? MCPT_OK : fail(MCPT_ERR_ARG, "light weights: negative, not finite or all zero");
}

int light_pick_refresh(mcpt_device* d, const double* areas)
{
    if (!d->pick || (d->pick->own_weights && d->pick->mode != MCPT_LIGHTS_TREE)) return MCPT_OK;   // (the tree's boxes follow the emitters whatever the weights)
    if (const int rc = pick_upload(d, *d->pick, areas)) return rc;
    d->ds.pick = d->pick->dpick;
    return MCPT_OK;
}

extern "C" {

int mcpt_scene_light_pick_table(const mcpt_scene* h, const double* weights, double* cdf, double* pdf)
{
    if (!h || !cdf || !pdf) return fail(MCPT_ERR_ARG, "null argument");
    if (h->s.lights.empty()) return fail(MCPT_ERR_ARG, "the scene has no lights");
    std::vector<double> c, p;
    int last = -1;
    if (!pick_table(h->s.lights, nullptr, weights, c, p, last)) return fail(MCPT_ERR_ARG, "light weights: negative, not finite or all zero");
    std::memcpy(cdf, c.data(), c.size() * sizeof(double));
    std::memcpy(pdf, p.data(), p.size() * sizeof(double));
    return MCPT_OK;
}

// the tree of the scene's own lights under `weights` (null: the default ones); MCPT_ERR_ARG as mcpt_scene_light_pick_table, or fewer than two lights
static int scene_tree(const mcpt_scene* h, const double* weights, std::vector<DLightNode>& nodes)
{
    if (!h) return fail(MCPT_ERR_ARG, "null argument");
    if (h->s.lights.size() < 2) return fail(MCPT_ERR_ARG, "a scene of fewer than two lights holds no light tree");
    std::vector<double> c, p, w, box;
    int last = -1;
    if (!pick_table(h->s.lights, nullptr, weights, c, p, last, &w)) return fail(MCPT_ERR_ARG, "light weights: negative, not finite or all zero");
    light_boxes(h->s, nullptr, box);
    tree_build(box, w, nodes);
    return MCPT_OK;
}

int mcpt_scene_light_tree(const mcpt_scene* h, const double* weights, int32_t* n_nodes, void* out)
{
    if (!n_nodes) return fail(MCPT_ERR_ARG, "null argument");
    std::vector<DLightNode> nodes;
    if (const int rc = scene_tree(h, weights, nodes)) return rc;
    *n_nodes = int32_t(nodes.size());
    if (out) std::memcpy(out, nodes.data(), nodes.size() * sizeof(DLightNode));
    return MCPT_OK;
}

int mcpt_scene_light_tree_pdf(const mcpt_scene* h, const double* weights, const double* p, const double* pn, int64_t n, double* pdf)
{
    if (n < 0 || (n > 0 && (!p || !pn || !pdf))) return fail(MCPT_ERR_ARG, "bad argument");
    std::vector<DLightNode> nodes;
    if (const int rc = scene_tree(h, weights, nodes)) return rc;
    const size_t nl = h->s.lights.size();
    for (int64_t i = 0; i < n; i++) tree_pdf(nodes, p + i * 3, pn + i * 3, pdf + size_t(i) * nl);
    return MCPT_OK;
}

int mcpt_device_set_light_sampling(mcpt_device* d, const mcpt_light_sampling* ls)
{
    if (int rc = light_sampling_check(ls)) return rc;
    if (const int rc = require_device()) return rc;
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    const size_t nl = d->scene->s.lights.size();
    if (const int rc = light_weights_check(ls, nl)) return rc;
    if (const int rc = motion_home(d)) return rc;              // (the default weights are key 0's areas)
    HIP_TRY(hipSetDevice(d->ordinal));
    std::shared_ptr<LightPickData> k;
    if (ls && ls->mode != MCPT_LIGHTS_ALL) {
        k = std::make_shared<LightPickData>();
        k->mode = ls->mode;
        k->own_weights = ls->num_weights > 0;
        if (k->own_weights) k->weights.assign(ls->weights, ls->weights + ls->num_weights);
        if (nl > 0) {
            std::vector<double> areas;
            if (d->upd && !k->own_weights) {                       // an updated device: the areas its light records hold now
                std::vector<DLight> cur(nl);
                HIP_TRY(hipDeviceSynchronize());
                HIP_TRY(hipMemcpy(cur.data(), d->lights.get(), nl * sizeof(DLight), hipMemcpyDeviceToHost));
                for (const DLight& l : cur) areas.push_back(l.total_area);
            }
            if (const int rc = pick_upload(d, *k, areas.empty() ? nullptr : areas.data())) return rc;
        }
    }
    HIP_TRY(hipDeviceSynchronize());           // (frames in flight may still read the table being replaced)
    d->pick = k;
    d->ds.pick = k ? k->dpick : DLightPick{};
    return MCPT_OK;
}

int mcpt_device_get_light_sampling(const mcpt_device* d, int32_t* mode, double* pdf)
{
    if (const int rc = require_device()) return rc;
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    if (mode) *mode = d->pick ? d->pick->mode : MCPT_LIGHTS_ALL;
    if (pdf) {
        const size_t nl = d->scene->s.lights.size();
        if (d->pick && d->pick->pdf.size() == nl) std::memcpy(pdf, d->pick->pdf.data(), nl * sizeof(double));
        else for (size_t l = 0; l < nl; l++) pdf[l] = 1.0;      // MCPT_LIGHTS_ALL: every light, every vertex
    }
    return MCPT_OK;
}

int mcpt_light_pick(mcpt_device* d, uint64_t seed, const int32_t* pix, const int32_t* k, int32_t depth, int64_t n, int32_t* light, double* pdf)
{
    if (!pix || !k || !light || !pdf || n < 0 || depth < 0 || depth >= MCPT_MAX_DEPTH) return fail(MCPT_ERR_ARG, "bad argument");
    if (const int rc = require_device()) return rc;
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    if (!pick_on(d->ds.pick)) return fail(MCPT_ERR_ARG, "the device does not pick lights (MCPT_LIGHTS_ALL, or a scene of fewer than two lights)");
    if (tree_on(d->ds.pick)) return fail(MCPT_ERR_ARG, "under MCPT_LIGHTS_TREE the pick depends on the vertex: mcpt_light_pick_at");
    if (n == 0) return MCPT_OK;
    HIP_TRY(hipSetDevice(d->ordinal));
    Staging S(d->stream.get());
    const int32_t *d_pix = nullptr, *d_k = nullptr;
    int32_t* d_light = nullptr;
    if (const int rc = S.in(pix, size_t(n), "the pixels", d_pix)) return rc;
    if (const int rc = S.in(k, size_t(n), "the samples", d_k)) return rc;
    if (const int rc = S.out(light, size_t(n), "the picked lights", d_light)) return rc;
    launch_light_pick(d->ds, seed, d_pix, d_k, depth, n, d_light, d->stream.get());
    if (const int rc = S.finish(launch_result())) return rc;
    for (int64_t i = 0; i < n; i++) pdf[i] = d->pick->pdf[size_t(light[i])];
    return MCPT_OK;
}

int mcpt_light_pick_at(mcpt_device* d, uint64_t seed, const int32_t* pix, const int32_t* k, int32_t depth, const double* p, const double* pn, int64_t n,
                       int32_t* light, double* pdf)
{
    if (!pix || !k || !p || !pn || !light || !pdf || n < 0 || depth < 0 || depth >= MCPT_MAX_DEPTH) return fail(MCPT_ERR_ARG, "bad argument");
    if (const int rc = require_device()) return rc;
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    if (!tree_on(d->ds.pick)) return fail(MCPT_ERR_ARG, "the device does not pick lights by tree (MCPT_LIGHTS_TREE on a scene of two or more lights)");
    if (n == 0) return MCPT_OK;
    HIP_TRY(hipSetDevice(d->ordinal));
    Staging S(d->stream.get());
    const int32_t *d_pix = nullptr, *d_k = nullptr;
    const double *d_p = nullptr, *d_pn = nullptr;
    int32_t* d_light = nullptr;
    double* d_pdf = nullptr;
    if (const int rc = S.in(pix, size_t(n), "the pixels", d_pix)) return rc;
    if (const int rc = S.in(k, size_t(n), "the samples", d_k)) return rc;
    if (const int rc = S.in(p, size_t(n) * 3, "the vertices", d_p)) return rc;
    if (const int rc = S.in(pn, size_t(n) * 3, "the vertices' normals", d_pn)) return rc;
    if (const int rc = S.out(light, size_t(n), "the picked lights", d_light)) return rc;
    if (const int rc = S.out(pdf, size_t(n), "the picks' probabilities", d_pdf)) return rc;
    launch_light_pick_at(d->ds, seed, d_pix, d_k, depth, d_p, d_pn, n, d_light, d_pdf, d->stream.get());
    return S.finish(launch_result());
}

}  // extern "C"
