// C ABI, output and render_scene (include/mcpt.h): the PNG / PFM writers of imshow, checkpoints of a frame and the identity they carry, the
// JPEG decoder, and render_scene(path, filename, N) of the reference -- one call from the scene files to the written picture, on one GPU
// or several, in one go, in checkpointed partitions or progressively.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "handles.hpp"
#include "jpeg_decoder.hpp"

using namespace mcpt;

extern "C" {

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
// An active environment (env: the device's, null or inactive: none) is mixed in the same way, after the lens: its size, scale and texels.
// So is light sampling that picks (pick: the device's; null, or a scene of fewer than two lights, where the mode changes no bit: nothing),
// last: the mode and the table's probabilities.
static uint64_t frame_tag(const Scene& s, const mcpt_lens* l, const EnvData* env, const LightPickData* pick)
{
    uint64_t h = scene_tag(s);
    auto mix = [&](const void* p, size_t n) { const unsigned char* b = static_cast<const unsigned char*>(p); for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; } };
    if (l && lens_active(*l)) {
        const char tag[] = "lens";
        const int64_t flags = l->flags;
        const double focus = l->focus_distance > 0.0 ? l->focus_distance : 0.0;     // (every F <= 0 is the same lens)
        mix(tag, 4); mix(&flags, sizeof flags); mix(&l->aperture, sizeof(double)); mix(&focus, sizeof focus);
    }
    if (env && env->Z > 0.0) {
        const char tag[] = "envm";
        const int64_t wh[2] = {env->W, env->H};
        mix(tag, 4); mix(wh, sizeof wh); mix(&env->scale, sizeof(double)); mix(env->rgb.data(), env->rgb.size() * sizeof(float));
    }
    if (pick && pick_on(pick->dpick)) {
        const char tag[] = "lpck";
        const int64_t mode = pick->mode;
        mix(tag, 4); mix(&mode, sizeof mode); mix(pick->pdf.data(), pick->pdf.size() * sizeof(double));
        if (tree_on(pick->dpick)) mix(pick->nodes.data(), pick->nodes.size() * sizeof(DLightNode));      // MCPT_LIGHTS_TREE: the node bytes too
    }
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
// guided (may be null) receives mcpt_progressive_denoise_guided's image with all defaults; saovs (may be null) the sample AOVs of the default G
// (depth in all channels; coverage: ns/G, ne/G, nm/G).
struct SceneAovs { std::vector<double> albedo, normal, depth, material; };
struct SceneSampleAovs { std::vector<double> albedo, normal, depth, coverage; };
static int render_scene_progressive(mcpt_device* dev, const mcpt_render_params& rp, const mcpt_render_scene_options& o, bool talk, std::vector<double>& img,
                                    std::vector<double>* err, std::vector<int32_t>* counts, std::vector<double>* denoised, SceneAovs* aovs,
                                    std::vector<double>* guided, SceneSampleAovs* saovs, int& rendered, mcpt_stats& local)
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
        int n = mcpt_progressive_next_pass(rp.spp, mcpt_progressive_done(pr), remaining, rate);
        if (adaptive && mcpt_progressive_done(pr) == 0) n = std::min(rp.spp, o.adaptive_min_spp);
        if (n <= 0 || (adaptive && mcpt_progressive_active(pr) == 0)) break;
        const auto ts = clk::now();
        const int64_t listed = mcpt_progressive_active(pr);
        mcpt_stats one{};
        if ((rc = mcpt_progressive_step(pr, n, &one))) break;
        rate = std::chrono::duration<double>(clk::now() - ts).count() / n;
        if (adaptive) rate = listed > 0 ? rate * double(mcpt_progressive_active(pr)) / double(listed) : 0.0;
        add_counts(local, one);
        local.ms_trace += one.ms_trace; local.ms_total += one.ms_total;
        measured = false;
        if (o.noise_target > 0 && !adaptive) {
            if ((rc = mcpt_progressive_noise(pr, &nz))) break;
            measured = true;
            if (nz.rel_error <= o.noise_target) break;
        }
    }
    if (rc == MCPT_OK && talk && !measured) rc = mcpt_progressive_noise(pr, &nz);
    if (rc == MCPT_OK) {
        rendered = mcpt_progressive_done(pr);
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
    if (rc == MCPT_OK && guided) {
        guided->assign(img.size(), 0.0);
        rc = mcpt_progressive_denoise_guided(pr, nullptr, nullptr, guided->data());
    }
    if (rc == MCPT_OK && saovs) {
        const size_t px = img.size() / 3;
        std::vector<int32_t> cnt(px * 3, 0);
        std::vector<double> depth(px, 0.0);
        saovs->albedo.assign(img.size(), 0.0);
        saovs->normal.assign(img.size(), 0.0);
        rc = mcpt_progressive_sample_aovs(pr, 0, cnt.data(), depth.data(), saovs->normal.data(), saovs->albedo.data());
        saovs->depth.resize(img.size());
        saovs->coverage.resize(img.size());
        const double G = double(std::min<int>(rp.spp, MCPT_GUIDE_SAMPLES));
        for (size_t i = 0; i < px; i++)
            for (size_t c = 0; c < 3; c++) { saovs->depth[3 * i + c] = depth[i]; saovs->coverage[3 * i + c] = double(cnt[3 * i + c]) / G; }
    }
    if (rc == MCPT_OK && talk) std::printf("progressive: %d of %d samples per pixel, relative error %.4g\n", mcpt_progressive_done(pr), rp.spp, nz.rel_error);
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
    return mcpt_render_scene_env(path, filename, spp, opt, opt_bytes, lens, nullptr, 1.0, stats);
}

int mcpt_render_scene_env(const char* path, const char* filename, int32_t spp, const mcpt_render_scene_options* opt, int64_t opt_bytes,
                          const mcpt_lens* lens, const char* environment_pfm, double environment_scale, mcpt_stats* stats)
{
    return mcpt_render_scene_motion(path, filename, spp, opt, opt_bytes, lens, environment_pfm, environment_scale, nullptr, nullptr, nullptr, stats);
}

// every render_scene entry point ends here (light_sampling == null: MCPT_LIGHTS_ALL)
static int render_scene_impl(const char* path, const char* filename, int32_t spp, const mcpt_render_scene_options* opt, int64_t opt_bytes,
                             const mcpt_lens* lens, const char* environment_pfm, double environment_scale, const char* end_obj,
                             const char* end_camera, const mcpt_shutter* shutter, const mcpt_light_sampling* light_sampling,
                             const mcpt_display_params* display, mcpt_stats* stats);

int mcpt_render_scene_motion(const char* path, const char* filename, int32_t spp, const mcpt_render_scene_options* opt, int64_t opt_bytes,
                             const mcpt_lens* lens, const char* environment_pfm, double environment_scale, const char* end_obj,
                             const char* end_camera, const mcpt_shutter* shutter, mcpt_stats* stats)
{
    return render_scene_impl(path, filename, spp, opt, opt_bytes, lens, environment_pfm, environment_scale, end_obj, end_camera, shutter, nullptr, nullptr, stats);
}

int mcpt_render_scene_lights(const char* path, const char* filename, int32_t spp, const mcpt_render_scene_options* opt, int64_t opt_bytes,
                             const mcpt_lens* lens, const char* environment_pfm, double environment_scale, const mcpt_light_sampling* light_sampling,
                             mcpt_stats* stats)
{
    return mcpt_render_scene_display(path, filename, spp, opt, opt_bytes, lens, environment_pfm, environment_scale, light_sampling, nullptr, stats);
}

int mcpt_render_scene_display(const char* path, const char* filename, int32_t spp, const mcpt_render_scene_options* opt, int64_t opt_bytes,
                              const mcpt_lens* lens, const char* environment_pfm, double environment_scale, const mcpt_light_sampling* light_sampling,
                              const mcpt_display_params* display, mcpt_stats* stats)
{
    return render_scene_impl(path, filename, spp, opt, opt_bytes, lens, environment_pfm, environment_scale, nullptr, nullptr, nullptr, light_sampling,
                             display, stats);
}

static int render_scene_impl(const char* path, const char* filename, int32_t spp, const mcpt_render_scene_options* opt, int64_t opt_bytes,
                             const mcpt_lens* lens, const char* environment_pfm, double environment_scale, const char* end_obj,
                             const char* end_camera, const mcpt_shutter* shutter, const mcpt_light_sampling* light_sampling,
                             const mcpt_display_params* display, mcpt_stats* stats)
{
    if (!path || !filename || spp <= 0 || opt_bytes < 0 || (opt_bytes > 0 && !opt)) return fail(MCPT_ERR_ARG, "bad argument");
    if (int drc = display_check(display)) return drc;
    if (display && (display->flags & MCPT_DISPLAY_RGBA)) return fail(MCPT_ERR_ARG, "render_scene writes RGB pictures: MCPT_DISPLAY_RGBA is refused");
    if (int lrc = lens_check(lens)) return lrc;
    if (int src = light_sampling_check(light_sampling)) return src;
    if (shutter) { if (int src = shutter_check(shutter)) return src; }
    if (!shutter && (end_obj || end_camera)) return fail(MCPT_ERR_ARG, "an end .obj or .camera needs a shutter");
    if (shutter && shutter->steps > spp) return fail(MCPT_ERR_ARG, "the shutter has more steps than the frame has samples per pixel");
    // the environment map is read and checked before anything else is read or written
    std::vector<float> env_rgb;
    mcpt_environment env{};
    if (environment_pfm) {
        int32_t ew = 0, eh = 0;
        if (int erc = mcpt_read_pfm(environment_pfm, &ew, &eh, nullptr, 0)) return erc;
        env_rgb.resize(size_t(ew) * size_t(eh) * 3);
        if (int erc = mcpt_read_pfm(environment_pfm, &ew, &eh, env_rgb.data(), int64_t(env_rgb.size()))) return erc;
        env.width = ew; env.height = eh; env.rgb = env_rgb.data(); env.scale = environment_scale;
        if (int erc = env_check(&env)) return erc;
    }
    mcpt_render_scene_options o{};
    if (opt) std::memcpy(&o, opt, std::min<size_t>(size_t(opt_bytes), sizeof o));
    const bool talk = !o.quiet;
    // a noise target, a time budget or the error image: the frame goes through a progressive handle (one GPU, no checkpoint)
    const bool adaptive = o.adaptive_min_spp > 0;
    const bool progressive = o.noise_target > 0 || o.time_budget_s > 0 || (o.output_flags & (MCPT_OUT_ERROR_PFM | MCPT_OUT_DENOISED | MCPT_OUT_AOV_PFM | MCPT_OUT_DENOISED_SAMPLES | MCPT_OUT_SAMPLE_AOV_PFM)) ||
                             adaptive;
    if (o.noise_target < 0 || o.time_budget_s < 0 || std::isnan(o.noise_target) || std::isnan(o.time_budget_s))
        return fail(MCPT_ERR_ARG, "noise_target and time_budget_s must be >= 0");
    if (o.adaptive_min_spp < 0 || o.adaptive_min_spp == 1 || (adaptive && (!(std::isfinite(o.abs_target) && o.abs_target >= 0.0) || std::isinf(o.noise_target))))
        return fail(MCPT_ERR_ARG, "adaptive_min_spp must be 0 or >= 2, the targets finite and >= 0");
    if (progressive && (o.checkpoint || o.num_devices != 0))
        return fail(MCPT_ERR_ARG, "a noise target, a time budget, an adaptive frame, MCPT_OUT_ERROR_PFM, MCPT_OUT_DENOISED, MCPT_OUT_AOV_PFM, "
                                  "MCPT_OUT_DENOISED_SAMPLES or MCPT_OUT_SAMPLE_AOV_PFM renders on one GPU without a checkpoint");
    if ((o.output_flags & (MCPT_OUT_DENOISED | MCPT_OUT_DENOISED_SAMPLES)) && spp < 2)
        return fail(MCPT_ERR_ARG, "MCPT_OUT_DENOISED and MCPT_OUT_DENOISED_SAMPLES need N >= 2 (a variance estimate)");
    if (shutter && (o.checkpoint || o.num_devices != 0 || adaptive ||
                    (o.output_flags & (MCPT_OUT_DENOISED | MCPT_OUT_AOV_PFM | MCPT_OUT_DENOISED_SAMPLES | MCPT_OUT_SAMPLE_AOV_PFM))))
        return fail(MCPT_ERR_ARG, "a motion frame renders on one GPU without a checkpoint, and neither adaptively nor with MCPT_OUT_DENOISED, MCPT_OUT_AOV_PFM or "
                                  "their sample-guided forms");
    // (the steps are contiguous sample ranges: a frame stopped at k < N would show the first part of the shutter only)
    if (shutter && (o.noise_target > 0 || o.time_budget_s > 0))
        return fail(MCPT_ERR_ARG, "a motion frame renders all its samples: a noise target or a time budget would stop it inside the shutter");
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    mcpt_scene* sc = nullptr;
    int rc = mcpt_scene_load_ex(path, filename, o.load_flags, &sc);
    if (rc) return rc;
    if (o.width > 0 && o.height > 0) mcpt_scene_set_resolution(sc, o.width, o.height);
    const Scene& s = sc->s;
    // key 1 of the motion is read and compared with the scene before a device is made or anything is written
    std::vector<double> v_end;
    mcpt_camera_key cam_end{};
    if (shutter) {
        std::string merr;
        if (end_obj) rc = load_end_positions(s, end_obj, o.load_flags, v_end, merr);
        if (rc == MCPT_OK && end_camera) rc = load_end_camera(end_camera, cam_end, merr);
        if (rc) { mcpt_scene_free(sc); return fail(rc, merr); }
    }
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
    if (rc == MCPT_OK && environment_pfm) rc = many ? mcpt_multi_set_environment(multi, &env) : mcpt_device_set_environment(dev, &env);
    if (rc == MCPT_OK && light_sampling) rc = many ? mcpt_multi_set_light_sampling(multi, light_sampling) : mcpt_device_set_light_sampling(dev, light_sampling);
    if (rc == MCPT_OK && shutter) rc = mcpt_device_set_motion(dev, end_obj ? v_end.data() : nullptr, end_camera ? &cam_end : nullptr, shutter);
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
    std::vector<double> guided;
    SceneSampleAovs saovs;
    if (progressive) {
        rc = render_scene_progressive(dev, rp, o, talk, img, (o.output_flags & MCPT_OUT_ERROR_PFM) ? &err_img : nullptr, adaptive ? &counts : nullptr,
                                      (o.output_flags & MCPT_OUT_DENOISED) ? &denoised : nullptr, (o.output_flags & MCPT_OUT_AOV_PFM) ? &aovs : nullptr,
                                      (o.output_flags & MCPT_OUT_DENOISED_SAMPLES) ? &guided : nullptr,
                                      (o.output_flags & MCPT_OUT_SAMPLE_AOV_PFM) ? &saovs : nullptr, rendered, local);
    } else if (!o.checkpoint) {
        rc = many ? mcpt_multi_render(multi, &rp, img.data(), &local) : mcpt_render(dev, &rp, img.data(), &local);
    } else {
        // the frame in `parts` tile partitions, saved after each; partitions a matching checkpoint already holds are skipped
        const int parts = o.checkpoint_parts > 0 ? o.checkpoint_parts : 8;
        std::vector<uint8_t> done(size_t(parts), 0);
        const uint64_t tag = frame_tag(s, lens, dev->env.get(), dev->pick.get());
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
            add_counts(local, one);
            local.ms_trace += one.ms_trace; local.ms_total += one.ms_total;
            done[size_t(part)] = 1;
            rc = checkpoint_save(o.checkpoint, img.data(), s.width, s.height, spp, o.seed, tag, parts, done.data(), cerr);
            if (rc) rc = fail(rc, cerr);
        }
    }
    const auto t2 = clk::now();
    if (rc == MCPT_OK) {
        if (talk) std::printf("Phase 2(ray tracing) = %.3f ms\n", std::chrono::duration<double, std::milli>(t2 - t1).count());
        std::vector<uint8_t> rgb(img.size());
        // a frame's picture: imshow's bytes, or -- with display parameters -- the display transform's (the frame is on the host by now)
        const auto picture = [&](const std::vector<double>& frame) {
            return display ? mcpt_display_host(frame.data(), int64_t(frame.size() / 3), display, rgb.data(), nullptr)
                           : mcpt_quantize_rgb8(frame.data(), int64_t(frame.size()), rgb.data());
        };
        rc = picture(img);
        const std::string prefix = o.output_prefix ? std::string(o.output_prefix) : std::string("../result/") + filename;
        const std::string stem = prefix + "-SPP" + std::to_string(rendered);            // imshow, MTPC.cpp:17-20 (a progressive frame stopped early: its own count)
        if (rc == MCPT_OK)
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
            rc = picture(denoised);
            const std::string dn = stem + ".denoised";
            if (rc == MCPT_OK) rc = (o.output_flags & MCPT_OUT_PNG_DEFLATE) ? mcpt_write_png_deflate((dn + ".png").c_str(), rgb.data(), s.width, s.height)
                                                          : mcpt_write_png((dn + ".png").c_str(), rgb.data(), s.width, s.height);
            if (rc == MCPT_OK && (o.output_flags & MCPT_OUT_PFM)) rc = mcpt_write_pfm((dn + ".pfm").c_str(), denoised.data(), s.width, s.height);
        }
        if (rc == MCPT_OK && (o.output_flags & MCPT_OUT_AOV_PFM)) {
            const std::pair<const char*, const std::vector<double>*> files[] = {
                {".albedo.pfm", &aovs.albedo}, {".normal.pfm", &aovs.normal}, {".depth.pfm", &aovs.depth}, {".material.pfm", &aovs.material}};
            for (const auto& f : files)
                if (rc == MCPT_OK) rc = mcpt_write_pfm((stem + f.first).c_str(), f.second->data(), s.width, s.height);
        }
        if (rc == MCPT_OK && !guided.empty()) {
            rc = picture(guided);
            const std::string dn = stem + ".denoised-samples";
            if (rc == MCPT_OK) rc = (o.output_flags & MCPT_OUT_PNG_DEFLATE) ? mcpt_write_png_deflate((dn + ".png").c_str(), rgb.data(), s.width, s.height)
                                                          : mcpt_write_png((dn + ".png").c_str(), rgb.data(), s.width, s.height);
            if (rc == MCPT_OK && (o.output_flags & MCPT_OUT_PFM)) rc = mcpt_write_pfm((dn + ".pfm").c_str(), guided.data(), s.width, s.height);
        }
        if (rc == MCPT_OK && (o.output_flags & MCPT_OUT_SAMPLE_AOV_PFM)) {
            const std::pair<const char*, const std::vector<double>*> files[] = {
                {".s-albedo.pfm", &saovs.albedo}, {".s-normal.pfm", &saovs.normal}, {".s-depth.pfm", &saovs.depth}, {".coverage.pfm", &saovs.coverage}};
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
