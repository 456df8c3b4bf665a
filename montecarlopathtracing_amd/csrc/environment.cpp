// C ABI, the environment light (include/mcpt.h: mcpt_device_set_environment ... mcpt_read_pfm): validation, the sampling tables in fp64,
// their upload, the test seams and the PFM reader.  The kernels that use it are in env.hpp.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "handles.hpp"

using namespace mcpt;

int env_check(const mcpt_environment* e)
{
    if (!e) return MCPT_OK;
    if (e->width < 1 || e->height < 1) return fail(MCPT_ERR_ARG, "mcpt_environment: width and height must be >= 1");
    if (!e->rgb) return fail(MCPT_ERR_ARG, "mcpt_environment: null texels");
    if (e->flags != 0 || e->reserved != 0) return fail(MCPT_ERR_ARG, "mcpt_environment.flags and .reserved must be 0");
    if (!std::isfinite(e->scale) || !(e->scale > 0.0)) return fail(MCPT_ERR_ARG, "mcpt_environment.scale must be finite and > 0");
    const size_t n = size_t(e->width) * size_t(e->height) * 3;
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(e->rgb[i]) || !(e->rgb[i] >= 0.0f)) return fail(MCPT_ERR_ARG, "mcpt_environment: a texel is NaN, inf or negative");
    return MCPT_OK;
}

// The tables of mcpt.h, in its operation order, sequential sums left to right.
int env_make(const mcpt_environment* e, std::shared_ptr<EnvData>& out)
{
    auto env = std::make_shared<EnvData>();
    const int W = e->width, H = e->height;
    env->W = W; env->H = H; env->scale = e->scale;
    env->rgb.assign(e->rgb, e->rgb + size_t(W) * H * 3);
    const double pi = 3.141592653589793, two_pi = 6.283185307179586;
    std::vector<double> c(size_t(H) + 1), marg(static_cast<size_t>(H)), cond(size_t(W) * size_t(H));
    for (int i = 0; i <= H; i++) c[i] = std::cos(pi * double(i) / double(H));
    c[0] = 1.0; c[H] = -1.0;
    double run = 0.0;
    for (int i = 0; i < H; i++) {
        const double omega = ((c[i] - c[i + 1]) * two_pi) / double(W);
        double row = 0.0;
        for (int j = 0; j < W; j++) {
            const float* t = &env->rgb[(size_t(i) * W + j) * 3];
            const double lum = (0.2126 * double(t[0]) + 0.7152 * double(t[1])) + 0.0722 * double(t[2]);
            row += lum * omega;
            cond[size_t(i) * W + j] = row;
        }
        run += row;
        marg[i] = run;
    }
    env->Z = run;
    if (env->Z > 0.0) {
        HIP_TRY(env->d_rgb.alloc(env->rgb.size()));
        HIP_TRY(hipMemcpy(env->d_rgb.get(), env->rgb.data(), env->rgb.size() * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(env->d_c.upload(c));
        HIP_TRY(env->d_marg.upload(marg));
        HIP_TRY(env->d_cond.upload(cond));
        DEnv& D = env->denv;
        D.rgb = env->d_rgb.get(); D.c = env->d_c.get(); D.marg = env->d_marg.get(); D.cond = env->d_cond.get();
        D.W = W; D.H = H; D.scale = env->scale; D.Z = env->Z;
    }
    out = std::move(env);
    return MCPT_OK;
}

extern "C" {

int mcpt_device_set_environment(mcpt_device* d, const mcpt_environment* e)
{
    if (int rc = env_check(e)) return rc;
    if (const int rc = require_device()) return rc;
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    HIP_TRY(hipSetDevice(d->ordinal));
    std::shared_ptr<EnvData> env;
    if (e) {
        if (const int rc = env_make(e, env)) return rc;
    }
    HIP_TRY(hipDeviceSynchronize());           // (frames in flight may still read the tables being replaced)
    d->env = env;
    d->ds.env = env ? env->denv : DEnv{};
    return MCPT_OK;
}

int mcpt_device_get_environment(const mcpt_device* d, int32_t* width, int32_t* height, double* scale, double* Z)
{
    if (const int rc = require_device()) return rc;
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    const EnvData* e = d->env.get();
    if (width) *width = e ? e->W : 0;
    if (height) *height = e ? e->H : 0;
    if (scale) *scale = e ? e->scale : 0.0;
    if (Z) *Z = e ? e->Z : 0.0;
    return MCPT_OK;
}

int mcpt_environment_eval(mcpt_device* d, const double* dirs, int64_t n, double* rgb)
{
    if (!dirs || !rgb || n < 0) return fail(MCPT_ERR_ARG, "bad argument");
    if (const int rc = require_device()) return rc;
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    if (!env_on(d->ds.env)) return fail(MCPT_ERR_ARG, "the device has no active environment");
    if (n == 0) return MCPT_OK;
    HIP_TRY(hipSetDevice(d->ordinal));
    Staging S(d->stream.get());
    const double* d_dirs = nullptr;
    double* d_rgb = nullptr;
    if (const int rc = S.in(dirs, size_t(n) * 3, "the directions", d_dirs)) return rc;
    if (const int rc = S.out(rgb, size_t(n) * 3, "the directions' radiance", d_rgb)) return rc;
    launch_env_eval(d->ds.env, d_dirs, n, d_rgb, d->stream.get());
    return S.finish(launch_result());
}

int mcpt_environment_sample(mcpt_device* d, uint64_t seed, const int32_t* pix, const int32_t* k, int32_t depth, int64_t n, double* dirs, double* pdf,
                            double* rgb)
{
    if (!pix || !k || !dirs || !pdf || !rgb || n < 0 || depth < 0 || depth >= MCPT_MAX_DEPTH) return fail(MCPT_ERR_ARG, "bad argument");
    if (const int rc = require_device()) return rc;
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    if (!env_on(d->ds.env)) return fail(MCPT_ERR_ARG, "the device has no active environment");
    if (n == 0) return MCPT_OK;
    HIP_TRY(hipSetDevice(d->ordinal));
    std::vector<double> o(size_t(n) * 7);                   // the kernel's rows: direction, probability, radiance
    Staging S(d->stream.get());
    const int32_t *d_pix = nullptr, *d_k = nullptr;
    double* d_out = nullptr;
    if (const int rc = S.in(pix, size_t(n), "the pixels", d_pix)) return rc;
    if (const int rc = S.in(k, size_t(n), "the samples", d_k)) return rc;
    if (const int rc = S.out(o.data(), o.size(), "the samples' rows", d_out)) return rc;
    launch_env_sample(d->ds.env, seed, d_pix, d_k, depth, d->ds.num_lights, n, d_out, d->stream.get());
    if (const int rc = S.finish(launch_result())) return rc;
    for (int64_t i = 0; i < n; i++) {
        const double* r = &o[size_t(i) * 7];
        dirs[i * 3] = r[0]; dirs[i * 3 + 1] = r[1]; dirs[i * 3 + 2] = r[2];
        pdf[i] = r[3];
        rgb[i * 3] = r[4]; rgb[i * 3 + 1] = r[5]; rgb[i * 3 + 2] = r[6];
    }
    return MCPT_OK;
}

// "PF\n<w> <h>\n<scale>\n" + float32 RGB rows, bottom row first; a negative scale means little-endian (the only kind mcpt_write_pfm writes;
// a big-endian file is byte-swapped)
int mcpt_read_pfm(const char* file, int32_t* width, int32_t* height, float* rgb, int64_t cap)
{
    if (!file || !width || !height || (rgb && cap < 0)) return fail(MCPT_ERR_ARG, "bad argument");
    FILE* fp = std::fopen(file, "rb");
    if (!fp) return fail(MCPT_ERR_IO, std::string("cannot open ") + file);
    char magic[3] = {0, 0, 0};
    int w = 0, h = 0;
    double sc = 0.0;
    const bool head = std::fscanf(fp, "%2s %d %d %lf", magic, &w, &h, &sc) == 4 && std::fgetc(fp) != EOF;   // (one whitespace byte ends the header)
    if (!head || std::strcmp(magic, "PF") != 0 || w < 1 || h < 1 || sc == 0.0 || !std::isfinite(sc)) {
        std::fclose(fp);
        return fail(MCPT_ERR_PARSE, std::string("not a colour PFM: ") + file);
    }
    *width = w; *height = h;
    if (!rgb) { std::fclose(fp); return MCPT_OK; }
    const size_t n = size_t(w) * size_t(h) * 3;
    if (size_t(cap) < n) { std::fclose(fp); return fail(MCPT_ERR_ARG, "mcpt_read_pfm: rgb holds fewer than width * height * 3 floats"); }
    std::vector<float> row(size_t(w) * 3);
    for (int y = h - 1; y >= 0; y--) {
        if (std::fread(row.data(), sizeof(float), row.size(), fp) != row.size()) { std::fclose(fp); return fail(MCPT_ERR_PARSE, std::string("short PFM: ") + file); }
        if (sc > 0.0)
            for (float& v : row) { uint32_t u; std::memcpy(&u, &v, 4); u = __builtin_bswap32(u); std::memcpy(&v, &u, 4); }
        std::memcpy(rgb + size_t(y) * w * 3, row.data(), row.size() * sizeof(float));
    }
    std::fclose(fp);
    return MCPT_OK;
}

}  // extern "C"
