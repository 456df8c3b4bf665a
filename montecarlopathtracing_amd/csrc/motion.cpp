// C ABI, a device's motion (include/mcpt.h: motion blur): two keyframes resident on the GPU, the shutter's steps joined by the stages of a
// geometry update (update.cpp) on vertices blended on the GPU (build_kernels.hip: k_blend_keys), the camera blended on the host, and the
// return to key 0 for everything that is not a motion frame.  Every step is an update of a static scene: no trace or logic kernel knows
// about time.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>

#include "build_kernels.hpp"
#include "handles.hpp"

using namespace mcpt;

namespace {

using Motion = mcpt_device::Motion;

// (the library is built with -ffp-contract=off: the expressions below round as written)
double shutter_time(const mcpt_shutter& s, int j) { return s.open + (s.close - s.open) * ((double(j) + 0.5) / double(s.steps)); }
double blend(double a, double b, double u) { return a == b ? a : (1.0 - u) * a + u * b; }
int first_sample(int N, int K, int j) { return int((int64_t(j) * N + K - 1) / K); }        // the smallest k with (k * K) / N >= j

mcpt_camera_key camera_of(const mcpt_device* d)
{
    mcpt_camera_key c{};
    const Vec3 src[3] = {d->cam_eye, d->cam_look_at, d->cam_up};
    double* dst[3] = {c.eye, c.look_at, c.up};
    for (int i = 0; i < 3; i++) { dst[i][0] = src[i].x; dst[i][1] = src[i].y; dst[i][2] = src[i].z; }
    c.fovy = d->cam_fovy;
    return c;
}

// key 0's camera again, exactly as it was (the kernels' record is kept, not derived again)
void camera_home(mcpt_device* d)
{
    Motion& m = *d->motion;
    if (!m.has_camera) return;
    d->ds.cam = m.cam0;
    d->cam_eye = Vec3{m.c0.eye[0], m.c0.eye[1], m.c0.eye[2]};
    d->cam_look_at = Vec3{m.c0.look_at[0], m.c0.look_at[1], m.c0.look_at[2]};
    d->cam_up = Vec3{m.c0.up[0], m.c0.up[1], m.c0.up[2]};
    d->cam_fovy = m.c0.fovy;
    d->dirs_ready = false;
    d->pos.reset();
}

// the device at step j: nothing of it is in flight
int go_to_step(mcpt_device* d, int j, double& ms_updates, double& max_ratio)
{
    Motion& m = *d->motion;
    const double u = shutter_time(m.shutter, j);
    if (m.has_camera) {
        mcpt_camera_key c{};
        for (int a = 0; a < 3; a++) {
            c.eye[a] = blend(m.c0.eye[a], m.c1.eye[a], u);
            c.look_at[a] = blend(m.c0.look_at[a], m.c1.look_at[a], u);
            c.up[a] = blend(m.c0.up[a], m.c1.up[a], u);
        }
        c.fovy = blend(m.c0.fovy, m.c1.fovy, u);
        if (const int rc = camera_check(c.eye, c.look_at, c.up, c.fovy)) return rc;
        camera_apply(d, c.eye, c.look_at, c.up, c.fovy);
    }
    if (m.has_geometry && !(m.away && m.at_step == j)) {
        const auto t0 = std::chrono::steady_clock::now();
        HIP_TRY(device_blend_keys(m.v0.get(), m.v1.get(), d->bi.t, u, d->upd->v9.get(), d->stream.get()));
        m.away = true; m.at_step = -1;             // (the staging array is no longer key 0's, whatever the update below does)
        mcpt_update_info info{};
        if (const int rc = refit_geometry(d, d->upd->v9.get(), &info)) return rc;
        m.at_step = j;
        if (m.cost0 < 0) m.cost0 = info.cost_before;        // the first step ever leaves key 0's own hierarchy
        if (m.cost0 > 0) max_ratio = std::max(max_ratio, info.cost_after / m.cost0);
        ms_updates += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return MCPT_OK;
}

int set_motion(mcpt_device* d, const double* v_end, bool on_device, const mcpt_camera_key* camera_end, const mcpt_shutter* shutter, hipStream_t stream)
{
    if (const int rc = shutter_check(shutter)) return rc;
    if (camera_end) { if (const int rc = camera_check(camera_end->eye, camera_end->look_at, camera_end->up, camera_end->fovy)) return rc; }
    if (const int rc = require_device()) return rc;
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    if (d->refs.load() > 1) return fail(MCPT_ERR_ARG, "a progressive frame of the device is alive: it is defined over one motion");
    if (const int rc = geometry_gate(d)) return rc;
    HIP_TRY(hipSetDevice(d->ordinal));
    if (const int rc = wait_for_frames(d)) return rc;
    if (const int rc = motion_home(d)) return rc;            // key 0 of the new motion is what the device holds: the old motion's key 0
    std::unique_ptr<Motion> m(new Motion);
    m->shutter = *shutter;
    m->c0 = m->c1 = camera_of(d);
    m->cam0 = d->ds.cam;
    if (camera_end) { m->c1 = *camera_end; m->has_camera = true; }
    if (v_end) {
        if (const int rc = stage_faces(d)) return rc;
        const size_t n = size_t(d->bi.t) * 9;
        HIP_TRY(m->v0.alloc(n));
        HIP_TRY(m->v1.alloc(n));
        if (on_device && stream) HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipMemcpy(m->v0.get(), d->upd->v9.get(), n * sizeof(double), hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy(m->v1.get(), v_end, n * sizeof(double), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
        m->has_geometry = true;
        m->cost0 = d->upd->cost;                    // (< 0: no update has computed it yet; the first step's cost_before then)
    }
    d->motion = std::move(m);
    return MCPT_OK;
}

}  // namespace

int shutter_check(const mcpt_shutter* s)
{
    if (!s) return fail(MCPT_ERR_ARG, "null shutter");
    if (!(std::isfinite(s->open) && std::isfinite(s->close) && 0.0 <= s->open && s->open <= s->close && s->close <= 1.0))
        return fail(MCPT_ERR_ARG, "shutter: finite times with 0 <= open <= close <= 1");
    if (s->steps < 1) return fail(MCPT_ERR_ARG, "shutter: steps must be >= 1");
    if (s->reserved != 0) return fail(MCPT_ERR_ARG, "mcpt_shutter.reserved must be 0");
    return MCPT_OK;
}

void motion_clear(mcpt_device* d) { d->motion.reset(); }

int motion_home(mcpt_device* d)
{
    if (!d->motion || !d->motion->away) return MCPT_OK;
    Motion& m = *d->motion;
    HIP_TRY(hipSetDevice(d->ordinal));
    if (const int rc = wait_for_frames(d)) return rc;
    if (const int rc = refit_geometry(d, m.v0.get(), nullptr)) return rc;
    m.away = false; m.at_step = -1;
    return MCPT_OK;
}

int motion_passes(mcpt_device* d, int k0, int n, int N, hipStream_t st, const std::function<int(int, int)>& run)
{
    Motion& m = *d->motion;
    const int K = m.shutter.steps;
    m.info = mcpt_motion_info{};
    int rc = MCPT_OK;
    for (int lo = k0; lo < k0 + n && rc == MCPT_OK;) {
        const int j = int((int64_t(lo) * K) / N);
        const int cnt = std::min(k0 + n, first_sample(N, K, j + 1)) - lo;
        // the piece before, and whatever the caller enqueued, reads the geometry that goes
        const hipError_t idle = hipStreamSynchronize(st);
        if (idle != hipSuccess) { rc = fail(MCPT_ERR_HIP, hipGetErrorString(idle)); break; }
        if ((rc = wait_for_frames(d))) break;
        if ((rc = go_to_step(d, j, m.info.ms_updates, m.info.max_cost_ratio))) break;
        rc = run(lo, cnt);
        m.info.steps_run++;
        lo += cnt;
    }
    // (the common exit, after a failure as well: the stream idle, the camera at key 0)
    const hipError_t e = hipStreamSynchronize(st);
    camera_home(d);
    if (rc == MCPT_OK && e != hipSuccess) rc = fail(MCPT_ERR_HIP, hipGetErrorString(e));
    return rc;
}

extern "C" {

int mcpt_device_set_motion(mcpt_device* d, const double* v_end, const mcpt_camera_key* camera_end, const mcpt_shutter* shutter)
{
    return set_motion(d, v_end, false, camera_end, shutter, nullptr);
}

int mcpt_device_set_motion_device(mcpt_device* d, const double* d_v_end, const mcpt_camera_key* camera_end, const mcpt_shutter* shutter, void* stream)
{
    return set_motion(d, d_v_end, true, camera_end, shutter, static_cast<hipStream_t>(stream));
}

int mcpt_device_clear_motion(mcpt_device* d)
{
    if (const int rc = require_device()) return rc;
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    if (!d->motion) return MCPT_OK;
    if (d->refs.load() > 1) return fail(MCPT_ERR_ARG, "a progressive frame of the device is alive: it is defined over one motion");
    if (const int rc = motion_home(d)) return rc;
    motion_clear(d);
    return MCPT_OK;
}

int mcpt_device_get_motion(const mcpt_device* d, mcpt_shutter* shutter, int32_t* has_geometry, int32_t* has_camera, mcpt_camera_key* camera_end)
{
    if (const int rc = require_device()) return rc;
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    const Motion* m = d->motion.get();
    if (shutter) *shutter = m ? m->shutter : mcpt_shutter{};
    if (has_geometry) *has_geometry = m && m->has_geometry ? 1 : 0;
    if (has_camera) *has_camera = m && m->has_camera ? 1 : 0;
    if (camera_end) *camera_end = m ? m->c1 : camera_of(d);
    return MCPT_OK;
}

int mcpt_device_motion_info(const mcpt_device* d, mcpt_motion_info* out)
{
    if (!out) return fail(MCPT_ERR_ARG, "null argument");
    if (const int rc = require_device()) return rc;
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    *out = d->motion ? d->motion->info : mcpt_motion_info{};
    return MCPT_OK;
}

double mcpt_shutter_time(double open, double close, int32_t steps, int32_t j)
{
    const mcpt_shutter s{open, close, steps, 0};
    if (!(std::isfinite(open) && std::isfinite(close) && 0.0 <= open && open <= close && close <= 1.0) || steps < 1 || j < 0 || j >= steps) return NAN;
    return shutter_time(s, j);
}

int32_t mcpt_shutter_step(int32_t spp, int32_t steps, int32_t k)
{
    if (spp < 1 || steps < 1 || steps > spp || k < 0 || k >= spp) return -1;
    return int32_t((int64_t(k) * steps) / spp);
}

}  // extern "C"
