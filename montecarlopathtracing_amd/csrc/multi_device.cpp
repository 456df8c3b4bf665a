// generateImg on several GPUs of one node behind the C ABI (mcpt_multi_*): one host thread per GPU, scene resident on every GPU,
// tiles dealt by mcpt_render_params.rank/world, end-of-frame exchange of compact pixel buffers into the first GPU's HBM over
// xGMI -- hipMemcpyPeerAsync by default, RCCL send/recv on request.  The reference has nothing like it (one OpenMP process,
// MTPC/pathTracing.cpp:303); this is what lets render_scene(path, filename, N) of MTPC/MTPC.cpp:35 use the whole node without
// a Python launcher.  Built on the library's public entry points, two pack/unpack kernels and the partition and statistics helpers of
// handles.hpp.
#include <hip/hip_runtime_api.h>

#include <dlfcn.h>

#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "handles.hpp"
#include "rccl_loader.hpp"          // loaded when MCPT_GATHER_RCCL is asked for

using mcpt::DevBuf;
using mcpt::Event;

namespace {

// A rank's buffers live on two GPUs: free_lists and mcpt_multi_free release each group with reset() while its device is current.
struct Rank {
    int ordinal = 0;
    mcpt_device* dev = nullptr;
    mcpt::Stream stream;
    DevBuf<double> d_frame;             // this rank's full-size frame (only its own pixels are written); rank 0's is THE frame
    DevBuf<int32_t> d_pixels;           // its pixel list, on its GPU
    DevBuf<double> d_compact;           // [n][3] on its GPU
    int64_t n = 0;
    // on devices[0]:
    DevBuf<double> d_stage;             // [n][3] where the compact buffer lands
    DevBuf<int32_t> d_pixels0;          // the same pixel list on devices[0]
    mcpt_stats stats{};
    int rc = MCPT_OK;
    std::string err;
    Event ev_start, ev_rendered;        // on the rank's stream: before its render / after its render (timing report)
    float render_ms = 0;
};

// One long-lived host thread per GPU (ranks 1..n-1; rank 0 works on the caller's thread): a frame hands each of them one job and
// waits for all.  Threads started per frame would pay their creation and the runtime's per-thread set-up inside every frame.
struct Workers {
    std::mutex mu;
    std::condition_variable cv_job, cv_done;
    std::function<void(int)> job;
    uint64_t generation = 0;
    int pending = 0;
    bool quit = false;
    std::vector<std::thread> threads;

    void start(int n_ranks)
    {
        for (int r = 1; r < n_ranks; r++)
            threads.emplace_back([this, r]() {
                uint64_t seen = 0;
                for (;;) {
                    std::function<void(int)> fn;
                    {
                        std::unique_lock<std::mutex> lk(mu);
                        cv_job.wait(lk, [&] { return quit || generation != seen; });
                        if (quit) return;
                        seen = generation;
                        fn = job;
                    }
                    fn(r);
                    {
                        std::lock_guard<std::mutex> lk(mu);
                        if (--pending == 0) cv_done.notify_all();
                    }
                }
            });
    }
    // fn(r) for every rank; rank 0 on the calling thread
    void run(const std::function<void(int)>& fn)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            job = fn; pending = int(threads.size()); generation++;
        }
        cv_job.notify_all();
        fn(0);
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return pending == 0; });
    }
    void stop()
    {
        { std::lock_guard<std::mutex> lk(mu); quit = true; }
        cv_job.notify_all();
        for (std::thread& t : threads) t.join();
        threads.clear();
    }
};

}  // namespace

struct mcpt_multi {
    const mcpt_scene* scene = nullptr;
    int width = 0, height = 0;
    int gather = MCPT_GATHER_PEER;
    int part_key[2] = {-1, -1};         // tile shape the pixel lists were made for ({-1,-1}: none)
    std::vector<Rank> ranks;
    Rccl rccl;
    std::vector<ncclComm_t> comms;
    Event ev0, ev1, ev_gather;          // on devices[0]'s stream: frame start, frame end, its own render done
    float gather_ms = 0;                // last frame: from rank 0's render being done to the last unpack (what the exchange adds)
    Workers workers;
};

static void free_lists(mcpt_multi* m)
{
    for (Rank& r : m->ranks) {
        (void)hipSetDevice(r.ordinal);
        r.d_pixels.reset();
        r.d_compact.reset();
        (void)hipSetDevice(m->ranks[0].ordinal);
        r.d_stage.reset();
        r.d_pixels0.reset();
        r.n = 0;
    }
}

// pixel lists of every rank for this tile shape, on the rank's GPU and on devices[0]
static int prepare_lists(mcpt_multi* m, const mcpt_render_params* p)
{
    const int key[2] = {p->tile_w, p->tile_h};
    if (m->ranks[0].d_pixels && std::memcmp(key, m->part_key, sizeof key) == 0) return MCPT_OK;
    free_lists(m);
    m->part_key[0] = m->part_key[1] = -1;       // whatever fails below, no list of this handle counts as valid
    const int world = int(m->ranks.size());
    for (int r = 0; r < world; r++) {
        Rank& R = m->ranks[size_t(r)];
        mcpt_render_params q = *p;
        q.rank = r; q.world = world;
        std::vector<int32_t> pix;
        if (const int rc = owned_pixels(m->width, m->height, &q, pix)) return rc;
        R.n = int64_t(pix.size());
        if (pix.empty()) pix.push_back(0);          // (a rank without pixels still gets buffers of one entry)
        HIP_TRY(hipSetDevice(R.ordinal));
        HIP_TRY(R.d_pixels.upload(pix));
        if (r > 0) {
            HIP_TRY(R.d_compact.alloc(pix.size() * 3));
            HIP_TRY(hipSetDevice(m->ranks[0].ordinal));
            HIP_TRY(R.d_stage.alloc(pix.size() * 3));
            HIP_TRY(R.d_pixels0.upload(pix));
        }
    }
    std::memcpy(m->part_key, key, sizeof key);
    return MCPT_OK;
}

extern "C" {

void mcpt_multi_free(mcpt_multi* m)
{
    if (!m) return;
    m->workers.stop();
    if (!m->ranks.empty()) free_lists(m);
    for (size_t i = 0; i < m->comms.size(); i++)
        if (m->comms[i] && m->rccl.CommDestroy) { (void)hipSetDevice(m->ranks[i].ordinal); (void)m->rccl.CommDestroy(m->comms[i]); }
    for (Rank& r : m->ranks) {
        (void)hipSetDevice(r.ordinal);
        r.d_frame.reset();
        r.ev_start.reset();
        r.ev_rendered.reset();
        r.stream.reset();
        if (r.dev) mcpt_device_free(r.dev);
    }
    m->ev0.reset();
    m->ev1.reset();
    m->ev_gather.reset();
    if (m->rccl.lib) dlclose(m->rccl.lib);
    delete m;
}

int mcpt_multi_num_devices(const mcpt_multi* m) { return m ? int(m->ranks.size()) : 0; }

// the same lens on every GPU of the group (mcpt_device_set_lens checks it; the first refusal leaves every device as it was)
int mcpt_multi_set_lens(mcpt_multi* m, const mcpt_lens* lens)
{
    mcpt_lens prev{};
    if (m && !m->ranks.empty()) (void)mcpt_device_get_lens(m->ranks[0].dev, &prev);
    if (!m) return mcpt_device_set_lens(nullptr, lens);       // the device entry point's checks and refusal of a null handle
    for (Rank& r : m->ranks) {
        const int rc = mcpt_device_set_lens(r.dev, lens);
        if (rc != MCPT_OK) {
            for (Rank& q : m->ranks) (void)mcpt_device_set_lens(q.dev, &prev);
            return rc;
        }
    }
    return MCPT_OK;
}

// the same environment on every GPU of the group (each device copies the texels; the first refusal clears it on every device)
int mcpt_multi_set_environment(mcpt_multi* m, const mcpt_environment* e)
{
    if (!m) return mcpt_device_set_environment(nullptr, e);   // the device entry point's checks and refusal of a null handle
    for (Rank& r : m->ranks) {
        const int rc = mcpt_device_set_environment(r.dev, e);
        if (rc) {
            for (Rank& q : m->ranks) (void)mcpt_device_set_environment(q.dev, nullptr);
            return rc;
        }
    }
    return MCPT_OK;
}

// the same light sampling on every GPU of the group.  The argument is checked against the scene before any device is touched: a call that
// is refused for its argument leaves every device as it was (a device that fails afterwards is a HIP error: the group goes back to ALL)
int mcpt_multi_set_light_sampling(mcpt_multi* m, const mcpt_light_sampling* ls)
{
    if (!m || m->ranks.empty()) return mcpt_device_set_light_sampling(nullptr, ls);   // the device entry point's checks and refusal of a null handle
    if (const int rc = light_sampling_check(ls)) return rc;
    if (const int rc = light_weights_check(ls, m->ranks[0].dev->scene->s.lights.size())) return rc;
    for (Rank& r : m->ranks) {
        const int rc = mcpt_device_set_light_sampling(r.dev, ls);
        if (rc) {
            for (Rank& q : m->ranks) (void)mcpt_device_set_light_sampling(q.dev, nullptr);
            return rc;
        }
    }
    return MCPT_OK;
}

// the same geometry on every GPU of the group, one device after the other (a device that fails refuses to render until an update succeeds)
int mcpt_multi_update_vertices(mcpt_multi* m, const double* v, int32_t mode, mcpt_update_info* info)
{
    if (!m) return mcpt_device_update_vertices(nullptr, v, mode, info);       // the device entry point's refusal of a null handle
    for (size_t i = 0; i < m->ranks.size(); i++)
        if (const int rc = mcpt_device_update_vertices(m->ranks[i].dev, v, mode, i == 0 ? info : nullptr)) return rc;
    return MCPT_OK;
}

int mcpt_multi_set_camera(mcpt_multi* m, const double eye[3], const double look_at[3], const double up[3], double fovy)
{
    if (!m) return mcpt_device_set_camera(nullptr, eye, look_at, up, fovy);
    for (Rank& r : m->ranks)
        if (const int rc = mcpt_device_set_camera(r.dev, eye, look_at, up, fovy)) return rc;
    return MCPT_OK;
}

int mcpt_multi_create(const mcpt_scene* scene, const int32_t* devices, int32_t num_devices, int32_t build_mode, int32_t gather, mcpt_multi** out)
{
    if (!scene || !out) return fail(MCPT_ERR_ARG, "null argument");
    *out = nullptr;
    if (gather != MCPT_GATHER_PEER && gather != MCPT_GATHER_RCCL) return fail(MCPT_ERR_ARG, "unknown gather mode");
    int visible = 0;
    if (const int rc = require_device(&visible)) return rc;
    std::vector<int32_t> ord;
    if (!devices || num_devices <= 0) {
        const int n = num_devices > 0 ? num_devices : visible;
        for (int i = 0; i < n; i++) ord.push_back(i);
    } else ord.assign(devices, devices + num_devices);
    for (int32_t o : ord) if (o < 0 || o >= visible) return fail(MCPT_ERR_NO_DEVICE, "device ordinal out of range");
    if (gather == MCPT_GATHER_RCCL) {
        std::vector<int32_t> u = ord;
        std::sort(u.begin(), u.end());
        if (std::adjacent_find(u.begin(), u.end()) != u.end()) return fail(MCPT_ERR_ARG, "MCPT_GATHER_RCCL needs distinct device ordinals");
    }
    mcpt_scene_info info;
    int rc = mcpt_scene_get_info(scene, &info);
    if (rc) return rc;
    std::unique_ptr<mcpt_multi, void (*)(mcpt_multi*)> m(new mcpt_multi, mcpt_multi_free);
    m->scene = scene; m->width = info.width; m->height = info.height; m->gather = gather;
    m->ranks.resize(ord.size());
    for (size_t i = 0; i < ord.size(); i++) m->ranks[i].ordinal = ord[i];
    // one thread per GPU: upload + (device) build of the scene, the rank's frame and stream
    const size_t frame_bytes = size_t(info.width) * info.height * 3 * sizeof(double);
    auto setup = [&](Rank& R) {
        R.rc = mcpt_device_create_ex(scene, R.ordinal, build_mode, &R.dev);
        if (R.rc) { R.err = mcpt_last_error(); return; }
        hipError_t e = hipSetDevice(R.ordinal);
        if (e == hipSuccess) e = create(R.stream, hipStreamCreateWithFlags, hipStreamNonBlocking);
        if (e == hipSuccess) e = R.d_frame.alloc_bytes(frame_bytes);
        if (e == hipSuccess) e = hipMemset(R.d_frame.get(), 0, frame_bytes);
        if (e == hipSuccess) e = create(R.ev_start, hipEventCreate);
        if (e == hipSuccess) e = create(R.ev_rendered, hipEventCreate);
        if (e != hipSuccess) { R.rc = MCPT_ERR_HIP; R.err = std::string("multi-device setup: ") + hipGetErrorString(e); }
    };
    {
        std::vector<std::thread> pool;
        for (size_t i = 1; i < m->ranks.size(); i++) pool.emplace_back(setup, std::ref(m->ranks[i]));
        setup(m->ranks[0]);
        for (std::thread& t : pool) t.join();
    }
    for (Rank& R : m->ranks) if (R.rc) return fail(R.rc, R.err);
    // peer access towards devices[0] where the hardware offers it (copies fall back to staging otherwise)
    for (size_t i = 1; i < m->ranks.size(); i++) {
        const int a = m->ranks[i].ordinal, b = m->ranks[0].ordinal;
        if (a == b) continue;
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, a, b) == hipSuccess && can) {
            (void)hipSetDevice(a);
            const hipError_t e = hipDeviceEnablePeerAccess(b, 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
        }
    }
    HIP_TRY(hipSetDevice(m->ranks[0].ordinal));
    HIP_TRY(create(m->ev0, hipEventCreate));
    HIP_TRY(create(m->ev1, hipEventCreate));
    HIP_TRY(create(m->ev_gather, hipEventCreate));
    m->workers.start(int(m->ranks.size()));
    if (gather == MCPT_GATHER_RCCL) {
        std::string err;
        const auto needed = [](const Rccl& r) { return r.CommInitAll && r.CommDestroy && r.GroupStart && r.GroupEnd && r.Send && r.Recv && r.GetErrorString; };
        if (!m->rccl.load(err, needed, mcpt::rccl_library())) return fail(MCPT_ERR_IO, err);
        m->comms.assign(ord.size(), nullptr);
        std::vector<int> devlist(ord.begin(), ord.end());
        const ncclResult_t r = m->rccl.CommInitAll(m->comms.data(), int(devlist.size()), devlist.data());
        if (r != ncclSuccess) return fail(MCPT_ERR_HIP, std::string("ncclCommInitAll: ") + m->rccl.GetErrorString(r));
    }
    *out = m.release();
    return MCPT_OK;
}

int mcpt_multi_render_device(mcpt_multi* m, const mcpt_render_params* p, double** d_img, mcpt_stats* stats)
{
    if (!m || !p || !d_img || p->spp <= 0) return fail(MCPT_ERR_ARG, "bad argument");
    *d_img = nullptr;
    if (stats) std::memset(stats, 0, sizeof *stats);
    int rc = prepare_lists(m, p);
    if (rc) return rc;
    const int world = int(m->ranks.size());
    Rank& R0 = m->ranks[0];
    HIP_TRY(hipSetDevice(R0.ordinal));
    HIP_TRY(hipEventRecord(m->ev0.get(), R0.stream.get()));
    const bool rccl = m->gather == MCPT_GATHER_RCCL && world > 1;
    const bool keep = (p->flags & MCPT_RENDER_KEEP_STATS) != 0 && !(p->flags & MCPT_RENDER_MEGAKERNEL);
    // one thread per GPU: render the rank's tiles, pack them, (peer mode) send them to devices[0]
    auto work = [&](int r) {
        Rank& R = m->ranks[size_t(r)];
        mcpt_render_params q = *p;
        q.rank = r; q.world = world;
        R.rc = MCPT_OK; R.err.clear();
        hipError_t e = hipSetDevice(R.ordinal);
        if (e == hipSuccess) e = hipEventRecord(R.ev_start.get(), R.stream.get());
        if (e != hipSuccess) { R.rc = MCPT_ERR_HIP; R.err = std::string("multi-device render: ") + hipGetErrorString(e); return; }
        // MCPT_RENDER_KEEP_STATS: the ranks' statistics stay on their devices (no read-back, no event queries inside the frame) until
        // mcpt_multi_collect_stats; one frame at a time all the same (MCPT_RENDER_PIPELINE is not passed on)
        q.flags &= ~MCPT_RENDER_PIPELINE;
        R.rc = mcpt_render_device(R.dev, &q, R.d_frame.get(), keep ? nullptr : &R.stats, R.stream.get());
        if (R.rc) { R.err = mcpt_last_error(); return; }
        e = hipSetDevice(R.ordinal);
        if (e == hipSuccess) e = hipEventRecord(R.ev_rendered.get(), R.stream.get());
        if (e == hipSuccess && r == 0) e = hipEventRecord(m->ev_gather.get(), R.stream.get());
        if (e == hipSuccess && r > 0 && R.n > 0) {
            mcpt::launch_pack_pixels(R.d_frame.get(), R.d_pixels.get(), R.n, R.d_compact.get(), R.stream.get());
            e = hipGetLastError();
            if (e == hipSuccess && !rccl)
                e = hipMemcpyPeerAsync(R.d_stage.get(), R0.ordinal, R.d_compact.get(), R.ordinal, size_t(R.n) * 3 * sizeof(double), R.stream.get());
        }
        if (e == hipSuccess && !rccl) e = hipStreamSynchronize(R.stream.get());
        if (e != hipSuccess) { R.rc = MCPT_ERR_HIP; R.err = std::string("multi-device render: ") + hipGetErrorString(e); }
    };
    m->workers.run(work);
    for (Rank& R : m->ranks) if (R.rc) return fail(R.rc, R.err);
    if (rccl) {
        // every rank's send and rank 0's receives as ONE group: each send is ordered after the rank's render + pack on its stream,
        // the receives after rank 0's render on its stream
        ncclResult_t nr = m->rccl.GroupStart();
        for (int r = 1; r < world && nr == ncclSuccess; r++) {
            Rank& R = m->ranks[size_t(r)];
            if (R.n <= 0) continue;
            nr = m->rccl.Send(R.d_compact.get(), size_t(R.n) * 3, ncclDouble, 0, m->comms[size_t(r)], R.stream.get());
            if (nr == ncclSuccess) nr = m->rccl.Recv(R.d_stage.get(), size_t(R.n) * 3, ncclDouble, r, m->comms[0], R0.stream.get());
        }
        const ncclResult_t ge = m->rccl.GroupEnd();
        if (nr == ncclSuccess) nr = ge;
        if (nr != ncclSuccess) return fail(MCPT_ERR_HIP, std::string("RCCL gather: ") + m->rccl.GetErrorString(nr));
        for (int r = 1; r < world; r++) { HIP_TRY(hipSetDevice(m->ranks[size_t(r)].ordinal)); HIP_TRY(hipStreamSynchronize(m->ranks[size_t(r)].stream.get())); }
    }
    HIP_TRY(hipSetDevice(R0.ordinal));
    for (int r = 1; r < world; r++) {
        Rank& R = m->ranks[size_t(r)];
        mcpt::launch_unpack_pixels(R.d_stage.get(), R.d_pixels0.get(), R.n, R0.d_frame.get(), R0.stream.get());
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(m->ev1.get(), R0.stream.get()));
    HIP_TRY(hipStreamSynchronize(R0.stream.get()));
    if (stats && !keep) {
        for (const Rank& R : m->ranks) {
            add_counts(*stats, R.stats);
            stats->ms_trace = std::max(stats->ms_trace, R.stats.ms_trace);
        }
        float ms = 0;
        (void)hipEventElapsedTime(&ms, m->ev0.get(), m->ev1.get());      // rank 0's stream from before its render to after the last unpack
        stats->ms_total = ms;
    }
    m->gather_ms = 0;
    (void)hipEventElapsedTime(&m->gather_ms, m->ev_gather.get(), m->ev1.get());
    for (Rank& R : m->ranks) {
        R.render_ms = 0;
        (void)hipSetDevice(R.ordinal);
        if (hipEventSynchronize(R.ev_rendered.get()) == hipSuccess) (void)hipEventElapsedTime(&R.render_ms, R.ev_start.get(), R.ev_rendered.get());
    }
    (void)hipGetLastError();
    (void)hipSetDevice(R0.ordinal);
    *d_img = R0.d_frame.get();
    return MCPT_OK;
}

// what the last frame's parts took (HIP events on each rank's own stream): render_ms[num_devices] (may be NULL), *gather_ms (may
// be NULL) = from devices[0]'s own render being done to the last rank's pixels being in place; *comm_ranks (may be NULL) = ranks the
// RCCL communicator reports (0 with MCPT_GATHER_PEER)
int mcpt_multi_last_timing(const mcpt_multi* m, double* render_ms, double* gather_ms, int32_t* comm_ranks)
{
    if (!m) return fail(MCPT_ERR_ARG, "null handle");
    if (render_ms) for (size_t i = 0; i < m->ranks.size(); i++) render_ms[i] = m->ranks[i].render_ms;
    if (gather_ms) *gather_ms = m->gather_ms;
    if (comm_ranks) {
        int n = 0;
        if (!m->comms.empty() && m->comms[0] && m->rccl.CommCount) (void)m->rccl.CommCount(m->comms[0], &n);
        *comm_ranks = n;
    }
    return MCPT_OK;
}

// statistics of every MCPT_RENDER_KEEP_STATS frame since the last call, summed over the GPUs (ms_trace, ms_total: the slowest GPU's sums)
int mcpt_multi_collect_stats(mcpt_multi* m, mcpt_stats* stats)
{
    if (!m || !stats) return fail(MCPT_ERR_ARG, "null argument");
    std::memset(stats, 0, sizeof *stats);
    for (Rank& R : m->ranks) {
        mcpt_stats s{};
        const int rc = mcpt_device_collect_stats(R.dev, &s);
        if (rc) return rc;
        add_counts(*stats, s);
        stats->ms_trace = std::max(stats->ms_trace, s.ms_trace);
        stats->ms_total = std::max(stats->ms_total, s.ms_total);
    }
    return MCPT_OK;
}

int mcpt_multi_render(mcpt_multi* m, const mcpt_render_params* p, double* img, mcpt_stats* stats)
{
    if (!img) return fail(MCPT_ERR_ARG, "null image");
    double* d = nullptr;
    const int rc = mcpt_multi_render_device(m, p, &d, stats);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(m->ranks[0].ordinal));
    HIP_TRY(hipMemcpy(img, d, size_t(m->width) * m->height * 3 * sizeof(double), hipMemcpyDeviceToHost));
    return MCPT_OK;
}

}  // extern "C"
