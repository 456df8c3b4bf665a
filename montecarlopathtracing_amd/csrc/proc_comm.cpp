// One process per GPU without torch in the process (mcpt_comm_*): the end-of-frame gather of a rank's pixels into rank 0's frame, a
// barrier and a small all-reduce, over an RCCL communicator that spans the PROCESSES of a launch (python -m torch.distributed.run starts
// them and hands out RANK / WORLD_SIZE; the ranks exchange RCCL's unique id themselves: montecarlopathtracing_amd/procs.py).  Why not
// torch.distributed for this: importing torch puts the wheel's HIP runtime under libmcpt.so's kernels -- here every rank
// runs the runtime the library was compiled against and /opt/rocm's own librccl.  The reference has nothing like it (one OpenMP process,
// MTPC/pathTracing.cpp:303); the in-process form of the same exchange is multi_device.cpp.
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "handles.hpp"
#include "rccl_loader.hpp"

using mcpt::DevBuf;

struct mcpt_comm {
    Rccl rccl;
    ncclComm_t comm = nullptr;
    int ordinal = 0, rank = 0, world = 1;
    mcpt::Stream stream;                        // the exchange's own stream
    mcpt::Event ev;
    // pixel lists of the partition the buffers were made for: frame width and height, tile_w, tile_h as the call gave them (world and rank
    // are the handle's).  A communicator is bound to no scene: the frame's size comes with every call.  {-1, ...}: no list is valid
    int key[4] = {-1, -1, -1, -1};
    int64_t n_own = 0;
    DevBuf<int32_t> d_pixels_own;               // this rank's pixels
    DevBuf<double> d_compact;                   // [n_own][3]
    std::vector<int64_t> n_of;                  // rank 0: pixels of every rank
    std::vector<DevBuf<int32_t>> d_pixels_of;   // rank 0: their lists, on this GPU
    std::vector<DevBuf<double>> d_stage_of;     // rank 0: where their buffers land
    DevBuf<double> d_red;                       // all-reduce scratch (64 doubles)
};

// the entry points of librccl a process communicator uses
static const auto comm_needs = [](const Rccl& r) {
    return r.GetUniqueId && r.CommInitRank && r.CommDestroy && r.GroupStart && r.GroupEnd && r.Send && r.Recv && r.AllReduce && r.GetErrorString;
};

#define NCCL_OR_FAIL(c, expr)                                                                           \
    do {                                                                                                \
        ncclResult_t r_ = (expr);                                                                       \
        if (r_ != ncclSuccess) return fail(MCPT_ERR_HIP, std::string(#expr) + ": " + (c)->rccl.GetErrorString(r_)); \
    } while (0)

static void free_lists(mcpt_comm* c)
{
    c->d_pixels_own.reset(); c->d_compact.reset(); c->d_pixels_of.clear(); c->d_stage_of.clear(); c->n_of.clear();
    for (int& k : c->key) k = -1;
    c->n_own = 0;
}

static int prepare_lists(mcpt_comm* c, const mcpt_scene* scene, const mcpt_render_params* p)
{
    const int key[4] = {scene->s.width, scene->s.height, p->tile_w, p->tile_h};
    if (key[0] <= 0 || key[1] <= 0) return fail(MCPT_ERR_ARG, "the scene has no frame size");
    if (c->d_pixels_own && std::memcmp(key, c->key, sizeof key) == 0) return MCPT_OK;
    free_lists(c);                              // (the key with them: whatever fails below, no list of this handle counts as valid)
    // rank r's pixels (a rank without pixels still gets buffers of one entry)
    auto list_of = [&](int r, std::vector<int32_t>& pix) -> int64_t {
        mcpt_render_params q = *p;
        q.rank = r; q.world = c->world;
        if (const int rc = owned_pixels(scene->s.width, scene->s.height, &q, pix)) return rc;
        const int64_t n = int64_t(pix.size());
        if (pix.empty()) pix.push_back(0);
        return n;
    };
    std::vector<int32_t> pix;
    int64_t n = list_of(c->rank, pix);
    if (n < 0) return int(n);
    c->n_own = n;
    HIP_TRY(c->d_pixels_own.upload(pix));
    HIP_TRY(c->d_compact.alloc(pix.size() * 3));
    if (c->rank == 0) {
        c->n_of.assign(size_t(c->world), 0); c->d_pixels_of.resize(size_t(c->world)); c->d_stage_of.resize(size_t(c->world));
        for (int r = 1; r < c->world; r++) {
            n = list_of(r, pix);
            if (n < 0) return int(n);
            c->n_of[size_t(r)] = n;
            HIP_TRY(c->d_pixels_of[size_t(r)].upload(pix));
            HIP_TRY(c->d_stage_of[size_t(r)].alloc(pix.size() * 3));
        }
    }
    std::memcpy(c->key, key, sizeof key);
    return MCPT_OK;
}

extern "C" {

int mcpt_comm_unique_id(uint8_t* id, int64_t cap)
{
    if (!id || cap < int64_t(sizeof(ncclUniqueId))) return fail(MCPT_ERR_ARG, "the id buffer needs 128 bytes");
    Rccl r;
    std::string err;
    if (!r.load(err, comm_needs, mcpt::rccl_library())) return fail(MCPT_ERR_IO, err);
    ncclUniqueId u;
    const ncclResult_t rc = r.GetUniqueId(&u);
    if (rc != ncclSuccess) return fail(MCPT_ERR_HIP, std::string("ncclGetUniqueId: ") + r.GetErrorString(rc));
    std::memcpy(id, &u, sizeof u);
    return int(sizeof u);           // (the library stays loaded: the id refers to its bootstrap state)
}

void mcpt_comm_free(mcpt_comm* c)
{
    if (!c) return;
    (void)hipSetDevice(c->ordinal);
    if (c->stream) (void)hipStreamSynchronize(c->stream.get());
    free_lists(c);
    c->d_red.reset();
    if (c->comm && c->rccl.CommDestroy) (void)c->rccl.CommDestroy(c->comm);
    delete c;                                   // (the event and the stream with it)
}

int mcpt_comm_create(int32_t ordinal, int32_t rank, int32_t world, const uint8_t* id, int64_t id_bytes, mcpt_comm** out)
{
    if (!out || !id || world < 1 || rank < 0 || rank >= world || id_bytes != int64_t(sizeof(ncclUniqueId))) return fail(MCPT_ERR_ARG, "bad argument");
    *out = nullptr;
    int visible = 0;
    if (const int rc = require_device(&visible)) return rc;
    if (ordinal < 0 || ordinal >= visible) return fail(MCPT_ERR_NO_DEVICE, "device ordinal out of range");
    std::unique_ptr<mcpt_comm, void (*)(mcpt_comm*)> c(new mcpt_comm, mcpt_comm_free);
    c->ordinal = ordinal; c->rank = rank; c->world = world;
    std::string err;
    if (!c->rccl.load(err, comm_needs, mcpt::rccl_library())) return fail(MCPT_ERR_IO, err);
    HIP_TRY(hipSetDevice(ordinal));
    HIP_TRY(create(c->stream, hipStreamCreateWithFlags, hipStreamNonBlocking));
    HIP_TRY(create(c->ev, hipEventCreateWithFlags, hipEventDisableTiming));
    HIP_TRY(c->d_red.alloc(64));
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof u);
    NCCL_OR_FAIL(c, c->rccl.CommInitRank(&c->comm, world, u, rank));
    *out = c.release();
    return MCPT_OK;
}

int mcpt_comm_size(const mcpt_comm* c)
{
    if (!c) return 0;
    int n = 0;
    if (c->rccl.CommCount && c->comm && c->rccl.CommCount(c->comm, &n) == ncclSuccess) return n;
    return c->world;
}

// Every rank: its own pixels of d_frame (frame layout, H*W*3 doubles on its GPU) travel as one compact buffer to rank 0, which puts them
// at their positions in ITS d_frame.  The exchange waits for what `stream` (the stream the frame was rendered on; NULL: the default
// stream) holds when the call is made, and the call returns when rank 0's frame is complete (ranks > 0: when their buffer is sent).
int mcpt_comm_gather_frame(mcpt_comm* c, const mcpt_scene* scene, const mcpt_render_params* p, double* d_frame, void* stream)
{
    if (!c || !scene || !p || !d_frame) return fail(MCPT_ERR_ARG, "null argument");
    HIP_TRY(hipSetDevice(c->ordinal));
    if (c->world == 1) return MCPT_OK;
    int rc = prepare_lists(c, scene, p);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(c->ev.get(), static_cast<hipStream_t>(stream)));
    HIP_TRY(hipStreamWaitEvent(c->stream.get(), c->ev.get(), 0));
    if (c->rank > 0) {
        if (c->n_own > 0) {
            mcpt::launch_pack_pixels(d_frame, c->d_pixels_own.get(), c->n_own, c->d_compact.get(), c->stream.get());
            HIP_TRY(hipGetLastError());
        }
        NCCL_OR_FAIL(c, c->rccl.GroupStart());
        if (c->n_own > 0) NCCL_OR_FAIL(c, c->rccl.Send(c->d_compact.get(), size_t(c->n_own) * 3, ncclDouble, 0, c->comm, c->stream.get()));
        NCCL_OR_FAIL(c, c->rccl.GroupEnd());
    } else {
        NCCL_OR_FAIL(c, c->rccl.GroupStart());
        for (int r = 1; r < c->world; r++)
            if (c->n_of[size_t(r)] > 0) NCCL_OR_FAIL(c, c->rccl.Recv(c->d_stage_of[size_t(r)].get(), size_t(c->n_of[size_t(r)]) * 3, ncclDouble, r, c->comm, c->stream.get()));
        NCCL_OR_FAIL(c, c->rccl.GroupEnd());
        for (int r = 1; r < c->world; r++)
            if (c->n_of[size_t(r)] > 0) {
                mcpt::launch_unpack_pixels(c->d_stage_of[size_t(r)].get(), c->d_pixels_of[size_t(r)].get(), c->n_of[size_t(r)], d_frame, c->stream.get());
                HIP_TRY(hipGetLastError());
            }
    }
    HIP_TRY(hipStreamSynchronize(c->stream.get()));
    return MCPT_OK;
}

// v[n] (n <= 64, host) reduced over the ranks in place: op 0 = sum, 1 = max.  Doubles as the barrier of the launch (n = 0 is allowed).
int mcpt_comm_allreduce(mcpt_comm* c, double* v, int32_t n, int32_t op)
{
    if (!c || n < 0 || n > 64 || (n > 0 && !v) || (op != 0 && op != 1)) return fail(MCPT_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(c->ordinal));
    double buf[64] = {0};
    const int m = n > 0 ? n : 1;
    if (n > 0) std::memcpy(buf, v, size_t(n) * sizeof(double));
    HIP_TRY(hipMemcpy(c->d_red.get(), buf, size_t(m) * sizeof(double), hipMemcpyHostToDevice));          // blocking: buf is pageable
    NCCL_OR_FAIL(c, c->rccl.AllReduce(c->d_red.get(), c->d_red.get(), size_t(m), ncclDouble, op == 0 ? ncclSum : ncclMax, c->comm, c->stream.get()));
    HIP_TRY(hipStreamSynchronize(c->stream.get()));
    HIP_TRY(hipMemcpy(buf, c->d_red.get(), size_t(m) * sizeof(double), hipMemcpyDeviceToHost));
    if (n > 0) std::memcpy(v, buf, size_t(n) * sizeof(double));
    return MCPT_OK;
}

}  // extern "C"
