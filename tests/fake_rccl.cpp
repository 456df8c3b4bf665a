// A stand-in for librccl that works within ONE process: the ranks of a communicator are threads of the test, all on one GPU, which RCCL
// itself refuses.  libmcpt.so loads it through MCPT_RCCL_LIBRARY (csrc/rccl_loader.hpp), so everything around the collective calls --
// the list preparation, the stream ordering, the pack and unpack kernels, the counts handed to send and receive, the error paths -- is
// the product's own code (csrc/proc_comm.cpp).  Plain C++ against <rccl/rccl.h> (types and the declarations the definitions below are
// held to) and the HIP runtime API; no device code.  tests/fake_rccl.py builds it; tests/test_gpu_comm_gather.py drives it.
//
// What it keeps of the real library:
//   communicators   ncclGetUniqueId gives distinct ids; ncclCommInitRank registers (id, rank, world) in a process-wide table and returns
//                   without waiting; communicators of different ids never see each other.  The ranks of an id "connect" at their first
//                   operation: it waits (bounded) until all `world` ranks of the id are registered, and once that has been seen it stays.
//   groups          between ncclGroupStart and ncclGroupEnd sends and receives are only queued, per thread; ncclGroupEnd posts the sends,
//                   then resolves the receives, then waits for its sends to be taken -- so a group of sends only cannot deadlock against
//                   a group of receives only, nor the other way round.  A send or receive outside a group is a group of one.
//   streams         a send's data is read after the work already on the sender's stream (an event recorded there); the copy is a
//                   device-to-device hipMemcpyAsync on the RECEIVER's stream behind a wait on that event; the sender's stream is made to
//                   wait for the copy (a second event), so the sender's buffer is not reused under it.
//   errors          a receive whose element count or type differs from its send is an error result on both sides, not a copy.
//   all-reduce      doubles, sum and max, on the host over the ranks of the id, reduced in rank order behind a barrier.
// Every wait for a peer is bounded: FAKE_RCCL_TIMEOUT_MS (default 5000), read when a communicator is created; a wait that reaches its
// bound returns an error result.  The HIP calls made while the table's lock is held only enqueue.
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unistd.h>
#include <vector>

#define EXPORT extern "C" __attribute__((visibility("default")))

namespace {

using Id = std::array<char, sizeof(ncclUniqueId)>;

struct Msg {                                // one posted send
    int src, dst;
    const void* buf;
    size_t count;
    ncclDataType_t type;
    hipEvent_t ready, copied;               // the sender's: data may be read / the copy is behind this on the receiver's stream
    int state = 0;                          // 0 posted, 1 copied, 2 refused by the receiver (count or type)
};

struct World {                              // the ranks of one id
    int world = 0;
    std::vector<bool> present;
    int registered = 0;
    bool connected = false;                 // all ranks were registered at one time
    std::deque<std::shared_ptr<Msg>> mail;
    // all-reduce: a barrier of generations
    uint64_t gen = 0;
    int arrived = 0;
    std::vector<std::vector<double>> in;
    std::vector<int> in_op;
    std::vector<double> result;
    bool result_bad = false;
};

struct Comm {
    Id id;
    World* w;
    int rank, world;
    std::chrono::milliseconds bound;
    std::vector<hipEvent_t> events;         // every event this rank's sends made: destroyed with the communicator
};

struct Op { bool send; void* buf; size_t count; ncclDataType_t type; int peer; Comm* c; hipStream_t stream; };

std::mutex g_mu;
std::condition_variable g_cv;
std::map<Id, World> g_worlds;
std::atomic<uint64_t> g_next_id{1};
thread_local int t_depth = 0;
thread_local std::vector<Op> t_ops;
thread_local std::string t_detail;          // what the last error result of this thread was about
thread_local ncclResult_t t_detail_of = ncclSuccess;

ncclResult_t error(ncclResult_t r, const std::string& what)
{
    t_detail = "fake_rccl: " + what;
    t_detail_of = r;
    return r;
}

size_t size_of(ncclDataType_t t)
{
    switch (t) {
    case ncclInt8: case ncclUint8: return 1;
    case ncclFloat16: case ncclBfloat16: return 2;
    case ncclInt32: case ncclUint32: case ncclFloat32: return 4;
    case ncclInt64: case ncclUint64: case ncclFloat64: return 8;
    default: return 0;
    }
}

using Clock = std::chrono::steady_clock;

// (lock held) waits until pred() or the deadline; false: the deadline was reached.  One call -- a group, an all-reduce -- has ONE deadline,
// its communicator's bound from where it began, however many peers it waits for.
template <class Pred>
bool wait_until(std::unique_lock<std::mutex>& lk, Clock::time_point deadline, Pred pred)
{
    return g_cv.wait_until(lk, deadline, pred);
}

// (lock held) the first operation of a rank waits for the other ranks of its id
ncclResult_t connect(std::unique_lock<std::mutex>& lk, Comm* c, Clock::time_point deadline)
{
    World* w = c->w;
    if (!wait_until(lk, deadline, [&] { return w->connected; }))
        return error(ncclSystemError, "rank " + std::to_string(c->rank) + ": only " + std::to_string(w->registered) + " of " + std::to_string(c->world) +
                                      " ranks joined this id within " + std::to_string(c->bound.count()) + " ms");
    return ncclSuccess;
}

ncclResult_t run_group(std::vector<Op>& ops)
{
    if (ops.empty()) return ncclSuccess;
    const Clock::time_point deadline = Clock::now() + ops[0].c->bound;
    std::unique_lock<std::mutex> lk(g_mu);
    for (Op& o : ops)
        if (const ncclResult_t r = connect(lk, o.c, deadline)) return r;
    ncclResult_t rc = ncclSuccess;
    // the sends are posted ...
    std::vector<std::pair<Op*, std::shared_ptr<Msg>>> sent;
    auto withdraw = [&](const Msg* m, Comm* c) {
        std::deque<std::shared_ptr<Msg>>& mail = c->w->mail;
        for (auto it = mail.begin(); it != mail.end(); ++it)
            if (it->get() == m) { mail.erase(it); break; }
    };
    for (Op& o : ops) {
        if (!o.send) continue;
        auto m = std::make_shared<Msg>();
        m->src = o.c->rank; m->dst = o.peer; m->buf = o.buf; m->count = o.count; m->type = o.type;
        hipError_t e = hipEventCreateWithFlags(&m->ready, hipEventDisableTiming);
        if (e == hipSuccess) { o.c->events.push_back(m->ready); e = hipEventCreateWithFlags(&m->copied, hipEventDisableTiming); }
        if (e == hipSuccess) { o.c->events.push_back(m->copied); e = hipEventRecord(m->ready, o.stream); }
        if (e != hipSuccess) {
            for (auto& sm : sent) withdraw(sm.second.get(), sm.first->c);       // nothing of a group that could not be posted stays behind
            return error(ncclUnhandledCudaError, std::string("posting a send: ") + hipGetErrorString(e));
        }
        o.c->w->mail.push_back(m);
        sent.emplace_back(&o, m);
    }
    if (!sent.empty()) g_cv.notify_all();
    // ... then the receives are resolved, each from the oldest send of its peer to this rank ...
    for (Op& o : ops) {
        if (o.send) continue;
        World* w = o.c->w;
        std::shared_ptr<Msg> m;
        const bool came = wait_until(lk, deadline, [&] {
            for (auto it = w->mail.begin(); it != w->mail.end(); ++it)
                if ((*it)->src == o.peer && (*it)->dst == o.c->rank && (*it)->state == 0) { m = *it; w->mail.erase(it); return true; }
            return false;
        });
        if (!came) {
            rc = error(ncclSystemError, "rank " + std::to_string(o.c->rank) + ": no send from rank " + std::to_string(o.peer) + " within " +
                                        std::to_string(o.c->bound.count()) + " ms");
            continue;
        }
        if (m->count != o.count || m->type != o.type) {
            m->state = 2;
            g_cv.notify_all();
            rc = error(ncclInvalidArgument, "rank " + std::to_string(o.c->rank) + " receives " + std::to_string(o.count) + " elements of type " +
                                            std::to_string(int(o.type)) + " from rank " + std::to_string(o.peer) + ", which sends " +
                                            std::to_string(m->count) + " of type " + std::to_string(int(m->type)));
            continue;
        }
        hipError_t e = hipStreamWaitEvent(o.stream, m->ready, 0);
        if (e == hipSuccess && o.count) e = hipMemcpyAsync(o.buf, m->buf, o.count * size_of(o.type), hipMemcpyDeviceToDevice, o.stream);
        if (e == hipSuccess) e = hipEventRecord(m->copied, o.stream);
        m->state = e == hipSuccess ? 1 : 2;
        g_cv.notify_all();
        if (e != hipSuccess) rc = error(ncclUnhandledCudaError, std::string("the copy on the receiver's stream: ") + hipGetErrorString(e));
    }
    // ... and every send waits to be taken; the sender's stream then waits for the copy
    for (auto& sm : sent) {
        Op& o = *sm.first;
        Msg* m = sm.second.get();
        if (!wait_until(lk, deadline, [&] { return m->state != 0; })) {
            withdraw(m, o.c);
            rc = error(ncclSystemError, "rank " + std::to_string(o.c->rank) + ": rank " + std::to_string(o.peer) + " did not receive within " +
                                        std::to_string(o.c->bound.count()) + " ms");
        } else if (m->state == 2) {
            rc = error(ncclInvalidArgument, "rank " + std::to_string(o.peer) + " refused the send of rank " + std::to_string(o.c->rank) + " (" +
                                            std::to_string(m->count) + " elements of type " + std::to_string(int(m->type)) + ")");
        } else if (hipStreamWaitEvent(o.stream, m->copied, 0) != hipSuccess) {
            rc = error(ncclUnhandledCudaError, "hipStreamWaitEvent on the sender's stream");
        }
    }
    return rc;
}

ncclResult_t queue(bool send, const void* buf, size_t count, ncclDataType_t type, int peer, ncclComm_t comm, hipStream_t stream)
{
    Comm* c = reinterpret_cast<Comm*>(comm);
    if (!c) return error(ncclInvalidArgument, "null communicator");
    if (peer < 0 || peer >= c->world || peer == c->rank) return error(ncclInvalidArgument, "peer " + std::to_string(peer) + " of rank " + std::to_string(c->rank));
    if (!size_of(type) || (count && !buf)) return error(ncclInvalidArgument, "buffer or type");
    t_ops.push_back(Op{send, const_cast<void*>(buf), count, type, peer, c, stream});
    if (t_depth > 0) return ncclSuccess;
    std::vector<Op> ops;
    ops.swap(t_ops);
    return run_group(ops);
}

}  // namespace

EXPORT ncclResult_t ncclGetUniqueId(ncclUniqueId* uniqueId)
{
    if (!uniqueId) return error(ncclInvalidArgument, "null id");
    std::memset(uniqueId, 0, sizeof *uniqueId);
    const uint64_t words[3] = {0x66616b655f726363ull, uint64_t(getpid()), g_next_id.fetch_add(1)};
    std::memcpy(uniqueId, words, sizeof words);
    return ncclSuccess;
}

EXPORT ncclResult_t ncclCommInitRank(ncclComm_t* comm, int nranks, ncclUniqueId commId, int rank)
{
    if (!comm || nranks < 1 || rank < 0 || rank >= nranks) return error(ncclInvalidArgument, "ncclCommInitRank: bad argument");
    *comm = nullptr;
    Id id;
    std::memcpy(id.data(), &commId, sizeof commId);
    long ms = 5000;
    if (const char* e = std::getenv("FAKE_RCCL_TIMEOUT_MS")) { const long v = std::atol(e); if (v > 0 && v <= 600000) ms = v; }
    std::lock_guard<std::mutex> lk(g_mu);
    World& w = g_worlds[id];
    if (w.world == 0) { w.world = nranks; w.present.assign(size_t(nranks), false); w.in.resize(size_t(nranks)); w.in_op.assign(size_t(nranks), 0); }
    if (w.world != nranks) return error(ncclInvalidArgument, "this id was first used for " + std::to_string(w.world) + " ranks, not " + std::to_string(nranks));
    if (w.present[size_t(rank)]) return error(ncclInvalidArgument, "rank " + std::to_string(rank) + " of this id exists already");
    w.present[size_t(rank)] = true;
    if (++w.registered == nranks) w.connected = true;
    Comm* c = new Comm{id, &w, rank, nranks, std::chrono::milliseconds(ms), {}};       // (std::map never moves its nodes)
    *comm = reinterpret_cast<ncclComm_t>(c);
    g_cv.notify_all();
    return ncclSuccess;
}

EXPORT ncclResult_t ncclCommDestroy(ncclComm_t comm)
{
    Comm* c = reinterpret_cast<Comm*>(comm);
    if (!c) return ncclSuccess;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        World* w = c->w;
        for (auto it = w->mail.begin(); it != w->mail.end();)
            it = (*it)->src == c->rank ? w->mail.erase(it) : it + 1;
        w->present[size_t(c->rank)] = false;
        if (--w->registered == 0) g_worlds.erase(c->id);
    }
    for (hipEvent_t e : c->events) (void)hipEventDestroy(e);       // (the caller has drained its stream: mcpt_comm_free synchronises it)
    delete c;
    return ncclSuccess;
}

EXPORT ncclResult_t ncclCommCount(const ncclComm_t comm, int* count)
{
    const Comm* c = reinterpret_cast<const Comm*>(comm);
    if (!c || !count) return error(ncclInvalidArgument, "ncclCommCount: null argument");
    *count = c->world;
    return ncclSuccess;
}

EXPORT ncclResult_t ncclGroupStart()
{
    t_depth++;
    return ncclSuccess;
}

EXPORT ncclResult_t ncclGroupEnd()
{
    if (t_depth <= 0) return error(ncclInvalidUsage, "ncclGroupEnd without ncclGroupStart");
    if (--t_depth > 0) return ncclSuccess;
    std::vector<Op> ops;
    ops.swap(t_ops);
    return run_group(ops);
}

EXPORT ncclResult_t ncclSend(const void* sendbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm, hipStream_t stream)
{
    return queue(true, sendbuff, count, datatype, peer, comm, stream);
}

EXPORT ncclResult_t ncclRecv(void* recvbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm, hipStream_t stream)
{
    return queue(false, recvbuff, count, datatype, peer, comm, stream);
}

EXPORT ncclResult_t ncclAllReduce(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, ncclRedOp_t op, ncclComm_t comm,
                                  hipStream_t stream)
{
    Comm* c = reinterpret_cast<Comm*>(comm);
    if (!c || !sendbuff || !recvbuff) return error(ncclInvalidArgument, "ncclAllReduce: null argument");
    if (datatype != ncclFloat64 || (op != ncclSum && op != ncclMax)) return error(ncclInvalidArgument, "ncclAllReduce: doubles, sum or max");
    std::vector<double> mine(count);
    if (count && (hipMemcpyAsync(mine.data(), sendbuff, count * sizeof(double), hipMemcpyDeviceToHost, stream) != hipSuccess ||
                  hipStreamSynchronize(stream) != hipSuccess))
        return error(ncclUnhandledCudaError, "ncclAllReduce: reading the input");
    {
        const Clock::time_point deadline = Clock::now() + c->bound;
        std::unique_lock<std::mutex> lk(g_mu);
        if (const ncclResult_t r = connect(lk, c, deadline)) return r;
        World* w = c->w;
        const uint64_t gen = w->gen;
        w->in[size_t(c->rank)] = mine;
        w->in_op[size_t(c->rank)] = int(op);
        if (++w->arrived == c->world) {
            // the last rank to arrive reduces, in rank order
            w->result = w->in[0];
            w->result_bad = false;
            for (int r = 1; r < c->world; r++) {
                const std::vector<double>& v = w->in[size_t(r)];
                if (v.size() != w->result.size() || w->in_op[size_t(r)] != w->in_op[0]) { w->result_bad = true; break; }
                for (size_t i = 0; i < v.size(); i++) w->result[i] = op == ncclSum ? w->result[i] + v[i] : (v[i] > w->result[i] ? v[i] : w->result[i]);
            }
            w->arrived = 0;
            w->gen++;
            g_cv.notify_all();
        } else if (!wait_until(lk, deadline, [&] { return w->gen != gen; })) {
            w->arrived--;                   // withdrawn: a later all-reduce of these ranks starts clean
            return error(ncclSystemError, "rank " + std::to_string(c->rank) + ": the all-reduce was not joined by every rank within " +
                                          std::to_string(c->bound.count()) + " ms");
        }
        if (w->result_bad) return error(ncclInvalidArgument, "the ranks' all-reduce calls differ in count or operation");
        mine = w->result;                   // (the next generation needs this rank too: the result stands until it has been read)
    }
    if (count && (hipMemcpyAsync(recvbuff, mine.data(), count * sizeof(double), hipMemcpyHostToDevice, stream) != hipSuccess ||
                  hipStreamSynchronize(stream) != hipSuccess))
        return error(ncclUnhandledCudaError, "ncclAllReduce: writing the result");
    return ncclSuccess;
}

EXPORT const char* ncclGetErrorString(ncclResult_t result)
{
    if (result != ncclSuccess && result == t_detail_of && !t_detail.empty()) return t_detail.c_str();
    switch (result) {
    case ncclSuccess: return "no error";
    case ncclUnhandledCudaError: return "fake_rccl: unhandled HIP error";
    case ncclSystemError: return "fake_rccl: system error";
    case ncclInvalidArgument: return "fake_rccl: invalid argument";
    case ncclInvalidUsage: return "fake_rccl: invalid usage";
    default: return "fake_rccl: error";
    }
}
