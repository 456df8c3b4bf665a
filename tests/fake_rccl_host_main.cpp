// tests/fake_rccl.cpp without a GPU, as a stand-alone program under the host sanitizers (tests/test_distributed_cpu.py compiles the two
// together): the HIP runtime calls the stand-in makes are defined HERE as host operations -- an event is a counted allocation, a copy is
// a memcpy made at once -- so what runs is the stand-in's own table, group queue, bounded waits and barrier, with the ranks as threads.
// Prints "ok" and the number of checks; any failed check is named on stderr and the exit status is 1.
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

static std::atomic<int> g_live_events{0}, g_copies{0}, g_checks{0}, g_failed{0};

extern "C" {
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = reinterpret_cast<hipEvent_t>(new int(0)); g_live_events++; return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { delete reinterpret_cast<int*>(e); g_live_events--; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { ++*reinterpret_cast<int*>(e); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t e, unsigned) { return *reinterpret_cast<int*>(e) > 0 ? hipSuccess : hipErrorInvalidValue; }   // (recorded before it is waited for)
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind, hipStream_t) { std::memcpy(dst, src, n); g_copies++; return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "host stub"; }
}

#define CHECK(x)                                                                         \
    do {                                                                                 \
        g_checks++;                                                                      \
        if (!(x)) { g_failed++; std::fprintf(stderr, "line %d: %s\n", __LINE__, #x); }   \
    } while (0)

using Secs = std::chrono::duration<double>;
static double now() { return Secs(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static const double kBound = 0.15;              // FAKE_RCCL_TIMEOUT_MS=150, set in main

static std::vector<ncclComm_t> comms(int world, int present = -1)
{
    ncclUniqueId id;
    CHECK(ncclGetUniqueId(&id) == ncclSuccess);
    std::vector<ncclComm_t> c(size_t(world), nullptr);
    for (int r = 0; r < (present < 0 ? world : present); r++) CHECK(ncclCommInitRank(&c[size_t(r)], world, id, r) == ncclSuccess);
    return c;
}
static void destroy(std::vector<ncclComm_t>& c) { for (ncclComm_t x : c) CHECK(ncclCommDestroy(x) == ncclSuccess); }

static void ranks(int world, const std::function<void(int)>& fn)
{
    std::vector<std::thread> t;
    for (int r = 0; r < world; r++) t.emplace_back(fn, r);
    for (std::thread& x : t) x.join();
}

static bool says(ncclResult_t r, const char* what) { return std::strstr(ncclGetErrorString(r), what) != nullptr; }

int main()
{
    setenv("FAKE_RCCL_TIMEOUT_MS", "150", 1);
    ncclUniqueId a, b;
    CHECK(ncclGetUniqueId(&a) == ncclSuccess && ncclGetUniqueId(&b) == ncclSuccess && std::memcmp(&a, &b, sizeof a) != 0);

    // a gather: ranks > 0 send their (different) counts in a group of sends only, rank 0 receives in a group of receives only; two
    // communicators of different ids run the same exchange at the same time and never see each other's data; many rounds (order of a
    // peer's sends is kept)
    for (int world : {2, 3, 5}) {
        std::vector<ncclComm_t> c[2] = {comms(world), comms(world)};
        int n = 0;
        CHECK(ncclCommCount(c[0][0], &n) == ncclSuccess && n == world);
        ranks(2 * world, [&](int t) {
            const int k = t / world, r = t % world;
            for (int round = 0; round < 40; round++) {
                if (r > 0) {
                    std::vector<double> v(size_t(r * 3));
                    for (size_t i = 0; i < v.size(); i++) v[i] = 1000.0 * k + 100.0 * r + round + 0.001 * double(i);
                    CHECK(ncclGroupStart() == ncclSuccess);
                    CHECK(ncclSend(v.data(), v.size(), ncclDouble, 0, c[k][size_t(r)], nullptr) == ncclSuccess);
                    CHECK(ncclGroupEnd() == ncclSuccess);           // (returns once the copy is made: v may go)
                } else {
                    std::vector<std::vector<double>> got{size_t(world)};
                    CHECK(ncclGroupStart() == ncclSuccess);
                    for (int p = world - 1; p >= 1; p--) {
                        got[size_t(p)].assign(size_t(p * 3), -1.0);
                        CHECK(ncclRecv(got[size_t(p)].data(), size_t(p * 3), ncclDouble, p, c[k][0], nullptr) == ncclSuccess);
                    }
                    CHECK(ncclGroupEnd() == ncclSuccess);
                    for (int p = 1; p < world; p++)
                        for (size_t i = 0; i < got[size_t(p)].size(); i++) CHECK(got[size_t(p)][i] == 1000.0 * k + 100.0 * p + round + 0.001 * double(i));
                }
            }
        });
        destroy(c[0]);
        destroy(c[1]);
    }

    // every rank sends and receives in one group (a ring): no deadlock
    {
        std::vector<ncclComm_t> c = comms(3);
        ranks(3, [&](int r) {
            double out = 10.0 + r, in = -1.0;
            CHECK(ncclGroupStart() == ncclSuccess);
            CHECK(ncclRecv(&in, 1, ncclDouble, (r + 2) % 3, c[size_t(r)], nullptr) == ncclSuccess);
            CHECK(ncclSend(&out, 1, ncclDouble, (r + 1) % 3, c[size_t(r)], nullptr) == ncclSuccess);
            CHECK(ncclGroupEnd() == ncclSuccess);
            CHECK(in == 10.0 + (r + 2) % 3);
        });
        // a count that differs, then a type that differs: an error on both sides, nothing copied; the communicator works afterwards
        for (int kind = 0; kind < 2; kind++) {
            const int copies = g_copies;
            ranks(2, [&](int r) {
                double v[4] = {1, 2, 3, 4};
                const ncclResult_t rc = r == 1 ? ncclSend(v, 4, ncclDouble, 0, c[1], nullptr)
                                               : ncclRecv(v, kind == 0 ? 3 : 4, kind == 0 ? ncclDouble : ncclInt64, 1, c[0], nullptr);
                CHECK(rc == ncclInvalidArgument && says(rc, r == 1 ? "refused the send of rank 1" : "which sends 4"));
            });
            CHECK(g_copies == copies);
        }
        // a peer that is there but never sends, a send nobody receives: an error at the bound; the withdrawn send is not delivered later
        double t0 = now();
        double lost = 77.0, in = -1.0;
        ncclResult_t rc = ncclRecv(&in, 1, ncclDouble, 2, c[0], nullptr);
        CHECK(rc == ncclSystemError && says(rc, "no send from rank 2") && now() - t0 >= kBound * 0.9 && now() - t0 < kBound + 1.0);
        t0 = now();
        rc = ncclSend(&lost, 1, ncclDouble, 0, c[2], nullptr);
        CHECK(rc == ncclSystemError && says(rc, "did not receive") && now() - t0 >= kBound * 0.9 && now() - t0 < kBound + 1.0);
        ranks(2, [&](int t) {
            double v = 5.0;
            CHECK((t == 0 ? ncclRecv(&v, 1, ncclDouble, 2, c[0], nullptr) : ncclSend(&v, 1, ncclDouble, 0, c[2], nullptr)) == ncclSuccess);
            CHECK(v == 5.0);
        });
        CHECK(ncclGroupEnd() == ncclInvalidUsage);
        CHECK(ncclSend(&lost, 1, ncclDouble, 3, c[0], nullptr) == ncclInvalidArgument && ncclSend(&lost, 1, ncclDouble, 0, c[0], nullptr) == ncclInvalidArgument);
        destroy(c);
    }

    // an id whose ranks never all join: every operation of those that did is an error at the bound (gather and all-reduce)
    {
        std::vector<ncclComm_t> c = comms(3, 2);
        ranks(2, [&](int r) {
            double v = 1.0, t0 = now();
            ncclResult_t rc = r == 0 ? ncclRecv(&v, 1, ncclDouble, 1, c[0], nullptr) : ncclSend(&v, 1, ncclDouble, 0, c[1], nullptr);
            CHECK(rc == ncclSystemError && says(rc, "only 2 of 3 ranks joined") && now() - t0 >= kBound * 0.9 && now() - t0 < kBound + 1.0);
            t0 = now();
            rc = ncclAllReduce(&v, &v, 1, ncclDouble, ncclSum, c[size_t(r)], nullptr);
            CHECK(rc == ncclSystemError && says(rc, "only 2 of 3 ranks joined") && now() - t0 < kBound + 1.0 && v == 1.0);
        });
        ncclUniqueId other;
        ncclComm_t x = nullptr;
        CHECK(ncclGetUniqueId(&other) == ncclSuccess && ncclCommInitRank(&x, 3, other, 2) == ncclSuccess);      // rank 2, on another id
        double v = 2.0;
        CHECK(ncclSend(&v, 1, ncclDouble, 0, x, nullptr) == ncclSystemError);
        CHECK(ncclCommDestroy(x) == ncclSuccess);
        c.resize(2);
        destroy(c);
    }

    // all-reduce: sum and max in rank order, twice on the same communicators; a rank that stays away is an error for the others at the
    // bound and leaves nothing behind; calls that differ in count or operation are refused for everyone
    {
        std::vector<ncclComm_t> c = comms(3);
        for (ncclRedOp_t op : {ncclSum, ncclMax})
            for (size_t n : {size_t(1), size_t(64)})
                for (int again = 0; again < 2; again++)
                    ranks(3, [&](int r) {
                        std::vector<double> v(n), out(n, -1.0);
                        for (size_t i = 0; i < n; i++) v[i] = double((7 * r + 3 * int(i)) % 11 - 4);
                        CHECK(ncclAllReduce(v.data(), out.data(), n, ncclDouble, op, c[size_t(r)], nullptr) == ncclSuccess);
                        for (size_t i = 0; i < n; i++) {
                            const double x0 = double((3 * int(i)) % 11 - 4), x1 = double((7 + 3 * int(i)) % 11 - 4), x2 = double((14 + 3 * int(i)) % 11 - 4);
                            CHECK(out[i] == (op == ncclSum ? x0 + x1 + x2 : std::max(x0, std::max(x1, x2))));
                        }
                    });
        ranks(2, [&](int r) {
            double v = 1.0;
            const ncclResult_t rc = ncclAllReduce(&v, &v, 1, ncclDouble, ncclSum, c[size_t(r)], nullptr);
            CHECK(rc == ncclSystemError && says(rc, "not joined by every rank") && v == 1.0);
        });
        ranks(3, [&](int r) {
            double v[2] = {1.0 + r, 0.0};
            const ncclResult_t rc = ncclAllReduce(v, v, r == 2 ? 2 : 1, ncclDouble, ncclSum, c[size_t(r)], nullptr);
            CHECK(rc == ncclInvalidArgument && says(rc, "differ in count or operation"));
        });
        ranks(3, [&](int r) {
            double v = 1.0 + r;
            CHECK(ncclAllReduce(&v, &v, 1, ncclDouble, r == 1 ? ncclMax : ncclSum, c[size_t(r)], nullptr) == ncclInvalidArgument);
        });
        ranks(3, [&](int r) {
            double v = 1.0 + r;
            CHECK(ncclAllReduce(&v, &v, 1, ncclDouble, ncclSum, c[size_t(r)], nullptr) == ncclSuccess && v == 6.0);
            float f = 1.0f;
            CHECK(ncclAllReduce(&f, &f, 1, ncclFloat, ncclSum, c[size_t(r)], nullptr) == ncclInvalidArgument);
        });
        destroy(c);
    }
    CHECK(g_live_events == 0);                  // every event went with its communicator
    if (g_failed) return 1;
    std::printf("ok %d\n", int(g_checks));
    return 0;
}
