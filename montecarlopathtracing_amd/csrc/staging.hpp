// The host steps every C API file of the query family shares (staging.cpp): the device gate, the mapping of a failed allocation, the
// device copies of a host-pointer call, and the lease of a workspace the device keeps between calls.  Host only: no .hip file includes it.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <limits>
#include <memory>
#include <type_traits>
#include <vector>

#include "hip_owned.hpp"

struct mcpt_device;

#pragma GCC visibility push(hidden)

constexpr int64_t kInt32Max = std::numeric_limits<int32_t>::max();

// what every call on a device asks before it touches one: a visible HIP device (MCPT_ERR_NO_DEVICE), a handle (MCPT_ERR_ARG), and the
// calling thread on the handle's device
int device_gate(mcpt_device* d);
// MCPT_ERR_ARG unless n is in 0 .. 2^31 - 1: "the number of <noun> must be in 0 .. 2^31 - 1"
int count_check(int64_t n, const char* noun);
// a failed allocation of a workspace or a copy: MCPT_ERR_NOMEM when the memory is not there, and the device stays usable
int alloc_result(hipError_t e, const char* what, size_t bytes);
// the launches since the last look: MCPT_OK, or MCPT_ERR_HIP with the runtime's text
int launch_result();

// b holds at least `count` elements afterwards (what they held is gone when it had to grow)
template <class T>
int grow(mcpt::DevBuf<T>& b, size_t count, const char* what)
{
    return alloc_result(b.grow(count), what, count * sizeof(T));
}

// The device copies of one host-pointer call.  The caller's arrays are pageable host memory, so the copies on either side of the device
// form block; the device form itself is ordered on `st`, the device's own stream.  The copies go with the object: finish() comes first.
class Staging {
public:
    explicit Staging(hipStream_t st) : st_(st) {}
    // dev = a device copy of host[0 .. count), filled now; a null host leaves dev null, an empty array still gets a pointer
    template <class T, class D>
    int in(const T* host, size_t count, const char* what, D*& dev)
    {
        static_assert(std::is_same<std::remove_const_t<D>, T>::value, "the copy has the array's type");
        void* p = nullptr;
        const int rc = add(host, nullptr, count * sizeof(T), what, p);
        dev = static_cast<T*>(p);
        return rc;
    }
    // what a null host gets of out(): a null dev, or device room all the same (the launch requires the array), which nobody reads back
    enum Absent { kNull, kRoom };
    // dev = device room for host[0 .. count), which finish() fills from it; a null host leaves dev null, or as `absent` says
    template <class T>
    int out(T* host, size_t count, const char* what, T*& dev, Absent absent = kNull)
    {
        void* p = nullptr;
        const int rc = add(nullptr, host, count * sizeof(T), what, p, absent == kRoom);
        dev = static_cast<T*>(p);
        return rc;
    }
    // dev = a device copy of host[0 .. count), filled now and copied back by finish() among the out() arrays: what the kernels do not
    // write comes back as the caller's own bytes; a null host leaves dev null
    template <class T>
    int inout(T* host, size_t count, const char* what, T*& dev)
    {
        void* p = nullptr;
        const int rc = add(host, host, count * sizeof(T), what, p);
        dev = static_cast<T*>(p);
        return rc;
    }
    // The end of the call, rc the device form's result: the stream is waited for, on failure as well -- nothing enqueued may still use a
    // copy when it goes -- and when all is well every out() and inout() array is copied back, in the order of those calls.
    int finish(int rc);

private:
    struct Copy { mcpt::DevBuf<char> dev; void* host; size_t bytes; };      // host: where finish() copies it back to, or null
    int add(const void* src, void* dst, size_t bytes, const char* what, void*& dev, bool room = false);
    hipStream_t st_;
    std::vector<Copy> copies_;
};

// A call's hold on a workspace the device keeps between calls (mcpt_device::Lightmap, AdaptiveQuery, Volume, Visibility, Baked,
// Reflection).  A device-form call returns with its kernels enqueued, so the workspace is no local of the call: its `done` event is
// recorded behind the call's last kernel and waited for before the next call writes there.  lease() makes the workspace on first use
// and waits; the Lease it arms records `done` on the call's stream on every way out of the call after that -- end(rc) where the call
// reports, the destructor (which, like hip_owned.hpp's, discards the result) where it has returned early.
class Lease {
public:
    Lease() = default;
    Lease(const Lease&) = delete;
    Lease& operator=(const Lease&) = delete;
    ~Lease() { if (done_) (void)hipEventRecord(done_, st_); }
    // waits for what the call before has enqueued, then holds the workspace for a call on st
    int begin(hipEvent_t done, hipStream_t st);
    // records `done`; rc, or MCPT_ERR_HIP when rc is MCPT_OK and the record fails
    int end(int rc);

private:
    hipEvent_t done_ = nullptr;
    hipStream_t st_ = nullptr;
};

int lease_event(mcpt::Event& done);                  // a workspace's `done` event, made on its first use

// Holds *slot for a call on st.  The first call makes it: the struct, its event, and whatever first(*slot) adds once (single words the
// call reads back through); a workspace that cannot be made whole is not kept.
template <class W, class First>
int lease(std::unique_ptr<W>& slot, hipStream_t st, Lease& l, First first)
{
    if (!slot) {
        slot = std::make_unique<W>();
        int rc = lease_event(slot->done);
        if (rc == MCPT_OK) rc = first(*slot);
        if (rc != MCPT_OK) {
            slot.reset();
            return rc;
        }
    }
    return l.begin(slot->done.get(), st);
}
template <class W>
int lease(std::unique_ptr<W>& slot, hipStream_t st, Lease& l)
{
    return lease(slot, st, l, [](W&) -> int { return MCPT_OK; });
}

#pragma GCC visibility pop
