// Owning handles of the host code's HIP resources: device and pinned buffers, events, streams; and the library's HIP_TRY.
// Destructors never synchronise and never report: they release and discard the result.  Whoever owns a buffer that an enqueued kernel
// may still use keeps it alive until after the synchronisation that ends that use.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mcpt.h"

namespace mcpt {

int set_error(int code, const std::string& msg);       // capi.cpp: sets the calling thread's mcpt_last_error, returns code

// One hipMalloc allocation (Pinned: one hipHostMalloc allocation) of T, with its size in bytes.
template <class T, bool Pinned = false>
class HipBuf {
public:
    HipBuf() = default;
    HipBuf(HipBuf&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    HipBuf& operator=(HipBuf&& o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; }
        return *this;
    }
    ~HipBuf() { reset(); }

    T* get() const { return p_; }
    T& operator[](size_t i) const { return p_[i]; }
    explicit operator bool() const { return p_ != nullptr; }
    size_t bytes() const { return bytes_; }
    void reset()
    {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr; bytes_ = 0;
    }
    T* release() { T* p = p_; p_ = nullptr; bytes_ = 0; return p; }

    // (whatever was held is released first)
    hipError_t alloc_bytes(size_t bytes)
    {
        reset();
        void* p = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
        if (e == hipSuccess) { p_ = static_cast<T*>(p); bytes_ = bytes; }
        return e;
    }
    hipError_t alloc(size_t n) { return alloc_bytes(std::max<size_t>(n, 1) * sizeof(T)); }     // an empty buffer still gets one element
    // nothing if the buffer holds `bytes` already; otherwise free, then allocate exactly that (empty after a failure)
    hipError_t grow_bytes(size_t bytes) { return bytes_ >= bytes ? hipSuccess : alloc_bytes(bytes); }
    hipError_t grow(size_t n) { return grow_bytes(n * sizeof(T)); }
    template <class A>
    hipError_t upload(const std::vector<T, A>& h)
    {
        hipError_t e = alloc(h.size());
        if (e == hipSuccess && !h.empty()) e = hipMemcpy(p_, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
        return e;
    }

private:
    T* p_ = nullptr;
    size_t bytes_ = 0;
};
template <class T> using DevBuf = HipBuf<T, false>;
template <class T> using HostBuf = HipBuf<T, true>;

struct EventDestroy { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
struct StreamDestroy { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventDestroy>;
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, StreamDestroy>;

// h = the handle make(&raw, args...) creates (hipEventCreate, hipEventCreateWithFlags, hipStreamCreateWithFlags)
template <class H, class F, class... A>
hipError_t create(H& h, F make, A... args)
{
    typename H::pointer raw = nullptr;
    const hipError_t e = make(&raw, args...);
    if (e == hipSuccess) h.reset(raw);
    return e;
}

}  // namespace mcpt

inline int fail(int code, const std::string& msg) { return mcpt::set_error(code, msg); }

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail(MCPT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)
