// The host steps every C API file of the query family shares (staging.hpp): the device gate, the mapping of a failed allocation, the
// device copies of a host-pointer call, the lease of a per-device workspace.
#include "staging.hpp"

#include <string>

#include "handles.hpp"

using namespace mcpt;

int device_gate(mcpt_device* d)
{
    if (const int rc = require_device()) return rc;
    if (!d) return fail(MCPT_ERR_ARG, "null device");
    HIP_TRY(hipSetDevice(d->ordinal));
    return MCPT_OK;
}

int count_check(int64_t n, const char* noun)
{
    return n >= 0 && n <= kInt32Max ? MCPT_OK : fail(MCPT_ERR_ARG, std::string("the number of ") + noun + " must be in 0 .. 2^31 - 1");
}

int alloc_result(hipError_t e, const char* what, size_t bytes)
{
    if (e == hipSuccess) return MCPT_OK;
    (void)hipGetLastError();                                    // the runtime keeps the failure as its last error: it has been reported here
    if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation)
        return fail(MCPT_ERR_NOMEM, std::string(what) + " (" + std::to_string(bytes) + " bytes) cannot be allocated");
    return fail(MCPT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

int launch_result()
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MCPT_OK : fail(MCPT_ERR_HIP, hipGetErrorString(e));
}

// one array of the call: src (in) is copied to the device now, dst (out) is remembered for finish(), both: an in-out array; neither: the
// array is absent, and gets device room only where `room` asks for it
int Staging::add(const void* src, void* dst, size_t bytes, const char* what, void*& dev, bool room)
{
    dev = nullptr;
    if (!src && !dst && !room) return MCPT_OK;
    DevBuf<char> b;
    if (const int rc = alloc_result(b.alloc(bytes), what, bytes)) return rc;
    dev = b.get();
    copies_.push_back(Copy{std::move(b), dst, bytes});
    if (src && bytes > 0) HIP_TRY(hipMemcpy(dev, src, bytes, hipMemcpyHostToDevice));
    return MCPT_OK;
}

int Staging::finish(int rc)
{
    const hipError_t e = hipStreamSynchronize(st_);
    if (rc == MCPT_OK && e != hipSuccess) rc = fail(MCPT_ERR_HIP, hipGetErrorString(e));
    if (rc != MCPT_OK) return rc;
    for (const Copy& c : copies_)
        if (c.host && c.bytes > 0) HIP_TRY(hipMemcpy(c.host, c.dev.get(), c.bytes, hipMemcpyDeviceToHost));
    return MCPT_OK;
}

int lease_event(Event& done)
{
    HIP_TRY(create(done, hipEventCreateWithFlags, hipEventDisableTiming));
    return MCPT_OK;
}

int Lease::begin(hipEvent_t done, hipStream_t st)
{
    HIP_TRY(hipEventSynchronize(done));
    done_ = done;
    st_ = st;
    return MCPT_OK;
}

int Lease::end(int rc)
{
    const hipError_t e = hipEventRecord(done_, st_);
    done_ = nullptr;
    if (rc == MCPT_OK && e != hipSuccess) return fail(MCPT_ERR_HIP, std::string("hipEventRecord: ") + hipGetErrorString(e));
    return rc;
}
