// C ABI of libmcpt.so (include/mcpt.h): what is not about one handle -- the calling thread's error, the version, the device count and
// the HIP runtime check.  The handles' entry points, which stand in for ray_intersect / generateImg / imshow / render_scene of the
// reference, are in the files handles.hpp lists.
#include <hip/hip_runtime_api.h>
#include <hip/hip_version.h>
#include <dlfcn.h>

#include <atomic>
#include <cstdio>
#include <string>

#include "handles.hpp"

using namespace mcpt;

namespace {
thread_local std::string g_error;
}  // namespace

// the calling thread's error message, for every translation unit of the library (hip_owned.hpp: fail, HIP_TRY)
namespace mcpt { int set_error(int code, const std::string& msg) { g_error = msg; return code; } }

extern "C" {

int mcpt_version(void) { return MCPT_VERSION; }
const char* mcpt_last_error(void) { return g_error.c_str(); }

const char* mcpt_knobs_describe(void) { return knobs_table(); }

int mcpt_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ------------------------------------------------------------------------------------------------ which HIP runtime is this?
// libmcpt.so's code objects are built by one hipcc; the libamdhip64.so they run on is whichever the process loaded first under that
// soname (a Python process that imported torch has the wheel's bundled runtime, not /opt/rocm's).  Kernels built by a newer compiler on
// an older runtime are the likeliest cause of the abort DESIGN 8a records, and nothing used to notice: now the first device creation
// compares the two versions and refuses when major.minor differ, unless the caller has said it knows (mcpt_allow_runtime_mismatch).
static std::atomic<int> g_allow_runtime_mismatch{0};

void mcpt_allow_runtime_mismatch(int32_t allow) { g_allow_runtime_mismatch.store(allow ? 1 : 0); }

// Pure comparison (CPU unit test): 0 when a library compiled against HIP `compiled` may run on runtime `runtime` (both encoded as
// HIP_VERSION: major * 10^7 + minor * 10^5 + patch), else MCPT_ERR_HIP with a message naming both and the runtime's file.
int mcpt_hip_runtime_check(int32_t compiled, int32_t runtime, const char* runtime_path, char* msg, int64_t cap)
{
    const int cmaj = compiled / 10000000, cmin = compiled / 100000 % 100, rmaj = runtime / 10000000, rmin = runtime / 100000 % 100;
    const bool ok = compiled > 0 && runtime > 0 && cmaj == rmaj && cmin == rmin;
    if (msg && cap > 0) {
        if (ok) msg[0] = 0;
        else
            std::snprintf(msg, size_t(cap),
                          "libmcpt.so was compiled against HIP %d.%d (%d) but this process runs on HIP runtime %d.%d (%d) loaded from %s: "
                          "another libamdhip64.so was loaded first (a Python process that imported torch has the wheel's).  Load libmcpt.so "
                          "before it, or call mcpt_allow_runtime_mismatch(1) / set MCPT_ALLOW_RUNTIME_MISMATCH=1 to run anyway",
                          cmaj, cmin, compiled, rmaj, rmin, runtime, (runtime_path && runtime_path[0]) ? runtime_path : "(unknown)");
    }
    return ok ? MCPT_OK : MCPT_ERR_HIP;
}

int mcpt_hip_runtime_info(int32_t* compiled, int32_t* runtime, char* path, int64_t cap)
{
    if (compiled) *compiled = HIP_VERSION;
    int rv = 0;
    if (hipRuntimeGetVersion(&rv) != hipSuccess) { (void)hipGetLastError(); rv = 0; }
    if (runtime) *runtime = rv;
    if (path && cap > 0) {
        path[0] = 0;
        Dl_info info;
        if (dladdr(reinterpret_cast<const void*>(static_cast<hipError_t (*)(int*)>(&hipRuntimeGetVersion)), &info) && info.dli_fname) std::snprintf(path, size_t(cap), "%s", info.dli_fname);
    }
    return MCPT_OK;
}

}  // extern "C"

// what mcpt_device_create asks before it touches a device (mcpt_multi_create through it)
int runtime_gate()
{
    int32_t compiled = 0, runtime = 0;
    char path[512], msg[1024];
    mcpt_hip_runtime_info(&compiled, &runtime, path, sizeof path);
    if (mcpt_hip_runtime_check(compiled, runtime, path, msg, sizeof msg) == MCPT_OK) return MCPT_OK;
    if (g_allow_runtime_mismatch.load() || read_knobs().allow_runtime_mismatch) {
        static std::atomic<int> told{0};
        if (!told.exchange(1)) std::fprintf(stderr, "libmcpt: %s -- running anyway, as asked\n", msg);
        return MCPT_OK;
    }
    return fail(MCPT_ERR_HIP, msg);
}

int require_device(int* visible)
{
    const int n = mcpt_device_count();
    if (visible) *visible = n;
    return n > 0 ? MCPT_OK : fail(MCPT_ERR_NO_DEVICE, "no HIP device available (libmcpt has no CPU fallback)");
}
