// librccl's entry points, loaded with dlopen when an exchange asks for RCCL (multi_device.cpp: MCPT_GATHER_RCCL; proc_comm.cpp): a
// library without it still loads.  Whoever loads it decides when it goes: mcpt_multi_free dlcloses its copy, a process communicator
// never does (the unique id refers to the library's bootstrap state).
#pragma once
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>          // types only
#include <dlfcn.h>

#include <string>

struct Rccl {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;

    // Loads the library and binds every entry point above that it has; false (and err) when it cannot be loaded or has_needed(*this),
    // the caller's test of the entry points it uses, fails.  (Callers pass a lambda: no instance of load is exported from libmcpt.so.)
    // `first` is MCPT_RCCL_LIBRARY (knobs.hpp: mcpt::rccl_library()): where it is not empty it is the first candidate.
    template <class Needed>
    bool load(std::string& err, Needed has_needed, const std::string& first)
    {
        if (!lib) {
            if (!first.empty()) lib = dlopen(first.c_str(), RTLD_NOW | RTLD_LOCAL);
            for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
                if (lib) break;
                lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            }
            if (!lib) { err = std::string("cannot load librccl: ") + dlerror(); return false; }
            auto sym = [&](const char* n) { return dlsym(lib, n); };
            GetUniqueId = reinterpret_cast<decltype(GetUniqueId)>(sym("ncclGetUniqueId"));
            CommInitAll = reinterpret_cast<decltype(CommInitAll)>(sym("ncclCommInitAll"));
            CommInitRank = reinterpret_cast<decltype(CommInitRank)>(sym("ncclCommInitRank"));
            CommDestroy = reinterpret_cast<decltype(CommDestroy)>(sym("ncclCommDestroy"));
            CommCount = reinterpret_cast<decltype(CommCount)>(sym("ncclCommCount"));
            GroupStart = reinterpret_cast<decltype(GroupStart)>(sym("ncclGroupStart"));
            GroupEnd = reinterpret_cast<decltype(GroupEnd)>(sym("ncclGroupEnd"));
            Send = reinterpret_cast<decltype(Send)>(sym("ncclSend"));
            Recv = reinterpret_cast<decltype(Recv)>(sym("ncclRecv"));
            AllReduce = reinterpret_cast<decltype(AllReduce)>(sym("ncclAllReduce"));
            GetErrorString = reinterpret_cast<decltype(GetErrorString)>(sym("ncclGetErrorString"));
        }
        if (!has_needed(*this)) { err = "librccl lacks an expected symbol"; return false; }
        return true;
    }
};
