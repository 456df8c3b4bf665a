"""Builds tests/fake_rccl.cpp, the stand-in for librccl that works within one process, into a directory of the caller's (a temporary one)
the way test_cpp_drop_in_render_scene compiles its main(): g++ against the HIP runtime libmcpt.so is linked with.  A version script keeps
the exports to the C entry points (the C++ library's weak template instances stay local)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM = os.environ.get("ROCM_PATH") or "/opt/rocm"
# what csrc/proc_comm.cpp's comm_needs asks of the library, and ncclCommCount (mcpt_comm_size)
ENTRY_POINTS = ("ncclGetUniqueId", "ncclCommInitRank", "ncclCommDestroy", "ncclGroupStart", "ncclGroupEnd", "ncclSend", "ncclRecv", "ncclAllReduce",
                "ncclGetErrorString", "ncclCommCount")
TIMEOUT_ENV = "FAKE_RCCL_TIMEOUT_MS"


def build(directory):
    """-> the path of libfake_rccl.so in `directory`"""
    directory = str(directory)
    out = os.path.join(directory, "libfake_rccl.so")
    script = os.path.join(directory, "fake_rccl.map")
    with open(script, "w") as fh:
        fh.write("{ global: %s; local: *; };\n" % "; ".join(ENTRY_POINTS))
    lib = os.path.join(ROCM, "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-fvisibility=hidden", "-pthread",
                           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), os.path.join(HERE, "fake_rccl.cpp"), "-o", out,
                           "-Wl,--version-script=" + script, "-L" + lib, "-lamdhip64", "-Wl,-rpath," + lib])
    return out


def exported(path):
    """the dynamic symbols a shared library defines"""
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip())
