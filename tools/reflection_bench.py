#!/usr/bin/env python3
"""Diagnostic: what reflection probes cost.  tools/volume_bench.py's method: every timed call is a _device call between two
HIP events on one stream, one warm-up call and --calls timed calls, medians.

    python tools/reflection_bench.py bake      [--res 64 --spp 64 --probes 1,64 --calls 5]
    python tools/reflection_bench.py prefilter [--res 128 --levels 128:4096,64:1024,32:256,16:64,8:16 --probes 4 --calls 5]
    python tools/reflection_bench.py lookup    [--receivers 1580000 --calls 5]

bake     : cornell-box; mcpt_bake_reflection_device of --probes probes at --res, --spp beside the plain mcpt_query_radiance_device (ray
           kind, spp 1) over as many rays -- the bake's own rays of its first chunk, repeated -- so the difference is the ray kernel, the
           fold and the chunking.
prefilter: a synthetic --res^2 map per probe (what the kernel costs does not depend on what the numbers mean) into the levels given as
           size:exponent.  Reported beside the time: the pairs, the fp64 operations a pair costs by the kernel's own arithmetic (5 for the
           dot product, the squarings and multiplications of ipow, 8 for the sums) and the share of the rate at which the vector units
           issue un-fused fp64 instructions that this comes to (39.3e12 lane operations a second: 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz;
           the library compiles without contraction, so no operation here is a fused pair).  Under rocprofv3 --pmc (a run of its own,
           no tracing) the kernel's name is k_reflection_prefilter.
lookup   : --receivers random directions and exponents into a five-level chain of 4 probes.
MCPT_LIB selects another build of the library.  One process; --time-limit seconds after its start the process ends itself.  One JSON
line per result."""
import argparse
import ctypes as C
import json
import os
import signal
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP64_ISSUE_PER_S = 256 * 4 * 16 * 2.4e9


def ipow_ops(n):
    """multiplications of the binary squaring for exponent n"""
    return 0 if n == 0 else bin(n).count("1") + n.bit_length() - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["bake", "prefilter", "lookup"])
    ap.add_argument("--res", type=int, default=None)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--probes", default=None)
    ap.add_argument("--levels", default="128:4096,64:1024,32:256,16:64,8:16")
    ap.add_argument("--receivers", type=int, default=1580000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--time-limit", type=int, default=420)
    a = ap.parse_args()
    signal.alarm(a.time_limit)                                   # SIGALRM's default action ends the process
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hip_rt
    import montecarlopathtracing_amd as M
    base = {"build": M.build_id()}
    L, hip = M.lib(), hip_rt.hip()
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    sc = M.Scene(os.path.join(ROOT, "scenes") + os.sep, "cornell-box", width=64, height=36)
    dev = M.Device(sc, 0)
    hip_rt.set_device(0)
    st = hip_rt.Stream()
    e0, e1 = C.c_void_p(), C.c_void_p()
    hip_rt.check(hip.hipEventCreate(C.byref(e0)))
    hip_rt.check(hip.hipEventCreate(C.byref(e1)))

    def once(call):
        hip_rt.check(hip.hipEventRecord(e0, st.h))
        call()
        hip_rt.check(hip.hipEventRecord(e1, st.h))
        hip_rt.check(hip.hipEventSynchronize(e1))
        t = C.c_float()
        hip_rt.check(hip.hipEventElapsedTime(C.byref(t), e0, e1))
        return t.value

    def timed(call):
        ms = [once(call) for _ in range(a.calls + 1)][1:]
        return {"ms": round(float(np.median(ms)), 4), "calls_ms": [round(t, 4) for t in ms]}

    def upload(arr):
        arr = np.ascontiguousarray(arr)
        buf = hip_rt.DeviceBuffer(arr.nbytes)
        hip_rt.check(hip.hipMemcpy(buf.ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes, 1))
        return buf

    rng = np.random.default_rng(a.seed)
    box, _ = dev.bvh_nodes()
    lo, hi = np.minimum(box[0, :3], box[0, 3:]), np.maximum(box[0, :3], box[0, 3:])

    if a.mode == "bake":
        R, S = a.res or 64, a.spp
        for n in [int(v) for v in (a.probes or "1,64").split(",")]:
            p = lo + (hi - lo) * rng.uniform(0.2, 0.8, size=(n, 3))
            rays_n = n * R * R * S
            d_p, d_rad = upload(p), hip_rt.DeviceBuffer(n * R * R * 24)
            res = timed(lambda: dev.bake_reflection_probes_device(d_p.ptr, n, d_rad.ptr, R, S, seed=a.seed, stream=st.h))
            print(json.dumps(dict(base, what="mcpt_bake_reflection_device", probes=n, res=R, spp=S, rays=rays_n, **res)), flush=True)
            # the plain query over as many rays: the bake's first rays (at most a chunk's), repeated to the bake's count
            chunk = min(rays_n, 1 << 22)
            rays, ids = dev.reflection_rays(p, R, S, np.arange(chunk, dtype=np.int64), seed=a.seed)
            d_rays, d_ids = upload(rays), upload(ids)
            d_mean, d_hits = hip_rt.DeviceBuffer(chunk * 24), hip_rt.DeviceBuffer(chunk * 4)
            qp = M.QueryParams(1, 0, a.seed, M.QUERY_RAY, 0, (C.c_int32 * 2)(0, 0))

            def query():
                for _ in range(rays_n // chunk):
                    assert L.mcpt_query_radiance_device(dev._h, d_rays.ptr, d_ids.ptr, chunk, C.byref(qp), d_mean.ptr, None, d_hits.ptr, None, st.h) == 0
            res = timed(query)
            print(json.dumps(dict(base, what="mcpt_query_radiance_device", rays=rays_n, calls_of=chunk, **res)), flush=True)
            for b in (d_p, d_rad, d_rays, d_ids, d_mean, d_hits):
                b.free()
        return

    levels = [tuple(int(v) for v in l.split(":")) for l in a.levels.split(",")]
    R = a.res or 128
    n = int(a.probes or 4)
    c = M.reflection_chain(R, levels)
    d_rad, d_chain = upload(rng.uniform(0.25, 1.25, size=(n, R * R, 3))), hip_rt.DeviceBuffer(n * c.num_texels * 24)
    if a.mode == "prefilter":
        res = timed(lambda: dev.prefilter_reflection_device(c, d_rad.ptr, n, d_chain.ptr, stream=st.h))
        # a pair whose cosine is positive (half of them, to the texels' discretisation) does all of it; the others the dot product alone
        pairs = [n * r * r * R * R for r, _ in levels]
        ops = sum(p * (5 + 0.5 * (ipow_ops(ns) + 8)) for p, (_, ns) in zip(pairs, levels))
        rate = ops / (res["ms"] * 1e-3)
        print(json.dumps(dict(base, what="mcpt_reflection_prefilter_device", probes=n, res=R, levels=levels, pairs=sum(pairs), fp64_ops=int(ops),
                              fp64_ops_per_s=round(rate, -9), share_of_fp64_issue=round(rate / FP64_ISSUE_PER_S, 4), **res)), flush=True)
        for r, ns in levels:                                      # level by level: the top level dominates
            one = M.reflection_chain(R, [(r, ns)])
            res = timed(lambda: dev.prefilter_reflection_device(one, d_rad.ptr, n, d_chain.ptr, stream=st.h))
            ops = n * r * r * R * R * (5 + 0.5 * (ipow_ops(ns) + 8))
            print(json.dumps(dict(base, what="mcpt_reflection_prefilter_device", probes=n, res=R, levels=[(r, ns)], pairs=n * r * r * R * R,
                                  share_of_fp64_issue=round(ops / (res["ms"] * 1e-3) / FP64_ISSUE_PER_S, 4), **res)), flush=True)
        return

    dev.prefilter_reflection_device(c, d_rad.ptr, n, d_chain.ptr, stream=st.h)
    m = a.receivers
    d_probe, d_d = upload(rng.integers(0, n, size=m).astype(np.int32)), upload(rng.normal(size=(m, 3)))
    d_x, d_out = upload(rng.uniform(0.0, 1.5 * levels[0][1], size=m)), hip_rt.DeviceBuffer(m * 24)
    res = timed(lambda: dev.reflection_lookup_device(c, d_chain.ptr, n, d_probe.ptr, d_d.ptr, d_x.ptr, m, d_out.ptr, stream=st.h))
    print(json.dumps(dict(base, what="mcpt_reflection_lookup_device", receivers=m, probes=n, levels=levels, bytes_per_receiver=4 + 24 + 8 + 24, **res)), flush=True)


if __name__ == "__main__":
    main()
