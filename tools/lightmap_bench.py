#!/usr/bin/env python3
"""Diagnostic: what a lightmap costs on top of the hemisphere query it is.

    python tools/lightmap_bench.py bake  [--scene cornell-box --size 2048 --spp 64 --dilate 2 --calls 5 --list-file F]
    python tools/lightmap_bench.py query --list-file F [--root OTHER_TREE --spp 64 --calls 5]

bake: the scene under grid_atlas; one warm-up call and --calls timed calls of mcpt_bake_lightmap_device into device buffers, each between
two HIP events on one stream; then the same for mcpt_query_radiance_device on the map's own texel list, uploaded beforehand.  With
--list-file the list (texels, q6) is written there.  query: only the query on the list read from --list-file, with the package of --root
-- another build of the library, the parent commit's for instance, which need not know lightmaps.  One process; --time-limit seconds after
its start the process ends itself.  Medians; one JSON line per result."""
import argparse
import ctypes as C
import json
import os
import signal
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["bake", "query"])
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--scene", default="cornell-box")
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dilate", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--list-file", default=None)
    ap.add_argument("--time-limit", type=int, default=240)
    a = ap.parse_args()
    signal.alarm(a.time_limit)                                   # SIGALRM's default action ends the process
    sys.path.insert(0, a.root)
    sys.path.insert(0, os.path.join(a.root, "tests"))

    import hip_rt
    import montecarlopathtracing_amd as M
    L, hip = M.lib(), hip_rt.hip()
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]

    sc = M.Scene(os.path.join(a.root, "scenes") + os.sep, a.scene, width=64, height=36)
    dev = M.Device(sc, 0)
    hip_rt.set_device(0)
    st = hip_rt.Stream()
    e0, e1 = C.c_void_p(), C.c_void_p()
    hip_rt.check(hip.hipEventCreate(C.byref(e0)))
    hip_rt.check(hip.hipEventCreate(C.byref(e1)))

    def upload(arr):
        b = hip_rt.DeviceBuffer(max(arr.nbytes, 8))
        hip_rt.check(hip.hipMemcpy(b.ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes, 1))
        return b

    def timed(call):
        ms = []
        for i in range(a.calls + 1):                             # the first call warms up
            hip_rt.check(hip.hipEventRecord(e0, st.h))
            rc = call()
            assert rc == 0, L.mcpt_last_error()
            hip_rt.check(hip.hipEventRecord(e1, st.h))
            hip_rt.check(hip.hipEventSynchronize(e1))
            t = C.c_float()
            hip_rt.check(hip.hipEventElapsedTime(C.byref(t), e0, e1))
            ms.append(t.value)
        return float(np.median(ms[1:])), [round(v, 3) for v in ms[1:]]

    base = {"build": M.build_id(), "scene": a.scene, "spp": a.spp}
    if a.mode == "bake":
        W = H = a.size
        uv = M.grid_atlas(sc.info.num_faces, W, H)
        owner, texels, q6 = dev.lightmap_texels(W, H, uv=uv)
        if a.list_file:
            np.savez(a.list_file, texels=texels, q6=q6)
        n = W * H
        d_uv = upload(uv)
        maps = [hip_rt.DeviceBuffer(n * 24), hip_rt.DeviceBuffer(n * 24), hip_rt.DeviceBuffer(n * 4), hip_rt.DeviceBuffer(n * 4)]
        lp = M.LightmapParams(W, H, a.spp, 0, a.seed, 0, a.dilate, (C.c_int32 * 2)(0, 0))
        med, all_ms = timed(lambda: L.mcpt_bake_lightmap_device(dev._h, d_uv.ptr, C.byref(lp), maps[0].ptr, maps[1].ptr, maps[2].ptr, maps[3].ptr,
                                                                None, st.h))
        print(json.dumps(dict(base, what="mcpt_bake_lightmap_device", width=W, height=H, dilate=a.dilate, covered=int(texels.size),
                              samples=int(texels.size) * a.spp, ms=round(med, 3), calls_ms=all_ms)))
    else:
        z = np.load(a.list_file)
        texels, q6 = np.ascontiguousarray(z["texels"]), np.ascontiguousarray(z["q6"])
    m = texels.size
    d_q, d_ids = upload(q6), upload(texels)
    out = [hip_rt.DeviceBuffer(m * 24), hip_rt.DeviceBuffer(m * 24), hip_rt.DeviceBuffer(m * 4)]
    qp = M.QueryParams(a.spp, 0, a.seed, M.QUERY_HEMISPHERE, 0, (C.c_int32 * 2)(0, 0))
    med, all_ms = timed(lambda: L.mcpt_query_radiance_device(dev._h, d_q.ptr, d_ids.ptr, m, C.byref(qp), out[0].ptr, out[1].ptr, out[2].ptr, None, st.h))
    print(json.dumps(dict(base, what="mcpt_query_radiance_device", queries=int(m), samples=int(m) * a.spp, ms=round(med, 3), calls_ms=all_ms)))


if __name__ == "__main__":
    main()
