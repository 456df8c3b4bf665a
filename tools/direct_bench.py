#!/usr/bin/env python3
"""Diagnostic: what the fused direct-light query costs beside what a caller does without it, by tools/any_hit_bench.py's
method: HIP events around the _device call on one stream, one warm-up and --calls timed calls in one process, medians, one JSON line per
result.

    python tools/direct_bench.py [--scene cornell-box --map 512 --spp 16 --calls 5]

The scene under grid_atlas at --map texels a side; its texel list as the receivers; the five-light mix of tests/direct_cases.py inside the
scene's bounds (a point, a spot, a sun, two rectangles: R = 3 + 2 spp slots per receiver).
  fused : mcpt_query_direct_device over the list, every output asked for;
  parts : the same slots as a ray list -- written once by mcpt_direct_rays, uploaded beforehand -- through mcpt_trace_any_device.  That
          is only the walk of what a caller does today: building the rays on the host (56 bytes per slot up), reading a byte per slot back
          and folding in numpy are reported as bytes and not timed;
  map   : mcpt_bake_direct_lightmap_device, the raster, list, query, scatter and one dilation round together.
The walked and occluded shares and the walks' counters come from one host-form call, outside the timing.  --time-limit seconds after its
start the process ends itself."""
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
    ap.add_argument("--scene", default="cornell-box")
    ap.add_argument("--map", type=int, default=512)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--time-limit", type=int, default=300)
    a = ap.parse_args()
    signal.alarm(a.time_limit)                                   # SIGALRM's default action ends the process
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))

    import direct_cases as DC
    import hip_rt
    import montecarlopathtracing_amd as M
    L, hip = M.lib(), hip_rt.hip()
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]

    sc = M.Scene(os.path.join(ROOT, "scenes") + os.sep, a.scene, width=64, height=36)
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

    nf = int(sc.info.num_faces)
    uv = M.grid_atlas(nf, a.map, a.map)
    _, texels, q6 = dev.lightmap_texels(a.map, a.map, uv=uv)
    n = int(texels.size)
    v = sc.faces()[0][:, :9].reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    lights, bias = DC.scene_lights(M, lo, hi), DC.bias_for(lo, hi)
    nl, R = len(lights), M.direct_slots(lights, a.spp)
    arr = (M.DirectLight * nl)(*lights)
    dp = M.DirectParams(a.spp, 0, a.seed, bias, 0, (C.c_int32 * 3)(0, 0, 0))
    base = {"build": M.build_id(), "scene": a.scene, "faces": nf, "map": a.map, "receivers": n, "lights": nl, "spp": a.spp, "slots": n * R}

    # fused
    d_q, d_ids = upload(q6), upload(texels)
    outs = [hip_rt.DeviceBuffer(n * 24), hip_rt.DeviceBuffer(n * 24), hip_rt.DeviceBuffer(n * nl * 24), hip_rt.DeviceBuffer(n * nl * 8)]
    med, all_ms = timed(lambda: L.mcpt_query_direct_device(dev._h, d_q.ptr, d_ids.ptr, n, arr, nl, C.byref(dp), outs[0].ptr, outs[1].ptr, outs[2].ptr,
                                                           outs[3].ptr, st.h))
    s = M.Stats()
    got = dev.direct_light(q6[:, :3], q6[:, 3:], lights, spp=a.spp, bias=bias, seed=a.seed, ids=texels, stats=s)
    walked = int(s.rays_primary)
    print(json.dumps(dict(base, what="mcpt_query_direct_device", ms=round(med, 3), calls_ms=all_ms, walked=walked, walked_share=round(walked / (n * R), 4),
                          mean_visibility=round(float(got["visibility"].mean()), 4), nodes_per_ray=round(s.node_visits / max(walked, 1), 2),
                          tris_per_ray=round(s.tri_tests / max(walked, 1), 2), bytes_up=n * 28 + nl * 152, bytes_back=n * (48 + 32 * nl))), flush=True)
    for b in [d_q, d_ids] + outs:
        b.free()

    # parts: the walk of the same slots as a ray list
    rays, tmax, g = dev.direct_rays(q6[:, :3], q6[:, 3:], lights, spp=a.spp, bias=bias, seed=a.seed, ids=texels)
    m = rays.shape[0]
    d_rays, d_tmax, d_occ = upload(rays), upload(tmax), hip_rt.DeviceBuffer(m)
    med, all_ms = timed(lambda: L.mcpt_trace_any_device(dev._h, d_rays.ptr, d_tmax.ptr, m, d_occ.ptr, st.h))
    s = M.Stats()
    occ = dev.any_hit(rays, tmax, stats=s)
    print(json.dumps(dict(base, what="mcpt_trace_any_device over mcpt_direct_rays' slots", ms=round(med, 3), calls_ms=all_ms, rays=m, walked=int((g > 0).sum()),
                          occluded_share_of_walked=round(float(occ[g > 0].mean()), 4), nodes_per_ray=round(s.node_visits / max(int((g > 0).sum()), 1), 2),
                          bytes_up=m * 56, bytes_back=m, not_timed="building the rays, the copies, the fold on the host")), flush=True)
    for b in (d_rays, d_tmax, d_occ):
        b.free()
    del rays, tmax, g, occ

    # map
    t = a.map * a.map
    dm = M.DirectMap(a.map, a.map, 1, 0)
    d_uv = upload(uv)
    outs = [hip_rt.DeviceBuffer(t * 24), hip_rt.DeviceBuffer(t * 24), hip_rt.DeviceBuffer(t * nl * 24), hip_rt.DeviceBuffer(t * nl * 8), hip_rt.DeviceBuffer(t * 4)]
    med, all_ms = timed(lambda: L.mcpt_bake_direct_lightmap_device(dev._h, d_uv.ptr, C.byref(dm), arr, nl, C.byref(dp), outs[0].ptr, outs[1].ptr, outs[2].ptr,
                                                                   outs[3].ptr, outs[4].ptr, None, st.h))
    print(json.dumps(dict(base, what="mcpt_bake_direct_lightmap_device, dilate 1", ms=round(med, 3), calls_ms=all_ms)), flush=True)


if __name__ == "__main__":
    main()
