#!/usr/bin/env python3
"""Diagnostic: what an ambient-occlusion map costs and what occlusion buys an irradiance volume.  tools/visibility_bench.py's
method.

    python tools/occlusion_bench.py bake   [--size 2048 --spp 64 --calls 5]
    python tools/occlusion_bench.py approx [--size 64 --spp 1024 --ref-spp 4096 --res 8]

bake  : cornell-box under grid_atlas at --size^2.  One warm-up call and --calls timed calls, each between two HIP events on one stream, of
        mcpt_bake_occlusion_lightmap_device, of mcpt_bake_lightmap_device on the same chart -- the yardstick: the radiance bake of the
        same rays -- and of mcpt_query_visibility_device over the map's texel list at the same sample count (the same number of rays,
        drawn over the sphere), taken in turn.  Medians.  The fold's traffic floor: 36 bytes read per ray (direction, leaf, distance) and
        56 written per entry, at 8 TB/s.  Under rocprofv3 --kernel-trace --stats (a run of its own) the kernels' names give the split:
        k_chunk_rays<1>, the trace engine's kernels, k_occ_fold, k_occ_scatter.  Run from the checkout of a build without the occlusion calls
        (the parent's), the tool times the lightmap bake alone.
approx: glassroom's own chart at --size^2: volumes of 8^3, 16^3 and 32^3 probes baked at --spp and the occlusion of the texel list at
        --spp with a reach of 1.5 cell diagonals, against Device.irradiance of the same list at --ref-spp.  The estimates: the plain
        lookup under the texel's normal; the plain lookup under the bent normal times ao; the visibility-weighted lookup (mask, normal
        bias a quarter of the smallest spacing) under the bent normal times ao, and, for comparison, under the texel's normal without
        ao.  Relative RMS error, median and the worst texel, over texels the reference lights.  Nothing is asserted.
One process; --time-limit seconds after its start the process ends itself.  One JSON line per result."""
import argparse
import ctypes as C
import json
import os
import signal
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8e12


def grid_over(M, dev, n, inset=0.02):
    box, _ = dev.bvh_nodes()
    lo, hi = np.minimum(box[0, :3], box[0, 3:]), np.maximum(box[0, :3], box[0, 3:])
    return M.volume_grid(lo + inset * (hi - lo), (1.0 - 2.0 * inset) * (hi - lo) / (n - 1), (n, n, n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["bake", "approx"])
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--spp", type=int, default=None)
    ap.add_argument("--res", type=int, default=8)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--falloff", choices=["hard", "linear", "square"], default="hard")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--time-limit", type=int, default=420)
    a = ap.parse_args()
    signal.alarm(a.time_limit)                                   # SIGALRM's default action ends the process
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import montecarlopathtracing_amd as M
    base = {"build": M.build_id()}
    scenes = os.path.join(ROOT, "scenes") + os.sep
    R = a.res

    def rel_error(E, ref, lit):
        rel = np.sqrt(((E - ref)[lit] ** 2).sum(axis=1)) / np.sqrt((ref[lit] ** 2).sum(axis=1))
        return dict(rel_rms=round(float(np.sqrt((rel ** 2).mean())), 4), rel_median=round(float(np.median(rel)), 4), rel_worst=round(float(rel.max()), 3),
                    mean_ratio=round(float(E[lit].mean() / ref[lit].mean()), 4))

    if a.mode == "approx":
        from conftest import extra_scene_dir
        size, spp = a.size or 64, a.spp or 1024
        sc = M.Scene(extra_scene_dir(), "glassroom", width=64, height=36)
        dev = M.Device(sc, 0)
        _, texels, q6 = dev.lightmap_texels(size, size)
        x, b = q6[:, :3], q6[:, 3:]
        ref, _, _ = dev.irradiance(x, b, a.ref_spp, seed=a.seed + 1000)
        lit = (ref > 0).all(axis=1)
        for n in (8, 16, 32):
            g = grid_over(M, dev, n)
            sh, _, _ = dev.bake_volume(g, spp, seed=a.seed)
            m, hits, back, valid = dev.bake_volume_visibility(g, spp, res=R, seed=a.seed)
            maxd = 1.5 * float(np.sqrt(sum(float(s) ** 2 for s in g.spacing)))
            # (glassroom winds its faces so that their stored normals point away from free space: the mask comes from the other count)
            if back.sum() * 2 > hits.sum():
                valid = ((hits - back) <= 0.25 * spp).astype(np.uint8)
            occ = dev.occlusion(x, b, spp, maxd, a.falloff, seed=a.seed + 7, ids=texels)
            ao, bent = occ["ao"][:, None], occ["bent"]
            vis = M.volume_visibility(R, maxd, 0.25 * min(g.spacing), 0.0)
            rows = [("plain(normal)", dev.volume_irradiance(g, sh, x, b)[0]),
                    ("plain(bent) * ao", dev.volume_irradiance(g, sh, x, bent)[0] * ao),
                    ("visible(normal)", dev.volume_irradiance_visible(g, sh, m, x, b, vis, valid=valid)[0]),
                    ("visible(bent) * ao", dev.volume_irradiance_visible(g, sh, m, x, bent, vis, valid=valid)[0] * ao)]
            for what, E in rows:
                print(json.dumps(dict(base, what="approx", estimate=what, scene="glassroom", size=size, probes=n ** 3, spp=spp, res=R, falloff=a.falloff,
                                      reach=round(maxd, 4), ref_spp=a.ref_spp, texels=int(texels.size), lit=int(lit.sum()),
                                      mean_ao=round(float(occ["ao"].mean()), 4), **rel_error(E, ref, lit))), flush=True)
        return

    import hip_rt
    L, hip = M.lib(), hip_rt.hip()
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    sc = M.Scene(scenes, "cornell-box", width=64, height=36)
    dev = M.Device(sc, 0)
    hip_rt.set_device(0)
    st = hip_rt.Stream()
    e0, e1 = C.c_void_p(), C.c_void_p()
    hip_rt.check(hip.hipEventCreate(C.byref(e0)))
    hip_rt.check(hip.hipEventCreate(C.byref(e1)))

    def once(call):
        hip_rt.check(hip.hipEventRecord(e0, st.h))
        rc = call()
        assert rc == 0, L.mcpt_last_error()
        hip_rt.check(hip.hipEventRecord(e1, st.h))
        hip_rt.check(hip.hipEventSynchronize(e1))
        t = C.c_float()
        hip_rt.check(hip.hipEventElapsedTime(C.byref(t), e0, e1))
        return t.value

    def timed_alternately(calls):
        """{name: (median, all)} of calls {name: callable}: one warm-up each, then --calls rounds that take every call in turn"""
        ms = {k: [] for k in calls}
        for i in range(a.calls + 1):
            for k, call in calls.items():
                ms[k].append(once(call))
        return {k: (float(np.median(v[1:])), [round(t, 3) for t in v[1:]]) for k, v in ms.items()}

    def upload(arr):
        arr = np.ascontiguousarray(arr)
        buf = hip_rt.DeviceBuffer(arr.nbytes)
        hip_rt.check(hip.hipMemcpy(buf.ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes, 1))
        return buf

    size, spp = a.size or 2048, a.spp or 64
    n = size * size
    uv = M.grid_atlas(sc.info.num_faces, size, size)
    _, texels, q6 = dev.lightmap_texels(size, size, uv=uv)
    covered = int(texels.size)
    box, _ = dev.bvh_nodes()
    reach = 0.25 * float(np.linalg.norm(box[0, 3:] - box[0, :3]))
    d_uv = upload(uv)
    d_irr = hip_rt.DeviceBuffer(n * 24)
    lp = M.LightmapParams(size, size, spp, 0, a.seed, 0, 0, (C.c_int32 * 2)(0, 0))
    calls = {"mcpt_bake_lightmap_device": lambda: L.mcpt_bake_lightmap_device(dev._h, d_uv.ptr, C.byref(lp), d_irr.ptr, None, None, None, None, st.h)}
    if hasattr(L, "mcpt_bake_occlusion_lightmap_device"):
        d_ao, d_err, d_bent = hip_rt.DeviceBuffer(n * 8), hip_rt.DeviceBuffer(n * 8), hip_rt.DeviceBuffer(n * 24)
        d_hits, d_back = hip_rt.DeviceBuffer(n * 4), hip_rt.DeviceBuffer(n * 4)
        d_p, d_m = upload(q6[:, :3]), hip_rt.DeviceBuffer(covered * R * R * 16)
        om = M.OcclusionMap(size, size, 0, 0)
        op = M.OcclusionParams(spp, 0, a.seed, {"hard": 0, "linear": 1, "square": 2}[a.falloff], 0, reach, 0, (C.c_int32 * 2)(0, 0))
        vp = M.VisibilityParams(spp, 0, a.seed, R, 0, reach, 0.25, 0, (C.c_int32 * 2)(0, 0))
        calls["mcpt_bake_occlusion_lightmap_device"] = lambda: L.mcpt_bake_occlusion_lightmap_device(
            dev._h, d_uv.ptr, C.byref(om), C.byref(op), d_ao.ptr, d_err.ptr, d_bent.ptr, d_hits.ptr, d_back.ptr, None, None, st.h)
        calls["mcpt_query_visibility_device"] = lambda: L.mcpt_query_visibility_device(dev._h, d_p.ptr, None, covered, C.byref(vp), d_m.ptr, d_hits.ptr,
                                                                                       d_back.ptr, None, None, st.h)
    res = timed_alternately(calls)
    floor_ms = (covered * spp * 36 + covered * 56) / HBM_BYTES_PER_S * 1e3
    for what, (med, all_ms) in res.items():
        print(json.dumps(dict(base, what=what, scene="cornell-box", size=size, covered=covered, spp=spp, rays=covered * spp, ms=round(med, 3), calls_ms=all_ms,
                              fold_floor_ms=round(floor_ms, 4))), flush=True)
    if "mcpt_bake_occlusion_lightmap_device" in res:
        t = res["mcpt_bake_occlusion_lightmap_device"][0]
        print(json.dumps(dict(base, what="ratios", occlusion_over_lightmap=round(t / res["mcpt_bake_lightmap_device"][0], 3),
                              occlusion_over_visibility=round(t / res["mcpt_query_visibility_device"][0], 3))))


if __name__ == "__main__":
    main()
