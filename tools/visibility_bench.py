#!/usr/bin/env python3
"""Diagnostic: what probe visibility costs and what it buys an irradiance volume.  tools/volume_bench.py's method.

    python tools/visibility_bench.py bake   [--grid 64 --spp 64 --res 8 --calls 5]
    python tools/visibility_bench.py lookup [--grid 64 --size 2048 --res 8 --calls 5]
    python tools/visibility_bench.py approx [--size 64 --spp 1024 --ref-spp 4096 --res 8]

bake  : cornell-box, a --grid^3 volume over the scene's bounds (2 % in from every side).  One warm-up call and --calls timed calls of
        mcpt_bake_volume_visibility_device, each between two HIP events on one stream, and the same of mcpt_bake_volume_device on the
        same grid -- the yardstick: the radiance bake of the same rays.  Medians.  The fold's traffic floor: 36 bytes read per ray
        (direction, leaf, distance) and 16 written per bin, at 8 TB/s.  Under rocprofv3 --kernel-trace --stats (a run of its own) the
        kernels' names give the split: k_chunk_rays<2>, the trace engine's kernels, k_vis_fold.  MCPT_LIB selects another build of the library.
lookup: that volume baked once (coefficients and moments) into device buffers; the receivers are the texel list of cornell-box under
        grid_atlas at --size^2.  mcpt_volume_irradiance_visible_device and mcpt_volume_irradiance_device timed alternately.
approx: glassroom's own chart at --size^2: volumes of 8^3, 16^3 and 32^3 probes baked at --spp, looked up plainly, under the baked
        valid mask, and under mask and visibility (normal_bias 0 and a quarter of the smallest spacing), against Device.irradiance of the
        same texel list at --ref-spp: relative RMS error, median and the worst texel, over texels the reference lights.
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
    ap.add_argument("mode", choices=["bake", "lookup", "approx"])
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--spp", type=int, default=None)
    ap.add_argument("--res", type=int, default=8)
    ap.add_argument("--ref-spp", type=int, default=4096)
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
                    mean_ratio=round(float(E[lit].mean() / ref[lit].mean()), 4), negative=int((E < 0).any(axis=1).sum()))

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
            # A scene whose faces wind so that their stored normals point away from free space reports its front faces as back faces
            # (cornell-box and glassroom do): the caller then takes the mask from the other count.
            flipped = bool(back.sum() * 2 > hits.sum())
            if flipped:
                valid = ((hits - back) <= 0.25 * spp).astype(np.uint8)
            base["winding"] = "flipped: mask from hits - back" if flipped else "as stored"
            rows = [("plain", dev.volume_irradiance(g, sh, x, b)), ("mask", dev.volume_irradiance(g, sh, x, b, valid=valid))]
            for bias in (0.0, 0.25 * min(g.spacing)):
                vis = M.volume_visibility(R, maxd, bias, 0.0)
                rows.append(("mask+visibility bias %.3g" % bias, dev.volume_irradiance_visible(g, sh, m, x, b, vis, valid=valid)))
            for what, (E, corners) in rows:
                print(json.dumps(dict(base, what="approx", lookup=what, scene="glassroom", size=size, probes=n ** 3, spp=spp, res=R, ref_spp=a.ref_spp,
                                      texels=int(texels.size), lit=int(lit.sum()), invalid_probes=int((valid == 0).sum()), unlit_receivers=int((corners[lit] == 0).sum()),
                                      **rel_error(E, ref, lit))), flush=True)
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
        return {k: (float(np.median(v[1:])), [round(t, 4) for t in v[1:]]) for k, v in ms.items()}

    def upload(arr):
        arr = np.ascontiguousarray(arr)
        buf = hip_rt.DeviceBuffer(arr.nbytes)
        hip_rt.check(hip.hipMemcpy(buf.ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes, 1))
        return buf

    n = a.grid
    probes, spp = n ** 3, a.spp or 64
    g = grid_over(M, dev, n)
    maxd = 1.5 * float(np.sqrt(sum(float(s) ** 2 for s in g.spacing)))
    d_sh, d_hits = hip_rt.DeviceBuffer(probes * 216), hip_rt.DeviceBuffer(probes * 4)
    d_m, d_back, d_valid = hip_rt.DeviceBuffer(probes * R * R * 16), hip_rt.DeviceBuffer(probes * 4), hip_rt.DeviceBuffer(probes)
    sp = M.ShParams(spp, 0, a.seed, 0, (C.c_int32 * 3)(0, 0, 0))
    vp = M.VisibilityParams(spp, 0, a.seed, R, 0, maxd, 0.25, 0, (C.c_int32 * 2)(0, 0))

    def bake_visibility():
        return L.mcpt_bake_volume_visibility_device(dev._h, C.byref(g), C.byref(vp), d_m.ptr, d_hits.ptr, d_back.ptr, d_valid.ptr, None, st.h)

    def bake_radiance():
        return L.mcpt_bake_volume_device(dev._h, C.byref(g), C.byref(sp), d_sh.ptr, None, d_hits.ptr, None, st.h)

    if a.mode == "bake":
        res = timed_alternately({"mcpt_bake_volume_device": bake_radiance, "mcpt_bake_volume_visibility_device": bake_visibility})
        floor_ms = (probes * spp * 36 + probes * R * R * 16) / HBM_BYTES_PER_S * 1e3
        for what, (med, all_ms) in res.items():
            print(json.dumps(dict(base, what=what, scene="cornell-box", probes=probes, spp=spp, res=R, ms=round(med, 3), calls_ms=all_ms,
                                  fold_floor_ms=round(floor_ms, 4))), flush=True)
        print(json.dumps(dict(base, what="ratio visibility / radiance bake", ratio=round(res["mcpt_bake_volume_visibility_device"][0] / res["mcpt_bake_volume_device"][0], 3))))
        return

    size = a.size or 2048
    uv = M.grid_atlas(sc.info.num_faces, size, size)
    _, texels, q6 = dev.lightmap_texels(size, size, uv=uv)
    m = int(texels.size)
    assert bake_radiance() == 0 and bake_visibility() == 0, L.mcpt_last_error()
    d_q, d_e, d_c = upload(q6), hip_rt.DeviceBuffer(m * 24), hip_rt.DeviceBuffer(m * 4)
    vis = M.volume_visibility(R, maxd, 0.0, 0.0)
    res = timed_alternately({
        "mcpt_volume_irradiance_device": lambda: L.mcpt_volume_irradiance_device(dev._h, C.byref(g), d_sh.ptr, None, d_q.ptr, m, d_e.ptr, None, st.h),
        "mcpt_volume_irradiance_device masked": lambda: L.mcpt_volume_irradiance_device(dev._h, C.byref(g), d_sh.ptr, d_valid.ptr, d_q.ptr, m, d_e.ptr, None, st.h),
        "mcpt_volume_irradiance_visible_device": lambda: L.mcpt_volume_irradiance_visible_device(dev._h, C.byref(g), d_sh.ptr, d_m.ptr, d_valid.ptr, C.byref(vis),
                                                                                                 d_q.ptr, m, d_e.ptr, None, st.h)})
    floor_ms = (m * 72 + probes * (216 + R * R * 16)) / HBM_BYTES_PER_S * 1e3
    for what, (med, all_ms) in res.items():
        print(json.dumps(dict(base, what=what, probes=probes, receivers=m, res=R, ms=round(med, 4), calls_ms=all_ms, floor_ms=round(floor_ms, 4))), flush=True)
    print(json.dumps(dict(base, what="ratio visible / plain lookup",
                          ratio=round(res["mcpt_volume_irradiance_visible_device"][0] / res["mcpt_volume_irradiance_device"][0], 3))))


if __name__ == "__main__":
    main()
