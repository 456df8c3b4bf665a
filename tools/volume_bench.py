#!/usr/bin/env python3
"""Diagnostic: what an irradiance volume costs and how well it stands in for a hemisphere query.

    python tools/volume_bench.py bake   [--grid 64 --spp 64 --calls 5]
    python tools/volume_bench.py lookup [--grid 64 --size 2048 --calls 5]
    python tools/volume_bench.py approx [--size 64 --spp 1024 --ref-spp 4096]

bake  : cornell-box, a --grid^3 volume over the scene's bounds (2 % in from every side).  One warm-up call and --calls timed calls of
        mcpt_bake_volume_device, each between two HIP events on one stream (6l's method), and the same of mcpt_query_sh_device on the
        grid's points uploaded beforehand -- the call a caller had before.  A library without the volume's symbols (--package-root: the
        package of another checkout, for the commit before) is timed on the probe query alone.  Medians.
lookup: that volume baked once into a device buffer; the receivers are the texel list of cornell-box under grid_atlas at --size^2,
        uploaded once.  mcpt_volume_irradiance_device timed as above, mcpt_volume_irradiance_host by the host clock on the same inputs,
        and the traffic floor n * (48 + 24) B + 216 B per probe at 8 TB/s (DESIGN 8's HBM rate).
approx: glassroom's own chart at --size^2: the lookup in volumes of 8^3, 16^3 and 32^3 probes baked at --spp against Device.irradiance
        of the same texel list at --ref-spp: relative RMS error and the worst texel, over texels the reference lights.
One process; --time-limit seconds after its start the process ends itself.  One JSON line per result."""
import argparse
import ctypes as C
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8e12


def grid_over(M, dev, n, inset=0.02):
    box, _ = dev.bvh_nodes()
    lo, hi = np.minimum(box[0, :3], box[0, 3:]), np.maximum(box[0, :3], box[0, 3:])
    return M.volume_grid(lo + inset * (hi - lo), (1.0 - 2.0 * inset) * (hi - lo) / (n - 1), (n, n, n))


def grid_points(lo, hi, n, inset=0.02):
    """the same grid's points for a package that has no volume_grid (the commit before)"""
    o, s = lo + inset * (hi - lo), (1.0 - 2.0 * inset) * (hi - lo) / (n - 1)
    iz, iy, ix = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    return np.stack([o[a] + i.reshape(-1).astype(np.float64) * s[a] for a, i in enumerate((ix, iy, iz))], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["bake", "lookup", "approx"])
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--spp", type=int, default=None)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose package and library are measured (default: this one)")
    ap.add_argument("--time-limit", type=int, default=420)
    a = ap.parse_args()
    signal.alarm(a.time_limit)                                   # SIGALRM's default action ends the process
    sys.path.insert(0, os.path.abspath(a.package_root))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import montecarlopathtracing_amd as M
    base = {"build": M.build_id()}
    scenes = os.path.join(ROOT, "scenes") + os.sep

    if a.mode == "approx":
        from conftest import extra_scene_dir
        size, spp = a.size or 64, a.spp or 1024
        sc = M.Scene(extra_scene_dir(), "glassroom", width=64, height=36)
        dev = M.Device(sc, 0)
        _, texels, q6 = dev.lightmap_texels(size, size)
        ref, ref_err, _ = dev.irradiance(q6[:, :3], q6[:, 3:], a.ref_spp, seed=a.seed + 1000)
        lit = (ref > 0).all(axis=1)
        for n in (8, 16, 32):
            g = grid_over(M, dev, n)
            sh, _, _ = dev.bake_volume(g, spp, seed=a.seed)
            E, _ = dev.volume_irradiance(g, sh, q6[:, :3], q6[:, 3:])
            rel = np.sqrt(((E - ref)[lit] ** 2).sum(axis=1)) / np.sqrt((ref[lit] ** 2).sum(axis=1))
            print(json.dumps(dict(base, what="approx", scene="glassroom", size=size, probes=n ** 3, spp=spp, ref_spp=a.ref_spp, texels=int(texels.size),
                                  lit=int(lit.sum()), rel_rms=round(float(np.sqrt((rel ** 2).mean())), 4), rel_median=round(float(np.median(rel)), 4),
                                  rel_worst=round(float(rel.max()), 3), mean_ratio=round(float(E[lit].mean() / ref[lit].mean()), 4),
                                  negative=int((E < 0).any(axis=1).sum()))))
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

    def upload(arr):
        arr = np.ascontiguousarray(arr)
        b = hip_rt.DeviceBuffer(arr.nbytes)
        hip_rt.check(hip.hipMemcpy(b.ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes, 1))
        return b

    n = a.grid
    probes = n ** 3
    spp = a.spp or 64
    has_volume = hasattr(M, "volume_grid")
    box, _ = dev.bvh_nodes()
    lo, hi = np.minimum(box[0, :3], box[0, 3:]), np.maximum(box[0, :3], box[0, 3:])
    d_sh, d_err, d_hits = hip_rt.DeviceBuffer(probes * 216), hip_rt.DeviceBuffer(probes * 216), hip_rt.DeviceBuffer(probes * 4)
    sp = M.ShParams(spp, 0, a.seed, 0, (C.c_int32 * 3)(0, 0, 0))
    g = grid_over(M, dev, n) if has_volume else None

    if a.mode == "bake":
        pts = M.volume_points(g) if has_volume else grid_points(lo, hi, n)
        d_p = upload(pts)
        order = ["query", "bake"] if has_volume else ["query"]
        for what in order:
            if what == "bake":
                med, all_ms = timed(lambda: L.mcpt_bake_volume_device(dev._h, C.byref(g), C.byref(sp), d_sh.ptr, d_err.ptr, d_hits.ptr, None, st.h))
            else:
                med, all_ms = timed(lambda: L.mcpt_query_sh_device(dev._h, d_p.ptr, None, probes, C.byref(sp), d_sh.ptr, d_err.ptr, d_hits.ptr, None, st.h))
            print(json.dumps(dict(base, what="mcpt_bake_volume_device" if what == "bake" else "mcpt_query_sh_device", scene="cornell-box", probes=probes,
                                  spp=spp, ms=round(med, 3), calls_ms=all_ms)))
        return

    size = a.size or 2048
    uv = M.grid_atlas(sc.info.num_faces, size, size)
    _, texels, q6 = dev.lightmap_texels(size, size, uv=uv)
    m = int(texels.size)
    assert L.mcpt_bake_volume_device(dev._h, C.byref(g), C.byref(sp), d_sh.ptr, None, None, None, st.h) == 0, L.mcpt_last_error()
    d_q, d_e, d_c = upload(q6), hip_rt.DeviceBuffer(m * 24), hip_rt.DeviceBuffer(m * 4)
    floor_ms = (m * 72 + probes * 216) / HBM_BYTES_PER_S * 1e3
    for corners in (False, True):
        med, all_ms = timed(lambda: L.mcpt_volume_irradiance_device(dev._h, C.byref(g), d_sh.ptr, None, d_q.ptr, m, d_e.ptr, d_c.ptr if corners else None,
                                                                    st.h))
        print(json.dumps(dict(base, what="mcpt_volume_irradiance_device", probes=probes, receivers=m, corners=corners, ms=round(med, 4),
                              calls_ms=all_ms, floor_ms=round(floor_ms, 4), over_floor=round(med / floor_ms, 2))))
    sh, E = np.zeros((probes, 9, 3)), np.zeros((m, 3))
    d_sh.to_host_async(sh, st.h)
    d_e.to_host_async(E, st.h)
    st.synchronize()
    t0 = time.perf_counter()
    hE, _ = M.volume_irradiance_host(g, sh, q6[:, :3], q6[:, 3:])
    host_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps(dict(base, what="mcpt_volume_irradiance_host", probes=probes, receivers=m, ms=round(host_ms, 1),
                          same_bits=bool(np.array_equal(E.view(np.uint64), hE.view(np.uint64))))))


if __name__ == "__main__":
    main()
