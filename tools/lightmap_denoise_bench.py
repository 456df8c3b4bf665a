#!/usr/bin/env python3
"""Diagnostic: what the lightmap denoiser costs and what it buys.

    python tools/lightmap_denoise_bench.py time  [--scene cornell-box --size 2048 --spp 64 --calls 5]
    python tools/lightmap_denoise_bench.py sweep [--size 512 --spp 64 --ref-spp 4096]
    python tools/lightmap_denoise_bench.py buys  [--size 512 --ref-spp 4096]

time : the scene under grid_atlas, baked once into device buffers; one warm-up call and --calls timed calls of
       mcpt_lightmap_denoise_device (defaults, dilate 2) on those buffers, each between two HIP events on one stream (6n's method); the
       bake itself is timed the same way beside it.  Medians.
sweep: glassroom on its own chart, cornell-box and veach-mis under grid_atlas: RMS relative error of the raw and the denoised --spp bake
       against a --ref-spp bake of another seed, for sigma_l in {1, 2, 4, 8}, sigma_p in {0.25, 1, 4}, K in {4, 5}.
buys : cornell-box (grid_atlas) and glassroom (own chart): raw and denoised RMS and 90th percentile at spp 64, 256 and 1024, and the raw
       sample count that would reach the denoised 64-sample error, by the 1 / sqrt(spp) law from the raw 64-sample error.
One process; --time-limit seconds after its start the process ends itself.  One JSON line per result."""
import argparse
import ctypes as C
import json
import os
import signal
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel_err(E, ref, mask):
    e, r = E[mask], ref[mask]
    return np.sqrt(((e - r) ** 2).sum(axis=1)) / np.sqrt((r ** 2).sum(axis=1))


def rms(x):
    return float(np.sqrt((x ** 2).mean()))


def open_scene(M, name, size):
    """(scene, chart or None) as the tests chart them: glassroom carries vt, the others get grid_atlas"""
    if name == "glassroom":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from conftest import extra_scene_dir
        return M.Scene(extra_scene_dir(), name, width=64, height=36), None
    sc = M.Scene(os.path.join(ROOT, "scenes") + os.sep, name, width=64, height=36)
    return sc, M.grid_atlas(sc.info.num_faces, size, size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["time", "sweep", "buys"])
    ap.add_argument("--scene", default="cornell-box")
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--spp", type=int, default=64)
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

    if a.mode == "time":
        import hip_rt
        L, hip = M.lib(), hip_rt.hip()
        hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        hip.hipEventSynchronize.argtypes = [C.c_void_p]
        hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        W = H = a.size or 2048
        sc, uv = open_scene(M, a.scene, W)
        dev = M.Device(sc, 0)
        hip_rt.set_device(0)
        st = hip_rt.Stream()
        e0, e1 = C.c_void_p(), C.c_void_p()
        hip_rt.check(hip.hipEventCreate(C.byref(e0)))
        hip_rt.check(hip.hipEventCreate(C.byref(e1)))

        def timed(call):
            ms = []
            for i in range(a.calls + 1):                         # the first call warms up
                hip_rt.check(hip.hipEventRecord(e0, st.h))
                rc = call()
                assert rc == 0, L.mcpt_last_error()
                hip_rt.check(hip.hipEventRecord(e1, st.h))
                hip_rt.check(hip.hipEventSynchronize(e1))
                t = C.c_float()
                hip_rt.check(hip.hipEventElapsedTime(C.byref(t), e0, e1))
                ms.append(t.value)
            return float(np.median(ms[1:])), [round(v, 3) for v in ms[1:]]

        n = W * H
        d_uv = None
        if uv is not None:
            d_uv = hip_rt.DeviceBuffer(uv.nbytes)
            hip_rt.check(hip.hipMemcpy(d_uv.ptr, uv.ctypes.data_as(C.c_void_p), uv.nbytes, 1))
        uvp = d_uv.ptr if d_uv else None
        irr, err, out, own = hip_rt.DeviceBuffer(n * 24), hip_rt.DeviceBuffer(n * 24), hip_rt.DeviceBuffer(n * 24), hip_rt.DeviceBuffer(n * 4)
        lp = M.LightmapParams(W, H, a.spp, 0, a.seed, 0, 0, (C.c_int32 * 2)(0, 0))
        med, all_ms = timed(lambda: L.mcpt_bake_lightmap_device(dev._h, uvp, C.byref(lp), irr.ptr, err.ptr, None, own.ptr, None, st.h))
        owner = np.zeros(n, dtype=np.int32)
        own.to_host_async(owner, st.h)
        st.synchronize()
        covered = int((owner >= 0).sum())
        print(json.dumps(dict(base, what="mcpt_bake_lightmap_device", scene=a.scene, width=W, height=H, spp=a.spp, dilate=0, covered=covered,
                              ms=round(med, 3), calls_ms=all_ms)))
        for K, dilate in ((M.LIGHTMAP_DENOISE_ITERATIONS, 2), (M.LIGHTMAP_DENOISE_ITERATIONS, 0), (0, 0)):
            dp = M.LightmapDenoiseParams(W, H, K, dilate, 0.0, 0.0, (C.c_int32 * 2)(0, 0))
            med, all_ms = timed(lambda: L.mcpt_lightmap_denoise_device(dev._h, uvp, C.byref(dp), irr.ptr, err.ptr, out.ptr, own.ptr, st.h))
            print(json.dumps(dict(base, what="mcpt_lightmap_denoise_device", scene=a.scene, width=W, height=H, iterations=K, dilate=dilate,
                                  covered=covered, ms=round(med, 3), calls_ms=all_ms)))
        return

    W = H = a.size or 512
    if a.mode == "sweep":
        for name in ("glassroom", "cornell-box", "veach-mis"):
            sc, uv = open_scene(M, name, W)
            dev = M.Device(sc, 0)
            ref, _, _, own = dev.bake_lightmap(W, H, a.ref_spp, uv=uv, seed=a.seed + 1000)
            lit = (own >= 0) & (ref > 0).all(axis=2)
            E, S, _, _ = dev.bake_lightmap(W, H, a.spp, uv=uv, seed=a.seed)
            raw = rms(rel_err(E, ref, lit))
            print(json.dumps(dict(base, what="sweep-raw", scene=name, size=W, spp=a.spp, covered=int((own >= 0).sum()), lit=int(lit.sum()),
                                  raw_rms=round(raw, 5))))
            for K in (4, 5):
                for sl in (1.0, 2.0, 4.0, 8.0):
                    for sp in (0.25, 1.0, 4.0):
                        out, _ = dev.denoise_lightmap(E, S, uv=uv, iterations=K, sigma_l=sl, sigma_p=sp)
                        den = rms(rel_err(out, ref, lit))
                        shift = float(out[lit].mean() / ref[lit].mean() - 1.0)
                        print(json.dumps(dict(what="sweep", scene=name, K=K, sigma_l=sl, sigma_p=sp, rms=round(den, 5), ratio=round(den / raw, 4),
                                              mean_shift=round(shift, 5))))
            dev.close()
            sc.close()
        return

    for name in ("cornell-box", "glassroom"):
        sc, uv = open_scene(M, name, W)
        dev = M.Device(sc, 0)
        ref, _, _, own = dev.bake_lightmap(W, H, a.ref_spp, uv=uv, seed=a.seed + 1000)
        lit = (own >= 0) & (ref > 0).all(axis=2)
        first = None
        for spp in (64, 256, 1024):
            E, S, _, _ = dev.bake_lightmap(W, H, spp, uv=uv, seed=a.seed)
            out, _ = dev.denoise_lightmap(E, S, uv=uv)
            r, d = rel_err(E, ref, lit), rel_err(out, ref, lit)
            rec = dict(base, what="buys", scene=name, size=W, spp=spp, covered=int((own >= 0).sum()), lit=int(lit.sum()), raw_rms=round(rms(r), 5),
                       raw_p90=round(float(np.percentile(r, 90)), 5), den_rms=round(rms(d), 5), den_p90=round(float(np.percentile(d, 90)), 5))
            if first is None:
                first = rec
                rec["raw_spp_for_den_rms"] = int(round(spp * (rec["raw_rms"] / rec["den_rms"]) ** 2))
            print(json.dumps(rec))
        dev.close()
        sc.close()


if __name__ == "__main__":
    main()
