#!/usr/bin/env python3
"""Diagnostic: the a-trous denoiser of progressive frames (mcpt_progressive_denoise_device), its time and what it does to the error.

    python tools/denoise_bench.py [--scene cornell-box --width 1280 --height 720 --spp 256 --calls 20]     # timing
    python tools/denoise_bench.py --quality [--spps 8,16,64 --width 1280 --height 720 --ref-spp 4096]      # error ratios
    python tools/denoise_bench.py --sweep [--width 320 --height 180]                                       # defaults against neighbours
    python tools/denoise_bench.py --lens --sweep [--width 320 --height 180]       # under a lens: raw, first-hit-guided, sample-guided
    python tools/denoise_bench.py --lens [--scene cornell-box --width 1280 --height 720 --spp 16 --calls 30]   # sample AOVs + guided filter, ms

Timing: the scene rendered to --spp samples in render_scene's passes, then one warm-up call (it also computes the AOVs) and --calls timed
calls of mcpt_progressive_denoise_device with the defaults, each between two HIP events on one stream; prints the median and the
algorithmic bytes and FP64 operations of one iteration.  Quality: for N in --spps, the RMS error over the surface pixels of the denoised
frame and of the estimate against a frame of --ref-spp samples of another seed, their ratio and the relative shift of the mean over the
surface pixels.  Sweep: the same ratio at N = 16 for a grid of (iterations, sigma_l, sigma_z) on cornell-box, veach-mis and glassroom.
--lens: the frames are rendered under a lens (jitter, aperture LENS_APERTURE[scene], focused at the look_at distance).  With --sweep, per
scene at N = 16, seed 7: the RMS error over ALL owned pixels (the filtered sets of the two filters differ) against a --ref-spp frame of
seed 99 under the same lens, of the estimate, of denoise() and of denoise_guided() for sigma_a in 0.02 .. 0.5 at G in 4, 16, 64 (G = 64 on a
handle of 64 samples per pixel of which N are rendered), and the relative shift of the frame's mean.  Without --sweep: the median of
--calls timed calls of mcpt_progressive_denoise_guided_device with the defaults (sample AOVs cached) and of calls that compute the sample
AOVs again (the default G after another G; host clock around the synchronised call, less the filter's median).
One JSON line per result."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# algorithmic traffic and arithmetic of one iteration per surface pixel (k_denoise_atrous): 25 taps read the neighbour's guide record
# (48 B: normal, depth, material) and its (e, v) record (32 B); the 3 x 3 variance prefilter reads 9 materials (4 B) and variances (8 B);
# one (e, v) record is written.  FP64 operations per tap: normal dot 5, max + 7 squarings 8, depth term 6, luminance 5 + difference and
# division 3, weight 4 (+ one exp), sums 3 + 3 + 3; prefilter 4 per tap, 3 for g and the luminance denominator.
BYTES_PER_PIXEL = 25 * (48 + 32) + 9 * (4 + 8) + 32
FLOPS_PER_PIXEL = 25 * (5 + 8 + 6 + 8 + 4 + 9) + 9 * 4 + 3 + 5


def _base(name):
    from conftest import SCENES, extra_scene_dir
    return extra_scene_dir() if name == "glassroom" else SCENES


def _open(M, name, w, h):
    sc = M.Scene(_base(name), name, width=w, height=h)
    return sc, M.Device(sc, 0)


def _render(M, dev, spp, seed):
    pr = dev.progressive(spp, seed=seed)
    while True:
        n = M.progressive_next_pass(spp, pr.done)
        if n == 0:
            break
        pr.step(n)
    return pr


def timing(M, a):
    import hip_rt
    sc, dev = _open(M, a.scene, a.width, a.height)
    pr = _render(M, dev, a.spp, a.seed)
    from montecarlopathtracing_amd._lib import check
    L, hip = M.lib(), hip_rt.hip()
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]
    hip_rt.set_device(0)
    st = hip_rt.Stream()
    buf = hip_rt.DeviceBuffer(a.width * a.height * 3 * 8)
    e0, e1 = C.c_void_p(), C.c_void_p()
    hip_rt.check(hip.hipEventCreate(C.byref(e0)))
    hip_rt.check(hip.hipEventCreate(C.byref(e1)))
    check(L.mcpt_progressive_denoise_device(pr._h, None, buf.ptr, st.h))      # warm-up (AOVs, workspace)
    st.synchronize()
    ms = []
    for _ in range(a.calls):
        hip_rt.check(hip.hipEventRecord(e0, st.h))
        check(L.mcpt_progressive_denoise_device(pr._h, None, buf.ptr, st.h))
        hip_rt.check(hip.hipEventRecord(e1, st.h))
        hip_rt.check(hip.hipEventSynchronize(e1))
        t = C.c_float()
        hip_rt.check(hip.hipEventElapsedTime(C.byref(t), e0, e1))
        ms.append(t.value)
    aov = pr.aovs()
    emit = [m for m in range(sc.info.num_materials) if sc.material(m)[2][3] >= 0]
    surface = int(((aov["material"] >= 0) & ~np.isin(aov["material"], emit)).sum())
    it = 5
    print(json.dumps({"scene": a.scene, "width": a.width, "height": a.height, "spp": a.spp, "calls": a.calls,
                      "median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "iterations": it,
                      "surface_pixels": surface, "bytes_per_iteration": BYTES_PER_PIXEL * surface,
                      "fp64_ops_per_iteration": FLOPS_PER_PIXEL * surface, "exp_per_iteration": 25 * surface}))
    for e in (e0, e1):
        hip.hipEventDestroy(e)
    buf.free()
    st.destroy()


def errors(M, name, w, h, spps, ref_spp, params_list, seed=7):
    import denoise_ref as R
    sc, dev = _open(M, name, w, h)
    ref = dev.generateImg(ref_spp, seed=99)
    emit = {m for m in range(sc.info.num_materials) if sc.material(m)[2][3] >= 0}
    for n in spps:
        pr = dev.progressive(n, seed=seed)
        pr.step(n)
        surf = R.surface_material(pr.aovs()["material"], np.ones((h, w), dtype=bool), emit) >= 0
        est = pr.image()
        raw = float(np.sqrt(np.mean((est[surf] - ref[surf]) ** 2)))
        for p in params_list:
            dn = pr.denoise(*p)
            rms = float(np.sqrt(np.mean((dn[surf] - ref[surf]) ** 2)))
            shift = (float(dn[surf].mean()) - float(est[surf].mean())) / float(est[surf].mean())
            print(json.dumps({"scene": name, "width": w, "height": h, "spp": n, "ref_spp": ref_spp, "iterations": p[0], "sigma_l": p[1],
                              "sigma_z": p[2], "rms_raw": raw, "rms_denoised": rms, "ratio": rms / raw, "mean_shift": shift}), flush=True)
        pr.close()


# the lens of --lens: aperture per scene, so that the blur circle of the scene's surfaces has a radius of about 4 pixels at 320 x 180 (every
# camera file looks at a point at distance 1, far in front of the geometry: the whole frame is out of focus)
LENS_APERTURE = {"cornell-box": 0.01, "veach-mis": 0.01, "glassroom": 0.02}
SIGMA_AS = (0.02, 0.05, 0.1, 0.2, 0.5)
GUIDE_COUNTS = (4, 16, 64)


def lens_errors(M, name, w, h, n, ref_spp, seed=7):
    sc, dev = _open(M, name, w, h)
    dev.set_lens(jitter=True, aperture=LENS_APERTURE[name])
    ref = dev.generateImg(ref_spp, seed=99)
    rms = lambda a: float(np.sqrt(np.mean((a - ref) ** 2)))      # noqa: E731
    base = {"scene": name, "width": w, "height": h, "spp": n, "ref_spp": ref_spp, "aperture": LENS_APERTURE[name]}
    for spp, counts in ((n, [G for G in GUIDE_COUNTS if G <= n]), (max(GUIDE_COUNTS), [G for G in GUIDE_COUNTS if G > n])):
        pr = dev.progressive(spp, seed=seed)                      # G <= spp: the larger G on a handle of that many samples, n of them rendered
        pr.step(n)
        est = pr.image()
        first = pr.denoise()
        raw, rf = rms(est), rms(first)
        if spp == n:
            print(json.dumps(dict(base, filter="first-hit", rms_raw=raw, rms=rf, ratio_raw=rf / raw,
                                  mean_shift=(float(first.mean()) - float(est.mean())) / float(est.mean()))), flush=True)
        for G in counts:
            for sa in SIGMA_AS:
                dn = pr.denoise_guided(samples=G, sigma_a=sa)
                r = rms(dn)
                print(json.dumps(dict(base, filter="samples", G=G, sigma_a=sa, rms_raw=raw, rms=r, ratio_raw=r / raw, ratio_first=r / rf,
                                      mean_shift=(float(dn.mean()) - float(est.mean())) / float(est.mean()))), flush=True)
        pr.close()


def lens_timing(M, a):
    import time
    import hip_rt
    from montecarlopathtracing_amd._lib import check
    sc, dev = _open(M, a.scene, a.width, a.height)
    dev.set_lens(jitter=True, aperture=LENS_APERTURE[a.scene])
    pr = dev.progressive(a.spp, seed=a.seed)
    pr.step(a.spp)
    L, hip = M.lib(), hip_rt.hip()
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]
    hip_rt.set_device(0)
    st = hip_rt.Stream()
    buf = hip_rt.DeviceBuffer(a.width * a.height * 3 * 8)
    e0, e1 = C.c_void_p(), C.c_void_p()
    hip_rt.check(hip.hipEventCreate(C.byref(e0)))
    hip_rt.check(hip.hipEventCreate(C.byref(e1)))
    check(L.mcpt_progressive_denoise_guided_device(pr._h, None, None, buf.ptr, st.h))      # warm-up (sample AOVs, workspace)
    st.synchronize()
    ms = []
    for _ in range(a.calls):
        hip_rt.check(hip.hipEventRecord(e0, st.h))
        check(L.mcpt_progressive_denoise_guided_device(pr._h, None, None, buf.ptr, st.h))
        hip_rt.check(hip.hipEventRecord(e1, st.h))
        hip_rt.check(hip.hipEventSynchronize(e1))
        t = C.c_float()
        hip_rt.check(hip.hipEventElapsedTime(C.byref(t), e0, e1))
        ms.append(t.value)
    G = min(a.spp, 16)
    other = M.GuideParams(max(1, G - 1), 0, 0.0)
    again = []
    for _ in range(max(3, a.calls // 3)):
        check(L.mcpt_progressive_denoise_guided_device(pr._h, None, C.byref(other), buf.ptr, st.h))
        st.synchronize()
        t0 = time.perf_counter()
        check(L.mcpt_progressive_denoise_guided_device(pr._h, None, None, buf.ptr, st.h))
        st.synchronize()
        again.append((time.perf_counter() - t0) * 1e3)
    filt = float(np.median(ms))
    counts = pr.sample_aovs()["counts"]
    print(json.dumps({"scene": a.scene, "width": a.width, "height": a.height, "spp": a.spp, "calls": a.calls, "aperture": LENS_APERTURE[a.scene],
                      "G": G, "filter_median_ms": filt, "filter_min_ms": float(np.min(ms)), "filter_max_ms": float(np.max(ms)),
                      "aovs_and_filter_median_ms": float(np.median(again)), "sample_aovs_ms": float(np.median(again)) - filt,
                      "rays": int(a.width * a.height * G), "filtered_pixels": int(((counts[..., 0] > 0) & (counts[..., 1] == 0)).sum())}))
    for e in (e0, e1):
        hip.hipEventDestroy(e)
    buf.free()
    st.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cornell-box")
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--spps", default="8,16,64")
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--lens", action="store_true")
    a = ap.parse_args()
    import montecarlopathtracing_amd as M
    if a.lens and a.sweep:
        for name in ("cornell-box", "veach-mis", "glassroom"):
            lens_errors(M, name, a.width, a.height, 16, a.ref_spp)
    elif a.lens:
        lens_timing(M, a)
    elif a.quality:
        for name in ("cornell-box", "glassroom"):
            errors(M, name, a.width, a.height, [int(v) for v in a.spps.split(",")], a.ref_spp, [(0, 0.0, 0.0)])
    elif a.sweep:
        grid = [(k, sl, sz) for k in (4, 5) for sl in (1.0, 2.0, 4.0, 8.0) for sz in (0.02, 0.05, 0.2)]
        for name in ("cornell-box", "veach-mis", "glassroom"):
            errors(M, name, a.width, a.height, [16], a.ref_spp, grid)
    else:
        timing(M, a)


if __name__ == "__main__":
    main()
