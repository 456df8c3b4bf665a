#!/usr/bin/env python3
"""Diagnostic: what a progressive frame's picture costs.

    python tools/display_bench.py [--scene cornell-box --width 1280 --height 720 --spp 16 --calls 15 --time-limit 240]

The scene is rendered to --spp samples on a progressive handle.  Then, for every curve with and without auto-exposure (auto_key 0.18, which
adds the histogram, its 3 KB read-back and a wait for the stream), one warm-up call and --calls (at least 9) timed calls of
mcpt_progressive_display_device into a device buffer, each between two HIP events on one stream; the host clock around the call and the
wait for its end is given too.  The route the library had before to the same bytes -- mcpt_progressive_image into a host frame, then
mcpt_quantize_rgb8 -- is timed by the host clock, as a caller sees it.  One process; --time-limit seconds after its start the process ends
itself.  Medians; one JSON line per result."""
import argparse
import ctypes as C
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cornell-box")
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--time-limit", type=int, default=240)
    a = ap.parse_args()
    a.calls = max(a.calls, 9)
    signal.alarm(a.time_limit)                                   # SIGALRM's default action ends the process

    import hip_rt
    import montecarlopathtracing_amd as M
    from conftest import SCENES
    from montecarlopathtracing_amd._lib import DisplayInfo, check
    L, hip = M.lib(), hip_rt.hip()
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]

    sc = M.Scene(SCENES, a.scene, width=a.width, height=a.height)
    dev = M.Device(sc, 0)
    dev.set_environment([0.5, 0.7, 1.0])
    pr = dev.progressive(a.spp, seed=a.seed)
    pr.step(a.spp)
    px = a.width * a.height
    hip_rt.set_device(0)
    st = hip_rt.Stream()
    out = hip_rt.DeviceBuffer(px * 4)
    e0, e1 = C.c_void_p(), C.c_void_p()
    hip_rt.check(hip.hipEventCreate(C.byref(e0)))
    hip_rt.check(hip.hipEventCreate(C.byref(e1)))
    base = {"scene": a.scene, "width": a.width, "height": a.height, "spp": a.spp, "calls": a.calls}

    # all-zero parameters first -- the earlier route's own bytes -- then every curve under the sRGB transfer
    configs = [("clamp", "linear", False)] + [(c, "srgb", auto) for c in ("clamp", "reinhard", "filmic") for auto in (False, True)]
    for curve, transfer, auto in configs:
        dp = M.make_display(auto_key=0.18 if auto else 0.0, white=4.0 if curve == "reinhard" and not auto else 0.0, curve=curve,
                            transfer=transfer)
        info = DisplayInfo()
        ev_ms, wall_ms = [], []
        for i in range(a.calls + 1):                         # the first call warms up (scratch frame, histogram slots)
            t0 = time.perf_counter()
            hip_rt.check(hip.hipEventRecord(e0, st.h))
            check(L.mcpt_progressive_display_device(pr._h, M.DISPLAY_ESTIMATE, C.byref(dp), out.ptr, C.byref(info), st.h))
            hip_rt.check(hip.hipEventRecord(e1, st.h))
            hip_rt.check(hip.hipEventSynchronize(e1))
            t1 = time.perf_counter()
            t = C.c_float()
            hip_rt.check(hip.hipEventElapsedTime(C.byref(t), e0, e1))
            if i:
                ev_ms.append(t.value)
                wall_ms.append((t1 - t0) * 1e3)
        print(json.dumps(dict(base, route="progressive_display_device", curve=curve, transfer=transfer, auto_exposure=auto,
                              median_event_ms=float(np.median(ev_ms)), min_event_ms=float(np.min(ev_ms)),
                              median_wall_ms=float(np.median(wall_ms)), exposure=info.exposure, counted=info.counted)), flush=True)

    # the earlier route: the fp64 frame to the host, the host loop to bytes
    img = np.zeros((a.height, a.width, 3))
    rgb = np.zeros((a.height, a.width, 3), dtype=np.uint8)
    ip, op = img.ctypes.data_as(C.POINTER(C.c_double)), rgb.ctypes.data_as(C.POINTER(C.c_uint8))
    read_ms, quant_ms = [], []
    for i in range(a.calls + 1):
        t0 = time.perf_counter()
        check(L.mcpt_progressive_image(pr._h, ip, None))
        t1 = time.perf_counter()
        check(L.mcpt_quantize_rgb8(ip, img.size, op))
        t2 = time.perf_counter()
        if i:
            read_ms.append((t1 - t0) * 1e3)
            quant_ms.append((t2 - t1) * 1e3)
    print(json.dumps(dict(base, route="progressive_image + quantize_rgb8", median_wall_ms=float(np.median(np.add(read_ms, quant_ms))),
                          median_image_ms=float(np.median(read_ms)), median_quantize_ms=float(np.median(quant_ms)),
                          frame_bytes=img.nbytes, picture_bytes=rgb.nbytes)), flush=True)
    # and the same bytes: the clamp curve without parameters is that route's picture
    got, _ = pr.display()
    print(json.dumps(dict(base, check="display() == quantize_rgb8(image())", equal=bool(np.array_equal(got, rgb)))), flush=True)
    for e in (e0, e1):
        hip.hipEventDestroy(e)
    out.free()
    st.destroy()
    pr.close()
    dev.close()
    sc.close()


if __name__ == "__main__":
    main()
