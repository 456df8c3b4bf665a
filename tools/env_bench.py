#!/usr/bin/env python3
"""Diagnostic: what an environment light costs.  The headline frame (cornell-box 1280x720, SPP 256 by default) on one GPU without an
environment, under a constant sky and under a 2048x1024 map, the three alternated in one process so that they see the same clocks and the
same caches; three frames of each by default, after one warm-up frame of each.  The map is made from a seed (a bright band over a smooth
sky); its tables are built on the host when it is set, and that time is reported as well.

    python tools/env_bench.py [--scene cornell-box] [--width 1280 --height 720] [--spp 256] [--frames 3] [--map 2048x1024] [--seed 0]

Prints one JSON line per frame (form, device ms of the frame = mcpt_stats.ms_total, ms of the trace launches, shadow and bounce rays) and a
summary line: the median of each form, their ratios to the frame without an environment, and the seconds set_environment took."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sky_map(w, h, seed):
    rng = np.random.default_rng(seed)
    y = np.linspace(1.0, 0.05, h)[:, None, None]
    m = np.broadcast_to(y * np.array([0.5, 0.7, 1.0]), (h, w, 3)).copy()
    m += rng.random((h, w, 3)) * 0.05
    m[h // 8:h // 8 + max(h // 64, 1), w // 3:w // 3 + max(w // 64, 1)] = 200.0      # a small, very bright sun
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cornell-box")
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--map", default="2048x1024")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import montecarlopathtracing_amd as M
    mw, mh = (int(v) for v in args.map.split("x"))
    big = sky_map(mw, mh, args.seed)
    sc = M.Scene(os.path.join(ROOT, "scenes") + os.sep, args.scene, width=args.width, height=args.height)
    dev = M.Device(sc, 0)
    forms = {"none": None, "constant": [0.6, 0.8, 1.0], "map": big}
    times = {k: [] for k in forms}
    build_s = []
    for i in range(args.frames + 1):                       # frame 0 of each form: warm-up (buffers sized, code loaded)
        for name, rgb in forms.items():
            t0 = time.perf_counter()
            dev.set_environment(rgb)
            if name == "map":
                build_s.append(time.perf_counter() - t0)
            st = M.Stats()
            dev.generateImg(args.spp, seed=args.seed, stats=st)
            if i == 0:
                continue
            times[name].append(st.ms_total)
            print(json.dumps({"form": name, "frame": i, "ms_total": round(st.ms_total, 3), "ms_trace": round(st.ms_trace, 3),
                              "rays_shadow": st.rays_shadow, "rays_bounce": st.rays_bounce, "launches": st.launches}), flush=True)
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({"scene": args.scene, "width": args.width, "height": args.height, "spp": args.spp, "map": args.map,
                      "build_id": M.build_id(), "median_ms": {k: round(v, 3) for k, v in med.items()},
                      "over_none": {k: round(v / med["none"], 4) for k, v in med.items()},
                      "set_environment_s": round(statistics.median(build_s), 4)}), flush=True)
    dev.close()
    sc.close()


if __name__ == "__main__":
    main()
