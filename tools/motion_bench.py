#!/usr/bin/env python3
"""What a shutter frame costs beside static frames of the same sample count.

For every scene and build mode, in one process, the forms alternated, median of three wall times:
  * static   : the one-shot frame, no motion;
  * passes K : a static progressive frame in K equal passes (what cutting a frame into K sample ranges costs by itself);
  * shutter K: the shutter frame in K steps between the scene and a sine field of 1 % of its diagonal, with the milliseconds
               mcpt_device_motion_info reports for the steps' updates.
shutter K - passes K is what the motion itself adds; DESIGN 6g sets it beside K x the ms_total of a refit (tools/animate_bench.py).

    python tools/motion_bench.py --scenes cornell-box:256,veach-mis:100,synthetic:1000000:16 --steps 1,4,16,64

One JSON line per measurement on stdout, each with the library's build id."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import montecarlopathtracing_amd as M                                  # noqa: E402
from animate_bench import MODES, describe, make, sine                  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def passes(dev, spp, k):
    pr = dev.progressive(spp, seed=1)
    while pr.done < spp:
        pr.step((spp + k - 1) // k)
    pr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell-box:256,veach-mis:100,synthetic:1000000:16", help="name:spp (synthetic:faces:spp)")
    ap.add_argument("--modes", default="host,device_sah")
    ap.add_argument("--steps", default="1,4,16,64")
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    a = ap.parse_args()
    for item in a.scenes.split(","):
        name, spp = item.rsplit(":", 1)
        spp = int(spp)
        g = describe(name, a.width, a.height)
        v0 = np.ascontiguousarray(g["v"], dtype=np.float64)
        v1 = sine(v0, 0.01)
        for mode in a.modes.split(","):
            sc, dev = make(g, v0, MODES[mode])
            dev.generateImg(spp, seed=1)                                # workspaces, primary directions
            for k in [int(x) for x in a.steps.split(",") if int(x) <= spp]:
                dev.set_motion(v_end=v1, steps=k)
                dev.generateImg(spp, seed=1)                            # staging, the refit's schedule, the frame's moments: one-off costs
                runs = {"static": [], "passes": [], "shutter": [], "updates": []}
                for _ in range(3):                                      # the three forms alternated
                    dev.clear_motion()
                    runs["static"].append(timed(lambda: dev.generateImg(spp, seed=1)))
                    runs["passes"].append(timed(lambda: passes(dev, spp, k)))
                    dev.set_motion(v_end=v1, steps=k)
                    runs["shutter"].append(timed(lambda: dev.generateImg(spp, seed=1)))
                    runs["updates"].append(dev.motion_info()["ms_updates"])
                info = dev.motion_info()
                dev.clear_motion()
                med = {f: round(statistics.median(r), 3) for f, r in runs.items()}
                print(json.dumps({"scene": name, "mode": mode, "faces": int(v0.shape[0]), "spp": spp, "steps": k, "ms_static": med["static"],
                                  "ms_passes": med["passes"], "ms_shutter": med["shutter"], "ms_updates": med["updates"],
                                  "ms_motion_adds": round(med["shutter"] - med["passes"], 3), "max_cost_ratio": round(info["max_cost_ratio"], 4),
                                  "build_id": M.build_id()}), flush=True)
            dev.close()
            sc.close()


if __name__ == "__main__":
    main()
