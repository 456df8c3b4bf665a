#!/usr/bin/env python3
"""What a geometry update costs and what a refitted hierarchy costs to walk.

For every scene and build mode, in one process, the forms alternated, median of three:
  * ms per update by refit and by rebuild, split as mcpt_update_info splits it, beside the ms of what there was before updates existed:
    mcpt_scene_create + mcpt_device_create_ex on the moved vertices + freeing the old pair ("recreate");
  * ms per frame and node visits / triangle tests per ray on the refitted hierarchy, the rebuilt one and a fresh device, after a sine
    field of amplitude 0, 1 %, 5 % and 25 % of the scene's diagonal on every vertex, with cost_after / (cost of the first build).

    python tools/animate_bench.py --scenes cornell-box,veach-mis,synthetic:20000,synthetic:1000000,synthetic:10000000

One JSON line per measurement on stdout."""
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
from montecarlopathtracing_amd import synthetic                        # noqa: E402

MODES = {"host": M.BUILD_HOST, "device": M.BUILD_DEVICE, "device_fast": M.BUILD_DEVICE_FAST, "device_sah": M.BUILD_DEVICE_SAH}


def describe(name, width, height):
    """the arrays of mcpt_scene_create for a scene (file scenes lose their textures: only build and walk are measured)"""
    if name.startswith("synthetic:"):
        return synthetic.generate(int(name.split(":")[1]), width=width, height=height)
    sc = M.Scene(os.path.join(ROOT, "scenes") + os.sep, name, width=width, height=height)
    g, m, _ = sc.faces()
    i = sc.info
    rec = np.array([sc.material(k)[1] for k in range(i.num_materials)])
    lights = [sc.light(k) for k in range(i.num_lights)]
    d = dict(v=np.ascontiguousarray(g[:, :9]), vn=np.ascontiguousarray(g[:, 9:18]), material=m, material_rec=rec,
             material_names=[sc.material(k)[0] for k in range(i.num_materials)],
             light_material=np.array([l[2] for l in lights], dtype=np.int32), light_radiance=np.array([l[1] for l in lights]),
             eye=list(i.eye), look_at=list(i.look_at), up=list(i.up), fovy=i.fovy, width=width, height=height)
    sc.close()
    return d


def make(g, v, build):
    sc = M.Scene.from_arrays(v, g["vn"], g["material"], g["material_rec"], g["light_material"], g["light_radiance"], g["eye"], g["look_at"],
                             g["up"], g["fovy"], g["width"], g["height"], material_names=g["material_names"], defer_build=build != M.BUILD_HOST)
    return sc, M.Device(sc, 0, build=build)


def sine(v, amplitude, phase=0.0):
    p = v.reshape(-1, 3)
    d = float(np.linalg.norm(p.max(axis=0) - p.min(axis=0)))
    k = 2.0 * np.pi / (0.37 * d)
    disp = np.stack([np.sin(k * p[:, 1] + 0.3 + phase), np.sin(k * p[:, 2] + 1.1 + phase), np.sin(k * p[:, 0] + 2.3 + phase)], axis=1)
    return np.ascontiguousarray((p + amplitude * d * disp).reshape(-1, 9))


def frame(dev, spp):
    dev.generateImg(spp, seed=1)
    ms, st = [], M.Stats()
    for _ in range(3):
        dev.generateImg(spp, seed=1, stats=st)
        ms.append(st.ms_total)
    return {"ms_frame": statistics.median(ms), "nodes_per_ray": st.node_visits / max(st.rays, 1), "tris_per_ray": st.tri_tests / max(st.rays, 1)}


def emit(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell-box,veach-mis,synthetic:20000")
    ap.add_argument("--modes", default="host,device_fast,device_sah")
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--amplitudes", default="0,0.01,0.05,0.25")
    a = ap.parse_args()
    for name in a.scenes.split(","):
        g = describe(name, a.width, a.height)
        v0 = np.ascontiguousarray(g["v"], dtype=np.float64)
        moved = [sine(v0, 0.01, phase=0.3 * k) for k in range(4)]
        for mode in a.modes.split(","):
            build = MODES[mode]
            sc, dev = make(g, v0, build)
            dev.update_vertices(moved[3], mode="refit")                 # staging and the schedule are one-off costs: not in the medians
            first = dev.update_vertices(v0, mode="rebuild")
            runs = {"refit": [], "rebuild": [], "recreate": []}
            for k in range(3):                                          # the three forms alternated
                runs["refit"].append(dev.update_vertices(moved[k], mode="refit"))
                runs["rebuild"].append(dev.update_vertices(moved[k], mode="rebuild"))
                t0 = time.perf_counter()
                sc2, dev2 = make(g, moved[k], build)
                dev.close()
                sc.close()
                runs["recreate"].append({"ms_total": (time.perf_counter() - t0) * 1e3})
                sc, dev = sc2, dev2
                dev.update_vertices(moved[k], mode="refit")             # (the new pair's one-off costs, again outside the medians)
            out = {"scene": name, "mode": mode, "faces": int(v0.shape[0])}
            for form, r in runs.items():
                for key in ("ms_reference", "ms_hierarchy", "ms_tables", "ms_total"):
                    if key in r[0]:
                        out["%s_%s" % (form, key)] = round(statistics.median(x[key] for x in r), 3)
            emit(kind="update", **out)
            base_cost = first["cost_after"]
            for amp in [float(x) for x in a.amplitudes.split(",")]:
                v = sine(v0, amp)
                dev.update_vertices(v0, mode="rebuild")
                info = dev.update_vertices(v, mode="refit")
                row = {"scene": name, "mode": mode, "amplitude": amp, "cost_ratio": info["cost_after"] / base_cost}
                row.update({"refit_" + k: round(x, 4) for k, x in frame(dev, a.spp).items()})
                dev.update_vertices(v, mode="rebuild")
                row.update({"rebuilt_" + k: round(x, 4) for k, x in frame(dev, a.spp).items()})
                fsc, fdev = make(g, v, build)
                row.update({"fresh_" + k: round(x, 4) for k, x in frame(fdev, a.spp).items()})
                fdev.close()
                fsc.close()
                emit(kind="frame", **row)
            dev.close()
            sc.close()


if __name__ == "__main__":
    main()
