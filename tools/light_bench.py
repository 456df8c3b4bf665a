#!/usr/bin/env python3
"""Diagnostic: what MCPT_LIGHTS_ONE and MCPT_LIGHTS_TREE buy on a room of many lights (tests/light_scenes.py).  The 10- and 40-light rooms at
1280x720, SPP 256 by default, on one GPU under "all" (every light at every vertex), "one" (one light per vertex from the global table) and
"tree" (one light per vertex from the light tree: distance and horizon), the modes alternated in one
process so that they see the same clocks and the same caches; three frames of each by default, after one warm-up frame of each.

    python tools/light_bench.py [--lights 10,40] [--width 1280 --height 720] [--spp 256] [--frames 3] [--seed 0]
                                [--rmse-lights 40 --rmse-width 640 --rmse-height 360 --rmse-spp 64 --rmse-ref-spp 4096]

Prints one JSON line per frame (mode, device ms of the frame = mcpt_stats.ms_total, shadow rays) and one summary line per room: the median
of each mode, the shadow rays, the bytes of wavefront state per path (wavefront.hip: wf_bytes_per_path, restated here) and the chunks a
frame of that many paths takes in the library's default workspace (half of the free HBM; an estimate from hipMemGetInfo, null without torch).
--rmse-lights N (0: skip): on the N-light room, the RMSE against an "all" frame of --rmse-ref-spp samples of "all" at --rmse-spp and of
"one" and of "tree", each at the sample count that takes the same measured time (the ratio of the modes' median ms per sample, measured at
--rmse-spp)."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def bytes_per_path(planes):
    """wf_bytes_per_path of `planes` shadow planes"""
    state = 4 + (6 + 3 * planes + (3 if planes == 1 else 6)) * 8 + planes * 4 + 4 + planes * 4 + 4 + 3 * 8
    return 2 * state + planes * 3 * 8


def chunks(paths, bpp):
    try:
        import torch
        free_b, _ = torch.cuda.mem_get_info()
    except Exception:
        return None
    cap = (free_b // 2 - 64 * 1024) // (bpp + 24)
    return int(-(-paths // max(cap, 1)))


def frames(M, dev, modes, spp, n, seed, label):
    times = {m: [] for m in modes}
    shadow = {}
    for i in range(n + 1):                                  # frame 0 of each mode: warm-up (buffers sized, code loaded)
        for m in modes:
            dev.set_light_sampling(m)
            st = M.Stats()
            dev.generateImg(spp, seed=seed, stats=st)
            if i == 0:
                continue
            times[m].append(st.ms_total)
            shadow[m] = st.rays_shadow
            shadow[m + "_skipped"] = st.shadow_skipped
            print(json.dumps(dict(label, mode=m, frame=i, spp=spp, ms_total=round(st.ms_total, 3), ms_trace=round(st.ms_trace, 3),
                                  rays_shadow=st.rays_shadow, shadow_skipped=st.shadow_skipped, rays_bounce=st.rays_bounce, launches=st.launches)), flush=True)
    dev.set_light_sampling(None)
    return {m: statistics.median(v) for m, v in times.items()}, shadow


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lights", default="10,40")
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rmse-lights", type=int, default=40)
    ap.add_argument("--rmse-width", type=int, default=640)
    ap.add_argument("--rmse-height", type=int, default=360)
    ap.add_argument("--rmse-spp", type=int, default=64)
    ap.add_argument("--rmse-ref-spp", type=int, default=4096)
    args = ap.parse_args()
    import light_scenes
    import montecarlopathtracing_amd as M
    d = tempfile.mkdtemp(prefix="light_bench_") + os.sep
    for nl in [int(v) for v in args.lights.split(",") if v]:
        name = "room%d" % nl
        light_scenes.write(d, name, nl, args.width, args.height)
        sc = M.Scene(d, name, width=args.width, height=args.height)
        dev = M.Device(sc, 0)
        med, shadow = frames(M, dev, ("all", "one", "tree"), args.spp, args.frames, args.seed, {"lights": nl})
        paths = args.width * args.height * args.spp
        bpp = {"all": bytes_per_path(nl), "one": bytes_per_path(1), "tree": bytes_per_path(1)}
        print(json.dumps({"lights": nl, "width": args.width, "height": args.height, "spp": args.spp, "build_id": M.build_id(),
                          "median_ms": {k: round(v, 3) for k, v in med.items()}, "all_over_one": round(med["all"] / med["one"], 3),
                          "tree_over_one": round(med["tree"] / med["one"], 3),
                          "rays_shadow": shadow, "bytes_per_path": bpp, "chunks": {k: chunks(paths, v) for k, v in bpp.items()}}), flush=True)
        dev.close()
        sc.close()
    if args.rmse_lights > 0:
        nl, w, h = args.rmse_lights, args.rmse_width, args.rmse_height
        name = "rmse%d" % nl
        light_scenes.write(d, name, nl, w, h)
        sc = M.Scene(d, name, width=w, height=h)
        dev = M.Device(sc, 0)
        ref = dev.generateImg(args.rmse_ref_spp, seed=args.seed + 1000)
        med, _ = frames(M, dev, ("all", "one", "tree"), args.rmse_spp, args.frames, args.seed, {"lights": nl, "rmse": True})

        def rmse(a):
            return float(np.sqrt(np.mean((a - ref) ** 2)))
        out = {"lights": nl, "width": w, "height": h, "ref_spp": args.rmse_ref_spp, "all_spp": args.rmse_spp, "all_ms": round(med["all"], 3)}
        for mode in ("one", "tree"):
            spp_m = max(1, int(round(args.rmse_spp * med["all"] / med[mode])))
            dev.set_light_sampling(mode)
            dev.generateImg(spp_m, seed=args.seed)                        # (sizes the buffers for this count)
            ms = []
            for _ in range(args.frames):
                st = M.Stats()
                img = dev.generateImg(spp_m, seed=args.seed, stats=st)
                ms.append(st.ms_total)
            out.update({mode + "_spp": spp_m, mode + "_ms": round(statistics.median(ms), 3), mode + "_rmse": round(rmse(img), 6)})
            img = dev.generateImg(args.rmse_spp, seed=args.seed)
            out[mode + "_rmse_at_all_spp"] = round(rmse(img), 6)
        dev.set_light_sampling(None)
        full = dev.generateImg(args.rmse_spp, seed=args.seed)
        out.update({"all_rmse": round(rmse(full), 6), "ref_mean": round(float(ref.mean()), 6)})
        print(json.dumps(out), flush=True)
        dev.close()
        sc.close()


if __name__ == "__main__":
    main()
