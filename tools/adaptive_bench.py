#!/usr/bin/env python3
"""Diagnostic: adaptive frames (mcpt_progressive_create_adaptive) against uniform progressive frames that stop on the frame-level noise
target, on one GPU.

    python tools/adaptive_bench.py [--scenes cornell-box,veach-mis] [--targets 0.05,0.02] [--spp 1024] [--min-spp 16] [--ref-spp 4096]
                                   [--width 1280 --height 720 --seed 0]
    python tools/adaptive_bench.py --one --scenes cornell-box --spp 256 --targets 0.05     # one adaptive frame, for a kernel trace

Uniform: the passes of render_scene's schedule (8, 8, 16, ...) until the frame's rel_error <= target or N.  Adaptive: rel_target = target,
a first pass of min_spp, then the schedule's doubling until no pixel is active or N.  Uniform_same_samples: a uniform frame of N = the
adaptive frame's samples per pixel (rounded down), rendered to the end.  Each form runs twice; the second run's wall time is reported
(the first sizes the frame's buffers).  Prints one JSON line per (scene, target, form): total
samples, passes, wall ms of the passes (each step returns with its pass finished), and the RMS and 90th percentile of the per-pixel
relative error |est - ref| / |ref| (RGB norms, pixels with ref != 0) against a frame of ref_spp samples of another seed.  --one renders a
single adaptive frame and prints the active count after every pass (run it under a kernel trace to time the selection kernels)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run_uniform(M, dev, N, seed, target):
    pr = dev.progressive(N, seed=seed)
    passes, t = [], 0.0
    while True:
        n = M.progressive_next_pass(N, pr.done)
        if n == 0:
            break
        t0 = time.perf_counter()
        pr.step(n)
        t += time.perf_counter() - t0
        passes.append(n)
        if pr.noise().rel_error <= target:
            break
    img = pr.image()
    samples = pr.done * dev.width * dev.height
    pr.close()
    return img, samples, passes, t * 1e3, None


def run_adaptive(M, dev, N, seed, target, min_spp):
    pr = dev.adaptive(N, target, 0.0, min_spp=min_spp, seed=seed)
    passes, active, t = [], [], 0.0
    n = min(N, min_spp)
    while pr.active > 0:
        t0 = time.perf_counter()
        pr.step(n)
        t += time.perf_counter() - t0
        passes.append(n)
        active.append(pr.active)
        n = M.progressive_next_pass(N, pr.done)
    img, cnt = pr.image(), pr.sample_counts()
    pr.close()
    return img, int(cnt.sum()), passes, t * 1e3, active


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell-box,veach-mis")
    ap.add_argument("--targets", default="0.05,0.02")
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--min-spp", type=int, default=16)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--one", action="store_true", help="one adaptive frame of the first scene and target, no reference")
    args = ap.parse_args()
    import numpy as np
    import montecarlopathtracing_amd as M
    from conftest import SCENES
    targets = [float(v) for v in args.targets.split(",")]
    for name in args.scenes.split(","):
        sc = M.Scene(SCENES, name, width=args.width, height=args.height)
        dev = M.Device(sc, 0)
        run_adaptive(M, dev, 32, args.seed + 7, 0.05, 8)           # warm-up: first launches load code objects
        run_uniform(M, dev, 32, args.seed + 7, 0.05)
        if args.one:
            _, samples, passes, ms, active = run_adaptive(M, dev, args.spp, args.seed, targets[0], args.min_spp)
            print(json.dumps({"scene": name, "spp": args.spp, "target": targets[0], "passes": passes, "active_after_pass": active,
                              "samples": samples, "wall_ms": ms}), flush=True)
            return
        ref = dev.generateImg(args.ref_spp, seed=args.seed + 1)
        rn = np.sqrt((ref ** 2).sum(axis=2)).ravel()
        ok = rn > 0

        def errors(img):
            e = np.sqrt(((img - ref) ** 2).sum(axis=2)).ravel()[ok] / rn[ok]
            return float(np.sqrt((e ** 2).mean())), float(np.percentile(e, 90))

        for target in targets:
            budget = None
            for form in ("uniform", "adaptive", "uniform_same_samples"):
                for rep in range(2):           # the second run is reported: the first sizes the frame's buffers for the pass sizes
                    if form == "uniform":
                        img, samples, passes, ms, active = run_uniform(M, dev, args.spp, args.seed, target)
                    elif form == "adaptive":
                        img, samples, passes, ms, active = run_adaptive(M, dev, args.spp, args.seed, target, args.min_spp)
                        budget = samples // (args.width * args.height)
                    else:                      # a uniform frame of N = the adaptive frame's average count, to the end
                        img, samples, passes, ms, active = run_uniform(M, dev, budget, args.seed, 0.0)
                    if rep == 0:
                        ms_first = ms
                rms, p90 = errors(img)
                print(json.dumps({"scene": name, "size": [args.width, args.height], "spp": args.spp, "target": target, "form": form,
                                  "samples": samples, "samples_per_pixel": samples / (args.width * args.height), "passes": len(passes),
                                  "pass_sizes": passes, "active_after_pass": active, "wall_ms": ms, "wall_ms_first_run": ms_first,
                                  "rel_err_rms": rms, "rel_err_p90": p90,
                                  "ref_spp": args.ref_spp, "build_id": M.build_id()}), flush=True)
        dev.close()
        sc.close()


if __name__ == "__main__":
    main()
