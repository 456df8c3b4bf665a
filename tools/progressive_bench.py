#!/usr/bin/env python3
"""Diagnostic: the headline frame as a progressive frame (mcpt_progressive_*) against the one-shot frame, on one GPU.

    python tools/progressive_bench.py [--passes P] [--steps K] [--warmup W] [--scene ... --width ... --height ... --spp ... --seed ...]

The frame is rendered in the passes of render_scene's schedule (8+8+16+32+... for P = 0, the default) or in P equal passes.  Both forms
render into HBM, and each step returns with its pass finished.  Prints one JSON line: ms per frame of both forms, the noise summaries'
own time, rel_error after every pass, and whether the final frame equals the one-shot frame bit for bit.  Scenes are prepared as
bench.py prepares them (its make_scene)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=0, help="0: render_scene's schedule; P > 0: P equal passes")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scene", default="cornell-box")
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tris", type=int, default=10_000_000, help="--scene synthetic: number of lattice triangles")
    ap.add_argument("--build", default="default", choices=["default", "host", "device", "device_fast", "device_sah"])
    args = ap.parse_args()
    if args.steps < 1 or args.passes < 0:
        ap.error("--steps >= 1 and --passes >= 0")

    import numpy as np
    import bench
    import hip_rt
    import montecarlopathtracing_amd as M
    scene, _, build_mode = bench.make_scene(M, args, talk=False)
    H, W, N = scene.info.height, scene.info.width, args.spp
    dev = M.Device(scene, 0, build=build_mode)
    if args.passes > 0:
        passes = [N // args.passes + (1 if i < N % args.passes else 0) for i in range(args.passes)]
        passes = [n for n in passes if n > 0]
    else:
        passes, done = [], 0
        while M.progressive_next_pass(N, done) > 0:
            passes.append(M.progressive_next_pass(N, done))
            done += passes[-1]
    buf, stream = hip_rt.DeviceBuffer(H * W * 24), hip_rt.Stream()

    def one_shot():
        dev.render_device(buf.ptr.value, N, args.seed, stream=stream.h.value)
        stream.synchronize()

    def progressive():
        pr = dev.progressive(N, seed=args.seed)
        t_steps, t_noise, rel = 0.0, 0.0, []
        for n in passes:
            t = time.perf_counter()
            pr.step(n)
            t_steps += time.perf_counter() - t
            t = time.perf_counter()
            rel.append(pr.noise().rel_error)
            t_noise += time.perf_counter() - t
        return pr, t_steps, t_noise, rel

    for _ in range(args.warmup):
        one_shot()
        progressive()[0].close()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one_shot()
    ms_one = (time.perf_counter() - t0) / args.steps * 1e3
    ms_steps, ms_noise = [], []
    for i in range(args.steps):
        pr, t_steps, t_noise, rel = progressive()
        ms_steps.append(t_steps * 1e3)
        ms_noise.append(t_noise * 1e3)
        if i < args.steps - 1:
            pr.close()
    ref = np.zeros((H, W, 3))
    buf.to_host_async(ref, stream.h)
    stream.synchronize()
    img = pr.image()
    pr.close()
    dev.close()
    ms_prog = sum(ms_steps) / len(ms_steps)
    print(json.dumps({
        "metric": "progressive frame (diagnostic): %s %dx%d SPP=%d in %d passes %s" % (args.scene, W, H, N, len(passes), passes),
        "passes": passes, "ms_per_frame_one_shot": ms_one, "ms_per_frame_progressive": ms_prog,
        "progressive_over_one_shot": ms_prog / ms_one, "ms_noise_summaries_per_frame": sum(ms_noise) / len(ms_noise),
        "rel_error_after_pass": rel, "final_equals_one_shot_bitwise": bool(np.array_equal(img.view(np.uint64), ref.view(np.uint64))),
        "steps": args.steps, "warmup": args.warmup, "build_id": M.build_id(),
        "note": "wall time of the passes (each step returns with its pass finished); the noise summaries after each pass timed apart"}),
        flush=True)


if __name__ == "__main__":
    main()
