#!/usr/bin/env python3
"""Diagnostic: what a lens costs.  The headline frame (cornell-box 1280x720, SPP 256 by default) on one GPU, without a lens and with
MCPT_LENS_JITTER (and, with --aperture, a thin lens as well), the two alternated in one process so that both see the same clocks and the
same caches; three frames of each by default, after one warm-up frame of each.

    python tools/lens_bench.py [--scene cornell-box] [--width 1280 --height 720] [--spp 256] [--frames 3] [--aperture 0] [--seed 0]

Prints one JSON line per frame (form, device ms of the frame = mcpt_stats.ms_total, ms of the trace launches, camera rays) and a summary
line: the median of each form and their ratio."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cornell-box")
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--aperture", type=float, default=0.0)
    ap.add_argument("--focus", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import montecarlopathtracing_amd as M
    sc = M.Scene(os.path.join(ROOT, "scenes") + os.sep, args.scene, width=args.width, height=args.height)
    dev = M.Device(sc, 0)
    forms = {"pinhole": {}, "lens": {"jitter": True, "aperture": args.aperture, "focus_distance": args.focus}}
    times = {k: [] for k in forms}
    for i in range(args.frames + 1):                       # frame 0 of each form: warm-up (buffers sized, code loaded)
        for name, lens in forms.items():
            dev.set_lens(**lens)
            st = M.Stats()
            dev.generateImg(args.spp, seed=args.seed, stats=st)
            if i == 0:
                continue
            times[name].append(st.ms_total)
            print(json.dumps({"form": name, "frame": i, "ms_total": round(st.ms_total, 3), "ms_trace": round(st.ms_trace, 3),
                              "rays_primary": st.rays_primary, "launches": st.launches}), flush=True)
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({"scene": args.scene, "width": args.width, "height": args.height, "spp": args.spp, "aperture": args.aperture,
                      "build_id": M.build_id(), "median_ms": {k: round(v, 3) for k, v in med.items()},
                      "lens_over_pinhole": round(med["lens"] / med["pinhole"], 4)}), flush=True)
    dev.close()
    sc.close()


if __name__ == "__main__":
    main()
