#!/usr/bin/env python3
"""Diagnostic: what adaptive queries and lightmaps cost and buy.

    python tools/adaptive_query_bench.py list     --list grid|lightmap --list-file F [--scene cornell-box --size 2048]
    python tools/adaptive_query_bench.py overhead --list-file F [--spp 64 --min-spps 64,16,4 --calls 5]
    python tools/adaptive_query_bench.py parent   --list-file F --root OTHER_TREE [--spp 64 --calls 5]
    python tools/adaptive_query_bench.py gain     [--scene cornell-box --size 512 --spp 1024 --min-spp 16 --targets 0.05,0.02 --ref-spp 4096]
    python tools/adaptive_query_bench.py one      --list-file F [--spp 64 --min-spp 4 --target 0.2]

list: writes a hemisphere list (texels / ids, q6) to F -- `grid`, the 64^3 points of the scene's bounding box with the normal +y, or
`lightmap`, the texel list of the scene under grid_atlas at --size.  overhead: one warm-up call and --calls timed calls, each between
two HIP events on one stream, of mcpt_query_radiance_device and of mcpt_query_radiance_adaptive_device with both targets 0 for every
min_spp of --min-spps (64: one pass, 16: three, 4: five).  parent: only mcpt_query_radiance_device with the package of --root, another
build of the library -- the parent commit's, which need not know adaptive queries.  gain: the adaptive bake at every target against
uniform bakes of the same mean sample count and of --spp, each held to a --ref-spp bake of another seed: mean samples per texel, passes,
time between HIP events around mcpt_bake_lightmap*_device, and the RMS and 90th percentile of |E - E_ref| / |E_ref| over the covered
texels.  one: a single adaptive call after a warm-up, for a kernel trace.  One process; --time-limit seconds after its start the process
ends itself.  Medians; one JSON line per result."""
import argparse
import ctypes as C
import json
import os
import signal
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["list", "overhead", "parent", "gain", "one"])
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--scene", default="cornell-box")
    ap.add_argument("--list", default="grid", choices=["grid", "lightmap"])
    ap.add_argument("--list-file", default=None)
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--spp", type=int, default=None)
    ap.add_argument("--min-spps", default="64,16,4")
    ap.add_argument("--min-spp", type=int, default=None)
    ap.add_argument("--targets", default="0.05,0.02")
    ap.add_argument("--target", type=float, default=0.2)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--time-limit", type=int, default=240)
    a = ap.parse_args()
    signal.alarm(a.time_limit)                                   # SIGALRM's default action ends the process
    sys.path.insert(0, a.root)
    sys.path.insert(0, os.path.join(a.root, "tests"))

    import hip_rt
    import montecarlopathtracing_amd as M
    L, hip = M.lib(), hip_rt.hip()
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]

    sc = M.Scene(os.path.join(ROOT, "scenes") + os.sep, a.scene, width=64, height=36)
    dev = M.Device(sc, 0)
    hip_rt.set_device(0)
    st = hip_rt.Stream()
    e0, e1 = C.c_void_p(), C.c_void_p()
    hip_rt.check(hip.hipEventCreate(C.byref(e0)))
    hip_rt.check(hip.hipEventCreate(C.byref(e1)))

    def upload(arr):
        b = hip_rt.DeviceBuffer(max(arr.nbytes, 8))
        hip_rt.check(hip.hipMemcpy(b.ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes, 1))
        return b

    def download(buf, out):
        hip_rt.check(hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), buf.ptr, out.nbytes, 2))
        return out

    def timed(call, calls=a.calls):
        ms = []
        for i in range(calls + 1):                               # the first call warms up
            hip_rt.check(hip.hipEventRecord(e0, st.h))
            rc = call()
            assert rc == 0, L.mcpt_last_error()
            hip_rt.check(hip.hipEventRecord(e1, st.h))
            hip_rt.check(hip.hipEventSynchronize(e1))
            t = C.c_float()
            hip_rt.check(hip.hipEventElapsedTime(C.byref(t), e0, e1))
            ms.append(t.value)
        return float(np.median(ms[1:] or ms)), [round(v, 3) for v in ms[1:]]

    base = {"build": M.build_id(), "scene": a.scene}

    if a.mode == "list":
        if a.list == "grid":
            box, _ = dev.bvh_nodes()
            lo, hi = np.minimum(box[0, :3], box[0, 3:]), np.maximum(box[0, :3], box[0, 3:])
            c = (np.arange(64) + 0.5) / 64.0
            p = np.stack(np.meshgrid(c, c, c, indexing="ij"), axis=-1).reshape(-1, 3) * (hi - lo) + lo
            q6 = np.ascontiguousarray(np.concatenate([p, np.tile([0.0, 1.0, 0.0], (p.shape[0], 1))], axis=1))
            texels = np.arange(p.shape[0], dtype=np.int32)
        else:
            size = a.size or 2048
            _, texels, q6 = dev.lightmap_texels(size, size, uv=M.grid_atlas(sc.info.num_faces, size, size))
        np.savez(a.list_file, texels=texels, q6=q6)
        print(json.dumps(dict(base, what="list", list=a.list, queries=int(texels.size))))
        return

    if a.mode in ("overhead", "parent", "one"):
        spp = a.spp or 64
        z = np.load(a.list_file)
        texels, q6 = np.ascontiguousarray(z["texels"]), np.ascontiguousarray(z["q6"])
        m = texels.size
        d_q, d_ids = upload(q6), upload(texels)
        out = [hip_rt.DeviceBuffer(m * 24), hip_rt.DeviceBuffer(m * 24), hip_rt.DeviceBuffer(m * 4), hip_rt.DeviceBuffer(m * 4)]
        qp = M.QueryParams(spp, 0, a.seed, M.QUERY_HEMISPHERE, 0, (C.c_int32 * 2)(0, 0))
        base.update(queries=int(m), spp=spp)
        if a.mode == "one":
            apar = M.AdaptiveParams(a.target, 0.0, a.min_spp or 4, 0)
            med, all_ms = timed(lambda: L.mcpt_query_radiance_adaptive_device(dev._h, d_q.ptr, d_ids.ptr, m, C.byref(qp), C.byref(apar), out[0].ptr, out[1].ptr,
                                                                              out[2].ptr, out[3].ptr, None, st.h), calls=1)
            counts = download(out[3], np.zeros(m, dtype=np.int32))
            print(json.dumps(dict(base, what="one adaptive call", target=a.target, min_spp=a.min_spp or 4, samples=int(counts.sum()), ms=round(med, 3),
                                  counts={int(k): int(v) for k, v in zip(*np.unique(counts, return_counts=True))})))
            return
        med, all_ms = timed(lambda: L.mcpt_query_radiance_device(dev._h, d_q.ptr, d_ids.ptr, m, C.byref(qp), out[0].ptr, out[1].ptr, out[2].ptr, None, st.h))
        print(json.dumps(dict(base, what="mcpt_query_radiance_device", samples=int(m) * spp, ms=round(med, 3), calls_ms=all_ms)))
        if a.mode == "parent":
            return
        want = download(out[0], np.zeros((m, 3)))
        for min_spp in [int(v) for v in a.min_spps.split(",")]:
            apar = M.AdaptiveParams(0.0, 0.0, min_spp, 0)
            med, all_ms = timed(lambda: L.mcpt_query_radiance_adaptive_device(dev._h, d_q.ptr, d_ids.ptr, m, C.byref(qp), C.byref(apar), out[0].ptr, out[1].ptr,
                                                                              out[2].ptr, out[3].ptr, None, st.h))
            got = download(out[0], np.zeros((m, 3)))
            print(json.dumps(dict(base, what="mcpt_query_radiance_adaptive_device, targets 0", min_spp=min_spp,
                                  passes=len(M.query_pass_boundaries(spp, min_spp)), samples=int(m) * spp, ms=round(med, 3), calls_ms=all_ms,
                                  equals_one_shot=bool(np.array_equal(got.view(np.uint64), want.view(np.uint64))))))
        return

    # gain
    size, spp, min_spp = a.size or 512, a.spp or 1024, a.min_spp or 16
    uv = M.grid_atlas(sc.info.num_faces, size, size)
    n = size * size
    d_uv = upload(uv)
    maps = [hip_rt.DeviceBuffer(n * 24), hip_rt.DeviceBuffer(n * 24), hip_rt.DeviceBuffer(n * 4), hip_rt.DeviceBuffer(n * 4), hip_rt.DeviceBuffer(n * 4)]

    def uniform(k, seed, calls):
        lp = M.LightmapParams(size, size, k, 0, seed, 0, 0, (C.c_int32 * 2)(0, 0))
        med, all_ms = timed(lambda: L.mcpt_bake_lightmap_device(dev._h, d_uv.ptr, C.byref(lp), maps[0].ptr, maps[1].ptr, maps[2].ptr, maps[3].ptr, None, st.h),
                            calls=calls)
        return download(maps[0], np.zeros((n, 3))), download(maps[3], np.zeros(n, dtype=np.int32)), med, all_ms

    ref, owner, _, _ = uniform(a.ref_spp, a.seed + 1, 0)
    covered = owner >= 0
    rn = np.sqrt((ref ** 2).sum(axis=1))
    ok = covered & (rn > 0)
    base.update(size=size, spp=spp, min_spp=min_spp, covered=int(covered.sum()), ref_spp=a.ref_spp)

    def errors(E):
        e = np.sqrt(((E - ref) ** 2).sum(axis=1))[ok] / rn[ok]
        return float(np.sqrt((e ** 2).mean())), float(np.percentile(e, 90))

    bounds = M.query_pass_boundaries(spp, min_spp).tolist()
    for target in [float(v) for v in a.targets.split(",")]:
        lp = M.LightmapParams(size, size, spp, 0, a.seed, 0, 0, (C.c_int32 * 2)(0, 0))
        apar = M.AdaptiveParams(target, 0.0, min_spp, 0)
        med, all_ms = timed(lambda: L.mcpt_bake_lightmap_adaptive_device(dev._h, d_uv.ptr, C.byref(lp), C.byref(apar), maps[0].ptr, maps[1].ptr, maps[2].ptr,
                                                                         maps[3].ptr, maps[4].ptr, None, st.h))
        E, counts = download(maps[0], np.zeros((n, 3))), download(maps[4], np.zeros(n, dtype=np.int32))
        mean_count = float(counts[covered].mean())
        rms, p90 = errors(E)
        print(json.dumps(dict(base, form="adaptive", target=target, samples_per_texel=round(mean_count, 2), passes=bounds.index(int(counts.max())) + 1,
                              ms=round(med, 3), calls_ms=all_ms, rel_err_rms=rms, rel_err_p90=p90,
                              counts={int(k): int(v) for k, v in zip(*np.unique(counts[covered], return_counts=True))})), flush=True)
        k = max(int(round(mean_count)), 1)
        E, _, med, all_ms = uniform(k, a.seed, a.calls)
        rms, p90 = errors(E)
        print(json.dumps(dict(base, form="uniform, the adaptive bake's mean count", target=target, samples_per_texel=k, ms=round(med, 3), calls_ms=all_ms,
                              rel_err_rms=rms, rel_err_p90=p90)), flush=True)
    E, _, med, all_ms = uniform(spp, a.seed, a.calls)
    rms, p90 = errors(E)
    print(json.dumps(dict(base, form="uniform, spp", samples_per_texel=spp, ms=round(med, 3), calls_ms=all_ms, rel_err_rms=rms, rel_err_p90=p90)), flush=True)


if __name__ == "__main__":
    main()
