#!/usr/bin/env python3
"""Diagnostic: what an any-hit answer costs beside the closest-hit call a caller makes without it.

    python tools/any_hit_bench.py any     [--scene cornell-box --rays 4194304 --points 2048 --calls 5 --save PREFIX]
    python tools/any_hit_bench.py closest --load PREFIX [--root OTHER_TREE --scene cornell-box --calls 5]

any: the scene under grid_atlas; the hemisphere rays of its texel list (mcpt_query_rays), --rays of them, uploaded beforehand; one warm-up
call and --calls timed calls, each between two HIP events on one stream, of mcpt_trace_any_device with tmax = a quarter of the scene's
diagonal (set a), with tmax = +inf (set b) and of this build's mcpt_trace_closest_device on the same rays; then a --points x --points matrix
of the list's surface points through mcpt_trace_any_pairs_device (t0 = 1e-4, t1 = 1 - 1e-4) and the same pairs as a ray list through
closest hit (set d).  The counters of both walks come from one host-form call each, outside the timing.  With --save the ray lists are
written to PREFIX.rays.npy and PREFIX.pairs.npy.  closest: only mcpt_trace_closest_device on the lists read from --load, with the package of
--root -- another build of the library, the parent commit's for instance, which need not know any-hit rays.  One process; --time-limit
seconds after its start the process ends itself.  Medians; one JSON line per result.  What a caller of closest hit moves besides -- 36 bytes
per ray read back (face, t, p) against 1 byte or 1 bit here, and 48 bytes per ray uploaded against none for a pair -- is reported as bytes,
not timed."""
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
    ap.add_argument("mode", choices=["any", "closest"])
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--scene", default="cornell-box", help="cornell-box, veach-mis or interior (generated, about 204 k triangles)")
    ap.add_argument("--rays", type=int, default=1 << 22)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--save", default=None)
    ap.add_argument("--load", default=None)
    ap.add_argument("--time-limit", type=int, default=300)
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

    if a.scene == "interior":
        import tempfile
        from montecarlopathtracing_amd import synthetic
        base = tempfile.mkdtemp(prefix="mcpt_interior_") + os.sep
        synthetic.write_interior(base, "interior", width=64, height=36)
        sc = M.Scene(base, "interior")
    else:
        sc = M.Scene(os.path.join(a.root, "scenes") + os.sep, a.scene, width=64, height=36)
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

    def timed(call):
        ms = []
        for i in range(a.calls + 1):                             # the first call warms up
            hip_rt.check(hip.hipEventRecord(e0, st.h))
            rc = call()
            assert rc == 0, L.mcpt_last_error()
            hip_rt.check(hip.hipEventRecord(e1, st.h))
            hip_rt.check(hip.hipEventSynchronize(e1))
            t = C.c_float()
            hip_rt.check(hip.hipEventElapsedTime(C.byref(t), e0, e1))
            ms.append(t.value)
        return float(np.median(ms[1:])), [round(v, 3) for v in ms[1:]]

    base = {"build": M.build_id(), "scene": a.scene, "faces": int(sc.info.num_faces)}

    def closest(rays, what):
        """mcpt_trace_closest_device on an uploaded list, and the walk's counters from one host-form call"""
        n = rays.shape[0]
        d_rays = upload(rays)
        out = [hip_rt.DeviceBuffer(n * 4), hip_rt.DeviceBuffer(n * 8), hip_rt.DeviceBuffer(n * 24)]
        med, all_ms = timed(lambda: L.mcpt_trace_closest_device(dev._h, d_rays.ptr, n, out[0].ptr, out[1].ptr, out[2].ptr, None, st.h))
        s = M.Stats()
        face = dev.ray_intersect(rays, stats=s)[0]
        print(json.dumps(dict(base, what="mcpt_trace_closest_device", set=what, rays=n, ms=round(med, 3), calls_ms=all_ms, hit_share=round(float((face >= 0).mean()), 4),
                              nodes_per_ray=round(s.node_visits / n, 2), tris_per_ray=round(s.tri_tests / n, 2), bytes_up=n * 48, bytes_back=n * 36)), flush=True)
        for b in [d_rays] + out:
            b.free()

    if a.mode == "closest":
        closest(np.load(a.load + ".rays.npy"), "a, b: the list's hemisphere rays")
        closest(np.load(a.load + ".pairs.npy"), "d: the pair matrix as a ray list")
        return

    # the hemisphere rays of the scene's texel list under grid_atlas, the smallest map that gives every face a cell of 8 texels
    nf = int(sc.info.num_faces)
    cells = int(np.ceil(np.sqrt(nf)))
    size = 1024
    while size // cells < 8:
        size *= 2
    uv = M.grid_atlas(nf, size, size)
    _, texels, q6 = dev.lightmap_texels(size, size, uv=uv)
    c = int(texels.size)
    spp = -(-a.rays // c)
    idx = np.repeat(np.arange(c), spp)[:a.rays]
    k = np.tile(np.arange(spp, dtype=np.int32), c)[:a.rays]
    rays = dev.query_rays(q6[idx], a.seed, k, kind="hemisphere", ids=texels[idx])
    n = rays.shape[0]
    box = sc.bvh_nodes()[0][0]
    diag = float(np.linalg.norm(box[:3] - box[3:]))
    d_rays = upload(rays)
    d_occ = hip_rt.DeviceBuffer(n)
    for what, lim in (("a: tmax = diagonal / 4", diag / 4), ("b: tmax = +inf", None)):
        tmax = np.full(n, lim) if lim is not None else None
        d_tmax = upload(tmax) if tmax is not None else None
        med, all_ms = timed(lambda: L.mcpt_trace_any_device(dev._h, d_rays.ptr, d_tmax.ptr if d_tmax else None, n, d_occ.ptr, st.h))
        s = M.Stats()
        occ = dev.any_hit(rays, tmax, stats=s)
        print(json.dumps(dict(base, what="mcpt_trace_any_device", set=what, map=size, covered=c, rays=n, ms=round(med, 3), calls_ms=all_ms,
                              occluded_share=round(float(occ.mean()), 4), nodes_per_ray=round(s.node_visits / n, 2), tris_per_ray=round(s.tri_tests / n, 2),
                              bytes_up=n * (48 + (8 if lim is not None else 0)), bytes_back=n)), flush=True)
        if d_tmax:
            d_tmax.free()
    d_rays.free()
    d_occ.free()
    closest(rays, "a, b: the list's hemisphere rays")
    if a.save:
        np.save(a.save + ".rays.npy", rays)
    del rays

    # set d: a matrix of the list's surface points
    m = min(a.points, c // 2)
    pick = np.random.default_rng(a.seed).permutation(c)[:2 * m]
    pa, pb = np.ascontiguousarray(q6[pick[:m], :3]), np.ascontiguousarray(q6[pick[m:], :3])
    W = (m + 63) // 64
    d_a, d_b, d_bits = upload(pa), upload(pb), hip_rt.DeviceBuffer(m * W * 8)
    pp = M.PairParams(1e-4, 1.0 - 1e-4, 0, 0)
    med, all_ms = timed(lambda: L.mcpt_trace_any_pairs_device(dev._h, d_a.ptr, m, d_b.ptr, m, C.byref(pp), d_bits.ptr, st.h))
    s = M.Stats()
    occ = dev.any_hit_pairs(pa, pb, 1e-4, 1.0 - 1e-4, stats=s)
    print(json.dumps(dict(base, what="mcpt_trace_any_pairs_device", set="d: %d x %d surface points" % (m, m), rays=m * m, ms=round(med, 3), calls_ms=all_ms,
                          occluded_share=round(float(occ.mean()), 4), nodes_per_ray=round(s.node_visits / (m * m), 2), tris_per_ray=round(s.tri_tests / (m * m), 2),
                          bytes_up=2 * m * 24, bytes_back=m * W * 8)), flush=True)
    pairs = M.pair_rays(pa, pb, 1e-4, 1.0 - 1e-4)[0]
    closest(pairs, "d: the pair matrix as a ray list")
    if a.save:
        np.save(a.save + ".pairs.npy", pairs)


if __name__ == "__main__":
    main()
