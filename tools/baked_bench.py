#!/usr/bin/env python3
"""Diagnostic: what a baked frame costs and how it compares with the path-traced one.  tools/volume_bench.py's method.

    python tools/baked_bench.py frame  [--width 1280 --height 720 --samples 1 --grid 64 --size 2048 --calls 5]
    python tools/baked_bench.py approx [--width 320 --height 180 --samples 16 --ref-spp 4096 --size 1024 --spp 256]
    python tools/baked_bench.py specular [--scene glassroom --width 1280 --height 720 --samples 1 --probe-grid 8 --probe-res 64 --calls 5]

frame : cornell-box at --width x --height.  The sources are synthetic (what a kernel costs does not depend on what the numbers mean): a
        --grid^3 volume over the scene's bounds, plain and with moments, and a --size^2 lightmap under grid_atlas, all in device buffers.
        One warm-up call and --calls timed calls of mcpt_render_baked_device per source, each between two HIP events on one stream,
        taken in turn; then mcpt_progressive_sample_aovs at the same sample count (the same rays and the same trace; a host call, timed
        by the clock around it, arrays not fetched, and it allocates its chunk buffers on every call) and mcpt_render_device at 256
        samples.  Medians.
        The shading kernel's traffic floor: 84 bytes read and 32 written per ray, at 8 TB/s.  Under rocprofv3 --kernel-trace --stats (a
        run of its own) the kernels' names give the split: k_baked_camera_rays, the trace engine's kernels, k_baked_shade, k_baked_fold.
        MCPT_LIB selects another build of the library.
approx: cornell-box and glassroom at --width x --height: frames lit by a lightmap of --size^2 baked at --spp and denoised (cornell-box under
        grid_atlas, glassroom under its own chart), and by volumes of 16^3 and 32^3 probes baked at --spp with their visibility, against
        the path-traced frame at --ref-spp: relative RMS difference and the ratio of the means over the pixels whose samples are all
        surface hits.  The two are not expected to agree (DESIGN 6s says why).
specular: --scene (glassroom under its sky, or veach-mis) at --width x --height.  The diffuse source is a synthetic 8^3 volume, the
        specular source a synthetic --probe-grid^3 reflection volume of --probe-res^2 probes in five levels (each half the size of the one
        before), plain and with moments, all in device buffers.  One warm-up call and --calls timed calls of mcpt_render_baked_device and
        of mcpt_render_baked_specular_device per source, between two HIP events on one stream, taken in turn.  Medians.  The specular
        kernel's traffic floor: 84 bytes read and 24 read and written again per ray (the direction's ray record, the hit and the
        radiance), at 8 TB/s; under rocprofv3 --kernel-trace --stats (a run of its own) k_baked_specular is the kernel's own time.
One process; --time-limit seconds after its start the process ends itself.  One JSON line per result."""
import argparse
import ctypes as C
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BYTES_PER_S = 8e12


def grid_over(M, dev, n, inset=0.02):
    box, _ = dev.bvh_nodes()
    lo, hi = np.minimum(box[0, :3], box[0, 3:]), np.maximum(box[0, :3], box[0, 3:])
    return M.volume_grid(lo + inset * (hi - lo), (1.0 - 2.0 * inset) * (hi - lo) / (n - 1), (n, n, n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["frame", "approx", "specular"])
    ap.add_argument("--scene", choices=["glassroom", "veach-mis"], default="glassroom")
    ap.add_argument("--probe-grid", type=int, default=8)
    ap.add_argument("--probe-res", type=int, default=64)
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--samples", type=int, default=None)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--res", type=int, default=8)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--time-limit", type=int, default=420)
    a = ap.parse_args()
    signal.alarm(a.time_limit)                                   # SIGALRM's default action ends the process
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import montecarlopathtracing_amd as M
    from montecarlopathtracing_amd import _lib
    base = {"build": M.build_id()}
    scenes = os.path.join(ROOT, "scenes") + os.sep
    R = a.res

    if a.mode == "approx":
        from conftest import extra_scene_dir
        Wd, Ht, G, size = a.width or 320, a.height or 180, a.samples or 16, a.size or 1024
        for name, path in (("cornell-box", scenes), ("glassroom", extra_scene_dir())):
            sc = M.Scene(path, name, width=Wd, height=Ht)
            dev = M.Device(sc, 0)
            dev.set_lens(jitter=True)
            ref = dev.generateImg(a.ref_spp, seed=a.seed + 1000)
            uv = M.grid_atlas(sc.info.num_faces, size, size) if name == "cornell-box" else None
            E, err, _, _ = dev.bake_lightmap(size, size, a.spp, uv=uv, seed=a.seed)
            Ed, owner = dev.denoise_lightmap(E, err, uv=uv, dilate=2)
            rows = [("lightmap %d^2 denoised" % size, M.baked_lightmap(Ed, uv=uv, owner=owner), {})]
            for n in (16, 32):
                g = grid_over(M, dev, n)
                sh, _, _ = dev.bake_volume(g, a.spp, seed=a.seed)
                m, hits, back, valid = dev.bake_volume_visibility(g, a.spp, res=R, seed=a.seed)
                if back.sum() * 2 > hits.sum():                  # a scene wound the other way: the mask from the other count
                    valid = ((hits - back) <= 0.25 * a.spp).astype(np.uint8)
                maxd = 1.5 * float(np.sqrt(sum(float(s) ** 2 for s in g.spacing)))
                vis = M.volume_visibility(R, maxd, 0.25 * min(g.spacing), 0.0)
                rows.append(("volume %d^3" % n, M.baked_volume(g, sh), dict(face_viewer=True)))
                rows.append(("volume %d^3 mask+visibility" % n, M.baked_volume(g, sh, valid=valid, moments=m, vis=vis), dict(face_viewer=True)))
            for what, source, flags in rows:
                got = dev.render_baked(source, samples=G, seed=a.seed + 1000, **flags)
                sel = got["counts"][..., 0] == G
                d, r = got["image"][sel], ref[sel]
                rel = np.sqrt(((d - r) ** 2).sum(axis=1)) / np.maximum(np.sqrt((r ** 2).sum(axis=1)), 1e-12)
                print(json.dumps(dict(base, what="approx", scene=name, source=what, width=Wd, height=Ht, samples=G, bake_spp=a.spp, ref_spp=a.ref_spp,
                                      pixels=int(sel.sum()), unlit=int((got["lit"][sel] == 0).sum()), rel_rms=round(float(np.sqrt((rel ** 2).mean())), 4),
                                      rel_median=round(float(np.median(rel)), 4), mean_ratio=round(float(d.mean() / r.mean()), 4))), flush=True)
            dev.close()
            sc.close()
        return

    import hip_rt
    L, hip = M.lib(), hip_rt.hip()
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    Wd, Ht, G, size = a.width or 1280, a.height or 720, a.samples or 1, a.size or 2048
    if a.mode == "specular":
        from conftest import extra_scene_dir
        import env_scenes
        sc = M.Scene(extra_scene_dir() if a.scene == "glassroom" else scenes, a.scene, width=Wd, height=Ht)
        dev = M.Device(sc, 0)
        if a.scene == "glassroom":
            dev.set_environment(*env_scenes.SKIES["map"])
    else:
        sc = M.Scene(scenes, "cornell-box", width=Wd, height=Ht)
        dev = M.Device(sc, 0)
    hip_rt.set_device(0)
    st = hip_rt.Stream()
    e0, e1 = C.c_void_p(), C.c_void_p()
    hip_rt.check(hip.hipEventCreate(C.byref(e0)))
    hip_rt.check(hip.hipEventCreate(C.byref(e1)))

    def once(call):
        hip_rt.check(hip.hipEventRecord(e0, st.h))
        rc = call()
        assert rc == 0, L.mcpt_last_error()
        hip_rt.check(hip.hipEventRecord(e1, st.h))
        hip_rt.check(hip.hipEventSynchronize(e1))
        t = C.c_float()
        hip_rt.check(hip.hipEventElapsedTime(C.byref(t), e0, e1))
        return t.value

    def upload(arr):
        arr = np.ascontiguousarray(arr)
        buf = hip_rt.DeviceBuffer(arr.nbytes)
        hip_rt.check(hip.hipMemcpy(buf.ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes, 1))
        return buf

    rng = np.random.default_rng(a.seed)
    if a.mode == "specular":
        px = Wd * Ht
        gd, gs = grid_over(M, dev, 8), grid_over(M, dev, a.probe_grid)
        probes = a.probe_grid ** 3
        levels = [(max(a.probe_res >> l, 1), ns) for l, ns in enumerate((4096, 512, 64, 8, 0))]
        desc = M.reflection_chain(a.probe_res, levels)
        maxd = 1.5 * float(np.sqrt(sum(float(v) ** 2 for v in gs.spacing)))
        vis = M.volume_visibility(R, maxd, 0.0, 0.0)
        d_sh = upload(rng.normal(size=(512, 9, 3)))
        d_chain = upload(rng.uniform(0.5, 1.5, size=(probes, desc.num_texels, 3)))
        mu = rng.uniform(0.0, maxd, size=(probes, R * R))
        d_m = upload(np.stack([mu, mu * mu + rng.uniform(0.0, 0.1 * maxd * maxd, size=mu.shape)], axis=2))
        d_img, d_slit = hip_rt.DeviceBuffer(px * 24), hip_rt.DeviceBuffer(px * 4)
        src = _lib.BakedSource()
        src.kind, src.grid, src.sh27 = M.BAKED_VOLUME, C.pointer(gd), d_sh.ptr
        fp = _lib.BakedFrameParams(G, M.BAKED_FACE_VIEWER, a.seed, 0, (C.c_int32 * 2)(0, 0))
        calls = {"plain": lambda: L.mcpt_render_baked_device(dev._h, C.byref(src), C.byref(fp), d_img.ptr, None, None, None, st.h)}
        keep = []
        for kind in ("specular", "specular visible"):
            sp = _lib.BakedSpecular()
            sp.grid, sp.chain, sp.chain_data = C.pointer(gs), C.pointer(desc), d_chain.ptr
            if kind == "specular visible":
                sp.moments, sp.visibility = d_m.ptr, C.pointer(vis)
            keep.append(sp)
            calls[kind] = lambda sp=sp: L.mcpt_render_baked_specular_device(dev._h, C.byref(src), C.byref(sp), C.byref(fp), d_img.ptr, None, None, d_slit.ptr, None, st.h)
        ms = {k: [] for k in calls}
        for i in range(a.calls + 1):
            for k, call in calls.items():
                ms[k].append(once(call))
        slit = np.zeros(px, dtype=np.int32)
        d_slit.to_host_async(slit, st.h)
        st.synchronize()
        floor_ms = px * G * (84 + 2 * 24) / HBM_BYTES_PER_S * 1e3
        for k, v in ms.items():
            print(json.dumps(dict(base, what="mcpt_render_baked_specular_device" if k != "plain" else "mcpt_render_baked_device", source=k, scene=a.scene,
                                  width=Wd, height=Ht, samples=G, probes=probes, probe_res=a.probe_res, chain_mb=round(probes * desc.num_texels * 24 / 1e6, 1),
                                  ms=round(float(np.median(v[1:])), 4), calls_ms=[round(t, 4) for t in v[1:]], specular_floor_ms=round(floor_ms, 4),
                                  specular_pixels=int((slit > 0).sum()))), flush=True)
        return
    n = a.grid
    probes = n ** 3
    g = grid_over(M, dev, n)
    maxd = 1.5 * float(np.sqrt(sum(float(s) ** 2 for s in g.spacing)))
    vis = M.volume_visibility(R, maxd, 0.0, 0.0)
    d_sh = upload(rng.normal(size=(probes, 9, 3)))
    mu = rng.uniform(0.0, maxd, size=(probes, R * R))
    d_m = upload(np.stack([mu, mu * mu + rng.uniform(0.0, 0.1 * maxd * maxd, size=mu.shape)], axis=2))
    d_irr = upload(rng.uniform(0.5, 1.5, size=(size, size, 3)))
    d_uv = upload(M.grid_atlas(sc.info.num_faces, size, size))
    px = Wd * Ht
    d_img, d_counts, d_lit = hip_rt.DeviceBuffer(px * 24), hip_rt.DeviceBuffer(px * 12), hip_rt.DeviceBuffer(px * 4)

    def source(kind):
        s = _lib.BakedSource()
        if kind == "lightmap":
            s.kind, s.width, s.height, s.irradiance3, s.uv6 = M.BAKED_LIGHTMAP, size, size, d_irr.ptr, d_uv.ptr
        else:
            s.kind, s.grid, s.sh27 = M.BAKED_VOLUME, C.pointer(g), d_sh.ptr
            if kind == "volume visible":
                s.moments, s.visibility = d_m.ptr, C.pointer(vis)
        return s

    calls = {}
    keep = []
    for kind in ("volume", "volume visible", "lightmap"):
        s = source(kind)
        fp = _lib.BakedFrameParams(G, 0, a.seed, 0, (C.c_int32 * 2)(0, 0))
        keep += [s, fp]
        calls[kind] = lambda s=s, fp=fp: L.mcpt_render_baked_device(dev._h, C.byref(s), C.byref(fp), d_img.ptr, d_counts.ptr, d_lit.ptr, None, st.h)
    ms = {k: [] for k in calls}
    for i in range(a.calls + 1):
        for k, call in calls.items():
            ms[k].append(once(call))
    rays = px * G
    floor_ms = rays * 116 / HBM_BYTES_PER_S * 1e3
    for k, v in ms.items():
        print(json.dumps(dict(base, what="mcpt_render_baked_device", source=k, scene="cornell-box", width=Wd, height=Ht, samples=G, probes=probes, size=size,
                              ms=round(float(np.median(v[1:])), 4), calls_ms=[round(t, 4) for t in v[1:]], shade_floor_ms=round(floor_ms, 4))), flush=True)
    # the same rays and the same trace without the shading: the sample AOVs of a progressive handle, recomputed on every call
    pr = dev.progressive(max(G, 2), seed=a.seed)
    other = 2 if G == 1 else 1
    wall = []
    for i in range(a.calls + 1):
        assert L.mcpt_progressive_sample_aovs(pr._h, other, None, None, None, None) == 0
        t0 = time.perf_counter()
        assert L.mcpt_progressive_sample_aovs(pr._h, G, None, None, None, None) == 0
        wall.append((time.perf_counter() - t0) * 1e3)
    pr.close()
    print(json.dumps(dict(base, what="mcpt_progressive_sample_aovs", samples=G, ms=round(float(np.median(wall[1:])), 4), calls_ms=[round(t, 4) for t in wall[1:]])), flush=True)
    rp = M.RenderParams(256, a.seed, 0, 1, 0, 0, 0)
    traced = [once(lambda: L.mcpt_render_device(dev._h, C.byref(rp), d_img.ptr, None, st.h)) for i in range(3)]
    print(json.dumps(dict(base, what="mcpt_render_device", spp=256, ms=round(float(np.median(traced[1:])), 3), calls_ms=[round(t, 3) for t in traced[1:]])), flush=True)


if __name__ == "__main__":
    main()
