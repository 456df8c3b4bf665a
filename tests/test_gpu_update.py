"""-m gpu: mcpt_device_update_vertices and mcpt_device_set_camera.  The culling hierarchy only culls, so a device whose
vertices were updated -- by a refit or by a rebuild -- must answer exactly as a device created from a fresh scene with the moved vertices:
every comparison below is bit for bit.  The fresh scene is the original .obj with its positions replaced (tests/anim_scenes.py), which
the CPU oracle loads as well."""
import os

import numpy as np
import pytest

import anim_scenes as A
import fast_bvh_ref as F
import refit_ref as R
from conftest import SCENES, extra_scene_dir, make_rays

pytestmark = pytest.mark.gpu

W, H, SPP = 96, 54, 2
KNOBS = ("MCPT_TRACE_ENGINE", "MCPT_FINISH_ENGINE", "MCPT_FINISH_PATHS", "MCPT_WORKSPACE_GB")
NAMES = ["cornell-box", "veach-mis", "glassroom", "synthetic"]
_cache = {}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def source(name, tmp_factory):
    """(directory, file name) of a test scene; the synthetic 20 k-triangle scene is written once"""
    if name == "synthetic":
        if "syn" not in _cache:
            from montecarlopathtracing_amd import synthetic
            d = str(tmp_factory.mktemp("syn")) + os.sep
            synthetic.write_obj(synthetic.generate(20000, width=W, height=H), d, "synthetic")
            _cache["syn"] = d
        return _cache["syn"], "synthetic"
    return (extra_scene_dir() if name == "glassroom" else SCENES), name


def base(mcpt, name, tmp_factory, size=(W, H)):
    """the scene (at this file's frame size unless another is asked for), its vertices [n, 9], the faces' materials and the light materials"""
    key = ("base", name) if size == (W, H) else ("base", name, size)
    if key not in _cache:
        d, f = source(name, tmp_factory)
        sc = mcpt.Scene(d, f, width=size[0], height=size[1])
        g, m, _ = sc.faces()
        lights = [sc.light(i)[2] for i in range(sc.info.num_lights)]
        _cache[key] = (sc, np.ascontiguousarray(g[:, :9]), m, lights)
    return _cache[key]


def deform(mcpt, name, what, tmp_factory):
    sc, v, m, lights = base(mcpt, name, tmp_factory)
    if what == "identity":
        return A.identity(v)
    if what == "rigid":
        # the object standing inside the room: cornell-box's is the material "Table" (this cornell-box has walls, a light and that one
        # object); elsewhere the largest non-emitter group
        names = [sc.material(i)[0] for i in range(sc.info.num_materials)]
        if "Table" in names:
            return A.rigid(v, np.nonzero(m == names.index("Table"))[0])
        counts = np.bincount(m)
        for l in lights:
            counts[l] = 0
        return A.rigid(v, np.nonzero(m == int(np.argmax(counts)))[0])
    if what == "mirror":
        # the same object turned inside out where it stands
        names = [sc.material(i)[0] for i in range(sc.info.num_materials)]
        return A.mirror(v, np.nonzero(m == names.index("Table"))[0])
    if what == "sine":
        return A.sine_field(v, 0.05)
    if what == "lights":
        return A.move_lights(v, m, lights)
    if what == "degenerate":
        return A.degenerate(A.sine_field(v, 0.01))
    if what.startswith("path"):
        return A.sine_field(v, 0.004 * int(what[4:]), phase=0.2 * int(what[4:]))
    raise KeyError(what)


def moved_files(mcpt, name, what, tmp_factory):
    """the directory of the scene's files with the deformation's positions"""
    key = ("files", name, what)
    if key not in _cache:
        d, f = source(name, tmp_factory)
        _cache[key] = A.write_moved(d, f, deform(mcpt, name, what, tmp_factory), str(tmp_factory.mktemp("moved")))
    return _cache[key], source(name, tmp_factory)[1]


def fresh(mcpt, name, what, build, tmp_factory, size=(W, H)):
    d, f = moved_files(mcpt, name, what, tmp_factory)
    sc = mcpt.Scene(d, f, width=size[0], height=size[1])
    return sc, mcpt.Device(sc, 0, build=build)


def rays_for(mcpt, name, tmp_factory, n=80000):
    key = ("rays", name, n)
    if key not in _cache:
        sc, v, _, _ = base(mcpt, name, tmp_factory)
        rng = np.random.default_rng(11)
        p = v.reshape(-1, 3)
        lo, hi = p.min(axis=0) - 0.2, p.max(axis=0) + 0.2
        o = lo + (hi - lo) * rng.random((n, 3))
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        d[::97, 0] = 0.0                                   # axis-parallel components among them
        tgt = p[rng.integers(0, p.shape[0], size=n // 4)]  # a quarter aimed at vertices (edges, shared corners)
        d[:n // 4] = tgt - o[:n // 4]
        _cache[key] = np.ascontiguousarray(np.hstack([o, d]))
    return _cache[key]


def observe(mcpt, dev, rays, mega=False):
    out = {"img": dev.generateImg(SPP, seed=5)}
    if mega:
        out["mega"] = dev.generateImg(SPP, seed=5, flags=mcpt.RENDER_MEGAKERNEL)
    for mode in (mcpt.TRACE_FAST, mcpt.TRACE_REFERENCE):
        dev.set_trace_mode(mode)
        f, t, p, pn = dev.ray_intersect(rays)
        out["hit%d" % mode] = (f, t, p, pn)
    dev.set_trace_mode(mcpt.TRACE_FAST)
    pix = np.arange(0, W * H, 7, dtype=np.int32)
    out["rad"] = dev.sample_radiance(3, pix, (pix % 3).astype(np.int32))
    out["nodes"] = dev.bvh_nodes()
    out["order"] = dev.leaf_order()
    return out


def assert_same(a, b, what):
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, tuple):
            for i, (p, q) in enumerate(zip(x, y)):
                assert same(p, q), "%s: %s[%d] differs (%d of %d)" % (what, k, i, int((bits(p) != bits(q)).sum()), bits(p).size)
        else:
            assert same(x, y), "%s: %s differs (%d of %d)" % (what, k, int((bits(x) != bits(y)).sum()), bits(x).size)


BUILDS = {"host": 0, "device": 1, "device_fast": 2, "device_sah": 3}


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name", NAMES)
def test_updated_device_is_a_fresh_device(mcpt, name, build, mode, tmp_path_factory):
    """Frame identity after deformations (b) rigid motion of one object, (c) a sine field of 5 % of the diagonal on every vertex, (d) the
    lights moved and scaled, (e) a collapsed triangle, a vertex outside the Morton cube and two coincident faces, applied one after the
    other to ONE device: frames (wavefront; the megakernel on the host build), 80 k closest hits in both trace modes, sample_radiance,
    bvh_nodes() and leaf_order() equal a fresh device's on a fresh scene with the moved vertices."""
    sc, v, m, lights = base(mcpt, name, tmp_path_factory)
    rays = rays_for(mcpt, name, tmp_path_factory)
    dev = mcpt.Device(sc, 0, build=BUILDS[build])
    for what in ("rigid", "sine", "lights", "degenerate"):
        if what == "lights" and not lights:
            continue
        nv = deform(mcpt, name, what, tmp_path_factory)
        info = dev.update_vertices(nv, mode=mode)
        assert info["mode"] == (0 if mode == "refit" else 1) and info["fast_enabled"] == 1
        assert same(dev.vertices(), nv)
        fsc, fdev = fresh(mcpt, name, what, BUILDS[build], tmp_path_factory)
        assert same(fsc.faces()[0][:, :9], nv), "the moved files do not hold the moved vertices"
        mega = build == "host" and what == "sine"
        assert_same(observe(mcpt, dev, rays, mega), observe(mcpt, fdev, rays, mega), "%s %s %s %s" % (name, build, mode, what))
        fdev.close()
        fsc.close()
    dev.close()


@pytest.mark.parametrize("engine", ["pool", "vote"])
@pytest.mark.parametrize("build", ["host", "device_sah"])
@pytest.mark.parametrize("name", NAMES)
def test_both_engines_after_a_refit(mcpt, name, build, engine, monkeypatch, tmp_path_factory):
    monkeypatch.setenv("MCPT_TRACE_ENGINE", engine)
    sc, v, _, _ = base(mcpt, name, tmp_path_factory)
    rays = rays_for(mcpt, name, tmp_path_factory)
    dev = mcpt.Device(sc, 0, build=BUILDS[build])
    for what in ("sine", "degenerate"):
        dev.update_vertices(deform(mcpt, name, what, tmp_path_factory), mode="refit")
        fsc, fdev = fresh(mcpt, name, what, BUILDS[build], tmp_path_factory)
        assert_same(observe(mcpt, dev, rays), observe(mcpt, fdev, rays), "%s %s %s %s" % (name, build, engine, what))
        fdev.close()
        fsc.close()
    dev.close()


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
@pytest.mark.parametrize("build", ["host", "device", "device_sah"])
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_morton_bounds_scenes_follow_the_new_vertices(mcpt, name, build, mode, tmp_path_factory):
    """A scene loaded with LOAD_MORTON_BOUNDS keys its Morton order on its own bounds: after an update the domain is that of the NEW
    vertices, so leaf_order, bvh_nodes, hits and frames equal those of the moved files loaded with the same flag -- and the order differs
    from the fixed cube's, so the flag is really at work."""
    d, f = source(name, tmp_path_factory)
    sc = mcpt.Scene(d, f, width=W, height=H, load_flags=mcpt.LOAD_MORTON_BOUNDS)
    rays = rays_for(mcpt, name, tmp_path_factory, n=20000)
    dev = mcpt.Device(sc, 0, build=BUILDS[build])
    for what in ("sine", "rigid"):
        dev.update_vertices(deform(mcpt, name, what, tmp_path_factory), mode=mode)
        md, mf = moved_files(mcpt, name, what, tmp_path_factory)
        fsc = mcpt.Scene(md, mf, width=W, height=H, load_flags=mcpt.LOAD_MORTON_BOUNDS)
        fdev = mcpt.Device(fsc, 0, build=BUILDS[build])
        assert_same(observe(mcpt, dev, rays), observe(mcpt, fdev, rays), "%s %s %s %s" % (name, build, mode, what))
        csc, cdev = fresh(mcpt, name, what, BUILDS[build], tmp_path_factory)
        assert not np.array_equal(cdev.leaf_order(), dev.leaf_order())
        for h in (fdev, fsc, cdev, csc):
            h.close()
    dev.close()
    sc.close()


@pytest.mark.parametrize("name", NAMES)
def test_oracle_agrees_after_an_update(mcpt, oracle, name, tmp_path_factory):
    """closest hits of the refitted device against the CPU oracle on the moved scene's files: face, t, p, pn bit for bit"""
    sc, v, _, _ = base(mcpt, name, tmp_path_factory)
    d, f = moved_files(mcpt, name, "sine", tmp_path_factory)
    osc = oracle.OracleScene(d + f, texture_dir=d, width=W, height=H)
    rays = make_rays(osc, 4000, 17)
    of, ot, op, opn = osc.trace_closest(rays)
    for build in ("host", "device_fast"):
        dev = mcpt.Device(sc, 0, build=BUILDS[build])
        dev.update_vertices(deform(mcpt, name, "sine", tmp_path_factory), mode="refit")
        gf, gt, gp, gpn = dev.ray_intersect(rays)
        hit = of >= 0
        assert np.array_equal(gf, of)
        assert same(gt[hit], ot[hit]) and same(gp[hit], op[hit]) and same(gpn[hit], opn[hit])
        dev.close()


@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name", ["cornell-box", "synthetic"])
def test_refit_structure(mcpt, name, build, tmp_path_factory):
    """After a refit: topology and triangle slots unchanged, the hierarchy valid for the moved faces within the recorded stack need, the
    node bytes exactly the numpy refit's, the cost figure numpy's to 1e-9 (fp64 sums of n terms in another order: n 2^-53 << 1e-9)."""
    sc, v, _, _ = base(mcpt, name, tmp_path_factory)
    dev = mcpt.Device(sc, 0, build=BUILDS[build])
    info0, nodes0, faces0 = dev.fast_hierarchy()
    # identity first: only axes where the builder's exponent was not the smallest one may change
    i_id = dev.update_vertices(v, mode="refit")
    _, nodes_id, faces_id = dev.fast_hierarchy()
    tl, th = v[faces0].reshape(-1, 3, 3).min(axis=1), v[faces0].reshape(-1, 3, 3).max(axis=1)
    ref_id, _, _ = R.refit(nodes0, tl, th)
    a, b = F.decode(nodes0), F.decode(nodes_id)
    changed = int((a["e"] != b["e"]).sum())
    print("%s %s: identity refit lowered the exponent on %d of %d node axes" % (name, build, changed, a["e"].size))
    assert np.array_equal(nodes_id, ref_id) and np.array_equal(faces_id, faces0)
    keep = (a["e"] == b["e"]).all(axis=1)
    assert np.array_equal(nodes_id[keep], nodes0[keep])
    assert i_id["leaves_moved"] == 0
    assert abs(i_id["cost_before"] - R.cost(nodes0)) <= 1e-9 * R.cost(nodes0)
    nv = deform(mcpt, name, "sine", tmp_path_factory)
    info = dev.update_vertices(nv, mode="refit")
    fi, nodes1, faces1 = dev.fast_hierarchy()
    c, e = F.decode(nodes0), F.decode(nodes1)
    assert np.array_equal(c["child"], e["child"]) and np.array_equal(c["nchild"], e["nchild"]) and np.array_equal(faces1, faces0)
    flo, fhi = nv.reshape(-1, 3, 3).min(axis=1), nv.reshape(-1, 3, 3).max(axis=1)
    F.check_hierarchy(nodes1, faces1, flo, fhi, stack_need=fi.cw_stack_need)
    ref, _, _ = R.refit(nodes0, flo[faces0], fhi[faces0])
    assert np.array_equal(nodes1, ref)
    assert abs(info["cost_after"] - R.cost(ref)) <= 1e-9 * R.cost(ref)
    assert info["leaves_moved"] > 0 and info["ms_total"] > 0
    dev.close()


def test_sequences(mcpt, tmp_path_factory):
    """A -> B -> A returns A's frame and A's refitted node bytes; ten refits along a path, a frame after each, against fresh devices at
    steps 0, 4 and 9; pipelined frames around updates are each the frame of their own geometry."""
    name = "cornell-box"
    sc, v, _, _ = base(mcpt, name, tmp_path_factory)
    dev = mcpt.Device(sc, 0, build=BUILDS["device_fast"])
    dev.update_vertices(v, mode="refit")
    img_a, nodes_a = dev.generateImg(SPP, seed=5), dev.fast_hierarchy()[1]
    dev.update_vertices(deform(mcpt, name, "sine", tmp_path_factory))
    assert not same(dev.generateImg(SPP, seed=5), img_a)
    dev.update_vertices(v)
    assert same(dev.generateImg(SPP, seed=5), img_a) and np.array_equal(dev.fast_hierarchy()[1], nodes_a)
    frames = []
    for step in range(10):
        dev.update_vertices(deform(mcpt, name, "path%d" % step, tmp_path_factory))
        frames.append(dev.generateImg(SPP, seed=5))
    for step in (0, 4, 9):
        fsc, fdev = fresh(mcpt, name, "path%d" % step, BUILDS["device_fast"], tmp_path_factory)
        assert same(fdev.generateImg(SPP, seed=5), frames[step]), step
        fdev.close()
    # pipelined: frame, update, frame, update, frame
    got = []
    for step in (0, 4, 9):
        dev.update_vertices(deform(mcpt, name, "path%d" % step, tmp_path_factory))
        got.append(dev.generateImg(SPP, seed=5, flags=mcpt.RENDER_PIPELINE))
    for g, step in zip(got, (0, 4, 9)):
        assert same(g, frames[step]), step
    dev.close()


def test_update_waits_for_frames_in_flight(mcpt, tmp_path_factory):
    """Frame, update, frame, update, frame with MCPT_RENDER_PIPELINE into device images on a side stream, nothing waited for in between:
    the update itself waits, so every frame is the frame of the geometry it was enqueued under."""
    import ctypes as C
    name = "cornell-box"
    sc, v, _, _ = base(mcpt, name, tmp_path_factory)
    hip = C.CDLL(mcpt.hip_runtime_path().split(", ")[0])
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0                         # hipStreamNonBlocking
    spp, nbytes = 64, W * H * 3 * 8
    geoms = [v] + [deform(mcpt, name, "path%d" % s, tmp_path_factory) for s in (4, 9)]
    want = []
    ref = mcpt.Device(sc, 0, build=BUILDS["device_fast"])
    for g in geoms:
        ref.update_vertices(g)
        want.append(ref.generateImg(spp, seed=5))
    ref.close()
    dev = mcpt.Device(sc, 0, build=BUILDS["device_fast"])
    bufs = []
    for k, g in enumerate(geoms):
        if k:
            dev.update_vertices(g)                                                       # the frame before may still be running
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), nbytes) == 0
        bufs.append(p)
        dev.render_device(p.value, spp, seed=5, flags=mcpt.RENDER_PIPELINE, stream=stream.value)
    assert hip.hipStreamSynchronize(stream) == 0
    for k, p in enumerate(bufs):
        img = np.zeros((H, W, 3))
        assert hip.hipMemcpy(img.ctypes.data_as(C.c_void_p), p, nbytes, 2) == 0          # hipMemcpyDeviceToHost
        assert same(img, want[k]), k
        assert hip.hipFree(p) == 0
    dev.close()
    assert hip.hipStreamDestroy(stream) == 0


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
@pytest.mark.parametrize("build", list(BUILDS))
def test_coordinates_out_of_range_and_back(mcpt, build, mode, tmp_path_factory):
    name = "cornell-box"
    sc, v, _, _ = base(mcpt, name, tmp_path_factory)
    dev = mcpt.Device(sc, 0, build=BUILDS[build])
    img0 = dev.generateImg(SPP, seed=5)
    bad = A.out_of_range(v)
    assert dev.update_vertices(bad, mode=mode)["fast_enabled"] == 0
    key = ("files", name, "range")
    if key not in _cache:
        d, f = source(name, tmp_path_factory)
        _cache[key] = A.write_moved(d, f, bad, str(tmp_path_factory.mktemp("range")))
    fsc = mcpt.Scene(_cache[key], name, width=W, height=H)
    fdev = mcpt.Device(fsc, 0, build=BUILDS[build])
    assert fdev.fast_hierarchy()[0].enabled == 0
    assert same(dev.generateImg(SPP, seed=5), fdev.generateImg(SPP, seed=5))
    assert dev.update_vertices(v, mode=mode)["fast_enabled"] == 1
    assert same(dev.generateImg(SPP, seed=5), img0)
    for h in (fdev, fsc, dev):
        h.close()


@pytest.mark.parametrize("lens", [False, True])
def test_set_camera(mcpt, lens, tmp_path_factory):
    name = "cornell-box"
    sc, v, _, _ = base(mcpt, name, tmp_path_factory)
    dev = mcpt.Device(sc, 0)
    if lens:
        dev.set_lens(aperture=0.02, focus_distance=3.0, jitter=True)
    first = dev.generateImg(SPP, seed=5)
    cam0 = dev.camera()
    i = sc.info
    assert np.array_equal(cam0["eye"], np.array(i.eye)) and cam0["fovy"] == i.fovy
    eye = cam0["eye"] + np.array([0.3, 0.2, -0.1])
    look = cam0["look_at"] + np.array([-0.1, 0.05, 0.0])
    up, fovy = np.array([0.1, 1.0, 0.05]), cam0["fovy"] * 0.8
    dev.set_camera(eye, look, up, fovy)
    d, f = source(name, tmp_path_factory)
    cdir = str(tmp_path_factory.mktemp("cam")) + os.sep
    A.write_moved(d, f, v, cdir)
    lines = [l for l in open(os.path.join(cdir, f + ".camera")) if not l.startswith(("eye", "lookat", "up", "fovy"))]
    with open(os.path.join(cdir, f + ".camera"), "w") as fh:
        fh.write("eye %r %r %r\nlookat %r %r %r\nup %r %r %r\nfovy %r\n" % (*map(float, eye), *map(float, look), *map(float, up), float(fovy)))
        fh.writelines(lines)
    fsc = mcpt.Scene(cdir, f, width=W, height=H)
    fdev = mcpt.Device(fsc, 0)
    if lens:
        fdev.set_lens(aperture=0.02, focus_distance=3.0, jitter=True)
    moved = dev.generateImg(SPP, seed=5)
    assert same(moved, fdev.generateImg(SPP, seed=5)) and not same(moved, first)
    dev.set_camera(cam0["eye"], cam0["look_at"], cam0["up"], cam0["fovy"])
    assert same(dev.generateImg(SPP, seed=5), first)


def test_lens_and_environment_after_a_refit(mcpt, tmp_path_factory):
    rng = np.random.default_rng(4)
    env = rng.random((8, 16, 3)).astype(np.float32) * 2.0
    for name, setup in (("glassroom", lambda d: d.set_lens(aperture=0.03, focus_distance=2.5, jitter=True, per_sample=True)),
                        ("veach-mis", lambda d: d.set_environment(env, 0.7))):
        sc, v, _, _ = base(mcpt, name, tmp_path_factory)
        dev = mcpt.Device(sc, 0, build=BUILDS["device_sah"])
        setup(dev)
        dev.update_vertices(deform(mcpt, name, "sine", tmp_path_factory))
        fsc, fdev = fresh(mcpt, name, "sine", BUILDS["device_sah"], tmp_path_factory)
        setup(fdev)
        assert same(dev.generateImg(SPP, seed=5), fdev.generateImg(SPP, seed=5)), name


def test_refusals(mcpt, tmp_path_factory):
    name = "cornell-box"
    sc, v, _, _ = base(mcpt, name, tmp_path_factory)
    dev = mcpt.Device(sc, 0)
    before = dev.generateImg(SPP, seed=5)
    for make in (lambda: dev.progressive(4, seed=1), lambda: dev.adaptive(8, 0.1, min_spp=2, seed=1)):
        pr = make()
        for mode in ("refit", "rebuild"):
            with pytest.raises(mcpt.McptError) as e:
                dev.update_vertices(deform(mcpt, name, "sine", tmp_path_factory), mode=mode)
            assert e.value.code == -3 and "progressive" in str(e.value)
        with pytest.raises(mcpt.McptError) as e:
            dev.set_camera([0, 0, 5], [0, 0, 0], [0, 1, 0], 40.0)
        assert e.value.code == -3 and "progressive" in str(e.value)
        assert same(dev.generateImg(SPP, seed=5), before) and same(dev.vertices(), v)
        pr.close()
    for eye, look, up, fovy in (([0, 0, 5], [0, 0, 5], [0, 1, 0], 40.0), ([0, 0, 5], [0, 0, 0], [0, 0, 1], 40.0),
                                ([0, 0, 5], [0, 0, 0], [0, 1, 0], 180.0), ([np.nan, 0, 5], [0, 0, 0], [0, 1, 0], 40.0)):
        with pytest.raises(mcpt.McptError) as e:
            dev.set_camera(eye, look, up, fovy)
        assert e.value.code == -3
    assert same(dev.generateImg(SPP, seed=5), before)
    nv = deform(mcpt, name, "sine", tmp_path_factory)
    hip_addr = np.int64(0)
    with pytest.raises(mcpt.McptError):                    # a numpy integer is an address too: the null one is refused by the library
        dev.update_vertices(hip_addr)
    with pytest.raises(ValueError):
        dev.update_vertices(v[:-1])
    with pytest.raises(ValueError):
        dev.update_vertices(v, mode="other")
    dev.update_vertices(nv)
    assert not same(dev.generateImg(SPP, seed=5), before)
    dev.close()


def test_device_pointer_form(mcpt, tmp_path_factory):
    """vertices already in HBM go through mcpt_device_update_vertices_device (a raw device pointer from the HIP runtime the library itself
    runs on): the same device state as the host form"""
    import ctypes as C
    name = "cornell-box"
    sc, v, _, _ = base(mcpt, name, tmp_path_factory)
    nv = deform(mcpt, name, "sine", tmp_path_factory)
    a, b = mcpt.Device(sc, 0), mcpt.Device(sc, 0)
    a.update_vertices(nv)
    hip = C.CDLL(mcpt.hip_runtime_path().split(", ")[0])
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    ptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(ptr), nv.nbytes) == 0
    assert hip.hipMemcpy(ptr, nv.ctypes.data_as(C.c_void_p), nv.nbytes, 1) == 0          # hipMemcpyHostToDevice
    info = b.update_vertices(int(ptr.value))
    assert hip.hipFree(ptr) == 0
    assert info["fast_enabled"] == 1
    assert same(a.generateImg(SPP, seed=5), b.generateImg(SPP, seed=5)) and same(b.vertices(), nv)


def test_multi_device(mcpt, tmp_path_factory):
    name = "cornell-box"
    sc, v, _, _ = base(mcpt, name, tmp_path_factory)
    nv = deform(mcpt, name, "sine", tmp_path_factory)
    one = mcpt.Device(sc, 0)
    one.update_vertices(nv)
    md = mcpt.MultiDevice(sc, devices=[0, 0, 0])
    info = md.update_vertices(nv)
    assert info["fast_enabled"] == 1
    assert same(md.generateImg(SPP, seed=5), one.generateImg(SPP, seed=5))
    cam = one.camera()
    eye = cam["eye"] + np.array([0.2, 0.1, 0.0])
    one.set_camera(eye, cam["look_at"], cam["up"], cam["fovy"])
    md.set_camera(eye, cam["look_at"], cam["up"], cam["fovy"])
    assert same(md.generateImg(SPP, seed=5), one.generateImg(SPP, seed=5))
    md.close()


def test_pre_test_rejects_no_candidate_after_a_refit(tmp_path):
    """the pre-test self-check build (csrc/variants/libmcpt_chk.so) renders a refitted scene and counts no rejected candidate"""
    import selfcheck
    ROOT = selfcheck.ROOT
    code = r'''
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import montecarlopathtracing_amd as M
import anim_scenes as A
sc = M.Scene(%r, "cornell-box", width=320, height=180)
v = np.ascontiguousarray(sc.faces()[0][:, :9])
for build in (M.BUILD_HOST, M.BUILD_DEVICE_FAST):
    dev = M.Device(sc, 0, build=build)
    dev.update_vertices(A.sine_field(v, 0.05), mode="refit")
    st = M.Stats()
    dev.generateImg(16, seed=7, stats=st)
    assert st.dom_rays > 0
    dev.close()
print("done")
''' % (ROOT, os.path.join(ROOT, "tests"), SCENES)
    out = selfcheck.run(code, timeout=600)
    assert out.returncode == 0 and "done" in out.stdout, out.stderr[-3000:]
    assert "PRE-TEST SELF-CHECK" not in out.stderr, out.stderr[-3000:]
    assert "exact tests per ray" in out.stderr
