"""-m gpu: motion blur (mcpt_device_set_motion).  A shutter frame is defined sample by sample through static scenes: sample k of step j is
what mcpt_sample_radiance returns on a FRESH device made from the files of the scene moved to V(u_j) (tests/anim_scenes.py), under the
camera C(u_j); the frame is the float fold of those.  u_j, the sample -> step map and the blend are restated in numpy (tests/motion_ref.py).
Every comparison is bit for bit (np.array_equal on the bit patterns), except the oracle cross-check, which keeps the project's 1e-9
relative for device against oracle."""
import os

import numpy as np
import pytest

import anim_scenes as A
import motion_ref as MR
from conftest import SCENES, extra_scene_dir

pytestmark = pytest.mark.gpu

W, H, N = 48, 32, 12
SEED = 5
ERR_ARG, ERR_PARSE = -3, -2
KNOBS = ("MCPT_TRACE_ENGINE", "MCPT_FINISH_ENGINE", "MCPT_FINISH_PATHS", "MCPT_WORKSPACE_GB")
BUILDS = {"host": 0, "device_fast": 2, "device_sah": 3}
SHUTTERS = [(0.0, 1.0), (0.25, 0.5), (1.0, 1.0)]
STEPS = [1, 3, N]
REL_TOL = 1e-9                  # per-sample radiance, device against oracle (test_gpu_parity.py)
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
    if name == "synthetic":
        if "syn" not in _cache:
            from montecarlopathtracing_amd import synthetic
            d = str(tmp_factory.mktemp("syn")) + os.sep
            synthetic.write_obj(synthetic.generate(20000, width=W, height=H), d, "synthetic")
            _cache["syn"] = d
        return _cache["syn"], "synthetic"
    return (extra_scene_dir() if name == "glassroom" else SCENES), name


def base(mcpt, name, tmp_factory):
    """the scene, key 0's vertices [n, 9], key 1's (each scene with the deformation named in the issue) and the scene's camera"""
    key = ("base", name)
    if key not in _cache:
        d, f = source(name, tmp_factory)
        sc = mcpt.Scene(d, f, width=W, height=H)
        g, m, _ = sc.faces()
        v0 = np.ascontiguousarray(g[:, :9])
        lights = [sc.light(i)[2] for i in range(sc.info.num_lights)]
        names = [sc.material(i)[0] for i in range(sc.info.num_materials)]
        if name == "cornell-box":
            v1 = A.rigid(v0, np.nonzero(m == names.index("Table"))[0]) if "Table" in names else A.sine_field(v0, 0.03)
        elif name == "veach-mis":
            v1 = A.move_lights(v0, m, lights)                  # the light tables change in every step
        else:
            v1 = A.sine_field(v0, 0.03)
        i = sc.info
        cam = {"eye": np.array(i.eye), "look_at": np.array(i.look_at), "up": np.array(i.up), "fovy": float(i.fovy)}
        _cache[key] = (sc, v0, np.ascontiguousarray(v1), cam)
    return _cache[key]


def moved_camera(cam, v0):
    """key 1's camera: the eye shifted by 4 % of the scene's diagonal, the target by 2 %, a little roll and zoom"""
    d = A.diagonal(v0)
    return {"eye": cam["eye"] + d * np.array([0.04, 0.01, -0.02]), "look_at": cam["look_at"] + d * np.array([-0.02, 0.0, 0.01]),
            "up": cam["up"] + np.array([0.05, 0.0, 0.02]), "fovy": cam["fovy"] * 0.9}


ENV = np.array([[[0.6, 0.7, 1.0], [0.2, 0.2, 0.3], [0.9, 0.8, 0.5], [0.1, 0.3, 0.2]], [[0.3, 0.25, 0.2], [0.05, 0.05, 0.1], [0.4, 0.3, 0.3], [0.2, 0.2, 0.2]]])
LENS = {"aperture": 0.02, "jitter": True}


def dress(dev, lens, env):
    if lens:
        dev.set_lens(**LENS)
    if env:
        dev.set_environment(ENV, 0.8)


def step_samples(mcpt, name, u, build, moves, lens, env, tmp_factory, want_files=False):
    """[W*H, N, 3]: every sample of every pixel on a fresh device of the scene at time u (moves = (geometry, camera)), and the files"""
    key = ("samples", name, float(u), build, moves, lens, env)
    if key not in _cache:
        _, v0, v1, cam = base(mcpt, name, tmp_factory)
        d, f = source(name, tmp_factory)
        if moves[0]:
            d = A.write_moved(d, f, np.ascontiguousarray(MR.blend(v0, v1, u)), str(tmp_factory.mktemp("step")))
        sc = mcpt.Scene(d, f, width=W, height=H)
        dev = mcpt.Device(sc, 0, build=BUILDS[build])
        dress(dev, lens, env)
        if moves[1]:
            c = MR.blend_camera(cam, moved_camera(cam, v0), u)
            dev.set_camera(c["eye"], c["look_at"], c["up"], c["fovy"])
        pix = np.repeat(np.arange(W * H, dtype=np.int32), N)
        ks = np.tile(np.arange(N, dtype=np.int32), W * H)
        _cache[key] = (dev.sample_radiance(SEED, pix, ks).reshape(W * H, N, 3), d, f)
        dev.close()
        sc.close()
    return _cache[key] if want_files else _cache[key][0]


def expected_samples(mcpt, name, shutter, K, build, moves, lens, env, tmp_factory):
    x = np.zeros((W * H, N, 3))
    for j, (k0, n) in enumerate(MR.step_ranges(N, K)):
        u = MR.shutter_time(shutter[0], shutter[1], K, j)
        x[:, k0:k0 + n] = step_samples(mcpt, name, u, build, moves, lens, env, tmp_factory)[:, k0:k0 + n]
    return x


def expected_frame(mcpt, name, shutter, K, build, moves, lens, env, tmp_factory):
    return MR.fold(expected_samples(mcpt, name, shutter, K, build, moves, lens, env, tmp_factory), N).reshape(H, W, 3)


def motion_device(mcpt, name, shutter, K, build, moves, lens, env, tmp_factory):
    sc, v0, v1, cam = base(mcpt, name, tmp_factory)
    dev = mcpt.Device(sc, 0, build=BUILDS[build])
    dress(dev, lens, env)
    dev.set_motion(v_end=v1 if moves[0] else None, camera_end=moved_camera(cam, v0) if moves[1] else None, shutter=shutter, steps=K)
    return dev


def check_case(mcpt, name, shutter, K, build, trace, moves, lens, env, tmp_factory, flags=0):
    dev = motion_device(mcpt, name, shutter, K, build, moves, lens, env, tmp_factory)
    dev.set_trace_mode(trace)
    img = dev.generateImg(N, seed=SEED, flags=flags)
    want = expected_frame(mcpt, name, shutter, K, build, moves, lens, env, tmp_factory)
    diff = int((bits(img) != bits(want)).sum())
    assert diff == 0, "%s shutter %s K %d %s trace %d: %d of %d channels differ" % (name, shutter, K, build, trace, diff, img.size)
    info = dev.motion_info()
    assert info["steps_run"] == K
    if moves[0]:
        assert info["ms_updates"] > 0 and info["max_cost_ratio"] > 0
    dev.close()
    return img


# ---- 1. composition
@pytest.mark.parametrize("trace", [0, 1])
@pytest.mark.parametrize("build", list(BUILDS))
def test_cornell_box_composes_over_the_full_grid(mcpt, build, trace, tmp_path_factory):
    """cornell-box, an object rotating and the camera moving: every K x shutter under this build and trace mode"""
    frames = []
    for K in STEPS:
        for shutter in SHUTTERS:
            frames.append(check_case(mcpt, "cornell-box", shutter, K, build, trace, (True, True), False, False, tmp_path_factory))
    assert not same(frames[0], frames[1]) and not same(frames[0], frames[3])        # the grid's frames are different frames


# every scene, build mode, trace mode, K and shutter occurs (cornell-box runs the full product above)
OTHERS = [("veach-mis", (0.0, 1.0), 3, "host", 0), ("veach-mis", (0.25, 0.5), N, "device_sah", 1), ("veach-mis", (1.0, 1.0), 1, "device_fast", 0),
          ("glassroom", (0.0, 1.0), N, "device_fast", 1), ("glassroom", (0.25, 0.5), 3, "host", 0), ("glassroom", (1.0, 1.0), 3, "device_sah", 0),
          ("synthetic", (0.0, 1.0), 3, "device_sah", 0), ("synthetic", (0.25, 0.5), 1, "host", 1), ("synthetic", (1.0, 1.0), N, "device_fast", 0)]


@pytest.mark.parametrize("name,shutter,K,build,trace", OTHERS)
def test_other_scenes_compose(mcpt, name, shutter, K, build, trace, tmp_path_factory):
    check_case(mcpt, name, shutter, K, build, trace, (True, True), False, False, tmp_path_factory)


def test_megakernel_renders_the_same_shutter_frame(mcpt, tmp_path_factory):
    check_case(mcpt, "cornell-box", (0.0, 1.0), 3, "host", 0, (True, True), False, False, tmp_path_factory, flags=mcpt.RENDER_MEGAKERNEL)


def test_samples_agree_with_the_oracle(mcpt, oracle, tmp_path_factory):
    """the per-sample values the composition test folds, held to the CPU oracle run on the same files (geometry moves, K = 3)"""
    name, shutter, K = "cornell-box", (0.0, 1.0), 3
    rng = np.random.default_rng(2)
    for j, (k0, n) in enumerate(MR.step_ranges(N, K)):
        u = MR.shutter_time(shutter[0], shutter[1], K, j)
        x, d, f = step_samples(mcpt, name, u, "host", (True, False), False, False, tmp_path_factory, want_files=True)
        osc = oracle.OracleScene(d + f, texture_dir=d, width=W, height=H)
        pix = rng.integers(0, W * H, size=60)
        ks = rng.integers(k0, k0 + n, size=60)
        o = np.array([osc.sample_radiance(SEED, int(p) // W, int(p) % W, int(k)) for p, k in zip(pix, ks)])
        g = x[pix, ks]
        assert np.array_equal(np.isnan(g), np.isnan(o))
        fin = np.isfinite(o).all(axis=1)
        err = np.abs(g[fin] - o[fin]).max(axis=1) / np.maximum(np.abs(o[fin]).max(axis=1), 1e-12)
        print("step %d: max relative error against the oracle %.3e over %d samples" % (j, err.max(), int(fin.sum())))
        assert err.max() <= REL_TOL and np.abs(o[fin]).sum() > 0
        osc.close()


# ---- 2. static equivalence
@pytest.mark.parametrize("build", list(BUILDS))
def test_equal_keys_render_the_static_frame(mcpt, build, tmp_path_factory):
    sc, v0, _, cam = base(mcpt, "cornell-box", tmp_path_factory)
    dev = mcpt.Device(sc, 0, build=BUILDS[build])
    static = dev.generateImg(N, seed=SEED)
    for K, shutter in ((1, (0.0, 1.0)), (5, (0.25, 0.5)), (N, (0.0, 1.0)), (7, (1.0, 1.0))):
        dev.set_motion(v_end=v0.copy(), camera_end=dict(cam), shutter=shutter, steps=K)
        assert same(dev.generateImg(N, seed=SEED), static), (K, shutter)
    dev.set_motion(steps=4)                                     # nothing moves at all
    assert same(dev.generateImg(N, seed=SEED), static)
    dev.set_motion(v_end=base(mcpt, "cornell-box", tmp_path_factory)[2], steps=3)
    assert not same(dev.generateImg(N, seed=SEED), static)
    dev.clear_motion()
    assert dev.motion is None and same(dev.generateImg(N, seed=SEED), static)
    dev.close()


# ---- 3. progressive
@pytest.mark.parametrize("lens", [False, True])
def test_progressive_passes_add_up_to_the_shutter_frame(mcpt, lens, tmp_path_factory):
    dev = motion_device(mcpt, "cornell-box", (0.0, 1.0), 3, "host", (True, True), lens, False, tmp_path_factory)
    one_shot = dev.generateImg(N, seed=SEED)
    seen = {}
    for passes in ((5, 5, 2), (1,) * N, (N,)):
        pr = dev.progressive(N, seed=SEED)
        for n in passes:
            pr.step(n)
            nz = pr.noise()
            state = (pr.image(), pr.stderr(), (nz.pixels, nz.sum_se2, nz.sum_mean2, nz.rel_error, nz.abs_rms))
            if pr.done in seen:
                for a, b in zip(seen[pr.done][:2], state[:2]):
                    assert same(a, b), (passes, pr.done)
                assert np.array_equal(np.array(seen[pr.done][2]).view(np.uint64), np.array(state[2]).view(np.uint64)), (passes, pr.done)
            else:
                seen[pr.done] = state
        assert pr.done == N and same(pr.image(), one_shot), passes
        pr.close()
    assert {5, 10, 12} <= set(seen) and seen[10][2][1] > 0
    assert same(dev.generateImg(N, seed=SEED), one_shot)
    dev.close()


# ---- 4. camera only, geometry only
@pytest.mark.parametrize("moves", [(False, True), (True, False)])
def test_one_key_may_stay(mcpt, moves, tmp_path_factory):
    for name, build in (("cornell-box", "device_fast"), ("glassroom", "host")):
        check_case(mcpt, name, (0.0, 1.0), 3, build, 0, moves, False, False, tmp_path_factory)


# ---- 5. key 0 is what queries see
@pytest.mark.parametrize("build", list(BUILDS))
def test_queries_see_key_0(mcpt, build, tmp_path_factory):
    sc, v0, v1, cam = base(mcpt, "cornell-box", tmp_path_factory)
    rng = np.random.default_rng(11)
    p = v0.reshape(-1, 3)
    lo, hi = p.min(axis=0) - 0.2, p.max(axis=0) + 0.2
    o = lo + (hi - lo) * rng.random((80000, 3))
    d = rng.normal(size=(80000, 3))
    d[:20000] = p[rng.integers(0, p.shape[0], size=20000)] - o[:20000]
    rays = np.ascontiguousarray(np.hstack([o, d / np.linalg.norm(d, axis=1, keepdims=True)]))
    pix = np.arange(0, W * H, 7, dtype=np.int32)

    def observe(dev):
        out = {}
        for mode in (0, 1):
            dev.set_trace_mode(mode)
            out["hit%d" % mode] = dev.ray_intersect(rays)
        dev.set_trace_mode(0)
        out["v"] = dev.vertices()
        out["nodes"] = dev.bvh_nodes()
        out["order"] = dev.leaf_order()
        out["rad"] = dev.sample_radiance(3, pix, (pix % 3).astype(np.int32))
        c = dev.camera()
        out["cam"] = np.hstack([c["eye"], c["look_at"], c["up"], [c["fovy"]]])
        return out

    plain = mcpt.Device(sc, 0, build=BUILDS[build])
    want = observe(plain)
    dev = mcpt.Device(sc, 0, build=BUILDS[build])
    dev.set_motion(v_end=v1, camera_end=moved_camera(cam, v0), shutter=(0.25, 0.5), steps=3)
    first = dev.generateImg(N, seed=SEED)
    second = dev.generateImg(N, seed=SEED)                      # two motion frames in a row, nothing in between
    assert same(first, second)
    got = observe(dev)
    for k in want:
        for a, b in zip(want[k] if isinstance(want[k], tuple) else (want[k],), got[k] if isinstance(got[k], tuple) else (got[k],)):
            assert same(a, b), k
    assert same(dev.generateImg(N, seed=SEED), first)           # ... and after the queries took the device back to key 0
    dev.generateImg(4, seed=9)                                  # frames do not depend on what was rendered before
    dev.generateImg(N, seed=SEED, flags=mcpt.RENDER_MEGAKERNEL)
    assert same(dev.generateImg(N, seed=SEED), first)
    dev.clear_motion()
    got = observe(dev)
    for k in want:
        for a, b in zip(want[k] if isinstance(want[k], tuple) else (want[k],), got[k] if isinstance(got[k], tuple) else (got[k],)):
            assert same(a, b), k
    assert same(dev.generateImg(N, seed=SEED), plain.generateImg(N, seed=SEED))
    dev.close()
    plain.close()


# ---- 6. lens and environment
@pytest.mark.parametrize("lens,env", [(True, True), (False, True), (True, False)])
def test_composition_under_a_lens_and_an_environment(mcpt, lens, env, tmp_path_factory):
    check_case(mcpt, "cornell-box", (0.0, 1.0), 3, "host", 0, (True, True), lens, env, tmp_path_factory)


def test_environment_progressive_passes(mcpt, tmp_path_factory):
    """pixels that see the sky in one step and geometry in another: passes still add up, and the estimate before N is the mean"""
    dev = motion_device(mcpt, "cornell-box", (0.0, 1.0), 3, "host", (True, True), False, True, tmp_path_factory)
    one_shot = dev.generateImg(N, seed=SEED)
    x = expected_samples(mcpt, "cornell-box", (0.0, 1.0), 3, "host", (True, True), False, True, tmp_path_factory)
    pr = dev.progressive(N, seed=SEED)
    pr.step(7)
    s1 = np.zeros((W * H, 3))
    for k in range(7):
        s1 = s1 + x[:, k]
    assert same(pr.image(), (s1 / 7).reshape(H, W, 3))
    pr.step(5)
    assert same(pr.image(), one_shot)
    pr.close()
    dev.close()


# ---- 7. vetting
def test_out_of_range_key_is_vetted_step_by_step(mcpt, tmp_path_factory):
    """key 1 has a coordinate of 1e200: every step's blend leaves [1e-150, 1e150], the reference-shaped walk answers, as on the fresh devices"""
    sc, v0, _, _ = base(mcpt, "cornell-box", tmp_path_factory)
    v1 = A.out_of_range(v0)
    dev = mcpt.Device(sc, 0, build=BUILDS["device_fast"])
    dev.set_motion(v_end=v1, shutter=(0.0, 1.0), steps=2)
    img = dev.generateImg(4, seed=SEED)
    x = np.zeros((W * H, 4, 3))
    pix, ks = np.repeat(np.arange(W * H, dtype=np.int32), 4), np.tile(np.arange(4, dtype=np.int32), W * H)
    for j, (k0, n) in enumerate(MR.step_ranges(4, 2)):
        v = np.ascontiguousarray(MR.blend(v0, v1, MR.shutter_time(0.0, 1.0, 2, j)))
        assert np.abs(v).max() > 1e150
        d = A.write_moved(SCENES, "cornell-box", v, str(tmp_path_factory.mktemp("oor")))
        fsc = mcpt.Scene(d, "cornell-box", width=W, height=H)
        fdev = mcpt.Device(fsc, 0, build=BUILDS["device_fast"])
        assert fdev.fast_hierarchy()[0].enabled == 0
        x[:, k0:k0 + n] = fdev.sample_radiance(SEED, pix, ks).reshape(W * H, 4, 3)[:, k0:k0 + n]
        fdev.close()
    assert same(img, MR.fold(x, 4).reshape(H, W, 3))
    assert dev.fast_hierarchy()[0].enabled == 1                 # key 0 again
    dev.close()


# ---- 8. refusals and clearing
def test_refusals_and_clearing(mcpt, tmp_path_factory):
    sc, v0, v1, cam = base(mcpt, "cornell-box", tmp_path_factory)
    dev = mcpt.Device(sc, 0)
    dev.set_motion(v_end=v1, camera_end=moved_camera(cam, v0), shutter=(0.25, 0.5), steps=3)
    m = dev.motion
    assert m["steps"] == 3 and m["shutter"] == (0.25, 0.5) and m["has_geometry"] and m["has_camera"]
    assert same(m["camera_end"]["eye"], moved_camera(cam, v0)["eye"])

    def refused(call):
        with pytest.raises(mcpt.McptError) as e:
            call()
        assert e.value.code == ERR_ARG and len(str(e.value)) > 25
    refused(lambda: dev.adaptive(N, 0.1))
    refused(lambda: dev.generateImg(N, seed=SEED, flags=mcpt.RENDER_PIPELINE))
    refused(lambda: dev.generateImg(2, seed=SEED))                                  # steps > spp
    refused(lambda: dev.progressive(2, seed=SEED))
    pr = dev.progressive(N, seed=SEED)
    pr.step(4)
    refused(pr.aovs)
    refused(pr.denoise)
    refused(lambda: dev.set_motion(v_end=v1, steps=2))                              # while a progressive handle lives
    refused(dev.clear_motion)
    refused(lambda: dev.update_vertices(v1))
    pr.close()
    assert dev.motion is not None
    static1 = mcpt.Device(sc, 0)
    static1.update_vertices(v1)
    dev.update_vertices(v1)                                                         # a new key 0: the motion is gone
    assert dev.motion is None and same(dev.generateImg(N, seed=SEED), static1.generateImg(N, seed=SEED))
    dev.set_motion(v_end=v0, steps=2)
    assert same(dev.vertices(), v1)
    c1 = moved_camera(cam, v0)
    dev.set_camera(c1["eye"], c1["look_at"], c1["up"], c1["fovy"])
    static1.set_camera(c1["eye"], c1["look_at"], c1["up"], c1["fovy"])
    assert dev.motion is None and same(dev.generateImg(N, seed=SEED), static1.generateImg(N, seed=SEED))
    with pytest.raises(ValueError):
        dev.set_motion(v_end=v0[:-1], steps=2)
    # a blended camera that is none fails the frame, not the process: up(u = 0.5) = 0.5 up - 0.5 up = 0
    dev.set_camera(cam["eye"], cam["look_at"], cam["up"], cam["fovy"])
    back = {"eye": cam["eye"], "look_at": cam["look_at"], "up": -cam["up"], "fovy": cam["fovy"]}
    dev.set_motion(camera_end=back, steps=1)
    refused(lambda: dev.generateImg(N, seed=SEED))
    dev.clear_motion()
    assert same(dev.camera()["eye"], cam["eye"])
    dev.close()
    static1.close()


def test_device_pointer_form(mcpt, tmp_path_factory):
    """key 1 already in HBM (mcpt_device_set_motion_device, a raw pointer from the HIP runtime the library itself runs on)"""
    import ctypes as C
    sc, v0, v1, _ = base(mcpt, "cornell-box", tmp_path_factory)
    a = mcpt.Device(sc, 0)
    a.set_motion(v_end=v1, steps=3)
    want = a.generateImg(N, seed=SEED)
    hip = C.CDLL(mcpt.hip_runtime_path())
    ptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(ptr), C.c_size_t(v1.nbytes)) == 0
    assert hip.hipMemcpy(ptr, v1.ctypes.data_as(C.c_void_p), C.c_size_t(v1.nbytes), 1) == 0
    b = mcpt.Device(sc, 0)
    b.set_motion(v_end=int(ptr.value), steps=3)
    assert hip.hipFree(ptr) == 0                                 # the device keeps its own copy of the keyframe
    assert same(b.generateImg(N, seed=SEED), want)
    a.close()
    b.close()


# ---- 9. render_scene
def test_render_scene_writes_the_shutter_frame(mcpt, tmp_path, tmp_path_factory):
    sc, v0, v1, cam = base(mcpt, "cornell-box", tmp_path_factory)
    c1 = moved_camera(cam, v0)
    end_dir = A.write_moved(SCENES, "cornell-box", v1, str(tmp_path / "end"))
    cam_file = str(tmp_path / "end.camera")
    with open(cam_file, "w") as f:
        f.write("eye %r %r %r\nlookat %r %r %r\nup %r %r %r\nfovy %r\nwidth 7\nheight 5\n" % (
            *map(float, c1["eye"]), *map(float, c1["look_at"]), *map(float, c1["up"]), float(c1["fovy"])))
    out = tmp_path / "out"
    out.mkdir()
    motion = {"end_obj": end_dir + "cornell-box.obj", "end_camera": cam_file, "shutter": (0.25, 0.5), "steps": 3}
    mcpt.render_scene(SCENES, "cornell-box", N, seed=SEED, width=W, height=H, output_prefix=str(out / "blur"), motion=motion)
    frame = expected_frame(mcpt, "cornell-box", (0.25, 0.5), 3, "host", (True, True), False, False, tmp_path_factory)
    assert os.listdir(out) == ["blur-SPP%d.png" % N]
    assert open(out / ("blur-SPP%d.png" % N), "rb").read() == bytes(mcpt.png_bytes(mcpt.imshow_rgb8(frame)))
    # the progressive route (the error image asks for it) writes the same picture
    mcpt.render_scene(SCENES, "cornell-box", N, seed=SEED, width=W, height=H, output_prefix=str(out / "prog"), motion=motion, output_flags=mcpt.OUT_ERROR_PFM)
    assert open(out / ("prog-SPP%d.png" % N), "rb").read() == open(out / ("blur-SPP%d.png" % N), "rb").read()
    # an end .obj of another scene -- another face count, or the same faces under other materials -- is refused before anything is written
    refused = tmp_path / "refused"
    refused.mkdir()
    text = open(end_dir + "cornell-box.obj").read().split("\n")
    faces = [i for i, l in enumerate(text) if l.startswith("f ")]
    short = str(tmp_path / "short.obj")
    open(short, "w").write("\n".join(text[:faces[-1]] + text[faces[-1] + 1:]))
    uses = [i for i, l in enumerate(text) if l.startswith("usemtl")]
    swapped = list(text)
    swapped[uses[0]], swapped[uses[1]] = text[uses[1]], text[uses[0]]
    other = str(tmp_path / "other.obj")
    open(other, "w").write("\n".join(swapped))
    for bad in (short, other):
        with pytest.raises(mcpt.McptError) as e:
            mcpt.render_scene(SCENES, "cornell-box", N, width=W, height=H, output_prefix=str(refused / "x"), motion=dict(motion, end_obj=bad))
        assert e.value.code == ERR_PARSE and os.listdir(refused) == []
