"""GPU: the environment light (mcpt_device_set_environment).  The device functions are the numpy restatement's (tests/env_ref.py); every
pipeline and hand-over path renders the same frame under a constant sky and a varying map; the per-sample lens route pins the fold of a
missed pixel; diffuse surfaces under known skies converge to their closed forms; an environment that is cleared or inactive changes
nothing; progressive, adaptive and several-device frames agree with the one-shot frame; the kernarg self-check holds."""
import os

import numpy as np
import pytest

import env_ref
import selfcheck
from conftest import ROOT, SCENES, extra_scene_dir

pytestmark = pytest.mark.gpu

W, H, N = 160, 90, 16
SCENE_NAMES = ["cornell-box", "veach-mis", "glassroom"]
KNOBS = ("MCPT_TRACE_ENGINE", "MCPT_FINISH_ENGINE", "MCPT_FINISH_PATHS", "MCPT_WORKSPACE_GB")
SEAM_CONFIGS = {
    "pool": ({"MCPT_TRACE_ENGINE": "pool"}, 0, 0),
    "vote": ({"MCPT_TRACE_ENGINE": "vote"}, 0, 0),
    "reference-walk": ({}, 1, 0),
    "finish-0": ({"MCPT_FINISH_PATHS": "0"}, 0, 0),
    "finish-500": ({"MCPT_FINISH_PATHS": "500"}, 0, 0),
    "finish-500-vote": ({"MCPT_FINISH_PATHS": "500", "MCPT_TRACE_ENGINE": "vote"}, 0, 0),
    "finish-lane": ({"MCPT_FINISH_ENGINE": "lane"}, 0, 0),
    "small-workspace": ({"MCPT_WORKSPACE_GB": "0.016"}, 0, 0),
    "megakernel": ({}, 0, 2),
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _base(name):
    return extra_scene_dir() if name == "glassroom" else SCENES


def _knobs(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _map(W_=64, H_=32, seed=3):
    rng = np.random.default_rng(seed)
    m = rng.random((H_, W_, 3)) * 2.0
    m[:, 10:14] *= 20.0
    m[H_ // 2:, :] *= 0.05
    m[5, :] = 0.0
    return m


SKIES = {"constant": ([0.6, 0.8, 1.0], 1.5), "map": (_map(), 0.7)}


# ---------------------------------------------------------------------------------------------------------------- 1. seams
@pytest.mark.parametrize("sky", sorted(SKIES))
def test_seams_match_the_restatement(mcpt, sky):
    rgb, scale = SKIES[sky]
    sc = mcpt.Scene(SCENES, "veach-mis", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    dev.set_environment(rgb, scale)
    ref = env_ref.EnvRef(rgb, scale)
    info = dev.environment
    assert info["width"] == ref.W and info["height"] == ref.H and info["scale"] == scale
    assert info["Z"] == ref.Z
    nl = sc.info.num_lights
    rng = np.random.default_rng(4)
    pix = rng.integers(0, W * H, size=5000).astype(np.int32)
    ks = rng.integers(0, 1000, size=5000).astype(np.int32)
    for depth in (0, 3):
        d, pdf, le = dev.environment_sample(9, pix, ks, depth)
        i, j, dr, pr, lr = ref.sample_u(*env_ref.vertex_uniforms(9, pix, ks, depth, nl))
        assert np.array_equal(_bits(pdf), _bits(pr)) and np.array_equal(_bits(le), _bits(lr))
        assert np.abs(d - dr).max() <= 1e-15
        # eval gives the drawn texel's radiance except where the direction lies on a column border
        ev = dev.environment_eval(d)
        ii, jj = ref.texel_of(d)
        phi = np.mod(np.arctan2(d[:, 2], d[:, 0]), 2 * np.pi) * ref.W / (2 * np.pi)
        near = np.abs(phi - np.round(phi)) * (2 * np.pi / ref.W) < 1e-12
        same = (ii == i) & (jj == j)
        assert np.all(same | near)
        assert np.array_equal(_bits(ev[same]), _bits(ref.eval(d)[same]))
    dirs = rng.normal(size=(3000, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    dirs = np.concatenate([dirs, [[0, 1, 0], [0, -1, 0], [1, 0, 0], [0, 0, 1], [-1, 0, 0]]])
    ev = dev.environment_eval(dirs)
    phi = np.mod(np.arctan2(dirs[:, 2], dirs[:, 0]), 2 * np.pi) * ref.W / (2 * np.pi)
    near = np.abs(phi - np.round(phi)) * (2 * np.pi / ref.W) < 1e-12
    assert np.array_equal(_bits(ev[~near]), _bits(ref.eval(dirs)[~near]))
    dev.set_environment(None)
    assert dev.environment is None
    with pytest.raises(mcpt.McptError):
        dev.environment_eval(dirs[:3])
    dev.close()
    sc.close()


# ---------------------------------------------------------------------------------------------------------------- 2. pipelines
@pytest.mark.parametrize("sky", sorted(SKIES))
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_every_pipeline_renders_the_same_frame(mcpt, monkeypatch, name, sky):
    rgb, scale = SKIES[sky]
    frames = {}
    for config in sorted(SEAM_CONFIGS):
        env, mode, flags = SEAM_CONFIGS[config]
        _knobs(monkeypatch, env)
        sc = mcpt.Scene(_base(name), name, width=W, height=H)
        dev = mcpt.Device(sc, 0)
        if mode:
            dev.set_trace_mode(mcpt.TRACE_REFERENCE)
        plain = dev.generateImg(N, seed=5, flags=flags)
        dev.set_environment(rgb, scale)
        frames[config] = dev.generateImg(N, seed=5, flags=flags)
        assert not np.array_equal(_bits(frames[config]), _bits(plain))
        dev.close()
        sc.close()
    ref = frames["megakernel"]
    for config, img in frames.items():
        bad = int((_bits(img) != _bits(ref)).sum())
        assert bad == 0, "%s %s %s: %d channels differ from the megakernel" % (name, sky, config, bad)


# ---------------------------------------------------------------------------------------------------------------- 3. lenses
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_lens_routes_under_an_environment(mcpt, monkeypatch, name):
    _knobs(monkeypatch, {})
    rgb, scale = SKIES["map"]
    sc = mcpt.Scene(SCENES, name, width=W, height=H)
    dev = mcpt.Device(sc, 0)
    dev.set_environment(rgb, scale)
    pin = dev.generateImg(N, seed=6)
    dev.set_lens(per_sample=True)
    for flags in (0, 2):
        assert np.array_equal(_bits(dev.generateImg(N, seed=6, flags=flags)), _bits(pin)), flags
    dev.set_lens(aperture=0.02, jitter=True)
    wf = dev.generateImg(N, seed=6)
    mk = dev.generateImg(N, seed=6, flags=2)
    assert np.array_equal(_bits(wf), _bits(mk))
    assert not np.array_equal(_bits(wf), _bits(pin))
    dev.close()
    sc.close()


# ---------------------------------------------------------------------------------------------------------------- 4. closed forms
def _floor_scene(mcpt, rho, width=32, height=18, half=50.0, size=None):
    """an upward (+y) diffuse quad of albedo rho at y = 0, seen from (0, 3, 0) looking down; no lights"""
    h = half if size is None else size
    v = np.array([[-h, 0, -h, -h, 0, h, h, 0, h], [-h, 0, -h, h, 0, h, h, 0, -h]], dtype=np.float64)
    vn = np.tile([0.0, 1.0, 0.0], (2, 3))
    rec = np.array([[rho, rho, rho, 0.0, 0.0, 0.0, 1.0, 1.0]])
    return mcpt.Scene.from_arrays(v, vn, np.zeros(2, dtype=np.int32), rec, np.zeros(0, dtype=np.int32), np.zeros((0, 3)), [0.0, 3.0, 0.0],
                                  [0.0, 0.0, 0.0], [0.0, 0.0, -1.0], 30.0, width, height)


def _z(img, expect):
    x = img.reshape(-1, 3)
    m = x.mean(axis=0)
    s = x.std(axis=0, ddof=1) / np.sqrt(x.shape[0])
    return np.abs(m - expect) / np.maximum(s, 1e-300)


@pytest.mark.parametrize("flags", [0, 2])
def test_diffuse_floor_under_a_constant_sky(mcpt, monkeypatch, flags):
    _knobs(monkeypatch, {})
    rho, L = 0.5, np.array([1.0, 2.0, 0.5])
    sc = _floor_scene(mcpt, rho)
    assert sc.info.num_lights == 0
    dev = mcpt.Device(sc, 0)
    assert np.all(dev.generateImg(4, seed=1, flags=flags) == 0.0)           # no lights, no sky: black
    dev.set_environment(L)
    img = dev.generateImg(256, seed=2, flags=flags)
    z = _z(img, rho * L)
    assert np.all(z < 5.0), z
    dev.close()
    sc.close()


def test_diffuse_floor_under_a_band(mcpt, monkeypatch):
    _knobs(monkeypatch, {})
    rho = 0.8
    W_, H_ = 16, 8
    m = np.zeros((H_, W_, 3))
    m[1, 3:6] = [[4.0, 2.0, 1.0], [1.0, 1.0, 1.0], [0.5, 3.0, 2.0]]
    sc = _floor_scene(mcpt, rho)
    dev = mcpt.Device(sc, 0)
    dev.set_environment(m)
    img = dev.generateImg(512, seed=3)
    t0, t1 = np.pi * 1 / H_, np.pi * 2 / H_
    dphi = 2 * np.pi / W_
    expect = rho / np.pi * m[1, 3:6].sum(axis=0) * dphi * (np.sin(t1) ** 2 - np.sin(t0) ** 2) / 2
    z = _z(img, expect)
    assert np.all(z < 5.0), (z, img.reshape(-1, 3).mean(axis=0), expect)
    dev.close()
    sc.close()


def _fold(x, n):
    acc = np.float32(0.0)
    for _ in range(n):
        acc = np.float32(np.float64(acc) + x / n)
    return np.float64(acc)


def test_missed_pixels_are_the_folded_sky(mcpt, monkeypatch):
    _knobs(monkeypatch, {})
    W_, H_, N_ = 48, 27, 8
    sc = _floor_scene(mcpt, 0.5, W_, H_, size=0.3)
    dev = mcpt.Device(sc, 0)
    rgb, scale = SKIES["map"]
    dev.set_environment(rgb, scale)
    pix = np.arange(W_ * H_, dtype=np.int32)
    rays = dev.camera_rays(1, pix, np.zeros_like(pix))
    face, _, _, _ = dev.ray_intersect(rays)
    miss = face < 0
    assert miss.sum() > 100 and (~miss).sum() > 20
    le = dev.environment_eval(rays[:, 3:])
    for flags in (0, 2):
        img = dev.generateImg(N_, seed=4, flags=flags).reshape(-1, 3)
        want = np.array([[_fold(x, N_) for x in row] for row in le[miss]])
        assert np.array_equal(_bits(img[miss]), _bits(want)), flags
    dev.close()
    sc.close()


# ---------------------------------------------------------------------------------------------------------------- 5. off means off
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_cleared_or_inactive_environment_changes_nothing(mcpt, monkeypatch, name):
    _knobs(monkeypatch, {})
    sc = mcpt.Scene(SCENES, name, width=W, height=H)
    dev = mcpt.Device(sc, 0)
    st0 = mcpt.Stats()
    ref = dev.generateImg(N, seed=8, stats=st0)
    dev.set_environment(*SKIES["map"])
    lit = dev.generateImg(N, seed=8)
    assert not np.array_equal(_bits(lit), _bits(ref))
    dev.set_environment(None)
    assert np.array_equal(_bits(dev.generateImg(N, seed=8)), _bits(ref))
    dev.set_environment(np.zeros((4, 8, 3)))
    assert dev.environment["Z"] == 0.0
    st1 = mcpt.Stats()
    assert np.array_equal(_bits(dev.generateImg(N, seed=8, stats=st1)), _bits(ref))
    for f in ("rays_primary", "rays_shadow", "rays_bounce", "shade_calls", "samples", "max_depth", "shadow_skipped"):
        assert getattr(st1, f) == getattr(st0, f), f
    with pytest.raises(mcpt.McptError):
        dev.environment_eval(np.array([[0.0, 1.0, 0.0]]))
    dev.close()
    sc.close()


# ---------------------------------------------------------------------------------------------------------------- 6. progressive, adaptive
@pytest.mark.parametrize("name", ["cornell-box", "glassroom"])
def test_progressive_and_adaptive_under_an_environment(mcpt, monkeypatch, name):
    _knobs(monkeypatch, {})
    sc = mcpt.Scene(_base(name), name, width=W, height=H)
    dev = mcpt.Device(sc, 0)
    dev.set_environment(*SKIES["map"])
    one = dev.generateImg(32, seed=7)
    pr = dev.progressive(32, seed=7)
    dev.set_environment(None)                  # (the handle keeps the environment it was created under)
    for n in (8, 8, 16):
        pr.step(n)
        if pr.done < 32:
            part = pr.image()
    assert np.array_equal(_bits(pr.image()), _bits(one))
    counts = dev.sample_radiance(7, np.arange(5, dtype=np.int32), np.zeros(5, dtype=np.int32))
    assert counts.shape == (5, 3)
    err = pr.stderr()
    pix = np.arange(W * H, dtype=np.int32)
    face, _, _, _ = dev.ray_intersect(dev.camera_rays(7, pix, np.zeros_like(pix)))
    miss = (face < 0).reshape(H, W)
    if miss.any():
        assert np.all(err[miss] == 0.0)
        assert np.array_equal(_bits(part[miss]), _bits(one[miss]))         # a missed pixel shows the frame's sky at every count
        den = pr.denoise(iterations=2)
        assert np.array_equal(_bits(den[miss]), _bits(pr.image()[miss]))
    pr.close()
    dev.set_environment(*SKIES["map"])
    ad = dev.adaptive(32, rel_target=0.0, min_spp=4, seed=7)
    while ad.active:
        ad.step(4)
    # hit pixels run to N; a missed pixel leaves the active list after the first pass, as it does without an environment, and shows the
    # frame's fold of Le from then on: the one-shot frame bit for bit
    img, counts = ad.image(), ad.sample_counts().reshape(H, W)
    assert np.array_equal(_bits(img), _bits(one)) and np.all(counts[~miss] == 32)
    if miss.any():
        assert np.all(counts[miss] == 4)
        assert np.all(ad.stderr()[miss] == 0.0)
    ad.close()
    dev.close()
    sc.close()


def test_multi_device_matches_the_device(mcpt, monkeypatch):
    _knobs(monkeypatch, {})
    sc = mcpt.Scene(SCENES, "cornell-box", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    dev.set_environment(*SKIES["map"])
    one = dev.generateImg(N, seed=9)
    dev.close()
    md = mcpt.MultiDevice(sc, [0])
    md.set_environment(*SKIES["map"])
    assert np.array_equal(_bits(md.generateImg(N, seed=9)), _bits(one))
    md.close()
    sc.close()


def test_lens_progressive_moments_are_the_samples(mcpt, monkeypatch):
    """A jittered lens under a varying map: every pixel's moments hold all of its samples, hit or not, in every pass -- the stderr and the
    partial estimates of the progressive handle are those of the per-sample radiance mcpt_sample_radiance gives for the same samples
    (pixels on an edge against the sky have passes in which no camera ray hits)."""
    _knobs(monkeypatch, {})
    W_, H_, N_ = 80, 45, 16
    sc = mcpt.Scene(SCENES, "cornell-box", width=W_, height=H_)
    dev = mcpt.Device(sc, 0)
    dev.set_environment(*SKIES["map"])
    dev.set_lens(aperture=0.05, jitter=True)
    pix = np.repeat(np.arange(W_ * H_, dtype=np.int32), N_)
    ks = np.tile(np.arange(N_, dtype=np.int32), W_ * H_)
    x = dev.sample_radiance(13, pix, ks).reshape(H_, W_, N_, 3)
    pr = dev.progressive(N_, seed=13)
    done = 0
    for n in (4, 4, 8):
        pr.step(n)
        done += n
        s1 = np.zeros((H_, W_, 3))
        s2 = np.zeros((H_, W_, 3))
        for k in range(done):
            s1 += x[:, :, k]
            s2 += x[:, :, k] * x[:, :, k]
        var = np.maximum((s2 - s1 * s1 / done) / (done - 1), 0.0) / done
        err = pr.stderr()
        assert np.allclose(err, np.sqrt(var), rtol=1e-9, atol=1e-15), np.abs(err - np.sqrt(var)).max()
        if done < N_:
            assert np.allclose(pr.image(), s1 / done, rtol=1e-12, atol=0.0)
    # the final frame is the one-shot frame
    assert np.array_equal(_bits(pr.image()), _bits(dev.generateImg(N_, seed=13)))
    pr.close()
    dev.close()
    sc.close()


# ---------------------------------------------------------------------------------------------------------------- 7. render_scene
def test_render_scene_environment_png_and_checkpoints(mcpt, tmp_path):
    """render_scene with an environment map: the PNG is the quantised Device frame; a checkpoint of a frame without the environment is
    not resumed by a frame with it, nor the reverse; a frame resumed from its own checkpoint is the uninterrupted one."""
    from PIL import Image
    out = str(tmp_path) + os.sep
    rgb, scale = SKIES["map"]
    pfm = out + "sky.pfm"
    mcpt.write_pfm(pfm, rgb)
    kw = dict(seed=9, width=80, height=60, quiet=True)
    mcpt.render_scene(SCENES, "cornell-box", 6, output_prefix=out + "sky", environment=pfm, environment_scale=scale, **kw)
    want_png = open(out + "sky-SPP6.png", "rb").read()
    sc = mcpt.Scene(SCENES, "cornell-box", width=80, height=60)
    dev = mcpt.Device(sc, 0)
    plain = dev.generateImg(6, seed=9)
    dev.set_environment(mcpt.read_pfm(pfm), scale)
    full = dev.generateImg(6, seed=9)
    assert np.array_equal(np.array(Image.open(out + "sky-SPP6.png").convert("RGB")), mcpt.imshow_rgb8(full))
    ck = out + "frame.ckp"
    mcpt.render_scene(SCENES, "cornell-box", 6, output_prefix=out + "first", checkpoint=ck, checkpoint_parts=5, environment=pfm,
                      environment_scale=scale, **kw)
    assert open(out + "first-SPP6.png", "rb").read() == want_png
    # the frame's own checkpoint with partitions 1 and 4 marked undone: only those are rendered again, the PNG is the same
    raw = bytearray(open(ck, "rb").read())
    head = 40
    missing = 0
    for r in (1, 4):
        raw[head + r] = 0
        missing += sc.owned_pixels(r, 5).size
    open(ck, "wb").write(bytes(raw))
    st = mcpt.Stats()
    mcpt.render_scene(SCENES, "cornell-box", 6, output_prefix=out + "resumed", checkpoint=ck, checkpoint_parts=5, environment=pfm,
                      environment_scale=scale, stats=st, **kw)
    assert open(out + "resumed-SPP6.png", "rb").read() == want_png and st.samples == missing * 6
    # not a frame without the environment: the public loader (that identity) refuses it, a plain run renders everything
    with pytest.raises(mcpt.McptError):
        mcpt.checkpoint_load(ck, sc, 6, 9, 5)
    st = mcpt.Stats()
    mcpt.render_scene(SCENES, "cornell-box", 6, output_prefix=out + "plain", checkpoint=ck, checkpoint_parts=5, stats=st, **kw)
    assert st.samples == 80 * 60 * 6
    assert np.array_equal(np.array(Image.open(out + "plain-SPP6.png").convert("RGB")), mcpt.imshow_rgb8(plain))
    # ... and the plain frame's checkpoint is not resumed by a frame with the environment
    st = mcpt.Stats()
    mcpt.render_scene(SCENES, "cornell-box", 6, output_prefix=out + "sky2", checkpoint=ck, checkpoint_parts=5, environment=pfm,
                      environment_scale=scale, stats=st, **kw)
    assert st.samples == 80 * 60 * 6 and open(out + "sky2-SPP6.png", "rb").read() == want_png
    # an all-zero map is inactive: the plain frame's identity, so its checkpoint resumes (nothing is left to render)
    mcpt.render_scene(SCENES, "cornell-box", 6, output_prefix=out + "plain2", checkpoint=ck, checkpoint_parts=5, **kw)
    zero = out + "zero.pfm"
    mcpt.write_pfm(zero, np.zeros((4, 8, 3)))
    st = mcpt.Stats()
    mcpt.render_scene(SCENES, "cornell-box", 6, output_prefix=out + "zero", checkpoint=ck, checkpoint_parts=5, environment=zero, stats=st, **kw)
    assert st.samples == 0
    assert np.array_equal(np.array(Image.open(out + "zero-SPP6.png").convert("RGB")), mcpt.imshow_rgb8(plain))
    dev.close()
    sc.close()


# ---------------------------------------------------------------------------------------------------------------- 8. kernarg self-check
def test_kernarg_self_check_with_an_environment():
    code = r'''
import os, sys
sys.path.insert(0, %r)
import montecarlopathtracing_amd as M
sc = M.Scene(%r, "veach-mis", width=160, height=90)
for engine in ("pool", "vote"):
    os.environ["MCPT_TRACE_ENGINE"] = engine
    dev = M.Device(sc, 0)
    dev.set_environment([0.5, 0.7, 1.0])
    dev.generateImg(8, seed=1, stats=M.Stats())
    dev.close()
print("done")
''' % (ROOT, SCENES)
    out = selfcheck.run(code, timeout=900)
    assert out.returncode == 0 and "done" in out.stdout, out.stderr[-3000:]
    found = selfcheck.kernarg_checks(out.stderr)
    assert len(found) == 2, found
    assert all(a == 0 for a, _ in found) and all(b > 0 for _, b in found), found
