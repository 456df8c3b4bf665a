"""GPU: the camera lens (mcpt_device_set_lens).  The per-sample route computes the pinhole frame's paths bit for bit (MCPT_LENS_PER_SAMPLE),
the wavefront and the megakernel agree under a real lens, the camera rays are the numpy restatement's (tests/lens_ref.py), depth of field
and antialiasing meet their exact geometric answers, and partitions, several devices, pipelined frames, render_scene's checkpoints and the
kernarg self-check hold under a lens."""
import os

import numpy as np
import pytest

import lens_ref
import selfcheck
from conftest import ROOT, SCENES, extra_scene_dir

pytestmark = pytest.mark.gpu

W, H, N = 160, 90, 16
SCENE_NAMES = ["cornell-box", "veach-mis", "glassroom"]
KNOBS = ("MCPT_TRACE_ENGINE", "MCPT_FINISH_ENGINE", "MCPT_FINISH_PATHS", "MCPT_WORKSPACE_GB")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _base(name):
    return extra_scene_dir() if name == "glassroom" else SCENES


def _env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# (environment, trace mode, render flags)
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


@pytest.mark.parametrize("config", sorted(SEAM_CONFIGS))
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_per_sample_route_is_the_pinhole_frame(mcpt, monkeypatch, name, config):
    """MCPT_LENS_PER_SAMPLE, no jitter, no aperture: every sample traces its own camera ray -- the pixel's primary ray -- and starts its
    path from its own first hit; the frame is the lens-less device's, bit for bit."""
    env, mode, flags = SEAM_CONFIGS[config]
    _env(monkeypatch, env)
    sc = mcpt.Scene(_base(name), name, width=W, height=H)
    dev = mcpt.Device(sc, 0)
    if mode:
        dev.set_trace_mode(mcpt.TRACE_REFERENCE)
    ref = dev.generateImg(N, seed=5, flags=flags)
    dev.set_lens(per_sample=True)
    assert dev.lens() == {"aperture": 0.0, "focus_distance": 0.0, "jitter": False, "per_sample": True}
    st = mcpt.Stats()
    got = dev.generateImg(N, seed=5, flags=flags, stats=st)
    bad = int((_bits(got) != _bits(ref)).sum())
    assert bad == 0, "%s %s: %d channels differ from the pinhole frame" % (name, config, bad)
    assert st.rays_primary == W * H * N and st.samples == W * H * N
    dev.set_lens()
    assert np.array_equal(_bits(dev.generateImg(N, seed=5, flags=flags)), _bits(ref))
    dev.close()
    sc.close()


@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_per_sample_seam_progressive_adaptive_and_samples(mcpt, monkeypatch, name):
    """The same seam through mcpt_sample_radiance, progressive passes 8+8+16 (image, error, noise summary), and adaptive frames with
    targets 0 and with real ones (images, sample counts, summaries)."""
    _env(monkeypatch, {})
    sc = mcpt.Scene(SCENES, name, width=W, height=H)
    dev = mcpt.Device(sc, 0)
    rng = np.random.default_rng(2)
    pix = rng.integers(0, W * H, size=300).astype(np.int32)
    ks = rng.integers(0, 64, size=300).astype(np.int32)
    runs = {}
    for lensed in (False, True):
        dev.set_lens(per_sample=lensed)
        out = {"samples": dev.sample_radiance(7, pix, ks)}
        pr = dev.progressive(32, seed=7)
        for n in (8, 8, 16):
            pr.step(n)
            out["noise%d" % pr.done] = pr.noise().as_dict()
        out["img"], out["err"] = pr.image(), pr.stderr()
        pr.close()
        for rel in (0.0, 0.05):
            ad = dev.adaptive(32, rel_target=rel, min_spp=4, seed=7)
            while ad.active:
                ad.step(4)
            out["ad%g" % rel] = (ad.image(), ad.stderr(), ad.sample_counts(), ad.noise().as_dict())
            ad.close()
        runs[lensed] = out
    a, b = runs[False], runs[True]
    assert np.array_equal(_bits(a["samples"]), _bits(b["samples"]))
    assert np.array_equal(_bits(a["img"]), _bits(b["img"])) and np.array_equal(_bits(a["err"]), _bits(b["err"]))
    for k in ("noise8", "noise16", "noise32"):
        assert a[k] == b[k], (k, a[k], b[k])
    for rel in (0.0, 0.05):
        x, y = a["ad%g" % rel], b["ad%g" % rel]
        assert np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(_bits(x[1]), _bits(y[1]))
        assert np.array_equal(x[2], y[2]) and x[3] == y[3], rel
    dev.set_lens()
    assert np.array_equal(_bits(a["ad0"][0]), _bits(dev.generateImg(32, seed=7)))
    dev.close()
    sc.close()


LENS = dict(aperture=0.02, focus_distance=0.0, jitter=True)
LENS_ENGINES = {"pool": ({"MCPT_TRACE_ENGINE": "pool"}, 0), "vote": ({"MCPT_TRACE_ENGINE": "vote"}, 0),
                "pool-reference": ({"MCPT_TRACE_ENGINE": "pool"}, 1), "vote-finish-500": ({"MCPT_TRACE_ENGINE": "vote", "MCPT_FINISH_PATHS": "500"}, 0)}


@pytest.mark.parametrize("config", sorted(LENS_ENGINES))
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_wavefront_equals_megakernel_under_a_lens(mcpt, monkeypatch, name, config):
    env, mode = LENS_ENGINES[config]
    _env(monkeypatch, env)
    sc = mcpt.Scene(_base(name), name, width=W, height=H)
    dev = mcpt.Device(sc, 0)
    if mode:
        dev.set_trace_mode(mcpt.TRACE_REFERENCE)
    pin = dev.generateImg(N, seed=3)
    dev.set_lens(**LENS)
    wf = dev.generateImg(N, seed=3)
    mk = dev.generateImg(N, seed=3, flags=mcpt.RENDER_MEGAKERNEL)
    bad = int((_bits(wf) != _bits(mk)).sum())
    assert bad == 0, "%s %s: %d channels differ between the wavefront and the megakernel" % (name, config, bad)
    assert (_bits(wf) != _bits(pin)).sum() > wf.size // 4          # the lens changes the picture
    # sample_radiance over k = 0..N-1, folded as the frame folds (float, x / N in k order), is the frame's pixel
    rng = np.random.default_rng(4)
    pix = np.sort(rng.choice(W * H, size=200, replace=False)).astype(np.int32)
    x = dev.sample_radiance(3, np.repeat(pix, N), np.tile(np.arange(N, dtype=np.int32), pix.size)).reshape(pix.size, N, 3)
    acc = np.zeros((pix.size, 3), dtype=np.float32)
    for k in range(N):
        acc = (acc.astype(np.float64) + x[:, k] / N).astype(np.float32)
    assert np.array_equal(_bits(acc.astype(np.float64)), _bits(wf.reshape(-1, 3)[pix]))
    dev.close()
    sc.close()


def _ulps(a, b):
    """|a - b| per component in ulps of the largest component of its 3-vector (origin, direction).  A 1-ulp difference of sin or cos
    reaches a component that cancels (f - o, eye + x^ r cos + y^ r sin) as an absolute error of the vector's scale, hundreds of that
    component's own ulps; against the vector's scale it stays one or two."""
    out = np.zeros(a.shape)
    for part in (slice(0, 3), slice(3, 6)):
        scale = np.spacing(np.abs(b[:, part]).max(axis=1))[:, None]
        out[:, part] = np.abs(a[:, part] - b[:, part]) / scale
    return out


@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_camera_rays_are_the_restatement(mcpt, name):
    sc = mcpt.Scene(SCENES, name, width=W, height=H)
    cam = lens_ref.Camera.from_info(sc.info)
    dev = mcpt.Device(sc, 0)
    rng = np.random.default_rng(5)
    pix = rng.integers(0, W * H, size=4000).astype(np.int32)
    ks = rng.integers(0, 1 << 20, size=4000).astype(np.int32)
    seed = 0x0123456789ABCDEF
    # the inactive lens: the reference's primary rays
    assert np.array_equal(_bits(dev.camera_rays(seed, pix, ks)), _bits(lens_ref.camera_ray(cam, seed, pix, ks)))
    dev.set_lens(jitter=True)
    got = dev.camera_rays(seed, pix, ks)
    assert np.array_equal(_bits(got), _bits(lens_ref.camera_ray(cam, seed, pix, ks, jitter=True)))
    for ap, fd in ((0.05, 0.0), (0.3, 2.5)):
        dev.set_lens(aperture=ap, focus_distance=fd, jitter=True)
        got = dev.camera_rays(seed, pix, ks)
        want = lens_ref.camera_ray(cam, seed, pix, ks, aperture=ap, focus_distance=fd, jitter=True)
        assert _ulps(got, want).max() <= 4, _ulps(got, want).max()
        off = got[:, :3] - np.array(cam.eye)
        a, b = np.array(cam.xhat), np.array(cam.up)
        # the origin lies in the plane of x^, y^ through the eye, within `aperture` of it (x^, y^ need not be orthogonal)
        G = np.array([[a @ a, a @ b], [a @ b, b @ b]])
        coef = np.linalg.solve(G, np.stack([off @ a, off @ b]))
        assert np.abs(off - (coef[0][:, None] * a + coef[1][:, None] * b)).max() <= 1e-12 * max(1.0, np.abs(cam.eye).max())
        r = np.sqrt(coef[0] ** 2 + coef[1] ** 2)
        assert r.max() <= ap * (1 + 1e-12) and r.max() > 0.9 * ap
    dev.close()
    sc.close()


def _plane_scene(mcpt, z, width=64, height=36, half=50.0, cx=1.5, cy=1.5):
    """a square emitter at depth z (normal +z) in front of an orthonormal camera at (1.5, 1.5, 3.5) looking down -z"""
    x0, x1, y0, y1 = cx - half, cx + half, cy - half, cy + half
    v = np.array([[x0, y0, z, x1, y0, z, x1, y1, z], [x0, y0, z, x1, y1, z, x0, y1, z]])
    vn = np.tile([0.0, 0.0, 1.0], (2, 3))
    mat = np.zeros(2, dtype=np.int32)
    rec = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0]])
    return mcpt.Scene.from_arrays(v, vn, mat, rec, [0], [[1.0, 1.0, 1.0]], [1.5, 1.5, 3.5], [1.5, 1.5, 2.5], [0.0, 1.0, 0.0], 60.0,
                                  width, height)


def test_depth_of_field_geometry(mcpt):
    F, ap = 2.0, 0.1
    W_, H_ = 64, 36
    pix = np.full(4096, (H_ // 2) * W_ + W_ // 3, dtype=np.int32)
    ks = np.arange(4096, dtype=np.int32)
    for D in (F, F / 2):
        sc = _plane_scene(mcpt, 3.5 - D, W_, H_)
        dev = mcpt.Device(sc, 0)
        dev.set_lens(aperture=0.0, focus_distance=F)
        f0, _, p0, _ = dev.ray_intersect(dev.camera_rays(11, pix[:1], ks[:1]))
        dev.set_lens(aperture=ap, focus_distance=F)
        face, _, p, _ = dev.ray_intersect(dev.camera_rays(11, pix, ks))
        assert f0[0] >= 0 and np.all(face >= 0)
        dist = np.sqrt(((p - p0[0]) ** 2).sum(axis=1))
        if D == F:
            assert dist.max() <= 1e-9 * F, dist.max()
        else:
            blur = ap * abs(1 - D / F)
            assert 0.9 * blur <= dist.max() <= (1 + 1e-9) * blur, (dist.max(), blur)
        dev.close()
        sc.close()


def _coverage(cam, X0, X1, Y0, Y1):
    """exact area fraction of every pixel square [pos.x, pos.x + pdx] x [pos.y - pdy, pos.y] covered by [X0, X1] x [Y0, Y1]"""
    pos = cam.pos
    px, py = cam.pdx[0], cam.pdy[1]
    ox = np.clip(np.minimum(pos[:, 0] + px, X1) - np.maximum(pos[:, 0], X0), 0.0, None)
    oy = np.clip(np.minimum(pos[:, 1], Y1) - np.maximum(pos[:, 1] - py, Y0), 0.0, None)
    return ox * oy / (px * py)


def test_antialiasing_meets_the_exact_coverage(mcpt):
    """An emitter quad of radiance 1 parallel to the image plane, nothing else; SPP 4096 with jitter: a pixel's value is the fraction of
    its square the quad's projection covers (1 / 4096 and every count of it are exact in float: the fold adds no rounding)."""
    W_, H_, N_ = 64, 36, 4096
    z, l = 0.5, 1.0
    D = 3.5 - z
    qx0, qx1, qy0, qy1 = 0.7131, 2.3377, 0.9214, 2.0529
    v = np.array([[qx0, qy0, z, qx1, qy0, z, qx1, qy1, z], [qx0, qy0, z, qx1, qy1, z, qx0, qy1, z]])
    vn = np.tile([0.0, 0.0, 1.0], (2, 3))
    rec = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0]])
    sc = mcpt.Scene.from_arrays(v, vn, np.zeros(2, dtype=np.int32), rec, [0], [[1.0, 1.0, 1.0]], [1.5, 1.5, 3.5], [1.5, 1.5, 2.5],
                                [0.0, 1.0, 0.0], 60.0, W_, H_)
    cam = lens_ref.Camera.from_info(sc.info)
    assert abs(np.dot(cam.xhat, cam.up)) == 0 and cam.xhat == [1.0, 0.0, 0.0]
    # the quad's projection on the image plane (z = 2.5, distance l from the eye)
    s = l / D
    a = _coverage(cam, 1.5 + (qx0 - 1.5) * s, 1.5 + (qx1 - 1.5) * s, 1.5 + (qy0 - 1.5) * s, 1.5 + (qy1 - 1.5) * s)
    dev = mcpt.Device(sc, 0)
    plain = dev.generateImg(N_, seed=21)[..., 0].ravel()
    assert np.all((plain == 0.0) | (plain == 1.0))                          # without the lens: every pixel 0 or L
    dev.set_lens(jitter=True)
    img = dev.generateImg(N_, seed=21)
    assert np.array_equal(_bits(img[..., 0]), _bits(img[..., 1])) and np.array_equal(_bits(img[..., 0]), _bits(img[..., 2]))
    got = img[..., 0].ravel()
    full, empty = a >= 1.0 - 1e-12, a == 0.0           # (a of a covered pixel is 1 up to the rounding of its overlap widths)
    edge = ~full & ~empty
    assert full.sum() > 100 and edge.sum() > 40 and empty.sum() > 100
    assert np.all(got[full] == 1.0) and np.all(got[empty] == 0.0)
    sigma = np.sqrt(a[edge] * (1 - a[edge]) / N_)
    assert np.all(np.abs(got[edge] - a[edge]) <= 5 * sigma + 1.0 / N_), np.max(np.abs(got[edge] - a[edge]) / (sigma + 1.0 / N_))
    between = (got > 1e-6) & (got < 1 - 1e-5)         # values no pinhole frame has: only at the quad's edges, and there
    assert not np.any(between & ~edge) and between.sum() >= 0.8 * edge.sum()
    dev.close()
    sc.close()


def test_partitions_devices_and_pipelined_frames(mcpt, monkeypatch):
    import hip_rt
    _env(monkeypatch, {})
    sc = mcpt.Scene(SCENES, "veach-mis", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    dev.set_lens(**LENS)
    one = dev.generateImg(N, seed=13)
    parts = np.zeros_like(one)
    for r in (0, 1):
        dev.generateImg(N, seed=13, rank=r, world=2, tile_w=16, tile_h=8, img=parts)
    assert np.array_equal(_bits(parts), _bits(one))
    md = mcpt.MultiDevice(sc, devices=[0, 0])
    md.set_lens(**LENS)
    assert np.array_equal(_bits(md.generateImg(N, seed=13)), _bits(one))
    md.close()
    seeds = (13, 14, 15, 16)
    want = [dev.generateImg(N, seed=sd) for sd in seeds]
    nbytes = W * H * 3 * 8
    streams = [hip_rt.Stream(), hip_rt.Stream()]
    frames = [hip_rt.DeviceBuffer(nbytes), hip_rt.DeviceBuffer(nbytes)]
    got = [np.zeros((H, W, 3)) for _ in seeds]
    for i, sd in enumerate(seeds):
        t = i & 1
        dev.render_device(frames[t].ptr.value, N, sd, flags=mcpt.RENDER_PIPELINE | mcpt.RENDER_KEEP_STATS, stream=streams[t].h.value)
        frames[t].to_host_async(got[i], streams[t].h)
    for s_ in streams:
        s_.synchronize()
    for x, y in zip(want, got):
        assert np.array_equal(_bits(x), _bits(y))
    st = dev.collect_stats()
    assert st.rays_primary == len(seeds) * W * H * N
    for f in frames:
        f.free()
    for s_ in streams:
        s_.destroy()
    dev.close()
    sc.close()


def test_render_scene_lens_png_and_checkpoints(mcpt, tmp_path):
    """render_scene under a lens: the PNG is the quantised API frame; a run resumed from its own checkpoint gives the uninterrupted
    frame byte for byte; a pinhole frame's checkpoint in the same place is not resumed by a lens run, nor the reverse."""
    from PIL import Image
    out = str(tmp_path) + os.sep
    kw = dict(seed=9, width=80, height=60, quiet=True)
    lens = mcpt.make_lens(**LENS)
    mcpt.render_scene(SCENES, "cornell-box", 6, output_prefix=out + "lens", lens=lens, **kw)
    want_png = open(out + "lens-SPP6.png", "rb").read()
    sc = mcpt.Scene(SCENES, "cornell-box", width=80, height=60)
    dev = mcpt.Device(sc, 0)
    dev.set_lens(**LENS)
    full = dev.generateImg(6, seed=9)
    assert np.array_equal(np.array(Image.open(out + "lens-SPP6.png").convert("RGB")), mcpt.imshow_rgb8(full))
    # its own checkpoint, then an "interrupted" copy of it: partitions 1 and 4 not done, their pixels zeroed
    ck = out + "frame.ckp"
    mcpt.render_scene(SCENES, "cornell-box", 6, output_prefix=out + "first", checkpoint=ck, checkpoint_parts=5, lens=lens, **kw)
    assert open(out + "first-SPP6.png", "rb").read() == want_png
    raw = bytearray(open(ck, "rb").read())
    head = 40                                              # magic, width, height, spp, parts, seed, frame tag
    img = np.frombuffer(bytes(raw[head + 5:]), dtype=np.float64).reshape(-1, 3).copy()
    missing = 0
    for r in (1, 4):
        raw[head + r] = 0
        px = sc.owned_pixels(r, 5)
        img[px] = 0.0
        missing += px.size
    raw[head + 5:] = img.tobytes()
    open(ck, "wb").write(bytes(raw))
    st = mcpt.Stats()
    mcpt.render_scene(SCENES, "cornell-box", 6, output_prefix=out + "resumed", checkpoint=ck, checkpoint_parts=5, lens=lens, stats=st, **kw)
    assert open(out + "resumed-SPP6.png", "rb").read() == want_png
    assert st.samples == missing * 6                       # only the two missing partitions were rendered
    # the lens frame's file is not a pinhole frame's: the public loader (pinhole identity) refuses it, a pinhole run renders everything
    with pytest.raises(mcpt.McptError):
        mcpt.checkpoint_load(ck, sc, 6, 9, 5)
    pin = mcpt.Device(sc, 0)
    pin_full = pin.generateImg(6, seed=9)
    st = mcpt.Stats()
    mcpt.render_scene(SCENES, "cornell-box", 6, output_prefix=out + "pin", checkpoint=ck, checkpoint_parts=5, stats=st, **kw)
    assert st.samples == 80 * 60 * 6
    assert np.array_equal(np.array(Image.open(out + "pin-SPP6.png").convert("RGB")), mcpt.imshow_rgb8(pin_full))
    # a partial pinhole checkpoint (the pinhole identity, unchanged by lenses) is not resumed by a lens run
    part = np.zeros_like(pin_full)
    for r in (0, 2, 3):
        pin.generateImg(6, seed=9, rank=r, world=5, img=part)
    mcpt.checkpoint_save(ck, sc, part, 6, 9, np.array([1, 0, 1, 1, 0], dtype=np.uint8))
    st = mcpt.Stats()
    mcpt.render_scene(SCENES, "cornell-box", 6, output_prefix=out + "lens2", checkpoint=ck, checkpoint_parts=5, lens=lens, stats=st, **kw)
    assert st.samples == 80 * 60 * 6 and open(out + "lens2-SPP6.png", "rb").read() == want_png
    pin.close()
    dev.close()
    sc.close()


def test_kernarg_self_check_with_a_lens(tmp_path):
    code = r'''
import os, sys
sys.path.insert(0, %r)
import montecarlopathtracing_amd as M
sc = M.Scene(%r, "veach-mis", width=160, height=90)
for engine in ("pool", "vote"):
    os.environ["MCPT_TRACE_ENGINE"] = engine
    dev = M.Device(sc, 0)
    dev.set_lens(aperture=0.02, jitter=True)
    pr = dev.progressive(32, seed=1)
    for n in (8, 8, 16):
        pr.step(n, stats=M.Stats())
    pr.close()
    dev.generateImg(8, seed=1, stats=M.Stats())
    dev.close()
print("done")
''' % (ROOT, SCENES)
    out = selfcheck.run(code, timeout=900)
    assert out.returncode == 0 and "done" in out.stdout, out.stderr[-3000:]
    found = selfcheck.kernarg_checks(out.stderr)
    assert len(found) == 8, found
    assert all(a == 0 for a, _ in found) and all(b > 0 for _, b in found), found
