"""GPU: light probes (mcpt_query_sh).  The probe rays are the numpy restatement's (tests/sh_ref.py); a probe is the fold of its rays, bit
for bit -- every sample a ray-kind sample of mcpt_query_radiance, which tests/test_gpu_query_oracle.py holds to the oracle -- under every
seam of the integrator and every path variant; ids key the path, not the position in the list; a constant sky and a known lamp have
their closed forms; the device form is the host form and progressive handles are untouched."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import env_scenes
import light_scenes
import query_ref
import sh_ref
from conftest import SCENES, extra_scene_dir
from test_gpu_query import KNOBS, SEAM_CONFIGS

pytestmark = pytest.mark.gpu

W, H = 64, 36
SCENE_NAMES = ["cornell-box", "veach-mis", "glassroom"]
INT_MAX = 2 ** 31 - 1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _base(name):
    return extra_scene_dir() if name == "glassroom" else SCENES


def _env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _bounds(dev):
    box, _ = dev.bvh_nodes()
    return np.minimum(box[0, :3], box[0, 3:]), np.maximum(box[0, :3], box[0, 3:])


def _inside(dev, rng, n):
    lo, hi = _bounds(dev)
    return lo + (hi - lo) * (0.1 + 0.8 * rng.random((n, 3)))


def _ulps_of(a, b):
    """|a - b| in ulps of b, per entry; where b is 0, a has to be 0"""
    a, b = np.asarray(a), np.asarray(b)
    out = np.where(b == 0.0, np.where(a == 0.0, 0.0, np.inf), np.abs(a - b) / np.spacing(np.abs(np.where(b == 0.0, 1.0, b))))
    return out


def test_probe_rays_are_the_restatement(mcpt):
    """mcpt_query_sh_rays against tests/sh_ref.py within 4 ulps (the bound the hemisphere kind holds for the same sincos, sqrt and normalize
    chain); the origin is the position, bit for bit."""
    sc = mcpt.Scene(SCENES, "cornell-box", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    rng = np.random.default_rng(6)
    n = 4000
    p = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-2, 2, size=(n, 1))
    p[:200] = 0.0
    ids = rng.integers(0, 2 ** 31, size=n).astype(np.int32)
    k = rng.integers(0, 2 ** 31, size=n).astype(np.int32)
    ids[:4], k[:4] = [0, INT_MAX, 0, INT_MAX], [0, 0, INT_MAX, INT_MAX]
    seed = 0x0123456789ABCDEF
    got = dev.sh_probe_rays(p, seed, k, ids=ids)
    want = sh_ref.probe_rays(p, seed, ids, k)
    assert _same(got[:, :3], p)
    u = query_ref.ulps(got, want)
    print("probe rays: max ulps", u.max())
    assert u.max() <= 4, u.max()
    assert np.abs((got[:, 3:] ** 2).sum(axis=1) - 1.0).max() <= 1e-15
    # without ids the list position is the id
    assert _same(dev.sh_probe_rays(p, seed, k), dev.sh_probe_rays(p, seed, k, ids=np.arange(n)))
    # the draw does not depend on the position
    assert _same(dev.sh_probe_rays(p[::-1], seed, k, ids=ids)[:, 3:], got[:, 3:])
    dev.close()
    sc.close()


def _samples(dev, p, ids, seed, base, spp):
    """per k = base .. base + spp - 1: the probe's ray through the ray kind of mcpt_query_radiance -> radiances, directions, hit flags"""
    xs, ds, hs = [], [], []
    for k in range(base, base + spp):
        rays = dev.sh_probe_rays(p, seed, np.full(p.shape[0], k, dtype=np.int32), ids=ids)
        assert _same(rays[:, :3], p)
        x, _, h = dev.radiance(rays, 1, seed, ids=ids, sample_base=k)
        xs.append(x); ds.append(rays[:, 3:]); hs.append(h)
    return xs, ds, hs


def _check_fold(mcpt, dev, p, ids, seed, spp, bases, label):
    """identity (b): sh and hits exactly, stderr as the restated expression gives it, under both pipelines.  Returns the samples of
    the last base."""
    some = False
    for base in bases:
        xs, ds, hs = _samples(dev, p, ids, seed, base, spp)
        want_sh, want_err = sh_ref.fold(xs, ds)
        want_hits = np.sum(hs, axis=0)
        some = some or np.abs(want_sh[:, 1:]).max() > 0
        for flags in (0, mcpt.RENDER_MEGAKERNEL):
            st = mcpt.Stats()
            sh, err, hits = dev.sh_probes(p, spp, seed, ids=ids, sample_base=base, flags=flags, stats=st)
            bad = int((_bits(sh) != _bits(want_sh)).sum())
            u = _ulps_of(err, want_err).max()
            print("%s base %d flags %d: %d of %d coefficients differ, stderr max ulps %g" % (label, base, flags, bad, sh.size, u))
            assert bad == 0, (label, base, flags, bad)
            assert np.array_equal(hits, want_hits), (label, base, flags)
            # the device's fp64 sqrt proved correctly rounded here (0 ulps in every case on the MI355X), so the error is held exactly
            assert _same(err, want_err), (label, base, flags, u)
            assert st.rays_primary == p.shape[0] * spp and st.samples == p.shape[0] * spp
    assert some
    return xs, ds, hs


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_a_probe_is_the_fold_of_its_rays(mcpt, monkeypatch, name):
    _env(monkeypatch, {})
    sc = mcpt.Scene(_base(name), name, width=W, height=H)
    dev = mcpt.Device(sc, 0)
    rng = np.random.default_rng(12)
    p = _inside(dev, rng, 64)
    ids = rng.integers(0, 2 ** 31, size=64).astype(np.int32)
    _check_fold(mcpt, dev, p, ids, 41, 8, (0, 2 ** 31 - 9), name)
    # spp 1: no error estimate
    sh, err, _ = dev.sh_probes(p, 1, 41, ids=ids)
    assert _same(err, np.zeros((64, 9, 3)))
    dev.close()
    sc.close()


@pytest.fixture(scope="module")
def default_probes(mcpt):
    """The list of the seam test and the default device's answers, computed once.  64 x 36 probes of 32 samples: the count of
    test_gpu_query.py's test_several_chunks, whose MCPT_WORKSPACE_GB=0.016 holds about 52 000 paths of this one-light scene, so the 73 728
    samples go in two chunks -- which the test below sees for itself in the number of trace launches."""
    saved = {k: os.environ.pop(k) for k in KNOBS if k in os.environ}
    try:
        sc = mcpt.Scene(SCENES, "cornell-box", width=W, height=H)
        dev = mcpt.Device(sc, 0)
        rng = np.random.default_rng(5)
        p = _inside(dev, rng, W * H)
        ids = rng.permutation(W * H).astype(np.int32)
        st = mcpt.Stats()
        res = dev.sh_probes(p, 32, 3, ids=ids, stats=st)
        dev.close()
        sc.close()
    finally:
        os.environ.update(saved)
    return p, ids, res, st.launches


@pytest.mark.parametrize("config", sorted(SEAM_CONFIGS))
def test_every_seam_gives_the_default_devices_probes(mcpt, monkeypatch, default_probes, config):
    env, mode, flags = SEAM_CONFIGS[config]
    p, ids, want, launches = default_probes
    _env(monkeypatch, env)
    sc = mcpt.Scene(SCENES, "cornell-box", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    if mode:
        dev.set_trace_mode(mcpt.TRACE_REFERENCE)
    st = mcpt.Stats()
    got = dev.sh_probes(p, 32, 3, ids=ids, flags=flags, stats=st)
    assert np.abs(want[0][:, 1:]).max() > 0 and want[2].max() > 0
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), config
    assert st.samples == W * H * 32
    if config == "small-workspace":
        assert st.launches > launches           # more trace launches than the default device's one chunk: at least two chunks
    dev.close()
    sc.close()


@pytest.fixture(scope="module")
def variant_dirs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gpu_sh_scenes")) + os.sep
    light_scenes.write(d, "room12", 12, W, H)
    env_scenes.open_scene(d, "open1", 1, W, H)
    return d


@pytest.mark.parametrize("variant", ["map", "one", "tree"])
def test_path_variants(mcpt, monkeypatch, variant_dirs, variant):
    """identity (b) under a lat-long environment on the open scene, and under the weighted and the tree light pick in the room of lights.
    Under the environment a ray that leaves the scene carries Le of its direction into the fold and is no hit."""
    _env(monkeypatch, {})
    sc = mcpt.Scene(variant_dirs, "open1" if variant == "map" else "room12", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    if variant == "map":
        dev.set_environment(*env_scenes.SKIES["map"])
    else:
        dev.set_light_sampling(variant)
    rng = np.random.default_rng(8)
    p = _inside(dev, rng, 64)
    ids = rng.integers(0, 2 ** 31, size=64).astype(np.int32)
    xs, ds, hs = _check_fold(mcpt, dev, p, ids, 77, 8, (0, 2 ** 31 - 9), variant)
    if variant == "map":
        miss = np.array(hs) == 0
        assert miss.sum() > 64 and (~miss).sum() > 64
        x, d = np.array(xs)[miss], np.array(ds)[miss]
        np.testing.assert_allclose(x, dev.environment_eval(d), rtol=1e-12, atol=0)
        assert x.max() > 0
        hits = dev.sh_probes(p, 8, 77, ids=ids, sample_base=2 ** 31 - 9)[2]
        assert np.array_equal(hits, 8 - miss.sum(axis=0))
    dev.close()
    sc.close()


def test_ids_key_the_probe_not_its_place_in_the_list(mcpt, monkeypatch):
    _env(monkeypatch, {})
    sc = mcpt.Scene(SCENES, "cornell-box", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    rng = np.random.default_rng(3)
    p = _inside(dev, rng, 200)
    ids = rng.integers(0, 2 ** 31, size=200).astype(np.int32)
    perm = rng.permutation(200)
    for flags in (0, mcpt.RENDER_MEGAKERNEL):
        a = dev.sh_probes(p, 8, 9, ids=ids, flags=flags)
        b = dev.sh_probes(p[perm], 8, 9, ids=ids[perm], flags=flags)
        assert a[0].max() > 0
        assert _same(a[0][perm], b[0]) and _same(a[1][perm], b[1]) and np.array_equal(a[2][perm], b[2])
    # a split sample range continues the same sums: a few roundings of terms no larger than the halves' largest coefficient
    s_a = dev.sh_probes(p, 4, 9, ids=ids, sample_base=0)[0]
    s_b = dev.sh_probes(p, 4, 9, ids=ids, sample_base=4)[0]
    np.testing.assert_allclose((s_a * 4 + s_b * 4) / 8, a[0], rtol=0, atol=1e-14 * (np.abs(s_a).max() + np.abs(s_b).max()))
    dev.close()
    sc.close()


def test_constant_sky(mcpt, monkeypatch):
    """One tiny triangle far from the probes under a constant sky c (float32-exact: the texels are float32): no ray hits, coefficient 0 is
    c * 2 sqrt(pi) -- the sum of 64 equal terms c * Y0, so 1e-14 relative has room -- and the others are 0 within 6 of their own standard
    errors."""
    _env(monkeypatch, {})
    v = np.array([[1000.0, 1000.0, 1000.0, 1000.001, 1000.0, 1000.0, 1000.0, 1000.001, 1000.0]])
    vn = np.tile([0.0, 0.0, 1.0], (1, 3))
    rec = np.array([[0.5, 0.5, 0.5, 0.0, 0.0, 0.0, 1.0, 1.0]])
    sc = mcpt.Scene.from_arrays(v, vn, np.array([0], dtype=np.int32), rec, np.zeros(0, dtype=np.int32), np.zeros((0, 3)), [0.0, 0.5, 5.0],
                                [0.0, 0.5, 0.0], [0.0, 1.0, 0.0], 60.0, W, H)
    dev = mcpt.Device(sc, 0)
    c = np.array([0.375, 0.75, 1.25])
    dev.set_environment(tuple(c), 1.0)
    p = np.random.default_rng(2).normal(size=(64, 3))
    for flags in (0, mcpt.RENDER_MEGAKERNEL):
        sh, err, hits = dev.sh_probes(p, 64, 5, flags=flags)
        assert not hits.any()
        assert np.abs(sh[:, 0, :] / (c * (2.0 * math.sqrt(math.pi))) - 1.0).max() <= 1e-14
        z = np.abs(sh[:, 1:, :]) / err[:, 1:, :]
        print("constant sky, flags %d: max |sh_i| / stderr, i = 1..8: %.2f" % (flags, z.max()))
        assert np.all(err[:, 1:, :] > 0) and np.all(np.abs(sh[:, 1:, :]) <= 6.0 * err[:, 1:, :]), z.max()
    dev.close()
    sc.close()


def _solid_angle(x, z, half, h):
    """of the square [-half, half]^2 at height h over the point (x, z): the sum over the four corner rectangles"""
    return sum(math.atan(a * b / (h * math.sqrt(a * a + b * b + h * h))) for a in (half - x, half + x) for b in (half - z, half + z))


def test_known_lamp(mcpt, monkeypatch):
    """test_gpu_query.py's test_known_irradiance scene -- an emitting square of side 2 and radiance 3 at height 1, facing down, over a black
    floor -- seen from probes at height 0.25, h = 0.75 under it: sh0 = 3 Y0 Omega with Omega the square's solid angle, and the
    y-coefficient, the integral of 3 C1 cos(theta) over it, 3 C1 pi F with F the form factor to a horizontal element.  6 sigma of the
    estimator's own error; the run is deterministic."""
    _env(monkeypatch, {})
    def quad(x0, x1, z0, z1, y, up):
        a, b, c, d = [x0, y, z0], [x1, y, z0], [x1, y, z1], [x0, y, z1]
        return [a + c + b, a + d + c] if up else [a + b + c, a + c + d]
    v = np.array(quad(-1, 1, -1, 1, 1.0, False) + quad(-6, 6, -6, 6, 0.0, True), dtype=np.float64)
    vn = np.concatenate([np.tile([0.0, -1.0, 0.0], (2, 3)), np.tile([0.0, 1.0, 0.0], (2, 3))])
    rec = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0]])
    sc = mcpt.Scene.from_arrays(v, vn, np.array([0, 0, 1, 1], dtype=np.int32), rec, [0], [[3.0, 3.0, 3.0]], [0.0, 0.5, 5.0], [0.0, 0.5, 0.0],
                                [0.0, 1.0, 0.0], 60.0, W, H)
    dev = mcpt.Device(sc, 0)
    xz = np.array([[0.0, 0.0], [1.0, 1.0], [0.5, 0.0], [1.0, 0.0], [0.5, 0.5], [-1.0, -1.0], [0.25, -0.75], [-0.5, 0.5]])
    p = np.stack([xz[:, 0], np.full(8, 0.25), xz[:, 1]], axis=1)
    h = 0.75
    omega = np.array([_solid_angle(x, z, 1.0, h) for x, z in xz])
    F = np.array([query_ref.square_form_factor(x, z, 1.0, h) for x, z in xz])
    assert abs(omega[0] - 4.0 * math.atan(1.0 / (h * math.sqrt(2.0 + h * h)))) < 1e-15 and abs(F[1] - F[5]) < 1e-15
    want0, want1 = 3.0 * sh_ref.C0 * omega, 3.0 * sh_ref.C1 * math.pi * F
    for flags in (0, mcpt.RENDER_MEGAKERNEL):
        sh, err, hits = dev.sh_probes(p, 4096, 2024, flags=flags)
        assert np.all(err[:, :2] > 0) and np.all(err < 0.1)
        z0, z1 = np.abs(sh[:, 0, 0] - want0) / err[:, 0, 0], np.abs(sh[:, 1, 0] - want1) / err[:, 1, 0]
        print("known lamp, flags %d: |sh0 - want| / stderr =" % flags, np.round(z0, 2), " |sh1 - want| / stderr =", np.round(z1, 2))
        assert np.all(np.abs(sh[:, 0, :] - want0[:, None]) <= 6.0 * err[:, 0, :]), z0
        assert np.all(np.abs(sh[:, 1, :] - want1[:, None]) <= 6.0 * err[:, 1, :]), z1
        odd = [2, 3, 4, 5, 7]
        zc = np.abs(sh[0, odd, 0]) / err[0, odd, 0]
        print("   the centred probe's coefficients 2, 3, 4, 5, 7 / stderr =", np.round(zc, 2))
        assert np.all(np.abs(sh[0, odd, :]) <= 6.0 * err[0, odd, :]), zc
        assert _same(sh[:, :, 0], sh[:, :, 1]) and _same(sh[:, :, 0], sh[:, :, 2]) and _same(err[:, :, 0], err[:, :, 2])
        again = dev.sh_probes(p, 4096, 2024, flags=flags)
        assert _same(again[0], sh) and _same(again[1], err) and np.array_equal(again[2], hits)
    dev.close()
    sc.close()


def test_device_form_and_handles(mcpt, monkeypatch):
    """The device form on the caller's buffers and stream is the host form, bit for bit; n == 0 is MCPT_OK; a live progressive handle's
    image does not change under probe calls."""
    import hip_rt
    _env(monkeypatch, {})
    sc = mcpt.Scene(SCENES, "veach-mis", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    rng = np.random.default_rng(14)
    n, spp, seed = 300, 6, 21
    p = np.ascontiguousarray(_inside(dev, rng, n))
    ids = rng.integers(0, 2 ** 31, size=n).astype(np.int32)
    want = dev.sh_probes(p, spp, seed, ids=ids, sample_base=3)
    L = mcpt.lib()
    hip = hip_rt.hip()
    d_p, d_ids = hip_rt.DeviceBuffer(p.nbytes), hip_rt.DeviceBuffer(ids.nbytes)
    d_sh, d_err, d_hits = hip_rt.DeviceBuffer(n * 27 * 8), hip_rt.DeviceBuffer(n * 27 * 8), hip_rt.DeviceBuffer(n * 4)
    hip_rt.check(hip.hipMemcpy(d_p.ptr, p.ctypes.data_as(C.c_void_p), p.nbytes, 1))
    hip_rt.check(hip.hipMemcpy(d_ids.ptr, ids.ctypes.data_as(C.c_void_p), ids.nbytes, 1))
    st = hip_rt.Stream()
    sp = mcpt.ShParams(spp, 3, seed, 0, (C.c_int32 * 3)(0, 0, 0))
    for stats in (None, mcpt.Stats()):
        rc = L.mcpt_query_sh_device(dev._h, d_p.ptr, d_ids.ptr, n, C.byref(sp), d_sh.ptr, d_err.ptr, d_hits.ptr,
                                    C.byref(stats) if stats is not None else None, st.h)
        assert rc == 0, mcpt.lib().mcpt_last_error()
        sh, err, hits = np.zeros((n, 9, 3)), np.zeros((n, 9, 3)), np.zeros(n, dtype=np.int32)
        d_sh.to_host_async(sh, st.h); d_err.to_host_async(err, st.h); d_hits.to_host_async(hits, st.h)
        st.synchronize()
        assert _same(sh, want[0]) and _same(err, want[1]) and np.array_equal(hits, want[2])
        if stats is not None:
            assert stats.samples == n * spp and stats.rays_primary == n * spp
    # stderr and hits may be left out; ids too (the position is the id)
    assert L.mcpt_query_sh_device(dev._h, d_p.ptr, None, n, C.byref(sp), d_sh.ptr, None, None, None, st.h) == 0
    sh = np.zeros((n, 9, 3))
    d_sh.to_host_async(sh, st.h)
    st.synchronize()
    assert _same(sh, dev.sh_probes(p, spp, seed, sample_base=3)[0])
    # n == 0: nothing is looked at or launched
    assert L.mcpt_query_sh_device(dev._h, None, None, 0, C.byref(sp), None, None, None, None, st.h) == 0
    assert L.mcpt_query_sh(dev._h, None, None, 0, C.byref(sp), None, None, None, None) == 0
    e = dev.sh_probes(np.zeros((0, 3)), 4)
    assert e[0].shape == (0, 9, 3) and e[2].shape == (0,)
    for b in (d_p, d_ids, d_sh, d_err, d_hits):
        b.free()
    st.destroy()
    # progressive handles
    runs = []
    for interrupted in (False, True):
        pr = dev.progressive(16, seed=4)
        pr.step(4)
        if interrupted:
            dev.sh_probes(p, 3, seed=4)
            dev.sh_probes(p[:99], 2, seed=9, flags=mcpt.RENDER_MEGAKERNEL, stats=mcpt.Stats())
        pr.step(4)
        runs.append((pr.image(), pr.stderr()))
        pr.close()
    assert _same(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1])
    dev.close()
    sc.close()
