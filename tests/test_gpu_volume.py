"""GPU: irradiance volumes (mcpt_bake_volume*, mcpt_volume_irradiance*).  The lookup kernel is the host form and the numpy restatement
(tests/volume_ref.py) bit for bit on the CPU test's inputs; a bake is sh_probes() of the grid's own points bit for bit, under both
pipelines, every seam of the integrator and an environment; bake and lookup chain on one stream without the host; a lightmap's texel list
goes into the lookup unchanged; progressive handles and the bake's workspace are left as they were."""
import ctypes as C
import os

import numpy as np
import pytest

import env_scenes
import volume_cases as VC
import volume_ref
from conftest import SCENES, extra_scene_dir
from test_gpu_query import KNOBS, SEAM_CONFIGS

pytestmark = pytest.mark.gpu

W, H = 64, 36
COUNTS = sorted(VC.GRIDS)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _bounds(dev):
    box, _ = dev.bvh_nodes()
    return np.minimum(box[0, :3], box[0, 3:]), np.maximum(box[0, :3], box[0, 3:])


def _inside_grid(mcpt, dev, counts, clamp_zero=False):
    """a grid over the middle 80 % of the scene's bounds, as test_gpu_sh.py's _inside places its probes"""
    lo, hi = _bounds(dev)
    c = np.array(counts)
    spacing = 0.8 * (hi - lo) / np.maximum(c - 1, 1)
    origin = lo + 0.1 * (hi - lo) if (c > 1).all() else lo + (hi - lo) * np.where(c > 1, 0.1, 0.37)
    return mcpt.volume_grid(origin, spacing, counts, clamp_zero=clamp_zero)


@pytest.fixture(scope="module")
def cornell(mcpt):
    saved = {k: os.environ.pop(k) for k in KNOBS if k in os.environ}
    try:
        sc = mcpt.Scene(SCENES, "cornell-box", width=W, height=H)
        dev = mcpt.Device(sc, 0)
    finally:
        os.environ.update(saved)
    yield dev
    dev.close()
    sc.close()


# ---- lookup

@pytest.fixture(scope="module")
def lookup_cases():
    """per grid: coefficients, mask, receivers and the restatement's answers for (masked, clamp), computed once"""
    out = {}
    for counts in COUNTS:
        sh, valid = VC.coefficients(counts), VC.mask(counts)
        x, b = VC.receivers(counts)
        origin, spacing = VC.GRIDS[counts]
        want = {(m, c): volume_ref.irradiance(origin, spacing, counts, sh, x, b, valid if m else None, c) for m in (False, True) for c in (False, True)}
        out[counts] = (sh, valid, x, b, want)
    return out


@pytest.mark.parametrize("counts", COUNTS)
def test_lookup_is_the_host_form_and_the_restatement(mcpt, cornell, lookup_cases, counts):
    """fp64 add, multiply, divide, square root and floor only: equality is asserted, as for the probes' and the lightmaps' helpers"""
    sh, valid, x, b, want = lookup_cases[counts]
    for masked in (False, True):
        for clamp in (False, True):
            g = VC.grid(mcpt, counts, clamp_zero=clamp)
            v = valid if masked else None
            for n in (1, 63, 64, 65, VC.N):
                # n receivers of the list from position 7 n on, around its end (n = 4001: the whole list, edge cases and all)
                xs, bs = np.roll(x, -7 * n, axis=0)[:n], np.roll(b, -7 * n, axis=0)[:n]
                E, corners = cornell.volume_irradiance(g, sh, xs, bs, valid=v)
                hE, hc = mcpt.volume_irradiance_host(g, sh, xs, bs, valid=v)
                wE, wc = (np.roll(a, -7 * n, axis=0)[:n] for a in want[(masked, clamp)])
                bad = int((_bits(E) != _bits(wE)).sum())
                if n == VC.N:
                    print("%r masked %d clamp %d: %d of %d values differ from the restatement" % (counts, masked, clamp, bad, E.size))
                assert bad == 0, (counts, masked, clamp, n, bad)
                assert _same(E, hE) and np.array_equal(corners, hc) and np.array_equal(corners, wc), (counts, masked, clamp, n)
    assert np.abs(want[(False, False)][0]).max() > 0


# ---- bake

def _check_bake(mcpt, dev, g, spp, seed, bases=(0, 2 ** 31 - 9), flagses=None):
    p = mcpt.volume_points(g)
    shape = (g.nz, g.ny, g.nx)
    some = False
    for base in bases:
        for flags in flagses if flagses is not None else (0, mcpt.RENDER_MEGAKERNEL):
            st = mcpt.Stats()
            sh, err, hits = dev.bake_volume(g, spp, seed=seed, sample_base=base, flags=flags, stats=st)
            want = dev.sh_probes(p, spp, seed=seed, sample_base=base, flags=flags)
            assert sh.shape == shape + (9, 3) and err.shape == shape + (9, 3) and hits.shape == shape
            assert _same(sh.reshape(-1, 9, 3), want[0]) and _same(err.reshape(-1, 9, 3), want[1]), (base, flags)
            assert np.array_equal(hits.reshape(-1), want[2]), (base, flags)
            assert st.rays_primary == p.shape[0] * spp and st.samples == p.shape[0] * spp
            some = some or np.abs(sh[..., 1:, :]).max() > 0
    assert some
    return sh


@pytest.mark.parametrize("counts", [(5, 4, 3), (1, 1, 1), (1, 7, 1)])
def test_a_bake_is_the_probe_query_of_the_grids_points(mcpt, cornell, counts):
    _check_bake(mcpt, cornell, _inside_grid(mcpt, cornell, counts), 8, 41)


def test_a_bake_under_an_environment(mcpt, monkeypatch):
    _env(monkeypatch, {})
    sc = mcpt.Scene(extra_scene_dir(), "glassroom", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    dev.set_environment(*env_scenes.SKIES["map"])
    _check_bake(mcpt, dev, _inside_grid(mcpt, dev, (5, 4, 3)), 8, 77)
    dev.close()
    sc.close()


SEAM_COUNTS = (16, 12, 12)          # 2304 probes of 32 samples: test_gpu_sh.py's count, two chunks under MCPT_WORKSPACE_GB=0.016


@pytest.fixture(scope="module")
def default_bake(mcpt, cornell):
    g = _inside_grid(mcpt, cornell, SEAM_COUNTS)
    st = mcpt.Stats()
    res = cornell.sh_probes(mcpt.volume_points(g), 32, 3, stats=st)
    return res, st.launches


@pytest.mark.parametrize("config", sorted(SEAM_CONFIGS))
def test_every_seam_gives_the_default_devices_bake(mcpt, monkeypatch, default_bake, config):
    env, mode, flags = SEAM_CONFIGS[config]
    want, launches = default_bake
    _env(monkeypatch, env)
    sc = mcpt.Scene(SCENES, "cornell-box", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    if mode:
        dev.set_trace_mode(mcpt.TRACE_REFERENCE)
    st = mcpt.Stats()
    got = dev.bake_volume(_inside_grid(mcpt, dev, SEAM_COUNTS), 32, seed=3, flags=flags, stats=st)
    assert np.abs(want[0][:, 1:]).max() > 0 and want[2].max() > 0
    for a, b in zip(got, want):
        assert np.array_equal(a.reshape(b.shape).view(np.uint8), b.view(np.uint8)), config
    assert st.samples == 2304 * 32
    if config == "small-workspace":
        assert st.launches > launches           # more trace launches than the default device's one chunk: at least two chunks
    dev.close()
    sc.close()


# ---- the device forms

def _upload(hip_rt, a):
    a = np.ascontiguousarray(a)
    b = hip_rt.DeviceBuffer(a.nbytes)
    hip_rt.check(hip_rt.hip().hipMemcpy(b.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes, 1))
    return b


def test_bake_and_lookup_chain_on_one_stream(mcpt, cornell):
    """mcpt_bake_volume_device on a side stream, its coefficients straight into mcpt_volume_irradiance_device on the same stream, no host
    wait in between; the receivers are the probes' own points under the six axis normals, so the answer is mcpt_sh_irradiance of the
    host-form bake, bit for bit.  Then a second bake right behind a device-form bake: the workspace's event keeps their points apart."""
    import hip_rt
    dev, L = cornell, mcpt.lib()
    g = _inside_grid(mcpt, dev, (5, 4, 3), clamp_zero=False)
    n, spp, seed = 60, 8, 19
    sh, err, hits = dev.bake_volume(g, spp, seed=seed)
    p = mcpt.volume_points(g)
    q6 = np.concatenate([np.repeat(p, 6, axis=0), np.tile(VC.AXES, (n, 1))], axis=1)
    want = mcpt.sh_irradiance(np.repeat(sh.reshape(n, 9, 3), 6, axis=0), q6[:, 3:])
    d_sh, d_err, d_hits = hip_rt.DeviceBuffer(n * 27 * 8), hip_rt.DeviceBuffer(n * 27 * 8), hip_rt.DeviceBuffer(n * 4)
    d_q, d_e, d_c = _upload(hip_rt, q6), hip_rt.DeviceBuffer(n * 6 * 3 * 8), hip_rt.DeviceBuffer(n * 6 * 4)
    st = hip_rt.Stream()
    sp = mcpt.ShParams(spp, 0, seed, 0, (C.c_int32 * 3)(0, 0, 0))
    assert L.mcpt_bake_volume_device(dev._h, C.byref(g), C.byref(sp), d_sh.ptr, d_err.ptr, d_hits.ptr, None, st.h) == 0, L.mcpt_last_error()
    assert L.mcpt_volume_irradiance_device(dev._h, C.byref(g), d_sh.ptr, None, d_q.ptr, n * 6, d_e.ptr, d_c.ptr, st.h) == 0, L.mcpt_last_error()
    E, corners, sh2, err2, hits2 = np.zeros((n * 6, 3)), np.zeros(n * 6, dtype=np.int32), np.zeros((n, 9, 3)), np.zeros((n, 9, 3)), np.zeros(n, dtype=np.int32)
    d_e.to_host_async(E, st.h); d_c.to_host_async(corners, st.h)
    d_sh.to_host_async(sh2, st.h); d_err.to_host_async(err2, st.h); d_hits.to_host_async(hits2, st.h)
    st.synchronize()
    assert _same(sh2, sh.reshape(n, 9, 3)) and _same(err2, err.reshape(n, 9, 3)) and np.array_equal(hits2, hits.reshape(-1))
    assert _same(E, want) and np.array_equal(corners, np.ones(n * 6)) and np.abs(E).max() > 0
    # a device-form bake of one grid, and at once a bake of another (larger: the list is reallocated) -- both give their own bits
    g2 = _inside_grid(mcpt, dev, (6, 5, 4))
    want2 = dev.sh_probes(mcpt.volume_points(g2), spp, seed=seed)
    stats = mcpt.Stats()
    assert L.mcpt_bake_volume_device(dev._h, C.byref(g), C.byref(sp), d_sh.ptr, None, None, None, st.h) == 0
    got2 = dev.bake_volume(g2, spp, seed=seed, stats=stats)
    sh3 = np.zeros((n, 9, 3))
    d_sh.to_host_async(sh3, st.h)
    st.synchronize()
    assert _same(sh3, sh.reshape(n, 9, 3))
    assert _same(got2[0].reshape(-1, 9, 3), want2[0]) and _same(got2[1].reshape(-1, 9, 3), want2[1]) and np.array_equal(got2[2].reshape(-1), want2[2])
    assert stats.samples == 120 * spp
    # n == 0: nothing is looked at or launched
    assert L.mcpt_volume_irradiance_device(dev._h, C.byref(g), None, None, None, 0, None, None, st.h) == 0
    assert L.mcpt_volume_irradiance(dev._h, C.byref(g), None, None, None, 0, None, None) == 0
    E0, c0 = dev.volume_irradiance(g, sh, np.zeros((0, 3)), np.zeros((0, 3)))
    assert E0.shape == (0, 3) and c0.shape == (0,)
    for b in (d_sh, d_err, d_hits, d_q, d_e, d_c):
        b.free()
    st.destroy()


def test_a_lightmaps_texel_list_goes_in_unchanged(mcpt, monkeypatch):
    _env(monkeypatch, {})
    sc = mcpt.Scene(extra_scene_dir(), "glassroom", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    owner, texels, q6 = dev.lightmap_texels(64, 64)
    assert texels.size > 100
    g = _inside_grid(mcpt, dev, (5, 4, 3), clamp_zero=True)
    sh = dev.bake_volume(g, 8, seed=5)[0]
    valid = VC.mask((5, 4, 3))
    for v in (None, valid):
        E, corners = dev.volume_irradiance(g, sh, q6[:, :3], q6[:, 3:], valid=v)
        hE, hc = mcpt.volume_irradiance_host(g, sh, q6[:, :3], q6[:, 3:], valid=v)
        assert _same(E, hE) and np.array_equal(corners, hc)
        assert E.max() > 0 and E.min() >= 0.0 and not np.signbit(E).any()
    dev.close()
    sc.close()


def test_progressive_handles_do_not_notice(mcpt, cornell):
    dev = cornell
    g = _inside_grid(mcpt, dev, (5, 4, 3))
    sh = VC.coefficients((5, 4, 3))
    x, b = VC.receivers((5, 4, 3))
    runs = []
    for interrupted in (False, True):
        pr = dev.progressive(16, seed=4)
        pr.step(4)
        if interrupted:
            dev.bake_volume(g, 3, seed=4)
            dev.bake_volume(g, 2, seed=9, flags=mcpt.RENDER_MEGAKERNEL, stats=mcpt.Stats())
            dev.volume_irradiance(g, sh, x, b)
        pr.step(4)
        runs.append((pr.image(), pr.stderr()))
        pr.close()
    assert _same(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1])
