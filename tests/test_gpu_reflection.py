"""GPU: reflection probes (mcpt_bake_reflection*, mcpt_reflection_rays, mcpt_reflection_prefilter*, mcpt_reflection_lookup*).  The rays of
a bake's entries are the numpy restatement's (tests/reflection_ref.py) bit for bit; a bake is radiance() with spp = 1 over its own rays,
folded per texel, bit for bit under both pipelines, both trace modes and engines, an environment and every chunking; the prefilter and
lookup kernels are the host forms bit for bit; bake, prefilter and lookup chain on one stream without the host; progressive handles,
volume bakes and baked frames are left as they were."""
import ctypes as C
import os

import numpy as np
import pytest

import env_scenes
import reflection_ref as RR
from conftest import SCENES, extra_scene_dir
from test_gpu_query import KNOBS, SEAM_CONFIGS

pytestmark = pytest.mark.gpu

W, H = 64, 36
SEED = 0x1234567887654321
# k_reflection_prefilter stages the source in tiles of 256 records and works in workgroups of 256 output texels: sources of 17^2 = 289,
# 23^2 = 529 and 32^2 = 1024 texels end inside, past and on a tile; a level of 17^2 = 289 texels ends inside its second workgroup
TILE = 256
# (source size, [(level size, exponent), ...]): source sizes 1, 5, 17, 23, 32; level sizes 1, 5, 16, 17; exponents 0, 1, 64, 65535
PREFILTER_CASES = [(1, [(5, 1), (1, 0)]),
                   (5, [(17, 65535), (16, 64), (5, 1), (1, 0)]),
                   (17, [(16, 64), (5, 1)]),
                   (23, [(17, 0)]),
                   (32, [(17, 65535), (1, 64), (16, 0)])]
LOOKUP_CASES = [(5, [(17, 65535), (16, 1000), (5, 64), (4, 7), (1, 3), (5, 2), (16, 1), (17, 0)]), (2, [(5, 65535), (4, 0)]), (1, [(4, 1)])]
NS = (1, 63, 64, 65, 4001)
BAKE_CONFIGS = ["pool", "vote", "reference-walk", "megakernel", "finish-0"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _probes(dev, n):
    """n points in free space: inside the middle of the scene's bounds"""
    box, _ = dev.bvh_nodes()
    lo, hi = np.minimum(box[0, :3], box[0, 3:]), np.maximum(box[0, :3], box[0, 3:])
    f = np.array([[0.5, 0.5, 0.5], [0.3, 0.6, 0.4], [0.7, 0.35, 0.62], [0.45, 0.7, 0.3]])[:n]
    return lo + (hi - lo) * f


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


# ---- rays

def test_rays_are_the_restatement_bit_for_bit(mcpt, cornell):
    """origins and ids exactly; the directions through camera_uniforms and the decode, which is add, multiply, divide and sqrt only"""
    p = _probes(cornell, 3)
    for R in (1, 2, 3, 5, 16):
        for S in (1, 3):
            for id_base in (None, np.array([700, 5, 2 ** 31 - R * R * S], dtype=np.int64)):      # (the last: the largest base there is)
                for base in (0, 7):
                    e = RR.entries_of(3, R, S)
                    rays, ids = cornell.reflection_rays(p, R, S, e, seed=SEED, sample_base=base, id_base=id_base)
                    want, wids = RR.rays(p, R, S, e, SEED, base, id_base)
                    assert np.array_equal(ids, wids) and _same(rays[:, :3], want[:, :3]), (R, S, base)
                    assert _same(rays[:, 3:], want[:, 3:]), (R, S, base, int((_bits(rays[:, 3:]) != _bits(want[:, 3:])).sum()))
                    assert np.abs((rays[:, 3:] ** 2).sum(axis=1) - 1.0).max() <= 1e-15
                    # every ray lies in its own texel, and a listed entry is the same ray wherever it stands in the list
                    st = RR.encode(rays[:, 3:])
                    b = (e % (R * R * S)) // S
                    assert np.array_equal(np.floor(st[:, 0] * R).astype(int), b % R) and np.array_equal(np.floor(st[:, 1] * R).astype(int), b // R)
                    pick = np.array([e[-1], e[0], e[len(e) // 2]])
                    r2, i2 = cornell.reflection_rays(p, R, S, pick, seed=SEED, sample_base=base, id_base=id_base)
                    assert _same(r2, rays[pick]) and np.array_equal(i2, ids[pick])
    # the samples of a texel differ, and so do the same entries under another sample_base
    rays, _ = cornell.reflection_rays(p, 2, 3, RR.entries_of(3, 2, 3), seed=SEED)
    assert len({tuple(r) for r in rays[:, 3:].tolist()}) == rays.shape[0]
    assert not _same(rays, cornell.reflection_rays(p, 2, 3, RR.entries_of(3, 2, 3), seed=SEED, sample_base=7)[0])


# ---- bake

def _check_bake(mcpt, dev, p, R, S, seed, base=0, id_base=None, ws=0, flags=0):
    """bake_reflection_probes against radiance(spp = 1) of its own rays, folded by the restatement"""
    n = p.shape[0]
    st = mcpt.Stats()
    rad, err, hits = dev.bake_reflection_probes(p, R, S, seed=seed, sample_base=base, id_base=id_base, workspace_rays=ws, flags=flags, stats=st)
    rays, ids = dev.reflection_rays(p, R, S, RR.entries_of(n, R, S), seed=seed, sample_base=base, id_base=id_base)
    qs = mcpt.Stats()
    x, xe, xh = dev.radiance(rays, 1, seed, ids=ids, sample_base=base, flags=flags, stats=qs)
    assert not xe.any()
    mean, se, h = RR.fold(x.reshape(n * R * R, S, 3), xh.reshape(n * R * R, S))
    what = (n, R, S, base, ws, flags)
    assert _same(rad.reshape(-1, 3), mean), (what, int((_bits(rad.reshape(-1, 3)) != _bits(mean)).sum()))
    assert _same(err.reshape(-1, 3), se) and np.array_equal(hits.reshape(-1), h), what
    assert st.rays_primary == st.samples == n * R * R * S, what
    assert (st.rays_shadow, st.rays_bounce, st.shade_calls) == (qs.rays_shadow, qs.rays_bounce, qs.shade_calls), what
    return rad, hits


@pytest.mark.parametrize("config", BAKE_CONFIGS)
def test_a_bake_is_the_fold_of_a_ray_query(mcpt, monkeypatch, config):
    """1 and 3 probes, R in {1, 5, 16}, S in {1, 2, 64}; one chunk, several, and one per texel.  The bakes follow one another on one
    device: the workspace grows and every bake waits for the event behind the one before."""
    env, mode, flags = SEAM_CONFIGS[config]
    _env(monkeypatch, env)
    sc = mcpt.Scene(SCENES, "cornell-box", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    if mode:
        dev.set_trace_mode(mcpt.TRACE_REFERENCE)
    p = _probes(dev, 3)
    lit = 0
    for n, R, S, base, ws in ((1, 1, 64, 0, 0), (3, 5, 2, 7, 0), (3, 5, 2, 7, 1), (3, 5, 2, 7, 23), (1, 16, 1, 0, 100), (3, 16, 1, 0, 0), (1, 5, 64, 3, 640)):
        rad, hits = _check_bake(mcpt, dev, p[:n], R, S, 11, base=base, ws=ws, flags=flags,
                                id_base=None if ws else np.arange(n, dtype=np.int64) * 100000 + 17)
        lit += int((rad > 0).any(axis=2).sum())
        assert hits.max() <= S and hits.min() >= 0
    assert lit > 100
    dev.close()
    sc.close()


def test_chunking_does_not_change_a_bake(mcpt, cornell):
    p = _probes(cornell, 3)
    want = cornell.bake_reflection_probes(p, 5, 3, seed=SEED, sample_base=2)
    for ws in (1, 3, 4, 74, 75 * 3, 10 ** 12):
        st = mcpt.Stats()
        got = cornell.bake_reflection_probes(p, 5, 3, seed=SEED, sample_base=2, workspace_rays=ws, stats=st)
        assert all(_same(a, b) if a.dtype == np.float64 else np.array_equal(a, b) for a, b in zip(got, want)), ws
        assert st.rays_primary == 3 * 25 * 3
    # the ids key the paths: another id_base, another map; the same ids given explicitly, the same map
    same = cornell.bake_reflection_probes(p, 5, 3, seed=SEED, sample_base=2, id_base=np.arange(3) * 75)
    other = cornell.bake_reflection_probes(p, 5, 3, seed=SEED, sample_base=2, id_base=np.arange(3) * 75 + 1)
    assert _same(same[0], want[0]) and not _same(other[0], want[0])
    assert cornell.bake_reflection_probes(np.zeros((0, 3)), 5, 3)[0].shape == (0, 25, 3)


def test_a_bake_under_an_environment(mcpt, monkeypatch):
    _env(monkeypatch, {})
    sc = mcpt.Scene(extra_scene_dir(), "glassroom", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    dev.set_environment(*env_scenes.SKIES["map"])
    rad, hits = _check_bake(mcpt, dev, _probes(dev, 2), 5, 4, 77, ws=30)
    assert (rad > 0).any()
    dev.close()
    sc.close()


# ---- prefilter

@pytest.mark.parametrize("case", range(len(PREFILTER_CASES)))
def test_prefilter_is_the_host_form_bit_for_bit(mcpt, cornell, case):
    R, levels = PREFILTER_CASES[case]
    assert TILE == 256
    for n in (1, 3):
        L = RR.source_map(n, R)
        c, got = cornell.prefilter_reflection(L, R, levels)
        want = mcpt.reflection_prefilter_host(c, L)
        assert got.shape == (n, RR.chain_texels(levels), 3)
        assert _same(got, want), (R, n, int((_bits(got) != _bits(want)).sum()))
    if case == 0:
        assert (~(got != 0).any(axis=2)).sum() > 0                  # the empty lobes of a 1 x 1 source: +0.0 from the kernel too


def test_prefilter_past_one_launch_of_probes(mcpt, cornell):
    """launch_reflection_prefilter cuts the probes into launches of 65 535 (blockIdx.y's limit) and offsets both pointers for the next
    launch: 65 537 probes of a 1 x 1 source under levels of 2 x 2 and 1 x 1 texels -- 5 chain texels a probe, 7.9 MB -- leave two probes to
    the second launch.  Every probe has a radiance of its own, so a probe read or written at another probe's place shows."""
    n, R, levels = 65537, 1, [(2, 1), (1, 0)]
    i = np.arange(n, dtype=np.float64)
    L = np.stack([0.25 + i, 0.5 + 3.0 * i, 1.0 / (1.0 + i)], axis=1).reshape(n, 1, 3)
    assert np.unique(L.reshape(n, 3), axis=0).shape[0] == n
    c, got = cornell.prefilter_reflection(L, R, levels)
    want = mcpt.reflection_prefilter_host(c, L)
    assert got.shape == want.shape == (n, 5, 3) and got.nbytes < 8 * 2 ** 20
    assert _same(got, want), int((_bits(got) != _bits(want)).sum())
    for p in (n - 2, n - 1, 65534):                                 # the second launch's two probes, and the first launch's last
        assert _same(got[p], want[p]) and (got[p, 4] > 0).all(), p
    assert not _same(got[n - 1], got[1]) and not _same(got[n - 2], got[0])      # (not the first launch's probes once more)
    assert len({tuple(r) for r in got[:, 4].tolist()}) == n                      # every probe's 1 x 1 level is its own


# ---- lookup

@pytest.mark.parametrize("case", range(len(LOOKUP_CASES)))
def test_lookup_is_the_host_form_bit_for_bit(mcpt, cornell, case):
    R, levels = LOOKUP_CASES[case]
    c = mcpt.reflection_chain(R, levels)
    chain = mcpt.reflection_prefilter_host(c, RR.source_map(3, R))
    d, x = RR.receivers(levels)
    probe = (np.arange(d.shape[0]) * 7 % 3).astype(np.int32)
    assert d.shape[0] >= 4001
    for n in NS + (d.shape[0],):
        ds, xs, ps = (np.roll(a, -7 * n, axis=0)[:n] for a in (d, x, probe))
        got = cornell.reflection_lookup(c, chain, ps, ds, xs)
        want = mcpt.reflection_lookup_host(c, chain, ps, ds, xs)
        assert _same(got, want), (n, int((_bits(got) != _bits(want)).sum()))


# ---- plumbing

def _upload(hip_rt, a):
    a = np.ascontiguousarray(a)
    b = hip_rt.DeviceBuffer(max(a.nbytes, 8))
    hip_rt.check(hip_rt.hip().hipMemcpy(b.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes, 1))
    return b


def test_bake_prefilter_and_lookup_chain_on_one_stream(mcpt, cornell):
    """the three _device forms on a side stream, each reading what the one before wrote, no host wait in between: the host-pointer
    forms' answer, bit for bit.  Receivers whose probe index is out of range get +0.0."""
    import hip_rt
    dev = cornell
    n, R, S = 2, 16, 16
    levels = [(16, 256), (8, 16), (4, 1)]
    p = _probes(dev, n)
    d, x = RR.receivers(levels, seed=5, n_random=300)
    m = d.shape[0]
    probe = (np.arange(m) % n).astype(np.int32)
    rad, err, hits = dev.bake_reflection_probes(p, R, S, seed=21)
    c, chain = dev.prefilter_reflection(rad, R, levels)
    want = dev.reflection_lookup(c, chain, probe, d, x)
    assert (want > 0).any()
    wild = probe.copy()
    wild[::5], wild[1::5], wild[2::25], wild[3::25] = -1, n, 2 ** 31 - 1, -2 ** 31
    T = c.num_texels
    d_p, d_probe, d_d, d_x = _upload(hip_rt, p), _upload(hip_rt, wild), _upload(hip_rt, d), _upload(hip_rt, x)
    d_rad, d_err, d_hits = hip_rt.DeviceBuffer(n * R * R * 24), hip_rt.DeviceBuffer(n * R * R * 24), hip_rt.DeviceBuffer(n * R * R * 4)
    d_chain, d_out = hip_rt.DeviceBuffer(n * T * 24), hip_rt.DeviceBuffer(m * 24)
    st = hip_rt.Stream()
    dev.bake_reflection_probes_device(d_p.ptr, n, d_rad.ptr, R, S, seed=21, workspace_rays=1000, d_stderr_ptr=d_err.ptr, d_hits_ptr=d_hits.ptr, stream=st.h)
    dev.prefilter_reflection_device(c, d_rad.ptr, n, d_chain.ptr, stream=st.h)
    dev.reflection_lookup_device(c, d_chain.ptr, n, d_probe.ptr, d_d.ptr, d_x.ptr, m, d_out.ptr, stream=st.h)
    # at once, on the library's stream: a larger bake (the workspace grows) -- it waits for the call above to leave the workspace
    big = dev.bake_reflection_probes(p, R, S + 3, seed=21)
    out, g_rad, g_err, g_hits, g_chain = np.zeros((m, 3)), np.zeros_like(rad), np.zeros_like(err), np.zeros_like(hits), np.zeros_like(chain)
    d_out.to_host_async(out, st.h); d_rad.to_host_async(g_rad, st.h); d_err.to_host_async(g_err, st.h); d_hits.to_host_async(g_hits, st.h)
    d_chain.to_host_async(g_chain, st.h)
    st.synchronize()
    assert _same(g_rad, rad) and _same(g_err, err) and np.array_equal(g_hits, hits) and _same(g_chain, chain)
    inside = (wild >= 0) & (wild < n)
    assert _same(out[inside], want[inside]) and not _bits(out[~inside]).any() and (~inside).sum() > 10
    assert all(_same(a, b) if a.dtype == np.float64 else np.array_equal(a, b) for a, b in zip(big, dev.bake_reflection_probes(p, R, S + 3, seed=21)))
    for b in (d_p, d_probe, d_d, d_x, d_rad, d_err, d_hits, d_chain, d_out):
        b.free()
    st.destroy()


def test_existing_state_does_not_notice(mcpt, cornell):
    """a progressive handle stepped before and after a bake gives the frame it gave; bake_volume and render_baked give the same bits
    around a reflection bake"""
    dev = cornell
    p = _probes(dev, 2)
    box, _ = dev.bvh_nodes()
    lo, hi = np.minimum(box[0, :3], box[0, 3:]), np.maximum(box[0, :3], box[0, 3:])
    g = mcpt.volume_grid(lo + 0.1 * (hi - lo), 0.8 * (hi - lo) / 2, (3, 3, 3))
    runs = []
    for interrupted in (False, True):
        pr = dev.progressive(16, seed=4)
        pr.step(4)
        sh = dev.bake_volume(g, 8, seed=19)[0]
        frame = dev.render_baked(mcpt.baked_volume(g, sh), samples=2, seed=5)
        if interrupted:
            rad = dev.bake_reflection_probes(p, 5, 4, seed=3, stats=mcpt.Stats())[0]
            c, chain = dev.prefilter_reflection(rad, 5, [(5, 8), (2, 1)])
            dev.reflection_lookup(c, chain, [0, 1], [[0, 0, 1.0], [1.0, 0, 0]], 3.0)
        pr.step(4)
        sh2 = dev.bake_volume(g, 8, seed=19)[0]
        frame2 = dev.render_baked(mcpt.baked_volume(g, sh2), samples=2, seed=5)
        assert _same(sh, sh2) and _same(frame["image"], frame2["image"])
        runs.append((pr.image(), pr.stderr(), sh, frame["image"]))
        pr.close()
    assert all(_same(a, b) for a, b in zip(runs[0], runs[1]))
