"""The host-pointer forms of the query family share one staging path (csrc/staging.hpp): device copies of the caller's arrays around the
device form.  Every form is called through the C ABI itself, once with every optional array absent and once with all of them present: the
mandatory answer is the same in every word; where a form takes ids, none means 0 .. n - 1; an empty list is answered MCPT_OK with the
caller's arrays untouched.  And the workspaces two kinds of call share on a device (the lightmap baker's and the denoiser's, the volume
bake's and the visibility grid bake's) pass from one call to the next: a sequence on one device answers what fresh devices answer.
The calls that are older than the family stand on the same path: closest hit (an absent face, t or p still has room on the device, an
absent pn has none), the (pixel, sample) seams of the camera, the environment and the light picks (one list answers what its two halves
answer), and the frames that go in and come back -- mcpt_render and a progressive handle's image, denoised frames and pictures under a
partition that owns some pixels: the others keep the caller's bytes, the owned ones are the device form's bit for bit.
cornell-box at the sizes of tests/query_family.py; the light picks in a room of tests/light_scenes.py."""
import ctypes as C
import os

import numpy as np
import pytest

import light_scenes
import query_family as QF
from conftest import SCENES
from guarded import Guarded
from hip_rt import Stream
from montecarlopathtracing_amd._lib import check
from montecarlopathtracing_amd.api import _adaptive_params, _p, _visibility_params

pytestmark = pytest.mark.gpu

KNOBS = ("MCPT_TRACE_ENGINE", "MCPT_FINISH_ENGINE", "MCPT_FINISH_PATHS", "MCPT_WORKSPACE_GB")
F64, I32, U8 = np.float64, np.int32, np.uint8
D, I, B = C.c_double, C.c_int32, C.c_uint8
MARK = {np.dtype(F64): 7.25, np.dtype(I32): -77, np.dtype(U8): 201}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _device(mcpt):
    sc = mcpt.Scene(SCENES, "cornell-box", width=QF.W, height=QF.H)
    return sc, mcpt.Device(sc, 0)


@pytest.fixture(scope="module")
def world(mcpt):
    saved = {k: os.environ.pop(k) for k in KNOBS if k in os.environ}
    try:
        sc, dev = _device(mcpt)
    finally:
        os.environ.update(saved)
    q = QF.lists(mcpt, sc.faces()[0][:, :9])
    yield mcpt, dev, q
    dev.close()
    sc.close()


def marked(shape, dtype):
    return np.full(shape, MARK[np.dtype(dtype)], dtype=dtype)


def untouched(*arrays):
    return all(a is None or (a == MARK[a.dtype]).all() for a in arrays)


def same(a, b):
    return np.array_equal(QF.bits(a), QF.bits(b))


def both(call):
    """call(opt) -> (mandatory arrays, optional arrays): with the optional ones absent and present, the mandatory ones are equal in every word"""
    bare, none = call(False)
    full, extra = call(True)
    assert all(x is None for x in none) and all(x is not None and not untouched(x) for x in extra)
    assert len(bare) == len(full) > 0 and all(same(a, b) and not untouched(a) for a, b in zip(bare, full))
    return full, extra


# ---- the query calls

def _radiance(world, n, ids, opt, sh=False, adaptive=False):
    mcpt, dev, q = world
    lst = np.ascontiguousarray(q["probes"][:n] if sh else q["rays"][:n])
    k = 27 if sh else 3
    mean, err, hits = marked((max(n, 1), k), F64), marked((max(n, 1), k), F64) if opt else None, marked(max(n, 1), I32) if opt else None
    counts = marked(max(n, 1), I32) if opt and adaptive else None
    st = mcpt.Stats() if opt else None
    stp = C.byref(st) if opt else None
    if sh:
        sp = mcpt.ShParams(QF.PROBE_SPP, 0, QF.SEED, 0, (C.c_int32 * 3)(0, 0, 0))
        check(mcpt.lib().mcpt_query_sh(dev._h, _p(lst, D), _p(ids, I), n, C.byref(sp), _p(mean, D), _p(err, D), _p(hits, I), stp))
    else:
        qp = mcpt.QueryParams(QF.ADAPTIVE_SPP if adaptive else QF.RAY_SPP, QF.RAY_BASE, QF.SEED, mcpt.QUERY_RAY, 0, (C.c_int32 * 2)(0, 0))
        if adaptive:
            ap = _adaptive_params(QF.ADAPTIVE_REL, 0.0, QF.ADAPTIVE_MIN)
            check(mcpt.lib().mcpt_query_radiance_adaptive(dev._h, _p(lst, D), _p(ids, I), n, C.byref(qp), C.byref(ap), _p(mean, D), _p(err, D), _p(hits, I),
                                                          _p(counts, I), stp))
        else:
            check(mcpt.lib().mcpt_query_radiance(dev._h, _p(lst, D), _p(ids, I), n, C.byref(qp), _p(mean, D), _p(err, D), _p(hits, I), stp))
    if opt and n > 0:
        assert st.samples > 0
    return (mean,), (err, hits) + ((counts,) if adaptive else ())


@pytest.mark.parametrize("form", ["radiance", "sh", "adaptive"])
def test_the_query_forms(world, form):
    kw = dict(sh=form == "sh", adaptive=form == "adaptive")
    n = QF.N_PROBES if form == "sh" else QF.N_RAYS
    (mean,), extra = both(lambda opt: _radiance(world, n, None, opt, **kw))
    (listed,), extra_listed = _radiance(world, n, np.arange(n, dtype=I32), True, **kw)
    assert same(mean, listed) and all(same(a, b) for a, b in zip(extra, extra_listed))
    (other,), _ = _radiance(world, n, np.arange(n, dtype=I32) + 1, True, **kw)
    assert not same(mean, other)                                                # (the ids are read)
    assert mean.max() > 0 and extra[1].max() > 0
    empty, empty_extra = _radiance(world, 0, None, True, **kw)
    assert untouched(*empty) and untouched(*empty_extra)


@pytest.mark.parametrize("sh", [False, True])
def test_the_ray_seams(world, sh):
    mcpt, dev, q = world
    n = QF.N_PROBES if sh else QF.N_RAYS
    lst = np.ascontiguousarray(q["probes"] if sh else q["rays"])
    k = (np.arange(n) % 5).astype(I32)

    def rays(n, ids):
        out = marked((max(n, 1), 6), F64)
        if sh:
            check(mcpt.lib().mcpt_query_sh_rays(dev._h, _p(lst, D), _p(ids, I), n, QF.SEED, _p(k, I), _p(out, D)))
        else:
            check(mcpt.lib().mcpt_query_rays(dev._h, _p(lst, D), _p(ids, I), n, QF.SEED, mcpt.QUERY_RAY, _p(k, I), _p(out, D)))
        return out
    got = rays(n, None)
    assert not untouched(got) and same(got, rays(n, np.arange(n, dtype=I32))) and untouched(rays(0, None))
    if sh:
        assert not same(got, rays(n, np.arange(n, dtype=I32) + 1))


# ---- lightmaps

def _bake_lightmap(mcpt, dev, size, opt, adaptive=False, dilate=2):
    E = marked((size, size, 3), F64)
    err, hits, owner = (marked((size, size, 3), F64), marked((size, size), I32), marked((size, size), I32)) if opt else (None, None, None)
    counts = marked((size, size), I32) if opt and adaptive else None
    lp = mcpt.LightmapParams(size, size, QF.ADAPTIVE_SPP if adaptive else QF.MAP_SPP, 0, QF.SEED, 0, dilate, (C.c_int32 * 2)(0, 0))
    if adaptive:
        ap = _adaptive_params(QF.ADAPTIVE_REL, 0.0, QF.ADAPTIVE_MIN)
        check(mcpt.lib().mcpt_bake_lightmap_adaptive(dev._h, None, C.byref(lp), C.byref(ap), _p(E, D), _p(err, D), _p(hits, I), _p(owner, I), _p(counts, I), None))
    else:
        check(mcpt.lib().mcpt_bake_lightmap(dev._h, None, C.byref(lp), _p(E, D), _p(err, D), _p(hits, I), _p(owner, I), None))
    return (E,), (err, hits, owner) + ((counts,) if adaptive else ())


def _denoise(mcpt, dev, E, err, opt, dilate=2):
    h, w = E.shape[:2]
    out, owner = marked((h, w, 3), F64), marked((h, w), I32) if opt else None
    dp = mcpt.LightmapDenoiseParams(w, h, 3, dilate, 0.0, 0.0, (C.c_int32 * 2)(0, 0))
    check(mcpt.lib().mcpt_lightmap_denoise(dev._h, None, C.byref(dp), _p(E, D), _p(err, D), _p(out, D), _p(owner, I)))
    return (out,), (owner,)


@pytest.mark.parametrize("adaptive", [False, True])
def test_the_lightmap_bakes(world, adaptive):
    mcpt, dev, _ = world
    (E,), extra = both(lambda opt: _bake_lightmap(mcpt, dev, QF.MAP, opt, adaptive))
    assert E.max() > 0 and (extra[2] >= 0).any()


def test_the_lightmap_denoiser_and_the_texel_list(world):
    mcpt, dev, _ = world
    (E,), (err, _, owner) = _bake_lightmap(mcpt, dev, QF.MAP, True, dilate=0)
    (out,), (down,) = both(lambda opt: _denoise(mcpt, dev, E, err, opt))
    assert out.max() > 0 and np.array_equal(down >= 0, owner >= 0)
    # the texel list: the count is the same whatever is asked for, and the lists are the owner map's
    L = mcpt.lib().mcpt_lightmap_texels
    n = L(dev._h, None, QF.MAP, QF.MAP, None, None, None, 0)
    assert n == int((owner >= 0).sum()) > 0
    own, texels, q6 = marked((QF.MAP, QF.MAP), I32), marked(n, I32), marked((n, 6), F64)
    assert L(dev._h, None, QF.MAP, QF.MAP, _p(own, I), _p(texels, I), _p(q6, D), n) == n
    assert np.array_equal(own, owner) and np.array_equal(texels, np.flatnonzero(owner.reshape(-1) >= 0)) and not untouched(q6)
    only = marked(n, I32)
    assert L(dev._h, None, QF.MAP, QF.MAP, None, _p(only, I), None, n) == n and np.array_equal(only, texels)


def test_the_lightmap_lookup(world):
    mcpt, dev, _ = world
    (E,), (_, _, owner) = _bake_lightmap(mcpt, dev, QF.MAP, True)
    uv = np.ascontiguousarray(np.random.default_rng(5).random((QF.N_RAYS, 2)))

    def look(n, opt, own=owner):
        e, taps = marked((max(n, 1), 3), F64), marked(max(n, 1), I32) if opt else None
        check(mcpt.lib().mcpt_lightmap_irradiance(dev._h, QF.MAP, QF.MAP, _p(E, D), _p(own, I), _p(uv, D), n, _p(e, D), _p(taps, I)))
        return (e,), (taps,)
    (e,), (taps,) = both(lambda opt: look(QF.N_RAYS, opt))
    he, ht = mcpt.lightmap_irradiance_host(E, uv, owner=owner)
    assert same(e, he) and np.array_equal(taps, ht) and e.max() > 0
    (plain,), _ = both(lambda opt: look(QF.N_RAYS, opt, None))                    # (the owner map is optional too)
    assert same(plain, mcpt.lightmap_irradiance_host(E, uv)[0])
    assert untouched(*sum(look(0, True), ()))


# ---- volumes and visibility

def _bake_volume(mcpt, dev, g, opt):
    shape = (g.nz, g.ny, g.nx)
    sh, err, hits = marked(shape + (9, 3), F64), marked(shape + (9, 3), F64) if opt else None, marked(shape, I32) if opt else None
    sp = mcpt.ShParams(QF.VOLUME_SPP, 0, QF.SEED, 0, (C.c_int32 * 3)(0, 0, 0))
    check(mcpt.lib().mcpt_bake_volume(dev._h, C.byref(g), C.byref(sp), _p(sh, D), _p(err, D), _p(hits, I), None))
    return (sh,), (err, hits)


def _visibility(mcpt, dev, q, n, ids, opt, grid=None):
    shape = (grid.nz, grid.ny, grid.nx) if grid is not None else (max(n, 1),)
    res = QF.GRID_VIS_RES if grid is not None else QF.VIS_RES
    m = marked(shape + (res * res, 2), F64)
    hits, back, valid = (marked(shape, I32), marked(shape, I32), marked(shape, U8)) if opt else (None, None, None)
    if grid is not None:
        vp = _visibility_params(QF.GRID_VIS_SPP, res, q["grid_distance"], QF.BACK_FRACTION, QF.SEED, 0, 0)
        check(mcpt.lib().mcpt_bake_volume_visibility(dev._h, C.byref(grid), C.byref(vp), _p(m, D), _p(hits, I), _p(back, I), _p(valid, B), None))
    else:
        p = np.ascontiguousarray(q["vis_probes"])
        vp = _visibility_params(QF.VIS_SPP, res, q["vis_distance"], QF.BACK_FRACTION, QF.SEED, 0, QF.VIS_WORKSPACE)
        check(mcpt.lib().mcpt_query_visibility(dev._h, _p(p, D), _p(ids, I), n, C.byref(vp), _p(m, D), _p(hits, I), _p(back, I), _p(valid, B), None))
    return (m,), (hits, back, valid)


def test_the_volume_and_visibility_bakes(world):
    mcpt, dev, q = world
    (sh,), (_, hits) = both(lambda opt: _bake_volume(mcpt, dev, q["grid"], opt))
    assert np.abs(sh).max() > 0 and hits.max() > 0
    n = QF.N_VIS
    (m,), extra = both(lambda opt: _visibility(mcpt, dev, q, n, None, opt))
    (listed,), extra_listed = _visibility(mcpt, dev, q, n, np.arange(n, dtype=I32), True)
    assert same(m, listed) and all(np.array_equal(a, b) for a, b in zip(extra, extra_listed))
    assert not same(m, _visibility(mcpt, dev, q, n, np.arange(n, dtype=I32) + 1, True)[0][0])
    assert untouched(*sum(_visibility(mcpt, dev, q, 0, None, True), ()))
    (gm,), (_, _, valid) = both(lambda opt: _visibility(mcpt, dev, q, 0, None, opt, grid=q["grid"]))
    assert (gm[..., 0] >= 0).any() and valid.any()


def test_the_volume_lookups(world):
    mcpt, dev, q = world
    g = q["grid"]
    (sh,), _ = _bake_volume(mcpt, dev, g, False)
    (moments,), (_, _, valid) = _visibility(mcpt, dev, q, 0, None, True, grid=g)
    vis = mcpt.volume_visibility(QF.GRID_VIS_RES, q["grid_distance"], normal_bias=0.01 * q["grid_distance"])
    recv = np.ascontiguousarray(np.concatenate([q["points"], q["normals"]], axis=1))
    valid = np.ascontiguousarray(valid)

    def look(n, opt, visible):
        e, corners = marked((max(n, 1), 3), F64), marked(max(n, 1), I32) if opt else None
        if visible:
            check(mcpt.lib().mcpt_volume_irradiance_visible(dev._h, C.byref(g), _p(sh, D), _p(moments, D), _p(valid if opt else None, B), C.byref(vis),
                                                            _p(recv, D), n, _p(e, D), _p(corners, I)))
        else:
            check(mcpt.lib().mcpt_volume_irradiance(dev._h, C.byref(g), _p(sh, D), _p(valid if opt else None, B), _p(recv, D), n, _p(e, D), _p(corners, I)))
        return (e,), (corners,)
    for visible in (False, True):
        # (the mask is an optional input: with it the answer may differ, so the two calls are held to the host form instead)
        host = mcpt.volume_irradiance_visible_host if visible else mcpt.volume_irradiance_host
        args = (g, sh, moments) if visible else (g, sh)
        kw = dict(vis=vis) if visible else {}
        for opt in (False, True):
            (e,), (corners,) = look(QF.N_POINTS, opt, visible)
            he, hc = host(*args, q["points"], q["normals"], valid=valid.reshape(-1) if opt else None, **kw)
            assert same(e, he) and (corners is None or np.array_equal(corners, hc)), (visible, opt)
            assert not untouched(e)
        assert untouched(*sum(look(0, True, visible), ()))


# ---- baked shading

def test_baked_radiance_and_the_baked_frame(world):
    mcpt, dev, q = world
    g = q["grid"]
    (sh,), _ = _bake_volume(mcpt, dev, g, False)
    (moments,), (_, _, valid) = _visibility(mcpt, dev, q, 0, None, True, grid=g)
    (E,), (_, _, owner) = _bake_lightmap(mcpt, dev, QF.MAP, True)
    vis = mcpt.volume_visibility(QF.GRID_VIS_RES, q["grid_distance"], normal_bias=0.01 * q["grid_distance"])
    sources = {"volume": mcpt.baked_volume(g, sh), "volume-visible": mcpt.baked_volume(g, sh, valid=valid, moments=moments, vis=vis),
               "lightmap": mcpt.baked_lightmap(E), "lightmap-owner": mcpt.baked_lightmap(E, owner=owner)}
    rays = np.ascontiguousarray(q["rays"])
    names = ("radiance", "kind", "face", "q6", "uv", "kd", "e", "lit")
    width = {"radiance": 3, "q6": 6, "uv": 2, "kd": 3, "e": 3}

    def radiance(s, n, opt):
        out = {k: marked((max(n, 1), width[k]), F64) if k in width else marked(max(n, 1), I32) for k in names if opt or k == "radiance"}
        o = mcpt.BakedOutputs(*[out[k].ctypes.data if k in out else None for k in names])
        check(mcpt.lib().mcpt_baked_radiance(dev._h, C.byref(s), _p(rays, D), n, 1, C.byref(o), None))
        return (out["radiance"],), tuple(out.get(k) for k in names[1:])

    def frame(s, opt):
        img = marked((QF.H, QF.W, 3), F64)
        counts, lit = (marked((QF.H, QF.W, 3), I32), marked((QF.H, QF.W), I32)) if opt else (None, None)
        fp = mcpt.BakedFrameParams(QF.FRAME_SAMPLES, 1, QF.SEED, 1000, (C.c_int32 * 2)(0, 0))
        check(mcpt.lib().mcpt_render_baked(dev._h, C.byref(s), C.byref(fp), _p(img, D), _p(counts, I), _p(lit, I), None))
        return (img,), (counts, lit)
    for key, source in sources.items():
        s = source.struct()
        (rad,), extra = both(lambda opt: radiance(s, QF.N_RAYS, opt))
        assert rad.max() > 0 and extra[-1].max() > 0, key
        assert untouched(*sum(radiance(s, 0, True), ())), key
        (img,), (counts, lit) = both(lambda opt: frame(s, opt))
        assert img.max() > 0 and (counts.sum(axis=2) == QF.FRAME_SAMPLES).all() and lit.max() > 0, key


# ---- reflection probes

def test_the_reflection_forms(world):
    mcpt, dev, q = world
    p = np.ascontiguousarray(q["refl_probes"])
    R, S, n = QF.REFL_RES, QF.REFL_SPP, QF.N_REFL
    rp = mcpt.ReflectionParams(S, 0, QF.SEED, R, 0, QF.REFL_WORKSPACE, (C.c_int32 * 4)(0, 0, 0, 0))

    def bake(n, base, opt):
        rad = marked((max(n, 1), R * R, 3), F64)
        err, hits = (marked((max(n, 1), R * R, 3), F64), marked((max(n, 1), R * R), I32)) if opt else (None, None)
        check(mcpt.lib().mcpt_bake_reflection(dev._h, _p(p, D), _p(base, I), n, C.byref(rp), _p(rad, D), _p(err, D), _p(hits, I), None))
        return (rad,), (err, hits)
    (rad,), extra = both(lambda opt: bake(n, None, opt))
    own = (np.arange(n) * R * R * S).astype(I32)
    (listed,), extra_listed = bake(n, own, True)
    assert same(rad, listed) and all(same(a, b) for a, b in zip(extra, extra_listed)) and rad.max() > 0
    assert not same(rad, bake(n, own + 1, True)[0][0])
    assert untouched(*sum(bake(0, None, True), ()))

    def rays(m, base):
        entry = np.arange(max(m, 1), dtype=np.int64) * 7 % (n * R * R * S)
        r6, ids = marked((max(m, 1), 6), F64), marked(max(m, 1), I32)
        check(mcpt.lib().mcpt_reflection_rays(dev._h, _p(p, D), _p(base, I), n, C.byref(rp), _p(entry, C.c_int64), m, _p(r6, D), _p(ids, I)))
        return r6, ids
    r6, ids = rays(40, None)
    l6, lids = rays(40, own)
    assert same(r6, l6) and np.array_equal(ids, lids) and not untouched(r6) and not untouched(ids) and untouched(*rays(0, None))
    assert not np.array_equal(ids, rays(40, own + 1)[1])

    c = mcpt.reflection_chain(R, [(4, 64), (2, 4)])
    T = c.num_texels

    def prefilter(n):
        chain = marked((max(n, 1), T, 3), F64)
        check(mcpt.lib().mcpt_reflection_prefilter(dev._h, C.byref(c), _p(rad, D), n, _p(chain, D)))
        return chain
    chain = prefilter(n)
    assert same(chain, mcpt.reflection_prefilter_host(c, rad)) and chain.max() > 0 and untouched(prefilter(0))

    m = 67
    rng = np.random.default_rng(9)
    probe, dirs, ns = (np.arange(m) % n).astype(I32), np.ascontiguousarray(rng.normal(size=(m, 3))), np.ascontiguousarray(rng.random(m) * 80.0)

    def lookup(m):
        out = marked((max(m, 1), 3), F64)
        check(mcpt.lib().mcpt_reflection_lookup(dev._h, C.byref(c), _p(chain, D), n, _p(probe, I), _p(dirs, D), _p(ns, D), m, _p(out, D)))
        return out
    out = lookup(m)
    assert same(out, mcpt.reflection_lookup_host(c, chain, probe, dirs, ns)) and out.max() > 0 and untouched(lookup(0))


# ---- the display transform

def test_the_display_form(world):
    mcpt, dev, _ = world
    img = np.ascontiguousarray(np.random.default_rng(3).random((QF.H * QF.W, 3)) * 2.0)
    kw = dict(auto_key=0.18, curve="reinhard", transfer="srgb")
    dp = mcpt.make_display(**kw)

    def show(n, opt):
        out = marked((max(n, 1), 3), U8)
        info = mcpt.DisplayInfo() if opt else None
        check(mcpt.lib().mcpt_display(dev._h, _p(img, D), n, C.byref(dp), _p(out, B), C.byref(info) if opt else None))
        return out
    a, b = show(QF.H * QF.W, False), show(QF.H * QF.W, True)
    assert np.array_equal(a, b) and np.array_equal(a, mcpt.display_host(img, **kw)[0]) and len(np.unique(a)) > 50
    assert untouched(show(0, True))


# ---- the workspaces that two kinds of call share

def test_a_sequence_on_one_device_is_what_fresh_devices_answer(world):
    mcpt, dev, q = world
    g = q["grid"]
    small = QF.MAP // 2
    first = _bake_lightmap(mcpt, dev, QF.MAP, True, dilate=0)
    E, err = first[0][0], first[1][0]
    steps = [("bake_lightmap", lambda d: _bake_lightmap(mcpt, d, QF.MAP, True, dilate=0)),
             ("lightmap_denoise", lambda d: _denoise(mcpt, d, E, err, True)),
             ("bake_volume_visibility", lambda d: _visibility(mcpt, d, q, 0, None, True, grid=g)),
             ("bake_volume", lambda d: _bake_volume(mcpt, d, g, True)),
             ("bake_lightmap, smaller", lambda d: _bake_lightmap(mcpt, d, small, True)),
             ("lightmap_denoise, larger again", lambda d: _denoise(mcpt, d, E, err, True))]
    flat = lambda r: r[0] + r[1]
    got = [flat(run(dev)) for _, run in steps]
    assert all(same(a, b) for a, b in zip(got[0], flat(first)))
    for (name, run), mine in zip(steps, got):
        sc, fresh = _device(mcpt)
        want = flat(run(fresh))
        fresh.close()
        sc.close()
        assert len(mine) == len(want) and all(same(a, b) for a, b in zip(mine, want)), name
        assert not untouched(*mine)


# ---- the calls older than the family: closest hit, the (pixel, sample) seams, the frames that go in and come back

N = QF.N_RAYS                                   # 257: more than one 256-lane workgroup, and odd
ERR_ARG = -3                                    # mcpt.h: MCPT_ERR_ARG
PART = (0, 2, 8, 4)                             # rank 0 of 2 over tiles of 8 x 4: some pixels of 64 x 36 are owned, some are not


@pytest.fixture(scope="module")
def stream(world):
    s = Stream()
    yield s
    s.destroy()


class OnDevice:
    """the arrays of one device-form call in tests/guarded.py buffers, as tests/test_gpu_extents.py holds them: put(a) uploads a and
    returns the device address, get(i) reads the i-th buffer back once the call's stream has been waited for"""

    def __init__(self):
        self.g = []

    def put(self, a):
        self.g.append((Guarded(np.ascontiguousarray(a), a.dtype, 0xFF), a.shape))
        return self.g[-1][0].ptr

    def get(self, i):
        g, shape = self.g[i]
        return g.payload().reshape(shape)

    def free(self):
        for g, _ in self.g:
            g.free()


def halves(call, n=N):
    """call(lo, hi) -> the marked output arrays of entries [lo, hi) after the call: asked twice it answers equally in every word, as one
    list it answers what its two halves answer, and an empty list leaves the arrays as they were"""
    whole, again = call(0, n), call(0, n)
    first, second = call(0, n // 2), call(n // 2, n)
    assert len(whole) > 0 and all(not untouched(a) for a in whole)
    assert all(same(a, b) for a, b in zip(whole, again))
    assert all(same(a, np.concatenate([x, y])) for a, x, y in zip(whole, first, second))
    assert untouched(*call(0, 0))
    return whole


def pairs(seed, samples=64):
    rng = np.random.default_rng(seed)
    return rng.integers(0, QF.W * QF.H, size=N).astype(I32), rng.integers(0, samples, size=N).astype(I32)


def test_closest_hit(world, stream):
    mcpt, dev, q = world
    L = mcpt.lib()
    rays = np.ascontiguousarray(q["rays"])
    names = ("face", "t", "p", "pn")

    def trace(n, present, st=None):
        out = {"face": marked(max(n, 1), I32), "t": marked(max(n, 1), F64), "p": marked((max(n, 1), 3), F64), "pn": marked((max(n, 1), 3), F64)}
        a = {k: out[k] if k in present else None for k in names}
        check(L.mcpt_trace_closest(dev._h, _p(rays, D), n, _p(a["face"], I), _p(a["t"], D), _p(a["p"], D), _p(a["pn"], D),
                                   C.byref(st) if st is not None else None))
        return out
    st = mcpt.Stats()
    trace(N, (), st)                                                            # every output absent: the call still runs
    assert st.launches == 1
    full = trace(N, names, st)
    assert st.launches == 1 and (full["face"] >= 0).any() and (full["face"] < 0).any() and all(not untouched(full[k]) for k in names)
    for k in names:                                                             # each alone: the same words, the others as they were
        alone = trace(N, (k,))
        assert same(alone[k], full[k]) and untouched(*[alone[o] for o in names if o != k]), k
    assert untouched(*trace(0, names).values())
    od = OnDevice()
    try:
        ptrs = [od.put(rays)] + [od.put(marked(full[k].shape, full[k].dtype)) for k in names]
        check(L.mcpt_trace_closest_device(dev._h, ptrs[0], N, ptrs[1], ptrs[2], ptrs[3], ptrs[4], stream.h))
        stream.synchronize()
        for i, k in enumerate(names):
            assert same(od.get(1 + i), full[k]), k
    finally:
        od.free()


@pytest.mark.parametrize("call", ["sample_radiance", "sample_radiance-lens", "camera_rays-lens"])
def test_the_pixel_sample_seams(world, call):
    mcpt, dev, _ = world
    L = mcpt.lib()
    pix, k = pairs(11)
    f, per = (L.mcpt_camera_rays, 6) if call.startswith("camera_rays") else (L.mcpt_sample_radiance, 3)

    def ask(lo, hi, pix=pix):
        out = marked((max(hi - lo, 1), per), F64)
        rc = f(dev._h, QF.SEED, _p(np.ascontiguousarray(pix[lo:hi]), I), _p(np.ascontiguousarray(k[lo:hi]), I), hi - lo, _p(out, D))
        return rc, out

    def answer(lo, hi):
        rc, out = ask(lo, hi)
        check(rc)
        return (out,)
    if call.endswith("-lens"):
        check(L.mcpt_device_set_lens(dev._h, C.byref(mcpt.make_lens(aperture=0.05, focus_distance=2.0, jitter=True))))
    try:
        (out,) = halves(answer)
        assert np.nan_to_num(np.abs(out)).max() > 0
        for bad in (QF.W * QF.H, -1):                                           # a pixel outside the frame: refused, nothing written
            off = pix.copy()
            off[N - 1] = bad
            rc, kept = ask(0, N, off)
            assert rc == ERR_ARG and "pixel index out of range" in L.mcpt_last_error().decode() and untouched(kept)
    finally:
        check(L.mcpt_device_set_lens(dev._h, None))


def test_the_environment_seams(world):
    """(tests/test_gpu_env.py holds the draw's radiance to mcpt_environment_eval at the drawn direction only away from the texels' column
    borders, so that identity is no word-for-word one and is left to it: here the halves)"""
    mcpt, dev, _ = world
    L = mcpt.lib()
    rng = np.random.default_rng(12)
    dirs = np.ascontiguousarray(rng.normal(size=(N, 3)))
    pix, k = pairs(13)
    dev.set_environment(0.05 + rng.random((4, 8, 3)), scale=1.5)                # 8 x 4 texels
    try:
        def evaluate(lo, hi):
            rgb = marked((max(hi - lo, 1), 3), F64)
            check(L.mcpt_environment_eval(dev._h, _p(np.ascontiguousarray(dirs[lo:hi]), D), hi - lo, _p(rgb, D)))
            return (rgb,)

        def draw(lo, hi):
            d, pdf, rgb = marked((max(hi - lo, 1), 3), F64), marked(max(hi - lo, 1), F64), marked((max(hi - lo, 1), 3), F64)
            check(L.mcpt_environment_sample(dev._h, QF.SEED, _p(np.ascontiguousarray(pix[lo:hi]), I), _p(np.ascontiguousarray(k[lo:hi]), I), 1, hi - lo,
                                            _p(d, D), _p(pdf, D), _p(rgb, D)))
            return d, pdf, rgb
        (rgb,) = halves(evaluate)
        d, pdf, le = halves(draw)
        assert rgb.min() > 0 and pdf.min() > 0 and le.min() > 0 and len(np.unique(QF.bits(le))) > 8
    finally:
        dev.set_environment(None)


@pytest.fixture(scope="module")
def room(mcpt, tmp_path_factory):
    """a room of five lights at the module's frame size, and a device of it"""
    directory = str(tmp_path_factory.mktemp("staging_room")) + os.sep
    light_scenes.write(directory, "room5", 5, QF.W, QF.H)
    saved = {k: os.environ.pop(k) for k in KNOBS if k in os.environ}
    try:
        sc = mcpt.Scene(directory, "room5", width=QF.W, height=QF.H)
        dev = mcpt.Device(sc, 0)
    finally:
        os.environ.update(saved)
    assert sc.info.num_lights == 5
    yield dev
    dev.close()
    sc.close()


@pytest.mark.parametrize("mode", ["one", "tree"])
def test_the_light_picks(mcpt, room, mode):
    L = mcpt.lib()
    pix, k = pairs(14)
    rng = np.random.default_rng(15)
    x0, x1, y0, y1, z0, z1 = light_scenes.ROOM
    p = np.ascontiguousarray(np.array([x0, y0, z0]) + np.array([x1 - x0, y1 - y0, z1 - z0]) * (0.1 + 0.8 * rng.random((N, 3))))
    pn = np.ascontiguousarray(rng.normal(size=(N, 3)))
    room.set_light_sampling(mode)

    def pick(lo, hi):
        light, pdf = marked(max(hi - lo, 1), I32), marked(max(hi - lo, 1), F64)
        a = (room._h, QF.SEED, _p(np.ascontiguousarray(pix[lo:hi]), I), _p(np.ascontiguousarray(k[lo:hi]), I), 2)
        if mode == "one":
            check(L.mcpt_light_pick(*a, hi - lo, _p(light, I), _p(pdf, D)))
        else:
            check(L.mcpt_light_pick_at(*a, _p(np.ascontiguousarray(p[lo:hi]), D), _p(np.ascontiguousarray(pn[lo:hi]), D), hi - lo, _p(light, I), _p(pdf, D)))
        return light, pdf
    try:
        light, pdf = halves(pick)
        assert light.min() >= 0 and light.max() < 5 and len(np.unique(light)) > 1 and (pdf > 0).all() and (pdf <= 1).all()
        if mode == "one":
            assert same(pdf, room.light_sampling()[1][light])                   # the table's entry of the light picked
    finally:
        room.set_light_sampling(None)


def _owned(world):
    mcpt, dev, _ = world
    owned = np.zeros(QF.W * QF.H, bool)
    owned[dev.scene.owned_pixels(*PART)] = True
    assert 0 < owned.sum() < QF.W * QF.H
    return owned


def _frame_held(host, device, owned, what):
    """a frame [H, W, c] of the host form beside the device form's: the pixels not owned hold the mark in every channel of both, the
    owned ones are equal in every word and were written"""
    h, d = host.reshape(owned.size, -1), device.reshape(owned.size, -1)
    mark = MARK[h.dtype]
    assert (h[~owned] == mark).all() and (d[~owned] == mark).all(), what
    assert same(h[owned], d[owned]) and not (h[owned] == mark).all(), what


def test_a_rendered_frame_goes_in_and_comes_back(world, stream):
    mcpt, dev, _ = world
    owned = _owned(world)
    rp = mcpt.RenderParams(2, QF.SEED, *PART, 0)
    img = marked((QF.H, QF.W, 3), F64)
    check(mcpt.lib().mcpt_render(dev._h, C.byref(rp), _p(img, D), None))
    od = OnDevice()
    try:
        check(mcpt.lib().mcpt_render_device(dev._h, C.byref(rp), od.put(marked((QF.H, QF.W, 3), F64)), None, stream.h))
        stream.synchronize()
        _frame_held(img, od.get(0), owned, "mcpt_render")
    finally:
        od.free()
    assert np.nan_to_num(img.reshape(-1, 3)[owned]).max() > 0


def test_progressive_frames_go_in_and_come_back(world, stream):
    mcpt, dev, _ = world
    L = mcpt.lib()
    owned = _owned(world)
    rp = mcpt.RenderParams(4, QF.SEED, *PART, 0)
    h = C.c_void_p()
    check(L.mcpt_progressive_create(dev._h, C.byref(rp), C.byref(h)))
    od = OnDevice()
    try:
        check(L.mcpt_progressive_step(h, 2, None))
        frame = lambda: marked((QF.H, QF.W, 3), F64)
        # the image alone, the standard error alone, both: an array present in two calls is the same in every word
        img, err, img2, err2 = frame(), frame(), frame(), frame()
        check(L.mcpt_progressive_image(h, _p(img, D), None))
        check(L.mcpt_progressive_image(h, None, _p(err, D)))
        check(L.mcpt_progressive_image(h, _p(img2, D), _p(err2, D)))
        assert same(img, img2) and same(err, err2) and not same(img, err)
        check(L.mcpt_progressive_image_device(h, od.put(frame()), od.put(frame()), stream.h))
        stream.synchronize()
        _frame_held(img, od.get(0), owned, "image")
        _frame_held(err, od.get(1), owned, "standard error")
        forms = {"denoise": (lambda a: L.mcpt_progressive_denoise(h, None, _p(a, D)),
                             lambda ptr: L.mcpt_progressive_denoise_device(h, None, ptr, stream.h), F64, 3),
                 "denoise_guided": (lambda a: L.mcpt_progressive_denoise_guided(h, None, None, _p(a, D)),
                                    lambda ptr: L.mcpt_progressive_denoise_guided_device(h, None, None, ptr, stream.h), F64, 3)}
        for name, ch in (("display rgb", 3), ("display rgba", 4)):
            dp = mcpt.make_display(auto_key=0.18, curve="reinhard", transfer="srgb", rgba=ch == 4)
            forms[name] = (lambda a, dp=dp: L.mcpt_progressive_display(h, 0, C.byref(dp), _p(a, B), None),
                           lambda ptr, dp=dp: L.mcpt_progressive_display_device(h, 0, C.byref(dp), ptr, None, stream.h), U8, ch)
        for name, (host_form, device_form, dtype, ch) in forms.items():
            out = marked((QF.H, QF.W, ch), dtype)
            check(host_form(out))
            check(device_form(od.put(marked((QF.H, QF.W, ch), dtype))))
            stream.synchronize()
            _frame_held(out, od.get(len(od.g) - 1), owned, name)
            assert ch != 4 or (out.reshape(-1, 4)[owned, 3] == 255).all()
    finally:
        od.free()
        L.mcpt_progressive_free(h)
