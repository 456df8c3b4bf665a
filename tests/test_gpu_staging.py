"""The host-pointer forms of the query family share one staging path (csrc/staging.hpp): device copies of the caller's arrays around the
device form.  Every form is called through the C ABI itself, once with every optional array absent and once with all of them present: the
mandatory answer is the same in every word; where a form takes ids, none means 0 .. n - 1; an empty list is answered MCPT_OK with the
caller's arrays untouched.  And the workspaces two kinds of call share on a device (the lightmap baker's and the denoiser's, the volume
bake's and the visibility grid bake's) pass from one call to the next: a sequence on one device answers what fresh devices answer.
cornell-box at the sizes of tests/query_family.py."""
import ctypes as C
import os

import numpy as np
import pytest

import query_family as QF
from conftest import SCENES
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
