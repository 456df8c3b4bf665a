"""GPU: the lightmap denoiser (mcpt_lightmap_denoise*).  The kernels against the numpy restatement (tests/lightmap_denoise_ref.py) on a
triangle soup, on real bakes and at sizes below the filter's steps; the identity at K = 0 and the dilation; texels that are not covered
are never read; charts that touch in the atlas but not in the world stay apart, by the distance stop alone; a fold keeps its two sides
apart by the normal stop; both forms, aliasing, the workspace shared with the baker, updated geometry; and what the filter buys."""
import ctypes as C

import numpy as np
import pytest

import hip_rt
import lightmap_denoise_ref as DR
import lightmap_ref as R
from conftest import SCENES, extra_scene_dir
from test_gpu_lightmap import BLACK, CAMERA, FLAT, GREY, _soup, _soup_scene

pytestmark = pytest.mark.gpu

RTOL = 1e-12                    # tests/test_gpu_denoise.py's bound for the same kind of sums with exp
NAN = float("nan")
# test_effectiveness: the measured figures times 1.25, the margin 6c gave its own pin
PIN_RATIO, PIN_SHIFT = 1.25 * 0.2678, 1.25 * 0.5668


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _maps(W, H, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.1, 5.0, (H, W, 3)), rng.uniform(0.01, 1.0, (H, W, 3))


def _against_restatement(got, own, want, wown, what):
    """covered texels -- and the texels a dilation filled from them, whose exactness as a dilation test_dilation_is_the_bakers holds --
    within RTOL relative; owner, and every texel that stayed uncovered, exact"""
    assert np.array_equal(own, wown), what
    data = wown != -1
    assert np.isfinite(got).all(), what
    rel = np.abs(got[data] - want[data]) / np.maximum(np.abs(want[data]), 1e-300)
    worst = float(rel.max()) if rel.size else 0.0
    assert worst <= RTOL, "%s: covered texels differ from the restatement by %.3e relative" % (what, worst)
    assert np.array_equal(_bits(got[~data]), _bits(want[~data])) and not _bits(got[~data]).any(), what
    return worst


@pytest.fixture(scope="module")
def soup(mcpt):
    uv, v, vn, mat = _soup()
    sc = _soup_scene(mcpt, uv, v, vn, mat)
    dev = mcpt.Device(sc, 0)
    yield sc, dev, uv, sc.faces()[0]
    dev.close()
    sc.close()


@pytest.mark.parametrize("size", [(1, 1), (3, 5), (67, 41), (257, 130)], ids=lambda s: "%dx%d" % s)
def test_kernels_are_the_restatement(mcpt, soup, size):
    """The soup scene: a shared chart with overlaps, both windings, a face without vertex normals and one without extent.  257 x 130 with
    K = 10: steps 16 .. 512 exceed one or both sides."""
    W, H = size
    sc, dev, uv, g = soup
    E, S = _maps(W, H, 11)
    owner = R.raster(uv, W, H, g[:, 24:27])
    assert not (owner == FLAT).any()
    guide = DR.guides(owner, uv, g)
    if size == (257, 130):
        assert (owner >= 0).sum() > 5000 and (owner == -1).sum() > 5000
    cases = [dict(iterations=k) for k in (0, 1, 5, 10)] + [dict(iterations=4, sigma_l=0.7, sigma_p=3.5)]
    for kw in cases:
        got, own = dev.denoise_lightmap(E, S, **kw)
        want, wown = DR.denoise_guided(E, S, owner, guide, **kw)
        worst = _against_restatement(got, own, want, wown, "%dx%d %r" % (W, H, kw))
        print("%dx%d %r: worst relative difference %.2e" % (W, H, kw, worst))
        if kw["iterations"] == 5 and W * H > 1000:
            cov = owner >= 0
            assert (got[cov] != E[cov]).any()                                   # it filtered
    # uv given is the scene's own vt
    got2, own2 = dev.denoise_lightmap(E, S, uv=uv, iterations=5)
    got1, own1 = dev.denoise_lightmap(E, S, iterations=5)
    assert _same(got1, got2) and np.array_equal(own1, own2)


def _scene_and_chart(mcpt, name):
    if name == "glassroom":                                 # its textured faces carry vt
        return mcpt.Scene(extra_scene_dir(), name, width=64, height=36), None
    sc = mcpt.Scene(SCENES, name, width=64, height=36)
    return sc, mcpt.grid_atlas(sc.info.num_faces, 128, 128, pad=0)


@pytest.mark.parametrize("case", ["glassroom", "glassroom-adaptive", "veach-mis"])
def test_real_bakes_against_the_restatement(mcpt, case):
    name = case.split("-adaptive")[0]
    sc, uv = _scene_and_chart(mcpt, name)
    dev = mcpt.Device(sc, 0)
    g = sc.faces()[0]
    chart = uv if uv is not None else g[:, 18:24]
    if case.endswith("adaptive"):
        E, S, hits, own0, counts = dev.bake_lightmap_adaptive(128, 128, 64, 0.1, uv=uv, seed=5)
        assert counts.max() > counts[own0 >= 0].min()
    else:
        E, S, hits, own0 = dev.bake_lightmap(128, 128, 16, uv=uv, seed=5)
    assert (own0 >= 0).sum() > 500 and (E > 0).any() and (S > 0).any()
    got, own = dev.denoise_lightmap(E, S, uv=uv, dilate=2)
    want, wown = DR.denoise(E, S, chart, g, dilate=2)
    assert np.array_equal(wown >= 0, own0 >= 0)
    worst = _against_restatement(got, own, want, wown, case)
    assert (wown < -1).any() or name == "glassroom"                               # (glassroom's own chart leaves no gutter in the map)
    print("%s: worst relative difference %.2e over %d covered texels" % (case, worst, (wown >= 0).sum()))
    dev.close()
    sc.close()


def test_identity_at_k0(mcpt, soup):
    sc, dev, uv, g = soup
    W, H = 67, 41
    E, S = _maps(W, H, 12)
    owner = R.raster(uv, W, H, g[:, 24:27])
    cov = owner >= 0
    got, own = dev.denoise_lightmap(E, S, iterations=0)
    assert np.array_equal(own, owner) and cov.any() and (~cov).any()
    assert np.array_equal(_bits(got[cov]), _bits(E[cov]))
    assert not _bits(got[~cov]).any()                                               # +0.0


@pytest.mark.parametrize("rounds", [1, 2, 64])
def test_dilation_is_the_bakers(mcpt, soup, rounds):
    """filled texels and owners are lightmap_ref's dilation of the filtered map, bit for bit"""
    sc, dev, uv, g = soup
    W, H = 257, 130
    E, S = _maps(W, H, 13)
    for k in (0, 3):
        base, own0 = dev.denoise_lightmap(E, S, iterations=k)
        got, own = dev.denoise_lightmap(E, S, iterations=k, dilate=rounds)
        want, wown = R.dilate(base, own0, rounds)
        assert np.array_equal(own, wown) and (own < -1).any()
        assert np.array_equal(_bits(got), _bits(want)), (k, rounds)


def test_uncovered_texels_are_never_neighbours(mcpt, soup):
    sc, dev, uv, g = soup
    W, H = 67, 41
    E, S = _maps(W, H, 14)
    a, own = dev.denoise_lightmap(E, S, dilate=2)
    assert (own == -1).any() and (own < -1).any() and (own >= 0).any()
    E2, S2 = E.copy(), S.copy()
    E2[own == -1] = NAN; E2[own < -1] = 1e300
    S2[own == -1] = 1e300; S2[own < -1] = NAN
    b, own2 = dev.denoise_lightmap(E2, S2, dilate=2)
    assert np.array_equal(own, own2) and np.array_equal(_bits(a), _bits(b)) and np.isfinite(a).all()


def _charted_scene(mcpt, v, vn, uv):
    """the charted faces, grey, and a small lamp far above them whose chart covers nothing (the last face)"""
    lamp_v = np.array([[0.0, 50.0, 0.0, 1.0, 50.0, 0.0, 0.0, 50.0, 1.0]])
    lamp_n = np.tile([0.0, -1.0, 0.0], (1, 3)).astype(np.float64)
    v, vn, uv = np.concatenate([v, lamp_v]), np.concatenate([vn, lamp_n]), np.concatenate([uv, np.zeros((1, 6))])
    mat = np.ones(v.shape[0], dtype=np.int32)
    mat[-1] = 0
    return mcpt.Scene.from_arrays(v, vn, mat, np.array([BLACK, GREY]), [0], [[3.0, 3.0, 3.0]], *CAMERA, vt=uv)


def test_seams(mcpt):
    """Two coplanar unit quads whose charts share the UV edge u = 1/2.  1001 units apart (1000 times their extent) nothing crosses the
    edge although the luminance stop is wide open; edge to edge in the world the same maps mix: the distance stop, and nothing else, did
    the separating."""
    W, H = 32, 16
    E = np.ones((H, W, 3)); E[:, W // 2:] = 100.0
    S = np.full((H, W, 3), 1e6)
    near = slice(W // 2 - 2, W // 2 + 2)
    for gap in (1001.0, 1.0):
        sc = _charted_scene(mcpt, *DR.two_quads(gap))
        dev = mcpt.Device(sc, 0)
        out, own = dev.denoise_lightmap(E, S)
        assert (own[:, :W // 2] >= 0).all() and (own[:, :W // 2] <= 1).all() and (own[:, W // 2:] >= 2).all() and (own[:, W // 2:] <= 3).all()
        want, wown = DR.denoise(E, S, sc.faces()[0][:, 18:24], sc.faces()[0])
        _against_restatement(out, own, want, wown, "gap %g" % gap)
        if gap > 1.0:
            assert np.abs(out / E - 1.0).max() <= 1e-12
        else:
            leak = np.abs(out[:, near] - E[:, near])
            print("leak at the shared edge, side by side: %.3g .. %.3g" % (leak.min(), leak.max()))
            assert (leak > 1.0).all()
        dev.close()
        sc.close()


def test_normal_stop(mcpt):
    """A floor and a wall charted contiguously: positions run on across the fold, the normals turn by a right angle, neither leaks"""
    W, H = 32, 16
    sc = _charted_scene(mcpt, *DR.floor_and_wall())
    dev = mcpt.Device(sc, 0)
    E = np.ones((H, W, 3)); E[:, W // 2:] = 100.0
    out, own = dev.denoise_lightmap(E, np.full((H, W, 3), 1e6))
    assert (own >= 0).all() and np.abs(out / E - 1.0).max() <= 1e-12
    dev.close()
    sc.close()


def _device_form(mcpt, dev, uv, E, S, stream, alias=False, **kw):
    """mcpt_lightmap_denoise_device on `stream`; (out, owner) once the stream has been synchronised"""
    H, W = E.shape[:2]
    n = W * H
    hip_rt.set_device(0)
    hip = hip_rt.hip()
    bufs = [hip_rt.DeviceBuffer(n * 24), hip_rt.DeviceBuffer(n * 24), hip_rt.DeviceBuffer(n * 24), hip_rt.DeviceBuffer(n * 4)]
    d_uv = hip_rt.DeviceBuffer(uv.nbytes) if uv is not None else None
    for b, a in ((bufs[0], E), (bufs[1], S), (d_uv, uv)):
        if b is not None:
            a = np.ascontiguousarray(a, dtype=np.float64)
            hip_rt.check(hip.hipMemcpy(b.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes, 1))
    d_out = bufs[0] if alias else bufs[2]
    dp = mcpt.LightmapDenoiseParams(W, H, kw.get("iterations", 5), kw.get("dilate", 0), kw.get("sigma_l", 0.0), kw.get("sigma_p", 0.0),
                                    (C.c_int32 * 2)(0, 0))
    rc = mcpt.lib().mcpt_lightmap_denoise_device(dev._h, d_uv.ptr if d_uv else None, C.byref(dp), bufs[0].ptr, bufs[1].ptr, d_out.ptr, bufs[3].ptr,
                                                 stream.h)
    assert rc == 0, mcpt.lib().mcpt_last_error()
    out, own = np.zeros((H, W, 3)), np.zeros((H, W), dtype=np.int32)
    d_out.to_host_async(out, stream.h)
    bufs[3].to_host_async(own, stream.h)
    stream.synchronize()
    for b in bufs + ([d_uv] if d_uv else []):
        b.free()
    return out, own


def test_forms_aliasing_and_repeats(mcpt, soup):
    """Two calls give the same bits; the device form on a side stream is the host form; out3 aliased to irradiance3 is the unaliased call"""
    sc, dev, uv, g = soup
    stream = hip_rt.Stream()
    for (W, H), kw in (((67, 41), dict(iterations=5, dilate=0)), ((257, 130), dict(iterations=3, dilate=3)), ((67, 41), dict(iterations=0, dilate=2)),
                       ((3, 5), dict(iterations=10, dilate=1, sigma_l=4.0))):
        E, S = _maps(W, H, 15)
        a = dev.denoise_lightmap(E, S, **kw)
        b = dev.denoise_lightmap(E, S, **kw)
        assert _same(a[0], b[0]) and np.array_equal(a[1], b[1])
        for alias in (False, True):
            for chart in (None, uv):
                d = _device_form(mcpt, dev, chart, E, S, stream, alias=alias, **kw)
                assert _same(d[0], a[0]) and np.array_equal(d[1], a[1]), (W, H, kw, alias)
    stream.destroy()


def test_neighbours_and_the_shared_workspace(mcpt):
    """A live progressive handle does not notice a call; a bake after a denoise and a denoise after a bake give what each gives alone"""
    sc, uv = _scene_and_chart(mcpt, "veach-mis")
    dev = mcpt.Device(sc, 0)
    stream = hip_rt.Stream()
    E, S = _maps(128, 128, 16)
    E2, S2 = _maps(64, 64, 17)
    bake_alone = dev.bake_lightmap(128, 128, 4, uv=uv, seed=21, dilate=3)
    runs = []
    for interrupted in (False, True):
        pr = dev.progressive(16, seed=4)
        pr.step(4)
        if interrupted:
            dev.denoise_lightmap(E, S, uv=uv, dilate=2)
            _device_form(mcpt, dev, uv, E2, S2, stream, iterations=2)
        pr.step(4)
        runs.append((pr.image(), pr.stderr()))
        pr.close()
    assert _same(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1])
    fresh = mcpt.Device(sc, 0)
    den_alone = fresh.denoise_lightmap(E, S, uv=uv, dilate=2)                    # on a device that has never baked
    fresh.close()
    den_after = dev.denoise_lightmap(E, S, uv=uv, dilate=2)                      # after a bake (and the calls above)
    assert _same(den_after[0], den_alone[0]) and np.array_equal(den_after[1], den_alone[1])
    bake_after = dev.bake_lightmap(128, 128, 4, uv=uv, seed=21, dilate=3)        # after a denoise
    for a, b in zip(bake_after, bake_alone):
        assert _same(a, b) if a.dtype == np.float64 else np.array_equal(a, b)
    # back to back without a wait in between: the device form, then a bake that waits for the event behind it
    small = dev.denoise_lightmap(E2, S2, uv=uv, iterations=2)
    d = _device_form(mcpt, dev, uv, E2, S2, stream, iterations=2)
    assert _same(d[0], small[0]) and np.array_equal(d[1], small[1])
    stream.destroy()
    dev.close()
    sc.close()


def test_updated_geometry(mcpt):
    """After update_vertices the guides are the moved faces': the result is a fresh device's on the moved scene"""
    uv, v, vn, mat = _soup()
    rng = np.random.default_rng(4)
    v2 = v * 1.25 + rng.uniform(-0.05, 0.05, size=v.shape)
    v2[FLAT, 3:6] = v2[FLAT, 0:3]
    v2[FLAT, 6:9] = v2[FLAT, 0:3]
    E, S = _maps(67, 41, 18)
    S = S * 20.0                                                                   # an open luminance stop: the distance stop decides
    sc = _soup_scene(mcpt, uv, v, vn, mat)
    dev = mcpt.Device(sc, 0)
    before = dev.denoise_lightmap(E, S)
    dev.update_vertices(v2)
    sc2 = _soup_scene(mcpt, uv, v2, vn, mat)
    fresh = mcpt.Device(sc2, 0)
    a, b = dev.denoise_lightmap(E, S, dilate=1), fresh.denoise_lightmap(E, S, dilate=1)
    assert _same(a[0], b[0]) and np.array_equal(a[1], b[1])
    want, wown = DR.denoise(E, S, uv, sc2.faces()[0], dilate=1)
    _against_restatement(a[0], a[1], want, wown, "moved")
    assert not _same(dev.denoise_lightmap(E, S)[0], before[0])
    fresh.close()
    sc2.close()
    dev.close()
    sc.close()


def test_a_chart_that_covers_nothing(mcpt):
    uv, v, vn, mat = _soup(flat=False)
    sc = _soup_scene(mcpt, uv, v, vn, mat, with_vt=False)
    dev = mcpt.Device(sc, 0)
    E, S = _maps(16, 16, 19)
    for kw in (dict(), dict(iterations=0), dict(dilate=3)):
        out, own = dev.denoise_lightmap(E, S, **kw)
        assert not _bits(out).any() and (own == -1).all()
    for bad in (NAN, float("inf")):
        uv2 = uv.copy()
        uv2[40, 3] = bad
        with pytest.raises(mcpt.McptError):
            dev.denoise_lightmap(E, S, uv=uv2)
    with pytest.raises(ValueError):
        dev.denoise_lightmap(E, S[:-1])
    dev.close()
    sc.close()


def _rms_rel(E, ref, mask):
    e, r = E[mask], ref[mask]
    rel = np.sqrt(((e - r) ** 2).sum(axis=1)) / np.sqrt((r ** 2).sum(axis=1))
    return float(np.sqrt((rel ** 2).mean()))


def test_effectiveness(mcpt):
    """glassroom with its own vt, 128 x 128, 16 samples per texel, the defaults, against a 4096-sample bake of another seed (6b / 6c's
    method): RMS of |E - E_ref| / |E_ref| over the covered texels with E_ref > 0.  The filter must help, and help as much as DESIGN 6p
    recorded (times 1.25); the mean over those texels must not shift by more than recorded (times 1.25)."""
    sc, uv = _scene_and_chart(mcpt, "glassroom")
    dev = mcpt.Device(sc, 0)
    ref, _, _, rown = dev.bake_lightmap(128, 128, 4096, seed=1234)
    lit = (rown >= 0) & (ref > 0).all(axis=2)
    print("covered %d, covered and lit %d of %d texels" % ((rown >= 0).sum(), lit.sum(), rown.size))
    assert lit.sum() >= rown.size // 2
    E, S, _, own = dev.bake_lightmap(128, 128, 16, seed=7)
    out, down = dev.denoise_lightmap(E, S)
    assert np.array_equal(down, own) and np.array_equal(own, rown)
    raw, den = _rms_rel(E, ref, lit), _rms_rel(out, ref, lit)
    shift = float(out[lit].mean()) / float(ref[lit].mean()) - 1.0
    print("effectiveness: raw %.4f denoised %.4f ratio %.4f mean shift %+.5f (the raw map's own: %+.5f)" % (
        raw, den, den / raw, shift, float(E[lit].mean()) / float(ref[lit].mean()) - 1.0))
    assert den / raw < 1.0
    assert den / raw <= PIN_RATIO and abs(shift) <= PIN_SHIFT, (den / raw, shift)
    dev.close()
    sc.close()
