"""GPU: lightmap baking (mcpt_lightmap_texels, mcpt_bake_lightmap*).  Coverage and the texel list are the numpy restatement's
(tests/lightmap_ref.py: every texel against every face), exactly; A LIGHTMAP IS, BIT FOR BIT, THE HEMISPHERE QUERY OF ITS OWN TEXEL LIST
(Device.irradiance, which tests/test_gpu_query_oracle.py holds to the oracle), under every seam of the integrator; a texel's samples are
keyed by the texel; the dilation is the restatement's; a known irradiance; both forms; updated geometry."""
import ctypes as C
import os

import numpy as np
import pytest

import hip_rt
import light_scenes
import lightmap_ref as R
import query_ref
from conftest import SCENES, extra_scene_dir
from test_gpu_query import KNOBS, SEAM_CONFIGS

pytestmark = pytest.mark.gpu

ZERO_VN = 12                    # a face of the generated scene whose three vertex normals are zero: its texels take the face normal
FLAT = R.OVERLAP_A              # ... and one whose three vertices coincide: no geometric normal, so it is skipped
BLACK = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0]
GREY = [0.7, 0.7, 0.7, 0.0, 0.0, 0.0, 1.0, 1.0]
CAMERA = ([0.0, 0.5, 5.0], [0.0, 0.5, 0.0], [0.0, 1.0, 0.0], 60.0, 64, 36)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _soup(flat=True, seed=1):
    """the arrays of a scene of 211 random triangles charted by the shared chart: faces 0 and 1 emit, ZERO_VN has no vertex normals and,
    with `flat`, FLAT no extent"""
    uv = R.shared_chart()
    n = uv.shape[0]
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1.0, 1.0, size=(n, 9))
    if flat:
        v[FLAT, 3:6] = v[FLAT, 0:3]
        v[FLAT, 6:9] = v[FLAT, 0:3]
    vn = rng.normal(size=(n, 9))
    vn[ZERO_VN] = 0.0
    mat = np.ones(n, dtype=np.int32)
    mat[:2] = 0
    return uv, v, vn, mat


def _soup_scene(mcpt, uv, v, vn, mat, with_vt=True):
    return mcpt.Scene.from_arrays(v, vn, mat, np.array([BLACK, GREY]), [0], [[3.0, 3.0, 3.0]], *CAMERA, vt=uv if with_vt else None)


@pytest.fixture(scope="module")
def soup(mcpt):
    """(scene, device, chart, faces' 27 doubles) of the generated scene, shared by the tests that only read it"""
    uv, v, vn, mat = _soup()
    sc = _soup_scene(mcpt, uv, v, vn, mat)
    dev = mcpt.Device(sc, 0)
    yield sc, dev, uv, sc.faces()[0]
    dev.close()
    sc.close()


@pytest.mark.parametrize("size", [(1, 1), (3, 5), (64, 64), (257, 130)], ids=lambda s: "%dx%d" % s)
def test_coverage_and_list_are_the_restatement(mcpt, soup, size):
    """owner exactly; texels ascending; q6 bit for bit (fp64 division is IEEE on the device)"""
    W, H = size
    sc, dev, uv, g = soup
    v9, vn9, nrm = g[:, 0:9], g[:, 9:18], g[:, 24:27]
    assert not R.normal_ok(nrm[FLAT]) and R.normal_ok(np.delete(nrm, FLAT, axis=0)).all()
    owner, texels, q6 = dev.lightmap_texels(W, H)
    want = R.raster(uv, W, H, nrm)
    assert owner.shape == (H, W) and np.array_equal(owner, want)
    assert not (owner == FLAT).any()
    assert np.array_equal(texels, np.flatnonzero(owner.reshape(-1) >= 0)) and (texels.size < 2 or np.all(np.diff(texels) > 0))
    w_texels, w_q6 = R.texel_list(want, uv, v9, vn9, nrm)
    assert np.array_equal(texels, w_texels)
    assert q6.shape == w_q6.shape
    bad = np.flatnonzero((_bits(q6) != _bits(w_q6)).any(axis=1))
    assert bad.size == 0, "%d of %d entries differ from the restatement, first at texel %d: %r against %r" % (
        bad.size, texels.size, texels[bad[0]], q6[bad[0]], w_q6[bad[0]])
    # uv=None is the scene's own vt
    o2, t2, q2 = dev.lightmap_texels(W, H, uv=uv)
    assert np.array_equal(o2, owner) and np.array_equal(t2, texels) and _same(q2, q6)
    if size == (64, 64):
        # the flat face's texels went to the next claimant, or to nobody: with a normal it would have owned some
        lost = R.covers(uv[FLAT], W, H)
        assert lost.any() and (R.raster(uv, W, H) == FLAT).any() and (owner[lost] != FLAT).all()
        assert (owner[lost] == -1).any() or (owner[lost] > FLAT).any()
        # the face without vertex normals carries its face normal
        mine = owner.reshape(-1)[texels] == ZERO_VN
        assert mine.any() and _same(q6[mine, 3:], np.tile(nrm[ZERO_VN], (mine.sum(), 1)))
        assert (owner == R.QUAD_LOW).any() and (owner == R.QUAD_HIGH).any()


def test_coverage_is_the_host_rasters_where_every_face_has_a_normal(mcpt):
    uv, v, vn, mat = _soup(flat=False)
    # the chart as the caller's, on a scene created without vt: uv=None then covers nothing, which is not an error
    sc = _soup_scene(mcpt, uv, v, vn, mat, with_vt=False)
    dev = mcpt.Device(sc, 0)
    for W, H in ((64, 64), (257, 130), (5, 3)):
        owner, texels, q6 = dev.lightmap_texels(W, H, uv=uv)
        assert np.array_equal(owner, mcpt.lightmap_raster(uv, W, H))
        o0, t0, q0 = dev.lightmap_texels(W, H)
        assert (o0 == -1).all() and t0.size == 0 and q0.shape == (0, 6)
    E, err, hits, own = dev.bake_lightmap(16, 16, 4, dilate=3)
    assert not E.any() and not err.any() and not hits.any() and (own == -1).all() and not np.signbit(E).any()
    for bad in (float("nan"), float("inf")):
        uv2 = uv.copy()
        uv2[40, 3] = bad
        with pytest.raises(mcpt.McptError):
            dev.bake_lightmap(16, 16, 4, uv=uv2)
        with pytest.raises(mcpt.McptError):
            dev.lightmap_texels(16, 16, uv=uv2)
    with pytest.raises(ValueError):
        dev.bake_lightmap(16, 16, 4, uv=uv[:-1])
    dev.close()
    sc.close()


def _check_bake(dev, W, H, uv, spp, seed, base, flags, stats=None):
    """bake_lightmap(dilate=0) is, at the covered texels, Device.irradiance of the map's own texel list, and +0.0 / +0.0 / 0 / -1 elsewhere"""
    owner, texels, q6 = dev.lightmap_texels(W, H, uv=uv)
    assert texels.size > 0
    E, err, hits, own = dev.bake_lightmap(W, H, spp, uv=uv, seed=seed, sample_base=base, flags=flags, stats=stats)
    qE, qerr, qhits = dev.irradiance(q6[:, :3], q6[:, 3:], spp, seed, ids=texels, sample_base=base, flags=flags)
    wE, werr, whits = R.scatter((H, W), texels, qE, qerr, qhits)
    assert np.array_equal(own, owner)
    bad = int((_bits(E) != _bits(wE)).sum()), int((_bits(err) != _bits(werr)).sum())
    assert bad == (0, 0), "%d irradiance and %d stderr channels differ from the query of the map's own list" % bad
    assert np.array_equal(hits, whits)
    if stats is not None:
        assert stats.rays_primary == texels.size * spp and stats.samples == texels.size * spp
    return E, hits, texels


def _scene_and_chart(mcpt, name):
    if name == "glassroom":                                 # its textured faces carry vt
        return mcpt.Scene(extra_scene_dir(), name, width=64, height=36), None
    sc = mcpt.Scene(SCENES, name, width=64, height=36)      # veach-mis has none: cells of 2 texels are the smallest a 128 x 128 map allows
    return sc, mcpt.grid_atlas(sc.info.num_faces, 128, 128, pad=0)


@pytest.mark.parametrize("name", ["glassroom", "veach-mis"])
def test_a_lightmap_is_its_query(mcpt, monkeypatch, name):
    """(cornell-box's 15 056 faces need cells of 2 texels in a 246 x 246 map at least, above this suite's 257 x 130: veach-mis stands in)"""
    _env(monkeypatch, {})
    sc, uv = _scene_and_chart(mcpt, name)
    dev = mcpt.Device(sc, 0)
    lit = 0
    for flags in (0, mcpt.RENDER_MEGAKERNEL):
        for base in (0, 2 ** 31 - 9):
            E, hits, texels = _check_bake(dev, 128, 128, uv, 8, 11, base, flags, stats=mcpt.Stats())
            lit += int((E > 0).any(axis=2).sum())
            assert hits.max() <= 8
    assert lit > 100
    dev.close()
    sc.close()


@pytest.mark.parametrize("config", sorted(SEAM_CONFIGS))
def test_a_lightmap_is_its_query_under_every_seam(mcpt, monkeypatch, config):
    env, mode, flags = SEAM_CONFIGS[config]
    _env(monkeypatch, env)
    sc, uv = _scene_and_chart(mcpt, "veach-mis")
    dev = mcpt.Device(sc, 0)
    if mode:
        dev.set_trace_mode(mcpt.TRACE_REFERENCE)
    E, hits, texels = _check_bake(dev, 128, 128, uv, 8, 5, 0, flags)
    assert (E > 0).any()
    dev.close()
    sc.close()


@pytest.fixture(scope="module")
def room_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gpu_lightmap_scenes")) + os.sep
    light_scenes.write(d, "room12", 12, 64, 36)
    return d


@pytest.mark.parametrize("variant", ["sky", "one", "tree"])
def test_a_lightmap_is_its_query_in_every_path_variant(mcpt, monkeypatch, room_dir, variant):
    _env(monkeypatch, {})
    if variant == "sky":
        sc, uv = _scene_and_chart(mcpt, "veach-mis")
        W = H = 128
    else:
        sc = mcpt.Scene(room_dir, "room12", width=64, height=36)
        W = H = 64
        uv = mcpt.grid_atlas(sc.info.num_faces, W, H)
    dev = mcpt.Device(sc, 0)
    if variant == "sky":
        dev.set_environment((0.3, 0.6, 1.1), 1.5)
    else:
        dev.set_light_sampling(variant)
    for flags in (0, mcpt.RENDER_MEGAKERNEL):
        E, hits, texels = _check_bake(dev, W, H, uv, 8, 77, 0, flags)
        assert (E > 0).any()
        if variant == "sky":
            assert (hits.reshape(-1)[texels] < 8).any()          # some rays do leave the scene
    dev.close()
    sc.close()


def test_keys_are_the_texels(mcpt, monkeypatch):
    """Half of the faces moved out of the map: the texels that remain keep their values bit for bit"""
    _env(monkeypatch, {})
    sc, uv = _scene_and_chart(mcpt, "veach-mis")
    dev = mcpt.Device(sc, 0)
    E, err, hits, own = dev.bake_lightmap(128, 128, 8, uv=uv, seed=3)
    moved = uv.copy()
    moved[1::2] += 5.0
    E2, err2, hits2, own2 = dev.bake_lightmap(128, 128, 8, uv=moved, seed=3)
    kept = own2 >= 0
    assert kept.any() and (own[kept] % 2 == 0).all() and np.array_equal(kept, (own >= 0) & (own % 2 == 0))
    assert np.array_equal(own2[kept], own[kept]) and (own2[~kept] == -1).all()
    assert _same(E2[kept], E[kept]) and _same(err2[kept], err[kept]) and np.array_equal(hits2[kept], hits[kept])
    assert (E[kept] > 0).any()
    assert not E2[~kept].any() and not err2[~kept].any() and not hits2[~kept].any()
    dev.close()
    sc.close()


def _quad(x0, x1, z0, z1, y, up):
    a, b, c, d = [x0, y, z0], [x1, y, z0], [x1, y, z1], [x0, y, z1]
    return [a + c + b, a + d + c] if up else [a + b + c, a + c + d]


def _lamp_scene(mcpt, chart):
    """test_known_irradiance's lamp (tests/test_gpu_query.py) -- a square of side 2, radiance 3, at height 1, facing down -- over a black
    floor of +-2; `chart` is the two floor triangles' (faces 2 and 3), the lamp's own two cover nothing"""
    v = np.array(_quad(-1, 1, -1, 1, 1.0, False) + _quad(-2, 2, -2, 2, 0.0, True), dtype=np.float64)
    vn = np.concatenate([np.tile([0.0, -1.0, 0.0], (2, 3)), np.tile([0.0, 1.0, 0.0], (2, 3))])
    uv = np.concatenate([np.zeros((2, 6)), np.asarray(chart, dtype=np.float64)])
    return mcpt.Scene.from_arrays(v, vn, np.array([0, 0, 1, 1], dtype=np.int32), np.array([BLACK, BLACK]), [0], [[3.0, 3.0, 3.0]], *CAMERA, vt=uv)


@pytest.mark.parametrize("rounds", [1, 2, 64])
def test_dilation_is_the_restatement(mcpt, monkeypatch, rounds):
    """A 257 x 130 map with a one-texel island (face 2, a tiny chart triangle about the centre of texel (100, 65)), a chart that touches
    the border (face 3, in the corner at the origin) and, right of x = 164, a region that 64 rounds do not reach"""
    _env(monkeypatch, {})
    W, H = 257, 130
    cx, cy = 100.5 / W, 65.5 / H
    island = [cx - 0.3 / W, cy - 0.3 / H, cx + 0.4 / W, cy - 0.2 / H, cx - 0.1 / W, cy + 0.4 / H]
    corner = [0.0, 0.0, 12.0 / W, 0.0, 0.0, 9.0 / H]
    sc = _lamp_scene(mcpt, [island, corner])
    dev = mcpt.Device(sc, 0)
    E0, err0, hits0, own0 = dev.bake_lightmap(W, H, 64, seed=9)
    assert (own0 == 2).sum() == 1 and own0[65, 100] == 2 and (E0[65, 100] > 0).all()
    assert own0[0, 0] == 3 and (own0 == 3).sum() > 20 and set(np.unique(own0)) == {-1, 2, 3}
    E, err, hits, own = dev.bake_lightmap(W, H, 64, seed=9, dilate=rounds)
    wE, wown = R.dilate(E0, own0, rounds)
    assert np.array_equal(own, wown)
    bad = int((_bits(E) != _bits(wE)).sum())
    assert bad == 0, "%d channels differ from the restatement after %d rounds" % (bad, rounds)
    assert _same(err, err0) and np.array_equal(hits, hits0)                      # stderr and hits are untouched
    # owner encodes the rounds: the island's ring of round r is the square of radius r about it
    assert np.array_equal(np.unique(own[own < -1]), np.arange(-1 - rounds, -1))
    assert (own == -1).any() and (own[:, 165:] == -1).all()
    for r in (1, rounds):
        if 65 + r < H:
            assert own[65 + r, 100 + r] == -1 - r and _same(E[65 + r, 100 + r], E0[65, 100])
    filled = own < -1
    assert not err[filled].any() and not hits[filled].any()
    dev.close()
    sc.close()


def test_known_irradiance(mcpt, monkeypatch):
    """The floor of +-2 charted onto an 8 x 8 map, 4096 samples per texel: every one of the 64 texels holds |E - 3 pi F| <= 6 E_stderr, F the
    point-to-parallel-rectangle form factor at the texel's own position -- the bar of tests/test_gpu_query.py's test of the same name.
    The floor ends at +-2 so that the closed form alone says every texel sees the lamp often enough: 4096 F >= 50 at all 64 centres."""
    _env(monkeypatch, {})
    W = H = 8
    sc = _lamp_scene(mcpt, [[0.0, 0.0, 1.0, 1.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0, 1.0, 1.0]])     # a -> (0, 0), b -> (1, 0), c -> (1, 1), d -> (0, 1)
    dev = mcpt.Device(sc, 0)
    owner, texels, q6 = dev.lightmap_texels(W, H)
    assert np.array_equal(texels, np.arange(64)) and set(np.unique(owner)) == {2, 3}
    pu, pv = R.centres(W, H)
    want_xz = np.stack(np.meshgrid(-2.0 + 4.0 * pu, -2.0 + 4.0 * pv), axis=-1).reshape(-1, 2)
    np.testing.assert_allclose(q6[:, [0, 2]], want_xz, rtol=0, atol=1e-14)
    assert not q6[:, [1, 3, 5]].any() and np.abs(q6[:, 4] - 1.0).max() <= 4e-16       # (the three weights sum to 1 within rounding)
    F = np.array([query_ref.square_form_factor(x, z, 1.0, 1.0) for x, z in q6[:, [0, 2]]]).reshape(H, W)
    assert (4096 * F >= 50).all(), (4096 * F).min()
    E, err, hits, own = dev.bake_lightmap(W, H, 4096, seed=2024)
    assert (hits > 0).all() and np.array_equal(own, owner)
    assert (err > 0).all()
    sigma = np.abs(E - 3.0 * np.pi * F[..., None]) / err
    print("known irradiance: |E - 3 pi F| / E_stderr per texel =\n", np.round(sigma[..., 0], 2))
    assert np.all(np.abs(E - 3.0 * np.pi * F[..., None]) <= 6.0 * err), sigma.max()
    assert _same(E[..., 0], E[..., 1]) and _same(E[..., 0], E[..., 2])
    dev.close()
    sc.close()


def _device_form(mcpt, dev, W, H, uv, spp, seed, dilate, flags, stream):
    """mcpt_bake_lightmap_device with stats == NULL on `stream`; the four maps once the stream has been synchronised"""
    n = W * H
    hip_rt.set_device(0)
    d_uv = hip_rt.DeviceBuffer(uv.nbytes) if uv is not None else None
    if uv is not None:
        hip_rt.check(hip_rt.hip().hipMemcpy(d_uv.ptr, uv.ctypes.data_as(C.c_void_p), uv.nbytes, 1))
    bufs = [hip_rt.DeviceBuffer(n * 24), hip_rt.DeviceBuffer(n * 24), hip_rt.DeviceBuffer(n * 4), hip_rt.DeviceBuffer(n * 4)]
    lp = mcpt.LightmapParams(W, H, spp, 0, seed, flags, dilate, (C.c_int32 * 2)(0, 0))
    rc = mcpt.lib().mcpt_bake_lightmap_device(dev._h, d_uv.ptr if d_uv else None, C.byref(lp), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, None,
                                              stream.h)
    assert rc == 0, mcpt.lib().mcpt_last_error()
    out = [np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W), dtype=np.int32), np.zeros((H, W), dtype=np.int32)]
    for b, o in zip(bufs, out):
        b.to_host_async(o, stream.h)
    stream.synchronize()
    for b in bufs + ([d_uv] if d_uv else []):
        b.free()
    return out


def test_forms_and_neighbours(mcpt, monkeypatch):
    """The device form on a side stream is the host form; a live progressive handle does not notice a bake"""
    _env(monkeypatch, {})
    sc, uv = _scene_and_chart(mcpt, "veach-mis")
    dev = mcpt.Device(sc, 0)
    stream = hip_rt.Stream()
    for dilate, flags in ((0, 0), (3, mcpt.RENDER_MEGAKERNEL)):
        host = dev.bake_lightmap(128, 128, 4, uv=uv, seed=21, dilate=dilate, flags=flags)
        device = _device_form(mcpt, dev, 128, 128, uv, 4, 21, dilate, flags, stream)
        assert _same(device[0], host[0]) and _same(device[1], host[1])
        assert np.array_equal(device[2], host[2]) and np.array_equal(device[3], host[3])
        assert (host[0] > 0).any() and ((host[3] < -1).any() == (dilate > 0))
    runs = []
    for interrupted in (False, True):
        pr = dev.progressive(16, seed=4)
        pr.step(4)
        if interrupted:
            dev.bake_lightmap(128, 128, 3, uv=uv, seed=4, dilate=2)
            _device_form(mcpt, dev, 64, 64, uv, 2, 9, 0, mcpt.RENDER_MEGAKERNEL, stream)
            dev.lightmap_texels(64, 64, uv=uv)
        pr.step(4)
        runs.append((pr.image(), pr.stderr()))
        pr.close()
    assert _same(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1])
    stream.destroy()
    dev.close()
    sc.close()


def test_updated_geometry(mcpt, monkeypatch):
    """After update_vertices the texel positions are the new ones and the bake is a fresh device's"""
    _env(monkeypatch, {})
    uv, v, vn, mat = _soup()
    rng = np.random.default_rng(4)
    v2 = v * 1.25 + rng.uniform(-0.05, 0.05, size=v.shape)
    v2[FLAT, 3:6] = v2[FLAT, 0:3]
    v2[FLAT, 6:9] = v2[FLAT, 0:3]
    sc = _soup_scene(mcpt, uv, v, vn, mat)
    dev = mcpt.Device(sc, 0)
    before = dev.lightmap_texels(64, 64)
    dev.update_vertices(v2)
    sc2 = _soup_scene(mcpt, uv, v2, vn, mat)
    fresh = mcpt.Device(sc2, 0)
    g = sc2.faces()[0]
    owner, texels, q6 = dev.lightmap_texels(64, 64)
    w_texels, w_q6 = R.texel_list(R.raster(uv, 64, 64, g[:, 24:27]), uv, g[:, 0:9], g[:, 9:18], g[:, 24:27])
    assert np.array_equal(owner, before[0]) and np.array_equal(texels, w_texels) and _same(q6, w_q6)
    assert not _same(q6[:, :3], before[2][:, :3])
    for flags in (0, mcpt.RENDER_MEGAKERNEL):
        a = dev.bake_lightmap(64, 64, 4, seed=6, dilate=1, flags=flags)
        b = fresh.bake_lightmap(64, 64, 4, seed=6, dilate=1, flags=flags)
        assert _same(a[0], b[0]) and _same(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
        assert (a[0] > 0).any()
    fresh.close()
    sc2.close()
    dev.close()
    sc.close()
