"""GPU: adaptive lightmaps (mcpt_bake_lightmap_adaptive*).  AN ADAPTIVE LIGHTMAP IS, BIT FOR BIT, THE ADAPTIVE HEMISPHERE QUERY OF ITS OWN
TEXEL LIST (Device.irradiance_adaptive with ids = texels, which tests/test_gpu_adaptive_query.py holds to the one-shot query), scattered as
a lightmap's, with the counts map beside it; with targets of 0 it is mcpt_bake_lightmap itself; dilation fills what the restatement
(tests/lightmap_ref.py) fills and leaves the counts 0 there; maps that cover one texel or nothing; both forms."""
import ctypes as C

import numpy as np
import pytest

import hip_rt
import lightmap_ref as R
import test_gpu_lightmap as TL

pytestmark = pytest.mark.gpu

SPP, MIN_SPP, REL = 64, 4, 0.2
BOUNDS = (4, 8, 16, 32, 64)
_bits, _same, _env = TL._bits, TL._same, TL._env


def _check_bake(dev, W, H, uv, seed, base, flags, stats=None):
    """bake_lightmap_adaptive(dilate=0) is, at the covered texels, irradiance_adaptive of the map's own texel list with ids = texels, and
    +0.0 / +0.0 / 0 / 0 elsewhere; owner is the coverage's"""
    owner, texels, q6 = dev.lightmap_texels(W, H, uv=uv)
    assert texels.size > 0
    E, err, hits, own, counts = dev.bake_lightmap_adaptive(W, H, SPP, REL, min_spp=MIN_SPP, uv=uv, seed=seed, sample_base=base, flags=flags, stats=stats)
    qE, qerr, qhits, qcounts = dev.irradiance_adaptive(q6[:, :3], q6[:, 3:], SPP, REL, min_spp=MIN_SPP, seed=seed, ids=texels, sample_base=base, flags=flags)
    wE, werr, whits = R.scatter((H, W), texels, qE, qerr, qhits)
    wcounts = np.zeros(W * H, dtype=np.int32)
    wcounts[texels] = qcounts
    assert np.array_equal(own, owner)
    bad = int((_bits(E) != _bits(wE)).sum()), int((_bits(err) != _bits(werr)).sum())
    assert bad == (0, 0), "%d irradiance and %d stderr channels differ from the adaptive query of the map's own list" % bad
    assert np.array_equal(hits, whits) and np.array_equal(counts, wcounts.reshape(H, W))
    assert set(np.unique(counts[own >= 0]).tolist()) <= set(BOUNDS) and not counts[own < 0].any()
    if stats is not None:
        assert stats.samples == int(qcounts.sum()) and stats.rays_primary == stats.samples
    return E, counts, own


@pytest.mark.parametrize("name", ["glassroom", "veach-mis"])
def test_an_adaptive_lightmap_is_its_adaptive_query(mcpt, monkeypatch, name):
    _env(monkeypatch, {})
    sc, uv = TL._scene_and_chart(mcpt, name)
    dev = mcpt.Device(sc, 0)
    for flags in (0, mcpt.RENDER_MEGAKERNEL):
        for base in (0, 2 ** 31 - 1 - 64):
            E, counts, own = _check_bake(dev, 128, 128, uv, 11, base, flags, stats=mcpt.Stats())
            seen = np.unique(counts[own >= 0])
            print("%s flags %d base %d: counts %s" % (name, flags, base, dict(zip(*np.unique(counts[own >= 0], return_counts=True)))))
            assert seen.size >= 2 and (E > 0).any()                  # some texels stop early, some do not
    # targets of 0: the uniform bake itself, every covered texel at spp
    for flags, dilate in ((0, 0), (mcpt.RENDER_MEGAKERNEL, 2)):
        a = dev.bake_lightmap_adaptive(128, 128, 8, 0.0, 0.0, min_spp=2, uv=uv, seed=3, dilate=dilate, flags=flags)
        b = dev.bake_lightmap(128, 128, 8, uv=uv, seed=3, dilate=dilate, flags=flags)
        assert _same(a[0], b[0]) and _same(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
        assert np.array_equal(a[4], np.where(b[3] >= 0, 8, 0))
    dev.close()
    sc.close()


def test_dilation_fills_what_the_restatement_fills(mcpt, monkeypatch):
    _env(monkeypatch, {})
    sc, uv = TL._scene_and_chart(mcpt, "veach-mis")
    dev = mcpt.Device(sc, 0)
    moved = uv.copy()
    moved[1::2] += 5.0                                      # half of the faces out of the map: gutters for the dilation to fill
    E0, err0, hits0, own0, counts0 = dev.bake_lightmap_adaptive(128, 128, SPP, REL, min_spp=MIN_SPP, uv=moved, seed=9)
    E, err, hits, own, counts = dev.bake_lightmap_adaptive(128, 128, SPP, REL, min_spp=MIN_SPP, uv=moved, seed=9, dilate=2)
    wE, wown = R.dilate(E0, own0, 2)
    assert np.array_equal(own, wown)
    bad = int((_bits(E) != _bits(wE)).sum())
    assert bad == 0, "%d channels differ from the restatement after 2 rounds" % bad
    filled = own < -1
    assert filled.any() and (own == -1).any()
    assert _same(err, err0) and np.array_equal(hits, hits0) and np.array_equal(counts, counts0)      # stderr, hits and counts are untouched
    assert not counts[filled].any() and not counts[own == -1].any() and (counts[own >= 0] >= 4).all()
    dev.close()
    sc.close()


def test_a_single_texel_and_an_empty_chart(mcpt, monkeypatch):
    _env(monkeypatch, {})
    sc = TL._lamp_scene(mcpt, [[0.0, 0.0, 1.0, 1.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0, 1.0, 1.0]])
    dev = mcpt.Device(sc, 0)
    st = mcpt.Stats()
    E, err, hits, own, counts = dev.bake_lightmap_adaptive(1, 1, SPP, REL, min_spp=MIN_SPP, seed=2, stats=st)
    assert E.shape == (1, 1, 3) and own[0, 0] in (2, 3) and counts[0, 0] in BOUNDS and (E[0, 0] > 0).all()
    assert st.samples == counts[0, 0]
    owner, texels, q6 = dev.lightmap_texels(1, 1)
    qE, qerr, qhits, qcounts = dev.irradiance_adaptive(q6[:, :3], q6[:, 3:], SPP, REL, min_spp=MIN_SPP, seed=2, ids=texels)
    assert _same(E[0, 0], qE[0]) and _same(err[0, 0], qerr[0]) and hits[0, 0] == qhits[0] and counts[0, 0] == qcounts[0]
    # a chart that covers nothing: no query is launched, the maps are all zero and owner all -1
    nothing = np.zeros((sc.info.num_faces, 6))
    st = mcpt.Stats()
    for dilate in (0, 3):
        E, err, hits, own, counts = dev.bake_lightmap_adaptive(16, 16, SPP, REL, min_spp=MIN_SPP, uv=nothing, dilate=dilate, stats=st)
        assert not E.any() and not err.any() and not hits.any() and not counts.any() and (own == -1).all() and st.samples == 0
    dev.close()
    sc.close()


def _device_form(mcpt, dev, W, H, uv, seed, dilate, flags, stream, with_counts=True):
    """mcpt_bake_lightmap_adaptive_device with stats == NULL on `stream`; the five maps once the stream has been synchronised"""
    n = W * H
    hip_rt.set_device(0)
    d_uv = hip_rt.DeviceBuffer(uv.nbytes)
    hip_rt.check(hip_rt.hip().hipMemcpy(d_uv.ptr, uv.ctypes.data_as(C.c_void_p), uv.nbytes, 1))
    bufs = [hip_rt.DeviceBuffer(n * 24), hip_rt.DeviceBuffer(n * 24), hip_rt.DeviceBuffer(n * 4), hip_rt.DeviceBuffer(n * 4), hip_rt.DeviceBuffer(n * 4)]
    lp = mcpt.LightmapParams(W, H, SPP, 0, seed, flags, dilate, (C.c_int32 * 2)(0, 0))
    ap = mcpt.AdaptiveParams(REL, 0.0, MIN_SPP, 0)
    rc = mcpt.lib().mcpt_bake_lightmap_adaptive_device(dev._h, d_uv.ptr, C.byref(lp), C.byref(ap), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr,
                                                       bufs[4].ptr if with_counts else None, None, stream.h)
    assert rc == 0, mcpt.lib().mcpt_last_error()
    out = [np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W), dtype=np.int32), np.zeros((H, W), dtype=np.int32), np.zeros((H, W), dtype=np.int32)]
    for b, o in zip(bufs, out):
        b.to_host_async(o, stream.h)
    stream.synchronize()
    for b in bufs + [d_uv]:
        b.free()
    return out


def test_the_device_form_is_the_host_form(mcpt, monkeypatch):
    _env(monkeypatch, {})
    sc, uv = TL._scene_and_chart(mcpt, "veach-mis")
    dev = mcpt.Device(sc, 0)
    stream = hip_rt.Stream()
    for dilate, flags in ((0, 0), (3, mcpt.RENDER_MEGAKERNEL)):
        host = dev.bake_lightmap_adaptive(128, 128, SPP, REL, min_spp=MIN_SPP, uv=uv, seed=21, dilate=dilate, flags=flags)
        for with_counts in (True, False):
            device = _device_form(mcpt, dev, 128, 128, uv, 21, dilate, flags, stream, with_counts)
            assert _same(device[0], host[0]) and _same(device[1], host[1])
            assert np.array_equal(device[2], host[2]) and np.array_equal(device[3], host[3])
            assert np.array_equal(device[4], host[4]) if with_counts else not device[4].any()
        assert (host[0] > 0).any() and np.unique(host[4]).size >= 3                  # 0 where nothing is covered, and two counts at least
    stream.destroy()
    dev.close()
    sc.close()
