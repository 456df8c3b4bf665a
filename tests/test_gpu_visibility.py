"""GPU: probe visibility (mcpt_query_visibility*, mcpt_bake_volume_visibility*, mcpt_volume_irradiance_visible*).  A bake is its parts bit
for bit -- the probe query's own rays (sh_probe_rays), the closest-hit entry (ray_intersect), the scene's face normals and the numpy fold
(tests/visibility_ref.py) -- at every sample count around a wave's 64, every map size, both trace modes and engines and any chunking; the
lookup kernel is the host form and the restatement; probes inside a closed body are found by the winding alone; a lit room no longer
leaks through the wall into a dark one; progressive handles and the volume bake are left as they were."""
import ctypes as C
import os

import numpy as np
import pytest

import visibility_ref
import volume_cases as VC
from conftest import SCENES
from test_gpu_query import KNOBS
from test_visibility_cpu import _dmax, _ref, moments_for

pytestmark = pytest.mark.gpu

W, H = 64, 36
COUNTS = sorted(VC.GRIDS)
INT_MAX = 2 ** 31 - 1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _bounds(dev):
    box, _ = dev.bvh_nodes()
    return np.minimum(box[0, :3], box[0, 3:]), np.maximum(box[0, :3], box[0, 3:])


def _inside_grid(mcpt, dev, counts, clamp_zero=False):
    """a grid over the middle 80 % of the scene's bounds (test_gpu_volume.py's recipe)"""
    lo, hi = _bounds(dev)
    c = np.array(counts)
    spacing = 0.8 * (hi - lo) / np.maximum(c - 1, 1)
    origin = lo + 0.1 * (hi - lo) if (c > 1).all() else lo + (hi - lo) * np.where(c > 1, 0.1, 0.37)
    return mcpt.volume_grid(origin, spacing, counts, clamp_zero=clamp_zero)


def _device(mcpt, env=None):
    saved = {k: os.environ.pop(k) for k in KNOBS if k in os.environ}
    os.environ.update(env or {})
    try:
        sc = mcpt.Scene(SCENES, "cornell-box", width=W, height=H)
        dev = mcpt.Device(sc, 0)
        if env and "MCPT_TRACE_ENGINE" in env:
            assert sc.trace_engine() == env["MCPT_TRACE_ENGINE"]            # (the knobs are read while the device is made)
    finally:
        for k in env or {}:
            os.environ.pop(k, None)
        os.environ.update(saved)
    return sc, dev


@pytest.fixture(scope="module")
def cornell(mcpt):
    sc, dev = _device(mcpt)
    yield dev
    dev.close()
    sc.close()


@pytest.fixture(scope="module")
def face_normals(cornell):
    return np.ascontiguousarray(cornell.scene.faces()[0][:, 24:27])


_PARTS = {}


def _parts(dev, normals, points, ids, seed, base, spp):
    """the traced rays of every probe, once per (list, seed, range): d [n, spp, 3], hit [n, spp], t [n, spp], nrm [n, spp, 3]"""
    key = (points.tobytes(), None if ids is None else np.asarray(ids).tobytes(), seed, base, spp)
    if key not in _PARTS:
        n = points.shape[0]
        the_ids = np.arange(n, dtype=np.int32) if ids is None else np.asarray(ids, dtype=np.int32)
        rays = dev.sh_probe_rays(np.repeat(points, spp, axis=0), seed, np.tile(np.arange(base, base + spp, dtype=np.int64), n).astype(np.int32),
                                 ids=np.repeat(the_ids, spp))
        assert _same(rays[:, :3], np.repeat(points, spp, axis=0))
        face, t, _, _ = dev.ray_intersect(rays)
        hit = face >= 0
        nrm = np.where(hit[:, None], normals[np.maximum(face, 0)], 0.0)
        _PARTS[key] = (rays[:, 3:].reshape(n, spp, 3), hit.reshape(n, spp), t.reshape(n, spp), nrm.reshape(n, spp, 3))
    return _PARTS[key]


def _want(parts, R, max_distance, max_back_fraction):
    d, hit, t, nrm = parts
    out = [visibility_ref.fold(d[i], hit[i], t[i], nrm[i], R, max_distance, max_back_fraction) for i in range(d.shape[0])]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.int32), np.array([o[2] for o in out], dtype=np.int32),
            np.array([o[3] for o in out], dtype=np.uint8))


def _assert_bake(got, want, what):
    m, hits, back, valid = (np.asarray(a) for a in got)
    n = want[0].shape[0]
    bad = int((_bits(m.reshape(want[0].shape)) != _bits(want[0])).sum())
    assert bad == 0, (what, bad)
    assert np.array_equal(hits.reshape(n), want[1]) and np.array_equal(back.reshape(n), want[2]) and np.array_equal(valid.reshape(n), want[3]), what


# ---- 1. the bake is its parts

MAXD, BACKF = 250.0, 0.25       # cornell-box is 550 units wide: some rays are clamped, some are not


@pytest.mark.parametrize("spp", [1, 63, 64, 65])
@pytest.mark.parametrize("counts", [(1, 1, 1), (1, 7, 1), (5, 4, 3)])
def test_a_grid_bake_is_its_parts(mcpt, cornell, face_normals, counts, spp):
    dev = cornell
    g = _inside_grid(mcpt, dev, counts)
    p = mcpt.volume_points(g)
    n = p.shape[0]
    seed = 100 + spp
    for base in (0, INT_MAX - spp):
        parts = _parts(dev, face_normals, p, None, seed, base, spp)
        for R in (1, 2, 8, 16):
            want = _want(parts, R, MAXD, BACKF)
            st = mcpt.Stats()
            got = dev.bake_volume_visibility(g, spp, res=R, max_distance=MAXD, max_back_fraction=BACKF, seed=seed, sample_base=base, stats=st)
            assert got[0].shape == (g.nz, g.ny, g.nx, R * R, 2) and got[1].shape == got[2].shape == got[3].shape == (g.nz, g.ny, g.nx)
            _assert_bake(got, want, (counts, spp, base, R))
            assert st.rays_primary == n * spp and st.samples == n * spp
            # the list form over the grid's points, and any chunking: the same bits
            for ws in (0, spp, 2 * spp + 1):
                lst = dev.probe_visibility(p, spp, res=R, max_distance=MAXD, max_back_fraction=BACKF, seed=seed, sample_base=base, workspace_rays=ws, stats=st)
                _assert_bake(lst, want, (counts, spp, base, R, ws))
                per = min(n, max(1, (ws or 2 ** 22) // spp))                 # whole probes per chunk, at least one
                assert st.launches == -(-n // per) and st.rays_primary == n * spp
        if base == 0:
            # the rays are the probe query's: so are the hits
            assert np.array_equal(got[1].reshape(-1), dev.sh_probes(p, spp, seed=seed)[2])
            moments = got[0].reshape(n, 256, 2)
            assert (moments[:, :, 0] == -1.0).any() or spp >= 256 * 4      # a 16 x 16 map of a few samples has bins without data ...
            some = moments[:, :, 0] >= 0.0
            assert some.any() and moments[some][:, 0].max() <= MAXD and (moments[~some] == [-1.0, 0.0]).all()
            assert (moments[some][:, 1] >= moments[some][:, 0] ** 2 * (1 - 1e-12)).all()
    assert want[1].max() > 0


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_a_list_bake_is_its_parts(mcpt, cornell, face_normals, n):
    """n probes at random points inside the box, under ids that are a permutation"""
    dev = cornell
    lo, hi = _bounds(dev)
    rng = np.random.default_rng(n)
    p = np.ascontiguousarray(lo + (hi - lo) * (0.1 + 0.8 * rng.random((n, 3))))
    ids = rng.permutation(n).astype(np.int32)
    spp, seed = 65, 7
    for the_ids in (None, ids):
        parts = _parts(dev, face_normals, p, the_ids, seed, 3, spp)
        for R in (8, 16):
            want = _want(parts, R, MAXD, BACKF)
            for ws in (0, 3 * spp):
                got = dev.probe_visibility(p, spp, res=R, max_distance=MAXD, max_back_fraction=BACKF, seed=seed, ids=the_ids, sample_base=3, workspace_rays=ws)
                assert got[0].shape == (n, R * R, 2)
                _assert_bake(got, want, (n, the_ids is not None, R, ws))
    if n > 1:
        a = dev.probe_visibility(p, spp, max_distance=MAXD, seed=seed, ids=ids)[0]
        b = dev.probe_visibility(p, spp, max_distance=MAXD, seed=seed)[0]
        assert not _same(a, b)                                              # the ids key the draw
    assert got[1].max() > 0


@pytest.mark.parametrize("engine", ["pool", "vote"])
def test_both_trace_modes_and_engines_give_the_same_bake(mcpt, cornell, face_normals, engine):
    g = _inside_grid(mcpt, cornell, (5, 4, 3))
    p = mcpt.volume_points(g)
    spp, seed = 65, 11
    parts = _parts(cornell, face_normals, p, None, seed, 0, spp)
    sc, dev = _device(mcpt, {"MCPT_TRACE_ENGINE": engine})
    try:
        for mode in (mcpt.TRACE_FAST, mcpt.TRACE_REFERENCE):
            dev.set_trace_mode(mode)
            for R in (8, 16):
                got = dev.bake_volume_visibility(g, spp, res=R, max_distance=MAXD, seed=seed, workspace_rays=7 * spp)
                _assert_bake(got, _want(parts, R, MAXD, BACKF), (engine, mode, R))
    finally:
        dev.close()
        sc.close()


def _upload(hip_rt, a):
    a = np.ascontiguousarray(a)
    b = hip_rt.DeviceBuffer(a.nbytes)
    hip_rt.check(hip_rt.hip().hipMemcpy(b.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes, 1))
    return b


def test_bake_and_lookup_chain_on_one_stream(mcpt, cornell):
    """mcpt_bake_volume_visibility_device on a side stream, its moments and its mask straight into mcpt_volume_irradiance_visible_device on
    the same stream, no host wait in between: the host forms' answers, bit for bit"""
    import hip_rt
    dev, L = cornell, mcpt.lib()
    counts, R, spp, seed = (5, 4, 3), 8, 64, 23
    g = _inside_grid(mcpt, dev, counts)
    n = 60
    maxd = 1.5 * float(np.sqrt(sum(s * s for s in g.spacing)))
    sh = dev.bake_volume(g, 8, seed=seed)[0]
    # (cornell-box winds its walls so that their stored normals point out of the room: every hit counts as one from behind, and only a
    # fraction of 1 keeps the probes.  The mask still travels through the chain.)
    m, hits, back, valid = dev.bake_volume_visibility(g, spp, res=R, max_distance=maxd, max_back_fraction=1.0, seed=seed)
    print("cornell-box: %d of %d hits are back-face hits" % (back.sum(), hits.sum()))
    assert valid.all()
    lo, hi = _bounds(dev)
    rng = np.random.default_rng(2)
    x = lo + (hi - lo) * rng.random((500, 3))
    b = rng.normal(size=(500, 3))
    vis = mcpt.volume_visibility(R, maxd, 0.0, 0.0)
    want_E, want_c = dev.volume_irradiance_visible(g, sh, m, x, b, vis, valid=valid)
    host_E, host_c = mcpt.volume_irradiance_visible_host(g, sh, m, x, b, vis, valid=valid)
    assert _same(want_E, host_E) and np.array_equal(want_c, host_c)
    plain_E, _ = dev.volume_irradiance(g, sh, x, b, valid=valid)
    assert np.abs(plain_E).max() > 0 and not _same(plain_E, want_E)         # the boxes in the room hide probes from receivers
    d_sh, d_q = _upload(hip_rt, sh), _upload(hip_rt, np.concatenate([x, b], axis=1))
    d_m, d_hits, d_back, d_valid = hip_rt.DeviceBuffer(n * R * R * 16), hip_rt.DeviceBuffer(n * 4), hip_rt.DeviceBuffer(n * 4), hip_rt.DeviceBuffer(n)
    d_e, d_c = hip_rt.DeviceBuffer(500 * 24), hip_rt.DeviceBuffer(500 * 4)
    st = hip_rt.Stream()
    vp = mcpt.VisibilityParams(spp, 0, seed, R, 0, maxd, 1.0, 0, (C.c_int32 * 2)(0, 0))
    assert L.mcpt_bake_volume_visibility_device(dev._h, C.byref(g), C.byref(vp), d_m.ptr, d_hits.ptr, d_back.ptr, d_valid.ptr, None, st.h) == 0, L.mcpt_last_error()
    assert L.mcpt_volume_irradiance_visible_device(dev._h, C.byref(g), d_sh.ptr, d_m.ptr, d_valid.ptr, C.byref(vis), d_q.ptr, 500, d_e.ptr, d_c.ptr, st.h) == 0, \
        L.mcpt_last_error()
    E, c, m2 = np.zeros((500, 3)), np.zeros(500, dtype=np.int32), np.zeros((n, R * R, 2))
    h2, b2, v2 = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
    for buf, arr in ((d_e, E), (d_c, c), (d_m, m2), (d_hits, h2), (d_back, b2), (d_valid, v2)):
        buf.to_host_async(arr, st.h)
    st.synchronize()
    assert _same(m2, m.reshape(n, R * R, 2)) and np.array_equal(h2, hits.reshape(-1)) and np.array_equal(b2, back.reshape(-1)) and np.array_equal(v2, valid.reshape(-1))
    assert _same(E, want_E) and np.array_equal(c, want_c) and np.abs(E).max() > 0
    # the list form's device form with only the moments asked for, and n == 0
    d_p = _upload(hip_rt, mcpt.volume_points(g))
    assert L.mcpt_query_visibility_device(dev._h, d_p.ptr, None, n, C.byref(vp), d_m.ptr, None, None, None, None, st.h) == 0, L.mcpt_last_error()
    d_m.to_host_async(m2, st.h)
    st.synchronize()
    assert _same(m2, m.reshape(n, R * R, 2))
    assert L.mcpt_query_visibility_device(dev._h, None, None, 0, C.byref(vp), None, None, None, None, None, st.h) == 0
    assert L.mcpt_volume_irradiance_visible_device(dev._h, C.byref(g), None, None, None, C.byref(vis), None, 0, None, None, st.h) == 0
    assert dev.probe_visibility(np.zeros((0, 3)), 4)[0].shape == (0, 64, 2)
    for buf in (d_sh, d_q, d_m, d_hits, d_back, d_valid, d_e, d_c, d_p):
        buf.free()
    st.destroy()


# ---- 2. the lookup kernel

@pytest.mark.parametrize("counts", COUNTS)
def test_lookup_is_the_host_form_and_the_restatement(mcpt, cornell, counts):
    R = {(1, 1, 1): 1, (1, 7, 1): 3, (5, 4, 3): 8, (33, 17, 9): 16}[counts]
    dmax = _dmax(counts)
    sh, valid, m = VC.coefficients(counts), VC.mask(counts), moments_for(counts, R, dmax)
    x, b = VC.receivers(counts)
    for masked in (False, True):
        for clamp in (False, True):
            for bias, minv in ((0.0, 0.0), (0.05, 1e-3)):
                g, v = VC.grid(mcpt, counts, clamp_zero=clamp), valid if masked else None
                vis = mcpt.volume_visibility(R, dmax, bias, minv)
                want = _ref(counts, sh, m, x, b, R, dmax, bias, minv, v, clamp)
                for n in (1, 63, 64, 65, VC.N):
                    xs, bs = np.roll(x, -7 * n, axis=0)[:n], np.roll(b, -7 * n, axis=0)[:n]
                    E, corners = cornell.volume_irradiance_visible(g, sh, m, xs, bs, vis, valid=v)
                    hE, hc = mcpt.volume_irradiance_visible_host(g, sh, m, xs, bs, vis, valid=v)
                    wE, wc = (np.roll(a, -7 * n, axis=0)[:n] for a in want)
                    bad = int((_bits(E) != _bits(wE)).sum())
                    assert bad == 0, (counts, masked, clamp, bias, n, bad)
                    assert _same(E, hE) and np.array_equal(corners, hc) and np.array_equal(corners, wc), (counts, masked, clamp, bias, n)
    assert np.abs(want[0]).max() > 0


# ---- 3, 4. rooms built by hand

def _box(lo, hi, inward):
    """the twelve triangles of an axis-aligned box whose stored face normals (normalize(cross(v0 - v1, v2 - v0)), the library's rule)
    point inward or outward: v [12, 9], vn [12, 9]"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    v, vn = [], []
    for axis in range(3):
        for side, bound in ((-1.0, lo), (1.0, hi)):
            u, w = (axis + 1) % 3, (axis + 2) % 3
            c = np.zeros((4, 3))
            c[:, axis] = bound[axis]
            c[:, u] = [lo[u], hi[u], hi[u], lo[u]]
            c[:, w] = [lo[w], lo[w], hi[w], hi[w]]
            want = np.zeros(3)
            want[axis] = -side if inward else side
            for tri in ((0, 1, 2), (0, 2, 3)):
                a, b2, c2 = c[tri[0]], c[tri[1]], c[tri[2]]
                if np.dot(np.cross(a - b2, c2 - a), want) < 0:
                    b2, c2 = c2, b2
                v.append(np.concatenate([a, b2, c2]))
                vn.append(np.tile(want, 3))
    return np.array(v), np.array(vn)


def _scene(mcpt, parts, emitter=None, absorber=None):
    """parts: (v, vn) pairs of diffuse grey geometry; emitter: one more pair whose material is a light; absorber: one more that is black"""
    extra = [e for e in (emitter, absorber) if e]
    v = np.concatenate([p[0] for p in parts] + [e[0] for e in extra])
    vn = np.concatenate([p[1] for p in parts] + [e[1] for e in extra])
    n_plain = sum(p[0].shape[0] for p in parts)
    mat = np.zeros(v.shape[0], dtype=np.int32)
    rec = [[0.7, 0.6, 0.5, 0.0, 0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0]]
    lights, radiance = np.zeros(0, dtype=np.int32), np.zeros((0, 3))
    if emitter:
        mat[n_plain:n_plain + emitter[0].shape[0]] = 1
        lights, radiance = np.array([1], dtype=np.int32), np.array([[40.0, 30.0, 20.0]])
    if absorber:
        mat[v.shape[0] - absorber[0].shape[0]:] = 2
    return mcpt.Scene.from_arrays(v, vn, mat, np.array(rec), lights, radiance, [1.0, 1.0, 1.9], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0], 60.0, 32, 18)


def test_probes_inside_a_closed_body_are_invalid(mcpt):
    """a closed room with inward faces around a closed cube with outward faces: from inside the cube every ray hits a back face, from the
    room none does -- by the winding alone, so the counts are exact"""
    sc = _scene(mcpt, [_box((0, 0, 0), (3, 3, 3), inward=True), _box((1, 1, 1), (2, 2, 2), inward=False)])
    nrm = sc.faces()[0][:, 24:27]
    want = np.concatenate([_box((0, 0, 0), (3, 3, 3), True)[1][:, :3], _box((1, 1, 1), (2, 2, 2), False)[1][:, :3]])
    assert np.array_equal(nrm, want)                                        # the stored normals are the ones meant
    dev = mcpt.Device(sc, 0)
    rng = np.random.default_rng(8)
    inside = 1.05 + 0.9 * rng.random((33, 3))
    room = 0.05 + 2.9 * rng.random((400, 3))
    room = room[((room < 0.95) | (room > 2.05)).any(axis=1)][:70]
    p = np.ascontiguousarray(np.concatenate([inside, room]))
    spp = 96
    for R in (8, 16):
        m, hits, back, valid = dev.probe_visibility(p, spp, res=R, max_distance=1.0, seed=5)
        assert np.array_equal(hits, np.full(p.shape[0], spp))
        assert np.array_equal(back[:33], np.full(33, spp)) and np.array_equal(valid[:33], np.zeros(33, dtype=np.uint8))
        assert np.array_equal(back[33:], np.zeros(70, dtype=np.int32)) and np.array_equal(valid[33:], np.ones(70, dtype=np.uint8))
        some = m[:, :, 0] >= 0
        assert m[some][:, 0].max() <= 1.0 and m[:33][some[:33]][:, 0].min() >= 0.05
    # the threshold itself: a fraction of 1 keeps even those
    assert dev.probe_visibility(p, spp, max_distance=1.0, max_back_fraction=1.0, seed=5)[3].all()
    dev.close()
    sc.close()


def test_a_lit_room_does_not_leak_into_a_dark_one(mcpt):
    """Two closed rooms, A over x in [0, 2] with an emitter under its ceiling and B over x in [2.1, 4.1] without light, one probe in each.
    No path from B reaches the light, so B's probe is exactly 0 and whatever the plain lookup gives a receiver in B is leak.  The limit
    E_visible <= 1e-2 E_plain is a condition, not a measurement: from A's probe the wall x = 2 lies at depth 0.45 / d_x, so the bins
    towards the receivers hold mu < 0.5 and var < 6e-4 against delta >= 0.2, a factor near 4e-6 (tests/test_visibility_cpu.py holds the
    restatement to a tenth of the limit on the plane's analytic depth)."""
    quad = np.array([[0.8, 1.9, 0.8], [1.2, 1.9, 0.8], [1.2, 1.9, 1.2], [0.8, 1.9, 1.2]])
    ev, evn = [], []
    for tri in ((0, 1, 2), (0, 2, 3)):
        a, b, c = quad[tri[0]], quad[tri[1]], quad[tri[2]]
        if np.cross(a - b, c - a)[1] > 0:
            b, c = c, b
        ev.append(np.concatenate([a, b, c]))
        evn.append(np.tile([0.0, -1.0, 0.0], 3))
    # The integrator starts every shadow and bounce ray 0.01 along its direction: from a vertex within 0.01 of a room's edge a ray starts
    # outside the room, and from the outside of A's walls a shadow ray starts inside A and reaches the emitter.  A black shell around B,
    # 0.05 off its walls, ends every path that leaves B that way with a throughput of exactly 0; neither probe and no receiver sees it.
    shell = _box((2.05, -0.05, -0.05), (4.15, 2.05, 2.05), inward=True)
    sc = _scene(mcpt, [_box((0, 0, 0), (2, 2, 2), inward=True), _box((2.1, 0, 0), (4.1, 2, 2), inward=True)], emitter=(np.array(ev), np.array(evn)),
                absorber=shell)
    dev = mcpt.Device(sc, 0)
    g = mcpt.volume_grid((1.55, 1.0, 1.0), (1.0, 1.0, 1.0), (2, 1, 1))
    assert np.allclose(mcpt.volume_points(g), [[1.55, 1, 1], [2.55, 1, 1]], rtol=0, atol=1e-15)
    R, spp, maxd = 8, 1024, 1.5
    sh = dev.bake_volume(g, spp, seed=3)[0]
    m, hits, back, valid = dev.bake_volume_visibility(g, spp, res=R, max_distance=maxd, seed=3)
    assert np.array_equal(hits.reshape(-1), [spp, spp]) and np.array_equal(back.reshape(-1), [0, 0]) and valid.all()
    assert np.array_equal(_bits(sh[0, 0, 1]), np.zeros((9, 3), dtype=np.uint64))       # B's probe: exactly +0.0
    assert (sh[0, 0, 0, 0] > 0).all()
    vis = mcpt.volume_visibility(R, maxd, 0.0, 0.0)
    rng = np.random.default_rng(4)
    nB = 200
    xB = np.stack([2.25 + 0.25 * rng.random(nB), 0.9 + 0.2 * rng.random(nB), 0.9 + 0.2 * rng.random(nB)], axis=1)
    bB = np.tile([-1.0, 0.0, 0.0], (nB, 1))
    plain, _ = dev.volume_irradiance(g, sh, xB, bB)
    seen, corners = dev.volume_irradiance_visible(g, sh, m, xB, bB, vis)
    assert (plain > 0).all()                                                # pure leak, in every channel
    ratio = seen / plain
    print("receivers in B: E_visible / E_plain between %.3e and %.3e" % (ratio.min(), ratio.max()))
    assert (seen <= 1e-2 * plain).all()
    assert (corners == 2).all() and (seen >= 0).all()
    # receivers in A, between the probe and the wall: the dark probe behind the wall loses its weight
    xA = np.stack([1.6 + 0.25 * rng.random(nB), 0.9 + 0.2 * rng.random(nB), 0.9 + 0.2 * rng.random(nB)], axis=1)
    plainA, _ = dev.volume_irradiance(g, sh, xA, bB)
    seenA, _ = dev.volume_irradiance_visible(g, sh, m, xA, bB, vis)
    gain = seenA / plainA
    print("receivers in A: E_visible / E_plain between %.4f and %.4f" % (gain.min(), gain.max()))
    assert (plainA > 0).all() and (seenA > plainA).all()
    dev.close()
    sc.close()


# ---- 5. what else lives on the device

def test_progressive_handles_and_volume_bakes_do_not_notice(mcpt, cornell):
    dev = cornell
    g = _inside_grid(mcpt, dev, (5, 4, 3))
    sh = VC.coefficients((5, 4, 3))
    x, b = VC.receivers((5, 4, 3))
    lo, hi = _bounds(dev)
    vis = mcpt.volume_visibility(8, 100.0)
    runs = []
    for interrupted in (False, True):
        pr = dev.progressive(16, seed=4)
        pr.step(4)
        if interrupted:
            m = dev.bake_volume_visibility(g, 5, seed=4, stats=mcpt.Stats())[0]
            dev.probe_visibility(mcpt.volume_points(g), 3, res=16, max_distance=100.0, workspace_rays=3)
            dev.volume_irradiance_visible(g, sh, m, lo + (hi - lo) * np.abs(np.sin(x)), b, vis)
        pr.step(4)
        runs.append((pr.image(), pr.stderr()))
        pr.close()
    assert _same(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1])
    # a plain volume bake right behind a device-form visibility bake of a larger grid, which shares the volume's point list
    import hip_rt
    L = mcpt.lib()
    want = dev.bake_volume(g, 8, seed=19)
    g2 = _inside_grid(mcpt, dev, (6, 5, 4))
    m2 = dev.bake_volume_visibility(g2, 16, seed=2)[0]
    st = hip_rt.Stream()
    d_m = hip_rt.DeviceBuffer(120 * 64 * 16)
    vp = mcpt.VisibilityParams(16, 0, 2, 8, 0, 1.5 * float(np.sqrt(sum(s * s for s in g2.spacing))), 0.25, 0, (C.c_int32 * 2)(0, 0))
    assert L.mcpt_bake_volume_visibility_device(dev._h, C.byref(g2), C.byref(vp), d_m.ptr, None, None, None, None, st.h) == 0, L.mcpt_last_error()
    got = dev.bake_volume(g, 8, seed=19)
    m3 = np.zeros((120, 64, 2))
    d_m.to_host_async(m3, st.h)
    st.synchronize()
    for a, c in zip(got, want):
        assert np.array_equal(a.view(np.uint8), c.view(np.uint8))
    assert _same(m3, m2.reshape(120, 64, 2))
    d_m.free()
    st.destroy()
