"""GPU: ambient occlusion (mcpt_query_occlusion*, mcpt_bake_occlusion_lightmap*).  A query is its parts bit for bit -- the irradiance
query's own rays (query_rays, kind "hemisphere"), the closest-hit entry (ray_intersect), the scene's face normals and the numpy fold
(tests/occlusion_ref.py) -- at every list length and sample count around a wave's 64, both ends of the sample range, every falloff, reaches
far under, inside and beyond the scene, any chunking, both trace modes and engines; the device form is the host form; a map is the query
of its own texel list, scattered and dilated by the restatement; scenes whose answer is exact by construction; a floor against a wall is
half open; after an update and under a motion the query is a fresh device's; progressive handles and the visibility bake, whose workspace
the query shares, are left as they were."""
import ctypes as C
import os

import numpy as np
import pytest

import occlusion_ref as OR
import test_gpu_visibility as TV
from conftest import SCENES
from test_gpu_query import KNOBS

pytestmark = pytest.mark.gpu

W, H = 64, 36
INT_MAX = 2 ** 31 - 1
FALLOFFS = ["hard", "linear", "square"]
# cornell-box is 550 units wide: nothing but a corner is nearer than 0.05 or 1.0, about half the rays end inside 250, all inside 1e30
REACHES = [0.05, 1.0, 250.0, 1e30]
KEYS = ("ao", "stderr", "bent", "hits", "back")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _differing(got, want):
    """the words in which two answers differ, over all five outputs"""
    return sum(int((_bits(got[k]).reshape(-1) != _bits(want[k]).reshape(-1)).sum()) for k in ("ao", "stderr", "bent")) + sum(
        int((np.asarray(got[k]).reshape(-1) != np.asarray(want[k]).reshape(-1)).sum()) for k in ("hits", "back"))


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


def _chart_of(scene):
    return np.ascontiguousarray(scene.faces()[0][:, 18:24]) * 0.15 + 0.2


@pytest.fixture(scope="module")
def cornell(mcpt):
    sc, dev = _device(mcpt)
    yield dev
    dev.close()
    sc.close()


@pytest.fixture(scope="module")
def chart(mcpt, cornell):
    """a chart for cornell-box that leaves a margin: the scene's own vt, which tile the whole unit square several times over, shrunk into
    the part of it beyond (0.2, 0.2)"""
    return _chart_of(cornell.scene)


@pytest.fixture(scope="module")
def surface(cornell, chart):
    """the surface points of cornell-box the tests take their lists from: lightmap_texels' list at 64 x 64"""
    owner, texels, q6 = cornell.lightmap_texels(64, 64, uv=chart)
    assert texels.size >= 65 * 7
    return q6


@pytest.fixture(scope="module")
def face_normals(cornell):
    return np.ascontiguousarray(cornell.scene.faces()[0][:, 24:27])


_PARTS = {}


def _parts(dev, normals, q6, ids, seed, base, spp):
    """the traced rays of every entry, once per (list, seed, range): rays [n * spp, 6], hit [n * spp], t [n * spp], nrm [n * spp, 3]"""
    key = (q6.tobytes(), None if ids is None else np.asarray(ids).tobytes(), seed, base, spp)
    if key not in _PARTS:
        n = q6.shape[0]
        the_ids = np.arange(n, dtype=np.int32) if ids is None else np.asarray(ids, dtype=np.int32)
        rays = dev.query_rays(np.repeat(q6, spp, axis=0), seed, np.tile(np.arange(base, base + spp, dtype=np.int64), n).astype(np.int32),
                              kind="hemisphere", ids=np.repeat(the_ids, spp))
        face, t, _, _ = dev.ray_intersect(rays)
        hit = face >= 0
        _PARTS[key] = (rays, hit, t, np.where(hit[:, None], normals[np.maximum(face, 0)], 0.0))
    return _PARTS[key]


def _entries(surface, n, spp):
    """n of the surface points, other ones for every (n, spp)"""
    at = (np.arange(n) * 7 + 13 * n + spp) % surface.shape[0]
    return np.ascontiguousarray(surface[at])


# ---- 1. the query is its parts

@pytest.mark.parametrize("spp", [1, 63, 64, 65])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_a_query_is_its_parts(mcpt, cornell, surface, face_normals, n, spp):
    dev = cornell
    q6 = _entries(surface, n, spp)
    perm = np.random.default_rng(n * 100 + spp).permutation(n).astype(np.int32)
    seed = 1000 + n
    worst = 0
    for ids, base in ((None, 0), (perm, 0), (perm, INT_MAX - spp)):
        parts = _parts(dev, face_normals, q6, ids, seed, base, spp)
        for falloff in FALLOFFS:
            for reach in REACHES:
                want = OR.fold(q6, *parts, spp, reach, falloff)
                # any chunking gives the same bits; the chunks are read back through the launches
                for ws in (0, spp, 2 * spp + 1) if reach in (1.0, 250.0) else (0,):
                    st = mcpt.Stats()
                    got = dev.occlusion(q6[:, :3], q6[:, 3:], spp, reach, falloff, seed=seed, ids=ids, sample_base=base, workspace_rays=ws, stats=st)
                    bad = _differing(got, want)
                    worst = max(worst, bad)
                    assert bad == 0, (n, spp, ids is not None, base, falloff, reach, ws, bad)
                    assert got["hits"].dtype == np.int32 and got["bent"].shape == (n, 3)
                    assert st.rays_primary == n * spp and st.samples == n * spp
                    per = min(n, max(1, (ws or 2 ** 22) // spp))               # whole entries per chunk, at least one
                    assert st.launches == -(-n // per)
                    if spp >= 2:
                        assert st.launches == {0: 1, spp: n, 2 * spp + 1: -(-n // 2)}[ws]
        if base == 0 and ids is None:
            # the rays are the irradiance query's: with every hit near, so are the hit counts
            assert np.array_equal(dev.occlusion(q6[:, :3], q6[:, 3:], spp, 1e30, seed=seed)["hits"], dev.irradiance(q6[:, :3], q6[:, 3:], spp, seed=seed)[2])
    print("n %d spp %d: at most %d words differ from the parts' fold" % (n, spp, worst))
    if n > 1 and spp > 1:
        a = dev.occlusion(q6[:, :3], q6[:, 3:], spp, 250.0, "linear", seed=seed, ids=perm)
        b = dev.occlusion(q6[:, :3], q6[:, 3:], spp, 250.0, "linear", seed=seed)
        assert _differing(a, b) > 0                                         # the ids key the draw
        assert 0.0 <= a["ao"].min() and a["ao"].max() <= 1.0 and a["hits"].max() > 0 and a["stderr"].max() > 0


@pytest.mark.parametrize("engine", ["pool", "vote"])
def test_both_trace_modes_and_engines_give_the_same_query(mcpt, cornell, surface, face_normals, engine):
    n, spp, seed = 65, 65, 11
    q6 = _entries(surface, n, spp)
    parts = _parts(cornell, face_normals, q6, None, seed, 0, spp)
    sc, dev = _device(mcpt, {"MCPT_TRACE_ENGINE": engine})
    try:
        for mode in (mcpt.TRACE_FAST, mcpt.TRACE_REFERENCE):
            dev.set_trace_mode(mode)
            for falloff, reach in (("hard", 250.0), ("linear", 250.0), ("square", 1e30)):
                got = dev.occlusion(q6[:, :3], q6[:, 3:], spp, reach, falloff, seed=seed, workspace_rays=7 * spp)
                assert _differing(got, OR.fold(q6, *parts, spp, reach, falloff)) == 0, (engine, mode, falloff)
    finally:
        dev.close()
        sc.close()


def _upload(hip_rt, a):
    a = np.ascontiguousarray(a)
    b = hip_rt.DeviceBuffer(max(a.nbytes, 8))
    hip_rt.check(hip_rt.hip().hipMemcpy(b.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes, 1))
    return b


def test_device_forms_on_a_side_stream_are_the_host_forms(mcpt, cornell, surface, chart):
    import hip_rt
    dev, L = cornell, mcpt.lib()
    n, spp, seed, reach = 130, 33, 23, 250.0
    q6 = _entries(surface, n, spp)
    ids = (np.arange(n, dtype=np.int32) * 7919 + 3)
    want = dev.occlusion(q6[:, :3], q6[:, 3:], spp, reach, "square", seed=seed, ids=ids)
    st = hip_rt.Stream()
    d_q, d_ids = _upload(hip_rt, q6), _upload(hip_rt, ids)
    d = {"ao": hip_rt.DeviceBuffer(n * 8), "stderr": hip_rt.DeviceBuffer(n * 8), "bent": hip_rt.DeviceBuffer(n * 24), "hits": hip_rt.DeviceBuffer(n * 4),
         "back": hip_rt.DeviceBuffer(n * 4)}
    op = mcpt.OcclusionParams(spp, 0, seed, mcpt.OCCLUSION_SQUARE, 0, reach, 5 * spp, (C.c_int32 * 2)(0, 0))
    assert L.mcpt_query_occlusion_device(dev._h, d_q.ptr, d_ids.ptr, n, C.byref(op), d["ao"].ptr, d["stderr"].ptr, d["bent"].ptr, d["hits"].ptr, d["back"].ptr,
                                         None, st.h) == 0, L.mcpt_last_error()
    got = {"ao": np.zeros(n), "stderr": np.zeros(n), "bent": np.zeros((n, 3)), "hits": np.zeros(n, dtype=np.int32), "back": np.zeros(n, dtype=np.int32)}
    for k in KEYS:
        d[k].to_host_async(got[k], st.h)
    st.synchronize()
    assert _differing(got, want) == 0
    # only the occlusion asked for, with statistics; and n == 0
    stats = mcpt.Stats()
    assert L.mcpt_query_occlusion_device(dev._h, d_q.ptr, d_ids.ptr, n, C.byref(op), d["ao"].ptr, None, None, None, None, C.byref(stats), st.h) == 0
    assert stats.rays_primary == n * spp and stats.launches == -(-n // 5)
    d["ao"].to_host_async(got["ao"], st.h)
    st.synchronize()
    assert np.array_equal(_bits(got["ao"]), _bits(want["ao"]))
    assert L.mcpt_query_occlusion_device(dev._h, None, None, 0, C.byref(op), None, None, None, None, None, None, st.h) == 0
    assert dev.occlusion(np.zeros((0, 3)), np.zeros((0, 3)), 4, 1.0)["bent"].shape == (0, 3)
    # the map's device form
    Wm, Hm, R = 33, 17, 2
    wmap = dev.bake_occlusion_lightmap(Wm, Hm, spp, reach, uv=chart, falloff="square", seed=seed, dilate=R)
    d_uv = _upload(hip_rt, chart)
    m = {"ao": hip_rt.DeviceBuffer(Wm * Hm * 8), "stderr": hip_rt.DeviceBuffer(Wm * Hm * 8), "bent": hip_rt.DeviceBuffer(Wm * Hm * 24),
         "hits": hip_rt.DeviceBuffer(Wm * Hm * 4), "back": hip_rt.DeviceBuffer(Wm * Hm * 4), "owner": hip_rt.DeviceBuffer(Wm * Hm * 4)}
    om = mcpt.OcclusionMap(Wm, Hm, R, 0)
    assert L.mcpt_bake_occlusion_lightmap_device(dev._h, d_uv.ptr, C.byref(om), C.byref(op), m["ao"].ptr, m["stderr"].ptr, m["bent"].ptr, m["hits"].ptr,
                                                 m["back"].ptr, m["owner"].ptr, None, st.h) == 0, L.mcpt_last_error()
    gmap = {k: np.zeros_like(wmap[k]) for k in wmap}
    for k in gmap:
        m[k].to_host_async(gmap[k], st.h)
    st.synchronize()
    assert _differing(gmap, wmap) == 0 and np.array_equal(gmap["owner"], wmap["owner"]) and (wmap["owner"] >= 0).any()
    for b in [d_q, d_ids, d_uv] + list(d.values()) + list(m.values()):
        b.free()
    st.destroy()


# ---- 2. the map

@pytest.mark.parametrize("dilate", [0, 1, 2, 3])
@pytest.mark.parametrize("size", [(16, 16), (33, 17)], ids=lambda s: "%dx%d" % s)
def test_a_map_is_the_query_of_its_texel_list(mcpt, cornell, chart, size, dilate):
    dev = cornell
    Wm, Hm = size
    spp, seed, reach = 17, 5, 250.0
    owner, texels, q6 = dev.lightmap_texels(Wm, Hm, uv=chart)
    assert 0 < texels.size < Wm * Hm
    st = mcpt.Stats()
    got = dev.bake_occlusion_lightmap(Wm, Hm, spp, reach, uv=chart, falloff="linear", seed=seed, dilate=dilate, workspace_rays=3 * spp, stats=st)
    assert got["ao"].shape == (Hm, Wm) and got["bent"].shape == (Hm, Wm, 3) and got["owner"].dtype == np.int32
    assert st.rays_primary == texels.size * spp and st.launches == -(-texels.size // 3)
    lst = dev.occlusion(q6[:, :3], q6[:, 3:], spp, reach, "linear", seed=seed, ids=texels)
    want = OR.scatter((Hm, Wm), texels, lst)
    want["ao"], want_owner = OR.dilate(want["ao"], owner, dilate)
    assert _differing(got, want) == 0
    # owner is the lightmap's, dilation included
    assert np.array_equal(got["owner"], want_owner) and np.array_equal(got["owner"], dev.bake_lightmap(Wm, Hm, 1, uv=chart, dilate=dilate)[3])
    # what no face covers and no round filled is exactly +0.0 and 0, in every map; filled texels carry an occlusion and nothing else
    empty, filled = got["owner"] == -1, got["owner"] < -1
    assert (empty.any() or dilate > 0) and (filled.any() == (dilate > 0))
    for k in KEYS:
        assert not np.ascontiguousarray(got[k][empty]).view(np.uint8).any(), k
        if k != "ao":
            assert not np.ascontiguousarray(got[k][filled]).view(np.uint8).any(), k
    if dilate:
        assert got["ao"][filled].max() > 0


def test_a_chart_that_covers_nothing_gives_empty_maps(mcpt, cornell, chart):
    st = mcpt.Stats()
    got = cornell.bake_occlusion_lightmap(8, 8, 4, 1.0, uv=chart + 5.0, dilate=1, stats=st)
    assert (got["owner"] == -1).all() and st.rays_primary == 0 and st.launches == 0
    for k in KEYS:
        assert not got[k].view(np.uint8).any()


# ---- 3. scenes whose answer is exact

def _quad(corners, want):
    """the two triangles of a quad whose stored face normal (normalize(cross(v0 - v1, v2 - v0)), the library's rule) is `want`"""
    c, want = np.asarray(corners, dtype=np.float64), np.asarray(want, dtype=np.float64)
    v = []
    for tri in ((0, 1, 2), (0, 2, 3)):
        a, b, c2 = c[tri[0]], c[tri[1]], c[tri[2]]
        if np.dot(np.cross(a - b, c2 - a), want) < 0:
            b, c2 = c2, b
        v.append(np.concatenate([a, b, c2]))
    return np.array(v), np.tile(want, (2, 3))


def test_a_floor_under_open_sky_is_open(mcpt):
    sc = TV._scene(mcpt, [_quad([[-5, 0, -5], [5, 0, -5], [5, 0, 5], [-5, 0, 5]], [0, 1, 0])])
    dev = mcpt.Device(sc, 0)
    rng = np.random.default_rng(1)
    n, spp = 70, 65
    p = np.stack([rng.uniform(-4, 4, n), np.zeros(n), rng.uniform(-4, 4, n)], axis=1)
    nrm = np.tile([0.0, 3.0, 0.0], (n, 1))
    for falloff in FALLOFFS:
        got = dev.occlusion(p, nrm, spp, 100.0, falloff, seed=2)
        assert np.array_equal(got["ao"], np.ones(n)) and not got["hits"].any() and not got["back"].any()
        assert np.array_equal(_bits(got["stderr"]), np.zeros(n, dtype=np.uint64))
        assert (got["bent"][:, 1] > 0.5).all() and np.allclose(np.linalg.norm(got["bent"], axis=1), 1.0, rtol=0, atol=1e-14)
    dev.close()
    sc.close()


def test_closed_bodies_count_exactly(mcpt):
    """tests/test_gpu_visibility.py's closed room of inward faces around a closed cube of outward faces: from the room's floor every ray
    ends on a face seen from its front, from inside the cube on one seen from behind -- by the winding alone"""
    sc = TV._scene(mcpt, [TV._box((0, 0, 0), (3, 3, 3), inward=True), TV._box((1, 1, 1), (2, 2, 2), inward=False)])
    dev = mcpt.Device(sc, 0)
    rng = np.random.default_rng(8)
    spp = 96
    # on the room's floor, ceiling and one wall, the normal into the room, of any length
    n = 66
    u, w = rng.uniform(0.1, 2.9, n), rng.uniform(0.1, 2.9, n)
    p = np.concatenate([np.stack([u, np.zeros(n), w], axis=1), np.stack([u, np.full(n, 3.0), w], axis=1), np.stack([np.zeros(n), u, w], axis=1)])
    nrm = np.concatenate([np.tile([0.0, 2.0, 0.0], (n, 1)), np.tile([0.0, -0.5, 0.0], (n, 1)), np.tile([1e-3, 0.0, 0.0], (n, 1))])
    got = dev.occlusion(p, nrm, spp, 1e30, "hard", seed=5, workspace_rays=1000)
    assert np.array_equal(_bits(got["ao"]), np.zeros(3 * n, dtype=np.uint64))
    assert np.array_equal(got["hits"], np.full(3 * n, spp)) and not got["back"].any() and not got["stderr"].any()
    assert np.array_equal(_bits(got["bent"]), _bits(np.array([OR.n_hat(b) for b in nrm])))         # nothing is open: the hemisphere rule's n^
    # a reach shorter than anything in sight opens every direction again
    assert np.array_equal(dev.occlusion(p, nrm, spp, 1e-3, "hard", seed=5)["ao"], np.ones(3 * n))
    # inside the cube, any normal
    inside = 1.05 + 0.9 * rng.random((33, 3))
    got = dev.occlusion(inside, rng.normal(size=(33, 3)), spp, 1e30, "linear", seed=5)
    assert np.array_equal(got["hits"], np.full(33, spp)) and np.array_equal(got["back"], got["hits"])
    dev.close()
    sc.close()


def test_a_floor_against_a_wall_is_half_open(mcpt):
    """A point on a floor, 0.05 from a perpendicular wall 1000 wide and high.  The wall's plane halves the cosine-weighted hemisphere about
    the floor's normal, so 0.5 of it is open; with a reach of 100 the rays that meet the wall further away than that stay open: those with
    |d.x| < 0.06 / 100, a share of the hemisphere below 5e-4.  Hence | ao - 0.5 | <= 5 stderr + 1e-3 (stderr is about 0.008 at 4096
    samples); the seed is fixed, so the outcome is one number and not a gamble."""
    floor = _quad([[-500, 0, -500], [500, 0, -500], [500, 0, 500], [-500, 0, 500]], [0, 1, 0])
    wall = _quad([[0, 0, -500], [0, 1000, -500], [0, 1000, 500], [0, 0, 500]], [1, 0, 0])
    sc = TV._scene(mcpt, [floor, wall])
    dev = mcpt.Device(sc, 0)
    got = dev.occlusion([[0.05, 0.0, 0.0]], [[0.0, 1.0, 0.0]], 4096, 100.0, "hard", seed=7)
    ao, err, bent = got["ao"][0], got["stderr"][0], got["bent"][0]
    print("floor against a wall: ao %.5f, stderr %.5f, bent %r, hits %d, back %d" % (ao, err, bent.tolist(), got["hits"][0], got["back"][0]))
    assert abs(ao - 0.5) <= 5.0 * err + 1e-3
    assert 0.006 < err < 0.009
    assert bent[0] > 0 and bent[1] > 0                                      # it leans away from the wall
    assert got["back"][0] == 0 and got["hits"][0] == 4096 - round(ao * 4096)
    dev.close()
    sc.close()


# ---- 4. after updates and under a motion

@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_an_updated_device_answers_as_a_fresh_one(mcpt, mode, tmp_path_factory):
    """as tests/test_gpu_update_queries.py holds the other calls: the query and the map on a device before the update (so that the
    workspaces exist and were made for another geometry) and after it, against a device made fresh from the moved files.  The table is
    mirrored: its stored normals turn, and the back-face counts with them."""
    import query_family as QF
    import test_gpu_update as TU
    import test_gpu_update_queries as TUQ
    name, size = "cornell-box", (QF.W, QF.H)
    sc, v, _, _ = TU.base(mcpt, name, tmp_path_factory, size=size)
    nv = TUQ.geometry(mcpt, name, "mirror", tmp_path_factory)
    uv = _chart_of(sc)

    def ask(d, geom):
        q = QF.lists(mcpt, geom)
        a = d.occlusion(q["points"], q["normals"], 65, q["vis_distance"], "linear", seed=QF.SEED, ids=q["point_ids"], workspace_rays=200)
        b = d.bake_occlusion_lightmap(33, 17, 33, q["vis_distance"], uv=uv, seed=QF.SEED, dilate=1)
        return a, b
    dev = mcpt.Device(sc, 0)
    before = ask(dev, v)
    dev.update_vertices(nv, mode=mode)
    after = ask(dev, nv)
    fsc, fdev = TU.fresh(mcpt, name, "mirror", None, tmp_path_factory, size=size)
    fresh = ask(fdev, nv)
    for got, want, was in zip(after, fresh, before):
        assert _differing(got, want) == 0
        assert _differing(got, was) > 0
    assert np.array_equal(after[1]["owner"], fresh[1]["owner"])
    assert (after[0]["back"] != ask(dev, nv)[0]["back"]).sum() == 0 and after[0]["hits"].max() > 0
    for h in (fdev, fsc, dev):
        h.close()


def test_under_a_motion_the_query_sees_key_0(mcpt, tmp_path_factory):
    import query_family as QF
    import test_gpu_update as TU
    import test_gpu_update_queries as TUQ
    name, size = "cornell-box", (QF.W, QF.H)
    sc, v0, _, _ = TU.base(mcpt, name, tmp_path_factory, size=size)
    v1 = TUQ.geometry(mcpt, name, "rigid", tmp_path_factory)
    uv = _chart_of(sc)
    q = QF.lists(mcpt, v0)
    dev = mcpt.Device(sc, 0)
    query = lambda: dev.occlusion(q["points"], q["normals"], 65, q["vis_distance"], "square", seed=QF.SEED, ids=q["point_ids"], workspace_rays=200)
    bake = lambda: dev.bake_occlusion_lightmap(33, 17, 33, q["vis_distance"], uv=uv, seed=QF.SEED, dilate=1)
    want = query(), bake()
    dev.set_motion(v_end=v1, shutter=(0.0, 1.0), steps=3)
    for call, w in zip((query, bake), want):
        dev.generateImg(3, seed=5)                                          # a motion frame: the geometry is left at the last shutter step
        info = dev.motion_info()
        assert info["steps_run"] == 3 and info["ms_updates"] > 0
        assert _differing(call(), w) == 0
    # ... and key 1 would have answered differently
    dev.clear_motion()
    dev.update_vertices(v1)
    assert _differing(query(), want[0]) > 0
    dev.close()


# ---- 5. what else lives on the device

def test_progressive_handles_and_visibility_bakes_do_not_notice(mcpt, cornell, surface, chart):
    dev = cornell
    q6 = _entries(surface, 300, 16)
    runs = []
    for interrupted in (False, True):
        pr = dev.progressive(16, seed=4)
        pr.step(4)
        if interrupted:
            dev.bake_occlusion_lightmap(33, 17, 5, 250.0, uv=chart, dilate=2, stats=mcpt.Stats())
            dev.occlusion(q6[:, :3], q6[:, 3:], 16, 250.0, "linear", workspace_rays=48)
        pr.step(4)
        runs.append((pr.image(), pr.stderr()))
        pr.close()
    assert np.array_equal(_bits(runs[0][0]), _bits(runs[1][0])) and np.array_equal(_bits(runs[0][1]), _bits(runs[1][1]))
    # a plain probe_visibility right behind a device-form occlusion query of a larger list, which shares the visibility workspace
    import hip_rt
    L = mcpt.lib()
    lo, hi = TV._bounds(dev)
    probes = lo + (hi - lo) * (0.1 + 0.8 * np.random.default_rng(3).random((9, 3)))
    ask = lambda: dev.probe_visibility(probes, 33, res=4, max_distance=250.0, seed=19)
    want = ask()
    n, spp = 300, 64
    want_ao = dev.occlusion(q6[:, :3], q6[:, 3:], spp, 250.0, seed=2)["ao"]
    st = hip_rt.Stream()
    d_q, d_ao = _upload(hip_rt, q6), hip_rt.DeviceBuffer(n * 8)
    op = mcpt.OcclusionParams(spp, 0, 2, mcpt.OCCLUSION_HARD, 0, 250.0, 0, (C.c_int32 * 2)(0, 0))
    assert L.mcpt_query_occlusion_device(dev._h, d_q.ptr, None, n, C.byref(op), d_ao.ptr, None, None, None, None, None, st.h) == 0, L.mcpt_last_error()
    got = ask()
    ao = np.zeros(n)
    d_ao.to_host_async(ao, st.h)
    st.synchronize()
    for a, c in zip(got, want):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(c).view(np.uint8))
    assert np.array_equal(_bits(ao), _bits(want_ao))
    d_q.free()
    d_ao.free()
    st.destroy()
