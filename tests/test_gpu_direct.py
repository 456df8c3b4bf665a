"""-m gpu: direct light from a caller's own lights (include/mcpt.h: direct light) on the GPU.  Every comparison is exact unless it says
otherwise.

  1. THE RULE: Device.direct_light == direct_fold_host(g, any_hit(rays, tmax)) of Device.direct_rays, bit for bit -- cornell-box 160x90 and
     veach-mis 64x48, a few hundred closest-hit points of camera rays with their face normals, five lights of all types inside the scene's
     bounds, fast and reference mode, spp in {1, 2, 7}, n in {1, 63, 64, 65, 257}; at n = 257 at least a tenth of the walked slots are
     occluded and at least a tenth are not;
  2. the seam against numpy (tests/direct_ref.py): rays, limits and factors bit for bit;
  3. hand values in a scene of one two-triangle wall;
  4. physics: a square rectangle light against the closed-form form factor, and a rectangle light against the path tracer's irradiance
     under an emitter quad with a blocker (5 standard errors; the runs are deterministic);
  5. extents: both _device forms through the C ABI on a side stream, every array in a Guarded buffer, both fills, both alignments at the
     largest size; NULL optional outputs; n = 0; the lights overwritten right after the call returns;
  6. the map: bake_direct_lightmap == direct_light of lightmap_texels' list with ids = texels, scattered, dilated by the lightmap's rule;
  7. state: after update_vertices, under a motion, between the passes of a live progressive handle.
Device.irradiance returns E = pi * (the query's mean radiance): that E is what case 4 compares a rectangle light's irradiance with."""
import ctypes as C
import math

import numpy as np
import pytest

import direct_cases as DC
import direct_ref as DR
import lightmap_ref as LR
import query_ref
from conftest import SCENES
from guarded import FILLS, Guarded

pytestmark = pytest.mark.gpu

SMALL = {"veach-mis": (64, 48), "cornell-box": (160, 90)}
SIZES = (1, 63, 64, 65, 257)
KEYS = ("irradiance", "stderr", "per_light", "visibility")
KNOBS = ("MCPT_TRACE_ENGINE", "MCPT_FINISH_ENGINE", "MCPT_FINISH_PATHS", "MCPT_WORKSPACE_GB")
PD = C.POINTER(C.c_double)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _differing(got, want):
    return sum(int((_bits(got[k]).reshape(-1) != _bits(want[k]).reshape(-1)).sum()) + (got[k].shape != want[k].shape) for k in KEYS)


def _bounds(dev):
    v = dev.scene.faces()[0][:, :9].reshape(-1, 3)
    return v.min(axis=0), v.max(axis=0)


class Small:
    """a scene at its small size, 300 receivers on what its camera sees, and the five-light mix inside its bounds"""
    def __init__(self, mcpt, oracle, name):
        w, h = SMALL[name]
        osc = oracle.OracleScene(SCENES + name, texture_dir=SCENES, width=w, height=h)
        rays = osc.primary_rays()
        osc.close()
        self.name = name
        self.sc = mcpt.Scene(SCENES, name, width=w, height=h)
        self.dev = mcpt.Device(self.sc, 0)
        face, _, p, _ = self.dev.ray_intersect(rays)
        self.points, self.normals = DC.camera_receivers(rays, face, p, np.ascontiguousarray(self.sc.faces()[0][:, 24:27]), 300, 3)
        assert self.points.shape[0] == 300
        self.lo, self.hi = _bounds(self.dev)
        self.lights = DC.scene_lights(mcpt, self.lo, self.hi)
        self.bias = DC.bias_for(self.lo, self.hi)
        assert sorted(L.type for L in self.lights) == [0, 1, 2, 3, 3] and sorted(L.flags for L in self.lights if L.type == 3) == [0, 1]

    def close(self):
        self.dev.close()
        self.sc.close()


@pytest.fixture(scope="module", params=["cornell-box", "veach-mis"])
def small(request, mcpt, oracle):
    s = Small(mcpt, oracle, request.param)
    yield s
    s.close()


@pytest.fixture(scope="module")
def cornell(mcpt, oracle):
    s = Small(mcpt, oracle, "cornell-box")
    yield s
    s.close()


# ============================================================================================== 1. the rule
@pytest.mark.parametrize("mode", ["fast", "reference"])
@pytest.mark.parametrize("spp", [1, 2, 7])
def test_the_rule(small, mcpt, mode, spp):
    s, dev = small, small.dev
    dev.set_trace_mode(mcpt.TRACE_REFERENCE if mode == "reference" else mcpt.TRACE_FAST)
    try:
        for n in SIZES:
            at = (np.arange(n) * 7 + 13 * n + spp) % 300
            p, nrm, ids = s.points[at], s.normals[at], (at * 3 + 5).astype(np.int32)
            kw = dict(spp=spp, bias=s.bias, seed=11 + spp, ids=ids, sample_base=2)
            rays, tmax, g = dev.direct_rays(p, nrm, s.lights, **kw)
            R = mcpt.direct_slots(s.lights, spp)
            assert R == 3 + 2 * spp and rays.shape == (n * R, 6) and tmax.shape == g.shape == (n * R,)
            occ = dev.any_hit(rays, tmax)
            walked = g > 0
            assert not occ[~walked].any()                        # a skipped slot has tmax 0: never occluded
            if n == 257:
                share = occ[walked].mean()
                print("%s %s spp %d: %d of %d slots walked, %.1f %% of them occluded" % (s.name, mode, spp, int(walked.sum()), walked.size, 100 * share))
                assert walked.sum() >= 257 and 0.1 <= share <= 0.9, "the case must not pass vacuously"
            want = mcpt.direct_fold_host(s.lights, g, occ, n, spp)
            st = mcpt.Stats()
            got = dev.direct_light(p, nrm, s.lights, stats=st, **kw)
            assert _differing(got, want) == 0, "%s %s spp %d n %d: %d words differ" % (s.name, mode, spp, n, _differing(got, want))
            assert st.rays_primary == int(walked.sum()) and st.launches == 1
            if n == 257:
                assert st.node_visits > 0 and st.tri_tests > 0
                assert got["irradiance"].max() > 0 and 0 < got["visibility"].sum() < got["visibility"].size
                if spp > 1:
                    assert got["stderr"].max() > 0
    finally:
        dev.set_trace_mode(mcpt.TRACE_FAST)


# ============================================================================================== 2. the seam against numpy
@pytest.mark.parametrize("spp", [1, 2, 7])
def test_the_seam_is_the_restatement(small, spp):
    s = small
    ids = (np.arange(300) * 5 + 1).astype(np.int32)
    kw = dict(spp=spp, bias=s.bias, seed=2 ** 40 + 9, ids=ids, sample_base=3)
    rays, tmax, g = s.dev.direct_rays(s.points, s.normals, s.lights, **kw)
    w_rays, w_tmax, w_g = DR.direct_rays(s.points, s.normals, s.lights, **kw)
    for got, want, what in ((rays, w_rays, "rays"), (tmax, w_tmax, "tmax"), (g, w_g, "g")):
        bad = _bits(got) != _bits(want)
        assert not bad.any(), "%s spp %d: %d of %d words of %s differ from the restatement" % (s.name, spp, int(bad.sum()), bad.size, what)
    assert (g > 0).any() and (g == 0).any()
    # without ids an entry's id is its index
    a = s.dev.direct_rays(s.points[:65], s.normals[:65], s.lights, spp=spp, bias=s.bias, seed=4)
    b = DR.direct_rays(s.points[:65], s.normals[:65], s.lights, spp=spp, bias=s.bias, seed=4, ids=np.arange(65))
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ============================================================================================== 3. hand values
def _quad(x0, x1, z0, z1, y, up):
    a, b, c, d = [x0, y, z0], [x1, y, z0], [x1, y, z1], [x0, y, z1]
    return [a + c + b, a + d + c] if up else [a + b + c, a + c + d]


def _scene(mcpt, quads, emitter=None, radiance=(3.0, 2.0, 1.0)):
    """black quads (x0, x1, z0, z1, y, up); emitter: one more, which emits `radiance`"""
    v, vn, mat = [], [], []
    for q in quads + ([emitter] if emitter else []):
        v += _quad(*q)
        vn += [[0.0, 1.0 if q[5] else -1.0, 0.0] * 3] * 2
        mat += [1 if q is emitter else 0] * 2
    rec = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0]] * 2)
    lights, rad = ([1], [list(radiance)]) if emitter else (np.zeros(0, dtype=np.int32), np.zeros((0, 3)))
    return mcpt.Scene.from_arrays(np.array(v, dtype=np.float64), np.array(vn, dtype=np.float64), np.array(mat, dtype=np.int32), rec, lights, rad,
                                  [0.0, 0.5, 5.0], [0.0, 0.5, 0.0], [0.0, 1.0, 0.0], 60.0, 32, 18)


@pytest.mark.parametrize("mode", ["fast", "reference"])
def test_hand_values_around_a_wall(mcpt, mode):
    """One wall of two triangles, y = 1, |x| <= 1, |z| <= 1.  Receiver A = (5, 0, 0) has open sky, receiver B = (-0.5, 0, 0) lies under the
    wall; both face up.  Over A every number is exact in fp64: r = 2, r2 = 4, w = (0, 1, 0), cr = 1.  The rays that must be blocked lean
    along x -- from B to (0.5, 2, 0) through the wall at x = 0 --: the closest hit's distance is (p.x - o.x) / d.x, the reference's own,
    and a ray with d.x = 0 has none; their values are held to the restatement."""
    sc = _scene(mcpt, [(-1.0, 1.0, -1.0, 1.0, 1.0, True)])
    dev = mcpt.Device(sc, 0)
    dev.set_trace_mode(mcpt.TRACE_REFERENCE if mode == "reference" else mcpt.TRACE_FAST)
    A, B, up, down = [5.0, 0.0, 0.0], [-0.5, 0.0, 0.0], [0.0, 3.0, 0.0], [0.0, -1.0, 0.0]
    over_B = [0.5, 2.0, 0.0]

    def open_value(p, n, L, **kw):
        """the restatement's answer with nothing occluded"""
        _, _, g = DR.direct_rays([p], [n], [L], **kw)
        return DR.fold([L], g, np.zeros(g.size, dtype=np.uint8), 1, kw.get("spp", 1))["irradiance"][0]
    one = lambda p, n, L, **kw: {k: v[0] for k, v in dev.direct_light([p], [n], [L], **kw).items()}
    col = (8.0, 4.0, 2.0)
    # a point light 2 above the receiver: g = 1 / 4
    got = one(A, up, mcpt.point_light([5.0, 2.0, 0.0], col))
    assert got["irradiance"].tolist() == [2.0, 1.0, 0.5] and got["per_light"].tolist() == [[2.0, 1.0, 0.5]] and got["visibility"].tolist() == [1.0]
    assert not _bits(got["stderr"]).any()
    # behind the wall: traced, occluded
    got = one(B, up, mcpt.point_light(over_B, col))
    assert not _bits(got["irradiance"]).any() and got["visibility"].tolist() == [0.0]
    st = mcpt.Stats()
    dev.direct_light([B], [up], [mcpt.point_light(over_B, col)], stats=st)
    assert st.rays_primary == 1
    # a normal that faces away: skipped, nothing walked, visibility +0.0
    st = mcpt.Stats()
    got = one(A, down, mcpt.point_light([5.0, 2.0, 0.0], col), stats=st)
    assert not _bits(got["irradiance"]).any() and not _bits(got["visibility"]).any() and st.rays_primary == 0
    # range just below r cuts the light off, r itself and just above do not
    for rng_, lit in ((np.nextafter(2.0, 0.0), False), (2.0, True), (np.nextafter(2.0, 3.0), True), (0.0, True)):
        got = one(A, up, mcpt.point_light([5.0, 2.0, 0.0], col, range=rng_))
        assert got["irradiance"].tolist() == ([2.0, 1.0, 0.5] if lit else [0.0, 0.0, 0.0]) and got["visibility"].tolist() == [1.0 if lit else 0.0]
    # a spot along (3, -4, 0) / 5: cs = 0.8 toward A.  x = (cs - cos_outer) / (cos_inner - cos_outer)
    def spot(ci, co):
        L = mcpt.spot_light([5.0, 2.0, 0.0], [3.0, -4.0, 0.0], col, 10.0, 20.0)
        L.cos_inner, L.cos_outer = ci, co
        return L
    cs = 0.8
    assert one(A, up, spot(0.95, cs))["irradiance"].tolist() == [0.0, 0.0, 0.0]                        # x = 0: outside
    assert one(A, up, spot(0.99, 0.9))["visibility"].tolist() == [0.0]                                 # x < 0
    got = one(A, up, spot(cs + 0.125, cs - 0.125))                                                     # x = 1/2: f = 1/2
    assert got["irradiance"].tolist() == [1.0, 0.5, 0.25] and got["visibility"].tolist() == [1.0]
    assert one(A, up, spot(cs, 0.5))["irradiance"].tolist() == [2.0, 1.0, 0.5]                         # x = 1
    assert one(A, up, spot(0.7, 0.5))["irradiance"].tolist() == [2.0, 1.0, 0.5]                        # x > 1: clamped
    # a directional light straight down: color itself in the open, nothing under the wall
    sun = mcpt.directional_light([0.0, -2.0, 0.0], col)
    assert one(A, up, sun)["irradiance"].tolist() == [8.0, 4.0, 2.0] and one(A, up, sun)["visibility"].tolist() == [1.0]
    lean = mcpt.directional_light([-1.0, -2.0, 0.0], col)                                              # travels down and to -x
    got = one(B, up, lean)
    assert not _bits(got["irradiance"]).any() and got["visibility"].tolist() == [0.0]
    got = one(A, up, lean)
    assert np.array_equal(_bits(got["irradiance"]), _bits(open_value(A, up, lean))) and got["irradiance"][0] > 7.0 and got["visibility"].tolist() == [1.0]
    assert one(A, down, sun)["visibility"].tolist() == [0.0]
    # a light within bias of the receiver is unoccluded although the wall lies between: tmax = sqrt(5) - 3 < 0
    got = one(B, up, mcpt.point_light(over_B, col), bias=3.0)
    assert np.array_equal(_bits(got["irradiance"]), _bits(open_value(B, up, mcpt.point_light(over_B, col), bias=3.0)))
    assert got["irradiance"][0] > 1.0 and got["visibility"].tolist() == [1.0]
    # a rectangle over A: one-sided toward A, one-sided away from it, two-sided away from it
    toward = mcpt.rect_light([4.5, 2.0, -0.5], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], col)                  # cross(u, v) = (0, -1, 0)
    away = mcpt.rect_light([4.5, 2.0, -0.5], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], col)
    both = mcpt.rect_light([4.5, 2.0, -0.5], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], col, two_sided=True)
    st = mcpt.Stats()
    lit = one(A, up, toward, spp=16, seed=3, stats=st)
    assert st.rays_primary == 16 and lit["visibility"].tolist() == [1.0] and lit["irradiance"][0] > 1.0 and lit["stderr"][0] > 0
    st = mcpt.Stats()
    got = one(A, up, away, spp=16, seed=3, stats=st)
    assert not _bits(got["irradiance"]).any() and not _bits(got["visibility"]).any() and st.rays_primary == 0
    got = one(A, up, both, spp=16, seed=3)
    assert got["visibility"].tolist() == [1.0] and got["irradiance"][0] > 1.0
    assert np.allclose(got["irradiance"] / got["irradiance"][2], [4.0, 2.0, 1.0], rtol=1e-12, atol=0)
    # no lights at all: +0.0 everywhere that is asked for
    got = dev.direct_light([A, B], [up, up], [])
    assert got["irradiance"].shape == (2, 3) and got["per_light"].shape == (2, 0, 3) and not _bits(got["irradiance"]).any() and not _bits(got["stderr"]).any()
    assert dev.direct_light(np.zeros((0, 3)), np.zeros((0, 3)), [sun])["irradiance"].shape == (0, 3)
    dev.close()
    sc.close()


# ============================================================================================== 4. physics
FF_SEED, FF_SPP = 1, 4096
FF_XZ = np.array([[0.0, 0.0], [1.0, 1.0], [0.5, 0.0], [0.25, -0.75], [-1.5, 0.5]])


def form_factor_case(mcpt):
    """a square of side 2 and radiance 1 at height 1, facing down, over five receivers at y = 0 that face up: E = pi F"""
    p = np.stack([FF_XZ[:, 0], np.zeros(5), FF_XZ[:, 1]], axis=1)
    nrm = np.tile([0.0, 1.0, 0.0], (5, 1))
    light = mcpt.rect_light([-1.0, 1.0, -1.0], [2.0, 0.0, 0.0], [0.0, 0.0, 2.0], (1.0, 1.0, 1.0))
    F = np.array([query_ref.square_form_factor(x, z, 1.0, 1.0) for x, z in FF_XZ])
    return p, nrm, light, F


def test_a_square_light_against_the_form_factor(mcpt):
    """Nothing is occluded (the only geometry is a floor far below), so the restatement is the whole answer: FF_SEED was picked on the
    CPU with tests/direct_ref.py, where |E - pi F| <= 5 stderr holds with room at every receiver, and the GPU's answer is that one bit for
    bit."""
    p, nrm, light, F = form_factor_case(mcpt)
    sc = _scene(mcpt, [(-6.0, 6.0, -6.0, 6.0, -50.0, True)])
    dev = mcpt.Device(sc, 0)
    got = dev.direct_light(p, nrm, [light], spp=FF_SPP, bias=0.01, seed=FF_SEED)
    E, err = got["irradiance"], got["stderr"]
    sigma = np.abs(E - math.pi * F[:, None]) / err
    print("form factor: E", E[:, 0], "pi F", math.pi * F, "|E - pi F| / stderr", np.round(sigma[:, 0], 2))
    assert np.all(err > 0) and np.all(np.abs(E - math.pi * F[:, None]) <= 5.0 * err), sigma
    assert np.array_equal(got["visibility"], np.ones((5, 1)))
    rays, tmax, g = DR.direct_rays(p, nrm, [light], spp=FF_SPP, bias=0.01, seed=FF_SEED)
    want = DR.fold([light], g, np.zeros(g.size, dtype=np.uint8), 5, FF_SPP)
    assert _differing(got, want) == 0
    dev.close()
    sc.close()


def test_a_rectangle_light_against_the_path_tracer(mcpt):
    """A black floor, an emitter quad of side 1 at height 2 that faces down, and a black blocker at height 1 that covers x >= 0.2: the
    path tracer's irradiance on the floor (hemisphere rays that end on the emitter; every material is black, so nothing else arrives) against
    a rectangle light of the quad's radiance 1e-3 in front of it.  Receivers on the lit side, the ones at x >= 0 in the penumbra.  Within 5
    combined standard errors per receiver and channel; both runs are deterministic."""
    rad = (3.0, 2.0, 1.0)
    sc = _scene(mcpt, [(-6.0, 6.0, -6.0, 6.0, 0.0, True), (0.2, 1.5, -1.0, 1.0, 1.0, False)], emitter=(-0.5, 0.5, -0.5, 0.5, 2.0, False), radiance=rad)
    dev = mcpt.Device(sc, 0)
    p = np.array([[x, 0.0, z] for x in (-1.5, -0.6, -0.3, 0.0, 0.2, 0.4) for z in (0.0, 0.4)])
    nrm = np.tile([0.0, 1.0, 0.0], (p.shape[0], 1))
    E, E_err, hits = dev.irradiance(p, nrm, 8192, seed=21)
    light = mcpt.rect_light([-0.5, 2.0 - 1e-3, -0.5], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], rad)
    got = dev.direct_light(p, nrm, [light], spp=2048, bias=0.01, seed=22)
    D, D_err, vis = got["irradiance"], got["stderr"], got["visibility"][:, 0]
    comb = np.sqrt(E_err * E_err + D_err * D_err)
    sigma = np.abs(E - D) / comb
    print("path tracer E", np.round(E[:, 0], 4), "\nrectangle    E", np.round(D[:, 0], 4), "\nvisibility", np.round(vis, 3), "\nsigma", np.round(sigma[:, 0], 2))
    assert np.all(E[:, 0] > 0) and np.all(D[:, 0] > 0) and np.all(comb > 0)
    assert np.all(np.abs(E - D) <= 5.0 * comb), sigma
    assert np.all(vis[:6] == 1.0) and np.all(vis[6:] < 1.0) and np.all(vis[6:] > 0.0)          # x < 0: fully lit; x >= 0: the penumbra
    dev.close()
    sc.close()


# ============================================================================================== 5. extents
def _light_array(mcpt, lights):
    return (mcpt.DirectLight * len(lights))(*lights)


def _params(mcpt, spp, bias, seed, sample_base=0):
    return mcpt.DirectParams(spp, sample_base, seed, bias, 0, (C.c_int32 * 3)(0, 0, 0))


@pytest.fixture(scope="module")
def side_stream():
    import hip_rt
    hip_rt.set_device(0)
    st = hip_rt.Stream()
    yield st
    st.destroy()


@pytest.mark.parametrize("n", SIZES)
def test_query_device_form_extents(cornell, mcpt, side_stream, n):
    s, dev, L = cornell, cornell.dev, mcpt.lib()
    nl, spp = 5, 3
    q = np.ascontiguousarray(np.concatenate([s.points[:n], s.normals[:n]], axis=1))
    ids = (np.arange(n) * 2 + 7).astype(np.int32)
    dp = _params(mcpt, spp, s.bias, 77, 1)
    host = dev.direct_light(s.points[:n], s.normals[:n], s.lights, spp=spp, bias=s.bias, seed=77, ids=ids, sample_base=1)
    if n == SIZES[-1]:
        assert host["irradiance"].max() > 0 and 0 < host["visibility"].sum() < n * nl
    for fill in FILLS:
        for skewed in ((False, True) if n == SIZES[-1] else (False,)):
            sk = 8 if skewed else 0
            g_q, g_ids = Guarded(q.reshape(-1), np.float64, fill, sk), Guarded(ids, np.int32, fill, 4 if skewed else 0)
            outs = {"irradiance": Guarded(n * 3 * 8, np.float64, fill, sk), "stderr": Guarded(n * 3 * 8, np.float64, fill, sk),
                    "per_light": Guarded(n * nl * 3 * 8, np.float64, fill, sk), "visibility": Guarded(n * nl * 8, np.float64, fill, sk)}
            arr = _light_array(mcpt, s.lights)
            rc = L.mcpt_query_direct_device(dev._h, g_q.ptr, g_ids.ptr, n, arr, nl, C.byref(dp), outs["irradiance"].ptr, outs["stderr"].ptr,
                                            outs["per_light"].ptr, outs["visibility"].ptr, side_stream.h)
            # the caller's lights are its own again as soon as the call has returned
            C.memset(arr, 0xFF, C.sizeof(arr))
            assert rc == 0, L.mcpt_last_error()
            side_stream.synchronize()
            what = "mcpt_query_direct_device n %d fill 0x%02X skew %d" % (n, fill, skewed)
            for k in KEYS:
                assert np.array_equal(_bits(outs[k].payload()), _bits(host[k]).reshape(-1)), what + " " + k
            for g, name in [(g_q, "q6"), (g_ids, "ids")] + [(outs[k], k) for k in KEYS]:
                g.check(what + " " + name)
                g.free()
    # NULL optional outputs are respected: only the irradiance is written, and it is the same
    g_q, g_ids, g_E = Guarded(q.reshape(-1), np.float64, 0xA5), Guarded(ids, np.int32, 0xA5), Guarded(n * 3 * 8, np.float64, 0xA5)
    assert L.mcpt_query_direct_device(dev._h, g_q.ptr, g_ids.ptr, n, _light_array(mcpt, s.lights), nl, C.byref(dp), g_E.ptr, None, None, None,
                                      side_stream.h) == 0
    side_stream.synchronize()
    assert np.array_equal(_bits(g_E.payload()), _bits(host["irradiance"]).reshape(-1))
    for g in (g_q, g_ids, g_E):
        g.check("NULL optional outputs")
        g.free()


def test_an_empty_query_writes_nothing(cornell, mcpt, side_stream):
    s, dev, L = cornell, cornell.dev, mcpt.lib()
    dp = _params(mcpt, 2, s.bias, 1)
    for fill in FILLS:
        g_q, g_E, g_v = Guarded(np.zeros(24), np.float64, fill), Guarded(4 * 3 * 8, np.float64, fill), Guarded(4 * 5 * 8, np.float64, fill)
        assert L.mcpt_query_direct_device(dev._h, g_q.ptr, None, 0, _light_array(mcpt, s.lights), 5, C.byref(dp), g_E.ptr, None, None, g_v.ptr,
                                          side_stream.h) == 0
        assert L.mcpt_query_direct_device(dev._h, None, None, 0, None, 0, C.byref(dp), None, None, None, None, side_stream.h) == 0
        side_stream.synchronize()
        assert np.all(g_E.payload().view(np.uint8) == fill) and np.all(g_v.payload().view(np.uint8) == fill)
        for g in (g_q, g_E, g_v):
            g.check("an empty call")
            g.free()
    got = dev.direct_light(np.zeros((0, 3)), np.zeros((0, 3)), s.lights)
    assert got["irradiance"].shape == (0, 3) and got["per_light"].shape == (0, 5, 3)


def _chart_of(scene):
    return np.ascontiguousarray(scene.faces()[0][:, 18:24]) * 0.15 + 0.2


@pytest.mark.parametrize("size", [(16, 16), (33, 17)], ids=lambda z: "%dx%d" % z)
def test_map_device_form_extents(cornell, mcpt, side_stream, size):
    s, dev, L = cornell, cornell.dev, mcpt.lib()
    Wm, Hm = size
    nl, spp, n = 5, 2, size[0] * size[1]
    uv = _chart_of(dev.scene)
    host = dev.bake_direct_lightmap(Wm, Hm, s.lights, spp=spp, uv=uv, bias=s.bias, seed=5, dilate=1)
    assert host["irradiance"].max() > 0
    dp = _params(mcpt, spp, s.bias, 5)
    dm = mcpt.DirectMap(Wm, Hm, 1, 0)
    for fill in FILLS:
        for skewed in ((False, True) if size == (33, 17) else (False,)):
            sk = 8 if skewed else 0
            g_uv = Guarded(uv.reshape(-1), np.float64, fill, sk)
            outs = {"irradiance": Guarded(n * 3 * 8, np.float64, fill, sk), "stderr": Guarded(n * 3 * 8, np.float64, fill, sk),
                    "per_light": Guarded(n * nl * 3 * 8, np.float64, fill, sk), "visibility": Guarded(n * nl * 8, np.float64, fill, sk)}
            g_owner = Guarded(n * 4, np.int32, fill, 4 if skewed else 0)
            arr = _light_array(mcpt, s.lights)
            rc = L.mcpt_bake_direct_lightmap_device(dev._h, g_uv.ptr, C.byref(dm), arr, nl, C.byref(dp), outs["irradiance"].ptr, outs["stderr"].ptr,
                                                    outs["per_light"].ptr, outs["visibility"].ptr, g_owner.ptr, None, side_stream.h)
            C.memset(arr, 0xFF, C.sizeof(arr))
            assert rc == 0, L.mcpt_last_error()
            side_stream.synchronize()
            what = "mcpt_bake_direct_lightmap_device %dx%d fill 0x%02X skew %d" % (Wm, Hm, fill, skewed)
            for k in KEYS:
                assert np.array_equal(_bits(outs[k].payload()), _bits(host[k]).reshape(-1)), what + " " + k
            assert np.array_equal(g_owner.payload(), host["owner"].reshape(-1)), what
            for g, name in [(g_uv, "uv"), (g_owner, "owner")] + [(outs[k], k) for k in KEYS]:
                g.check(what + " " + name)
                g.free()
    # NULL optional outputs
    g_uv, g_E = Guarded(uv.reshape(-1), np.float64, 0xFF), Guarded(n * 3 * 8, np.float64, 0xFF)
    assert L.mcpt_bake_direct_lightmap_device(dev._h, g_uv.ptr, C.byref(dm), _light_array(mcpt, s.lights), nl, C.byref(dp), g_E.ptr, None, None, None,
                                              None, None, side_stream.h) == 0
    side_stream.synchronize()
    assert np.array_equal(_bits(g_E.payload()), _bits(host["irradiance"]).reshape(-1))
    g_uv.check("uv"); g_E.check("irradiance alone")
    g_uv.free(); g_E.free()


# ============================================================================================== 6. the map
def _scatter(shape, texels, lst, nl):
    H, W = shape
    out = {"irradiance": np.zeros((H * W, 3)), "stderr": np.zeros((H * W, 3)), "per_light": np.zeros((H * W, nl, 3)), "visibility": np.zeros((H * W, nl))}
    for k in KEYS:
        out[k][texels] = lst[k]
    return {"irradiance": out["irradiance"].reshape(H, W, 3), "stderr": out["stderr"].reshape(H, W, 3),
            "per_light": out["per_light"].reshape(H, W, nl, 3), "visibility": out["visibility"].reshape(H, W, nl)}


@pytest.mark.parametrize("dilate", [0, 2])
@pytest.mark.parametrize("chart", ["own", "grid"])
@pytest.mark.parametrize("size", [(16, 16), (33, 17)], ids=lambda z: "%dx%d" % z)
def test_a_map_is_the_query_of_its_texel_list(cornell, mcpt, size, chart, dilate):
    s, dev = cornell, cornell.dev
    Wm, Hm = size
    nfaces = dev.scene.info.num_faces
    if chart == "own":
        uv = _chart_of(dev.scene)
    else:
        # a grid atlas needs two texels a cell: the first faces at a cell each, the others off the map
        uv = np.full((nfaces, 6), 7.0)
        k = (min(Wm, Hm) // 4) ** 2
        uv[:k] = mcpt.grid_atlas(k, Wm, Hm, pad=0)
    spp, seed = 3, 8
    owner, texels, q6 = dev.lightmap_texels(Wm, Hm, uv=uv)
    assert 0 < texels.size < Wm * Hm
    st = mcpt.Stats()
    got = dev.bake_direct_lightmap(Wm, Hm, s.lights, spp=spp, uv=uv, bias=s.bias, seed=seed, sample_base=1, dilate=dilate, stats=st)
    assert got["irradiance"].shape == (Hm, Wm, 3) and got["per_light"].shape == (Hm, Wm, 5, 3) and got["visibility"].shape == (Hm, Wm, 5)
    st2 = mcpt.Stats()
    lst = dev.direct_light(q6[:, :3], q6[:, 3:], s.lights, spp=spp, bias=s.bias, seed=seed, ids=texels, sample_base=1, stats=st2)
    assert st.rays_primary == st2.rays_primary > 0 and st.launches == 1
    want = _scatter((Hm, Wm), texels, lst, 5)
    want["irradiance"], want_owner = LR.dilate(want["irradiance"], owner, dilate)
    assert _differing(got, want) == 0
    assert np.array_equal(got["owner"], want_owner) and np.array_equal(got["owner"], dev.bake_lightmap(Wm, Hm, 1, uv=uv, dilate=dilate)[3])
    empty, filled = got["owner"] == -1, got["owner"] < -1
    assert (empty.any() or dilate > 0) and (filled.any() == (dilate > 0))
    for k in KEYS:
        assert not np.ascontiguousarray(got[k][empty]).view(np.uint8).any(), k
        if k != "irradiance":
            assert not np.ascontiguousarray(got[k][filled]).view(np.uint8).any(), k
    assert got["irradiance"].max() > 0


def test_a_chart_that_covers_nothing_launches_nothing(cornell, mcpt):
    st = mcpt.Stats()
    got = cornell.dev.bake_direct_lightmap(8, 8, cornell.lights, spp=4, uv=_chart_of(cornell.dev.scene) + 5.0, dilate=1, stats=st)
    assert (got["owner"] == -1).all() and st.rays_primary == 0 and st.launches == 0
    for k in KEYS:
        assert not got[k].view(np.uint8).any()


# ============================================================================================== 7. state
def _ask(mcpt, dev, geom, uv):
    p = geom.reshape(-1, 3)
    lo, hi = p.min(axis=0), p.max(axis=0)
    lights, bias = DC.scene_lights(mcpt, lo, hi), DC.bias_for(lo, hi)
    import query_family as QF
    q = QF.lists(mcpt, geom)
    out = []
    for mode in (mcpt.TRACE_FAST, mcpt.TRACE_REFERENCE):
        dev.set_trace_mode(mode)
        out.append(dev.direct_light(q["points"], q["normals"], lights, spp=3, bias=bias, seed=QF.SEED, ids=q["point_ids"]))
    dev.set_trace_mode(mcpt.TRACE_FAST)
    out.append(dev.bake_direct_lightmap(33, 17, lights, spp=2, uv=uv, bias=bias, seed=QF.SEED, dilate=1))
    return out


@pytest.mark.parametrize("update", ["refit", "rebuild"])
def test_after_an_update_a_fresh_devices_answers(mcpt, tmp_path_factory, update):
    import test_gpu_update as TU
    name, size = "cornell-box", SMALL["cornell-box"]
    sc, v, _, _ = TU.base(mcpt, name, tmp_path_factory, size=size)
    nv = TU.deform(mcpt, name, "rigid", tmp_path_factory)
    uv = _chart_of(sc)
    dev = mcpt.Device(sc, 0)
    before = _ask(mcpt, dev, v, uv)
    dev.update_vertices(nv, mode=update)
    after = _ask(mcpt, dev, v, uv)                              # (the same lights and list as before, on the new geometry)
    fsc, fdev = TU.fresh(mcpt, name, "rigid", 0, tmp_path_factory, size=size)
    fresh = _ask(mcpt, fdev, v, uv)
    for got, want, was in zip(after, fresh, before):
        assert _differing(got, want) == 0
        assert _differing(got, was) > 0, "the answers did not change with the geometry"
    assert np.array_equal(after[2]["owner"], fresh[2]["owner"])
    for h in (fdev, fsc, dev):
        h.close()


def test_under_a_motion_key_0_and_a_live_handle_undisturbed(mcpt, tmp_path_factory):
    import test_gpu_update as TU
    name, size = "cornell-box", SMALL["cornell-box"]
    sc, v0, _, _ = TU.base(mcpt, name, tmp_path_factory, size=size)
    v1 = TU.deform(mcpt, name, "rigid", tmp_path_factory)
    uv = _chart_of(sc)
    dev = mcpt.Device(sc, 0)
    want = _ask(mcpt, dev, v0, uv)
    dev.set_motion(v_end=v1, shutter=(0.0, 1.0), steps=3)
    dev.generateImg(3, seed=5)                                  # a motion frame: the geometry is left at the last shutter step
    assert dev.motion_info()["steps_run"] == 3
    got = _ask(mcpt, dev, v0, uv)
    for g, w in zip(got, want):
        assert _differing(g, w) == 0, "under a motion the answers are not key 0's"
    dev.clear_motion()

    def handle(interrupted):
        pr = dev.progressive(12, seed=9)
        for step in range(3):
            pr.step(4)
            if interrupted:
                for g, w in zip(_ask(mcpt, dev, v0, uv), want):
                    assert _differing(g, w) == 0
        out = (pr.image(), pr.stderr())
        pr.close()
        return out
    plain, mixed = handle(False), handle(True)
    assert plain[0].max() > 0 and TU.same(plain[0], mixed[0]) and TU.same(plain[1], mixed[1])
    dev.update_vertices(v1)                                     # ... and key 1 would have answered differently
    assert _differing(_ask(mcpt, dev, v0, uv)[0], want[0]) > 0
    dev.close()
