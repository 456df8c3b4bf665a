"""GPU: radiance queries (mcpt_query_radiance).  A query whose rays are a frame's camera rays, keyed by pixel, is that frame's samples bit
for bit, under every seam of the integrator; ids and sample_base key the path, not the position in the list; every path variant; the
hemisphere rays are the numpy restatement's (tests/query_ref.py) and a hemisphere query is the fold of its rays; an exact sky, a known
irradiance; progressive handles are untouched."""
import os

import numpy as np
import pytest

import light_scenes
import query_ref
from conftest import SCENES, extra_scene_dir

pytestmark = pytest.mark.gpu

W, H, N = 64, 36, 8
SCENE_NAMES = ["cornell-box", "veach-mis", "glassroom"]
KNOBS = ("MCPT_TRACE_ENGINE", "MCPT_FINISH_ENGINE", "MCPT_FINISH_PATHS", "MCPT_WORKSPACE_GB")
LENS = dict(aperture=0.02, focus_distance=0.0, jitter=True)

# (environment, trace mode, render flags): the seams of tests/test_gpu_lens.py
SEAM_CONFIGS = {
    "pool": ({"MCPT_TRACE_ENGINE": "pool"}, 0, 0),
    "vote": ({"MCPT_TRACE_ENGINE": "vote"}, 0, 0),
    "reference-walk": ({}, 1, 0),
    "finish-0": ({"MCPT_FINISH_PATHS": "0"}, 0, 0),
    "finish-500": ({"MCPT_FINISH_PATHS": "500"}, 0, 0),
    "finish-lane": ({"MCPT_FINISH_ENGINE": "lane"}, 0, 0),
    "small-workspace": ({"MCPT_WORKSPACE_GB": "0.016"}, 0, 0),
    "megakernel": ({}, 0, 2),
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _base(name):
    return extra_scene_dir() if name == "glassroom" else SCENES


def _env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _frame_rays(dev, seed):
    return dev.camera_rays(seed, np.arange(W * H, dtype=np.int32), np.zeros(W * H, dtype=np.int32))


def _bounds(dev):
    box, _ = dev.bvh_nodes()
    return np.minimum(box[0, :3], box[0, 3:]), np.maximum(box[0, :3], box[0, 3:])


@pytest.mark.parametrize("config", sorted(SEAM_CONFIGS))
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_a_frames_rays_give_the_frames_samples(mcpt, monkeypatch, name, config):
    """The camera rays of a frame as a query list keyed by pixel: mean and standard error are the progressive frame's after N samples, bit
    for bit, on every pixel whose primary ray hit; the others are exactly +0.0 with no hits."""
    env, mode, flags = SEAM_CONFIGS[config]
    _env(monkeypatch, env)
    sc = mcpt.Scene(_base(name), name, width=W, height=H)
    dev = mcpt.Device(sc, 0)
    if mode:
        dev.set_trace_mode(mcpt.TRACE_REFERENCE)
    seed = 5
    rays = _frame_rays(dev, seed)
    pr = dev.progressive(2 * N, seed=seed, flags=flags)
    pr.step(N)
    img, err = pr.image().reshape(-1, 3), pr.stderr().reshape(-1, 3)
    pr.close()
    st = mcpt.Stats()
    mean, se, hits = dev.radiance(rays, N, seed, flags=flags, stats=st)
    face = dev.ray_intersect(rays)[0]
    hit = face >= 0
    assert hit.sum() > W * H // 4
    assert np.array_equal(hits, np.where(hit, N, 0))
    bad = int((_bits(mean[hit]) != _bits(img[hit])).sum()), int((_bits(se[hit]) != _bits(err[hit])).sum())
    assert bad == (0, 0), "%s %s: %d mean and %d stderr channels differ from the progressive frame" % (name, config, bad[0], bad[1])
    zero = np.zeros(((~hit).sum(), 3))
    assert _same(mean[~hit], zero) and _same(se[~hit], zero)           # +0.0, not -0.0
    assert st.rays_primary == W * H * N and st.samples == W * H * N
    dev.close()
    sc.close()


def _check_keys(dev, rays_of, seed, rng, flags=0):
    """radiance(rays[pix], 1, ids=pix, sample_base=k) is sample_radiance(seed, pix, k), bit for bit"""
    for k in (0, 5, 63):
        pix = rng.permutation(W * H)[:100].astype(np.int32)
        want = dev.sample_radiance(seed, pix, np.full(100, k, dtype=np.int32))
        mean, se, hits = dev.radiance(rays_of(pix, k), 1, seed, ids=pix, sample_base=k, flags=flags)
        assert _same(mean, want), k
        assert _same(se, np.zeros((100, 3)))
        yield pix, k, mean, hits


def test_ids_and_sample_base_key_the_path(mcpt, monkeypatch):
    _env(monkeypatch, {})
    sc = mcpt.Scene(SCENES, "cornell-box", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    seed = 0x1234567887654321
    rng = np.random.default_rng(3)
    rays = _frame_rays(dev, seed)
    for flags in (0, mcpt.RENDER_MEGAKERNEL):
        seen = list(_check_keys(dev, lambda pix, k: rays[pix], seed, rng, flags))
        assert sum(int(h.sum()) for _, _, _, h in seen) > 100
    # the same under a real lens, its rays taken from the camera-ray seam: a query does not care where its rays came from
    dev.set_lens(**LENS)
    for flags in (0, mcpt.RENDER_MEGAKERNEL):
        list(_check_keys(dev, lambda pix, k: dev.camera_rays(seed, pix, np.full(pix.size, k, dtype=np.int32)), seed, rng, flags))
    dev.set_lens()
    # a split sample range continues the same sums: spp 4 at bases 0 and 4 against spp 8
    pix = rng.permutation(W * H)[:100].astype(np.int32)
    m_a = dev.radiance(rays[pix], 4, seed, ids=pix, sample_base=0)[0]
    m_b = dev.radiance(rays[pix], 4, seed, ids=pix, sample_base=4)[0]
    m_8 = dev.radiance(rays[pix], 8, seed, ids=pix)[0]
    assert m_8.max() > 0
    np.testing.assert_allclose((m_a * 4 + m_b * 4) / 8, m_8, rtol=1e-15, atol=0)
    # ids, not list positions: the list reversed gives the answers reversed
    back = dev.radiance(rays[pix][::-1], 8, seed, ids=pix[::-1])[0]
    assert _same(back[::-1], m_8)
    dev.close()
    sc.close()


@pytest.fixture(scope="module")
def room_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gpu_query_scenes")) + os.sep
    light_scenes.write(d, "room12", 12, W, H)
    return d


@pytest.mark.parametrize("variant", ["sky", "one", "tree", "sky-one"])
def test_every_path_variant(mcpt, monkeypatch, room_dir, variant):
    _env(monkeypatch, {})
    if variant == "sky":
        sc = mcpt.Scene(SCENES, "cornell-box", width=W, height=H)
    else:
        sc = mcpt.Scene(room_dir, "room12", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    if variant.startswith("sky"):
        dev.set_environment((0.3, 0.6, 1.1), 1.5)
    if variant != "sky":
        dev.set_light_sampling(variant.split("-")[-1])
    seed = 77
    rng = np.random.default_rng(8)
    rays = _frame_rays(dev, seed)
    for flags in (0, mcpt.RENDER_MEGAKERNEL):
        for pix, k, mean, hits in _check_keys(dev, lambda pix, k: rays[pix], seed, rng, flags):
            if variant.startswith("sky"):
                miss = hits == 0
                np.testing.assert_allclose(mean[miss], dev.environment_eval(rays[pix][miss, 3:]), rtol=1e-12, atol=0)
    if variant == "sky":
        assert (dev.radiance(rays, 1, seed)[2] == 0).sum() > 0           # the frame does see the sky
    dev.close()
    sc.close()


def _hemisphere_cases(rng, n):
    """positions, normals, ids, sample indices: random ones, axis-aligned normals, normals with two equal smallest components, positions
    at the origin"""
    a = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-2, 2, size=(n, 1))
    b = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 3, size=(n, 1))
    axes = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [-1.0, 0, 0], [0, -2.5, 0], [0, 0, -1e-3]])
    b[:600] = axes[np.arange(600) % 6]
    ties = np.array([[1.0, 1.0, 5.0], [3.0, -1.0, 1.0], [2.0, 7.0, -2.0], [1.0, 1.0, 1.0], [-1.0, 1.0, -1.0], [0.5, -4.0, 0.5]])
    b[600:1200] = ties[np.arange(600) % 6] * 10.0 ** rng.uniform(-2, 2, size=(600, 1))
    a[1200:1400] = 0.0
    ids = rng.integers(0, 2 ** 31, size=n).astype(np.int32)
    k = rng.integers(0, 2 ** 31, size=n).astype(np.int32)
    return np.concatenate([a, b], axis=1), ids, k


def test_hemisphere_rays_are_the_restatement(mcpt):
    """mcpt_query_rays against tests/query_ref.py within 4 ulps (the bound the thin lens holds for the same sincos and sqrt chain); every
    direction on the normal's side.  The offset: o is a + d * 0.01 in fp64, checked as exactly that sum of the device's own d -- at a
    position of size 1 the difference o - a itself carries the rounding of o, 1e-16 absolute and so 1e-14 of 0.01, which no
    implementation can avoid -- and the length of the offset vector d * 0.01 is 0.01 to 1e-15 relative; where the position is the origin,
    o - a is that vector and the literal |o - a| = 0.01 is checked as well."""
    sc = mcpt.Scene(SCENES, "cornell-box", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    q, ids, k = _hemisphere_cases(np.random.default_rng(6), 4000)
    seed = 0x0123456789ABCDEF
    got = dev.query_rays(q, seed, k, kind="hemisphere", ids=ids)
    want = query_ref.hemisphere_rays(q, seed, ids, k)
    u = query_ref.ulps(got, want)
    assert u.max() <= 4, u.max()
    _, _, nh = query_ref.basis(q[:, 3:])
    assert np.all((got[:, 3:] * nh).sum(axis=1) > 0)
    off = got[:, 3:] * 0.01
    assert _same(got[:, :3], q[:, :3] + off)
    assert np.abs(np.sqrt((off * off).sum(axis=1)) / 0.01 - 1.0).max() <= 1e-15
    at0 = slice(1200, 1400)
    d0 = got[at0, :3] - q[at0, :3]
    assert np.abs(np.sqrt((d0 * d0).sum(axis=1)) / 0.01 - 1.0).max() <= 1e-15
    # without ids the list position is the id; kind "ray" returns the rays as given
    got_pos = dev.query_rays(q, seed, k, kind="hemisphere")
    assert _same(got_pos, dev.query_rays(q, seed, k, kind="hemisphere", ids=np.arange(4000)))
    rays = got.copy()
    assert _same(dev.query_rays(rays, seed, k, kind="ray", ids=ids), rays)
    dev.close()
    sc.close()


def _surface_points(dev, rng, n):
    """points on the floor and two walls of the scene's bounding box with the (unnormalised) normals that face inwards"""
    lo, hi = _bounds(dev)
    u = lo + (hi - lo) * (0.2 + 0.6 * rng.random((n, 3)))
    nrm = np.zeros((n, 3))
    which = np.arange(n) % 3
    u[which == 0, 1] = lo[1]; nrm[which == 0] = [0.0, 2.5, 0.0]
    u[which == 1, 0] = lo[0]; nrm[which == 1] = [0.7, 0.0, 0.0]
    u[which == 2, 0] = hi[0]; nrm[which == 2] = [-1.0, 0.0, 0.0]
    return u, nrm


def test_a_hemisphere_query_is_the_fold_of_its_rays(mcpt, monkeypatch):
    _env(monkeypatch, {})
    sc = mcpt.Scene(SCENES, "cornell-box", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    rng = np.random.default_rng(12)
    p, nrm = _surface_points(dev, rng, 64)
    q = np.concatenate([p, nrm], axis=1)
    ids = rng.integers(0, 2 ** 31, size=64).astype(np.int32)
    seed, spp = 41, 8
    s1 = np.zeros((64, 3))
    nhit = np.zeros(64, dtype=np.int64)
    for j in range(spp):
        rays = dev.query_rays(q, seed, np.full(64, j, dtype=np.int32), kind="hemisphere", ids=ids)
        x, _, h = dev.radiance(rays, 1, seed, ids=ids, sample_base=j)
        s1 = s1 + x
        nhit += h
    want = s1 / spp
    assert want.max() > 0
    for flags in (0, mcpt.RENDER_MEGAKERNEL):
        E, E_err, hits = dev.irradiance(p, nrm, spp, seed, ids=ids, flags=flags)
        mean = dev._query(q, ids, spp, seed, 0, mcpt.QUERY_HEMISPHERE, flags, None)[0]
        assert _same(mean, want), flags
        assert np.array_equal(hits, nhit)
        assert _same(E, np.pi * mean) and np.all(E_err >= 0)
    dev.close()
    sc.close()


def test_exact_sky(mcpt, monkeypatch):
    """Above the scene, facing up, under a constant sky whose radiance survives eight additions and the division without rounding"""
    _env(monkeypatch, {})
    sc = mcpt.Scene(SCENES, "cornell-box", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    sky = (0.5, 0.25, 1.0)
    dev.set_environment(sky, 1.0)
    lo, hi = _bounds(dev)
    rng = np.random.default_rng(2)
    p = lo + (hi - lo) * rng.random((50, 3))
    p[:, 1] = hi[1] + 1.0
    nrm = np.tile([0.0, 1.0, 0.0], (50, 1))
    for flags in (0, mcpt.RENDER_MEGAKERNEL):
        mean, se, hits = dev._query(np.concatenate([p, nrm], axis=1), None, 8, 9, 0, mcpt.QUERY_HEMISPHERE, flags, None)
        assert _same(mean, np.tile(sky, (50, 1))) and _same(se, np.zeros((50, 3))) and not hits.any()
    dev.close()
    sc.close()


def test_known_irradiance(mcpt, monkeypatch):
    """An emitting square of side 2 and radiance 3 at height 1, facing down, over a black floor: the cosine-weighted mean at a floor point
    under it is 3 F, F the point-to-parallel-rectangle form factor summed over the four corner rectangles.  6 sigma of the estimator's own
    error; the run is deterministic."""
    _env(monkeypatch, {})
    def quad(x0, x1, z0, z1, y, up):
        a, b, c, d = [x0, y, z0], [x1, y, z0], [x1, y, z1], [x0, y, z1]
        return [a + c + b, a + d + c] if up else [a + b + c, a + c + d]
    v = np.array(quad(-1, 1, -1, 1, 1.0, False) + quad(-6, 6, -6, 6, 0.0, True), dtype=np.float64)
    vn = np.concatenate([np.tile([0.0, -1.0, 0.0], (2, 3)), np.tile([0.0, 1.0, 0.0], (2, 3))])
    rec = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0]])
    sc = mcpt.Scene.from_arrays(v, vn, np.array([0, 0, 1, 1], dtype=np.int32), rec, [0], [[3.0, 3.0, 3.0]], [0.0, 0.5, 5.0], [0.0, 0.5, 0.0],
                                [0.0, 1.0, 0.0], 60.0, W, H)
    dev = mcpt.Device(sc, 0)
    xz = np.array([[0.0, 0.0], [1.0, 1.0], [0.5, 0.0], [1.0, 0.0], [0.5, 0.5], [-1.0, -1.0], [0.25, -0.75], [-0.5, 0.5]])
    p = np.stack([xz[:, 0], np.zeros(8), xz[:, 1]], axis=1)
    nrm = np.tile([0.0, 1.0, 0.0], (8, 1))
    F = np.array([query_ref.square_form_factor(x, z, 1.0, 1.0) for x, z in xz])
    assert abs(F[0] - 0.55413) < 1e-4 and abs(F[1] - F[5]) < 1e-15
    for flags in (0, mcpt.RENDER_MEGAKERNEL):
        mean, se, hits = dev._query(np.concatenate([p, nrm], axis=1), None, 4096, 2024, 0, mcpt.QUERY_HEMISPHERE, flags, None)
        assert np.all(se > 0) and np.all(se < 0.05)
        dev_sigma = np.abs(mean - 3.0 * F[:, None]) / se
        print("known irradiance, flags %d: |mean - 3F| / stderr =" % flags, np.round(dev_sigma[:, 0], 2))
        assert np.all(np.abs(mean - 3.0 * F[:, None]) <= 6.0 * se), dev_sigma
        assert _same(mean[:, 0], mean[:, 1]) and _same(mean[:, 0], mean[:, 2])
        assert np.array_equal(hits, np.rint(mean[:, 0] / 3.0 * 4096).astype(np.int32))      # every hit is the emitter
        E, E_err, _ = dev.irradiance(p, nrm, 4096, 2024, flags=flags)
        assert _same(E, np.pi * mean) and _same(E_err, np.pi * se)
    dev.close()
    sc.close()


def test_handles_are_untouched(mcpt, monkeypatch):
    _env(monkeypatch, {})
    sc = mcpt.Scene(SCENES, "veach-mis", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    rays = _frame_rays(dev, 1)
    runs = []
    for interrupted in (False, True):
        pr = dev.progressive(16, seed=4)
        pr.step(4)
        if interrupted:
            dev.radiance(rays, 3, seed=4)
            dev.radiance(rays[:99], 2, seed=9, flags=mcpt.RENDER_MEGAKERNEL, stats=mcpt.Stats())
        pr.step(4)
        runs.append((pr.image(), pr.stderr()))
        pr.close()
    assert _same(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1])
    dev.close()
    sc.close()


def test_several_chunks(mcpt, monkeypatch):
    """MCPT_WORKSPACE_GB=0.016 holds about 52 000 paths of a one-light scene: 64 x 36 queries of 32 samples go in two chunks, whose
    source pass and fold start at a slot other than 0.  The answers are the one-chunk device's and the progressive frame's, bit for bit,
    for rays and for surface points."""
    n_s = 32
    sc = mcpt.Scene(SCENES, "cornell-box", width=W, height=H)
    rng = np.random.default_rng(5)
    ids = rng.permutation(W * H).astype(np.int32)
    out = {}
    for ws in ("", "0.016"):
        _env(monkeypatch, {"MCPT_WORKSPACE_GB": ws} if ws else {})
        dev = mcpt.Device(sc, 0)
        rays = _frame_rays(dev, 3)
        st = mcpt.Stats()
        res = dev.radiance(rays[ids], n_s, 3, ids=ids, stats=st)
        p, nrm = _surface_points(dev, np.random.default_rng(1), W * H)
        hemi = dev.irradiance(p, nrm, n_s, 3)
        pr = dev.progressive(2 * n_s, seed=3)
        pr.step(n_s)
        out[ws] = (res, hemi, st.launches, pr.image().reshape(-1, 3)[ids], pr.stderr().reshape(-1, 3)[ids])
        assert st.samples == W * H * n_s
        pr.close()
        dev.close()
    one, two = out[""], out["0.016"]
    assert two[2] > one[2]                                  # more trace launches: more than one chunk
    for a, b in zip(one[0] + one[1], two[0] + two[1]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    hit = two[0][2] > 0
    assert _same(two[0][0][hit], two[3][hit]) and _same(two[0][1][hit], two[4][hit])
    sc.close()
