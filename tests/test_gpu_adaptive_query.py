"""GPU: adaptive radiance queries (mcpt_query_radiance_adaptive*).  QUERY i OF AN ADAPTIVE CALL IS, BIT FOR BIT, QUERY i OF
mcpt_query_radiance WITH spp = counts[i] (Device.radiance / Device.irradiance, which tests/test_gpu_query_oracle.py holds to the oracle);
the decisions are the numpy restatement's (tests/adaptive_query_ref.py) on the call's own samples; targets of 0 give the one-shot call;
the compaction at edge shapes, on lists whose counts follow from the rays; ids key the queries, not positions; every seam of the
integrator, the megakernel form and a pass of several chunks; both forms, live progressive handles, updated geometry, the statistics.

spp = 64 and min_spp = 4 throughout: the boundaries 4, 8, 16, 32, 64."""
import ctypes as C
import os

import numpy as np
import pytest

import adaptive_query_ref as A
import env_scenes
import hip_rt
import light_scenes
import query_cases as QC
from conftest import SCENES, extra_scene_dir
from test_gpu_query import KNOBS, SEAM_CONFIGS

pytestmark = pytest.mark.gpu

W, H = QC.W, QC.H
SPP, MIN_SPP, REL = 64, 4, 0.2
BOUNDS = (4, 8, 16, 32, 64)
BASES = (0, 2 ** 31 - 1 - 64)
SCENE_NAMES = ["cornell-box", "veach-mis", "glassroom"]
# the seams of tests/test_gpu_query.py and a workspace of 0.0101 GB, about 33 000 paths: a pass of 16 or 32 samples of a few thousand
# queries takes several chunks, whose fold starts at a slot of the active list other than 0
CONFIGS = dict(SEAM_CONFIGS, **{"chunked-pass": ({"MCPT_WORKSPACE_GB": "0.0101"}, 0, 0)})


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _base(name):
    return extra_scene_dir() if name == "glassroom" else SCENES


def _adaptive(dev, kind, q, ids, seed, base, rel=REL, abs_target=0.0, spp=SPP, min_spp=MIN_SPP, flags=0, stats=None):
    """(mean, stderr, hits, counts) of the adaptive call, the mean unscaled for either kind"""
    return dev._query_adaptive(np.ascontiguousarray(q), ids, spp, rel, abs_target, min_spp, seed, base, kind, flags, stats)


def _one_shot(dev, kind, q, ids, spp, seed, base, flags=0):
    return dev._query(np.ascontiguousarray(q), ids, spp, seed, base, kind, flags, None)


def _check_rule(dev, kind, q, ids, seed, base, got, flags=0, label=""):
    """the yardstick: every count is a boundary, and the queries that stopped at c are the one-shot call's with spp = c, bit for bit"""
    mean, err, hits, counts = got
    assert set(np.unique(counts).tolist()) <= set(BOUNDS), (label, np.unique(counts))
    for c in np.unique(counts):
        sel = np.flatnonzero(counts == c)
        # (without ids the position in the caller's list is the id)
        m1, e1, h1 = _one_shot(dev, kind, q[sel], sel.astype(np.int32) if ids is None else ids[sel], int(c), seed, base, flags)
        bad = int((_bits(mean[sel]) != _bits(m1)).sum()), int((_bits(err[sel]) != _bits(e1)).sum()), int((hits[sel] != h1).sum())
        assert bad == (0, 0, 0), "%s count %d: %d mean, %d stderr channels and %d hit counts differ from the one-shot call" % ((label, c) + bad)
    return np.unique(counts)


@pytest.fixture(scope="module")
def lists(oracle):
    """{scene: {"ray": Group, "hemisphere": Group}} of tests/query_cases.py: 5 mm in front of surfaces, and surface points"""
    out = {}
    for name in SCENE_NAMES:
        base = _base(name)
        osc = oracle.OracleScene(base + name, texture_dir=base, width=W, height=H)
        g = QC.build(osc)
        out[name] = {"ray": g["front"], "hemisphere": g["hemi"]}
        osc.close()
    return out


# ------------------------------------------------------------------------------------------------------------------ 1. the yardstick
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_an_adaptive_query_is_the_one_shot_query_at_its_own_count(mcpt, monkeypatch, lists, name):
    _env(monkeypatch, {})
    sc = mcpt.Scene(_base(name), name, width=W, height=H)
    dev = mcpt.Device(sc, 0)
    for kind_name, kind in (("ray", mcpt.QUERY_RAY), ("hemisphere", mcpt.QUERY_HEMISPHERE)):
        g = lists[name][kind_name]
        assert 0 < g.n <= 1500
        ids = g.ids["random"]
        for base in BASES:
            st = mcpt.Stats()
            got = _adaptive(dev, kind, g.q, ids, 17, base, stats=st)
            seen = _check_rule(dev, kind, g.q, ids, 17, base, got, label="%s %s base %d" % (name, kind_name, base))
            print("%s %s base %d: counts %s" % (name, kind_name, base, dict(zip(*np.unique(got[3], return_counts=True)))))
            assert seen.size >= 3, (name, kind_name, base, seen)       # a list that never stops, or always stops at once, shows nothing
            assert st.samples == int(got[3].sum()) and st.rays_primary == st.samples
    # the public methods are pi times the hemisphere answers, and the ray answers themselves
    g = lists[name]["hemisphere"]
    E, E_err, hits, counts = dev.irradiance_adaptive(g.q[:, :3], g.q[:, 3:], SPP, REL, min_spp=MIN_SPP, seed=17, ids=g.ids["random"])
    m, e, h, c = _adaptive(dev, mcpt.QUERY_HEMISPHERE, g.q, g.ids["random"], 17, 0)
    assert _same(E, np.pi * m) and _same(E_err, np.pi * e) and np.array_equal(hits, h) and np.array_equal(counts, c)
    g = lists[name]["ray"]
    r = dev.radiance_adaptive(g.q, SPP, REL, min_spp=MIN_SPP, seed=17, ids=g.ids["random"])
    m, e, h, c = _adaptive(dev, mcpt.QUERY_RAY, g.q, g.ids["random"], 17, 0)
    assert _same(r[0], m) and _same(r[1], e) and np.array_equal(r[2], h) and np.array_equal(r[3], c)
    dev.close()
    sc.close()


# --------------------------------------------------------------------------------------------------------------- 2. the decisions
@pytest.mark.parametrize("kind_name", ["ray", "hemisphere"])
def test_the_decisions_are_the_rules(mcpt, monkeypatch, lists, kind_name):
    """Every sample of 300 queries fetched as an spp = 1 call of the ray kind (the hemisphere kind's rays from the query_rays seam, as
    tests/test_gpu_sh.py fetches a probe's), folded and judged by the restatement: counts, mean, stderr and hits are equal, exactly."""
    _env(monkeypatch, {})
    sc = mcpt.Scene(SCENES, "cornell-box", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    g = lists["cornell-box"][kind_name]
    pick = np.sort(np.random.default_rng(3).permutation(g.n)[:300])
    q, ids = g.q[pick], g.ids["random"][pick]
    kind = mcpt.QUERY_RAY if kind_name == "ray" else mcpt.QUERY_HEMISPHERE
    seed = 23
    for base in BASES:
        x, hit = np.zeros((300, SPP, 3)), np.zeros((300, SPP), dtype=bool)
        for j in range(SPP):
            k = base + j
            rays = q if kind_name == "ray" else dev.query_rays(q, seed, np.full(300, k, dtype=np.int32), kind="hemisphere", ids=ids)
            x[:, j], _, h = dev.radiance(rays, 1, seed, ids=ids, sample_base=k)
            hit[:, j] = h > 0
        for rel, abs_target in ((REL, 0.0), (0.05, 0.0), (0.0, 0.5), (0.1, 0.05)):
            w_counts, w_mean, w_err, w_hits = A.answers(x, hit, SPP, MIN_SPP, rel, abs_target)
            mean, err, hits, counts = _adaptive(dev, kind, q, ids, seed, base, rel=rel, abs_target=abs_target)
            bad = (int((counts != w_counts).sum()), int((_bits(mean) != _bits(w_mean)).sum()), int((_bits(err) != _bits(w_err)).sum()),
                   int((hits != w_hits).sum()))
            print("%s base %d rel %g abs %g: %d counts, %d mean, %d stderr channels, %d hits differ; counts %s"
                  % ((kind_name, base, rel, abs_target) + bad + (dict(zip(*np.unique(counts, return_counts=True))),)))
            assert bad == (0, 0, 0, 0), (kind_name, base, rel, abs_target, bad)
    dev.close()
    sc.close()


# --------------------------------------------------------------------------------------------------------------- 3. targets of 0
def test_targets_of_zero_give_the_one_shot_call(mcpt, monkeypatch, lists):
    _env(monkeypatch, {})
    sc = mcpt.Scene(SCENES, "cornell-box", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    for kind_name, kind in (("ray", mcpt.QUERY_RAY), ("hemisphere", mcpt.QUERY_HEMISPHERE)):
        g = lists["cornell-box"][kind_name]
        ids = g.ids["random"]
        for flags in (0, mcpt.RENDER_MEGAKERNEL):
            want = _one_shot(dev, kind, g.q, ids, SPP, 5, 3, flags)
            assert want[0].max() > 0
            st = mcpt.Stats()
            for min_spp, passes in ((MIN_SPP, 5), (100, 1)):              # min_spp above spp: one pass
                mean, err, hits, counts = _adaptive(dev, kind, g.q, ids, 5, 3, rel=0.0, abs_target=0.0, min_spp=min_spp, flags=flags, stats=st)
                assert (counts == SPP).all()
                assert _same(mean, want[0]) and _same(err, want[1]) and np.array_equal(hits, want[2]), (kind_name, flags, min_spp)
                assert st.samples == g.n * SPP and st.rays_primary == g.n * SPP
            # a target so large that everything stops at once is the one-shot call of 4 samples
            mean, err, hits, counts = _adaptive(dev, kind, g.q, ids, 5, 3, rel=0.0, abs_target=1e100, flags=flags)
            want4 = _one_shot(dev, kind, g.q, ids, 4, 5, 3, flags)
            assert (counts == 4).all() and _same(mean, want4[0]) and _same(err, want4[1]) and np.array_equal(hits, want4[2])
    dev.close()
    sc.close()


# ---------------------------------------------------------------------------------------------------- 4. compaction at edge shapes
@pytest.fixture(scope="module")
def lamp_room(mcpt):
    """cornell-box, its device, and two families of rays from inside the room: up at the lamp from below its footprint, and
    down at what lies under it (the floor or a box top: diffuse)"""
    saved = {k: os.environ.pop(k) for k in KNOBS if k in os.environ}
    sc = mcpt.Scene(SCENES, "cornell-box", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    os.environ.update(saved)
    g, mat, _ = sc.faces()
    _, radiance, light_mat, _ = sc.light(0)
    v = g[mat == light_mat, 0:9].reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    assert hi[1] - lo[1] < 1e-3 * (hi[0] - lo[0])                    # the lamp is a flat patch in a plane of constant y
    assert all(float(r).is_integer() and r > 0 for r in radiance)    # ... whose radiance four additions and the division leave exact
    rng = np.random.default_rng(9)
    n = 1025
    o = np.zeros((n, 3))
    o[:, 0] = 0.5 * (lo[0] + hi[0]) + (hi[0] - lo[0]) * rng.uniform(-0.4, 0.4, n)
    o[:, 2] = 0.5 * (lo[2] + hi[2]) + (hi[2] - lo[2]) * rng.uniform(-0.4, 0.4, n)
    o[:, 1] = lo[1] - 0.3
    # (a shade off the axis: the reference's slab test, which the device reproduces, loses rays with a direction component of exactly 0)
    lamp = np.concatenate([o, np.tile(QC.unit([0.01, 1.0, 0.013]), (n, 1))], axis=1)
    wall = np.concatenate([o, np.tile(QC.unit([0.01, -1.0, 0.013]), (n, 1))], axis=1)
    # what the counts are derived from: a lamp ray's first hit is the emitter, a wall ray's is not and is diffuse
    f_lamp, f_wall = dev.ray_intersect(lamp)[0], dev.ray_intersect(wall)[0]
    assert (f_lamp >= 0).all() and (mat[f_lamp] == light_mat).all()
    assert (f_wall >= 0).all() and (mat[f_wall] != light_mat).all()
    for m in np.unique(mat[f_wall]):
        rec = sc.material(int(m))[1]
        assert rec[:3].max() > 0 and not rec[3:6].any()              # Kd > 0, Ks = 0
    yield dev, lamp, wall, np.asarray(radiance, dtype=np.float64)
    dev.close()
    sc.close()


PATTERNS = ("all-lamp", "all-wall", "alternating", "first-64-lamp", "last-wall")


def _pattern(name, n):
    """True where the ray looks at the lamp"""
    i = np.arange(n)
    return {"all-lamp": i >= 0, "all-wall": i < 0, "alternating": i % 2 == 0, "first-64-lamp": i < 64, "last-wall": i < n - 1}[name]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_compaction_at_edge_shapes(mcpt, lamp_room, n):
    """Every sample of a lamp ray is the lamp's radiance: its variance is exactly 0 and it stops at b_0 = 4.  A wall ray's samples differ,
    and rel_target = 1e-6 asks for a million times less noise than 64 samples leave: it never stops.  So the counts are 4 or 64 by the
    ray's kind -- derived from the list, not measured -- for lists around the wave and block sizes of the compaction."""
    dev, lamp, wall, radiance = lamp_room
    rng = np.random.default_rng(n)
    for pattern in PATTERNS:
        is_lamp = _pattern(pattern, n)
        q = np.ascontiguousarray(np.where(is_lamp[:, None], lamp[:n], wall[:n]))
        ids = rng.integers(0, 2 ** 31 - 1, size=n).astype(np.int32)
        st = mcpt.Stats()
        got = _adaptive(dev, mcpt.QUERY_RAY, q, ids, 31, 0, rel=1e-6, stats=st)
        mean, err, hits, counts = got
        assert np.array_equal(counts, np.where(is_lamp, 4, 64)), (n, pattern, counts)
        assert st.samples == int(4 * is_lamp.sum() + 64 * (~is_lamp).sum()) and st.rays_primary == st.samples
        if pattern == "all-lamp":
            assert st.samples == 4 * n                                # the list is empty after the first pass: nothing more is launched
        assert _same(mean[is_lamp], np.tile(radiance, (int(is_lamp.sum()), 1))) and not err[is_lamp].any() and (hits[is_lamp] == 4).all()
        assert (hits[~is_lamp] == 64).all() and (err[~is_lamp] > 0).any(axis=1).all()
        _check_rule(dev, mcpt.QUERY_RAY, q, ids, 31, 0, got, label="n %d %s" % (n, pattern))


# ------------------------------------------------------------------------------------------------------------ 5. keys, not positions
def test_keys_not_positions(mcpt, monkeypatch, lists):
    _env(monkeypatch, {})
    sc = mcpt.Scene(SCENES, "veach-mis", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    rng = np.random.default_rng(4)
    for kind_name, kind in (("ray", mcpt.QUERY_RAY), ("hemisphere", mcpt.QUERY_HEMISPHERE)):
        g = lists["veach-mis"][kind_name]
        ids = g.ids["random"]
        a = _adaptive(dev, kind, g.q, ids, 8, 0)
        assert np.unique(a[3]).size >= 2
        perm = rng.permutation(g.n)
        b = _adaptive(dev, kind, g.q[perm], ids[perm], 8, 0)
        assert _same(b[0], a[0][perm]) and _same(b[1], a[1][perm]) and np.array_equal(b[2], a[2][perm]) and np.array_equal(b[3], a[3][perm])
        c = _adaptive(dev, kind, g.q, None, 8, 0)
        d = _adaptive(dev, kind, g.q, np.arange(g.n, dtype=np.int32), 8, 0)
        assert _same(c[0], d[0]) and _same(c[1], d[1]) and np.array_equal(c[2], d[2]) and np.array_equal(c[3], d[3])
        assert np.unique(c[3]).size >= 2
        _check_rule(dev, kind, g.q, None, 8, 0, c, label="veach-mis %s, no ids" % kind_name)
    dev.close()
    sc.close()


# ------------------------------------------------------------------------------------------------------------------------ 6. seams
@pytest.fixture(scope="module")
def seam_cases(oracle, tmp_path_factory):
    """[(label, directory, scene, sky or None, light pick or None, kind, list, ids)]: the lat-long sky on the open scene with the far
    group's rays, many of which miss and carry Le(d); the room of 9 lights under both picks with surface points, three times over under
    other ids so that a pass is longer than a small workspace"""
    d = str(tmp_path_factory.mktemp("gpu_adaptive_query_scenes")) + os.sep
    env_scenes.open_scene(d, "aq_open", 1, W, H)
    light_scenes.write(d, "aq_room9", 9, W, H)
    rng = np.random.default_rng(6)
    out = []
    osc = oracle.OracleScene(d + "aq_open", texture_dir=d, width=W, height=H)
    far = QC.build(osc)["far"]
    osc.close()
    q = np.tile(far.q, (4, 1))
    out.append(("open-sky", d, "aq_open", "map", None, 0, q, rng.integers(0, 2 ** 31 - 1, size=q.shape[0]).astype(np.int32)))
    osc = oracle.OracleScene(d + "aq_room9", texture_dir=d, width=W, height=H)
    hemi = QC.build(osc)["hemi"]
    osc.close()
    q = np.tile(hemi.q, (3, 1))
    ids = rng.integers(0, 2 ** 31 - 1, size=q.shape[0]).astype(np.int32)
    out.append(("room9-one", d, "aq_room9", None, "one", 1, q, ids))
    out.append(("room9-tree", d, "aq_room9", None, "tree", 1, q, ids))
    return out


_DEFAULT = {}           # label -> the default device's answers and trace launches: computed once per module


def _seam_run(mcpt, case, mode, flags):
    label, d, name, sky, pick, kind, q, ids = case
    sc = mcpt.Scene(d, name, width=W, height=H)
    dev = mcpt.Device(sc, 0)
    if mode:
        dev.set_trace_mode(mcpt.TRACE_REFERENCE)
    if sky:
        dev.set_environment(*env_scenes.SKIES[sky])
    if pick:
        dev.set_light_sampling(pick)
    st = mcpt.Stats()
    got = _adaptive(dev, kind, q, ids, 13, 0, flags=flags, stats=st)
    dev.close()
    sc.close()
    return got, st.launches, st.samples


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_every_seam_gives_the_default_devices_bits_and_counts(mcpt, monkeypatch, seam_cases, config):
    env, mode, flags = CONFIGS[config]
    for case in seam_cases:
        label = case[0]
        if label not in _DEFAULT:
            _env(monkeypatch, {})
            _DEFAULT[label] = _seam_run(mcpt, case, 0, 0)
            mean, err, hits, counts = _DEFAULT[label][0]
            print("%s: %d queries, counts %s, %d launches" % (label, counts.size, dict(zip(*np.unique(counts, return_counts=True))), _DEFAULT[label][1]))
            assert np.unique(counts).size >= 3 and mean.max() > 0
            if label == "open-sky":
                missed = hits == 0
                assert missed.sum() > 100 and (mean[missed] > 0).any() and (counts[missed] < SPP).any()     # missed rays carry Le(d) and stop
        _env(monkeypatch, env)
        (mean, err, hits, counts), launches, samples = _seam_run(mcpt, case, mode, flags)
        (m0, e0, h0, c0), launches0, samples0 = _DEFAULT[label]
        bad = int((counts != c0).sum()), int((_bits(mean) != _bits(m0)).sum()), int((_bits(err) != _bits(e0)).sum()), int((hits != h0).sum())
        assert bad == (0, 0, 0, 0), "%s under %s: %d counts, %d mean and %d stderr channels, %d hit counts differ from the default device's" % ((label, config) + bad)
        assert samples == samples0 == int(c0.sum())
        if config == "chunked-pass":
            print("%s: %d trace launches against the default device's %d" % (label, launches, launches0))
            if label != "open-sky":                                      # (half of its rays miss and stop after the first pass)
                assert launches > launches0, (label, launches, launches0)    # more trace launches: a pass took more than one chunk


# ---------------------------------------------------------------------------------------------------------- 7. forms and neighbours
def _device_form(mcpt, dev, kind, q, ids, seed, stream, want=(True, True, True), flags=0):
    """mcpt_query_radiance_adaptive_device with stats == NULL on `stream`; want: which of stderr3, hits, counts are asked for"""
    n = q.shape[0]
    hip_rt.set_device(0)
    d_q, d_ids = hip_rt.DeviceBuffer(q.nbytes), hip_rt.DeviceBuffer(ids.nbytes)
    hip_rt.check(hip_rt.hip().hipMemcpy(d_q.ptr, q.ctypes.data_as(C.c_void_p), q.nbytes, 1))
    hip_rt.check(hip_rt.hip().hipMemcpy(d_ids.ptr, ids.ctypes.data_as(C.c_void_p), ids.nbytes, 1))
    bufs = [hip_rt.DeviceBuffer(n * 24), hip_rt.DeviceBuffer(n * 24), hip_rt.DeviceBuffer(n * 4), hip_rt.DeviceBuffer(n * 4)]
    qp = mcpt.QueryParams(SPP, 0, seed, kind, flags, (C.c_int32 * 2)(0, 0))
    ap = mcpt.AdaptiveParams(REL, 0.0, MIN_SPP, 0)
    ptr = [bufs[0].ptr] + [b.ptr if w else None for b, w in zip(bufs[1:], want)]
    rc = mcpt.lib().mcpt_query_radiance_adaptive_device(dev._h, d_q.ptr, d_ids.ptr, n, C.byref(qp), C.byref(ap), ptr[0], ptr[1], ptr[2], ptr[3], None,
                                                        stream.h)
    assert rc == 0, mcpt.lib().mcpt_last_error()
    out = [np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)]
    for b, o in zip(bufs, out):
        b.to_host_async(o, stream.h)
    stream.synchronize()
    for b in bufs + [d_q, d_ids]:
        b.free()
    return out


def test_forms_and_neighbours(mcpt, monkeypatch, lists):
    _env(monkeypatch, {})
    sc = mcpt.Scene(SCENES, "veach-mis", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    stream = hip_rt.Stream()
    g = lists["veach-mis"]["hemisphere"]
    q, ids = g.q, g.ids["random"]
    kind = mcpt.QUERY_HEMISPHERE
    st = mcpt.Stats()
    host = _adaptive(dev, kind, q, ids, 21, 0, stats=st)
    assert np.unique(host[3]).size >= 3
    assert st.samples == int(host[3].sum()) and st.rays_primary == st.samples and st.launches > 0
    # the device form on a side stream is the host form, and every optional output may be left out
    for flags in (0, mcpt.RENDER_MEGAKERNEL):
        ref = host if flags == 0 else _adaptive(dev, kind, q, ids, 21, 0, flags=flags)
        for want in ((True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False)):
            out = _device_form(mcpt, dev, kind, q, ids, 21, stream, want, flags)
            assert _same(out[0], ref[0]), (flags, want)
            for i, w in enumerate(want):
                if w:
                    assert np.array_equal(out[1 + i].view(np.uint8), np.ascontiguousarray(ref[1 + i]).view(np.uint8)), (flags, want, i)
                else:
                    assert not out[1 + i].any()                      # (its buffer was never handed over)
    # ... in the host form as well
    L = mcpt.lib()
    PD, P32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    qp = mcpt.QueryParams(SPP, 0, 21, kind, 0, (C.c_int32 * 2)(0, 0))
    ap = mcpt.AdaptiveParams(REL, 0.0, MIN_SPP, 0)
    for leave in range(3):
        mean, err, hits, counts = np.zeros((g.n, 3)), np.zeros((g.n, 3)), np.zeros(g.n, dtype=np.int32), np.zeros(g.n, dtype=np.int32)
        args = [err.ctypes.data_as(PD), hits.ctypes.data_as(P32), counts.ctypes.data_as(P32)]
        args[leave] = None
        assert L.mcpt_query_radiance_adaptive(dev._h, q.ctypes.data_as(PD), ids.ctypes.data_as(P32), g.n, C.byref(qp), C.byref(ap), mean.ctypes.data_as(PD),
                                              args[0], args[1], args[2], None) == 0
        assert _same(mean, host[0])
        for i, a in enumerate((err, hits, counts)):
            assert not a.any() if i == leave else np.array_equal(a.view(np.uint8), np.ascontiguousarray(host[1 + i]).view(np.uint8))
    # an empty list is not an error
    e = _adaptive(dev, kind, np.zeros((0, 6)), None, 21, 0)
    assert all(a.shape[0] == 0 for a in e)
    # a live progressive handle steps to the same frame with adaptive calls in between
    runs = []
    for interrupted in (False, True):
        pr = dev.progressive(16, seed=4)
        pr.step(4)
        if interrupted:
            _adaptive(dev, kind, q, ids, 4, 0)
            _adaptive(dev, kind, q[:99], ids[:99], 9, 0, flags=mcpt.RENDER_MEGAKERNEL, stats=mcpt.Stats())
            _device_form(mcpt, dev, kind, q, ids, 4, stream)
        pr.step(4)
        runs.append((pr.image(), pr.stderr()))
        pr.close()
    assert _same(runs[0][0], runs[1][0]) and _same(runs[0][1], runs[1][1])
    stream.destroy()
    dev.close()
    sc.close()


def test_updated_geometry(mcpt, monkeypatch):
    """After update_vertices the call is a fresh device's: the generated scene of tests/test_gpu_lightmap.py, its surface points taken
    from the updated geometry's own texel list"""
    import test_gpu_lightmap as TL
    _env(monkeypatch, {})
    uv, v, vn, mat = TL._soup()
    rng = np.random.default_rng(4)
    v2 = v * 1.25 + rng.uniform(-0.05, 0.05, size=v.shape)
    v2[TL.FLAT, 3:6] = v2[TL.FLAT, 0:3]
    v2[TL.FLAT, 6:9] = v2[TL.FLAT, 0:3]
    sc = TL._soup_scene(mcpt, uv, v, vn, mat)
    dev = mcpt.Device(sc, 0)
    sc2 = TL._soup_scene(mcpt, uv, v2, vn, mat)
    fresh = mcpt.Device(sc2, 0)
    _, texels, q = fresh.lightmap_texels(64, 64)
    assert texels.size > 500
    before = _adaptive(dev, mcpt.QUERY_HEMISPHERE, q, texels, 6, 0)
    dev.update_vertices(v2)
    for flags in (0, mcpt.RENDER_MEGAKERNEL):
        after = _adaptive(dev, mcpt.QUERY_HEMISPHERE, q, texels, 6, 0, flags=flags)
        want = _adaptive(fresh, mcpt.QUERY_HEMISPHERE, q, texels, 6, 0, flags=flags)
        assert _same(after[0], want[0]) and _same(after[1], want[1]) and np.array_equal(after[2], want[2]) and np.array_equal(after[3], want[3])
        assert want[0].max() > 0 and np.unique(want[3]).size >= 2
    assert not _same(after[0], before[0])
    fresh.close()
    sc2.close()
    dev.close()
    sc.close()
