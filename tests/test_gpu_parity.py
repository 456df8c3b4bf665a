"""-m gpu: the HIP path (through the C ABI) against the CPU oracle on identical inputs.

Bars: closest-hit face index, t, p, pn BIT-EXACT (fp64, no FMA contraction); per-sample radiance within
1e-9 relative (libm differences between glibc and the device math library; discrete flips are counted and
must stay below 1e-4 of the samples); images within the same tolerance per pixel."""
import numpy as np
import pytest

from conftest import SCENES, make_rays

pytestmark = pytest.mark.gpu

import os  # noqa: E402

from conftest import ROOT  # noqa: E402

REL_TOL = 1e-9

# Discrete flips, MEASURED (tools/flip_probe.py, random camera samples per scene, 160x90): cornell-box 0, veach-mis 0 of 20 000,
# glassroom 12 of 20 000 (22 of 40 000 before the shading code took 1-ulp square roots), interior 6 of 20 000 (6 of 40 000 before) --
# and every one of them sits on a path with a ray that starts ON the surface it leaves: the reference gives refraction /
# total-reflection rays no 0.01 offset (pathTracing.cpp:102,109), so whether such a ray re-hits its own triangle is decided by the
# sign of a t_x that is pure rounding noise, and a last-bit difference upstream (device libm vs glibc, the device's 1-ulp roots and
# 2-ulp reciprocals) flips it: 12 of 655 such paths in glassroom (1.8 %), 6 of 353 in interior (1.7 %).  Paths without such a ray:
# 0 flips in 79 000; the largest relative difference of an unflipped sample is 7e-13.  Budgets = 2 x observed: per sample of the
# whole scene (images), per path with an on-surface ray (sample test).
FLIP_BUDGET = {"cornell-box": 2.5e-5, "veach-mis": 2.5e-5, "glassroom": 1.2e-3, "interior": 6e-4}
ON_SURFACE_FLIP_RATE = 0.035        # of the paths that have an on-surface ray
OTHER_FLIP_RATE = 2.5e-5            # of all other paths (none observed)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


from conftest import extra_scene_dir  # noqa: E402

EXTRA = extra_scene_dir()


# glassroom (tests/scenes_extra, CRLF files): refraction incl. total internal reflection (Ni 1.5), a Phong lobe (Ns 60), a
# textured quad, and a second light larger than the first (the frozen light-area distribution Q1 then never reaches most of
# it) -- the branches the two shipped scenes do not execute.
# interior: a small instance of the generated textured interior that stands in for the reference's unshipped bedroom scene
# (synthetic.write_interior): five textured materials, smooth-shaded displaced grids, a glass and a glossy ball, two lights.
@pytest.fixture(scope="module", params=["cornell-box", "veach-mis", "glassroom", "interior"])
def pair(request, oracle, mcpt, tmp_path_factory):
    name = request.param
    w, h = (160, 90)
    base = EXTRA if name == "glassroom" else SCENES
    if name == "interior":
        from montecarlopathtracing_amd import synthetic
        base = str(tmp_path_factory.mktemp("interior")) + os.sep
        synthetic.write_interior(base, "interior", width=w, height=h, detail=0.1)
    osc = oracle.OracleScene(base + name, texture_dir=base, width=w, height=h)
    sc = mcpt.Scene(base, name, width=w, height=h)
    dev = mcpt.Device(sc, 0)
    yield name, osc, sc, dev
    for d in _ENGINE_DEVS.pop(name, {}).values():
        d.close()
    for k in [k for k in _ORACLE_CACHE if k[0] == name]:
        del _ORACLE_CACHE[k]
    dev.close()
    sc.close()
    osc.close()


# The library picks the closest-hit engine by scene size (every test scene here is small: the pool engine).  The tests that hold the
# HIP path to the ORACLE directly run once per engine -- the voting engine is what BASELINE configs 4 and 5 use -- on a device created
# with MCPT_TRACE_ENGINE forced; what the oracle says is computed once per scene and kept for the second engine.
_ENGINE_DEVS = {}
_ORACLE_CACHE = {}
ENGINES = ["pool", "vote"]


def _engine_device(pair, mcpt, engine):
    name, osc, sc, dev = pair
    devs = _ENGINE_DEVS.setdefault(name, {})
    if engine not in devs:
        old = os.environ.get("MCPT_TRACE_ENGINE")
        os.environ["MCPT_TRACE_ENGINE"] = engine
        try:
            assert sc.trace_engine() == engine
            devs[engine] = mcpt.Device(sc, 0)
        finally:
            if old is None:
                del os.environ["MCPT_TRACE_ENGINE"]
            else:
                os.environ["MCPT_TRACE_ENGINE"] = old
    return devs[engine]


def _cached(name, what, fn):
    key = (name, what)
    if key not in _ORACLE_CACHE:
        _ORACLE_CACHE[key] = fn()
    return _ORACLE_CACHE[key]


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("mode", ["reference", "fast"])
def test_closest_hit_bit_exact(pair, oracle, mcpt, mode, engine):
    name, osc, sc, _ = pair
    if mode == "reference" and engine == "vote":
        pytest.skip("the reference-shaped walk has no engine: covered by the pool-parametrised run")
    dev = _engine_device(pair, mcpt, engine)
    rays = make_rays(osc, 40000, seed=11)
    of, ot, op, opn = _cached(name, "closest", lambda: osc.trace_closest(rays))
    st = mcpt.Stats()
    dev.set_trace_mode(mcpt.TRACE_REFERENCE if mode == "reference" else mcpt.TRACE_FAST)
    try:
        gf, gt, gp, gpn = dev.ray_intersect(rays, stats=st)
    finally:
        dev.set_trace_mode(mcpt.TRACE_FAST)
    assert np.array_equal(of, gf), "closest-hit face index differs on %d rays" % int((of != gf).sum())
    hit = of >= 0
    assert hit.sum() > 1000
    assert np.array_equal(_bits(ot[hit]), _bits(gt[hit]))
    assert np.array_equal(_bits(op[hit]), _bits(gp[hit]))
    assert np.array_equal(_bits(opn[hit]), _bits(gpn[hit]))
    if mode == "reference":      # same walk -> same work
        ost = oracle.Stats()
        osc.trace_closest(rays, stats=ost)
        assert st.node_visits == ost.box_tests and st.tri_tests == ost.tri_tests


def test_fast_walk_equals_reference_walk_bulk(pair, mcpt):
    """2 M rays, GPU against GPU: the accelerated walk must return the reference-shaped walk's answer bit for bit
    (the latter is pinned to the oracle above).  Includes rays leaving surface points (the shadow/bounce pattern)."""
    name, osc, sc, dev = pair
    rng = np.random.default_rng(2024)
    base = make_rays(osc, 200000, seed=3)
    f0, t0, p0, _ = dev.ray_intersect(base)
    hit = f0 >= 0
    # secondary rays from hit points: random directions and grazing directions, origin offset like nextRay / shade
    o = p0[hit]
    n2 = o.shape[0]
    d = rng.normal(size=(n2, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sec = np.hstack([o + 0.01 * d, d])
    sec2 = np.hstack([o, d])                      # refraction rays start exactly on the surface
    reps = []
    for s_ in range(8):
        reps.append(make_rays(osc, 200000, seed=100 + s_))
    rays = np.vstack([base, sec, sec2] + reps)
    dev.set_trace_mode(mcpt.TRACE_REFERENCE)
    rf, rt, rp, rpn = dev.ray_intersect(rays)
    dev.set_trace_mode(mcpt.TRACE_FAST)
    st = mcpt.Stats()
    ff, ft, fp, fpn = dev.ray_intersect(rays, stats=st)
    assert np.array_equal(rf, ff), "%d of %d rays differ" % (int((rf != ff).sum()), rays.shape[0])
    h = rf >= 0
    assert np.array_equal(_bits(rt[h]), _bits(ft[h])) and np.array_equal(_bits(rp[h]), _bits(fp[h]))
    assert np.array_equal(_bits(rpn[h]), _bits(fpn[h]))


def test_deferred_ray_list_overflow(oracle, mcpt, monkeypatch):
    """Rays with a zero direction component are deferred to the reference-shaped walk through a side list; with the list
    shrunk to 8 entries the second pass must recognise them by scanning.  Results stay bit-exact."""
    monkeypatch.setenv("MCPT_SLOW_LIST", "8")
    osc = oracle.OracleScene(SCENES + "veach-mis", texture_dir=SCENES, width=64, height=48)
    sc = mcpt.Scene(SCENES, "veach-mis", width=64, height=48)
    dev = mcpt.Device(sc, 0)
    rays = make_rays(osc, 20000, seed=77)
    assert int((rays[:, 3:] == 0).any(axis=1).sum()) > 100
    of, ot, op, opn = osc.trace_closest(rays)
    gf, gt, gp, gpn = dev.ray_intersect(rays)
    assert np.array_equal(of, gf)
    h = of >= 0
    assert np.array_equal(_bits(ot[h]), _bits(gt[h])) and np.array_equal(_bits(opn[h]), _bits(gpn[h]))
    dev.close()
    sc.close()
    osc.close()


def test_stack_overflow_is_handed_to_the_one_lane_walk(oracle, mcpt, monkeypatch):
    """The trace engine runs with a 27-entry stack per lane (4 waves per SIMD) on a hierarchy that may need up to 35 entries in the
    worst case; a ray that would push past its stack is handed to the one-lane walk, which has the deep stack.  No ray of the
    measured scenes does, so the hand-over is forced here: with the engine's stack cut to 6 entries a good share of the rays take
    it, and closest hits and images stay bit-exact."""
    monkeypatch.setenv("MCPT_TEST_STACK_CAP", "6")
    monkeypatch.setenv("MCPT_FINISH_PATHS", "0")
    osc = oracle.OracleScene(SCENES + "cornell-box", texture_dir=SCENES, width=160, height=90)
    sc = mcpt.Scene(SCENES, "cornell-box", width=160, height=90)
    dev = mcpt.Device(sc, 0)
    rays = make_rays(osc, 40000, seed=19)
    of, ot, op, opn = osc.trace_closest(rays)
    gf, gt, gp, gpn = dev.ray_intersect(rays)
    assert np.array_equal(of, gf)
    h = of >= 0
    assert np.array_equal(_bits(ot[h]), _bits(gt[h])) and np.array_equal(_bits(op[h]), _bits(gp[h])) and np.array_equal(_bits(opn[h]), _bits(gpn[h]))
    st = mcpt.Stats()
    a = dev.generateImg(8, seed=3, stats=st)
    b = dev.generateImg(8, seed=3, flags=mcpt.RENDER_MEGAKERNEL)
    assert np.array_equal(_bits(a), _bits(b))
    dev.close()
    monkeypatch.delenv("MCPT_TEST_STACK_CAP")
    plain = mcpt.Device(sc, 0)
    st0 = mcpt.Stats()
    c = plain.generateImg(8, seed=3, stats=st0)
    assert np.array_equal(_bits(a), _bits(c))
    assert st.dom_node_visits < 0.8 * st0.dom_node_visits      # the engine really gave rays away (its own node visits dropped)
    plain.close(); sc.close(); osc.close()


@pytest.mark.parametrize("engine", ENGINES)
def test_sample_radiance(pair, oracle, mcpt, engine):
    name, osc, sc, _ = pair
    dev = _engine_device(pair, mcpt, engine)
    rng = np.random.default_rng(5)
    n = 6000
    pix = rng.integers(0, osc.width * osc.height, size=n).astype(np.int32)
    k = rng.integers(0, 64, size=n).astype(np.int32)
    g = dev.sample_radiance(77, pix, k)

    def from_oracle():
        o = np.zeros((n, 3))
        on_surface = np.zeros(n, dtype=bool)        # the path has a refraction / total-reflection ray (starts on the surface)
        for i, (p, kk) in enumerate(zip(pix, k)):
            st = oracle.Stats()
            o[i] = osc.sample_radiance(77, int(p // osc.width), int(p % osc.width), int(kk), stats=st)
            on_surface[i] = st.rays_on_surface > 0
        return o, on_surface
    o, on_surface = _cached(name, "samples", from_oracle)
    # a NaN compares false with everything: without this a NaN sample would count as "not flipped"
    assert np.array_equal(np.isnan(g), np.isnan(o)), "NaN masks differ on %d samples" % int((np.isnan(g) != np.isnan(o)).any(axis=1).sum())
    scale = np.maximum(np.abs(o).max(axis=1), 1e-12)
    err = np.abs(g - o).max(axis=1) / scale
    flip = err > REL_TOL
    assert int((flip & ~on_surface).sum()) <= int(n * OTHER_FLIP_RATE), "radiance mismatch on %d ordinary samples (max rel %.3e)" % (
        int((flip & ~on_surface).sum()), err[~on_surface].max())
    assert int((flip & on_surface).sum()) <= max(2, int(on_surface.sum() * ON_SURFACE_FLIP_RATE) + 1), (int((flip & on_surface).sum()), int(on_surface.sum()))
    if name in ("glassroom", "interior"):
        assert on_surface.sum() > 50
    assert np.abs(o).sum() > 0
    same = ~flip
    assert abs(g[same].sum() - o[same].sum()) <= 1e-9 * abs(o[same]).sum()


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("pipeline", ["wavefront", "megakernel"])
def test_image_matches_oracle(pair, oracle, mcpt, pipeline, engine):
    name, osc, sc, _ = pair
    if pipeline == "megakernel" and engine == "vote":
        pytest.skip("the megakernel walks the reference-shaped tree one lane per sample: no engine involved beyond the primary rays")
    dev = _engine_device(pair, mcpt, engine)
    spp = 8

    def from_oracle():
        ost = oracle.Stats()
        return osc.render(spp, seed=3, stats=ost), ost
    ref, ost = _cached(name, "image", from_oracle)
    st = mcpt.Stats()
    img = dev.generateImg(spp, seed=3, stats=st, flags=mcpt.RENDER_MEGAKERNEL if pipeline == "megakernel" else 0)
    assert img.shape == ref.shape
    assert np.array_equal(np.isnan(img), np.isnan(ref)), "NaN masks differ on %d channels" % int((np.isnan(img) != np.isnan(ref)).sum())
    scale = np.maximum(np.abs(ref), 1e-6)
    rel = np.abs(img - ref) / scale
    bad = int((rel > 1e-6).sum())      # float accumulator: 1 ulp of fp32 ~ 6e-8
    budget = max(3, int(img.size * spp * FLIP_BUDGET[name]))      # img.size counts channels: 3 per flipped sample
    assert bad <= budget, "%d pixel channels differ (max rel %.3e)" % (bad, rel.max())
    # a flipped sample can be a firefly (radiance / 0.6^depth): the image mean moves with the flip budget
    assert abs(img.mean() - ref.mean()) <= (2e-3 + 25 * FLIP_BUDGET[name]) * ref.mean()
    assert (rel <= 1e-6).mean() >= 0.97
    if name not in ("glassroom", "interior"):   # same work was done (a flipped path does different work)
        assert st.rays_shadow + st.shadow_skipped == ost.rays_shadow and st.rays_bounce == ost.rays_bounce
        assert st.shade_calls == ost.shade_calls
    assert st.samples == ost.samples
    assert int((mcpt.imshow_rgb8(img) != oracle.quantize(ref)).sum()) <= max(8, budget)


def test_pipelines_agree_bitwise(pair, mcpt):
    """wavefront + fast walk vs megakernel + reference walk: same arithmetic per sample, so the same bits."""
    name, osc, sc, dev = pair
    a = dev.generateImg(16, seed=21)
    b = dev.generateImg(16, seed=21, flags=mcpt.RENDER_MEGAKERNEL)
    assert np.array_equal(_bits(a), _bits(b)), "%d channels differ" % int((_bits(a) != _bits(b)).sum())


def test_partition_independent(pair, mcpt):
    name, osc, sc, dev = pair
    full = dev.generateImg(4, seed=9)
    parts = np.zeros_like(full)
    for r in range(3):
        dev.generateImg(4, seed=9, rank=r, world=3, img=parts)
    assert np.array_equal(_bits(full), _bits(parts))


def test_chunked_frame_equals_single_chunk(mcpt, monkeypatch):
    """By default the path state of a whole frame sits in HBM at once; with a 16-MB workspace the same frame takes dozens of
    chunks (and the small tail launches of each).  Same samples, same arithmetic: the same bits."""
    monkeypatch.setenv("MCPT_FINISH_PATHS", "500")        # keep the wavefront iterations going in the small chunks too
    monkeypatch.delenv("MCPT_WORKSPACE_GB", raising=False)
    sc = mcpt.Scene(SCENES, "cornell-box", width=160, height=120)
    one = mcpt.Device(sc, 0)
    st1 = mcpt.Stats()
    a = one.generateImg(12, seed=4, stats=st1)
    one.close()
    monkeypatch.setenv("MCPT_WORKSPACE_GB", "0.016")
    many = mcpt.Device(sc, 0)
    st2 = mcpt.Stats()
    b = many.generateImg(12, seed=4, stats=st2)
    many.close()
    sc.close()
    assert st2.launches > 2 * st1.launches
    assert np.array_equal(_bits(a), _bits(b))
    assert (st1.rays_shadow + st1.shadow_skipped, st1.rays_bounce, st1.shade_calls) == (st2.rays_shadow + st2.shadow_skipped, st2.rays_bounce, st2.shade_calls)


@pytest.mark.parametrize("finish_paths", ["0", "500"])
@pytest.mark.parametrize("mode", ["fast", "reference"])
def test_wavefront_iterations_against_megakernel_and_oracle(pair, oracle, mcpt, monkeypatch, finish_paths, mode):
    """The path the full-size frames take: with the hand-over to k_wf_finish switched off (0) or pushed to the last 500 paths,
    every bounce of the 160x90 frames runs k_wf_logic<false> (resolve + shade), WfRaySource fetch/store in k_wf_trace (fast) or
    k_wf_trace_reference, the T/L folding of the one-light case and the unfolded state of the several-light scenes.  Held to
    the megakernel (one lane per sample, reference-shaped walk) bit for bit and to the oracle inside the flip budget.
    MCPT_FINISH_PATHS is read when the device is created, hence a device of its own."""
    name, osc, sc, dev0 = pair
    monkeypatch.setenv("MCPT_FINISH_PATHS", finish_paths)
    dev = mcpt.Device(sc, 0)
    try:
        dev.set_trace_mode(mcpt.TRACE_REFERENCE if mode == "reference" else mcpt.TRACE_FAST)
        spp = 8
        st = mcpt.Stats()
        a = dev.generateImg(spp, seed=3, stats=st)
        b = dev.generateImg(spp, seed=3, flags=mcpt.RENDER_MEGAKERNEL)
        assert np.array_equal(_bits(a), _bits(b)), "%d channels differ from the megakernel" % int((_bits(a) != _bits(b)).sum())
        assert st.launches >= 5, st.launches                  # the bounce loop really ran as wavefront iterations
        if mode == "fast" and finish_paths == "0":
            assert st.dom_rays > 0.9 * (st.rays_shadow + st.rays_bounce)     # ... and its rays went through k_wf_trace
        ref = osc.render(spp, seed=3)
        assert np.array_equal(np.isnan(a), np.isnan(ref)), "NaN masks differ on %d channels" % int((np.isnan(a) != np.isnan(ref)).sum())
        rel = np.abs(a - ref) / np.maximum(np.abs(ref), 1e-6)
        bad = int((rel > 1e-6).sum())
        assert bad <= max(3, int(a.size * spp * FLIP_BUDGET[name])), "%d pixel channels differ from the oracle" % bad
    finally:
        dev.close()


def test_logic_ring_many_rounds_in_two_blocks(pair, mcpt, monkeypatch):
    """The later passes of k_wf_logic resolve in rounds of 512 positions per block, park the vertices that go on in a ring in LDS
    (1024 slots) and shade them 256 at a time, every wave full (wavefront_logic.hip).  With the logic grid forced down to two blocks
    (MCPT_LOGIC_GRID=2) a 160x90 SPP-16 frame -- 230 k samples, some 100 k positions in the first later pass -- takes each block
    through a hundred resolve rounds: the ring wraps dozens of times, resolve rounds that leave fewer than 256 vertices waiting are
    followed by another, the drain at the end shades a partial round.  One light (folded state) and several (unfolded) through the
    scene fixture; the hand-over to the finishing pass switched off so that every bounce is a logic pass.  Bit for bit against the
    megakernel, with the same counts."""
    name, osc, sc, dev0 = pair
    monkeypatch.setenv("MCPT_FINISH_PATHS", "0")
    monkeypatch.setenv("MCPT_LOGIC_GRID", "2")
    dev = mcpt.Device(sc, 0)
    try:
        sa, sb = mcpt.Stats(), mcpt.Stats()
        a = dev.generateImg(16, seed=11, stats=sa)
        b = dev.generateImg(16, seed=11, flags=mcpt.RENDER_MEGAKERNEL)
        assert np.array_equal(_bits(a), _bits(b)), "%d channels differ from the megakernel" % int((_bits(a) != _bits(b)).sum())
        assert sa.launches >= 5, sa.launches
        c = dev0.generateImg(16, seed=11, stats=sb)           # (the fixture's device: default grid, finishing pass on)
        assert np.array_equal(_bits(a), _bits(c))
        assert (sa.rays_shadow + sa.shadow_skipped, sa.rays_bounce, sa.shade_calls) == (sb.rays_shadow + sb.shadow_skipped, sb.rays_bounce, sb.shade_calls)
    finally:
        dev.close()


def test_pool_engine_equals_voting_engine(pair, mcpt, monkeypatch):
    """The library picks the closest-hit engine by scene size (mcpt_scene_trace_engine): the pool engine, whose rays live in LDS
    (csrc/trace_pool.hpp: stateless wave steps on slots claimed with LDS atomics), for the primary rays, mcpt_trace_closest and every
    trace launch of a small scene, the voting engine for large ones; MCPT_TRACE_ENGINE=vote / pool forces either.  Same tests on the
    same triangles: face / t / p / pn of 300 k rays (camera, interior, adversarial, on-surface origins) and whole wavefront frames with
    the hand-over to k_wf_finish switched off must be equal bit for bit, with the same work (nodes stepped on, triangles visited)."""
    name, osc, sc, dev0 = pair
    base = make_rays(osc, 200000, seed=21)
    f0, t0, p0, n0 = dev0.ray_intersect(base)
    hit = f0 >= 0
    rng = np.random.default_rng(8)
    d = rng.normal(size=(int(hit.sum()), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.vstack([base, np.hstack([p0[hit] + 0.01 * d, d])[:60000], np.hstack([p0[hit], d])[:40000]])
    monkeypatch.setenv("MCPT_FINISH_PATHS", "0")
    monkeypatch.setenv("MCPT_TRACE_ENGINE", "vote")
    assert sc.trace_engine() == "vote"
    dv = mcpt.Device(sc, 0)
    monkeypatch.setenv("MCPT_TRACE_ENGINE", "pool")
    assert sc.trace_engine() == "pool"
    dp = mcpt.Device(sc, 0)
    try:
        sv, sp = mcpt.Stats(), mcpt.Stats()
        rv = dv.ray_intersect(rays, stats=sv)
        rp = dp.ray_intersect(rays, stats=sp)
        assert np.array_equal(rv[0], rp[0]), "%d faces differ" % int((rv[0] != rp[0]).sum())
        h = rv[0] >= 0
        for a, b in zip(rv[1:], rp[1:]):
            assert np.array_equal(_bits(a[h]), _bits(b[h]))
        for spp in (1, 8):                  # (a tiny launch per bounce; then some tens of thousands of rays per launch)
            a = dv.generateImg(spp, seed=5, stats=sv)
            b = dp.generateImg(spp, seed=5, stats=sp)
            assert np.array_equal(_bits(a), _bits(b)), "%d channels differ" % int((_bits(a) != _bits(b)).sum())
            assert sv.dom_rays == sp.dom_rays
            # (a ray the pool engine defers -- a walk deeper than its 8 LDS + 19 spill entries (27 in all; 36 under MCPT_SHORT_KERNEL=0),
            # a leader whose own box fails -- finishes in the one-lane walk, which counts elsewhere)
            assert abs(sv.dom_node_visits - sp.dom_node_visits) <= 0.01 * sv.dom_node_visits and abs(sv.dom_tri_tests - sp.dom_tri_tests) <= 0.01 * sv.dom_tri_tests
            assert sp.dom_rays > 0.9 * (sp.rays_shadow + sp.rays_bounce)
    finally:
        dv.close()
        dp.close()


def test_finishing_pass_in_pool_form_equals_the_lane_form(pair, mcpt, monkeypatch):
    """The finishing pass exists in two forms: one lane per path in lock-step (k_wf_finish: what scenes of the voting engine run) and the
    pool engine in path mode (k_wf_finish_pool, trace_pool.hpp with PP::kPaths: a workgroup owns the paths its LDS-resident rays belong
    to, SHADE is a step class, no ray goes through memory; what small scenes run from 1.5 M paths down).  Same vertex functions, same
    tests on the same triangles: whole frames must be equal bit for bit -- to each other and to the megakernel -- with the same counts,
    whether the pass takes every path straight after the first logic pass (small frames), takes over late (hand-over forced down to
    2 000 paths) or adopts more paths than its path slots hold at once (one light: 640 per CU; the 160x90 SPP-32 frame hands over
    ~400 k).  Covers one, two and five lights (cornell-box, glassroom / interior, veach-mis: 10, 6 and 3 path slots per lane)."""
    name, osc, sc, dev0 = pair
    monkeypatch.setenv("MCPT_FINISH_ENGINE", "lane")
    lane = mcpt.Device(sc, 0)
    monkeypatch.delenv("MCPT_FINISH_ENGINE")
    pool = mcpt.Device(sc, 0)
    monkeypatch.setenv("MCPT_FINISH_PATHS", "2000")
    late = mcpt.Device(sc, 0)
    try:
        for spp in (1, 8, 32):
            sl, sp, sa = mcpt.Stats(), mcpt.Stats(), mcpt.Stats()
            a = lane.generateImg(spp, seed=3, stats=sl)
            b = pool.generateImg(spp, seed=3, stats=sp)
            c = late.generateImg(spp, seed=3, stats=sa)
            m = pool.generateImg(spp, seed=3, flags=mcpt.RENDER_MEGAKERNEL)
            assert np.array_equal(_bits(a), _bits(b)), "%d channels differ between the two forms" % int((_bits(a) != _bits(b)).sum())
            assert np.array_equal(_bits(b), _bits(c)) and np.array_equal(_bits(b), _bits(m))
            for s in (sp, sa):
                assert (s.rays_shadow, s.rays_bounce, s.shade_calls, s.shadow_skipped, s.max_depth) == \
                       (sl.rays_shadow, sl.rays_bounce, sl.shade_calls, sl.shadow_skipped, sl.max_depth)
            assert sp.launches <= sa.launches          # (the late hand-over runs more wavefront iterations)
        assert a.sum() > 0
    finally:
        for d in (lane, pool, late):
            d.close()


def _gpu_emitter_map(mcpt, sc, dev):
    """[H, W] bool from the product's own frame: at SPP 1 a pixel whose primary hit is an emitter holds the light's radiance
    exactly -- rounded to float, the accumulator is a glm::vec3 (pathTracing.cpp:141-144, :301; k_primary_dirs -> primary hits
    -> k_wf_logic<true> -> k_fold_samples) -- and nothing else does."""
    img = dev.generateImg(1, seed=1)
    emit = np.zeros(img.shape[:2], dtype=bool)
    for l in range(sc.info.num_lights):
        emit |= (img == sc.light(l)[1].astype(np.float32).astype(np.float64)[None, None, :]).all(axis=2)
    return emit


def test_published_renders_pin_the_gpu_path(mcpt):
    """What the reference's published renders pin (tests/pins_common.py), applied to the HIP path at native resolution:
    (1) pixel-exact: every pixel whose primary hit is an emitter is (255,255,255) in every published render of the scene --
    4 922 pixels of cornell-box (and only 4 other pixels of cornell-box-SPP25.png are saturated), 45 266 of veach-mis;
    (2) Monte-Carlo precision: z-scores of all 16x16 blocks against two GPU renders at the published SPP are standard normal
    (blocks whose pixels saturate: the one-sided band of pins_common.py, where the reference's racy RNG meets imshow's clamp)."""
    import pins_common as P
    sc = mcpt.Scene(SCENES, "cornell-box")                  # native 1024x1024 camera
    dev = mcpt.Device(sc, 0)
    got = P.check_emitter_pixels(_gpu_emitter_map(mcpt, sc, dev), "cornell-box")
    assert all(v[0] == 4922 for v in got.values()) and got["cornell_spp25"][1] == 4, got
    qa, qb = (mcpt.imshow_rgb8(dev.generateImg(25, seed=s)) for s in (101, 102))
    assert P.block_stats("cornell_spp25", qa, qb)[0].shape == (4096, 3)
    print(P.assert_matches_published("cornell_spp25", qa, qb, "cornell-box SPP25, all blocks", mean_tol=0.1, rms=(0.9, 1.12)))
    dev.close()
    sc.close()
    sc = mcpt.Scene(SCENES, "veach-mis")                    # native 1200x900
    dev = mcpt.Device(sc, 0)
    got = P.check_emitter_pixels(_gpu_emitter_map(mcpt, sc, dev), "veach-mis")
    assert got["veach_spp10"][0] == 45266 and got["veach_spp100"][0] == 45266, got
    for name, spp in (("veach_spp10", 10), ("veach_spp100", 100)):
        qa, qb = (mcpt.imshow_rgb8(dev.generateImg(spp, seed=s)) for s in (201, 202))
        print(P.assert_matches_published(name, qa, qb, "veach-mis %s, all blocks" % name, mean_tol=0.2, rms=(0.85, 1.2), tail=0.01))
    dev.close()
    sc.close()


def test_pre_test_rejects_no_candidate(tmp_path):
    """The trace engine's conservative fp32 pre-test (trace_fast.hpp: tri_pre_reject) may only skip triangles that cannot become the
    closest hit.  The self-check build of the library (csrc/variants/libmcpt_chk.so, -DMCPT_PRE_CHECK, compiled by
    __graft_entry__.build()) puts every REJECTED triangle through the reference's exact test as well and counts those that pass it
    with a positive t_k not behind the leader: the count must be zero over whole frames of every test scene -- wavefront iterations
    forced (no hand-over to the one-lane finishing kernel), hierarchies built on the host and on the GPU -- and the pre-test must
    really have been at work (most visited triangles rejected)."""
    import selfcheck
    code = r'''
import os, sys
sys.path.insert(0, %r)
import montecarlopathtracing_amd as M
from montecarlopathtracing_amd import synthetic
tmp = sys.argv[1] + os.sep
synthetic.write_interior(tmp, "interior", width=320, height=180, detail=0.3)
scenes = [(%r, "cornell-box"), (%r, "veach-mis"), (%r, "glassroom"), (tmp, "interior")]
for base, name in scenes:
    sc = M.Scene(base, name, width=320, height=180)
    for build in (M.BUILD_HOST, M.BUILD_DEVICE_FAST):
        dev = M.Device(sc, 0, build=build)
        st = M.Stats()
        dev.generateImg(16, seed=7, stats=st)
        assert st.dom_rays > 0
        dev.close()
    sc.close()
sc = synthetic.make_scene(M, 300000, defer_build=True, width=320, height=180)
dev = M.Device(sc, 0)
dev.generateImg(8, seed=7, stats=M.Stats())
print("done")
''' % (ROOT, SCENES, SCENES, EXTRA)
    out = selfcheck.run(code, tmp_path, timeout=900)
    assert out.returncode == 0 and "done" in out.stdout, out.stderr[-3000:]
    assert "SELF-CHECK" not in out.stderr, selfcheck.pre_test_failures(out.stderr)[:6]
    shares = selfcheck.survivor_shares(out.stderr)
    assert len(shares) >= 9 and max(shares) < 60.0, shares


@pytest.mark.parametrize("name", ["cornell-box", "veach-mis", "synthetic"])
def test_device_build_equals_host_build(mcpt, oracle, name, tmp_path):
    """Morton keys, stable radix sort, leaf records and the level-by-level union on the GPU (build_kernels.hip) against the
    host build (bvh_build.cpp): every node box, the leaf order, and the rendered image, bit for bit -- and, for the scenes that exist as
    files, the device's arrays against the ORACLE's directly (BVH.cpp:44-85, morton code.cpp, D2's stable order)."""
    from montecarlopathtracing_amd import synthetic
    if name == "synthetic":
        g = synthetic.generate(150000, width=96, height=54)     # above 2^17 triangles: the host's SAH build runs its worker threads
        args = (g["v"], g["vn"], g["material"], g["material_rec"], g["light_material"], g["light_radiance"], g["eye"], g["look_at"],
                g["up"], g["fovy"], g["width"], g["height"])
        sc = mcpt.Scene.from_arrays(*args)
        deferred = mcpt.Scene.from_arrays(*args, defer_build=True)
    else:
        sc = mcpt.Scene(SCENES, name, width=96, height=54)
        deferred = None
    host = mcpt.Device(sc, 0, build=mcpt.BUILD_HOST)
    dev = mcpt.Device(sc, 0, build=mcpt.BUILD_DEVICE)
    hb, hl = sc.bvh_nodes()[0], sc.leaf_order()
    db, dleaf = dev.bvh_nodes()
    assert np.array_equal(dev.leaf_order(), hl)
    assert np.array_equal(_bits(db), _bits(hb))
    assert np.array_equal(_bits(host.bvh_nodes()[0]), _bits(hb))
    if name != "synthetic":
        osc = oracle.OracleScene(SCENES + name, texture_dir=SCENES, width=96, height=54)
        obox, olvl, oleaf = osc.bvh_nodes()
        assert np.array_equal(dev.leaf_order(), osc.leaf_order())
        assert np.array_equal(_bits(db), _bits(obox)), "%d of %d device-built node planes differ from the oracle's" % (int((_bits(db) != _bits(obox)).sum()), db.size)
        assert np.array_equal(dleaf[olvl == olvl.max()], oleaf[olvl == olvl.max()])
        osc.close()
    a = host.generateImg(4, seed=5)
    b = dev.generateImg(4, seed=5)
    assert np.array_equal(_bits(a), _bits(b)) and a.sum() > 0
    if deferred is not None:
        d2 = mcpt.Device(deferred, 0)              # no host build at all
        assert np.array_equal(_bits(d2.generateImg(4, seed=5)), _bits(a))
        d2.close()
    host.close()
    dev.close()


def test_morton_bounds_scene_same_answers(mcpt, oracle):
    """MCPT_LOAD_MORTON_BOUNDS changes the leaf order (hence the reference-shaped tree and the tie-break index k) and nothing
    else: both walks still agree with each other, the device build still equals the host build, and against the parity-mode
    scene every ray finds the same distance; only rays with two equidistant candidates may name the other triangle."""
    plain = mcpt.Scene(SCENES, "veach-mis", width=96, height=54)
    sc = mcpt.Scene(SCENES, "veach-mis", width=96, height=54, load_flags=mcpt.LOAD_MORTON_BOUNDS)
    osc = oracle.OracleScene(SCENES + "veach-mis", texture_dir=SCENES, width=96, height=54)
    rays = make_rays(osc, 60000, seed=11)
    osc.close()
    d0 = mcpt.Device(plain, 0)
    host = mcpt.Device(sc, 0, build=mcpt.BUILD_HOST)
    dev = mcpt.Device(sc, 0, build=mcpt.BUILD_DEVICE)
    assert np.array_equal(dev.leaf_order(), sc.leaf_order())
    assert np.array_equal(_bits(dev.bvh_nodes()[0]), _bits(sc.bvh_nodes()[0]))
    f0, t0, p0, _ = d0.ray_intersect(rays)
    f1, t1, p1, _ = host.ray_intersect(rays)
    host.set_trace_mode(mcpt.TRACE_REFERENCE)
    f2, t2, p2, _ = host.ray_intersect(rays)
    assert np.array_equal(f1, f2) and np.array_equal(_bits(t1[f1 >= 0]), _bits(t2[f2 >= 0]))
    assert np.array_equal(f0 >= 0, f1 >= 0)
    h = f0 >= 0
    assert np.array_equal(_bits(t0[h]), _bits(t1[h]))
    assert (f0 != f1).mean() < 2e-3
    a = host.generateImg(4, seed=5)
    b = dev.generateImg(4, seed=5)
    assert np.array_equal(_bits(a), _bits(b)) and a.sum() > 0
    for d in (d0, host, dev):
        d.close()


def test_render_scene_outputs_and_resume(mcpt, tmp_path, monkeypatch):
    """render_scene with the output options: compressed PNG = the same pixels as the reference-format PNG, the PFM = the
    linear frame, and a frame resumed from a checkpoint that holds 3 of 5 partitions = the uninterrupted frame, bit for bit."""
    from PIL import Image
    out = str(tmp_path) + os.sep
    kw = dict(seed=9, width=80, height=60, quiet=True)
    mcpt.render_scene(SCENES, "cornell-box", 6, output_prefix=out + "plain", **kw)
    mcpt.render_scene(SCENES, "cornell-box", 6, output_prefix=out + "z", output_flags=mcpt.OUT_PNG_DEFLATE | mcpt.OUT_PFM, **kw)
    a = np.array(Image.open(out + "plain-SPP6.png").convert("RGB"))
    b = np.array(Image.open(out + "z-SPP6.png").convert("RGB"))
    assert np.array_equal(a, b) and os.path.getsize(out + "z-SPP6.png") < os.path.getsize(out + "plain-SPP6.png")
    sc = mcpt.Scene(SCENES, "cornell-box", width=80, height=60)
    dev = mcpt.Device(sc, 0)
    full = dev.generateImg(6, seed=9)
    raw = open(out + "z-SPP6.pfm", "rb").read()
    head = b"PF\n80 60\n-1.0\n"
    assert raw.startswith(head)
    assert np.array_equal(np.frombuffer(raw[len(head):], dtype="<f4").reshape(60, 80, 3)[::-1], full.astype(np.float32))
    assert np.array_equal(mcpt.imshow_rgb8(full), a)
    # an interrupted run: partitions 0, 2, 3 of 5 are in the checkpoint
    part = np.zeros_like(full)
    for r in (0, 2, 3):
        dev.generateImg(6, seed=9, rank=r, world=5, img=part)
    ck = out + "frame.ckp"
    mcpt.checkpoint_save(ck, sc, part, 6, 9, np.array([1, 0, 1, 1, 0], dtype=np.uint8))
    st = mcpt.Stats()
    # (no finishing pass from here on: every bounce goes through k_wf_trace, whose share dom_* counts -- a frame this small is otherwise
    # handed to the finishing pass after its first vertex; the frame is the same either way)
    monkeypatch.setenv("MCPT_FINISH_PATHS", "0")
    mcpt.render_scene(SCENES, "cornell-box", 6, output_prefix=out + "resumed", checkpoint=ck, checkpoint_parts=5, stats=st, **kw)
    assert open(out + "resumed-SPP6.png", "rb").read() == open(out + "plain-SPP6.png", "rb").read()
    img, done = mcpt.checkpoint_load(ck, sc, 6, 9, 5)
    assert done.all() and np.array_equal(_bits(img), _bits(full))
    assert 0 < st.samples < 80 * 60 * 6              # only the two missing partitions were rendered
    assert st.dom_rays > 0                           # ... and their statistics keep the trace kernel's share
    # a progressive frame (a noise target no pass reaches: every sample) reports that share as well
    sp = mcpt.Stats()
    mcpt.render_scene(SCENES, "cornell-box", 6, output_prefix=out + "prog", noise_target=1e-12, stats=sp, **kw)
    assert open(out + "prog-SPP6.png", "rb").read() == open(out + "plain-SPP6.png", "rb").read()
    assert sp.samples == 80 * 60 * 6 and sp.dom_rays > 0
    # a checkpoint of another frame (different seed) is ignored, not trusted
    mcpt.render_scene(SCENES, "cornell-box", 6, output_prefix=out + "other", checkpoint=ck, checkpoint_parts=5,
                      **dict(kw, seed=10))
    assert open(out + "other-SPP6.png", "rb").read() != open(out + "plain-SPP6.png", "rb").read()
    dev.close()
    sc.close()


@pytest.mark.parametrize("mode", ["fast", "sah"])
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis", "synthetic"])
def test_fast_hierarchy_built_on_device(mcpt, oracle, name, mode):
    """MCPT_BUILD_DEVICE_FAST: the culling hierarchy is a 4-wide tree over the Morton order, built by build_kernels.hip instead
    of the host's SAH builder; MCPT_BUILD_DEVICE_SAH: clusters grown on the GPU by locally-ordered clustering and collapsed there,
    the host's builder over the clusters.  A hierarchy only culls, so nothing may change: the fast walk on it agrees with the
    reference-shaped walk ray for ray, bit for bit, and the image equals the one rendered on the host-built hierarchy.  The clustered
    tree must also be about as good as the host's SAH tree: at most 1.3x its node steps + triangle visits on these rays."""
    from montecarlopathtracing_amd import synthetic
    if name == "synthetic":
        g = synthetic.generate(60000, width=96, height=54)
        sc = mcpt.Scene.from_arrays(g["v"], g["vn"], g["material"], g["material_rec"], g["light_material"], g["light_radiance"], g["eye"],
                                    g["look_at"], g["up"], g["fovy"], g["width"], g["height"], defer_build=True)
        rng = np.random.default_rng(8)
        o = np.array(g["eye"])[None, :] + rng.normal(size=(50000, 3)) * 0.3
        d = rng.normal(size=(50000, 3))
        d[::50, 0] = 0.0                                            # some rays for the reference-shaped side list
        rays = np.hstack([o, d / np.linalg.norm(d, axis=1, keepdims=True)])
        host = mcpt.Device(sc, 0)                                   # Morton order on the GPU, SAH hierarchy on the host
    else:
        sc = mcpt.Scene(SCENES, name, width=96, height=54)
        osc = oracle.OracleScene(SCENES + name, texture_dir=SCENES, width=96, height=54)
        rays = make_rays(osc, 50000, seed=31)
        osc.close()
        host = mcpt.Device(sc, 0, build=mcpt.BUILD_HOST)
    dev = mcpt.Device(sc, 0, build=mcpt.BUILD_DEVICE_FAST if mode == "fast" else mcpt.BUILD_DEVICE_SAH)
    st_h, st_d = mcpt.Stats(), mcpt.Stats()
    f0, t0, p0, n0 = host.ray_intersect(rays, stats=st_h)
    f1, t1, p1, n1 = dev.ray_intersect(rays, stats=st_d)
    dev.set_trace_mode(mcpt.TRACE_REFERENCE)
    f2, t2, p2, n2 = dev.ray_intersect(rays)
    assert (f1 >= 0).sum() > 1000
    for f, t, p, n in ((f0, t0, p0, n0), (f2, t2, p2, n2)):
        assert np.array_equal(f, f1)
        h = f1 >= 0
        assert np.array_equal(_bits(t[h]), _bits(t1[h])) and np.array_equal(_bits(p[h]), _bits(p1[h])) and np.array_equal(_bits(n[h]), _bits(n1[h]))
    # it really was the fast walk on the device-built tree: far fewer steps than the exhaustive reference walk
    assert st_d.node_visits < 0.2 * rays.shape[0] * sc.info.num_faces / 8
    if mode == "sah":
        assert st_d.node_visits + st_d.tri_tests <= 1.3 * (st_h.node_visits + st_h.tri_tests), (st_d.node_visits, st_h.node_visits, st_d.tri_tests, st_h.tri_tests)
        # the clustering is deterministic (ordered compaction, no atomics in the layout): a second build is the same tree
        dev2 = mcpt.Device(sc, 0, build=mcpt.BUILD_DEVICE_SAH)
        st_2 = mcpt.Stats()
        f3, t3, p3, n3 = dev2.ray_intersect(rays, stats=st_2)
        dev2.close()
        assert np.array_equal(f3, f1) and (st_2.node_visits, st_2.tri_tests) == (st_d.node_visits, st_d.tri_tests)
    dev.set_trace_mode(mcpt.TRACE_FAST)
    a = host.generateImg(4, seed=5)
    b = dev.generateImg(4, seed=5)
    assert np.array_equal(_bits(a), _bits(b)) and a.sum() > 0
    host.close()
    dev.close()


def test_multi_device_frame_equals_single_device(mcpt):
    """mcpt_multi_* (the GPUs of a node behind one C-ABI call: a host thread per GPU, tiles dealt like rank/world, compact pixel
    buffers gathered into the first GPU's HBM): the frame must equal mcpt_render's bit for bit whatever the number of ranks.
    On a one-GPU box the ranks share GPU 0 -- three resident copies of the scene, three concurrent renders, two peer copies that
    degenerate to device-to-device copies -- which exercises everything but the xGMI hop; with every visible GPU (one here) it
    is the degenerate world of 1.  The RCCL form is created and torn down (ncclCommInitAll over the visible GPUs)."""
    sc = mcpt.Scene(SCENES, "cornell-box", width=200, height=120)
    dev = mcpt.Device(sc, 0)
    st1 = mcpt.Stats()
    want = dev.generateImg(8, seed=5, stats=st1)
    dev.close()
    for devices in (None, [0, 0, 0]):
        md = mcpt.MultiDevice(sc, devices)
        assert md.num_devices == (mcpt.device_count() if devices is None else 3)
        st = mcpt.Stats()
        got = md.generateImg(8, seed=5, stats=st)
        again = md.generateImg(8, seed=5)
        md.close()
        assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(again), _bits(want))
        assert st.samples == st1.samples and st.rays_primary == st1.rays_primary
        assert (st.rays_shadow + st.shadow_skipped, st.rays_bounce, st.shade_calls) == (st1.rays_shadow + st1.shadow_skipped, st1.rays_bounce, st1.shade_calls)
    md = mcpt.MultiDevice(sc, list(range(mcpt.device_count())), gather=mcpt.GATHER_RCCL)
    assert np.array_equal(_bits(md.generateImg(8, seed=5)), _bits(want))
    render_ms, gather_ms, comm_ranks = md.last_timing()
    assert comm_ranks == mcpt.device_count() and len(render_ms) == md.num_devices and render_ms.min() > 0 and gather_ms >= 0
    with pytest.raises(mcpt.McptError):
        sc.set_resolution(100, 60)                                     # a device created from this scene is alive
    md.close()
    with pytest.raises(mcpt.McptError):
        mcpt.MultiDevice(sc, [0, 0], gather=mcpt.GATHER_RCCL)          # RCCL wants distinct GPUs
    sc.set_resolution(100, 60)                                         # every device is gone again: the camera may change
    assert (sc.info.width, sc.info.height) == (100, 60)
    sc.close()


def test_pipelined_frames_equal_sequential_frames(mcpt):
    """A sequence of frames with two in flight (RENDER_PIPELINE | RENDER_KEEP_STATS: the device's two frame slots, two streams, two
    frame buffers; no frame waits for its statistics) gives, frame for frame, the bits of the same frames rendered one at a time,
    and the statistics collected afterwards are the sums of theirs.  (Streams and buffers through the HIP runtime directly: what
    montecarlopathtracing_amd.dist.DistributedRenderer(pipeline=True) does with torch's.)"""
    import hip_rt
    sc = mcpt.Scene(SCENES, "cornell-box", width=640, height=360)
    dev = mcpt.Device(sc, 0)
    seeds = (1, 2, 3, 4, 5)
    want, sums = [], {"samples": 0, "rays_shadow": 0, "rays_bounce": 0, "shade_calls": 0, "launches": 0, "rays_primary": 0, "dom_rays": 0}
    for sd in seeds:
        st = mcpt.Stats()
        want.append(dev.generateImg(24, seed=sd, stats=st))
        for k in sums:
            sums[k] += getattr(st, k)
    nbytes = 640 * 360 * 3 * 8
    streams = [hip_rt.Stream(), hip_rt.Stream()]
    frames = [hip_rt.DeviceBuffer(nbytes), hip_rt.DeviceBuffer(nbytes)]
    got = [np.zeros((360, 640, 3)) for _ in seeds]
    for i, sd in enumerate(seeds):
        t = i & 1
        dev.render_device(frames[t].ptr.value, 24, sd, flags=mcpt.RENDER_PIPELINE | mcpt.RENDER_KEEP_STATS, stream=streams[t].h.value)
        frames[t].to_host_async(got[i], streams[t].h)            # before the frame after next overwrites the buffer (same stream)
    for st_ in streams:
        st_.synchronize()
    for a, b in zip(want, got):
        assert np.array_equal(_bits(a), _bits(b))
    st = dev.collect_stats()
    for k in sums:
        assert getattr(st, k) == sums[k], (k, getattr(st, k), sums[k])
    assert st.ms_trace > 0 and st.ms_total >= st.ms_trace
    again = dev.collect_stats()
    assert again.samples == 0 and again.rays_shadow == 0 and again.ms_total == 0        # collected means started over
    assert np.array_equal(_bits(dev.generateImg(24, seed=3)), _bits(want[2]))            # and the plain entry still works afterwards
    for f in frames:
        f.free()
    for st_ in streams:
        st_.destroy()
    dev.close(); sc.close()


def test_cpp_drop_in_render_scene(mcpt, tmp_path):
    """The C++ surface a user of the reference switches to: a main() that includes include/mtpc_compat.hpp and calls
    render_scene(path, filename, N) exactly like MTPC/MTPC.cpp:78, compiled here with g++ against libmcpt.so, and the mtpc
    command-line stand-in.  Both must write the PNG the ctypes path writes, byte for byte -- also on "all GPUs"."""
    import subprocess
    csrc = os.path.join(ROOT, "montecarlopathtracing_amd", "csrc")
    src = tmp_path / "main.cpp"
    src.write_text('''#include "mtpc_compat.hpp"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv)
{
    mtpc::options().seed = 9; mtpc::options().width = 96; mtpc::options().height = 64; mtpc::options().quiet = 1;
    mtpc::options().output_prefix = argv[3];
    if (argc > 4) mtpc::options().num_devices = std::atoi(argv[4]);
    if (!render_scene(argv[1], argv[2], 6)) { std::fprintf(stderr, "%s\\n", mcpt_last_error()); return 1; }
    return 0;
}
''')
    exe = str(tmp_path / "dropin")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe, "-L" + csrc, "-lmcpt",
                           "-Wl,-rpath," + csrc])
    out = str(tmp_path) + os.sep
    mcpt.render_scene(SCENES, "cornell-box", 6, seed=9, width=96, height=64, output_prefix=out + "py")
    want = open(out + "py-SPP6.png", "rb").read()
    subprocess.check_call([exe, SCENES, "cornell-box", out + "cpp"], cwd=str(tmp_path))
    assert open(out + "cpp-SPP6.png", "rb").read() == want
    subprocess.check_call([exe, SCENES, "cornell-box", out + "all", "-1"], cwd=str(tmp_path))
    assert open(out + "all-SPP6.png", "rb").read() == want
    mcpt.render_scene(SCENES, "cornell-box", 6, seed=9, width=96, height=64, output_prefix=out + "three", devices=[0, 0, 0])
    assert open(out + "three-SPP6.png", "rb").read() == want
    # the command-line stand-in for the reference's main(): it writes ../result/<filename>-SPP<N>.png relative to the cwd
    run = tmp_path / "run"
    run.mkdir()
    (tmp_path / "result").mkdir()
    subprocess.check_call([os.path.join(csrc, "mtpc"), SCENES, "cornell-box", "6", "9", "96", "64"], cwd=str(run), stdout=subprocess.DEVNULL)
    assert open(str(tmp_path / "result" / "cornell-box-SPP6.png"), "rb").read() == want


EDGE_MTL = "newmtl grey\nKd 0.6 0.5 0.4\nKs 0 0 0\nNs 1\nNi 1\nnewmtl lamp\nKd 0 0 0\nKs 0 0 0\nNs 1\nNi 1\n"
EDGE_OBJ_HEAD = ("v -2 0 -2\nv 2 0 -2\nv 2 0 2\nv -2 0 2\nv -0.5 1.9 -0.5\nv 0.5 1.9 -0.5\nv 0.5 1.9 0.5\nv -0.5 1.9 0.5\n"
                 "vn 0 1 0\nvn 0 -1 0\nvt 0 0\n")
EDGE_CASES = {
    # a single triangle and nothing else: one leaf, a root that is a leaf, every path ends after one vertex, no light at all
    "one-triangle-no-light": ("usemtl grey\nf 1/1/1 2/1/1 3/1/1\n", ""),
    # floor + lamp, plus a zero-area triangle (NaN normal: the triangle test can never pass) and a repeated face (exact tie in t)
    "degenerate-and-duplicate": ("usemtl grey\nf 1/1/1 2/1/1 3/1/1\nf 1/1/1 3/1/1 4/1/1\nf 1/1/1 1/1/1 2/1/1\nf 1/1/1 2/1/1 3/1/1\n"
                                 "usemtl lamp\nf 5/2/1 6/2/1 7/2/1\nf 5/2/1 7/2/1 8/2/1\n", "mtlname lamp 12 12 12\n"),
    # the camera names a light twice: light_map keeps the last entry, lights[] both (two shadow rays per vertex, nl = 2)
    "light-listed-twice": ("usemtl grey\nf 1/1/1 2/1/1 3/1/1\nf 1/1/1 3/1/1 4/1/1\nusemtl lamp\nf 5/2/1 6/2/1 7/2/1\nf 5/2/1 7/2/1 8/2/1\n",
                           "mtlname lamp 5 5 5\nmtlname lamp 7 7 7\n"),
}


@pytest.mark.parametrize("case", sorted(EDGE_CASES))
@pytest.mark.parametrize("size", [(1, 1), (33, 17)])
def test_edge_scenes(mcpt, oracle, tmp_path, case, size):
    """Smallest and oddest inputs the reader accepts (see EDGE_CASES), at a 1x1 frame and a ragged one (neither a multiple of
    the 32x8 tile nor of a wave): closest hit bit-exact in both walks, image against the oracle, every pipeline the same bits."""
    faces, lights = EDGE_CASES[case]
    w, h = size
    d = str(tmp_path) + os.sep
    open(d + "e.obj", "w").write(EDGE_OBJ_HEAD + faces)
    open(d + "e.mtl", "w").write(EDGE_MTL)
    open(d + "e.camera", "w").write("eye 0.3 1.0 3.5\nlookat 0 0.8 0\nup 0 1 0\nfovy 50\nwidth %d\nheight %d\n%s" % (w, h, lights))
    osc = oracle.OracleScene(d + "e", texture_dir=d)
    sc = mcpt.Scene(d, "e")
    dev = mcpt.Device(sc, 0)
    rays = make_rays(osc, 4000, seed=3)
    of, ot, op, opn = osc.trace_closest(rays)
    for mode in (mcpt.TRACE_FAST, mcpt.TRACE_REFERENCE):
        dev.set_trace_mode(mode)
        gf, gt, gp, gpn = dev.ray_intersect(rays)
        assert np.array_equal(of, gf)
        hh = of >= 0
        assert np.array_equal(_bits(ot[hh]), _bits(gt[hh])) and np.array_equal(_bits(op[hh]), _bits(gp[hh]))
    dev.set_trace_mode(mcpt.TRACE_FAST)
    ref = osc.render(5, seed=2)
    a = dev.generateImg(5, seed=2)
    b = dev.generateImg(5, seed=2, flags=mcpt.RENDER_MEGAKERNEL)
    parts = np.zeros_like(a)
    for r in range(3):
        dev.generateImg(5, seed=2, rank=r, world=3, img=parts)
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(parts))
    assert np.allclose(a, ref, rtol=1e-6, atol=1e-12)
    if not lights:
        assert not a.any()
    elif w > 1:
        assert a.sum() > 0
    dev.close()
    sc.close()
    osc.close()


def test_bench_line_keeps_its_contract(tmp_path):
    """bench.py prints one JSON line with the fields the driver and the judge read (a small frame here; the default is the
    1280x720 SPP-256 frame).  The CPU leg is exercised too, on its bounded sample."""
    import json
    import subprocess
    import sys
    # large enough for wavefront iterations to run before the finishing kernel takes over (the roofline is k_wf_trace's)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--width", "640", "--height", "360",
                          "--spp", "16", "--cpu-seconds", "2"], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["unit"] == "Mrays/s" and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["vs_baseline"] is None and d["scaling"] in ("strong", "weak")
    assert "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # the plain form drives the product's own multi-GPU entry (mcpt_multi_*, RCCL communicator of one here), one frame at a time,
    # in a process that has not loaded torch's copy of the HIP runtime
    assert d["config"]["launcher"].startswith("capi") and d["config"]["frames_in_flight"] == 1 and d["latency_ms_per_frame"] == d["ms_per_step"]
    assert d["rccl_ranks"] == 1 and d["gather"] == "rccl" and len(d["per_rank_render_ms"]) == 1 and "torch" not in d["hip_runtime"]
    assert len(d["build_id"]) == 16
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert (r["bytes_per_unit"]["node_visit"], r["bytes_per_unit"]["triangle_test"], r["bytes_per_unit"]["ray"]) == (32, 48, 64)
    assert r["record_bytes_rate_GBs"] > r["achieved"] and r["traffic"] is None and "not a profiled workload" in r["traffic_source"]
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and r["achieved"] > 0 and "traffic" in r
    # the dominant kernel is named after the engine the library picked for the scene (cornell-box: small, hence the pool engine)
    assert (r["engine"], r["kernel"]) in (("pool", "k_wf_trace_pool"), ("vote", "k_wf_trace"))
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0 and c["unit"] == "Mrays/s" and c["sample"]
    # ... and the reference-style figure beside it: the reference's own parallel structure, min(SPP, 8) threads per pixel
    rs = c["reference_style"]
    assert rs["threads"] == 8 and rs["value"] > 0 and rs["unit"] == "Mrays/s" and "pathTracing.cpp:300-320" in rs["sample"]
    assert rs["value"] < c["value"]             # <= 8 threads and a fork/join per pixel against every core of the socket


def test_one_process_per_gpu_without_torch(mcpt, tmp_path):
    """The launcher form of N GPUs: `python -m torch.distributed.run ... bench.py --gpus N` starts one process per GPU, and the ranks
    gather their frames over an RCCL communicator they build themselves (mcpt_comm_*, montecarlopathtracing_amd/procs.py) -- torch
    is not imported by them, so they pass the runtime gate like every other caller.  On the one-GPU test box: a launch of one (the
    communicator of one rank, its all-reduce and barrier, the gather that has nothing to move) through bench.py under the launcher's
    environment, and through the class directly; the frame equals the plain one-GPU frame."""
    import json
    import subprocess
    import sys
    from montecarlopathtracing_amd.procs import ProcessGroup
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29512")
    png = str(tmp_path / "procs.png")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--width", "320", "--height", "180",
                          "--spp", "8", "--no-cpu-baseline", "--save-png", png], capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.strip()][-1])
    assert d["config"]["launcher"].startswith("procs") and d["rccl_ranks"] == 1 and "torch" not in d["hip_runtime"] and d["n_gpus"] == 1
    assert d["value"] > 0 and d["config"]["frames_in_flight"] == 1
    plain = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0", "--width", "320", "--height", "180", "--spp", "8",
                            "--no-cpu-baseline", "--save-png", str(tmp_path / "plain.png")], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert plain.returncode == 0, plain.stderr[-2000:]
    assert open(png, "rb").read() == open(str(tmp_path / "plain.png"), "rb").read()
    # the class itself, in this process
    pg = ProcessGroup(0, rank=0, world=1)
    try:
        assert pg.size() == 1
        v = pg.allreduce([1.5, -2.0, 7.0], op="sum")
        assert list(v) == [1.5, -2.0, 7.0] and list(pg.allreduce([3.0], op="max")) == [3.0]
        pg.barrier()
        sc = mcpt.Scene(SCENES, "cornell-box", width=64, height=36)
        dev = mcpt.Device(sc, 0)
        import hip_rt
        buf = hip_rt.DeviceBuffer(64 * 36 * 24)
        st = hip_rt.Stream()
        dev.render_device(buf.ptr.value, 2, 5, 0, 1, 0, 0, flags=0, stats=None, stream=st.h.value)
        pg.gather_frame(sc, buf.ptr.value, stream=st.h.value)
        got = np.zeros((36, 64, 3))
        buf.to_host_async(got, st.h)
        st.synchronize()
        assert np.array_equal(_bits(got), _bits(dev.generateImg(2, seed=5)))
        buf.free(); st.destroy(); dev.close(); sc.close()
    finally:
        pg.close()


def test_bench_dumps_the_frame_of_its_last_step(mcpt, tmp_path):
    """bench.py --dump-outputs DIR: the frame the timed path returned in its last step, as DIR/frame.npy in float64 -- the same bits
    whatever the number of steps, and the frame a one-GPU render of the same scene files returns."""
    import importlib.util
    import json
    import shutil
    import subprocess
    import sys
    frames = []
    for steps, warmup in ((2, 1), (1, 0)):
        d = tmp_path / ("dump%d" % steps)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", str(warmup), "--width", "320",
                              "--height", "180", "--spp", "8", "--no-cpu-baseline", "--dump-outputs", str(d)],
                             capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert out.returncode == 0, out.stderr[-2000:]
        line = json.loads([ln for ln in out.stdout.splitlines() if ln.strip()][-1])
        assert line["steps"] == steps and line["dumped_outputs"]["files"] == ["frame.npy"]
        f = np.load(str(d / "frame.npy"))
        assert f.dtype == np.float64 and f.shape == (180, 320, 3) and f.max() > 0
        frames.append(f)
    assert np.array_equal(_bits(frames[0]), _bits(frames[1]))
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    scene_dir = bench.write_scene_dir("cornell-box", 320, 180)
    sc = mcpt.Scene(scene_dir, "cornell-box")
    dev = mcpt.Device(sc, 0)
    try:
        assert np.array_equal(_bits(frames[0]), _bits(dev.generateImg(8, seed=0)))
    finally:
        dev.close()
        sc.close()
        shutil.rmtree(scene_dir, ignore_errors=True)


def test_bench_refuses_more_gpus_than_visible_and_quotes_only_profiles_of_the_loaded_build(mcpt, tmp_path):
    """`python bench.py --gpus N` without a launcher needs N visible GPUs (exit code 2, nothing on stdout).  Counters quoted from
    profiles/ must come from the build that is loaded: committed_profile() matches the file's build_id against mcpt_build_id()."""
    import importlib.util
    import json
    import subprocess
    import sys
    n = mcpt.device_count() + 1
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "1", "--warmup", "0"], capture_output=True, text=True,
                         timeout=300, cwd=str(tmp_path))
    assert out.returncode == 2 and not out.stdout.strip() and "visible" in out.stderr
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    prof = tmp_path / "profiles"
    prof.mkdir()
    (prof / "r09_final_hbm_traffic.json").write_text(json.dumps({"bytes_per_launch": 1.0, "build_id": "0123456789abcdef"}))
    old_root = bench.ROOT
    bench.ROOT = str(tmp_path)
    try:
        f, j, why = bench.committed_profile("r*_final_hbm_traffic.json", mcpt.build_id())
        assert f is None and j is None and "another build" in why
        f, j, why = bench.committed_profile("r*_final_hbm_traffic.json", "0123456789abcdef")
        assert j["bytes_per_launch"] == 1.0 and why is None
    finally:
        bench.ROOT = old_root


def _oracle_pixels_of_full_frame(oracle, prefix, texture_dir, spp, seed, full, name):
    """A BASELINE frame at its own size and SPP against the oracle where the oracle can follow in seconds: a 64x36-pixel crop
    around the frame's centre and 2 000 pixels drawn at random (400 on the interior), every one at the full SPP (a pixel is the float fold of its spp
    samples in order on both sides, so a pixel either agrees to the accumulator's rounding or holds a flipped sample)."""
    osc = oracle.OracleScene(prefix, texture_dir=texture_dir)
    H, W = osc.height, osc.width
    assert full.shape == (H, W, 3)
    ref = np.zeros((H, W, 3))
    r0, c0 = H // 2 - 18, W // 2 - 32
    osc.render(spp, seed=seed, rows=(r0, r0 + 36), cols=(c0, c0 + 64), img=ref)
    mask = np.zeros((H, W), dtype=bool)
    mask[r0:r0 + 36, c0:c0 + 64] = True
    # the scattered pixels: a 1x1 crop is one block of the oracle's OpenMP loop, so the pixels are spread over host threads here (ctypes
    # drops the GIL, the scene is read-only, every call writes its own pixel of `ref`).  The exhaustive walk of the reference costs
    # ~170 box tests per ray on cornell-box and thousands on the 204 k-triangle interior: fewer pixels there.
    import concurrent.futures
    rng = np.random.default_rng(2024)
    picks = [divmod(int(p), W) for p in rng.choice(H * W, size=2000 if name != "interior" else 400, replace=False)]
    picks = [(r, c) for r, c in picks if not mask[r, c]]
    workers = max(1, min(32, (os.cpu_count() or 8) - 1))

    def some(chunk):
        for r, c in chunk:
            osc.render(spp, seed=seed, rows=(r, r + 1), cols=(c, c + 1), nthreads=1, img=ref)
    with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as pool:
        list(pool.map(some, [picks[i::workers] for i in range(workers)]))
    for r, c in picks:
        mask[r, c] = True
    osc.close()
    got, want = full[mask], ref[mask]
    rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-6)
    bad = int((rel > 1e-6).sum())
    budget = max(3, int(got.size * spp * FLIP_BUDGET[name]))       # channels x samples per pixel x flips per sample
    assert bad <= budget, "%s: %d of %d pixel channels differ from the oracle (max rel %.3e)" % (name, bad, got.size, rel.max())
    assert want.mean() > 0 and abs(got.mean() - want.mean()) <= (2e-3 + 25 * FLIP_BUDGET[name]) * want.mean()
    return int(mask.sum()), bad


def test_config1_workload_on_the_gpu(mcpt, oracle):
    """BASELINE config 1's workload -- cornell-box 400x400 SPP 2, the reference's own CPU-runnable case -- whole image, HIP path
    against the oracle."""
    import bench
    d = bench.write_scene_dir("cornell-box", 400, 400)
    sc = mcpt.Scene(d, "cornell-box")
    dev = mcpt.Device(sc, 0)
    st = mcpt.Stats()
    img = dev.generateImg(2, seed=0, stats=st)
    osc = oracle.OracleScene(d + "cornell-box", texture_dir=d)
    ost = oracle.Stats()
    ref = osc.render(2, seed=0, stats=ost)
    rel = np.abs(img - ref) / np.maximum(np.abs(ref), 1e-6)
    bad = int((rel > 1e-6).sum())
    assert bad <= max(3, int(img.size * 2 * FLIP_BUDGET["cornell-box"])), "%d pixel channels differ (max rel %.3e)" % (bad, rel.max())
    assert st.samples == ost.samples == 400 * 400 * 2
    assert st.rays_shadow + st.shadow_skipped == ost.rays_shadow and st.rays_bounce == ost.rays_bounce and st.shade_calls == ost.shade_calls
    assert int((mcpt.imshow_rgb8(img) != oracle.quantize(ref)).sum()) <= 8
    osc.close(); dev.close(); sc.close()


@pytest.mark.parametrize("name,spp", [("cornell-box", 256), ("veach-mis", 100), ("interior", 256)])
def test_full_size_frame_properties(mcpt, oracle, monkeypatch, name, spp, tmp_path):
    """BASELINE's own frames (configs 2, 3 and 4: cornell-box 1280x720 SPP 256, veach-mis SPP 100, and the generated textured
    interior of 204 k triangles that stands in for the unshipped bedroom scene, SPP 256), which the oracle cannot finish in
    seconds, through properties that do
    not depend on size: rendering it again gives the same bits; the 8-rank tile partition assembles to the same bits; a frame
    cut into chunks by a small workspace gives the same bits; its mean agrees with an independent seed's within Monte-Carlo
    error; every ray the statistics count was traced (samples = pixels x SPP, rays = shadow + bounce).  And directly against the
    oracle where it can follow: a 64x36 crop and 2 000 random pixels at the full SPP (_oracle_pixels_of_full_frame)."""
    import bench
    if name == "interior":
        from montecarlopathtracing_amd import synthetic
        d = str(tmp_path) + os.sep
        synthetic.write_interior(d, "interior", width=1280, height=720)
    else:
        d = bench.write_scene_dir(name, 1280, 720)
    monkeypatch.delenv("MCPT_WORKSPACE_GB", raising=False)
    sc = mcpt.Scene(d, name)
    if name == "interior":
        assert sc.info.num_faces > 200000
    dev = mcpt.Device(sc, 0)
    st = mcpt.Stats()
    full = dev.generateImg(spp, seed=0, stats=st)
    again = dev.generateImg(spp, seed=0)
    assert np.array_equal(_bits(full), _bits(again))
    n_pix, n_bad = _oracle_pixels_of_full_frame(oracle, d + name, d, spp, 0, full, name)       # held to the oracle at full size and SPP
    print("%s 1280x720 SPP %d: %d pixels against the oracle, %d channels outside 1e-6" % (name, spp, n_pix, n_bad))
    assert st.samples == 1280 * 720 * spp and st.rays_primary == 1280 * 720
    assert st.rays_shadow > 0 and st.rays_bounce > 0 and st.shade_calls >= st.rays_bounce * 0.9
    parts = np.zeros_like(full)
    for r in range(8):
        dev.generateImg(spp, seed=0, rank=r, world=8, img=parts)
    assert np.array_equal(_bits(full), _bits(parts))
    other = dev.generateImg(spp, seed=12345)
    assert not np.array_equal(_bits(full), _bits(other))
    assert abs(other.mean() - full.mean()) < 5e-3 * full.mean()
    dev.close()
    monkeypatch.setenv("MCPT_WORKSPACE_GB", "6")               # 6 GB of path state: about 14 chunks
    small = mcpt.Device(sc, 0)
    st2 = mcpt.Stats()
    chunked = small.generateImg(spp, seed=0, stats=st2)
    assert st2.launches > 2 * st.launches
    assert np.array_equal(_bits(full), _bits(chunked))
    small.close()
    sc.close()


def test_config5_frame_at_its_own_size(mcpt):
    """BASELINE config 5 as it is written: the synthetic 10 M-triangle scene (reference structures built on the GPU) at 3840x2160,
    SPP 1024 -- 8.5 G camera samples, ~24 s per frame on one MI355X, path state streamed through HBM in ~20 chunks.  The frame is
    rendered once whole and once as the 8 tile partitions an 8-GPU node would render; both must give the same bits, every sample and
    ray must be accounted for, and the picture must be a picture (lit, not saturated)."""
    from montecarlopathtracing_amd import synthetic
    sc = synthetic.make_scene(mcpt, 10_000_000, defer_build=True, width=3840, height=2160)
    assert sc.info.num_faces >= 10_000_000
    dev = mcpt.Device(sc, 0)
    st = mcpt.Stats()
    full = dev.generateImg(1024, seed=0, stats=st)
    assert st.samples == 3840 * 2160 * 1024 and st.rays_primary == 3840 * 2160
    assert st.rays_shadow > st.samples // 4 and st.rays_bounce > st.samples // 8
    parts = np.zeros_like(full)
    rays = 0
    for r in range(8):
        s8 = mcpt.Stats()
        dev.generateImg(1024, seed=0, rank=r, world=8, img=parts, stats=s8)
        rays += s8.rays_shadow + s8.rays_bounce
    assert np.array_equal(_bits(full), _bits(parts))
    assert rays == st.rays_shadow + st.rays_bounce
    q = mcpt.imshow_rgb8(full)
    assert 1 < q.mean() < 245 and (q > 0).mean() > 0.02          # a dim scene: four small quad lights over 10 M small triangles
    dev.close(); sc.close()


def test_ten_million_triangles(mcpt):
    """Config 5's scene at its real size (10 M triangles, generated; reference structures built on the GPU): the host's threaded
    SAH hierarchy and the GPU-clustered one give the same hits and the same image, both walks agree on a sample of rays (the
    reference-shaped walk visits 20 M nodes per ray, so a small sample), frames repeat and partition bit for bit."""
    from montecarlopathtracing_amd import synthetic
    sc = synthetic.make_scene(mcpt, 10_000_000, defer_build=True, width=320, height=180)
    assert sc.info.num_faces >= 10_000_000
    a = mcpt.Device(sc, 0)                                      # fast hierarchy: SAH on the host (worker threads)
    b = mcpt.Device(sc, 0, build=mcpt.BUILD_DEVICE_FAST)        # fast hierarchy: clusters on the GPU + SAH over them
    rng = np.random.default_rng(2)
    i = sc.info
    eye = np.array(i.eye)
    look = np.array(i.look_at)
    o = eye[None, :] + rng.normal(size=(200000, 3)) * 0.05
    d = (look - eye)[None, :] + rng.normal(size=(200000, 3)) * 0.4 * np.linalg.norm(look - eye)     # a wide cone around the view axis
    rays = np.hstack([o, d / np.linalg.norm(d, axis=1, keepdims=True)])
    fa, ta, pa, na = a.ray_intersect(rays)
    fb, tb, pb, nb = b.ray_intersect(rays)
    h = fa >= 0
    assert h.sum() > 10000, int(h.sum())
    assert np.array_equal(fa, fb)
    assert np.array_equal(_bits(ta[h]), _bits(tb[h])) and np.array_equal(_bits(pa[h]), _bits(pb[h])) and np.array_equal(_bits(na[h]), _bits(nb[h]))
    a.set_trace_mode(mcpt.TRACE_REFERENCE)
    fr, tr, pr, nr = a.ray_intersect(rays[:64])
    a.set_trace_mode(mcpt.TRACE_FAST)
    assert np.array_equal(fr, fa[:64]) and np.array_equal(_bits(tr[fr >= 0]), _bits(ta[:64][fr >= 0]))
    # the same scene with the hierarchy grown on the GPU by locally-ordered clustering (MCPT_BUILD_DEVICE_SAH): same answers, and about
    # the host tree's work per ray (the Morton-cluster build b needs ~1.9x its node visits)
    import time
    t0 = time.time()
    c = mcpt.Device(sc, 0, build=mcpt.BUILD_DEVICE_SAH)
    t_build = time.time() - t0
    sa, sc_ = mcpt.Stats(), mcpt.Stats()
    a.ray_intersect(rays, stats=sa)
    fc, tc, pc, nc = c.ray_intersect(rays, stats=sc_)
    assert np.array_equal(fa, fc) and np.array_equal(_bits(ta[h]), _bits(tc[h])) and np.array_equal(_bits(pa[h]), _bits(pc[h])) and np.array_equal(_bits(na[h]), _bits(nc[h]))
    assert sc_.node_visits + sc_.tri_tests <= 1.3 * (sa.node_visits + sa.tri_tests), (sc_.node_visits, sa.node_visits, sc_.tri_tests, sa.tri_tests)
    print("10 M triangles, MCPT_BUILD_DEVICE_SAH: device created in %.2f s; node visits %.2fx, triangle visits %.2fx the host tree's" % (
        t_build, sc_.node_visits / sa.node_visits, sc_.tri_tests / sa.tri_tests))
    c.close()
    ia = a.generateImg(4, seed=1)
    ib = b.generateImg(4, seed=1)
    assert ia.sum() > 0 and np.array_equal(_bits(ia), _bits(ib)) and np.array_equal(_bits(ia), _bits(a.generateImg(4, seed=1)))
    parts = np.zeros_like(ia)
    for r in range(4):
        b.generateImg(4, seed=1, rank=r, world=4, img=parts)
    assert np.array_equal(_bits(ia), _bits(parts))
    a.close(); b.close(); sc.close()
