"""-m gpu: the closest-hit engines' hand-over paths and launch shapes, held bit for bit to answers that do not depend on them.

Every path here is a fallback or a launch shape of the fast walk: a ray whose stack would overflow goes to the one-lane walk (a deferred
list and k_trace_slow / k_wf_trace_slow in the trace launches, an in-place walk with pp.lane_stack in the pool engine's finishing pass), a
deferred list that overflows makes the slow pass scan every slot (and re-walk all of them when an undecided ray did not fit: redo_all),
the deep-stack kernel forms run under MCPT_SHORT_KERNEL=0, the pool engine keeps stack entries past its 8 LDS entries in a spill area,
scenes above MCPT_PRE_TEST_MAX_TRIS walk without pre-test records, and the claim schedule takes its chunk from three knobs.  None of them
may change an answer, so every case asserts
  (a) closest hits of make_rays() (face, t, p, pn) equal to the CPU oracle's bit for bit, and frames equal to the default device's frame
      and to the megakernel frame (reference-shaped walk, no engine; pinned to the oracle by test_gpu_parity.py) bit for bit;
  (b) that the path was reached, from the work counters the API returns, against the same device without the stressing knob:
      - a re-walk adds the abandoned part of a walk to the total: node_visits rises (ray_intersect, primary hits, finishing pass);
      - a hand-over in k_wf_trace moves work out of it: its own dom_node_visits falls;
      - the pool form of the finishing pass walks in place: its rise over the uncapped device is larger than the lane form's (whose
        finishing walks have the deep stack and are not capped; both forms share the primary hits), i.e. the in-place walk ran;
      - redo_all re-walks every slot: node_visits rises over the same capped run with the full list;
      - no pre-test records: MCPT_PRINT_DIAG's k_wf_trace line reports every visited triangle as a survivor (100.0 %).

Where each path is reached:
- the pool engine's in-place one-lane walk in path mode: test_stack_handover[*-pool] (rise of the pool form over the lane form);
- the voting engine's stack hand-over (k_trace_slow, k_wf_trace_slow): test_stack_handover[*-vote] (ray_intersect and primary-hit
  rises, k_wf_trace's own share falls);
- the overflow scan and redo_all, either engine, ray_intersect and the wavefront frame: test_handover_with_list_overflow;
- k_wf_trace<36,3>, k_trace_persistent<*,36,3> and the pool engine at 36 entries: every *-deep case and test_deep_form_unstressed;
  MCPT_TEST_STACK_CAP=30 is honoured only there, but no ray of these scenes needs more than 27 entries, so that case shows equal work
  (the cap leaves walks that fit alone) rather than a hand-over;
- the pool engine's spill area: test_spill_area_is_reached (deep scene; the cap-11 cases hand over only rays past 8 entries);
- no pre-test records: test_no_pre_test_records;
- the claim schedule under the chunk and block knobs, and batches that straddle 64-slot fetches: test_launch_shapes,
  test_ray_batches_straddling_64_slot_fetches (answers and work; the schedule itself is restated in test_trace_schedule_cpu.py).

Devices are created per case (knobs are read at creation) and closed at once; what the oracle and the default device say is computed
once per scene and kept for the module, like test_gpu_parity.py does.

Thinned axes (the cross product would be ~400 devices):
- the stack caps 4 and 6 run on the three shipped scenes (cornell-box: one light; veach-mis: five lights and rays with zero direction
  components that the fast walk may not take; glassroom: on-surface refraction rays), cap 11 and 30 on the generated deep scene only:
  on the shipped scenes no ray is shown to need more than 8 entries, so a cap of 11 would reach nothing there (test_spill_area_is_reached);
- the deferred-list overflow (MCPT_SLOW_LIST 1 and 8) runs with ray_intersect and the wavefront frame, the two entry points with a
  deferred list (the finishing pass walks in place), on veach-mis (caps 4, 6) and the deep scene (cap 11);
- launch shapes run on cornell-box and veach-mis with the default stack form: the schedule does not look at the stack, and the
  deep-stack form's launches are the same code with another template argument (covered by every *-deep case);
- no pre-test runs with the short form on the three shipped scenes (the records are read the same way by both forms)."""
import os
import re

import numpy as np
import pytest

from conftest import SCENES, extra_scene_dir, make_rays

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 160, 90, 2, 3
N_RAYS = 8192
BIG = "1000000000"          # MCPT_FINISH_PATHS: the finishing pass takes every frame right after the first logic pass
KNOBS = ("MCPT_TRACE_ENGINE", "MCPT_FINISH_ENGINE", "MCPT_FINISH_PATHS", "MCPT_SHORT_KERNEL", "MCPT_TEST_STACK_CAP", "MCPT_SLOW_LIST",
         "MCPT_PRE_TEST_MAX_TRIS", "MCPT_TRACE_MIN_CHUNK", "MCPT_TRACE_MAX_CHUNK", "MCPT_TRACE_BLOCK_RAYS", "MCPT_PRINT_DIAG")
FORMS = {"short": {}, "deep": {"MCPT_SHORT_KERNEL": "0"}}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _deep_geometry():
    """3 000 large triangles, all through the middle of the box, and a lamp above them: every ray through the middle crosses hundreds of
    them, every node's children overlap, and the walk pushes up to three siblings per level (synthetic.write_obj's dict)."""
    rng = np.random.default_rng(1234)
    n = 3000
    c = rng.uniform(-0.3, 0.3, size=(n, 1, 3))
    v = (c + rng.normal(scale=1.0, size=(n, 3, 3))).reshape(n, 9)
    lamp = np.array([[-0.5, 3.5, -0.5, 0.5, 3.5, -0.5, 0.5, 3.5, 0.5], [-0.5, 3.5, -0.5, 0.5, 3.5, 0.5, -0.5, 3.5, 0.5]])
    v = np.vstack([v, lamp])
    e1, e2 = v[:, 3:6] - v[:, 0:3], v[:, 6:9] - v[:, 0:3]
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    mat = np.zeros(v.shape[0], dtype=np.int32)
    mat[n:] = 1
    rec = np.array([[0.6, 0.5, 0.4, 0, 0, 0, 1, 1], [0, 0, 0, 0, 0, 0, 1, 1]], dtype=np.float64)
    return dict(v=v, vn=np.tile(nrm, 3), material=mat, material_rec=rec, material_names=["grey", "lamp"],
                light_material=np.array([1], dtype=np.int32), light_radiance=np.full((1, 3), 12.0),
                eye=[1.5, 2.5, 6.5], look_at=[0.0, 0.0, 0.0], up=[0.0, 1.0, 0.0], fovy=50.0, width=W, height=H)


class _World:
    """per scene: oracle scene, library scene, rays and the oracle's closest hits, the default and megakernel frames"""

    def __init__(self, mcpt, oracle, tmp):
        self.M, self.O, self.tmp = mcpt, oracle, tmp
        self.scenes = {}
        self.base = {}
        self.n_runs = 0

    def scene(self, name):
        if name not in self.scenes:
            if name == "deep":
                from montecarlopathtracing_amd import synthetic
                base = str(self.tmp.mktemp("deep")) + os.sep
                synthetic.write_obj(_deep_geometry(), base, "deep")
            else:
                base = extra_scene_dir() if name == "glassroom" else SCENES
            osc = self.O.OracleScene(base + name, texture_dir=base, width=W, height=H)
            sc = self.M.Scene(base, name, width=W, height=H)
            rays = make_rays(osc, N_RAYS, seed=29)
            want = osc.trace_closest(rays)
            dev = self.device(sc, {})
            try:
                frame = dev.generateImg(SPP, seed=SEED)
                mega = dev.generateImg(SPP, seed=SEED, flags=self.M.RENDER_MEGAKERNEL)
            finally:
                dev.close()
            assert np.array_equal(_bits(frame), _bits(mega))
            self.scenes[name] = dict(osc=osc, sc=sc, rays=rays, want=want, frame=frame, mega=mega)
        return self.scenes[name]

    def device(self, sc, knobs):
        old = {k: os.environ.get(k) for k in KNOBS}
        try:
            for k in KNOBS:
                os.environ.pop(k, None)
            os.environ.update({k: str(v) for k, v in knobs.items()})
            if "MCPT_TRACE_ENGINE" in knobs:
                assert sc.trace_engine() == knobs["MCPT_TRACE_ENGINE"]
            return self.M.Device(sc, 0)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v

    def run(self, name, knobs, rays=True, frame=True):
        """(a) for a device created under `knobs`; returns (Stats of ray_intersect, Stats of the frame)"""
        s = self.scene(name)
        dev = self.device(s["sc"], knobs)
        sr, sf = self.M.Stats(), self.M.Stats()
        try:
            if rays:
                # (every run takes the rays in another order: a slot the run left unwritten cannot pass by holding what an earlier run
                # of the same rays left in a recycled buffer)
                self.n_runs += 1
                perm = np.random.default_rng(self.n_runs).permutation(s["rays"].shape[0])
                gf, gt, gp, gpn = dev.ray_intersect(np.ascontiguousarray(s["rays"][perm]), stats=sr)
                of, ot, op, opn = (a[perm] for a in s["want"])
                assert np.array_equal(of, gf), "%s %s: %d of %d rays hit another face than the oracle's" % (name, knobs, int((of != gf).sum()), of.size)
                h = of >= 0
                for a, b in ((ot, gt), (op, gp), (opn, gpn)):
                    assert np.array_equal(_bits(a[h]), _bits(b[h])), "%s %s: t / p / pn differ from the oracle's" % (name, knobs)
            if frame:
                img = dev.generateImg(SPP, seed=SEED, stats=sf)
                assert np.array_equal(_bits(img), _bits(s["frame"])), "%s %s: %d channels differ from the default frame" % (
                    name, knobs, int((_bits(img) != _bits(s["frame"])).sum()))
                assert np.array_equal(_bits(img), _bits(s["mega"]))
        finally:
            dev.close()
        return sr, sf

    def baseline(self, name, knobs, **kw):
        """the same run without the stressing knobs, once per set of knobs"""
        key = (name, tuple(sorted(knobs.items())), tuple(sorted(kw.items())))
        if key not in self.base:
            self.base[key] = self.run(name, knobs, **kw)
        return self.base[key]

    def close(self):
        for s in self.scenes.values():
            s["sc"].close()
            s["osc"].close()


@pytest.fixture(scope="module")
def world(mcpt, oracle, tmp_path_factory):
    w = _World(mcpt, oracle, tmp_path_factory)
    yield w
    w.close()


def _engine_forms(engine):
    """the frame forms of an engine: the wavefront frame (every bounce through k_wf_trace), the finishing pass that runs where this
    engine runs (pool: k_wf_finish_pool, in-place walk; vote: k_wf_finish, lane form) and, for the pool engine, the lane form beside it"""
    f = {"wavefront": {"MCPT_FINISH_PATHS": "0"}, "finish": {"MCPT_FINISH_PATHS": BIG}}
    if engine == "pool":
        f["lane"] = {"MCPT_FINISH_PATHS": BIG, "MCPT_FINISH_ENGINE": "lane"}
    return f


STACK_CASES = [(s, c) for s in ("cornell-box", "veach-mis", "glassroom") for c in (4, 6)] + [("deep", 11)]


def _stack_ids(p):
    return "%s-cap%d" % p


# ------------------------------------------------------------------------------------------------------- 1 + 3: stack hand-over
# (cap 30 only in the deep form: the short form's 27 entries are below it, so there it is the uncapped run of test_deep_form_unstressed)
STACK_PARAMS = [(c, f) for c in STACK_CASES for f in FORMS] + [(("deep", 30), "deep")]


@pytest.mark.parametrize("engine", ["pool", "vote"])
@pytest.mark.parametrize("case,form", STACK_PARAMS, ids=["%s-%s" % (_stack_ids(c), f) for c, f in STACK_PARAMS])
def test_stack_handover(world, engine, form, case):
    """MCPT_TEST_STACK_CAP at every entry point: ray_intersect (ArrayRaySource), generateImg's primary hits (PrimaryRaySource) and
    bounces in k_wf_trace* (wavefront frame, MCPT_FINISH_PATHS=0), the finishing pass in the engine's own form and, for the pool engine,
    the lane form."""
    name, cap = case
    plain = dict(FORMS[form], MCPT_TRACE_ENGINE=engine)
    capped = dict(plain, MCPT_TEST_STACK_CAP=str(cap))
    rise = {}
    for fname, fk in _engine_forms(engine).items():
        sr0, sf0 = world.baseline(name, dict(plain, **fk), rays=fname == "wavefront")
        sr, sf = world.run(name, dict(capped, **fk), rays=fname == "wavefront")
        if cap == 30:
            # no ray of these scenes needs more than 27 entries: the cap is honoured (the deep form's 36 entries are cut to 30) but hands
            # nothing over, so the work is the uncapped deep form's -- the cap leaves every walk that fits alone
            assert (sr.node_visits, sf.node_visits, sf.dom_node_visits) == (sr0.node_visits, sf0.node_visits, sf0.dom_node_visits)
            continue
        if fname == "wavefront":
            assert sr.node_visits > sr0.node_visits, ("ray_intersect: no ray re-walked", sr.node_visits, sr0.node_visits)
            assert sf.dom_node_visits < sf0.dom_node_visits, ("k_wf_trace gave no ray away", sf.dom_node_visits, sf0.dom_node_visits)
        assert sf.node_visits > sf0.node_visits, (fname, "no primary hit re-walked", sf.node_visits, sf0.node_visits)
        rise[fname] = sf.node_visits - sf0.node_visits
    if engine == "pool" and cap != 30:
        assert rise["finish"] > rise["lane"], ("no in-place walk in k_wf_finish_pool", rise)


# ------------------------------------------------------------------------------------------------------- 2 + 3: list overflow
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("engine", ["pool", "vote"])
@pytest.mark.parametrize("slow", [1, 8])
@pytest.mark.parametrize("case", [("veach-mis", 4), ("veach-mis", 6), ("deep", 11)], ids=_stack_ids)
def test_handover_with_list_overflow(world, engine, form, slow, case):
    """Stack hand-overs into a deferred list of 1 or 8 entries: the rays that do not fit set redo_all, and the slow pass re-walks every
    slot.  veach-mis also has rays with a zero direction component, which the fast walk may not take (they go to the list first)."""
    name, cap = case
    capped = dict(FORMS[form], MCPT_TRACE_ENGINE=engine, MCPT_TEST_STACK_CAP=str(cap), MCPT_FINISH_PATHS="0")
    plain = dict(capped)
    del plain["MCPT_TEST_STACK_CAP"]
    if name == "veach-mis":
        assert int((world.scene(name)["rays"][:, 3:] == 0).any(axis=1).sum()) > 100
    sr0, sf0 = world.baseline(name, plain)
    sr1, sf1 = world.baseline(name, capped)
    sr, sf = world.run(name, dict(capped, MCPT_SLOW_LIST=str(slow)))
    # redo_all.  With the full list the slow pass re-walks the rays in it: those the fast walk may not take and those handed over.  With
    # the list overflowed it scans every slot and re-walks those the fast walk may not take -- and, with redo_all set, every other slot
    # too.  Without redo_all the handed-over rays that did not fit would be left unwritten (fewer re-walks than with the full list, and
    # (a) fails); with it there are more.  The capped runs above show that rays are handed over (test_stack_handover).
    assert sr1.node_visits > sr0.node_visits
    assert sr.node_visits > sr1.node_visits, ("ray_intersect: no redo_all", sr.node_visits, sr1.node_visits, sr0.node_visits)
    assert sf.node_visits > sf1.node_visits, ("frame: no redo_all", sf.node_visits, sf1.node_visits, sf0.node_visits)


# ------------------------------------------------------------------------------------------------------- 3: deep form unstressed
@pytest.mark.parametrize("engine", ["pool", "vote"])
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis", "glassroom", "deep"])
def test_deep_form_unstressed(world, engine, name):
    """MCPT_SHORT_KERNEL=0 without a cap: the voting engine's <36,3> kernels and the pool engine at a 36-entry cap, every entry point.
    Same answers, and the same work as the short form wherever no ray needs more than the short form's 27 entries."""
    for fname, fk in _engine_forms(engine).items():
        sr, sf = world.run(name, dict(FORMS["deep"], MCPT_TRACE_ENGINE=engine, **fk), rays=fname == "wavefront")
        sr0, sf0 = world.baseline(name, dict(MCPT_TRACE_ENGINE=engine, **fk), rays=fname == "wavefront")
        if fname == "wavefront":
            assert sr.node_visits == sr0.node_visits, (sr.node_visits, sr0.node_visits)
            assert sf.dom_node_visits == sf0.dom_node_visits, (sf.dom_node_visits, sf0.dom_node_visits)


# ------------------------------------------------------------------------------------------------------- 4: spill area
def test_spill_area_is_reached(world, mcpt):
    """The pool engine keeps entries 0..7 of a ray's stack in LDS and the rest in a global spill area (trace_pool.hpp st_put / st_get).
    A cap of 11 hands over only the rays that would push past entry 8 (sp > cap - 3); if the capped run does more work than the
    uncapped one, some ray went past its 8 LDS entries, so the uncapped runs of that scene -- every test above -- used the spill area.
    The generated deep scene is built for that (and its hierarchy is checked: every box exact, the stack need as recorded)."""
    import fast_bvh_ref as R
    s = world.scene("deep")
    dev = world.device(s["sc"], {"MCPT_TRACE_ENGINE": "pool"})
    try:
        info, nodes, faces = dev.fast_hierarchy()
    finally:
        dev.close()
    assert info.enabled == 1
    lo, hi = R.face_boxes(s["sc"].faces()[0])
    R.check_hierarchy(nodes, faces, lo, hi, stack_need=info.cw_stack_need)
    assert 11 < info.cw_stack_need < 36, info.cw_stack_need
    for form in FORMS:
        plain = dict(FORMS[form], MCPT_TRACE_ENGINE="pool", MCPT_FINISH_PATHS="0")
        sr0, sf0 = world.baseline("deep", plain)
        sr, sf = world.baseline("deep", dict(plain, MCPT_TEST_STACK_CAP="11"))
        assert sr.node_visits > sr0.node_visits and sf.dom_node_visits < sf0.dom_node_visits, form


def test_deferred_rays_are_reported_against_the_dominant_kernels_rays(world, mcpt, capfd, tmp_path):
    """MCPT_PRINT_DIAG's account of the hand-over, read back from the device counters by name: on the deep scene under a cap of 11 entries
    k_wf_trace defers rays to the exact walk, and both lines that quote the kernel's ray count quote Stats.dom_rays."""
    from montecarlopathtracing_amd import synthetic
    base = str(tmp_path) + os.sep
    synthetic.write_obj(_deep_geometry(), base, "deep")
    sc = mcpt.Scene(base, "deep", width=48, height=32)
    dev = world.device(sc, {"MCPT_TEST_STACK_CAP": "11", "MCPT_FINISH_PATHS": "0", "MCPT_PRINT_DIAG": "1"})
    st = mcpt.Stats()
    try:
        capfd.readouterr()
        dev.generateImg(2, seed=SEED, stats=st)
        err = capfd.readouterr().err
    finally:
        dev.close()
        sc.close()
    print(err)
    deferred = re.findall(r"rays deferred to the exact walk by k_wf_trace: (\d+) of (\d+)", err)
    traced = re.findall(r"k_wf_trace: (\d+) rays,", err)
    assert len(deferred) == 1 and len(traced) == 1, err
    a, b = (int(x) for x in deferred[0])
    assert a > 0 and b == st.dom_rays and int(traced[0]) == st.dom_rays, (a, b, traced, st.dom_rays)


# ------------------------------------------------------------------------------------------------------- 5: no pre-test
_SURVIVE = re.compile(r"k_wf_trace: (\d+) rays, .*\(([0-9.]+) % of the visited triangles survive the pre-test\)")


@pytest.mark.parametrize("engine", ["pool", "vote"])
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis", "glassroom"])
def test_no_pre_test_records(world, capfd, engine, name):
    """MCPT_PRE_TEST_MAX_TRIS=0: no scene gets the fp32 pre-test records (F.pre == nullptr), every visited triangle goes to the exact
    test.  Same answers and the same node and triangle visits; MCPT_PRINT_DIAG shows the pre-test rejected nothing (100 % survive),
    where the default device's run rejects some."""
    for fname, fk in _engine_forms(engine).items():
        plain = dict(MCPT_TRACE_ENGINE=engine, MCPT_PRINT_DIAG="1", **fk)
        wave = fname == "wavefront"
        sr0, sf0 = world.baseline(name, plain, rays=wave)
        out0 = capfd.readouterr().err
        sr, sf = world.run(name, dict(plain, MCPT_PRE_TEST_MAX_TRIS="0"), rays=wave)
        out = capfd.readouterr().err
        assert (sf.node_visits, sf.tri_tests) == (sf0.node_visits, sf0.tri_tests)
        if wave:
            assert (sr.node_visits, sr.tri_tests) == (sr0.node_visits, sr0.tri_tests)
            m = _SURVIVE.findall(out)
            assert m and all(float(p) == 100.0 for n, p in m if int(n) > 0), out
            m0 = _SURVIVE.findall(out0)
            assert not m0 or any(float(p) < 100.0 for n, p in m0 if int(n) > 0), out0


# ------------------------------------------------------------------------------------------------------- 6: launch shapes
SHAPES = {
    "chunk64": {"MCPT_TRACE_MIN_CHUNK": "64", "MCPT_TRACE_MAX_CHUNK": "64"},
    "tail_only": {"MCPT_TRACE_MIN_CHUNK": "16777216", "MCPT_TRACE_MAX_CHUNK": "16777216"},
    "block256": {"MCPT_TRACE_BLOCK_RAYS": "256"},
    "one_block": {"MCPT_TRACE_BLOCK_RAYS": "1073741824"},
}


@pytest.mark.parametrize("engine", ["pool", "vote"])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_launch_shapes(world, engine, shape, name):
    """Other claim schedules (tests/test_trace_schedule_cpu.py restates them): chunks of 64, chunks so large that every claim is a tail
    ticket, a block per 256 rays, one block for everything.  The voting engine's closest-hit and primary launches take persistent_chunk
    and a block per 256 rays whatever the knobs say (kernels.hip launch_persistent), so for them only the answers are asserted; its
    k_wf_trace launches and every pool-engine launch follow the knobs.  The work is that of the default schedule: a schedule decides
    which wave walks a ray, not how."""
    for fname, fk in _engine_forms(engine).items():
        wave = fname == "wavefront"
        sr, sf = world.run(name, dict(SHAPES[shape], MCPT_TRACE_ENGINE=engine, **fk), rays=wave)
        sr0, sf0 = world.baseline(name, dict(MCPT_TRACE_ENGINE=engine, **fk), rays=wave)
        assert (sf.node_visits, sf.tri_tests, sf.dom_node_visits) == (sf0.node_visits, sf0.tri_tests, sf0.dom_node_visits)
        if wave:
            assert (sr.node_visits, sr.tri_tests) == (sr0.node_visits, sr0.tri_tests)


BATCHES = [1, 2, 63, 64, 65, 255, 257, 4095, 4097, 4096 * 7 + 1]


@pytest.mark.parametrize("engine", ["pool", "vote"])
@pytest.mark.parametrize("shape", ["default"] + list(SHAPES))
def test_ray_batches_straddling_64_slot_fetches(world, engine, shape):
    """ray_intersect batches of 1 .. 4096 * 7 + 1 rays under every launch shape: claims that end inside a 64-slot fetch, a single
    partial fetch, one ticket, tail tickets only.  The rays are drawn from make_rays() of veach-mis."""
    s = world.scene("veach-mis")
    dev = world.device(s["sc"], dict(SHAPES.get(shape, {}), MCPT_TRACE_ENGINE=engine))
    try:
        n_all = s["rays"].shape[0]
        for n in BATCHES:
            idx = np.random.default_rng(n).integers(0, n_all, size=n)        # (other rays in every slot from one batch to the next)
            gf, gt, gp, gpn = dev.ray_intersect(np.ascontiguousarray(s["rays"][idx]))
            of, ot, op, opn = (a[idx] for a in s["want"])
            assert np.array_equal(of, gf), (n, int((of != gf).sum()))
            h = of >= 0
            for a, b in ((ot, gt), (op, gp), (opn, gpn)):
                assert np.array_equal(_bits(a[h]), _bits(b[h])), n
    finally:
        dev.close()
