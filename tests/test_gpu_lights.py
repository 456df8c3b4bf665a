"""-m gpu: the path pipelines against the oracle across light counts (tests/light_scenes.py).

The number of lights nl shapes every path kernel: the per-light planes of the wavefront state (wavefront.hip: wf_carve) and of the
pool-form finishing pass's path records (wavefront_logic.hip: WfPaths), the ray slots a path takes in the pool form (R = nl + 1 of
KT = 20 per lane, NP = KT / R paths per lane), the gate between the pool form and the lane form (nl + 1 <= KT / 2), the chunk size of a
frame (per-light state per path).  Counts here: 3, 4, 6 (NP = 5, 4, 2), 9 (NP = 2, R * NP = KT: the path mask reaches bit 19),
10 (the first count past the gate: the lane form), 20 and 40 (large per-light state, many chunks in a small workspace).

(a) the "finite" scenes against the oracle, under both trace engines: per-sample radiance, SPP-4 frames of both pipelines with the
    oracle's work counts, 8-bit output;
(b) every route through the pipelines -- megakernel, wavefront without a finishing pass, the finishing pass in pool and lane form,
    a late hand-over, a two-block logic grid, a small workspace, partitions, the voting engine -- gives the same frame bit for bit
    and the same counts;
(c) under a lens the wavefront equals the megakernel; progressive passes add up to the one-shot frame;
(d) the "nan" scenes: NaN exactly where the oracle has it, the finite values within the bars of (a), every route the same bits."""
import os

import numpy as np
import pytest

import light_scenes

pytestmark = pytest.mark.gpu

REL_TOL = 1e-9                  # per-sample radiance (test_gpu_parity.py)
IMG_TOL = 1e-6                  # per image channel: float accumulator
OTHER_FLIP_RATE = 2.5e-5        # of paths without an on-surface ray (test_gpu_parity.py); these scenes have none
N_SAMPLES = 3000
KNOBS = ("MCPT_TRACE_ENGINE", "MCPT_FINISH_ENGINE", "MCPT_FINISH_PATHS", "MCPT_WORKSPACE_GB", "MCPT_LOGIC_GRID")

# (lights, variant, width, height)
CASES = {"nl3": (3, "finite", 96, 64), "nl4": (4, "finite", 96, 64), "nl6": (6, "finite", 96, 64), "nl9": (9, "finite", 96, 64),
         "nl9-ragged": (9, "finite", 33, 17), "nl10": (10, "finite", 96, 64), "nl20": (20, "finite", 96, 64),
         "nl40": (40, "finite", 96, 64), "nl3-nan": (3, "nan", 96, 64), "nl10-nan": (10, "nan", 96, 64)}
FINITE = [c for c in CASES if CASES[c][1] == "finite" and CASES[c][2] == 96]
NAN = [c for c in CASES if CASES[c][1] == "nan"]

# knob settings of the wavefront routes (each device is created while its setting is in the environment)
DEVICES = {
    "default": {},
    "pool": {"MCPT_TRACE_ENGINE": "pool"},
    "vote": {"MCPT_TRACE_ENGINE": "vote"},
    "no-finish": {"MCPT_FINISH_PATHS": "0"},
    "vote-no-finish": {"MCPT_TRACE_ENGINE": "vote", "MCPT_FINISH_PATHS": "0"},
    "finish-lane": {"MCPT_FINISH_ENGINE": "lane"},
    "late-finish": {"MCPT_FINISH_PATHS": "2000"},
    "logic-grid-2": {"MCPT_LOGIC_GRID": "2", "MCPT_FINISH_PATHS": "0"},
    "small-workspace": {"MCPT_WORKSPACE_GB": "0.011"},
}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _counts(st):
    return (st.rays_shadow + st.shadow_skipped, st.rays_bounce, st.shade_calls, st.samples)


class Case:
    def __init__(self, key, oracle, mcpt, directory):
        self.key = key
        self.nl, self.variant, self.w, self.h = CASES[key]
        self.mcpt = mcpt
        name = "lights_" + key.replace("-", "_")
        light_scenes.write(directory, name, self.nl, self.w, self.h, variant=self.variant)
        self.osc = oracle.OracleScene(directory + name, texture_dir=directory, width=self.w, height=self.h)
        self.sc = mcpt.Scene(directory, name, width=self.w, height=self.h)
        assert self.sc.info.num_lights == self.nl == self.osc.num_lights
        self.devs = {}

    def device(self, which):
        if which not in self.devs:
            saved = {k: os.environ.pop(k, None) for k in KNOBS}
            try:
                os.environ.update(DEVICES[which])
                if "MCPT_TRACE_ENGINE" in DEVICES[which]:
                    assert self.sc.trace_engine() == DEVICES[which]["MCPT_TRACE_ENGINE"]
                self.devs[which] = self.mcpt.Device(self.sc, 0)
            finally:
                for k, v in saved.items():
                    os.environ.pop(k, None)
                    if v is not None:
                        os.environ[k] = v
        return self.devs[which]

    def oracle_cached(self, what, fn):
        key = (self.key, what)
        if key not in _ORACLE_CACHE:
            _ORACLE_CACHE[key] = fn()
        return _ORACLE_CACHE[key]

    def close(self):
        for d in self.devs.values():
            d.close()
        self.sc.close()
        self.osc.close()


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("gpu_light_scenes")) + os.sep


_CASES = {}
_ORACLE_CACHE = {}          # (case, what) -> the oracle's answer: computed once per module, kept when a case's devices go


@pytest.fixture(scope="module")
def cases(oracle, mcpt, scene_dir):
    """one Case per key, built on first use and kept for the module (the oracle's answers are computed once per case)"""
    def get(key):
        if key not in _CASES:
            # one case alive at a time: the previous one's devices go before the next one's are created
            for k in list(_CASES):
                _CASES.pop(k).close()
            _CASES[key] = Case(key, oracle, mcpt, scene_dir)
        return _CASES[key]
    yield get
    for k in list(_CASES):
        _CASES.pop(k).close()
    _ORACLE_CACHE.clear()


def _oracle_samples(c, oracle):
    rng = np.random.default_rng(5)
    pix = rng.integers(0, c.w * c.h, size=N_SAMPLES).astype(np.int32)
    k = rng.integers(0, 64, size=N_SAMPLES).astype(np.int32)

    def run():
        o = np.zeros((N_SAMPLES, 3))
        on_surface = 0
        for i, (p, kk) in enumerate(zip(pix, k)):
            st = oracle.Stats()
            o[i] = c.osc.sample_radiance(77, int(p // c.w), int(p % c.w), int(kk), stats=st)
            on_surface += st.rays_on_surface
        assert on_surface == 0
        return o
    return pix, k, c.oracle_cached("samples", run)


def _oracle_image(c, oracle, spp=4):
    def run():
        ost = oracle.Stats()
        img = c.osc.render(spp, seed=3, stats=ost)
        assert ost.rays_on_surface == 0
        return img, ost
    return c.oracle_cached(("image", spp), run)


def _check_samples(g, o):
    """NaN exactly where the oracle has it; the finite samples within REL_TOL (no flip budget: no on-surface rays here)"""
    assert np.array_equal(np.isnan(g), np.isnan(o)), "NaN masks differ on %d samples" % int((np.isnan(g) != np.isnan(o)).any(axis=1).sum())
    fin = np.isfinite(o).all(axis=1)
    assert np.isfinite(g[fin]).all()
    scale = np.maximum(np.abs(o[fin]).max(axis=1), 1e-12)
    err = np.abs(g[fin] - o[fin]).max(axis=1) / scale
    flips = int((err > REL_TOL).sum())
    assert flips <= int(g.shape[0] * OTHER_FLIP_RATE), "radiance mismatch on %d samples (max rel %.3e)" % (flips, err.max())
    assert abs(g[fin].sum() - o[fin].sum()) <= 1e-9 * np.abs(o[fin]).sum() and np.abs(o[fin]).sum() > 0
    return fin


def _check_image(img, ref, spp, oracle, mcpt):
    """NaN masks equal; finite channels within IMG_TOL (flip budget of one sample); the 8-bit output equal wherever they are"""
    assert img.shape == ref.shape
    assert np.array_equal(np.isnan(img), np.isnan(ref)), "NaN masks differ on %d channels" % int((np.isnan(img) != np.isnan(ref)).sum())
    fin = np.isfinite(ref)
    assert np.isfinite(img[fin]).all()
    rel = np.abs(img[fin] - ref[fin]) / np.maximum(np.abs(ref[fin]), 1e-6)
    bad = int((rel > IMG_TOL).sum())
    assert bad <= max(3, int(img.size * spp * OTHER_FLIP_RATE)), "%d pixel channels differ (max rel %.3e)" % (bad, rel.max())
    png = int((mcpt.imshow_rgb8(img) != oracle.quantize(ref)).sum())
    assert png <= bad, "%d 8-bit channels differ (%d channels off the bar)" % (png, bad)


# ---------------------------------------------------------------------------------------------- (a) and (d): against the oracle
@pytest.mark.parametrize("engine", ["pool", "vote"])
@pytest.mark.parametrize("key", FINITE + NAN)
def test_sample_radiance(cases, oracle, key, engine):
    c = cases(key)
    pix, k, o = _oracle_samples(c, oracle)
    g = c.device(engine).sample_radiance(77, pix, k)
    _check_samples(g, o)
    nan = np.isnan(o).any(axis=1)
    if c.variant == "finite":
        assert not nan.any()
    else:
        assert 0 < nan.sum() < 0.5 * nan.size, nan.sum()         # the no-triangle regime is really reached


@pytest.mark.parametrize("engine", ["pool", "vote"])
@pytest.mark.parametrize("key", FINITE + NAN)
def test_image_matches_oracle(cases, oracle, mcpt, key, engine):
    c = cases(key)
    spp = 4
    ref, ost = _oracle_image(c, oracle, spp)
    # the wavefront with its default finishing pass (small frames: every path handed over after the first logic pass), without one
    # (every bounce a pass of k_wf_logic), and the megakernel (one lane per sample, no engine beyond the primary rays)
    pipelines = [("wavefront", engine, 0), ("wavefront without a finishing pass", "no-finish" if engine == "pool" else "vote-no-finish", 0)]
    if engine == "pool":
        pipelines.append(("megakernel", engine, mcpt.RENDER_MEGAKERNEL))
    for what, which, flags in pipelines:
        st = mcpt.Stats()
        img = c.device(which).generateImg(spp, seed=3, stats=st, flags=flags)
        _check_image(img, ref, spp, oracle, mcpt)
        assert st.rays_shadow + st.shadow_skipped == ost.rays_shadow, what
        assert (st.rays_bounce, st.shade_calls, st.samples) == (ost.rays_bounce, ost.shade_calls, ost.samples), what
    if c.variant == "finite":
        assert np.isfinite(ref).all()
    else:
        assert np.isnan(ref).any() and np.isfinite(ref).any()


def test_megakernel_traces_lights_behind_the_surface(oracle, mcpt, scene_dir):
    """Without a light pick the reference traces a shadow ray to every light, also to one behind the surface, whose answer it does not
    use.  The megakernel does the same and counts it in rays_shadow; the wavefront leaves such a ray out and counts it as skipped.  Two
    lights, one sunk below the floor: behind the floor at every vertex there."""
    name, w, h, spp = "lights_sunk", 16, 16, 4
    light_scenes.write(scene_dir, name, 2, w, h, sunk=(1,))
    osc = oracle.OracleScene(scene_dir + name, texture_dir=scene_dir, width=w, height=h)
    sc = mcpt.Scene(scene_dir, name, width=w, height=h)
    dev = mcpt.Device(sc, 0)
    try:
        ost, wst, mst = oracle.Stats(), mcpt.Stats(), mcpt.Stats()
        ref = osc.render(spp, seed=3, stats=ost)
        wf = dev.generateImg(spp, seed=3, stats=wst)
        mk = dev.generateImg(spp, seed=3, stats=mst, flags=mcpt.RENDER_MEGAKERNEL)
        # with the primary rays on the reference-shaped walk too, every ray of the frame is walked as the oracle walks it: the same work
        rst = mcpt.Stats()
        dev.set_trace_mode(mcpt.TRACE_REFERENCE)
        mk_ref = dev.generateImg(spp, seed=3, stats=rst, flags=mcpt.RENDER_MEGAKERNEL)
    finally:
        dev.close()
        sc.close()
        osc.close()
    print("shadow rays: oracle %d, megakernel %d (+ %d skipped), wavefront %d (+ %d skipped)"
          % (ost.rays_shadow, mst.rays_shadow, mst.shadow_skipped, wst.rays_shadow, wst.shadow_skipped))
    assert ost.rays_on_surface == 0
    assert ost.rays_shadow > wst.rays_shadow > 0                    # the scene really has lights behind surfaces
    assert wst.rays_shadow + wst.shadow_skipped == ost.rays_shadow
    assert (mst.rays_shadow, mst.shadow_skipped) == (ost.rays_shadow, 0)
    assert (mst.rays_bounce, mst.shade_calls, mst.samples) == (ost.rays_bounce, ost.shade_calls, ost.samples)
    assert int((_bits(mk) != _bits(wf)).sum()) == 0
    print("work: oracle %d box tests, %d triangle tests; megakernel %d node visits, %d triangle tests"
          % (ost.box_tests, ost.tri_tests, rst.node_visits, rst.tri_tests))
    assert (rst.node_visits, rst.tri_tests) == (ost.box_tests, ost.tri_tests)       # the rays behind the surface included
    assert (rst.rays_shadow, rst.shadow_skipped) == (ost.rays_shadow, 0) and int((_bits(mk_ref) != _bits(mk)).sum()) == 0
    _check_image(mk, ref, spp, oracle, mcpt)


# ---------------------------------------------------------------------------------------------- (b) and (d): every route
@pytest.mark.parametrize("key", list(CASES))
def test_every_route_gives_the_same_frame(cases, mcpt, key):
    c = cases(key)
    for spp in ((4, 32) if c.nl <= 9 else (4,)):
        base_st = mcpt.Stats()
        base = c.device("default").generateImg(spp, seed=3, stats=base_st)
        routes = {}
        st = mcpt.Stats()
        routes["megakernel"] = (c.device("default").generateImg(spp, seed=3, flags=mcpt.RENDER_MEGAKERNEL, stats=st), _counts(st))
        for which in ("no-finish", "finish-lane", "late-finish", "logic-grid-2", "small-workspace", "vote", "pool"):
            st = mcpt.Stats()
            routes[which] = (c.device(which).generateImg(spp, seed=3, stats=st), _counts(st))
        parts = np.zeros_like(base)
        total = np.zeros(4, dtype=np.int64)
        for r in range(3):
            st = mcpt.Stats()
            c.device("default").generateImg(spp, seed=3, rank=r, world=3, img=parts, stats=st)
            total += np.array(_counts(st), dtype=np.int64)
        routes["partitions"] = (parts, tuple(int(x) for x in total))
        for which, (img, counts) in routes.items():
            bad = int((_bits(img) != _bits(base)).sum())
            assert bad == 0, "%s spp %d: %d channels differ from the default route" % (which, spp, bad)
            assert counts == _counts(base_st), (which, spp, counts, _counts(base_st))
        assert base_st.samples == c.w * c.h * spp
        if c.variant == "nan":
            assert np.isnan(base).any() and np.isfinite(base).any()
        else:
            assert np.isfinite(base).all() and base.sum() > 0


# ---------------------------------------------------------------------------------------------- (c) lens and progressive
LENS = dict(aperture=0.02, focus_distance=0.0, jitter=True, per_sample=True)


@pytest.mark.parametrize("key", ["nl10", "nl40"])
def test_wavefront_equals_megakernel_under_a_lens(cases, mcpt, key):
    c = cases(key)
    dev = c.device("default")
    pin = dev.generateImg(8, seed=3)
    dev.set_lens(**LENS)
    try:
        wf = dev.generateImg(8, seed=3)
        mk = dev.generateImg(8, seed=3, flags=mcpt.RENDER_MEGAKERNEL)
    finally:
        dev.set_lens()
    bad = int((_bits(wf) != _bits(mk)).sum())
    assert bad == 0, "%d channels differ between the wavefront and the megakernel" % bad
    assert (_bits(wf) != _bits(pin)).sum() > wf.size // 4          # the lens changes the picture
    assert np.isfinite(wf).all()


def test_progressive_passes_add_up(cases, mcpt):
    c = cases("nl40")
    for which in ("default", "small-workspace"):
        dev = c.device(which)
        ref = dev.generateImg(16, seed=5)
        pr = dev.progressive(16, seed=5)
        try:
            for n in (1, 6, 2, 7):
                pr.step(n)
            assert pr.done == 16
            img = pr.image()
        finally:
            pr.close()
        bad = int((_bits(img) != _bits(ref)).sum())
        assert bad == 0, "%s: %d channels differ from the one-shot frame" % (which, bad)
