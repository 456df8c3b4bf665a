"""-m gpu: MCPT_LIGHTS_ONE and MCPT_LIGHTS_TREE against an oracle that picks (oracle/mcpt_oracle.c: orc_scene_set_light_pick, pinned by
tests/test_light_pick_oracle_cpu.py), sample by sample and frame by frame.

Every pipeline shades a picked light through one function (csrc/vertex.hpp: light_sample_one), so the pipelines' agreement with each other
cannot see a mistake in it, and the z tests of test_gpu_light_pick.py / test_gpu_light_tree.py cannot see one on a small share of the
vertices.  Here the oracle is set to the device's mode and weights -- its table and tree are the numpy restatements', which other tests hold
to the library's bit for bit -- and walks the same paths (the pick draws from a Philox block nothing else uses), so the comparison keeps
test_gpu_lights.py's per-sample bar, helpers and constants; there is no tolerance of this file's own.

With a pick the lights share ONE plane of the wavefront state: R = 2 ray slots per path whatever nl is, and the gate between the pool form
and the lane form of the finishing pass is always open.  What nl still shapes: the Philox block base of the bounce, environment and pick
draws (nl, nl + 1, nl + 2, nl + 3), the length of the table (its binary search, the clamp to the last light of non-zero weight) and the
depth of the tree, ceil(log2 nl) levels.

(a) the rooms of light_scenes.py at 2 (the smallest table, the tree of one inner node), 3 (an odd median split), 9, 9 at 33x17 (a partial
    wave and a partial tile), 10 and 40 lights (the deepest tree, the longest table) under the default weights; 2 lights under [1, 3]; 40
    lights under caller weights with zeros (the last light's among them: the clamp; lights never picked) and a 10^6 ratio (a large 1 / p);
    the "nan" rooms of 3 and 10 lights -- under both modes: per-sample radiance under both trace engines, SPP-4 frames of the wavefront
    with and without its finishing pass and of the megakernel, their 8-bit output, the oracle's work counts;
(b) under the tree at 10 lights, the routes that carry T * c / p across a hand-over (the lane form, a late hand-over, a two-block logic
    grid, a small workspace), each against the oracle's frame;
(c) ENV x PICK: env_scenes.open_scene with 2 and 3 lights under the "map" sky, with test_gpu_env_oracle.py's comparison and bars (the glass
    box has on-surface rays: its flip budget is theirs);
(d) the comparison's power: the oracle made wrong on purpose (1 / p at depth 0 only; the light's draws from block 0) fails the same check.

The "nan" rooms: with a pick a sample goes NaN only where the PICKED light's area draw finds no triangle, and that light has no light
before it to inherit a material from -- NaN must appear exactly where the oracle has it.  The oracle alone, with the sample set and the seed
of test_gpu_lights.py, reaches a NaN share above 0 and below 0.5 on both rooms in both modes; no seed had to be chosen."""
import os

import numpy as np
import pytest

import env_scenes
import light_pick_ref as LP
import light_scenes
import light_tree_ref as LT
import test_gpu_env_oracle as TE
import test_gpu_lights as TL

pytestmark = pytest.mark.gpu

MODES = ("one", "tree")


def _zeros_and_ratio(nl):
    """caller weights over six decades (1 and 10^6 are both there) with zeros at the first, a middle and the last light"""
    w = 10.0 ** np.random.default_rng(40).uniform(0.0, 6.0, size=nl)
    w[1], w[2] = 1.0, 1e6
    w[[0, nl // 2, nl - 1]] = 0.0
    return w


# key -> (lights, variant, width, height, caller weights or None)
CASES = {"nl2": (2, "finite", 96, 64, None), "nl2-w13": (2, "finite", 96, 64, np.array([1.0, 3.0])), "nl3": (3, "finite", 96, 64, None),
         "nl9": (9, "finite", 96, 64, None), "nl9-ragged": (9, "finite", 33, 17, None), "nl10": (10, "finite", 96, 64, None),
         "nl40": (40, "finite", 96, 64, None), "nl40-zeros": (40, "finite", 96, 64, _zeros_and_ratio(40)),
         "nl3-nan": (3, "nan", 96, 64, None), "nl10-nan": (10, "nan", 96, 64, None)}
ROUTES = ("finish-lane", "late-finish", "logic-grid-2", "small-workspace")

_ORACLE_CACHE = {}          # (case, mode, what) -> the oracle's answer: computed once per module


class _Picking:
    """what a case of either kind adds to its parent: the mode both sides are in, devices that follow it, a cache keyed by it"""
    mode = None

    def set_mode(self, mode):
        """mode: None ("all"), "one" or "tree" -- on the oracle now, on each device when it is next asked for"""
        self.mode = mode
        if mode is None:
            self.osc.set_light_pick(0)
        elif mode == "one":
            self.osc.set_light_pick(1, pick_ref=LP.PickRef.of_scene(self.sc, self.weights))
        else:
            self.osc.set_light_pick(2, tree_ref=LT.TreeRef.of_scene(self.sc, self.weights))

    def device(self, which):
        dev = super().device(which)
        if self.dev_mode.get(which) != self.mode:
            dev.set_light_sampling(self.mode, None if self.mode is None else self.weights)
            self.dev_mode[which] = self.mode
        assert dev.light_sampling()[0] == (self.mode or "all")
        return dev

    def cache_key(self, what):
        return (self.key, self.mode, what)

    def oracle_cached(self, what, fn):
        key = self.cache_key(what)
        if key not in _ORACLE_CACHE:
            _ORACLE_CACHE[key] = fn()
        return _ORACLE_CACHE[key]


class Case(_Picking, TL.Case):
    def __init__(self, key, oracle, mcpt, directory):
        self.key = key
        self.nl, self.variant, self.w, self.h, self.weights = CASES[key]
        self.mcpt = mcpt
        name = "pick_" + key.replace("-", "_")
        light_scenes.write(directory, name, self.nl, self.w, self.h, variant=self.variant)
        self.osc = oracle.OracleScene(directory + name, texture_dir=directory, width=self.w, height=self.h)
        self.sc = mcpt.Scene(directory, name, width=self.w, height=self.h)
        assert self.sc.info.num_lights == self.nl == self.osc.num_lights
        self.devs, self.dev_mode = {}, {}


class EnvCase(_Picking, TE.Case):
    def __init__(self, nl, oracle, mcpt, directory):
        self.key, self.kind, self.nl, self.w, self.h, self.weights = "open-nl%d" % nl, "open", nl, 96, 64, None
        self.mcpt = mcpt
        name = "pick_open_nl%d" % nl
        env_scenes.open_scene(directory, name, nl, self.w, self.h)
        self.osc = oracle.OracleScene(directory + name, texture_dir=directory, width=self.w, height=self.h)
        self.sc = mcpt.Scene(directory, name, width=self.w, height=self.h)
        assert self.sc.info.num_lights == self.nl == self.osc.num_lights
        self.devs, self.dev_sky, self.dev_mode, self.sky = {}, {}, {}, None

    def cache_key(self, what):
        return (self.key, self.sky, self.mode, what)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in TL.KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("gpu_pick_oracle_scenes")) + os.sep


@pytest.fixture(scope="module")
def cases(oracle, mcpt, scene_dir):
    """one case alive at a time (the previous one's devices go before the next one's are created); the oracle's answers outlive it"""
    made = {}

    def get(key):
        if key not in made:
            for k in list(made):
                made.pop(k).close()
            made[key] = Case(key, oracle, mcpt, scene_dir) if key in CASES else EnvCase(key, oracle, mcpt, scene_dir)
        return made[key]
    yield get
    for k in list(made):
        made.pop(k).close()
    _ORACLE_CACHE.clear()


def _report(what, g, o):
    """the figures of a comparison, printed before it is asserted: the largest relative error, the samples over REL_TOL, the NaN share"""
    fin = np.isfinite(o).all(axis=1) & np.isfinite(g).all(axis=1)
    err = np.abs(g[fin] - o[fin]).max(axis=1) / np.maximum(np.abs(o[fin]).max(axis=1), 1e-12)
    print("%s: max rel %.3e, %d of %d samples over %g, NaN share %.4f (oracle) %.4f (device)"
          % (what, err.max(), int((err > TL.REL_TOL).sum()), g.shape[0], TL.REL_TOL, np.isnan(o).any(axis=1).mean(), np.isnan(g).any(axis=1).mean()))


# ---------------------------------------------------------------------------------------------- (a) the rooms
@pytest.mark.parametrize("engine", ["pool", "vote"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", list(CASES))
def test_sample_radiance(cases, oracle, key, mode, engine):
    c = cases(key)
    c.set_mode(mode)
    pix, k, o = TL._oracle_samples(c, oracle)                    # (asserts that no ray started on a surface)
    g = c.device(engine).sample_radiance(77, pix, k)
    _report("%s %s %s" % (key, mode, engine), g, o)
    TL._check_samples(g, o)
    nan = np.isnan(o).any(axis=1)
    if c.variant == "finite":
        assert not nan.any()
    else:
        assert 0 < nan.sum() < 0.5 * nan.size, nan.sum()         # the picked light's no-triangle regime is really reached


@pytest.mark.parametrize("engine", ["pool", "vote"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", list(CASES))
def test_image_matches_oracle(cases, oracle, mcpt, key, mode, engine):
    c = cases(key)
    spp = 4
    c.set_mode(None)
    _, ast = TL._oracle_image(c, oracle, spp)
    c.set_mode(mode)
    ref, ost = TL._oracle_image(c, oracle, spp)
    # the oracle's own paths are its mode-0 paths; one shadow ray per vertex in place of nl
    assert (ost.rays_bounce, ost.shade_calls, ost.samples) == (ast.rays_bounce, ast.shade_calls, ast.samples)
    assert ast.rays_shadow % c.nl == 0 and ost.rays_shadow == ast.rays_shadow // c.nl > 0
    pipelines = [("wavefront", engine, 0), ("wavefront without a finishing pass", "no-finish" if engine == "pool" else "vote-no-finish", 0)]
    if engine == "pool":
        pipelines.append(("megakernel", engine, mcpt.RENDER_MEGAKERNEL))
    for what, which, flags in pipelines:
        st = mcpt.Stats()
        img = c.device(which).generateImg(spp, seed=3, stats=st, flags=flags)
        TL._check_image(img, ref, spp, oracle, mcpt)
        assert st.rays_shadow + st.shadow_skipped == ost.rays_shadow, what
        assert (st.rays_bounce, st.shade_calls, st.samples) == (ost.rays_bounce, ost.shade_calls, ost.samples), what
    if c.variant == "finite":
        assert np.isfinite(ref).all()
    else:
        assert np.isnan(ref).any() and np.isfinite(ref).any()


# ---------------------------------------------------------------------------------------------- (b) routes with a hand-over
@pytest.mark.parametrize("route", ROUTES)
def test_route_matches_oracle_under_the_tree(cases, oracle, mcpt, route):
    c = cases("nl10")
    c.set_mode("tree")
    ref, ost = TL._oracle_image(c, oracle, 4)
    st = mcpt.Stats()
    img = c.device(route).generateImg(4, seed=3, stats=st)
    TL._check_image(img, ref, 4, oracle, mcpt)
    assert st.rays_shadow + st.shadow_skipped == ost.rays_shadow
    assert (st.rays_bounce, st.shade_calls, st.samples) == (ost.rays_bounce, ost.shade_calls, ost.samples)


# ---------------------------------------------------------------------------------------------- (c) under an environment
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nl", [2, 3])
def test_open_scene_under_a_sky(cases, oracle, mcpt, nl, mode):
    """ENV = 1 with PICK = 1, 2: the picked light's plane and the environment's, each with its own shadow ray; 1 / p never reaches the
    environment's term.  (mcpt's Stats carries no count of the environment's shadow rays to hold against the oracle's env_shadow; they are in
    rays_shadow + shadow_skipped, which is held.)"""
    c = cases(nl)
    c.set_sky("map")
    c.set_mode(mode)
    pix, k, o, on_surface, kinds = TE._oracle_samples(c, oracle)
    assert np.isfinite(o).all() and kinds["env_shadow_clear"] > 0 and kinds["env_shadow"] > kinds["env_shadow_clear"]
    for engine in ("pool", "vote"):
        g = c.device(engine).sample_radiance(TE.SEED, pix, k)
        _report("open-nl%d %s %s" % (nl, mode, engine), g, o)
        TE._check_samples(g, o, on_surface)
    ref, ost, miss = TE._oracle_frame(c, oracle)
    rate = TE._flip_rate(on_surface)
    for what, which, flags in (("wavefront", "pool", 0), ("megakernel", "pool", mcpt.RENDER_MEGAKERNEL)):
        st = mcpt.Stats()
        img = c.device(which).generateImg(TE.SPP, seed=3, stats=st, flags=flags)
        TE._check_frame(what, img, st, ref, ost, miss, rate, oracle, mcpt)
    c.set_mode(None)
    ast = TE._oracle_frame(c, oracle)[1]
    # per vertex: the environment's shadow ray as in mode 0, and one light's in place of nl
    assert (ost.env_shadow, ost.env_shadow_clear) == (ast.env_shadow, ast.env_shadow_clear) and ost.env_shadow > 0
    assert (ost.rays_shadow - ost.env_shadow) * nl == ast.rays_shadow - ast.env_shadow > 0


# ---------------------------------------------------------------------------------------------- (d) the comparison's power
@pytest.mark.parametrize("mode", MODES)
def test_a_wrong_oracle_fails_the_sample_check(cases, oracle, mode):
    """Nothing wrong goes into the library: the ORACLE is made wrong (oracle_lib.set_light_pick(wrong=...)), in the two ways a z test of
    block means is weakest against -- the factor 1 / p applied at depth 0 only, and the picked light's draws taken from block 0 -- and the
    device's samples, which pass against the right oracle, fail the same check against each."""
    c = cases("nl9")
    c.set_mode(mode)
    pix, k, o = TL._oracle_samples(c, oracle)
    g = c.device("pool").sample_radiance(77, pix, k)
    TL._check_samples(g, o)
    table, tree = LP.PickRef.of_scene(c.sc), LT.TreeRef.of_scene(c.sc)
    try:
        for wrong in (1, 2):
            c.osc.set_light_pick(1 if mode == "one" else 2, pick_ref=table, tree_ref=tree, wrong=wrong)
            bad = np.array([c.osc.sample_radiance(77, int(p // c.w), int(p % c.w), int(kk)) for p, kk in zip(pix[:600], k[:600])])
            _report("nl9 %s against the oracle with wrong = %d" % (mode, wrong), g[:600], bad)
            with pytest.raises(AssertionError):
                TL._check_samples(g[:600], bad)
    finally:
        c.set_mode(mode)
