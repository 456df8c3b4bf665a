"""-m gpu: the environment light against the oracle's environment mode (oracle/mcpt_oracle.c, restated from include/mcpt.h and pinned by
tests/test_env_cpu.py), sample by sample and frame by frame.

env_light_sample, env_escape and env_camera_miss (csrc/env.hpp) are shared by every pipeline, so the pipelines' agreement with each other
(test_gpu_env.py) cannot see a mistake in them or in what the kernels pass to them.  Here:
(a) scenes with 0, 1, 2, 3 and 5 lights (env_scenes.open_scene without and with an emitter, light_scenes' nl3, cornell-box, glassroom,
    veach-mis) under test_gpu_env.py's two skies: per-sample radiance under both trace engines within REL_TOL of the oracle; SPP-4 frames
    of the wavefront (default finishing pass, none, the lane form) and of the megakernel within IMG_TOL of orc_render, with its 8-bit
    output and its work counts; on the open scene the oracle's counters prove every kind of environment path was reached;
(b) the edge maps (env_scenes.EDGE_MAPS) at the device seams against env_ref, bit for bit, and a 48x27 frame of the open scene under each
    map against the oracle."""
import os

import numpy as np
import pytest

import env_ref
import env_scenes
import light_scenes
from conftest import SCENES, extra_scene_dir

pytestmark = pytest.mark.gpu

REL_TOL = 1e-9                  # per-sample radiance (test_gpu_parity.py)
IMG_TOL = 1e-6                  # per image channel: float accumulator
ON_SURFACE_FLIP_RATE = 0.035    # of the paths that have an on-surface ray (test_gpu_parity.py)
OTHER_FLIP_RATE = 2.5e-5        # of all other paths (test_gpu_parity.py)
N_SAMPLES = 3000
SPP = 4
SEED = 77
KNOBS = ("MCPT_TRACE_ENGINE", "MCPT_FINISH_ENGINE", "MCPT_FINISH_PATHS", "MCPT_WORKSPACE_GB", "MCPT_LOGIC_GRID")
DEVICES = {
    "pool": {"MCPT_TRACE_ENGINE": "pool"},
    "vote": {"MCPT_TRACE_ENGINE": "vote"},
    "no-finish": {"MCPT_TRACE_ENGINE": "pool", "MCPT_FINISH_PATHS": "0"},
    "finish-lane": {"MCPT_TRACE_ENGINE": "pool", "MCPT_FINISH_ENGINE": "lane"},
}
# what a frame is rendered through: (device, render flags); the megakernel flag is looked up when the module runs
PIPELINES = [("wavefront", "pool", 0), ("wavefront without a finishing pass", "no-finish", 0), ("lane finishing form", "finish-lane", 0),
             ("megakernel", "pool", "RENDER_MEGAKERNEL")]

# key -> (kind, lights, width, height)
CASES = {"open-nl0": ("open", 0, 96, 64), "open-nl1": ("open", 1, 96, 64), "nl3": ("lights", 3, 96, 64),
         "cornell-box": ("shipped", 1, 96, 64), "glassroom": ("shipped", 2, 96, 64), "veach-mis": ("shipped", 5, 96, 64),
         "edge": ("open", 0, 48, 27)}
# floors of the oracle's counters over the sample set of an open scene: every kind of environment path is really reached
PATH_FLOORS = {"env_shadow_clear": 100, "env_shadow_blocked": 20, "env_escape_specular": 20, "env_escape_transmission": 10,
               "camera_miss": 100}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _counts(st):
    return (st.rays_shadow + st.shadow_skipped, st.rays_bounce, st.shade_calls, st.samples)


class Case:
    def __init__(self, key, oracle, mcpt, directory):
        self.key = key
        self.kind, self.nl, self.w, self.h = CASES[key]
        self.mcpt = mcpt
        if self.kind == "open":
            name = "env_open_nl%d_%dx%d" % (self.nl, self.w, self.h)
            env_scenes.open_scene(directory, name, self.nl, self.w, self.h)
            base = directory
        elif self.kind == "lights":
            name = "env_lights_nl%d" % self.nl
            light_scenes.write(directory, name, self.nl, self.w, self.h)
            base = directory
        else:
            name = key
            base = extra_scene_dir() if key == "glassroom" else SCENES
        self.osc = oracle.OracleScene(base + name, texture_dir=base, width=self.w, height=self.h)
        self.sc = mcpt.Scene(base, name, width=self.w, height=self.h)
        assert self.sc.info.num_lights == self.nl == self.osc.num_lights
        self.devs = {}
        self.dev_sky = {}
        self.sky = None

    def device(self, which):
        if which not in self.devs:
            saved = {k: os.environ.pop(k, None) for k in KNOBS}
            try:
                os.environ.update(DEVICES[which])
                self.devs[which] = self.mcpt.Device(self.sc, 0)
            finally:
                for k, v in saved.items():
                    os.environ.pop(k, None)
                    if v is not None:
                        os.environ[k] = v
        dev = self.devs[which]
        if self.dev_sky.get(which) != self.sky:
            dev.set_environment(*self.sky_value())
            self.dev_sky[which] = self.sky
        return dev

    def set_sky(self, sky):
        """sky: a key of env_scenes.SKIES or of env_scenes.EDGE_MAPS"""
        self.sky = sky
        z = self.osc.set_environment(*self.sky_value())
        assert z == env_ref.EnvRef(*self.sky_value()).Z > 0

    def sky_value(self):
        return env_scenes.SKIES[self.sky] if self.sky in env_scenes.SKIES else env_scenes.EDGE_MAPS[self.sky]

    def oracle_cached(self, what, fn):
        key = (self.key, self.sky, what)
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
    return str(tmp_path_factory.mktemp("gpu_env_scenes")) + os.sep


_CASES = {}
_ORACLE_CACHE = {}          # (case, sky, what) -> the oracle's answer: computed once per module


@pytest.fixture(scope="module")
def cases(oracle, mcpt, scene_dir):
    """one Case per key, built on first use; one case alive at a time (the previous one's devices go before the next one's are made)"""
    def get(key):
        if key not in _CASES:
            for k in list(_CASES):
                _CASES.pop(k).close()
            _CASES[key] = Case(key, oracle, mcpt, scene_dir)
        return _CASES[key]
    yield get
    for k in list(_CASES):
        _CASES.pop(k).close()
    _ORACLE_CACHE.clear()


ENV_FIELDS = ("env_shadow", "env_shadow_clear", "env_escape_specular", "env_escape_transmission", "camera_miss")


def _oracle_samples(c, oracle):
    rng = np.random.default_rng(5)
    pix = rng.integers(0, c.w * c.h, size=N_SAMPLES).astype(np.int32)
    k = rng.integers(0, 64, size=N_SAMPLES).astype(np.int32)

    def run():
        o = np.zeros((N_SAMPLES, 3))
        on_surface = np.zeros(N_SAMPLES, dtype=bool)
        kinds = dict.fromkeys(ENV_FIELDS, 0)
        for i, (p, kk) in enumerate(zip(pix, k)):
            st = oracle.Stats()
            o[i] = c.osc.sample_radiance(SEED, int(p // c.w), int(p % c.w), int(kk), stats=st)
            on_surface[i] = st.rays_on_surface > 0
            for f in ENV_FIELDS:
                kinds[f] += getattr(st, f)
        return o, on_surface, kinds
    return (pix, k) + c.oracle_cached("samples", run)


def _oracle_frame(c, oracle):
    def run():
        ost = oracle.Stats()
        img = c.osc.render(SPP, seed=3, stats=ost)
        miss = c.osc.trace_closest(c.osc.primary_rays())[0].reshape(c.h, c.w) < 0
        return img, ost, miss
    return c.oracle_cached("frame", run)


def _check_samples(g, o, on_surface):
    """NaN exactly where the oracle has it; the finite samples within REL_TOL, under test_gpu_parity's flip budgets"""
    assert np.array_equal(np.isnan(g), np.isnan(o)), "NaN masks differ on %d samples" % int((np.isnan(g) != np.isnan(o)).any(axis=1).sum())
    fin = np.isfinite(o).all(axis=1)
    assert np.isfinite(g[fin]).all()
    scale = np.maximum(np.abs(o).max(axis=1), 1e-12)
    err = np.where(fin, np.abs(g - o).max(axis=1), 0.0) / scale
    flip = err > REL_TOL
    n = g.shape[0]
    assert int((flip & ~on_surface).sum()) <= int(n * OTHER_FLIP_RATE), "radiance mismatch on %d ordinary samples (max rel %.3e)" % (
        int((flip & ~on_surface).sum()), err[~on_surface].max())
    assert int((flip & on_surface).sum()) <= max(2, int(on_surface.sum() * ON_SURFACE_FLIP_RATE) + 1), (
        int((flip & on_surface).sum()), int(on_surface.sum()))
    same = fin & ~flip
    assert abs(g[same].sum() - o[same].sum()) <= 1e-9 * np.abs(o[same]).sum() and np.abs(o[same]).sum() > 0


def _flip_rate(on_surface):
    """expected flipped samples per sample: test_gpu_parity's rates weighted by the share of paths with an on-surface ray"""
    return OTHER_FLIP_RATE + ON_SURFACE_FLIP_RATE * float(on_surface.mean())


def _check_frame(what, img, st, ref, ost, miss, rate, oracle, mcpt):
    """finite channels within IMG_TOL (flip budget); a missed pixel is the oracle's fold of Le bit for bit; the 8-bit output equal wherever
    the channels agree; the oracle's work counts (exactly, but for the paths a flip may send another way)"""
    assert img.shape == ref.shape
    assert np.array_equal(np.isnan(img), np.isnan(ref)), "%s: NaN masks differ on %d channels" % (what, int((np.isnan(img) != np.isnan(ref)).sum()))
    fin = np.isfinite(ref)
    assert np.isfinite(img[fin]).all(), what
    rel = np.abs(img[fin] - ref[fin]) / np.maximum(np.abs(ref[fin]), 1e-6)
    bad = int((rel > IMG_TOL).sum())
    budget = max(3, int(img.size * SPP * rate))
    assert bad <= budget, "%s: %d pixel channels differ (max rel %.3e, budget %d)" % (what, bad, rel.max(), budget)
    assert np.array_equal(_bits(img[miss]), _bits(ref[miss])), what
    png = int((mcpt.imshow_rgb8(img) != oracle.quantize(ref)).sum())
    assert png <= bad, "%s: %d 8-bit channels differ (%d channels off the bar)" % (what, png, bad)
    want = (ost.rays_shadow, ost.rays_bounce, ost.shade_calls, ost.samples)
    got = _counts(st)
    if ost.rays_on_surface == 0:
        assert got == want, (what, got, want)
    else:                        # a flipped refraction path does other work (test_gpu_parity.py): the bar of its image mean
        for g, w in zip(got, want):
            assert abs(g - w) <= (2e-3 + 25 * rate) * w, (what, got, want)


@pytest.mark.parametrize("sky", sorted(env_scenes.SKIES))
@pytest.mark.parametrize("key", [k for k in CASES if k != "edge"])
def test_against_the_oracle(cases, oracle, mcpt, key, sky):
    c = cases(key)
    c.set_sky(sky)
    pix, k, o, on_surface, kinds = _oracle_samples(c, oracle)
    for engine in ("pool", "vote"):
        g = c.device(engine).sample_radiance(SEED, pix, k)
        _check_samples(g, o, on_surface)
    if c.kind == "open":
        seen = dict(kinds, env_shadow_blocked=kinds["env_shadow"] - kinds["env_shadow_clear"])
        for f, floor in PATH_FLOORS.items():
            assert seen[f] >= floor, (f, seen)
    ref, ost, miss = _oracle_frame(c, oracle)
    rate = _flip_rate(on_surface)
    for what, which, flags in PIPELINES:
        st = mcpt.Stats()
        img = c.device(which).generateImg(SPP, seed=3, stats=st, flags=getattr(mcpt, flags) if isinstance(flags, str) else flags)
        _check_frame(what, img, st, ref, ost, miss, rate, oracle, mcpt)
    assert ost.env_shadow > 0 and ost.rays_shadow > 0


# ---------------------------------------------------------------------------------------------- (b) the edge maps
EDGE = sorted(env_scenes.EDGE_MAPS)


@pytest.mark.parametrize("name", EDGE)
def test_edge_map_seams_match_the_restatement(cases, name):
    c = cases("edge")
    c.set_sky(name)
    rgb, scale = env_scenes.EDGE_MAPS[name]
    dev = c.device("pool")
    ref = env_ref.EnvRef(rgb, scale)
    info = dev.environment
    assert (info["width"], info["height"], info["scale"]) == (ref.W, ref.H, scale) and info["Z"] == ref.Z > 0
    rng = np.random.default_rng(len(name) + 100)
    pix = rng.integers(0, c.w * c.h, size=5000).astype(np.int32)
    ks = rng.integers(0, 1000, size=5000).astype(np.int32)
    dirs = [rng.normal(size=(3000, 3)), [[0, 1, 0], [0, -1, 0], [1, 0, 0], [0, 0, 1], [-1, 0, 0], [0, 0, -1], [1, 0, -1e-9]]]
    for depth in (0, 5):
        d, pdf, le = dev.environment_sample(9, pix, ks, depth)
        i, j, dr, pr, lr = ref.sample_u(*env_ref.vertex_uniforms(9, pix, ks, depth, c.nl))
        assert np.array_equal(_bits(pdf), _bits(pr)) and np.array_equal(_bits(le), _bits(lr)), depth
        assert np.abs(d - dr).max() <= 1e-15, depth
        assert np.all(ref.lum[i, j] > 0) and np.all(np.isfinite(pdf) & (pdf > 0)) and np.isfinite(le).all()
        dirs.append(d)
    dirs = np.concatenate(dirs)
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    phi = np.mod(np.arctan2(dirs[:, 2], dirs[:, 0]), 2 * np.pi) * ref.W / (2 * np.pi)
    keep = np.abs(phi - np.round(phi)) * (2 * np.pi / ref.W) >= 1e-12
    assert np.array_equal(_bits(dev.environment_eval(dirs)[keep]), _bits(ref.eval(dirs)[keep]))


@pytest.mark.parametrize("name", EDGE)
def test_edge_map_frames_match_the_oracle(cases, oracle, mcpt, name):
    c = cases("edge")
    c.set_sky(name)
    ref, ost, miss = _oracle_frame(c, oracle)
    assert miss.any() and not miss.all() and np.isfinite(ref).all()
    # the flip budget with the frame's on-surface rays per sample for the share of paths that have one (an upper bound of it)
    rate = OTHER_FLIP_RATE + ON_SURFACE_FLIP_RATE * min(1.0, ost.rays_on_surface / ost.samples)
    for what, which, flags in PIPELINES:
        st = mcpt.Stats()
        img = c.device(which).generateImg(SPP, seed=3, stats=st, flags=getattr(mcpt, flags) if isinstance(flags, str) else flags)
        _check_frame("%s, %s" % (name, what), img, st, ref, ost, miss, rate, oracle, mcpt)
