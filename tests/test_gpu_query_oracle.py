"""-m gpu: radiance queries (mcpt_query_radiance) away from the camera against the oracle's ray-keyed entry (oracle/mcpt_oracle.c:
orc_ray_radiance, the integrator of orc_sample_radiance entered by ray; pinned by tests/test_query_oracle_cpu.py), sample by sample.

A query list is a second sample source of the render loop (k_query_pass, k_query_samples, k_query_fold), and tests/test_gpu_query.py holds
it to a frame's own camera rays, an exact sky, one form factor and the numpy restatement of the hemisphere rays.  None of those sends a ray
a camera never sends.  Here the lists of tests/query_cases.py do: origins 5 mm in front of surfaces (an extra 0.01 along d, harmless from the
eye, skips the wall), behind walls and inside solids (first hits on back faces), inside glass (the refraction's exit branch and total
reflection at depth 0), on surfaces, at interior points along the axes and face diagonals, far outside the scene, and surface points for the
hemisphere kind, among them points in concave corners whose origin 0.01 along d lies behind the neighbouring wall; ids up to 2^31 - 1 and
sample indices up to 2^31 - 2.  The comparison keeps test_gpu_env_oracle.py's helpers, bars and flip allowances (test_gpu_parity.py's); there
is no tolerance of this file's own.

(a) every ray group at every k of query_cases.K under both id vectors: dev.radiance(rays, 1, seed, ids, sample_base = k) against
    orc_ray_radiance under the pool and vote engines (the megakernel too on glassroom inside-glass and cornell-box front); hits exact list
    by list, the radiance through _check_samples over a device's eight lists together (the allowance is a rate: see
    _samples_against_the_oracle).  In the on-surface group every sample counts as an on-surface path: its source ray is one;
(b) the seams (the reference walk, no finishing pass, its lane form, a small workspace, the megakernel) on glassroom behind + inside-glass
    and cornell-box front: equal to the default device bit for bit, as the suite asserts for frames, and so to the oracle as in (a);
(c) env_scenes.open_scene under the "map" sky (the far group's misses bring Le(d)) and a light_scenes room of 9 lights under "one" and
    "tree" (the behind group picks at back-face vertices), the oracle given the restatements of the library's table and tree;
(d) spp = 8 at sample_base 0 and 2^31 - 9: mean and stderr against query_cases.fold of the oracle's eight samples on the queries none of
    whose samples is over REL_TOL, the excluded queries bounded by (a)'s allowance for the same samples; hits and the statistics;
(e) the hemisphere kind on hemi and hemi-corner: the device against the oracle run on tests/query_ref.py's rays (within 4 ulps of the
    device's, test_gpu_query.py; REL_TOL is nine decades above that), and dev.irradiance = pi times that;
(f) the comparison's power: the oracle made wrong on purpose (wrong = 1, the ray leaves o + d * 0.01, on cornell-box front; wrong = 2, the
    key's pixel word is the list position, on cornell-box behind) fails the same check, while the permutation-id list reversed passes.

Measured on an MI355X on 2026-10-19 (the figures each test prints before it asserts); the whole file runs in under 4 s:
  samples   without on-surface paths -- every group of cornell-box and veach-mis, the room of 9 lights under "one" and "tree": 0 samples over
            REL_TOL in every list under both engines and the megakernel, largest relative error 3.8e-10 (one sample of cornell-box
            on-surface; 3.8e-11 elsewhere); hits exact in every list of every scene.  With them, samples over REL_TOL / allowance / on-surface
            paths over a device's eight lists, the same under pool and vote: glassroom front 10 / 20 / 545, behind 6 / 18 / 489,
            inside-glass 13 / 91 / 2578 (the megakernel too), on-surface 6 / 394 / 11232, axes 6 / 13 / 355, far 2 / 7 / 180; open scene far
            1 / 11 / 299, inside-glass 14 / 210 / 5986 -- every one on a path with an on-surface ray, test_gpu_parity.py's refraction flips
            at its rate (1.8 % there; 0.2 % to 1.8 % here).  List by list a front, behind, axes or far list of glassroom has 17 to 66 such
            paths and 0 to 4 flips against an allowance of 2 or 3: glassroom front, random ids, k = 0 has 4 of 60 -- why the lists go
            through the check together.
  seams     the reference walk, no finishing pass, the lane form, 0.016 GB and the megakernel: 0 means, 0 standard errors and 0 hit
            counts differ from the default device's at spp 1, 8 and 48 on the three lists (0.016 GB takes the 1404 and 1332 queries of
            48 samples in 2 trace launches where the default takes 1; the reference walk and the wavefront without a finishing pass
            take 12 to 20).
  variants  open scene, far: 376 of 750 rays miss and bring Le(d), 371 not black; 318 of 387 environment shadow rays leave the scene.  Room
            of 9 lights, behind: 799 first vertices on a back face under either pick, 2065 shadow rays for 2090 shade calls.
  means     spp 8 at bases 0 and 2^31 - 9: the excluded queries are 0 on cornell-box and veach-mis and at most 13 of 568 (allowance 88) on
            glassroom; on the others mean and stderr within 4.8e-11 of the sample's scale (cornell-box on-surface; 1.1e-12 elsewhere);
            hits exact; rays_primary = samples = n * 8; shade calls and bounce rays equal the oracle's on cornell-box and veach-mis,
            within 8 of 19888 on glassroom.
  hemi      cornell-box hemi and hemi-corner: 0 of 10656 and 0 of 3504 samples over REL_TOL, largest relative error 4.8e-12; glassroom
            7 / 20 and 12 / 19 (hemi, the two bases), 1 / 2 and 1 / 2 (hemi-corner).  irradiance is pi times the mean, bit for bit, in both
            pipelines.
  power     wrong = 1 on cornell-box front: 429 of 1332 samples over REL_TOL against an allowance of 2 (0 against the right oracle), hits
            differ on 414 queries; wrong = 2 on cornell-box behind: 657 of 1332 (0 against the right oracle); the permutation-id list
            reversed: 0 against the right oracle, 663 against wrong = 2.  Each fails the check, as it must."""
import os

import numpy as np
import pytest

import env_scenes
import light_pick_ref as LP
import light_scenes
import light_tree_ref as LT
import query_cases as QC
import test_gpu_env_oracle as TE
from conftest import SCENES, extra_scene_dir
from test_lens_oracle_cpu import flip_allowance
from test_query_oracle_cpu import HEMI_PAIRS, RAY_PAIRS

pytestmark = pytest.mark.gpu

SEED = TE.SEED
W, H = QC.W, QC.H
# key -> (kind, scene name or None, lights, sky, light pick)
CASES = {"cornell-box": ("shipped", "cornell-box", 1, None, None), "glassroom": ("shipped", "glassroom", 2, None, None),
         "veach-mis": ("shipped", "veach-mis", 5, None, None), "open-sky": ("open", None, 1, "map", None),
         "nl9-one": ("lights", None, 9, None, "one"), "nl9-tree": ("lights", None, 9, None, "tree")}
# the devices of test_gpu_env_oracle.py and two more seams; "reference-walk" is the pool device under MCPT_TRACE_REFERENCE
DEVICES = dict(TE.DEVICES, **{"small-workspace": {"MCPT_TRACE_ENGINE": "pool", "MCPT_WORKSPACE_GB": "0.016"},
                              "reference-walk": {"MCPT_TRACE_ENGINE": "pool"}})
SEAMS = ("reference-walk", "no-finish", "finish-lane", "small-workspace")
SEAM_PAIRS = [("glassroom", "behind"), ("glassroom", "inside-glass"), ("cornell-box", "front")]
MEGAKERNEL_PAIRS = [("glassroom", "inside-glass"), ("cornell-box", "front")]
VARIANT_PAIRS = [("open-sky", "far"), ("open-sky", "inside-glass"), ("nl9-one", "behind"), ("nl9-tree", "behind"), ("nl9-tree", "front")]

_ORACLE_CACHE = {}          # (case, group, ids, base, spp, wrong) -> the oracle's answer: computed once per module


class Case(TE.Case):
    """test_gpu_env_oracle's case at query_cases' frame size, with its sky or light pick on both sides and the query lists of its scene"""

    def __init__(self, key, oracle, mcpt, directory):
        self.key = key
        self.kind, name, self.nl, self.sky, self.pick = CASES[key]
        self.w, self.h, self.mcpt = W, H, mcpt
        if self.kind == "open":
            name, base = "query_open_nl%d" % self.nl, directory
            env_scenes.open_scene(directory, name, self.nl, W, H)
        elif self.kind == "lights":
            name, base = "query_lights_nl%d" % self.nl, directory
            light_scenes.write(directory, name, self.nl, W, H)
        else:
            base = extra_scene_dir() if name == "glassroom" else SCENES
        self.osc = oracle.OracleScene(base + name, texture_dir=base, width=W, height=H)
        self.sc = mcpt.Scene(base, name, width=W, height=H)
        assert self.sc.info.num_lights == self.nl == self.osc.num_lights
        self.groups = QC.build(self.osc)                     # (from the scene alone, before a sky or a pick is set)
        self.devs, self.dev_sky = {}, {}
        if self.sky:
            self.set_sky(self.sky)
        if self.pick == "one":
            self.osc.set_light_pick(1, pick_ref=LP.PickRef.of_scene(self.sc))
        elif self.pick == "tree":
            self.osc.set_light_pick(2, tree_ref=LT.TreeRef.of_scene(self.sc))

    def device(self, which):
        if which not in self.devs:
            saved = {k: os.environ.pop(k, None) for k in TE.KNOBS}
            try:
                os.environ.update(DEVICES[which])
                dev = self.devs[which] = self.mcpt.Device(self.sc, 0)
            finally:
                for k, v in saved.items():
                    os.environ.pop(k, None)
                    if v is not None:
                        os.environ[k] = v
            if which == "reference-walk":
                dev.set_trace_mode(self.mcpt.TRACE_REFERENCE)
            if self.sky:
                dev.set_environment(*self.sky_value())
            if self.pick:
                dev.set_light_sampling(self.pick)
            # a lens must not enter a query: every device carries one
            dev.set_lens(aperture=0.3, focus_distance=2.5, jitter=True)
        dev = self.devs[which]
        assert dev.light_sampling()[0] == (self.pick or "all") and (dev.environment is not None) == bool(self.sky)
        return dev

    def oracle_samples(self, group, ids, base, spp, wrong=0):
        """x (n, spp, 3), hit (n, spp), on_surface (n, spp) of the oracle and its statistics, cached per module"""
        key = (self.key, group, ids, base, spp, wrong)
        if key not in _ORACLE_CACHE:
            g = self.groups[group]
            st = self.oracle_lib.Stats()
            _ORACLE_CACHE[key] = QC.oracle_samples(self.osc, g, SEED, g.ids[ids], base, spp, wrong=wrong, stats=st) + (st,)
        return _ORACLE_CACHE[key]


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in TE.KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("gpu_query_oracle_scenes")) + os.sep


@pytest.fixture(scope="module")
def cases(oracle, mcpt, scene_dir):
    """one case alive at a time (the previous one's devices go before the next one's are created); the oracle's answers outlive it"""
    made = {}

    def get(key):
        if key not in made:
            for k in list(made):
                made.pop(k).close()
            made[key] = Case(key, oracle, mcpt, scene_dir)
            made[key].oracle_lib = oracle
        return made[key]
    yield get
    for k in list(made):
        made.pop(k).close()
    _ORACLE_CACHE.clear()


def _rel(g, o):
    """per sample: the largest channel error over the sample's scale, _check_samples' measure (0 where the oracle is not finite)"""
    fin = np.isfinite(o).all(axis=-1)
    return np.where(fin, np.abs(g - o).max(axis=-1), 0.0) / np.maximum(np.abs(o).max(axis=-1), 1e-12)


def _report(what, g, o, on_surface):
    """the figures of a comparison, printed before it is asserted: the largest relative error, the samples over REL_TOL, the allowance and
    the on-surface paths"""
    err = _rel(g, o)
    print("%s: max rel %.3e, %d of %d samples over %g (allowance %d, %d on-surface paths)"
          % (what, err.max(), int((err > TE.REL_TOL).sum()), g.shape[0], TE.REL_TOL, flip_allowance(on_surface), int(on_surface.sum())))
    for i in np.flatnonzero(err > TE.REL_TOL)[:12]:
        print("    sample %d%s: device %s, oracle %s" % (i, " (on-surface path)" if on_surface[i] else "", g[i].tolist(), o[i].tolist()))


def _on_surface(group, on):
    """the on-surface paths of a comparison: the oracle's, and in the on-surface group every sample -- its source ray is one"""
    return np.ones_like(on) if group == "on-surface" else on


def _check(what, group, got, hits, x, hit, on):
    """one sample per query: the device's (mean of spp = 1, hits) against the oracle's"""
    on = _on_surface(group, on)
    _report(what, got, x, on)
    assert np.array_equal(hits, hit.astype(np.int32)), "%s: hits differ on %d queries" % (what, int((hits != hit).sum()))
    TE._check_samples(got, x, on)


# ---------------------------------------------------------------------------------------------- (a) samples, ray kind
def _samples_against_the_oracle(c, key, group, devices, flags=0):
    """Every list of the group -- both id vectors, every k of query_cases.K -- on every device: hits exact and the figures list by list; the
    radiance through _check_samples over the lists of a device together.  The flip allowance is a RATE (3.5 % of the paths that have an
    on-surface ray, 2.5e-5 of the others) and one list of glassroom has some 60 such paths, of which the known refraction flips
    (test_gpu_parity.py: 1.8 % measured) take 0 to 4: a rate asked of 60 paths decides by chance (allowance 3), asked of the 480 of the eight
    lists it does not -- and int(0.035 * sum) + 1 is never more than the lists' own allowances added up."""
    g = c.groups[group]
    assert g.n >= 100
    for which in devices:
        got, want, surface = [], [], []
        for ids in ("random", "permutation"):
            for k in QC.K:
                x, hit, on, _ = c.oracle_samples(group, ids, k, 1)
                mean, err, hits = c.device(which).radiance(g.q, 1, SEED, ids=g.ids[ids], sample_base=k, flags=flags)
                what = "%s %s %s ids, k %d, %s%s" % (key, group, ids, k, which, ", megakernel" if flags else "")
                _report(what, mean, x[:, 0], _on_surface(group, on[:, 0]))
                assert not err.any()
                assert np.array_equal(hits, hit[:, 0].astype(np.int32)), "%s: hits differ on %d queries" % (what, int((hits != hit[:, 0]).sum()))
                assert np.array_equal(np.isnan(mean), np.isnan(x[:, 0]))
                got.append(mean), want.append(x[:, 0]), surface.append(_on_surface(group, on[:, 0]))
        got, want, surface = np.concatenate(got), np.concatenate(want), np.concatenate(surface)
        _report("%s %s, %s%s, the %d lists together" % (key, group, which, ", megakernel" if flags else "", 2 * len(QC.K)), got, want, surface)
        TE._check_samples(got, want, surface)


@pytest.mark.parametrize("key,group", RAY_PAIRS)
def test_ray_samples(cases, key, group):
    _samples_against_the_oracle(cases(key), key, group, ("pool", "vote"))


@pytest.mark.parametrize("key,group", MEGAKERNEL_PAIRS)
def test_ray_samples_megakernel(cases, mcpt, key, group):
    _samples_against_the_oracle(cases(key), key, group, ("pool",), flags=mcpt.RENDER_MEGAKERNEL)


# ---------------------------------------------------------------------------------------------- (b) seams
@pytest.mark.parametrize("key,group", SEAM_PAIRS)
def test_seams(cases, mcpt, key, group):
    """The suite holds frames of the reference walk, of the wavefront without its finishing pass, of the lane form, of a small workspace and
    of the megakernel to the default device's bit for bit (test_gpu_parity.py); so are a query list's answers at spp 1, 8 and 48 (1332 queries
    of 48 samples are more paths than 0.016 GB holds at once: test_gpu_query.py's test_several_chunks), and the default device's are the oracle's
    as in (a)."""
    c = cases(key)
    g = c.groups[group]
    ids = g.ids["random"]
    for spp, base in ((1, QC.K[3]), (QC.SPP_MEAN, QC.MEAN_BASES[0]), (48, QC.K[1])):
        st = mcpt.Stats()
        want = c.device("pool").radiance(g.q, spp, SEED, ids=ids, sample_base=base, stats=st)
        if spp == 1:
            x, hit, on, _ = c.oracle_samples(group, "random", base, 1)
            _check("%s %s, k %d, default device" % (key, group, base), group, want[0], want[2], x[:, 0], hit[:, 0], on[:, 0])
        runs = [(s, c.device(s), 0) for s in SEAMS] + [("megakernel", c.device("pool"), mcpt.RENDER_MEGAKERNEL)]
        for what, dev, flags in runs:
            s2 = mcpt.Stats()
            got = dev.radiance(g.q, spp, SEED, ids=ids, sample_base=base, flags=flags, stats=s2)
            differ = [int((TE._bits(a) != TE._bits(b)).any(axis=1).sum()) for a, b in zip(got[:2], want[:2])]
            print("%s %s spp %d, %s: %d means and %d standard errors differ from the default device's; launches %d (default %d)"
                  % (key, group, spp, what, differ[0], differ[1], s2.launches, st.launches))
            assert differ == [0, 0] and np.array_equal(got[2], want[2]), what
            assert s2.samples == s2.rays_primary == g.n * spp
            if what != "megakernel":
                assert (s2.rays_bounce, s2.shade_calls) == (st.rays_bounce, st.shade_calls), what


# ---------------------------------------------------------------------------------------------- (c) variants
@pytest.mark.parametrize("key,group", VARIANT_PAIRS)
def test_variants(cases, key, group):
    c = cases(key)
    g = c.groups[group]
    _samples_against_the_oracle(c, key, group, ("pool", "vote"))
    x, hit, on, st = c.oracle_samples(group, "random", QC.K[1], 1)
    if c.sky:
        miss = ~hit[:, 0]
        le = c.osc.env_eval(g.q[miss, 3:])
        print("%s %s: %d misses bring Le(d), %d of them not black; environment shadow rays %d (%d clear), escapes %d + %d"
              % (key, group, int(miss.sum()), int((le > 0).any(axis=1).sum()), st.env_shadow, st.env_shadow_clear, st.env_escape_specular,
                 st.env_escape_transmission))
        assert np.array_equal(TE._bits(x[miss, 0]), TE._bits(le)) and st.camera_miss == int(miss.sum())
        if group == "far":
            assert miss.sum() >= 100 and (le > 0).any(axis=1).sum() >= 50 and st.env_shadow_clear > 0
    if c.pick:
        back = (g.q[:, 3:] * c.osc.trace_closest(g.q)[3]).sum(axis=1) > 0
        print("%s %s: %d first vertices on a back face, %d shadow rays for %d shade calls" % (key, group, int((back & hit[:, 0]).sum()),
                                                                                               st.rays_shadow, st.shade_calls))
        assert st.rays_shadow <= st.shade_calls                          # one light per vertex
        if group == "behind":
            assert (back & hit[:, 0]).sum() >= 100


# ---------------------------------------------------------------------------------------------- (d) means
def _device_samples(c, g, kind, ids, base, spp):
    """the device's own samples base .. base + spp - 1, one spp = 1 query per index (the hemisphere kind through its ray seam)"""
    dev = c.device("pool")
    x, hits = np.zeros((g.n, spp, 3)), np.zeros((g.n, spp), dtype=np.int32)
    for j in range(spp):
        rays = g.q if kind == "ray" else dev.query_rays(g.q, SEED, np.full(g.n, base + j, dtype=np.int32), kind="hemisphere", ids=ids)
        x[:, j], _, hits[:, j] = dev.radiance(rays, 1, SEED, ids=ids, sample_base=base + j)
    return x, hits


def _check_means(what, c, mcpt, group, base):
    """spp = SPP_MEAN: every sample as in (a); mean and stderr at REL_TOL of the sample's scale -- the largest of the query's eight samples,
    what a mean of them and an error of that mean are made of -- on the queries without a sample over REL_TOL; hits; the statistics"""
    g = c.groups[group]
    spp, ids = QC.SPP_MEAN, g.ids["random"]
    x, hit, on, ost = c.oracle_samples(group, "random", base, spp)
    on = _on_surface(group, on)
    gx, ghits = _device_samples(c, g, g.kind, ids, base, spp)
    flat = lambda a: a.reshape((g.n * spp,) + a.shape[2:])
    _report("%s: the %d samples" % (what, g.n * spp), flat(gx), flat(x), flat(on))
    TE._check_samples(flat(gx), flat(x), flat(on))
    assert np.array_equal(ghits, hit.astype(np.int32))
    excluded = (_rel(gx, x) > TE.REL_TOL).any(axis=1)
    assert excluded.sum() <= flip_allowance(flat(on))
    st = mcpt.Stats()
    if g.kind == "ray":
        mean, err, hits = c.device("pool").radiance(g.q, spp, SEED, ids=ids, sample_base=base, stats=st)
    else:
        mean, err, hits = c.device("pool")._query(g.q, ids, spp, SEED, base, mcpt.QUERY_HEMISPHERE, 0, st)
    want_mean, want_err = QC.fold(x)
    scale = np.maximum(np.abs(x).max(axis=(1, 2)), 1e-12)
    keep = ~excluded
    e_mean = np.abs(mean - want_mean).max(axis=1) / scale
    e_err = np.abs(err - want_err).max(axis=1) / scale
    print("%s: %d of %d queries excluded (allowance %d); mean within %.3e, stderr within %.3e of the sample's scale; shade calls %d, bounce rays %d "
          "(oracle %d, %d; %d on-surface rays)" % (what, int(excluded.sum()), g.n, flip_allowance(flat(on)), e_mean[keep].max(), e_err[keep].max(),
                                                   st.shade_calls, st.rays_bounce, ost.shade_calls, ost.rays_bounce, ost.rays_on_surface))
    assert np.isfinite(mean).all() and np.isfinite(err).all() and (err >= 0).all()
    assert e_mean[keep].max() <= TE.REL_TOL and e_err[keep].max() <= TE.REL_TOL
    assert np.array_equal(hits, hit.sum(axis=1).astype(np.int32))
    assert st.rays_primary == st.samples == g.n * spp == ost.samples
    if ost.rays_on_surface == 0 and group != "on-surface":
        assert (st.shade_calls, st.rays_bounce) == (ost.shade_calls, ost.rays_bounce)
    assert want_mean.max() > 0 and (want_err > 0).any()
    return mean, err, hits


@pytest.mark.parametrize("base", QC.MEAN_BASES)
@pytest.mark.parametrize("key,group", RAY_PAIRS)
def test_means(cases, mcpt, key, group, base):
    _check_means("%s %s spp %d at %d" % (key, group, QC.SPP_MEAN, base), cases(key), mcpt, group, base)


# ---------------------------------------------------------------------------------------------- (e) the hemisphere kind
@pytest.mark.parametrize("base", QC.MEAN_BASES)
@pytest.mark.parametrize("key,group", HEMI_PAIRS)
def test_hemisphere_kind(cases, mcpt, key, group, base):
    c = cases(key)
    g = c.groups[group]
    mean, err, hits = _check_means("%s %s spp %d at %d" % (key, group, QC.SPP_MEAN, base), c, mcpt, group, base)
    for flags in (0, mcpt.RENDER_MEGAKERNEL):
        E, E_err, E_hits = c.device("pool").irradiance(g.q[:, :3], g.q[:, 3:], QC.SPP_MEAN, SEED, ids=g.ids["random"], sample_base=base, flags=flags)
        assert np.array_equal(TE._bits(E), TE._bits(np.pi * mean)) and np.array_equal(TE._bits(E_err), TE._bits(np.pi * err)), flags
        assert np.array_equal(E_hits, hits)


# ---------------------------------------------------------------------------------------------- (f) the comparison's power
def test_a_ray_that_leaves_an_offset_along_fails_the_check(cases):
    """wrong = 1: the oracle's ray leaves o + d * 0.01.  The device, which passes against the right oracle, fails the same check."""
    c = cases("cornell-box")
    g = c.groups["front"]
    k = QC.K[1]
    mean, _, hits = c.device("pool").radiance(g.q, 1, SEED, ids=g.ids["random"], sample_base=k)
    x, hit, on, _ = c.oracle_samples("front", "random", k, 1)
    _check("cornell-box front against the right oracle", "front", mean, hits, x[:, 0], hit[:, 0], on[:, 0])
    bad, bad_hit, _, _ = c.oracle_samples("front", "random", k, 1, wrong=1)
    _report("cornell-box front against the oracle with wrong = 1", mean, bad[:, 0], on[:, 0])
    print("hits differ on %d queries" % int((hits != bad_hit[:, 0]).sum()))
    with pytest.raises(AssertionError):
        TE._check_samples(mean, bad[:, 0], on[:, 0])
    assert (hits != bad_hit[:, 0]).sum() > 0


def test_a_key_made_of_the_list_position_fails_the_check(cases):
    """wrong = 2: the oracle's pixel word is the list position.  The device fails the check on the random ids; on the permutation ids with
    the list reversed (position n - 1 - i, id perm[i]) it passes against the right oracle and fails against the wrong one."""
    c = cases("cornell-box")
    g = c.groups["behind"]
    k = QC.K[1]
    dev = c.device("pool")
    mean, _, hits = dev.radiance(g.q, 1, SEED, ids=g.ids["random"], sample_base=k)
    x, hit, on, _ = c.oracle_samples("behind", "random", k, 1)
    _check("cornell-box behind against the right oracle", "behind", mean, hits, x[:, 0], hit[:, 0], on[:, 0])
    bad = c.oracle_samples("behind", "random", k, 1, wrong=2)[0]
    _report("cornell-box behind against the oracle with wrong = 2", mean, bad[:, 0], on[:, 0])
    with pytest.raises(AssertionError):
        TE._check_samples(mean, bad[:, 0], on[:, 0])
    q, perm = g.q[::-1], g.ids["permutation"][::-1]
    mean, _, hits = dev.radiance(q, 1, SEED, ids=perm, sample_base=k)
    x, hit, on = c.osc.ray_radiance(SEED, q, k, ids=perm)
    _check("cornell-box behind reversed, permutation ids", "behind", mean, hits, x, hit, on)
    forward = c.oracle_samples("behind", "permutation", k, 1)[0]
    assert np.array_equal(TE._bits(x[::-1]), TE._bits(forward[:, 0]))                 # the oracle's answers go with the ids too
    bad = c.osc.ray_radiance(SEED, q, k, ids=perm, wrong=2)[0]
    _report("... against the oracle with wrong = 2", mean, bad, on)
    with pytest.raises(AssertionError):
        TE._check_samples(mean, bad, on)
