"""-m gpu: the path pipelines against the oracle across material edge cases (tests/material_scenes.py; the conditions under which the
comparison means something are tests/test_material_scenes_cpu.py's, whose sample plan this takes).

Every path kernel shades through vertex.hpp (vertex_surface, bounce_sample, first_vertex_throughput) and shade_common.hpp (brdf_sample,
refract_dir, frcp, fsqrt), and what those do is decided by a material's Kd, Ks, Ns, Ni and map_Kd.  The other oracle tests run the
materials the shipped scenes and light_scenes.py happen to have; here every swatch of material_scenes.ROWS is an edge of those functions.
There is no tolerance of this file's own: REL_TOL and OTHER_FLIP_RATE are test_gpu_lights.py's, ON_SURFACE_FLIP_RATE test_gpu_parity.py's,
asked of every row on its own (with test_gpu_parity.py's floor of 2 for the on-surface paths), so that a failure names the material.

(a) sample_radiance on the plan against the oracle, "opaque" and "glass", under the pool and vote engines, row by row;
(b) frames: "opaque" at 96x64 and a ragged 33x17, SPP 4, against orc_render as test_gpu_lights._check_image does, with the oracle's
    shadow, bounce, shade and sample counts -- the wavefront's default route, without a finishing pass, the vote engine, the megakernel;
    "glass": every route of test_gpu_lights.DEVICES gives the megakernel's frame bit for bit with equal counters (against the oracle
    the samples of (a) carry it);
(c) the first vertex shaded per sample -- set_lens(aperture=0, jitter=True), the oracle's lens set to match: the samples of rows O7, G5 and
    G6 (a texel with Ks, a texel on glass, interpolated normals on glass) meet the bars of (a); the wavefront equals the megakernel;
(d) light picks "one" and "tree" on "glass", the oracle given the restatements of the library's table and tree
    (test_gpu_light_pick_oracle.py's mixin and report): the samples of the plan; and frames under a pick, where the wavefront state is
    folded and the first vertex's throughput is formed again from the pixel's record -- "opaque" against the oracle's frame, "glass"
    against the megakernel's;
(e) the caller's rays: dev.radiance against orc_ray_radiance on 257 rays, 86 of which start inside the bodies of G1-G6 -- their first hit
    is from inside, cos_in > 0 at depth 0, which no camera path reaches -- axis-parallel directions among them
    (test_gpu_query_oracle.py's check);
(f) O10 (Ni 0.8) equals the device's own Ni 1 sibling bit for bit, samples and frame.

Measured on an MI355X on 2026-10-21 (the figures each test prints before it asserts).  The whole file -- 14 tests, scenes of 148 and
288 faces, devices cached per case -- runs in 2.1 s; test_gpu_lights.py, in the same session, in 7.6 s.
  samples   "opaque": 0 of 2200 samples over REL_TOL under both engines, largest relative error 2.6e-13.  "glass", the same under pool and
            vote: 0 of the 2903 samples without an on-surface ray; with one, samples over REL_TOL / on-surface samples (rate): G1 2 / 117
            (0.017), G2 0 / 130, G3 1 / 83 (0.012), G4 2 / 78 (0.026), G5 3 / 120 (0.025), G6 1 / 126 (0.008) -- 9 of 654, 1.4 %,
            test_gpu_parity.py's refraction flips at its rate (1.8 % there).  Samples of the opaque rows whose path reaches a glass body
            after a bounce: O4 2 / 6, O6 1 / 4, O7 2 / 8, O9 2 / 6, O10 2 / 2, none on O1-O3, O5, O8 (17 such samples) -- 9 of 43, inside
            the floor of 2 on every row.  Supposed, not measured: the hit point of a lobe bounce carries the last bits of sincos and pow,
            which differ between glibc and the device library, so whether the on-surface ray that leaves it meets its own triangle again is
            drawn anew on either side; a path that meets the glass first starts from a primary hit that is the oracle's bit for bit.
            G4's body: on the common box (half 0.19, turned -22 and 26 degrees) 4 of its 78 on-surface samples were over REL_TOL against an
            allowance of 3 -- with 0 of 2891 samples without an on-surface ray over it in that run, every mismatch of the file sat on a
            path with an on-surface ray; the first differing ray itself was not traced.  The body was made thicker and turned less
            (material_scenes.BODY) and the cap kept: 2 / 78.
  frames    "opaque" at 96x64 and 33x17: the four pipelines meet test_gpu_lights._check_image with the oracle's counts; "glass": the nine
            routes of test_gpu_lights.DEVICES give the megakernel's frame and counters, 0 channels differ.
  jitter    O7 0 / 7, G5 2 / 112, G6 3 / 117 on-surface samples over REL_TOL, 0 of 364 others (largest relative error 3.4e-14), the same
            under pool and vote; the wavefront equals the megakernel.
  picks     "one": 14 of 3600 samples over REL_TOL, "tree": 15, every one on a path with an on-surface ray; per row as under "all" but
            G1 1 / 117, G4 1 / 78 ("one") and 2 / 78 ("tree"), O4 1 / 6, O9 1 / 6; 0 of 2903 others, largest relative error 5.1e-13.
  power     each of these one-line changes, on a scratch build that was then discarded, against the same file (samples over REL_TOL of a
            row's 200, G4's 400; "collateral" rows are reached by a bounce from the row that changed):
            1. bounce_sample's lobe test reads m->kd instead of kd: test_sample_radiance (4 cases), test_opaque_frames_match_the_oracle
               (2), test_first_vertex_shaded_per_sample and test_light_picks (2) fail -- O7 48 ("opaque"),
               49 ("glass"), 43 under jitter; G5 11 (8 of them on on-surface paths), 7 under jitter; collateral O2 2, O3 1, O9 2.
            2. first_vertex_throughput takes materials[].kd instead of ps->kd: test_frames_under_a_pick fails under "one" (266 channels of
               the 96x64 "opaque" frame over IMG_TOL against an allowance of 3, the largest by a factor 3e5) and under "tree" (268); every
               other test passes.  Before that test existed the change failed nothing: with two lights and no pick the wavefront state
               is not folded, the first vertex's throughput is stored and the function is never called -- the case the file lacked.
            3. m->Ni > 1 becomes m->Ni != 1: the same tests as under 1 but test_first_vertex_shaded_per_sample, and
               test_ni_below_one_is_the_opaque_material -- O10 121 of 200; collateral O4 8, O9 9, O5 2, O6 2, O2 1, O3 1.
            4. 1 / (Ns + 1) becomes 1 / Ns guarded to 1: the same tests as under 1 -- O1 101, O3 105, O4 106, O10 102, O7 49, G3 47, G4 182
               of 400; O2 (Ns 0, where the guard gives the right exponent) 8, all collateral.
            5. refract_dir takes cosi as a double: test_sample_radiance on "glass" (2), test_first_vertex_shaded_per_sample and
               test_light_picks (2) -- of the on-surface samples G1 69 / 117, G2 26 / 130, G3 35 / 83, G4 14 / 78, G5 53 / 120, G6 60 / 126
               and 0 of the others; every "opaque" test passes.
            (1, 3, 4 and 5 were run before test_frames_under_a_pick existed and while test_callers_rays still tripped over a check of its
            own on rays with a zero direction component: those two tests are not among the figures of these four.)"""
import os

import numpy as np
import pytest

import material_scenes as MS
import test_gpu_light_pick_oracle as PO
import test_gpu_lights as TL
import test_gpu_query_oracle as QO
import test_material_scenes_cpu as TC
from test_gpu_lights import OTHER_FLIP_RATE, REL_TOL
from test_gpu_parity import ON_SURFACE_FLIP_RATE

pytestmark = pytest.mark.gpu

SEED = TC.SEED
SPP = 4
# key -> (variant, width, height, the rows swapped for their siblings)
CASES = {"opaque": ("opaque", 96, 64, ()), "opaque-ragged": ("opaque", 33, 17, ()), "glass": ("glass", 96, 64, ()),
         "opaque-O10-sibling": ("opaque", 96, 64, ("O10",))}
LENS = dict(aperture=0.0, jitter=True)
LENS_ROWS = ("O7", "G5", "G6")
N_RAYS, N_INSIDE = 257, 86

_ORACLE_CACHE = {}          # (case, what) -> the oracle's answer: computed once per module


class Case(TL.Case):
    """test_gpu_lights' case -- its knob-built devices -- on a scene of material_scenes"""

    def __init__(self, key, oracle, mcpt, directory):
        self.key = key
        self.variant, self.w, self.h, siblings = CASES[key]
        self.mcpt, self.oracle = mcpt, oracle
        name = "materials_" + key.replace("-", "_")
        self.info = MS.write(directory, name, self.w, self.h, variant=self.variant, siblings={r: True for r in siblings})
        self.osc = oracle.OracleScene(directory + name, texture_dir=directory, width=self.w, height=self.h)
        self.sc = mcpt.Scene(directory, name, width=self.w, height=self.h)
        self.nl = 2
        assert self.sc.info.num_lights == self.nl == self.osc.num_lights
        self.devs, self.dev_mode, self.weights = {}, {}, None

    def oracle_cached(self, what, fn):
        key = (self.key, what)
        if key not in _ORACLE_CACHE:
            _ORACLE_CACHE[key] = fn()
        return _ORACLE_CACHE[key]

    def plan(self):
        """test_material_scenes_cpu's plan of the scene, with the oracle's samples and their on-surface flags"""
        def run():
            pix, k, row_of = TC.sample_plan(self.osc, self.info)
            return (pix, k, row_of) + TC.oracle_samples(self.oracle, self.osc, pix, k)
        return self.oracle_cached("plan", run)


class PickCase(PO._Picking, Case):
    """the case under a light pick: the mode on the oracle and on each device as it is asked for"""

    def oracle_cached(self, what, fn):
        return Case.oracle_cached(self, (self.mode, what), fn)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in TL.KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("gpu_material_scenes")) + os.sep


@pytest.fixture(scope="module")
def cases(oracle, mcpt, scene_dir):
    """one case alive at a time (the previous one's devices go before the next one's are created); the oracle's answers outlive it"""
    made = {}

    def get(key, cls=Case):
        if (key, cls) not in made:
            for k in list(made):
                made.pop(k).close()
            made[(key, cls)] = cls(key, oracle, mcpt, scene_dir)
        return made[(key, cls)]
    yield get
    for k in list(made):
        made.pop(k).close()
    _ORACLE_CACHE.clear()


def _check_rows(what, g, o, on_surface, row_of):
    """Row by row: NaN nowhere; the samples within REL_TOL but for OTHER_FLIP_RATE of those without an on-surface ray and
    ON_SURFACE_FLIP_RATE (floor 2) of those with one.  Every row's figures are printed before any is asserted; returns the flipped."""
    assert np.isfinite(o).all() and np.isfinite(g).all(), "%s: %d samples are not finite" % (what, int((~np.isfinite(g)).any(axis=1).sum()))
    err = np.abs(g - o).max(axis=1) / np.maximum(np.abs(o).max(axis=1), 1e-12)
    flip = err > REL_TOL
    failed = []
    for i in np.unique(row_of):
        row, m = MS.ROW_NAMES[i], row_of == i
        n, on = int(m.sum()), on_surface & m
        plain, surf = int((flip & m & ~on_surface).sum()), int((flip & on).sum())
        allow_plain, allow_surf = int(n * OTHER_FLIP_RATE), max(2, int(on.sum() * ON_SURFACE_FLIP_RATE) + 1)
        unflipped = err[m & ~flip]
        print("%s %s: %d of %d ordinary samples over %g (allowance %d), %d of %d on-surface samples (rate %.4f, allowance %d), max rel of the others %.2e"
              % (what, row, plain, n - int(on.sum()), REL_TOL, allow_plain, surf, int(on.sum()), surf / max(1, int(on.sum())), allow_surf,
                 unflipped.max() if unflipped.size else 0.0))
        if plain > allow_plain or surf > allow_surf:
            failed.append((row, plain, surf))
    assert not failed, "%s: rows over their allowance (row, ordinary, on-surface): %s" % (what, failed)
    same = ~flip
    assert abs(g[same].sum() - o[same].sum()) <= 1e-9 * np.abs(o[same]).sum() and np.abs(o[same]).sum() > 0
    return flip


# ---------------------------------------------------------------------------------------------- (a) samples against the oracle
@pytest.mark.parametrize("engine", ["pool", "vote"])
@pytest.mark.parametrize("key", ["opaque", "glass"])
def test_sample_radiance(cases, key, engine):
    c = cases(key)
    pix, k, row_of, o, on_surface = c.plan()
    assert on_surface.any() == (key == "glass")
    g = c.device(engine).sample_radiance(SEED, pix, k)
    _check_rows("%s %s" % (key, engine), g, o, on_surface, row_of)


# ---------------------------------------------------------------------------------------------- (b) frames
@pytest.mark.parametrize("key", ["opaque", "opaque-ragged"])
def test_opaque_frames_match_the_oracle(cases, oracle, mcpt, key):
    c = cases(key)
    ref, ost = TL._oracle_image(c, oracle, SPP)                       # (asserts that no ray started on a surface)
    assert np.isfinite(ref).all()
    for what, which, flags in (("wavefront", "default", 0), ("no-finish", "no-finish", 0), ("vote", "vote", 0),
                               ("megakernel", "default", mcpt.RENDER_MEGAKERNEL)):
        st = mcpt.Stats()
        img = c.device(which).generateImg(SPP, seed=3, stats=st, flags=flags)
        TL._check_image(img, ref, SPP, oracle, mcpt)
        assert st.rays_shadow + st.shadow_skipped == ost.rays_shadow, what
        assert (st.rays_bounce, st.shade_calls, st.samples) == (ost.rays_bounce, ost.shade_calls, ost.samples), what


def test_glass_every_route_gives_the_megakernel_frame(cases, mcpt):
    c = cases("glass")
    st = mcpt.Stats()
    base = c.device("default").generateImg(SPP, seed=3, flags=mcpt.RENDER_MEGAKERNEL, stats=st)
    assert np.isfinite(base).all() and base.sum() > 0 and st.samples == c.w * c.h * SPP
    for which in TL.DEVICES:
        s2 = mcpt.Stats()
        img = c.device(which).generateImg(SPP, seed=3, stats=s2)
        bad = int((TL._bits(img) != TL._bits(base)).sum())
        assert bad == 0, "%s: %d channels differ from the megakernel" % (which, bad)
        assert TL._counts(s2) == TL._counts(st), (which, TL._counts(s2), TL._counts(st))


# ---------------------------------------------------------------------------------------------- (c) the first vertex per sample
def test_first_vertex_shaded_per_sample(cases, mcpt):
    c = cases("glass")
    pix, k, row_of, _, _ = c.plan()
    mine = np.isin(row_of, [MS.ROW_NAMES.index(r) for r in LENS_ROWS])
    pix, k, row_of = pix[mine], k[mine], row_of[mine]
    c.osc.set_lens(**LENS)
    try:
        o, on_surface = c.oracle_cached("lens", lambda: TC.oracle_samples(c.oracle, c.osc, pix, k))
    finally:
        c.osc.set_lens()
    pinhole = c.plan()[3][mine]
    assert TC.differing(o, pinhole).mean() > 0.5                        # the jittered rays are other rays
    for engine in ("pool", "vote"):
        dev = c.device(engine)
        dev.set_lens(**LENS)
        try:
            g = dev.sample_radiance(SEED, pix, k)
            if engine == "pool":
                wf = dev.generateImg(SPP, seed=3)
                mk = dev.generateImg(SPP, seed=3, flags=mcpt.RENDER_MEGAKERNEL)
        finally:
            dev.set_lens()
        _check_rows("glass under jitter, %s" % engine, g, o, on_surface, row_of)
    bad = int((TL._bits(wf) != TL._bits(mk)).sum())
    assert bad == 0, "%d channels differ between the wavefront and the megakernel" % bad
    assert np.isfinite(wf).all() and wf.sum() > 0


# ---------------------------------------------------------------------------------------------- (d) light picks
@pytest.mark.parametrize("mode", PO.MODES)
def test_light_picks(cases, mode):
    c = cases("glass", PickCase)
    c.set_mode(mode)
    try:
        pix, k, row_of, o, on_surface = c.plan()                         # (cached by mode: the oracle's samples under the pick)
        for engine in ("pool", "vote"):
            g = c.device(engine).sample_radiance(SEED, pix, k)
            PO._report("glass %s %s" % (mode, engine), g, o)
            _check_rows("glass %s %s" % (mode, engine), g, o, on_surface, row_of)
    finally:
        c.set_mode(None)
    assert TC.differing(o, c.plan()[3]).mean() > 0.5                    # one light per vertex: other samples than under "all"


@pytest.mark.parametrize("mode", PO.MODES)
def test_frames_under_a_pick(cases, oracle, mcpt, mode):
    """With a pick the lights share one plane of the wavefront state, and the state is folded as with one light: the first logic pass
    stores no throughput, and its readers form it again from the pixel's PrimarySurface (vertex.hpp: first_vertex_throughput) -- the
    texel's kd of O7's pixels among them, which the scenes of two lights reach under no other setting.  "opaque" against the oracle's
    frame under the same pick; on "glass" every such route gives the megakernel's frame bit for bit."""
    c = cases("opaque", PickCase)
    c.set_mode(mode)
    try:
        ref, ost = TL._oracle_image(c, oracle, SPP)
        for what, which, flags in (("wavefront", "default", 0), ("no-finish", "no-finish", 0), ("finish-lane", "finish-lane", 0),
                                   ("late-finish", "late-finish", 0), ("megakernel", "default", mcpt.RENDER_MEGAKERNEL)):
            st = mcpt.Stats()
            img = c.device(which).generateImg(SPP, seed=3, stats=st, flags=flags)
            TL._check_image(img, ref, SPP, oracle, mcpt)
            assert st.rays_shadow + st.shadow_skipped == ost.rays_shadow, what
            assert (st.rays_bounce, st.shade_calls, st.samples) == (ost.rays_bounce, ost.shade_calls, ost.samples), what
    finally:
        c.set_mode(None)
    c = cases("glass", PickCase)
    c.set_mode(mode)
    try:
        base = c.device("default").generateImg(SPP, seed=3, flags=mcpt.RENDER_MEGAKERNEL)
        for which in ("default", "no-finish", "finish-lane", "late-finish", "vote"):
            bad = int((TL._bits(c.device(which).generateImg(SPP, seed=3)) != TL._bits(base)).sum())
            assert bad == 0, "%s: %d channels differ from the megakernel" % (which, bad)
    finally:
        c.set_mode(None)


# ---------------------------------------------------------------------------------------------- (e) the caller's rays
def _query_rays(osc, info):
    """N_RAYS rays: N_INSIDE start inside the bodies of G1-G6 (in turn), the others anywhere in the room; every seventh direction is
    parallel to an axis, every seventh lies in a coordinate plane"""
    rng = np.random.default_rng(9)
    x0, x1, y0, y1, z0, z1 = MS.ROOM
    rays, inside_row = np.zeros((N_RAYS, 6)), np.full(N_RAYS, -1)
    for i in range(N_RAYS):
        d = rng.normal(size=3)
        if i % 7 == 3:
            d = np.zeros(3)
            d[rng.integers(3)] = rng.choice([-1.0, 1.0])
        elif i % 7 == 5:
            d[rng.integers(3)] = 0.0
        d /= np.linalg.norm(d)
        if i < N_INSIDE:
            row = MS.GLASS_ROWS[i % len(MS.GLASS_ROWS)]
            off = rng.normal(size=3)
            o = MS.centre(row) + off / np.linalg.norm(off) * MS.inner_radius(row) * rng.random() ** (1.0 / 3.0)
            inside_row[i] = MS.ROW_NAMES.index(row)
        else:
            o = np.array([x0, y0, z0]) + 0.05 + (np.array([x1 - x0, y1 - y0, z1 - z0]) - 0.1) * rng.random(3)
        rays[i] = np.concatenate([o, d])
    return rays, inside_row


def test_callers_rays(cases, mcpt):
    c = cases("glass")
    rays, inside_row = _query_rays(c.osc, c.info)
    face, _, _, pn = c.osc.trace_closest(rays)
    inside = inside_row >= 0
    axis = (rays[:, 3:] == 0.0).any(axis=1)
    # (the reference's slab test divides by the direction's components: with a zero among them it meets 0 / 0, and such a ray may find
    # nothing, in the oracle and in the library alike -- the hits are compared below)
    for i in np.flatnonzero(inside & ~axis):                           # the first hit is the body's own face, met from inside
        first, n = c.info["rows"][MS.ROW_NAMES[inside_row[i]]]
        assert first <= face[i] < first + n and np.dot(rays[i, 3:], pn[i]) > 0, i
    assert inside.sum() == N_INSIDE and axis.sum() >= 2 * (N_RAYS // 7) and (inside & axis).sum() >= 2 * (N_INSIDE // 7)
    assert (face[axis] >= 0).any()
    ids = np.random.default_rng(10).integers(0, 2 ** 31 - 1, size=N_RAYS).astype(np.int32)
    for kk in (0, 41):
        x, hit, on = c.oracle_cached(("rays", kk), lambda: c.osc.ray_radiance(SEED, rays, kk, ids=ids))
        assert hit[~axis].all() and np.isfinite(x).all() and on[inside].sum() >= N_INSIDE // 4
        for which, flags in (("pool", 0), ("vote", 0), ("pool", mcpt.RENDER_MEGAKERNEL)):
            mean, err, hits = c.device(which).radiance(rays, 1, SEED, ids=ids, sample_base=kk, flags=flags)
            assert not err.any()
            QO._check("glass, the caller's rays, k %d, %s%s" % (kk, which, ", megakernel" if flags else ""), "rays", mean, hits, x, hit, on)


# ---------------------------------------------------------------------------------------------- (f) Ni 0.8 is Ni 1
def test_ni_below_one_is_the_opaque_material(cases, mcpt):
    c = cases("opaque")
    pix, k, row_of, _, _ = c.plan()
    mine = row_of == MS.ROW_NAMES.index("O10")
    g = c.device("default").sample_radiance(SEED, pix[mine], k[mine])
    img = c.device("default").generateImg(SPP, seed=3)
    s = cases("opaque-O10-sibling")
    assert s.sc.material([s.sc.material(j)[0] for j in range(s.sc.info.num_materials)].index("O10"))[1][7] == 1.0
    g2 = s.device("default").sample_radiance(SEED, pix[mine], k[mine])
    img2 = s.device("default").generateImg(SPP, seed=3)
    assert np.array_equal(TL._bits(g), TL._bits(g2)) and np.array_equal(TL._bits(img), TL._bits(img2))
    assert (g > 0).any() and np.isfinite(img).all()
