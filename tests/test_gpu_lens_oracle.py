"""-m gpu: frames under a camera lens (mcpt_device_set_lens) against an oracle that has the lens (oracle/mcpt_oracle.c: orc_scene_set_lens,
restated from the "camera lens" paragraph of include/mcpt.h and pinned by tests/test_lens_oracle_cpu.py), sample by sample and frame by
frame.

Under a lens every route takes its ray from one camera_ray (csrc/camera.hpp), shades the first vertex through one shade_path / vertex.hpp,
answers a missed sample by one env_camera_miss and folds by one k_fold_lens, so the routes' agreement with each other (test_gpu_lens.py)
cannot see a mistake they share, and the MCPT_LENS_PER_SAMPLE seam proves the per-sample route only where all of a pixel's rays coincide --
where a first vertex shaded with the pixel's direction, hit, material or texel instead of the sample's, a missed sample that takes Le of the
pixel's direction, or a fold that skips a pixel because its pinhole ray missed, are all invisible.  Here the oracle traces a camera ray per
sample, and the comparison keeps test_gpu_env_oracle.py's helpers, bars and flip allowances (test_gpu_parity.py's); there is no tolerance
of this file's own.

Lenses: jitter (the flag only), thin (aperture 0.05, F = 0), thin-jitter-far (aperture 0.3, F = 2.5, jitter).
Scenes at 96x64: cornell-box (also at 33x17: a partial wave and a partial tile), glassroom (view-dependent first vertices: refraction, an
Ns-60 lobe, a textured quad), veach-mis (five lights, glossy plates), a light_scenes room of 9 lights under MCPT_LIGHTS_TREE (the pick draws at
the sample's own first vertex), env_scenes.open_scene(1 light) under the "map" sky (silhouette pixels where some samples hit and some miss).

(a) dev.camera_rays against the oracle's: bit for bit under jitter, within test_gpu_lens.py's _ulps <= 4 under the thin lenses;
(b) per-sample radiance of 3000 random (pix, k < 64) under the pool and vote engines: NaN exactly where the oracle has it, the finite
    samples at REL_TOL under the flip allowance;
(c) SPP-4 frames of the wavefront (default finishing pass, none, the lane form) and of the megakernel: the image, its 8-bit output,
    rays_primary == W*H*4 and the work counts (mcpt's Stats carries no count of camera misses to hold against the oracle's camera_miss; the
    oracle's is held to its own traced rays in test_lens_oracle_cpu.py, and a pixel all of whose samples miss must be the oracle's fold of
    Le bit for bit here);
(d) a progressive handle, passes 1 + 3, on the open scene: image() under thin-jitter-far against the oracle's frame; under jitter, where the
    rays are the same bits, the handle's "hit" pixels (mcpt_noise) are those where SOME sample's camera ray hit -- the oracle's closest hits
    of the oracle's camera rays;
(e) the sample AOVs at G = 4 under jitter and thin against a numpy fold (guide_ref.fold, the header's k order in fp64) of the oracle's
    closest hits of the oracle's camera rays, a hit classified by its material's light index;
(f) the comparison's power: the oracle made wrong on purpose (set_lens(wrong=1): the first vertex shaded with the pixel's pinhole wo, on
    glassroom; wrong=2: a missed sample takes Le of the pixel's pinhole direction, on the open scene) fails the same check (b).

Under the thin lenses the device's and the oracle's rays differ by a few ulps of the vector's scale (sin / cos); REL_TOL is nine decades above
that, and a different first triangle needs a ray within ~1e-15 of an edge.

Measured on an MI355X on 2026-10-18 (the figures each test prints before it asserts):
  rays      bit for bit under jitter in every case; under the thin lenses at most 4.00 ulps (veach-mis, thin, k < 2^20), 2.00 elsewhere.
  samples   without on-surface paths (cornell-box at both sizes, veach-mis, the room of 9 lights under the tree): 0 of 3000 over REL_TOL under
            every lens and both engines, largest relative error 7.1e-13.  With them, samples over REL_TOL / allowance, the same under both
            engines: glassroom 2 / 5 (jitter), 0 / 5 (thin), 4 / 5 (thin-jitter-far); open scene 1 / 7, 0 / 7, 0 / 7 -- test_gpu_parity.py's
            refraction flips; where none flipped the largest relative error is 4.0e-13.  No sample failed under a thin lens only: the unmeasured point above held,
            no ray of 3 x 5 x 3000 samples and 3 x 6 frames fell on another triangle than the oracle's.
  frames    the four pipelines give the same figures in every case.  Channels over IMG_TOL of 18432: 0 on the scenes without on-surface
            paths; glassroom 33 / 63 / 60 (jitter / thin / thin-jitter-far), open scene 18 / 15 / 24 (budgets 105 and 150 upward);
            rays_primary = samples = 24576 everywhere; bounce rays and shade calls equal the oracle's on the scenes without on-surface
            paths, within 5 of 20900 and 7 of 35000 on glassroom.
  handle    passes 1 + 3 under thin-jitter-far: 24 channels over IMG_TOL, the one-shot frame's; under jitter 3700 hit pixels on both sides
            (the pixel's pinhole ray hits on 3601), sum_se2 within 3.1e-16 of the sum over the oracle's mask (bound 1.2e-12).
  AOVs      counts equal in all six cases; under jitter depth, albedo and normal bit for bit, and the first-hit normals too; under thin
            depth within 3.8e-16, normal within 2.0e-14, albedo bit for bit.  Before the AOV kernels took the normal from the closest
            hit (hit_normal) they took shading's blend, which multiplies by a reciprocal of |n|^2 where the closest hit divides: 296 of
            4130 surface pixels of cornell-box and 2211 of 3673 of the open scene then differed from the oracle's fold in the last bit.
  power     wrong = 1 on glassroom: 67 of 3000 samples over REL_TOL against an allowance of 5 (3 against the right oracle); wrong = 2 on the
            open scene: 883 against 7 (0 against the right oracle).  Both fail the check, as they must."""
import os

import numpy as np
import pytest

import env_scenes
import guide_ref as GR
import light_scenes
import light_tree_ref as LT
import test_gpu_env_oracle as TE
from conftest import SCENES, extra_scene_dir
from test_gpu_lens import _ulps
from test_lens_oracle_cpu import LENSES, POWER, flip_allowance

pytestmark = pytest.mark.gpu

SPP, SEED = TE.SPP, TE.SEED
G = 4
# key -> (kind, scene name or None, lights, width, height, sky, light pick)
CASES = {"cornell-box": ("shipped", "cornell-box", 1, 96, 64, None, None),
         "cornell-box-ragged": ("shipped", "cornell-box", 1, 33, 17, None, None),
         "glassroom": ("shipped", "glassroom", 2, 96, 64, None, None),
         "veach-mis": ("shipped", "veach-mis", 5, 96, 64, None, None),
         "nl9-tree": ("lights", None, 9, 96, 64, None, "tree"),
         "open-sky": ("open", None, 1, 96, 64, "map", None)}

_ORACLE_CACHE = {}          # (case, lens, what) -> the oracle's answer: computed once per module


class Case(TE.Case):
    """test_gpu_env_oracle's case -- its knob-built devices, its sky -- with a lens both sides are under and, for the room, the tree"""

    def __init__(self, key, oracle, mcpt, directory):
        self.key = key
        self.kind, name, self.nl, self.w, self.h, sky, self.pick = CASES[key]
        self.mcpt = mcpt
        if self.kind == "open":
            name, base = "lens_open_nl%d" % self.nl, directory
            env_scenes.open_scene(directory, name, self.nl, self.w, self.h)
        elif self.kind == "lights":
            name, base = "lens_lights_nl%d" % self.nl, directory
            light_scenes.write(directory, name, self.nl, self.w, self.h)
        else:
            base = extra_scene_dir() if name == "glassroom" else SCENES
        self.osc = oracle.OracleScene(base + name, texture_dir=base, width=self.w, height=self.h)
        self.sc = mcpt.Scene(base, name, width=self.w, height=self.h)
        assert self.sc.info.num_lights == self.nl == self.osc.num_lights
        self.devs, self.dev_sky, self.dev_lens, self.sky, self.lens = {}, {}, {}, None, None
        if sky:
            self.set_sky(sky)
        if self.pick:
            self.osc.set_light_pick(2, tree_ref=LT.TreeRef.of_scene(self.sc))

    def set_lens(self, lens, wrong=0):
        """lens: a key of LENSES or a dict of set_lens's arguments -- on the oracle now, on each device when it is next asked for"""
        self.lens = lens
        self.osc.set_lens(wrong=wrong, **self.lens_value())

    def lens_value(self):
        return LENSES[self.lens] if isinstance(self.lens, str) else dict(self.lens)

    def device(self, which):
        fresh = which not in self.devs
        dev = super().device(which)
        if fresh and self.pick:
            dev.set_light_sampling(self.pick)
        if self.dev_lens.get(which) != self.lens:
            dev.set_lens(**self.lens_value())
            self.dev_lens[which] = self.lens
        want = dict(dict(aperture=0.0, focus_distance=0.0, jitter=False, per_sample=False), **self.lens_value())
        assert dev.lens() == want and dev.light_sampling()[0] == (self.pick or "all")
        return dev

    def oracle_cached(self, what, fn):
        key = (self.key, str(self.lens), what)
        if key not in _ORACLE_CACHE:
            _ORACLE_CACHE[key] = fn()
        return _ORACLE_CACHE[key]


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in TE.KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("gpu_lens_oracle_scenes")) + os.sep


@pytest.fixture(scope="module")
def cases(oracle, mcpt, scene_dir):
    """one case alive at a time (the previous one's devices go before the next one's are created); the oracle's answers outlive it"""
    made = {}

    def get(key):
        if key not in made:
            for k in list(made):
                made.pop(k).close()
            made[key] = Case(key, oracle, mcpt, scene_dir)
        return made[key]
    yield get
    for k in list(made):
        made.pop(k).close()
    _ORACLE_CACHE.clear()


def _report(what, g, o, on_surface):
    """the figures of a comparison, printed before it is asserted: the largest relative error, the samples over REL_TOL and the allowance"""
    fin = np.isfinite(o).all(axis=1) & np.isfinite(g).all(axis=1)
    err = np.abs(g[fin] - o[fin]).max(axis=1) / np.maximum(np.abs(o[fin]).max(axis=1), 1e-12)
    print("%s: max rel %.3e, %d of %d samples over %g (allowance %d, %d on-surface paths), NaN samples %d (oracle) %d (device)"
          % (what, err.max(), int((err > TE.REL_TOL).sum()), g.shape[0], TE.REL_TOL, flip_allowance(on_surface), int(on_surface.sum()),
             int(np.isnan(o).any(axis=1).sum()), int(np.isnan(g).any(axis=1).sum())))


def _oracle_frame(c, oracle):
    """orc_render at SPP, its statistics, the oracle's camera rays of every sample of the frame and the mask of the samples that miss"""
    def run():
        ost = oracle.Stats()
        img = c.osc.render(SPP, seed=3, stats=ost)
        pix = np.repeat(np.arange(c.w * c.h, dtype=np.int32), SPP)
        k = np.tile(np.arange(SPP, dtype=np.int32), c.w * c.h)
        miss = (c.osc.trace_closest(c.osc.camera_rays(3, pix, k))[0] < 0).reshape(c.h, c.w, SPP)
        return img, ost, miss
    return c.oracle_cached("frame", run)


# ---------------------------------------------------------------------------------------------- (a) and (b): rays and samples
@pytest.mark.parametrize("lens", sorted(LENSES))
@pytest.mark.parametrize("key", list(CASES))
def test_rays_and_sample_radiance(cases, oracle, key, lens):
    c = cases(key)
    c.set_lens(lens)
    pix, k, o, on_surface, kinds = TE._oracle_samples(c, oracle)
    rng = np.random.default_rng(6)
    far_pix = rng.integers(0, c.w * c.h, size=2000).astype(np.int32)
    far_k = rng.integers(0, 1 << 20, size=2000).astype(np.int32)
    dev = c.device("pool")
    for p, kk, seed in ((pix, k, SEED), (far_pix, far_k, 0x0123456789ABCDEF)):
        got, want = dev.camera_rays(seed, p, kk), c.osc.camera_rays(seed, p, kk)
        if lens == "jitter":
            assert np.array_equal(TE._bits(got), TE._bits(want)), "%d rays differ" % int((TE._bits(got) != TE._bits(want)).any(axis=1).sum())
        else:
            u = _ulps(got, want).max()
            print("%s %s: the device's rays within %.2f ulps of the oracle's" % (key, lens, u))
            assert u <= 4, u
    assert (o > 0).any(axis=1).mean() > 0.1
    if c.sky:
        assert kinds["camera_miss"] > 100                       # missed samples that bring Le are among the set
    for engine in ("pool", "vote"):
        g = c.device(engine).sample_radiance(SEED, pix, k)
        _report("%s %s %s" % (key, lens, engine), g, o, on_surface)
        TE._check_samples(g, o, on_surface)


# ---------------------------------------------------------------------------------------------- (c) frames
def _check_lens_frame(what, img, st, c, oracle, mcpt, on_surface):
    ref, ost, miss = _oracle_frame(c, oracle)
    fin = np.isfinite(ref)
    rel = np.abs(img[fin] - ref[fin]) / np.maximum(np.abs(ref[fin]), 1e-6)
    print("%s: max rel %.3e, %d of %d channels over %g; primary rays %d, samples %d, bounce %d, shade calls %d (oracle %d %d %d %d)"
          % (what, rel.max(), int((rel > TE.IMG_TOL).sum()), img.size, TE.IMG_TOL, st.rays_primary, st.samples, st.rays_bounce, st.shade_calls,
             ost.rays_primary, ost.samples, ost.rays_bounce, ost.shade_calls))
    # a pixel all of whose samples miss: 0, or the oracle's fold of Le, bit for bit (TE._check_frame's `miss`)
    TE._check_frame(what, img, st, ref, ost, miss.all(axis=2), TE._flip_rate(on_surface), oracle, mcpt)
    assert st.rays_primary == ost.rays_primary == c.w * c.h * SPP and st.samples == c.w * c.h * SPP, what
    return miss


@pytest.mark.parametrize("lens", sorted(LENSES))
@pytest.mark.parametrize("key", list(CASES))
def test_frames(cases, oracle, mcpt, key, lens):
    c = cases(key)
    c.set_lens(lens)
    on_surface = TE._oracle_samples(c, oracle)[3]
    for what, which, flags in TE.PIPELINES:
        st = mcpt.Stats()
        img = c.device(which).generateImg(SPP, seed=3, stats=st, flags=getattr(mcpt, flags) if isinstance(flags, str) else flags)
        miss = _check_lens_frame("%s %s, %s" % (key, lens, what), img, st, c, oracle, mcpt, on_surface)
    ost = _oracle_frame(c, oracle)[1]
    if c.sky:                                                    # silhouette pixels: some samples hit, some miss
        assert (miss.any(axis=2) & ~miss.all(axis=2)).sum() >= 10 and ost.camera_miss == int(miss.sum())
    assert ost.rays_shadow > 0 and ost.rays_bounce > 0


# ---------------------------------------------------------------------------------------------- (d) a progressive handle
def test_progressive_passes_against_the_oracle(cases, oracle, mcpt):
    c = cases("open-sky")
    c.set_lens("thin-jitter-far")
    on_surface = TE._oracle_samples(c, oracle)[3]
    pr = c.device("pool").progressive(SPP, seed=3)
    try:
        total = mcpt.Stats()
        for n in (1, 3):
            st = mcpt.Stats()
            pr.step(n, stats=st)
            for f in ("rays_primary", "rays_shadow", "shadow_skipped", "rays_bounce", "shade_calls", "samples"):
                setattr(total, f, getattr(total, f) + getattr(st, f))
        assert pr.done == SPP
        _check_lens_frame("open-sky thin-jitter-far, progressive 1 + 3", pr.image(), total, c, oracle, mcpt, on_surface)
    finally:
        pr.close()


def test_progressive_hit_pixels_are_those_some_sample_hit(cases, oracle, mcpt):
    """under jitter the device's rays are the oracle's bit for bit, so the pixels the handle counts as hit (mcpt_noise: pixels, and the sums
    taken over them) are exactly those where some sample's camera ray hit in the oracle"""
    c = cases("open-sky")
    c.set_lens("jitter")
    miss = _oracle_frame(c, oracle)[2]
    hit = ~miss.all(axis=2)
    pinhole_hit = (c.osc.trace_closest(c.osc.primary_rays())[0] >= 0).reshape(c.h, c.w)
    assert (hit & ~pinhole_hit).sum() > 5 and (miss.any(axis=2) & hit).sum() > 20        # the two meanings differ on this frame
    pr = c.device("pool").progressive(SPP, seed=3)
    try:
        pr.step(1)
        pr.step(3)
        noise, err, img = pr.noise(), pr.stderr(), pr.image()
    finally:
        pr.close()
    se2 = float((err[hit] ** 2).sum())
    # a sum of n positive terms, each the square of a rounded root: within (n + 2) half-ulps of any other order of summation
    bound = (3 * int(hit.sum()) + 2) * 2.0 ** -53
    print("hit pixels: device %d, oracle %d (pinhole %d); sum_se2 device %.17g, over the oracle's mask %.17g (rel %.2e, bound %.2e)"
          % (noise.pixels, int(hit.sum()), int(pinhole_hit.sum()), noise.sum_se2, se2, abs(noise.sum_se2 - se2) / se2, bound))
    assert noise.pixels == int(hit.sum())
    assert abs(noise.sum_se2 - se2) <= bound * se2
    pin_se2 = float((err[pinhole_hit] ** 2).sum())        # the other meaning -- the pixel's pinhole ray hit -- would not pass
    assert abs(noise.sum_se2 - pin_se2) > bound * pin_se2
    assert np.isfinite(img).all()


# ---------------------------------------------------------------------------------------------- (e) sample AOVs
def _aov_reference(c):
    """guide_ref.fold of the oracle's closest hits of the oracle's own camera rays of samples 0 .. G-1 of every pixel, a hit classified by
    its material's light index; plain: the pixels none of whose surface samples is textured (the albedo there is the material's Kd);
    last, the normals of the closest hits of the pixels' unjittered pinhole rays, what the first-hit AOVs keep under a lens (0 off a surface)"""
    n = c.w * c.h
    pix = np.tile(np.arange(n, dtype=np.int32), G)
    k = np.repeat(np.arange(G, dtype=np.int32), n)
    face, t, _, pn = c.osc.trace_closest(c.osc.camera_rays(3, pix, k))
    recs = [c.osc.material(m) for m in range(c.osc.num_materials)]
    kd = np.array([r[1][:3] for r in recs])
    textured = np.array([r[2][0] != 0 for r in recs])
    emitter = np.array([r[2][3] >= 0 for r in recs])
    mat = c.osc.faces()[1][np.maximum(face, 0)]
    kind = np.where(face < 0, GR.MISS, np.where(emitter[mat], GR.EMITTER, GR.SURFACE)).reshape(G, n)
    counts, depth, normal, albedo = GR.fold(kind, t.reshape(G, n), kd[mat].reshape(G, n, 3), GR.unit(pn).reshape(G, n, 3))
    plain = ~((kind == GR.SURFACE) & textured[mat].reshape(G, n)).any(axis=0)
    pface, _, _, ppn = c.osc.trace_closest(c.osc.primary_rays())
    first = np.where(((pface >= 0) & ~emitter[c.osc.faces()[1][np.maximum(pface, 0)]])[:, None], ppn, 0.0)
    return counts, depth, normal, albedo, plain, first


AOV_SCENES = ["cornell-box", "glassroom", "open-sky"]


def _sample_aovs(c, lens):
    """the device's sample AOVs at G under `lens` and its first-hit normals, flattened per pixel, and the oracle's fold"""
    c.set_lens(lens)
    ref = c.oracle_cached("aovs", lambda: _aov_reference(c))
    pr = c.device("pool").progressive(SPP, seed=3)
    try:
        s = pr.sample_aovs(G)
        first = pr.aovs()["normal"].reshape(-1, 3)
    finally:
        pr.close()
    return (s["counts"].reshape(-1, 3), s["depth"].reshape(-1), s["normal"].reshape(-1, 3), s["albedo"].reshape(-1, 3), first), ref


def _normal_figures(got_n, normal, some):
    """pixels whose normal differs in any bit (-0.0 taken as +0.0: a sum that starts at +0.0), the largest difference over the length"""
    differ = int((TE._bits(got_n + 0.0) != TE._bits(normal + 0.0)).any(axis=1).sum())
    return differ, float((np.linalg.norm(got_n - normal, axis=1)[some] / np.linalg.norm(normal, axis=1)[some]).max())


@pytest.mark.parametrize("lens", ["jitter", "thin"])
@pytest.mark.parametrize("key", AOV_SCENES)
def test_sample_aovs(cases, key, lens):
    """counts equal; under jitter (the same rays, bit for bit) depth, albedo and normal bit for bit, under thin the sums within 1e-12
    relative (the rays differ by ulps).  The albedo is compared where no surface sample of the pixel is textured: there it is the material's
    Kd (the texel's path is held by the per-sample radiance on glassroom).  The normal is the closest hit's (csrc/dev_common.hpp:
    hit_normal, the pn of mcpt_trace_closest), in the first-hit AOVs too, which keep the pixel's unjittered pinhole ray under a lens."""
    (got_c, got_d, got_n, got_a, got_first), (counts, depth, normal, albedo, plain, first) = _sample_aovs(cases(key), lens)
    some = counts[:, 0] > 0

    def rel(a, b):
        return float((np.abs(a - b) / np.maximum(np.abs(b), 1e-300))[np.abs(b) > 0].max())
    print("%s %s sample AOVs: %d pixels' counts differ; bits differ on depth %d, normal %d, albedo (untextured) %d of %d surface pixels; "
          "max rel depth %.2e, normal %.2e (of its length), albedo %.2e; first-hit normals differ on %d pixels"
          % (key, lens, int((got_c != counts).any(axis=1).sum()), int((TE._bits(got_d) != TE._bits(depth)).sum()), _normal_figures(got_n, normal, some)[0],
             int((TE._bits(got_a[plain]) != TE._bits(albedo[plain])).any(axis=1).sum()), int(some.sum()), rel(got_d, depth),
             _normal_figures(got_n, normal, some)[1], rel(got_a[plain], albedo[plain]), int((TE._bits(got_first + 0.0) != TE._bits(first + 0.0)).any(axis=1).sum())))
    assert np.array_equal(got_c, counts), "%d pixels' counts differ" % int((got_c != counts).any(axis=1).sum())
    assert np.all(counts.sum(axis=1) == G) and some.sum() > 1000 and (plain & some).sum() > 1000
    if key == "open-sky":
        assert ((counts[:, 2] > 0) & (counts[:, 2] < G)).sum() >= 10                       # silhouettes: the lens mixes kinds within a pixel
    assert np.all(got_d[~some] == 0.0) and np.all(got_n[~some] == 0.0) and np.all(got_a[~some] == 0.0)
    if lens == "jitter":
        assert np.array_equal(TE._bits(got_d), TE._bits(depth))
        assert np.array_equal(TE._bits(got_a[plain]), TE._bits(albedo[plain]))
        assert np.array_equal(TE._bits(got_n + 0.0), TE._bits(normal + 0.0))                # (-0.0 taken as +0.0: a sum that starts at +0.0)
    else:
        assert np.all(np.abs(got_d - depth) <= 1e-12 * np.abs(depth))
        assert np.all(np.abs(got_a[plain] - albedo[plain]) <= 1e-12 * np.abs(albedo[plain]))
        assert np.all(np.linalg.norm(got_n - normal, axis=1) <= 1e-12 * np.linalg.norm(normal, axis=1))
    assert np.array_equal(TE._bits(got_first + 0.0), TE._bits(first + 0.0)) and np.abs(first).sum() > 0


# ---------------------------------------------------------------------------------------------- (f) the comparison's power
@pytest.mark.parametrize("wrong", [1, 2])
def test_a_wrong_oracle_fails_the_sample_check(cases, oracle, wrong):
    """Nothing wrong goes into the library: the ORACLE is made wrong (oracle_lib.set_lens(wrong=...)) in the two ways the routes' agreement
    cannot see, and the device's samples, which pass against the right oracle, fail the same check against each.  The scenes, lenses and
    sample set are those of test_lens_oracle_cpu.py, which counts the samples each wrong mode moves against the flip allowance."""
    which, lens = POWER[wrong]
    c = cases(which)
    c.set_lens(lens)
    pix, k, o, on_surface, _ = TE._oracle_samples(c, oracle)
    g = c.device("pool").sample_radiance(SEED, pix, k)
    _report("%s %s" % (which, lens), g, o, on_surface)
    TE._check_samples(g, o, on_surface)
    try:
        c.osc.set_lens(wrong=wrong, **lens)
        bad = np.array([c.osc.sample_radiance(SEED, int(p // c.w), int(p % c.w), int(kk)) for p, kk in zip(pix, k)])
        _report("%s against the oracle with wrong = %d" % (which, wrong), g, bad, on_surface)
        with pytest.raises(AssertionError):
            TE._check_samples(g, bad, on_surface)
    finally:
        c.set_lens(lens)
