"""-m gpu: MCPT_LIGHTS_ONE -- one shadow ray per vertex from a weighted light pick (include/mcpt.h: light sampling).

(a) the device's pick against the numpy restatement (tests/light_pick_ref.py), light index and probability bit for bit;
(b) the one-hot identity: on a diffuse-only copy of the light scenes, sum over l of sample_radiance("one", weights = e_l) is
    sample_radiance("all") within 1e-12 relative per channel -- the paths are the same in both modes, 1 / p = 1 exactly and every term is
    non-negative, so the sides differ in summation order only, (nl + depth) * 2^-53: the bar is derived, with two orders of slack;
(c) the cases in which the mode changes nothing give the "all" frame and statistics bit for bit;
(d) every route of test_gpu_lights.py gives the same "one" frame bit for bit and the same counts; bounce rays, shade calls and samples
    are the "all" frame's (the paths are the same), shadow rays + skipped are the "all" frame's divided by the light count, exactly;
(e) "one" - "all" per sample has block means consistent with 0 under pins_common.assert_standard_normal and its bars; a restatement
    with one light's factor halved fails the same test (made in numpy alone: nothing wrong goes into the library);
(f) progressive, adaptive, denoised, lens, environment, updated, motion, MultiDevice and checkpointed frames pick the setting up."""
import os

import numpy as np
import pytest

import anim_scenes as A
import light_pick_ref as LP
import light_scenes
import motion_ref as MR
import pins_common
import test_gpu_lights as TL
from conftest import SCENES

pytestmark = pytest.mark.gpu

W, H = 96, 64
bits = TL._bits


def same(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in TL.KNOBS:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("gpu_pick_scenes")) + os.sep


def write_scene(directory, nl, diffuse_only=False):
    name = "pick%d%s" % (nl, "d" if diffuse_only else "")
    if not os.path.exists(directory + name + ".obj"):
        light_scenes.write(directory, name, nl, W, H)
        if diffuse_only:                      # the Glossy material's Ks set to 0: every bounce of the scene is a diffuse one
            lines = open(directory + name + ".mtl").read().splitlines()
            at = lines.index("newmtl Glossy")
            ks = next(i for i in range(at, len(lines)) if lines[i].startswith("Ks "))
            lines[ks] = "Ks 0.0 0.0 0.0"
            open(directory + name + ".mtl", "w").write("\n".join(lines) + "\n")
    return name


class Room:
    """a light scene and its devices, one per route of test_gpu_lights.py (created while the route's knobs are in the environment)"""
    def __init__(self, mcpt, directory, nl, diffuse_only=False):
        self.mcpt, self.nl, self.dir = mcpt, nl, directory
        self.name = write_scene(directory, nl, diffuse_only)
        self.sc = mcpt.Scene(directory, self.name, width=W, height=H)
        assert self.sc.info.num_lights == nl
        self.devs = {}

    def device(self, which="default"):
        if which not in self.devs:
            saved = {k: os.environ.pop(k, None) for k in TL.KNOBS}
            try:
                os.environ.update(TL.DEVICES[which])
                self.devs[which] = self.mcpt.Device(self.sc, 0)
            finally:
                for k, v in saved.items():
                    os.environ.pop(k, None)
                    if v is not None:
                        os.environ[k] = v
        return self.devs[which]

    def close(self):
        for d in self.devs.values():
            d.close()
        self.sc.close()


@pytest.fixture(scope="module")
def rooms(mcpt, scene_dir):
    made = {}

    def get(nl, diffuse_only=False):
        key = (nl, diffuse_only)
        if key not in made:
            for k in list(made):              # one room alive at a time
                made.pop(k).close()
            made[key] = Room(mcpt, scene_dir, nl, diffuse_only)
        return made[key]
    yield get
    for k in list(made):
        made.pop(k).close()


def triples(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, W * H, size=n).astype(np.int32), rng.integers(0, 4096, size=n).astype(np.int32)


# ---------------------------------------------------------------------------------------------- (a) the pick
@pytest.mark.parametrize("weights", ["default", "caller"])
@pytest.mark.parametrize("nl", [3, 10, 40])
def test_pick_matches_the_restatement(rooms, nl, weights):
    r = rooms(nl)
    dev = r.device()
    w = None
    if weights == "caller":
        w = np.random.default_rng(nl).uniform(0.05, 3.0, size=nl)
        w[[0, nl // 2, nl - 1] if nl > 3 else [1]] = 0.0             # zeros at the ends and in the middle
    dev.set_light_sampling("one", w)
    try:
        ref = LP.PickRef.of_scene(r.sc, w)
        mode, pdf = dev.light_sampling()
        assert mode == "one" and same(pdf, ref.pdf)
        seen = np.zeros(nl, dtype=np.int64)
        for depth in (0, 1, 2, 5, 17, 63):
            pix, k = triples(700, 100 * nl + depth)
            light, p = dev.light_pick(1234567 + depth, pix, k, depth)
            want_l, want_p = ref.pick(1234567 + depth, pix, k, depth)
            assert np.array_equal(light, want_l), "depth %d: %d picks differ" % (depth, int((light != want_l).sum()))
            assert same(p, want_p)
            seen += np.bincount(light, minlength=nl)
        assert (seen[ref.w == 0] == 0).all()                     # a light of weight 0 never appears
        assert (seen[ref.pdf > 0.02] > 0).all()
        with pytest.raises(r.mcpt.McptError):
            dev.light_pick(1, [0], [0], 64)
    finally:
        dev.set_light_sampling(None)
    with pytest.raises(r.mcpt.McptError):
        dev.light_pick(1, [0], [0], 0)                           # the device does not pick
    for bad in ([1.0] * (nl + 1), [0.0] * nl, [-1.0] + [1.0] * (nl - 1), [float("nan")] + [1.0] * (nl - 1)):
        with pytest.raises(r.mcpt.McptError):
            dev.set_light_sampling("one", bad)
        assert dev.light_sampling()[0] == "all"


# ---------------------------------------------------------------------------------------------- (b) the one-hot identity
def _non_emitter_samples(room, n, seed):
    """(pix, k) of n camera samples whose primary hit is a surface that is not an emitter (the pinhole: the hit depends on the pixel)"""
    dev = room.device()
    pix, k = triples(n, seed)
    face = dev.ray_intersect(dev.camera_rays(0, pix, k))[0]
    mat = room.sc.faces()[1]
    lights = [room.sc.light(i)[2] for i in range(room.nl)]
    keep = (face >= 0) & ~np.isin(mat[np.maximum(face, 0)], lights)
    assert keep.sum() > 0.8 * n
    return pix[keep], k[keep]


def _per_light(dev, nl, seed, pix, k):
    out = np.zeros((nl, pix.shape[0], 3))
    for l in range(nl):
        e = np.zeros(nl)
        e[l] = 1.0
        dev.set_light_sampling("one", e)
        out[l] = dev.sample_radiance(seed, pix, k)
    dev.set_light_sampling(None)
    return out


@pytest.mark.parametrize("nl", [3, 10])
def test_one_hot_weights_add_up_to_all(rooms, oracle, nl):
    r = rooms(nl, diffuse_only=True)
    # on the CPU first: no material can bounce other than diffusely (an emitter is then only ever reached by a diffuse bounce, which
    # adds nothing: every term of a sample is a light sample's), and the oracle finds the chosen samples finite
    for m in range(r.sc.info.num_materials):
        rec = r.sc.material(m)[1]
        assert not np.any(rec[3:6]) and rec[7] == 1.0, "material %d is not diffuse-only" % m
    pix, k = _non_emitter_samples(r, 1500, 7 + nl)
    osc = oracle.OracleScene(r.dir + r.name, texture_dir=r.dir, width=W, height=H)
    o = np.array([osc.sample_radiance(41, int(p // W), int(p % W), int(kk)) for p, kk in zip(pix[:300], k[:300])])
    osc.close()
    assert np.isfinite(o).all() and (o >= 0).all() and o.sum() > 0
    dev = r.device()
    ref = dev.sample_radiance(41, pix, k)
    assert np.allclose(ref[:300], o, rtol=TL.REL_TOL, atol=0)       # the "all" side is the oracle-pinned one
    parts = _per_light(dev, nl, 41, pix, k)
    assert (parts >= 0).all() and np.isfinite(parts).all()
    total = parts.sum(axis=0)
    rel = np.abs(total - ref) / np.maximum(np.abs(ref), 1e-300)
    rel[ref == 0] = np.where(total[ref == 0] == 0, 0.0, np.inf)
    print("one-hot identity, %d lights: max relative difference %.3e over %d samples" % (nl, rel.max(), pix.shape[0]))
    assert rel.max() <= 1e-12
    assert (ref > 0).any(axis=1).mean() > 0.5


# ---------------------------------------------------------------------------------------------- (c) neutral cases
def test_one_light_scene_and_cleared_setting_are_neutral(mcpt, rooms):
    sc = mcpt.Scene(SCENES, "cornell-box", width=80, height=60)
    dev = mcpt.Device(sc, 0)
    assert sc.info.num_lights == 1 and dev.light_sampling()[0] == "all"
    st0, st1 = mcpt.Stats(), mcpt.Stats()
    base = dev.generateImg(8, seed=2, stats=st0)
    dev.set_light_sampling("one")
    assert dev.light_sampling()[0] == "one" and dev.light_sampling()[1][0] == 1.0
    one = dev.generateImg(8, seed=2, stats=st1)
    mk = dev.generateImg(8, seed=2, flags=mcpt.RENDER_MEGAKERNEL)
    assert same(one, base) and same(mk, base) and TL._counts(st0) == TL._counts(st1)
    dev.close()
    sc.close()
    r = rooms(10)
    never, dev = r.device("pool"), r.device("default")
    st0, st1 = mcpt.Stats(), mcpt.Stats()
    base = never.generateImg(4, seed=3, stats=st0)                  # a device that was never set
    dev.set_light_sampling("one")
    assert not same(dev.generateImg(4, seed=3), base)
    dev.set_light_sampling(None)
    again = dev.generateImg(4, seed=3, stats=st1)
    assert same(again, base) and TL._counts(st0) == TL._counts(st1)
    assert same(dev.light_sampling()[1], np.ones(10))


# ---------------------------------------------------------------------------------------------- (d) routes and counts
ROUTES = ("no-finish", "finish-lane", "late-finish", "logic-grid-2", "small-workspace", "vote", "pool")


@pytest.mark.parametrize("nl", [10, 40])
def test_every_route_gives_the_same_frame(rooms, mcpt, nl):
    r = rooms(nl)
    spp = 4
    all_st = mcpt.Stats()
    all_img = r.device().generateImg(spp, seed=3, stats=all_st)
    for d in ("default",) + ROUTES:
        r.device(d).set_light_sampling("one")
    base_st = mcpt.Stats()
    base = r.device().generateImg(spp, seed=3, stats=base_st)
    assert np.isfinite(base).all() and base.sum() > 0 and not same(base, all_img)
    routes = {}
    st = mcpt.Stats()
    routes["megakernel"] = (r.device().generateImg(spp, seed=3, flags=mcpt.RENDER_MEGAKERNEL, stats=st), TL._counts(st))
    for which in ROUTES:
        st = mcpt.Stats()
        routes[which] = (r.device(which).generateImg(spp, seed=3, stats=st), TL._counts(st))
    parts = np.zeros_like(base)
    total = np.zeros(4, dtype=np.int64)
    for rank in range(3):
        st = mcpt.Stats()
        r.device().generateImg(spp, seed=3, rank=rank, world=3, img=parts, stats=st)
        total += np.array(TL._counts(st), dtype=np.int64)
    routes["partitions"] = (parts, tuple(int(x) for x in total))
    for which, (img, counts) in routes.items():
        bad = int((bits(img) != bits(base)).sum())
        assert bad == 0, "%s: %d channels differ from the default route" % (which, bad)
        assert counts == TL._counts(base_st), (which, counts, TL._counts(base_st))
    # the paths are the "all" frame's; one shadow ray (or one skipped) per vertex instead of nl
    a, o = TL._counts(all_st), TL._counts(base_st)
    assert o[1:] == a[1:]
    assert a[0] % nl == 0 and o[0] == a[0] // nl
    # the same expectation: the frames' means agree to a few per cent at 4 samples per pixel
    assert abs(base.mean() / all_img.mean() - 1.0) < 0.1
    for d in ("default",) + ROUTES:
        r.device(d).set_light_sampling(None)


# ---------------------------------------------------------------------------------------------- (e) unbiased
# Blocks for pins_common.assert_standard_normal (bars: |mean z| < 0.2, rms in 0.8 .. 1.25).  The three channels of a block move together, so
# B blocks are about B independent z: their mean has a standard deviation of 1 / sqrt(B), 0.058 at B = 300 -- the 0.2 bar is then 3.5
# sigma away.  A sample's difference is skewed (most picks give a little less than "all", a few give 1 / p times more), and a block's
# sigma rises with its mean, which pulls z below 0 by about skewness / (2 sqrt(block)): blocks of thousands of samples keep that under
# the bar for a skewness of a few tens.
BLOCKS = 300
BLOCK = 4096                    # the same for the test and its cross-check
PATH_BLOCK = BLOCK


def test_one_minus_all_has_zero_mean(rooms):
    r = rooms(10)
    dev = r.device()
    pix, k = triples(BLOCKS * BLOCK, 99)
    ref = dev.sample_radiance(5, pix, k)
    dev.set_light_sampling("one")
    one = dev.sample_radiance(5, pix, k)
    dev.set_light_sampling(None)
    assert np.isfinite(one).all() and np.isfinite(ref).all()
    diff, sigma = LP.block_z(one - ref, BLOCK)
    live = (sigma > 0).all(axis=1)
    print(pins_common.assert_standard_normal(diff[live], sigma[live], "one - all, 10 lights"))


def test_a_halved_factor_fails_the_same_test(rooms):
    """The test's power, in numpy alone: on the diffuse-only room every sample is the sum of its lights' parts (the one-hot identity), so
    part[l*] / p[l*] with l* the restatement's pick is another unbiased estimator of it -- and stops being one when a light's factor is
    halved.  Its limit: this is NOT the library's estimator, which picks anew at every vertex (per-vertex, per-light terms are not to be had
    from outside the kernels); it keeps the light picked at depth 0 for the whole path, on the diffuse-only room.  Same blocks, same block
    size, same bars and the same table as test_one_minus_all_has_zero_mean: it shows that those bars catch a factor that is off by 2 in an
    estimator of this family, not that they would catch every error in the library's."""
    r = rooms(10, diffuse_only=True)
    dev = r.device()
    pix, k = _non_emitter_samples(r, int(BLOCKS * PATH_BLOCK * 1.2), 23)
    n = BLOCKS * PATH_BLOCK
    assert pix.shape[0] >= n
    pix, k = pix[:n], k[:n]
    ref = dev.sample_radiance(5, pix, k)
    parts = _per_light(dev, 10, 5, pix, k)
    table = LP.PickRef.of_scene(r.sc)
    light = table.pick(5, pix, k, 0)[0]
    good = LP.path_pick_estimate(parts, light, table.inv)
    diff, sigma = LP.block_z(good - ref, PATH_BLOCK)
    print(pins_common.assert_standard_normal(diff, sigma, "numpy estimator, right factors"))
    wrong = table.inv.copy()
    wrong[int(np.argmax(parts.sum(axis=(1, 2))))] *= 0.5           # the light that gives the most
    bad = LP.path_pick_estimate(parts, light, wrong)
    diff, sigma = LP.block_z(bad - ref, PATH_BLOCK)
    with pytest.raises(AssertionError):
        pins_common.assert_standard_normal(diff, sigma, "numpy estimator, one factor halved")


# ---------------------------------------------------------------------------------------------- (f) compositions
def test_progressive_and_adaptive_frames(rooms):
    r = rooms(40)
    for which in ("default", "small-workspace"):
        dev = r.device(which)
        dev.set_light_sampling("one")
        ref = dev.generateImg(16, seed=5)
        pr = dev.progressive(16, seed=5)
        for n in (1, 6, 2, 7):
            pr.step(n)
        assert pr.done == 16
        img = pr.image()
        pr.close()
        assert same(img, ref), which
        ad = dev.adaptive(16, 0.0, 0.0, min_spp=4, seed=5)                  # targets 0: no pixel ever stops
        for n in (4, 5, 7):
            ad.step(n)
        assert ad.done == 16 and ad.active == 0
        img = ad.image()
        ad.close()
        assert same(img, ref), which
        dev.set_light_sampling(None)
        assert not same(dev.generateImg(16, seed=5), ref)


def test_denoised_frame(rooms):
    """a denoised frame under "one": the same on two routes (its inputs are the frame's moments and the first-hit AOVs), the AOVs those of
    the "all" frame (the paths are the same), the picture not"""
    r = rooms(10)
    out = {}
    for which in ("default", "small-workspace"):
        dev = r.device(which)
        for mode in ("one", None):
            dev.set_light_sampling(mode)
            pr = dev.progressive(8, seed=5)
            pr.step(3)
            pr.step(5)
            out[which, mode] = (pr.denoise(), pr.image(), pr.aovs())
            pr.close()
    dn, img, aov = out["default", "one"]
    assert np.isfinite(dn).all() and dn.sum() > 0 and not same(dn, img)
    assert same(dn, out["small-workspace", "one"][0]) and same(img, out["small-workspace", "one"][1])
    assert not same(dn, out["default", None][0])
    for name, a in aov.items():
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(out["default", None][2][name]).view(np.uint8)), name


def test_updated_device_equals_a_fresh_one(rooms, mcpt, tmp_path_factory):
    """update_vertices moves and scales every emitter: the default weights follow the new areas, whichever of the two calls comes first"""
    r = rooms(10)
    g, m, _ = r.sc.faces()
    v0 = np.ascontiguousarray(g[:, :9])
    v1 = np.ascontiguousarray(A.move_lights(v0, m, [r.sc.light(i)[2] for i in range(10)], scale=1.05, shift=(0.01, -0.004, 0.006)))
    d = A.write_moved(r.dir, r.name, v1, str(tmp_path_factory.mktemp("pick_moved")))
    sc = mcpt.Scene(d, r.name, width=W, height=H)
    fresh = mcpt.Device(sc, 0)
    fresh.set_light_sampling("one")
    st0 = mcpt.Stats()
    want, want_pdf = fresh.generateImg(4, seed=6, stats=st0), fresh.light_sampling()[1]
    assert same(want_pdf, LP.PickRef.of_scene(sc).pdf)
    for first in ("set", "update"):
        dev = mcpt.Device(r.sc, 0)
        if first == "set":
            dev.set_light_sampling("one")
            before = dev.light_sampling()[1]
            dev.update_vertices(v1)
            assert not same(before, want_pdf)
        else:
            dev.update_vertices(v1)
            dev.set_light_sampling("one")
        assert same(dev.light_sampling()[1], want_pdf), first
        st = mcpt.Stats()
        img = dev.generateImg(4, seed=6, stats=st)
        assert same(img, want) and TL._counts(st) == TL._counts(st0), first
        mk = dev.generateImg(4, seed=6, flags=mcpt.RENDER_MEGAKERNEL)
        assert same(mk, want), first
        w = np.linspace(1.0, 2.0, 10)
        dev.set_light_sampling("one", w)                             # the caller's weights do not follow the areas
        dev.update_vertices(v0)
        assert same(dev.light_sampling()[1], LP.PickRef(w).pdf)
        dev.close()
    fresh.close()
    sc.close()


@pytest.mark.parametrize("nl", [10, 40])
def test_wavefront_equals_megakernel_under_a_lens(rooms, mcpt, nl):
    dev = rooms(nl).device()
    dev.set_light_sampling("one")
    pin = dev.generateImg(8, seed=3)
    dev.set_lens(**TL.LENS)
    try:
        wf = dev.generateImg(8, seed=3)
        mk = dev.generateImg(8, seed=3, flags=mcpt.RENDER_MEGAKERNEL)
    finally:
        dev.set_lens()
        dev.set_light_sampling(None)
    assert same(wf, mk) and np.isfinite(wf).all()
    assert (bits(wf) != bits(pin)).sum() > wf.size // 4


def test_environment_keeps_its_own_shadow_ray(rooms, mcpt):
    r = rooms(10)
    sky = np.array([[[0.6, 0.7, 1.0], [0.2, 0.2, 0.3]], [[0.3, 0.25, 0.2], [0.05, 0.05, 0.1]]])
    frames = {}
    for which in ("default", "finish-lane", "no-finish"):
        dev = r.device(which)
        dev.set_environment(sky, 0.8)
        dev.set_light_sampling("one")
        st = mcpt.Stats()
        frames[which] = dev.generateImg(4, seed=3, stats=st)
        # per vertex: the picked light's shadow ray and the environment's, whatever the light count
        assert 0 < st.rays_shadow <= 2 * st.shade_calls and st.rays_shadow + st.shadow_skipped <= 2 * st.shade_calls, which
        if which == "default":
            st = mcpt.Stats()
            mk = dev.generateImg(4, seed=3, flags=mcpt.RENDER_MEGAKERNEL, stats=st)
            assert same(mk, frames[which]) and st.rays_shadow <= 2 * st.shade_calls
        dev.set_environment(None)
        dev.set_light_sampling(None)
    assert same(frames["finish-lane"], frames["default"]) and same(frames["no-finish"], frames["default"])


def test_motion_frame_equals_fresh_devices(rooms, mcpt, tmp_path_factory):
    r = rooms(10)
    N, K, shutter, seed = 8, 2, (0.25, 0.75), 11
    g, m, _ = r.sc.faces()
    v0 = np.ascontiguousarray(g[:, :9])
    v1 = np.ascontiguousarray(A.move_lights(v0, m, [r.sc.light(i)[2] for i in range(10)], scale=1.05, shift=(0.01, -0.004, 0.006)))
    dev = mcpt.Device(r.sc, 0)
    dev.set_light_sampling("one")
    before = dev.light_sampling()[1]
    dev.set_motion(v_end=v1, shutter=shutter, steps=K)
    img = dev.generateImg(N, seed=seed)
    pix = np.repeat(np.arange(W * H, dtype=np.int32), N)
    ks = np.tile(np.arange(N, dtype=np.int32), W * H)
    x = np.zeros((W * H, N, 3))
    for j, (k0, n) in enumerate(MR.step_ranges(N, K)):
        u = MR.shutter_time(shutter[0], shutter[1], K, j)
        d = A.write_moved(r.dir, r.name, np.ascontiguousarray(MR.blend(v0, v1, u)), str(tmp_path_factory.mktemp("pick_step")))
        sc = mcpt.Scene(d, r.name, width=W, height=H)
        fresh = mcpt.Device(sc, 0)
        fresh.set_light_sampling("one")
        assert not same(fresh.light_sampling()[1], before)         # the emitters' areas, hence the default weights, move with the step
        x[:, k0:k0 + n] = fresh.sample_radiance(seed, pix, ks).reshape(W * H, N, 3)[:, k0:k0 + n]
        fresh.close()
        sc.close()
    want = MR.fold(x, N).reshape(H, W, 3)
    bad = int((bits(img) != bits(want)).sum())
    assert bad == 0, "%d of %d channels differ" % (bad, img.size)
    assert same(dev.sample_radiance(seed, pix[:64], ks[:64]), _static(mcpt, r, seed, pix[:64], ks[:64]))      # key 0 again, its weights too
    assert same(dev.light_sampling()[1], before)
    dev.close()


def _static(mcpt, r, seed, pix, ks):
    d = mcpt.Device(r.sc, 0)
    d.set_light_sampling("one")
    out = d.sample_radiance(seed, pix, ks)
    d.close()
    return out


def test_multi_device_equals_the_single_device(rooms, mcpt):
    r = rooms(10)
    dev = r.device()
    dev.set_light_sampling("one")
    st1 = mcpt.Stats()
    ref = dev.generateImg(6, seed=4, stats=st1)
    dev.set_light_sampling(None)
    md = mcpt.MultiDevice(r.sc, devices=[0, 0], gather=mcpt.GATHER_PEER)
    md.set_light_sampling("one")
    st = mcpt.Stats()
    img = md.generateImg(6, seed=4, stats=st)
    assert same(img, ref) and TL._counts(st) == TL._counts(st1)
    for bad in ([1.0] * 9, [0.0] * 10, [-1.0] + [1.0] * 9):          # a refused argument changes no device of the group
        with pytest.raises(mcpt.McptError):
            md.set_light_sampling("one", bad)
        assert same(md.generateImg(6, seed=4), ref)
    md.set_light_sampling(None)
    assert not same(md.generateImg(6, seed=4), ref)
    md.close()


def test_checkpoint_keeps_to_its_setting(rooms, mcpt, tmp_path):
    r = rooms(10)
    out = str(tmp_path) + os.sep
    kw = dict(seed=9, width=W, height=H, quiet=True, checkpoint_parts=4)
    ck = out + "frame.ckp"
    st = mcpt.Stats()
    mcpt.render_scene(r.dir, r.name, 4, output_prefix=out + "one", checkpoint=ck, light_sampling="one", stats=st, **kw)
    assert st.samples == W * H * 4
    dev = r.device()
    dev.set_light_sampling("one")
    want = mcpt.imshow_rgb8(dev.generateImg(4, seed=9))
    dev.set_light_sampling(None)
    from PIL import Image
    assert np.array_equal(np.array(Image.open(out + "one-SPP4.png").convert("RGB")), want)
    st = mcpt.Stats()
    mcpt.render_scene(r.dir, r.name, 4, output_prefix=out + "again", checkpoint=ck, light_sampling="one", stats=st, **kw)
    assert st.samples == 0                                          # loads under "one": nothing left to render
    with pytest.raises(mcpt.McptError):
        mcpt.checkpoint_load(ck, r.sc, 4, 9, 4)                     # not the "all" frame's identity
    ck2 = out + "copy.ckp"
    open(ck2, "wb").write(open(ck, "rb").read())
    st = mcpt.Stats()
    mcpt.render_scene(r.dir, r.name, 4, output_prefix=out + "all", checkpoint=ck, stats=st, **kw)
    assert st.samples == W * H * 4                                  # refused under "all": everything is rendered
    mcpt.checkpoint_load(ck, r.sc, 4, 9, 4)                         # ... and the file now is the "all" frame's, as it always was
    st = mcpt.Stats()
    mcpt.render_scene(r.dir, r.name, 4, output_prefix=out + "w", checkpoint=ck2, light_sampling={"mode": "one", "weights": np.ones(10)}, stats=st, **kw)
    assert st.samples == W * H * 4                                  # refused under other weights too
    # a scene of one light renders the same bits in both modes: one identity, the checkpoint of either resumes under the other
    ck3 = out + "box.ckp"
    kw = dict(seed=9, width=80, height=60, quiet=True, checkpoint_parts=4)
    mcpt.render_scene(SCENES, "cornell-box", 4, output_prefix=out + "box", checkpoint=ck3, **kw)
    st = mcpt.Stats()
    mcpt.render_scene(SCENES, "cornell-box", 4, output_prefix=out + "box1", checkpoint=ck3, light_sampling="one", stats=st, **kw)
    assert st.samples == 0
    assert open(out + "box1-SPP4.png", "rb").read() == open(out + "box-SPP4.png", "rb").read()
