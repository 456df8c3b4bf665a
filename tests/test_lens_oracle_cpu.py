"""No GPU: the oracle's camera lens (oracle/mcpt_oracle.c: orc_scene_set_lens, orc_camera_rays), the side tests/test_gpu_lens_oracle.py
holds the devices to.  The lens is restated there from the "camera lens" paragraph of include/mcpt.h; here it is pinned:

(a) orc_camera_rays equals the numpy restatement tests/lens_ref.py on cornell-box and veach-mis, on random (pix, k < 2^20) under a 64-bit
    seed: bit for bit without a lens and under jitter (no transcendentals), within test_gpu_lens.py's own _ulps(...) <= 4 under the thin
    lenses (C's sin / cos and numpy's may differ by an ulp);
(b) without a lens, after one was set and cleared, and under MCPT_LENS_PER_SAMPLE alone, orc_sample_radiance (300 samples) and a 33x17
    SPP-3 orc_render are an untouched scene's bit for bit, statistics included -- under PER_SAMPLE the frame traces W*H*spp primary rays,
    so rays_primary and the walk's box / triangle tests become those of the untouched scene at faithful cost (which re-traces the primary
    ray per sample as well) and every other figure stays;
(c) under a lens orc_render (either cost) is the float fold over k of orc_sample_radiance bit for bit, missed samples included, and its
    statistics are the samples' summed; camera_miss counts the samples whose own camera ray hits nothing;
(d) bad arguments are refused and keep the previous lens;
(e) the two deliberately wrong modes (set_lens(wrong=1 | 2)) differ from the right oracle on more samples of the GPU test's own sample
    set than that test's flip allowance, and fail its check.  Measured here (3000 samples, seed 77, 96x64):
      wrong = 1, glassroom, jitter + aperture 0.05 : 64 of 3000 samples differ (allowance 5) -- the first vertices that are view
                 dependent (glass, the Ns-60 lobe); a diffuse first vertex does not move at all, which is why the pipelines' agreement and
                 a picture's look cannot stand in for this comparison
      wrong = 2, open scene, "map" sky, thin-jitter-far : 883 of 3000 samples differ (allowance 7), all of them missed samples"""
import os

import numpy as np
import pytest

import env_scenes
import lens_ref
import test_gpu_env_oracle as TE
from conftest import SCENES, extra_scene_dir
from test_gpu_lens import _ulps

W, H, SPP = 33, 17, 3
LENSES = {"jitter": dict(jitter=True), "thin": dict(aperture=0.05), "thin-jitter-far": dict(aperture=0.3, focus_distance=2.5, jitter=True)}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def stats_dict(st):
    return {f: getattr(st, f) for f, _ in st._fields_}


def samples(oracle, osc, seed, pix, k):
    """orc_sample_radiance of samples (pix[i], k[i]): radiance (n, 3) and the statistics of all of them (max_depth: the largest)"""
    st = oracle.Stats()
    out = np.array([osc.sample_radiance(seed, int(p // osc.width), int(p % osc.width), int(kk), stats=st) for p, kk in zip(pix, k)])
    return out, stats_dict(st)


@pytest.fixture(scope="module")
def open_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("lens_oracle_scenes")) + os.sep
    env_scenes.open_scene(d, "open_small", 1, W, H)
    env_scenes.open_scene(d, "open", 1, 96, 64)
    return d


def _scene(oracle, open_dir, which, w=W, h=H):
    """cornell-box (no environment: a camera ray past the box brings 0), or the open scene under the "map" sky (misses that bring Le)"""
    if which == "cornell-box":
        return oracle.OracleScene(SCENES + which, texture_dir=SCENES, width=w, height=h)
    osc = oracle.OracleScene(open_dir + ("open_small" if w == W else "open"), texture_dir=open_dir, width=w, height=h)
    assert osc.set_environment(*env_scenes.SKIES["map"]) > 0
    return osc


# ---------------------------------------------------------------------------------------------- (a) the rays
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_camera_rays_equal_the_restatement(oracle, name):
    w, h = 160, 90
    osc = oracle.OracleScene(SCENES + name, texture_dir=SCENES, width=w, height=h)
    c = osc.camera
    cam = lens_ref.Camera(c[0:3], c[3:6], c[6:9], c[9], w, h)
    rng = np.random.default_rng(5)
    pix = rng.integers(0, w * h, size=4000).astype(np.int32)
    ks = rng.integers(0, 1 << 20, size=4000).astype(np.int32)
    seed = 0x0123456789ABCDEF
    pin = osc.camera_rays(seed, pix, ks)
    assert np.array_equal(bits(pin), bits(lens_ref.camera_ray(cam, seed, pix, ks)))
    assert np.array_equal(bits(pin), bits(np.array([osc.primary_ray(int(p // w), int(p % w)) for p in pix])))     # the reference's primary rays
    osc.set_lens(per_sample=True)
    assert np.array_equal(bits(osc.camera_rays(seed, pix, ks)), bits(pin))
    osc.set_lens(jitter=True)
    jit = osc.camera_rays(seed, pix, ks)
    assert np.array_equal(bits(jit), bits(lens_ref.camera_ray(cam, seed, pix, ks, jitter=True)))
    assert (bits(jit[:, 3:]) != bits(pin[:, 3:])).any(axis=1).all() and np.array_equal(bits(jit[:, :3]), bits(pin[:, :3]))
    for ap, fd in ((0.05, 0.0), (0.3, 2.5)):
        osc.set_lens(aperture=ap, focus_distance=fd, jitter=True)
        got = osc.camera_rays(seed, pix, ks)
        want = lens_ref.camera_ray(cam, seed, pix, ks, aperture=ap, focus_distance=fd, jitter=True)
        u = _ulps(got, want).max()
        print("%s aperture %g F %g: the oracle's rays within %.2f ulps of the restatement's" % (name, ap, fd, u))
        assert u <= 4, u
        assert np.abs(np.linalg.norm(got[:, 3:], axis=1) - 1.0).max() <= 4e-16
        r = np.linalg.norm(got[:, :3] - np.array(cam.eye), axis=1)           # (x^ and y^ are orthogonal in both scenes)
        assert abs(np.dot(cam.xhat, cam.up)) <= 1e-15 and 0.9 * ap < r.max() <= ap * (1 + 1e-12)
    osc.set_lens()
    assert np.array_equal(bits(osc.camera_rays(seed, pix, ks)), bits(pin))
    with pytest.raises(ValueError):
        osc.camera_rays(seed, [w * h], [0])
    with pytest.raises(ValueError):
        osc.camera_rays(seed, [0], [-1])
    osc.close()


# ---------------------------------------------------------------------------------------------- (b) the pinhole is what it was
@pytest.mark.parametrize("which", ["cornell-box", "open-sky"])
def test_no_lens_and_per_sample_alone_are_the_untouched_scene(oracle, open_dir, which):
    never, used = _scene(oracle, open_dir, which), _scene(oracle, open_dir, which)
    rng = np.random.default_rng(8)
    pix, k = rng.integers(0, W * H, size=300), rng.integers(0, 64, size=300)
    want, want_st = samples(oracle, never, 77, pix, k)
    ost, fst = oracle.Stats(), oracle.Stats()
    frame = never.render(SPP, seed=3, stats=ost)
    faithful = never.render(SPP, seed=3, stats=fst, faithful_cost=True)
    assert np.array_equal(bits(frame), bits(faithful)) and fst.rays_primary == W * H * SPP and ost.rays_primary == W * H
    used.set_lens(**LENSES["thin-jitter-far"])
    lensed = used.render(SPP, seed=3)
    assert (bits(lensed) != bits(frame)).sum() > frame.size // 4                 # the lens had been taken: another frame
    for lens in (dict(), dict(per_sample=True)):
        used.set_lens(**lens)
        got, got_st = samples(oracle, used, 77, pix, k)
        assert np.array_equal(bits(got), bits(want)) and got_st == want_st, lens          # a sample traces its primary ray either way
        for cost in (False, True):
            st = oracle.Stats()
            img = used.render(SPP, seed=3, stats=st, faithful_cost=cost)
            assert np.array_equal(bits(img), bits(frame)), (lens, cost)
            if lens and not cost:
                assert st.rays_primary == W * H * SPP
                assert stats_dict(st) == stats_dict(fst)                                  # the walk's work: one primary ray per sample
                walk = ("rays_primary", "box_tests", "tri_tests")
                assert {f: v for f, v in stats_dict(st).items() if f not in walk} == {f: v for f, v in stats_dict(ost).items() if f not in walk}
            else:
                assert stats_dict(st) == stats_dict(fst if cost else ost), (lens, cost)
    assert (ost.camera_miss > 0) == (which == "open-sky") and np.isfinite(frame).all() and frame.sum() > 0     # (counted under a sky only)
    never.close()
    used.close()


# ---------------------------------------------------------------------------------------------- (c) the frame is the fold of its samples
@pytest.mark.parametrize("lens", sorted(LENSES))
@pytest.mark.parametrize("which", ["cornell-box", "open-sky"])
def test_lens_frame_is_the_fold_of_its_samples(oracle, open_dir, which, lens):
    osc = _scene(oracle, open_dir, which)
    osc.set_lens(**LENSES[lens])
    st = oracle.Stats()
    frame = osc.render(SPP, seed=3, stats=st)
    fst = oracle.Stats()
    assert np.array_equal(bits(osc.render(SPP, seed=3, stats=fst, faithful_cost=True)), bits(frame)) and stats_dict(fst) == stats_dict(st)
    pix = np.repeat(np.arange(W * H), SPP)
    k = np.tile(np.arange(SPP), W * H)
    x, sst = samples(oracle, osc, 3, pix, k)
    x = x.reshape(W * H, SPP, 3)
    acc = np.zeros((W * H, 3), dtype=np.float32)
    for j in range(SPP):                                                          # float += double / spp, in k order
        acc = (acc.astype(np.float64) + x[:, j] / SPP).astype(np.float32)
    assert np.array_equal(bits(acc.astype(np.float64)), bits(frame.reshape(-1, 3)))
    assert sst == stats_dict(st) and st.rays_primary == st.samples == W * H * SPP
    # the samples that miss are those whose OWN camera ray hits nothing; with a sky they bring Le of their own direction
    rays = osc.camera_rays(3, pix, k)
    miss = osc.trace_closest(rays)[0] < 0
    if which == "open-sky":
        assert st.camera_miss == int(miss.sum()) > 0
        assert np.array_equal(bits(x.reshape(-1, 3)[miss]), bits(osc.env_eval(rays[miss, 3:])))
        mixed = miss.reshape(W * H, SPP)
        assert (mixed.any(axis=1) & ~mixed.all(axis=1)).any()                     # silhouette pixels: some samples hit, some miss
    else:                                                                         # without one a missed sample is 0 and is not counted
        assert st.camera_miss == 0 and np.all(x.reshape(-1, 3)[miss] == 0.0)
    assert 0 < miss.sum() < miss.size
    osc.close()


# ---------------------------------------------------------------------------------------------- (d) arguments
def test_bad_lenses_are_refused_and_keep_the_previous_one(oracle):
    osc = oracle.OracleScene(SCENES + "cornell-box", texture_dir=SCENES, width=W, height=H)
    L = oracle.lib()
    osc.set_lens(**LENSES["thin-jitter-far"])
    pix, k = np.arange(0, W * H, 7), np.arange(0, W * H, 7) % 64
    rays, rad = osc.camera_rays(9, pix, k), samples(oracle, osc, 9, pix, k)
    for bad in [(4, 0.0, 0.0), (-1, 0.0, 0.0), (1, -0.1, 0.0), (0, float("nan"), 0.0), (0, float("inf"), 0.0), (1, 0.1, float("nan")),
                (1, 0.1, float("inf")), (1, 0.1, float("-inf"))]:
        assert L.orc_scene_set_lens(osc.h, *bad) == -1, bad
        assert np.array_equal(bits(osc.camera_rays(9, pix, k)), bits(rays)), bad
    got = samples(oracle, osc, 9, pix, k)
    assert np.array_equal(bits(got[0]), bits(rad[0])) and got[1] == rad[1]
    with pytest.raises(ValueError):
        osc.set_lens(aperture=-1.0)
    assert L.orc_scene_set_lens_wrong(osc.h, 3) == -1 and L.orc_scene_set_lens_wrong(osc.h, -1) == -1
    assert L.orc_scene_set_lens(osc.h, 0, 0.0, -5.0) == 0                        # a focus distance <= 0 is |look_at - eye|: fine
    with pytest.raises(ValueError):
        osc.set_lens(wrong=1)                                                     # nothing to get wrong without an active lens
    osc.close()


# ---------------------------------------------------------------------------------------------- (e) the wrong oracles are seen
def gpu_sample_set(w, h):
    """test_gpu_env_oracle._oracle_samples' set: what tests/test_gpu_lens_oracle.py compares"""
    rng = np.random.default_rng(5)
    return rng.integers(0, w * h, size=TE.N_SAMPLES).astype(np.int32), rng.integers(0, 64, size=TE.N_SAMPLES).astype(np.int32)


def flip_allowance(on_surface):
    """the mismatches TE._check_samples lets pass, of both kinds together"""
    return int(on_surface.shape[0] * TE.OTHER_FLIP_RATE) + max(2, int(on_surface.sum() * TE.ON_SURFACE_FLIP_RATE) + 1)


POWER = {1: ("glassroom", dict(jitter=True, aperture=0.05)), 2: ("open-sky", LENSES["thin-jitter-far"])}


@pytest.mark.parametrize("wrong", [1, 2])
def test_the_sample_check_fails_against_a_wrong_oracle(oracle, open_dir, wrong):
    which, lens = POWER[wrong]
    w, h = 96, 64
    if which == "glassroom":
        base = extra_scene_dir()
        osc = oracle.OracleScene(base + which, texture_dir=base, width=w, height=h)
    else:
        osc = _scene(oracle, open_dir, which, w, h)
    pix, k = gpu_sample_set(w, h)
    osc.set_lens(**lens)
    right = np.zeros((pix.shape[0], 3))
    on_surface = np.zeros(pix.shape[0], dtype=bool)
    for i, (p, kk) in enumerate(zip(pix, k)):
        st = oracle.Stats()
        right[i] = osc.sample_radiance(TE.SEED, int(p // w), int(p % w), int(kk), stats=st)
        on_surface[i] = st.rays_on_surface > 0
    TE._check_samples(right, right.copy(), on_surface)
    osc.set_lens(wrong=wrong, **lens)
    bad, _ = samples(oracle, osc, TE.SEED, pix, k)
    differ = np.abs(right - bad).max(axis=1) > TE.REL_TOL * np.maximum(np.abs(right).max(axis=1), 1e-12)
    allow = flip_allowance(on_surface)
    print("wrong = %d on %s: %d of %d samples differ (allowance %d)" % (wrong, which, int(differ.sum()), pix.shape[0], allow))
    assert differ.sum() > allow
    with pytest.raises(AssertionError):
        TE._check_samples(right, bad, on_surface)
    if wrong == 2:                                                                # only missed samples move
        miss = osc.trace_closest(osc.camera_rays(TE.SEED, pix, k))[0] < 0
        assert not (differ & ~miss).any() and miss.sum() > differ.sum() > 0
    osc.set_lens(**lens)                                                          # (setting a lens leaves the right answers)
    again, _ = samples(oracle, osc, TE.SEED, pix[:200], k[:200])
    assert np.array_equal(bits(again), bits(right[:200]))
    osc.close()
