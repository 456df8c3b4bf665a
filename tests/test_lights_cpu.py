"""CPU: the many-light test scenes (tests/light_scenes.py) load the same way in the product and in the oracle, and each variant
is what it claims to be -- every oracle sample finite ("finite"), or NaN where the reference's "no triangle chosen" meets a surface
facing the origin ("nan").  The GPU side of these scenes is tests/test_gpu_lights.py."""
import os

import numpy as np
import pytest

import light_scenes

LIGHT_COUNTS = [3, 4, 6, 9, 10, 20, 40]
W, H = 33, 17


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("light_scenes")) + os.sep


def test_generator_has_room_for_every_count():
    assert max(LIGHT_COUNTS) <= light_scenes.MAX_LIGHTS


@pytest.mark.parametrize("variant", ["finite", "nan"])
@pytest.mark.parametrize("nl", LIGHT_COUNTS)
def test_loaders_agree_and_variant_holds(scene_dir, oracle, mcpt, nl, variant):
    name = "lights%d_%s" % (nl, variant)
    mats = light_scenes.write(scene_dir, name, nl, W, H, variant=variant)
    osc = oracle.OracleScene(scene_dir + name, texture_dir=scene_dir, width=W, height=H)
    sc = mcpt.Scene(scene_dir, name, width=W, height=H)
    try:
        assert osc.num_lights == nl and sc.info.num_lights == nl
        areas = []
        for i in range(nl):
            on, orad, omat, oarea = osc.light(i)
            gn, grad, gmat, garea = sc.light(i)
            assert on == gn == mats[i]
            assert omat == gmat and osc.material(omat)[0] == sc.material(gmat)[0] == mats[i]
            assert np.array_equal(_bits(orad), _bits(grad)), (i, orad, grad)
            assert np.array_equal(_bits(oarea), _bits(garea)), (i, oarea, garea)
            areas.append(oarea)
        areas = np.array(areas)
        assert np.isfinite(areas).all() and (areas > 0).all()
        assert areas[1] == areas[0]                              # the translated copy: exactly the same area
        rad = np.array([osc.light(i)[1] for i in range(nl)])
        assert rad.max() > 10 * rad.min()
        if variant == "finite":
            assert (areas >= areas[0]).all() and areas.max() > 2 * areas[0]
        else:
            assert (areas <= areas[0]).all() and (areas < areas[0]).sum() == nl - 2
        st = oracle.Stats()
        img = osc.render(2, seed=3, stats=st)
        assert st.rays_on_surface == 0                           # no refraction: the tight oracle bars apply
        assert st.rays_shadow > 0 and img.sum() != 0
        if variant == "finite":
            assert np.isfinite(img).all()
        else:
            frac = np.isnan(img).any(axis=2).mean()
            assert 0 < frac < 0.8, frac
            assert not np.isinf(img).any()
    finally:
        sc.close()
        osc.close()


@pytest.mark.parametrize("nl", [3, 10])
def test_nan_samples_are_the_no_triangle_case(scene_dir, oracle, nl):
    """Per sample, NaN comes only from the "nan" variant and only on some samples; the "finite" twin of the same light count has
    none on the same samples."""
    out = {}
    for variant in ("finite", "nan"):
        name = "samples%d_%s" % (nl, variant)
        light_scenes.write(scene_dir, name, nl, W, H, variant=variant)
        osc = oracle.OracleScene(scene_dir + name, texture_dir=scene_dir, width=W, height=H)
        rng = np.random.default_rng(1)
        out[variant] = np.array([osc.sample_radiance(5, int(r), int(c), int(k))
                                 for r, c, k in zip(rng.integers(0, H, 400), rng.integers(0, W, 400), rng.integers(0, 16, 400))])
        osc.close()
    assert np.isfinite(out["finite"]).all()
    nan = np.isnan(out["nan"]).any(axis=1)
    assert 0 < nan.sum() < 0.5 * nan.size
    assert np.array_equal(np.isnan(out["nan"]).all(axis=1), nan)    # a NaN sample is NaN in every channel
