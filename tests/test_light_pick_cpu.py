"""No GPU: MCPT_LIGHTS_ONE's host side -- the pick table of a scene against its numpy restatement (tests/light_pick_ref.py), bit for bit,
the inputs it refuses, and the C ABI's new surface."""
import ctypes as C
import os

import numpy as np
import pytest

import light_pick_ref as LP
import light_scenes
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "mcpt.h")
NEW = ["mcpt_device_set_light_sampling", "mcpt_device_get_light_sampling", "mcpt_multi_set_light_sampling", "mcpt_scene_light_pick_table",
       "mcpt_light_pick", "mcpt_render_scene_lights"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def scenes(mcpt, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("pick_scenes")) + os.sep
    out = {}
    for nl in (3, 10, 40):
        light_scenes.write(d, "pick%d" % nl, nl, 48, 32)
        out[nl] = mcpt.Scene(d, "pick%d" % nl, width=48, height=32)
    yield out
    for s in out.values():
        s.close()


def same_table(scene, weights):
    cdf, pdf, inv = scene.light_pick_table(weights)
    ref = LP.PickRef.of_scene(scene, weights)
    assert np.array_equal(bits(cdf), bits(ref.cdf))
    assert np.array_equal(bits(pdf), bits(ref.pdf))
    assert np.array_equal(bits(inv), bits(ref.inv))
    nl = cdf.shape[0]
    assert abs(float(pdf.sum()) - 1.0) <= nl * 2.0 ** -52
    assert (np.diff(cdf) >= 0).all() and cdf[-1] > 0
    return cdf, pdf, inv


@pytest.mark.parametrize("nl", [3, 10, 40])
def test_default_table(scenes, nl):
    sc = scenes[nl]
    assert sc.info.num_lights == nl
    cdf, pdf, inv = same_table(sc, None)
    assert (pdf > 0).all()                       # every light of these scenes has power
    lights = [sc.light(i) for i in range(nl)]
    w = np.array([((0.2126 * l[1][0] + 0.7152 * l[1][1]) + 0.0722 * l[1][2]) * l[3] for l in lights])
    assert np.array_equal(bits(pdf), bits(w / cdf[-1]))
    assert pdf.max() / pdf.min() > 30            # lights two orders of magnitude apart: the weights tell them apart


@pytest.mark.parametrize("nl", [3, 10, 40])
def test_caller_weights(scenes, nl):
    sc = scenes[nl]
    rng = np.random.default_rng(nl)
    w = rng.uniform(0.1, 5.0, size=nl)
    same_table(sc, w)
    for zero in ([0], [nl - 1], [nl // 2], [0, nl - 1], [0, nl // 2, nl - 1] if nl > 3 else [0, 1]):
        wz = w.copy()
        wz[zero] = 0.0
        cdf, pdf, inv = same_table(sc, wz)
        assert (pdf[zero] == 0).all() and (inv[zero] == 0).all()
        ref = LP.PickRef(wz)
        u = np.concatenate([np.linspace(0.0, 1.0, 4001)[:-1], [1.0 - 2.0 ** -33, 2.0 ** -33]])
        picked = ref.pick_u(u)
        assert not np.isin(picked, zero).any()   # a light of weight 0 is never picked, at either end of the range
        assert set(picked.tolist()) == set(np.nonzero(wz > 0)[0].tolist())
    for l in range(nl):                          # one-hot weights: probability 1 and a factor of exactly 1
        e = np.zeros(nl)
        e[l] = 1.0
        cdf, pdf, inv = same_table(sc, e)
        assert pdf[l] == 1.0 and inv[l] == 1.0 and pdf.sum() == 1.0


def test_all_zero_power_falls_back_to_uniform(mcpt, tmp_path):
    d = str(tmp_path) + os.sep
    light_scenes.write(d, "dark", 4, 32, 32)
    cam = open(d + "dark.camera").read().splitlines()
    with open(d + "dark.camera", "w") as f:       # every light's radiance 0
        f.write("\n".join(" ".join(l.split()[:2] + ["0.0", "0.0", "0.0"]) if l.startswith("mtlname") else l for l in cam) + "\n")
    sc = mcpt.Scene(d, "dark", width=32, height=32)
    assert all(not sc.light(i)[1].any() for i in range(4))
    cdf, pdf, inv = same_table(sc, None)
    assert np.array_equal(cdf, [1.0, 2.0, 3.0, 4.0]) and (pdf == 0.25).all() and (inv == 4.0).all()
    sc.close()


def test_rejected_inputs(mcpt, scenes):
    sc = scenes[3]
    for bad in ([0.0, 0.0, 0.0], [1.0, -1.0, 1.0], [1.0, float("nan"), 1.0], [1.0, float("inf"), 1.0], [-0.0, 0.0, 0.0]):
        with pytest.raises(mcpt.McptError):
            sc.light_pick_table(bad)
        with pytest.raises(ValueError):
            LP.PickRef(bad)
    with pytest.raises(ValueError):
        sc.light_pick_table([1.0, 1.0])
    L = mcpt.lib()
    cdf = np.zeros(3)
    assert L.mcpt_scene_light_pick_table(None, None, cdf.ctypes.data_as(C.POINTER(C.c_double)), cdf.ctypes.data_as(C.POINTER(C.c_double))) == -3
    assert L.mcpt_scene_light_pick_table(sc._h, None, None, None) == -3
    with pytest.raises(ValueError):
        mcpt.make_light_sampling("some")
    with pytest.raises(ValueError):
        mcpt.make_light_sampling("all", [1.0])
    ls, keep = mcpt.make_light_sampling("one", [1.0, 2.0])
    assert (ls.mode, ls.num_weights) == (mcpt.LIGHTS_ONE, 2) and keep is not None
    assert mcpt.make_light_sampling(None) == (None, None)


def test_header_and_symbols(mcpt):
    hdr = open(HEADER).read()
    L = mcpt.lib()
    assert L.mcpt_version() == int(hdr.split("#define MCPT_VERSION")[1].split()[0])
    for name in NEW:
        assert name + "(" in hdr, name
        assert hasattr(L, name), name
        assert name in mcpt._lib.EXPORTS
    assert "#define MCPT_LIGHTS_ALL 0" in hdr and "#define MCPT_LIGHTS_ONE 1" in hdr
    assert "typedef struct { int32_t mode, num_weights; const double* weights; } mcpt_light_sampling;" in hdr
    assert C.sizeof(mcpt.LightSampling) == 16
    # without a GPU the device entry points check their arguments first, then report that there is no device
    bad = mcpt.LightSampling(7, 0, None)
    assert L.mcpt_device_set_light_sampling(None, C.byref(bad)) == -3
    w = (C.c_double * 2)(1.0, 2.0)
    bad = mcpt.LightSampling(mcpt.LIGHTS_ONE, 0, w)
    assert L.mcpt_device_set_light_sampling(None, C.byref(bad)) == -3
    assert L.mcpt_render_scene_lights(b"/nonexistent/", b"none", 1, None, 0, None, None, 1.0, C.byref(bad), None) == -3
    if mcpt.device_count() == 0:
        ok = mcpt.LightSampling(mcpt.LIGHTS_ONE, 0, None)
        assert L.mcpt_device_set_light_sampling(None, C.byref(ok)) == -4
        assert L.mcpt_device_set_light_sampling(None, None) == -4
