"""Not gpu: the C-ABI surface of motion blur -- symbols, struct layouts against the C compiler, the two pure functions against the numpy
restatement (tests/motion_ref.py), and the argument errors that come before the device check."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import motion_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "scenes") + os.sep
NEW = ["mcpt_device_set_motion", "mcpt_device_set_motion_device", "mcpt_device_clear_motion", "mcpt_device_get_motion", "mcpt_device_motion_info",
       "mcpt_shutter_time", "mcpt_shutter_step", "mcpt_render_scene_motion"]
ERR_ARG, ERR_NO_DEVICE = -3, -4
SHUTTERS = [(0.0, 1.0), (0.25, 0.5), (1.0, 1.0), (0.0, 0.0), (0.1, 0.7), (1.0 / 3.0, 2.0 / 3.0)]
# K = 1, K = N, N not divisible by K, N = 1, and a large frame
FRAMES = [(12, 1), (12, 12), (12, 5), (13, 3), (1, 1), (7, 7), (100, 64), (256, 3), (2 ** 20, 1000)]


def test_symbols_are_declared_and_exported(mcpt):
    from montecarlopathtracing_amd import _lib
    L = mcpt.lib()
    hdr = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    for sym in NEW:
        assert (sym + "(") in hdr and sym in _lib.EXPORTS and hasattr(L, sym), sym
    for t in ("} mcpt_shutter;", "} mcpt_camera_key;", "} mcpt_motion_info;"):
        assert t in hdr
    assert L.mcpt_version() == 105 and "#define MCPT_VERSION 105" in hdr


def test_struct_layouts_match_the_header(tmp_path):
    from montecarlopathtracing_amd import _lib
    structs = {"mcpt_shutter": _lib.Shutter, "mcpt_camera_key": _lib.CameraKey, "mcpt_motion_info": _lib.MotionInfo}
    lines = []
    for name, cls in structs.items():
        lines.append("  printf(\"%%zu\\n\", sizeof(%s));\n" % name)
        lines += ["  printf(\"%%zu\\n\", offsetof(%s, %s));\n" % (name, f) for f, _ in cls._fields_]
    src = tmp_path / "layout_motion.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"mcpt.h\"\nint main(void) {\n" + "".join(lines) + "  return 0;\n}\n")
    exe = tmp_path / "layout_motion"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = list(map(int, subprocess.check_output([str(exe)]).split()))
    want = []
    for cls in structs.values():
        want.append(C.sizeof(cls))
        want += [getattr(cls, f).offset for f, _ in cls._fields_]
    assert got == want


@pytest.mark.parametrize("open,close", SHUTTERS)
def test_shutter_time_is_the_reference(mcpt, open, close):
    L = mcpt.lib()
    for K in (1, 2, 3, 5, 12, 64, 1000):
        for j in sorted({0, 1 % K, K // 2, K - 1}):
            got, want = L.mcpt_shutter_time(open, close, K, j), MR.shutter_time(open, close, K, j)
            assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (open, close, K, j, got, want)
            assert open <= got <= close
        assert math.isnan(L.mcpt_shutter_time(open, close, K, K)) and math.isnan(L.mcpt_shutter_time(open, close, K, -1))
    if open == close:
        assert L.mcpt_shutter_time(open, close, 7, 3) == open


@pytest.mark.parametrize("N,K", FRAMES)
def test_shutter_step_tiles_the_frame(mcpt, N, K):
    L = mcpt.lib()
    ks = range(N) if N <= 4096 else list(range(0, N, 997)) + [N - 1]
    steps = np.array([L.mcpt_shutter_step(N, K, k) for k in ks])
    assert np.array_equal(steps, [MR.shutter_step(N, K, k) for k in ks])
    assert steps[0] == 0 and steps[-1] == K - 1 and np.all(np.diff(steps) >= 0)         # contiguous ranges in ascending order
    if N <= 4096:
        counts = np.bincount(steps, minlength=K)
        assert counts.min() >= 1 and counts.sum() == N                                    # every step is non-empty, the ranges tile [0, N)
        assert MR.step_ranges(N, K) == [(int(np.argmax(steps == j)), int(counts[j])) for j in range(K)]
        assert np.all(np.diff(steps) <= 1)
    assert L.mcpt_shutter_step(N, K, N) == -1 and L.mcpt_shutter_step(N, K, -1) == -1
    assert L.mcpt_shutter_step(N, N + 1, 0) == -1 and L.mcpt_shutter_step(N, 0, 0) == -1 and L.mcpt_shutter_step(0, 1, 0) == -1


def test_blend_reference_properties():
    """of the numpy restatement itself (the GPU file holds the library's blend to it): what the header promises of the blend"""
    rng = np.random.default_rng(4)
    a, b = rng.normal(size=1000), rng.normal(size=1000)
    b[::7] = a[::7]
    assert np.array_equal(MR.blend(a, b, 0.0), a) and np.array_equal(MR.blend(a, b, 1.0), b)
    for u in (0.125, 1.0 / 6.0, 0.7, MR.shutter_time(0.25, 0.5, 3, 1)):
        x = MR.blend(a, b, u)
        assert np.array_equal(x[::7], a[::7])                       # a coordinate that does not move keeps its bits
        assert np.array_equal(MR.blend(a, a, u), a)
        assert np.all((x >= np.minimum(a, b) - 1e-15) & (x <= np.maximum(a, b) + 1e-15))
    assert np.isnan(MR.blend([1.0], [np.inf], 0.0))[0] and MR.blend([1.0], [1e200], 0.5)[0] == 0.5 + 0.5 * 1e200


BAD_SHUTTERS = [(0.5, 0.25, 1, 0), (-0.1, 0.5, 1, 0), (0.0, 1.5, 1, 0), (0.0, 1.0, 0, 0), (0.0, 1.0, -3, 0), (float("nan"), 1.0, 1, 0),
                (0.0, float("inf"), 1, 0), (float("-inf"), 0.5, 1, 0), (0.0, 1.0, 1, 1)]


def test_invalid_shutters_come_before_the_device_check(mcpt):
    from montecarlopathtracing_amd import _lib
    L = mcpt.lib()
    nd = ERR_NO_DEVICE if L.mcpt_device_count() == 0 else ERR_ARG      # what a NULL device gets once the arguments are valid
    for s in BAD_SHUTTERS:
        sh = _lib.Shutter(*s)
        assert L.mcpt_device_set_motion(None, None, None, C.byref(sh)) == ERR_ARG, s
        assert b"shutter" in L.mcpt_last_error()
        assert L.mcpt_device_set_motion_device(None, None, None, C.byref(sh), None) == ERR_ARG, s
    assert L.mcpt_device_set_motion(None, None, None, None) == ERR_ARG
    bad_cam = _lib.CameraKey((C.c_double * 3)(0, 0, 1), (C.c_double * 3)(0, 0, 1), (C.c_double * 3)(0, 1, 0), 40.0)      # eye == look_at
    good = _lib.Shutter(0.0, 1.0, 4, 0)
    assert L.mcpt_device_set_motion(None, None, C.byref(bad_cam), C.byref(good)) == ERR_ARG
    assert L.mcpt_device_set_motion(None, None, None, C.byref(good)) == nd
    assert L.mcpt_device_set_motion_device(None, None, None, C.byref(good), None) == nd
    assert L.mcpt_device_clear_motion(None) == nd
    assert L.mcpt_device_get_motion(None, None, None, None, None) == nd
    assert L.mcpt_device_motion_info(None, None) == ERR_ARG
    info = _lib.MotionInfo()
    assert L.mcpt_device_motion_info(None, C.byref(info)) == nd


@pytest.mark.parametrize("shutter", BAD_SHUTTERS + [(0.0, 1.0, 5, 0)])
def test_render_scene_refuses_invalid_motions_before_writing(mcpt, tmp_path, shutter):
    """an invalid shutter, or more steps than samples, is MCPT_ERR_ARG before a scene is read, a device is asked for or a file is written"""
    from montecarlopathtracing_amd import _lib
    L = mcpt.lib()
    o = _lib.RenderSceneOptions()
    o.quiet, o.width, o.height = 1, 16, 9
    prefix = str(tmp_path / "out").encode()
    o.output_prefix = prefix
    sh = _lib.Shutter(*shutter)
    rc = L.mcpt_render_scene_motion(SCENES.encode(), b"cornell-box", 4, C.byref(o), C.sizeof(o), None, None, 1.0, None, None, C.byref(sh), None)
    assert rc == ERR_ARG and os.listdir(tmp_path) == []


def test_render_scene_motion_refusals(mcpt, tmp_path):
    """what a motion frame does not combine with, and an end key without a shutter"""
    sh = {"shutter": (0.0, 1.0), "steps": 2}
    out = str(tmp_path / "out")
    for kw in ({"checkpoint": str(tmp_path / "ck")}, {"devices": [0]}, {"adaptive_min_spp": 2, "noise_target": 0.1}, {"output_flags": mcpt.OUT_DENOISED},
               {"output_flags": mcpt.OUT_AOV_PFM}, {"noise_target": 0.05}, {"time_budget_s": 1.0}):     # (a frame stopped early: part of the shutter)
        with pytest.raises(mcpt.McptError) as e:
            mcpt.render_scene(SCENES, "cornell-box", 4, width=16, height=9, output_prefix=out, motion=sh, **kw)
        assert e.value.code == ERR_ARG, kw
    from montecarlopathtracing_amd import _lib
    o = _lib.RenderSceneOptions()
    rc = mcpt.lib().mcpt_render_scene_motion(SCENES.encode(), b"cornell-box", 4, C.byref(o), C.sizeof(o), None, None, 1.0, b"x.obj", None, None, None)
    assert rc == ERR_ARG and os.listdir(tmp_path) == []
