"""Not gpu: the C-ABI surface of the camera lens -- symbols, the mcpt_lens layout against the C compiler, argument errors with a null
device, render_scene's refusals of invalid lenses before any file is written, and the numpy restatement (lens_ref) pinned to the
oracle's primary rays and Philox stream."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import lens_ref
from conftest import ROOT, SCENES

ERR_ARG, ERR_NO_DEVICE = -3, -4
NAMES = ["mcpt_device_set_lens", "mcpt_device_get_lens", "mcpt_camera_rays", "mcpt_multi_set_lens", "mcpt_render_scene_lens"]


def _null_device_rc(mcpt):
    """what a null handle with valid arguments gives: no device at all, or a refused handle"""
    return ERR_NO_DEVICE if mcpt.device_count() <= 0 else ERR_ARG


def test_lens_symbols_are_declared_and_exported(mcpt):
    from montecarlopathtracing_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for sym in NAMES:
        assert (sym + "(") in hdr and sym in _lib.EXPORTS and hasattr(L, sym), sym
    assert "#define MCPT_LENS_JITTER      1" in hdr and "#define MCPT_LENS_PER_SAMPLE  2" in hdr
    assert mcpt.LENS_JITTER == 1 and mcpt.LENS_PER_SAMPLE == 2
    assert "} mcpt_lens;" in hdr
    assert mcpt.lib().mcpt_version() == 105


def test_lens_layout_matches_the_header(mcpt, tmp_path):
    from montecarlopathtracing_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [n for n, _ in _lib.Lens._fields_]
    assert fields == ["flags", "reserved", "aperture", "focus_distance"]
    src = tmp_path / "layout_lens.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"mcpt.h\"\nint main(void) {\n  printf(\"%zu\\n\", sizeof(mcpt_lens));\n"
                   + "".join("  printf(\"%%zu\\n\", offsetof(mcpt_lens, %s));\n" % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout_lens"
    subprocess.check_call([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert out[0] == C.sizeof(_lib.Lens) == 24
    for i, f in enumerate(fields):
        assert out[1 + i] == getattr(_lib.Lens, f).offset, f


BAD_LENSES = [(4, 0, 0.0, 0.0), (-1, 0, 0.0, 0.0), (0, 1, 0.0, 0.0), (0, 0, -1e-300, 0.0), (0, 0, float("nan"), 0.0),
              (0, 0, float("inf"), 0.0), (0, 0, 0.1, float("nan")), (0, 0, 0.1, float("inf")), (1, 0, 0.1, float("-inf"))]
GOOD_LENSES = [(0, 0, 0.0, 0.0), (1, 0, 0.0, 0.0), (2, 0, 0.0, 0.0), (3, 0, 0.5, 2.0), (1, 0, 0.1, -3.0)]


def test_argument_errors_with_a_null_device(mcpt):
    L = mcpt.lib()
    nd = _null_device_rc(mcpt)
    for f, r, a, fd in BAD_LENSES:
        lens = mcpt.Lens(f, r, a, fd)
        assert L.mcpt_device_set_lens(None, C.byref(lens)) == ERR_ARG, (f, r, a, fd)
        assert L.mcpt_multi_set_lens(None, C.byref(lens)) == ERR_ARG, (f, r, a, fd)
    for f, r, a, fd in GOOD_LENSES:
        lens = mcpt.Lens(f, r, a, fd)
        assert L.mcpt_device_set_lens(None, C.byref(lens)) == nd
        assert L.mcpt_multi_set_lens(None, C.byref(lens)) == nd
    assert L.mcpt_device_set_lens(None, None) == nd                # NULL lens: the pinhole
    assert L.mcpt_device_get_lens(None, None) == ERR_ARG
    out = mcpt.Lens()
    assert L.mcpt_device_get_lens(None, C.byref(out)) == nd
    pix = np.zeros(4, dtype=np.int32)
    rays = np.zeros((4, 6))
    P32 = C.POINTER(C.c_int32)
    PD = C.POINTER(C.c_double)
    ok = (pix.ctypes.data_as(P32), pix.ctypes.data_as(P32), 4, rays.ctypes.data_as(PD))
    assert L.mcpt_camera_rays(None, 0, *ok) == nd
    assert L.mcpt_camera_rays(None, 0, None, ok[1], 4, ok[3]) == ERR_ARG
    assert L.mcpt_camera_rays(None, 0, ok[0], None, 4, ok[3]) == ERR_ARG
    assert L.mcpt_camera_rays(None, 0, ok[0], ok[1], 4, None) == ERR_ARG
    assert L.mcpt_camera_rays(None, 0, ok[0], ok[1], -1, ok[3]) == ERR_ARG


@pytest.mark.parametrize("lens", BAD_LENSES)
def test_render_scene_refuses_invalid_lenses_before_writing(mcpt, tmp_path, lens):
    ckpt = tmp_path / "frame.ckpt"
    for kw in ({}, {"checkpoint": str(ckpt)}, {"noise_target": 0.1}, {"devices": [0, 0]}):
        with pytest.raises(mcpt.McptError) as e:
            mcpt.render_scene(SCENES, "cornell-box", 4, width=16, height=9, output_prefix=str(tmp_path / "out"), lens=mcpt.Lens(*lens), **kw)
        assert e.value.code == ERR_ARG, (lens, kw)
        assert os.listdir(tmp_path) == [], (lens, kw)


def test_render_scene_lens_argument_forms(mcpt, tmp_path):
    """valid lenses reach the device (or the missing one); a dict is a Device.set_lens argument list"""
    if mcpt.device_count() > 0:
        pytest.skip("renders on a GPU: tests/test_gpu_lens.py")
    for lens in (mcpt.make_lens(0.1, jitter=True), {"aperture": 0.0, "per_sample": True}, mcpt.Lens()):
        with pytest.raises(mcpt.McptError) as e:
            mcpt.render_scene(SCENES, "cornell-box", 4, width=16, height=9, output_prefix=str(tmp_path / "out"), lens=lens)
        assert e.value.code == ERR_NO_DEVICE
    l = mcpt.make_lens(0.25, 3.0, jitter=True, per_sample=True)
    assert (l.flags, l.reserved, l.aperture, l.focus_distance) == (3, 0, 0.25, 3.0)


def test_camera_uniforms_are_the_rng_seam(oracle):
    rng = np.random.default_rng(1)
    pix = rng.integers(0, 1 << 20, size=64)
    k = rng.integers(0, 4096, size=64)
    for seed in (0, 7, 0x1234567890ABCDEF):
        u = lens_ref.camera_uniforms(seed, pix, k)
        for i in range(64):
            for slot in range(4):
                assert u[slot][i] == oracle.uniform(seed, int(pix[i]), int(k[i]), 0xFFFF, slot)


@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_inactive_lens_is_the_oracles_primary_ray(mcpt, oracle, name):
    """pinhole, no jitter: lens_ref.camera_ray = orc_primary_ray bit for bit on every pixel (pins the restatement's frame and corners)"""
    W, H = 64, 36
    sc = mcpt.Scene(SCENES, name, width=W, height=H)
    cam = lens_ref.Camera.from_info(sc.info)
    osc = oracle.OracleScene(SCENES + name, texture_dir=SCENES, width=W, height=H)
    want = osc.primary_rays()
    pix = np.arange(W * H)
    for k in (0, 5):
        got = lens_ref.camera_ray(cam, 3, pix, np.full(pix.shape, k))
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), np.abs(got - want).max()
    # jitter stays inside the pixel square; the thin lens's origins on the disk of radius aperture about the eye
    got = lens_ref.camera_ray(cam, 3, pix, np.zeros_like(pix), aperture=0.05, focus_distance=2.0, jitter=True)
    off = got[:, :3] - np.array(cam.eye)
    skew = abs(float(np.dot(cam.xhat, cam.up)))       # (x^ and y^ need not be orthogonal: |o - eye|^2 <= r^2 (1 + |x^.y^|))
    assert np.all(np.sqrt((off * off).sum(axis=1)) <= 0.05 * np.sqrt(1 + skew) * (1 + 1e-12))
    sc.close()
