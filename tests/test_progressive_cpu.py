"""Not gpu: the C-ABI surface of progressive frames -- symbols, argument errors without a device, the render_scene options as ctypes sees
them against the C compiler's layout, and the pass schedule (mcpt_progressive_next_pass, a pure function)."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conftest import ROOT, SCENES

ERR_ARG, ERR_NO_DEVICE = -3, -4
NAMES = ["mcpt_progressive_create", "mcpt_progressive_step", "mcpt_progressive_done", "mcpt_progressive_noise", "mcpt_progressive_image",
         "mcpt_progressive_image_device", "mcpt_progressive_next_pass", "mcpt_progressive_free"]


def test_progressive_symbols_are_declared_and_exported(mcpt):
    from montecarlopathtracing_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for sym in NAMES:
        assert (sym + "(") in hdr and sym in _lib.EXPORTS and hasattr(L, sym), sym
    assert "MCPT_OUT_ERROR_PFM    4" in hdr and mcpt.OUT_ERROR_PFM == 4


def test_argument_errors_without_a_device(mcpt):
    L = mcpt.lib()
    rp = mcpt.RenderParams(64, 0, 0, 1, 0, 0, 0)
    h = C.c_void_p()
    rc = L.mcpt_progressive_create(None, C.byref(rp), C.byref(h))
    assert rc == (ERR_NO_DEVICE if mcpt.device_count() == 0 else ERR_ARG) and not h.value
    assert L.mcpt_progressive_create(None, None, C.byref(h)) == ERR_ARG
    assert L.mcpt_progressive_step(None, 8, None) == ERR_ARG
    assert L.mcpt_progressive_step(None, 0, None) == ERR_ARG
    assert L.mcpt_progressive_step(None, -1, None) == ERR_ARG
    assert L.mcpt_progressive_done(None) == ERR_ARG
    assert L.mcpt_progressive_noise(None, C.byref(mcpt.Noise())) == ERR_ARG
    assert L.mcpt_progressive_image(None, None, None) == ERR_ARG
    assert L.mcpt_progressive_image_device(None, None, None, None) == ERR_ARG
    L.mcpt_progressive_free(None)


@pytest.mark.parametrize("kw", [dict(noise_target=0.01, checkpoint="x.ckpt"), dict(time_budget_s=1.0, devices=-1),
                                dict(output_flags=4, devices=[0]), dict(noise_target=-1.0), dict(time_budget_s=float("nan"))])
def test_render_scene_refuses_progressive_combinations(mcpt, tmp_path, kw):
    """checkpoints and several GPUs are out of the progressive path's scope: refused before anything is loaded or rendered"""
    with pytest.raises(mcpt.McptError) as e:
        mcpt.render_scene(SCENES, "cornell-box", 16, output_prefix=str(tmp_path / "x"), **kw)
    assert e.value.code == ERR_ARG
    assert os.listdir(tmp_path) == []


def test_render_scene_options_layout_matches_the_header(mcpt, tmp_path):
    from montecarlopathtracing_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [n for n, _ in _lib.RenderSceneOptions._fields_]
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"mcpt.h\"\nint main(void) {\n"
                   "  printf(\"%zu\\n\", sizeof(mcpt_render_scene_options));\n"
                   + "".join("  printf(\"%%zu\\n\", offsetof(mcpt_render_scene_options, %s));\n" % f for f in fields)
                   + "  printf(\"%zu %zu\\n\", sizeof(mcpt_noise), offsetof(mcpt_noise, sum_mean2));\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    assert int(out[0]) == C.sizeof(_lib.RenderSceneOptions)
    for i, f in enumerate(fields):
        assert int(out[1 + i]) == getattr(_lib.RenderSceneOptions, f).offset, f
    size, off = (int(v) for v in out[1 + len(fields)].split())
    assert size == C.sizeof(_lib.Noise) and off == _lib.Noise.sum_mean2.offset


INF = float("inf")


@pytest.mark.parametrize("spp, done, remaining, rate, want", [
    # doubling: 8, then min(N - done, done)
    (256, 0, INF, 0.0, 8), (256, 8, INF, 0.0, 8), (256, 16, INF, 0.0, 16), (256, 32, INF, 0.0, 32), (256, 64, INF, 0.0, 64),
    (256, 128, INF, 0.0, 128), (256, 256, INF, 0.0, 0),
    # clipped at N
    (5, 0, INF, 0.0, 5), (64, 8, INF, 0.0, 8), (20, 16, INF, 0.0, 4), (100, 64, INF, 0.0, 36), (1, 0, INF, 0.0, 1), (64, 64, INF, 0.0, 0),
    (64, 70, INF, 0.0, 0), (0, 0, INF, 0.0, 0), (64, -1, INF, 0.0, 0),
    # the time cap: floor(remaining / rate) from the second pass on
    (256, 32, 1.0, 0.0625, 16), (256, 32, 10.0, 0.0625, 32), (256, 32, 0.125, 0.0625, 2), (256, 64, 4.0, 0.0625, 64),
    (256, 64, 3.9375, 0.0625, 63), (256, 32, 0.1, 0.0625, 1), (256, 8, 1.0, 0.0, 8),
    # ... and the stop
    (256, 32, 0.03125, 0.0625, 0), (256, 32, 0.0, 0.0625, 0), (256, 32, -1.0, 0.0625, 0), (256, 32, float("nan"), 0.0625, 0),
    # the first pass is not capped (no rate yet; a frame needs one pass)
    (256, 0, 1e-9, 0.0, 8), (256, 0, -1.0, 1.0, 8),
])
def test_next_pass_schedule(mcpt, spp, done, remaining, rate, want):
    assert mcpt.progressive_next_pass(spp, done, remaining, rate) == want


def test_schedule_of_the_headline_frame(mcpt):
    done, passes = 0, []
    while True:
        n = mcpt.progressive_next_pass(256, done)
        if n == 0:
            break
        passes.append(n)
        done += n
    assert passes == [8, 8, 16, 32, 64, 128] and done == 256
