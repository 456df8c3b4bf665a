"""Not gpu: the C-ABI surface of adaptive frames -- symbols, argument errors with and without a device, render_scene's refusals, and the
new structs as ctypes sees them against the C compiler's layout."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conftest import ROOT, SCENES

ERR_ARG, ERR_NO_DEVICE = -3, -4
NAMES = ["mcpt_progressive_create_adaptive", "mcpt_progressive_active", "mcpt_progressive_active_pixels", "mcpt_progressive_sample_counts"]


def test_adaptive_symbols_are_declared_and_exported(mcpt):
    from montecarlopathtracing_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for sym in NAMES:
        assert (sym + "(") in hdr and sym in _lib.EXPORTS and hasattr(L, sym), sym
    assert "MCPT_OUT_SPP_PFM      8" in hdr and mcpt.OUT_SPP_PFM == 8
    assert "mcpt_adaptive_params;" in hdr


def _create(mcpt, rel=0.05, ab=0.0, min_spp=16, spp=64, params=True, rp=True):
    rpar = mcpt.RenderParams(spp, 0, 0, 1, 0, 0, 0)
    ap = mcpt.AdaptiveParams(rel, ab, min_spp, 0)
    h = C.c_void_p()
    rc = mcpt.lib().mcpt_progressive_create_adaptive(None, C.byref(rpar) if rp else None, C.byref(ap) if params else None, C.byref(h))
    assert not h.value
    return rc


def test_create_without_a_device(mcpt):
    """valid arguments: no HIP device -> MCPT_ERR_NO_DEVICE; on a GPU machine the null device is the bad argument"""
    want = ERR_NO_DEVICE if mcpt.device_count() == 0 else ERR_ARG
    assert _create(mcpt) == want
    assert _create(mcpt, rel=0.0, ab=0.0, min_spp=2) == want
    assert _create(mcpt, min_spp=1000) == want             # above N: clamped, not refused


@pytest.mark.parametrize("kw", [dict(rel=-0.01), dict(ab=-1.0), dict(rel=float("nan")), dict(ab=float("nan")), dict(rel=float("inf")),
                                dict(ab=float("inf")), dict(min_spp=1), dict(min_spp=0), dict(min_spp=-4), dict(spp=0), dict(spp=-8),
                                dict(params=False), dict(rp=False)])
def test_argument_errors_on_any_machine(mcpt, kw):
    assert _create(mcpt, **kw) == ERR_ARG


def test_null_out_and_null_handles(mcpt):
    L = mcpt.lib()
    rp = mcpt.RenderParams(64, 0, 0, 1, 0, 0, 0)
    ap = mcpt.AdaptiveParams(0.05, 0.0, 16, 0)
    assert L.mcpt_progressive_create_adaptive(None, C.byref(rp), C.byref(ap), None) == ERR_ARG
    assert L.mcpt_progressive_active(None) == ERR_ARG
    assert L.mcpt_progressive_active_pixels(None, None) == ERR_ARG
    buf = (C.c_int32 * 4)()
    assert L.mcpt_progressive_active_pixels(None, buf) == ERR_ARG
    assert L.mcpt_progressive_sample_counts(None, buf) == ERR_ARG
    assert L.mcpt_progressive_sample_counts(None, None) == ERR_ARG


@pytest.mark.parametrize("kw", [dict(adaptive_min_spp=16, checkpoint="x.ckpt"), dict(adaptive_min_spp=16, devices=-1),
                                dict(adaptive_min_spp=16, devices=[0]), dict(adaptive_min_spp=16, noise_target=0.05, checkpoint="y.ckpt"),
                                dict(adaptive_min_spp=1), dict(adaptive_min_spp=-2), dict(adaptive_min_spp=16, abs_target=-1.0),
                                dict(adaptive_min_spp=16, abs_target=float("nan")), dict(adaptive_min_spp=16, noise_target=float("inf"))])
def test_render_scene_refuses_adaptive_combinations(mcpt, tmp_path, kw):
    """checkpoints, several GPUs and bad targets: refused before anything is loaded or written"""
    with pytest.raises(mcpt.McptError) as e:
        mcpt.render_scene(SCENES, "cornell-box", 16, output_prefix=str(tmp_path / "x"), **kw)
    assert e.value.code == ERR_ARG
    assert os.listdir(tmp_path) == []


def _offsets(tmp_path, struct, fields, cls):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / ("layout_%s.c" % struct)
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"mcpt.h\"\nint main(void) {\n"
                   "  printf(\"%%zu\\n\", sizeof(%s));\n" % struct
                   + "".join("  printf(\"%%zu\\n\", offsetof(%s, %s));\n" % (struct, f) for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / ("layout_%s" % struct)
    subprocess.check_call([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert out[0] == C.sizeof(cls), struct
    for i, f in enumerate(fields):
        assert out[1 + i] == getattr(cls, f).offset, (struct, f)


def test_struct_layouts_match_the_header(mcpt, tmp_path):
    from montecarlopathtracing_amd import _lib
    _offsets(tmp_path, "mcpt_adaptive_params", [n for n, _ in _lib.AdaptiveParams._fields_], _lib.AdaptiveParams)
    _offsets(tmp_path, "mcpt_render_scene_options", [n for n, _ in _lib.RenderSceneOptions._fields_], _lib.RenderSceneOptions)
    assert C.sizeof(_lib.AdaptiveParams) == 24
    names = [n for n, _ in _lib.RenderSceneOptions._fields_]
    assert names[-3:] == ["adaptive_min_spp", "reserved2", "abs_target"]
