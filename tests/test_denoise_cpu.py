"""Not gpu: the C-ABI surface of the first-hit AOVs and the denoiser (symbols, the parameter struct against the C compiler's layout,
argument errors without a device, render_scene's refusals), and the numpy restatement of the filter (tests/denoise_ref.py) against
hand computations on synthetic frames."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_ref as R
from conftest import ROOT, SCENES
from test_adaptive_cpu import _offsets

ERR_ARG = -3
NAMES = ["mcpt_progressive_aovs", "mcpt_progressive_denoise", "mcpt_progressive_denoise_device"]


def test_denoise_symbols_are_declared_and_exported(mcpt):
    from montecarlopathtracing_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for sym in NAMES:
        assert (sym + "(") in hdr and sym in _lib.EXPORTS and hasattr(L, sym), sym
    assert "MCPT_OUT_DENOISED    16" in hdr and mcpt.OUT_DENOISED == 16
    assert "MCPT_OUT_AOV_PFM     32" in hdr and mcpt.OUT_AOV_PFM == 32
    assert "THE DENOISED IMAGE IS BIASED" in hdr


def test_denoise_params_layout_matches_the_header(mcpt, tmp_path):
    from montecarlopathtracing_amd import _lib
    _offsets(tmp_path, "mcpt_denoise_params", [n for n, _ in _lib.DenoiseParams._fields_], _lib.DenoiseParams)
    assert C.sizeof(_lib.DenoiseParams) == 24


@pytest.mark.parametrize("dp", [None, (0, 0, 0.0, 0.0), (11, 0, 0.0, 0.0), (-1, 0, 0.0, 0.0), (5, 1, 0.0, 0.0), (5, 0, -1.0, 0.0),
                                (5, 0, 0.0, float("nan")), (5, 0, float("inf"), 0.0)])
def test_null_handle_and_bad_parameters(mcpt, dp):
    L = mcpt.lib()
    p = C.byref(mcpt.DenoiseParams(*dp)) if dp is not None else None
    img = np.zeros(12)
    ptr = img.ctypes.data_as(C.POINTER(C.c_double))
    assert L.mcpt_progressive_denoise(None, p, ptr) == ERR_ARG
    assert L.mcpt_progressive_denoise(None, p, None) == ERR_ARG
    assert L.mcpt_progressive_denoise_device(None, p, None, None) == ERR_ARG
    assert L.mcpt_progressive_aovs(None, None, None, None, None) == ERR_ARG


@pytest.mark.parametrize("kw", [dict(output_flags=16, checkpoint="x.ckpt"), dict(output_flags=32, devices=-1),
                                dict(output_flags=16 | 32, devices=[0]), dict(output_flags=32, checkpoint="y.ckpt")])
def test_render_scene_refuses_denoise_combinations(mcpt, tmp_path, kw):
    """the flags make the frame progressive: checkpoints and several GPUs are refused before anything is loaded or written"""
    with pytest.raises(mcpt.McptError) as e:
        mcpt.render_scene(SCENES, "cornell-box", 16, output_prefix=str(tmp_path / "x"), **kw)
    assert e.value.code == ERR_ARG
    assert os.listdir(tmp_path) == []


def test_render_scene_refuses_denoising_one_sample(mcpt, tmp_path):
    with pytest.raises(mcpt.McptError) as e:
        mcpt.render_scene(SCENES, "cornell-box", 1, output_prefix=str(tmp_path / "x"), output_flags=16)
    assert e.value.code == ERR_ARG
    assert os.listdir(tmp_path) == []


def _frame(h, w, rng, value=None):
    est = rng.random((h, w, 3)) if value is None else np.full((h, w, 3), value)
    se2 = rng.random((h, w, 3)) * 1e-3
    normal = np.zeros((h, w, 3))
    normal[..., 2] = 1.0
    depth = np.full((h, w), 3.0)
    albedo = np.full((h, w, 3), 0.5)
    smat = np.zeros((h, w), dtype=np.int64)
    return est, se2, smat, normal, depth, albedo


def test_constant_frame_comes_back_unchanged():
    est, se2, smat, normal, depth, albedo = _frame(37, 53, np.random.default_rng(1), value=0.3)
    out = R.denoise(est, se2, smat, normal, depth, albedo, iterations=5)
    assert np.allclose(out, est, rtol=1e-14, atol=0.0)          # a few ulps: five rounds of weighted means


def test_step_across_two_materials_is_kept_exactly():
    """left and right halves of two materials, constant within each: no tap crosses the edge, and with power-of-two values (albedo 1)
    every weighted mean is exact"""
    h, w = 24, 40
    est, se2, smat, normal, depth, albedo = _frame(h, w, np.random.default_rng(2), value=0.25)
    est[:, w // 2:] = 2.0
    smat[:, w // 2:] = 1
    albedo[:] = 1.0
    out = R.denoise(est, se2, smat, normal, depth, albedo, iterations=5)
    assert np.array_equal(out.view(np.uint64), est.view(np.uint64))
    # the same frame as one material: the edge blurs
    blurred = R.denoise(est, se2, np.zeros_like(smat), normal, depth, albedo, iterations=5, sigma_l=1e6)
    assert not np.array_equal(blurred, est)


def test_no_iterations_is_the_input_bit_for_bit():
    est, se2, smat, normal, depth, albedo = _frame(9, 11, np.random.default_rng(3))
    out = R.denoise(est, se2, smat, normal, depth, albedo, iterations=0)
    assert np.array_equal(out.view(np.uint64), est.view(np.uint64))


def test_non_surface_pixels_pass_through_and_are_not_neighbours():
    est, se2, smat, normal, depth, albedo = _frame(16, 16, np.random.default_rng(4))
    smat[5, 7] = -1
    smat[0, :] = -1
    out = R.denoise(est, se2, smat, normal, depth, albedo, iterations=3)
    assert np.array_equal(out[5, 7], est[5, 7]) and np.array_equal(out[0], est[0])
    est2 = est.copy()
    est2[5, 7] = 1e9
    est2[0, :] = -1e9
    assert np.array_equal(R.denoise(est2, se2, smat, normal, depth, albedo, iterations=3)[smat >= 0], out[smat >= 0])


def test_variance_update_on_a_5x5_frame_by_hand():
    """one material, equal normals and depths, a constant colour (L = 0): every tap inside the frame weighs h[dx] h[dy].  At the centre
    all 25 taps count (sum w = 1); at a corner the 3 x 3 inside the frame (sum w = (11/16)^2)."""
    rng = np.random.default_rng(5)
    est, se2, smat, normal, depth, albedo = _frame(5, 5, rng, value=0.4)
    _, e, v = R.denoise(est, se2, smat, normal, depth, albedo, iterations=1, state=True)
    a = np.maximum(albedo, 0.01)
    v0 = sum(((R.LUM[c] * R.LUM[c]) * se2[..., c]) / (a[..., c] * a[..., c]) for c in range(3))
    h = R.H5
    centre = sum((h[dx + 2] * h[dy + 2]) ** 2 * v0[2 + dy, 2 + dx] for dy in range(-2, 3) for dx in range(-2, 3))
    assert v[2, 2] == pytest.approx(centre, rel=1e-15)
    sw = sum(h[dx + 2] * h[dy + 2] for dy in range(0, 3) for dx in range(0, 3))
    assert sw == pytest.approx((11 / 16) ** 2, rel=1e-15)
    corner = sum((h[dx + 2] * h[dy + 2]) ** 2 * v0[dy, dx] for dy in range(0, 3) for dx in range(0, 3)) / (sw * sw)
    assert v[0, 0] == pytest.approx(corner, rel=1e-15)
    assert np.allclose(e, 0.4 / 0.5, rtol=4e-16, atol=0.0)


def test_edge_stops_hold_a_noisy_frame_back():
    """depth and normal terms: a pixel whose depth or normal differs by a lot takes (almost) nothing from its neighbours"""
    rng = np.random.default_rng(6)
    est, se2, smat, normal, depth, albedo = _frame(12, 12, rng)
    depth[6, 6] = 0.3                       # D = 2.7 / (0.05 * 0.3) = 180 against every neighbour
    out = R.denoise(est, se2, smat, normal, depth, albedo, iterations=1)
    assert out[6, 6] == pytest.approx(est[6, 6], rel=1e-12)
    depth[6, 6] = 3.0
    normal[3, 3] = (0.0, 1.0, 0.0)
    out = R.denoise(est, se2, smat, normal, depth, albedo, iterations=1)
    assert np.allclose(out[3, 3], est[3, 3], rtol=1e-12)
