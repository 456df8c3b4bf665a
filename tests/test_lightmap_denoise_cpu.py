"""CPU: the lightmap denoiser without a device (include/mcpt.h: lightmap denoising).  The symbols, the struct's layout, the refusals and
their order; and the numpy restatement (tests/lightmap_denoise_ref.py) alone, on cases whose answer is known without a GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import lightmap_denoise_ref as DR
import lightmap_ref as R
from conftest import ROOT

ERR_ARG, ERR_NO_DEVICE = -3, -4
NAMES = ["mcpt_lightmap_denoise", "mcpt_lightmap_denoise_device"]
PD, P32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _null_device_rc(mcpt):
    """what a null handle with valid arguments gives: no device at all, or a refused handle"""
    return ERR_NO_DEVICE if mcpt.device_count() <= 0 else ERR_ARG


def _message(mcpt):
    return mcpt.lib().mcpt_last_error().decode()


def test_denoise_symbols_are_declared_and_exported(mcpt):
    from montecarlopathtracing_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for sym in NAMES:
        assert (sym + "(") in hdr and sym in _lib.EXPORTS and hasattr(L, sym), sym
    assert "} mcpt_lightmap_denoise_params;" in hdr and "THE DENOISED MAP IS BIASED" in hdr and "ESSENTIALLY UNFILTERED" in hdr
    assert "about 128 bytes per texel" in hdr
    assert "#define MCPT_VERSION 105" in hdr and mcpt.lib().mcpt_version() == 105
    for name, value in (("ITERATIONS", mcpt.LIGHTMAP_DENOISE_ITERATIONS), ("MAX_ITERATIONS", mcpt.LIGHTMAP_DENOISE_MAX_ITERATIONS),
                        ("SIGMA_L", mcpt.LIGHTMAP_DENOISE_SIGMA_L), ("SIGMA_P", mcpt.LIGHTMAP_DENOISE_SIGMA_P)):
        line = [l for l in hdr.splitlines() if l.startswith("#define MCPT_LIGHTMAP_DENOISE_" + name + " ")]
        assert len(line) == 1 and float(line[0].split()[2]) == value, name
    assert DR.DEFAULTS == dict(iterations=mcpt.LIGHTMAP_DENOISE_ITERATIONS, sigma_l=mcpt.LIGHTMAP_DENOISE_SIGMA_L, sigma_p=mcpt.LIGHTMAP_DENOISE_SIGMA_P)
    assert callable(mcpt.Device.denoise_lightmap)


def test_denoise_params_layout_matches_the_header(mcpt, tmp_path):
    from montecarlopathtracing_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [n for n, _ in _lib.LightmapDenoiseParams._fields_]
    assert fields == ["width", "height", "iterations", "dilate", "sigma_l", "sigma_p", "reserved"]
    src = tmp_path / "layout_lightmap_denoise.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"mcpt.h\"\nint main(void) {\n  printf(\"%zu\\n\", sizeof(mcpt_lightmap_denoise_params));\n"
                   + "".join("  printf(\"%%zu\\n\", offsetof(mcpt_lightmap_denoise_params, %s));\n" % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout_lightmap_denoise"
    subprocess.check_call([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert out[0] == C.sizeof(_lib.LightmapDenoiseParams) == 40
    for i, f in enumerate(fields):
        assert out[1 + i] == getattr(_lib.LightmapDenoiseParams, f).offset, f


def _dp(mcpt, width=8, height=8, iterations=5, dilate=0, sigma_l=0.0, sigma_p=0.0, reserved=(0, 0)):
    return mcpt.LightmapDenoiseParams(width, height, iterations, dilate, sigma_l, sigma_p, (C.c_int32 * 2)(*reserved))


NAN, INF = float("nan"), float("inf")
# (what the message must mention, keyword overrides), in the documented order of refusal
BAD_PARAMS = [("width", dict(width=0)), ("width", dict(width=16385)), ("width", dict(height=0)), ("width", dict(height=-5)), ("width", dict(height=16385)),
              ("iterations", dict(iterations=-1)), ("iterations", dict(iterations=11)),
              ("dilate", dict(dilate=-1)), ("dilate", dict(dilate=65)),
              ("sigma_l", dict(sigma_l=-1.0)), ("sigma_l", dict(sigma_l=NAN)), ("sigma_l", dict(sigma_l=INF)),
              ("sigma_p", dict(sigma_p=-1e-300)), ("sigma_p", dict(sigma_p=NAN)), ("sigma_p", dict(sigma_p=-INF)),
              ("reserved", dict(reserved=(1, 0))), ("reserved", dict(reserved=(0, -1)))]


def test_refusals_come_in_order_and_before_the_missing_device(mcpt):
    L = mcpt.lib()
    nd = _null_device_rc(mcpt)
    uv = R.shared_chart()
    E, S, O = np.ones((8, 8, 3)), np.ones((8, 8, 3)), np.zeros((8, 8, 3))

    def host(dp, uv6=uv, irr=E, err=S, out=O):
        p = lambda a: a.ctypes.data_as(PD) if a is not None else None
        return L.mcpt_lightmap_denoise(None, p(uv6), C.byref(dp) if dp is not None else None, p(irr), p(err), p(out), None)

    def device(dp, uv6=uv, irr=E, err=S, out=O):
        p = lambda a: a.ctypes.data if a is not None else None
        return L.mcpt_lightmap_denoise_device(None, p(uv6), C.byref(dp) if dp is not None else None, p(irr), p(err), p(out), None, None)

    for what, kw in BAD_PARAMS:
        for call in (host, device):
            assert call(_dp(mcpt, **kw)) == ERR_ARG, kw
            assert what in _message(mcpt), (kw, _message(mcpt))
    # the order: each refusal is reported although everything after it is wrong as well
    order = [("width", dict(width=0)), ("iterations", dict(iterations=11)), ("dilate", dict(dilate=65)), ("sigma_l", dict(sigma_l=-1.0)),
             ("sigma_p", dict(sigma_p=NAN)), ("reserved", dict(reserved=(0, 1)))]
    for i, (what, _) in enumerate(order):
        kw = {}
        for _, later in order[i:]:
            kw.update(later)
        for call in (host, device):
            assert call(_dp(mcpt, **kw), irr=None, err=None, out=None) == ERR_ARG and what in _message(mcpt), (what, _message(mcpt))
    for call in (host, device):
        assert call(None, irr=None) == ERR_ARG and "parameters" in _message(mcpt)
        assert call(_dp(mcpt), irr=None, err=None, out=None) == ERR_ARG and "irradiance" in _message(mcpt)
        assert call(_dp(mcpt), err=None, out=None) == ERR_ARG and "stderr" in _message(mcpt)
        assert call(_dp(mcpt), out=None) == ERR_ARG and "output" in _message(mcpt)
    # valid arguments: the missing device (or the refused null handle) is what is left to report
    for kw in (dict(), dict(iterations=0), dict(iterations=10), dict(dilate=64), dict(width=16384, height=1), dict(sigma_l=8.0, sigma_p=0.25)):
        assert host(_dp(mcpt, **kw)) == nd and device(_dp(mcpt, **kw)) == nd, kw
        assert host(_dp(mcpt, **kw), uv6=None) == nd, kw
    assert host(_dp(mcpt), out=E) == nd and device(_dp(mcpt), out=E) == nd          # out3 may be irradiance3


# ---- the restatement alone

def _quads(gap, W=32, H=16):
    v, vn, uv = DR.two_quads(gap)
    g = DR.faces27_of(v, vn, uv)
    owner = R.raster(uv, W, H, g[:, 24:27])
    return uv, g, owner


def test_restatement_guides_of_a_plain_chart():
    """two unit quads, each on half of a 32 x 16 map: every texel is covered, a texel's side is 1/16 of a world unit, positions are the
    texel centres and normals +y"""
    uv, g, owner = _quads(1.0)
    cov, p, nhat, h = DR.guides(owner, uv, g)
    assert cov.all() and set(np.unique(owner)) == {0, 1, 2, 3}
    np.testing.assert_allclose(h, 1.0 / 16.0, rtol=1e-15)
    pu, pv = R.centres(32, 16)
    np.testing.assert_allclose(p[..., 0], np.broadcast_to(2.0 * pu, (16, 32)), atol=1e-14)
    np.testing.assert_allclose(p[..., 2], np.broadcast_to(pv[:, None], (16, 32)), atol=1e-14)
    assert not p[..., 1].any() and np.array_equal(nhat, np.broadcast_to([0.0, 1.0, 0.0], (16, 32, 3)))


def test_restatement_k0_is_the_identity_on_covered_texels():
    uv = R.shared_chart()
    rng = np.random.default_rng(3)
    v, vn = rng.uniform(-1, 1, (uv.shape[0], 9)), rng.normal(size=(uv.shape[0], 9))
    g = DR.faces27_of(v, vn, uv)
    E, S = rng.uniform(0.1, 5.0, (41, 67, 3)), rng.uniform(0.01, 1.0, (41, 67, 3))
    out, own = DR.denoise(E, S, uv, g, iterations=0)
    cov = own >= 0
    assert cov.any() and (~cov).any()
    assert np.array_equal(_bits(out[cov]), _bits(E[cov]))
    assert not _bits(out[~cov]).any()                                             # +0.0, not -0.0
    assert np.array_equal(own, R.raster(uv, 67, 41, g[:, 24:27]))


def test_restatement_keeps_a_constant_map_constant():
    uv, g, owner = _quads(1.0)
    E = np.full((16, 32, 3), 1.0) * np.array([0.25, 1.0, 3.0])
    for S in (np.zeros_like(E), np.full_like(E, 0.3)):
        out, _ = DR.denoise(E, S, uv, g, iterations=5)
        np.testing.assert_allclose(out, E, rtol=1e-14)


def test_restatement_never_reads_a_texel_that_is_not_covered():
    uv = R.shared_chart()
    rng = np.random.default_rng(5)
    v, vn = rng.uniform(-1, 1, (uv.shape[0], 9)), rng.normal(size=(uv.shape[0], 9))
    g = DR.faces27_of(v, vn, uv)
    E, S = rng.uniform(0.1, 5.0, (41, 67, 3)), rng.uniform(0.01, 1.0, (41, 67, 3))
    a, own = DR.denoise(E, S, uv, g, iterations=5, dilate=2)
    E2, S2 = E.copy(), S.copy()
    E2[own == -1] = NAN; E2[own < -1] = 1e300
    S2[own == -1] = 1e300; S2[own < -1] = NAN
    assert (own == -1).any() and (own < -1).any()
    b, own2 = DR.denoise(E2, S2, uv, g, iterations=5, dilate=2)
    assert np.array_equal(own, own2) and np.array_equal(_bits(a), _bits(b)) and np.isfinite(a).all()
    # ... and it did filter: covered texels with a covered neighbour on their own face moved
    cov = own >= 0
    assert (a[cov] != E[cov]).any()


def test_restatement_seam():
    """Charts that share a UV edge but lie 1000 quads apart do not mix, under a luminance stop that is wide open; side by side they do"""
    W, H = 32, 16
    E = np.ones((H, W, 3)); E[:, W // 2:] = 100.0
    S = np.full((H, W, 3), 1e6)
    uv, g, owner = _quads(1001.0)
    assert ((owner[:, :W // 2] == 0) | (owner[:, :W // 2] == 1)).all() and (owner[:, W // 2:] >= 2).all()
    out, _ = DR.denoise(E, S, uv, g, iterations=5)
    assert np.abs(out / E - 1.0).max() <= 1e-12
    uv, g, owner = _quads(1.0)
    out, _ = DR.denoise(E, S, uv, g, iterations=5)
    near = slice(W // 2 - 2, W // 2 + 2)
    assert (np.abs(out[:, near] - E[:, near]) > 1.0).all(), np.abs(out[:, near] - E[:, near]).min()
    print("leak at the shared edge, side by side: %.3g .. %.3g" % (np.abs(out[:, near] - E[:, near]).min(), np.abs(out[:, near] - E[:, near]).max()))


def test_restatement_normal_stop():
    """A floor and a wall charted contiguously: positions run on across the fold, the normals turn by a right angle, nothing leaks"""
    W, H = 32, 16
    v, vn, uv = DR.floor_and_wall()
    g = DR.faces27_of(v, vn, uv)
    E = np.ones((H, W, 3)); E[:, W // 2:] = 100.0
    out, own = DR.denoise(E, np.full((H, W, 3), 1e6), uv, g, iterations=5)
    assert (own >= 0).all() and np.abs(out / E - 1.0).max() <= 1e-12


@pytest.mark.parametrize("size", [(1, 1), (3, 5), (5, 3)], ids=lambda s: "%dx%d" % s)
def test_restatement_on_a_map_smaller_than_the_largest_step(size):
    """K = 10 reaches step 512: every tap but the centre's leaves the map, and the answer stays a weighted mean of the inputs"""
    W, H = size
    uv, g, owner = _quads(1.0, W, H)
    rng = np.random.default_rng(8)
    E, S = rng.uniform(0.5, 2.0, (H, W, 3)), rng.uniform(0.05, 0.5, (H, W, 3))
    out, own = DR.denoise(E, S, uv, g, iterations=10)
    assert (own >= 0).all() and np.isfinite(out).all()
    assert (out >= E.min(axis=(0, 1)) - 1e-12).all() and (out <= E.max(axis=(0, 1)) + 1e-12).all()
    if size == (1, 1):
        assert np.array_equal(_bits(out), _bits(E * 1.0)) or np.abs(out / E - 1.0).max() <= 1e-15
