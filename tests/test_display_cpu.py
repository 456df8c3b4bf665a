"""Not gpu: the display transform's C-ABI surface and its host form -- symbols, struct layouts against the C compiler, mcpt_display_host
against imshow's bytes and against the numpy restatement (tests/display_ref.py), mcpt_display_exposure on hand-built histograms, and every
refusal."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import display_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mcpt_display_histogram_device", "mcpt_display_histogram", "mcpt_display_exposure", "mcpt_display_device", "mcpt_display",
       "mcpt_display_host", "mcpt_progressive_display", "mcpt_progressive_display_device", "mcpt_render_scene_display"]
ERR_ARG = -3
CURVES = {"clamp": DR.CLAMP, "reinhard": DR.REINHARD, "filmic": DR.FILMIC}
EXPOSURES = (1.0, 0.18, 4.0)
W, H = 160, 90


@pytest.fixture(scope="module")
def frame():
    return DR.log_uniform_frame(H, W, 20240607)


def test_symbols_are_declared_and_exported(mcpt):
    from montecarlopathtracing_amd import _lib
    L = mcpt.lib()
    hdr = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    for sym in NEW:
        assert (sym + "(") in hdr and sym in _lib.EXPORTS and hasattr(L, sym), sym
    for t in ("} mcpt_display_params;", "} mcpt_display_info;", "#define MCPT_DISPLAY_BINS   384", "#define MCPT_DISPLAY_SLOTS  387"):
        assert t in hdr
    assert L.mcpt_version() == 105 and "#define MCPT_VERSION 105" in hdr
    assert (mcpt.DISPLAY_BINS, mcpt.DISPLAY_SLOTS) == (DR.BINS, DR.SLOTS)


def test_struct_layouts_match_the_header(tmp_path):
    from montecarlopathtracing_amd import _lib
    structs = {"mcpt_display_params": _lib.DisplayParams, "mcpt_display_info": _lib.DisplayInfo}
    lines = []
    for name, cls in structs.items():
        lines.append("  printf(\"%%zu\\n\", sizeof(%s));\n" % name)
        lines += ["  printf(\"%%zu\\n\", offsetof(%s, %s));\n" % (name, f) for f, _ in cls._fields_]
    consts = ["MCPT_CURVE_CLAMP", "MCPT_CURVE_REINHARD", "MCPT_CURVE_FILMIC", "MCPT_TRANSFER_LINEAR", "MCPT_TRANSFER_SRGB", "MCPT_DISPLAY_RGBA",
              "MCPT_DISPLAY_ESTIMATE", "MCPT_DISPLAY_DENOISED", "MCPT_DISPLAY_DENOISED_GUIDED"]
    lines += ["  printf(\"%%d\\n\", %s);\n" % c for c in consts]
    src = tmp_path / "layout_display.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"mcpt.h\"\nint main(void) {\n" + "".join(lines) + "  return 0;\n}\n")
    exe = tmp_path / "layout_display"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = list(map(int, subprocess.check_output([str(exe)]).split()))
    want = []
    for cls in structs.values():
        want.append(C.sizeof(cls))
        want += [getattr(cls, f).offset for f, _ in cls._fields_]
    from montecarlopathtracing_amd import api
    want += [api.CURVE_CLAMP, api.CURVE_REINHARD, api.CURVE_FILMIC, api.TRANSFER_LINEAR, api.TRANSFER_SRGB, api.DISPLAY_RGBA,
             api.DISPLAY_ESTIMATE, api.DISPLAY_DENOISED, api.DISPLAY_DENOISED_GUIDED]
    assert got == want


def _awkward_frame():
    """a seeded frame with negatives, values above 1, both infinities and every exact k / 255"""
    rng = np.random.default_rng(77)
    img = rng.uniform(-0.5, 1.5, size=(48, 64, 3))
    flat = img.reshape(-1)
    flat[:256] = np.arange(256) / 255.0
    flat[256:512] = np.nextafter(np.arange(256) / 255.0, -1.0)
    flat[512:516] = (np.inf, -np.inf, 1e300, -1e300)
    flat[516:520] = (0.0, -0.0, 1.0, 5e-324)
    return img


def test_zero_parameters_are_imshow(mcpt):
    img = _awkward_frame()
    want = mcpt.imshow_rgb8(img)
    got, info = mcpt.display_host(img)
    assert got.shape == img.shape and got.dtype == np.uint8 and np.array_equal(got, want)
    assert info == {"exposure": 1.0, "white": 0.0, "log_average": 0.0, "l_percentile": 0.0, "counted": 0, "skipped": 0}
    # a NULL parameter pointer: the same bytes
    out = np.zeros(img.shape, dtype=np.uint8)
    rc = mcpt.lib().mcpt_display_host(img.ctypes.data_as(C.POINTER(C.c_double)), img.size // 3, None, out.ctypes.data_as(C.POINTER(C.c_uint8)), None)
    assert rc == 0 and np.array_equal(out, want)
    assert (want == 0).any() and (want == 255).any() and len(np.unique(want)) == 256
    nan = np.full((1, 3, 3), np.nan)
    nan[0, 1, 1] = 0.5
    assert np.array_equal(mcpt.display_host(nan)[0].reshape(-1), [0, 0, 0, 0, 127, 0, 0, 0, 0])
    rgba, _ = mcpt.display_host(img, rgba=True)
    assert rgba.shape == img.shape[:2] + (4,) and np.array_equal(rgba[..., :3], want) and np.all(rgba[..., 3] == 255)


def test_host_histogram_resolution_is_the_reference(mcpt, frame):
    """the info record of a call that takes the histogram: counts, log average (two libms: 1e-12), percentile edge and exposure"""
    img = DR.edge_frame(1023, 5).reshape(1, -1, 3)
    for f in (frame, img):
        slots = DR.histogram(f)
        la, lp = DR.exposure(slots, 0.0)
        _, info = mcpt.display_host(f, auto_key=0.18, curve="reinhard")
        assert info["counted"] == int(slots[1:].sum()) and info["skipped"] == int(slots[0])
        assert info["l_percentile"] == lp and abs(info["log_average"] - la) <= 1e-12 * la
        assert abs(info["exposure"] - 0.18 / la) <= 1e-12 * (0.18 / la)
        assert info["white"] == max(1.0, info["exposure"] * lp)
    assert DR.histogram(img)[0] > 0 and DR.histogram(img)[1] > 0 and DR.histogram(img)[DR.SLOTS - 1] > 0


@pytest.mark.parametrize("curve", ["clamp", "reinhard", "filmic"])
def test_linear_transfer_is_exact(mcpt, frame, curve):
    whites = (0.0, 2.5) if curve == "reinhard" else (0.0,)
    for e in EXPOSURES:
        for white in whites:
            got, info = mcpt.display_host(frame, exposure=e, white=white, curve=curve)
            er, wr = DR.resolve(frame, e, 0.0, 0.0, white, CURVES[curve])
            assert info["exposure"] == er == e and (curve != "reinhard" or info["white"] == wr)
            if curve == "reinhard" and white == 0.0:
                assert wr == max(1.0, e * DR.exposure(DR.histogram(frame))[1]) and info["counted"] == W * H
            want, _ = DR.display(frame, er, wr, CURVES[curve], DR.LINEAR)
            assert np.array_equal(got, want), (curve, e, white, int((got != want).sum()))
            assert len(np.unique(got)) > 100                                     # (the frame spans the bytes)
    # the awkward values as well: infinities, negatives, denormals, NaN
    edge = DR.edge_frame(1023, 9).reshape(3, 341, 3)
    got, info = mcpt.display_host(edge, exposure=0.5, white=3.0, curve=curve, rgba=True)
    want, _ = DR.display(edge, 0.5, 3.0, CURVES[curve], DR.LINEAR, rgba=True)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("curve", ["clamp", "reinhard", "filmic"])
def test_srgb_transfer_is_exact_away_from_rounding_ties(mcpt, frame, curve):
    for e in EXPOSURES:
        er, wr = DR.resolve(frame, e, 0.0, 0.0, 0.0, CURVES[curve])
        want, mask = DR.display(frame, er, wr, CURVES[curve], DR.SRGB)
        left_out = int((~mask).sum())
        assert left_out <= 1e-4 * mask.size, (curve, e, left_out)                 # asserted on the reference alone, before any comparison
        if curve == "clamp":
            assert left_out == 0
        got, info = mcpt.display_host(frame, exposure=e, curve=curve, transfer="srgb")
        assert np.array_equal(got[mask], want[mask]), (curve, e, int((got != want)[mask].sum()))
        assert not np.array_equal(got, mcpt.display_host(frame, exposure=e, curve=curve)[0])


def _slots(**kv):
    s = np.zeros(DR.SLOTS, dtype=np.int64)
    for k, v in kv.items():
        s[int(k[1:])] = v
    return s


def test_display_exposure_on_hand_built_slots(mcpt):
    def both(slots, p=0.0):
        got, want = mcpt.display_exposure(slots, p), DR.exposure(slots, p)
        assert got[1] == want[1], (got, want)
        assert got[0] == want[0] or abs(got[0] - want[0]) <= 1e-12 * abs(want[0]), (got, want)
        return got
    # everything in one bin: bin 24 * 8 + 3 = [1.375, 1.5), centre 1.4375
    la, lp = both(_slots(s197=1000))
    assert lp == 1.5 and abs(la - 1.4375) <= 1e-12 * 1.4375
    # only under- and over-range: the under slot counts at bin 0's centre, the over slot at bin 383's
    la, lp = both(_slots(s1=3, s386=1), 0.5)
    assert lp == math.ldexp(1.125, -24)
    assert abs(la - 2.0 ** ((3 * math.log2(math.ldexp(1.0625, -24)) + math.log2(math.ldexp(1.9375, 23))) / 4)) <= 1e-12 * la
    assert both(_slots(s1=3, s386=1), 1.0)[1] == math.ldexp(2.0, 23)
    assert both(_slots(s386=7))[1] == 2.0 ** 24 and both(_slots(s1=7))[1] == math.ldexp(1.125, -24)
    # nothing counted (skipped pixels do not count)
    assert both(_slots()) == (0.0, 0.0) and both(_slots(s0=99)) == (0.0, 0.0)
    # the percentile landing exactly on a bin's running count: 100 pixels, 25 per bin in bins 192 .. 195 = [1, 1.125) ... [1.375, 1.5)
    s = _slots(s194=25, s195=25, s196=25, s197=25)
    assert both(s, 0.25)[1] == 1.125 and both(s, 0.26)[1] == 1.25 and both(s, 0.5)[1] == 1.25 and both(s, 0.75)[1] == 1.375
    assert both(s, 0.751)[1] == 1.5 and both(s, 1.0)[1] == 1.5 and both(s, 0.001)[1] == 1.125
    assert both(s)[1] == both(s, 0.99)[1] == 1.5                                  # 0: 0.99
    # the skipped slot changes nothing
    s2 = s.copy()
    s2[0] = 10 ** 9
    assert both(s2, 0.5) == both(s, 0.5)
    # counts beyond 2^32
    big = _slots(s100=2 ** 33, s300=2 ** 33 + 1)
    assert both(big, 0.5)[1] == DR.exposure(big, 0.5)[1]
    L = mcpt.lib()
    la, lp = C.c_double(), C.c_double()
    for bad_p in (-0.1, 1.0001, float("nan"), float("inf")):
        assert L.mcpt_display_exposure(s.ctypes.data_as(C.POINTER(C.c_int64)), bad_p, C.byref(la), C.byref(lp)) == ERR_ARG
    neg = s.copy()
    neg[5] = -1
    assert L.mcpt_display_exposure(neg.ctypes.data_as(C.POINTER(C.c_int64)), 0.5, C.byref(la), C.byref(lp)) == ERR_ARG
    assert L.mcpt_display_exposure(None, 0.5, C.byref(la), C.byref(lp)) == ERR_ARG


def test_auto_exposure_with_nothing_counted(mcpt):
    img = np.zeros((4, 5, 3))
    img[0, 0] = (np.nan, 1.0, 1.0)
    img[1, 1] = (-1.0, -1.0, -1.0)
    got, info = mcpt.display_host(img, exposure=2.0, auto_key=0.18, curve="reinhard")
    assert info == {"exposure": 2.0, "white": 1.0, "log_average": 0.0, "l_percentile": 0.0, "counted": 0, "skipped": 20}
    want, _ = DR.display(img, 2.0, 1.0, DR.REINHARD, DR.LINEAR)
    assert np.array_equal(got, want)


BAD = [dict(reserved=1), dict(curve=3), dict(curve=-1), dict(transfer=2), dict(transfer=-1), dict(flags=2), dict(flags=-1),
       dict(exposure=-1.0), dict(exposure=float("nan")), dict(exposure=float("inf")), dict(auto_key=-0.18), dict(auto_key=float("inf")),
       dict(auto_key=float("nan")), dict(white=-2.0), dict(white=float("nan")), dict(white=float("inf")), dict(percentile=-0.5),
       dict(percentile=1.5), dict(percentile=float("nan"))]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: "%s=%r" % next(iter(b.items())))
def test_refusals(mcpt, bad):
    from montecarlopathtracing_amd import _lib
    L = mcpt.lib()
    dp = _lib.DisplayParams()
    for k, v in bad.items():
        setattr(dp, k, v)
    img = np.full((2, 2, 3), 0.5)
    out = np.full((2, 2, 4), 0xA5, dtype=np.uint8)
    ip, op = img.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_uint8))
    assert L.mcpt_display_host(ip, 4, C.byref(dp), op, None) == ERR_ARG
    assert b"display" in L.mcpt_last_error() and np.all(out == 0xA5)
    # the forms that need a GPU and a handle refuse the parameters before they look at either
    assert L.mcpt_display(None, ip, 4, C.byref(dp), op, None) == ERR_ARG
    assert L.mcpt_display_device(None, None, 4, C.byref(dp), None, None, None) == ERR_ARG
    assert L.mcpt_progressive_display(None, 0, C.byref(dp), op, None) == ERR_ARG
    assert L.mcpt_progressive_display_device(None, 0, C.byref(dp), None, None, None) == ERR_ARG
    assert L.mcpt_render_scene_display(b"", b"no-such-scene", 1, None, 0, None, None, 1.0, None, C.byref(dp), None) == ERR_ARG


def test_refusals_of_arguments(mcpt):
    L = mcpt.lib()
    img = np.full((2, 2, 3), 0.5)
    out = np.zeros((2, 2, 3), dtype=np.uint8)
    ip, op = img.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_uint8))
    assert L.mcpt_display_host(ip, -1, None, op, None) == ERR_ARG
    assert L.mcpt_display_host(None, 4, None, op, None) == ERR_ARG and L.mcpt_display_host(ip, 4, None, None, None) == ERR_ARG
    assert L.mcpt_display_host(None, 0, None, None, None) == 0                      # an empty frame
    from montecarlopathtracing_amd import _lib
    rgba = _lib.DisplayParams(flags=1)
    assert L.mcpt_render_scene_display(b"", b"no-such-scene", 1, None, 0, None, None, 1.0, None, C.byref(rgba), None) == ERR_ARG
    with pytest.raises(KeyError):
        mcpt.make_display(curve="aces")
    with pytest.raises(ValueError):
        mcpt.render_scene("", "x", 1, display={"curve": "filmic"}, motion={"steps": 1})
