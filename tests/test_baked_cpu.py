"""Not gpu: baked frames (include/mcpt.h: baked frames) as far as they go without a device.  The symbols and struct layouts against the
header; every refusal in the header's order, before the missing device; mcpt_lightmap_irradiance_host against the numpy restatement
(tests/baked_ref.py) bit for bit on maps of 1 x 1 to 64 x 64 texels -- texel centres, edges, corners, coordinates outside the map, of
+-1e300 and 1e-300, random points; no owner map, a random one, one that owns nothing --; a linear map comes back as the linear function;
the restatement's own radiance and fold against hand computations; and baked.hpp under the address and undefined-behaviour sanitizers in
a stand-alone program (tests/baked_sanitize_main.cpp) on NaN, infinities, +-1e300 and maps one texel wide."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import baked_ref as BR
from conftest import ROOT

ERR_ARG, ERR_NO_DEVICE = -3, -4
NAMES = ["mcpt_lightmap_irradiance_host", "mcpt_lightmap_irradiance", "mcpt_lightmap_irradiance_device", "mcpt_baked_radiance",
         "mcpt_baked_radiance_device", "mcpt_render_baked", "mcpt_render_baked_device"]
NAN, INF = float("nan"), float("inf")
CSRC = os.path.join(ROOT, "montecarlopathtracing_amd", "csrc")


def _null_device_rc(mcpt):
    return ERR_NO_DEVICE if mcpt.device_count() <= 0 else ERR_ARG


def _message(mcpt):
    return mcpt.lib().mcpt_last_error().decode()


MESSAGES = []        # the messages of the calls of the last _lookups or _calls, call by call


def _noting(L, rc):
    MESSAGES.append(L.mcpt_last_error().decode() if rc != 0 else "")
    return rc


def _said(word, calls=slice(None)):
    """every one of the last helper's calls (or of `calls` among them) was refused with `word` in its message"""
    return all(word in m for m in MESSAGES[calls])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _pi(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None


# ---- symbols and layouts

def test_baked_symbols_are_declared_and_exported(mcpt):
    from montecarlopathtracing_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for sym in NAMES:
        assert (sym + "(") in hdr and sym in _lib.EXPORTS and hasattr(L, sym), sym
    for s in ("mcpt_baked_source", "mcpt_baked_outputs", "mcpt_baked_frame_params"):
        assert ("} %s;" % s) in hdr
    assert "#define MCPT_VERSION 105" in hdr and mcpt.lib().mcpt_version() == 105
    for name, v in (("MCPT_BAKED_VOLUME", mcpt.BAKED_VOLUME), ("MCPT_BAKED_LIGHTMAP", mcpt.BAKED_LIGHTMAP), ("MCPT_BAKED_MISS", mcpt.BAKED_MISS),
                    ("MCPT_BAKED_EMITTER", mcpt.BAKED_EMITTER), ("MCPT_BAKED_SURFACE", mcpt.BAKED_SURFACE),
                    ("MCPT_BAKED_FACE_VIEWER", mcpt.BAKED_FACE_VIEWER), ("MCPT_BAKED_LIGHTING_ONLY", mcpt.BAKED_LIGHTING_ONLY)):
        line = [l for l in hdr.splitlines() if l.startswith("#define %s " % name)]
        assert len(line) == 1 and int(line[0].split()[2]) == v, name
    assert (BR.MISS, BR.EMITTER, BR.SURFACE) == (mcpt.BAKED_MISS, mcpt.BAKED_EMITTER, mcpt.BAKED_SURFACE)
    for f in ("lightmap_irradiance", "lightmap_irradiance_device", "baked_radiance", "baked_radiance_device", "render_baked", "render_baked_device"):
        assert callable(getattr(mcpt.Device, f))
    for f in ("lightmap_irradiance_host", "baked_volume", "baked_lightmap"):
        assert callable(getattr(mcpt, f))


def test_struct_layouts_match_the_header(mcpt, tmp_path):
    from montecarlopathtracing_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    if cc is None:
        pytest.skip("no C compiler")
    structs = [("mcpt_baked_source", _lib.BakedSource, 112,
                ["kind", "flags", "grid", "sh27", "valid", "moments", "visibility", "uv6", "width", "height", "irradiance3", "owner", "reserved"]),
               ("mcpt_baked_outputs", _lib.BakedOutputs, 80, ["radiance3", "kind", "face", "q6", "uv2", "kd3", "e3", "lit", "reserved"]),
               ("mcpt_baked_frame_params", _lib.BakedFrameParams, 32, ["samples", "flags", "seed", "workspace_rays", "reserved"])]
    body = ""
    for name, cls, _, fields in structs:
        assert [n for n, _ in cls._fields_] == fields
        body += "  printf(\"%%zu\\n\", sizeof(%s));\n" % name + "".join("  printf(\"%%zu\\n\", offsetof(%s, %s));\n" % (name, f) for f in fields)
    src = tmp_path / "layout_baked.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"mcpt.h\"\nint main(void) {\n" + body + "  return 0;\n}\n")
    exe = tmp_path / "layout_baked"
    subprocess.check_call([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    at = 0
    for name, cls, size, fields in structs:
        assert out[at] == C.sizeof(cls) == size, name
        for i, f in enumerate(fields):
            assert out[at + 1 + i] == getattr(cls, f).offset, (name, f)
        at += 1 + len(fields)


# ---- refusals

def _lookups(L, W, H, E, owner, uv, n, e, device=True):
    """the return codes of the host form, the host-pointer form and (device=True) the device form on a NULL device"""
    del MESSAGES[:]
    rc = [_noting(L, L.mcpt_lightmap_irradiance_host(W, H, _pd(E), _pi(owner), _pd(uv), n, _pd(e), None)),
          _noting(L, L.mcpt_lightmap_irradiance(None, W, H, _pd(E), _pi(owner), _pd(uv), n, _pd(e), None))]
    if device:
        addr = lambda a: a.ctypes.data if a is not None else None
        rc.append(_noting(L, L.mcpt_lightmap_irradiance_device(None, W, H, addr(E), addr(owner), addr(uv), n, addr(e), None, None)))
    return rc


def test_lookup_refusals_come_in_order_and_before_the_missing_device(mcpt):
    L = mcpt.lib()
    nd = _null_device_rc(mcpt)
    E, uv, e = np.ones((4, 5, 3)), np.full((3, 2), 0.5), np.zeros((3, 3))
    # the size first -- before a bad count and NULL arrays
    for W, H in ((0, 4), (5, 0), (-1, 4), (16385, 4), (5, 16385)):
        assert _lookups(L, W, H, None, None, None, -1, None) == [ERR_ARG] * 3 and _said("16384"), (W, H)
    # then the count, then the arrays
    for n in (-1, 2 ** 31, 2 ** 40):
        assert _lookups(L, 5, 4, None, None, None, n, None) == [ERR_ARG] * 3 and _said("chart coordinates")
    for drop in range(3):
        args = [E, uv, e]
        args[drop] = None
        assert _lookups(L, 5, 4, args[0], None, args[1], 3, args[2]) == [ERR_ARG] * 3 and _said("null"), drop
    # the host-pointer forms look at the coordinates; the device form does not
    for bad in (NAN, INF, -INF):
        uv2 = uv.copy()
        uv2[1, 1] = bad
        assert _lookups(L, 5, 4, E, None, uv2, 3, e) == [ERR_ARG, ERR_ARG, nd] and _said("chart coordinate 1", slice(0, 2)), bad
    # valid arguments: the host form answers, the others miss the device; the limits themselves pass; n == 0 needs no arrays
    assert _lookups(L, 5, 4, E, None, uv, 3, e) == [0, nd, nd]
    if nd == ERR_NO_DEVICE:
        assert "device" in _message(mcpt).lower()
    assert _lookups(L, 5, 4, None, None, None, 0, None) == [0, nd, nd]
    assert _lookups(L, 16384, 1, np.ones((1, 16384, 3)), None, uv, 3, e) == [0, nd, nd]
    got, taps = mcpt.lightmap_irradiance_host(E, np.zeros((0, 2)))
    assert got.shape == (0, 3) and taps.shape == (0,)


def _grid(mcpt, **kw):
    g = mcpt.volume_grid(kw.get("origin", (0.0, 0.0, 0.0)), kw.get("spacing", (1.0, 1.0, 1.0)), kw.get("counts", (2, 2, 2)))
    g.flags = kw.get("flags", 0)
    return g


class _Src:
    """a mcpt_baked_source over arrays this object keeps alive"""

    def __init__(self, mcpt, kind, grid="good", sh=True, moments=False, vis=None, width=5, height=4, irr=True, flags=0, reserved=0):
        from montecarlopathtracing_amd import _lib
        self.keep = [np.ones((8, 9, 3)), np.tile([0.5, 0.3], (8, 4, 1)), np.ones((4, 5, 3)), _grid(mcpt) if grid == "good" else grid, vis]
        s = _lib.BakedSource()
        s.kind, s.flags = kind, flags
        s.reserved[3] = reserved
        if self.keep[3] is not None:
            s.grid = C.pointer(self.keep[3])
        s.sh27 = self.keep[0].ctypes.data if sh else None
        s.moments = self.keep[1].ctypes.data if moments else None
        if vis is not None:
            s.visibility = C.pointer(vis)
        s.width, s.height = width, height
        s.irradiance3 = self.keep[2].ctypes.data if irr else None
        self.s = s


def _calls(mcpt, src, n=-1, rays=None, flags=-1, outputs="null", fp="null", img=None):
    """the return codes of the four baked calls on a NULL device: radiance host and device form (bad n, flags and NULL outputs unless
    given), frame host and device form (NULL parameters unless given)"""
    from montecarlopathtracing_amd import _lib
    L = mcpt.lib()
    s = C.byref(src.s) if src is not None else None
    o = C.byref(outputs) if outputs != "null" else None
    p = C.byref(fp) if fp != "null" else None
    del MESSAGES[:]
    return [_noting(L, L.mcpt_baked_radiance(None, s, _pd(rays), n, flags, o, None)),
            _noting(L, L.mcpt_baked_radiance_device(None, s, rays.ctypes.data if rays is not None else None, n, flags, o, None, None)),
            _noting(L, L.mcpt_render_baked(None, s, p, _pd(img), None, None, None)),
            _noting(L, L.mcpt_render_baked_device(None, s, p, img.ctypes.data if img is not None else None, None, None, None, None))]


def test_source_refusals_come_in_order_and_before_everything_else(mcpt):
    V, LM = mcpt.BAKED_VOLUME, mcpt.BAKED_LIGHTMAP
    bad = [ERR_ARG] * 4
    assert _calls(mcpt, None) == bad and _said("null baked source")
    for kind in (0, 3, -1):
        assert _calls(mcpt, _Src(mcpt, kind, grid=None, sh=False, irr=False, flags=1, reserved=1)) == bad and _said("MCPT_BAKED_VOLUME")
    assert _calls(mcpt, _Src(mcpt, V, grid=None, sh=False, flags=1, reserved=1)) == bad and _said("flags")
    assert _calls(mcpt, _Src(mcpt, V, grid=None, sh=False, reserved=1)) == bad and _said("reserved")
    # a volume: the grid (NULL first, then its fields in order), the coefficients, then -- with moments -- the visibility struct
    assert _calls(mcpt, _Src(mcpt, V, grid=None, sh=False)) == bad and _said("null volume grid")
    for kw, word in ((dict(origin=(NAN, 0, 0)), "origin"), (dict(spacing=(0.0, 1, 1)), "spacing"), (dict(counts=(0, 1, 1)), "at least one probe"),
                     (dict(flags=2), "flag")):
        assert _calls(mcpt, _Src(mcpt, V, grid=_grid(mcpt, **kw), sh=False)) == bad and _said(word), kw
    assert _calls(mcpt, _Src(mcpt, V, sh=False, moments=True)) == bad and _said("null coefficients")
    assert _calls(mcpt, _Src(mcpt, V, moments=True)) == bad and _said("null volume visibility")
    for kw, word in ((dict(res=0), "res"), (dict(res=17), "res"), (dict(max_distance=0.0), "max_distance"), (dict(normal_bias=-1.0), "normal_bias"),
                     (dict(min_visibility=2.0), "min_visibility")):
        vis = mcpt.volume_visibility(**dict(dict(res=2, max_distance=1.0), **kw))
        assert _calls(mcpt, _Src(mcpt, V, moments=True, vis=vis)) == bad and _said(word), kw
    # a volume without moments does not look at the visibility struct, nor at the lightmap's fields
    ok = _Src(mcpt, V, vis=mcpt.volume_visibility(res=0), width=0, irr=False)
    assert _calls(mcpt, ok) == bad and _said("unknown baked flag", slice(0, 2)) and _said("null baked frame parameters", slice(2, 4))
    # a lightmap: the size, then the map; the volume's fields are not read
    for W, H in ((0, 4), (5, 16385)):
        assert _calls(mcpt, _Src(mcpt, LM, grid=None, sh=False, width=W, height=H, irr=False)) == bad and _said("16384")
    assert _calls(mcpt, _Src(mcpt, LM, grid=None, sh=False, irr=False)) == bad and _said("null irradiance map")
    assert _calls(mcpt, _Src(mcpt, LM, grid=None, sh=False)) == bad and _said("unknown baked flag", slice(0, 2)) and _said("null baked frame parameters", slice(2, 4))


def test_call_refusals_come_in_order_and_before_the_missing_device(mcpt):
    from montecarlopathtracing_amd import _lib
    nd = _null_device_rc(mcpt)
    rays, img = np.tile([0.0, 0, 0, 0, 0, 1.0], (3, 1)), np.zeros((2, 2, 3))
    for src in (_Src(mcpt, mcpt.BAKED_VOLUME), _Src(mcpt, mcpt.BAKED_VOLUME, moments=True, vis=mcpt.volume_visibility(2, 1.0)),
                _Src(mcpt, mcpt.BAKED_LIGHTMAP, grid=None, sh=False)):
        out = _lib.BakedOutputs()
        # radiance: flags, the count, the rays, the outputs and their reserved words
        for flags in (4, 8, -1):
            assert _calls(mcpt, src, flags=flags)[:2] == [ERR_ARG] * 2 and _said("unknown baked flag", slice(0, 2))
        for n in (-1, 2 ** 31, 2 ** 40):
            assert _calls(mcpt, src, n=n, flags=3)[:2] == [ERR_ARG] * 2 and _said("number of rays", slice(0, 2))
        assert _calls(mcpt, src, n=3, flags=0)[:2] == [ERR_ARG] * 2 and _said("null rays", slice(0, 2))
        assert _calls(mcpt, src, n=3, rays=rays, flags=0)[:2] == [ERR_ARG] * 2 and _said("null baked outputs", slice(0, 2))
        out.reserved[1] = 1
        assert _calls(mcpt, src, n=3, rays=rays, flags=0, outputs=out)[:2] == [ERR_ARG] * 2 and _said("reserved", slice(0, 2))
        out.reserved[1] = 0
        assert _calls(mcpt, src, n=3, rays=rays, flags=3, outputs=out)[:2] == [nd] * 2
        assert _calls(mcpt, src, n=0, flags=0, outputs=out)[:2] == [nd] * 2                    # n == 0 still misses the device first
        # frames: the parameters (NULL, samples, flags, workspace_rays, reserved), then the image
        assert _calls(mcpt, src)[2:] == [ERR_ARG] * 2 and _said("null baked frame parameters", slice(2, 4))
        # (samples, flags, workspace_rays, reserved): each line mends the field the line before was refused for and leaves the later ones bad
        for (samples, flags, ws, reserved), word in (((0, 4, -1, 1), "samples"), ((65537, 4, -1, 1), "samples"), ((1, 4, -1, 1), "unknown baked flag"),
                                                     ((1, 3, -1, 1), "workspace_rays"), ((1, 3, 0, 1), "reserved")):
            fp = _lib.BakedFrameParams(samples, flags, 1, ws, (C.c_int32 * 2)(0, reserved))
            assert _calls(mcpt, src, fp=fp)[2:] == [ERR_ARG] * 2 and _said(word, slice(2, 4)), (word, MESSAGES)
        fp = _lib.BakedFrameParams(65536, 3, 1, 2 ** 40, (C.c_int32 * 2)(0, 0))
        assert _calls(mcpt, src, fp=fp)[2:] == [ERR_ARG] * 2 and _said("null image", slice(2, 4))
        assert _calls(mcpt, src, fp=fp, img=img)[2:] == [nd] * 2
        if nd == ERR_NO_DEVICE:
            assert "device" in _message(mcpt).lower()


def test_api_validates_shapes(mcpt):
    E, uv = np.ones((4, 5, 3)), np.zeros((3, 2))
    with pytest.raises(ValueError):
        mcpt.lightmap_irradiance_host(np.ones((4, 5)), uv)
    with pytest.raises(ValueError):
        mcpt.lightmap_irradiance_host(E, np.zeros((3, 3)))
    with pytest.raises(ValueError):
        mcpt.lightmap_irradiance_host(E, uv, owner=np.zeros((5, 4), dtype=np.int32))
    with pytest.raises(ValueError):
        mcpt.baked_lightmap(E, uv=np.zeros((3, 5)))
    with pytest.raises(ValueError):
        mcpt.baked_volume(_grid(mcpt), np.ones((7, 9, 3)))
    with pytest.raises(ValueError):
        mcpt.baked_volume(_grid(mcpt), np.ones((8, 9, 3)), vis=mcpt.volume_visibility(2, 1.0))
    with pytest.raises(ValueError):
        mcpt.baked_volume(_grid(mcpt), np.ones((8, 9, 3)), moments=np.ones((8, 4, 2)))
    src = mcpt.baked_volume(_grid(mcpt), np.ones((8, 9, 3)), valid=np.ones(8, dtype=np.uint8), moments=np.ones((8, 4, 2)), vis=mcpt.volume_visibility(2, 1.0))
    s = src.struct()
    assert s.kind == mcpt.BAKED_VOLUME and s.sh27 == src.sh.ctypes.data and s.valid == src.valid.ctypes.data and s.moments == src.moments.ctypes.data
    lm = mcpt.baked_lightmap(E, owner=np.zeros((4, 5)))
    s = lm.struct()
    assert (s.kind, s.width, s.height, s.uv6) == (mcpt.BAKED_LIGHTMAP, 5, 4, None) and s.owner == lm.owner.ctypes.data and lm.owner.dtype == np.int32


# ---- the lookup

@pytest.fixture(scope="module")
def lookup_cases():
    """per size: the map, a random owner map, the coordinates, and the restatement's answers for (none, random, nothing owned)"""
    out = {}
    for W, H in BR.SIZES:
        E, own, uv = BR.lightmap(W, H), BR.owner_map(W, H), BR.coordinates(W, H)
        owners = (None, own, np.full((H, W), -1, dtype=np.int32))
        out[(W, H)] = (E, owners, uv, [BR.lightmap_irradiance(E, uv, o) for o in owners])
    return out


@pytest.mark.parametrize("size", BR.SIZES)
def test_host_lookup_is_the_restatement_bit_for_bit(mcpt, lookup_cases, size):
    """fp64 add, multiply, divide and floor only: equality is asserted"""
    E, owners, uv, want = lookup_cases[size]
    assert uv.shape[0] >= BR.N_RANDOM + size[0] * size[1] and (np.abs(uv) == 1e300).any() and (np.abs(uv) == 1e-300).any()
    assert (uv < 0).any(axis=0).all() and (uv > 1).any(axis=0).all()
    for o, (we, wt) in zip(owners, want):
        e, taps = mcpt.lightmap_irradiance_host(E, uv, owner=o)
        assert _same(e, we) and np.array_equal(taps, wt), size
        assert np.isfinite(e).all() and taps.min() >= 0 and taps.max() <= 4
    # nothing owned: +0.0 and no taps
    e, taps = mcpt.lightmap_irradiance_host(E, uv, owner=owners[2])
    assert not _bits(e).any() and not taps.any()
    # no owner map: every coordinate has at least one tap, a 1 x 1 map exactly one
    assert want[0][1].min() >= 1 and (size != (1, 1) or (want[0][1] == 1).all())
    assert (want[1][1] == 0).any() or size == (1, 1) or (owners[1] != -1).all()


@pytest.mark.parametrize("size", BR.SIZES)
def test_a_texel_centre_gets_the_texels_value(mcpt, lookup_cases, size):
    """f == 0.0 on both axes at (x + 0.5) / W of these sizes: the map's own bits, one tap; with an owner map, +0.0 where the texel is -1"""
    E, owners, uv, _ = lookup_cases[size]
    W, H = size
    c = BR.centres(W, H)
    assert _same(c, uv[:W * H])
    e, taps = mcpt.lightmap_irradiance_host(E, c)
    assert _same(e, E.reshape(-1, 3)) and (taps == 1).all()
    e, taps = mcpt.lightmap_irradiance_host(E, c, owner=owners[1])
    owned = owners[1].reshape(-1) != -1
    assert _same(e[owned], E.reshape(-1, 3)[owned]) and (taps[owned] == 1).all() and not _bits(e[~owned]).any() and not taps[~owned].any()


def test_a_permuted_list_gives_permuted_answers(mcpt, lookup_cases):
    E, owners, uv, want = lookup_cases[(5, 4)]
    perm = np.random.default_rng(3).permutation(uv.shape[0])
    for o, (we, wt) in zip(owners, want):
        e, taps = mcpt.lightmap_irradiance_host(E, uv[perm], owner=o)
        assert _same(e, we[perm]) and np.array_equal(taps, wt[perm])


@pytest.mark.parametrize("size", BR.SIZES)
def test_weights_sum_to_one_within_4_ulps(mcpt, lookup_cases, size):
    """in the restatement, and through the entry point: a map of ones comes back as the sum of the weights"""
    W, H = size
    _, owners, uv, _ = lookup_cases[size]
    ulp = np.finfo(np.float64).eps
    worst = 0.0
    for o in owners[:2]:
        _, w, count = BR.taps(W, H, uv, o)
        total = w.sum(axis=1)
        e, taps = mcpt.lightmap_irradiance_host(np.ones((H, W, 3)), uv, owner=o)
        lit = count > 0
        for s in (total[lit], e[lit, 0], e[lit, 2]):
            worst = max(worst, float(np.abs(s - 1.0).max()) / ulp)
        assert (w >= 0.0).all() and (w <= 1.0).all()
    print("%r: the weights' sum is off 1 by at most %.2f ulps" % (size, worst))
    assert worst <= 4.0


@pytest.mark.parametrize("size", BR.SIZES)
def test_a_linear_map_comes_back_linear(mcpt, size):
    """E = a + b pu + c pv at the texel centres: bilinear blending reproduces it inside the hull of the centres in exact arithmetic; in
    fp64 within 1e-12 of the terms' size, the bound tests/test_volume_cpu.py holds its linear fields to"""
    W, H = size
    rng = np.random.default_rng([21, W, H])
    a, b, c = rng.normal(size=3) * 3.0, rng.normal(size=3) * 5.0, rng.normal(size=3) * 7.0
    cen = BR.centres(W, H)
    E = (a + cen[:, :1] * b + cen[:, 1:] * c).reshape(H, W, 3)
    lo, hi = cen.min(axis=0), cen.max(axis=0)
    uv = lo + (hi - lo) * rng.random((4000, 2))
    e, taps = mcpt.lightmap_irradiance_host(E, uv)
    want = a + uv[:, :1] * b + uv[:, 1:] * c
    size_of_terms = np.abs(a) + np.abs(uv[:, :1] * b) + np.abs(uv[:, 1:] * c)
    rel = float((np.abs(e - want) / size_of_terms).max())
    print("%r: a linear map is off the linear function by at most %.3e of the terms' size" % (size, rel))
    assert rel <= 1e-12 and (taps >= 1).all()


# ---- the restatement against hand computations

def test_restatement_against_hand_computations():
    # the lookup: a 2 x 2 map, u = 0.5 -> s = 0.5 on both axes, every weight a quarter
    E = np.array([[[1.0, 2, 3], [5.0, 6, 7]], [[9.0, 10, 11], [13.0, 14, 15]]])
    e, taps = BR.lightmap_irradiance(E, [[0.5, 0.5]])
    assert e.tolist() == [[7.0, 8.0, 9.0]] and taps.tolist() == [4]
    # u = 0.375 -> s = 0.25: weights 0.75, 0.25 in x; v = 0.25 -> s = 0: row 0 alone
    e, taps = BR.lightmap_irradiance(E, [[0.375, 0.25]])
    assert e.tolist() == [[2.0, 3.0, 4.0]] and taps.tolist() == [2]
    # texel (0, 0) not owned: the other tap takes it all
    e, taps = BR.lightmap_irradiance(E, [[0.375, 0.25]], owner=np.array([[-1, 0], [0, 0]]))
    assert e.tolist() == [[5.0, 6.0, 7.0]] and taps.tolist() == [1]
    # outside: the border's texel; NaN: texel 0
    e, taps = BR.lightmap_irradiance(E, [[1e300, -1e300], [NAN, NAN], [7.0, 7.0]])
    assert e.tolist() == [[5.0, 6, 7], [1.0, 2, 3], [13.0, 14, 15]] and taps.tolist() == [1, 1, 1]
    # the chart coordinate of a hit: the corner weights blend the chart's corners
    uv = BR.chart_uv(np.array([[0.0, 0.0, 1.0, 0.0, 0.0, 1.0]]), np.array([[0.5, 0.25, 0.25]]))
    assert uv.tolist() == [[0.25, 0.25]]
    g = BR.barycentric(np.array([[0.0, 0, 0]]), np.array([[2.0, 0, 0]]), np.array([[0.0, 2, 0]]), np.array([[0.5, 1.0, 0.0]]))
    assert g.tolist() == [[0.25, 0.25, 0.5]]
    # one sample of each kind, both flags
    kind = np.array([BR.SURFACE, BR.EMITTER, BR.MISS])
    kd, e3 = np.tile([0.5, 0.25, 1.0], (3, 1)), np.tile([BR.PI, 2 * BR.PI, 4 * BR.PI], (3, 1))
    emitted, missed = np.tile([17.0, 12.0, 4.0], (3, 1)), np.tile([0.125, 0.25, 0.5], (3, 1))
    assert BR.radiance(kind, kd, e3, emitted, missed).tolist() == [[0.5, 0.5, 4.0], [17.0, 12.0, 4.0], [0.125, 0.25, 0.5]]
    assert BR.radiance(kind, kd, e3, emitted, missed, lighting_only=True).tolist() == [[1.0, 2.0, 4.0], [17.0, 12.0, 4.0], [0.125, 0.25, 0.5]]
    pn, fn, d = np.array([[0.0, 0, 2.0], [0.0, 0, 0], [NAN, 0, 0]]), np.tile([0.0, 1.0, 0.0], (3, 1)), np.tile([0.0, 1.0, 1.0], (3, 1))
    assert BR.shading_normal(pn, fn, d, False).tolist() == [[0.0, 0, 2.0], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0]]
    assert BR.shading_normal(pn, fn, d, True).tolist() == [[-0.0, -0.0, -2.0], [-0.0, -1.0, -0.0], [-0.0, -1.0, -0.0]]
    assert BR.shading_normal(pn, fn, -d, True).tolist() == [[0.0, 0, 2.0], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0]]
    # the fold of G = 3: a surface sample that found nothing, an emitter, a lit surface sample
    L = np.array([[[0.0, 0.0, 0.0], [17.0, 12.0, 4.0], [1.0, 0.5, 0.25]]])
    px, counts, lit = BR.fold(L, np.array([[BR.SURFACE, BR.EMITTER, BR.SURFACE]]), np.array([[0, 0, 3]]))
    assert px.tolist() == [[6.0, 12.5 / 3.0, 4.25 / 3.0]] and counts.tolist() == [[2, 1, 0]] and lit.tolist() == [1]


# ---- baked.hpp under the sanitizers

def test_lookup_under_address_and_undefined_sanitizers(tmp_path):
    """A stand-alone program, not the library: nothing loaded into this process is instrumented."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "baked_sanitize")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "baked_sanitize_main.cpp")])
    edge = [NAN, INF, -INF, 1e300, -1e300, 1e-300, -1e-300, 0.0, -0.0, 1.0, 0.5, 0.999999, 2.5, -2.5, 1e17, 3e9, -3e9]
    cases = [(W, H, mode, u, v) for W, H in ((1, 1), (1, 7), (7, 1), (5, 4)) for mode in (0, 1, 2) for u in edge for v in edge]
    text = "".join("%d %d %d %r %r\n" % c for c in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases)
    got = np.array([[float.fromhex(x) for x in l.split()[:3]] for l in lines])
    taps = np.array([int(l.split()[3]) for l in lines])
    at = 0
    per = len(edge) ** 2
    for W, H in ((1, 1), (1, 7), (7, 1), (5, 4)):
        T = np.arange(W * H)
        E = ((3 * T[:, None] + np.arange(3) + 1) / 4.0).reshape(H, W, 3)
        for mode in (0, 1, 2):
            own = None if mode == 0 else np.where((T % 3 == 0) | (mode == 2), -1, T % 7).astype(np.int32).reshape(H, W)
            uv = np.array([c[3:] for c in cases[at:at + per]])
            we, wt = BR.lightmap_irradiance(E, uv, own)
            assert _same(got[at:at + per], we) and np.array_equal(taps[at:at + per], wt), (W, H, mode)
            at += per
