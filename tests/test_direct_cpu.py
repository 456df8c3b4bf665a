"""Not gpu: direct light from a caller's own lights (include/mcpt.h: direct light) as far as it goes without a device.  The seven symbols
and the three structs' layouts against the header; every refusal in the header's order, before the missing device; mcpt_direct_slots
and mcpt_direct_fold_host against the numpy restatement (tests/direct_ref.py) bit for bit -- n in {1, 5}, light mixes of 0, 1, 2 and 5
lights that hold every type, spp in {1, 2, 7}, all-occluded, none-occluded and random bytes, with skipped slots --; and the
host-compiled parts of csrc/direct.hpp under the address and undefined-behaviour sanitizers in a stand-alone program
(tests/direct_sanitize_main.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import direct_ref as DR
from conftest import ROOT

CSRC = os.path.join(ROOT, "montecarlopathtracing_amd", "csrc")
ERR_ARG, ERR_NO_DEVICE = -3, -4
NAMES = ["mcpt_query_direct", "mcpt_query_direct_device", "mcpt_direct_slots", "mcpt_direct_rays", "mcpt_direct_fold_host",
         "mcpt_bake_direct_lightmap", "mcpt_bake_direct_lightmap_device"]
PD, PU8, PI32 = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
INT_MAX = 2 ** 31 - 1
NAN, INF = float("nan"), float("inf")


def _null_device_rc(mcpt):
    return ERR_NO_DEVICE if mcpt.device_count() <= 0 else ERR_ARG


def _message(mcpt):
    return mcpt.lib().mcpt_last_error().decode()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _mix(mcpt, nl):
    """nl lights; the mixes of 2 and 5 hold every type between them, the one of 5 every type and both sidedness settings"""
    five = [mcpt.point_light((0.3, 2.0, -0.4), (8.0, 4.0, 2.0), range=9.0),
            mcpt.rect_light((-0.5, 1.5, -0.5), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (3.0, 2.0, 1.0)),
            mcpt.spot_light((1.0, 1.0, 1.0), (-1.0, -1.0, -1.0), (5.0, 5.0, 7.0), 20.0, 35.0),
            mcpt.directional_light((0.2, -1.0, 0.1), (0.5, 0.25, 0.125)),
            mcpt.rect_light((-0.5, 2.5, 0.5), (0.0, 0.0, 1.0), (0.5, 0.25, 0.0), (1.0, 0.5, 4.0), two_sided=True)]
    return {0: [], 1: five[1:2], 2: [five[2], five[3]], 5: five}[nl]


def test_direct_symbols_are_declared_and_exported(mcpt):
    from montecarlopathtracing_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for sym in NAMES:
        assert (sym + "(") in hdr and sym in _lib.EXPORTS and hasattr(L, sym), sym
    for t in ("mcpt_direct_light", "mcpt_direct_params", "mcpt_direct_map"):
        assert "} %s;" % t in hdr
    assert "#define MCPT_VERSION 105" in hdr and mcpt.lib().mcpt_version() == 105
    for f in ("direct_light", "direct_rays", "bake_direct_lightmap"):
        assert callable(getattr(mcpt.Device, f))
    for f in ("point_light", "spot_light", "directional_light", "rect_light", "direct_slots", "direct_fold_host"):
        assert callable(getattr(mcpt, f))
    assert (mcpt.LIGHT_POINT, mcpt.LIGHT_SPOT, mcpt.LIGHT_DIRECTIONAL, mcpt.LIGHT_RECT, mcpt.LIGHT_TWO_SIDED) == (0, 1, 2, 3, 1)
    for name, v in (("POINT", 0), ("SPOT", 1), ("DIRECTIONAL", 2), ("RECT", 3), ("TWO_SIDED", 1)):
        assert any(line.split()[:3] == ["#define", "MCPT_LIGHT_" + name, str(v)] for line in hdr.splitlines()), name


def test_direct_struct_layouts_match_the_header(mcpt, tmp_path):
    from montecarlopathtracing_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    if cc is None:
        pytest.skip("no C compiler")
    structs = [("mcpt_direct_light", _lib.DirectLight, 152, ["type", "flags", "position", "direction", "u", "v", "color", "cos_inner", "cos_outer", "range"]),
               ("mcpt_direct_params", _lib.DirectParams, 40, ["spp", "sample_base", "seed", "bias", "flags", "reserved"]),
               ("mcpt_direct_map", _lib.DirectMap, 16, ["width", "height", "dilate", "reserved"])]
    body = ""
    for cname, rec, _, fields in structs:
        assert [n for n, _ in rec._fields_] == fields
        body += "  printf(\"%%zu\\n\", sizeof(%s));\n" % cname + "".join("  printf(\"%%zu\\n\", offsetof(%s, %s));\n" % (cname, f) for f in fields)
    src = tmp_path / "layout_direct.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"mcpt.h\"\nint main(void) {\n" + body + "  return 0;\n}\n")
    exe = tmp_path / "layout_direct"
    subprocess.check_call([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    at = 0
    for cname, rec, size, fields in structs:
        assert out[at] == C.sizeof(rec) == size, cname
        for i, f in enumerate(fields):
            assert out[at + 1 + i] == getattr(rec, f).offset, (cname, f)
        at += 1 + len(fields)


# ---- the light helpers

def test_light_helpers_fill_the_records(mcpt):
    p = mcpt.point_light((1, 2, 3), (4, 5, 6), range=7)
    assert (p.type, p.flags, list(p.position), list(p.color), p.range) == (0, 0, [1.0, 2.0, 3.0], [4.0, 5.0, 6.0], 7.0)
    s = mcpt.spot_light((0, 1, 0), (0, -1, 0), (1, 1, 1), 60.0, 90.0)
    assert s.type == 1 and list(s.direction) == [0.0, -1.0, 0.0] and abs(s.cos_inner - 0.5) < 1e-15 and abs(s.cos_outer) < 1e-15
    d = mcpt.directional_light((0, -1, 0), (2, 2, 2))
    assert d.type == 2 and list(d.direction) == [0.0, -1.0, 0.0]
    r = mcpt.rect_light((0, 0, 0), (1, 0, 0), (0, 0, 1), (1, 1, 1), two_sided=True)
    assert (r.type, r.flags, list(r.u), list(r.v)) == (3, 1, [1.0, 0.0, 0.0], [0.0, 0.0, 1.0])
    assert mcpt.rect_light((0, 0, 0), (1, 0, 0), (0, 0, 1), (1, 1, 1)).flags == 0
    with pytest.raises(ValueError):
        mcpt.point_light((1, 2), (1, 1, 1))
    with pytest.raises(ValueError):
        mcpt.direct_slots([object()])


# ---- mcpt_direct_slots and mcpt_direct_fold_host against the restatement

@pytest.mark.parametrize("spp", [1, 2, 7])
@pytest.mark.parametrize("nl", [0, 1, 2, 5])
def test_direct_slots_are_the_restatements(mcpt, nl, spp):
    lights = _mix(mcpt, nl)
    assert mcpt.direct_slots(lights, spp) == DR.slots(lights, spp) == sum(spp if L.type == 3 else 1 for L in lights)


def _factors(kind, n, R, seed):
    """g [n * R] with skipped slots (+0.0) among them, and the occlusion bytes of `kind`"""
    rng = np.random.default_rng([seed, n, R])
    g = rng.random(n * R) * 3.0
    g[rng.random(n * R) < 0.3] = 0.0
    if n * R:
        g[0] = 0.0
        g[-1] = 1e-300
    occ = {"all": np.ones(n * R, dtype=np.uint8), "none": np.zeros(n * R, dtype=np.uint8), "random": (rng.random(n * R) < 0.5).astype(np.uint8)}[kind]
    return g, occ


@pytest.mark.parametrize("kind", ["all", "none", "random"])
@pytest.mark.parametrize("spp", [1, 2, 7])
@pytest.mark.parametrize("nl", [0, 1, 2, 5])
@pytest.mark.parametrize("n", [1, 5])
def test_direct_fold_host_is_the_restatement_bit_for_bit(mcpt, n, nl, spp, kind):
    lights = _mix(mcpt, nl)
    R = DR.slots(lights, spp)
    g, occ = _factors(kind, n, R, 7)
    got = mcpt.direct_fold_host(lights, g, occ, n, spp)
    want = DR.fold(lights, g, occ, n, spp)
    for key in ("irradiance", "stderr", "per_light", "visibility"):
        assert got[key].shape == want[key].shape and np.array_equal(_bits(got[key]), _bits(want[key])), key
    assert got["per_light"].shape == (n, nl, 3) and got["visibility"].shape == (n, nl)
    if nl == 0:
        assert not got["irradiance"].any() and not got["stderr"].any()
        return
    # the restatement against the contract's words, on the last entry: visibility is lit / traced of the slots with g > 0
    gi, oi = g.reshape(n, R)[-1], occ.reshape(n, R)[-1]
    at = 0
    for l, L in enumerate(lights):
        m = DR.light_slots(L, spp)
        tr = gi[at:at + m] > 0
        lit = tr & (oi[at:at + m] == 0)
        assert want["visibility"][-1, l] == (lit.sum() / tr.sum() if tr.sum() else 0.0)
        if kind == "all":
            assert not want["per_light"][-1, l].any()
        at += m
    if kind == "all":
        assert not want["irradiance"].any() and not want["stderr"].any() and not want["visibility"].any()
    if spp == 1:
        assert not want["stderr"].any()


def test_fold_hand_values(mcpt):
    """a point light of colour (8, 4, 2) with g = 1/4 open: (2, 1, 0.5); a rectangle of two samples, one occluded"""
    lights = [mcpt.point_light((0, 2, 0), (8, 4, 2)), mcpt.rect_light((0, 0, 0), (1, 0, 0), (0, 0, 1), (2, 2, 2))]
    got = mcpt.direct_fold_host(lights, [0.25, 1.0, 3.0], [0, 0, 1], 1, spp=2)
    assert got["per_light"][0].tolist() == [[2.0, 1.0, 0.5], [1.0, 1.0, 1.0]] and got["irradiance"][0].tolist() == [3.0, 2.0, 1.5]
    assert got["visibility"][0].tolist() == [1.0, 0.5]
    # s1 = 2, s2 = 4: var = (4 - 4 / 2) / 1 = 2, se2 = 1
    assert got["stderr"][0].tolist() == [1.0, 1.0, 1.0]
    got = mcpt.direct_fold_host(lights, [0.0, 0.0, 0.0], [0, 1, 0], 1, spp=2)
    assert not got["irradiance"].any() and got["visibility"][0].tolist() == [0.0, 0.0]


# ---- refusals

def _dp(mcpt, spp=1, sample_base=0, seed=0, bias=0.01, flags=0, reserved=(0, 0, 0)):
    return mcpt.DirectParams(spp, sample_base, seed, bias, flags, (C.c_int32 * 3)(*reserved))


def _ptr(a, t=PD):
    return a.ctypes.data_as(t) if a is not None else None


def _addr(a):
    return a.ctypes.data if a is not None else None


class _Args:
    """valid arguments of every call for n entries under `lights`, each replaceable"""
    def __init__(self, mcpt, lights, n=4, spp=2):
        self.mcpt = mcpt
        self.arr = (mcpt.DirectLight * len(lights))(*lights) if lights else None
        self.nl = len(lights)
        self.n = n
        self.R = DR.slots(lights, spp)
        self.q = np.tile(np.array([0.0, 0.0, 0.0, 0.0, 1.0, 0.0]), (max(n, 1), 1))
        self.E = np.zeros((max(n, 1), 3))
        m = max(n * self.R, 1)
        self.rays, self.tmax, self.g, self.occ = np.zeros((m, 6)), np.zeros(m), np.zeros(m), np.zeros(m, dtype=np.uint8)
        self.map = mcpt.DirectMap(8, 8, 0, 0)
        self.Emap = np.zeros((8, 8, 3))


OWN = object()                                                  # "the _Args object's own array"


def _calls(L, a, dp, n=None, arr=OWN, nl=None, q=OWN, E=OWN, seam=OWN, fold_in=OWN, dm=OWN, Emap=OWN):
    """the seven calls' answers with a null device: [query, query_device, rays, fold_host, map, map_device] and slots"""
    n = a.n if n is None else n
    arr = a.arr if arr is OWN else arr
    nl = a.nl if nl is None else nl
    q = a.q if q is OWN else q
    E = a.E if E is OWN else E
    rays, tmax, g = (a.rays, a.tmax, a.g) if seam is OWN else seam
    fg, focc = (a.g, a.occ) if fold_in is OWN else fold_in
    dm = a.map if dm is OWN else dm
    Emap = a.Emap if Emap is OWN else Emap
    dpp = C.byref(dp) if dp is not None else None
    dmp = C.byref(dm) if dm is not None else None
    calls = [lambda: L.mcpt_query_direct(None, _ptr(q), None, n, arr, nl, dpp, _ptr(E), None, None, None, None),
             lambda: L.mcpt_query_direct_device(None, _addr(q), None, n, arr, nl, dpp, _addr(E), None, None, None, None),
             lambda: L.mcpt_direct_rays(None, _ptr(q), None, n, arr, nl, dpp, _ptr(rays), _ptr(tmax), _ptr(g)),
             lambda: L.mcpt_direct_fold_host(arr, nl, dpp, _ptr(fg), _ptr(focc, PU8), n, _ptr(E), None, None, None),
             lambda: L.mcpt_bake_direct_lightmap(None, None, dmp, arr, nl, dpp, _ptr(Emap), None, None, None, None, None),
             lambda: L.mcpt_bake_direct_lightmap_device(None, None, dmp, arr, nl, dpp, _addr(Emap), None, None, None, None, None, None)]
    got, a.msgs = [], []
    for call in calls:
        got.append(call())
        a.msgs.append(L.mcpt_last_error().decode())         # (each call's own message: a call that succeeds leaves the last one)
    return got


# the parameters' refusals in the header's order: each is refused with a message of its own and wins over everything after it
PARAM_ORDER = [("spp", dict(spp=0)), ("sample_base must be", dict(sample_base=-1)), ("sample_base + spp", dict(spp=2, sample_base=INT_MAX - 1)),
               ("bias", dict(bias=-1.0)), ("flags", dict(flags=1)), ("reserved", dict(reserved=(0, 0, 1)))]
PARAM_BAD = [dict(spp=-5), dict(sample_base=-2 ** 31), dict(spp=INT_MAX, sample_base=1), dict(bias=NAN), dict(bias=INF), dict(bias=-1e-300),
             dict(flags=-1), dict(reserved=(1, 0, 0)), dict(reserved=(0, -1, 0))]


def test_parameter_refusals_come_in_order_and_before_the_missing_device(mcpt):
    L = mcpt.lib()
    a = _Args(mcpt, _mix(mcpt, 5))
    assert _calls(L, a, None) == [ERR_ARG] * 6 and "null direct parameters" in _message(mcpt)
    for i, (word, kw) in enumerate(PARAM_ORDER):
        merged = {}
        for _, later in reversed(PARAM_ORDER[i:]):
            merged.update(later)
        merged.update(kw)
        # ... and over the lights, the count and the arrays
        assert _calls(L, a, _dp(mcpt, **merged), n=-1, arr=None, nl=-1, q=None, E=None, Emap=None) == [ERR_ARG] * 6 and word in _message(mcpt), (word, _message(mcpt))
    for kw in PARAM_BAD:
        assert _calls(L, a, _dp(mcpt, **kw)) == [ERR_ARG] * 6, kw
    assert L.mcpt_direct_slots(a.arr, a.nl, 0) == ERR_ARG and "spp" in _message(mcpt)
    # the limits pass: bias 0, the largest sample range
    nd = _null_device_rc(mcpt)
    for kw in (dict(bias=0.0), dict(spp=1, sample_base=INT_MAX - 1), dict(bias=1.7e308), dict(seed=2 ** 64 - 1)):
        got = _calls(L, _Args(mcpt, _mix(mcpt, 2), spp=1), _dp(mcpt, **kw))
        assert got == [nd, nd, nd, 0, nd, nd], (kw, got, _message(mcpt))


def _bad_lights(mcpt):
    """(word of the message, a light that must be refused), in the header's per-light order"""
    P, S, D, Rc = mcpt.point_light, mcpt.spot_light, mcpt.directional_light, mcpt.rect_light

    def edit(L, **kw):
        for k, v in kw.items():
            setattr(L, k, (C.c_double * 3)(*v) if isinstance(v, tuple) else v)
        return L
    ok_spot = lambda: S((0, 1, 0), (0, -1, 0), (1, 1, 1), 20.0, 30.0)
    ok_rect = lambda: Rc((0, 1, 0), (1, 0, 0), (0, 0, 1), (1, 1, 1))
    return [("unknown type", edit(P((0, 1, 0), (1, 1, 1)), type=4)), ("unknown type", edit(P((0, 1, 0), (1, 1, 1)), type=-1)),
            ("flags", edit(ok_rect(), flags=2)), ("flags", edit(ok_rect(), flags=3)), ("flags", edit(P((0, 1, 0), (1, 1, 1)), flags=1)),
            ("flags", edit(ok_spot(), flags=1)), ("flags", edit(D((0, -1, 0), (1, 1, 1)), flags=1)),
            ("not finite", P((NAN, 1, 0), (1, 1, 1))), ("not finite", P((0, 1, 0), (1, INF, 1))), ("not finite", P((0, 1, 0), (1, 1, 1), range=NAN)),
            ("not finite", edit(ok_spot(), direction=(0.0, -INF, 0.0))), ("not finite", edit(ok_spot(), cos_inner=NAN)),
            ("not finite", D((NAN, -1, 0), (1, 1, 1))), ("not finite", edit(ok_rect(), u=(1.0, NAN, 0.0))), ("not finite", edit(ok_rect(), v=(INF, 0.0, 0.0))),
            ("direction", edit(ok_spot(), direction=(0.0, 0.0, 0.0))), ("direction", D((0, 0, 0), (1, 1, 1))), ("direction", D((1.5e308, 1.5e308, 0), (1, 1, 1))),
            ("cross", edit(ok_rect(), v=(2.0, 0.0, 0.0))), ("cross", edit(ok_rect(), u=(0.0, 0.0, 0.0))), ("cross", edit(ok_rect(), u=(1e200, 0.0, 0.0), v=(0.0, 0.0, 1e200))),
            ("cosines", edit(ok_spot(), cos_inner=0.5, cos_outer=0.5)), ("cosines", edit(ok_spot(), cos_inner=0.2, cos_outer=0.7)),
            ("cosines", edit(ok_spot(), cos_inner=1.5, cos_outer=0.0)), ("cosines", edit(ok_spot(), cos_inner=0.5, cos_outer=-1.5)),
            ("range", P((0, 1, 0), (1, 1, 1), range=-1.0)), ("range", edit(ok_spot(), range=-1e-300))]


def test_light_refusals_come_in_order_and_before_the_missing_device(mcpt):
    L = mcpt.lib()
    nd = _null_device_rc(mcpt)
    good = _mix(mcpt, 5)
    a = _Args(mcpt, good)
    dp = _dp(mcpt, spp=2)
    # the count, then the array, over the entries' count and the arrays
    for nl in (-1, 4097, INT_MAX):
        assert _calls(L, a, dp, n=-1, nl=nl, q=None, E=None, Emap=None) == [ERR_ARG] * 6 and "lights" in _message(mcpt)
        assert L.mcpt_direct_slots(a.arr, nl, 2) == ERR_ARG
    assert _calls(L, a, dp, n=-1, arr=None, q=None, E=None, Emap=None) == [ERR_ARG] * 6 and "null lights" in _message(mcpt)
    assert L.mcpt_direct_slots(None, 5, 2) == ERR_ARG and "null lights" in _message(mcpt)
    # every bad light, alone and behind good ones: refused by every call with its own word, naming its index
    for word, bad in _bad_lights(mcpt):
        for lights in ([bad], good[:3] + [bad] + good[3:]):
            b = _Args(mcpt, lights)
            assert _calls(L, b, dp, n=-1, q=None, E=None, Emap=None) == [ERR_ARG] * 6, word
            assert word in _message(mcpt) and ("light %d" % (len(lights) - 1 if len(lights) == 1 else 3)) in _message(mcpt), (word, _message(mcpt))
            assert L.mcpt_direct_slots(b.arr, b.nl, 2) == ERR_ARG and word in _message(mcpt)
    # per light the order is the header's: the type before the flags before the components before the lengths before the cosines before the range
    chain = [("unknown type", dict(type=7)), ("flags", dict(flags=2)), ("not finite", dict(position=(NAN, 0.0, 0.0))), ("direction", dict(direction=(0.0, 0.0, 0.0))),
             ("cosines", dict(cos_inner=0.1, cos_outer=0.9)), ("range", dict(range=-1.0))]
    for i in range(len(chain)):
        spot = mcpt.spot_light((0, 1, 0), (0, -1, 0), (1, 1, 1), 20.0, 30.0)
        for _, kw in chain[i:]:                                 # fault i and every later one
            for k, v in kw.items():
                setattr(spot, k, (C.c_double * 3)(*v) if isinstance(v, tuple) else v)
        b = _Args(mcpt, [spot])
        assert _calls(L, b, dp) == [ERR_ARG] * 6 and chain[i][0] in _message(mcpt), (chain[i][0], _message(mcpt))
    # an earlier light's fault is reported before a later one's
    first = mcpt.point_light((0, 1, 0), (1, 1, 1), range=-1.0)
    second = mcpt.point_light((0, 1, 0), (1, 1, 1))
    second.type = 9
    assert _calls(L, _Args(mcpt, [first, second]), dp) == [ERR_ARG] * 6 and "light 0" in _message(mcpt) and "range" in _message(mcpt)
    # fields a type does not read are not looked at
    p = mcpt.point_light((0, 1, 0), (1, 1, 1))
    p.direction, p.u, p.cos_inner = (C.c_double * 3)(NAN, NAN, NAN), (C.c_double * 3)(INF, 0, 0), NAN
    d = mcpt.directional_light((0, -1, 0), (1, 1, 1))
    d.position, d.range, d.cos_outer = (C.c_double * 3)(NAN, NAN, NAN), -1.0, NAN
    r = mcpt.rect_light((0, 1, 0), (1, 0, 0), (0, 0, 1), (1, 1, 1))
    r.direction, r.range, r.cos_inner = (C.c_double * 3)(0, 0, 0), NAN, 9.0
    b = _Args(mcpt, [p, d, r], spp=2)
    assert _calls(L, b, dp) == [nd, nd, nd, 0, nd, nd], _message(mcpt)
    assert L.mcpt_direct_slots(b.arr, 3, 2) == 4
    # the limits of the cosines and the light count pass
    s = mcpt.spot_light((0, 1, 0), (0, -1, 0), (1, 1, 1), 0.0, 180.0)
    s.cos_inner, s.cos_outer = 1.0, -1.0
    assert L.mcpt_direct_slots((mcpt.DirectLight * 4096)(*([s] * 4096)), 4096, 1) == 4096


def test_count_and_array_refusals_come_last_and_before_the_missing_device(mcpt):
    L = mcpt.lib()
    nd = _null_device_rc(mcpt)
    lights = _mix(mcpt, 5)
    a = _Args(mcpt, lights, n=4, spp=2)
    dp = _dp(mcpt, spp=2)
    entry = [0, 1, 2, 3]                                        # the calls that take a list
    for n in (-1, 2 ** 31, 2 ** 40):
        got = _calls(L, a, dp, n=n, q=None, E=None)
        assert [got[i] for i in entry] == [ERR_ARG] * 4 and all("entries" in a.msgs[i] for i in entry)
    # n * R: R = 7 at spp 2 -- 306783378 entries fit (2147483646 slots), one more does not; the bound wins over the arrays
    assert a.R == 7
    for n, fits in ((306783378, True), (306783379, False), (INT_MAX, False)):
        got = _calls(L, a, dp, n=n, q=None, E=None)
        assert [got[i] for i in entry] == [ERR_ARG] * 4 and all(("slots" in a.msgs[i]) == (not fits) for i in entry), (n, a.msgs)
    big = _dp(mcpt, spp=INT_MAX)                                # a rectangle of 2^31 - 1 samples: R alone passes the bound with a second light
    b = _Args(mcpt, lights[:2], n=1, spp=1)
    got = _calls(L, b, big, n=1)
    assert [got[i] for i in entry] == [ERR_ARG] * 4 and all("slots" in b.msgs[i] for i in entry)
    # then the arrays
    got = _calls(L, a, dp, q=None)
    assert got[:3] == [ERR_ARG] * 3 and all("null" in m for m in a.msgs[:3])
    got = _calls(L, a, dp, E=None)
    assert [got[0], got[1], got[3]] == [ERR_ARG] * 3 and all("null" in a.msgs[i] for i in (0, 1, 3))
    for seam in ((None, a.tmax, a.g), (a.rays, None, a.g), (a.rays, a.tmax, None)):
        assert _calls(L, a, dp, seam=seam)[2] == ERR_ARG and "null" in a.msgs[2]
    for fold_in in ((None, a.occ), (a.g, None)):
        assert _calls(L, a, dp, fold_in=fold_in)[3] == ERR_ARG and "null" in a.msgs[3]
    # then the hemisphere kind's list checks, in the host-pointer forms alone
    for bad in (np.array([NAN, 0, 0, 0, 1, 0.0]), np.array([0, 0, 0, 0, 0, 0.0]), np.array([0, 0, 0, INF, 1, 0.0])):
        q = a.q.copy()
        q[2] = bad
        got = _calls(L, a, dp, q=q)
        assert got == [ERR_ARG, nd, ERR_ARG, 0, nd, nd], (bad, got)
    ids = np.array([0, 1, -1, 3], dtype=np.int32)
    assert L.mcpt_query_direct(None, _ptr(a.q), _ptr(ids, PI32), 4, a.arr, a.nl, C.byref(dp), _ptr(a.E), None, None, None, None) == ERR_ARG
    # the map: its own fields first and in order, then the parameters and lights, then the one required map
    D = mcpt.DirectMap
    assert _calls(L, a, dp, dm=None)[4:] == [ERR_ARG] * 2 and "null direct map" in _message(mcpt)
    for word, dm in (("16384", D(0, 8, -1, 1)), ("16384", D(8, 16385, -1, 1)), ("dilate", D(8, 8, -1, 1)), ("dilate", D(8, 8, 65, 1)), ("reserved", D(8, 8, 0, 1))):
        assert _calls(L, a, None, dm=dm, Emap=None)[4:] == [ERR_ARG] * 2 and word in _message(mcpt), (word, _message(mcpt))
    assert _calls(L, a, _dp(mcpt, spp=0), Emap=None)[4:] == [ERR_ARG] * 2 and "spp" in _message(mcpt)
    assert _calls(L, a, dp, Emap=None)[4:] == [ERR_ARG] * 2 and "null irradiance map" in _message(mcpt)
    # valid arguments: the host fold answers, the others miss the device; n == 0 needs no arrays; no lights at all is a call
    assert _calls(L, a, dp) == [nd, nd, nd, 0, nd, nd]
    assert _calls(L, a, dp, n=0, q=None, E=None, seam=(None, None, None), fold_in=(None, None)) == [nd, nd, nd, 0, nd, nd]
    assert _calls(L, _Args(mcpt, [], n=3), dp, seam=(None, None, None), fold_in=(None, None)) == [nd, nd, nd, 0, nd, nd]
    if nd == ERR_NO_DEVICE:
        assert _calls(L, a, dp)[0] == nd and "device" in _message(mcpt).lower()


def test_fold_host_leaves_absent_outputs_and_empty_lists_alone(mcpt):
    L = mcpt.lib()
    lights = _mix(mcpt, 5)
    arr = (mcpt.DirectLight * 5)(*lights)
    dp = _dp(mcpt, spp=2)
    g, occ = _factors("random", 3, 7, 1)
    E = np.full((3, 3), 7.5)
    assert L.mcpt_direct_fold_host(arr, 5, C.byref(dp), _ptr(g), _ptr(occ, PU8), 0, _ptr(E), None, None, None) == 0 and np.all(E == 7.5)
    assert L.mcpt_direct_fold_host(arr, 5, C.byref(dp), _ptr(g), _ptr(occ, PU8), 3, _ptr(E), None, None, None) == 0
    assert np.array_equal(_bits(E), _bits(DR.fold(lights, g, occ, 3, 2)["irradiance"]))
    # no lights: every output that is asked for is +0.0
    E, err = np.full((3, 3), 7.5), np.full((3, 3), -1.0)
    assert L.mcpt_direct_fold_host(None, 0, C.byref(dp), None, None, 3, _ptr(E), _ptr(err), None, None) == 0
    assert not _bits(E).any() and not _bits(err).any()


# ---- direct.hpp under the sanitizers

def _line(L, a, b, bias, xi1, xi2):
    v = [L.type, L.flags, *L.position, *L.direction, *L.u, *L.v, L.cos_inner, L.cos_outer, L.range, *a, *b, bias, xi1, xi2]
    return "slot " + " ".join(repr(float(x)) if not isinstance(x, int) else str(x) for x in v) + "\n"


def test_light_arithmetic_and_fold_under_address_and_undefined_sanitizers(mcpt, tmp_path):
    """A stand-alone program, not the library: nothing loaded into this process is instrumented."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "direct_sanitize")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "direct_sanitize_main.cpp")])
    lights = _mix(mcpt, 5) + [mcpt.point_light((0.0, 0.0, 0.0), (1, 1, 1)), mcpt.point_light((0.0, 0.005, 0.0), (1, 1, 1))]
    recv = [[0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [NAN, 0.0, 1.0], [INF, -INF, 1.0], [1.7e308, -1.7e308, 1.7e308], [1e-310, 5e-324, -5e-324],
            [0.25, -0.6, 0.8], [0.3, 2.0, -0.4]]
    normals = [[0.0, 1.0, 0.0], [0.0, -2.0, 0.0], [NAN, 1.0, 0.0], [INF, 1.0, 0.0], [1.7e308, 1.7e308, 0.0], [5e-324, 0.0, 0.0], [0.0, 0.0, 0.0], [0.3, 0.4, -0.5]]
    cases = [(l, L, a, b, bias) for l, L in enumerate(lights) for a in recv for b in normals for bias in (0.01, 0.0)]
    xi = (0.25, 0.625)
    text = "".join(_line(L, a, b, bias, *xi) for _, L, a, b, bias in cases)
    # the fold: n = 5 entries under the mix of five at spp 3, into arrays of exactly n * 3, n * nl * 3 and n * nl
    fl = _mix(mcpt, 5)
    n, spp = 5, 3
    R = DR.slots(fl, spp)
    g, occ = _factors("random", n, R, 3)
    text += "fold %d %d %d\n" % (n, spp, len(fl)) + "".join("%d %d %r %r %r\n" % (L.type, L.flags, *L.color) for L in fl)
    text += "".join("%r %d\n" % (float(g[k]), occ[k]) for k in range(n * R))
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases) + n

    def same(got, want):
        return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(_bits(got)[~np.isnan(got)], _bits(want)[~np.isnan(want)])
    bad, traced, within = 0, 0, 0
    for (l, L, a, b, bias), line in zip(cases, lines):
        got = np.array([float.fromhex(x) for x in line.split()])
        # the restatement with the program's uniforms in the place of the draw
        orig = DR.uniforms
        DR.uniforms = lambda seed, ids, k, ll: [np.full(1, xi[0]), np.full(1, xi[1])]
        try:
            with np.errstate(all="ignore"):
                rays, tmax, gg = DR.direct_rays([a], [b], [L], spp=1, bias=bias)
        finally:
            DR.uniforms = orig
        want = np.concatenate([rays[0], tmax, gg])
        bad += not same(got, want)
        traced += got[7] > 0
        within += got[7] > 0 and got[6] <= 0
        # a skipped slot is exactly o = a, d = 0, tmax = 0, g = +0.0
        if not got[7] > 0:
            assert same(got[:3], np.array(a)) and not _bits(got[3:]).any(), line
    assert bad == 0
    assert traced > 50 and within >= 1                          # slots are walked, and the light within bias has tmax <= 0 with g > 0
    # a light at the receiver (r2 = 0) is skipped
    at = [i for i, c in enumerate(cases) if c[0] == 5 and c[2] == [0.0, 0.0, 0.0] and c[3] == [0.0, 1.0, 0.0]]
    assert at and all(float.fromhex(lines[i].split()[7]) == 0.0 for i in at)
    want = DR.fold(fl, g, occ, n, spp)
    for i in range(n):
        got = np.array([float.fromhex(x) for x in lines[len(cases) + i].split()])
        w = np.concatenate([want["irradiance"][i], want["stderr"][i], want["per_light"][i].reshape(-1), want["visibility"][i]])
        assert np.array_equal(_bits(got), _bits(w)), i
