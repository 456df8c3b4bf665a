"""Not gpu: reflection probes (include/mcpt.h: reflection probes) as far as they go without a device.  The symbols and struct layouts
against the header; every refusal in the header's order, before the missing device; the octahedral map's properties (a texel's centre
lies in its own mcpt_visibility_bin, the solid angles sum to 4 pi); mcpt_reflection_texels, mcpt_reflection_prefilter_host and
mcpt_reflection_lookup_host against the numpy restatement (tests/reflection_ref.py) bit for bit; a constant and a linear map through
the prefilter, the seams, the empty lobe and the exactness of a level's own exponent; and reflection.hpp under the address and
undefined-behaviour sanitizers in a stand-alone program (tests/reflection_sanitize_main.cpp)."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import reflection_ref as RR
from conftest import ROOT

ERR_ARG, ERR_NO_DEVICE = -3, -4
NAMES = ["mcpt_reflection_texels", "mcpt_bake_reflection", "mcpt_bake_reflection_device", "mcpt_reflection_rays", "mcpt_reflection_prefilter_host",
         "mcpt_reflection_prefilter", "mcpt_reflection_prefilter_device", "mcpt_reflection_lookup_host", "mcpt_reflection_lookup",
         "mcpt_reflection_lookup_device"]
NAN, INF = float("nan"), float("inf")
CSRC = os.path.join(ROOT, "montecarlopathtracing_amd", "csrc")

# (source size, [(level size, exponent), ...]): source sizes 1, 2, 5, 17, 23, 32; level sizes 1, 4, 5, 16, 17; exponents 0, 1, 7, 64, 1000,
# 65535; chains of 1, 2 and 8 levels
CASES = [(1, [(4, 1)]),
         (2, [(5, 65535), (4, 0)]),
         (5, [(17, 65535), (16, 1000), (5, 64), (4, 7), (1, 3), (5, 2), (16, 1), (17, 0)]),
         (17, [(16, 64), (5, 1)]),
         (23, [(17, 7)]),
         (32, [(4, 1000), (17, 0)])]
PROBES = 2


def _null_device_rc(mcpt):
    return ERR_NO_DEVICE if mcpt.device_count() <= 0 else ERR_ARG


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def _pi(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None


def _addr(a):
    return a.ctypes.data if a is not None else None


MESSAGES = []        # the messages of the calls of the last helper, call by call


def _noting(L, rc):
    MESSAGES.append(L.mcpt_last_error().decode() if rc != 0 else "")
    return rc


def _said(word, calls=slice(None)):
    return all(word in m for m in MESSAGES[calls])


# ---- symbols and layouts

def test_reflection_symbols_are_declared_and_exported(mcpt):
    from montecarlopathtracing_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for sym in NAMES:
        assert (sym + "(") in hdr and sym in _lib.EXPORTS and hasattr(L, sym), sym
    for s in ("mcpt_reflection_params", "mcpt_reflection_chain"):
        assert ("} %s;" % s) in hdr
    assert "#define MCPT_VERSION 105" in hdr and mcpt.lib().mcpt_version() == 105
    for f in ("bake_reflection_probes", "bake_reflection_probes_device", "reflection_rays", "prefilter_reflection", "prefilter_reflection_device",
              "reflection_lookup", "reflection_lookup_device"):
        assert callable(getattr(mcpt.Device, f))
    for f in ("reflection_chain", "reflection_texels", "reflection_prefilter_host", "reflection_lookup_host"):
        assert callable(getattr(mcpt, f))
    block = hdr[hdr.index("---- reflection probes"):]
    assert "80 bytes per ray" in block and "Not covered:" in block
    for word in ("specular term in baked frames", "blending probes by position", "parallax correction", "GGX", "real-valued level exponents",
                 "fp32 or fp16 storage", "adaptive stopping", "multi-device group and render_scene"):
        assert word in block[block.index("Not covered:"):], word


def test_struct_layouts_match_the_header(mcpt, tmp_path):
    from montecarlopathtracing_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    if cc is None:
        pytest.skip("no C compiler")
    structs = [("mcpt_reflection_params", _lib.ReflectionParams, 48, ["spp", "sample_base", "seed", "res", "flags", "workspace_rays", "reserved"]),
               ("mcpt_reflection_chain", _lib.ReflectionChain, 88, ["res", "num_levels", "level_res", "level_ns", "reserved"])]
    body = ""
    for name, cls, _, fields in structs:
        assert [n for n, _ in cls._fields_] == fields
        body += "  printf(\"%%zu\\n\", sizeof(%s));\n" % name + "".join("  printf(\"%%zu\\n\", offsetof(%s, %s));\n" % (name, f) for f in fields)
    src = tmp_path / "layout_reflection.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"mcpt.h\"\nint main(void) {\n" + body + "  return 0;\n}\n")
    exe = tmp_path / "layout_reflection"
    subprocess.check_call([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    at = 0
    for name, cls, size, fields in structs:
        assert out[at] == C.sizeof(cls) == size, name
        for i, f in enumerate(fields):
            assert out[at + 1 + i] == getattr(cls, f).offset, (name, f)
        at += 1 + len(fields)


# ---- refusals

def _params(mcpt, spp=1, sample_base=0, res=2, flags=0, ws=0, reserved=0):
    return mcpt.ReflectionParams(spp, sample_base, 9, res, flags, ws, (C.c_int32 * 4)(0, 0, 0, reserved))


def _bakes(mcpt, p, n, p3, rad, id_base=None):
    """the return codes of the bake's host-pointer and device form and of the ray seam (one entry) on a NULL device"""
    L = mcpt.lib()
    pp = C.byref(p) if p is not None else None
    entry, rays, ids = np.zeros(1, dtype=np.int64), np.zeros((1, 6)), np.zeros(1, dtype=np.int32)
    del MESSAGES[:]
    return [_noting(L, L.mcpt_bake_reflection(None, _pd(p3), _pi(id_base), n, pp, _pd(rad), None, None, None)),
            _noting(L, L.mcpt_bake_reflection_device(None, _addr(p3), _addr(id_base), n, pp, _addr(rad), None, None, None, None)),
            _noting(L, L.mcpt_reflection_rays(None, _pd(p3), _pi(id_base), n, pp, entry.ctypes.data_as(C.POINTER(C.c_int64)), 1, _pd(rays), _pi(ids)))]


def test_bake_refusals_come_in_order_and_before_the_missing_device(mcpt):
    nd = _null_device_rc(mcpt)
    bad = [ERR_ARG] * 3
    p3, rad = np.zeros((3, 3)), np.zeros((3, 4, 3))
    assert _bakes(mcpt, None, -1, None, None) == bad and _said("null reflection parameters")
    # (spp, sample_base, res, flags, workspace_rays, reserved, n): each line mends the field the line before was refused for
    for (spp, base, res, flags, ws, reserved, n), word in (((0, -1, 0, 1, -1, 1, -1), "spp"), ((1, -1, 0, 1, -1, 1, -1), "sample_base"),
                                                           ((1, 0, 0, 1, -1, 1, -1), "res"), ((1, 0, 257, 1, -1, 1, -1), "res"),
                                                           ((1, 0, 256, 1, -1, 1, -1), "flag"), ((1, 0, 256, 4, -1, 1, -1), "flag"),
                                                           ((1, 0, 256, 2, -1, 1, -1), "workspace_rays"), ((1, 0, 256, 2, 0, 1, -1), "reserved"),
                                                           ((1, 0, 256, 0, 2 ** 40, 0, -1), "number of probes"),
                                                           ((1, 0, 256, 0, 0, 0, 2 ** 15), "2^31 - 1"), ((2 ** 31 - 1, 0, 2, 0, 0, 0, 1), "2^31 - 1"),
                                                           ((2 ** 29, 0, 2, 0, 0, 0, 1), "2^31 - 1"), ((1, 0, 256, 0, 0, 0, 2 ** 62), "2^31 - 1")):
        assert _bakes(mcpt, _params(mcpt, spp, base, res, flags, ws, reserved), n, None, None) == bad and _said(word), (word, MESSAGES)
    # the arrays, then -- in the host-pointer forms -- what they hold
    assert _bakes(mcpt, _params(mcpt), 3, None, rad)[:2] == bad[:2] and _said("null probe list or radiance", slice(0, 2))
    assert _bakes(mcpt, _params(mcpt), 3, p3, None)[:2] == bad[:2] and _said("null probe list or radiance", slice(0, 2))
    for v in (NAN, INF, -INF):
        q = p3.copy()
        q[1, 2] = v
        assert _bakes(mcpt, _params(mcpt), 3, q, rad) == [ERR_ARG, nd, ERR_ARG] and _said("probe 1", slice(0, 3, 2)), v
    assert _bakes(mcpt, _params(mcpt), 3, p3, rad, np.array([0, -1, 0], dtype=np.int32)) == [ERR_ARG, nd, ERR_ARG] and _said("negative id_base", slice(0, 3, 2))
    assert _bakes(mcpt, _params(mcpt), 3, p3, rad, np.array([0, 5, 2 ** 31 - 3], dtype=np.int32)) == [ERR_ARG, nd, ERR_ARG] and _said("probe 2", slice(0, 3, 2))
    # valid arguments miss the device; so do the limits themselves and n == 0, which needs no arrays
    assert _bakes(mcpt, _params(mcpt), 3, p3, rad, np.array([0, 5, 2 ** 31 - 4], dtype=np.int32)) == [nd] * 3
    assert _bakes(mcpt, _params(mcpt, spp=2 ** 29 - 1, flags=2, ws=2 ** 62), 1, p3, rad) == [nd] * 3
    assert _bakes(mcpt, _params(mcpt), 0, None, None)[:2] == [nd] * 2
    assert _said("device", slice(0, 2))
    # the seam's own: the count of entries, its arrays, an entry outside the call
    L = mcpt.lib()
    e, rays, ids = np.array([0, 12], dtype=np.int64), np.zeros((2, 6)), np.zeros(2, dtype=np.int32)
    pe = e.ctypes.data_as(C.POINTER(C.c_int64))
    p = _params(mcpt)
    assert L.mcpt_reflection_rays(None, _pd(p3), None, 3, C.byref(p), pe, -1, _pd(rays), _pi(ids)) == ERR_ARG
    assert L.mcpt_reflection_rays(None, _pd(p3), None, 3, C.byref(p), None, 2, _pd(rays), _pi(ids)) == ERR_ARG
    assert L.mcpt_reflection_rays(None, _pd(p3), None, 3, C.byref(p), pe, 2, _pd(rays), _pi(ids)) == ERR_ARG and "entry 1" in L.mcpt_last_error().decode()
    e[1] = 11
    assert L.mcpt_reflection_rays(None, _pd(p3), None, 3, C.byref(p), pe, 2, _pd(rays), _pi(ids)) == nd


def _chain(mcpt, res=2, levels=((2, 4), (1, 1)), **patch):
    c = mcpt.reflection_chain(res, levels)
    for k, v in patch.items():
        if k == "num_levels":
            c.num_levels = v
        else:
            getattr(c, k)[v[0]] = v[1]
    return c


def _chain_calls(mcpt, c, n=-1, rad=None, chain=None, m=-1, probe=None, d3=None, x=None, out=None):
    """the return codes of the three prefilter forms and the three lookup forms on a NULL device"""
    L = mcpt.lib()
    cc = C.byref(c) if c is not None else None
    filtered = chain.copy() if chain is not None else None          # the prefilter's output: the lookups read `chain` as it was given
    del MESSAGES[:]
    return [_noting(L, L.mcpt_reflection_prefilter_host(cc, _pd(rad), n, _pd(filtered))),
            _noting(L, L.mcpt_reflection_prefilter(None, cc, _pd(rad), n, _pd(filtered))),
            _noting(L, L.mcpt_reflection_prefilter_device(None, cc, _addr(rad), n, _addr(filtered), None)),
            _noting(L, L.mcpt_reflection_lookup_host(cc, _pd(chain), n, _pi(probe), _pd(d3), _pd(x), m, _pd(out))),
            _noting(L, L.mcpt_reflection_lookup(None, cc, _pd(chain), n, _pi(probe), _pd(d3), _pd(x), m, _pd(out))),
            _noting(L, L.mcpt_reflection_lookup_device(None, cc, _addr(chain), n, _addr(probe), _addr(d3), _addr(x), m, _addr(out), None))]


def test_chain_refusals_come_in_field_order_and_before_everything_else(mcpt):
    bad = [ERR_ARG] * 6
    assert _chain_calls(mcpt, None) == bad and _said("null reflection chain")
    for patch, word in ((dict(res=0), "res must be"), (dict(res=257), "res must be"), (dict(num_levels=0), "num_levels"), (dict(num_levels=9), "num_levels"),
                        (dict(level_res=(1, 0)), "level_res"), (dict(level_res=(0, 257)), "level_res"), (dict(level_res=(2, 1)), "level_res"),
                        (dict(level_ns=(0, -1)), "level_ns"), (dict(level_ns=(0, 65536)), "level_ns"), (dict(level_ns=(1, 4)), "level_ns"),
                        (dict(level_ns=(1, 5)), "level_ns"), (dict(level_ns=(7, 1)), "level_ns"), (dict(reserved=(3, 1)), "reserved")):
        c = _chain(mcpt, **({"res": patch.pop("res")} if "res" in patch else {}), **patch)
        assert _chain_calls(mcpt, c) == bad and _said(word), (word, MESSAGES)
    # a chain that mends a field and leaves the later ones bad is refused for the first of those
    c = _chain(mcpt, level_res=(1, 0), level_ns=(1, 9), reserved=(0, 1))
    assert _chain_calls(mcpt, c) == bad and _said("level_res")
    # the limits themselves pass: 8 levels, 256, 65535 and 0
    c = mcpt.reflection_chain(256, [(256, 65535), (1, 7), (2, 6), (3, 5), (4, 4), (5, 3), (6, 1), (256, 0)])
    assert _chain_calls(mcpt, c) == bad and _said("number of probes")


def test_prefilter_and_lookup_refusals_come_in_order_and_before_the_missing_device(mcpt):
    nd = _null_device_rc(mcpt)
    c = _chain(mcpt)
    rad, chain = np.ones((2, 4, 3)), np.ones((2, 5, 3))
    probe, d3, x, out = np.array([0, 1, 1], dtype=np.int32), np.tile([0.0, 0.6, -0.8], (3, 1)), np.array([0.0, 2.5, 9.0]), np.zeros((3, 3))
    for n in (-1, 2 ** 31, 2 ** 40):
        assert _chain_calls(mcpt, c, n=n) == [ERR_ARG] * 6 and _said("number of probes")
    for m in (-1, 2 ** 31):
        assert _chain_calls(mcpt, c, n=2, rad=rad, chain=chain, m=m)[3:] == [ERR_ARG] * 3 and _said("number of receivers", slice(3, 6))
    assert _chain_calls(mcpt, c, n=2, rad=None, chain=chain)[:3] == [ERR_ARG] * 3 and _said("null radiance or chain", slice(0, 3))
    assert _chain_calls(mcpt, c, n=2, rad=rad, chain=None)[:3] == [ERR_ARG] * 3 and _said("null radiance or chain", slice(0, 3))
    for drop in range(5):
        args = [chain, probe, d3, x, out]
        args[drop] = None
        assert _chain_calls(mcpt, c, 2, rad, args[0], 3, *args[1:])[3:] == [ERR_ARG] * 3 and _said("null chain", slice(3, 6)), drop
    # the host-pointer forms look at the values; the device forms do not
    for v in (NAN, INF, -INF):
        r2 = rad.copy()
        r2[1, 3, 2] = v
        assert _chain_calls(mcpt, c, 2, r2, chain, 3, probe, d3, x, out)[:3] == [ERR_ARG, ERR_ARG, nd] and _said("not finite", slice(0, 2))
        c2 = chain.copy()
        c2[0, 4, 1] = v
        assert _chain_calls(mcpt, c, 2, rad, c2, 3, probe, d3, x, out)[3:] == [ERR_ARG, ERR_ARG, nd] and _said("the chain", slice(3, 5))
    for bad_d in ([0.0, 0.0, 0.0], [NAN, 0.0, 1.0], [INF, 0.0, 1.0], [1e308, 1e308, 1e308]):
        d2 = d3.copy()
        d2[1] = bad_d
        assert _chain_calls(mcpt, c, 2, rad, chain, 3, probe, d2, x, out)[3:] == [ERR_ARG, ERR_ARG, nd] and _said("receiver 1: direction", slice(3, 5)), bad_d
    for bad_p in (-1, 2):
        p2 = probe.copy()
        p2[2] = bad_p
        assert _chain_calls(mcpt, c, 2, rad, chain, 3, p2, d3, x, out)[3:] == [ERR_ARG, ERR_ARG, nd] and _said("receiver 2: probe index", slice(3, 5)), bad_p
    for bad_x in (-1e-300, NAN, INF):
        x2 = x.copy()
        x2[0] = bad_x
        assert _chain_calls(mcpt, c, 2, rad, chain, 3, probe, d3, x2, out)[3:] == [ERR_ARG, ERR_ARG, nd] and _said("receiver 0: the exponent", slice(3, 5)), bad_x
    # valid arguments: the host forms answer, the others miss the device; n == 0 and m == 0 need no arrays
    assert _chain_calls(mcpt, c, 2, rad, chain, 3, probe, d3, x, out) == [0, nd, nd, 0, nd, nd]
    if nd == ERR_NO_DEVICE:
        assert "device" in mcpt.lib().mcpt_last_error().decode().lower()
    assert _chain_calls(mcpt, c, n=0, m=0) == [0, nd, nd, 0, nd, nd]
    # mcpt_reflection_texels: the size; either pointer may be NULL
    L = mcpt.lib()
    for res in (0, -1, 257):
        assert L.mcpt_reflection_texels(res, None, None) == ERR_ARG and "res" in L.mcpt_last_error().decode()
    d, w = np.zeros((4, 3)), np.zeros(4)
    assert L.mcpt_reflection_texels(2, _pd(d), None) == 0 and L.mcpt_reflection_texels(2, None, _pd(w)) == 0 and L.mcpt_reflection_texels(256, None, None) == 0
    assert _same(d, RR.texels(2)[0]) and _same(w, RR.texels(2)[1])


def test_api_validates_shapes(mcpt):
    c = mcpt.reflection_chain(2, [(2, 4), (1, 1)])
    assert (c.res, c.num_levels, list(c.level_res), list(c.level_ns), c.num_texels) == (2, 2, [2, 1, 0, 0, 0, 0, 0, 0], [4, 1, 0, 0, 0, 0, 0, 0], 5)
    with pytest.raises(ValueError):
        mcpt.reflection_chain(2, [(1, 1)] * 9)
    with pytest.raises(ValueError):
        mcpt.reflection_chain(2, [(1, 1.5)])
    with pytest.raises(ValueError):
        mcpt.reflection_texels(2.0)
    with pytest.raises(ValueError):
        mcpt.reflection_prefilter_host(c, np.ones((2, 5, 3)))
    with pytest.raises(ValueError):
        mcpt.reflection_lookup_host(c, np.ones((2, 4, 3)), [0], [[0, 0, 1.0]], 1.0)
    with pytest.raises(ValueError):
        mcpt.reflection_lookup_host(c, np.ones((2, 5, 3)), [0, 1], [[0, 0, 1.0]], 1.0)
    with pytest.raises(ValueError):
        mcpt.reflection_lookup_host(c, np.ones((2, 5, 3)), [0.5], [[0, 0, 1.0]], 1.0)
    assert mcpt.reflection_lookup_host(c, np.ones((2, 5, 3)), [1], [[0, 0, 2.0]], 1.0).tolist() == [[1.0, 1.0, 1.0]]
    with pytest.raises(mcpt.McptError):
        mcpt.reflection_texels(0)


# ---- the map

def test_restatement_against_hand_computations():
    # the six axes: the square's centre, the middles of its edges' halves, its corners' direction
    st = RR.encode([[0, 0, 2.0], [3.0, 0, 0], [0, -4.0, 0], [0, 0, -1.0], [1.0, 1.0, 0.0]])
    assert st.tolist() == [[0.5, 0.5], [1.0, 0.5], [0.5, 0.0], [1.0, 1.0], [0.75, 0.75]]
    assert RR.decode([0.5, 1.0, 0.0], [0.5, 0.5, 0.0]).tolist() == [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [-0.0, -0.0, -1.0]]
    # the wrap: an edge reflects the tap back and mirrors the other coordinate; a corner does both in turn and lands on the corner
    # opposite -- all four corners are the direction (0, 0, -1)
    x, y = RR.wrap(4, [-1, 4, 1, 2, -1, 4], [1, 1, -1, 4, -1, 4])
    assert list(zip(x.tolist(), y.tolist())) == [(0, 2), (3, 2), (2, 0), (1, 3), (3, 3), (0, 0)]
    x, y = RR.wrap(1, [-1, 0, 1, 1], [0, 1, -1, 1])
    assert x.tolist() == [0] * 4 and y.tolist() == [0] * 4
    assert RR.ipow(np.array([2.0, 0.5, 3.0]), 0).tolist() == [1.0, 1.0, 1.0] and RR.ipow(np.array([2.0, 0.5, 3.0]), 5).tolist() == [32.0, 0.03125, 243.0]
    assert RR.ipow(np.array([0.9]), 65535)[0] == 0.0 and RR.ipow(np.array([1.0]), 65535)[0] == 1.0
    # the fold of S = 2 and of S = 1
    mean, err, hits = RR.fold(np.array([[[1.0, 2.0, 4.0], [3.0, 2.0, 0.0]]]), np.array([[1, 0]]))
    assert mean.tolist() == [[2.0, 2.0, 2.0]] and err.tolist() == [[1.0, 0.0, 2.0]] and hits.tolist() == [1]
    mean, err, hits = RR.fold(np.array([[[1.0, 2.0, 4.0]]]), np.array([[1]]))
    assert mean.tolist() == [[1.0, 2.0, 4.0]] and err.tolist() == [[0.0, 0.0, 0.0]] and hits.tolist() == [1]
    # entries: probe 1, texel 2, sample 1 of R = 2, S = 3 is entry (1 * 4 + 2) * 3 + 1; its id follows id_base
    rays, ids = RR.rays([[0.0, 0, 0], [1.0, 2.0, 3.0]], 2, 3, [19], seed=5, id_base=[100, 1000])
    assert ids.tolist() == [1007] and rays[0, :3].tolist() == [1.0, 2.0, 3.0]
    st = RR.encode(rays[:, 3:])
    assert 0.0 <= st[0, 0] <= 0.5 and 0.5 <= st[0, 1] <= 1.0                 # texel 2 = (x 0, y 1) of 2 x 2
    assert RR.rays([[0.0, 0, 0], [1.0, 2.0, 3.0]], 2, 3, [19], seed=5)[1].tolist() == [19]


@pytest.mark.parametrize("R", list(range(1, 17)))
def test_a_texels_centre_lies_in_its_own_visibility_bin(mcpt, R):
    d, w = mcpt.reflection_texels(R)
    rd, rw = RR.texels(R)
    assert _same(d, rd) and _same(w, rw)
    assert np.array_equal(mcpt.visibility_bin(d, R), np.arange(R * R))
    assert np.abs(np.sqrt((d * d).sum(axis=1)) - 1.0).max() <= 4e-16 and (w > 0).all()
    # encode is decode's inverse at the centres (away from the seams' sign choice: compared through the bin above and here by value)
    b = np.arange(R * R)
    centre = np.stack([((b % R) + 0.5) / R, ((b // R) + 0.5) / R], axis=1)
    st = RR.encode(d)
    inner = (np.abs(np.abs(2 * centre[:, 0] - 1) + np.abs(2 * centre[:, 1] - 1) - 1.0) > 1e-9)      # not on the equator's diagonal
    assert np.abs(st - centre)[inner].max(initial=0.0) <= 1e-14             # a handful of roundings of numbers of size 1


@pytest.mark.parametrize("R,bound", [(16, 1e-5), (64, 1e-7), (256, 1e-7)])
def test_solid_angles_sum_to_the_sphere(mcpt, R, bound):
    """the midpoint rule's error: measured 1.76e-6 at R = 16 and 7.5e-9 at R = 64"""
    d, w = mcpt.reflection_texels(R)
    assert _same(d, RR.texels(R)[0]) and _same(w, RR.texels(R)[1])
    rel = math.fsum(w.tolist()) / (4.0 * math.pi) - 1.0
    print("R = %d: the solid angles' sum is off 4 pi by %.3e" % (R, rel))
    assert abs(rel) <= bound


# ---- bit for bit against the restatement

@pytest.fixture(scope="module")
def chains(mcpt):
    """per case: the source maps, the chain struct, the restatement's chain, the receivers and the restatement's answers"""
    out = []
    for R, levels in CASES:
        L = RR.source_map(PROBES, R)
        want = RR.prefilter(L, R, levels)
        d, x = RR.receivers(levels)
        probe = (np.arange(d.shape[0]) * 7 % PROBES).astype(np.int32)
        out.append((R, levels, L, mcpt.reflection_chain(R, levels), want, probe, d, x, RR.lookup(want, levels, probe, d, x)))
    return out


@pytest.mark.parametrize("case", range(len(CASES)))
def test_host_prefilter_is_the_restatement_bit_for_bit(mcpt, chains, case):
    """fp64 add, multiply, divide and sqrt only: equality is asserted"""
    R, levels, L, c, want, _, _, _, _ = chains[case]
    got = mcpt.reflection_prefilter_host(c, L)
    assert got.shape == (PROBES, RR.chain_texels(levels), 3) and np.isfinite(got).all()
    assert _same(got, want), "%d of %d values differ" % ((_bits(got) != _bits(want)).sum(), got.size)
    assert not (got < 0).any() and not (_bits(got) == _bits(np.array(-0.0))).any()
    # a permuted list of probes gives permuted chains
    assert _same(mcpt.reflection_prefilter_host(c, L[::-1]), want[::-1])


@pytest.mark.parametrize("case", range(len(CASES)))
def test_host_lookup_is_the_restatement_bit_for_bit(mcpt, chains, case):
    R, levels, _, c, chain, probe, d, x, want = chains[case]
    ns = [e for _, e in levels]
    assert d.shape[0] >= 4000 + RR.chain_texels(levels) and (np.abs(d) == 1e300).any() and (np.abs(d) == 1e-300).any() and (d[:, 2] == 0).any()
    assert all((x == e).any() for e in ns) and (x > ns[0]).any() and (len(ns) < 2 or ((x < ns[0]) & (x > ns[-1])).any())
    got = mcpt.reflection_lookup_host(c, chain, probe, d, x)
    assert _same(got, want), "%d of %d values differ" % ((_bits(got) != _bits(want)).sum(), got.size)
    assert np.isfinite(got).all()
    perm = np.random.default_rng(3).permutation(d.shape[0])
    assert _same(mcpt.reflection_lookup_host(c, chain, probe[perm], d[perm], x[perm]), want[perm])


@pytest.mark.parametrize("case", range(len(CASES)))
def test_a_levels_own_exponent_reads_that_level_alone(mcpt, chains, case):
    """x == ns[l]: the value is the lookup in a chain that holds level l only, bit for bit; and a texel's centre reads the texel"""
    R, levels, _, c, chain, _, _, _, _ = chains[case]
    first = 0
    d = RR.receivers(levels, seed=11, n_random=500)[0]
    probe = (np.arange(d.shape[0]) % PROBES).astype(np.int32)
    for Rl, ns in levels:
        alone = np.ascontiguousarray(chain[:, first:first + Rl * Rl, :])
        got = mcpt.reflection_lookup_host(c, chain, probe, d, float(ns))
        want = mcpt.reflection_lookup_host(mcpt.reflection_chain(R, [(Rl, ns)]), alone, probe, d, 123.0)
        assert _same(got, want), (Rl, ns)
        # the centre's s * R - 0.5 is a whole number but for the rounding of encode(decode()): the other taps weigh 1e-16 or so
        at = mcpt.reflection_lookup_host(c, chain, np.zeros(Rl * Rl, dtype=np.int32), RR.texels(Rl)[0], float(ns))
        assert np.abs(at - chain[0, first:first + Rl * Rl, :]).max() <= 1e-12 * chain[0].max(), (Rl, ns)
        first += Rl * Rl


# ---- properties

def test_a_constant_map_prefilters_to_the_constant(mcpt):
    """W and A are sequential sums of R_src^2 terms of one sign: first-order bound 2 R_src^2 ulps on their quotient.  Measured: at most
    48 ulps at R = 64"""
    value = np.array([3.7, 0.1, 1e6])
    worst = {}
    for R in (5, 23, 64):
        c = mcpt.reflection_chain(R, [(8, 1000), (8, 64), (8, 1), (8, 0)])
        got = mcpt.reflection_prefilter_host(c, np.broadcast_to(value, (1, R * R, 3)))
        assert (got > 0).all()
        worst[R] = float((np.abs(got - value) / np.spacing(value)).max())
        assert worst[R] <= 2.0 * R * R, worst
    print("a constant map is off the constant by at most %r ulps" % worst)


def test_a_linear_map_prefilters_to_the_lobes_mean(mcpt):
    """L = d.z under cos^ns about r: the hemisphere integral of cos^ns d.z over that of cos^ns is r.z (ns + 1) / (ns + 2).  Source 64, level
    8, measured 1.3e-4, 1.0e-4, 9.7e-6 and 1.1e-5 for ns = 1, 8, 64 and 512"""
    R, Ro = 64, 8
    dz = RR.texels(R)[0][:, 2]
    rz = RR.texels(Ro)[0][:, 2]
    L = np.repeat(dz[None, :, None], 3, axis=2)
    seen = {}
    for ns in (1, 8, 64, 512):
        got = mcpt.reflection_prefilter_host(mcpt.reflection_chain(R, [(Ro, ns)]), L)[0, :, 0]
        seen[ns] = float(np.abs(got - rz * (ns + 1.0) / (ns + 2.0)).max())
    print("L = d.z prefilters to r.z (ns + 1) / (ns + 2) within %r" % seen)
    assert all(seen[ns] <= 1e-3 for ns in (1, 8, 64)), seen


@pytest.mark.parametrize("R", [1, 2, 5, 16])
def test_the_lookup_is_continuous_across_the_seams(mcpt, R):
    """a level sampled from a linear function of the direction: directions 1e-13 either side of x = 0 and of y = 0 below the horizon, and
    of z = 0, read values within 1e-9 of one another (measured <= 1.7e-10; a wrong wrap is off by the map's own range)"""
    cen = RR.texels(R)[0]
    level = (cen @ np.array([[1.0, -2.0, 0.5], [0.7, 0.3, -1.1], [-0.4, 1.3, 0.9]]) + np.array([2.0, 3.0, 4.0]))[None]
    c = mcpt.reflection_chain(R, [(R, 7)])
    t = np.linspace(-0.95, 0.95, 39)
    e = 1e-13
    worst = 0.0
    for lo, hi in ((np.stack([np.full_like(t, -e), t, np.full_like(t, -0.4)], 1), np.stack([np.full_like(t, e), t, np.full_like(t, -0.4)], 1)),
                   (np.stack([t, np.full_like(t, -e), np.full_like(t, -0.4)], 1), np.stack([t, np.full_like(t, e), np.full_like(t, -0.4)], 1)),
                   (np.stack([t, 1.0 - np.abs(t), np.full_like(t, -e)], 1), np.stack([t, 1.0 - np.abs(t), np.full_like(t, e)], 1)),
                   (np.stack([t, np.abs(t) - 1.0, np.full_like(t, -e)], 1), np.stack([t, np.abs(t) - 1.0, np.full_like(t, e)], 1))):
        z = np.zeros(lo.shape[0], dtype=np.int32)
        a, b = mcpt.reflection_lookup_host(c, level, z, lo, 7.0), mcpt.reflection_lookup_host(c, level, z, hi, 7.0)
        assert _same(a, RR.lookup(level, [(R, 7)], z, lo, 7.0)) and _same(b, RR.lookup(level, [(R, 7)], z, hi, 7.0))
        worst = max(worst, float(np.abs(a - b).max()))
    print("R = %d: the lookup jumps by at most %.3e across a seam" % (R, worst))
    assert worst <= 1e-9


def test_an_empty_lobe_gives_plus_zero(mcpt, chains):
    # a 1 x 1 source lies at +z: of a 4 x 4 level the four inner texels see it and the twelve on the rim (z <= 0) see nothing
    R, levels, L, c, want, _, _, _, _ = chains[0]
    assert (R, levels) == (1, [(4, 1)])
    got = mcpt.reflection_prefilter_host(c, L)
    empty = ~(got != 0).any(axis=2)
    assert empty.sum(axis=1).tolist() == [12, 12] and not _bits(got[empty]).any()
    inner = [5, 6, 9, 10]
    assert not empty[:, inner].any() and (np.abs(got[:, inner, :] - L) <= 2 * np.spacing(L)).all()       # (g L) / g: the one texel itself
    # cos^65535 underflows between the four texels of a 2 x 2 source and most of a 5 x 5 level
    R, levels, L, c, want, _, _, _, _ = chains[1]
    assert (R, levels[0]) == (2, (5, 65535))
    got = mcpt.reflection_prefilter_host(c, L)[:, :25, :]
    empty = ~(got != 0).any(axis=2)
    assert empty.any() and not _bits(got[empty]).any() and _same(got, want[:, :25, :])


# ---- reflection.hpp under the sanitizers

def test_prefilter_and_lookup_under_address_and_undefined_sanitizers(tmp_path):
    """A stand-alone program, not the library: nothing loaded into this process is instrumented."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "reflection_sanitize")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "reflection_sanitize_main.cpp")])
    edge = [NAN, INF, -INF, 1e300, -1e300, 1e-300, -1e-300, 0.0, -0.0, 1.0, -0.5]
    xs = [0.0, 1.0, 64.5, NAN, INF, -1.0, 1e300, 7.0, 3.5]
    probes_of = [-1, 0, 1, 2, 3, 2 ** 31, -2 ** 40]
    dirs = [(a, b, c) for a in edge for b in edge for c in edge]
    for R, levels, n in ((1, [(4, 7), (1, 0)], 2), (5, [(5, 65535), (4, 64), (1, 1)], 3)):
        recv = [(probes_of[i % len(probes_of)], d, xs[i % len(xs)]) for i, d in enumerate(dirs)]
        text = "%d %d %d\n" % (R, len(levels), n) + "".join("%d %d\n" % l for l in levels) + "".join("%d %r %r %r %r\n" % ((p,) + d + (x,)) for p, d, x in recv)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
        vals = np.array([[float.fromhex(v) for v in l.split()] for l in out.stdout.splitlines()])
        T = RR.chain_texels(levels)
        assert vals.shape == (n * T + len(recv), 3)
        b = np.arange(R * R)
        L = (7.0 * np.arange(n)[:, None, None] + 3.0 * b[None, :, None] + np.arange(3)[None, None, :] + 1.0) / 8.0
        chain = RR.prefilter(L, R, levels)
        assert _same(vals[:n * T].reshape(n, T, 3), chain)
        got = vals[n * T:]
        d = np.array([r[1] for r in recv])
        p, x = np.array([r[0] for r in recv]), np.array([r[2] for r in recv])
        with np.errstate(all="ignore"):
            l = np.abs(d).sum(axis=1)
        inside = (p >= 0) & (p < n)
        ok = inside & np.isfinite(l) & (l > 0) & np.isfinite(x) & (x >= 0)
        assert ok.sum() > 50
        assert _same(got[ok], RR.lookup(chain, levels, p[ok], d[ok], x[ok]))
        assert not _bits(got[~inside]).any()                                  # a probe out of range: +0.0
