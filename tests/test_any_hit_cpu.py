"""Not gpu: any-hit rays (include/mcpt.h: any-hit rays) as far as they go without a device.  The five symbols and the struct's layout
against the header; every refusal of the five calls in the header's order, before the missing device; mcpt_pair_rays against the numpy
restatement (tests/any_hit_ref.py) bit for bit -- (na, nb) = (1, 1), (3, 63), (2, 64), (5, 65), random points, a == b, and components
0, -0, 1e+-300 and denormals, under (t0, t1) = (0, 1), (1e-4, 1 - 1e-4), (0.25, 0.5) --; empty lists, which leave the caller's arrays
untouched; the restatement's packing against hand values; and the host-compiled parts of any_hit.hpp under the address and
undefined-behaviour sanitizers in a stand-alone program (tests/any_hit_sanitize_main.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import any_hit_ref as AR
from conftest import ROOT

CSRC = os.path.join(ROOT, "montecarlopathtracing_amd", "csrc")
ERR_ARG, ERR_NO_DEVICE = -3, -4
NAMES = ["mcpt_trace_any", "mcpt_trace_any_device", "mcpt_pair_rays", "mcpt_trace_any_pairs", "mcpt_trace_any_pairs_device"]
PD, PU8, PU64 = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
INT_MAX = 2 ** 31 - 1
NAN, INF = float("nan"), float("inf")
SHAPES = [(1, 1), (3, 63), (2, 64), (5, 65)]
INTERVALS = [(0.0, 1.0), (1e-4, 1.0 - 1e-4), (0.25, 0.5)]


def _null_device_rc(mcpt):
    return ERR_NO_DEVICE if mcpt.device_count() <= 0 else ERR_ARG


def _message(mcpt):
    return mcpt.lib().mcpt_last_error().decode()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_any_hit_symbols_are_declared_and_exported(mcpt):
    from montecarlopathtracing_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for sym in NAMES:
        assert (sym + "(") in hdr and sym in _lib.EXPORTS and hasattr(L, sym), sym
    assert "} mcpt_pair_params;" in hdr
    assert "#define MCPT_VERSION 105" in hdr and mcpt.lib().mcpt_version() == 105
    for f in ("any_hit", "any_hit_pairs"):
        assert callable(getattr(mcpt.Device, f))
    assert callable(mcpt.pair_rays)


def test_pair_params_layout_matches_the_header(mcpt, tmp_path):
    from montecarlopathtracing_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    if cc is None:
        pytest.skip("no C compiler")
    fields = ["t0", "t1", "flags", "reserved"]
    assert [n for n, _ in _lib.PairParams._fields_] == fields
    body = "  printf(\"%zu\\n\", sizeof(mcpt_pair_params));\n" + "".join("  printf(\"%%zu\\n\", offsetof(mcpt_pair_params, %s));\n" % f for f in fields)
    src = tmp_path / "layout_any.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"mcpt.h\"\nint main(void) {\n" + body + "  return 0;\n}\n")
    exe = tmp_path / "layout_any"
    subprocess.check_call([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert out[0] == C.sizeof(_lib.PairParams) == 24
    for i, f in enumerate(fields):
        assert out[1 + i] == getattr(_lib.PairParams, f).offset, f


# ---- mcpt_pair_rays against the restatement

def _points(kind, na, nb, seed=0):
    rng = np.random.default_rng([seed, na, nb])
    if kind == "random":
        return rng.normal(size=(na, 3)) * 3.0, rng.normal(size=(nb, 3)) * 3.0
    if kind == "same":
        p = rng.normal(size=(max(na, nb), 3))
        return p[:na].copy(), p[:nb].copy()
    edge = np.array([0.0, -0.0, 1e300, -1e300, 1e-300, -1e-300, 5e-324, -5e-324, 2.5e-310, 1.0, -3.0])
    return edge[rng.integers(edge.size, size=(na, 3))], edge[rng.integers(edge.size, size=(nb, 3))]


@pytest.mark.parametrize("t0,t1", INTERVALS)
@pytest.mark.parametrize("kind", ["random", "same", "edge"])
@pytest.mark.parametrize("na,nb", SHAPES)
def test_pair_rays_are_the_restatement_bit_for_bit(mcpt, na, nb, kind, t0, t1):
    a, b = _points(kind, na, nb)
    rays, tmax = mcpt.pair_rays(a, b, t0, t1)
    want, want_tmax = AR.pair_rays(a, b, t0, t1)
    assert rays.shape == (na * nb, 6) and np.array_equal(_bits(rays), _bits(want))
    assert _bits(np.array([tmax]))[0] == _bits(np.array([want_tmax]))[0] and tmax == t1 - t0
    # the restatement against its own words, entry by entry: d = b - a, o = a + (t0 * d), pair (i, j) at i * nb + j
    i, j = na - 1, nb - 1
    with np.errstate(all="ignore"):
        d = b[j] - a[i]
        o = a[i] + np.float64(t0) * d
    assert np.array_equal(_bits(want[i * nb + j]), _bits(np.concatenate([o, d])))
    if kind == "same":
        k = min(na, nb) - 1
        assert not want[k * nb + k, 3:].any() and np.array_equal(_bits(want[k * nb + k, :3]), _bits(a[k] + np.float64(t0) * np.zeros(3)))


def test_the_restatements_packing_against_hand_values():
    m = np.zeros((2, 65), dtype=bool)
    m[0, 0] = m[0, 63] = m[0, 64] = m[1, 1] = True
    bits = AR.pack(m)
    assert bits.shape == (2, 2) and bits.dtype == np.uint64
    assert bits.tolist() == [[(1 << 63) | 1, 1], [2, 0]]
    assert np.array_equal(AR.unpack(bits, 65), m) and not AR.padding(bits, 65).any()
    bits[1, 1] = np.uint64(2)                                    # column 65 of a row of 65: padding
    assert AR.padding(bits, 65).tolist() == [0, 1] and np.array_equal(AR.unpack(bits, 65), m)
    assert [AR.row_words(n) for n in (0, 1, 63, 64, 65, 128, 129)] == [0, 1, 1, 1, 2, 2, 3]
    assert AR.pack(np.zeros((3, 0), dtype=bool)).shape == (3, 0)
    # the rule: strict, IEEE, misses never
    face, t = np.array([0, 3, -1, 2, 2]), np.array([1.0, 1.0, 0.5, 1.0, 1.0])
    assert AR.occluded(face, t, np.array([1.0, np.nextafter(1.0, 2.0), 9.0, NAN, INF])).tolist() == [False, True, False, False, True]
    assert AR.occluded(face, t, None).tolist() == [True, True, False, True, True]
    assert AR.occluded(face, t, 0.0).tolist() == [False] * 5


# ---- refusals

def _pp(mcpt, t0=0.0, t1=1.0, flags=0, reserved=0):
    return mcpt.PairParams(t0, t1, flags, reserved)


def _ptr(a, t=PD):
    return a.ctypes.data_as(t) if a is not None else None


def _addr(a):
    return a.ctypes.data if a is not None else None


def _ray_calls(L, rays, tmax, n, occ):
    """the two ray forms with a null device (the device form's pointers are not looked at)"""
    return [L.mcpt_trace_any(None, _ptr(rays), _ptr(tmax), n, _ptr(occ, PU8), None),
            L.mcpt_trace_any_device(None, _addr(rays), _addr(tmax), n, _addr(occ), None)]


def _pair_calls(L, pp, a, na, b, nb, bits, rays=None, tmax=None):
    """the host function and the two matrix forms with a null device"""
    ppp = C.byref(pp) if pp is not None else None
    return [L.mcpt_pair_rays(_ptr(a), na, _ptr(b), nb, ppp, _ptr(rays), _ptr(tmax)),
            L.mcpt_trace_any_pairs(None, _ptr(a), na, _ptr(b), nb, ppp, _ptr(bits, PU64), None),
            L.mcpt_trace_any_pairs_device(None, _addr(a), na, _addr(b), nb, ppp, _addr(bits), None)]


def test_ray_refusals_come_in_order_and_before_the_missing_device(mcpt):
    L = mcpt.lib()
    nd = _null_device_rc(mcpt)
    rays, tmax, occ = np.zeros((8, 6)), np.ones(8), np.zeros(8, dtype=np.uint8)
    # the count wins over the arrays
    for n in (-1, 2 ** 31, 2 ** 40):
        assert _ray_calls(L, None, None, n, None) == [ERR_ARG] * 2 and "rays" in _message(mcpt)
    assert _ray_calls(L, None, tmax, 8, occ) == [ERR_ARG] * 2 and "null" in _message(mcpt)
    assert _ray_calls(L, rays, tmax, 8, None) == [ERR_ARG] * 2 and "null" in _message(mcpt)
    # valid arguments miss the device; the limits may be absent; the bound itself passes; n == 0 needs no arrays
    assert _ray_calls(L, rays, tmax, 8, occ) == [nd] * 2
    assert _ray_calls(L, rays, None, 8, occ) == [nd] * 2
    assert L.mcpt_trace_any_device(None, 8, None, INT_MAX, 8, None) == nd
    assert _ray_calls(L, None, None, 0, None) == [nd] * 2
    if nd == ERR_NO_DEVICE:
        assert "device" in _message(mcpt).lower()


# the parameters' refusals in the header's order: each is refused with a message of its own and wins over everything after it
ORDER = [("flags", dict(flags=1)), ("reserved", dict(reserved=1)), ("t0 and t1", dict(t0=0.5, t1=0.5))]
BAD = [dict(flags=-1), dict(flags=2 ** 20), dict(reserved=-1), dict(t0=NAN), dict(t1=NAN), dict(t1=INF), dict(t0=-INF), dict(t0=-1e-300),
       dict(t0=1.0, t1=1.0), dict(t0=0.75, t1=0.25), dict(t0=-0.5, t1=0.5)]


def test_pair_refusals_come_in_order_and_before_the_missing_device(mcpt):
    L = mcpt.lib()
    nd = _null_device_rc(mcpt)
    a, b = np.zeros((3, 3)), np.ones((65, 3))
    bits, rays, tmax = np.zeros((3, 2), dtype=np.uint64), np.zeros((3 * 65, 6)), np.zeros(1)
    ok = dict(bits=bits, rays=rays, tmax=tmax)
    assert _pair_calls(L, None, a, 3, b, 65, **ok) == [ERR_ARG] * 3 and "null pair parameters" in _message(mcpt)
    for i, (word, kw) in enumerate(ORDER):
        merged = {}
        for _, later in reversed(ORDER[i:]):
            merged.update(later)
        merged.update(kw)
        # ... and over the counts and the arrays
        assert _pair_calls(L, _pp(mcpt, **merged), None, -1, None, -1, None) == [ERR_ARG] * 3 and word in _message(mcpt), (word, _message(mcpt))
    for kw in BAD:
        assert _pair_calls(L, _pp(mcpt, **kw), a, 3, b, 65, **ok) == [ERR_ARG] * 3, kw
    # then the counts, the first list's before the second's, over the arrays
    for n in (-1, 2 ** 31, 2 ** 40):
        assert _pair_calls(L, _pp(mcpt), None, n, None, -1, None) == [ERR_ARG] * 3 and "first points" in _message(mcpt)
        assert _pair_calls(L, _pp(mcpt), None, 3, None, n, None) == [ERR_ARG] * 3 and "second points" in _message(mcpt)
    # then the matrix's words: (2^31 - 1) rows of one word pass, of two words do not; 63 rows of the longest row pass, 64 do not
    for na, nb, fits in ((INT_MAX, 64, True), (INT_MAX, 65, False), (63, INT_MAX, True), (64, INT_MAX, False), (INT_MAX, INT_MAX, False)):
        got = _pair_calls(L, _pp(mcpt), None, na, None, nb, None)
        if fits:
            assert got == [ERR_ARG] * 3 and "null point list" in _message(mcpt), (na, nb)
        else:
            assert got == [ERR_ARG] * 3 and "words" in _message(mcpt), (na, nb)
    # then the arrays: a list with a non-zero count, the outputs when there is a pair at all
    assert _pair_calls(L, _pp(mcpt), None, 3, b, 65, **ok) == [ERR_ARG] * 3 and "null point list" in _message(mcpt)
    assert _pair_calls(L, _pp(mcpt), a, 3, None, 65, **ok) == [ERR_ARG] * 3 and "null point list" in _message(mcpt)
    assert _pair_calls(L, _pp(mcpt), None, 3, None, 0, None) == [ERR_ARG] * 3 and "null point list" in _message(mcpt)
    assert _pair_calls(L, _pp(mcpt), a, 3, b, 65, None, rays=None, tmax=tmax) == [ERR_ARG] * 3 and "null output" in _message(mcpt)
    assert L.mcpt_pair_rays(_ptr(a), 3, _ptr(b), 65, C.byref(_pp(mcpt)), _ptr(rays), None) == ERR_ARG and "null output" in _message(mcpt)
    # valid arguments: the host function answers, the matrix forms miss the device; the limits of the interval pass
    assert _pair_calls(L, _pp(mcpt), a, 3, b, 65, **ok) == [0, nd, nd]
    assert _pair_calls(L, _pp(mcpt, t0=0.0, t1=5e-324), a, 3, b, 65, **ok) == [0, nd, nd]
    assert _pair_calls(L, _pp(mcpt, t0=1e300, t1=1.7e308), a, 3, b, 65, **ok) == [0, nd, nd]
    if nd == ERR_NO_DEVICE:
        assert L.mcpt_trace_any_pairs(None, _ptr(a), 3, _ptr(b), 65, C.byref(_pp(mcpt)), _ptr(bits, PU64), None) == nd and "device" in _message(mcpt).lower()
    # an empty list needs no outputs (and not the other list's array when that is empty too)
    assert _pair_calls(L, _pp(mcpt), None, 0, b, 65, None) == [0, nd, nd]
    assert _pair_calls(L, _pp(mcpt), a, 3, None, 0, None) == [0, nd, nd]
    assert _pair_calls(L, _pp(mcpt), None, 0, None, 0, None) == [0, nd, nd]


def test_empty_lists_leave_the_callers_arrays_untouched(mcpt):
    L = mcpt.lib()
    a, b = np.ones((3, 3)), np.ones((4, 3))
    for na, nb in ((0, 4), (3, 0), (0, 0)):
        rays, tmax = np.full((12, 6), 7.5), np.full(1, -2.5)
        assert L.mcpt_pair_rays(_ptr(a), na, _ptr(b), nb, C.byref(_pp(mcpt, 0.25, 0.5)), _ptr(rays), _ptr(tmax)) == 0
        assert np.all(rays == 7.5) and tmax[0] == -2.5
    rays, tmax = mcpt.pair_rays(np.zeros((0, 3)), b)
    assert rays.shape == (0, 6) and tmax == 1.0
    rays, tmax = mcpt.pair_rays(a, np.zeros((0, 3)), 0.25, 0.5)
    assert rays.shape == (0, 6) and tmax == 0.25


def test_api_validates_its_arguments(mcpt):
    a, b = np.zeros((2, 3)), np.zeros((3, 3))
    with pytest.raises(ValueError):
        mcpt.pair_rays(np.zeros((2, 2)), b)
    with pytest.raises(ValueError):
        mcpt.pair_rays(a, np.zeros(3))
    with pytest.raises(mcpt.McptError):
        mcpt.pair_rays(a, b, 0.5, 0.5)
    with pytest.raises(mcpt.McptError):
        mcpt.pair_rays(a, b, 0.0, INF)
    assert mcpt.pair_rays(a, b)[0].shape == (6, 6)


# ---- any_hit.hpp under the sanitizers

def test_pair_arithmetic_and_indexing_under_address_and_undefined_sanitizers(tmp_path):
    """A stand-alone program, not the library: nothing loaded into this process is instrumented."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "any_hit_sanitize")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "any_hit_sanitize_main.cpp")])
    vecs = [[0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [NAN, 0.0, 1.0], [INF, -INF, 1.0], [1e300, -1e300, 1e300], [1e-300, 5e-324, -5e-324],
            [0.25, -0.6, 0.8], [1.7e308, -1.7e308, 1.0]]
    cases = [(t0, t1, a, b) for (t0, t1) in INTERVALS + [(0.0, 5e-324), (1e300, 1.7e308), (NAN, INF)] for a in vecs for b in vecs]
    text = "".join("%r %r %r %r %r %r %r %r\n" % (c[0], c[1], *c[2], *c[3]) for c in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases) + 1
    bad = 0
    for c, line in zip(cases, lines):
        got = np.array([float.fromhex(x) for x in line.split()])
        rays, tmax = AR.pair_rays(np.array([c[2]]), np.array([c[3]]), c[0], c[1])
        with np.errstate(invalid="ignore"):
            want = np.concatenate([rays[0], [np.float64(c[1]) - np.float64(c[0])]])
        same = np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(_bits(got)[~np.isnan(got)], _bits(want)[~np.isnan(want)])
        bad += not same
    assert bad == 0
    # the matrix the program packed through the header's helpers is the restatement's
    i, j = np.arange(5)[:, None], np.arange(65)[None, :]
    words = [int(w, 16) for w in lines[-1].split()[1:]]
    assert lines[-1].startswith("matrix") and words == AR.pack((i + j) % 3 == 0).reshape(-1).tolist()
