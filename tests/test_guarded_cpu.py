"""tests/guarded.py without a GPU: the offset arithmetic of Guarded (where the payload sits, which bytes are the bands, what the message of a
damaged band or a modified input says) against host memory standing in for the allocation -- the device sits behind guarded._alloc and
guarded._copy, which are replaced here.  And the coverage table of tests/test_gpu_extents.py against include/mcpt.h: every entry point
that takes a d_* argument has a row, none of them NOT COVERED, so a new device form cannot arrive untested."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import guarded
from guarded import G, Guarded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def host(monkeypatch):
    """host arrays in place of device allocations: {address: array}"""
    live = {}

    def alloc(nbytes, fill):
        a = np.full(nbytes, fill, np.uint8)
        live[a.ctypes.data] = a
        return a.ctypes.data, lambda: live.pop(a.ctypes.data)

    def copy(dst, src, nbytes, kind):
        assert kind in (guarded.H2D, guarded.D2H)
        C.memmove(dst, src, nbytes)
    monkeypatch.setattr(guarded, "_alloc", alloc)
    monkeypatch.setattr(guarded, "_copy", copy)
    return live


def test_fill_values():
    assert np.isnan(guarded.fill_value(np.float64, 0xFF)) and guarded.fill_value(np.int32, 0xFF) == -1
    a5 = guarded.fill_value(np.float64, 0xA5)
    assert np.isfinite(a5) and -1e-100 < a5 < 0 and guarded.fill_value(np.int32, 0xA5) == -1515870811
    assert guarded.fill_value(np.uint8, 0xA5) == 0xA5
    assert G > 256 * 27 * 8                                 # a 256-thread block overrunning the widest record stays inside a band


@pytest.mark.parametrize("dtype, skew", [(np.float64, 0), (np.float64, 8), (np.int32, 4), (np.uint8, 1), (np.uint8, 0)])
@pytest.mark.parametrize("fill", guarded.FILLS)
def test_layout(host, dtype, skew, fill):
    n = 7
    g = Guarded(n * np.dtype(dtype).itemsize, dtype, fill, skew)
    (base, whole), = host.items()
    assert g.base == base and whole.size == G + skew + g.nbytes + G and (whole == fill).all()
    assert g.ptr == base + G + skew and g.ptr % np.dtype(dtype).itemsize == 0
    assert (g.lo, g.hi, g.total) == guarded.payload_range(g.nbytes, skew) == (G + skew, G + skew + g.nbytes, whole.size)
    assert (g.payload().view(np.uint8) == fill).all() and g.payload().dtype == dtype and g.payload().size == n
    g.check("out")                                          # an output's payload may hold anything
    whole[g.lo:g.hi] = 3
    g.check("out")
    assert (g.payload().view(np.uint8) == 3).all()
    g.free()
    assert not host
    g.free()                                                # (twice is harmless)


def test_an_input_is_uploaded_to_the_payload_and_held_to_it(host):
    a = np.arange(5, dtype=np.int32) * 1000 + 1
    g = Guarded(a, np.int32, 0xA5, skew=4)
    (whole,) = host.values()
    assert np.array_equal(whole[g.lo:g.hi].view(np.int32), a) and np.array_equal(g.payload(), a)
    assert (whole[:g.lo] == 0xA5).all() and (whole[g.hi:] == 0xA5).all()
    g.check("ids")
    whole[g.lo + 9] ^= 0x10
    with pytest.raises(AssertionError, match=r"ids: input payload modified at byte \+9 of 20 .*holds 0x%02X, 0x%02X was uploaded" % (
            a.view(np.uint8)[9] ^ 0x10, a.view(np.uint8)[9])):
        g.check("ids")
    a[0] = 7                                                # (the caller's array may change afterwards: the upload is what counts)
    whole[g.lo + 9] ^= 0x10
    g.check("ids")


@pytest.mark.parametrize("skew", [0, 8])
def test_the_damaged_offset_is_relative_to_the_payload(host, skew):
    g = Guarded(24, np.float64, 0xFF, skew)
    (whole,) = host.values()
    for at, side, rel in ((g.lo - 1, "front", -1), (0, "front", -(G + skew)), (g.hi, "back", 24), (g.total - 1, "back", 24 + G - 1)):
        whole[at] = 0x00
        assert guarded.damage(whole, 24, skew, 0xFF) == (side, rel, 0)
        with pytest.raises(AssertionError, match=r"mean3: %s band damaged at byte %s of the payload \(24 bytes, fill 0xFF, skew %d\): holds 0x00"
                           % (side, re.escape("%+d" % rel), skew)):
            g.check("mean3")
        whole[at] = 0xFF
        g.check("mean3")
    whole[g.lo - 8:g.lo] = 1                                # (the first damaged byte is the one reported, the front band before the back)
    whole[g.hi + 5] = 1
    assert guarded.damage(whole, 24, skew, 0xFF) == ("front", -8, 1)
    whole[g.lo - 8:g.lo] = 0xFF
    assert guarded.damage(whole, 24, skew, 0xFF) == ("back", 29, 1)


def test_an_empty_payload(host):
    g = Guarded(0, np.float64, 0xFF)
    assert g.payload().size == 0 and g.total == 2 * G
    g.check("empty")
    next(iter(host.values()))[G] = 0
    with pytest.raises(AssertionError, match=r"back band damaged at byte \+0"):
        g.check("empty")


# ---- the coverage table

def device_pointer_symbols():
    """every function of include/mcpt.h one of whose parameters is named d_*"""
    text = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = []
    for m in re.finditer(r"\b(mcpt_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        if re.search(r"\bd_[A-Za-z]\w*", m.group(2)):
            out.append(m.group(1))
    return out


def table_rows():
    src = open(os.path.join(ROOT, "tests", "test_gpu_extents.py")).read()
    doc = src.split('"""')[1]
    return {m.group(1): m.group(2) for m in re.finditer(r"^\s*(mcpt_\w+)\s*\|(.*)$", doc, flags=re.M)}


def test_every_device_pointer_entry_point_has_a_row_in_the_extents_table():
    symbols = device_pointer_symbols()
    assert len(symbols) == len(set(symbols)) >= 34 and "mcpt_trace_closest_device" in symbols and "mcpt_sh_basis" not in symbols
    rows = table_rows()
    missing = [s for s in symbols if s not in rows]
    assert not missing, "include/mcpt.h declares device-pointer entry points tests/test_gpu_extents.py does not list: %s" % missing
    stale = [s for s in rows if s not in symbols]
    assert not stale, "tests/test_gpu_extents.py lists symbols include/mcpt.h does not declare with a d_* argument: %s" % stale
    src = open(os.path.join(ROOT, "tests", "test_gpu_extents.py")).read()
    for s, row in rows.items():
        cols = [c.strip() for c in row.split("|")]
        assert len(cols) == 3 and all(cols), (s, row)       # the case, its sizes, the block constant
        elsewhere = re.match(r"(test_gpu_\w+\.py)::(test_\w+)$", cols[0])
        if elsewhere:                                       # a row that names a test of another file: the call is looked for there
            other = open(os.path.join(ROOT, "tests", elsewhere.group(1))).read()
            assert "def %s(" % elsewhere.group(2) in other and "lib.%s(" % s in other, "%s: no call in %s" % (s, elsewhere.group(1))
            assert "pytestmark = pytest.mark.gpu" in other and "Guarded(" in other
        if not cols[0].startswith("NOT COVERED"):
            assert src.count(s) >= 2, "%s has a row but no call in the file" % s
    assert not [s for s, row in rows.items() if "NOT COVERED" in row]
