"""A caller's device array as an engine's sub-allocator would hand it out: somewhere inside a larger allocation, between neighbours, only
naturally aligned, holding whatever was there before.  tests/hip_rt.py's DeviceBuffer is an allocation of exactly the payload's size,
zeroed, at hipMalloc's alignment and read back over the payload alone, so a store one entry past the end, an output that adds into what
it finds, or a 16-byte access through an 8-byte-aligned pointer all pass under it.

Guarded(array_or_nbytes, dtype, fill, skew) is ONE allocation of G + skew + nbytes + G bytes, every byte of it `fill`, with the payload at
offset G + skew.  G = 65536 is more than a 256-thread block overrunning the widest record of include/mcpt.h does (27 doubles: 256 * 216 =
55 296 bytes), so an overrun lands in a band, where check() finds it, and does not fault.  skew is 0 or the element size: natural alignment
is never broken.  Given an array the buffer is an INPUT (the array is uploaded and check() also holds the payload to it); given a byte
count it is an OUTPUT.  The two fills in use: 0xFF (every float64 a NaN, every int32 -1) and 0xA5 (a tiny negative finite double, a large
negative int32).  Reads are synchronous copies: synchronise the call's stream first.

The device sits behind _alloc and _copy alone, which tests/test_guarded_cpu.py replaces by host memory to test the arithmetic here."""
import ctypes as C

import numpy as np

G = 65536
FILLS = (0xFF, 0xA5)
H2D, D2H = 1, 2


def _alloc(nbytes, fill):
    """nbytes of device memory, every byte `fill` -> (address, a function that frees it)"""
    from hip_rt import check, hip
    p = C.c_void_p()
    check(hip().hipMalloc(C.byref(p), nbytes))
    check(hip().hipMemset(p, fill, nbytes))
    return p.value, lambda: hip().hipFree(p)


def _copy(dst, src, nbytes, kind):
    """a synchronous copy between two addresses (kind: H2D or D2H)"""
    from hip_rt import check, hip
    if nbytes:
        check(hip().hipMemcpy(C.c_void_p(dst), C.c_void_p(src), nbytes, kind))


def fill_value(dtype, fill):
    """the element of `dtype` whose every byte is `fill`"""
    return np.full(np.dtype(dtype).itemsize, fill, np.uint8).view(dtype)[0]


def payload_range(nbytes, skew):
    """[lo, hi) of the payload inside the allocation, and the allocation's size"""
    lo = G + skew
    return lo, lo + nbytes, lo + nbytes + G


def damage(whole, nbytes, skew, fill):
    """the first byte of an allocation's bands that is not `fill`: None, or (side, offset relative to the payload's first byte, value);
    the front band is [-(G + skew), 0), the back band [nbytes, nbytes + G)"""
    lo, hi, total = payload_range(nbytes, skew)
    assert whole.dtype == np.uint8 and whole.shape == (total,)
    for side, a, b in (("front", 0, lo), ("back", hi, total)):
        bad = np.flatnonzero(whole[a:b] != fill)
        if bad.size:
            at = a + int(bad[0])
            return side, at - lo, int(whole[at])
    return None


def altered(got, sent):
    """the first byte in which an input's payload differs from what was uploaded: None, or (offset, value, what was sent)"""
    bad = np.flatnonzero(got != sent)
    return (int(bad[0]), int(got[bad[0]]), int(sent[bad[0]])) if bad.size else None


class Guarded:
    def __init__(self, array_or_nbytes, dtype, fill, skew=0):
        self.dtype = np.dtype(dtype)
        assert skew in (0, self.dtype.itemsize) and 0 <= fill <= 255
        self.fill, self.skew = fill, skew
        self.sent = None
        if isinstance(array_or_nbytes, np.ndarray):
            a = np.ascontiguousarray(array_or_nbytes)
            assert a.dtype == self.dtype, (a.dtype, self.dtype)
            self.nbytes = a.nbytes
        else:
            a = None
            self.nbytes = int(array_or_nbytes)
            assert self.nbytes % self.dtype.itemsize == 0
        self.lo, self.hi, self.total = payload_range(self.nbytes, skew)
        self.base, self._free = _alloc(self.total, fill)
        if a is not None:
            self.upload(a)

    @property
    def ptr(self):
        """the payload's device address"""
        return self.base + self.lo

    def upload(self, a):
        a = np.ascontiguousarray(a)
        assert a.dtype == self.dtype and a.nbytes == self.nbytes, (a.dtype, a.nbytes, self.nbytes)
        self.sent = a.reshape(-1).view(np.uint8).copy()
        _copy(self.ptr, self.sent.ctypes.data, self.nbytes, H2D)

    def payload(self):
        out = np.empty(self.nbytes // self.dtype.itemsize, self.dtype)
        _copy(out.ctypes.data, self.ptr, self.nbytes, D2H)
        return out

    def whole(self):
        out = np.empty(self.total, np.uint8)
        _copy(out.ctypes.data, self.base, self.total, D2H)
        return out

    def check(self, what):
        """every byte outside the payload is still the fill; an input's payload is still what was uploaded"""
        whole = self.whole()
        d = damage(whole, self.nbytes, self.skew, self.fill)
        assert d is None, "%s: %s band damaged at byte %+d of the payload (%d bytes, fill 0x%02X, skew %d): holds 0x%02X" % (
            what, d[0], d[1], self.nbytes, self.fill, self.skew, d[2])
        if self.sent is not None:
            d = altered(whole[self.lo:self.hi], self.sent)
            assert d is None, "%s: input payload modified at byte %+d of %d (fill 0x%02X, skew %d): holds 0x%02X, 0x%02X was uploaded" % (
                what, d[0], self.nbytes, self.fill, self.skew, d[1], d[2])

    def free(self):
        if self._free is not None:
            self._free()
            self._free = None
