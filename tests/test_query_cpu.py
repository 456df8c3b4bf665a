"""Not gpu: the C-ABI surface of radiance queries (mcpt_query_radiance, mcpt_query_radiance_device, mcpt_query_rays) -- symbols, the
mcpt_query_params layout against the C compiler, every refusal with a null device through the C ABI and through api.py, and the
orthonormal frame of the numpy restatement (tests/query_ref.py)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import query_ref
from conftest import ROOT

ERR_ARG, ERR_NO_DEVICE = -3, -4
NAMES = ["mcpt_query_radiance", "mcpt_query_radiance_device", "mcpt_query_rays"]
PD, P32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
INT_MAX = 2 ** 31 - 1


def _null_device_rc(mcpt):
    """what a null handle with valid arguments gives: no device at all, or a refused handle"""
    return ERR_NO_DEVICE if mcpt.device_count() <= 0 else ERR_ARG


def test_query_symbols_are_declared_and_exported(mcpt):
    from montecarlopathtracing_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for sym in NAMES:
        assert (sym + "(") in hdr and sym in _lib.EXPORTS and hasattr(L, sym), sym
    assert "#define MCPT_QUERY_RAY        0" in hdr and "#define MCPT_QUERY_HEMISPHERE 1" in hdr
    assert (mcpt.QUERY_RAY, mcpt.QUERY_HEMISPHERE) == (0, 1)
    assert "} mcpt_query_params;" in hdr and "THE IRRADIANCE IS" in hdr
    assert "#define MCPT_VERSION 105" in hdr and mcpt.lib().mcpt_version() == 105
    for f in ("radiance", "irradiance", "query_rays"):
        assert callable(getattr(mcpt.Device, f))


def test_query_params_layout_matches_the_header(mcpt, tmp_path):
    from montecarlopathtracing_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [n for n, _ in _lib.QueryParams._fields_]
    assert fields == ["spp", "sample_base", "seed", "kind", "flags", "reserved"]
    src = tmp_path / "layout_query.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"mcpt.h\"\nint main(void) {\n  printf(\"%zu\\n\", sizeof(mcpt_query_params));\n"
                   + "".join("  printf(\"%%zu\\n\", offsetof(mcpt_query_params, %s));\n" % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout_query"
    subprocess.check_call([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert out[0] == C.sizeof(_lib.QueryParams) == 32
    for i, f in enumerate(fields):
        assert out[1 + i] == getattr(_lib.QueryParams, f).offset, f


def _params(mcpt, spp=4, sample_base=0, seed=1, kind=0, flags=0, reserved=(0, 0)):
    return mcpt.QueryParams(spp, sample_base, seed, kind, flags, (C.c_int32 * 2)(*reserved))


RAYS = np.array([[0.0, 0.0, 0.0, 1.0, 0.0, 0.0], [1.0, 2.0, 3.0, 0.0, 0.6, 0.8], [0.5, 0.5, 0.5, 0.0, 0.0, -1.0]])
POINTS = np.array([[0.0, 0.0, 0.0, 0.0, 2.5, 0.0], [1.0, 2.0, 3.0, 1e-3, -1e-3, 1e-3], [0.5, 0.5, 0.5, 3.0, 4.0, 12.0]])

# (what, keyword overrides of the parameters) -- refused whatever the list holds
BAD_PARAMS = [("spp 0", dict(spp=0)), ("spp negative", dict(spp=-3)), ("sample_base negative", dict(sample_base=-1)),
              ("sample_base + spp past 2^31 - 1", dict(spp=2, sample_base=INT_MAX - 1)), ("sample_base + spp past 2^31 - 1", dict(spp=INT_MAX, sample_base=1)),
              ("unknown kind", dict(kind=2)), ("unknown kind", dict(kind=-1)), ("unknown flag", dict(flags=1)), ("unknown flag", dict(flags=4)),
              ("unknown flag", dict(flags=8)), ("unknown flag", dict(flags=2 | 4)), ("reserved", dict(reserved=(1, 0))), ("reserved", dict(reserved=(0, -1)))]


def _bad_lists():
    """(what, kind, q6, ids): lists the host-pointer forms refuse"""
    out = []
    for c in range(6):
        for v in (float("nan"), float("inf"), float("-inf")):
            for kind, base in ((0, RAYS), (1, POINTS)):
                q = base.copy()
                q[1, c] = v
                out.append(("component %d = %r" % (c, v), kind, q, None))
    q = RAYS.copy(); q[2, 3:] = [0.0, 0.0, -(1.0 + 1e-8)]
    out.append(("direction too long", 0, q, None))
    q = RAYS.copy(); q[0, 3:] = [1.0 - 1e-8, 0.0, 0.0]
    out.append(("direction too short", 0, q, None))
    q = RAYS.copy(); q[0, 3:] = 0.0
    out.append(("zero direction", 0, q, None))
    q = POINTS.copy(); q[2, 3:] = 0.0
    out.append(("zero normal", 1, q, None))
    q = POINTS.copy(); q[2, 3:] = [1e-200, 0.0, 0.0]
    out.append(("normal whose length underflows to zero", 1, q, None))
    q = POINTS.copy(); q[2, 3:] = [1e200, 1e200, 0.0]
    out.append(("normal whose length overflows", 1, q, None))
    out.append(("negative id", 0, RAYS.copy(), np.array([0, -1, 2], dtype=np.int32)))
    out.append(("negative id", 1, POINTS.copy(), np.array([-2 ** 31, 1, 2], dtype=np.int32)))
    return out


def _call(L, q, ids, n, qp, mean, err=None, hits=None):
    return L.mcpt_query_radiance(None, q.ctypes.data_as(PD) if q is not None else None, ids.ctypes.data_as(P32) if ids is not None else None, n,
                                 C.byref(qp) if qp is not None else None, mean.ctypes.data_as(PD) if mean is not None else None,
                                 err.ctypes.data_as(PD) if err is not None else None, hits.ctypes.data_as(P32) if hits is not None else None, None)


def _message(mcpt):
    return mcpt.lib().mcpt_last_error().decode()


def test_refusals_come_before_the_missing_device(mcpt):
    L = mcpt.lib()
    nd = _null_device_rc(mcpt)
    mean, err, hits = np.zeros((3, 3)), np.zeros((3, 3)), np.zeros(3, dtype=np.int32)
    for what, kw in BAD_PARAMS:
        for kind, q in ((0, RAYS), (1, POINTS)):
            kw2 = dict(kind=kind)
            kw2.update(kw)
            qp = _params(mcpt, **kw2)
            assert _call(L, q, None, 3, qp, mean, err, hits) == ERR_ARG, what
            assert _message(mcpt), what
            # the device form refuses the same parameters (its pointers are not looked at)
            assert L.mcpt_query_radiance_device(None, q.ctypes.data, None, 3, C.byref(qp), mean.ctypes.data, None, None, None, None) == ERR_ARG, what
            assert _message(mcpt), what
    for n in (-1, 2 ** 31, 2 ** 40):
        assert _call(L, RAYS, None, n, _params(mcpt), mean) == ERR_ARG and _message(mcpt)
        assert L.mcpt_query_radiance_device(None, RAYS.ctypes.data, None, n, C.byref(_params(mcpt)), mean.ctypes.data, None, None, None, None) == ERR_ARG
    assert _call(L, None, None, 3, _params(mcpt), mean) == ERR_ARG and _message(mcpt)
    assert _call(L, RAYS, None, 3, _params(mcpt), None) == ERR_ARG and _message(mcpt)
    assert _call(L, RAYS, None, 3, None, mean) == ERR_ARG and _message(mcpt)
    assert L.mcpt_query_radiance_device(None, None, None, 3, C.byref(_params(mcpt)), mean.ctypes.data, None, None, None, None) == ERR_ARG
    assert L.mcpt_query_radiance_device(None, RAYS.ctypes.data, None, 3, C.byref(_params(mcpt)), None, None, None, None, None) == ERR_ARG
    for what, kind, q, ids in _bad_lists():
        assert _call(L, q, ids, 3, _params(mcpt, kind=kind), mean, err, hits) == ERR_ARG, what
        assert "query" in _message(mcpt), what
    # valid arguments: the missing device (or the refused null handle) is what is left to report
    ids = np.array([7, 0, INT_MAX], dtype=np.int32)
    for kind, q in ((0, RAYS), (1, POINTS)):
        for kw in (dict(), dict(flags=2), dict(spp=1, sample_base=INT_MAX - 1), dict(spp=INT_MAX), dict(seed=2 ** 64 - 1)):
            qp = _params(mcpt, kind=kind, **kw)
            assert _call(L, q, ids, 3, qp, mean, err, hits) == nd, kw
            assert _call(L, q, None, 3, qp, mean) == nd, kw
            assert L.mcpt_query_radiance_device(None, q.ctypes.data, None, 3, C.byref(qp), mean.ctypes.data, None, None, None, None) == nd
    # a direction within 1e-9 of unit length is taken
    q = RAYS.copy(); q[0, 3:] = [1.0 + 4e-10, 0.0, 0.0]
    assert _call(L, q, None, 3, _params(mcpt), mean) == nd
    assert _call(L, None, None, 0, _params(mcpt), None) == nd         # n == 0 needs no arrays


def test_query_rays_refusals(mcpt):
    L = mcpt.lib()
    nd = _null_device_rc(mcpt)
    k = np.array([0, 5, INT_MAX], dtype=np.int32)
    out = np.zeros((3, 6))

    def call(q, ids, n, kind, ks, rays):
        return L.mcpt_query_rays(None, q.ctypes.data_as(PD) if q is not None else None, ids.ctypes.data_as(P32) if ids is not None else None, n, 9,
                                 kind, ks.ctypes.data_as(P32) if ks is not None else None, rays.ctypes.data_as(PD) if rays is not None else None)
    assert call(RAYS, None, 3, 0, k, out) == nd and call(POINTS, None, 3, 1, k, out) == nd
    for args in ((None, None, 3, 0, k, out), (RAYS, None, 3, 0, None, out), (RAYS, None, 3, 0, k, None), (RAYS, None, -1, 0, k, out),
                 (RAYS, None, 2 ** 31, 0, k, out), (RAYS, None, 3, 2, k, out), (RAYS, None, 3, -1, k, out),
                 (RAYS, None, 3, 0, np.array([0, -1, 0], dtype=np.int32), out)):
        assert call(*args) == ERR_ARG and _message(mcpt)
    for what, kind, q, ids in _bad_lists():
        assert call(q, ids, 3, kind, k, out) == ERR_ARG, what


def _null_dev(mcpt):
    dev = mcpt.Device.__new__(mcpt.Device)
    dev._h = None
    return dev


def test_api_refusals(mcpt):
    """api.py: shapes and dtypes are ValueErrors; what the library refuses arrives as McptError with its code and message"""
    dev = _null_dev(mcpt)
    nd = _null_device_rc(mcpt)
    for bad in (np.zeros((3, 5)), np.zeros(6), np.zeros((2, 3, 6))):
        with pytest.raises(ValueError):
            dev.radiance(bad, 4)
        with pytest.raises(ValueError):
            dev.query_rays(bad, 0, np.zeros(3, dtype=np.int32))
    with pytest.raises(ValueError):
        dev.irradiance(np.zeros((3, 3)), np.zeros((2, 3)), 4)
    with pytest.raises(ValueError):
        dev.irradiance(np.zeros((3, 2)), np.zeros((3, 2)), 4)
    for ids in (np.zeros(2, dtype=np.int32), np.zeros(3), np.array([0, 1, 2 ** 31])):
        with pytest.raises(ValueError):
            dev.radiance(RAYS, 4, ids=ids)
    for kw in (dict(spp=2.5), dict(spp=2 ** 31), dict(spp=4, sample_base=1.0), dict(spp=4, flags="2")):
        with pytest.raises(ValueError):
            dev.radiance(RAYS, **kw)
    with pytest.raises(ValueError):
        dev.query_rays(RAYS, 0, np.zeros(3, dtype=np.int32), kind="sphere")
    with pytest.raises(ValueError):
        dev.query_rays(RAYS, 0, np.zeros(2, dtype=np.int32))
    with pytest.raises(ValueError):
        dev.query_rays(RAYS, 0, np.zeros(3))
    for what, kw in BAD_PARAMS:
        if "kind" in kw or "reserved" in kw:
            continue
        args = dict(spp=4)
        args.update(kw)
        for f in (lambda: dev.radiance(RAYS, **args), lambda: dev.irradiance(POINTS[:, :3], POINTS[:, 3:], **args)):
            with pytest.raises(mcpt.McptError) as e:
                f()
            assert e.value.code == ERR_ARG and str(e.value), what
    for what, kind, q, ids in _bad_lists():
        with pytest.raises(mcpt.McptError) as e:
            if kind == 0:
                dev.radiance(q, 4, ids=ids)
            else:
                dev.irradiance(q[:, :3], q[:, 3:], 4, ids=ids)
        assert e.value.code == ERR_ARG and "query" in str(e.value), what
        with pytest.raises(mcpt.McptError) as e:
            dev.query_rays(q, 0, np.zeros(3, dtype=np.int32), kind="ray" if kind == 0 else "hemisphere", ids=ids)
        assert e.value.code == ERR_ARG, what
    for f in (lambda: dev.radiance(RAYS, 4, seed=3, ids=[5, 6, 7], sample_base=2, flags=mcpt.RENDER_MEGAKERNEL, stats=mcpt.Stats()),
              lambda: dev.irradiance(POINTS[:, :3], POINTS[:, 3:], 4), lambda: dev.query_rays(POINTS, 1, [0, 1, 2], kind="hemisphere")):
        with pytest.raises(mcpt.McptError) as e:
            f()
        assert e.value.code == nd


def test_the_restatements_frame_is_orthonormal():
    rng = np.random.default_rng(11)
    n = rng.normal(size=(10000, 3)) * 10.0 ** rng.uniform(-3, 3, size=(10000, 1))
    special = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.0, -2.0, 0.0], [1.0, 1.0, 5.0], [3.0, -1.0, 1.0], [1.0, 1.0, 1.0],
                        [-1.0, 1.0, -1.0], [0.0, 0.0, -1e-3]])
    n = np.concatenate([n, special])
    t, s, nh = query_ref.basis(n)
    for a in (t, s, nh):
        assert np.abs((a * a).sum(axis=1) - 1.0).max() <= 1e-15
    for a, b in ((t, s), (t, nh), (s, nh)):
        assert np.abs((a * b).sum(axis=1)).max() <= 1e-15
    # right-handed, n^ along the normal, and the axis rule: the lowest of equal smallest components
    assert np.abs(np.cross(t, s) - nh).max() <= 1e-15
    assert np.all((nh * n).sum(axis=1) > 0)
    t3, _, _ = query_ref.basis(special)
    assert np.array_equal(t3[0], [0.0, 0.0, -1.0])      # n = +X: e = Y (the lowest of y, z), t = cross(Y, X) = -Z
    assert np.array_equal(t3[1], [0.0, 0.0, 1.0])       # n = +Y: e = X, t = cross(X, Y) = +Z
    assert np.array_equal(t3[2], [0.0, -1.0, 0.0])      # n = +Z: e = X, t = cross(X, Z) = -Y
    assert t3[4][0] == 0.0 and t3[6][0] == 0.0           # x == y smallest, all equal: e = X, so t has no x
    assert t3[5][1] == 0.0                              # |y| == |z| smallest: e = Y
