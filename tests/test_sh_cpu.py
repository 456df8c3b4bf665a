"""Not gpu: the C-ABI surface of light probes (mcpt_query_sh, mcpt_query_sh_device, mcpt_query_sh_rays, mcpt_sh_basis, mcpt_sh_radiance,
mcpt_sh_irradiance) -- symbols, the mcpt_sh_params layout against the C compiler, every refusal with a null device through the C ABI and
through api.py, the host helpers against the numpy restatement (tests/sh_ref.py) bit for bit, and what the restatement itself has to be:
an orthonormal basis, the cosine lobe's factors, a uniform draw."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import sh_ref
from conftest import ROOT

ERR_ARG, ERR_NO_DEVICE = -3, -4
NAMES = ["mcpt_query_sh", "mcpt_query_sh_device", "mcpt_query_sh_rays", "mcpt_sh_basis", "mcpt_sh_radiance", "mcpt_sh_irradiance"]
PD, P32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
INT_MAX = 2 ** 31 - 1
AXES = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])


def _null_device_rc(mcpt):
    """what a null handle with valid arguments gives: no device at all, or a refused handle"""
    return ERR_NO_DEVICE if mcpt.device_count() <= 0 else ERR_ARG


def _message(mcpt):
    return mcpt.lib().mcpt_last_error().decode()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_sh_symbols_are_declared_and_exported(mcpt):
    from montecarlopathtracing_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for sym in NAMES:
        assert (sym + "(") in hdr and sym in _lib.EXPORTS and hasattr(L, sym), sym
    assert "} mcpt_sh_params;" in hdr and "A PROBE IS MEANT TO SIT IN FREE SPACE" in hdr
    # the feature is detected by symbol: the version and the query kinds stay
    assert "#define MCPT_VERSION 105" in hdr and mcpt.lib().mcpt_version() == 105
    from montecarlopathtracing_amd import api
    assert sorted(api._QUERY_KINDS) == ["hemisphere", "ray"]
    for f in ("sh_probes", "sh_probe_rays"):
        assert callable(getattr(mcpt.Device, f))
    for f in ("sh_basis", "sh_radiance", "sh_irradiance"):
        assert callable(getattr(mcpt, f))
    # the basis constants as the header writes them
    for c in ("0.28209479177387814", "0.4886025119029199", "1.0925484305920792", "0.31539156525252005", "0.5462742152960396",
              "12.566370614359172", "3.141592653589793", "2.0943951023931953", "0.7853981633974483"):
        assert c in hdr, c


def test_sh_params_layout_matches_the_header(mcpt, tmp_path):
    from montecarlopathtracing_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    if cc is None:
        pytest.skip("no C compiler")
    fields = [n for n, _ in _lib.ShParams._fields_]
    assert fields == ["spp", "sample_base", "seed", "flags", "reserved"]
    src = tmp_path / "layout_sh.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"mcpt.h\"\nint main(void) {\n  printf(\"%zu\\n\", sizeof(mcpt_sh_params));\n"
                   + "".join("  printf(\"%%zu\\n\", offsetof(mcpt_sh_params, %s));\n" % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout_sh"
    subprocess.check_call([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert out[0] == C.sizeof(_lib.ShParams) == 32
    for i, f in enumerate(fields):
        assert out[1 + i] == getattr(_lib.ShParams, f).offset, f


def _params(mcpt, spp=4, sample_base=0, seed=1, flags=0, reserved=(0, 0, 0)):
    return mcpt.ShParams(spp, sample_base, seed, flags, (C.c_int32 * 3)(*reserved))


POINTS = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [0.5, -0.5, 1e-3]])

# (what, keyword overrides of the parameters) -- refused whatever the list holds: mcpt_query_radiance's, less the kind
BAD_PARAMS = [("spp 0", dict(spp=0)), ("spp negative", dict(spp=-3)), ("sample_base negative", dict(sample_base=-1)),
              ("sample_base + spp past 2^31 - 1", dict(spp=2, sample_base=INT_MAX - 1)), ("sample_base + spp past 2^31 - 1", dict(spp=INT_MAX, sample_base=1)),
              ("unknown flag", dict(flags=1)), ("unknown flag", dict(flags=4)), ("unknown flag", dict(flags=8)), ("unknown flag", dict(flags=2 | 4)),
              ("reserved", dict(reserved=(1, 0, 0))), ("reserved", dict(reserved=(0, -1, 0))), ("reserved", dict(reserved=(0, 0, 7)))]


def _bad_lists():
    """(what, p3, ids): lists the host-pointer forms refuse"""
    out = []
    for c in range(3):
        for v in (float("nan"), float("inf"), float("-inf")):
            p = POINTS.copy()
            p[1, c] = v
            out.append(("component %d = %r" % (c, v), p, None))
    out.append(("negative id", POINTS.copy(), np.array([0, -1, 2], dtype=np.int32)))
    out.append(("negative id", POINTS.copy(), np.array([-2 ** 31, 1, 2], dtype=np.int32)))
    return out


def _call(L, p3, ids, n, sp, sh, err=None, hits=None):
    return L.mcpt_query_sh(None, p3.ctypes.data_as(PD) if p3 is not None else None, ids.ctypes.data_as(P32) if ids is not None else None, n,
                           C.byref(sp) if sp is not None else None, sh.ctypes.data_as(PD) if sh is not None else None,
                           err.ctypes.data_as(PD) if err is not None else None, hits.ctypes.data_as(P32) if hits is not None else None, None)


def _call_device(L, p3, n, sp, sh):
    return L.mcpt_query_sh_device(None, p3.ctypes.data if p3 is not None else None, None, n, C.byref(sp), sh.ctypes.data if sh is not None else None,
                                  None, None, None, None)


def test_refusals_come_before_the_missing_device(mcpt):
    L = mcpt.lib()
    nd = _null_device_rc(mcpt)
    sh, err, hits = np.zeros((3, 9, 3)), np.zeros((3, 9, 3)), np.zeros(3, dtype=np.int32)
    for what, kw in BAD_PARAMS:
        sp = _params(mcpt, **kw)
        assert _call(L, POINTS, None, 3, sp, sh, err, hits) == ERR_ARG, what
        assert _message(mcpt), what
        # the device form refuses the same parameters (its pointers are not looked at)
        assert _call_device(L, POINTS, 3, sp, sh) == ERR_ARG, what
        assert _message(mcpt), what
    for n in (-1, 2 ** 31, 2 ** 40):
        assert _call(L, POINTS, None, n, _params(mcpt), sh) == ERR_ARG and _message(mcpt)
        assert _call_device(L, POINTS, n, _params(mcpt), sh) == ERR_ARG
    assert _call(L, None, None, 3, _params(mcpt), sh) == ERR_ARG and _message(mcpt)
    assert _call(L, POINTS, None, 3, _params(mcpt), None) == ERR_ARG and _message(mcpt)
    assert _call(L, POINTS, None, 3, None, sh) == ERR_ARG and _message(mcpt)
    assert _call_device(L, None, 3, _params(mcpt), sh) == ERR_ARG
    assert _call_device(L, POINTS, 3, _params(mcpt), None) == ERR_ARG
    # the order is mcpt_query_radiance's: the sample range before the count before the flags before reserved before the pointers
    for kw, n, p3, word in ((dict(spp=0, flags=1), -1, None, "spp"), (dict(flags=1, reserved=(1, 0, 0)), -1, None, "number of queries"),
                            (dict(flags=1, reserved=(1, 0, 0)), 3, None, "flag"), (dict(reserved=(1, 0, 0)), 3, None, "reserved"),
                            (dict(), 3, None, "null")):
        assert _call(L, p3, None, n, _params(mcpt, **kw), sh) == ERR_ARG
        assert word in _message(mcpt), (kw, _message(mcpt))
    for what, p3, ids in _bad_lists():
        assert _call(L, p3, ids, 3, _params(mcpt), sh, err, hits) == ERR_ARG, what
        assert "probe" in _message(mcpt), what
    # valid arguments: the missing device (or the refused null handle) is what is left to report
    ids = np.array([7, 0, INT_MAX], dtype=np.int32)
    for kw in (dict(), dict(flags=2), dict(spp=1, sample_base=INT_MAX - 1), dict(spp=INT_MAX), dict(seed=2 ** 64 - 1)):
        sp = _params(mcpt, **kw)
        assert _call(L, POINTS, ids, 3, sp, sh, err, hits) == nd, kw
        assert _call(L, POINTS, None, 3, sp, sh) == nd, kw
        assert _call_device(L, POINTS, 3, sp, sh) == nd, kw
    assert _call(L, None, None, 0, _params(mcpt), None) == nd         # n == 0 needs no arrays


def test_probe_rays_refusals(mcpt):
    L = mcpt.lib()
    nd = _null_device_rc(mcpt)
    k = np.array([0, 5, INT_MAX], dtype=np.int32)
    out = np.zeros((3, 6))

    def call(p3, ids, n, ks, rays):
        return L.mcpt_query_sh_rays(None, p3.ctypes.data_as(PD) if p3 is not None else None, ids.ctypes.data_as(P32) if ids is not None else None, n, 9,
                                    ks.ctypes.data_as(P32) if ks is not None else None, rays.ctypes.data_as(PD) if rays is not None else None)
    assert call(POINTS, None, 3, k, out) == nd and call(POINTS, np.array([7, 0, INT_MAX], dtype=np.int32), 3, k, out) == nd
    for args in ((None, None, 3, k, out), (POINTS, None, 3, None, out), (POINTS, None, 3, k, None), (POINTS, None, -1, k, out),
                 (POINTS, None, 2 ** 31, k, out), (POINTS, None, 3, np.array([0, -1, 0], dtype=np.int32), out)):
        assert call(*args) == ERR_ARG and _message(mcpt)
    for what, p3, ids in _bad_lists():
        assert call(p3, ids, 3, k, out) == ERR_ARG, what


def test_host_helper_refusals(mcpt):
    L = mcpt.lib()
    d = AXES[:3].copy()
    sh = np.ones((3, 9, 3))
    y, out = np.zeros((3, 9)), np.zeros((3, 3))
    p = lambda a: a.ctypes.data_as(PD) if a is not None else None      # noqa: E731
    assert L.mcpt_sh_basis(p(d), 3, p(y)) == 0 and L.mcpt_sh_radiance(p(sh), p(d), 3, p(out)) == 0 and L.mcpt_sh_irradiance(p(sh), p(d), 3, p(out)) == 0
    assert L.mcpt_sh_basis(None, 0, None) == ERR_ARG        # a NULL pointer is refused whatever n is
    for args in ((None, 3, y), (d, 3, None), (d, -1, y)):
        assert L.mcpt_sh_basis(p(args[0]), args[1], p(args[2])) == ERR_ARG and _message(mcpt)
    for f in (L.mcpt_sh_radiance, L.mcpt_sh_irradiance):
        for args in ((None, d, 3, out), (sh, None, 3, out), (sh, d, 3, None), (sh, d, -1, out)):
            assert f(p(args[0]), p(args[1]), args[2], p(args[3])) == ERR_ARG and _message(mcpt)
    for v in (float("nan"), float("inf"), float("-inf")):
        bad_d = d.copy(); bad_d[1, 2] = v
        bad_sh = sh.copy(); bad_sh[2, 8, 1] = v
        assert L.mcpt_sh_basis(p(bad_d), 3, p(y)) == ERR_ARG and "finite" in _message(mcpt)
        for f in (L.mcpt_sh_radiance, L.mcpt_sh_irradiance):
            assert f(p(sh), p(bad_d), 3, p(out)) == ERR_ARG and "finite" in _message(mcpt)
            assert f(p(bad_sh), p(d), 3, p(out)) == ERR_ARG and "finite" in _message(mcpt)
    for what, nrm in (("zero", [0.0, 0.0, 0.0]), ("underflowing", [1e-200, 0.0, 0.0]), ("overflowing", [1e200, 1e200, 0.0])):
        bad_n = d.copy(); bad_n[2] = nrm
        assert L.mcpt_sh_irradiance(p(sh), p(bad_n), 3, p(out)) == ERR_ARG and "normal" in _message(mcpt), what
    # ... of which only the zero length troubles a direction: the basis takes what it is given
    assert L.mcpt_sh_basis(p(np.zeros((3, 3))), 3, p(y)) == 0


def _null_dev(mcpt):
    dev = mcpt.Device.__new__(mcpt.Device)
    dev._h = None
    return dev


def test_api_refusals(mcpt):
    """api.py: shapes and dtypes are ValueErrors; what the library refuses arrives as McptError with its code and message"""
    dev = _null_dev(mcpt)
    nd = _null_device_rc(mcpt)
    for bad in (np.zeros((3, 6)), np.zeros(3), np.zeros((2, 3, 3)), np.zeros((3, 2))):
        with pytest.raises(ValueError):
            dev.sh_probes(bad, 4)
        with pytest.raises(ValueError):
            dev.sh_probe_rays(bad, 0, np.zeros(3, dtype=np.int32))
        with pytest.raises(ValueError):
            mcpt.sh_basis(bad)
        with pytest.raises(ValueError):
            mcpt.sh_radiance(np.zeros((3, 9, 3)), bad)
        with pytest.raises(ValueError):
            mcpt.sh_irradiance(np.zeros((3, 9, 3)), bad)
    for bad_sh in (np.zeros((3, 27)), np.zeros((2, 9, 3)), np.zeros((3, 3, 9)), np.zeros((9, 3))):
        with pytest.raises(ValueError):
            mcpt.sh_radiance(bad_sh, POINTS)
        with pytest.raises(ValueError):
            mcpt.sh_irradiance(bad_sh, POINTS)
    for ids in (np.zeros(2, dtype=np.int32), np.zeros(3), np.array([0, 1, 2 ** 31])):
        with pytest.raises(ValueError):
            dev.sh_probes(POINTS, 4, ids=ids)
        with pytest.raises(ValueError):
            dev.sh_probe_rays(POINTS, 0, np.zeros(3, dtype=np.int32), ids=ids)
    for kw in (dict(spp=2.5), dict(spp=2 ** 31), dict(spp=4, sample_base=1.0), dict(spp=4, flags="2")):
        with pytest.raises(ValueError):
            dev.sh_probes(POINTS, **kw)
    with pytest.raises(ValueError):
        dev.sh_probe_rays(POINTS, 0, np.zeros(2, dtype=np.int32))
    with pytest.raises(ValueError):
        dev.sh_probe_rays(POINTS, 0, np.zeros(3))
    for what, kw in BAD_PARAMS:
        if "reserved" in kw:
            continue
        args = dict(spp=4)
        args.update(kw)
        with pytest.raises(mcpt.McptError) as e:
            dev.sh_probes(POINTS, **args)
        assert e.value.code == ERR_ARG and str(e.value), what
    for what, p3, ids in _bad_lists():
        with pytest.raises(mcpt.McptError) as e:
            dev.sh_probes(p3, 4, ids=ids)
        assert e.value.code == ERR_ARG and "probe" in str(e.value), what
        with pytest.raises(mcpt.McptError) as e:
            dev.sh_probe_rays(p3, 0, np.zeros(3, dtype=np.int32), ids=ids)
        assert e.value.code == ERR_ARG, what
    for f in (lambda: dev.sh_probes(POINTS, 4, seed=3, ids=[5, 6, 7], sample_base=2, flags=mcpt.RENDER_MEGAKERNEL, stats=mcpt.Stats()),
              lambda: dev.sh_probes(POINTS, 4), lambda: dev.sh_probe_rays(POINTS, 1, [0, 1, 2])):
        with pytest.raises(mcpt.McptError) as e:
            f()
        assert e.value.code == nd
    with pytest.raises(mcpt.McptError) as e:
        mcpt.sh_irradiance(np.zeros((3, 9, 3)), np.zeros((3, 3)))
    assert e.value.code == ERR_ARG


def test_the_constants_are_their_square_roots():
    pi = math.pi
    for got, want in ((sh_ref.C0, 1.0 / (2.0 * math.sqrt(pi))), (sh_ref.C1, math.sqrt(3.0 / (4.0 * pi))), (sh_ref.C2, math.sqrt(15.0 / (4.0 * pi))),
                      (sh_ref.C3, math.sqrt(5.0 / (16.0 * pi))), (sh_ref.C4, math.sqrt(15.0 / (16.0 * pi))), (sh_ref.FOUR_PI, 4.0 * pi),
                      (sh_ref.TWO_PI, 2.0 * pi), (sh_ref.A[0], pi), (sh_ref.A[1], 2.0 * pi / 3.0), (sh_ref.A[4], pi / 4.0)):
        assert abs(got - want) <= np.spacing(want), (got, want)          # the nearest double, or its neighbour where the expression rounds twice


def _directions():
    rng = np.random.default_rng(21)
    d = rng.normal(size=(4000, 3))
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    return np.concatenate([d, AXES]), rng


def test_host_helpers_are_the_restatement(mcpt):
    d, rng = _directions()
    n = d.shape[0]
    assert np.array_equal(_bits(mcpt.sh_basis(d)), _bits(sh_ref.basis(d)))
    sh = rng.normal(size=(n, 9, 3)) * 10.0 ** rng.uniform(-3, 3, size=(n, 1, 1))
    assert np.array_equal(_bits(mcpt.sh_radiance(sh, d)), _bits(sh_ref.radiance(sh, d)))
    # normals of any length: the helper normalises as the restatement does
    nrm = d * 10.0 ** rng.uniform(-3, 3, size=(n, 1))
    assert np.array_equal(_bits(mcpt.sh_irradiance(sh, nrm)), _bits(sh_ref.irradiance(sh, nrm)))
    assert np.array_equal(_bits(mcpt.sh_irradiance(sh, d)), _bits(sh_ref.irradiance(sh, d)))
    # n == 0
    assert mcpt.sh_basis(np.zeros((0, 3))).shape == (0, 9) and mcpt.sh_irradiance(np.zeros((0, 9, 3)), np.zeros((0, 3))).shape == (0, 3)


def test_the_basis_is_orthonormal():
    """On sh_ref alone.  Y_i Y_j is a polynomial of degree <= 4 in (x, y, z): Gauss-Legendre with 8 nodes in z (exact to degree 15) times
    the uniform rule with 16 nodes in phi (exact for trigonometric degree <= 15) integrates it exactly."""
    z, wz = np.polynomial.legendre.leggauss(8)
    m = 16
    phi = 2.0 * math.pi * (np.arange(m) + 0.5) / m
    Z, P = np.meshgrid(z, phi, indexing="ij")
    W = np.repeat(wz[:, None], m, axis=1) * (2.0 * math.pi / m)
    r = np.sqrt(1.0 - Z * Z)
    d = np.stack([r * np.cos(P), r * np.sin(P), Z], axis=-1).reshape(-1, 3)
    Y = sh_ref.basis(d)
    G = (Y[:, :, None] * Y[:, None, :] * W.reshape(-1)[:, None, None]).sum(axis=0)
    assert np.abs(G - np.eye(9)).max() <= 1e-12, np.abs(G - np.eye(9)).max()


def test_irradiance_of_unit_coefficients_and_of_constant_radiance(mcpt):
    d, rng = _directions()
    n = d.shape[0]
    Y = sh_ref.basis(sh_ref._nrm(d))            # (the irradiance normalises what it is given, a unit vector too)
    for i in range(9):
        sh = np.zeros((n, 9, 3))
        sh[:, i, :] = 1.0
        want = np.repeat((sh_ref.A[i] * Y[:, i])[:, None], 3, axis=1)
        for E in (sh_ref.irradiance(sh, d), mcpt.sh_irradiance(sh, d)):
            assert np.array_equal(_bits(E + 0.0), _bits(want + 0.0)), i         # (+ 0.0: the sum starts at +0.0, so a -0.0 term arrives as +0.0)
        assert sh_ref.A[i] == (math.pi, 2.0943951023931953, 0.7853981633974483)[sh_ref.BAND[i]]
    # constant radiance c: sh0 = c 2 sqrt(pi), the rest 0, and E = pi c for any normal, of any length
    c = np.array([0.3, 1.0, 17.25])
    sh = np.zeros((n, 9, 3))
    sh[:, 0, :] = c * (2.0 * math.sqrt(math.pi))
    nrm = d * 10.0 ** rng.uniform(-3, 3, size=(n, 1))
    for E in (sh_ref.irradiance(sh, nrm), mcpt.sh_irradiance(sh, nrm)):
        assert np.abs(E / (math.pi * c) - 1.0).max() <= 1e-15


def test_the_draw_is_uniform():
    """On sh_ref alone: over 10^5 keys the mean of d is 0 and the mean of d_i d_j is delta_ij / 3, each within 5 sigma of the sample's own
    standard error."""
    rng = np.random.default_rng(4)
    n = 100000
    ids = rng.integers(0, 2 ** 31, size=n)
    k = rng.integers(0, 2 ** 31, size=n)
    d = sh_ref.sphere_dirs(0x9E3779B97F4A7C15, ids, k)
    assert np.abs((d * d).sum(axis=1) - 1.0).max() <= 1e-15
    se = d.std(axis=0, ddof=1) / math.sqrt(n)
    assert np.all(np.abs(d.mean(axis=0)) <= 5.0 * se), d.mean(axis=0) / se
    for i in range(3):
        for j in range(i, 3):
            q = d[:, i] * d[:, j]
            s = q.std(ddof=1) / math.sqrt(n)
            assert abs(q.mean() - (1.0 / 3.0 if i == j else 0.0)) <= 5.0 * s, (i, j, q.mean(), s)
    # both hemispheres and every octant are reached
    assert len(set(map(tuple, (d > 0).tolist()))) == 8
