"""Not gpu: probe visibility on the host (mcpt_visibility_bin, mcpt_volume_irradiance_visible_host) against the numpy restatement
(tests/visibility_ref.py) bit for bit, the two identities the header promises -- with every factor 1 the lookup is the plain one under
the same mask, and on a valid probe it is that probe's own mcpt_sh_irradiance --, receivers nothing sees, indifference to the list's
order, and every refusal of the block's eight calls, each before the missing device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import visibility_ref
import volume_cases as VC
from conftest import ROOT

ERR_ARG, ERR_NO_DEVICE = -3, -4
NAMES = ["mcpt_visibility_bin", "mcpt_query_visibility", "mcpt_query_visibility_device", "mcpt_bake_volume_visibility",
         "mcpt_bake_volume_visibility_device", "mcpt_volume_irradiance_visible_host", "mcpt_volume_irradiance_visible",
         "mcpt_volume_irradiance_visible_device"]
PD, P32, PU8 = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
INT_MAX = 2 ** 31 - 1
COUNTS = sorted(VC.GRIDS)
RES = [1, 2, 3, 8, 16]
NAN, INF = float("nan"), float("inf")


def _null_device_rc(mcpt):
    return ERR_NO_DEVICE if mcpt.device_count() <= 0 else ERR_ARG


def _message(mcpt):
    return mcpt.lib().mcpt_last_error().decode()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def moments_for(counts, R, dmax, seed=0):
    """[nprobes, R * R, 2] synthetic maps: means in (0, dmax) with m2 >= mean^2, a fifth of the bins without data, a fifth with a
    variance of exactly 0"""
    rng = np.random.default_rng([seed, 41, R, *counts])
    n = counts[0] * counts[1] * counts[2]
    mu = dmax * (0.02 + 0.96 * rng.random((n, R * R)))
    m2 = mu * mu + (0.3 * dmax * rng.random((n, R * R))) ** 2
    kind = rng.random((n, R * R))
    m2 = np.where(kind < 0.2, mu * mu, m2)
    none = kind > 0.8
    return np.ascontiguousarray(np.stack([np.where(none, -1.0, mu), np.where(none, 0.0, m2)], axis=2))


def _dmax(counts):
    return 1.5 * float(np.sqrt(sum(s * s for s in VC.GRIDS[counts][1])))


def _ref(counts, sh, m, x, b, R, dmax, bias=0.0, minv=0.0, valid=None, clamp=False):
    origin, spacing = VC.GRIDS[counts]
    return visibility_ref.irradiance(origin, spacing, counts, sh, m, x, b, R, dmax, bias, minv, valid, clamp)


def test_visibility_symbols_are_declared_and_exported(mcpt):
    from montecarlopathtracing_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for sym in NAMES:
        assert (sym + "(") in hdr and sym in _lib.EXPORTS and hasattr(L, sym), sym
    assert "} mcpt_visibility_params;" in hdr and "} mcpt_volume_visibility;" in hdr
    assert "#define MCPT_VERSION 105" in hdr and mcpt.lib().mcpt_version() == 105
    for f in ("probe_visibility", "bake_volume_visibility", "volume_irradiance_visible"):
        assert callable(getattr(mcpt.Device, f))
    for f in ("visibility_bin", "volume_visibility", "volume_irradiance_visible_host"):
        assert callable(getattr(mcpt, f))


def test_struct_layouts_match_the_header(mcpt, tmp_path):
    from montecarlopathtracing_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    if cc is None:
        pytest.skip("no C compiler")
    structs = [("mcpt_visibility_params", _lib.VisibilityParams, 56,
                ["spp", "sample_base", "seed", "res", "reserved0", "max_distance", "max_back_fraction", "workspace_rays", "reserved"]),
               ("mcpt_volume_visibility", _lib.VolumeVisibility, 48, ["res", "flags", "max_distance", "normal_bias", "min_visibility", "reserved"])]
    body = ""
    for name, cls, _, fields in structs:
        assert [n for n, _ in cls._fields_] == fields
        body += "  printf(\"%%zu\\n\", sizeof(%s));\n" % name + "".join("  printf(\"%%zu\\n\", offsetof(%s, %s));\n" % (name, f) for f in fields)
    src = tmp_path / "layout_vis.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"mcpt.h\"\nint main(void) {\n" + body + "  return 0;\n}\n")
    exe = tmp_path / "layout_vis"
    subprocess.check_call([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    at = 0
    for name, cls, size, fields in structs:
        assert out[at] == C.sizeof(cls) == size, name
        for i, f in enumerate(fields):
            assert out[at + 1 + i] == getattr(cls, f).offset, (name, f)
        at += 1 + len(fields)


def _directions():
    rng = np.random.default_rng(17)
    d = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    d += [[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    for z in (0.0, -0.0):
        d += [[1, 0, z], [0, 1, z], [-1, 0, z], [0.3, -0.7, z], [-0.5, -0.5, z], [0.5, 0.5, z]]
    # u or v exactly on a bin edge: k / R for the tested R, on both hemispheres
    for R in RES:
        for k in range(-R, R + 1):
            u = k / R
            for z in (1.0, -1.0):
                d += [[u, 0.0, (1.0 - abs(u)) * z], [0.0, u, (1.0 - abs(u)) * z], [u, 1.0 - abs(u), 0.0 * z]]
    d += [[0.5, 0.5, 0], [0.25, 0.25, 0.5], [0.25, -0.25, -0.5]]
    d += [[1e-300, 0, 0], [0, -1e-300, 0], [1e-300, 1e-300, 1e-300], [1e-300, -1e-300, -1e-300], [1e-300, 1.0, 0], [1.0, 1e-300, -1e-300]]
    d += [[1e300, 1e300, -1e300], [1e-310, 0, 0]]
    r = rng.normal(size=(4000, 3)) * 10.0 ** rng.uniform(-3, 3, size=(4000, 1))
    return np.concatenate([np.array(d, dtype=np.float64), r])


@pytest.mark.parametrize("R", RES)
def test_bin_helper_is_the_restatement(mcpt, R):
    d = _directions()
    got = mcpt.visibility_bin(d, R)
    want = visibility_ref.bin_of(d, R)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert got.min() >= 0 and got.max() <= R * R - 1
    assert len(set(got.tolist())) == R * R                                  # every bin is reached
    # the axes, spelled out: +x is the right edge's middle, +z the centre, -z a corner
    ax = mcpt.visibility_bin(np.array([[1.0, 0, 0], [0, 0, 1.0], [0, 0, -1.0]]), R)
    assert ax.tolist() == [min(R // 2, R - 1) * R + R - 1, (R // 2) * R + R // 2, (R - 1) * R + R - 1]


def test_bin_helper_refuses(mcpt):
    L = mcpt.lib()
    out = np.zeros(4, dtype=np.int32)
    good = np.tile([0.0, 0.6, 0.8], (4, 1))
    for bad in ([NAN, 0, 1], [0, INF, 1], [0, 1, -INF], [0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [1e308, 1e308, 1e308]):
        d = good.copy()
        d[2] = bad
        assert L.mcpt_visibility_bin(d.ctypes.data_as(PD), 4, 8, out.ctypes.data_as(P32)) == ERR_ARG, bad
        assert "direction 2" in _message(mcpt)
        with pytest.raises(mcpt.McptError):
            mcpt.visibility_bin(d, 8)
    for R in (0, -1, 17, 2 ** 20):
        assert L.mcpt_visibility_bin(good.ctypes.data_as(PD), 4, R, out.ctypes.data_as(P32)) == ERR_ARG and "res" in _message(mcpt)
    assert L.mcpt_visibility_bin(good.ctypes.data_as(PD), -1, 8, out.ctypes.data_as(P32)) == ERR_ARG
    assert L.mcpt_visibility_bin(None, 4, 8, out.ctypes.data_as(P32)) == ERR_ARG
    assert L.mcpt_visibility_bin(good.ctypes.data_as(PD), 4, 8, None) == ERR_ARG
    assert L.mcpt_visibility_bin(None, 0, 8, None) == 0
    assert mcpt.visibility_bin(np.zeros((0, 3)), 8).shape == (0,)
    with pytest.raises(ValueError):
        mcpt.visibility_bin(np.zeros((3, 2)), 8)


@pytest.mark.parametrize("bias,minv", [(0.0, 0.0), (0.05, 0.0), (0.0, 1e-3), (0.05, 1e-3)])
@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("counts", COUNTS)
def test_host_lookup_is_the_restatement_bit_for_bit(mcpt, counts, masked, clamp, bias, minv):
    R = {(1, 1, 1): 1, (1, 7, 1): 3, (5, 4, 3): 8, (33, 17, 9): 16}[counts] if not masked else {(1, 1, 1): 16, (1, 7, 1): 8, (5, 4, 3): 2, (33, 17, 9): 3}[counts]
    dmax = _dmax(counts)
    sh, m = VC.coefficients(counts), moments_for(counts, R, dmax)
    x, b = VC.receivers(counts)
    valid = VC.mask(counts) if masked else None
    vis = mcpt.volume_visibility(R, dmax, bias, minv)
    E, corners = mcpt.volume_irradiance_visible_host(VC.grid(mcpt, counts, clamp_zero=clamp), sh, m, x, b, vis, valid=valid)
    want_E, want_c = _ref(counts, sh, m, x, b, R, dmax, bias, minv, valid, clamp)
    bad = int((_bits(E) != _bits(want_E)).sum())
    print("%r R %d masked %d clamp %d bias %g min %g: %d of %d values differ, corners 0..%d" % (counts, R, masked, clamp, bias, minv, bad, E.size, corners.max()))
    assert bad == 0
    assert np.array_equal(corners, want_c)
    assert np.all(np.isfinite(E)) and np.abs(E).max() > 0
    if clamp:
        assert E.min() == 0.0 and not np.signbit(E).any()
    # the factors do something: the plain lookup under the same mask answers differently somewhere
    plain, _ = mcpt.volume_irradiance_host(VC.grid(mcpt, counts, clamp_zero=clamp), sh, x, b, valid=valid if masked else np.ones(len(sh), dtype=np.uint8))
    if counts != (1, 1, 1):
        assert not _same(plain, E)


@pytest.mark.parametrize("R", [1, 8])
@pytest.mark.parametrize("counts", COUNTS)
def test_with_every_factor_one_the_lookup_is_the_plain_one(mcpt, counts, R):
    """identity (a): moments all (-1, 0)"""
    n = counts[0] * counts[1] * counts[2]
    sh = VC.coefficients(counts)
    x, b = VC.receivers(counts)
    m = np.tile([-1.0, 0.0], (n, R * R, 1))
    for clamp in (False, True):
        g = VC.grid(mcpt, counts, clamp_zero=clamp)
        for bias, minv in ((0.0, 0.0), (0.05, 1e-3)):
            vis = mcpt.volume_visibility(R, _dmax(counts), bias, minv)
            for valid in (None, VC.mask(counts)):
                E, c = mcpt.volume_irradiance_visible_host(g, sh, m, x, b, vis, valid=valid)
                pE, pc = mcpt.volume_irradiance_host(g, sh, x, b, valid=valid if valid is not None else np.ones(n, dtype=np.uint8))
                assert _same(E, pE) and np.array_equal(c, pc)


@pytest.mark.parametrize("counts", COUNTS)
def test_on_a_valid_probe_the_lookup_is_that_probes_irradiance(mcpt, counts):
    """identity (b): every probe of the grid, normal_bias 0, a full mask and random masks that keep the probe"""
    R, dmax = 8, _dmax(counts)
    sh, m = VC.coefficients(counts), moments_for(counts, R, dmax, seed=3)
    pp = VC.probe_points(counts)
    n = pp.shape[0]
    rng = np.random.default_rng(9)
    g = VC.grid(mcpt, counts)
    for k in range(4):
        b = np.tile(VC.AXES[k], (n, 1)) if k < 2 else rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 3, size=(n, 1))
        want = mcpt.sh_irradiance(sh, b)
        for minv in (0.0, 1e-3):
            vis = mcpt.volume_visibility(R, dmax, 0.0, minv)
            for valid in (None, np.ones(n, dtype=np.uint8), VC.mask(counts, seed=k, keep=0.3)):
                keep = np.ones(n, dtype=bool) if valid is None else valid != 0
                E, corners = mcpt.volume_irradiance_visible_host(g, sh, m, pp[keep], b[keep], vis, valid=valid)
                assert _same(E, want[keep]) and np.array_equal(corners, np.ones(keep.sum()))


def test_a_receiver_nothing_sees_gives_zero(mcpt):
    """var = 0 and dc > mu at every corner, min_visibility = 0: every factor is 0"""
    counts, R = (5, 4, 3), 8
    origin, spacing = (np.array(v) for v in VC.GRIDS[counts])
    n = 60
    sh = VC.coefficients(counts)
    m = np.tile([0.01, 0.01 * 0.01], (n, R * R, 1))
    rng = np.random.default_rng(5)
    x = origin + (np.array([1, 1, 0]) + 0.2 + 0.6 * rng.random((50, 3))) * spacing       # well inside cells: further than 0.01 from every probe
    b = rng.normal(size=(50, 3))
    g = VC.grid(mcpt, counts)
    E, corners = mcpt.volume_irradiance_visible_host(g, sh, m, x, b, mcpt.volume_visibility(R, 2.0, 0.0, 0.0))
    assert np.array_equal(corners, np.zeros(50, dtype=np.int32))
    assert np.array_equal(_bits(E), np.zeros((50, 3), dtype=np.uint64))                   # +0.0, not -0.0
    # a floor under the factor brings every corner back, with the plain weights: the factors are all equal
    E2, c2 = mcpt.volume_irradiance_visible_host(g, sh, m, x, b, mcpt.volume_visibility(R, 2.0, 0.0, 0.5))
    assert np.array_equal(c2, np.full(50, 8)) and np.abs(E2).min() > 0
    want, wc = _ref(counts, sh, m, x, b, R, 2.0, 0.0, 0.5)
    assert _same(E2, want) and np.array_equal(c2, wc)


def test_a_permuted_list_gives_permuted_answers(mcpt):
    counts, R = (5, 4, 3), 8
    dmax = _dmax(counts)
    sh, valid, m = VC.coefficients(counts), VC.mask(counts), moments_for(counts, R, dmax)
    x, b = VC.receivers(counts)
    perm = np.random.default_rng(1).permutation(VC.N)
    g, vis = VC.grid(mcpt, counts), mcpt.volume_visibility(R, dmax, 0.05, 0.0)
    E, c = mcpt.volume_irradiance_visible_host(g, sh, m, x, b, vis, valid=valid)
    E2, c2 = mcpt.volume_irradiance_visible_host(g, sh, m, x[perm], b[perm], vis, valid=valid)
    assert _same(E[perm], E2) and np.array_equal(c[perm], c2)
    # the arrays may come shaped as the bakes return them
    E3, _ = mcpt.volume_irradiance_visible_host(g, sh.reshape(3, 4, 5, 9, 3), m.reshape(3, 4, 5, R * R, 2), x, b, vis, valid=valid.reshape(3, 4, 5))
    assert _same(E, E3)


def test_the_leak_limit_holds_on_analytic_depths_with_a_tenth_to_spare(mcpt):
    """tests/test_gpu_visibility.py's two rooms without a GPU: 1024 numpy-drawn uniform directions per probe, the depth of the rooms'
    own planes, the fold and the lookup of the restatement and of the host form.  Receivers in the dark room B keep less than a
    thousandth of what the plain lookup leaks to them -- the GPU test asserts a hundredth."""
    rng = np.random.default_rng(12)
    R, spp, maxd = 8, 1024, 1.5
    probes = np.array([[1.55, 1.0, 1.0], [2.55, 1.0, 1.0]])
    rooms = [((0.0, 0.0, 0.0), (2.0, 2.0, 2.0)), ((2.1, 0.0, 0.0), (4.1, 2.0, 2.0))]
    moments = []
    for o, (lo, hi) in zip(probes, rooms):
        d = rng.normal(size=(spp, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        with np.errstate(divide="ignore"):
            t = np.min(np.where(d > 0, (np.array(hi) - o) / d, (np.array(lo) - o) / d), axis=1)
        moments.append(visibility_ref.fold(d, np.ones(spp, dtype=bool), t, -d, R, maxd, 0.25)[0])
    moments = np.stack(moments)
    sh = np.zeros((2, 9, 3))
    sh[0, 0] = [3.0, 2.0, 1.0]
    g = mcpt.volume_grid((1.55, 1.0, 1.0), (1.0, 1.0, 1.0), (2, 1, 1))
    n = 500
    x = np.stack([2.25 + 0.25 * rng.random(n), 0.9 + 0.2 * rng.random(n), 0.9 + 0.2 * rng.random(n)], axis=1)
    b = np.tile([-1.0, 0.0, 0.0], (n, 1))
    plain, _ = mcpt.volume_irradiance_host(g, sh, x, b)
    seen, corners = mcpt.volume_irradiance_visible_host(g, sh, moments, x, b, mcpt.volume_visibility(R, maxd))
    want, _ = visibility_ref.irradiance((1.55, 1.0, 1.0), (1.0, 1.0, 1.0), (2, 1, 1), sh, moments, x, b, R, maxd)
    assert _same(seen, want) and (plain > 0).all()
    ratio = (seen / plain).max()
    # the bins towards the receivers: what the limit's reasoning says of them
    toward = np.unique(visibility_ref.bin_of(x - probes[0], R))
    mu, m2 = moments[0, toward, 0], moments[0, toward, 1]
    print("leak: E_visible / E_plain <= %.3e; bins %r: mu %.4f .. %.4f, var <= %.2e" % (ratio, toward.tolist(), mu.min(), mu.max(), (m2 - mu * mu).max()))
    assert ratio <= 1e-3
    assert mu.max() <= 0.5 and (m2 - mu * mu).max() <= 6e-4
    # and receivers in A gain: the probe behind the wall loses its weight
    xa = x - [0.65, 0.0, 0.0]
    plain_a, _ = mcpt.volume_irradiance_host(g, sh, xa, b)
    seen_a, _ = mcpt.volume_irradiance_visible_host(g, sh, moments, xa, b, mcpt.volume_visibility(R, maxd))
    assert (seen_a > plain_a).all()


# ---- refusals

def _grid(mcpt, origin=(0.1, 0.2, 0.3), spacing=(0.3, 0.7, 1.1), counts=(2, 2, 2), flags=0, reserved=(0, 0, 0, 0)):
    return mcpt.VolumeGrid((C.c_double * 3)(*origin), (C.c_double * 3)(*spacing), counts[0], counts[1], counts[2], flags, (C.c_int32 * 4)(*reserved))


def _vp(mcpt, spp=4, sample_base=0, seed=1, res=2, reserved0=0, max_distance=1.0, max_back_fraction=0.25, workspace_rays=0, reserved=(0, 0)):
    return mcpt.VisibilityParams(spp, sample_base, seed, res, reserved0, max_distance, max_back_fraction, workspace_rays, (C.c_int32 * 2)(*reserved))


def _vv(mcpt, res=2, flags=0, max_distance=1.0, normal_bias=0.0, min_visibility=0.0, reserved=(0, 0, 0, 0)):
    return mcpt.VolumeVisibility(res, flags, max_distance, normal_bias, min_visibility, (C.c_int32 * 4)(*reserved))


def _ptr(a, t=PD):
    return a.ctypes.data_as(t) if a is not None else None


def _addr(a):
    return a.ctypes.data if a is not None else None


def _bakes(L, g, vp, p3, n, m, ids=None):
    """the four bakes with a null device (the device forms' pointers are not looked at); the grid forms only when g is given"""
    vpp = C.byref(vp) if vp is not None else None
    out = [L.mcpt_query_visibility(None, _ptr(p3), _ptr(ids, P32), n, vpp, _ptr(m), None, None, None, None),
           L.mcpt_query_visibility_device(None, _addr(p3), _addr(ids), n, vpp, _addr(m), None, None, None, None, None)]
    if g is not False:
        gp = C.byref(g) if g is not None else None
        out += [L.mcpt_bake_volume_visibility(None, gp, vpp, _ptr(m), None, None, None, None),
                L.mcpt_bake_volume_visibility_device(None, gp, vpp, _addr(m), None, None, None, None, None)]
    return out


def _lookups(L, g, vv, sh, m, valid, q, n, e, device=True):
    """the three forms of the lookup with a null device (the device form's pointers are not looked at; device=False: the other two)"""
    gp, vvp = C.byref(g) if g is not None else None, C.byref(vv) if vv is not None else None
    out = [L.mcpt_volume_irradiance_visible_host(gp, _ptr(sh), _ptr(m), _ptr(valid, PU8), vvp, _ptr(q), n, _ptr(e), None),
           L.mcpt_volume_irradiance_visible(None, gp, _ptr(sh), _ptr(m), _ptr(valid, PU8), vvp, _ptr(q), n, _ptr(e), None)]
    if device:
        out.append(L.mcpt_volume_irradiance_visible_device(None, gp, _addr(sh), _addr(m), None, vvp, _addr(q), n, _addr(e), None, None))
    return out


# the bakes' refusals in the header's order: each entry is refused with a message of its own, and wins over everything after it
BAKE_ORDER = [("spp must", dict(spp=0)), ("sample_base must", dict(sample_base=-1)), ("sample_base + spp", dict(spp=2, sample_base=INT_MAX - 1)),
              ("res must", dict(res=17)), ("max_distance", dict(max_distance=0.0)), ("max_back_fraction", dict(max_back_fraction=1.5)),
              ("workspace_rays", dict(workspace_rays=-1)), ("reserved", dict(reserved=(0, 1)))]
BAD_BAKE = [dict(spp=-3), dict(res=0), dict(res=-1), dict(max_distance=NAN), dict(max_distance=INF), dict(max_distance=-1.0),
            dict(max_back_fraction=NAN), dict(max_back_fraction=-0.1), dict(max_back_fraction=INF), dict(workspace_rays=-2 ** 40),
            dict(reserved0=1), dict(reserved=(3, 0))]
LOOKUP_ORDER = [("res must", dict(res=0)), ("flags", dict(flags=1)), ("max_distance", dict(max_distance=-1.0)), ("normal_bias", dict(normal_bias=-0.1)),
                ("min_visibility", dict(min_visibility=2.0)), ("reserved", dict(reserved=(0, 0, 0, 1)))]
BAD_LOOKUP = [dict(res=17), dict(flags=-1), dict(max_distance=NAN), dict(max_distance=INF), dict(max_distance=0.0), dict(normal_bias=NAN),
              dict(normal_bias=INF), dict(min_visibility=NAN), dict(min_visibility=-0.5), dict(reserved=(1, 0, 0, 0))]


def test_bake_refusals_come_in_order_and_before_the_missing_device(mcpt):
    L = mcpt.lib()
    nd = _null_device_rc(mcpt)
    good = _grid(mcpt)
    p3, m = np.zeros((8, 3)) + 0.5, np.zeros((8, 4, 2))
    # NULL parameters; the grid forms: a NULL grid or NULL parameters, before an invalid grid is looked at
    assert _bakes(L, good, None, p3, 8, m) == [ERR_ARG] * 4 and "null" in _message(mcpt)
    assert _bakes(L, None, _vp(mcpt), p3, 8, m)[2:] == [ERR_ARG] * 2 and "null" in _message(mcpt)
    bad_grid = _grid(mcpt, counts=(0, 2, 2))
    assert _bakes(L, bad_grid, None, p3, 8, m)[2:] == [ERR_ARG] * 2 and "null" in _message(mcpt)
    # an invalid grid before bad parameters
    assert _bakes(L, bad_grid, _vp(mcpt, spp=0), p3, 8, None)[2:] == [ERR_ARG] * 2 and "at least one probe" in _message(mcpt)
    # the parameters, in order
    for i, (word, kw) in enumerate(BAKE_ORDER):
        merged = {}
        for _, later in reversed(BAKE_ORDER[i:]):
            merged.update(later)
        merged.update(kw)
        got = _bakes(L, good, _vp(mcpt, **merged), None, -1, None)
        assert got == [ERR_ARG] * 4 and word in _message(mcpt), (word, _message(mcpt))
    for kw in BAD_BAKE:
        assert _bakes(L, good, _vp(mcpt, **kw), p3, 8, m) == [ERR_ARG] * 4, kw
    # then the count, then the arrays (the grid forms have a count of their own)
    for n in (-1, 2 ** 31, 2 ** 40):
        assert _bakes(L, False, _vp(mcpt), None, n, None) == [ERR_ARG] * 2 and "probes" in _message(mcpt)
    assert _bakes(L, good, _vp(mcpt), None, 8, m) == [ERR_ARG] * 2 + [nd] * 2
    assert _bakes(L, good, _vp(mcpt), p3, 8, None) == [ERR_ARG] * 4
    # the host-pointer list form looks at the list; the device form does not
    ids = np.arange(8, dtype=np.int32)
    ids[3] = -1
    assert L.mcpt_query_visibility(None, _ptr(p3), _ptr(ids, P32), 8, C.byref(_vp(mcpt)), _ptr(m), None, None, None, None) == ERR_ARG
    assert "probe 3" in _message(mcpt)
    assert _bakes(L, False, _vp(mcpt), p3, 8, m, ids) == [ERR_ARG, nd]
    for v in (NAN, INF, -INF):
        p2 = p3.copy()
        p2[5, 1] = v
        assert L.mcpt_query_visibility(None, _ptr(p2), None, 8, C.byref(_vp(mcpt)), _ptr(m), None, None, None, None) == ERR_ARG
        assert "probe 5" in _message(mcpt)
    # valid arguments miss the device; the limits themselves pass
    assert _bakes(L, good, _vp(mcpt), p3, 8, m) == [nd] * 4
    assert _bakes(L, good, _vp(mcpt, spp=1, sample_base=INT_MAX - 1, res=16, max_back_fraction=1.0, workspace_rays=2 ** 62), p3, 8, np.zeros((8, 256, 2))) == [nd] * 4
    assert _bakes(L, good, _vp(mcpt, res=1, max_back_fraction=0.0, max_distance=1e-300), p3, 8, m) == [nd] * 4
    if nd == ERR_NO_DEVICE:
        assert "device" in _message(mcpt).lower()
    # n == 0 needs no arrays -- the forms still miss the device first
    assert _bakes(L, False, _vp(mcpt), None, 0, None) == [nd] * 2


def test_lookup_refusals_come_in_order_and_before_the_missing_device(mcpt):
    L = mcpt.lib()
    nd = _null_device_rc(mcpt)
    good = _grid(mcpt)
    sh, q, e = np.ones((8, 9, 3)), np.tile([0.2, 0.3, 0.4, 0.0, 0.0, 1.0], (3, 1)), np.zeros((3, 3))
    m = np.tile([0.5, 0.3], (8, 4, 1))
    # the grid's errors first -- before a NULL struct, a bad count and NULL arrays
    assert _lookups(L, None, None, None, None, None, None, -1, None) == [ERR_ARG] * 3 and "grid" in _message(mcpt)
    for kw, word in ((dict(origin=(NAN, 0, 0)), "origin"), (dict(spacing=(0.0, 1, 1)), "spacing"), (dict(counts=(0, 1, 1)), "at least one probe"),
                     (dict(flags=2), "flag"), (dict(reserved=(0, 0, 0, 1)), "reserved")):
        assert _lookups(L, _grid(mcpt, **kw), None, None, None, None, None, -1, None) == [ERR_ARG] * 3 and word in _message(mcpt), kw
    # then the struct: NULL, then its fields in order
    assert _lookups(L, good, None, None, None, None, None, -1, None) == [ERR_ARG] * 3 and "null volume visibility" in _message(mcpt)
    for i, (word, kw) in enumerate(LOOKUP_ORDER):
        merged = {}
        for _, later in reversed(LOOKUP_ORDER[i:]):
            merged.update(later)
        assert _lookups(L, good, _vv(mcpt, **merged), None, None, None, None, -1, None) == [ERR_ARG] * 3 and word in _message(mcpt), (word, _message(mcpt))
    for kw in BAD_LOOKUP:
        assert _lookups(L, good, _vv(mcpt, **kw), sh, m, None, q, 3, e) == [ERR_ARG] * 3, kw
    # then the count, then the arrays
    for n in (-1, 2 ** 31, 2 ** 40):
        assert _lookups(L, good, _vv(mcpt), None, None, None, None, n, None) == [ERR_ARG] * 3 and "receivers" in _message(mcpt)
    for drop in range(4):
        args = [sh, m, q, e]
        args[drop] = None
        assert _lookups(L, good, _vv(mcpt), args[0], args[1], None, args[2], 3, args[3]) == [ERR_ARG] * 3, drop
    # the host-pointer forms look at the arrays: mcpt_volume_irradiance's checks ...
    s2 = sh.copy()
    s2[1, 2, 0] = NAN
    assert _lookups(L, good, _vv(mcpt), s2, m, None, q, 3, e, device=False) == [ERR_ARG] * 2 and "coefficient" in _message(mcpt)
    q2 = q.copy()
    q2[1, 3:] = 0.0
    assert _lookups(L, good, _vv(mcpt), sh, m, None, q2, 3, e, device=False) == [ERR_ARG] * 2 and "normal" in _message(mcpt)
    # ... then the moments: finite with a mean >= 0, or exactly (-1, 0)
    for mom in ([NAN, 0.3], [0.5, NAN], [INF, 0.3], [0.5, INF], [-0.5, 0.3], [-1.0, 0.3], [-1.0, -0.5], [-2.0, 0.0]):
        m2 = m.copy()
        m2[6, 3] = mom
        assert _lookups(L, good, _vv(mcpt), sh, m2, None, q, 3, e, device=False) == [ERR_ARG] * 2, mom
        assert "probe 6, bin 3" in _message(mcpt)
        assert _lookups(L, good, _vv(mcpt), sh, m2, None, q, 3, e)[2] == nd                 # the device form does not look
        assert _lookups(L, good, _vv(mcpt), s2, m2, None, q, 3, e, device=False) == [ERR_ARG] * 2 and "coefficient" in _message(mcpt)
    for mom in ([-1.0, 0.0], [-1.0, -0.0], [0.0, 0.0], [0.5, 0.0], [1e300, 1e300]):
        m2 = m.copy()
        m2[6, 3] = mom
        assert _lookups(L, good, _vv(mcpt), sh, m2, None, q, 3, e) == [0, nd, nd], mom
    # valid arguments: the host form answers, the others miss the device; the limits themselves pass
    assert _lookups(L, good, _vv(mcpt), sh, m, None, q, 3, e) == [0, nd, nd]
    assert _lookups(L, good, _vv(mcpt, res=16, min_visibility=1.0, normal_bias=1e300), sh, np.tile([0.5, 0.3], (8, 256, 1)), None, q, 3, e) == [0, nd, nd]
    assert _lookups(L, good, _vv(mcpt), None, None, None, None, 0, None) == [0, nd, nd]
    E, c = mcpt.volume_irradiance_visible_host(good, sh, m, np.zeros((0, 3)), np.zeros((0, 3)), _vv(mcpt))
    assert E.shape == (0, 3) and c.shape == (0,)


def test_api_validates_shapes(mcpt):
    g = _grid(mcpt)
    sh, x, m = np.ones((8, 9, 3)), np.zeros((3, 3)), np.tile([0.5, 0.3], (8, 4, 1))
    vis = mcpt.volume_visibility(2, 1.0)
    assert (vis.res, vis.flags, vis.max_distance, vis.normal_bias, vis.min_visibility) == (2, 0, 1.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        mcpt.volume_irradiance_visible_host(g, sh, np.ones((8, 9, 2)), x, x + 1, vis)
    with pytest.raises(ValueError):
        mcpt.volume_irradiance_visible_host(g, sh, np.ones((8, 4, 3)), x, x + 1, vis)
    with pytest.raises(ValueError):
        mcpt.volume_irradiance_visible_host(g, sh, m, x, x + 1, (2, 1.0))
    with pytest.raises(ValueError):
        mcpt.volume_irradiance_visible_host(g, np.ones((7, 9, 3)), m, x, x + 1, vis)
    with pytest.raises(ValueError):
        mcpt.volume_visibility(2.5, 1.0)
    with pytest.raises(mcpt.McptError):
        mcpt.volume_irradiance_visible_host(g, sh, m, x, x + 1, mcpt.volume_visibility(2, -1.0))
