"""Not gpu: ambient occlusion (include/mcpt.h: ambient occlusion) as far as it goes without a device.  The symbols and both struct layouts
against the header; every refusal of the five calls in the header's order, before the missing device; mcpt_occlusion_fold_host against
the numpy restatement (tests/occlusion_ref.py) bit for bit on synthetic rays -- 1 and 7 entries of 1 to 65 samples, the three falloffs,
distances of 0, denormal, exactly max_distance, either side of it and 1e300, misses, entries nothing of which is open, entries whose
weighted directions cancel, face normals on both sides of the ray --; indifference to the list's order; and occlusion.hpp under the
address and undefined-behaviour sanitizers in a stand-alone program (tests/occlusion_sanitize_main.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import occlusion_ref as OR
from conftest import ROOT

CSRC = os.path.join(ROOT, "montecarlopathtracing_amd", "csrc")
ERR_ARG, ERR_NO_DEVICE = -3, -4
NAMES = ["mcpt_query_occlusion", "mcpt_query_occlusion_device", "mcpt_occlusion_fold_host", "mcpt_bake_occlusion_lightmap",
         "mcpt_bake_occlusion_lightmap_device"]
PD, P32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
INT_MAX = 2 ** 31 - 1
NAN, INF = float("nan"), float("inf")
FALLOFFS = ["hard", "linear", "square"]


def _null_device_rc(mcpt):
    return ERR_NO_DEVICE if mcpt.device_count() <= 0 else ERR_ARG


def _message(mcpt):
    return mcpt.lib().mcpt_last_error().decode()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want):
    return all(np.array_equal(_bits(got[k]), _bits(want[k])) for k in ("ao", "stderr", "bent")) and all(
        got[k].dtype == np.int32 and np.array_equal(got[k], want[k]) for k in ("hits", "back"))


def test_occlusion_symbols_are_declared_and_exported(mcpt):
    from montecarlopathtracing_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for sym in NAMES:
        assert (sym + "(") in hdr and sym in _lib.EXPORTS and hasattr(L, sym), sym
    assert "} mcpt_occlusion_params;" in hdr and "} mcpt_occlusion_map;" in hdr
    for i, name in enumerate(("HARD", "LINEAR", "SQUARE")):
        assert "#define MCPT_OCCLUSION_%s %d" % (name.ljust(6), i) in hdr and getattr(mcpt, "OCCLUSION_" + name) == i
    assert "#define MCPT_VERSION 105" in hdr and mcpt.lib().mcpt_version() == 105
    for f in ("occlusion", "bake_occlusion_lightmap"):
        assert callable(getattr(mcpt.Device, f))
    assert callable(mcpt.occlusion_fold_host)


def test_struct_layouts_match_the_header(mcpt, tmp_path):
    from montecarlopathtracing_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("g++")
    if cc is None:
        pytest.skip("no C compiler")
    structs = [("mcpt_occlusion_params", _lib.OcclusionParams, 48,
                ["spp", "sample_base", "seed", "falloff", "flags", "max_distance", "workspace_rays", "reserved"]),
               ("mcpt_occlusion_map", _lib.OcclusionMap, 16, ["width", "height", "dilate", "reserved"])]
    body = ""
    for name, cls, _, fields in structs:
        assert [n for n, _ in cls._fields_] == fields
        body += "  printf(\"%%zu\\n\", sizeof(%s));\n" % name + "".join("  printf(\"%%zu\\n\", offsetof(%s, %s));\n" % (name, f) for f in fields)
    src = tmp_path / "layout_occ.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"mcpt.h\"\nint main(void) {\n" + body + "  return 0;\n}\n")
    exe = tmp_path / "layout_occ"
    subprocess.check_call([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    at = 0
    for name, cls, size, fields in structs:
        assert out[at] == C.sizeof(cls) == size, name
        for i, f in enumerate(fields):
            assert out[at + 1 + i] == getattr(cls, f).offset, (name, f)
        at += 1 + len(fields)


# ---- the fold against the restatement

MAXD = 0.75
EDGE_T = [0.0, 5e-324, 1e-310, MAXD, np.nextafter(MAXD, 0.0), np.nextafter(MAXD, 1.0), 1e300, 0.1, 0.5]


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def synthetic(n, spp, seed=0):
    """n entries of spp rays: random normals and directions, a third of the rays miss, the distances go round EDGE_T and random values
    either side of MAXD, the face normals lie on either side of the ray.  Entry 0's rays all hit at distance 0 (nothing is open under
    any falloff); with n == 7, entry 1's open directions cancel exactly (pairs d, -d that all miss) and entry 2 misses everything."""
    rng = np.random.default_rng([seed, n, spp])
    normals = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 3, size=(n, 1))
    points = rng.normal(size=(n, 3))
    m = n * spp
    d = _unit(rng.normal(size=(m, 3)))
    hit = (rng.random(m) > 1.0 / 3.0).astype(np.int32)
    t = np.where(rng.random(m) < 0.5, 2.0 * MAXD * rng.random(m), np.array(EDGE_T)[np.arange(m) % len(EDGE_T)])
    fn = _unit(rng.normal(size=(m, 3)))
    hit[:spp], t[:spp] = 1, 0.0
    if n >= 3:
        s = slice(spp, 2 * spp)
        half = spp // 2
        d[s][1:2 * half:2] = -d[s][0:2 * half:2]                                       # d, -d, d', -d', ...: the sum is back at 0 after every pair
        if spp % 2:
            d[s][-1], hit[s.stop - 1], t[s.stop - 1] = [0.0, 0.0, 1.0], 1, 0.0          # (the odd one out is closed: v = 0)
        hit[spp:spp + 2 * half] = 0
        hit[2 * spp:3 * spp] = 0
    rays = np.concatenate([rng.normal(size=(m, 3)), d], axis=1)
    return points, normals, rays, hit, t, fn


@pytest.mark.parametrize("falloff", FALLOFFS)
@pytest.mark.parametrize("spp", [1, 2, 63, 64, 65])
@pytest.mark.parametrize("n", [1, 7])
def test_host_fold_is_the_restatement_bit_for_bit(mcpt, n, spp, falloff):
    points, normals, rays, hit, t, fn = synthetic(n, spp)
    got = mcpt.occlusion_fold_host(points, normals, rays, hit, t, fn, spp, MAXD, falloff)
    want = OR.fold(np.concatenate([points, normals], axis=1), rays, hit, t, fn, spp, MAXD, falloff)
    assert _same(got, want)
    assert np.all((got["ao"] >= 0.0) & (got["ao"] <= 1.0)) and np.all(got["back"] <= got["hits"]) and np.all(got["hits"] <= spp)
    # entry 0: every sample is closed, whatever the falloff (t = 0): ao is +0.0 and bent falls back to the hemisphere rule's n^, on bits
    assert _bits(got["ao"][:1])[0] == 0 and got["hits"][0] == spp
    assert np.array_equal(_bits(got["bent"][0]), _bits(OR.n_hat(normals[0])))
    if spp == 1:
        assert np.array_equal(_bits(got["stderr"]), np.zeros(n, dtype=np.uint64))       # exactly +0.0
    if n == 7:
        # entry 1: the open directions cancel exactly: the same fallback; entry 2: everything is open
        assert got["ao"][1] == (1.0 if spp % 2 == 0 else (spp - 1) / spp if spp > 1 else 0.0)
        assert np.array_equal(_bits(got["bent"][1]), _bits(OR.n_hat(normals[1])))
        assert got["ao"][2] == 1.0 and got["hits"][2] == 0 and got["back"][2] == 0 and got["stderr"][2] == 0.0
        # both sides of the faces are met, and the edge distances fall on the side the rule says
        if spp >= 63:
            assert 0 < got["back"].sum() < got["hits"].sum()
    near = (hit != 0) & (t < MAXD)
    assert np.array_equal(got["hits"], near.reshape(n, spp).sum(axis=1))


def test_edge_distances_fall_where_the_rule_says(mcpt):
    """one entry per distance, spp = 1: t == max_distance and beyond are open, anything under it is near"""
    n = len(EDGE_T)
    normals = np.tile([0.0, 0.0, 2.0], (n, 1))
    rays = np.tile([0.0, 0.0, 0.0, 0.0, 0.6, 0.8], (n, 1))
    t = np.array(EDGE_T)
    fn = np.tile([0.0, 0.0, -1.0], (n, 1))
    for falloff in FALLOFFS:
        got = mcpt.occlusion_fold_host(np.zeros((n, 3)), normals, rays, np.ones(n), t, fn, 1, MAXD, falloff)
        x = t / MAXD
        with np.errstate(over="ignore"):
            want_v = np.where(t < MAXD, {"hard": 0.0 * x, "linear": x, "square": x * x}[falloff], 1.0)
        assert np.array_equal(_bits(got["ao"]), _bits(want_v))
        assert got["hits"].tolist() == [int(v < MAXD) for v in t] and got["back"].tolist() == [0] * n
        assert np.array_equal(got["stderr"], np.zeros(n))
        # the face looks at the ray: flipped, every near hit is a back-face hit
        flipped = mcpt.occlusion_fold_host(np.zeros((n, 3)), normals, rays, np.ones(n), t, -fn, 1, MAXD, falloff)
        assert np.array_equal(flipped["back"], got["hits"])
        # a miss is open whatever its distance says
        miss = mcpt.occlusion_fold_host(np.zeros((n, 3)), normals, rays, np.zeros(n), t, fn, 1, MAXD, falloff)
        assert np.array_equal(miss["ao"], np.ones(n)) and not miss["hits"].any()
        assert np.array_equal(_bits(miss["bent"]), _bits(np.tile(np.array([0.0, 0.6, 0.8]) / np.sqrt((0.0 * 0.0 + 0.6 * 0.6) + 0.8 * 0.8), (n, 1))))


def test_a_permuted_list_gives_permuted_answers(mcpt):
    n, spp = 7, 65
    points, normals, rays, hit, t, fn = synthetic(n, spp, seed=3)
    perm = np.random.default_rng(1).permutation(n)
    idx = (perm[:, None] * spp + np.arange(spp)[None, :]).ravel()
    a = mcpt.occlusion_fold_host(points, normals, rays, hit, t, fn, spp, MAXD, "linear")
    b = mcpt.occlusion_fold_host(points[perm], normals[perm], rays[idx], hit[idx], t[idx], fn[idx], spp, MAXD, "linear")
    assert _same({k: v[perm] for k, v in a.items()}, b)


def test_the_library_and_the_restatement_against_hand_computations(mcpt):
    d = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    hit, t = np.array([1, 1, 0, 1]), np.array([0.5, 0.25, 0.1, 2.0])
    fn = np.array([[0.0, 0.0, 1.0], [0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    # the same hand values through mcpt_occlusion_fold_host
    rays, nrm = np.concatenate([np.zeros((4, 3)), d], axis=1), np.array([[0.0, 0.0, 3.0]])
    got = mcpt.occlusion_fold_host(np.zeros((1, 3)), nrm, rays, hit, t, fn, 4, 1.0, "linear")
    assert got["ao"][0] == 2.75 / 4 and (got["hits"][0], got["back"][0]) == (2, 1)
    assert got["stderr"][0] == np.sqrt(((2.3125 - 2.75 * 2.75 / 4) / 3) / 4)
    assert got["bent"][0].tolist() == (np.array([1.0, 0.25, 1.5]) / np.sqrt((1.0 + 0.0625) + 2.25)).tolist()
    got = mcpt.occlusion_fold_host(np.zeros((1, 3)), nrm, rays[:2], hit[:2], t[:2], fn[:2], 2, 1.0, "hard")
    assert (got["ao"][0], got["stderr"][0], got["hits"][0], got["back"][0]) == (0.0, 0.0, 2, 1) and got["bent"][0].tolist() == [0.0, 0.0, 1.0]
    assert mcpt.occlusion_fold_host(np.zeros((1, 3)), nrm, rays, hit, t, fn, 4, 1.0, "square")["ao"][0] == (0.25 + 0.0625 + 2.0) / 4
    ao, err, bent, hits, back = OR.fold_entry([0.0, 0.0, 3.0], d, hit, t, fn, 1.0, "linear")
    # v = 0.5, 0.25, 1, 1: s1 = 2.75, s2 = 2.3125, b = (1, 0.25, 1.5)
    assert ao == 2.75 / 4 and (hits, back) == (2, 1)
    assert err == np.sqrt(((2.3125 - 2.75 * 2.75 / 4) / 3) / 4)
    assert bent.tolist() == (np.array([1.0, 0.25, 1.5]) / np.sqrt((1.0 + 0.0625) + 2.25)).tolist()
    ao, err, bent, hits, back = OR.fold_entry([0.0, 0.0, 3.0], d[:2], hit[:2], t[:2], fn[:2], 1.0, "hard")
    assert (ao, err, hits, back) == (0.0, 0.0, 2, 1) and bent.tolist() == [0.0, 0.0, 1.0]
    assert OR.fold_entry([0.0, 0.0, 3.0], d, hit, t, fn, 1.0, "square")[0] == (0.25 + 0.0625 + 2.0) / 4
    # the dilation: one covered texel in a 3 x 4 map spreads a ring a round
    ao_map, owner = np.zeros((3, 4)), np.full((3, 4), -1)
    ao_map[1, 1], owner[1, 1] = 0.5, 7
    a1, o1 = OR.dilate(ao_map, owner, 1)
    assert o1.tolist() == [[-2, -2, -2, -1], [-2, 7, -2, -1], [-2, -2, -2, -1]] and a1[:, :3].tolist() == [[0.5] * 3] * 3 and not a1[:, 3].any()
    a2, o2 = OR.dilate(ao_map, owner, 2)
    assert o2[:, 3].tolist() == [-3, -3, -3] and a2[:, 3].tolist() == [0.5, 0.5, 0.5] and np.array_equal(o2[:, :3], o1[:, :3])


# ---- refusals

def _op(mcpt, spp=4, sample_base=0, seed=1, falloff=0, flags=0, max_distance=1.0, workspace_rays=0, reserved=(0, 0)):
    return mcpt.OcclusionParams(spp, sample_base, seed, falloff, flags, max_distance, workspace_rays, (C.c_int32 * 2)(*reserved))


def _om(mcpt, width=8, height=4, dilate=0, reserved=0):
    return mcpt.OcclusionMap(width, height, dilate, reserved)


def _ptr(a, t=PD):
    return a.ctypes.data_as(t) if a is not None else None


def _addr(a):
    return a.ctypes.data if a is not None else None


def _queries(L, op, q6, n, ao, ids=None, fold=None):
    """the two query forms with a null device (the device form's pointers are not looked at) and the host fold"""
    opp = C.byref(op) if op is not None else None
    rays, hit, t, fn = fold if fold is not None else (None, None, None, None)
    return [L.mcpt_query_occlusion(None, _ptr(q6), _ptr(ids, P32), n, opp, _ptr(ao), None, None, None, None, None),
            L.mcpt_query_occlusion_device(None, _addr(q6), _addr(ids), n, opp, _addr(ao), None, None, None, None, None, None),
            L.mcpt_occlusion_fold_host(_ptr(q6), _ptr(rays), _ptr(hit, P32), _ptr(t), _ptr(fn), n, opp, _ptr(ao), None, None, None, None)]


def _host(L, op, q6, n, ao, ids=None):
    return L.mcpt_query_occlusion(None, _ptr(q6), _ptr(ids, P32), n, C.byref(op), _ptr(ao), None, None, None, None, None)


def _maps(L, om, op, ao):
    omp, opp = C.byref(om) if om is not None else None, C.byref(op) if op is not None else None
    return [L.mcpt_bake_occlusion_lightmap(None, None, omp, opp, _ptr(ao), None, None, None, None, None, None),
            L.mcpt_bake_occlusion_lightmap_device(None, None, omp, opp, _addr(ao), None, None, None, None, None, None, None)]


# the parameters' refusals in the header's order: each entry is refused with a message of its own, and wins over everything after it
ORDER = [("spp must", dict(spp=0)), ("sample_base must", dict(sample_base=-1)), ("sample_base + spp", dict(spp=2, sample_base=INT_MAX - 1)),
         ("falloff", dict(falloff=3)), ("flags", dict(flags=1)), ("max_distance", dict(max_distance=0.0)), ("workspace_rays", dict(workspace_rays=-1)),
         ("reserved", dict(reserved=(0, 1)))]
BAD = [dict(spp=-3), dict(falloff=-1), dict(falloff=2 ** 20), dict(flags=-1), dict(flags=2), dict(max_distance=NAN), dict(max_distance=INF),
       dict(max_distance=-1.0), dict(workspace_rays=-2 ** 40), dict(reserved=(3, 0))]
MAP_ORDER = [("width and height", dict(width=0)), ("dilate", dict(dilate=65)), ("reserved", dict(reserved=1))]
BAD_MAP = [dict(width=16385), dict(height=0), dict(height=-1), dict(height=16385), dict(dilate=-1), dict(reserved=-1)]


def test_query_refusals_come_in_order_and_before_the_missing_device(mcpt):
    L = mcpt.lib()
    nd = _null_device_rc(mcpt)
    q6, ao = np.tile([0.1, 0.2, 0.3, 0.0, 0.0, 1.0], (8, 1)), np.zeros(8)
    fold = (np.zeros((32, 6)), np.zeros(32, dtype=np.int32), np.zeros(32), np.zeros((32, 3)))
    assert _queries(L, None, q6, 8, ao, fold=fold) == [ERR_ARG] * 3 and "null occlusion parameters" in _message(mcpt)
    for i, (word, kw) in enumerate(ORDER):
        merged = {}
        for _, later in reversed(ORDER[i:]):
            merged.update(later)
        merged.update(kw)
        assert _queries(L, _op(mcpt, **merged), None, -1, None) == [ERR_ARG] * 3 and word in _message(mcpt), (word, _message(mcpt))
    for kw in BAD:
        assert _queries(L, _op(mcpt, **kw), q6, 8, ao, fold=fold) == [ERR_ARG] * 3, kw
    # then the count, then the two required arrays
    for n in (-1, 2 ** 31, 2 ** 40):
        assert _queries(L, _op(mcpt), None, n, None) == [ERR_ARG] * 3 and "entries" in _message(mcpt)
    assert _queries(L, _op(mcpt), None, 8, ao, fold=fold) == [ERR_ARG] * 3 and "null" in _message(mcpt)
    assert _queries(L, _op(mcpt), q6, 8, None, fold=fold) == [ERR_ARG] * 3 and "null" in _message(mcpt)
    # the host-pointer form looks at the list, as the hemisphere kind does; the device form does not
    ids = np.arange(8, dtype=np.int32)
    ids[3] = -1
    assert _host(L, _op(mcpt), q6, 8, ao, ids) == ERR_ARG and "query 3" in _message(mcpt)
    assert _queries(L, _op(mcpt), q6, 8, ao, ids)[1] == nd
    for col, v in ((1, NAN), (4, INF), (0, -INF)):
        q2 = q6.copy()
        q2[5, col] = v
        assert _host(L, _op(mcpt), q2, 8, ao) == ERR_ARG and "query 5" in _message(mcpt)
        assert _queries(L, _op(mcpt), q2, 8, ao)[1] == nd
    q2 = q6.copy()
    q2[2, 3:] = 0.0
    assert _host(L, _op(mcpt), q2, 8, ao) == ERR_ARG and "normal" in _message(mcpt)
    # the host fold wants its four arrays
    for drop in range(4):
        f = list(fold)
        f[drop] = None
        assert _queries(L, _op(mcpt), q6, 8, ao, fold=f)[2] == ERR_ARG and "null" in _message(mcpt)
    # valid arguments: the fold answers, the queries miss the device; the limits themselves pass
    assert _queries(L, _op(mcpt), q6, 8, ao, fold=fold) == [nd, nd, 0]
    one = (np.zeros((8, 6)), np.zeros(8, dtype=np.int32), np.zeros(8), np.zeros((8, 3)))
    assert _queries(L, _op(mcpt, spp=1, sample_base=INT_MAX - 1, falloff=2, max_distance=1e-300, workspace_rays=2 ** 62), q6, 8, ao, fold=one) == [nd, nd, 0]
    if nd == ERR_NO_DEVICE:
        assert _host(L, _op(mcpt), q6, 8, ao) == nd and "device" in _message(mcpt).lower()
    # n == 0 needs no arrays: the fold is done, the queries still miss the device first
    assert _queries(L, _op(mcpt), None, 0, None) == [nd, nd, 0]
    got = mcpt.occlusion_fold_host(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 6)), np.zeros(0), np.zeros(0), np.zeros((0, 3)), 4, 1.0)
    assert got["ao"].shape == (0,) and got["bent"].shape == (0, 3)


def test_map_refusals_come_in_order_and_before_the_missing_device(mcpt):
    L = mcpt.lib()
    nd = _null_device_rc(mcpt)
    ao = np.zeros((4, 8))
    assert _maps(L, None, _op(mcpt), ao) == [ERR_ARG] * 2 and "null occlusion map" in _message(mcpt)
    # the map's own fields, in order, before NULL parameters and before the parameters' errors
    for i, (word, kw) in enumerate(MAP_ORDER):
        merged = {}
        for _, later in reversed(MAP_ORDER[i:]):
            merged.update(later)
        merged.update(kw)
        assert _maps(L, _om(mcpt, **merged), None, None) == [ERR_ARG] * 2 and word in _message(mcpt), (word, _message(mcpt))
    for kw in BAD_MAP:
        assert _maps(L, _om(mcpt, **kw), _op(mcpt), ao) == [ERR_ARG] * 2, kw
    assert _maps(L, _om(mcpt), None, ao) == [ERR_ARG] * 2 and "null occlusion parameters" in _message(mcpt)
    for i, (word, kw) in enumerate(ORDER):
        merged = {}
        for _, later in reversed(ORDER[i:]):
            merged.update(later)
        merged.update(kw)
        assert _maps(L, _om(mcpt), _op(mcpt, **merged), None) == [ERR_ARG] * 2 and word in _message(mcpt), (word, _message(mcpt))
    for kw in BAD:
        assert _maps(L, _om(mcpt), _op(mcpt, **kw), ao) == [ERR_ARG] * 2, kw
    assert _maps(L, _om(mcpt), _op(mcpt), None) == [ERR_ARG] * 2 and "null occlusion map array" in _message(mcpt)
    assert _maps(L, _om(mcpt), _op(mcpt), ao) == [nd] * 2
    assert _maps(L, _om(mcpt, width=16384, height=1, dilate=64), _op(mcpt), np.zeros(16384)) == [nd] * 2


def test_api_validates_its_arguments(mcpt):
    p, nr = np.zeros((2, 3)), np.tile([0.0, 0.0, 1.0], (2, 1))
    rays, hit, t, fn = np.zeros((8, 6)), np.zeros(8), np.zeros(8), np.zeros((8, 3))
    with pytest.raises(ValueError):
        mcpt.occlusion_fold_host(p, nr[:1], rays, hit, t, fn, 4, 1.0)
    with pytest.raises(ValueError):
        mcpt.occlusion_fold_host(p, nr, rays[:7], hit, t, fn, 4, 1.0)
    with pytest.raises(ValueError):
        mcpt.occlusion_fold_host(p, nr, rays, hit, t, fn, 4, 1.0, falloff="cubic")
    with pytest.raises(ValueError):
        mcpt.occlusion_fold_host(p, nr, rays, hit, t, fn, 4.0, 1.0)
    with pytest.raises(mcpt.McptError):
        mcpt.occlusion_fold_host(p, nr, rays, hit, t, fn, 4, -1.0)
    with pytest.raises(mcpt.McptError):
        mcpt.occlusion_fold_host(p, nr, rays, hit, t, fn, 4, 1.0, falloff=3)
    assert mcpt.occlusion_fold_host(p, nr, rays, hit, t, fn, 4, 1.0, falloff=mcpt.OCCLUSION_SQUARE)["ao"].tolist() == [1.0, 1.0]


# ---- occlusion.hpp under the sanitizers

def test_fold_under_address_and_undefined_sanitizers(tmp_path):
    """A stand-alone program, not the library: nothing loaded into this process is instrumented."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "occlusion_sanitize")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "occlusion_sanitize_main.cpp")])
    edge = [NAN, INF, -INF, 1e300, -1e300, 1e-300, 0.0, -0.0, 0.5]
    vecs = [[0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [NAN, 0.0, 1.0], [INF, 0.0, 1.0], [1e300, -1e300, 1e300], [1e-300, 0.0, 0.0], [0.0, 0.6, 0.8]]
    cases = []
    for falloff in (0, 1, 2):
        for md in (0.75, 1e300, 1e-300, INF, NAN, 0.0):
            for t in edge:
                for hit in (0, 1):
                    cases.append((falloff, md, vecs[6], vecs[6], t, hit, vecs[6]))
        for nrm in vecs:
            for d in vecs:
                for f in (vecs[0], vecs[2], vecs[4], vecs[6]):
                    cases.append((falloff, 0.75, nrm, d, 0.5, 1, f))
                cases.append((falloff, 0.75, nrm, d, 0.5, 0, vecs[6]))
    text = "".join("%d %r %r %r %r %r %r %r %r %d %r %r %r\n" % (c[0], c[1], *c[2], *c[3], c[4], c[5], *c[6]) for c in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases)
    bad = 0
    for c, line in zip(cases, lines):
        w = line.split()
        got = np.array([float.fromhex(x) for x in w[:5]])
        d = np.array([c[3], [-x for x in c[3]], c[3]], dtype=np.float64)
        t = np.array([c[4], c[4], c[4] / 2.0])
        ao, err, bent, hits, back = OR.fold_entry(c[2], d, np.full(3, c[5]), t, np.tile(np.array(c[6], dtype=np.float64), (3, 1)), c[1], c[0])
        want = np.array([ao, err, *bent])
        same = np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(_bits(got)[~np.isnan(got)], _bits(want)[~np.isnan(want)])
        bad += not (same and (int(w[5]), int(w[6])) == (hits, back))
    assert bad == 0
