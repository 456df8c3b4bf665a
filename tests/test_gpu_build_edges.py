"""GPU-built culling hierarchies (MCPT_BUILD_DEVICE_FAST: build_kernels.hip device_build_fast, MCPT_BUILD_DEVICE_SAH:
device_build_ploc, and the host-built one over the device's Morton order, MCPT_BUILD_DEVICE) at edge shapes and with every build
knob off its default.  Each case checks, per builder:
- the reference tree (BUILD_DEVICE) against the host build and the oracle, bit for bit;
- the structure of the hierarchy the fast walk walks (Device.fast_hierarchy) with the exact checker of tests/fast_bvh_ref.py, and
  that the fast walk is on (a comparison of "fast" against "reference" would otherwise compare the reference walk with itself);
- ray answers: the fast walk against the reference walk on the same device (face, t, p, pn bit for bit) and against the oracle, on
  make_rays() plus one ray from outside the scene at an interior point of every triangle (and grazing rays in a flat scene's plane);
- a second device built the same way holds the same node bytes;
- the frame equals the host-built device's, bit for bit."""
import os
import zlib

import numpy as np
import pytest

from conftest import SCENES, make_rays
import fast_bvh_ref as R

pytestmark = pytest.mark.gpu

W, H = 40, 30
BUILDS = ("device", "fast", "sah")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _mode(M, build):
    return {"host": M.BUILD_HOST, "device": M.BUILD_DEVICE, "fast": M.BUILD_DEVICE_FAST, "sah": M.BUILD_DEVICE_SAH}[build]


# ------------------------------------------------------------------------------------------------------------------ geometries
def _rand_tris(rng, n, lo=-1.0, hi=1.0, size=0.4):
    c = rng.uniform(lo, hi, size=(n, 1, 3))
    return (c + rng.normal(scale=size, size=(n, 3, 3))).reshape(n, 9)


def _grid(n=64, size=4.0):
    """n x n quads in the plane y = 0 (2 n^2 triangles of equal area)"""
    s = np.linspace(-size / 2, size / 2, n + 1)
    x0, z0 = np.meshgrid(s[:-1], s[:-1], indexing="ij")
    x1, z1 = x0 + size / n, z0 + size / n
    x0, z0, x1, z1 = (q.reshape(-1) for q in (x0, z0, x1, z1))
    y = np.zeros_like(x0)
    a = np.stack([x0, y, z0, x1, y, z1, x1, y, z0], axis=1)
    b = np.stack([x0, y, z0, x0, y, z1, x1, y, z1], axis=1)
    return np.vstack([a, b])


def _lamp(v, flat=False):
    """two lamp triangles above the geometry's box (in its plane when flat), facing down"""
    p = v.reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    c, s = 0.5 * (lo + hi), max(float((hi - lo).max()), 1e-300)
    y = lo[1] if flat else hi[1] + 0.2 * s
    x0, x1, z0, z1 = c[0] - 0.25 * s, c[0] + 0.25 * s, c[2] - 0.25 * s, c[2] + 0.25 * s
    return np.array([[x0, y, z0, x1, y, z0, x1, y, z1], [x0, y, z0, x1, y, z1, x0, y, z1]])


def _scene(v, lamp_rows):
    """synthetic.write_obj's dict: faces v [n,9] (lamp_rows of them are the lamp), camera framing the box"""
    v = np.ascontiguousarray(v, dtype=np.float64)
    n = v.shape[0]
    e1, e2 = v[:, 3:6] - v[:, 0:3], v[:, 6:9] - v[:, 0:3]
    nrm = np.cross(e1, e2)
    ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(ln > 0, nrm / np.where(ln > 0, ln, 1.0), np.array([0.0, 1.0, 0.0]))
    mat = np.zeros(n, dtype=np.int32)
    mat[lamp_rows] = 1
    p = v.reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    c, s = 0.5 * (lo + hi), float((hi - lo).max())
    rec = np.array([[0.6, 0.5, 0.4, 0, 0, 0, 1, 1], [0, 0, 0, 0, 0, 0, 1, 1]], dtype=np.float64)
    return dict(v=v, vn=np.tile(nrm, 3), material=mat, material_rec=rec, material_names=["grey", "lamp"],
                light_material=np.array([1], dtype=np.int32), light_radiance=np.full((1, 3), 12.0),
                eye=list(c + s * np.array([0.35, 1.1, 1.9])), look_at=list(c), up=[0.0, 1.0, 0.0], fovy=50.0, width=W, height=H)


def _with_lamp(v, flat=False):
    lamp = _lamp(v, flat)
    return _scene(np.vstack([v, lamp]), np.arange(v.shape[0], v.shape[0] + 2))


def _tiny(n):
    # n triangles in all, the first one the lamp
    return _scene(_rand_tris(np.random.default_rng(100 + n), n), [0])


def _random(n):
    # n triangles in all: n - 2 random ones, a lamp quad
    return _with_lamp(_rand_tris(np.random.default_rng(200 + n), n - 2, size=0.15))


def _flat():
    # every triangle, the lamp too, in the plane y = 0.25: the scene box has no extent in y (Morton domain inv = 0, e = -126)
    rng = np.random.default_rng(7)
    v = _rand_tris(rng, 2000, size=0.1)
    v[:, 1::3] = 0.25
    return _with_lamp(v, flat=True)


def _duplicates():
    # 512 exact copies each of two triangles: equal Morton keys, tied PLOC areas, rays that tie in t
    two = np.array([[-1, 0, -1, 1, 0, -1, 0, 0.5, 1], [-1, 0.2, 1, 1, 0.2, 1, 0, 0.9, -1]], dtype=np.float64)
    return _with_lamp(np.repeat(two, 512, axis=0))


def _wall_and_dust():
    # one triangle spanning the box (PLOC's max_area rule keeps it on its own: the single-leaf-cluster branch), 5000 specks
    rng = np.random.default_rng(9)
    dust = _rand_tris(rng, 5000, size=0.004)
    wall = np.array([[-1.5, -1.5, -1.2, 3.0, -1.5, -1.2, -1.5, 3.0, 1.4]])
    return _with_lamp(np.vstack([wall, dust]))


def _scaled(scale, offset):
    g = _grid() * scale
    g = (g.reshape(-1, 3) + np.asarray(offset)).reshape(-1, 9)
    return _with_lamp(g)


def _zero_area():
    rng = np.random.default_rng(11)
    v = _rand_tris(rng, 600, size=0.2)
    v[::10, 3:6] = v[::10, 0:3]                                   # two equal vertices
    v[5::10, 6:9] = 0.5 * (v[5::10, 0:3] + v[5::10, 3:6])         # collinear (exactly: the midpoint of a power-of-two scaled sum)
    return _with_lamp(v)


GEOMETRIES = {
    **{"tiny%d" % n: (lambda n=n: _tiny(n)) for n in (1, 2, 3, 4, 5)},
    **{"random%d" % n: (lambda n=n: _random(n)) for n in (63, 64, 65, 255, 256, 257, 1025)},
    "flat": _flat,
    "duplicates": _duplicates,
    "grid64": lambda: _with_lamp(_grid()),
    "wall_and_dust": _wall_and_dust,
    "grid_1e-12": lambda: _scaled(1e-12, (0.0, 0.0, 0.0)),
    "grid_1e12_negative": lambda: _scaled(1e12, (-3e12, -1e12, -5e12)),           # every coordinate negative
    "grid_mm_at_1e6": lambda: _scaled(1e-3 / (4.0 / 64), (1e6, -1e6 + 0.3, 2e6)),  # 1 mm cells, origins rounded down to fp32
    "zero_area": _zero_area,
}
# The fast walk is on for every case (mcpt_device_create's gate: coordinates within [1e-150, 1e150], the largest within
# [1e-15, 1e15], stack need and depth below kFastMaxDepth): the scaled grids are chosen inside that window.
FAST_OFF = {}


# ---------------------------------------------------------------------------------------------------------------------- rays
def _tri_rays(v, rng, box_lo, box_hi):
    """one ray per non-degenerate triangle: from outside the box at a strictly interior barycentric point"""
    v = v.reshape(-1, 3, 3)
    area = np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)
    v = v[area > 0]
    b = rng.uniform(0.1, 1.0, size=(v.shape[0], 3))
    b /= b.sum(axis=1, keepdims=True)
    p = (b[:, :, None] * v).sum(axis=1)
    u = rng.normal(size=p.shape)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    diag = max(float(np.linalg.norm(box_hi - box_lo)), 1e-300)
    return np.hstack([p + 2.0 * diag * u, -u])


def _grazing_rays(v, rng, n, y):
    """rays in the plane y (d.y = 0) from outside the box towards points of the triangles, plus a few just above and below it"""
    p = v.reshape(-1, 3)
    lo, hi = p.min(0), p.max(0)
    tgt = v.reshape(-1, 3, 3).mean(axis=1)[rng.integers(0, v.shape[0], size=n)]
    ang = rng.uniform(0, 2 * np.pi, size=n)
    u = np.stack([np.cos(ang), np.zeros(n), np.sin(ang)], axis=1)
    o = tgt + 2.0 * float(np.linalg.norm(hi - lo)) * u
    o[:, 1] = y
    o[::3, 1] = np.nextafter(y, np.inf)
    o[1::3, 1] = np.nextafter(y, -np.inf)
    return np.hstack([o, -u])


# ---------------------------------------------------------------------------------------------------------------------- checks
def _check_structure(M, dev, scene, expect_builder, why_off=None):
    info, nodes, faces = dev.fast_hierarchy()
    assert info.n_nodes == nodes.shape[0] and info.n_tris == scene.info.num_faces
    assert info.builder in expect_builder, (info.builder, expect_builder)
    if why_off:
        assert info.enabled == 0, why_off
    else:
        assert info.enabled == 1, "fast walk off: need %d, depth %d" % (info.cw_stack_need, info.max_depth)
    lo, hi = R.face_boxes(scene.faces()[0])
    fig = R.check_hierarchy(nodes, faces, lo, hi, stack_need=info.cw_stack_need)
    return info, nodes, faces, fig


def _trace_both(M, dev, rays):
    st = M.Stats()
    fast = dev.ray_intersect(rays, stats=st)
    dev.set_trace_mode(M.TRACE_REFERENCE)
    ref = dev.ray_intersect(rays)
    dev.set_trace_mode(M.TRACE_FAST)
    f0, t0, p0, n0 = fast
    f1, t1, p1, n1 = ref
    assert np.array_equal(f0, f1), "%d of %d rays: other face" % (int((f0 != f1).sum()), f0.size)
    h = f0 >= 0
    assert np.array_equal(_bits(t0[h]), _bits(t1[h])) and np.array_equal(_bits(p0[h]), _bits(p1[h])) and np.array_equal(_bits(n0[h]), _bits(n1[h]))
    return fast, st


def _check_oracle(fast, want):
    gf, gt, gp, _ = fast
    of, ot, op, _ = want
    assert np.array_equal(gf, of), "%d of %d rays: other face than the oracle" % (int((gf != of).sum()), gf.size)
    h = of >= 0
    assert np.array_equal(_bits(gt[h]), _bits(ot[h])) and np.array_equal(_bits(gp[h]), _bits(op[h]))


def _expect(M, build):
    return {"device": (M.FAST_BUILT_HOST,), "fast": (M.FAST_BUILT_DEVICE_FAST,),
            "sah": (M.FAST_BUILT_DEVICE_PLOC, M.FAST_BUILT_PLOC_FELL_BACK)}[build]


@pytest.mark.parametrize("case", list(GEOMETRIES))
def test_edge_geometry(mcpt, oracle, tmp_path, case):
    from montecarlopathtracing_amd import synthetic
    M = mcpt
    g = GEOMETRIES[case]()
    d = str(tmp_path) + os.sep
    synthetic.write_obj(g, d, "e")
    sc = M.Scene(d, "e")
    arr = M.Scene.from_arrays(g["v"], g["vn"], g["material"], g["material_rec"], g["light_material"], g["light_radiance"], g["eye"],
                              g["look_at"], g["up"], g["fovy"], g["width"], g["height"], material_names=g["material_names"], defer_build=True)
    gf, gm, _ = sc.faces()
    af, am, _ = arr.faces()
    assert np.array_equal(_bits(gf[:, :18]), _bits(af[:, :18])) and np.array_equal(gm, am), "the .obj and the arrays are one scene"
    osc = oracle.OracleScene(d + "e", texture_dir=d)
    rng = np.random.default_rng(zlib.crc32(case.encode()))
    box, _, _ = osc.bvh_nodes()
    rays = [make_rays(osc, 3000, seed=17), _tri_rays(g["v"], rng, box[0, 3:], box[0, :3])]
    if case == "flat":
        rays.append(_grazing_rays(g["v"], rng, 2000, float(g["v"][0, 1])))
    rays = np.ascontiguousarray(np.vstack(rays))
    want = osc.trace_closest(rays)
    hb, hl = sc.bvh_nodes()[0], sc.leaf_order()
    obox, _, _ = osc.bvh_nodes()
    assert np.array_equal(hl, osc.leaf_order()) and np.array_equal(_bits(hb), _bits(obox))
    host = M.Device(sc, 0, build=M.BUILD_HOST)
    _check_structure(M, host, sc, (M.FAST_BUILT_HOST,), FAST_OFF.get(case))
    frame = host.generateImg(4, seed=3)
    assert frame.sum() > 0
    _check_oracle(_trace_both(M, host, rays)[0], want)
    host.close()
    for build in BUILDS:
        dev = M.Device(sc, 0, build=_mode(M, build))
        if build == "device":                               # the reference tree built on the GPU, down to one triangle
            db, _ = dev.bvh_nodes()
            assert np.array_equal(dev.leaf_order(), hl) and np.array_equal(_bits(db), _bits(hb))
        info, nodes, faces, fig = _check_structure(M, dev, sc, _expect(M, build), FAST_OFF.get(case))
        fast, st = _trace_both(M, dev, rays)
        _check_oracle(fast, want)
        assert np.array_equal(_bits(dev.generateImg(4, seed=3)), _bits(frame))
        dev.close()
        again = M.Device(sc, 0, build=_mode(M, build))
        i2, n2, f2 = again.fast_hierarchy()
        again.close()
        assert np.array_equal(n2, nodes) and np.array_equal(f2, faces), "a second build of the same scene differs"
        # the same scene given as arrays, with no host build at all: the same hierarchy, the same frame
        dd = M.Device(arr, 0, build=_mode(M, build))
        i3, n3, f3 = dd.fast_hierarchy()
        assert np.array_equal(n3, nodes) and np.array_equal(f3, faces)
        if build == "device":
            assert np.array_equal(_bits(dd.generateImg(4, seed=3)), _bits(frame))
        dd.close()
    osc.close()


# ------------------------------------------------------------------------------------------------------------------ knob sweep
KNOBS = ([("MCPT_CLUSTER_LEAF", v, "fast") for v in (1, 2, 3, 5, 8)] +
         [("MCPT_CLUSTER_LEVELS", v, "fast") for v in (1, 2, 5)] +
         [("MCPT_PLOC_CLUSTER", v, "sah") for v in (4, 64, 65536)] +
         [("MCPT_PLOC_RADIUS", v, "sah") for v in (1, 64)] +
         [("MCPT_PLOC_LEAF", v, "sah") for v in (1, 8)] +
         [("MCPT_PLOC_HEIGHT", v, "sah") for v in (3, 24)] +
         [("MCPT_PLOC_BUDGET", v, "sah") for v in (3, 30)] +
         [("MCPT_PLOC_AREA", 0, "sah")] +
         [("MCPT_PLOC_CT", v, "sah") for v in (0.05, 20)] +
         [("MCPT_PLOC_CL", v, "sah") for v in (-0.5, 20)])
_BASE = {}


def _knob_scene(M, oracle, name):
    """(scene, rays, host frame, host ray answers) of a knob-sweep scene, once per session"""
    if name not in _BASE:
        from montecarlopathtracing_amd import synthetic
        rng = np.random.default_rng(23)
        if name == "cornell-box":
            sc = M.Scene(SCENES, name, width=96, height=54)
            osc = oracle.OracleScene(SCENES + name, texture_dir=SCENES, width=96, height=54)
            box, _, _ = osc.bvh_nodes()
            v = sc.faces()[0][:, :9]
            rays = np.vstack([make_rays(osc, 6000, seed=29), _tri_rays(v, rng, box[0, 3:], box[0, :3])])
            osc.close()
        else:
            g = synthetic.generate(20000, width=96, height=54)
            sc = M.Scene.from_arrays(g["v"], g["vn"], g["material"], g["material_rec"], g["light_material"], g["light_radiance"], g["eye"],
                                     g["look_at"], g["up"], g["fovy"], g["width"], g["height"])
            p = g["v"].reshape(-1, 3)
            lo, hi = p.min(0), p.max(0)
            o = lo + (hi - lo) * rng.random((6000, 3))
            dd = rng.normal(size=(6000, 3))
            dd[::7, 1] = 0.0
            rays = np.vstack([np.hstack([o, dd / np.linalg.norm(dd, axis=1, keepdims=True)]), _tri_rays(g["v"], rng, lo, hi)])
        rays = np.ascontiguousarray(rays)
        host = M.Device(sc, 0, build=M.BUILD_HOST)
        frame = host.generateImg(4, seed=3)
        want = host.ray_intersect(rays)
        host.close()
        _BASE[name] = (sc, rays, frame, want)
    return _BASE[name]


def _build_and_check(M, sc, rays, frame, want, build):
    dev = M.Device(sc, 0, build=_mode(M, build))
    info, nodes, faces, fig = _check_structure(M, dev, sc, _expect(M, build))
    fast, st = _trace_both(M, dev, rays)
    _check_oracle(fast, want)
    assert np.array_equal(_bits(dev.generateImg(4, seed=3)), _bits(frame))
    dev.close()
    again = M.Device(sc, 0, build=_mode(M, build))
    _, n2, f2 = again.fast_hierarchy()
    again.close()
    assert np.array_equal(n2, nodes) and np.array_equal(f2, faces), "a second build of the same scene differs"
    return info, fig


@pytest.mark.parametrize("name", ["cornell-box", "synthetic20k"])
@pytest.mark.parametrize("knob,value,build", KNOBS, ids=["%s=%s" % (k, v) for k, v, _ in KNOBS])
def test_build_knob(mcpt, oracle, monkeypatch, name, knob, value, build):
    """one knob off its default (read at device creation); the ray answers are the host-built device's, which the oracle pins"""
    sc, rays, frame, want = _knob_scene(mcpt, oracle, name)
    monkeypatch.setenv(knob, str(value))
    info, fig = _build_and_check(mcpt, sc, rays, frame, want, build)
    if knob == "MCPT_CLUSTER_LEAF":
        # leaves of up to `value` triangles from Morton groups
        assert fig["leaves"] <= sc.info.num_faces
    if build == "sah" and knob not in ("MCPT_PLOC_CLUSTER", "MCPT_PLOC_BUDGET"):
        assert info.builder == mcpt.FAST_BUILT_DEVICE_PLOC
    if (knob, value) == ("MCPT_PLOC_BUDGET", 30):
        # a budget of 30 leaves room for the tree above only over at most 8 clusters (budget + levels above + 2 <= 35): both
        # scenes leave more, so the device takes the Morton builder
        assert info.builder == mcpt.FAST_BUILT_PLOC_FELL_BACK


@pytest.mark.parametrize("name", ["synthetic20k"])
def test_ploc_falls_back_to_the_morton_builder(mcpt, oracle, monkeypatch, name):
    """clusters of at most four triangles with a stack budget of 30 leave no room for the tree over the ~5000 clusters
    (device_build_ploc returns hipErrorNotSupported): the device takes device_build_fast, reports it, and answers the same"""
    sc, rays, frame, want = _knob_scene(mcpt, oracle, name)
    monkeypatch.setenv("MCPT_PLOC_CLUSTER", "4")
    monkeypatch.setenv("MCPT_PLOC_BUDGET", "30")
    info, fig = _build_and_check(mcpt, sc, rays, frame, want, "sah")
    assert info.builder == mcpt.FAST_BUILT_PLOC_FELL_BACK and info.clusters == 0


def test_ploc_reports_its_clusters(mcpt, oracle):
    sc, rays, frame, want = _knob_scene(mcpt, oracle, "synthetic20k")
    dev = mcpt.Device(sc, 0, build=mcpt.BUILD_DEVICE_SAH)
    info, _, _ = dev.fast_hierarchy()
    dev.close()
    assert info.builder == mcpt.FAST_BUILT_DEVICE_PLOC and 1 < info.clusters < sc.info.num_faces


# ------------------------------------------------------------------------------------------------------------------ positive control
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_host_built_hierarchy_passes_the_checker(mcpt, name):
    """the accessor and the checker on the host's own builder, which mcpt_scene_fast_bvh_stats checks independently: the same
    triangle order, the same depth, nesting_ok"""
    sc = mcpt.Scene(SCENES, name, width=96, height=54)
    n_bin, depth, stats_order, nesting_ok = sc.fast_bvh_stats()
    assert nesting_ok
    dev = mcpt.Device(sc, 0, build=mcpt.BUILD_HOST)
    info, nodes, faces, fig = _check_structure(mcpt, dev, sc, (mcpt.FAST_BUILT_HOST,))
    dev.close()
    assert np.array_equal(faces, sc.leaf_order()[stats_order])
    assert info.max_depth == depth and info.clusters == 0
    assert 0 < info.n_nodes <= n_bin                   # a 4-wide collapse of the binary tree
