"""Geometry updates without a GPU: the numpy refit (tests/refit_ref.py) against the hierarchy checker on hierarchies made in numpy, and
the C ABI's new entry points as far as they go without a device."""
import ctypes as C
import os

import numpy as np
import pytest

import fast_bvh_ref as F
import refit_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mcpt_device_update_vertices", "mcpt_device_update_vertices_device", "mcpt_device_get_vertices", "mcpt_device_set_camera",
       "mcpt_device_get_camera", "mcpt_multi_update_vertices", "mcpt_multi_set_camera"]


def _triangles(n, seed, spread=3.0):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.0, spread, size=(n, 1, 3))
    v = c + rng.normal(scale=0.05, size=(n, 3, 3))
    v = v[np.argsort(v[:, :, 0].mean(axis=1))]            # some locality for the leaves
    return v


def _boxes(v):
    return v.min(axis=1), v.max(axis=1)


@pytest.mark.parametrize("n,per_leaf,seed", [(1, 4, 1), (5, 1, 2), (97, 4, 3), (400, 8, 4), (1000, 3, 5)])
def test_refit_follows_the_geometry(n, per_leaf, seed):
    v = _triangles(n, seed)
    lo, hi = _boxes(v)
    nodes = R.build(lo, hi, per_leaf)
    faces = np.arange(n)
    F.check_hierarchy(nodes, faces, lo, hi)
    rng = np.random.default_rng(seed + 100)
    moved = v + rng.normal(scale=0.4, size=(n, 1, 3)) + 0.7
    mlo, mhi = _boxes(moved)
    with pytest.raises(F.HierarchyError):                  # the checker sees the stale boxes
        F.check_hierarchy(nodes, faces, mlo, mhi)
    refitted, blo, bhi = R.refit(nodes, mlo, mhi)
    F.check_hierarchy(refitted, faces, mlo, mhi)
    a, b = F.decode(nodes), F.decode(refitted)
    assert np.array_equal(a["child"], b["child"]) and np.array_equal(a["nchild"], b["nchild"])
    assert np.array_equal(blo[0], mlo.min(axis=0)) and np.array_equal(bhi[0], mhi.max(axis=0))
    assert R.cost(refitted) > 0


@pytest.mark.parametrize("n,per_leaf,seed", [(97, 4, 3), (400, 8, 4), (1000, 3, 5)])
def test_identity_and_round_trip(n, per_leaf, seed):
    v = _triangles(n, seed)
    lo, hi = _boxes(v)
    nodes = R.build(lo, hi, per_leaf)
    same, _, _ = R.refit(nodes, lo, hi)
    # the builder's exponent (from log2) is the smallest one on all of these inputs: an identity refit leaves the bytes as they were
    assert np.array_equal(same, nodes)
    moved = v * 1.7 - 0.3
    mlo, mhi = _boxes(moved)
    b, _, _ = R.refit(nodes, mlo, mhi)
    assert not np.array_equal(b, nodes)
    back, _, _ = R.refit(b, lo, hi)
    assert np.array_equal(back, nodes)


def test_exponent_is_minimal():
    """one exponent lower never fits: the first check of the rule, p + 255 * 2^(e-1) >= hi, fails"""
    rng = np.random.default_rng(9)
    for _ in range(2000):
        lo = float(rng.normal()) * 10.0 ** rng.integers(-6, 6)
        ext = float(abs(rng.normal())) * 10.0 ** rng.integers(-9, 6)
        pf, e, ql, qh = R.quantise_min([lo, lo + 0.3 * ext], [lo + 0.5 * ext, lo + ext])
        p = float(pf)
        assert p <= lo and p + 255.0 * np.ldexp(1.0, e) >= lo + ext
        assert e == -126 or p + 255.0 * np.ldexp(1.0, e - 1) < lo + ext
        ref = F.quantise([lo, lo + 0.3 * ext], [lo + 0.5 * ext, lo + ext])
        assert ref[1] >= e and (ref[1] > e or (ref[2], ref[3]) == (ql, qh))


def test_mirror_turns_a_body_inside_out(mcpt):
    """anim_scenes.mirror on cornell-box's "Table" and on random triangles: for every mirrored face the sign of n . (face centroid - c), c the
    body's centroid, is the opposite of the original's, where n = (v1 - v2) x (v3 - v1) is the normal the loader and an update store; the
    body keeps its centroid and its extent; every other face keeps its bits"""
    import anim_scenes as A
    from conftest import SCENES
    sc = mcpt.Scene(SCENES, "cornell-box", width=64, height=36)
    g, m, _ = sc.faces()
    names = [sc.material(i)[0] for i in range(sc.info.num_materials)]
    table = np.nonzero(m == names.index("Table"))[0]
    rng = np.random.default_rng(6)
    soup = rng.normal(size=(300, 9))
    for v, faces in ((np.ascontiguousarray(g[:, :9]), table), (soup, np.arange(0, 300, 3))):
        w = A.mirror(v, faces)
        rest = np.setdiff1d(np.arange(v.shape[0]), faces)
        assert np.array_equal(w[rest].view(np.uint64), v[rest].view(np.uint64)) and not np.array_equal(w[faces], v[faces])
        c = v[faces].reshape(-1, 3).mean(axis=0)
        assert np.abs(w[faces].reshape(-1, 3).mean(axis=0) - c).max() <= 1e-12 * np.abs(v[faces]).max()
        lo, hi = v[faces].reshape(-1, 3).min(axis=0), v[faces].reshape(-1, 3).max(axis=0)
        wl, wh = w[faces].reshape(-1, 3).min(axis=0), w[faces].reshape(-1, 3).max(axis=0)
        assert np.array_equal(wl[1:], lo[1:]) and np.array_equal(wh[1:], hi[1:])      # y and z untouched; x in [2c - hi, 2c - lo]
        assert wl[0] == 2.0 * c[0] - hi[0] and wh[0] == 2.0 * c[0] - lo[0]
        side = lambda x: (A.face_normals(x[faces]) * (x[faces].reshape(-1, 3, 3).mean(axis=1) - c)).sum(axis=1)
        a, b = side(v), side(w)
        decided = np.abs(a) > 1e-9 * np.abs(a).max()          # (a face whose plane holds c faces neither way)
        assert decided.sum() > 0.9 * faces.size
        assert np.array_equal(np.sign(b[decided]), -np.sign(a[decided]))
        assert np.abs(a + b).max() <= 1e-9 * np.abs(a).max()
    sc.close()


def test_new_symbols_and_null_handles(mcpt):
    from montecarlopathtracing_amd import _lib
    L = mcpt.lib()
    hdr = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    for sym in NEW:
        assert (sym + "(") in hdr and sym in _lib.EXPORTS and hasattr(L, sym), sym
    assert L.mcpt_version() == 105
    ERR_ARG = L.mcpt_device_get_leaf_order(None, None)      # what the other device entry points give a null handle, with or without a device
    assert ERR_ARG != 0
    v = np.zeros(9)
    pv = v.ctypes.data_as(C.POINTER(C.c_double))
    e = (C.c_double * 3)(0, 0, 1)
    info = _lib.UpdateInfo()
    assert L.mcpt_device_update_vertices(None, pv, 0, C.byref(info)) == ERR_ARG
    assert L.mcpt_device_update_vertices_device(None, None, 0, None, None) == ERR_ARG
    assert L.mcpt_device_get_vertices(None, pv) == ERR_ARG
    assert L.mcpt_device_set_camera(None, e, e, e, 40.0) == ERR_ARG
    assert L.mcpt_device_get_camera(None, e, e, e, None) == ERR_ARG
    assert L.mcpt_multi_update_vertices(None, pv, 0, None) == ERR_ARG
    assert L.mcpt_multi_set_camera(None, e, e, e, 40.0) == ERR_ARG
    assert b"null" in L.mcpt_last_error()


def test_update_info_layout(tmp_path):
    """the Python mirror of mcpt_update_info has the header's size and offsets"""
    import subprocess
    from montecarlopathtracing_amd import _lib
    src = tmp_path / "s.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"mcpt.h\"\nint main(void) {\n"
                   "  printf(\"%zu %zu %zu\\n\", sizeof(mcpt_update_info), offsetof(mcpt_update_info, ms_reference), offsetof(mcpt_update_info, cost_after));\n"
                   "  return 0; }\n")
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    size, o1, o2 = map(int, subprocess.check_output([str(exe)]).split())
    assert (size, o1, o2) == (C.sizeof(_lib.UpdateInfo), _lib.UpdateInfo.ms_reference.offset, _lib.UpdateInfo.cost_after.offset)
