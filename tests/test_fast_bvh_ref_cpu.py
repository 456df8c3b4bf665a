"""The hierarchy checker of tests/fast_bvh_ref.py on hand-built trees, no GPU: it accepts a valid tree (also one whose planes are not
representable in fp64) and rejects each kind of damage a builder could do -- without these controls the GPU tests that run it on
device-built trees could pass vacuously."""
import numpy as np
import pytest

import fast_bvh_ref as R


def _tree():
    """six triangles: root = [leaf of slots 0-1, node 1]; node 1 = four one-triangle leaves (slots 2..5).  tri_faces a permutation."""
    rng = np.random.default_rng(5)
    v = rng.uniform(-3.0, 3.0, size=(6, 9))
    v[:, 1::3] += np.arange(6)[:, None] * 4.0            # apart in y, so that every plane is tight against one triangle
    faces = np.array([4, 0, 5, 2, 1, 3], dtype=np.int32)
    lo, hi = R.face_boxes(v)
    tlo, thi = lo[faces], hi[faces]
    inner = R.make_node([tlo[k] for k in range(2, 6)], [thi[k] for k in range(2, 6)], [R.leaf_ref(k, 1) for k in range(2, 6)])
    root = R.make_node([tlo[:2].min(0), tlo[2:].min(0)], [thi[:2].max(0), thi[2:].max(0)], [R.leaf_ref(0, 2), 1])
    rec = np.array([root, inner], dtype=R.CW_DTYPE)
    return rec, faces, lo, hi


def test_accepts_a_valid_tree():
    rec, faces, lo, hi = _tree()
    got = R.check_hierarchy(R.encode(rec), faces, lo, hi, stack_need=4)
    assert got == {"nodes": 2, "leaves": 5, "depth": 2, "need": 4}     # root pushes 1, node 1 pushes 3


def test_record_layout_round_trips():
    rec, _, _, _ = _tree()
    raw = R.encode(rec)
    assert raw.shape == (2, 64) and raw.dtype == np.uint8
    assert R.decode(raw.tobytes()).tobytes() == rec.tobytes()
    assert R.split_leaf(R.leaf_ref(1234, 8)) == (1234, 8)


def test_planes_are_exact_where_fp64_is_not():
    """p = 2^20, step 2^-126: fl(p + q * 2^-126) = p, but the plane is above p -- a box ending at p is not inside [p + 2^-126, ..]"""
    r = np.zeros(1, dtype=R.CW_DTYPE)
    r["p"][0] = [2.0 ** 20, 0, 0]
    r["e"][0] = [-126, 0, 0]
    r["qlo"][0] = [1, 0, 0]
    r["qhi"][0] = [255, 1, 1]
    lo_s, lo_r, _, _ = R.planes(r)
    assert lo_s[0, 0, 0] == 2.0 ** 20 and lo_r[0, 0, 0] == 2.0 ** -126
    assert not R._le(lo_s[0, 0, 0], lo_r[0, 0, 0], 2.0 ** 20)
    assert R._le(lo_s[0, 0, 0], lo_r[0, 0, 0], np.nextafter(2.0 ** 20, np.inf))


def test_accepts_planes_on_a_far_offset_grid():
    """millimetre triangles near 1e6: the grid origin is rounded down to fp32, the step is far below its ulp"""
    v = np.array([[1e6 + 0.001, 1e6, -1e6, 1e6 + 0.002, 1e6 + 0.001, -1e6, 1e6, 1e6 + 0.003, -1e6 - 0.001]])
    lo, hi = R.face_boxes(v)
    root = R.make_node([lo[0]], [hi[0]], [R.leaf_ref(0, 1)])
    R.check_hierarchy(R.encode(np.array([root])), np.array([0]), lo, hi, stack_need=0)


def _rejects(rec, faces, lo, hi, match, stack_need=4):
    with pytest.raises(R.HierarchyError, match=match):
        R.check_hierarchy(R.encode(rec), faces, lo, hi, stack_need=stack_need)


@pytest.mark.parametrize("node,slot", [(0, 0), (1, 2)])
@pytest.mark.parametrize("side", ["lo", "hi"])
def test_rejects_a_plane_one_step_inward(node, slot, side):
    rec, faces, lo, hi = _tree()
    a = 1                                                  # y: the triangles are apart there, every slot's planes are tight
    sh = 8 * slot
    q = (int(rec[node]["q" + side][a]) >> sh) & 255
    q2 = q + 1 if side == "lo" else q - 1
    assert 0 <= q2 <= 255
    rec[node]["q" + side][a] = (int(rec[node]["q" + side][a]) & ~(255 << sh)) | (q2 << sh)
    _rejects(rec, faces, lo, hi, "do not contain")


def test_rejects_a_dropped_triangle():
    rec, faces, lo, hi = _tree()
    rec[0]["child"][0] = R.leaf_ref(0, 1)                 # slot 1 no longer referenced
    _rejects(rec, faces, lo, hi, "referenced")


def test_rejects_a_duplicated_reference():
    rec, faces, lo, hi = _tree()
    rec[1]["child"][3] = R.leaf_ref(2, 1)                 # slot 2 twice, slot 5 never
    _rejects(rec, faces, lo, hi, "referenced")


def test_rejects_a_cycle_and_a_shared_node():
    rec, faces, lo, hi = _tree()
    cyc = rec.copy()
    cyc[1]["child"][3] = 0                                # node 1 -> root
    _rejects(cyc, faces, lo, hi, "reached twice")
    shared = np.array([rec[0], rec[1], rec[1]])
    shared[0]["child"][0] = 1                             # root -> node 1 twice (and node 2 unreached)
    shared[0]["child"][1] = 1
    _rejects(shared, faces, lo, hi, "reached twice")


def test_rejects_an_unreached_node_and_a_bad_reference():
    rec, faces, lo, hi = _tree()
    extra = np.array([rec[0], rec[1], rec[1]])
    _rejects(extra, faces, lo, hi, "not reached")
    bad = rec.copy()
    bad[0]["child"][1] = 7
    _rejects(bad, faces, lo, hi, "refers to node 7")


def test_rejects_nchild_count_and_leaf_size():
    rec, faces, lo, hi = _tree()
    r = rec.copy()
    r[1]["nchild"] = 3
    _rejects(r, faces, lo, hi, "nchild")
    r = rec.copy()
    r[0]["child"][0] = -1 - ((0 << 4) | 9)               # ten triangles: the walk would read count - 1 = 1 from three bits
    _rejects(r, faces, lo, hi, "leaf of 10")


def test_rejects_a_stack_need_above_the_recorded_one_and_a_wrong_face_list():
    rec, faces, lo, hi = _tree()
    _rejects(rec, faces, lo, hi, "stack entries", stack_need=3)
    f = faces.copy()
    f[0] = f[1]
    _rejects(rec, f, lo, hi, "permutation")
    _rejects(rec, faces[:5], lo, hi, "permutation")
