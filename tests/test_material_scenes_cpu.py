"""Not gpu: the scenes of tests/material_scenes.py through both loaders, and what the oracle alone says about them -- the conditions
under which tests/test_gpu_materials.py's comparison means something.

(a) both loaders return the same material records, light tables and faces for both variants (test_host_parity.py's comparison);
(b) at 96x64 every row is the primary hit of at least 40 pixels;
(c) the sample plan -- per row 200 (pixel, k) pairs on the row's pixels from a fixed seed (G4: 400, see PLAN_SIZE), defined here once and
    imported by the GPU test: every oracle sample is finite, "opaque" has no on-surface ray on any sample, each of G1-G6 has at least 50
    on-surface samples;
(d) sensitivity, from the reference alone: for every row but O10 the oracle's answers on the row's samples differ from the sibling
    scene's by more than 1e-6 relative on at least 10 % of them -- about 3x the widest flip allowance of the GPU test and 4000x the
    ordinary one, so a kernel that ignored the row's parameter cannot hide in the allowance;
(e) O10 (Ni 0.8) equals its Ni 1 sibling bit for bit.

Measured (the figures the tests print): pixels per row 149 (G1) to 201 (O11); on-surface samples: G1 117, G2 130, G3 83, G4 78 of its 400
(34 of 200 before), G5 120, G6 126, and 0 to 9 on the opaque rows of the glass variant (a bounce that reaches a glass body); share of a
row's samples that differ from the sibling's, opaque variant: O1 0.755, O2 0.53, O3 0.535, O4 0.515, O5 0.96, O6 1.0, O7 0.93, O8 0.855,
O9 0.925, O10 0 (bit for bit), O11 1.0; glass rows: G1 0.585, G2 0.115, G3 0.385, G4 0.532, G5 0.995, G6 0.955.  G2's sibling changes
Ks alone, so only the samples whose Fresnel draw reflects can move: 0.055 with both lights in front of the swatches, where the far faces
of a body are dark; one light went behind them (material_scenes.LIGHT_CENTRES), the material stayed."""
import os

import numpy as np
import pytest

import material_scenes as MS

W, H = 96, 64
SEED = 77
PER_ROW = 200
# G4 takes twice as many: with Ni 10, rf0 = (9 / 11)^2 = 0.67, so a vertex on it refracts with probability below 0.6 * 0.33 = 0.2 (Russian
# roulette, then the Fresnel draw) -- 200 samples cannot be asked for 50 on-surface paths, 400 can
PLAN_SIZE = {"G4": 2 * PER_ROW}
MIN_PIXELS = 40
MIN_ON_SURFACE = 50
SENSITIVE_REL = 1e-6
SENSITIVE_SHARE = 0.10


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def row_pixels(osc, info):
    """{row: the pixels (row-major indices, ascending) whose pinhole ray's closest hit is a face of the row's body}"""
    face = osc.trace_closest(osc.primary_rays())[0]
    return {row: np.flatnonzero((face >= first) & (face < first + n)).astype(np.int32) for row, (first, n) in info["rows"].items()}


def sample_plan(osc, info):
    """The sample plan of a variant: (pix, k, row_of) -- per row, in material_scenes.ROWS' order, per_row (pixel, k < 64) pairs on the
    row's pixels from a fixed seed; row_of[i] is the index of sample i's row in material_scenes.ROW_NAMES."""
    pixels = row_pixels(osc, info)
    pix, k, row_of = [], [], []
    for i, row in enumerate(MS.ROW_NAMES):
        if row not in pixels:
            continue
        rng = np.random.default_rng(1000 + i)
        per_row = PLAN_SIZE.get(row, PER_ROW)
        pix.append(rng.choice(pixels[row], size=per_row))
        k.append(rng.integers(0, 64, size=per_row))
        row_of.append(np.full(per_row, i))
    return np.concatenate(pix).astype(np.int32), np.concatenate(k).astype(np.int32), np.concatenate(row_of)


def oracle_samples(oracle, osc, pix, k, seed=SEED):
    """the oracle's radiance (n, 3) of camera samples (pix[i], k[i]) and whether each path had an on-surface ray (n,) bool"""
    o = np.zeros((pix.shape[0], 3))
    on_surface = np.zeros(pix.shape[0], dtype=bool)
    for i, (p, kk) in enumerate(zip(pix, k)):
        st = oracle.Stats()
        o[i] = osc.sample_radiance(seed, int(p // osc.width), int(p % osc.width), int(kk), stats=st)
        on_surface[i] = st.rays_on_surface > 0
    return o, on_surface


def differing(a, b, rel=SENSITIVE_REL):
    """per sample: whether a and b differ by more than rel of the larger one's scale"""
    scale = np.maximum(np.maximum(np.abs(a).max(axis=1), np.abs(b).max(axis=1)), 1e-12)
    return np.abs(a - b).max(axis=1) / scale > rel


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("material_scenes")) + os.sep


@pytest.fixture(scope="module", params=list(MS.VARIANTS))
def variant(request, oracle, scene_dir):
    """(variant, scene name, what write() returned, the oracle's scene, the plan, the oracle's samples and their on-surface flags)"""
    v = request.param
    name = "materials_" + v
    info = MS.write(scene_dir, name, W, H, variant=v)
    osc = oracle.OracleScene(scene_dir + name, texture_dir=scene_dir, width=W, height=H)
    pix, k, row_of = sample_plan(osc, info)
    o, on_surface = oracle_samples(oracle, osc, pix, k)
    yield v, name, info, osc, (pix, k, row_of), o, on_surface
    osc.close()


def test_loaders_agree(variant, mcpt, scene_dir):
    v, name, info, osc, _, _, _ = variant
    sc = mcpt.Scene(scene_dir, name, width=W, height=H)
    try:
        i = sc.info
        assert (i.num_faces, i.num_materials, i.num_lights, i.width, i.height) == \
            (osc.num_faces, osc.num_materials, osc.num_lights, osc.width, osc.height)
        assert i.num_lights == 2 and i.num_faces == 16 + 12 * (len(MS.VARIANTS[v]) - (v == "glass")) + 80 * (v == "glass")
        cam = np.array(list(i.eye) + list(i.look_at) + list(i.up) + [i.fovy])
        assert np.array_equal(_bits(cam), _bits(osc.camera))
        og, om, ok = osc.faces()
        g, m, k = sc.faces()
        assert np.array_equal(_bits(og), _bits(g)) and np.array_equal(om, m) and np.array_equal(ok, k)
        names = []
        for j in range(i.num_materials):
            a, b = osc.material(j), sc.material(j)
            assert a[0] == b[0] and np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(a[2], b[2]), a[0]
            names.append(a[0])
        assert [r for r in MS.ROW_NAMES if r in names] == MS.VARIANTS[v]
        for row, _, mat, _, _ in MS.ROWS:               # the records are the table's
            if row in names:
                _, rec, fl = sc.material(names.index(row))
                assert tuple(rec) == mat["kd"] + mat["ks"] + (mat["ns"], mat["ni"]), row
                assert bool(fl[0]) == bool(mat["tex"]) and (fl[3] >= 0) == (row == "O11"), row
                if mat["tex"]:
                    assert (fl[1], fl[2]) == MS.TEXTURES[mat["tex"]].shape[1::-1], row
        for j in range(i.num_lights):
            a, b = osc.light(j), sc.light(j)
            assert a[0] == b[0] == info["lights"][j] and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]
        # light 0 is not larger than light 1: the lamp's quad is exactly as large as light 1's, whose material also has O11's body
        assert abs(sc.light(0)[3] - MS.LIGHT_SIDE ** 2) < 1e-12 and sc.light(0)[3] < sc.light(1)[3]
    finally:
        sc.close()


def test_every_row_is_seen(variant):
    v, _, info, osc, _, _, _ = variant
    pixels = row_pixels(osc, info)
    print("%s: pixels per row %s" % (v, {r: len(p) for r, p in pixels.items()}))
    assert list(pixels) == MS.VARIANTS[v]
    for row, p in pixels.items():
        assert len(p) >= MIN_PIXELS, (row, len(p))
    # the map's coordinates leave the unit square on both sides: floor wraps below 0 and above 1
    g = osc.faces()[0]
    first, n = info["rows"]["O7"]
    vt = g[first:first + n, 18:24]
    assert vt.min() == MS.VT_LO < 0 and vt.max() == MS.VT_HI > 1


def test_plan_against_the_oracle(variant):
    v, _, _, _, (pix, k, row_of), o, on_surface = variant
    assert pix.shape[0] == sum(PLAN_SIZE.get(r, PER_ROW) for r in MS.VARIANTS[v])
    assert np.isfinite(o).all()
    per_row = {MS.ROW_NAMES[i]: int(on_surface[row_of == i].sum()) for i in np.unique(row_of)}
    print("%s: on-surface samples per row %s" % (v, per_row))
    if v == "opaque":
        assert not on_surface.any()
    else:
        for row in MS.GLASS_ROWS:
            assert per_row[row] >= MIN_ON_SURFACE, (row, per_row[row])
        for row in MS.OPAQUE_ROWS:
            assert per_row[row] < PER_ROW // 2, (row, per_row[row])           # (a bounce may still reach a glass body)
    lit = (o > 0).any(axis=1)
    for i in np.unique(row_of):
        # a row that shows black says nothing; O8 is black, and O1 (Kd 0) is lit through its bounce alone, which Russian roulette ends
        # on 40 % of the samples
        if MS.ROW_NAMES[i] != "O8":
            assert lit[row_of == i].mean() > 0.25, MS.ROW_NAMES[i]


def test_every_row_is_sensitive_to_its_parameter(variant, oracle, scene_dir):
    """the oracle on the row's samples in the scene where that row alone is its sibling"""
    v, _, _, _, (pix, k, row_of), o, _ = variant
    shares = {}
    for i in np.unique(row_of):
        row = MS.ROW_NAMES[i]
        name = "materials_%s_sib_%s" % (v, row)
        MS.write(scene_dir, name, W, H, variant=v, siblings={row: True})
        sib = oracle.OracleScene(scene_dir + name, texture_dir=scene_dir, width=W, height=H)
        try:
            mine = row_of == i
            s, _ = oracle_samples(oracle, sib, pix[mine], k[mine])
        finally:
            sib.close()
        shares[row] = float(differing(o[mine], s).mean())
        if row == "O10":
            assert np.array_equal(_bits(o[mine]), _bits(s)), "Ni 0.8 differs from Ni 1"
    print("%s: share of a row's samples that differ from its sibling's %s" % (v, {r: round(s, 3) for r, s in shares.items()}))
    for row, share in shares.items():
        if row != "O10":
            assert share >= SENSITIVE_SHARE, (row, share)
