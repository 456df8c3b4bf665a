"""No GPU: the oracle's light pick (oracle/mcpt_oracle.c: orc_scene_set_light_pick), the side tests/test_gpu_light_pick_oracle.py holds
the devices to.

(a) the oracle's pick alone equals the numpy restatements bit for bit: mode 1 against light_pick_ref.PickRef.pick, mode 2 against
    light_tree_ref.TreeRef.pick on light_tree_ref.vertex_set (horizon and culling edges by construction), at 2, 3, 9 and 40 lights, under
    the default weights and caller weights with zeros (the last light's among them);
(b) mode 0 is what it was: a scene that was set to mode 1 and cleared gives the samples, the frame and the statistics of a scene that was
    never touched, bit for bit;
(c) on a scene of one light modes 1 and 2 are mode 0 bit for bit (p = 1);
(d) the one-hot anchor, on the oracle alone: on the diffuse-only room the sum over l of mode 1 under weights e_l is mode 0 within
    test_gpu_light_pick's derived 1e-12 (the sides differ in summation order only), and mode 2 under e_l is mode 1 under e_l bit for bit
    (every branch of the descent is forced: p = 1) -- the new branch hangs on the old loop;
(e) the oracle's two deliberately wrong answers (set_light_pick(wrong=1 | 2)) fail test_gpu_lights._check_samples against the right one:
    a sample-by-sample comparison sees what a z test of block means does not."""
import os

import numpy as np
import pytest

import light_pick_ref as LP
import light_scenes
import light_tree_ref as LT
import test_gpu_light_pick as GP
import test_gpu_lights as TL
from conftest import SCENES

COUNTS = (2, 3, 9, 40)
W, H = 48, 32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def zero_weights(nl):
    """caller weights with zeros: always the last light's; from 9 lights on also the first's and one in the middle"""
    w = np.random.default_rng(200 + nl).uniform(0.1, 5.0, size=nl)
    w[[0, nl // 2, nl - 1] if nl >= 9 else [nl - 1]] = 0.0
    return w


def stats_tuple(st):
    return tuple(getattr(st, f) for f, _ in st._fields_)


@pytest.fixture(scope="module")
def rooms(mcpt, oracle, tmp_path_factory):
    """nl -> (directory, name, the product's host-side scene -- for the refs' default weights and light boxes --, an oracle scene)"""
    d = str(tmp_path_factory.mktemp("pick_oracle_scenes")) + os.sep
    out = {}
    for nl in COUNTS:
        name = "room%d" % nl
        light_scenes.write(d, name, nl, W, H)
        out[nl] = (d, name, mcpt.Scene(d, name, width=W, height=H), oracle.OracleScene(d + name, texture_dir=d, width=W, height=H))
    yield out
    for _, _, sc, osc in out.values():
        sc.close()
        osc.close()


# ---------------------------------------------------------------------------------------------- (a) the pick
@pytest.mark.parametrize("weights", ["default", "zeros"])
@pytest.mark.parametrize("nl", COUNTS)
def test_table_pick_equals_the_restatement(rooms, nl, weights):
    _, _, sc, osc = rooms[nl]
    ref = LP.PickRef.of_scene(sc, zero_weights(nl) if weights == "zeros" else None)
    osc.set_light_pick(1, pick_ref=ref)
    try:
        seen = np.zeros(nl, dtype=np.int64)
        for depth in (0, 1, 5, 63):
            pix, k = GP.triples(1500, 100 * nl + depth)
            light, pdf, inv = osc.light_pick(1234567 + depth, pix, k, depth)
            want_l, want_p = ref.pick(1234567 + depth, pix, k, depth)
            assert np.array_equal(light, want_l), "depth %d: %d picks differ" % (depth, int((light != want_l).sum()))
            assert np.array_equal(bits(inv), bits(ref.inv[want_l]))           # the factor the shading scales by: the table's own quotient
            assert np.array_equal(bits(pdf), bits(1.0 / ref.inv[want_l])) and np.abs(pdf / want_p - 1.0).max() <= 2.0 ** -52
            seen += np.bincount(light, minlength=nl)
        assert (seen[ref.w == 0] == 0).all() and seen[ref.last] > 0           # a light of weight 0 never appears; the clamp's light does
        assert (seen[ref.pdf > 0.02] > 0).all()
    finally:
        osc.set_light_pick(0)
    with pytest.raises(ValueError):
        osc.light_pick(1, [0], [0], 0)                                       # the scene does not pick


@pytest.mark.parametrize("weights", ["default", "zeros"])
@pytest.mark.parametrize("nl", COUNTS)
def test_tree_pick_equals_the_restatement(rooms, nl, weights):
    _, _, sc, osc = rooms[nl]
    ref = LT.TreeRef.of_scene(sc, zero_weights(nl) if weights == "zeros" else None)
    osc.set_light_pick(2, tree_ref=ref)
    try:
        vp, vn = LT.vertex_set(ref, seed=nl)
        reps = -(-2100 // vp.shape[0])
        p, pn = np.tile(vp, (reps, 1)), np.tile(vn, (reps, 1))
        seen = np.zeros(nl, dtype=np.int64)
        met = {}
        for depth in (0, 1, 63):
            pix, k = GP.triples(p.shape[0], 100 * nl + depth)
            light, pdf, inv = osc.light_pick(77 + depth, pix, k, depth, p, pn)
            want_l, want_p, trace = ref.pick(77 + depth, pix, k, depth, p, pn)
            assert np.array_equal(light, want_l), "depth %d: %d picks differ" % (depth, int((light != want_l).sum()))
            assert np.array_equal(bits(pdf), bits(want_p)) and np.array_equal(bits(inv), bits(1.0 / want_p))
            seen += np.bincount(light, minlength=nl)
            for f, v in trace.items():
                met[f] = met.get(f, False) | v.any()
        assert (seen[ref.w == 0] == 0).all() and (seen > 0).sum() >= min(int((ref.w > 0).sum()), 2)
        for case in ("both_culled_root", "one_culled", "s_zero", "s_below_inside_margin", "dist_zero"):
            assert met[case], "nl %d: no vertex met %s" % (nl, case)          # the edges the vertex set is built for were walked
        with pytest.raises(ValueError):
            osc.light_pick(1, [0], [0], 0)                                   # the tree needs a vertex
    finally:
        osc.set_light_pick(0)


def test_setter_refuses_what_does_not_fit_the_scene(rooms, oracle):
    _, _, sc, osc = rooms[3]
    other = rooms[9][2]
    with pytest.raises(ValueError):
        osc.set_light_pick(1, pick_ref=LP.PickRef.of_scene(other))           # a table of 9 lights
    with pytest.raises(ValueError):
        osc.set_light_pick(2, tree_ref=LT.TreeRef.of_scene(other))
    with pytest.raises(ValueError):
        osc.set_light_pick(3)
    with pytest.raises(ValueError):
        osc.set_light_pick(0, wrong=1)                                       # nothing to get wrong without a pick
    st0, st1 = oracle.Stats(), oracle.Stats()
    a = osc.sample_radiance(5, 20, 20, 1, stats=st0)
    assert oracle.lib().orc_scene_set_light_pick(osc.h, 1, None, None, 3, 0, 1.0, None, 0) == -1
    b = osc.sample_radiance(5, 20, 20, 1, stats=st1)
    assert np.array_equal(bits(a), bits(b)) and stats_tuple(st0) == stats_tuple(st1)      # a refused setting changes nothing


# ---------------------------------------------------------------------------------------------- (b) mode 0 is what it was
def test_mode_0_is_unchanged_after_a_pick_was_set_and_cleared(oracle, tmp_path):
    d = str(tmp_path) + os.sep
    light_scenes.write(d, "never", 10, 33, 17)
    never = oracle.OracleScene(d + "never", texture_dir=d, width=33, height=17)
    used = oracle.OracleScene(d + "never", texture_dir=d, width=33, height=17)
    w = np.linspace(1.0, 3.0, 10)
    used.set_light_pick(1, pick_ref=LP.PickRef(w))
    picked = used.render(2, seed=3)
    used.set_light_pick(0)
    pix, k = np.random.default_rng(4).integers(0, 33 * 17, size=200), np.random.default_rng(5).integers(0, 64, size=200)
    for p, kk in zip(pix, k):
        st0, st1 = oracle.Stats(), oracle.Stats()
        a = never.sample_radiance(77, int(p // 33), int(p % 33), int(kk), stats=st0)
        b = used.sample_radiance(77, int(p // 33), int(p % 33), int(kk), stats=st1)
        assert np.array_equal(bits(a), bits(b)) and stats_tuple(st0) == stats_tuple(st1)
    st0, st1 = oracle.Stats(), oracle.Stats()
    a, b = never.render(2, seed=3, stats=st0), used.render(2, seed=3, stats=st1)
    assert np.array_equal(bits(a), bits(b)) and stats_tuple(st0) == stats_tuple(st1)
    assert st0.rays_shadow > 0 and st0.rays_shadow % 10 == 0 and np.isfinite(a).all()
    assert not np.array_equal(bits(picked), bits(a))                         # the setting had been taken: the picked frame is another
    never.close()
    used.close()


# ---------------------------------------------------------------------------------------------- (c) one light: p = 1
def test_one_light_scene_is_mode_0_in_every_mode(mcpt, oracle):
    w, h = 33, 17
    sc = mcpt.Scene(SCENES, "cornell-box", width=w, height=h)
    osc = oracle.OracleScene(SCENES + "cornell-box", texture_dir=SCENES, width=w, height=h)
    assert osc.num_lights == 1
    table, tree = LP.PickRef.of_scene(sc), LT.TreeRef.of_scene(sc)
    assert table.inv[0] == 1.0 and tree.nodes.shape[0] == 1
    pix, k = np.random.default_rng(6).integers(0, w * h, size=150), np.random.default_rng(7).integers(0, 64, size=150)
    out = {}
    for mode in (0, 1, 2):
        osc.set_light_pick(mode, pick_ref=table, tree_ref=tree)
        st = oracle.Stats()
        img = osc.render(2, seed=3, stats=st)
        sst = oracle.Stats()
        smp = np.array([osc.sample_radiance(77, int(p // w), int(p % w), int(kk), stats=sst) for p, kk in zip(pix, k)])
        out[mode] = (img, smp, stats_tuple(st), stats_tuple(sst))
    for mode in (1, 2):
        assert np.array_equal(bits(out[mode][0]), bits(out[0][0])) and np.array_equal(bits(out[mode][1]), bits(out[0][1])), mode
        assert out[mode][2:] == out[0][2:], mode
    assert out[0][0].sum() > 0 and out[0][2][1] > 0                          # light, and shadow rays
    sc.close()
    osc.close()


# ---------------------------------------------------------------------------------------------- (d) the one-hot anchor
def _non_emitter_samples(osc, n, seed, w, h):
    """(pix, k) of n camera samples whose primary hit is a surface that is not an emitter (the pinhole: the hit depends on the pixel)"""
    pix, k = GP.triples(n, seed)
    pix = pix % (w * h)
    rays = np.array([osc.primary_ray(int(p // w), int(p % w)) for p in pix])
    face = osc.trace_closest(rays)[0]
    mat = osc.faces()[1]
    lights = [osc.light(i)[2] for i in range(osc.num_lights)]
    keep = (face >= 0) & ~np.isin(mat[np.maximum(face, 0)], lights)
    assert keep.sum() > 0.8 * n
    return pix[keep], k[keep]


@pytest.mark.parametrize("nl", [3, 10])
def test_one_hot_weights_add_up_to_mode_0(mcpt, oracle, tmp_path, nl):
    d = str(tmp_path) + os.sep
    name = GP.write_scene(d, nl, diffuse_only=True)
    sc = mcpt.Scene(d, name, width=GP.W, height=GP.H)
    osc = oracle.OracleScene(d + name, texture_dir=d, width=GP.W, height=GP.H)
    for m in range(osc.num_materials):
        rec = osc.material(m)[1]
        assert not np.any(rec[3:6]) and rec[7] == 1.0, "material %d is not diffuse-only" % m
    pix, k = _non_emitter_samples(osc, 400, 7 + nl, GP.W, GP.H)

    def samples():
        return np.array([osc.sample_radiance(41, int(p // GP.W), int(p % GP.W), int(kk)) for p, kk in zip(pix, k)])
    ref = samples()
    assert np.isfinite(ref).all() and (ref >= 0).all() and (ref > 0).any(axis=1).mean() > 0.5
    total = np.zeros_like(ref)
    for l in range(nl):
        e = np.zeros(nl)
        e[l] = 1.0
        osc.set_light_pick(1, pick_ref=LP.PickRef(e))
        one = samples()
        osc.set_light_pick(2, tree_ref=LT.TreeRef.of_scene(sc, e))
        tree = samples()
        assert np.array_equal(bits(tree), bits(one)), "light %d" % l
        assert (one >= 0).all() and np.isfinite(one).all()
        total += one
    rel = np.abs(total - ref) / np.maximum(np.abs(ref), 1e-300)
    rel[ref == 0] = np.where(total[ref == 0] == 0, 0.0, np.inf)
    print("one-hot identity on the oracle, %d lights: max relative difference %.3e over %d samples" % (nl, rel.max(), pix.shape[0]))
    assert rel.max() <= 1e-12
    sc.close()
    osc.close()


# ---------------------------------------------------------------------------------------------- (e) the wrong oracles are seen
@pytest.mark.parametrize("mode", [1, 2])
def test_the_sample_check_fails_against_a_wrong_oracle(rooms, oracle, mode):
    """wrong = 1 touches only paths that reach a lit vertex at depth > 0, wrong = 2 only vertices whose pick is not light 0: a share of the
    samples -- and the sample check, which allows int(n * OTHER_FLIP_RATE) = 0 mismatches here, fails on both."""
    _, _, sc, osc = rooms[9]
    table, tree = LP.PickRef.of_scene(sc), LT.TreeRef.of_scene(sc)
    pix, k = GP.triples(600, 11)
    pix = pix % (W * H)

    def samples(wrong):
        osc.set_light_pick(mode, pick_ref=table, tree_ref=tree, wrong=wrong)
        return np.array([osc.sample_radiance(77, int(p // W), int(p % W), int(kk)) for p, kk in zip(pix, k)])
    try:
        right = samples(0)
        TL._check_samples(right, samples(0))
        for wrong in (1, 2):
            bad = samples(wrong)
            with pytest.raises(AssertionError):
                TL._check_samples(right, bad)
            share = (np.abs(right - bad).max(axis=1) > TL.REL_TOL * np.abs(right).max(axis=1)).mean()
            print("mode %d, wrong %d: %.1f %% of the samples differ" % (mode, wrong, 100 * share))
            assert 0.02 < share < 1.0
    finally:
        osc.set_light_pick(0)
