"""-m gpu: MCPT_LIGHTS_TREE -- one shadow ray per vertex, the light picked by a descent of the light tree (include/mcpt.h: light sampling).

(a) the device's pick at given vertices against the numpy restatement (tests/light_tree_ref.py) and the host's walk, bit for bit;
(b) the anchor to the oracle-pinned mode: under one-hot weights the pick's probability is 1, so "tree" samples equal "one" samples bit for
    bit, and their sum over the lights is the "all" sample within 1e-12 (test_gpu_light_pick.py's bar, derived there);
(c) the paths are the "all" frame's, one shadow ray or one skip per vertex, never more skips than "one" for the same draws; every route of
    test_gpu_lights.py gives the same frame and counts;
(d) "tree" - "all" per sample has block means consistent with 0 (pins_common's bars, the blocks of test_one_minus_all_has_zero_mean), and a
    numpy estimator whose probability comes from a wrong importance fails the same test;
(e) on the 40-light room the frame's RMSE against a 1024-sample "all" frame is lower under "tree" than under "one" at 16 samples per pixel;
(f) progressive, adaptive, denoised, lens, environment, updated, motion, MultiDevice and checkpointed frames pick the setting up;
(g) clearing the setting and one-light scenes are neutral, and "all" / "one" frames equal those recorded from the commit before this mode
    existed (tests/golden/light_modes_parent.npz)."""
import os

import numpy as np
import pytest

import anim_scenes as A
import light_pick_ref as LP
import light_scenes
import light_tree_ref as LT
import motion_ref as MR
import pins_common
import test_gpu_light_pick as P
import test_gpu_lights as TL
from conftest import ROOT, SCENES
from test_gpu_light_pick import _clean_env, rooms, scene_dir  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

W, H = P.W, P.H
bits, same, triples = P.bits, P.same, P.triples


def caller_weights(nl):
    w = np.random.default_rng(nl).uniform(0.05, 3.0, size=nl)
    if nl > 2:
        w[[0, nl // 2] if nl > 3 else [1]] = 0.0
    return w


# ---------------------------------------------------------------------------------------------- (a) the pick seam
@pytest.mark.parametrize("weights", ["default", "caller"])
@pytest.mark.parametrize("nl", [2, 3, 10, 40])
def test_pick_at_matches_the_restatement(rooms, nl, weights):
    r = rooms(nl)
    dev = r.device()
    w = caller_weights(nl) if weights == "caller" else None
    dev.set_light_sampling("tree", w)
    try:
        ref = LT.TreeRef.of_scene(r.sc, w)
        mode, root_pdf = dev.light_sampling()
        assert mode == "tree" and same(root_pdf, ref.table.pdf)          # the root's distribution
        vp, vn = LT.vertex_set(ref, seed=nl)
        reps = -(-2100 // vp.shape[0])
        p, pn = np.tile(vp, (reps, 1)), np.tile(vn, (reps, 1))
        host = r.sc.light_tree_pdf(vp, vn, w)
        host = np.tile(host, (reps, 1))
        seen = np.zeros(nl, dtype=np.int64)
        for depth in (0, 1, 63):
            pix, k = triples(p.shape[0], 100 * nl + depth)
            light, q = dev.light_pick_at(77 + depth, pix, k, depth, p, pn)
            want_l, want_q, _ = ref.pick(77 + depth, pix, k, depth, p, pn)
            assert np.array_equal(light, want_l), "depth %d: %d picks differ" % (depth, int((light != want_l).sum()))
            assert same(q, want_q)
            assert same(q, host[np.arange(p.shape[0]), light])
            seen += np.bincount(light, minlength=nl)
        assert (seen[ref.w == 0] == 0).all() and (seen > 0).sum() >= min(nl, 2)
        with pytest.raises(r.mcpt.McptError):
            dev.light_pick(1, [0], [0], 0)                               # no vertex, no pick under "tree"
        with pytest.raises(r.mcpt.McptError):
            dev.light_pick_at(1, [0], [0], 64, vp[:1], vn[:1])
        dev.set_light_sampling("one")
        with pytest.raises(r.mcpt.McptError):
            dev.light_pick_at(1, [0], [0], 0, vp[:1], vn[:1])            # the device does not pick by tree
    finally:
        dev.set_light_sampling(None)
    for bad in ([1.0] * (nl + 1), [0.0] * nl, [-1.0] + [1.0] * (nl - 1), [float("nan")] + [1.0] * (nl - 1)):
        with pytest.raises(r.mcpt.McptError):
            dev.set_light_sampling("tree", bad)
        assert dev.light_sampling()[0] == "all"


# ---------------------------------------------------------------------------------------------- (b) the anchor
@pytest.mark.parametrize("nl", [3, 10])
def test_one_hot_tree_equals_one_hot_one(rooms, nl):
    r = rooms(nl, diffuse_only=True)
    dev = r.device()
    pix, k = P._non_emitter_samples(r, 1500, 7 + nl)
    ref = dev.sample_radiance(41, pix, k)
    total = np.zeros_like(ref)
    for l in range(nl):
        e = np.zeros(nl)
        e[l] = 1.0
        dev.set_light_sampling("one", e)
        one = dev.sample_radiance(41, pix, k)
        dev.set_light_sampling("tree", e)
        tree = dev.sample_radiance(41, pix, k)
        assert same(tree, one), "light %d" % l
        total += tree
    dev.set_light_sampling(None)
    rel = np.abs(total - ref) / np.maximum(np.abs(ref), 1e-300)
    rel[ref == 0] = np.where(total[ref == 0] == 0, 0.0, np.inf)
    print("one-hot identity under the tree, %d lights: max relative difference %.3e" % (nl, rel.max()))
    assert rel.max() <= 1e-12 and (ref > 0).any(axis=1).mean() > 0.5


# ---------------------------------------------------------------------------------------------- (c) paths, counts, routes
@pytest.mark.parametrize("nl", [10, 40])
def test_same_paths_and_every_route(rooms, mcpt, nl):
    r = rooms(nl)
    spp = 4
    all_st, one_st, base_st = mcpt.Stats(), mcpt.Stats(), mcpt.Stats()
    all_img = r.device().generateImg(spp, seed=3, stats=all_st)
    r.device().set_light_sampling("one")
    one_img = r.device().generateImg(spp, seed=3, stats=one_st)
    for d in ("default",) + P.ROUTES:
        r.device(d).set_light_sampling("tree")
    try:
        base = r.device().generateImg(spp, seed=3, stats=base_st)
        assert np.isfinite(base).all() and base.sum() > 0 and not same(base, all_img) and not same(base, one_img)
        routes = {}
        st = mcpt.Stats()
        routes["megakernel"] = (r.device().generateImg(spp, seed=3, flags=mcpt.RENDER_MEGAKERNEL, stats=st), TL._counts(st), st.shadow_skipped)
        for which in P.ROUTES:
            st = mcpt.Stats()
            routes[which] = (r.device(which).generateImg(spp, seed=3, stats=st), TL._counts(st), st.shadow_skipped)
        parts = np.zeros_like(base)
        total = np.zeros(5, dtype=np.int64)
        for rank in range(3):
            st = mcpt.Stats()
            r.device().generateImg(spp, seed=3, rank=rank, world=3, img=parts, stats=st)
            total += np.array(TL._counts(st) + (st.shadow_skipped,), dtype=np.int64)
        routes["partitions"] = (parts, tuple(int(x) for x in total[:4]), int(total[4]))
        for which, (img, counts, skipped) in routes.items():
            bad = int((bits(img) != bits(base)).sum())
            assert bad == 0, "%s: %d channels differ from the default route" % (which, bad)
            assert counts == TL._counts(base_st) and skipped == base_st.shadow_skipped, (which, counts, TL._counts(base_st))
    finally:
        for d in ("default",) + P.ROUTES:
            r.device(d).set_light_sampling(None)
    a, o, t = TL._counts(all_st), TL._counts(one_st), TL._counts(base_st)
    assert t[1:] == a[1:] and t == o                                # the "all" frame's paths; one ray or one skip per vertex
    assert a[0] % nl == 0 and t[0] == a[0] // nl
    print("%d lights: skipped %d under one, %d under tree, of %d vertices" % (nl, one_st.shadow_skipped, base_st.shadow_skipped, t[0]))
    assert base_st.shadow_skipped <= one_st.shadow_skipped          # horizon culling only removes wasted picks
    assert abs(base.mean() / all_img.mean() - 1.0) < 0.1


# ---------------------------------------------------------------------------------------------- (d) unbiased
def test_tree_minus_all_has_zero_mean(rooms):
    r = rooms(10)
    dev = r.device()
    pix, k = triples(P.BLOCKS * P.BLOCK, 99)
    ref = dev.sample_radiance(5, pix, k)
    dev.set_light_sampling("tree")
    tree = dev.sample_radiance(5, pix, k)
    dev.set_light_sampling(None)
    assert np.isfinite(tree).all() and np.isfinite(ref).all()
    diff, sigma = LP.block_z(tree - ref, P.BLOCK)
    live = (sigma > 0).all(axis=1)
    print(pins_common.assert_standard_normal(diff[live], sigma[live], "tree - all, 10 lights"))


def test_a_wrong_importance_in_the_pdf_fails_the_same_test(rooms):
    """The test's power, in numpy alone, as test_a_halved_factor_fails_the_same_test: on the diffuse-only room every sample is the sum of its
    lights' parts, so part[l*] / p(l* | vertex) with l* the restatement's tree pick at the sample's first vertex is another unbiased
    estimator of it -- as long as every light has a positive probability: the light is kept for the whole path, so the vertex's normal is
    left out (pn = 0: no horizon, the distance term alone).  Dividing by the probability a WRONG importance gives (the weight without the
    distance term) while picking with the right one is biased, and the same blocks and bars say so.  Its limit is the same as the halved
    factor's: this is an estimator of the library's family, not the library's."""
    r = rooms(10, diffuse_only=True)
    dev = r.device()
    n = P.BLOCKS * P.PATH_BLOCK
    pix, k = P._non_emitter_samples(r, int(n * 1.2), 23)
    assert pix.shape[0] >= n
    pix, k = pix[:n], k[:n]
    rays = dev.camera_rays(0, pix, k)
    t = dev.ray_intersect(rays)[1]
    p = rays[:, :3] + rays[:, 3:6] * t[:, None]
    ref = dev.sample_radiance(5, pix, k)
    parts = P._per_light(dev, 10, 5, pix, k)
    tree = LT.TreeRef.of_scene(r.sc)
    u = LP.pick_uniform(5, pix, k, 0, 10)
    zero = np.zeros_like(p)
    light, pdf, _ = tree.descend(u, p, zero)
    i = np.arange(n)
    good = parts[light, i] / pdf[:, None]
    diff, sigma = LP.block_z(good - ref, P.PATH_BLOCK)
    print(pins_common.assert_standard_normal(diff, sigma, "numpy tree estimator, right probabilities"))
    light2, wrong_pdf, _ = tree.descend(u, p, zero, wrong_pdf=True)
    assert np.array_equal(light, light2) and not same(pdf, wrong_pdf)
    bad = parts[light, i] / wrong_pdf[:, None]
    diff, sigma = LP.block_z(bad - ref, P.PATH_BLOCK)
    with pytest.raises(AssertionError):
        pins_common.assert_standard_normal(diff, sigma, "numpy tree estimator, probabilities of a wrong importance")


# ---------------------------------------------------------------------------------------------- (e) it buys something
def test_lower_error_than_one_at_equal_samples(rooms):
    r = rooms(40)
    dev = r.device()
    truth = dev.generateImg(1024, seed=1)
    rmse = {}
    for mode in ("one", "tree"):
        dev.set_light_sampling(mode)
        rmse[mode] = float(np.sqrt(np.mean((dev.generateImg(16, seed=2) - truth) ** 2)))
    dev.set_light_sampling(None)
    print("40 lights, 96x64, 16 samples per pixel: RMSE one %.5f, tree %.5f, ratio %.3f" % (rmse["one"], rmse["tree"], rmse["one"] / rmse["tree"]))
    assert rmse["tree"] < rmse["one"]


# ---------------------------------------------------------------------------------------------- (f) riders
def test_progressive_and_adaptive_frames(rooms):
    dev = rooms(40).device()
    dev.set_light_sampling("tree")
    ref = dev.generateImg(16, seed=5)
    pr = dev.progressive(16, seed=5)
    for n in (1, 6, 2, 7):
        pr.step(n)
    img = pr.image()
    pr.close()
    assert same(img, ref)
    ad = dev.adaptive(16, 0.0, 0.0, min_spp=4, seed=5)
    for n in (4, 5, 7):
        ad.step(n)
    assert ad.done == 16 and ad.active == 0
    img = ad.image()
    ad.close()
    assert same(img, ref)
    dev.set_light_sampling(None)
    assert not same(dev.generateImg(16, seed=5), ref)


def test_denoised_frame_keeps_its_aovs(rooms):
    dev = rooms(10).device()
    out = {}
    for mode in ("tree", None):
        dev.set_light_sampling(mode)
        pr = dev.progressive(8, seed=5)
        pr.step(3)
        pr.step(5)
        out[mode] = (pr.denoise(), pr.image(), pr.aovs())
        pr.close()
    dn, img, aov = out["tree"]
    assert np.isfinite(dn).all() and dn.sum() > 0 and not same(dn, img) and not same(dn, out[None][0])
    for name, a in aov.items():
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(out[None][2][name]).view(np.uint8)), name


def test_lens_form_equals_the_megakernel(rooms, mcpt):
    dev = rooms(10).device()
    dev.set_light_sampling("tree")
    pin = dev.generateImg(8, seed=3)
    dev.set_lens(**TL.LENS)
    try:
        wf = dev.generateImg(8, seed=3)
        mk = dev.generateImg(8, seed=3, flags=mcpt.RENDER_MEGAKERNEL)
        pix, k = triples(500, 3)
        sr = dev.sample_radiance(3, pix, k)
    finally:
        dev.set_lens()
        dev.set_light_sampling(None)
    assert same(wf, mk) and np.isfinite(wf).all() and np.isfinite(sr).all()
    assert (bits(wf) != bits(pin)).sum() > wf.size // 4


def test_environment_keeps_its_own_plane(rooms, mcpt):
    r = rooms(10)
    sky = np.array([[[0.6, 0.7, 1.0], [0.2, 0.2, 0.3]], [[0.3, 0.25, 0.2], [0.05, 0.05, 0.1]]])
    frames = {}
    for which in ("default", "finish-lane", "no-finish"):
        dev = r.device(which)
        dev.set_environment(sky, 0.8)
        dev.set_light_sampling("tree")
        st = mcpt.Stats()
        frames[which] = dev.generateImg(4, seed=3, stats=st)
        assert 0 < st.rays_shadow <= 2 * st.shade_calls and st.rays_shadow + st.shadow_skipped <= 2 * st.shade_calls, which
        if which == "default":
            mk = dev.generateImg(4, seed=3, flags=mcpt.RENDER_MEGAKERNEL)
            assert same(mk, frames[which])
            dev.set_light_sampling("one")
            assert not same(dev.generateImg(4, seed=3), frames[which])
        dev.set_environment(None)
        dev.set_light_sampling(None)
    assert same(frames["finish-lane"], frames["default"]) and same(frames["no-finish"], frames["default"])


def _moved(r, nl):
    g, m, _ = r.sc.faces()
    v0 = np.ascontiguousarray(g[:, :9])
    v1 = np.ascontiguousarray(A.move_lights(v0, m, [r.sc.light(i)[2] for i in range(nl)], scale=1.05, shift=(0.01, -0.004, 0.006)))
    return v0, v1, m


def test_updated_device_equals_a_fresh_one(rooms, mcpt, tmp_path_factory):
    r = rooms(10)
    v0, v1, m = _moved(r, 10)
    d = A.write_moved(r.dir, r.name, v1, str(tmp_path_factory.mktemp("tree_moved")))
    sc = mcpt.Scene(d, r.name, width=W, height=H)
    assert sc.light_tree().tobytes() != r.sc.light_tree().tobytes()
    fresh = mcpt.Device(sc, 0)
    fresh.set_light_sampling("tree")
    st0 = mcpt.Stats()
    want = fresh.generateImg(4, seed=6, stats=st0)
    ref = LT.TreeRef.of_scene(sc)
    vp, vn = LT.vertex_set(ref, seed=1)
    pix, k = triples(vp.shape[0], 8)
    want_pick = ref.pick(9, pix, k, 1, vp, vn)
    wts = np.linspace(1.0, 2.0, 10)
    for first, mode in (("set", "refit"), ("update", "rebuild")):
        dev = mcpt.Device(r.sc, 0)
        if first == "set":
            dev.set_light_sampling("tree")
            dev.update_vertices(v1, mode=mode)
        else:
            dev.update_vertices(v1, mode=mode)
            dev.set_light_sampling("tree")
        light, q = dev.light_pick_at(9, pix, k, 1, vp, vn)
        assert np.array_equal(light, want_pick[0]) and same(q, want_pick[1]), first
        st = mcpt.Stats()
        img = dev.generateImg(4, seed=6, stats=st)
        assert same(img, want) and TL._counts(st) == TL._counts(st0), first
        assert same(dev.generateImg(4, seed=6, flags=mcpt.RENDER_MEGAKERNEL), want), first
        dev.set_light_sampling("tree", wts)                          # the caller's weights stay, the boxes follow the emitters
        dev.update_vertices(v0, mode=mode)
        back = LT.TreeRef.of_scene(r.sc, wts).pick(9, pix, k, 1, vp, vn)
        light, q = dev.light_pick_at(9, pix, k, 1, vp, vn)
        assert np.array_equal(light, back[0]) and same(q, back[1]), first
        dev.close()
    fresh.close()
    sc.close()


def test_motion_frame_equals_fresh_devices(rooms, mcpt, tmp_path_factory):
    r = rooms(10)
    N, K, shutter, seed = 8, 2, (0.25, 0.75), 11
    v0, v1, _ = _moved(r, 10)
    dev = mcpt.Device(r.sc, 0)
    dev.set_light_sampling("tree")
    dev.set_motion(v_end=v1, shutter=shutter, steps=K)
    img = dev.generateImg(N, seed=seed)
    pix = np.repeat(np.arange(W * H, dtype=np.int32), N)
    ks = np.tile(np.arange(N, dtype=np.int32), W * H)
    x = np.zeros((W * H, N, 3))
    for j, (k0, n) in enumerate(MR.step_ranges(N, K)):
        u = MR.shutter_time(shutter[0], shutter[1], K, j)
        d = A.write_moved(r.dir, r.name, np.ascontiguousarray(MR.blend(v0, v1, u)), str(tmp_path_factory.mktemp("tree_step")))
        sc = mcpt.Scene(d, r.name, width=W, height=H)
        fresh = mcpt.Device(sc, 0)
        fresh.set_light_sampling("tree")
        x[:, k0:k0 + n] = fresh.sample_radiance(seed, pix, ks).reshape(W * H, N, 3)[:, k0:k0 + n]
        fresh.close()
        sc.close()
    want = MR.fold(x, N).reshape(H, W, 3)
    bad = int((bits(img) != bits(want)).sum())
    assert bad == 0, "%d of %d channels differ" % (bad, img.size)
    static = mcpt.Device(r.sc, 0)
    static.set_light_sampling("tree")
    assert same(dev.sample_radiance(seed, pix[:64], ks[:64]), static.sample_radiance(seed, pix[:64], ks[:64]))     # key 0 again, its tree too
    static.close()
    dev.close()


def test_multi_device_equals_the_single_device(rooms, mcpt):
    r = rooms(10)
    dev = r.device()
    dev.set_light_sampling("tree")
    st1 = mcpt.Stats()
    ref = dev.generateImg(6, seed=4, stats=st1)
    dev.set_light_sampling(None)
    md = mcpt.MultiDevice(r.sc, devices=[0, 0], gather=mcpt.GATHER_PEER)
    md.set_light_sampling("tree")
    st = mcpt.Stats()
    img = md.generateImg(6, seed=4, stats=st)
    assert same(img, ref) and TL._counts(st) == TL._counts(st1)
    with pytest.raises(mcpt.McptError):
        md.set_light_sampling("tree", [1.0] * 9)
    assert same(md.generateImg(6, seed=4), ref)
    md.close()


def test_checkpoint_keeps_to_its_setting(rooms, mcpt, tmp_path):
    r = rooms(10)
    out = str(tmp_path) + os.sep
    kw = dict(seed=9, width=W, height=H, quiet=True, checkpoint_parts=4)
    ck = out + "frame.ckp"
    st = mcpt.Stats()
    mcpt.render_scene(r.dir, r.name, 4, output_prefix=out + "one", checkpoint=ck, light_sampling="one", stats=st, **kw)
    assert st.samples == W * H * 4
    keep = open(ck, "rb").read()
    st = mcpt.Stats()
    mcpt.render_scene(r.dir, r.name, 4, output_prefix=out + "tree", checkpoint=ck, light_sampling="tree", stats=st, **kw)
    assert st.samples == W * H * 4                                  # written under "one": not resumed under "tree"
    dev = r.device()
    dev.set_light_sampling("tree")
    want = mcpt.imshow_rgb8(dev.generateImg(4, seed=9))
    dev.set_light_sampling(None)
    from PIL import Image
    assert np.array_equal(np.array(Image.open(out + "tree-SPP4.png").convert("RGB")), want)
    st = mcpt.Stats()
    mcpt.render_scene(r.dir, r.name, 4, output_prefix=out + "again", checkpoint=ck, light_sampling="tree", stats=st, **kw)
    assert st.samples == 0                                          # ... and under "tree" its own file is
    st = mcpt.Stats()
    mcpt.render_scene(r.dir, r.name, 4, output_prefix=out + "one2", checkpoint=ck, light_sampling="one", stats=st, **kw)
    assert st.samples == W * H * 4                                  # nor the reverse
    open(ck, "wb").write(keep)
    st = mcpt.Stats()
    mcpt.render_scene(r.dir, r.name, 4, output_prefix=out + "one3", checkpoint=ck, light_sampling="one", stats=st, **kw)
    assert st.samples == 0                                          # the "one" frame's identity is what it was


# ---------------------------------------------------------------------------------------------- (g) neutral
def test_one_light_scene_and_cleared_setting_are_neutral(mcpt, rooms):
    sc = mcpt.Scene(SCENES, "cornell-box", width=80, height=60)
    dev = mcpt.Device(sc, 0)
    st0, st1 = mcpt.Stats(), mcpt.Stats()
    base = dev.generateImg(8, seed=2, stats=st0)
    dev.set_light_sampling("tree")
    assert dev.light_sampling()[0] == "tree" and dev.light_sampling()[1][0] == 1.0
    tree = dev.generateImg(8, seed=2, stats=st1)
    mk = dev.generateImg(8, seed=2, flags=mcpt.RENDER_MEGAKERNEL)
    assert same(tree, base) and same(mk, base) and TL._counts(st0) == TL._counts(st1)
    dev.close()
    sc.close()
    r = rooms(10)
    never, dev = r.device("pool"), r.device("default")
    st0, st1 = mcpt.Stats(), mcpt.Stats()
    base = never.generateImg(4, seed=3, stats=st0)
    dev.set_light_sampling("tree")
    assert not same(dev.generateImg(4, seed=3), base)
    dev.set_light_sampling(None)
    again = dev.generateImg(4, seed=3, stats=st1)
    assert same(again, base) and TL._counts(st0) == TL._counts(st1)
    assert same(dev.light_sampling()[1], np.ones(10))


def test_all_and_one_frames_are_the_parent_commits(mcpt, tmp_path):
    """frames and counts recorded on an MI355X from the commit before MCPT_LIGHTS_TREE existed: both older modes keep every bit"""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "light_modes_parent.npz"))
    w, h, spp, seed = (int(x) for x in gold["params"])
    d = str(tmp_path) + os.sep
    for nl in (10, 40):
        light_scenes.write(d, "room%d" % nl, nl, w, h)
        sc = mcpt.Scene(d, "room%d" % nl, width=w, height=h)
        dev = mcpt.Device(sc, 0)
        for mode in ("all", "one"):
            dev.set_light_sampling(mode)
            st = mcpt.Stats()
            img = dev.generateImg(spp, seed=seed, stats=st)
            assert same(img, gold["img_%s_%d" % (mode, nl)]), (nl, mode)
            assert same(dev.generateImg(spp, seed=seed, flags=mcpt.RENDER_MEGAKERNEL), img)
            counts = [st.rays_shadow, st.shadow_skipped, st.rays_bounce, st.shade_calls, st.samples]
            assert counts == [int(x) for x in gold["counts_%s_%d" % (mode, nl)]], (nl, mode)
        dev.close()
        sc.close()
