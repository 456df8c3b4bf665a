"""GPU: the sample AOVs of progressive frames (mcpt_progressive_sample_aovs).  Without a lens they are the first-hit AOVs; under a lens
they are the fold (tests/guide_ref.py) of the closest hits of the frame's own camera rays, rebuilt from the public seams
mcpt_camera_rays and mcpt_trace_closest; the same bits under every trace configuration, before and after samples were rendered, on
partitioned and adaptive handles; argument errors."""
import ctypes as C

import numpy as np
import pytest

import guide_ref as GR
from conftest import SCENES, extra_scene_dir
from test_gpu_progressive import CONFIGS

pytestmark = pytest.mark.gpu

W, H = 157, 93                       # partial 16 x 16 tiles on both axes
BOTH = ["cornell-box", "glassroom"]
ERR_ARG = -3
LENSES = {"jitter": dict(jitter=True), "jitter-aperture": dict(jitter=True, aperture=0.03), "aperture": dict(aperture=0.03)}
SEED = 5


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _zbits(a):
    """the bits with -0.0 taken as +0.0: a sum that starts at +0.0 never returns -0.0"""
    return _bits(np.asarray(a, dtype=np.float64) + 0.0)


def _base(name):
    return extra_scene_dir() if name == "glassroom" else SCENES


def _open(mcpt, name, w=W, h=H):
    sc = mcpt.Scene(_base(name), name, width=w, height=h)
    return sc, mcpt.Device(sc, 0)


def _materials(sc):
    """per material: kd, textured?, emitter?"""
    recs = [sc.material(m) for m in range(sc.info.num_materials)]
    kd = np.array([r[1][:3] for r in recs])
    textured = np.array([r[2][0] != 0 for r in recs])
    emitter = np.array([r[2][3] >= 0 for r in recs])
    return kd, textured, emitter


def _same(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


# ---- 1. the seam: a pinhole's G rays coincide, and the sample AOVs are the first-hit AOVs
@pytest.mark.parametrize("name", BOTH)
def test_pinhole_sample_aovs_are_the_first_hit_aovs(mcpt, name):
    sc, dev = _open(mcpt, name)
    _, _, emitter = _materials(sc)
    dev.set_lens(per_sample=True)
    pr = dev.progressive(8, seed=SEED)
    first = pr.aovs()
    hit = first["material"] >= 0
    emit = hit & emitter[np.maximum(first["material"], 0)]
    surf = hit & ~emit
    assert surf.any() and (~surf).any()
    nhat = GR.unit(first["normal"])
    for G in (1, 2):
        s = pr.sample_aovs(G)
        want = np.zeros((H, W, 3), dtype=np.int32)
        want[surf, 0] = G
        want[emit, 1] = G
        want[~hit, 2] = G
        assert np.array_equal(s["counts"], want), (name, G)
        assert np.array_equal(_bits(s["depth"][surf]), _bits(first["depth"][surf])), (name, G)
        assert np.array_equal(_bits(s["albedo"]), _bits(first["albedo"])), (name, G)       # the textured floor included
        assert np.array_equal(_zbits(s["normal"]), _zbits(nhat)), (name, G)     # the first-hit normal divided by its length
        assert np.all(s["depth"][~surf] == 0.0)
    # no lens at all, G = 3: (x + x + x) / 3 rounds twice
    dev.set_lens()
    s = dev.progressive(8, seed=SEED).sample_aovs(3)
    assert np.array_equal(s["counts"][..., 0] == 3, surf)
    for got, ref in ((s["depth"][surf], first["depth"][surf]), (s["albedo"][surf], first["albedo"][surf]), (s["normal"][surf], nhat[surf])):
        assert np.all(np.abs(got - ref) <= 4 * np.spacing(np.abs(ref)))


# ---- 2. against the public seams
def _seam_reference(sc, dev, G, owned_pix):
    """the fold of the closest hits of the camera rays of samples 0 .. G-1 of the pixels: counts, depth, normal, albedo and the mask
    of pixels none of whose surface samples hit a textured material"""
    kd, textured, emitter = _materials(sc)
    _, fmat, _ = sc.faces()
    n = owned_pix.shape[0]
    pix = np.tile(owned_pix, G)
    ks = np.repeat(np.arange(G, dtype=np.int32), n)
    face, t, _, pn = dev.ray_intersect(dev.camera_rays(SEED, pix, ks))
    mat = fmat[np.maximum(face, 0)]
    kind = np.where(face < 0, GR.MISS, np.where(emitter[mat], GR.EMITTER, GR.SURFACE)).reshape(G, n)
    counts, depth, normal, albedo = GR.fold(kind, t.reshape(G, n), kd[mat].reshape(G, n, 3), GR.unit(pn).reshape(G, n, 3))
    plain = ~((kind == GR.SURFACE) & textured[mat].reshape(G, n)).any(axis=0)
    return counts, depth, normal, albedo, plain


def _check_against_seams(mcpt, name, lens, G, spp=16):
    sc, dev = _open(mcpt, name)
    dev.set_lens(**LENSES[lens])
    pr = dev.progressive(max(spp, G), seed=SEED)
    s = pr.sample_aovs(G)
    allpix = np.arange(W * H, dtype=np.int32)
    counts, depth, normal, albedo, plain = _seam_reference(sc, dev, G, allpix)
    label = "%s %s G=%d" % (name, lens, G)
    got_c = s["counts"].reshape(-1, 3)
    assert np.array_equal(got_c, counts), "%s: %d pixels' counts differ" % (label, int((got_c != counts).any(axis=1).sum()))
    assert np.all(counts.sum(axis=1) == G)
    assert np.array_equal(_bits(s["depth"].reshape(-1)), _bits(depth)), label
    assert np.array_equal(_bits(s["albedo"].reshape(-1, 3)[plain]), _bits(albedo[plain])), label
    # shading's normal (vertex_surface) against the closest-hit normal: the same blend by another sequence of operations
    dn = np.linalg.norm(s["normal"].reshape(-1, 3) - normal, axis=1)
    assert np.all(dn <= 1e-12 * np.linalg.norm(normal, axis=1)), "%s: max %.3e" % (label, dn.max())
    assert np.all(s["normal"].reshape(-1, 3)[counts[:, 0] == 0] == 0.0)
    return counts


@pytest.mark.parametrize("G", [1, 3, 16])
@pytest.mark.parametrize("lens", sorted(LENSES))
@pytest.mark.parametrize("name", BOTH)
def test_sample_aovs_are_the_fold_of_the_public_seams(mcpt, name, lens, G):
    counts = _check_against_seams(mcpt, name, lens, G)
    if name == "cornell-box" and G == 16:                          # the lens mixes kinds within a pixel (the edge of the ceiling light)
        assert ((counts > 0).sum(axis=1) > 1).any()


def test_sample_aovs_across_the_chunk_boundary(mcpt):
    """G = 128 on 157 x 93 pixels: 1.87 M rays, two chunks of whole pixels"""
    assert W * H * 128 > 1 << 20
    _check_against_seams(mcpt, "cornell-box", "jitter-aperture", 128)


# ---- 3. invariance
@pytest.mark.parametrize("name", BOTH)
def test_sample_aovs_are_the_same_under_every_configuration(mcpt, monkeypatch, name):
    ref = None
    for config in sorted(CONFIGS):
        env, mode, flags = CONFIGS[config]
        for k in ("MCPT_TRACE_ENGINE", "MCPT_FINISH_ENGINE", "MCPT_FINISH_PATHS", "MCPT_WORKSPACE_GB"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        sc, dev = _open(mcpt, name)
        if mode:
            dev.set_trace_mode(mcpt.TRACE_REFERENCE)
        dev.set_lens(**LENSES["jitter-aperture"])
        pr = dev.progressive(8, seed=SEED, flags=flags)
        before = pr.sample_aovs(5)
        pr.step(1)
        pr.step(1)
        fresh = dev.progressive(8, seed=SEED, flags=flags)
        fresh.step(2)
        after = fresh.sample_aovs(5)
        assert _same(before, after), "%s %s: before / after two steps" % (name, config)
        if ref is None:
            ref = before
        assert _same(ref, before), "%s %s" % (name, config)


# ---- 4. partitions and adaptive handles
def test_partition_keeps_the_callers_values_and_adaptive_is_uniform(mcpt):
    sc, dev = _open(mcpt, "glassroom")
    dev.set_lens(**LENSES["jitter-aperture"])
    whole = dev.progressive(16, seed=SEED).sample_aovs(4)
    L = mcpt.lib()
    seen = np.zeros((H, W), dtype=bool)
    for rank in range(3):
        pr = dev.progressive(16, seed=SEED, rank=rank, world=3)
        owned = np.zeros(W * H, dtype=bool)
        owned[dev.scene.owned_pixels(rank, 3)] = True
        owned = owned.reshape(H, W)
        assert 0 < owned.sum() < owned.size
        counts = np.full((H, W, 3), -7, dtype=np.int32)
        depth, normal, albedo = np.full((H, W), -7.25), np.full((H, W, 3), -7.25), np.full((H, W, 3), -7.25)
        D, I = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        assert L.mcpt_progressive_sample_aovs(pr._h, 4, counts.ctypes.data_as(I), depth.ctypes.data_as(D), normal.ctypes.data_as(D),
                                              albedo.ctypes.data_as(D)) == 0
        assert np.all(counts[~owned] == -7) and np.all(depth[~owned] == -7.25) and np.all(normal[~owned] == -7.25) and np.all(albedo[~owned] == -7.25)
        assert np.array_equal(counts[owned], whole["counts"][owned]) and np.array_equal(_bits(depth[owned]), _bits(whole["depth"][owned]))
        assert np.array_equal(_bits(normal[owned]), _bits(whole["normal"][owned])) and np.array_equal(_bits(albedo[owned]), _bits(whole["albedo"][owned]))
        seen |= owned
    assert seen.all()
    ad = dev.adaptive(16, 0.1, min_spp=8, seed=SEED)
    ad.step(8)
    assert _same(ad.sample_aovs(4), whole)


# ---- 5. arguments
def test_argument_errors_and_recomputation(mcpt):
    sc, dev = _open(mcpt, "cornell-box")
    dev.set_lens(**LENSES["jitter-aperture"])
    L = mcpt.lib()
    pr = dev.progressive(6, seed=SEED)
    D, I = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    counts = np.zeros((H, W, 3), dtype=np.int32)
    depth = np.zeros((H, W))
    assert L.mcpt_progressive_sample_aovs(pr._h, 7, counts.ctypes.data_as(I), None, None, None) == ERR_ARG       # spp + 1
    assert L.mcpt_progressive_sample_aovs(pr._h, -1, counts.ctypes.data_as(I), None, None, None) == ERR_ARG
    assert L.mcpt_progressive_sample_aovs(pr._h, 6, None, None, None, None) == 0
    assert L.mcpt_progressive_sample_aovs(pr._h, 6, None, depth.ctypes.data_as(D), None, None) == 0              # every pointer NULL but one
    assert L.mcpt_progressive_sample_aovs(pr._h, 6, counts.ctypes.data_as(I), None, None, None) == 0
    assert np.all(counts.sum(axis=2) == 6) and depth.max() > 0.0
    # the default G = min(spp, 16); another G gives that G's values, and the first again
    a6, a2, d = pr.sample_aovs(6), pr.sample_aovs(2), pr.sample_aovs(0)
    assert np.all(a2["counts"].sum(axis=2) == 2) and _same(d, a6) and not np.array_equal(a2["depth"], a6["depth"])
    assert _same(pr.sample_aovs(6), a6) and _same(dev.progressive(6, seed=SEED).sample_aovs(2), a2)
    big = dev.progressive(40, seed=SEED)
    assert np.all(big.sample_aovs()["counts"].sum(axis=2) == GR.GUIDE_SAMPLES)
    # reserved != 0, a bad sigma_a and bad sample counts in the guided filter's struct
    pr.step(2)
    img = np.zeros((H, W, 3))
    ptr = img.ctypes.data_as(D)
    for bad in [(0, 1, 0.0), (7, 0, 0.0), (-1, 0, 0.0), (0, 0, -1.0), (0, 0, float("nan")), (0, 0, float("inf"))]:
        assert L.mcpt_progressive_denoise_guided(pr._h, None, C.byref(mcpt.GuideParams(*bad)), ptr) == ERR_ARG, bad
    assert L.mcpt_progressive_denoise_guided(pr._h, C.byref(mcpt.DenoiseParams(5, 1, 0.0, 0.0)), None, ptr) == ERR_ARG
    assert L.mcpt_progressive_denoise_guided(pr._h, None, None, None) == ERR_ARG
    assert L.mcpt_progressive_denoise_guided(pr._h, None, None, ptr) == 0
    one = dev.progressive(6, seed=SEED)
    one.step(1)
    assert L.mcpt_progressive_denoise_guided(one._h, None, None, ptr) == ERR_ARG                                 # done < 2
    # a handle under a motion
    dev2 = _open(mcpt, "cornell-box")[1]
    dev2.set_motion(steps=2)
    mo = dev2.progressive(6, seed=SEED)
    assert L.mcpt_progressive_sample_aovs(mo._h, 2, counts.ctypes.data_as(I), None, None, None) == ERR_ARG
    mo.step(6)
    assert L.mcpt_progressive_denoise_guided(mo._h, None, None, ptr) == ERR_ARG
