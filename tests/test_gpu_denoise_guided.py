"""GPU: the denoiser guided by sample AOVs (mcpt_progressive_denoise_guided).  The kernel is the numpy restatement (tests/guide_ref.py) on
uniform, adaptive and partitioned handles under a lens; pass-through pixels are the estimate bit for bit; the result is deterministic and
leaves the handle -- the first-hit AOVs and filter included -- as it was; what it does to the error of a frame under depth of field; and
render_scene writes what the API computes."""
import os

import numpy as np
import pytest

import guide_ref as GR
from conftest import SCENES, extra_scene_dir
from test_gpu_progressive import _pfm

pytestmark = pytest.mark.gpu

W, H = 160, 90
ODD = (157, 93)                      # partial 16 x 16 tiles on both axes
SCENE_NAMES = ["cornell-box", "veach-mis", "glassroom"]
ERR_ARG = -3
LENS = dict(jitter=True, aperture=0.02)
# test_guided_denoise_is_effective: 320 x 180, N = 16, seed 7, lens jitter + APERTURE (focused at the look_at distance), against a 4096-sample
# frame of seed 99 under the same lens; RMS error over all owned pixels, all defaults (measured on an MI355X).  Each bound is
# the measured ratio plus a quarter of its distance to 1; the mean shift's is twice the measured one, as test_gpu_denoise pins its own.
# By this measure the guided filter does NOT beat the first-hit-guided one on any of the three scenes (guided / first-hit-guided: 1.182
# cornell-box, 1.249 veach-mis, 1.150 glassroom): pixels with an emitter sample pass through unfiltered, and under an aperture those -- the
# blurred rims of the lights, radiance 40-50 at partial coverage -- carry most of the frame's squared error.  So no scene is held to that
# ratio (DESIGN 6j says so); the test prints it and asserts the ratio to the raw estimate and the mean shift.
APERTURE = {"cornell-box": 0.01, "glassroom": 0.02}
MAX_RATIO_TO_RAW = {"cornell-box": 0.9971, "glassroom": 0.9450}     # measured 0.9961, 0.9267
MAX_MEAN_SHIFT = {"cornell-box": 0.014, "glassroom": 0.044}         # measured -0.0070, -0.0219
# (K, sigma_l, sigma_z, G, sigma_a); all zero: the defaults
CASES = [(0, 0.0, 0.0, 0, 0.0), (0, 2.0, 0.0, 0, 0.0), (1, 0.0, 0.0, 3, 0.0), (5, 0.0, 0.0, 16, 0.0), (3, 1.5, 0.2, 4, 0.05)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _base(name):
    return extra_scene_dir() if name == "glassroom" else SCENES


def _open(mcpt, name, w=W, h=H, lens=LENS):
    sc = mcpt.Scene(_base(name), name, width=w, height=h)
    dev = mcpt.Device(sc, 0)
    if lens:
        dev.set_lens(**lens)
    return sc, dev


# ---- 1. the kernel against the numpy restatement, pass-through, pixels not owned
def _check_against_reference(pr, case, label):
    K, sl, sz, G, sa = case
    fill = np.full((pr.device.height, pr.device.width, 3), -7.25)
    got = pr.denoise_guided(K, sl, sz, G, sa, img=fill.copy())
    defaults = K == 0 and sl == 0.0 and sz == 0.0
    Gu = G or min(pr.spp, GR.GUIDE_SAMPLES)
    aov = pr.sample_aovs(G)
    owned = pr.sample_counts() > 0
    est, err = pr.image(), pr.stderr()
    ref = GR.denoise(est, err * err, owned, aov["counts"], aov["normal"], aov["depth"], aov["albedo"], Gu,
                     GR.DEFAULTS["iterations"] if defaults else K, sl or GR.DEFAULTS["sigma_l"], sz or GR.DEFAULTS["sigma_z"], sa or GR.SIGMA_A)
    filt = GR.filtered_pixels(aov["counts"], owned)
    assert np.array_equal(_bits(got[~owned]), _bits(fill[~owned])), label + ": pixels not owned were written"
    passthru = owned & ~filt
    assert np.array_equal(_bits(got[passthru]), _bits(est[passthru])), label + ": pass-through pixels are not the estimate"
    assert filt.sum() > 0
    rel = np.abs(got[filt] - ref[filt]) / np.maximum(np.abs(ref[filt]), 1e-300)
    assert np.all((got[filt] == ref[filt]) | (rel <= 1e-12)), "%s: max rel %.3e" % (label, rel.max())
    return got, est, filt


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_kernel_matches_numpy_uniform(mcpt, name):
    sc, dev = _open(mcpt, name)
    pr = dev.progressive(64, seed=11)
    pr.step(16)
    image = pr.image()
    for case in CASES:
        got, est, filt = _check_against_reference(pr, case, "%s uniform %r" % (name, case))
        if case[0] == 0 and case[1] != 0.0:                        # K = 0: the estimate, mcpt_progressive_image, bit for bit
            assert np.array_equal(_bits(got), _bits(image))
        else:
            assert not np.array_equal(_bits(got[filt]), _bits(est[filt]))
    counts = pr.sample_aovs()["counts"]
    assert ((counts[..., 0] > 0) & (counts[..., 0] < GR.GUIDE_SAMPLES)).any()     # partial coverage occurs


def test_kernel_matches_numpy_adaptive_odd_size(mcpt):
    sc, dev = _open(mcpt, "glassroom", *ODD)
    pr = dev.adaptive(64, 0.1, min_spp=8, seed=12)
    pr.step(8)
    if pr.active:
        pr.step(8)
    for case in CASES:
        _check_against_reference(pr, case, "adaptive %r" % (case,))


@pytest.mark.parametrize("rank", [0, 1, 2])
def test_kernel_matches_numpy_partitioned(mcpt, rank):
    """world 3: the pixels of the other ranks are absent neighbours and are not written"""
    sc, dev = _open(mcpt, "cornell-box", *ODD)
    pr = dev.progressive(32, seed=13, rank=rank, world=3)
    pr.step(8)
    owned = pr.sample_counts() > 0
    assert 0 < owned.sum() < owned.size
    for case in CASES:
        _check_against_reference(pr, case, "rank %d %r" % (rank, case))


# ---- 2. determinism, 3. the handle and the first-hit path stay as they were
def _state(pr):
    aov = pr.aovs()
    return [pr.image(), pr.stderr(), pr.sample_counts(), pr.denoise()] + [aov[k] for k in sorted(aov)], pr.noise().as_dict()


def _same_state(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a[0], b[0])) and a[1] == b[1]


def test_guided_denoise_is_deterministic_and_reads_only(mcpt):
    sc, dev = _open(mcpt, "glassroom")
    a = dev.progressive(64, seed=21)
    for n in (16, 16):
        a.step(n)
    b = dev.progressive(64, seed=21)
    for n in (8, 8, 4, 12):
        b.step(n)
    before = _state(a)
    d1 = a.denoise_guided()
    a.sample_aovs(3)
    d2 = a.denoise_guided()
    assert np.array_equal(_bits(d1), _bits(d2))
    assert np.array_equal(_bits(d1), _bits(b.denoise_guided()))
    assert _same_state(before, _state(a))
    assert not np.array_equal(_bits(d1), _bits(before[0][3]))      # not the first-hit-guided frame
    # a handle that never ran the first-hit filter before the guided one gives the same first-hit frame
    c = dev.progressive(64, seed=21)
    c.step(32)
    c.denoise_guided()
    assert np.array_equal(_bits(c.denoise()), _bits(before[0][3]))


def test_pinhole_first_hit_aovs_are_unchanged(mcpt):
    sc, dev = _open(mcpt, "cornell-box", lens=None)
    pr = dev.progressive(16, seed=22)
    pr.step(4)
    before = _state(pr)
    g = pr.denoise_guided()
    assert _same_state(before, _state(pr))
    assert not np.array_equal(_bits(g), _bits(before[0][0]))       # it filtered


# ---- 4. effectiveness
def _errors(mcpt, name, w=320, h=180, n=16, ref_spp=4096):
    sc, dev = _open(mcpt, name, w, h, lens=dict(jitter=True, aperture=APERTURE[name]))
    ref = dev.generateImg(ref_spp, seed=99)
    pr = dev.progressive(n, seed=7)
    pr.step(n)
    est, first, guided = pr.image(), pr.denoise(), pr.denoise_guided()
    rms = lambda a: float(np.sqrt(np.mean((a - ref) ** 2)))   # noqa: E731
    shift = abs(float(guided.mean()) - float(est.mean())) / float(est.mean())
    return rms(guided) / rms(first), rms(guided) / rms(est), shift


@pytest.mark.parametrize("name", sorted(APERTURE))
def test_guided_denoise_is_effective(mcpt, name):
    to_first, to_raw, shift = _errors(mcpt, name)
    print("%s: guided / first-hit-guided RMS error %.4f, guided / raw %.4f, mean shift %.4f" % (name, to_first, to_raw, shift))
    assert to_raw <= MAX_RATIO_TO_RAW[name], "%s: ratio to the estimate %.4f" % (name, to_raw)
    assert shift <= MAX_MEAN_SHIFT[name], "%s: mean shift %.4f" % (name, shift)


# ---- 5. render_scene
def test_render_scene_outputs(mcpt, tmp_path):
    name, spp = "cornell-box", 16
    kw = dict(width=W, height=H, seed=3, lens=dict(LENS))
    plain, old, full = str(tmp_path / "plain"), str(tmp_path / "old"), str(tmp_path / "full")
    mcpt.render_scene(SCENES, name, spp, output_prefix=plain, **kw)
    mcpt.render_scene(SCENES, name, spp, output_prefix=old, output_flags=mcpt.OUT_DENOISED | mcpt.OUT_PFM, **kw)
    mcpt.render_scene(SCENES, name, spp, output_prefix=full,
                      output_flags=mcpt.OUT_DENOISED | mcpt.OUT_DENOISED_SAMPLES | mcpt.OUT_SAMPLE_AOV_PFM | mcpt.OUT_PFM, **kw)
    stem = "%s-SPP%d" % (full, spp)
    data = lambda p: open(p, "rb").read()   # noqa: E731
    assert data("%s-SPP%d.png" % (plain, spp)) == data(stem + ".png")
    for ext in (".denoised.png", ".denoised.pfm", ".pfm"):
        assert data("%s-SPP%d%s" % (old, spp, ext)) == data(stem + ext), ext
    for ext in (".denoised-samples.png", ".denoised-samples.pfm", ".s-albedo.pfm", ".s-normal.pfm", ".s-depth.pfm", ".coverage.pfm"):
        assert os.path.exists(stem + ext), ext
    sc, dev = _open(mcpt, name)
    pr = dev.progressive(spp, seed=3)
    pr.step(spp)
    guided = pr.denoise_guided()
    assert np.array_equal(_pfm(stem + ".denoised-samples.pfm"), guided.astype(np.float32))
    from PIL import Image
    assert np.array_equal(np.array(Image.open(stem + ".denoised-samples.png").convert("RGB")), mcpt.imshow_rgb8(guided))
    aov = pr.sample_aovs()
    assert np.array_equal(_pfm(stem + ".s-albedo.pfm"), aov["albedo"].astype(np.float32))
    assert np.array_equal(_pfm(stem + ".s-normal.pfm"), aov["normal"].astype(np.float32))
    assert np.array_equal(_pfm(stem + ".s-depth.pfm"), np.repeat(aov["depth"].astype(np.float32)[..., None], 3, axis=2))
    assert np.array_equal(_pfm(stem + ".coverage.pfm"), (aov["counts"] / float(min(spp, GR.GUIDE_SAMPLES))).astype(np.float32))
    for flag in (mcpt.OUT_DENOISED_SAMPLES, mcpt.OUT_SAMPLE_AOV_PFM):
        for bad in (dict(checkpoint=str(tmp_path / "x.ckpt")), dict(devices=[0])):
            with pytest.raises(mcpt.McptError) as e:
                mcpt.render_scene(SCENES, name, spp, output_prefix=str(tmp_path / "bad"), output_flags=flag, **kw, **bad)
            assert e.value.code == ERR_ARG
