"""-m gpu: the display transform on the GPU (include/mcpt.h: display transform).  The histogram kernel's counts are the numpy restatement's
(tests/display_ref.py) integer for integer, on frames that sit on the bin edges and on renders; the map's bytes are mcpt_display_host's and
the restatement's for every curve, both transfers, RGB and RGBA, the dword and the byte store path; a partitioned handle counts and writes
its owned pixels only; the denoised sources are the denoisers' frames; the handle is left as it was; and render_scene writes what the API
computes."""
import ctypes as C

import numpy as np
import pytest

import display_ref as DR
from conftest import SCENES, extra_scene_dir

pytestmark = pytest.mark.gpu

W, H = 160, 90
ODD = (157, 93)
SIZES = (1, 3, 4, 5, 255, 256, 257, 1023)      # shorter than one lane's four pixels, every tail length, one block and one pixel more, many blocks
CURVES = {"clamp": DR.CLAMP, "reinhard": DR.REINHARD, "filmic": DR.FILMIC}
TRANSFERS = {"linear": DR.LINEAR, "srgb": DR.SRGB}
SKY = [0.5, 0.7, 1.0]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _open(mcpt, name, w=W, h=H, sky=None, lens=None):
    sc = mcpt.Scene(extra_scene_dir() if name == "glassroom" else SCENES, name, width=w, height=h)
    dev = mcpt.Device(sc, 0)
    if sky is not None:
        dev.set_environment(sky)
    if lens:
        dev.set_lens(**lens)
    return sc, dev


@pytest.fixture(scope="module")
def device(mcpt):
    sc, dev = _open(mcpt, "cornell-box")
    yield dev
    dev.close()
    sc.close()


@pytest.fixture(scope="module")
def frame():
    return DR.log_uniform_frame(H, W, 20240607)


def _same_bytes(got, want, mask, label):
    """exact where the reference says the byte does not hang on pow's last bits (everywhere under the linear transfer)"""
    left_out = int((~mask).sum())
    assert left_out <= 1e-4 * mask.size, (label, left_out)                   # on the reference alone, before anything is compared
    g, w = got[..., :3], want[..., :3]
    assert np.array_equal(g[mask], w[mask]), (label, int((g != w)[mask].sum()))
    if got.shape[-1] == 4:
        assert np.all(got[..., 3] == 255), label


# ---- 1. histogram
@pytest.mark.parametrize("n", SIZES)
def test_histogram_of_edge_frames(device, n):
    img = DR.edge_frame(n, 100 + n)
    want = DR.histogram(img)
    got = device.luminance_histogram(img)
    assert got.dtype == np.int64 and got.sum() == n and np.array_equal(got, want), np.flatnonzero(got != want)
    # one repeated value: every lane of every block hits one LDS slot
    same = np.tile(np.array([[0.3, 0.6, 0.9]]), (n, 1))
    got = device.luminance_histogram(same)
    assert np.array_equal(got, DR.histogram(same)) and got.max() == n
    # the second call starts from cleared slots
    assert np.array_equal(device.luminance_histogram(img), want)


def test_histogram_of_edge_frames_covers_the_special_slots():
    img = DR.edge_frame(1023, 100 + 1023)
    s = DR.histogram(img)
    assert s[0] >= 5 and s[1] >= 3 and s[DR.SLOTS - 1] >= 3 and s[2] >= 1 and s[DR.SLOTS - 2] >= 1 and (s[2:-1] > 0).sum() > 100


@pytest.mark.parametrize("name", ["cornell-box", "glassroom"])
def test_histogram_of_renders(mcpt, name):
    sc, dev = _open(mcpt, name, *ODD, sky=SKY)
    img = dev.generateImg(4, seed=3)
    got = dev.luminance_histogram(img)
    assert np.array_equal(got, DR.histogram(img)) and got.sum() == ODD[0] * ODD[1] and (got[2:-1] > 0).sum() > 8
    dev.close()
    sc.close()


# ---- 2. map
def _check_map(mcpt, device, img, curve, transfer, rgba, label, **kw):
    got, info = device.display(img, curve=curve, transfer=transfer, rgba=rgba, **kw)
    host, hinfo = mcpt.display_host(img, curve=curve, transfer=transfer, rgba=rgba, **kw)
    assert info["counted"] == hinfo["counted"] and info["skipped"] == hinfo["skipped"] and info["l_percentile"] == hinfo["l_percentile"]
    assert info == hinfo, (label, info, hinfo)                     # (the exposure is resolved on the host from integer counts in both forms)
    want, mask = DR.display(img, info["exposure"], info["white"], CURVES[curve], TRANSFERS[transfer], rgba=rgba)
    assert got.shape == want.shape == host.shape
    _same_bytes(got, want, mask, label + " vs numpy")
    _same_bytes(got, host, mask, label + " vs host")
    if transfer == "linear":
        assert np.array_equal(got, host) and np.array_equal(got, want), label
    return got, info


@pytest.mark.parametrize("transfer", ["linear", "srgb"])
@pytest.mark.parametrize("curve", ["clamp", "reinhard", "filmic"])
def test_map_is_the_host_form_and_the_reference(mcpt, device, frame, curve, transfer):
    for rgba in (False, True):
        for n in SIZES:
            img = DR.edge_frame(n, 300 + n)
            _check_map(mcpt, device, img, curve, transfer, rgba, "%s %s n=%d rgba=%d" % (curve, transfer, n, rgba), exposure=0.75, white=3.0)
        got, info = _check_map(mcpt, device, frame, curve, transfer, rgba, "%s %s frame auto" % (curve, transfer), auto_key=0.18)
        assert info["counted"] == W * H and info["exposure"] != 1.0 and len(np.unique(got[..., :3])) > 100
    odd = DR.log_uniform_frame(ODD[1], ODD[0], 5)                 # 14601 pixels: a one-pixel tail
    _check_map(mcpt, device, odd, curve, transfer, False, "%s %s odd" % (curve, transfer), exposure=4.0, auto_key=0.18, percentile=0.9)


def test_zero_parameters_are_imshow(mcpt, device, frame):
    for img in (frame, DR.edge_frame(1023, 8).reshape(3, 341, 3), DR.edge_frame(5, 8)):
        got, info = device.display(img)
        assert np.array_equal(got, mcpt.imshow_rgb8(np.where(np.isnan(img), 0.0, img)))
        assert np.array_equal(got, mcpt.display_host(img)[0]) and info["exposure"] == 1.0 and info["counted"] == 0
    plain = np.random.default_rng(3).uniform(-0.5, 1.5, size=(H, W, 3))
    assert np.array_equal(device.display(plain)[0], mcpt.imshow_rgb8(plain))


@pytest.fixture(scope="module")
def hip(mcpt):
    h = C.CDLL(mcpt.hip_runtime_path().split(", ")[0])
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    h.hipFree.argtypes = [C.c_void_p]
    h.hipDeviceSynchronize.argtypes = []
    return h


@pytest.mark.parametrize("rgba", [False, True])
def test_output_offset_by_one_byte(mcpt, device, hip, rgba):
    """an output pointer that is not aligned takes the byte-store path: the same bytes, and nothing outside them"""
    bpp = 4 if rgba else 3
    for n in (5, 1023):
        img = DR.edge_frame(n, 500 + n)
        want, _ = device.display(img, curve="filmic", transfer="srgb", rgba=rgba, exposure=0.5)
        d_img, d_out = C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(d_img), img.nbytes) == 0 and hip.hipMalloc(C.byref(d_out), n * bpp + 32) == 0
        assert hip.hipMemcpy(d_img, img.ctypes.data_as(C.c_void_p), img.nbytes, 1) == 0
        for offset in (0, 1, 4):                                          # 4: aligned for RGB dwords, not for RGBA's 16-byte stores
            assert hip.hipMemset(d_out, 0xA5, n * bpp + 32) == 0
            device.display_device(d_img.value, n, d_out.value + offset, curve="filmic", transfer="srgb", rgba=rgba, exposure=0.5)
            assert hip.hipDeviceSynchronize() == 0
            back = np.zeros(n * bpp + 32, dtype=np.uint8)
            assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), d_out, back.nbytes, 2) == 0
            assert np.array_equal(back[offset:offset + n * bpp], want.reshape(-1)), (n, offset)
            assert np.all(back[:offset] == 0xA5) and np.all(back[offset + n * bpp:] == 0xA5), (n, offset)
        assert hip.hipFree(d_img) == 0 and hip.hipFree(d_out) == 0


# ---- 3. a partitioned handle: its owned pixels only
@pytest.mark.parametrize("rgba", [False, True])
def test_partitioned_handle_counts_and_writes_owned_pixels_only(mcpt, rgba):
    sc, dev = _open(mcpt, "cornell-box", *ODD, sky=SKY)
    pr = dev.progressive(8, seed=4, rank=1, world=3)
    pr.step(8)
    owned = np.zeros(ODD[0] * ODD[1], dtype=bool)
    owned[sc.owned_pixels(rank=1, world=3)] = True
    owned = owned.reshape(ODD[1], ODD[0])
    assert 0 < owned.sum() < owned.size
    est = pr.image()
    fill = np.full((ODD[1], ODD[0], 4 if rgba else 3), 0xA5, dtype=np.uint8)
    got, info = pr.display(out=fill.copy(), auto_key=0.18, curve="reinhard", rgba=rgba)
    slots = DR.histogram(est[owned])
    la, lp = DR.exposure(slots)
    assert info["counted"] == int(slots[1:].sum()) and info["skipped"] == int(slots[0]) and info["counted"] + info["skipped"] == owned.sum()
    assert info["l_percentile"] == lp and abs(info["log_average"] - la) <= 1e-12 * la
    # (a histogram of the whole scratch frame would count the zeros of the pixels not owned as skipped)
    want, _ = DR.display(est, info["exposure"], info["white"], DR.REINHARD, DR.LINEAR, rgba=rgba)
    assert np.array_equal(got[owned], want[owned])
    assert np.all(got[~owned] == 0xA5)                                    # every other byte, alpha bytes included
    assert np.array_equal(got[owned], mcpt.display_host(est[owned], exposure=info["exposure"], white=info["white"], curve="reinhard", rgba=rgba)[0])
    pr.close()
    dev.close()
    sc.close()


# ---- 4. sources, and the handle stays as it was
def _state(pr):
    nz = pr.noise()
    return [_bits(pr.image()), _bits(pr.stderr()), pr.sample_counts().copy(), _bits([nz.sum_se2, nz.sum_mean2, nz.rel_error]), pr.done]


def _same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_sources_and_handle_state(mcpt):
    sc, dev = _open(mcpt, "cornell-box", sky=SKY)
    pr = dev.progressive(16, seed=6)
    pr.step(8)
    before = _state(pr)
    kw = dict(auto_key=0.18, curve="filmic")
    est, info = pr.display(**kw)
    assert info["counted"] + info["skipped"] == W * H
    assert np.array_equal(est, mcpt.display_host(pr.image(), **kw)[0]) and np.array_equal(est, pr.display("estimate", **kw)[0])
    dn, _ = pr.display("denoised", **kw)
    assert np.array_equal(dn, mcpt.display_host(pr.denoise(), **kw)[0]) and not np.array_equal(dn, est)
    assert np.array_equal(dn, pr.display("denoised", **kw)[0])
    rgba, _ = pr.display("denoised", rgba=True, **kw)
    assert np.array_equal(rgba[..., :3], dn) and np.all(rgba[..., 3] == 255)
    assert np.array_equal(pr.display()[0], mcpt.imshow_rgb8(pr.image()))               # no parameters: imshow's bytes
    assert _same_state(before, _state(pr))
    pr.step(8)                                                                          # the frame goes on, and completes as the one-shot frame
    assert np.array_equal(_bits(pr.image()), _bits(dev.generateImg(16, seed=6)))
    with pytest.raises(KeyError):
        pr.display("albedo")
    with pytest.raises(mcpt.McptError) as e:
        pr.display(7)
    assert e.value.code == -3
    pr.close()
    one = dev.progressive(4, seed=6)
    one.step(1)
    with pytest.raises(mcpt.McptError) as e:                                            # the denoiser's own refusal: no variance estimate yet
        one.display("denoised")
    assert e.value.code == -3
    one.close()
    dev.close()
    sc.close()


def test_guided_source_on_a_lens_frame(mcpt):
    sc, dev = _open(mcpt, "cornell-box", lens=dict(jitter=True, aperture=0.02))
    pr = dev.progressive(16, seed=2)
    pr.step(16)
    before = _state(pr)
    kw = dict(exposure=1.5, curve="reinhard", transfer="linear")
    got, info = pr.display("denoised_guided", **kw)
    want, hinfo = mcpt.display_host(pr.denoise_guided(), **kw)
    assert np.array_equal(got, want) and info == hinfo and info["white"] >= 1.0
    assert np.array_equal(got, pr.display("denoised_guided", **kw)[0])
    assert not np.array_equal(got, pr.display("estimate", **kw)[0])
    assert _same_state(before, _state(pr))
    pr.close()
    dev.close()
    sc.close()


# ---- 5. render_scene
def test_render_scene_display(mcpt, tmp_path):
    from PIL import Image
    out = str(tmp_path) + "/"
    sky = out + "sky.pfm"
    mcpt.write_pfm(sky, np.tile(np.array([[SKY]]), (1, 1, 1)))
    kw = dict(seed=9, width=64, height=36, quiet=True, environment=sky, environment_scale=3.0)
    mcpt.render_scene(SCENES, "cornell-box", 4, output_prefix=out + "plain", output_flags=mcpt.OUT_PFM, **kw)
    mcpt.render_scene(SCENES, "cornell-box", 4, output_prefix=out + "none", output_flags=mcpt.OUT_PFM, display=None, **kw)
    assert open(out + "plain-SPP4.png", "rb").read() == open(out + "none-SPP4.png", "rb").read()
    # all-zero parameters: the same bytes again
    mcpt.render_scene(SCENES, "cornell-box", 4, output_prefix=out + "zero", display={}, **kw)
    assert open(out + "plain-SPP4.png", "rb").read() == open(out + "zero-SPP4.png", "rb").read()
    disp = dict(auto_key=0.18, curve="filmic", transfer="srgb")
    mcpt.render_scene(SCENES, "cornell-box", 4, output_prefix=out + "tone", output_flags=mcpt.OUT_PFM | mcpt.OUT_DENOISED, display=disp, **kw)
    assert open(out + "tone-SPP4.pfm", "rb").read() == open(out + "plain-SPP4.pfm", "rb").read()      # the PFM stays linear
    sc = mcpt.Scene(SCENES, "cornell-box", width=64, height=36)
    dev = mcpt.Device(sc, 0)
    dev.set_environment(mcpt.read_pfm(sky), 3.0)
    pr = dev.progressive(4, seed=9)
    pr.step(4)
    want, info = pr.display(**disp)
    png = np.array(Image.open(out + "tone-SPP4.png").convert("RGB"))
    assert np.array_equal(png, want) and info["exposure"] != 1.0
    assert not np.array_equal(png, np.array(Image.open(out + "plain-SPP4.png").convert("RGB")))
    dn = np.array(Image.open(out + "tone-SPP4.denoised.png").convert("RGB"))
    assert np.array_equal(dn, pr.display("denoised", **disp)[0])
    with pytest.raises(mcpt.McptError) as e:
        mcpt.render_scene(SCENES, "cornell-box", 4, output_prefix=out + "bad", display=dict(rgba=True), **kw)
    assert e.value.code == -3
    pr.close()
    dev.close()
    sc.close()
