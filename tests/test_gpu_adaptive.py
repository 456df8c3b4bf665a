"""GPU: adaptive frames (mcpt_progressive_create_adaptive, render_scene's adaptive_min_spp).  Targets of 0 give the one-shot frame; a pixel
that stops at k holds the uniform frame's estimate at k bit for bit; the selection is exactly the documented rule; the GPU compaction
keeps order at full size; partitions, the summary and render_scene's outputs agree; and the adaptive frame spends samples better."""
import os

import numpy as np
import pytest

from conftest import SCENES, extra_scene_dir
from test_gpu_progressive import CONFIGS, _pfm

pytestmark = pytest.mark.gpu

W, H, N = 160, 90, 64


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _base(name):
    return extra_scene_dir() if name == "glassroom" else SCENES


def _open(mcpt, name, w=W, h=H):
    sc = mcpt.Scene(_base(name), name, width=w, height=h)
    return sc, mcpt.Device(sc, 0)


def _criterion(s1, s2, k, rel, ab):
    """mcpt.h's stopping rule for hit pixels after k samples, in the kernel's operation order: True = stop"""
    var = (s2 - s1 * s1 / k) / (k - 1)
    se2c = np.where(var > 0.0, var, 0.0) / k
    mean = s1 / k
    se2 = (se2c[:, 0] + se2c[:, 1]) + se2c[:, 2]
    m2 = (mean[:, 0] * mean[:, 0] + mean[:, 1] * mean[:, 1]) + mean[:, 2] * mean[:, 2]
    return se2 < (rel * rel) * m2 + ab * ab


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis", "glassroom"])
def test_zero_targets_give_the_one_shot_frame(mcpt, monkeypatch, name, config):
    env, mode, flags = CONFIGS[config]
    for k in ("MCPT_TRACE_ENGINE", "MCPT_FINISH_ENGINE", "MCPT_FINISH_PATHS", "MCPT_WORKSPACE_GB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc, dev = _open(mcpt, name)
    if mode:
        dev.set_trace_mode(mcpt.TRACE_REFERENCE)
    ref = dev.generateImg(N, seed=5, flags=flags)
    pr = dev.adaptive(N, 0.0, 0.0, min_spp=16, seed=5, flags=flags)
    for n in (16, 16, 32):
        pr.step(n)
    assert pr.done == N and pr.active == 0
    img = pr.image()
    bad = int((_bits(img) != _bits(ref)).sum())
    assert bad == 0, "%s %s: %d channels differ from the one-shot frame" % (name, config, bad)
    cnt = pr.sample_counts()
    hit = img.sum(axis=2) > 0
    assert (cnt[hit] == N).all()
    with pytest.raises(mcpt.McptError):
        pr.step(8)
    pr.close()
    dev.close()
    sc.close()


def _target_for(img, err, q):
    """a relative target at the q-quantile of the pixels' own relative errors (hit pixels)"""
    se2 = (err ** 2).sum(axis=2).ravel()
    m2 = (img ** 2).sum(axis=2).ravel()
    ok = m2 > 0
    return float(np.quantile(np.sqrt(se2[ok] / m2[ok]), q))


@pytest.mark.parametrize("name", ["cornell-box", "veach-mis"])
def test_prefix_property(mcpt, name):
    sc, dev = _open(mcpt, name)
    seed, passes = 7, (16, 16, 32)
    one_shot = dev.generateImg(N, seed=seed)
    uni = dev.progressive(N, seed=seed)
    snap = {}
    for n in passes:
        uni.step(n)
        snap[uni.done] = (uni.image(), uni.stderr())
    uni.close()
    rel = _target_for(*snap[16], q=0.35)
    pr = dev.adaptive(N, rel, 0.0, min_spp=16, seed=seed)
    for n in passes:
        pr.step(n)
    img, err, cnt = pr.image(), pr.stderr(), pr.sample_counts()
    hit = one_shot.sum(axis=2) > 0
    share = {k: float((cnt[hit] == k).mean()) for k in (16, 32, 64)}
    print("%s rel_target %.5f: share of hit pixels stopped at 16 / 32 / 64: %s" % (name, rel, share))
    assert share[16] > 0.1 and share[32] > 0.05 and share[64] > 0.1
    assert set(np.unique(cnt)) <= {16, 32, 64}
    full = cnt == N
    assert np.array_equal(_bits(img[full]), _bits(one_shot[full]))
    for k in (16, 32):
        at = cnt == k
        assert np.array_equal(_bits(img[at]), _bits(snap[k][0][at])), k
        assert np.array_equal(_bits(err[at]), _bits(snap[k][1][at])), k
    assert np.array_equal(_bits(err[full]), _bits(snap[64][1][full]))
    pr.close()
    dev.close()
    sc.close()


def test_selection_is_exactly_the_criterion(mcpt):
    """64x36, N = 64.  The first pass (4 < min_spp) keeps exactly the hit pixels; after every later pass the list equals the rule applied in
    numpy to moments recomputed from mcpt_sample_radiance in k order (test_moments_are_exact), and each stopped pixel's count is the pass
    boundary at which it stopped."""
    w, h, n_spp, seed, min_spp, ab = 64, 36, 64, 13, 8, 1e-3
    sc, dev = _open(mcpt, "veach-mis", w, h)
    npx = w * h
    pix = np.arange(npx, dtype=np.int32)
    x = dev.sample_radiance(seed, np.repeat(pix, n_spp), np.tile(np.arange(n_spp, dtype=np.int32), npx)).reshape(npx, n_spp, 3)
    s1 = np.zeros((npx, 3))
    s2 = np.zeros((npx, 3))
    mom = {}
    for i in range(n_spp):
        s1 = s1 + x[:, i]
        s2 = s2 + x[:, i] * x[:, i]
        mom[i + 1] = (s1, s2)
    # the target: the median pixel's own relative error at k = 8
    a, b = mom[8]
    var = np.maximum((b - a * a / 8) / 7, 0.0) / 8
    m2 = (a * a / 64).sum(axis=1)
    rel = float(np.median(np.sqrt(var.sum(axis=1)[m2 > 0] / m2[m2 > 0])))
    pr = dev.adaptive(n_spp, rel, ab, min_spp=min_spp, seed=seed)
    pr.step(4)
    hit_list = pr.active_pixels()
    img4 = pr.image().reshape(-1, 3)
    assert set(np.flatnonzero(img4.sum(axis=1) > 0)) <= set(hit_list.tolist())
    stopped_at = np.full(npx, -1)
    stopped_at[np.setdiff1d(pix, hit_list)] = 4
    active = hit_list
    drops = []
    for n in (4, 8, 16, 32):
        pr.step(n)
        k = pr.done
        a, b = mom[k]
        stop = _criterion(a[active], b[active], k, rel, ab)
        want = active[~stop]
        got = pr.active_pixels() if k < n_spp else want      # at N the frame is complete: active() is 0
        assert np.array_equal(got, want), (k, got.size, want.size)
        stopped_at[active[stop]] = k
        drops.append(int(stop.sum()))
        active = want
    stopped_at[active] = n_spp
    print("rel_target %.5f: stopped after 8/16/32/64: %s, at N: %d" % (rel, drops, active.size))
    assert sum(d > 0 for d in drops[:3]) >= 2
    cnt = pr.sample_counts().ravel()
    assert np.array_equal(cnt, stopped_at)
    pr.close()
    dev.close()
    sc.close()


def _keep_fractions(r8, rel, ks):
    kept, out = r8 > -1, []
    for k in ks:
        now = kept & ~(r8 * np.sqrt(8.0 / k) < rel)
        out.append(now.sum() / max(kept.sum(), 1))
        kept = now
    return out


def test_compaction_at_full_size(mcpt):
    """1280x720: the list after every pass is ascending and a subset of the previous one; the pixels whose count is `done` are exactly the
    previous list (the selection writes the count of every pixel it looks at, then drops the ones that stop).  The target
    is set from a uniform frame's errors at 8 samples so that each pass keeps a share of the list between 20 % and 80 %."""
    name, w, h, n_spp, seed = "veach-mis", 1280, 720, 512, 3
    passes = (8, 24, 96, 384)                   # k = 8, 32, 128, 512: the errors halve from pass to pass
    sc, dev = _open(mcpt, name, w, h)
    uni = dev.progressive(n_spp, seed=seed)
    uni.step(8)
    img8, err8 = uni.image(), uni.stderr()
    uni.close()
    se2 = (err8 ** 2).sum(axis=2).ravel()
    m2 = (img8 ** 2).sum(axis=2).ravel()
    r8 = np.sqrt(se2[m2 > 0] / m2[m2 > 0])
    cands = np.quantile(r8, np.linspace(0.05, 0.6, 56))
    rel = float(min(cands, key=lambda t: max(abs(f - 0.5) for f in _keep_fractions(r8, t, (8, 32, 128)))))
    pr = dev.adaptive(n_spp, rel, 0.0, min_spp=8, seed=seed)
    prev = np.arange(w * h, dtype=np.int32)
    fractions = []
    for n in passes[:-1]:
        pr.step(n)
        lst = pr.active_pixels()
        cnt = pr.sample_counts().ravel()
        assert lst.size == pr.active
        assert (np.diff(lst) > 0).all()
        assert np.isin(lst, prev).all()
        assert np.array_equal(prev, np.flatnonzero(cnt == pr.done))
        assert np.array_equal(lst, np.flatnonzero(cnt == pr.done)[np.isin(prev, lst)])
        if pr.done > 8:
            fractions.append(lst.size / prev.size)
        prev = lst
    print("rel_target %.5f: kept shares after 32 / 128: %s; after 8: %d pixels" % (rel, fractions, np.count_nonzero(cnt >= 32)))
    pr.close()
    for f in fractions:
        assert 0.2 <= f <= 0.8, fractions
    # a target every pixel meets: all stop at min_spp, and the frame is the uniform frame at min_spp
    pr = dev.adaptive(n_spp, 0.0, 1e9, min_spp=8, seed=seed)
    pr.step(8)
    assert pr.active == 0 and pr.active_pixels().size == 0
    with pytest.raises(mcpt.McptError):
        pr.step(8)
    assert np.array_equal(_bits(pr.image()), _bits(img8)) and np.array_equal(_bits(pr.stderr()), _bits(err8))
    assert (pr.sample_counts() == 8).all()
    pr.close()
    dev.close()
    sc.close()


def test_partitions_make_the_frame(mcpt):
    sc, dev = _open(mcpt, "cornell-box")
    whole = dev.adaptive(N, 0.05, 0.0, min_spp=16, seed=4)
    for n in (16, 16, 32):
        whole.step(n)
    ref_img, ref_cnt = whole.image(), whole.sample_counts()
    whole.close()
    assert len(np.unique(ref_cnt)) > 1
    img = np.full((H, W, 3), -1.0)
    cnt = np.full((H, W), -1, dtype=np.int32)
    for rank in (0, 1, 2):
        pr = dev.adaptive(N, 0.05, 0.0, min_spp=16, seed=4, rank=rank, world=3)
        for n in (16, 16, 32):
            if pr.active == 0:
                break
            pr.step(n)
        pr.image(img)
        pr.sample_counts(cnt)
        pr.close()
    assert np.array_equal(_bits(img), _bits(ref_img))
    assert np.array_equal(cnt, ref_cnt)
    dev.close()
    sc.close()


def test_summary(mcpt):
    """deterministic across handles, and the sums of image(), stderr() and the counts (all n_p < N: image() is the fp64 mean)"""
    sc, dev = _open(mcpt, "veach-mis")
    uni = dev.progressive(N, seed=2)
    uni.step(16)
    rel = _target_for(uni.image(), uni.stderr(), q=0.4)
    uni.close()
    seen = []
    for _ in range(2):
        pr = dev.adaptive(N, rel, 0.0, min_spp=16, seed=2)
        pr.step(8)
        hit_list = pr.active_pixels()               # 8 < min_spp: only the misses have stopped
        pr.step(8)
        pr.step(16)
        nz = pr.noise()
        seen.append((nz.sum_se2, nz.sum_mean2, nz.pixels, nz.rel_error, nz.abs_rms, nz.done))
        img, err, cnt = pr.image(), pr.stderr(), pr.sample_counts()
        pr.close()
    assert seen[0] == seen[1]
    se2, m2, npx, rel, ab, done = seen[0]
    assert done == 32 and npx == hit_list.size and len(np.unique(cnt.ravel()[hit_list])) == 2
    assert abs(float((err ** 2).sum()) - se2) <= 1e-12 * se2
    assert abs(float((img ** 2).sum()) - m2) <= 1e-12 * m2
    assert abs(rel - np.sqrt(se2 / m2)) <= 1e-12 * rel and abs(ab - np.sqrt(se2 / (3 * npx))) <= 1e-12 * ab
    dev.close()
    sc.close()


def _pixel_rel_errors(est, ref):
    d = np.sqrt(((est - ref) ** 2).sum(axis=2)).ravel()
    r = np.sqrt((ref ** 2).sum(axis=2)).ravel()
    ok = r > 0
    return d[ok] / r[ok]


def test_adaptive_spends_samples_better(mcpt):
    """veach-mis, N = 256, rel_target 0.1, min_spp 64: an adaptive frame and a uniform frame of no more total samples against a 4096-sample
    frame of another seed.  Every input is seeded, so the values are fixed: the first run on an MI355X measured 137.7 samples per pixel for
    the adaptive frame and a 90th-percentile per-pixel relative error of 0.1727 against 0.1897 for the uniform frame of 137 (ratio 0.910).
    The bounds are pinned around those.  (With min_spp 16 the same comparison goes the other way)"""
    N_, rel, min_spp = 256, 0.1, 64
    sc, dev = _open(mcpt, "veach-mis")
    pr = dev.adaptive(N_, rel, 0.0, min_spp=min_spp, seed=21)
    n = min_spp
    while pr.active > 0:
        pr.step(n)
        n = mcpt.progressive_next_pass(N_, pr.done)
    est, cnt = pr.image(), pr.sample_counts()
    pr.close()
    total = int(cnt.sum())
    spp_u = total // (W * H)
    uni = dev.generateImg(spp_u, seed=21)
    ref = dev.generateImg(4096, seed=22)
    pa = float(np.percentile(_pixel_rel_errors(est, ref), 90))
    pu = float(np.percentile(_pixel_rel_errors(uni, ref), 90))
    print("adaptive: %d samples (%.1f per pixel), p90 %.4f; uniform SPP %d: p90 %.4f; ratio %.4f" % (total, total / (W * H), pa, spp_u, pu, pa / pu))
    assert spp_u * W * H <= total and 130 <= total / (W * H) <= 145
    assert pa < pu
    assert 0.86 <= pa / pu <= 0.96
    dev.close()
    sc.close()


def test_render_scene_adaptive(mcpt, tmp_path):
    name, spp, min_spp = "cornell-box", N, 16
    kw = dict(width=W, height=H, seed=3)
    mcpt.render_scene(SCENES, name, spp, output_prefix=str(tmp_path / "plain"), **kw)
    plain = open(tmp_path / ("plain-SPP%d.png" % spp), "rb").read()
    mcpt.render_scene(SCENES, name, spp, output_prefix=str(tmp_path / "zero"), adaptive_min_spp=min_spp, **kw)
    assert open(tmp_path / ("zero-SPP%d.png" % spp), "rb").read() == plain
    # a target that stops some pixels: the frame is named after the largest count, the map holds every pixel's
    sc = mcpt.Scene(SCENES, name, width=W, height=H)
    dev = mcpt.Device(sc, 0)
    uni = dev.progressive(spp, seed=3)
    uni.step(min_spp)
    rel = _target_for(uni.image(), uni.stderr(), q=0.6)
    uni.close()
    pr = dev.adaptive(spp, rel, 0.0, min_spp=min_spp, seed=3)
    n = min_spp
    while pr.active > 0:
        pr.step(n)
        n = mcpt.progressive_next_pass(spp, pr.done)
    k = pr.done
    want_png = mcpt.png_bytes(mcpt.imshow_rgb8(pr.image()))
    want_cnt = pr.sample_counts()
    pr.close()
    print("render_scene adaptive: rel_target %.5f, stopped at %d, counts %s" % (rel, k, np.unique(want_cnt)))
    assert len(np.unique(want_cnt)) > 1
    mcpt.render_scene(SCENES, name, spp, output_prefix=str(tmp_path / "ad"), adaptive_min_spp=min_spp, noise_target=rel,
                      output_flags=mcpt.OUT_SPP_PFM, **kw)
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("ad-")) == ["ad-SPP%d.png" % k, "ad-SPP%d.spp.pfm" % k]
    assert open(tmp_path / ("ad-SPP%d.png" % k), "rb").read() == want_png
    got = _pfm(tmp_path / ("ad-SPP%d.spp.pfm" % k))
    for c in range(3):
        assert np.array_equal(got[:, :, c], want_cnt.astype(np.float32))
    dev.close()
    sc.close()
