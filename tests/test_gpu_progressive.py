"""GPU: progressive frames (mcpt_progressive_*, render_scene's noise target / time budget / error image).  Sample ranges add up to
the one-shot frame bit for bit under every engine and chunking; the moments, the standard error and the frame summary are exact and
deterministic; the error estimate behaves like one."""
import os

import numpy as np
import pytest

import selfcheck
from conftest import ROOT, SCENES, extra_scene_dir

pytestmark = pytest.mark.gpu

W, H, N = 160, 90, 64


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _base(name):
    return extra_scene_dir() if name == "glassroom" else SCENES


# (environment, trace mode, render flags) of every configuration the ranges are checked under
CONFIGS = {
    "pool": ({"MCPT_TRACE_ENGINE": "pool"}, 0, 0),
    "vote": ({"MCPT_TRACE_ENGINE": "vote"}, 0, 0),
    "finish-lane": ({"MCPT_FINISH_ENGINE": "lane"}, 0, 0),
    "no-finish": ({"MCPT_FINISH_PATHS": "0"}, 0, 0),
    "reference-walk": ({}, 1, 0),
    "megakernel": ({}, 0, 2),
    "small-workspace": ({"MCPT_WORKSPACE_GB": "0.016"}, 0, 0),     # 16 MiB: every pass spans several chunks
}


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("name", ["cornell-box", "veach-mis", "glassroom"])
def test_ranges_add_up_bit_for_bit(mcpt, monkeypatch, name, config):
    env, mode, flags = CONFIGS[config]
    for k in ("MCPT_TRACE_ENGINE", "MCPT_FINISH_ENGINE", "MCPT_FINISH_PATHS", "MCPT_WORKSPACE_GB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = mcpt.Scene(_base(name), name, width=W, height=H)
    dev = mcpt.Device(sc, 0)
    if mode:
        dev.set_trace_mode(mcpt.TRACE_REFERENCE)
    ref = dev.generateImg(N, seed=5, flags=flags)
    for split in ([1, 7, 24, 32], [64]):
        pr = dev.progressive(N, seed=5, flags=flags)
        for n in split:
            pr.step(n)
        assert pr.done == N
        img = pr.image()
        bad = int((_bits(img) != _bits(ref)).sum())
        assert bad == 0, "%s %s split %s: %d channels differ from the one-shot frame" % (name, config, split, bad)
        pr.close()
    dev.close()
    sc.close()


@pytest.mark.parametrize("flags", [0, 2], ids=["wavefront", "megakernel"])
def test_moments_are_exact(mcpt, flags):
    """image() = s1/24 and stderr() at done = 24, recomputed on the host from mcpt_sample_radiance in fp64 in k order: bit for bit.
    k_sample_radiance traces its primary ray with the reference walk; the closest hit (leaf, t, p) is bit-identical in both walks
    (test_gpu_parity), so its samples are the frame's samples."""
    sc = mcpt.Scene(SCENES, "cornell-box", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    pr = dev.progressive(N, seed=9, flags=flags)
    for n in (8, 16):
        pr.step(n)
    assert pr.done == 24
    img, err = pr.image(), pr.stderr()
    hit = np.flatnonzero(img.reshape(-1, 3).sum(axis=1) > 0)
    rng = np.random.default_rng(3)
    pix = np.sort(rng.choice(hit, size=min(500, hit.size), replace=False)).astype(np.int32)
    k = 24
    x = dev.sample_radiance(9, np.repeat(pix, k), np.tile(np.arange(k, dtype=np.int32), pix.size)).reshape(pix.size, k, 3)
    s1 = np.zeros((pix.size, 3))
    s2 = np.zeros((pix.size, 3))
    for i in range(k):                          # the kernel's order: s1 += x, s2 += x*x, one sample at a time
        s1 = s1 + x[:, i]
        s2 = s2 + x[:, i] * x[:, i]
    mean = s1 / k
    var = (s2 - s1 * s1 / k) / (k - 1)
    se = np.sqrt(np.where(var > 0, var, 0.0) / k)
    got_m = img.reshape(-1, 3)[pix]
    got_e = err.reshape(-1, 3)[pix]
    assert np.array_equal(_bits(got_m), _bits(mean)), np.abs(got_m - mean).max()
    assert np.array_equal(_bits(got_e), _bits(se)), np.abs(got_e - se).max()
    pr.close()
    dev.close()
    sc.close()


def test_summary_is_deterministic(mcpt):
    sc = mcpt.Scene(SCENES, "veach-mis", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    seen = []
    for split in ([32], [8, 8, 16], [32]):        # the last one on a handle of its own, like the others
        pr = dev.progressive(N, seed=2)
        for n in split:
            pr.step(n)
        nz = pr.noise()
        seen.append((nz.sum_se2, nz.sum_mean2, nz.pixels, nz.rel_error, nz.abs_rms))
        img, err = pr.image(), pr.stderr()
        pr.close()
    assert seen[0] == seen[1] == seen[2]
    se2, m2, npx, rel, ab = seen[0]
    assert npx > 0 and rel > 0
    assert abs(float((err ** 2).sum()) - se2) <= 1e-12 * se2
    assert abs(float((img ** 2).sum()) - m2) <= 1e-12 * m2
    assert abs(rel - np.sqrt(se2 / m2)) <= 1e-12 * rel and abs(ab - np.sqrt(se2 / (3 * npx))) <= 1e-12 * ab
    dev.close()
    sc.close()


def test_error_behaves(mcpt):
    """rel_error falls like 1/sqrt(k), and the standard error is calibrated: z against a frame of another seed at 4096 samples.
    Every input is seeded, so the values are fixed: the first run on an MI355X measured a ratio of 0.4963 (1/sqrt(4) = 0.5) and a median
    |z| of 0.7241 over 24351 channels (a Gaussian's is 0.674; the radiance's tails are heavier).  The bounds are pinned around those."""
    sc = mcpt.Scene(SCENES, "cornell-box", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    pr = dev.progressive(N, seed=11)
    pr.step(16)
    r16 = pr.noise().rel_error
    pr.step(48)
    r64 = pr.noise().rel_error
    est, err = pr.image(), pr.stderr()
    ref = dev.progressive(4096, seed=12)
    ref.step(4096)
    rest, rerr = ref.image(), ref.stderr()
    hit = (err > 0) & (rerr > 0)
    z = (est[hit] - rest[hit]) / np.sqrt(err[hit] ** 2 + rerr[hit] ** 2)
    med = float(np.median(np.abs(z)))
    print("rel_error 16: %.5f 64: %.5f ratio %.4f; median |z| %.4f over %d channels" % (r16, r64, r64 / r16, med, hit.sum()))
    assert 0.45 <= r64 / r16 <= 0.55
    assert 0.62 <= med <= 0.82
    for h in (pr, ref):
        h.close()
    dev.close()
    sc.close()


def test_partitions_make_the_frame(mcpt):
    sc = mcpt.Scene(SCENES, "cornell-box", width=W, height=H)
    dev = mcpt.Device(sc, 0)
    ref = dev.generateImg(N, seed=4)
    img = np.full((H, W, 3), -1.0)
    for rank in (0, 1):
        pr = dev.progressive(N, seed=4, rank=rank, world=2)
        pr.step(8)
        pr.step(56)
        assert pr.noise().pixels > 0
        pr.image(img)                      # pixels of the other rank keep what img holds
        pr.close()
    assert np.array_equal(_bits(img), _bits(ref))
    dev.close()
    sc.close()


def _pfm(path):
    data = open(path, "rb").read()
    head = data.split(b"\n", 3)
    w, h = (int(v) for v in head[1].split())
    assert head[0] == b"PF" and float(head[2]) < 0
    return np.frombuffer(head[3], dtype="<f4").reshape(h, w, 3)[::-1]


def test_render_scene_progressive(mcpt, tmp_path):
    name, spp = "cornell-box", N
    kw = dict(width=W, height=H, seed=3)
    mcpt.render_scene(SCENES, name, spp, output_prefix=str(tmp_path / "plain"), **kw)
    plain = open(tmp_path / ("plain-SPP%d.png" % spp), "rb").read()
    # a target no schedule point reaches: the whole frame, the plain call's bytes
    mcpt.render_scene(SCENES, name, spp, output_prefix=str(tmp_path / "hard"), noise_target=1e-12, **kw)
    assert open(tmp_path / ("hard-SPP%d.png" % spp), "rb").read() == plain
    # a reachable one: the rel_error of the schedule's point 16 stops the frame there
    sc = mcpt.Scene(SCENES, name, width=W, height=H)
    dev = mcpt.Device(sc, 0)
    pr = dev.progressive(spp, seed=3)
    pr.step(mcpt.progressive_next_pass(spp, 0))
    pr.step(mcpt.progressive_next_pass(spp, 8))
    assert pr.done == 16
    target = pr.noise().rel_error
    at16 = mcpt.png_bytes(mcpt.imshow_rgb8(pr.image()))
    pr.close()
    mcpt.render_scene(SCENES, name, spp, output_prefix=str(tmp_path / "easy"), noise_target=target, **kw)
    assert open(tmp_path / "easy-SPP16.png", "rb").read() == at16
    assert not os.path.exists(tmp_path / ("easy-SPP%d.png" % spp))
    # the error image alone: the same PNG, and the standard error as fp32
    mcpt.render_scene(SCENES, name, spp, output_prefix=str(tmp_path / "err"), output_flags=mcpt.OUT_ERROR_PFM, **kw)
    assert open(tmp_path / ("err-SPP%d.png" % spp), "rb").read() == plain
    pr = dev.progressive(spp, seed=3)
    pr.step(spp)
    want = pr.stderr().astype(np.float32)
    pr.close()
    got = _pfm(tmp_path / ("err-SPP%d.err.pfm" % spp))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # time budgets: one that is spent by the first pass, one that is never spent
    mcpt.render_scene(SCENES, name, spp, output_prefix=str(tmp_path / "fast"), time_budget_s=1e-9, **kw)
    assert sorted(f for f in os.listdir(tmp_path) if f.startswith("fast-")) == ["fast-SPP8.png"]
    mcpt.render_scene(SCENES, name, spp, output_prefix=str(tmp_path / "slow"), time_budget_s=1e9, **kw)
    assert open(tmp_path / ("slow-SPP%d.png" % spp), "rb").read() == plain
    dev.close()
    sc.close()


def test_kernarg_self_check_counts_no_mismatch(tmp_path):
    """The -DMCPT_PRE_CHECK build compares the WfArgs the trace kernels read through the kernarg segment (wf_kernarg_args) with their
    by-value copy at entry, over the passes of a progressive frame (sample_base != 0) and a plain one: no mismatch, and checks made."""
    code = r'''
import sys
sys.path.insert(0, %r)
import montecarlopathtracing_amd as M
sc = M.Scene(%r, "veach-mis", width=160, height=90)
for engine in ("pool", "vote"):
    import os
    os.environ["MCPT_TRACE_ENGINE"] = engine
    dev = M.Device(sc, 0)
    pr = dev.progressive(32, seed=1)
    for n in (8, 8, 16):
        pr.step(n, stats=M.Stats())
    pr.close()
    dev.generateImg(8, seed=1, stats=M.Stats())
    dev.close()
print("done")
''' % (ROOT, SCENES)
    out = selfcheck.run(code, timeout=900)
    assert out.returncode == 0 and "done" in out.stdout, out.stderr[-3000:]
    found = selfcheck.kernarg_checks(out.stderr)
    assert len(found) == 8, found
    assert all(a == 0 for a, _ in found) and all(b > 0 for _, b in found), found
