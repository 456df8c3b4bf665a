"""Not gpu: the C-ABI surface of adaptive queries and lightmaps (mcpt_query_pass_boundaries, mcpt_query_radiance_adaptive*,
mcpt_bake_lightmap_adaptive*) -- symbols, the pass boundaries against the numpy restatement (tests/adaptive_query_ref.py), every refusal
of the four device entries in the documented order with a null device, api.py's own refusals, and the restatement itself on hand-made
sample sets whose answer is known without it."""
import ctypes as C
import os

import numpy as np
import pytest

import adaptive_query_ref as A
import lightmap_ref as R
import test_lightmap_cpu as TL
import test_query_cpu as TQ
from conftest import ROOT

ERR_ARG = TQ.ERR_ARG
NAMES = ["mcpt_query_pass_boundaries", "mcpt_query_radiance_adaptive", "mcpt_query_radiance_adaptive_device", "mcpt_bake_lightmap_adaptive",
         "mcpt_bake_lightmap_adaptive_device"]
PD, P32 = TQ.PD, TQ.P32
INT_MAX = 2 ** 31 - 1
BOUNDARY_CASES = [(1, 2), (2, 2), (64, 4), (100, 16), (7, 16), (INT_MAX, 2), (INT_MAX, 2 ** 30 + 1)]

# (what the message must mention, keyword overrides of mcpt_adaptive_params), in the documented order of refusal
BAD_ADAPTIVE = [("finite", dict(rel_target=float("nan"))), ("finite", dict(rel_target=float("inf"))), ("finite", dict(rel_target=-1e-300)),
                ("finite", dict(abs_target=float("nan"))), ("finite", dict(abs_target=float("-inf"))), ("finite", dict(abs_target=-0.5)),
                ("min_spp", dict(min_spp=1)), ("min_spp", dict(min_spp=0)), ("min_spp", dict(min_spp=-7)),
                ("reserved", dict(reserved=1)), ("reserved", dict(reserved=-1))]


def _ap(mcpt, rel_target=0.1, abs_target=0.0, min_spp=4, reserved=0):
    return mcpt.AdaptiveParams(rel_target, abs_target, min_spp, reserved)


def _message(mcpt):
    return mcpt.lib().mcpt_last_error().decode()


def test_symbols_are_declared_and_exported(mcpt):
    from montecarlopathtracing_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for sym in NAMES:
        assert (sym + "(") in hdr and sym in _lib.EXPORTS and hasattr(L, sym), sym
    assert "#define MCPT_VERSION 105" in hdr and mcpt.lib().mcpt_version() == 105
    for f in ("radiance_adaptive", "irradiance_adaptive", "bake_lightmap_adaptive"):
        assert callable(getattr(mcpt.Device, f))
    assert callable(mcpt.query_pass_boundaries)
    # the gap the query and lightmap blocks named is closed; the probe block keeps its own
    assert "adaptive stopping of queries" not in hdr
    assert "bands above 2, adaptive stopping. */" in hdr
    for words in ("THERE IS NO MISS RULE", "IS, BIT FOR BIT, QUERY i OF mcpt_query_radiance WITH spp = counts[i]", "ABS_TARGET DOES",
                  "AFTER EVERY PASS BUT\n * THE LAST IT WAITS FOR THE STREAM"):
        assert words in hdr, words


@pytest.mark.parametrize("spp,min_spp", BOUNDARY_CASES)
def test_pass_boundaries_are_the_restatement(mcpt, spp, min_spp):
    L = mcpt.lib()
    want = A.boundaries(spp, min_spp)
    assert want[-1] == spp and want[0] == min(spp, min_spp) and all(b == min(2 * a, spp) for a, b in zip(want, want[1:]))
    n = L.mcpt_query_pass_boundaries(spp, min_spp, None, 0)
    assert n == len(want)
    got = np.full(n + 1, -7, dtype=np.int32)
    assert L.mcpt_query_pass_boundaries(spp, min_spp, got.ctypes.data_as(P32), n) == n
    assert got[:n].tolist() == want and got[n] == -7
    assert mcpt.query_pass_boundaries(spp, min_spp).tolist() == want
    # a list that is too short is refused and left as it was
    if n > 0:
        small = np.full(n, -7, dtype=np.int32)
        assert L.mcpt_query_pass_boundaries(spp, min_spp, small.ctypes.data_as(P32), n - 1) == ERR_ARG and "boundaries" in _message(mcpt)
        assert (small == -7).all()


def test_pass_boundaries_known_values_and_refusals(mcpt):
    assert A.boundaries(64, 4) == [4, 8, 16, 32, 64] and A.boundaries(100, 16) == [16, 32, 64, 100] and A.boundaries(7, 16) == [7]
    assert A.boundaries(1, 2) == [1] and A.boundaries(2, 2) == [2]
    assert A.boundaries(INT_MAX, 2) == [2 ** j for j in range(1, 31)] + [INT_MAX]          # 2 * 2^30 does not fit 32 bits
    assert A.boundaries(INT_MAX, 2 ** 30 + 1) == [2 ** 30 + 1, INT_MAX]
    L = mcpt.lib()
    out = np.zeros(40, dtype=np.int32)
    o = out.ctypes.data_as(P32)
    for spp, min_spp, cap, what in ((0, 4, 40, "spp"), (-1, 4, 40, "spp"), (64, 1, 40, "min_spp"), (64, 0, 40, "min_spp"), (64, -2, 40, "min_spp"),
                                    (64, 4, -1, "cap")):
        assert L.mcpt_query_pass_boundaries(spp, min_spp, o, cap) == ERR_ARG and what in _message(mcpt), (spp, min_spp, cap)
    for bad in (2.5, 2 ** 31, "4"):
        with pytest.raises(ValueError):
            mcpt.query_pass_boundaries(bad, 4)
        with pytest.raises(ValueError):
            mcpt.query_pass_boundaries(64, bad)
    with pytest.raises(mcpt.McptError) as e:
        mcpt.query_pass_boundaries(64, 1)
    assert e.value.code == ERR_ARG


def _query_calls(mcpt):
    """the two query entries with a null device: f(q, ids, n, qp, ap, mean) -> return code"""
    L = mcpt.lib()
    err, hits, counts = np.zeros((3, 3)), np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32)

    def host(q, ids, n, qp, ap, mean):
        return L.mcpt_query_radiance_adaptive(None, q.ctypes.data_as(PD) if q is not None else None, ids.ctypes.data_as(P32) if ids is not None else None, n,
                                              C.byref(qp) if qp is not None else None, C.byref(ap) if ap is not None else None,
                                              mean.ctypes.data_as(PD) if mean is not None else None, err.ctypes.data_as(PD), hits.ctypes.data_as(P32),
                                              counts.ctypes.data_as(P32), None)

    def device(q, ids, n, qp, ap, mean):
        return L.mcpt_query_radiance_adaptive_device(None, q.ctypes.data if q is not None else None, ids.ctypes.data if ids is not None else None, n,
                                                     C.byref(qp) if qp is not None else None, C.byref(ap) if ap is not None else None,
                                                     mean.ctypes.data if mean is not None else None, None, None, None, None, None)
    return host, device


def test_query_refusals_come_in_order_before_the_missing_device(mcpt):
    nd = TQ._null_device_rc(mcpt)
    host, device = _query_calls(mcpt)
    mean = np.zeros((3, 3))
    ap = _ap(mcpt)
    bad_ap = _ap(mcpt, rel_target=float("nan"), min_spp=0, reserved=3)
    # mcpt_query_radiance's own refusals, whatever the adaptive parameters are
    for what, kw in TQ.BAD_PARAMS:
        for kind, q in ((0, TQ.RAYS), (1, TQ.POINTS)):
            kw2 = dict(kind=kind)
            kw2.update(kw)
            qp = TQ._params(mcpt, **kw2)
            for call in (host, device):
                for a in (ap, bad_ap, None):
                    assert call(q, None, 3, qp, a, mean) == ERR_ARG and _message(mcpt), what
                    assert "adaptive" not in _message(mcpt) and "target" not in _message(mcpt) and "min_spp" not in _message(mcpt), (what, _message(mcpt))
    for call in (host, device):
        for n in (-1, 2 ** 31, 2 ** 40):
            assert call(TQ.RAYS, None, n, TQ._params(mcpt), bad_ap, mean) == ERR_ARG and "number of queries" in _message(mcpt)
        assert call(None, None, 3, TQ._params(mcpt), bad_ap, mean) == ERR_ARG and "null query list" in _message(mcpt)
        assert call(TQ.RAYS, None, 3, TQ._params(mcpt), bad_ap, None) == ERR_ARG and "null query list" in _message(mcpt)
        assert call(TQ.RAYS, None, 3, None, bad_ap, mean) == ERR_ARG and "null query parameters" in _message(mcpt)
    # the host form's look at the list comes before the adaptive parameters as well
    for what, kind, q, ids in TQ._bad_lists():
        assert host(q, ids, 3, TQ._params(mcpt, kind=kind), bad_ap, mean) == ERR_ARG, what
        assert "query" in _message(mcpt) and "target" not in _message(mcpt), what
    # then the adaptive parameters: null, the targets, min_spp, reserved -- each reported although everything after it is wrong too
    order = [("finite", dict(rel_target=-1.0)), ("min_spp", dict(min_spp=1)), ("reserved", dict(reserved=9))]
    for kind, q in ((0, TQ.RAYS), (1, TQ.POINTS)):
        qp = TQ._params(mcpt, kind=kind)
        for call in (host, device):
            assert call(q, None, 3, qp, None, mean) == ERR_ARG and "null adaptive parameters" in _message(mcpt)
            for what, kw in BAD_ADAPTIVE:
                assert call(q, None, 3, qp, _ap(mcpt, **kw), mean) == ERR_ARG and what in _message(mcpt), (kw, _message(mcpt))
            for i, (what, _) in enumerate(order):
                kw = {}
                for _, later in order[i:]:
                    kw.update(later)
                assert call(q, None, 3, qp, _ap(mcpt, **kw), mean) == ERR_ARG and what in _message(mcpt), (what, _message(mcpt))
            assert call(q, None, 3, qp, _ap(mcpt, abs_target=-1.0, min_spp=1), mean) == ERR_ARG and "finite" in _message(mcpt)
    # valid arguments: the missing device (or the refused null handle) is what is left to report
    ids = np.array([7, 0, INT_MAX], dtype=np.int32)
    for kind, q in ((0, TQ.RAYS), (1, TQ.POINTS)):
        for kw in (dict(), dict(flags=2), dict(spp=1, sample_base=INT_MAX - 1), dict(spp=INT_MAX), dict(seed=2 ** 64 - 1)):
            qp = TQ._params(mcpt, kind=kind, **kw)
            for a in (ap, _ap(mcpt, 0.0, 0.0, 2), _ap(mcpt, 0.0, 1e300, INT_MAX)):
                assert host(q, ids, 3, qp, a, mean) == nd and host(q, None, 3, qp, a, mean) == nd and device(q, None, 3, qp, a, mean) == nd, kw
    assert host(None, None, 0, TQ._params(mcpt), ap, None) == nd          # n == 0 needs no arrays
    assert host(None, None, 0, TQ._params(mcpt), None, None) == ERR_ARG   # ... but its parameters are still looked at


def test_lightmap_refusals_come_in_order_before_the_missing_device(mcpt):
    L = mcpt.lib()
    nd = TQ._null_device_rc(mcpt)
    uv = R.shared_chart()
    E = np.zeros((8, 8, 3))
    cnt = np.zeros((8, 8), dtype=np.int32)

    def host(lp, ap, uv6=uv, out=E):
        return L.mcpt_bake_lightmap_adaptive(None, uv6.ctypes.data_as(PD) if uv6 is not None else None, C.byref(lp) if lp is not None else None,
                                             C.byref(ap) if ap is not None else None, out.ctypes.data_as(PD) if out is not None else None, None, None, None,
                                             cnt.ctypes.data_as(P32), None)

    def device(lp, ap, out=E):
        return L.mcpt_bake_lightmap_adaptive_device(None, uv.ctypes.data, C.byref(lp) if lp is not None else None, C.byref(ap) if ap is not None else None,
                                                    out.ctypes.data if out is not None else None, None, None, None, None, None, None)

    ap = _ap(mcpt)
    bad_ap = _ap(mcpt, rel_target=float("inf"), min_spp=1, reserved=2)
    # the lightmap's own refusals first, in its order
    for what, kw in TL.BAD_PARAMS:
        for call in (host, device):
            for a in (ap, bad_ap, None):
                assert call(TL._lp(mcpt, **kw), a) == ERR_ARG and what in _message(mcpt), (kw, _message(mcpt))
    for call in (host, device):
        assert call(None, bad_ap) == ERR_ARG and "null lightmap parameters" in _message(mcpt)
        assert call(TL._lp(mcpt), bad_ap, out=None) == ERR_ARG and "irradiance" in _message(mcpt)
        # then the adaptive parameters
        assert call(TL._lp(mcpt), None) == ERR_ARG and "null adaptive parameters" in _message(mcpt)
        for what, kw in BAD_ADAPTIVE:
            assert call(TL._lp(mcpt), _ap(mcpt, **kw)) == ERR_ARG and what in _message(mcpt), (kw, _message(mcpt))
        assert call(TL._lp(mcpt), _ap(mcpt, rel_target=-1.0, min_spp=1, reserved=1)) == ERR_ARG and "finite" in _message(mcpt)
        assert call(TL._lp(mcpt), _ap(mcpt, min_spp=1, reserved=1)) == ERR_ARG and "min_spp" in _message(mcpt)
    for kw in (dict(), dict(flags=2), dict(dilate=64), dict(width=16384, height=1), dict(spp=1, sample_base=INT_MAX - 1)):
        assert host(TL._lp(mcpt, **kw), ap) == nd and device(TL._lp(mcpt, **kw), ap) == nd, kw
        assert host(TL._lp(mcpt, **kw), ap, uv6=None) == nd, kw


def test_api_refusals(mcpt):
    dev = TQ._null_dev(mcpt)
    nd = TQ._null_device_rc(mcpt)
    with pytest.raises(ValueError):
        dev.radiance_adaptive(np.zeros((3, 5)), 64, 0.1)
    with pytest.raises(ValueError):
        dev.irradiance_adaptive(np.zeros((3, 3)), np.zeros((2, 3)), 64, 0.1)
    for kw in (dict(spp=2.5), dict(spp=2 ** 31), dict(spp=64, sample_base=1.0), dict(spp=64, flags="2"), dict(spp=64, min_spp=4.0),
               dict(spp=64, min_spp=2 ** 31)):
        with pytest.raises(ValueError):
            dev.radiance_adaptive(TQ.RAYS, rel_target=0.1, **kw)
    for kw in (dict(min_spp=1.5), dict(dilate=2 ** 31), dict(spp=None)):
        args = dict(spp=64, rel_target=0.1)
        args.update(kw)
        with pytest.raises(ValueError):
            dev.bake_lightmap_adaptive(8, 8, **args)
    for kw in (dict(rel_target=-0.1), dict(rel_target=0.1, abs_target=float("nan")), dict(rel_target=0.1, min_spp=1), dict(rel_target=0.1, spp=0)):
        args = dict(spp=64)
        args.update(kw)
        for f in (lambda: dev.radiance_adaptive(TQ.RAYS, **args), lambda: dev.irradiance_adaptive(TQ.POINTS[:, :3], TQ.POINTS[:, 3:], **args),
                  lambda: dev.bake_lightmap_adaptive(8, 8, **args)):
            with pytest.raises(mcpt.McptError) as e:
                f()
            assert e.value.code == ERR_ARG and str(e.value), kw
    for f in (lambda: dev.radiance_adaptive(TQ.RAYS, 64, 0.1, 0.01, min_spp=4, seed=3, ids=[5, 6, 7], sample_base=2, flags=mcpt.RENDER_MEGAKERNEL,
                                            stats=mcpt.Stats()),
              lambda: dev.irradiance_adaptive(TQ.POINTS[:, :3], TQ.POINTS[:, 3:], 64, 0.1)):
        with pytest.raises(mcpt.McptError) as e:
            f()
        assert e.value.code == nd


# ---------------------------------------------------------------------------------------------- the restatement on hand-made samples
def _tile(sample, n, K):
    return np.tile(np.asarray(sample, dtype=np.float64), (n, K, 1))


def test_identical_samples_stop_at_the_first_boundary():
    """every sample x the same: the variance is 0 but for the rounding of the k additions behind s1 and s2 -- s2 carries at most (k + 1) u
    and s1 * s1 / k at most (2 k + 3) u of relative error, u = 2^-53, so se2 <= (3 k + 4) u / (k - 1) * x * x, which is 7e-16 x * x at
    k = 3 and less above: every rel_target from 1e-6 up stops the query at b_0, for values whose squares round as well.  The mean
    carries the k additions and the division: (k + 1) u."""
    u = 2.0 ** -53
    vals = np.array([[18.4, 15.6, 8.0], [1.0, 1.0, 1.0], [0.1, 0.7, 1e-3], [1e10, 3.3, 1e-10], [0.0, 0.0, 2.5]])
    x = np.repeat(vals[:, None, :], 64, axis=1)
    hit = np.ones((5, 64), dtype=bool)
    for rel in (1e-6, 0.2, 10.0):
        for spp, min_spp in ((64, 4), (64, 16), (50, 3)):
            counts, mean, err, hits = A.answers(x, hit, spp, min_spp, rel, 0.0)
            assert (counts == min_spp).all() and (hits == min_spp).all()
            k = min_spp
            np.testing.assert_allclose(mean, vals, rtol=(k + 1) * u, atol=0)
            assert (err <= np.sqrt((3 * k + 4) * u / (k - 1)) * vals).all()
    # min_spp above spp: one pass, no decision
    counts, mean, err, hits = A.answers(x, hit, 7, 16, 0.2, 0.0)
    assert (counts == 7).all()


def test_all_zero_samples_stop_only_under_an_absolute_target():
    x = np.zeros((3, 64, 3))
    hit = np.zeros((3, 64), dtype=bool)
    for rel in (0.0, 0.2, 1e6):
        counts, mean, err, hits = A.answers(x, hit, 64, 4, rel, 0.0)
        assert (counts == 64).all() and not mean.any() and not err.any() and not hits.any()          # 0 < 0 is false
    counts, mean, err, hits = A.answers(x, hit, 64, 4, 0.0, 1e-300)
    assert (counts == 64).all()                                                                      # abs2 underflows to 0
    for a in (1e-150, 1e-3):
        counts, mean, err, hits = A.answers(x, hit, 64, 4, 0.0, a)
        assert (counts == 4).all() and not mean.any() and not err.any()


def test_targets_of_zero_never_stop_anything():
    rng = np.random.default_rng(5)
    x = rng.random((40, 64, 3)) * 10.0 ** rng.uniform(-3, 3, size=(40, 1, 1))
    x[:5] = 2.0                                              # identical samples too: se2 = 0 is not < 0
    x[5:8] = 0.0
    hit = rng.random((40, 64)) < 0.7
    for spp, min_spp in ((64, 4), (64, 2), (37, 5)):
        counts, mean, err, hits = A.answers(x, hit, spp, min_spp, 0.0, 0.0)
        assert (counts == spp).all()
        assert np.array_equal(hits, hit[:, :spp].sum(axis=1))
        s1 = np.zeros((40, 3))
        for k in range(spp):
            s1 = s1 + x[:, k]
        assert np.array_equal(mean, s1 / spp)


def test_the_inequality_is_strict():
    """samples 1 and 3 on one channel: s1 = 4, s2 = 10, v = (10 - 16 / 2) / 1 = 2, se2 = 1; m = 2, m2 = 4.  With rel_target = 0.5 the
    threshold rel2 * m2 is exactly 1 = se2: the query goes on; one ulp more and it stops.  The same with the threshold made of abs2."""
    x = np.zeros((1, 4, 3))
    x[0, :, 0] = [1.0, 3.0, 2.0, 2.0]
    hit = np.ones((1, 4), dtype=bool)
    assert not A.stops(np.array([[4.0, 0.0, 0.0]]), np.array([[10.0, 0.0, 0.0]]), 2, 0.5, 0.0)[0]
    assert A.answers(x, hit, 4, 2, 0.5, 0.0)[0][0] == 4
    assert A.answers(x, hit, 4, 2, np.nextafter(0.5, 1.0), 0.0)[0][0] == 2
    assert A.answers(x, hit, 4, 2, np.nextafter(0.5, 0.0), 0.0)[0][0] == 4
    assert A.answers(x, hit, 4, 2, 0.0, 1.0)[0][0] == 4                     # abs2 = 1 = se2
    assert A.answers(x, hit, 4, 2, 0.0, np.nextafter(1.0, 2.0))[0][0] == 2
    # the answers of the query that stopped at 2 are the fold of its two samples
    counts, mean, err, hits = A.answers(x, hit, 4, 2, 0.6, 0.0)
    assert counts[0] == 2 and hits[0] == 2 and np.array_equal(mean[0], [2.0, 0.0, 0.0]) and np.array_equal(err[0], [1.0, 0.0, 0.0])
    # ... and of the one that went on, of all four: s1 = 8, s2 = 18, v = (18 - 16) / 3, se = sqrt(v / 4)
    counts, mean, err, hits = A.answers(x, hit, 4, 2, 0.5, 0.0)
    assert np.array_equal(mean[0], [2.0, 0.0, 0.0]) and err[0, 0] == np.sqrt(((18.0 - 64.0 / 4.0) / 3.0) / 4.0)
