"""numpy restatement of the sample AOVs (mcpt_progressive_sample_aovs) and of the filter they guide (mcpt_progressive_denoise_guided), in
fp64 with the header's operation order: the fold sums a pixel's samples sequentially in k order, the filter is denoise_ref's with the
material test dropped and the albedo term A in the weight.  The GPU tests compare the kernels with it; the CPU tests check it against
denoise_ref and hand computations."""
import numpy as np

import denoise_ref as R

MISS, EMITTER, SURFACE = 0, 1, 2
GUIDE_SAMPLES = 16
SIGMA_A = 0.2
DEFAULTS = dict(R.DEFAULTS, samples=GUIDE_SAMPLES, sigma_a=SIGMA_A)


def unit(pn):
    """pn / |pn| with the length sqrt((x x + y y) + z z); a zero vector stays 0"""
    return R.unit_normals(pn)


def fold(kind, t, kd, nhat):
    """per-sample arrays [G, ...] (kind: MISS / EMITTER / SURFACE; t [G, ...], kd and nhat [G, ..., 3]) -> counts [..., 3] int32 (ns, ne,
    nm), depth, normal, albedo: sequential sums over the surface samples in k order, each divided by ns (0 where ns == 0)"""
    kind = np.asarray(kind)
    G = kind.shape[0]
    shape = kind.shape[1:]
    ns = np.zeros(shape, dtype=np.int32)
    ne = np.zeros(shape, dtype=np.int32)
    nm = np.zeros(shape, dtype=np.int32)
    st = np.zeros(shape)
    sk = np.zeros(shape + (3,))
    sn = np.zeros(shape + (3,))
    for k in range(G):
        s = kind[k] == SURFACE
        ns += s
        ne += kind[k] == EMITTER
        nm += kind[k] == MISS
        st = np.where(s, st + t[k], st)
        sk = np.where(s[..., None], sk + kd[k], sk)
        sn = np.where(s[..., None], sn + nhat[k], sn)
    d = np.maximum(ns, 1).astype(np.float64)
    some = ns > 0
    depth = np.where(some, st / d, 0.0)
    albedo = np.where(some[..., None], sk / d[..., None], 0.0)
    normal = np.where(some[..., None], sn / d[..., None], 0.0)
    return np.stack([ns, ne, nm], axis=-1).astype(np.int32), depth, normal, albedo


def filtered_pixels(counts, owned):
    counts = np.asarray(counts)
    return np.asarray(owned, dtype=bool) & (counts[..., 0] > 0) & (counts[..., 1] == 0)


def demodulation(counts, albedo, G):
    """m = max((ns / G) * albedo, 0.01) per channel"""
    cov = np.asarray(counts)[..., 0].astype(np.float64) / float(G)
    m = cov[..., None] * np.asarray(albedo, dtype=np.float64)
    return np.where(m > 0.01, m, 0.01)


def atrous(e, v, filt, nhat, depth, m, s, sigma_l, sigma_z, sigma_a):
    """one iteration at step s over the filtered pixels: (e', v'); other pixels keep e and v"""
    sv = np.zeros_like(v)
    sk = np.zeros_like(v)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            fq, ins = R._shift(filt, dx, dy, False)
            vq, _ = R._shift(v, dx, dy)
            ok = filt & ins & fq
            kw = R.B3[dx + 1] * R.B3[dy + 1]
            sv = np.where(ok, sv + kw * vq, sv)
            sk = np.where(ok, sk + kw, sk)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        g = sv / sk
        lp = R._lum(e)
        lden = sigma_l * np.sqrt(g) + 1e-10
        sw = np.zeros_like(v)
        se = np.zeros_like(e)
        svv = np.zeros_like(v)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                fq, ins = R._shift(filt, s * dx, s * dy, False)
                ok = filt & ins & fq
                eq, _ = R._shift(e, s * dx, s * dy)
                vq, _ = R._shift(v, s * dx, s * dy)
                if dx == 0 and dy == 0:
                    nw = np.ones_like(v)
                    dz = np.zeros_like(v)
                    da = np.zeros_like(v)
                else:
                    nq, _ = R._shift(nhat, s * dx, s * dy)
                    tq, _ = R._shift(depth, s * dx, s * dy)
                    mq, _ = R._shift(m, s * dx, s * dy)
                    d = (nhat[..., 0] * nq[..., 0] + nhat[..., 1] * nq[..., 1]) + nhat[..., 2] * nq[..., 2]
                    nw = np.where(d > 0.0, d, 0.0)
                    for _ in range(7):
                        nw = nw * nw
                    dz = np.abs(tq - depth) / (((sigma_z * depth) * float(s)) * float(max(abs(dx), abs(dy))))
                    da = ((np.abs(mq[..., 0] - m[..., 0]) + np.abs(mq[..., 1] - m[..., 1])) + np.abs(mq[..., 2] - m[..., 2])) / sigma_a
                dl = np.abs(R._lum(eq) - lp) / lden
                w = ((R.H5[dx + 2] * R.H5[dy + 2]) * nw) * np.exp((-dz - dl) - da)
                sw = np.where(ok, sw + w, sw)
                se = np.where(ok[..., None], se + w[..., None] * eq, se)
                svv = np.where(ok, svv + (w * w) * vq, svv)
        e2 = np.where(filt[..., None], se / sw[..., None], e)
        v2 = np.where(filt, svv / (sw * sw), v)
    return e2, v2


def denoise(est, se2, owned, counts, normal, depth, albedo, G, iterations=5, sigma_l=2.0, sigma_z=0.05, sigma_a=SIGMA_A):
    """the guided filter's frame ([H,W,3]) from the estimate, its squared standard error, the owned mask and the sample AOVs of G samples"""
    est = np.asarray(est, dtype=np.float64)
    out = est.copy()
    if iterations == 0:
        return out
    filt = filtered_pixels(counts, owned)
    nhat = unit(normal)
    depth = np.asarray(depth, dtype=np.float64)
    m = demodulation(counts, albedo, G)
    se2 = np.asarray(se2, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = est / m
        v = 0.0
        for c in range(3):
            v = v + ((R.LUM[c] * R.LUM[c]) * se2[..., c]) / (m[..., c] * m[..., c])
    for i in range(iterations):
        e, v = atrous(e, v, filt, nhat, depth, m, 1 << i, sigma_l, sigma_z, sigma_a)
    out[filt] = (m * e)[filt]
    return out
