"""numpy restatement of mcpt_progressive_denoise (mcpt.h): the edge-avoiding a-trous filter over the surface pixels of a progressive
frame, in fp64 with the header's operation order (vectorised over pixels, every per-pixel sum in tap order).  The GPU tests compare the
kernel with it; the CPU tests check it against hand computations."""
import numpy as np

LUM = (0.2126, 0.7152, 0.0722)
H5 = (1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16)
B3 = (0.25, 0.5, 0.25)
DEFAULTS = dict(iterations=5, sigma_l=2.0, sigma_z=0.05)


def surface_material(material, owned, emitters):
    """material where p is a surface pixel (owned, a hit, not an emitter), else -1"""
    material = np.asarray(material)
    surf = owned & (material >= 0) & ~np.isin(material, list(emitters))
    return np.where(surf, material, -1).astype(np.int64)


def unit_normals(normal):
    n = np.asarray(normal, dtype=np.float64)
    ln = np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where((ln > 0.0)[..., None], n / ln[..., None], 0.0)


def _lum(e):
    return (LUM[0] * e[..., 0] + LUM[1] * e[..., 1]) + LUM[2] * e[..., 2]


def _shift(a, dx, dy, fill=0):
    """b[y, x] = a[y + dy, x + dx] where that is inside the frame, else fill; and the inside mask"""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    inside = np.zeros((h, w), dtype=bool)
    y0, y1 = max(0, -dy), min(h, h - dy)
    x0, x1 = max(0, -dx), min(w, w - dx)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        inside[y0:y1, x0:x1] = True
    return b, inside


def demodulate(est, se2, albedo):
    a = np.where(albedo > 0.01, albedo, 0.01)
    e = est / a
    v = 0.0
    for c in range(3):
        v = v + ((LUM[c] * LUM[c]) * se2[..., c]) / (a[..., c] * a[..., c])
    return a, e, v


def atrous(e, v, smat, nhat, depth, s, sigma_l, sigma_z):
    """one iteration at step s over the surface pixels (smat >= 0): (e', v'); other pixels keep e and v"""
    surf = smat >= 0
    sv = np.zeros_like(v)
    sk = np.zeros_like(v)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            mq, ins = _shift(smat, dx, dy, -1)
            vq, _ = _shift(v, dx, dy)
            ok = surf & ins & (mq == smat)
            kw = B3[dx + 1] * B3[dy + 1]
            sv = np.where(ok, sv + kw * vq, sv)
            sk = np.where(ok, sk + kw, sk)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        g = sv / sk
        lp = _lum(e)
        lden = sigma_l * np.sqrt(g) + 1e-10
        sw = np.zeros_like(v)
        se = np.zeros_like(e)
        svv = np.zeros_like(v)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                mq, ins = _shift(smat, s * dx, s * dy, -1)
                ok = surf & ins & (mq == smat)
                eq, _ = _shift(e, s * dx, s * dy)
                vq, _ = _shift(v, s * dx, s * dy)
                if dx == 0 and dy == 0:
                    nw = np.ones_like(v)
                    dz = np.zeros_like(v)
                else:
                    nq, _ = _shift(nhat, s * dx, s * dy)
                    tq, _ = _shift(depth, s * dx, s * dy)
                    d = (nhat[..., 0] * nq[..., 0] + nhat[..., 1] * nq[..., 1]) + nhat[..., 2] * nq[..., 2]
                    nw = np.where(d > 0.0, d, 0.0)
                    for _ in range(7):
                        nw = nw * nw
                    dz = np.abs(tq - depth) / (((sigma_z * depth) * float(s)) * float(max(abs(dx), abs(dy))))
                dl = np.abs(_lum(eq) - lp) / lden
                w = ((H5[dx + 2] * H5[dy + 2]) * nw) * np.exp(-dz - dl)
                sw = np.where(ok, sw + w, sw)
                se = np.where(ok[..., None], se + w[..., None] * eq, se)
                svv = np.where(ok, svv + (w * w) * vq, svv)
        e2 = np.where(surf[..., None], se / sw[..., None], e)
        v2 = np.where(surf, svv / (sw * sw), v)
    return e2, v2


def denoise(est, se2, smat, normal, depth, albedo, iterations=5, sigma_l=2.0, sigma_z=0.05, state=False):
    """the denoised frame ([H,W,3]); smat = surface_material(...).  state=True: also (e, v) after the last iteration"""
    est = np.asarray(est, dtype=np.float64)
    out = est.copy()
    if iterations == 0:
        return (out, None, None) if state else out
    smat = np.asarray(smat)
    surf = smat >= 0
    nhat = unit_normals(normal)
    depth = np.asarray(depth, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        a, e, v = demodulate(est, np.asarray(se2, dtype=np.float64), np.asarray(albedo, dtype=np.float64))
    for i in range(iterations):
        e, v = atrous(e, v, smat, nhat, depth, 1 << i, sigma_l, sigma_z)
    out[surf] = (a * e)[surf]
    return (out, e, v) if state else out
