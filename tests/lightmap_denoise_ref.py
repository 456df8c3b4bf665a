"""numpy restatement of mcpt_lightmap_denoise (include/mcpt.h: lightmap denoising), written from the header: the guides of the covered
texels, the a-trous iterations in UV space and the output.  fp64 in the header's operation order (vectorised over texels, every per-texel
sum in tap order; numpy rounds every operation on its own, as the library's un-contracted code does).  Coverage, the texel list and the
dilation are tests/lightmap_ref.py's.  The GPU tests compare the kernels with it; the CPU tests check it against cases done by hand."""
import numpy as np

import lightmap_ref as L
from denoise_ref import B3, H5, _lum, _shift, unit_normals

LUM = (0.2126, 0.7152, 0.0722)
DEFAULTS = dict(iterations=5, sigma_l=2.0, sigma_p=1.0)


def guides(owner, uv6, faces27):
    """(covered [H, W] bool, p [H, W, 3], nhat [H, W, 3], h [H, W]) of a coverage map; faces27 = Scene.faces()[0]: per face v1 v2 v3,
    vn1 vn2 vn3, vt (6) and the face normal.  Everything is 0 where a texel is not covered."""
    height, width = owner.shape
    uv6 = np.asarray(uv6, dtype=np.float64).reshape(-1, 6)
    g = np.asarray(faces27, dtype=np.float64)
    v9, vn9, nrm = g[:, 0:9], g[:, 9:18], g[:, 24:27]
    texels, q6 = L.texel_list(owner, uv6, v9, vn9, nrm)
    f = owner.reshape(-1)[texels]
    with np.errstate(all="ignore"):
        e1, e2 = v9[f, 3:6] - v9[f, 0:3], v9[f, 6:9] - v9[f, 0:3]
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        a2w = np.sqrt((cx * cx + cy * cy) + cz * cz)
        a2c = L.area2_of(uv6[f].T)
        hh = np.sqrt(a2w / (np.abs(a2c) * (float(width) * float(height))))
    n = height * width
    p, nhat, h = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    p[texels], nhat[texels], h[texels] = q6[:, :3], unit_normals(q6[:, 3:]), hh
    return owner >= 0, p.reshape(height, width, 3), nhat.reshape(height, width, 3), h.reshape(height, width)


def prepare(E, E_err):
    """(e, v) of every texel: e the irradiance, v = sum_c (w_c w_c)(se_c se_c) in channel order"""
    E, E_err = np.asarray(E, dtype=np.float64), np.asarray(E_err, dtype=np.float64)
    with np.errstate(all="ignore"):
        v = np.zeros(E.shape[:2])
        for c in range(3):
            v = v + (LUM[c] * LUM[c]) * (E_err[..., c] * E_err[..., c])
    return E.copy(), v


def atrous(e, v, cov, p, nhat, h, s, sigma_l, sigma_p):
    """one iteration at step s over the covered texels: (e', v'); other texels keep e and v, which nobody reads"""
    sv, sk = np.zeros_like(v), np.zeros_like(v)
    with np.errstate(all="ignore"):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                cq, ins = _shift(cov, dx, dy, False)
                vq, _ = _shift(v, dx, dy)
                ok = cov & ins & cq
                kw = B3[dx + 1] * B3[dy + 1]
                sv = np.where(ok, sv + kw * vq, sv)
                sk = np.where(ok, sk + kw, sk)
        g = sv / sk
        lp = _lum(e)
        lden = sigma_l * np.sqrt(g) + 1e-10
        hs = h * float(s)
        sw, se, svv = np.zeros_like(v), np.zeros_like(e), np.zeros_like(v)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                cq, ins = _shift(cov, s * dx, s * dy, False)
                ok = cov & ins & cq
                eq, _ = _shift(e, s * dx, s * dy)
                vq, _ = _shift(v, s * dx, s * dy)
                if dx == 0 and dy == 0:
                    nw, dd = np.ones_like(v), np.zeros_like(v)
                else:
                    nq, _ = _shift(nhat, s * dx, s * dy)
                    pq, _ = _shift(p, s * dx, s * dy)
                    d = (nhat[..., 0] * nq[..., 0] + nhat[..., 1] * nq[..., 1]) + nhat[..., 2] * nq[..., 2]
                    nw = np.where(d > 0.0, d, 0.0)
                    for _ in range(7):
                        nw = nw * nw
                    r = pq - p
                    dist = np.sqrt((r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2])
                    t = dist / (hs * np.sqrt(float(dx * dx + dy * dy))) - 1.0
                    dd = np.where(t > 0.0, t, 0.0) / sigma_p
                dl = np.abs(_lum(eq) - lp) / lden
                w = ((H5[dx + 2] * H5[dy + 2]) * nw) * np.exp(-dd - dl)
                sw = np.where(ok, sw + w, sw)
                se = np.where(ok[..., None], se + w[..., None] * eq, se)
                svv = np.where(ok, svv + (w * w) * vq, svv)
        e2 = np.where(cov[..., None], se / sw[..., None], e)
        v2 = np.where(cov, svv / (sw * sw), v)
    return e2, v2


def denoise_guided(E, E_err, owner, guide, iterations=5, sigma_l=0.0, sigma_p=0.0, dilate=0):
    """(out [H, W, 3], owner [H, W]) from the maps, the raster's owner and guides() of it; a sigma of 0 is its default"""
    sigma_l = sigma_l if sigma_l > 0.0 else DEFAULTS["sigma_l"]
    sigma_p = sigma_p if sigma_p > 0.0 else DEFAULTS["sigma_p"]
    cov, p, nhat, h = guide
    e, v = prepare(E, E_err)
    for i in range(iterations):
        e, v = atrous(e, v, cov, p, nhat, h, 1 << i, sigma_l, sigma_p)
    out = np.where(cov[..., None], e, 0.0)
    return L.dilate(out, owner, dilate)


def denoise(E, E_err, uv6, faces27, iterations=5, sigma_l=0.0, sigma_p=0.0, dilate=0):
    """the whole call: coverage (the faces whose geometric normal has no length are skipped), guides, filter, dilation"""
    height, width = np.asarray(E).shape[:2]
    owner = L.raster(uv6, width, height, np.asarray(faces27)[:, 24:27])
    return denoise_guided(E, E_err, owner, guides(owner, uv6, faces27), iterations, sigma_l, sigma_p, dilate)


# ---- the seam scene of the CPU and GPU tests: two unit quads in the plane y = 0 whose charts share the UV edge u = 1/2.  Quad A is
# x in [0, 1]; quad B the same quad shifted by `gap` along x.  gap = 1: edge to edge in the world, as in the chart.
def two_quads(gap):
    """(v [4, 9], vn [4, 9], uv [4, 6]) of the faces A0 A1 B0 B1"""
    def quad(x0, u0):
        a, b, c, d = [x0, 0.0, 0.0], [x0 + 1.0, 0.0, 0.0], [x0 + 1.0, 0.0, 1.0], [x0, 0.0, 1.0]
        ua, ub, uc, ud = [u0, 0.0], [u0 + 0.5, 0.0], [u0 + 0.5, 1.0], [u0, 1.0]
        return [a + c + b, a + d + c], [ua + uc + ub, ua + ud + uc]
    va, ua = quad(0.0, 0.0)
    vb, ub = quad(float(gap), 0.5)
    v = np.array(va + vb, dtype=np.float64)
    vn = np.tile([0.0, 1.0, 0.0], (4, 3)).astype(np.float64)
    return v, vn, np.array(ua + ub, dtype=np.float64)


def floor_and_wall():
    """(v [4, 9], vn [4, 9], uv [4, 6]): a unit floor (y = 0, normal +y) and a unit wall (x = 1, normal -x) that meet in the edge x = 1, y = 0
    and are charted contiguously, the floor on u in [0, 1/2] and the wall on u in [1/2, 1]: positions are continuous across u = 1/2"""
    fa, fb, fc, fd = [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 1.0], [0.0, 0.0, 1.0]
    wa, wb, wc, wd = [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [1.0, 1.0, 1.0], [1.0, 0.0, 1.0]
    def chart(u0):
        ua, ub, uc, ud = [u0, 0.0], [u0 + 0.5, 0.0], [u0 + 0.5, 1.0], [u0, 1.0]
        return [ua + uc + ub, ua + ud + uc]
    v = np.array([fa + fc + fb, fa + fd + fc, wa + wc + wb, wa + wd + wc], dtype=np.float64)
    vn = np.concatenate([np.tile([0.0, 1.0, 0.0], (2, 3)), np.tile([-1.0, 0.0, 0.0], (2, 3))]).astype(np.float64)
    return v, vn, np.array(chart(0.0) + chart(0.5), dtype=np.float64)


def faces27_of(v, vn, uv):
    """what Scene.faces()[0] holds for a scene of these arrays: v, vn, vt and the geometric normal (v2 - v1) x (v3 - v1), unnormalised
    -- only its having a length matters here"""
    e1, e2 = v[:, 3:6] - v[:, 0:3], v[:, 6:9] - v[:, 0:3]
    return np.concatenate([v, vn, uv, np.cross(e1, e2)], axis=1)
