"""Direct light from a caller's own lights (include/mcpt.h: direct light) restated in numpy, expression by expression in the header's
order: the slots of a list (rays, limits, factors g: what mcpt_direct_rays writes) and the fold of factors and occlusion bytes (what
mcpt_direct_fold_host and the fused kernel compute).  fp64 throughout; only + - * / and sqrt enter, all of them correctly rounded in
numpy as on the device, so the comparisons are bit for bit.  The rectangle's uniforms are lens_ref's Philox at depth 0xFFFE, block l; n^
is query_ref's."""
import numpy as np

import lens_ref
import query_ref

POINT, SPOT, DIRECTIONAL, RECT = 0, 1, 2, 3
TWO_SIDED = 1
DIRECT_RNG_DEPTH = 0xFFFE


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _len(a):
    a = np.asarray(a, dtype=np.float64)
    return np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])


def _cross(a, b):
    return np.array([a[1] * b[2] - b[1] * a[2], b[0] * a[2] - a[0] * b[2], a[0] * b[1] - b[0] * a[1]])


def _f(L, name):
    return np.array(list(getattr(L, name)), dtype=np.float64)


def light_slots(L, spp):
    return spp if L.type == RECT else 1


def slots(lights, spp):
    return sum(light_slots(L, spp) for L in lights)


def uniforms(seed, ids, k, l):
    """xi1, xi2 of sample k of light l for the entries with ids `ids`: words 0 and 1 of the block (id, k, 0xFFFE << 16 | l, 'MCPT')"""
    ids = np.asarray(ids, dtype=np.uint64)
    w = lens_ref.philox4x32_10(ids, np.full(ids.shape, k, dtype=np.uint64), np.full(ids.shape, (DIRECT_RNG_DEPTH << 16) | l, dtype=np.uint64),
                               np.full(ids.shape, 0x4D435054, dtype=np.uint64), int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    return [(x.astype(np.float64) + 0.5) * 2.0 ** -32 for x in w[:2]]


def _slot(L, l, a, nh, ids, bias, seed, k):
    """the slot of light L (index l), sample index k, for every entry: (rays [n, 6], tmax [n], g [n])"""
    n = a.shape[0]
    bias = np.float64(bias)
    with np.errstate(all="ignore"):
        if L.type == DIRECTIONAL:
            d = _f(L, "direction")
            w = np.broadcast_to(-(d / _len(d)), (n, 3))
            cr = _dot(nh, w)
            ok = cr > 0.0
            g = cr
            tmax = np.full(n, np.inf)
        else:
            p = _f(L, "position")
            if L.type == RECT:
                u, v = _f(L, "u"), _f(L, "v")
                N = _cross(u, v)
                A = _len(N)
                Nh = N / A
                xi1, xi2 = uniforms(seed, ids, k, l)
                y = (p[None, :] + u[None, :] * xi1[:, None]) + v[None, :] * xi2[:, None]
            else:
                y = np.broadcast_to(p, (n, 3))
            Lv = y - a
            r2 = (Lv[:, 0] * Lv[:, 0] + Lv[:, 1] * Lv[:, 1]) + Lv[:, 2] * Lv[:, 2]
            ok = np.isfinite(r2) & (r2 > 0.0)
            r = np.sqrt(r2)
            w = Lv / r[:, None]
            cr = _dot(nh, w)
            ok &= cr > 0.0
            if L.type == RECT:
                cl = -_dot(np.broadcast_to(Nh, (n, 3)), w)
                if L.flags & TWO_SIDED:
                    cl = np.abs(cl)
                ok &= cl > 0.0
                g = ((cr * cl) / r2) * A
            else:
                if L.range > 0.0:
                    ok &= ~(r > L.range)
                g = cr / r2
                if L.type == SPOT:
                    d = _f(L, "direction")
                    sh = d / _len(d)
                    cs = -_dot(np.broadcast_to(sh, (n, 3)), w)
                    x = (cs - np.float64(L.cos_outer)) / (np.float64(L.cos_inner) - np.float64(L.cos_outer))
                    ok &= x > 0.0
                    x = np.where(x < 1.0, x, 1.0)
                    f = (x * x) * (3.0 - 2.0 * x)
                    g = g * f
            tmax = r - bias
        ok &= g > 0.0
        o = a + w * bias
    rays = np.concatenate([np.where(ok[:, None], o, a), np.where(ok[:, None], w, 0.0)], axis=1)
    return rays, np.where(ok, tmax, 0.0), np.where(ok, g, 0.0)


def direct_rays(points, normals, lights, spp=1, bias=0.01, seed=0, ids=None, sample_base=0):
    """(rays [n * R, 6], tmax [n * R], g [n * R]): slot s of entry i at i * R + s, lights in order, a rectangle's samples in j order"""
    a = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    nh = query_ref._nrm(np.asarray(normals, dtype=np.float64).reshape(-1, 3))
    n = a.shape[0]
    ids = np.arange(n) if ids is None else np.asarray(ids)
    R = slots(lights, spp)
    rays, tmax, g = np.zeros((n, R, 6)), np.zeros((n, R)), np.zeros((n, R))
    s = 0
    for l, L in enumerate(lights):
        for j in range(light_slots(L, spp)):
            rays[:, s], tmax[:, s], g[:, s] = _slot(L, l, a, nh, ids, bias, seed, sample_base + j)
            s += 1
    return rays.reshape(-1, 6), tmax.reshape(-1), g.reshape(-1)


def fold(lights, g, occluded, n, spp=1):
    """the fold of g [n * R] and occluded [n * R]: dict of irradiance [n, 3], stderr [n, 3], per_light [n, nl, 3], visibility [n, nl]"""
    nl = len(lights)
    R = slots(lights, spp)
    g = np.asarray(g, dtype=np.float64).reshape(n, R)
    occ = (np.asarray(occluded) != 0).reshape(n, R)
    E, V = np.zeros((n, 3)), np.zeros((n, 3))
    per_light, vis = np.zeros((n, nl, 3)), np.zeros((n, nl))
    s = 0
    with np.errstate(all="ignore"):
        for l, L in enumerate(lights):
            color = _f(L, "color")
            m = light_slots(L, spp)
            traced = np.zeros(n, dtype=np.int64)
            lit = np.zeros(n, dtype=np.int64)
            s1, s2, El = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
            for j in range(m):
                tr = g[:, s] > 0.0
                op = tr & ~occ[:, s]
                traced += tr
                lit += op
                x = np.where(op[:, None], color[None, :] * g[:, s, None], 0.0)
                if L.type == RECT:
                    s1 = s1 + x
                    s2 = s2 + x * x
                else:
                    El = x
                s += 1
            se2 = np.zeros((n, 3))
            if L.type == RECT:
                El = s1 / spp
                if spp >= 2:
                    var = (s2 - s1 * s1 / spp) / (spp - 1)
                    se2 = np.where(var > 0.0, var, 0.0) / spp
            E = E + El
            V = V + se2
            per_light[:, l] = El
            vis[:, l] = np.where(traced > 0, lit.astype(np.float64) / np.maximum(traced, 1).astype(np.float64), 0.0)
    return {"irradiance": E, "stderr": np.sqrt(V), "per_light": per_light, "visibility": vis}
