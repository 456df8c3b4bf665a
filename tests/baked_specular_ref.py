"""Baked specular restated in numpy (include/mcpt.h: baked specular): the reflection volume's lookup -- volume_ref.corners or
visibility_ref.factors for the corners and weights, reflection_ref.lookup for every corner's value, the blend in j order -- the mirror
direction of a baked surface sample, the radiance with the specular term and the per-pixel count, each expression in the header's order,
and the inputs the CPU and GPU tests share.  tests/test_baked_specular_cpu.py holds this to mcpt_reflection_volume_lookup_host,
tests/test_gpu_baked_specular.py holds the kernels to it."""
import numpy as np

import baked_ref as BR
import reflection_ref as RR
import visibility_ref
import volume_ref

GRIDS = [(1, 1, 1), (2, 1, 1), (1, 3, 1), (2, 2, 2), (3, 2, 2)]           # (nx, ny, nz)
CHAINS = {"one-texel": (1, [(1, 4)]), "one-level": (4, [(4, 12)]), "three-levels": (8, [(8, 64), (4, 8), (2, 0)])}     # res, [(level_res, ns)]
ORIGIN, SPACING = (0.1, -0.4, 0.3), (0.3, 0.7, 0.45)                      # not dyadic: the snap is needed
VIS_RES = 4
N_RANDOM = 4000


def weights(origin, spacing, counts, x, b, valid=None, moments=None, vis=None):
    """(P [n, 8], w [n, 8]): the corners and weights of receivers at x with normals b -- mcpt_volume_irradiance's, or with moments
    (vis = (res, max_distance, normal_bias, min_visibility)) mcpt_volume_irradiance_visible's"""
    x, b = np.asarray(x, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if moments is None:
        P, w, _ = volume_ref.corners(origin, spacing, counts, x, valid)
        return P, w
    R, max_distance, normal_bias, min_visibility = vis
    with np.errstate(over="ignore"):                        # (receivers at +-1e300: the distance overflows, as in the library)
        P, w, f = visibility_ref.factors(origin, spacing, counts, moments, x, b, R, max_distance, normal_bias, min_visibility)
    if valid is not None:
        w = np.where(np.asarray(valid).reshape(-1)[P] == 0, 0.0, w)
    w = w * f
    W = np.zeros(x.shape[0])
    for j in range(8):
        W = W + w[:, j]
    lit = W > 0.0
    return P, np.where(lit[:, None], w / np.where(lit, W, 1.0)[:, None], 0.0)


def volume_lookup(origin, spacing, counts, levels, chain, x, b, d, e, valid=None, moments=None, vis=None):
    """(out [n, 3], corners [n]) of receivers at x with normals b, directions d and exponents e in chain [nprobes, T, 3]"""
    chain = np.asarray(chain, dtype=np.float64).reshape(-1, RR.chain_texels(levels), 3)
    n = np.asarray(x).shape[0]
    e = np.broadcast_to(np.asarray(e, dtype=np.float64), (n,))
    P, w = weights(origin, spacing, counts, x, b, valid, moments, vis)
    out = np.zeros((n, 3))
    for j in range(8):
        on = w[:, j] != 0.0                 # a corner of weight 0.0 contributes nothing and is not read
        v = RR.lookup(chain, levels, P[:, j], d, e)
        out = np.where(on[:, None], out + w[:, j, None] * v, out)
    return out, (w > 0.0).sum(axis=1).astype(np.int32)


def mirror(d, n):
    """(r [m, 3], ok [m]): r = d * (n . n) - n * (2 (d . n)), and whether its 1-norm is > 0 and finite"""
    d, n = np.asarray(d, dtype=np.float64), np.asarray(n, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        dn = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
        nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        r = d * nn[:, None] - n * (2.0 * dn)[:, None]
        l = (np.abs(r[:, 0]) + np.abs(r[:, 1])) + np.abs(r[:, 2])
    return r, (l > 0.0) & (l < np.inf)


def exponent(ns):
    ns = np.asarray(ns, dtype=np.float64)
    return np.where(ns >= 0.0, ns, 0.0)


def radiance(D, ks, R, spec, lighting_only=False):
    """L [m, 3] = D + ks * R on the rows with a specular term (D + R under lighting_only), D elsewhere"""
    return np.where(np.asarray(spec)[:, None], D + (R if lighting_only else ks * R), D)


def count(slit):
    """slit [n, G] of a pixel's samples -> the samples whose lookup found a probe"""
    return (np.asarray(slit) > 0).sum(axis=1).astype(np.int32)


def fold(L, kind, lit, slit):
    """baked_ref.fold of a pixel's samples [n, G, ...] with the specular count: (pixel [n, 3], counts [n, 3], lit [n], slit [n])"""
    return BR.fold(L, kind, lit) + (count(slit),)


# ---- the inputs the lookup's tests share

def chain_data(counts, res, levels, seed=3):
    """[nprobes, T, 3]: reflection_ref.source_map's positive maps under the prefilter, a different map per probe"""
    n = counts[0] * counts[1] * counts[2]
    return RR.prefilter(RR.source_map(n, res, seed=seed), res, levels)


def masks(counts, seed=4):
    """(None, a random mask that keeps probe 0 and, where there are two, drops the last, no probe valid)"""
    n = counts[0] * counts[1] * counts[2]
    rng = np.random.default_rng([seed, n])
    m = (rng.random(n) < 0.6).astype(np.uint8)
    m[0] = 1
    if n >= 2:
        m[-1] = 0
    return None, m, np.zeros(n, dtype=np.uint8)


def moments_of(counts, seed=5):
    """(moments [nprobes, 16, 2], vis = (res, max_distance, normal_bias, min_visibility)): a mean within the grid's reach, a variance on
    top, a tenth of the bins without samples"""
    n = counts[0] * counts[1] * counts[2]
    rng = np.random.default_rng([seed, n])
    dmax = 1.5
    mu = rng.uniform(0.0, dmax, size=(n, VIS_RES * VIS_RES))
    m = np.stack([mu, mu * mu + rng.uniform(0.0, 0.1 * dmax * dmax, size=mu.shape)], axis=2)
    m[rng.random(mu.shape) < 0.1] = (-1.0, 0.0)
    return m, (VIS_RES, dmax, 0.02, 0.0)


def receivers(counts, levels, seed=6):
    """(x [m, 3], b [m, 3], d [m, 3], e [m]): every probe's own position first (nprobes of them), the cell centres, positions outside the
    grid on every side and at +-1e300, N_RANDOM random ones in and around the grid; directions and exponents from
    reflection_ref.receivers -- the levels' texel centres, the seams, exponents at, between, below and above the levels'"""
    rng = np.random.default_rng([seed, counts[0], counts[1], counts[2]])
    o, s, c = np.array(ORIGIN), np.array(SPACING), np.array(counts)
    probes = volume_ref.points(ORIGIN, SPACING, counts)
    iz, iy, ix = np.meshgrid(np.arange(max(c[2] - 1, 1)), np.arange(max(c[1] - 1, 1)), np.arange(max(c[0] - 1, 1)), indexing="ij")
    cells = o + (np.stack([ix, iy, iz], axis=-1).reshape(-1, 3) + 0.5) * s
    hi = o + (c - 1) * s
    outside = []
    for a in range(3):
        for v in (o[a] - 0.37, hi[a] + 0.41, -1e300, 1e300):
            p = o + rng.random((6, 3)) * (hi - o)
            p[:, a] = v
            outside.append(p)
    outside.append(np.array([[1e300, -1e300, 1e300], [-1e300, -1e300, -1e300]]))
    rnd = o - 0.3 * s + rng.random((N_RANDOM, 3)) * ((hi - o) + 0.6 * s)
    x = np.concatenate([probes, cells] + outside + [rnd])
    m = x.shape[0]
    b = rng.normal(size=(m, 3))
    d_all, e_all = RR.receivers(levels, seed=seed, n_random=N_RANDOM)
    pick = np.concatenate([np.arange(m - N_RANDOM) % (d_all.shape[0] - N_RANDOM), np.arange(d_all.shape[0] - N_RANDOM, d_all.shape[0])])
    return np.ascontiguousarray(x), np.ascontiguousarray(b), np.ascontiguousarray(d_all[pick]), np.ascontiguousarray(e_all[pick])


def specular_rays(eye, geom, face_ks, n, seed=8):
    """n rays from `eye` to random points on the faces whose material has a ks component != 0 (geom [t, 27]: v1, v2, v3 first)"""
    rng = np.random.default_rng(seed)
    faces = np.flatnonzero(face_ks)
    f = faces[rng.integers(0, faces.shape[0], size=n)]
    u, v = rng.random(n), rng.random(n)
    flip = u + v > 1.0
    u, v = np.where(flip, 1.0 - u, u), np.where(flip, 1.0 - v, v)
    p = geom[f, 0:3] * (1.0 - u - v)[:, None] + geom[f, 3:6] * u[:, None] + geom[f, 6:9] * v[:, None]
    d = p - np.asarray(eye, dtype=np.float64)
    return np.ascontiguousarray(np.concatenate([np.tile(np.asarray(eye, dtype=np.float64), (n, 1)), d], axis=1))

