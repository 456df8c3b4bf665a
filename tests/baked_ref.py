"""Baked frames restated in numpy (include/mcpt.h: baked frames): the lightmap's lookup by chart coordinate, the chart coordinate of a hit,
the radiance of a sample and the fold of a pixel's samples, each expression in the header's order (numpy does not contract), and the
inputs the CPU and GPU tests share.  tests/test_baked_cpu.py holds this to mcpt_lightmap_irradiance_host and to hand computations,
tests/test_gpu_baked.py holds the kernels to it."""
import numpy as np

MISS, EMITTER, SURFACE = 0, 1, 2
PI = 3.141592653589793
N_RANDOM = 4000
SIZES = [(1, 1), (1, 7), (7, 1), (5, 4), (64, 64)]          # (width, height)


def axis(u, size):
    """one axis of the lookup: (i0, i1, w0, w1) of chart coordinates u in a map of `size` texels"""
    u = np.asarray(u, dtype=np.float64)
    top = float(size - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        s = u * float(size) - 0.5
        s = np.where(s > 0.0, s, 0.0)
        s = np.where(s < top, s, top)
    if size >= 2:
        i0 = np.minimum(np.floor(s).astype(np.int64), size - 2)
        i1 = i0 + 1
        f = s - i0.astype(np.float64)
    else:
        i0 = np.zeros(u.shape, dtype=np.int64)
        i1 = i0
        f = np.zeros(u.shape)
    return i0, i1, 1.0 - f, f


def taps(width, height, uv, owner=None):
    """(T [n, 4], w [n, 4], count [n]): texel and weight of tap j = dy * 2 + dx after the owner rule"""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    x0, x1, wx0, wx1 = axis(uv[:, 0], width)
    y0, y1, wy0, wy1 = axis(uv[:, 1], height)
    xs, ys, wxs, wys = (x0, x1), (y0, y1), (wx0, wx1), (wy0, wy1)
    T = np.stack([ys[j >> 1] * width + xs[j & 1] for j in range(4)], axis=1)
    w = np.stack([wxs[j & 1] * wys[j >> 1] for j in range(4)], axis=1)
    if owner is not None:
        own = np.asarray(owner).reshape(-1)
        w = np.where(own[T] == -1, 0.0, w)
        total = np.zeros(uv.shape[0])
        for j in range(4):
            total = total + w[:, j]
        any_ = total > 0.0
        with np.errstate(invalid="ignore", divide="ignore"):
            w = np.where(any_[:, None], w / total[:, None], 0.0)
    return T, w, (w > 0.0).sum(axis=1).astype(np.int32)


def lightmap_irradiance(E, uv, owner=None):
    """(e [n, 3], taps [n]) of chart coordinates uv [n, 2] in the map E [height, width, 3]"""
    E = np.asarray(E, dtype=np.float64)
    height, width = E.shape[:2]
    T, w, count = taps(width, height, uv, owner)
    flat = E.reshape(-1, 3)
    e = np.zeros((T.shape[0], 3))
    for j in range(4):
        e = e + w[:, j:j + 1] * flat[T[:, j]]
    e = np.where((count > 0)[:, None], e, 0.0)
    return e, count


def _cross(a, b):
    # Vertex::cross as the kernels spell it (dev_common.hpp)
    return np.stack([a[:, 1] * b[:, 2] - b[:, 1] * a[:, 2], b[:, 0] * a[:, 2] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]], axis=1)


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def barycentric(v1, v2, v3, p):
    """the quotient form mcpt_trace_closest uses for pn: g [n, 3]"""
    e1, e2, e3 = v3 - v2, v1 - v3, v2 - v1
    d1, d2, d3 = p - v1, p - v2, p - v3
    n = _cross(e1, e2)
    an = _dot(n, n)
    return np.stack([_dot(_cross(e1, d3), n) / an, _dot(_cross(e2, d1), n) / an, _dot(_cross(e3, d2), n) / an], axis=1)


def chart_uv(rows6, g):
    """u = (au * g.x + bu * g.y) + cu * g.z, v likewise: [n, 2]"""
    u = (rows6[:, 0] * g[:, 0] + rows6[:, 2] * g[:, 1]) + rows6[:, 4] * g[:, 2]
    v = (rows6[:, 1] * g[:, 0] + rows6[:, 3] * g[:, 1]) + rows6[:, 5] * g[:, 2]
    return np.stack([u, v], axis=1)


def shading_normal(pn, face_normal, d, face_viewer):
    """pn, the face's stored normal where pn's squared length is 0 or not finite, negated under face_viewer where it points along d"""
    pn = np.asarray(pn, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        l2 = (pn[:, 0] * pn[:, 0] + pn[:, 1] * pn[:, 1]) + pn[:, 2] * pn[:, 2]
    bad = ~((l2 > 0.0) & (l2 < np.inf))
    n = np.where(bad[:, None], face_normal, pn)
    if face_viewer:
        along = ((d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]) > 0.0
        n = np.where(along[:, None], -n, n)
    return n


def radiance(kind, kd, e, emitted, missed, lighting_only=False):
    """L [n, 3] of samples of `kind`: (kd * e) / pi on a surface (e / pi under lighting_only), the light's radiance, the environment's"""
    kind = np.asarray(kind)
    surf = e / PI if lighting_only else (kd * e) / PI
    return np.where((kind == SURFACE)[:, None], surf, np.where((kind == EMITTER)[:, None], emitted, missed))


def fold(L, kind, lit):
    """A pixel's samples, [n, G, ...] in k order -> (pixel [n, 3], counts [n, 3] = (surface, emitter, miss), lit [n])"""
    L = np.asarray(L, dtype=np.float64)
    G = L.shape[1]
    s = np.zeros((L.shape[0], 3))
    for k in range(G):
        s = s + L[:, k]
    kind, lit = np.asarray(kind), np.asarray(lit)
    counts = np.stack([(kind == SURFACE).sum(axis=1), (kind == EMITTER).sum(axis=1), (kind == MISS).sum(axis=1)], axis=1).astype(np.int32)
    return s / float(G), counts, ((kind == SURFACE) & (lit > 0)).sum(axis=1).astype(np.int32)


# ---- the inputs the lookup's tests share

def lightmap(width, height, seed=0):
    """E [height, width, 3]: random, positive, a few decades"""
    rng = np.random.default_rng([seed, 11, width, height])
    return rng.uniform(0.5, 1.5, size=(height, width, 3)) * 10.0 ** rng.uniform(-2, 1, size=(height, width, 1))


def owner_map(width, height, seed=0, keep=0.7):
    """owner [height, width]: a face index, a dilation round's mark (-2, -3) or -1"""
    rng = np.random.default_rng([seed, 12, width, height])
    own = rng.integers(0, 40, size=(height, width)).astype(np.int32)
    own[rng.random((height, width)) < 0.1] = -2
    own[rng.random((height, width)) < 0.05] = -3
    own[rng.random((height, width)) >= keep] = -1
    return own


def centres(width, height):
    x, y = np.meshgrid(np.arange(width), np.arange(height))
    return np.stack([(x.reshape(-1) + 0.5) / width, (y.reshape(-1) + 0.5) / height], axis=1)


def coordinates(width, height, seed=0):
    """uv [n, 2]: every texel centre first (width * height of them), texel edges and corners, coordinates below 0 and above 1 on each
    side, components of +-1e300 and 1e-300, and N_RANDOM random points in and a little around the map"""
    rng = np.random.default_rng([seed, 13, width, height])
    parts = [centres(width, height)]
    ex, ey = np.meshgrid(np.arange(width + 1) / width, np.arange(height + 1) / height)
    corners = np.stack([ex.reshape(-1), ey.reshape(-1)], axis=1)
    parts.append(corners)                                                            # texel corners
    edge = corners.copy()
    edge[:, 1] = rng.random(edge.shape[0])
    parts.append(edge)                                                               # a texel edge in u
    edge = corners.copy()
    edge[:, 0] = rng.random(edge.shape[0])
    parts.append(edge)                                                               # ... and in v
    for a in range(2):
        for lo in (True, False):
            p = rng.random((40, 2))
            p[:, a] = -rng.uniform(1e-9, 3.0, size=40) if lo else 1.0 + rng.uniform(1e-9, 3.0, size=40)
            parts.append(p)
    big = rng.random((24, 2))
    vals = [1e300, -1e300, 1e-300, -1e-300]
    for r in range(24):
        big[r, r % 2] = vals[(r // 2) % 4]
    big[-3:] = [[1e300, -1e300], [-1e300, 1e300], [1e-300, 1e-300]]
    parts.append(big)
    parts.append(-0.25 + 1.5 * rng.random((N_RANDOM, 2)))
    return np.ascontiguousarray(np.concatenate(parts))
