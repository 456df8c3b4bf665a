"""Reflection probes (include/mcpt.h: reflection probes) restated in numpy: the octahedral encode and decode, the texels' centres and solid
angles, the wrap across the square's seams, the integer power, the rays of a bake's entries, the per-texel fold, the Phong prefilter and
the lookup in a chain.  fp64 in the header's operation order -- add, subtract, multiply, divide, sqrt and floor only, so the library's
answers are compared bit for bit.  Every sum is accumulated sequentially (never np.sum); the vectors run over outputs, not over terms."""
import numpy as np

import lens_ref

MAX_RES, MAX_LEVELS, MAX_NS = 256, 8, 65535


def _fold(u, v):
    """the lower hemisphere's fold, from the old u and v"""
    return (1.0 - np.abs(v)) * np.where(u >= 0.0, 1.0, -1.0), (1.0 - np.abs(u)) * np.where(v >= 0.0, 1.0, -1.0)


def encode(d):
    """(s, t) [n, 2] of directions d [n, 3] of any non-zero finite length"""
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    with np.errstate(all="ignore"):
        l = (np.abs(x) + np.abs(y)) + np.abs(z)
        u, v = x / l, y / l
        fu, fv = _fold(u, v)
        u, v = np.where(z < 0.0, fu, u), np.where(z < 0.0, fv, v)
        return np.stack([u * 0.5 + 0.5, v * 0.5 + 0.5], axis=1)


def square(s, t):
    """the folded, unnormalised (u, v, z) of the points (s, t) of the square"""
    u, v = 2.0 * np.asarray(s, dtype=np.float64) - 1.0, 2.0 * np.asarray(t, dtype=np.float64) - 1.0
    z = (1.0 - np.abs(u)) - np.abs(v)
    fu, fv = _fold(u, v)
    return np.where(z < 0.0, fu, u), np.where(z < 0.0, fv, v), z


def decode(s, t):
    """unit directions [n, 3] of the points (s, t)"""
    u, v, z = square(s, t)
    l = np.sqrt((u * u + v * v) + z * z)
    return np.stack([u / l, v / l, z / l], axis=1)


def texels(R):
    """(d [R * R, 3], w [R * R]): the centre direction and the midpoint-rule solid angle of texel b = y * R + x"""
    b = np.arange(R * R)
    x, y = (b % R).astype(np.float64), (b // R).astype(np.float64)
    u, v, z = square((x + 0.5) / float(R), (y + 0.5) / float(R))
    n2 = (u * u + v * v) + z * z
    l = np.sqrt(n2)
    return np.stack([u / l, v / l, z / l], axis=1), ((2.0 / float(R)) * (2.0 / float(R))) / (n2 * l)


def wrap(R, x, y):
    """taps (x, y), x and y in -1 .. R, across the square's edges into 0 .. R - 1"""
    x, y = np.array(x, dtype=np.int64), np.array(y, dtype=np.int64)
    out = (x < 0) | (x >= R)
    x, y = np.where(out, np.where(x < 0, -1 - x, 2 * R - 1 - x), x), np.where(out, R - 1 - y, y)
    out = (y < 0) | (y >= R)
    y, x = np.where(out, np.where(y < 0, -1 - y, 2 * R - 1 - y), y), np.where(out, R - 1 - x, x)
    return x, y


def ipow(c, n):
    """c ** n for an integer n >= 0 by binary squaring in the header's order"""
    c = np.asarray(c, dtype=np.float64)
    r, b, n = np.ones_like(c), c.copy(), int(n)
    with np.errstate(under="ignore"):
        while n > 0:
            if n & 1:
                r = r * b
            n >>= 1
            if n:
                b = b * b
    return r


# ---- the bake

def entries_of(n, R, S):
    return np.arange(n * R * R * S, dtype=np.int64)


def rays(points, R, S, entries, seed, sample_base=0, id_base=None):
    """(rays [m, 6], ids [m]) of the listed entries e = (i * R * R + b) * S + j"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    e = np.asarray(entries, dtype=np.int64)
    per = R * R * S
    i, rest = e // per, e % per
    b = rest // S
    base = i * per if id_base is None else np.asarray(id_base, dtype=np.int64)[i]
    ids = base + rest
    u0, u1, _, _ = lens_ref.camera_uniforms(seed, ids, np.full(ids.shape, sample_base, dtype=np.int64))
    x, y = (b % R).astype(np.float64), (b // R).astype(np.float64)
    d = decode((x + u0) / float(R), (y + u1) / float(R))
    return np.concatenate([p[i], d], axis=1), ids.astype(np.int32)


def fold(x, hit):
    """(mean [T, 3], stderr [T, 3], hits [T]) of the samples x [T, S, 3] and their hit counts hit [T, S], in j order with the query's
    own expressions"""
    x = np.asarray(x, dtype=np.float64)
    T, S = x.shape[:2]
    s1, s2, hits = np.zeros((T, 3)), np.zeros((T, 3)), np.zeros(T, dtype=np.int32)
    for j in range(S):
        s1 = s1 + x[:, j]
        s2 = s2 + x[:, j] * x[:, j]
        hits = hits + np.asarray(hit)[:, j].astype(np.int32)
    mean = s1 / float(S)
    if S < 2:
        return mean, np.zeros((T, 3)), hits
    var = (s2 - s1 * s1 / float(S)) / float(S - 1)
    return mean, np.sqrt(np.where(var > 0.0, var, 0.0) / float(S)), hits


# ---- the prefilter

def chain_texels(levels):
    return sum(r * r for r, _ in levels)


def prefilter(L, R, levels):
    """chain [n, T, 3] of the maps L [n, R * R, 3] under levels = [(level_res, ns), ...]: per output texel the sums W and A over the
    source texels in ascending order"""
    L = np.asarray(L, dtype=np.float64).reshape(-1, R * R, 3)
    n = L.shape[0]
    d, w = texels(R)
    out = np.zeros((n, chain_texels(levels), 3))
    first = 0
    for Ro, ns in levels:
        r, _ = texels(Ro)
        m = Ro * Ro
        W, A = np.zeros(m), np.zeros((n, m, 3))
        for b in range(R * R):
            c = (r[:, 0] * d[b, 0] + r[:, 1] * d[b, 1]) + r[:, 2] * d[b, 2]
            on = c > 0.0
            if not on.any():
                continue
            with np.errstate(under="ignore"):
                g = w[b] * ipow(c[on], ns)
                W[on] += g
                A[:, on, :] += g[None, :, None] * L[:, b, None, :]
        lit = W > 0.0
        with np.errstate(all="ignore"):
            out[:, first:first + m, :] = np.where(lit[None, :, None], A / W[None, :, None], 0.0)
        first += m
    return out


# ---- the lookup

def level_value(chain, probe, first, R, d):
    """the bilinear value [q, 3] of directions d [q, 3] in the R x R level that starts at texel `first` of chain[probe[q]]"""
    st = encode(d)

    def axis(s):
        with np.errstate(invalid="ignore"):
            a = s * float(R) - 0.5
            a = np.where(a > -1.0, a, -1.0)
            a = np.where(a < float(R) - 0.5, a, float(R) - 0.5)
        fl = np.floor(a)
        return fl.astype(np.int64), a - fl

    x0, fx = axis(st[:, 0])
    y0, fy = axis(st[:, 1])
    taps = [wrap(R, x0 + dx, y0 + dy) for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1))]
    w = [(1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy]
    v = [chain[probe, first + ty * R + tx, :] for tx, ty in taps]
    return ((w[0][:, None] * v[0] + w[1][:, None] * v[1]) + w[2][:, None] * v[2]) + w[3][:, None] * v[3]


def wt(a):
    return 1.0 / np.sqrt(np.asarray(a, dtype=np.float64) + 1.0)


def lookup(chain, levels, probe, d, x):
    """[q, 3]: the radiance chain [n, T, 3] holds for receiver q = (probe[q], d[q], x[q])"""
    chain = np.asarray(chain, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    probe = np.asarray(probe, dtype=np.int64)
    x = np.broadcast_to(np.asarray(x, dtype=np.float64), probe.shape)
    n = len(levels)
    first = np.concatenate([[0], np.cumsum([r * r for r, _ in levels])])
    ns = np.array([e for _, e in levels], dtype=np.float64)
    values = [level_value(chain, probe, int(first[l]), levels[l][0], d) for l in range(n)]
    out = np.zeros((d.shape[0], 3))
    done = np.zeros(d.shape[0], dtype=bool)
    top = (x >= ns[0]) if n > 1 else np.ones(d.shape[0], dtype=bool)
    out[top] = values[0][top]
    done |= top
    last = ~done & (x <= ns[n - 1])
    out[last] = values[n - 1][last]
    done |= last
    for l in range(n - 1):
        pick = ~done & (x > ns[l + 1])
        a = (wt(x) - wt(ns[l])) / (wt(ns[l + 1]) - wt(ns[l]))
        blend = (1.0 - a)[:, None] * values[l] + a[:, None] * values[l + 1]
        out[pick] = np.where((a == 0.0)[:, None], values[l], blend)[pick]
        done |= pick
    assert done.all()
    return out


# ---- the tests' inputs

def source_map(n, R, seed=1):
    """n maps of R x R texels of positive radiance with a few bright texels"""
    rng = np.random.default_rng([seed, n, R])
    L = rng.random((n, R * R, 3)) + 0.25
    L[:, rng.integers(0, R * R, size=max(1, R // 2)), :] *= 40.0
    return L


def receivers(levels, seed=2, n_random=4000):
    """(d [m, 3], x [m]): texel centres of every level, the axes, the z = 0 equator, the seams (x or y = +-1e-300 with z < 0), +-1e300,
    random directions; x at, between and beyond the levels' exponents"""
    rng = np.random.default_rng(seed)
    parts = [texels(r)[0] for r, _ in levels]
    axes = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])
    phi = np.linspace(0.0, 2.0 * np.pi, 37)
    equator = np.stack([np.cos(phi), np.sin(phi), np.zeros_like(phi)], axis=1)
    seams = np.array([[sx * 1e-300, y, -0.5] for sx in (1.0, -1.0) for y in (-0.7, -0.2, 0.0, 0.3, 0.9)]
                     + [[x, sy * 1e-300, -0.5] for sy in (1.0, -1.0) for x in (-0.7, -0.2, 0.0, 0.3, 0.9)]
                     + [[sx * 1e-300, sy * 1e-300, -1.0] for sx in (1.0, -1.0) for sy in (1.0, -1.0)])
    huge = np.array([[1e300, 0.5e300, -1e300], [-1e300, 1e300, 1e300], [1e300, -1e-300, -1e300], [-1e300, -1e300, -1e300], [1e300, 0.0, 0.0]])
    rnd = rng.normal(size=(n_random, 3)) * 10.0 ** rng.uniform(-3, 3, size=(n_random, 1))
    d = np.concatenate(parts + [axes, equator, seams, huge, rnd])
    ns = sorted({float(e) for _, e in levels})
    xs = list(ns) + [0.5 * (a + b) for a, b in zip(ns[:-1], ns[1:])] + [ns[-1] * 2.0 + 1.0, ns[-1] + 0.25, max(ns[0] - 0.5, 0.0), 0.0, 1e300, 0.3]
    xs += [np.nextafter(e, np.inf) for e in ns] + [np.nextafter(e, -np.inf) for e in ns if e > 0]
    x = np.array(xs)[np.arange(d.shape[0]) % len(xs)]
    x[-n_random // 2:] = rng.uniform(0.0, ns[-1] * 1.5 + 2.0, size=n_random // 2)
    return d, x
