"""numpy restatement of the lightmap baker's own steps (include/mcpt.h: lightmaps): coverage, the texel list, the scatter and the
dilation.  Coverage tests EVERY texel against EVERY face -- no boxes, no early outs -- in the header's operation order; numpy rounds every
fp64 operation on its own, as the library's un-contracted code does.  Also the chart the CPU and GPU tests share."""
import numpy as np


def centres(width, height):
    """(pu [W], pv [H]): the texel centres along each axis"""
    return (np.arange(width) + 0.5) / width, (np.arange(height) + 0.5) / height


def area2_of(uv):
    au, av, bu, bv, cu, cv = uv
    return (bu - au) * (cv - av) - (bv - av) * (cu - au)


def edges(uv, pu, pv):
    """(e_a, e_b, e_c) of the centres (pu, pv), which broadcast"""
    au, av, bu, bv, cu, cv = uv
    ea = (bu - pu) * (cv - pv) - (bv - pv) * (cu - pu)
    eb = (cu - pu) * (av - pv) - (cv - pv) * (au - pu)
    ec = (au - pu) * (bv - pv) - (av - pv) * (bu - pu)
    return ea, eb, ec


def normal_ok(n):
    """the face takes part: its geometric normal has a length that is neither zero nor NaN nor infinite"""
    with np.errstate(all="ignore"):
        l2 = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
        return (l2 > 0.0) & (l2 < np.inf)


def covers(uv, width, height):
    """[H, W] bool: the texels whose centre the chart triangle uv covers (all False for a triangle that is skipped)"""
    pu, pv = centres(width, height)
    with np.errstate(all="ignore"):
        a2 = area2_of(uv)
        if not np.isfinite(a2) or a2 == 0.0:
            return np.zeros((height, width), dtype=bool)
        ea, eb, ec = edges(uv, pu[None, :], pv[:, None])
        if a2 > 0.0:
            return (ea >= 0.0) & (eb >= 0.0) & (ec >= 0.0)
        return (ea <= 0.0) & (eb <= 0.0) & (ec <= 0.0)


def raster(uv6, width, height, face_normals=None):
    """owner [H, W] int32: the lowest face that covers each texel, or -1; face_normals [n, 3] (or None) skips the faces whose normal has
    no length"""
    uv6 = np.asarray(uv6, dtype=np.float64).reshape(-1, 6)
    owner = np.full((height, width), -1, dtype=np.int32)
    ok = np.ones(uv6.shape[0], dtype=bool) if face_normals is None else normal_ok(np.asarray(face_normals, dtype=np.float64))
    for f in range(uv6.shape[0] - 1, -1, -1):           # descending: the lowest face writes last
        if ok[f]:
            owner[covers(uv6[f], width, height)] = f
    return owner


def texel_list(owner, uv6, v9, vn9, face_normals):
    """(texels [n] ascending, q6 [n, 6]) of a coverage map: position and normal of every covered texel on its owner"""
    height, width = owner.shape
    uv6 = np.asarray(uv6, dtype=np.float64).reshape(-1, 6)
    texels = np.flatnonzero(owner.reshape(-1) >= 0).astype(np.int32)
    f = owner.reshape(-1)[texels]
    pu, pv = centres(width, height)
    pu, pv = pu[texels % width], pv[texels // width]
    uv = uv6[f].T
    with np.errstate(all="ignore"):
        a2 = area2_of(uv)
        ea, eb, ec = edges(uv, pu, pv)
        wa, wb, wc = (ea / a2)[:, None], (eb / a2)[:, None], (ec / a2)[:, None]
        v, vn = np.asarray(v9, dtype=np.float64).reshape(-1, 9)[f], np.asarray(vn9, dtype=np.float64).reshape(-1, 9)[f]
        pos = (v[:, 0:3] * wa + v[:, 3:6] * wb) + v[:, 6:9] * wc
        nrm = (vn[:, 0:3] * wa + vn[:, 3:6] * wb) + vn[:, 6:9] * wc
        own = normal_ok(nrm)
    nrm = np.where(own[:, None], nrm, np.asarray(face_normals, dtype=np.float64).reshape(-1, 3)[f])
    return texels, np.concatenate([pos, nrm], axis=1)


def scatter(shape, texels, E, E_err, hits):
    """the maps (E [H, W, 3], E_stderr [H, W, 3], hits [H, W]) of a list's answers; everything else +0.0 / +0.0 / 0"""
    height, width = shape
    m_e, m_err, m_hits = np.zeros((height * width, 3)), np.zeros((height * width, 3)), np.zeros(height * width, dtype=np.int32)
    m_e[texels], m_err[texels], m_hits[texels] = E, E_err, hits
    return m_e.reshape(height, width, 3), m_err.reshape(height, width, 3), m_hits.reshape(height, width)


def dilate(E, owner, rounds):
    """(E, owner) after `rounds` rounds of dilation: a texel that is not valid takes the mean of its valid neighbours of the round before,
    summed from 0.0 in row-major order, and its owner becomes -1 - round"""
    E, owner = np.array(E, dtype=np.float64), np.array(owner, dtype=np.int32)
    height, width = owner.shape
    for r in range(1, rounds + 1):
        valid = owner != -1
        s, c = np.zeros_like(E), np.zeros((height, width), dtype=np.int64)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                # destination texels (y, x) whose neighbour (y + dy, x + dx) lies inside the map
                ys = slice(max(0, -dy), height - max(0, dy))
                xs = slice(max(0, -dx), width - max(0, dx))
                yn = slice(max(0, -dy) + dy, height - max(0, dy) + dy)
                xn = slice(max(0, -dx) + dx, width - max(0, dx) + dx)
                v = valid[yn, xn]
                s[ys, xs] = s[ys, xs] + np.where(v[..., None], E[yn, xn], 0.0)
                c[ys, xs] += v
        fill = ~valid & (c > 0)
        E[fill] = s[fill] / c[fill][:, None].astype(np.float64)
        owner[fill] = -1 - r
    return E, owner


# ---- the chart the tests share.  Face indices of its named parts:
QUAD_LOW, QUAD_HIGH = 0, 1          # a quad split on its diagonal, dyadic UVs, opposite windings
OVERLAP_A, OVERLAP_B = 2, 3         # two faces that overlap each other (and the quad)
ZERO_AREA, POINT = 4, 5             # collinear corners; three equal corners
OUTSIDE_A, OUTSIDE_B = 6, 7         # wholly outside [0, 1]^2
PARTLY_A, PARTLY_B = 8, 9           # partly outside
SLIVER = 10                         # covers no centre of a 1x1, 3x5, 64x64 or 257x130 map
N_NAMED, N_RANDOM = 11, 200


def shared_chart(seed=7):
    """[211, 6]: the named parts above, then 200 random triangles of both windings, small and large, some across the map's border"""
    lo, hi = 33.0 / 128.0, 97.0 / 128.0     # centres of texels 16 and 48 of a 64-texel axis: corners ON texel centres
    named = [
        [lo, lo, hi, lo, hi, hi],           # a b c: counter-clockwise
        [lo, lo, lo, hi, hi, hi],           # a d c: clockwise; shares the diagonal a-c, on which u == v
        [0.1, 0.1, 0.6, 0.15, 0.2, 0.7],
        [0.15, 0.05, 0.5, 0.5, 0.05, 0.6],
        [0.25, 0.5, 0.5, 0.5, 0.75, 0.5],
        [0.625, 0.125, 0.625, 0.125, 0.625, 0.125],
        [1.5, 1.5, 2.5, 1.5, 1.5, 2.5],
        [-2.0, -1.0, -1.0, -1.0, -1.5, -0.2],
        [0.8, 0.8, 1.4, 0.9, 0.9, 1.3],
        [-0.3, 0.4, 0.2, 0.5, -0.1, 0.9],
        [0.05, 0.9001, 0.95, 0.9001, 0.5, 0.9002],
    ]
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-0.1, 1.1, size=(N_RANDOM, 1, 2))
    size = 10.0 ** rng.uniform(-2.5, -0.7, size=(N_RANDOM, 1, 1))
    tri = centre + size * rng.uniform(-1.0, 1.0, size=(N_RANDOM, 3, 2))
    return np.concatenate([np.array(named), tri.reshape(N_RANDOM, 6)])
