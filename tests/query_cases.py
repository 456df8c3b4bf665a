"""Query lists away from the camera, shared by tests/test_query_oracle_cpu.py (which asserts on the oracle alone that every group is what it
claims to be) and tests/test_gpu_query_oracle.py (which holds mcpt_query_radiance to orc_ray_radiance on them).

Every list is made deterministically from the oracle's own closest hits (p, pn, face) of the oracle's camera rays d_cam of the scene at
W x H = 64 x 36, at most LIMIT queries per group:

  front         p - d_cam * 0.005, 5 mm in front of a surface; a random unit direction: first hits a few millimetres from the origin, which
                an extra 0.01 along d would skip
  behind        p + d_cam * 0.001: outside the room, behind walls, inside solids; a random unit direction: first hits on back faces, misses
  inside-glass  the `behind` origins whose first hit is on a material with Ni > 1, eight random directions each: the exit branch of the
                refraction (cos_in > 0, total reflection) at depth 0
  on-surface    p itself, what a refraction ray does; a random unit direction
  axes          interior points (in no wall's plane); the six +-axis directions and the twelve face diagonals
  far           origins outside the scene's bounds, aimed at interior points; every fifth aimed away
  hemi          hemisphere kind: position p, normal = the hit's normal turned towards the camera's side (unnormalised, as the oracle gives it)
  hemi-corner   `hemi` points closest to another surface: those from which one of the six axis rays meets another triangle in less
                than 0.01 (the oracle's closest hit), so that the origin 0.01 along a sample's direction can lie behind that triangle;
                looked for among the hits of the pixels' rays and of 16 jittered camera rays per pixel (one ray per pixel finds a handful)

Each list comes with two id vectors -- random in [0, 2^31 - 1], and a permutation of 0 .. n-1 -- and is asked for at the sample indices K.
Directions are normalised until |(dx dx + dy dy) + dz dz - 1| <= 1e-9, the host form's check."""
import numpy as np

import query_ref

W, H = 64, 36
LIMIT = 1500
K = (0, 5, 63, 2 ** 31 - 2)
ID_MAX = 2 ** 31 - 1
SPP_MEAN = 8
MEAN_BASES = (0, 2 ** 31 - 1 - SPP_MEAN)
RAY_GROUPS = ("front", "behind", "inside-glass", "on-surface", "axes", "far")
HEMI_GROUPS = ("hemi", "hemi-corner")
NEAR = 0.01                     # the offset of a shadow ray, a bounce ray and a hemisphere sample
CORNER_SAMPLES = 16             # jittered camera rays per pixel that hemi-corner looks for its points among

_AXES = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])
_DIAGONALS = np.array([[a, b, 0.0] for a in (1.0, -1.0) for b in (1.0, -1.0)] + [[a, 0.0, b] for a in (1.0, -1.0) for b in (1.0, -1.0)]
                      + [[0.0, a, b] for a in (1.0, -1.0) for b in (1.0, -1.0)])


def unit(d):
    """d / |d| with |d|^2 summed as the host form sums it; checked against its bound"""
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    if d.shape[0] == 0:
        return d
    d = d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
    assert np.abs(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) - 1.0).max() <= 1e-9
    return d


def _directions(rng, n):
    return unit(rng.normal(size=(n, 3)))


class Group:
    """one query list: q (n, 6), kind "ray" or "hemisphere", the two id vectors"""

    def __init__(self, name, q, rng):
        self.name = name
        self.kind = "hemisphere" if name in HEMI_GROUPS else "ray"
        self.q = np.ascontiguousarray(q, dtype=np.float64)
        self.n = self.q.shape[0]
        self.ids = {"random": rng.integers(0, ID_MAX, size=self.n, endpoint=True).astype(np.int32),
                    "permutation": rng.permutation(self.n).astype(np.int32)}
        if self.n:
            self.ids["random"][0] = ID_MAX                   # the largest id is always among them


def _pick(rng, idx, limit=LIMIT):
    """at most `limit` of idx, in increasing order"""
    return idx if idx.size <= limit else np.sort(rng.choice(idx, size=limit, replace=False))


def bounds(osc):
    box = osc.bvh_nodes()[0][0]
    return np.minimum(box[:3], box[3:]), np.maximum(box[:3], box[3:])


def corner_mask(osc, p, face):
    """the points p (on the triangles `face`) from which an axis ray meets ANOTHER triangle closer than NEAR"""
    near = np.zeros(p.shape[0], dtype=bool)
    for a in _AXES:
        f, t, _, _ = osc.trace_closest(np.concatenate([p, np.tile(a, (p.shape[0], 1))], axis=1))
        near |= (f >= 0) & (f != face) & (t > 1e-9) & (t < NEAR)
    return near


def build(osc, seed=2024):
    """{group name: Group} for the oracle scene osc at W x H; the scene is left without a lens"""
    assert (osc.width, osc.height) == (W, H), "query_cases: the scene at %d x %d" % (W, H)
    rng = np.random.default_rng(seed)
    cam = osc.primary_rays()
    face, _, p, pn = osc.trace_closest(cam)
    hit = np.flatnonzero(face >= 0)
    d_cam = cam[:, 3:]
    ni = np.array([osc.material(m)[1][7] for m in range(osc.num_materials)])
    glass = ni[osc.faces()[1][np.maximum(face, 0)]] > 1
    lo, hi = bounds(osc)
    out = {}

    def add(name, q):
        out[name] = Group(name, q, rng)

    i = _pick(rng, hit)
    add("front", np.concatenate([p[i] - d_cam[i] * 0.005, _directions(rng, i.size)], axis=1))
    i = _pick(rng, hit)
    add("behind", np.concatenate([p[i] + d_cam[i] * 0.001, _directions(rng, i.size)], axis=1))
    i = np.repeat(_pick(rng, np.flatnonzero((face >= 0) & glass), LIMIT // 8), 8)
    add("inside-glass", np.concatenate([p[i] + d_cam[i] * 0.001, _directions(rng, i.size)], axis=1))
    i = _pick(rng, hit)
    add("on-surface", np.concatenate([p[i], _directions(rng, i.size)], axis=1))
    dirs = np.concatenate([_AXES, unit(_DIAGONALS)])
    pts = lo + (hi - lo) * (0.1 + 0.8 * rng.random((LIMIT // dirs.shape[0], 3)))
    add("axes", np.concatenate([np.repeat(pts, dirs.shape[0], axis=0), np.tile(dirs, (pts.shape[0], 1))], axis=1))
    n = LIMIT // 2
    centre, size = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    o = centre + _directions(rng, n) * size * rng.uniform(1.5, 4.0, size=(n, 1))
    d = unit(lo + (hi - lo) * rng.random((n, 3)) - o)
    d[::5] = -d[::5]
    add("far", np.concatenate([o, d], axis=1))
    # the hemisphere kind: the hit's normal turned towards the side the camera ray came from
    towards = np.where(((d_cam * pn).sum(axis=1) < 0)[:, None], pn, -pn)
    i = _pick(rng, hit)
    add("hemi", np.concatenate([p[i], towards[i]], axis=1))
    # corners: a pixel's one ray lands within NEAR of another triangle on a handful of pixels only, so the candidates are the hits of
    # CORNER_SAMPLES jittered camera rays per pixel (the oracle's own, MCPT_LENS_JITTER) on top of the pixels' pinhole rays
    osc.set_lens(jitter=True)
    pix = np.tile(np.arange(W * H, dtype=np.int32), CORNER_SAMPLES)
    jit = osc.camera_rays(seed, pix, np.repeat(np.arange(CORNER_SAMPLES, dtype=np.int32), W * H))
    osc.set_lens()
    jface, _, jp, jpn = osc.trace_closest(jit)
    cand_p, cand_f = np.concatenate([p[hit], jp[jface >= 0]]), np.concatenate([face[hit], jface[jface >= 0]])
    cand_n = np.concatenate([towards[hit], np.where(((jit[:, 3:] * jpn).sum(axis=1) < 0)[:, None], jpn, -jpn)[jface >= 0]])
    i = _pick(rng, np.flatnonzero(corner_mask(osc, cand_p, cand_f)))
    add("hemi-corner", np.concatenate([cand_p[i], cand_n[i]], axis=1))
    return out


def fold(x):
    """the header's "fold" of x (n, spp, 3) in k order: mean and standard error (include/mcpt.h: radiance queries)"""
    spp = x.shape[1]
    s1, s2 = np.zeros((x.shape[0], 3)), np.zeros((x.shape[0], 3))
    for j in range(spp):
        s1 = s1 + x[:, j]
        s2 = s2 + x[:, j] * x[:, j]
    mean = s1 / spp
    if spp < 2:
        return mean, np.zeros_like(mean)
    return mean, np.sqrt(np.maximum((s2 - s1 * s1 / spp) / (spp - 1), 0.0) / spp)


def sample_rays(group, seed, ids, k):
    """the rays of sample k (one index for all, or one per query) of the group's queries under `ids`: the list itself, or the numpy
    restatement of the hemisphere kind (tests/query_ref.py)"""
    if group.kind == "ray":
        return group.q
    return query_ref.hemisphere_rays(group.q, seed, ids, np.broadcast_to(np.asarray(k, dtype=np.int64), (group.n,)))


def oracle_samples(osc, group, seed, ids, base, spp, wrong=0, stats=None):
    """orc_ray_radiance on samples base .. base + spp - 1 of every query of the group, one call per sample index in k order:
    x (n, spp, 3), hit (n, spp), on_surface (n, spp); stats, if given, takes the sum"""
    x, hit, on = np.zeros((group.n, spp, 3)), np.zeros((group.n, spp), dtype=bool), np.zeros((group.n, spp), dtype=bool)
    for j in range(spp):
        x[:, j], hit[:, j], on[:, j] = osc.ray_radiance(seed, sample_rays(group, seed, ids, base + j), base + j, ids=ids, wrong=wrong, stats=stats)
    return x, hit, on
