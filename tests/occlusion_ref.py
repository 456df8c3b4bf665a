"""Ambient occlusion (include/mcpt.h: ambient occlusion) restated in numpy: the fold of an entry's traced rays into its occlusion, standard
error, bent normal and hit counts -- the sums in a Python loop over the samples, in sample order --, and the lightmap's dilation rule on one channel.
fp64 in the header's operation order: every operation is an IEEE add, multiply, divide or square root, so the library's answers are these
bit for bit."""
import numpy as np

HARD, LINEAR, SQUARE = 0, 1, 2
FALLOFFS = {"hard": HARD, "linear": LINEAR, "square": SQUARE}


def n_hat(b):
    """the hemisphere rule's unit normal of b [3]"""
    b = np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        return b / np.sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2])


def fold(q6, rays6, hit, t, n3, spp, max_distance, falloff):
    """The fold of n entries q6 [n, 6] over their n * spp rays, sample j of entry i at i * spp + j: rays6 [n * spp, 6], hit [n * spp]
    whether each ray hit anything, t [n * spp] the hits' distances, n3 [n * spp, 3] the hit triangles' stored face normals (anything
    where the ray missed).  The sums run in a Python loop over the samples, in sample order, for all entries at once.  Returns a dict
    like Device.occlusion's: ao [n], stderr [n], bent [n, 3], hits [n], back [n]."""
    falloff = FALLOFFS.get(falloff, falloff)
    q6 = np.asarray(q6, dtype=np.float64).reshape(-1, 6)
    n = q6.shape[0]
    d = np.asarray(rays6, dtype=np.float64).reshape(n, spp, 6)[:, :, 3:]
    hit = np.asarray(hit).reshape(n, spp) != 0
    t = np.asarray(t, dtype=np.float64).reshape(n, spp)
    nrm = np.asarray(n3, dtype=np.float64).reshape(n, spp, 3)
    md = np.float64(max_distance)
    s1, s2, b = np.zeros(n), np.zeros(n), np.zeros((n, 3))
    hits, back = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    with np.errstate(all="ignore"):
        for j in range(spp):
            near = hit[:, j] & (t[:, j] < md)
            x = t[:, j] / md
            v = np.where(near, 0.0 * np.zeros(n) if falloff == HARD else (x if falloff == LINEAR else x * x), 1.0)
            s1 = s1 + v
            s2 = s2 + v * v
            b = b + d[:, j] * v[:, None]
            hits += near
            dot = (d[:, j, 0] * nrm[:, j, 0] + d[:, j, 1] * nrm[:, j, 1]) + d[:, j, 2] * nrm[:, j, 2]
            back += near & (dot > 0.0)
        ao = s1 / np.float64(spp)
        err = np.zeros(n)
        if spp >= 2:
            var = (s2 - s1 * s1 / np.float64(spp)) / np.float64(spp - 1)
            err = np.sqrt(np.where(var > 0.0, var, 0.0) / np.float64(spp))
        l = np.sqrt((b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2])
        own = (l > 0.0) & np.isfinite(l)
        nb = q6[:, 3:]
        nl = np.sqrt((nb[:, 0] * nb[:, 0] + nb[:, 1] * nb[:, 1]) + nb[:, 2] * nb[:, 2])
        bent = np.where(own[:, None], b / l[:, None], nb / nl[:, None])
    return {"ao": ao, "stderr": err, "bent": bent, "hits": hits, "back": back}


def fold_entry(normal, d, hit, t, nrm, max_distance, falloff):
    """One entry: normal [3] its own, d [spp, 3] its rays' directions in sample order, hit, t and nrm as fold's.  Returns (ao, stderr,
    bent [3], hits, back)."""
    d = np.asarray(d, dtype=np.float64)
    q6 = np.concatenate([np.zeros(3), np.asarray(normal, dtype=np.float64)])[None]
    o = fold(q6, np.concatenate([np.zeros_like(d), d], axis=1), hit, t, nrm, d.shape[0], max_distance, falloff)
    return o["ao"][0], o["stderr"][0], o["bent"][0], int(o["hits"][0]), int(o["back"][0])


def dilate(ao, owner, rounds):
    """The lightmap's dilation on one channel: ao [H, W], owner [H, W] (>= 0: a face, -1: not covered).  In round r every texel whose
    owner is -1 and that has c >= 1 neighbours (dy, dx in -1 .. 1, row-major, inside the map) with another owner becomes s / c, s = 0.0
    plus their values of the round before in that order, and its owner -1 - r.  Returns (ao, owner) after `rounds` rounds."""
    ao, owner = np.array(ao, dtype=np.float64), np.array(owner, dtype=np.int32)
    H, W = owner.shape
    for r in range(1, rounds + 1):
        a2, o2 = ao.copy(), owner.copy()
        for y, x in zip(*np.nonzero(owner == -1)):
            s, c = np.float64(0.0), 0
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and owner[yy, xx] != -1:
                        s = s + ao[yy, xx]
                        c += 1
            if c > 0:
                a2[y, x] = s / np.float64(c)
                o2[y, x] = -1 - r
        ao, owner = a2, o2
    return ao, owner


def scatter(shape, texels, answers):
    """the answers of a texel list (a dict like fold's) put into maps of shape (H, W), +0.0 and 0 elsewhere"""
    H, W = shape
    out = {"ao": np.zeros(H * W), "stderr": np.zeros(H * W), "bent": np.zeros((H * W, 3)), "hits": np.zeros(H * W, dtype=np.int32),
           "back": np.zeros(H * W, dtype=np.int32)}
    for k in out:
        out[k][texels] = answers[k]
    return {k: v.reshape((H, W) + v.shape[1:]) for k, v in out.items()}
