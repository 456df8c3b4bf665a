"""Probe visibility (include/mcpt.h: probe visibility) restated in numpy: the octahedral bin of a direction, the fold of a probe's traced
rays into depth moments and hit counts (the sums in a Python loop, in sample order), and the irradiance volume's lookup with a factor
per corner, vectorised over the receivers.  fp64 in the header's operation order: every operation is an IEEE add, multiply, divide,
square root or floor, so the library's answers are these bit for bit."""
import numpy as np

import sh_ref
import volume_ref


def bin_of(d, R):
    """[n] the bin of every direction d [n, 3] (finite, not zero) in an R x R map"""
    d = np.asarray(d, dtype=np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    l = (np.abs(x) + np.abs(y)) + np.abs(z)
    u, v = x / l, y / l
    fu = (1.0 - np.abs(v)) * np.where(u >= 0.0, 1.0, -1.0)
    fv = (1.0 - np.abs(u)) * np.where(v >= 0.0, 1.0, -1.0)
    u, v = np.where(z < 0.0, fu, u), np.where(z < 0.0, fv, v)
    bx = np.clip(np.floor((u * 0.5 + 0.5) * float(R)).astype(np.int64), 0, R - 1)
    by = np.clip(np.floor((v * 0.5 + 0.5) * float(R)).astype(np.int64), 0, R - 1)
    return (by * R + bx).astype(np.int32)


def fold(d, hit, t, nrm, R, max_distance, max_back_fraction):
    """One probe: d [spp, 3] its rays' directions in sample order, hit [spp] whether each hit anything, t [spp] the hits' distances, nrm
    [spp, 3] the hit triangles' stored face normals (anything where the ray missed).  Returns (moments [R * R, 2], hits, back, valid)."""
    spp = d.shape[0]
    b = bin_of(d, R)
    c = np.zeros(R * R, dtype=np.int64)
    s1, s2 = np.zeros(R * R), np.zeros(R * R)
    hits = back = 0
    for k in range(spp):
        h = bool(hit[k])
        hits += h
        dot = (d[k, 0] * nrm[k, 0] + d[k, 1] * nrm[k, 1]) + d[k, 2] * nrm[k, 2]
        back += bool(h and dot > 0.0)
        r = (t[k] if t[k] < max_distance else max_distance) if h else max_distance
        r = np.float64(r)
        c[b[k]] += 1
        s1[b[k]] = s1[b[k]] + r
        s2[b[k]] = s2[b[k]] + r * r
    m = np.empty((R * R, 2))
    some = c > 0
    cs = np.where(some, c, 1).astype(np.float64)
    m[:, 0] = np.where(some, s1 / cs, -1.0)
    m[:, 1] = np.where(some, s2 / cs, 0.0)
    return m, hits, back, 1 if float(back) <= max_back_fraction * float(spp) else 0


def factors(origin, spacing, counts, moments, x, b, R, max_distance, normal_bias, min_visibility):
    """(P [n, 8], w [n, 8] the trilinear weights before any mask, f [n, 8] the corners' factors)"""
    nx, ny, nz = counts
    n = x.shape[0]
    moments = np.asarray(moments, dtype=np.float64).reshape(-1, R * R, 2)
    ax = [volume_ref.axis(x[:, a], origin[a], spacing[a], counts[a]) for a in range(3)]
    l = np.sqrt((b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2])
    xb = np.stack([x[:, a] + (b[:, a] / l) * normal_bias for a in range(3)], axis=1)
    P, w, f = [], [], []
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(8):
            dj = (j & 1, (j >> 1) & 1, j >> 2)
            Pj = (ax[2][dj[2]] * ny + ax[1][dj[1]]) * nx + ax[0][dj[0]]
            wj = (ax[0][2 + dj[0]] * ax[1][2 + dj[1]]) * ax[2][2 + dj[2]]
            c = [origin[a] + ax[a][dj[a]].astype(np.float64) * spacing[a] for a in range(3)]
            vx, vy, vz = xb[:, 0] - c[0], xb[:, 1] - c[1], xb[:, 2] - c[2]
            dist = np.sqrt((vx * vx + vy * vy) + vz * vz)
            near = dist == 0.0
            sd = np.where(near, 1.0, dist)
            dirs = np.stack([np.where(near, 1.0, vx / sd), np.where(near, 0.0, vy / sd), np.where(near, 0.0, vz / sd)], axis=1)
            bj = bin_of(dirs, R)
            mu, m2 = moments[Pj, bj, 0], moments[Pj, bj, 1]
            dc = np.where(dist < max_distance, dist, max_distance)
            var = m2 - mu * mu
            var = np.where(var > 0.0, var, 0.0)
            delta = dc - mu
            ch = var / (var + delta * delta)
            fj = (ch * ch) * ch
            fj = np.where(near | (mu < 0.0) | (dc <= mu), 1.0, fj)
            fj = np.where(fj > min_visibility, fj, min_visibility)
            P.append(Pj), w.append(wj), f.append(fj)
    return np.stack(P, axis=1), np.stack(w, axis=1), np.stack(f, axis=1)


def irradiance(origin, spacing, counts, sh, moments, x, b, R, max_distance, normal_bias=0.0, min_visibility=0.0, valid=None, clamp_zero=False):
    """(E [n, 3], corners [n]) of receivers at x [n, 3] with normals b [n, 3]; sh [nprobes, 9, 3], moments [nprobes, R * R, 2]"""
    sh = np.asarray(sh, dtype=np.float64).reshape(-1, 9, 3)
    x, b = np.asarray(x, dtype=np.float64), np.asarray(b, dtype=np.float64)
    P, w, f = factors(origin, spacing, counts, moments, x, b, R, max_distance, normal_bias, min_visibility)
    if valid is not None:
        w = np.where(np.asarray(valid).reshape(-1)[P] == 0, 0.0, w)
    w = w * f
    W = np.zeros(x.shape[0])
    for j in range(8):
        W = W + w[:, j]
    lit = W > 0.0
    w = np.where(lit[:, None], w / np.where(lit, W, 1.0)[:, None], 0.0)
    c = np.zeros((x.shape[0], 9, 3))
    for j in range(8):
        c = c + w[:, j, None, None] * sh[P[:, j]]
    E = sh_ref.irradiance(c, b)
    E = np.where(lit[:, None], E, 0.0)
    if clamp_zero:
        E = np.where(E > 0.0, E, 0.0)
    return E, (w > 0.0).sum(axis=1).astype(np.int32)
