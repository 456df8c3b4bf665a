"""Irradiance volumes (include/mcpt.h: irradiance volumes) restated in numpy: the positions of a probe grid and the trilinear lookup
between its probes, vectorised over the receivers, fp64 in the header's operation order.  Every operation is an IEEE add, multiply,
divide, square root or floor, so the library's answers are these bit for bit."""
import numpy as np

import sh_ref


def points(origin, spacing, counts):
    """[nz * ny * nx, 3]: probe (ix, iy, iz) at row (iz * ny + iy) * nx + ix"""
    nx, ny, nz = counts
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([origin[a] + i.reshape(-1).astype(np.float64) * spacing[a] for a, i in enumerate((ix, iy, iz))], axis=1)


def axis(x, origin, spacing, n, snap=True):
    """(i0, i1, w0, w1) of coordinates x along an axis of n probes; snap=False leaves the header's snap out (to show what it is for)"""
    g = (x - origin) / spacing
    g = np.where(g > 0.0, g, 0.0)
    g = np.where(g < float(n - 1), g, float(n - 1))
    if n == 1:
        i0 = np.zeros(x.shape, dtype=np.int64)
        return i0, i0, 1.0 - np.zeros(x.shape), np.zeros(x.shape)
    i0 = np.minimum(np.floor(g).astype(np.int64), n - 2)
    f = g - i0.astype(np.float64)
    if snap:
        on0 = x == origin + i0.astype(np.float64) * spacing
        on1 = x == origin + (i0 + 1).astype(np.float64) * spacing
        f = np.where(on0, 0.0, np.where(on1, 1.0, f))
    return i0, i0 + 1, 1.0 - f, f


def corners(origin, spacing, counts, x, valid=None, snap=True):
    """(P [n, 8], w [n, 8], lit [n]): the corners' probes and weights after the mask, and whether anything is left"""
    nx, ny, nz = counts
    ax = [axis(x[:, a], origin[a], spacing[a], counts[a], snap) for a in range(3)]
    P, w = [], []
    for j in range(8):
        dx, dy, dz = j & 1, (j >> 1) & 1, j >> 2
        P.append((ax[2][dz] * ny + ax[1][dy]) * nx + ax[0][dx])
        w.append((ax[0][2 + dx] * ax[1][2 + dy]) * ax[2][2 + dz])
    P, w = np.stack(P, axis=1), np.stack(w, axis=1)
    lit = np.ones(x.shape[0], dtype=bool)
    if valid is not None:
        w = np.where(np.asarray(valid).reshape(-1)[P] == 0, 0.0, w)
        W = np.zeros(x.shape[0])
        for j in range(8):
            W = W + w[:, j]
        lit = W > 0.0
        w = np.where(lit[:, None], w / np.where(lit, W, 1.0)[:, None], 0.0)
    return P, w, lit


def irradiance(origin, spacing, counts, sh, x, b, valid=None, clamp_zero=False, snap=True):
    """(E [n, 3], corners [n]) of receivers at x [n, 3] with normals b [n, 3]; sh [nprobes, 9, 3]"""
    sh = np.asarray(sh, dtype=np.float64).reshape(-1, 9, 3)
    x, b = np.asarray(x, dtype=np.float64), np.asarray(b, dtype=np.float64)
    P, w, lit = corners(origin, spacing, counts, x, valid, snap)
    c = np.zeros((x.shape[0], 9, 3))
    for j in range(8):
        c = c + w[:, j, None, None] * sh[P[:, j]]
    E = sh_ref.irradiance(c, b)
    E = np.where(lit[:, None], E, 0.0)
    if clamp_zero:
        E = np.where(E > 0.0, E, 0.0)
    return E, (w > 0.0).sum(axis=1).astype(np.int32)
