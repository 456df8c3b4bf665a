"""Light probes (include/mcpt.h: light probes) restated in numpy: the uniform sphere draw from the camera-uniform block, the real
spherical-harmonic basis of bands 0..2, the radiance and the irradiance a probe's coefficients give, and the fold of a probe's samples.
fp64 in the header's index order and operation order; sin and cos are numpy's, so a comparison of rays with the device allows a few ulps."""
import numpy as np

import lens_ref

TWO_PI = 6.283185307179586
FOUR_PI = 12.566370614359172
C0 = 0.28209479177387814         # 1 / (2 sqrt(pi))
C1 = 0.4886025119029199          # sqrt(3 / (4 pi))
C2 = 1.0925484305920792          # sqrt(15 / (4 pi))
C3 = 0.31539156525252005         # sqrt(5 / (16 pi))
C4 = 0.5462742152960396          # sqrt(15 / (16 pi))
A = np.array([3.141592653589793] + [2.0943951023931953] * 3 + [0.7853981633974483] * 5)     # A_l of coefficient i
BAND = np.array([0, 1, 1, 1, 2, 2, 2, 2, 2])


def _nrm(a):
    d = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    return a / d[:, None]


def sphere_dirs(seed, ids, k):
    """[n, 3]: the direction of sample k[i] of the probe with id ids[i]"""
    u0, u1, _, _ = lens_ref.camera_uniforms(seed, np.asarray(ids, dtype=np.int64), np.asarray(k, dtype=np.int64))
    z = 1.0 - 2.0 * u0
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    phi = TWO_PI * u1
    return _nrm(np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1))


def probe_rays(points, seed, ids, k):
    """[n, 6] = origin (the point itself), direction"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    return np.concatenate([p, sphere_dirs(seed, ids, k)], axis=1)


def basis(d):
    """[n, 9]: Y_0..8 of the unit directions d [n, 3]"""
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return np.stack([np.full(x.shape, C0), C1 * y, C1 * z, C1 * x, C2 * (x * y), C2 * (y * z), C3 * (3.0 * (z * z) - 1.0), C2 * (x * z),
                     C4 * (x * x - y * y)], axis=1)


def radiance(sh, d):
    """[n, 3]: sum_i sh[:, i, :] * Y_i(d), in index order from 0.0"""
    Y = basis(d)
    out = np.zeros((Y.shape[0], 3))
    for i in range(9):
        out = out + sh[:, i, :] * Y[:, i, None]
    return out


def irradiance(sh, normals):
    """[n, 3]: sum_i (A_l(i) * Y_i(n^)) * sh[:, i, :], in index order from 0.0, n^ = n / |n|"""
    Y = basis(_nrm(np.asarray(normals, dtype=np.float64).reshape(-1, 3)))
    out = np.zeros((Y.shape[0], 3))
    for i in range(9):
        out = out + (A[i] * Y[:, i])[:, None] * sh[:, i, :]
    return out


def fold(x, d):
    """The probe fold of samples x [spp][n, 3] with directions d [spp][n, 3], in k order: (sh [n, 9, 3], stderr [n, 9, 3])"""
    spp = len(x)
    n = x[0].shape[0]
    s1, s2 = np.zeros((n, 9, 3)), np.zeros((n, 9, 3))
    for k in range(spp):
        v = x[k][:, None, :] * basis(d[k])[:, :, None]
        s1 = s1 + v
        s2 = s2 + v * v
    sh = FOUR_PI * (s1 / spp)
    if spp < 2:
        return sh, np.zeros((n, 9, 3))
    var = (s2 - s1 * s1 / spp) / (spp - 1)
    return sh, FOUR_PI * np.sqrt(np.maximum(var, 0.0) / spp)
