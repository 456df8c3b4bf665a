"""MCPT_QUERY_HEMISPHERE (include/mcpt.h: radiance queries) restated in numpy: the frame about a normal, the cosine-weighted direction
from the camera-uniform block, the ray that leaves 0.01 along it.  fp64 in the header's operation order; sin and cos are numpy's, so a
comparison with the device allows a few ulps."""
import math

import numpy as np

import lens_ref

OFFSET = 0.01
TWO_PI = 6.283185307179586


def _nrm(a):
    d = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    return a / d[:, None]


def _cross(a, b):
    """Vertex::cross as dev_common.hpp writes it"""
    return np.stack([a[:, 1] * b[:, 2] - b[:, 1] * a[:, 2], b[:, 0] * a[:, 2] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]], axis=1)


def basis(normals):
    """(t, s, n^) per normal: n^ = b / |b|; e = the coordinate axis on which |n^| is smallest, the lowest among equals;
    t = normalize(cross(e, n^)), s = cross(n^, t)"""
    n = _nrm(np.asarray(normals, dtype=np.float64).reshape(-1, 3))
    axis = np.argmin(np.abs(n), axis=1)             # the first of equal minima
    e = np.zeros_like(n)
    e[np.arange(n.shape[0]), axis] = 1.0
    t = _nrm(_cross(e, n))
    s = _cross(n, t)
    return t, s, n


def hemisphere_rays(q6, seed, ids, k):
    """[n, 6] = origin, direction of sample k[i] of hemisphere query i (position, normal) with id ids[i]"""
    q6 = np.asarray(q6, dtype=np.float64).reshape(-1, 6)
    a = q6[:, :3]
    t, s, n = basis(q6[:, 3:])
    u0, u1, _, _ = lens_ref.camera_uniforms(seed, np.asarray(ids, dtype=np.int64), np.asarray(k, dtype=np.int64))
    r = np.sqrt(u0)
    phi = TWO_PI * u1
    z = np.sqrt(np.maximum(0.0, 1.0 - u0))
    x, y = r * np.cos(phi), r * np.sin(phi)
    d = _nrm((t * x[:, None] + s * y[:, None]) + n * z[:, None])
    o = a + d * OFFSET
    return np.concatenate([o, d], axis=1)


def ulps(a, b):
    """|a - b| per component in ulps of the largest component of its 3-vector (origin, direction): the measure the thin lens's rays are
    held to (tests/test_gpu_lens.py: _ulps)"""
    out = np.zeros(a.shape)
    for part in (slice(0, 3), slice(3, 6)):
        scale = np.spacing(np.abs(b[:, part]).max(axis=1))[:, None]
        out[:, part] = np.abs(a[:, part] - b[:, part]) / scale
    return out


def rect_form_factor(a, b, h):
    """the form factor from a surface element to a parallel rectangle of sides a, b at height h above it, one corner over the element"""
    X, Y = a / h, b / h
    return (1.0 / (2.0 * math.pi)) * (X / math.sqrt(1 + X * X) * math.atan(Y / math.sqrt(1 + X * X))
                                      + Y / math.sqrt(1 + Y * Y) * math.atan(X / math.sqrt(1 + Y * Y)))


def square_form_factor(x, z, half, h):
    """... to the square [-half, half]^2 at height h from the point (x, z) under it: the sum over the four corner rectangles"""
    return sum(rect_form_factor(a, b, h) for a in (half - x, half + x) for b in (half - z, half + z))
