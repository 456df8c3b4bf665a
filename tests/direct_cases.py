"""What tests/test_gpu_direct.py builds its cases from: the receivers of a camera's closest hits and a five-light mix placed inside a
scene's bounds.  No device here: the oracle's closest hit stands in for the GPU's when the occluded share of a mix is worked out on the
CPU."""
import numpy as np


def camera_receivers(rays, face, p, face_normals, count, seed):
    """`count` of the hit points of `rays` with their faces' stored normals, turned toward the ray's origin: (points, normals)"""
    hit = np.flatnonzero(face >= 0)
    pick = hit[np.random.default_rng(seed).permutation(hit.size)[:count]]
    n = face_normals[face[pick]].copy()
    back = np.einsum("ij,ij->i", n, rays[pick, 3:]) > 0
    n[back] = -n[back]
    return np.ascontiguousarray(p[pick]), np.ascontiguousarray(n)


def scene_lights(mcpt, lo, hi):
    """Five lights of all four types, both rectangle sidedness settings, inside the box lo .. hi: a point light with a range that ends
    inside the scene, a spot across it, a sun from above, a one-sided rectangle shining up and a two-sided one upright, each placed where
    cornell-box and veach-mis both see it from some of their camera's hit points and not from others."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    c, s = 0.5 * (lo + hi), hi - lo
    at = lambda fx, fy, fz: (c + s * np.array([fx, fy, fz])).tolist()
    return [mcpt.point_light(at(0.15, 0.3, 0.1), (8.0, 4.0, 2.0), range=0.9 * float(np.linalg.norm(s))),
            mcpt.rect_light(at(-0.1, -0.1, 0.3), (0.0, 0.0, 0.25 * s[2]), (0.25 * s[0], 0.0, 0.0), (3.0, 2.0, 1.0)),
            mcpt.spot_light(at(-0.35, 0.1, 0.3), (s * np.array([0.7, -0.4, -0.6])).tolist(), (5.0, 5.0, 7.0), 25.0, 45.0),
            mcpt.directional_light((0.3, -1.0, 0.2), (0.5, 0.25, 0.125)),
            mcpt.rect_light(at(0.2, -0.3, 0.2), (0.0, 0.3 * s[1], 0.0), (0.0, 0.0, 0.2 * s[2]), (1.0, 0.5, 4.0), two_sided=True)]


def bias_for(lo, hi):
    """the shadow rays' offset: a thousandth of the box's diagonal"""
    return 1e-3 * float(np.linalg.norm(np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64)))
