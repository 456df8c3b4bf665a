"""Inputs the irradiance-volume tests share (tests/test_volume_cpu.py, tests/test_gpu_volume.py): four grids whose origins and spacings
are not dyadic, random coefficients, and a list of N receivers that holds the grid's edge cases."""
import numpy as np

N = 4001
# (nx, ny, nz) -> origin, spacing
GRIDS = {
    (1, 1, 1): ((0.1, -0.7, 1.3), (0.3, 0.37, 1.1)),
    (1, 7, 1): ((-2.3, 0.1, 5.7), (0.7, 0.3, 0.9)),
    (5, 4, 3): ((0.1, 0.2, -0.3), (0.3, 0.7, 1.1)),
    (33, 17, 9): ((-1.7, 0.123, 2.9), (0.0371, 0.113, 0.29)),
}
AXES = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])
MAX_ON_PROBES = 1500


def grid(mcpt, counts, clamp_zero=False):
    origin, spacing = GRIDS[counts]
    return mcpt.volume_grid(origin, spacing, counts, clamp_zero=clamp_zero)


def probe_points(counts):
    """the grid's positions by the header's expression (tests/volume_ref.py: points)"""
    import volume_ref
    origin, spacing = GRIDS[counts]
    return volume_ref.points(origin, spacing, counts)


def coefficients(counts, seed=0):
    """[nprobes, 9, 3]: random, both signs, a few decades"""
    rng = np.random.default_rng([seed, *counts])
    n = counts[0] * counts[1] * counts[2]
    return rng.normal(size=(n, 9, 3)) * 10.0 ** rng.uniform(-2, 1, size=(n, 1, 1))


def mask(counts, seed=0, keep=0.7):
    rng = np.random.default_rng([seed, 77, *counts])
    return (rng.random(counts[0] * counts[1] * counts[2]) < keep).astype(np.uint8)


def receivers(counts, seed=0, n=N):
    """(points [n, 3], normals [n, 3]).  The list holds: the probe positions themselves (all of them, or a random MAX_ON_PROBES where the
    grid has more: the 33 x 17 x 9 grid's 5049 do not fit, and the on-probe test takes every probe on its own); points on cell faces (one
    coordinate a probe's) and edges (two); the far corner; points outside on each of the six sides, and outside on all three axes;
    components of +-1e100 and 1e-100; random points in and a little around the grid.  Normals: random directions of length 1e-3 .. 1e3."""
    rng = np.random.default_rng([seed, 5, *counts])
    origin, spacing = (np.array(v) for v in GRIDS[counts])
    c = np.array(counts)
    pp = probe_points(counts)
    lo, hi = pp[0], pp[-1]
    span = np.maximum(hi - lo, spacing)
    parts = []
    on = pp if pp.shape[0] <= MAX_ON_PROBES else pp[rng.choice(pp.shape[0], MAX_ON_PROBES, replace=False)]
    parts.append(on)

    def inside(m):
        return lo + (hi - lo) * rng.random((m, 3))

    def snap_axes(p, axes_per_point):
        p = p.copy()
        for r in range(p.shape[0]):
            for a in rng.permutation(3)[:axes_per_point]:
                p[r, a] = origin[a] + float(rng.integers(0, c[a])) * spacing[a]
        return p
    parts.append(snap_axes(inside(300), 1))                      # cell faces
    parts.append(snap_axes(inside(300), 2))                      # cell edges
    parts.append(np.array([hi, hi + 0.5 * spacing, np.nextafter(hi, lo), np.nextafter(hi, 2 * hi - lo + 1.0)]))      # the far corner and about it
    for a in range(3):                                           # the six sides
        for sign, edge in ((-1.0, lo), (1.0, hi)):
            p = inside(40)
            p[:, a] = edge[a] + sign * span[a] * rng.uniform(1e-9, 3.0, size=40)
            parts.append(p)
    out = inside(60)                                             # outside on all three axes
    out = np.where(rng.random((60, 3)) < 0.5, lo - span * rng.random((60, 3)), hi + span * rng.random((60, 3)))
    parts.append(out)
    big = inside(90)                                             # huge and tiny components
    vals = [1e100, -1e100, 1e-100]
    for r in range(90):
        big[r, r % 3] = vals[(r // 3) % 3]
    big[-3:] = [[1e100, -1e100, 1e100], [-1e100, -1e100, -1e100], [1e-100, 1e-100, 1e-100]]
    parts.append(big)
    have = sum(p.shape[0] for p in parts)
    assert have < n
    m = n - have
    parts.append(lo - 0.25 * span + (hi - lo + 0.5 * span) * rng.random((m, 3)))
    pts = np.ascontiguousarray(np.concatenate(parts))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    nrm = d * 10.0 ** rng.uniform(-3, 3, size=(n, 1))
    nrm[:6] = AXES
    return pts, np.ascontiguousarray(nrm)
