"""Test scenes with many lights, written as .obj/.mtl/.camera (+ a .png.ppm texture) so that they load through the file surface
of both the product (mcpt.Scene) and the oracle (oracle_lib.OracleScene).

A closed room (x in [-2, 2], y in [-1, 1.5], z in [-2, 2.6]) around the origin, diffuse walls, one Phong box (Ks 0.8, Ns 60), one
textured quad; no material refracts (Ni 1 everywhere), so no path has a ray that starts on the surface it leaves.  n_lights
lights, each with its own material and radiance (two orders of magnitude apart), on the ceiling, on the walls and behind the
box, some facing away from the room.  Light meshes are one triangle, a two-triangle quad or a tessellated disc whose triangle list
starts with two zero-area triangles, has a zero-area triangle in the middle and a repeated triangle (ties and flat steps in the
light's area cdf).

variant "finite": light 0 is the smallest light; the others are exactly as large (light 1, a translated copy on a dyadic grid) or
up to ~4x larger.  The reference draws the light point with rnd = u * area(light 0) (its frozen static range), so every light
always finds a triangle and every sample is finite.
variant "nan": light 0 is the largest; the later lights are slightly smaller, so now and then rnd lands past a later light's
total area, no triangle is chosen, the light point and normal stay (0, 0, 0) and the cosine is 0 / 0: the sample goes NaN
wherever the surface faces the origin -- as in the reference."""
import math
import os

import numpy as np

ROOM = (-2.0, 2.0, -1.0, 1.5, -2.0, 2.6)
H_SLIVER = 1.0 / 16.0          # zero-area triangles: three collinear, axis-aligned points a dyadic step apart (the law of cosines
                               # in the area computation then gives cos = +-1 exactly and an area of exactly 0)


def _slots():
    """(centre, U, V, N) of every place a light may go: U, V in-plane unit axes, N the side the light faces.  In-plane centre
    coordinates are dyadic, so a translated copy of a light has exactly the same edge vectors (and area)."""
    x0, x1, y0, y1, z0, z1 = ROOM
    s = []
    for iz, z in enumerate((-1.5, -0.75, 0.0, 0.75, 1.5, 2.125)):          # ceiling: 5 x 6, facing down (every fourth faces up)
        for ix, x in enumerate((-1.5, -0.75, 0.0, 0.75, 1.5)):
            n = (0.0, 1.0, 0.0) if (ix + iz) % 4 == 3 else (0.0, -1.0, 0.0)
            s.append(((x, y1 - 0.02, z), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), n))
    for x in (-1.25, -0.25, 1.25):                                            # back wall
        for y in (-0.25, 0.75):
            s.append(((x, y, z0 + 0.02), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)))
    for z in (0.75, 1.75):                                                    # left wall (the poster is further back)
        for y in (-0.25, 0.75):
            s.append(((x0 + 0.02, y, z), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)))
    for z in (-1.25, 0.75):                                                   # right wall, the last two facing the wall
        for y in (-0.25, 0.75):
            s.append(((x1 - 0.02, y, z), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0) if z > 0 else (-1.0, 0.0, 0.0)))
    s.append(((0.75, -0.625, -1.75), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, -1.0)))   # behind the box, facing the back wall
    s.append(((-1.5, -0.625, -1.25), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)))    # a free-standing panel, low in the room
    return s


MAX_LIGHTS = len(_slots())


def _tri_area(a, b, c):
    """the reference's law-of-cosines area (what both loaders compute); used here only to size the lights"""
    la, lb, lc = np.linalg.norm(b - a), np.linalg.norm(c - a), np.linalg.norm(c - b)
    cc = (la * la + lb * lb - lc * lc) / (2 * la * lb)
    return la * lb * math.sqrt(max(0.0, 1 - cc * cc)) / 2


def _shape(kind, area, rng):
    """2-D triangles [(a, b, c)] of a light mesh of about `area` around (0, 0)"""
    if kind == "quad":
        h = math.sqrt(area) / 2
        return [((-h, -h), (h, -h), (h, h)), ((-h, -h), (h, h), (-h, h))]
    if kind == "tri":
        leg = math.sqrt(2 * area)
        return [((-leg / 2, -leg / 2), (leg / 2, -leg / 2), (-leg / 2, leg / 2))]
    n = int(rng.integers(12, 61))                        # disc: n fan triangles, 2 leading slivers, 1 in the middle, 1 repeat
    r = math.sqrt(2 * area / ((n + 1) * math.sin(2 * math.pi / n)))
    ang = rng.uniform(0, 2 * math.pi)
    rim = [(r * math.cos(ang + 2 * math.pi * i / n), r * math.sin(ang + 2 * math.pi * i / n)) for i in range(n)]
    fan = [((0.0, 0.0), rim[i], rim[(i + 1) % n]) for i in range(n)]
    h = H_SLIVER
    lead = [((0.0, 0.0), (h, 0.0), (2 * h, 0.0)), ((0.0, h), (0.0, 0.0), (0.0, 2 * h))]     # cos = 1 and cos = -1
    mid = ((-h, 0.0), (-2 * h, 0.0), (0.0, 0.0))
    rep = fan[int(rng.integers(n))]
    return lead + fan[: n // 2] + [mid, rep] + fan[n // 2:]


def _mesh_area(tris2):
    return sum(_tri_area(*(np.array(p + (0.0,)) for p in t)) for t in tris2)


def _texture(size, rng):
    y, x = np.mgrid[0:size, 0:size] / float(size)
    g = (np.floor(x * 8) + np.floor(y * 8)) % 2
    noise = rng.random((size, size))
    img = np.stack([0.2 + 0.6 * g, 0.3 + 0.4 * noise, 0.8 - 0.5 * g], -1)
    return (np.clip(img, 0, 1) * 255).astype(np.uint8)


def write(directory, name, n_lights, width, height, variant="finite", seed=1, sunk=()):
    """Write <directory>/<name>.{obj,mtl,camera} and its texture; returns the light materials' names in light order.
    sunk: indices of lights that go 0.25 below the floor instead, facing up -- below the horizon of the floor and of every other
    surface that faces up, and hidden from the whole room."""
    assert variant in ("finite", "nan")
    slots = _slots()
    assert 1 <= n_lights <= len(slots), "at most %d lights" % len(slots)
    rng = np.random.default_rng(seed * 1000 + n_lights + (0 if variant == "finite" else 500))
    x0, x1, y0, y1, z0, z1 = ROOM
    parts = []            # (material, [3-D triangle vertices], normal, uv?)

    def quad3(mat, p0, p1, p2, p3, n):
        parts.append((mat, [(p0, p1, p2), (p0, p2, p3)], n, True))

    # walls (diffuse), normals into the room
    quad3("Floor", (x0, y0, z1), (x1, y0, z1), (x1, y0, z0), (x0, y0, z0), (0, 1, 0))
    quad3("Ceiling", (x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1), (0, -1, 0))
    quad3("BackWall", (x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (0, 0, 1))
    quad3("FrontWall", (x1, y0, z1), (x0, y0, z1), (x0, y1, z1), (x1, y1, z1), (0, 0, -1))
    quad3("LeftWall", (x0, y0, z1), (x0, y0, z0), (x0, y1, z0), (x0, y1, z1), (1, 0, 0))
    quad3("RightWall", (x1, y0, z0), (x1, y0, z1), (x1, y1, z1), (x1, y1, z0), (-1, 0, 0))
    # Phong box
    bx0, bx1, by0, by1, bz0, bz1 = 0.35, 1.2, y0, -0.15, -1.45, -0.55
    quad3("Glossy", (bx0, by0, bz1), (bx1, by0, bz1), (bx1, by1, bz1), (bx0, by1, bz1), (0, 0, 1))
    quad3("Glossy", (bx1, by0, bz0), (bx0, by0, bz0), (bx0, by1, bz0), (bx1, by1, bz0), (0, 0, -1))
    quad3("Glossy", (bx0, by0, bz0), (bx0, by0, bz1), (bx0, by1, bz1), (bx0, by1, bz0), (-1, 0, 0))
    quad3("Glossy", (bx1, by0, bz1), (bx1, by0, bz0), (bx1, by1, bz0), (bx1, by1, bz1), (1, 0, 0))
    quad3("Glossy", (bx0, by1, bz1), (bx1, by1, bz1), (bx1, by1, bz0), (bx0, by1, bz0), (0, 1, 0))
    # textured quad on the left wall
    quad3("Poster", (x0 + 0.01, -0.3, -0.2), (x0 + 0.01, -0.3, -1.5), (x0 + 0.01, 0.7, -1.5), (x0 + 0.01, 0.7, -0.2), (1, 0, 0))

    # light sizes: light 0 a dyadic quad; light 1 (if any) its translated copy; the rest by variant
    base_side = 0.1875 if variant == "finite" else 0.375
    a0 = base_side * base_side
    kinds = ["quad", "quad"] + [("tri", "quad", "disc")[i % 3] for i in range(2, n_lights)]
    order = [0, 1] + list(2 + rng.permutation(len(slots) - 2))
    levels = rng.permutation(np.linspace(0.0, 1.0, n_lights)) if n_lights > 1 else [0.5]     # radiance 0.5 .. 50, spread evenly
    lights = []
    for i in range(n_lights):
        if i < 2:
            h = base_side / 2
            tris2 = [((-h, -h), (h, -h), (h, h)), ((-h, -h), (h, h), (-h, h))]
        else:
            if variant == "finite":
                f = float(rng.uniform(1.05, 4.0))
            else:                       # a ~5 % chance per vertex that some light finds no triangle, whatever the count
                f = 1.0 - (0.05 / max(1, n_lights - 1)) * float(rng.uniform(0.5, 1.5))
            tris2 = _shape(kinds[i], a0 * f, rng)
            got = _mesh_area(tris2)
            if variant == "finite":
                assert got > 1.02 * a0
            else:
                assert got < a0
        c, U, V, N = slots[order[i]]
        if i in sunk:
            c, N = (c[0], y0 - 0.25, c[2]), (0.0, 1.0, 0.0)
        c, U, V = np.array(c), np.array(U), np.array(V)
        tris3 = [tuple(tuple(c + a * U + b * V) for a, b in t) for t in tris2]
        mat = "Lamp%02d" % i
        parts.append((mat, tris3, N, False))
        rad = 10.0 ** (-0.3 + 2.0 * levels[i]) * rng.uniform(0.6, 1.0, size=3)
        lights.append((mat, [float("%.4g" % v) for v in rad]))

    tex = _texture(64, rng)
    with open(os.path.join(directory, "tex_poster.png.ppm"), "wb") as f:
        f.write(b"P6\n64 64\n255\n" + tex.tobytes())
    mats = {"Floor": ((0.7, 0.7, 0.65), (0, 0, 0), 1), "Ceiling": ((0.8, 0.8, 0.8), (0, 0, 0), 1),
            "BackWall": ((0.6, 0.65, 0.7), (0, 0, 0), 1), "FrontWall": ((0.5, 0.5, 0.5), (0, 0, 0), 1),
            "LeftWall": ((0.63, 0.065, 0.05), (0, 0, 0), 1), "RightWall": ((0.14, 0.45, 0.091), (0, 0, 0), 1),
            "Glossy": ((0.15, 0.12, 0.1), (0.8, 0.8, 0.8), 60), "Poster": ((1, 1, 1), (0, 0, 0), 1)}
    for mat, _ in lights:
        mats[mat] = ((0, 0, 0), (0, 0, 0), 1)
    with open(os.path.join(directory, name + ".mtl"), "w") as f:
        for m, (kd, ks, ns) in mats.items():
            f.write("newmtl %s\nKd %r %r %r\nKs %r %r %r\nNs %r\nNi 1\n" % (m, *map(float, kd), *map(float, ks), float(ns)))
            if m == "Poster":
                f.write("map_Kd tex_poster.png\n")
    with open(os.path.join(directory, name + ".obj"), "w") as f:
        base = 1
        for mat, tris, n, uv in parts:
            lines = []
            for t in tris:
                for p in t:
                    lines.append("v %r %r %r" % tuple(map(float, p)))
            lines += ["vn %r %r %r" % tuple(map(float, n))] * (3 * len(tris))
            for j in range(len(tris)):      # texture coordinates: the unit square over each quad, any for the lights
                lines += (["vt 0.0 0.0", "vt 1.0 0.0", "vt 1.0 1.0"] if j % 2 == 0 else ["vt 0.0 0.0", "vt 1.0 1.0", "vt 0.0 1.0"]) if uv else ["vt 0.5 0.5"] * 3
            lines.append("usemtl %s" % mat)
            for j in range(len(tris)):
                a, b, c = base + 3 * j, base + 3 * j + 1, base + 3 * j + 2
                lines.append("f %d/%d/%d %d/%d/%d %d/%d/%d" % (a, a, a, b, b, b, c, c, c))
            f.write("\n".join(lines) + "\n")
            base += 3 * len(tris)
    with open(os.path.join(directory, name + ".camera"), "w") as f:
        f.write("eye 0.1 0.15 2.4\nlookat 0.0 0.0 0.0\nup 0 1 0\nfovy 70\nwidth %d\nheight %d\n" % (width, height))
        for mat, rad in lights:
            f.write("mtlname %s %r %r %r\n" % (mat, *rad))
    return [m for m, _ in lights]
