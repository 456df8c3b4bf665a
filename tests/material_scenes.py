"""Test scenes of material edge cases, written as .obj/.mtl/.camera (+ .png.ppm textures) so that they load through the file surface of
both the product (mcpt.Scene) and the oracle (oracle_lib.OracleScene) -- like light_scenes.py, whose "finite" regime this keeps.

A closed diffuse room (x in [-2, 2], y in [-1.2, 1.3], z in [-2, 2.6]) with two equal dyadic quad lights on the ceiling, one in front of
the swatches and one behind them, so that the far faces of a body -- where a ray that went in meets the surface from inside -- are lit
too (light 1 is a translated copy of light 0: the reference's frozen light-area range never runs past a light, no sample goes NaN).  The camera looks
down -z at a 6 x 3 grid of swatches that float in front of the back wall.  Each swatch is one material on its own small closed body -- a
box turned about x and y, so that no face is axis-aligned and lit bounce rays leave it towards the room; G6 is an icosphere of 80 faces.

variant "opaque": rows O1-O11; no material refracts, so no path has a ray that starts on the surface it leaves.
variant "glass":  O1-O11 and G1-G6.

ROWS is the table: name, what the row probes, its material, and its sibling -- the same material with the edge parameter moved to the
nearest ordinary value.  write(..., siblings={row: True}) swaps the named rows for their siblings; the geometry stays (G6's sibling has
the same faces with flat normals), so a row covers the same pixels in both.

O5 is written as it was asked for (Kd .8, Ks .3, Ns 20).  With |Kd| / |Ks| = 2.7 it is never specular -- O6's regime at another ratio;
materials that take both lobes are O2, O3, O4 and O10 (|Kd| / |Ks| = 0.16) and the mid texels of O7."""
import math
import os

import numpy as np

ROOM = (-2.0, 2.0, -1.2, 1.3, -2.0, 2.6)
LIGHT_SIDE = 0.5
LIGHT_CENTRES = ((0.0, 1.28, 1.0), (0.0, 1.28, -1.5))          # in front of the swatches and behind them: back faces are lit too
LIGHT_RADIANCE = ((12.0, 11.0, 9.0), (6.0, 8.0, 10.0))
GRID_X = (-1.35, -0.81, -0.27, 0.27, 0.81, 1.35)
GRID_Y = (0.77, 0.05, -0.67)
GRID_Z = -0.8
BOX_HALF = 0.19
SPHERE_RADIUS = 0.25
VT_LO, VT_HI = -0.75, 1.5            # texture coordinates over every quad of a body: floor wraps on both sides

GLOSSY_KD = (0.15, 0.12, 0.1)

# 5 x 3 (width x height): a black texel, a white texel, mid texels (R, G, B)
TEX_SWATCH = np.array([[(0, 0, 0), (255, 255, 255), (128, 64, 32), (40, 90, 200), (90, 90, 90)],
                       [(200, 180, 20), (16, 16, 16), (255, 0, 0), (60, 140, 60), (230, 230, 230)],
                       [(10, 120, 110), (140, 30, 160), (75, 75, 20), (255, 255, 255), (0, 0, 0)]], dtype=np.uint8)
# 3 x 2: mid texels only
TEX_GLASS = np.array([[(200, 40, 40), (40, 200, 40), (40, 40, 200)], [(120, 120, 20), (20, 120, 120), (160, 160, 160)]], dtype=np.uint8)
TEXTURES = {"tex_swatch.png": TEX_SWATCH, "tex_glass.png": TEX_GLASS}


def _mean_colour(tex):
    return tuple(float(v) for v in tex.reshape(-1, 3).astype(np.float64).mean(axis=0) / 255.0)


def _mat(kd, ks=0.0, ns=1.0, ni=1.0, tex=None):
    kd = (kd,) * 3 if np.isscalar(kd) else tuple(kd)
    ks = (ks,) * 3 if np.isscalar(ks) else tuple(ks)
    return dict(kd=tuple(map(float, kd)), ks=tuple(map(float, ks)), ns=float(ns), ni=float(ni), tex=tex)


# (row, what it probes, material, what the sibling is, the sibling's material)
# special siblings: "not-a-light" -- the body takes a twin material that is no emitter; "flat" -- the same faces with face normals
ROWS = [
    ("O1", "Kd 0 with Ks: always the specular lobe, a near-mirror exponent", _mat(0.0, 0.8, 1e4),
     "Kd .15 .12 .1", _mat(GLOSSY_KD, 0.8, 1e4)),
    ("O2", "Ns 0: cos = pow(u, 1), a lobe that is uniform in cos and dips below the horizon", _mat(GLOSSY_KD, 0.8, 0.0),
     "Ns 60", _mat(GLOSSY_KD, 0.8, 60.0)),
    ("O3", "Ns 0.5: a fractional exponent, pow(u, 1 / 1.5)", _mat(GLOSSY_KD, 0.8, 0.5),
     "Ns 60", _mat(GLOSSY_KD, 0.8, 60.0)),
    ("O4", "Ns 3: a low exponent", _mat(GLOSSY_KD, 0.8, 3.0),
     "Ns 60", _mat(GLOSSY_KD, 0.8, 60.0)),
    ("O5", "Kd .8 Ks .3 Ns 20 as asked for: |Kd| / |Ks| = 2.7, the lobe test always false", _mat(0.8, 0.3, 20.0),
     "Kd .2", _mat(0.2, 0.3, 20.0)),
    ("O6", "Ks != 0 and |Kd| >= |Ks|: never specular", _mat(0.9, 0.5, 60.0),
     "Kd .3", _mat(0.3, 0.5, 60.0)),
    ("O7", "a texel's kd in the lobe choice: black, white and mid texels, vt from -0.75 to 1.5", _mat(1.0, 0.5, 30.0, tex="tex_swatch.png"),
     "the map's mean colour as Kd", _mat(_mean_colour(TEX_SWATCH), 0.5, 30.0)),
    ("O8", "Kd 0 Ks 0: black, every weight 0", _mat(0.0, 0.0, 1.0),
     "Kd .5", _mat(0.5, 0.0, 1.0)),
    ("O9", "Kd 1.5 .2 .2: a channel above 1", _mat((1.5, 0.2, 0.2), 0.0, 1.0),
     "Kd 1 .2 .2", _mat((1.0, 0.2, 0.2), 0.0, 1.0)),
    ("O10", "Ni 0.8: opaque, the test is Ni > 1", _mat(GLOSSY_KD, 0.8, 60.0, 0.8),
     "Ni 1", _mat(GLOSSY_KD, 0.8, 60.0, 1.0)),
    ("O11", "light 1's material with Ks, Ns, Ni > 1 and a map: the light check comes first", _mat(0.5, 0.5, 10.0, 1.5, tex="tex_swatch.png"),
     "the same record on a material that is no light", "not-a-light"),
    ("G1", "Ni 1.0001: rf0 2.5e-9, refract_dir's float cost2 at its threshold", _mat(GLOSSY_KD, 0.8, 60.0, 1.0001),
     "Ni 1", _mat(GLOSSY_KD, 0.8, 60.0, 1.0)),
    ("G2", "Ni 1.33 with Ks 0: the Fresnel-reflect case falls through to a diffuse lobe on glass", _mat((0.6, 0.7, 0.8), 0.0, 1.0, 1.33),
     "Ks .8 Ns 60", _mat((0.6, 0.7, 0.8), 0.8, 60.0, 1.33)),
    ("G3", "Ni 2.417 Ks .9 Ns 500: total reflection from 24.4 degrees", _mat(0.1, 0.9, 500.0, 2.417),
     "Ni 1.5", _mat(0.1, 0.9, 500.0, 1.5)),
    ("G4", "Ni 10: rf0 0.67, total reflection from 5.7 degrees", _mat(GLOSSY_KD, 0.8, 60.0, 10.0),
     "Ni 1.5", _mat(GLOSSY_KD, 0.8, 60.0, 1.5)),
    ("G5", "Ni 1.5 with a map: a texel's kd on glass", _mat(1.0, 0.8, 60.0, 1.5, tex="tex_glass.png"),
     "the map's mean colour as Kd", _mat(_mean_colour(TEX_GLASS), 0.8, 60.0, 1.5)),
    ("G6", "Ni 1.5 on an icosphere with per-vertex normals: cos_in and the refraction normal from pn", _mat(GLOSSY_KD, 0.8, 60.0, 1.5),
     "flat normals", "flat"),
]
ROW_NAMES = [r[0] for r in ROWS]
OPAQUE_ROWS = [r for r in ROW_NAMES if r.startswith("O")]
GLASS_ROWS = [r for r in ROW_NAMES if r.startswith("G")]
VARIANTS = {"opaque": OPAQUE_ROWS, "glass": OPAQUE_ROWS + GLASS_ROWS}
# the slot of each row in the grid (column, line): the glass bodies on the bottom line
SLOT = {r: (i % 6, i // 6) for i, r in enumerate(OPAQUE_ROWS)}
SLOT.update({r: (i, 2) for i, r in enumerate(GLASS_ROWS)})
SLOT["O11"] = (5, 1)
# bodies that differ from the common box (half = BOX_HALF, turned -22..-28 degrees about x and -24..26 about y).  G4: thicker and turned
# less, so that its faces are met less grazingly -- on the common box 4 of its 78 on-surface samples left REL_TOL on the GPU, one more than
# test_gpu_materials.py's allowance, every one of them on a path with an on-surface ray (test_gpu_parity.py's refraction flips)
BODY = {"G4": dict(half=0.22, turn=(-12.0, 8.0))}


def centre(row):
    cx, cy = SLOT[row]
    return np.array([GRID_X[cx], GRID_Y[cy], GRID_Z])


def half_size(row):
    return BODY.get(row, {}).get("half", BOX_HALF)


def inner_radius(row):
    """the radius of a ball around centre(row) that lies inside the row's body"""
    return 0.9 * (half_size(row) if row != "G6" else SPHERE_RADIUS * 0.9)


def _rotation(row):
    i = ROW_NAMES.index(row)
    ax, ay = BODY.get(row, {}).get("turn", (-22.0 - 3.0 * (i % 3), (-24.0, -12.0, 14.0, 26.0)[i % 4]))
    ax, ay = math.radians(ax), math.radians(ay)
    rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
    ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    return ry @ rx


def _box(c, half, rot):
    """[(triangle, normals, uvs)] of a closed box: 12 triangles wound counter-clockwise seen from outside"""
    out = []
    uv = ((VT_LO, VT_LO), (VT_HI, VT_LO), (VT_HI, VT_HI), (VT_LO, VT_HI))
    for a in range(3):
        b, d = (a + 1) % 3, (a + 2) % 3
        for s in (1.0, -1.0):
            corners = ((-1, -1), (1, -1), (1, 1), (-1, 1)) if s > 0 else ((-1, -1), (-1, 1), (1, 1), (1, -1))
            q = []
            for sb, sd in corners:
                v = np.zeros(3)
                v[a], v[b], v[d] = s * half, sb * half, sd * half
                q.append(c + rot @ v)
            n = rot[:, a] * s
            for i0, i1, i2 in ((0, 1, 2), (0, 2, 3)):
                out.append(((q[i0], q[i1], q[i2]), (n, n, n), (uv[i0], uv[i1], uv[i2])))
    return out


def _icosphere(c, radius, rot, smooth):
    """80 triangles: an icosahedron, every face split in four, on the sphere; normals per vertex (smooth) or per face"""
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    unit = lambda x: x / np.linalg.norm(x)
    v = [unit(rot @ np.array(p, dtype=np.float64)) for p in v]
    out = []
    for i0, i1, i2 in f:
        a, b, d = v[i0], v[i1], v[i2]
        ab, bd, da = unit(a + b), unit(b + d), unit(d + a)
        for tri in ((a, ab, da), (b, bd, ab), (d, da, bd), (ab, bd, da)):
            if np.dot(np.cross(tri[1] - tri[0], tri[2] - tri[0]), tri[0] + tri[1] + tri[2]) < 0:
                tri = (tri[0], tri[2], tri[1])
            pts = tuple(c + radius * p for p in tri)
            fn = unit(np.cross(pts[1] - pts[0], pts[2] - pts[0]))
            nrm = tri if smooth else (fn, fn, fn)
            uvs = tuple((VT_LO + (VT_HI - VT_LO) * (0.5 + 0.5 * p[0]), VT_LO + (VT_HI - VT_LO) * (0.5 + 0.5 * p[1])) for p in tri)
            out.append((pts, nrm, uvs))
    return out


def write(directory, name, width, height, variant="glass", siblings=None):
    """Write <directory>/<name>.{obj,mtl,camera} and the textures.  Returns {"lights": the light materials' names in light order,
    "rows": {row: (first face, number of faces)} in the file's face order}."""
    rows = VARIANTS[variant]
    siblings = {r: bool(v) for r, v in (siblings or {}).items()}
    assert set(siblings) <= set(rows), "siblings name rows of the variant"
    x0, x1, y0, y1, z0, z1 = ROOM
    parts = []            # (material, [(triangle, normals, uvs)])
    unit_uv = ((0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0))

    def quad3(mat, p0, p1, p2, p3, n, uv=unit_uv):
        q = [np.array(p, dtype=np.float64) for p in (p0, p1, p2, p3)]
        n = np.array(n, dtype=np.float64)
        parts.append((mat, [((q[a], q[b], q[c]), (n, n, n), (uv[a], uv[b], uv[c])) for a, b, c in ((0, 1, 2), (0, 2, 3))]))

    quad3("Floor", (x0, y0, z1), (x1, y0, z1), (x1, y0, z0), (x0, y0, z0), (0, 1, 0))
    quad3("Ceiling", (x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1), (0, -1, 0))
    quad3("BackWall", (x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (0, 0, 1))
    quad3("FrontWall", (x1, y0, z1), (x0, y0, z1), (x0, y1, z1), (x1, y1, z1), (0, 0, -1))
    quad3("LeftWall", (x0, y0, z1), (x0, y0, z0), (x0, y1, z0), (x0, y1, z1), (1, 0, 0))
    quad3("RightWall", (x1, y0, z0), (x1, y0, z1), (x1, y1, z1), (x1, y1, z0), (-1, 0, 0))
    # the two lights: dyadic quads facing down; light 1's material is row O11's
    light_names = ("Lamp00", "O11")
    h = LIGHT_SIDE / 2
    flat_uv = ((0.5, 0.5),) * 4
    for mat, (cx, cy, cz) in zip(light_names, LIGHT_CENTRES):
        quad3(mat, (cx - h, cy, cz - h), (cx + h, cy, cz - h), (cx + h, cy, cz + h), (cx - h, cy, cz + h), (0, -1, 0), uv=flat_uv)

    mats = {"Floor": _mat((0.7, 0.7, 0.65)), "Ceiling": _mat(0.8), "BackWall": _mat((0.6, 0.65, 0.7)), "FrontWall": _mat(0.5),
            "LeftWall": _mat((0.63, 0.065, 0.05)), "RightWall": _mat((0.14, 0.45, 0.091)), "Lamp00": _mat(0.0)}
    for row, _, mat, _, sib in ROWS:
        if row not in rows:
            continue
        sibling = siblings.get(row, False)
        body_mat = row
        if row == "O11":
            mats["O11"] = mat                       # light 1 keeps the record either way
            if sibling:
                body_mat, mats["O11body"] = "O11body", mat
        else:
            mats[row] = sib if sibling and isinstance(sib, dict) else mat
        if row == "G6":
            tris = _icosphere(centre(row), SPHERE_RADIUS, _rotation(row), smooth=not sibling)
        else:
            tris = _box(centre(row), half_size(row), _rotation(row))
        parts.append((body_mat, tris))

    for tex, img in TEXTURES.items():
        with open(os.path.join(directory, tex + ".ppm"), "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())
    with open(os.path.join(directory, name + ".mtl"), "w") as f:
        for m, r in mats.items():
            f.write("newmtl %s\nKd %r %r %r\nKs %r %r %r\nNs %r\nNi %r\n" % ((m,) + r["kd"] + r["ks"] + (r["ns"], r["ni"])))
            if r["tex"]:
                f.write("map_Kd %s\n" % r["tex"])
    faces = {}
    with open(os.path.join(directory, name + ".obj"), "w") as f:
        base, nface = 1, 0
        for mat, tris in parts:
            lines = []
            for pts, _, _ in tris:
                lines += ["v %r %r %r" % tuple(map(float, p)) for p in pts]
            for _, nrm, _ in tris:
                lines += ["vn %r %r %r" % tuple(map(float, n)) for n in nrm]
            for _, _, uvs in tris:
                lines += ["vt %r %r" % tuple(map(float, t)) for t in uvs]
            lines.append("usemtl %s" % mat)
            for j in range(len(tris)):
                a, b, c = base + 3 * j, base + 3 * j + 1, base + 3 * j + 2
                lines.append("f %d/%d/%d %d/%d/%d %d/%d/%d" % (a, a, a, b, b, b, c, c, c))
            f.write("\n".join(lines) + "\n")
            row = "O11" if mat == "O11body" else mat
            if row in SLOT and len(tris) > 2:
                faces[row] = (nface, len(tris))
            base += 3 * len(tris)
            nface += len(tris)
    with open(os.path.join(directory, name + ".camera"), "w") as f:
        f.write("eye 0.0 0.05 2.4\nlookat 0.0 0.05 0.0\nup 0 1 0\nfovy 40\nwidth %d\nheight %d\n" % (width, height))
        for mat, rad in zip(light_names, LIGHT_RADIANCE):
            f.write("mtlname %s %r %r %r\n" % ((mat,) + rad))
    return {"lights": list(light_names), "rows": faces}
