"""Scenes and skies for the environment light against the oracle, written as .obj/.mtl/.camera so that they load through the file surface
of both the product (mcpt.Scene) and the oracle (oracle_lib.OracleScene), in the style of light_scenes.py.

open_scene: an open scene under the sky -- a diffuse floor whose vertex normals are not of unit length and differ per vertex (so the
interpolated normal is not of unit length either), a Phong plate (Ks 0.8, Ns 200) tilted towards the camera, a glass box (Ni 1.5) and,
with n_lights >= 1, one small emitter facing down; n_lights = 2 and 3 add a larger emitter facing down over the left of the floor and a
larger one standing to the right of the box, facing it -- each its own material and radiance, none smaller than the first (the reference draws
every light's point over the first light's area: every draw finds a triangle, nothing goes NaN).  The upper part of the frame and the rays past the floor's far edge see the sky.  Every
kind of environment path is reached: shadow rays that leave the scene and shadow rays that the plate, the box or the emitter block,
SPECULAR escapes off the plate and the box, TRANSMISSION escapes out of the box, camera rays that miss.

floor_scene: one upward quad at y = 0 of a single material, seen from (0, 3, 0) looking down (or, look_up, looking up: every camera
ray misses) -- for closed forms.

SKIES are test_gpu_env.py's two skies; EDGE_MAPS the maps at the edges of the tables and the draw."""
import os

import numpy as np


def sky_map(W=64, H=32, seed=3):
    """test_gpu_env.py's 64 x 32 map: a bright strip, a dim lower hemisphere, a black row"""
    rng = np.random.default_rng(seed)
    m = rng.random((H, W, 3)) * 2.0
    m[:, 10:14] *= 20.0
    m[H // 2:, :] *= 0.05
    m[5, :] = 0.0
    return m


SKIES = {"constant": ([0.6, 0.8, 1.0], 1.5), "map": (sky_map(), 0.7)}


def _edge_maps():
    rng = np.random.default_rng(11)
    m = {}
    m["1x1"] = (np.array([[[0.7, 0.5, 0.3]]]), 1.3)
    m["one-row"] = (rng.random((1, 16, 3)) + 0.1, 1.0)                 # H = 1: one band from pole to pole
    m["one-column"] = (rng.random((8, 1, 3)) + 0.1, 1.0)              # W = 1
    m["2x2"] = (rng.random((2, 2, 3)) + 0.05, 2.0)
    top = np.zeros((8, 16, 3))
    top[0] = rng.random((16, 3)) + 0.1
    m["top-row"] = (top, 1.0)                                          # all weight at the north pole
    bottom = np.zeros((8, 16, 3))
    bottom[-1] = rng.random((16, 3)) + 0.1
    m["bottom-row"] = (bottom, 1.0)                                    # ... and at the south pole
    zr = rng.random((9, 12, 3)) + 0.1
    zr[[0, 4, 8]] = 0.0
    m["zero-rows"] = (zr, 1.0)                                         # zero-weight rows at both ends and in the middle
    first = np.zeros((6, 10, 3))
    first[:, 0] = rng.random((6, 3)) + 0.1
    m["first-column"] = (first, 1.0)                                   # phi in [0, 2 pi / W): the wrap of atan2
    last = np.zeros((6, 10, 3))
    last[:, -1] = rng.random((6, 3)) + 0.1
    m["last-column"] = (last, 1.0)                                     # phi just under 2 pi
    single = np.zeros((7, 9, 3))
    single[3, 5] = (2.0, 1.5, 1.0)
    m["single-texel"] = (single, 1.0)
    wide = np.full((4, 8, 3), 0.5)
    wide[1, 0::2] = 1e30
    wide[1, 1::2] = 1e-30
    m["1e30-next-to-1e-30"] = (wide, 1.0)
    m["subnormal"] = (np.full((4, 8, 3), 1e-40), 1.0)                   # float32 subnormals only
    m["scale-1e-3"] = (sky_map(), 1e-3)
    m["scale-1e3"] = (sky_map(), 1e3)
    return m


EDGE_MAPS = _edge_maps()


def _quad(p0, p1, p2, p3, normals):
    n0, n1, n2, n3 = normals
    return [((p0, n0), (p1, n1), (p2, n2)), ((p0, n0), (p2, n2), (p3, n3))]


def _box(x0, x1, y0, y1, z0, z1):
    """the six faces of an axis-aligned box, outward unit normals"""
    q = []
    q += _quad((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1), [(0, 0, 1)] * 4)
    q += _quad((x1, y0, z0), (x0, y0, z0), (x0, y1, z0), (x1, y1, z0), [(0, 0, -1)] * 4)
    q += _quad((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0), [(-1, 0, 0)] * 4)
    q += _quad((x1, y0, z1), (x1, y0, z0), (x1, y1, z0), (x1, y1, z1), [(1, 0, 0)] * 4)
    q += _quad((x0, y1, z1), (x1, y1, z1), (x1, y1, z0), (x0, y1, z0), [(0, 1, 0)] * 4)
    q += _quad((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1), [(0, -1, 0)] * 4)
    return q


def _write(directory, name, parts, mats, camera, lights=()):
    """parts: [(material, [triangle = three (vertex, normal) pairs])]; mats: name -> (Kd, Ks, Ns, Ni); camera: (eye, lookat, up, fovy,
    width, height); lights: [(material, radiance)]"""
    with open(os.path.join(directory, name + ".mtl"), "w") as f:
        for m, (kd, ks, ns, ni) in mats.items():
            f.write("newmtl %s\nKd %r %r %r\nKs %r %r %r\nNs %r\nNi %r\n" % (m, *map(float, kd), *map(float, ks), float(ns), float(ni)))
    with open(os.path.join(directory, name + ".obj"), "w") as f:
        base = 1
        for mat, tris in parts:
            lines = ["v %r %r %r" % tuple(map(float, v)) for t in tris for v, _ in t]
            lines += ["vn %r %r %r" % tuple(map(float, n)) for t in tris for _, n in t]
            lines += ["vt 0.5 0.5"] * (3 * len(tris))
            lines.append("usemtl %s" % mat)
            for j in range(len(tris)):
                a = base + 3 * j
                lines.append("f %d/%d/%d %d/%d/%d %d/%d/%d" % (a, a, a, a + 1, a + 1, a + 1, a + 2, a + 2, a + 2))
            f.write("\n".join(lines) + "\n")
            base += 3 * len(tris)
    eye, at, up, fovy, width, height = camera
    with open(os.path.join(directory, name + ".camera"), "w") as f:
        f.write("eye %r %r %r\nlookat %r %r %r\nup %r %r %r\nfovy %r\nwidth %d\nheight %d\n"
                % (*map(float, eye), *map(float, at), *map(float, up), float(fovy), width, height))
        for mat, rad in lights:
            f.write("mtlname %s %r %r %r\n" % (mat, *map(float, rad)))


def open_scene(directory, name, n_lights, width, height):
    """Write <directory>/<name>.{obj,mtl,camera}: the open scene with 0 to 3 lights."""
    assert n_lights in (0, 1, 2, 3)
    # the floor: vertex normals of lengths 1.3 .. 2.2, tilted a little each its own way
    floor_n = [(0.1, 1.6, -0.05), (-0.08, 2.2, 0.1), (0.05, 1.3, 0.12), (-0.1, 1.9, -0.07)]
    parts = [("Floor", _quad((-3, 0, 3), (3, 0, 3), (3, 0, -3), (-3, 0, -3), floor_n))]
    # the Phong plate, leaning back: its normal (0, 0.4, 1.2) / |.| faces the camera and the sky
    pn = tuple(np.array([0.0, 0.4, 1.2]) / np.linalg.norm([0.0, 0.4, 1.2]))
    parts.append(("Plate", _quad((-1.7, 0.1, -1.2), (-0.2, 0.1, -1.2), (-0.2, 1.3, -1.6), (-1.7, 1.3, -1.6), [pn] * 4)))
    # the glass box, clear of the floor
    parts.append(("Glass", _box(0.2, 1.5, 0.05, 1.1, -0.7, 0.5)))
    mats = {"Floor": ((0.6, 0.55, 0.5), (0, 0, 0), 1, 1), "Plate": ((0.05, 0.05, 0.05), (0.8, 0.8, 0.8), 200, 1),
            "Glass": ((0, 0, 0), (0.9, 0.9, 0.9), 100, 1.5)}
    lights = []
    if n_lights:
        parts.append(("Lamp", _quad((-0.3, 2.2, -0.3), (0.3, 2.2, -0.3), (0.3, 2.2, 0.3), (-0.3, 2.2, 0.3), [(0, -1, 0)] * 4)))
        mats["Lamp"] = ((0, 0, 0), (0, 0, 0), 1, 1)
        lights.append(("Lamp", (6.0, 6.0, 5.0)))
    if n_lights >= 2:                  # 0.75 x 0.75 (the first lamp is 0.6 x 0.6), lower and to the left
        parts.append(("Lamp1", _quad((-1.75, 1.9, 0.5), (-1.0, 1.9, 0.5), (-1.0, 1.9, 1.25), (-1.75, 1.9, 1.25), [(0, -1, 0)] * 4)))
        mats["Lamp1"] = ((0, 0, 0), (0, 0, 0), 1, 1)
        lights.append(("Lamp1", (1.5, 2.5, 4.0)))
    if n_lights >= 3:                  # 0.75 x 1.0, upright at x = 2.25, facing -x: the box's right side and the floor under it
        parts.append(("Lamp2", _quad((2.25, 0.25, -0.5), (2.25, 0.25, 0.5), (2.25, 1.0, 0.5), (2.25, 1.0, -0.5), [(-1, 0, 0)] * 4)))
        mats["Lamp2"] = ((0, 0, 0), (0, 0, 0), 1, 1)
        lights.append(("Lamp2", (9.0, 4.0, 1.0)))
    _write(directory, name, parts, mats, ((0, 1.6, 3.6), (0, 0.35, -0.3), (0, 1, 0), 55, width, height), lights)


def floor_scene(directory, name, kd, ks=(0, 0, 0), ns=1, width=32, height=18, half=50.0, look_up=False):
    """Write <directory>/<name>.{obj,mtl,camera}: an upward quad (unit normals) of one material at y = 0, no lights, seen from (0, 3, 0)
    looking down -- or looking up, away from it, so that every camera ray misses."""
    h = half
    parts = [("Surface", _quad((-h, 0, -h), (-h, 0, h), (h, 0, h), (h, 0, -h), [(0, 1, 0)] * 4))]
    at = (0, 6, 0) if look_up else (0, 0, 0)
    _write(directory, name, parts, {"Surface": (kd, ks, ns, 1)}, ((0, 3, 0), at, (0, 0, -1), 30, width, height))
