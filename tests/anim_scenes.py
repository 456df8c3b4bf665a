"""Deformations of the test scenes for the geometry-update tests, all deterministic, and the moved scene written back as files: the CPU
oracle loads from files only, and a scene with textures can only be made from files, so "a fresh scene with the moved vertices" is the
original .obj with its positions replaced, coordinates written with repr() (exact through atof).

v is always [num_faces, 9]: v1 v2 v3 of every face in .obj order (Scene.faces()[0][:, :9])."""
import os
import shutil

import numpy as np


def diagonal(v):
    p = v.reshape(-1, 3)
    return float(np.linalg.norm(p.max(axis=0) - p.min(axis=0)))


def identity(v):
    return v.copy()


def rigid(v, faces, degrees=30.0, shift=(0.05, 0.0, -0.04)):
    """the faces `faces` rotated about the vertical (y) axis through their centroid and shifted"""
    out = v.copy()
    p = out[faces].reshape(-1, 3)
    c = p.mean(axis=0)
    a = np.deg2rad(degrees)
    rot = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    out[faces] = ((p - c) @ rot.T + c + np.asarray(shift)).reshape(-1, 9)
    return out


def mirror(v, faces):
    """the faces `faces` reflected in the plane x = c through their centroid: the body keeps its place, and as every face keeps the order
    of its vertices its winding turns inside out (a reflection turns (v1 - v2) x (v3 - v1) into minus its own mirror image)"""
    out = v.copy()
    p = out[faces].reshape(-1, 3)
    c = p.mean(axis=0)
    p[:, 0] = 2.0 * c[0] - p[:, 0]
    out[faces] = p.reshape(-1, 9)
    return out


def face_normals(v):
    """the faces' geometric normals as the loader and an update form them, (v1 - v2) x (v3 - v1), not normalised"""
    return np.cross(v[:, 0:3] - v[:, 3:6], v[:, 6:9] - v[:, 0:3])


def sine_field(v, amplitude=0.05, phase=0.0):
    """every vertex displaced by a sine field of `amplitude` x the scene's diagonal (a function of position: shared vertices stay shared)"""
    p = v.reshape(-1, 3)
    d = diagonal(v)
    k = 2.0 * np.pi / (0.37 * d)
    disp = np.stack([np.sin(k * p[:, 1] + 0.3 + phase), np.sin(k * p[:, 2] + 1.1 + phase), np.sin(k * p[:, 0] + 2.3 + phase)], axis=1)
    return (p + amplitude * d * disp).reshape(-1, 9)


def move_lights(v, material, light_materials, scale=1.3, shift=(0.1, 0.05, -0.07)):
    """every emitter moved and scaled about its own centroid (areas, CDFs and area0 change)"""
    out = v.copy()
    for i, m in enumerate(light_materials):
        f = np.nonzero(material == m)[0]
        p = out[f].reshape(-1, 3)
        c = p.mean(axis=0)
        out[f] = ((p - c) * (scale + 0.1 * i) + c + np.asarray(shift) * (1 + i)).reshape(-1, 9)
    return out


def degenerate(v):
    """one triangle collapsed to zero area, one vertex outside the Morton cube [-1, 4]^3, two faces made coincident"""
    out = v.copy()
    n = out.shape[0]
    a, b, c, d = n // 7, n // 3, n // 2, n // 2 + 1
    out[a, 3:6] = out[a, 0:3]
    out[a, 6:9] = out[a, 0:3]
    out[b, 0:3] = [5.5, -1.75, 4.25]
    out[d] = out[c]
    return out


def out_of_range(v):
    out = v.copy()
    out[out.shape[0] // 5, 4] = 1e200
    return out


def write_moved(src_dir, name, v, dst_dir):
    """<src_dir>/<name>.obj with its positions replaced by v, into dst_dir with the .mtl, the .camera and every other file of src_dir the
    scene may name (textures).  Each face gets three position lines of its own; vn, vt and the faces' other indices stay as they are."""
    os.makedirs(dst_dir, exist_ok=True)
    for f in os.listdir(src_dir):
        if not f.endswith(".obj") and os.path.isfile(os.path.join(src_dir, f)):
            shutil.copy(os.path.join(src_dir, f), dst_dir)
    head, body, face = [], [], 0
    for line in open(os.path.join(src_dir, name + ".obj")):
        line = line.rstrip("\n")
        if line.startswith("v "):
            continue
        if line.startswith("f "):
            corners = line[2:].split(" ")
            new = []
            for c, tok in enumerate(corners[:3]):
                rest = tok.split("/", 1)
                new.append("%d/%s" % (3 * face + c + 1, rest[1]))
            body.append("f " + " ".join(new))
            face += 1
        else:
            body.append(line)
    assert face == v.shape[0], (face, v.shape)
    for q in v.reshape(-1, 3):
        head.append("v %r %r %r" % (float(q[0]), float(q[1]), float(q[2])))
    with open(os.path.join(dst_dir, name + ".obj"), "w") as f:
        f.write("\n".join(head + body) + "\n")
    return dst_dir + os.sep
