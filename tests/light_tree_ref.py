"""numpy restatement of MCPT_LIGHTS_TREE (include/mcpt.h: light sampling), written from the header's text and independent of the C++: the
tree's builder (leaf boxes, median split, preorder numbering), a node's importance by distance and horizon, and the descent with the
draw of MCPT_LIGHTS_ONE.  Everything is fp64 with + - * / and comparisons in the header's order, so node arrays, picked lights and
probabilities match the library bit for bit.  The walk also keeps a trace of the cases it met, which the tests assert on."""
import numpy as np

import light_pick_ref as LP

NODE = np.dtype([("lo", "<f8", 3), ("hi", "<f8", 3), ("w", "<f8"), ("left", "<i4"), ("right", "<i4")])
assert NODE.itemsize == 64


def light_boxes(scene):
    """(nl, 2, 3): exact min / max of the vertices of every light's faces"""
    g, m, _ = scene.faces()
    v = np.ascontiguousarray(g[:, :9]).reshape(-1, 3, 3)
    out = np.zeros((scene.info.num_lights, 2, 3))
    for l in range(scene.info.num_lights):
        mine = v[m == scene.light(l)[2]].reshape(-1, 3)
        out[l, 0], out[l, 1] = mine.min(axis=0), mine.max(axis=0)
    return out


def boxes_of_vertices(v9, face_mat, light_mats):
    v = np.asarray(v9).reshape(-1, 3, 3)
    out = np.zeros((len(light_mats), 2, 3))
    for l, mat in enumerate(light_mats):
        mine = v[face_mat == mat].reshape(-1, 3)
        out[l, 0], out[l, 1] = mine.min(axis=0), mine.max(axis=0)
    return out


def build(boxes, w):
    """the node array: preorder, root 0; split at the median of the box centres along the widest axis of the centres' bounds (lowest axis
    among equals), ties by light index, the first ceil(n / 2) go left"""
    nodes = []

    def centre(l, a):
        return (float(boxes[l, 0, a]) + float(boxes[l, 1, a])) * 0.5

    def make(ids):
        me = len(nodes)
        nodes.append(None)
        if len(ids) == 1:
            l = ids[0]
            nodes[me] = (tuple(boxes[l, 0]), tuple(boxes[l, 1]), float(w[l]), ~l, ~l)
            return me
        spans = []
        for a in range(3):
            c = [centre(l, a) for l in ids]
            spans.append(max(c) - min(c))
        axis = 0
        for a in (1, 2):
            if spans[a] > spans[axis]:
                axis = a
        ids = sorted(ids, key=lambda l: (centre(l, axis), l))
        half = (len(ids) + 1) // 2
        left = make(ids[:half])
        right = make(ids[half:])
        L, R = nodes[left], nodes[right]
        nodes[me] = (tuple(min(x, y) for x, y in zip(L[0], R[0])), tuple(max(x, y) for x, y in zip(L[1], R[1])), L[2] + R[2], left, right)
        return me

    make(list(range(len(w))))
    out = np.zeros(len(nodes), dtype=NODE)
    for i, n in enumerate(nodes):
        out[i] = n
    return out


def importance(nodes, idx, p, pn, wrong=False):
    """(I, s, margin) of nodes[idx[i]] seen from vertex i.  wrong: a deliberately wrong importance (no distance term), for the power test."""
    lo, hi, W = nodes["lo"][idx], nodes["hi"][idx], nodes["w"][idx]
    c = (lo + hi) * 0.5
    h = (hi - lo) * 0.5
    d = c - p
    a = np.abs(pn)
    s = ((d[:, 0] * pn[:, 0] + d[:, 1] * pn[:, 1]) + d[:, 2] * pn[:, 2]) + ((h[:, 0] * a[:, 0] + h[:, 1] * a[:, 1]) + h[:, 2] * a[:, 2])
    pinf = np.maximum(np.maximum(np.abs(p[:, 0]), np.abs(p[:, 1])), np.abs(p[:, 2]))
    cinf = np.maximum(np.maximum(np.abs(c[:, 0]), np.abs(c[:, 1])), np.abs(c[:, 2]))
    hinf = np.maximum(np.maximum(h[:, 0], h[:, 1]), h[:, 2])
    margin = (1e-9 * ((a[:, 0] + a[:, 1]) + a[:, 2])) * ((pinf + cinf) + hinf)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    h2 = (h[:, 0] * h[:, 0] + h[:, 1] * h[:, 1]) + h[:, 2] * h[:, 2]
    D = np.maximum(1.0, np.maximum(d2, h2))
    I = np.where(s < -margin, 0.0, W if wrong else W / D)
    return I, s, margin, d2


def branch(nodes, n, p, pn, wrong=False):
    """at inner nodes n[i]: (pL, forced) -- forced = -1 go left with probability 1, +1 go right, 0 draw -- and the trace's facts"""
    l, r = nodes["left"][n], nodes["right"][n]
    iL, sL, mL, dL = importance(nodes, l, p, pn, wrong)
    iR, sR, mR, dR = importance(nodes, r, p, pn, wrong)
    both = (iL == 0.0) & (iR == 0.0)
    facts = {"both_culled": both & ((sL < -mL) & (sR < -mR)), "one_culled": (sL < -mL) != (sR < -mR),
             "s_zero": (sL == 0.0) | (sR == 0.0), "s_below_inside_margin": ((sL < 0.0) & (sL >= -mL)) | ((sR < 0.0) & (sR >= -mR)),
             "dist_zero": (dL == 0.0) | (dR == 0.0)}
    iL = np.where(both, nodes["w"][l], iL)
    iR = np.where(both, nodes["w"][r], iR)
    forced = np.where(iR == 0.0, -1, np.where(iL == 0.0, 1, 0))
    with np.errstate(invalid="ignore", divide="ignore"):
        pL = iL / (iL + iR)
    return pL, forced, facts


class TreeRef:
    def __init__(self, boxes, weights):
        self.table = LP.PickRef(weights)
        self.w = self.table.w
        self.nl = self.w.shape[0]
        self.nodes = build(np.asarray(boxes, dtype=np.float64), self.w)

    @classmethod
    def of_scene(cls, scene, weights=None):
        return cls(light_boxes(scene), LP.PickRef.of_scene(scene, weights).w)

    def descend(self, u, p, pn, wrong_pdf=False):
        """(light, pdf, trace) for the draws u at the vertices (p, pn); wrong_pdf: the pick as it is, the probability from a wrong importance"""
        u = np.array(u, dtype=np.float64)
        p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
        pn = np.ascontiguousarray(pn, dtype=np.float64).reshape(-1, 3)
        n = np.zeros(u.shape[0], dtype=np.int64)
        pdf = np.ones(u.shape[0])
        trace = {}
        level = 0
        while True:
            live = self.nodes["left"][n] >= 0
            if not live.any():
                break
            at = np.nonzero(live)[0]
            pL, forced, facts = branch(self.nodes, n[at], p[at], pn[at])
            for k, v in facts.items():
                trace.setdefault(k, np.zeros(u.shape[0], dtype=bool))[at] |= v
                if level == 0:
                    trace[k + "_root"] = trace[k].copy()
            q = pL
            if wrong_pdf:
                q = branch(self.nodes, n[at], p[at], pn[at], wrong=True)[0]
            uu = u[at]
            left = np.where(forced == -1, True, np.where(forced == 1, False, uu < pL))
            draw = forced == 0
            with np.errstate(invalid="ignore", divide="ignore"):
                u[at] = np.where(draw, np.where(left, uu / pL, (uu - pL) / (1.0 - pL)), uu)
                pdf[at] = np.where(draw, np.where(left, pdf[at] * q, pdf[at] * (1.0 - q)), pdf[at])
            n[at] = np.where(left, self.nodes["left"][n[at]], self.nodes["right"][n[at]])
            level += 1
        self.depth = level
        return (~self.nodes["left"][n]).astype(np.int32), pdf, trace

    def pick(self, seed, pix, k, depth, p, pn):
        return self.descend(LP.pick_uniform(seed, pix, k, depth, self.nl), p, pn)

    def pdf_all(self, p, pn):
        """(n, nl): the probability of every light at every vertex"""
        p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
        pn = np.ascontiguousarray(pn, dtype=np.float64).reshape(-1, 3)
        prob = np.zeros((self.nodes.shape[0], p.shape[0]))
        prob[0] = 1.0
        out = np.zeros((p.shape[0], self.nl))
        for i in range(self.nodes.shape[0]):            # preorder: a parent comes before its children
            l, r = int(self.nodes["left"][i]), int(self.nodes["right"][i])
            if l < 0:
                out[:, ~l] = prob[i]
                continue
            pL, forced, _ = branch(self.nodes, np.full(p.shape[0], i), p, pn)
            with np.errstate(invalid="ignore"):
                prob[l] = np.where(forced == -1, prob[i], np.where(forced == 1, 0.0, prob[i] * pL))
                prob[r] = np.where(forced == -1, 0.0, np.where(forced == 1, prob[i], prob[i] * (1.0 - pL)))
        return out


ROOM = (-2.0, 2.0, -1.0, 1.5, -2.0, 2.6)


def vertex_set(tree, seed=0):
    """Vertices (p, pn) that meet, by construction, the cases the tests name: on each room surface with its normal; at a light's box centre;
    inside an inner node's box; 10^3 room sizes away; the horizon plane exactly through a box corner and an ulp to either side (and
    just past the culling margin); every light below the horizon; pn = 0; one of the root's children below the horizon."""
    rng = np.random.default_rng(seed)
    x0, x1, y0, y1, z0, z1 = ROOM
    P, N = [], []

    def add(p, n):
        P.append([float(c) for c in p])
        N.append([float(c) for c in n])

    for _ in range(6):
        x, y, z = rng.uniform(x0, x1), rng.uniform(y0, y1), rng.uniform(z0, z1)
        add((x, y0, z), (0, 1, 0)); add((x, y1, z), (0, -1, 0)); add((x, y, z0), (0, 0, 1))
        add((x, y, z1), (0, 0, -1)); add((x0, y, z), (1, 0, 0)); add((x1, y, z), (-1, 0, 0))
        d = rng.normal(size=3)
        add((x, y, z), d / np.linalg.norm(d))                                  # in the room, any normal
    nodes = tree.nodes
    leaves = np.nonzero(nodes["left"] < 0)[0]
    for i in leaves[:3]:
        c = (nodes["lo"][i] + nodes["hi"][i]) * 0.5
        add(c, (0.3, -0.9, 0.2)); add(c, (0, 1, 0))                            # |c - p|^2 = 0
    root_c = (nodes["lo"][0] + nodes["hi"][0]) * 0.5
    add(root_c, (0, 1, 0)); add(root_c + 0.01, (0.5, 0.5, -0.7))               # inside the root's box
    far = 1e3 * (x1 - x0)
    add((far, 0.7 * far, -1.2 * far), (-1, -0.7, 1.2)); add((far, 0.7 * far, -1.2 * far), (1, 0.7, -1.2)); add((-far, 0.0, 0.0), (1, 0, 0))
    # the horizon plane of pn = +y through the top corner of a leaf's box: (c.y - p.y) + h.y == 0 exactly, found by search around hi.y
    i = leaves[0]
    lo, hi = nodes["lo"][i], nodes["hi"][i]
    cy, hy = (lo[1] + hi[1]) * 0.5, (hi[1] - lo[1]) * 0.5
    py = float(hi[1])
    for _ in range(8):
        s = (cy - py) + hy
        if s == 0.0:
            break
        py = np.nextafter(py, np.inf if s > 0 else -np.inf)
    assert (cy - py) + hy == 0.0
    px, pz = float(lo[0]) - 0.5, float(lo[2]) - 0.25                           # dyadic offsets: the x and z terms are multiplied by pn = 0
    for y in (py, np.nextafter(py, np.inf), np.nextafter(py, -np.inf), py + 1e-6, py - 1e-6):
        add((px, y, pz), (0, 1, 0))
    top = float(nodes["hi"][0][1])
    add((0.1, top + 0.25, 0.2), (0, 1, 0)); add((x1 + 1.0, 0.0, 0.0), (1, 0, 0))   # every light below the horizon
    add((0.3, 0.2, 0.1), (0, 0, 0)); add((-1.0, 1.0, 2.0), (0.0, -0.0, 0.0))   # pn = 0
    L, R = int(nodes["left"][0]), int(nodes["right"][0])
    cl, cr = (nodes["lo"][L] + nodes["hi"][L]) * 0.5, (nodes["lo"][R] + nodes["hi"][R]) * 0.5
    add((cl + cr) * 0.5, cr - cl); add((cl + cr) * 0.5, cl - cr)               # between the root's children, facing one of them
    add(cl + (cl - cr), cl - cr); add(cr + (cr - cl), cr - cl)                 # beyond one child, looking away from both / ...
    return np.array(P), np.array(N)
