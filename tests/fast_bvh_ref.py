"""numpy restatement of what a valid culling hierarchy of the fast walk is (mcpt.h: mcpt_device_fast_hierarchy), checked in exact
arithmetic.  A node is the 64-byte CwNode record (device_scene.hpp): per axis a plane is p + q * 2^e with p an fp32 number, q in
0..255 and e in -126..127.  Such a sum is not always representable in fp64 (p = 1e6, e = -126), so every decoded plane is held as
the unevaluated pair (s, r) of TwoSum, s = fl(p + x), s + r = p + x exactly, and planes are compared with the geometry through that
pair: the comparisons below are exact, not within a tolerance.

check_hierarchy() asserts:
- every triangle slot is referenced by exactly one leaf, and the slots' faces are a permutation of the scene's faces;
- every node is reached from the root (node 0) exactly once: no node twice, no cycle, no node left over;
- nchild is the number of non-empty slots, a leaf holds 1..8 triangles (the walk decodes count - 1 from three bits);
- every non-empty slot's planes contain the exact fp64 box of all the triangles below it (leaf: its triangles; inner: its subtree);
- the walk's stack need, recomputed with its push rule (trace_fast.hpp: a node pushes its hit children but the nearest, at most
  nchild - 1 entries, and walks on into the nearest), is at most the recorded cw_stack_need.
"""
import numpy as np

EMPTY = -0x80000000
MAX_LEAF = 8

CW_DTYPE = np.dtype([("p", "<f4", 3), ("e", "i1", 3), ("nchild", "u1"), ("qlo", "<u4", 3), ("qhi", "<u4", 3), ("child", "<i4", 4),
                     ("pad", "<u4", 2)])
assert CW_DTYPE.itemsize == 64


def decode(nodes):
    """raw records ([n, 64] uint8 or bytes) -> structured array of CW_DTYPE"""
    if isinstance(nodes, (bytes, bytearray)):
        nodes = np.frombuffer(nodes, dtype=np.uint8)
    a = np.ascontiguousarray(np.asarray(nodes, dtype=np.uint8)).reshape(-1, 64)
    return a.view(CW_DTYPE).reshape(-1)


def encode(rec):
    return np.ascontiguousarray(rec).view(np.uint8).reshape(-1, 64)


def leaf_ref(first, count):
    return -1 - ((first << 4) | (count - 1))


def split_leaf(ref):
    r = -1 - int(ref)
    return r >> 4, (r & 15) + 1


def face_boxes(geom27):
    """exact boxes of the faces (Scene.faces()[0]: v1 v2 v3 first), lo [n,3], hi [n,3]"""
    v = np.asarray(geom27, dtype=np.float64)[:, :9].reshape(-1, 3, 3)
    return v.min(axis=1), v.max(axis=1)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def planes(rec):
    """exact planes of every slot: (lo_s, lo_r, hi_s, hi_r), each [n, 4, 3], plane = s + r"""
    p = rec["p"].astype(np.float64)[:, None, :]
    sc = np.ldexp(1.0, rec["e"].astype(np.int64))[:, None, :]
    sh = (8 * np.arange(4, dtype=np.uint32))[None, :, None]
    qlo = ((rec["qlo"][:, None, :] >> sh) & 255).astype(np.float64)
    qhi = ((rec["qhi"][:, None, :] >> sh) & 255).astype(np.float64)
    lo_s, lo_r = _two_sum(np.broadcast_to(p, qlo.shape), qlo * sc)       # q * 2^e: at most 8 significant bits, exact
    hi_s, hi_r = _two_sum(np.broadcast_to(p, qhi.shape), qhi * sc)
    return lo_s, lo_r, hi_s, hi_r


def _le(s, r, b):
    """s + r <= b exactly (b an fp64 number, (s, r) a TwoSum pair)"""
    return (s < b) | ((s == b) & (r <= 0))


def _ge(s, r, b):
    return (s > b) | ((s == b) & (r >= 0))


class HierarchyError(AssertionError):
    pass


def check_hierarchy(nodes, tri_faces, face_lo, face_hi, stack_need=None):
    """Raise HierarchyError at the first violation; return a dict of figures of the tree (nodes, leaves, depth, need)."""
    rec = decode(nodes)
    n = rec.shape[0]
    tri_faces = np.asarray(tri_faces, dtype=np.int64)
    nt = tri_faces.shape[0]
    nf = face_lo.shape[0]

    def fail(msg):
        raise HierarchyError(msg)

    if nt != nf or not np.array_equal(np.sort(tri_faces), np.arange(nf)):
        fail("tri_faces is not a permutation of the %d faces (%d slots)" % (nf, nt))
    if nf > 0 and n == 0:
        fail("no nodes over %d triangles" % nf)
    if not np.all(np.isfinite(rec["p"])):
        fail("non-finite grid origin")
    if np.any(rec["e"] < -126):
        fail("grid step exponent below -126")
    tlo, thi = face_lo[tri_faces], face_hi[tri_faces]        # box of triangle slot k
    # ---- walk the tree from the root: references, coverage, order
    child = rec["child"].astype(np.int64)
    visited = np.zeros(n, dtype=bool)
    cover = np.zeros(nt, dtype=np.int64)
    order = []                                               # nodes, parents before children
    depth = np.zeros(n, dtype=np.int64)
    stack = [0] if n else []
    if n:
        visited[0] = True
    leaves = 0
    while stack:
        i = stack.pop()
        order.append(i)
        nonempty = 0
        for c in range(4):
            ref = int(child[i, c])
            if ref == EMPTY:
                continue
            nonempty += 1
            if ref >= 0:
                if ref >= n:
                    fail("node %d slot %d refers to node %d of %d" % (i, c, ref, n))
                if visited[ref]:
                    fail("node %d is reached twice (again from node %d slot %d): a shared subtree or a cycle" % (ref, i, c))
                visited[ref] = True
                depth[ref] = depth[i] + 1
                stack.append(ref)
            else:
                first, count = split_leaf(ref)
                if count > MAX_LEAF:
                    fail("node %d slot %d: leaf of %d triangles" % (i, c, count))
                if first < 0 or first + count > nt:
                    fail("node %d slot %d: leaf [%d, %d) outside the %d triangle slots" % (i, c, first, first + count, nt))
                cover[first:first + count] += 1
                leaves += 1
        if nonempty != int(rec["nchild"][i]):
            fail("node %d: nchild %d, %d non-empty slots" % (i, int(rec["nchild"][i]), nonempty))
    if n and not visited.all():
        fail("%d of %d nodes are not reached from the root" % (int((~visited).sum()), n))
    if np.any(cover != 1):
        bad = np.nonzero(cover != 1)[0]
        fail("%d triangle slots referenced %s times, not once (first: slot %d, face %d)" % (bad.size, sorted(set(cover[bad].tolist())), bad[0], tri_faces[bad[0]]))
    # ---- exact boxes bottom up, planes against them
    lo_s, lo_r, hi_s, hi_r = planes(rec)
    blo = np.full((n, 3), np.inf)
    bhi = np.full((n, 3), -np.inf)
    need = np.zeros(n, dtype=np.int64)
    for i in reversed(order):
        below = 0
        for c in range(4):
            ref = int(child[i, c])
            if ref == EMPTY:
                continue
            if ref >= 0:
                clo, chi = blo[ref], bhi[ref]
                below = max(below, int(need[ref]))
            else:
                first, count = split_leaf(ref)
                clo, chi = tlo[first:first + count].min(axis=0), thi[first:first + count].max(axis=0)
            ok_lo = _le(lo_s[i, c], lo_r[i, c], clo)
            ok_hi = _ge(hi_s[i, c], hi_r[i, c], chi)
            if not (ok_lo.all() and ok_hi.all()):
                a = int(np.nonzero(~(ok_lo & ok_hi))[0][0])
                fail("node %d slot %d (%s) axis %d: planes [%r, %r] do not contain [%r, %r]" %
                     (i, c, "node %d" % ref if ref >= 0 else "leaf %d+%d" % split_leaf(ref), a, lo_s[i, c, a] + lo_r[i, c, a],
                      hi_s[i, c, a] + hi_r[i, c, a], clo[a], chi[a]))
            blo[i] = np.minimum(blo[i], clo)
            bhi[i] = np.maximum(bhi[i], chi)
        need[i] = int(rec["nchild"][i]) - 1 + below
    got = int(need[0]) if n else 0
    if stack_need is not None and got > stack_need:
        fail("the walk may hold %d stack entries, the builder recorded %d" % (got, stack_need))
    return {"nodes": n, "leaves": leaves, "depth": int(depth.max()) + 1 if n else 0, "need": got}


# ---------------------------------------------------------------------------------------------------------------------- building
def quantise(kid_lo, kid_hi):
    """one axis of a node over boxes kid_lo[k], kid_hi[k] with the builders' rule (build_kernels.hip: k_fast_level): (p, e, qlo, qhi)"""
    lo, hi = min(kid_lo), max(kid_hi)
    pf = np.float32(lo)
    if float(pf) > lo:
        pf = np.nextafter(pf, np.float32(-np.inf))
    p = float(pf)
    e = -126
    if hi - p > 0:
        e = max(-126, int(np.ceil(np.log2((hi - p) / 255.0))))
    while True:
        sc = np.ldexp(1.0, e)
        ql, qh, ok = [], [], p + 255.0 * sc >= hi
        for a, b in zip(kid_lo, kid_hi):
            l = min(max(np.floor((a - p) / sc), 0.0), 255.0)
            h = min(max(np.ceil((b - p) / sc), 0.0), 255.0)
            while l > 0 and p + l * sc > a:
                l -= 1
            while h < 255 and p + h * sc < b:
                h += 1
            ok = ok and p + l * sc <= a and p + h * sc >= b
            ql.append(int(l))
            qh.append(int(h))
        if ok:
            return pf, e, ql, qh
        e += 1


def make_node(kid_lo, kid_hi, refs):
    """one CwNode record over up to four children with exact boxes kid_lo[k] / kid_hi[k] ([3] each) and references refs[k]"""
    r = np.zeros(1, dtype=CW_DTYPE)[0]
    r["nchild"] = len(refs)
    for a in range(3):
        pf, e, ql, qh = quantise([b[a] for b in kid_lo], [b[a] for b in kid_hi])
        r["p"][a], r["e"][a] = pf, e
        r["qlo"][a] = sum(q << (8 * c) for c, q in enumerate(ql))
        r["qhi"][a] = sum(q << (8 * c) for c, q in enumerate(qh))
    r["child"][:] = EMPTY
    r["child"][:len(refs)] = refs
    return r
