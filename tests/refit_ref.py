"""numpy restatement of a refit of the fast walk's culling hierarchy (mcpt.h: MCPT_UPDATE_REFIT; build_kernels.hip: k_refit_level) and of
the cost figure of mcpt_update_info.  A refit keeps every node's child[] and nchild and the triangle slots; bottom up, a leaf slot's box is
the exact union of its triangles' fp64 boxes, an inner slot's box the child node's own exact box, and every node is quantised again with
the builders' one rule (fast_bvh_ref.quantise) -- except that the exponent search starts below every exponent that can pass
(255 * 2^e >= hi - p needs e > ilogb(hi - p) - 9) and steps up, so that the exponent is the smallest one whatever log2 rounds to."""
import math

import numpy as np

import fast_bvh_ref as F


def quantise_min(kid_lo, kid_hi):
    """one axis: (p, e, qlo[k], qhi[k]) with the smallest exponent e >= -126 for which every plane fits in 0..255"""
    lo, hi = min(kid_lo), max(kid_hi)
    pf = np.float32(lo)
    if float(pf) > lo:
        pf = np.nextafter(pf, np.float32(-np.inf))
    p = float(pf)
    e = -126
    ext = hi - p
    if ext > 0:
        e = min(127, max(-126, (math.frexp(ext)[1] - 1) - 9)) if math.isfinite(ext) else 127
    while True:
        sc = math.ldexp(1.0, e)
        ql, qh, ok = [], [], p + 255.0 * sc >= hi
        for a, b in zip(kid_lo, kid_hi):
            l = min(max(math.floor((a - p) / sc), 0.0), 255.0)
            h = min(max(math.ceil((b - p) / sc), 0.0), 255.0)
            while l > 0 and p + l * sc > a:
                l -= 1
            while h < 255 and p + h * sc < b:
                h += 1
            ok = ok and p + l * sc <= a and p + h * sc >= b
            ql.append(int(l))
            qh.append(int(h))
        if ok or e >= 127:
            return pf, e, ql, qh
        e += 1


def levels(rec):
    """the nodes in breadth-first order from the root (parents before children)"""
    n = rec.shape[0]
    order, seen = ([0], {0}) if n else ([], set())
    head = 0
    while head < len(order):
        for ref in rec["child"][order[head]]:
            ref = int(ref)
            if 0 <= ref < n and ref not in seen:
                seen.add(ref)
                order.append(ref)
        head += 1
    return order


def refit(nodes, tri_lo, tri_hi):
    """nodes ([n, 64] uint8) refitted to the triangle slots' boxes tri_lo / tri_hi ([n_tris, 3]): the new records ([n, 64] uint8) and
    the nodes' own exact boxes (lo [n, 3], hi [n, 3])"""
    rec = F.decode(nodes).copy()
    n = rec.shape[0]
    blo, bhi = np.full((n, 3), np.inf), np.full((n, 3), -np.inf)
    for i in reversed(levels(rec)):
        slots, klo, khi = [], [], []
        for c in range(4):
            ref = int(rec["child"][i, c])
            if ref == F.EMPTY:
                continue
            if ref >= 0:
                lo, hi = blo[ref], bhi[ref]
            else:
                first, count = F.split_leaf(ref)
                lo, hi = tri_lo[first:first + count].min(axis=0), tri_hi[first:first + count].max(axis=0)
            slots.append(c)
            klo.append(lo)
            khi.append(hi)
        blo[i], bhi[i] = np.min(klo, axis=0), np.max(khi, axis=0)
        for a in range(3):
            pf, e, ql, qh = quantise_min([float(b[a]) for b in klo], [float(b[a]) for b in khi])
            rec["p"][i, a], rec["e"][i, a] = pf, e
            rec["qlo"][i, a] = sum(q << (8 * c) for c, q in zip(slots, ql))
            rec["qhi"][i, a] = sum(q << (8 * c) for c, q in zip(slots, qh))
    return F.encode(rec).copy(), blo, bhi


def _slot_boxes(rec):
    p = rec["p"].astype(np.float64)[:, None, :]
    sc = np.ldexp(1.0, rec["e"].astype(np.int64))[:, None, :]
    sh = (8 * np.arange(4, dtype=np.uint32))[None, :, None]
    lo = p + ((rec["qlo"][:, None, :] >> sh) & 255).astype(np.float64) * sc
    hi = p + ((rec["qhi"][:, None, :] >> sh) & 255).astype(np.float64) * sc
    return lo, hi                                       # [n, 4, 3]


def cost(nodes):
    """sum over the non-empty child slots of (area of the stored box x (1 for a node, triangle count for a leaf)) / the root's area, the
    root's box being the union of node 0's stored child boxes; areas are dx dy + dy dz + dz dx of the decoded planes in fp64"""
    rec = F.decode(nodes)
    lo, hi = _slot_boxes(rec)
    d = hi - lo
    area = d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]
    child = rec["child"].astype(np.int64)
    used = child != F.EMPTY
    weight = np.where(child >= 0, 1.0, (((-1 - child) & 15) + 1).astype(np.float64))
    total = float(np.sum(np.where(used, area * weight, 0.0)))
    r = used[0]
    e = hi[0][r].max(axis=0) - lo[0][r].min(axis=0)
    return total / float(e[0] * e[1] + e[1] * e[2] + e[2] * e[0])


def build(tri_lo, tri_hi, per_leaf=4):
    """a complete 4-ary hierarchy over the triangle slots in their order (leaves of per_leaf consecutive slots), root = node 0, made
    with fast_bvh_ref.make_node: the records ([n, 64] uint8)"""
    t = tri_lo.shape[0]
    groups = (t + per_leaf - 1) // per_leaf
    sizes, n = [], groups
    while True:
        n = (n + 3) // 4
        sizes.append(n)
        if n == 1:
            break
    base = [sum(sizes[d + 1:]) for d in range(len(sizes))]
    rec = np.zeros(sum(sizes), dtype=F.CW_DTYPE)
    lo = [tri_lo[g * per_leaf:(g + 1) * per_leaf].min(axis=0) for g in range(groups)]
    hi = [tri_hi[g * per_leaf:(g + 1) * per_leaf].max(axis=0) for g in range(groups)]
    refs = [F.leaf_ref(g * per_leaf, min(per_leaf, t - g * per_leaf)) for g in range(groups)]
    for d, size in enumerate(sizes):
        nlo, nhi, nrefs = [], [], []
        for i in range(size):
            ks = range(4 * i, min(4 * i + 4, len(lo)))
            rec[base[d] + i] = F.make_node([lo[k] for k in ks], [hi[k] for k in ks], [refs[k] for k in ks])
            nlo.append(np.min([lo[k] for k in ks], axis=0))
            nhi.append(np.max([hi[k] for k in ks], axis=0))
            nrefs.append(base[d] + i)
        lo, hi, refs = nlo, nhi, nrefs
    return F.encode(rec).copy()
