"""A numpy restatement of any-hit rays (include/mcpt.h: any-hit rays) for the tests: the ray of a point pair with its roundings in the
order written, the packing of a bool matrix into 64-bit words, and the rule itself from a closest-hit answer.  float64 throughout;
numpy's elementwise +, -, * are single IEEE operations (no contraction)."""
import numpy as np


def pair_rays(a, b, t0, t1):
    """a [na, 3], b [nb, 3] -> (rays6 [na * nb, 6], tmax): pair (i, j) at i * nb + j; d = b - a; o = a + t0 * d (product, then sum)"""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        d = b[None, :, :] - a[:, None, :]
        s = np.float64(t0) * d
        o = a[:, None, :] + s
    return np.ascontiguousarray(np.concatenate([o, d], axis=2).reshape(-1, 6)), float(np.float64(t1) - np.float64(t0))


def row_words(nb):
    return (nb + 63) // 64


def pack(m):
    """bool [na, nb] -> uint64 [na, W]: pair (i, j) is bit j & 63 of word [i, j >> 6]; padding bits 0"""
    m = np.asarray(m, dtype=bool)
    na, nb = m.shape
    W = row_words(nb)
    out = np.zeros((na, W), dtype=np.uint64)
    for j in range(nb):
        out[:, j >> 6] |= m[:, j].astype(np.uint64) << np.uint64(j & 63)
    return out


def unpack(bits, nb):
    """uint64 [na, W] -> bool [na, nb] (the padding bits are not looked at)"""
    bits = np.asarray(bits, dtype=np.uint64)
    j = np.arange(nb)
    return ((bits[:, j >> 6] >> (j & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)


def padding(bits, nb):
    """the padding bits of every row's last word, as one uint64 per row (all zero when the matrix is well formed)"""
    bits = np.asarray(bits, dtype=np.uint64)
    left = nb & 63
    if bits.shape[1] == 0 or left == 0:
        return np.zeros(bits.shape[0], dtype=np.uint64)
    return bits[:, -1] >> np.uint64(left)


def occluded(face, t, tmax):
    """THE RULE: face >= 0 and t < tmax, the IEEE comparison (a NaN limit is never occluded); tmax None: +inf"""
    face, t = np.asarray(face), np.asarray(t, dtype=np.float64)
    lim = np.full(t.shape, np.inf) if tmax is None else np.broadcast_to(np.asarray(tmax, dtype=np.float64), t.shape)
    with np.errstate(invalid="ignore"):
        return (face >= 0) & (t < lim)
