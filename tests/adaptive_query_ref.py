"""numpy restatement of the adaptive query call (include/mcpt.h: adaptive queries): the pass boundaries, the stopping rule with every
parenthesis written out, and the answers -- counts, means, standard errors, hits -- from the per-sample radiance of every query.  fp64
throughout; the sums are folded in k order by a Python loop over k, never by a pairwise sum."""
import numpy as np


def boundaries(spp, min_spp):
    """b_0 = min(min_spp, spp), b_{j+1} = min(2 b_j, spp), up to spp itself (Python integers: nothing overflows)"""
    b = [min(int(min_spp), int(spp))]
    while b[-1] < spp:
        b.append(min(2 * b[-1], int(spp)))
    return b


def se2_channels(s1, s2, k):
    """per channel: max((s2 - s1 * s1 / k) / (k - 1), 0) / k, k >= 2"""
    kd = np.float64(k)
    var = (s2 - ((s1 * s1) / kd)) / np.float64(k - 1)
    return np.where(var > 0.0, var, 0.0) / kd


def stops(s1, s2, k, rel_target, abs_target):
    """se2 < rel2 * m2 + abs2 for the sums s1, s2 (n, 3) after k samples: a bool per query"""
    rel2 = np.float64(rel_target) * np.float64(rel_target)
    abs2 = np.float64(abs_target) * np.float64(abs_target)
    e = se2_channels(s1, s2, k)
    m = s1 / np.float64(k)
    se2 = ((e[:, 0] + e[:, 1]) + e[:, 2])
    m2 = (((m[:, 0] * m[:, 0]) + (m[:, 1] * m[:, 1])) + (m[:, 2] * m[:, 2]))
    return se2 < ((rel2 * m2) + abs2)


def answers(x, hit, spp, min_spp, rel_target, abs_target):
    """x (n, K, 3): the radiance of samples sample_base .. sample_base + K - 1 of every query, hit (n, K) their rays' hit flags, K >= spp.
    Returns (counts, mean, stderr, hits) of the adaptive call with these parameters."""
    x = np.asarray(x, dtype=np.float64)
    hit = np.asarray(hit)
    n = x.shape[0]
    assert x.shape[1] >= spp and hit.shape == x.shape[:2]
    s1, s2 = np.zeros((n, 3)), np.zeros((n, 3))
    hits = np.zeros(n, dtype=np.int64)
    counts = np.zeros(n, dtype=np.int64)
    active = np.ones(n, dtype=bool)
    prev = 0
    for b in boundaries(spp, min_spp):
        if not active.any():
            break
        for k in range(prev, b):
            xa = x[active, k]
            s1[active] = s1[active] + xa
            s2[active] = s2[active] + (xa * xa)
            hits[active] += hit[active, k].astype(np.int64)
        counts[active] = b
        if b < spp:
            active &= ~stops(s1, s2, b, rel_target, abs_target)
        prev = b
    c = counts.astype(np.float64)[:, None]
    mean = s1 / c
    err = np.zeros((n, 3))
    for cnt in np.unique(counts):
        sel = counts == cnt
        if cnt >= 2:
            err[sel] = np.sqrt(se2_channels(s1[sel], s2[sel], int(cnt)))
    return counts.astype(np.int32), mean, err, hits.astype(np.int32)
