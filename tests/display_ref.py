"""numpy restatement of the display transform (include/mcpt.h: display transform), written from the header's text: the luminance histogram
in integer operations on the bits of Y, mcpt_display_exposure, the parameters' resolution and the map, fp64 in the header's operation
order (numpy contracts nothing)."""
import math

import numpy as np

BINS, SLOTS = 384, 387
CLAMP, REINHARD, FILMIC = 0, 1, 2
LINEAR, SRGB = 0, 1


def luminance(img):
    a = np.ascontiguousarray(img, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return (0.2126 * a[:, 0] + 0.7152 * a[:, 1]) + 0.0722 * a[:, 2]


def slots_of(Y):
    """the slot of every luminance: 0 skipped, 1 under, 2 .. 385 the bins, 386 over"""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    bits = Y.view(np.uint64)
    with np.errstate(invalid="ignore"):
        counted = np.isfinite(Y) & (Y > 0.0)
    expo = ((bits >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64)
    b = (expo - 1023 + 24) * 8 + ((bits >> np.uint64(49)) & np.uint64(7)).astype(np.int64)
    s = np.where(b < 0, 1, np.where(b >= BINS, SLOTS - 1, b + 2))
    return np.where(counted, s, 0)


def histogram(img):
    return np.bincount(slots_of(luminance(img)), minlength=SLOTS).astype(np.int64)


def _bin(s):
    return 0 if s == 1 else (BINS - 1 if s == SLOTS - 1 else s - 2)


def exposure(slots, percentile=0.0):
    """(log_average, l_percentile); percentile 0: 0.99"""
    p = percentile if percentile > 0.0 else 0.99
    counted, acc = 0, 0.0
    for s in range(1, SLOTS):
        n = int(slots[s])
        if n == 0:
            continue
        b = _bin(s)
        acc += float(n) * math.log2(math.ldexp(1.0 + ((b & 7) + 0.5) / 8.0, (b >> 3) - 24))
        counted += n
    if counted == 0:
        return 0.0, 0.0
    la = 2.0 ** (acc / float(counted))
    target = math.ceil(p * float(counted))
    run = 0
    for s in range(1, SLOTS):
        run += int(slots[s])
        if int(slots[s]) and run >= target:
            b = _bin(s)
            return la, math.ldexp(1.0 + ((b & 7) + 1.0) / 8.0, (b >> 3) - 24)
    raise AssertionError("the running count never reached its target")


def resolve(img, exposure_=0.0, auto_key=0.0, percentile=0.0, white=0.0, curve=CLAMP):
    """(e, w) the map runs with, as the library resolves them from the frame"""
    e = exposure_ if exposure_ > 0.0 else 1.0
    la = lp = 0.0
    if auto_key > 0.0 or (curve == REINHARD and white == 0.0):
        la, lp = exposure(histogram(img), percentile)
        if auto_key > 0.0 and la > 0.0:
            e = e * (auto_key / la)
    w = white
    if curve == REINHARD and w == 0.0:
        w = max(1.0, e * lp)
    return e, w


def pre_quantise(img, e, w, curve=CLAMP, transfer=LINEAR):
    """y * 255 per channel (LINEAR: before truncation; SRGB: before the + 0.5 and the floor), shape of img"""
    a = np.ascontiguousarray(img, dtype=np.float64)
    c = a.reshape(-1, 3)
    with np.errstate(all="ignore"):
        x = e * c
        x = np.where(x > 0.0, x, 0.0)
        x = np.where(x < 2.0 ** 64, x, 2.0 ** 64)
        if curve == REINHARD:
            Yx = (0.2126 * x[:, 0] + 0.7152 * x[:, 1]) + 0.0722 * x[:, 2]
            s = (1.0 + Yx / (w * w)) / (1.0 + Yx)
            y = np.where((Yx == 0.0)[:, None], 0.0, x * s[:, None])
        elif curve == FILMIC:
            y = (x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14)
        else:
            y = x
        y = np.where(y < 1.0, y, 1.0)
        if transfer == SRGB:
            y = np.where(y <= 0.0031308, 12.92 * y, 1.055 * np.power(y, 1.0 / 2.4) - 0.055)
        return (y * 255).reshape(a.shape)


def quantise(v255, transfer=LINEAR):
    if transfer == SRGB:
        return np.floor(v255 + 0.5).astype(np.uint8)
    return np.minimum(np.maximum(v255, 0.0), 255.0).astype(np.uint8)


def srgb_mask(v255):
    """the channels whose byte does not hang on the last bits of pow: y * 255 + 0.5 farther than 1e-6 from an integer"""
    t = v255 + 0.5
    return np.abs(t - np.round(t)) > 1e-6


def display(img, e, w, curve=CLAMP, transfer=LINEAR, rgba=False):
    """(bytes [..., 3 or 4], mask of the channels that are exact [..., 3])"""
    v = pre_quantise(img, e, w, curve, transfer)
    out = quantise(v, transfer)
    mask = srgb_mask(v) if transfer == SRGB else np.ones(v.shape, dtype=bool)
    if rgba:
        out = np.concatenate([out, np.full(out.shape[:-1] + (1,), 255, dtype=np.uint8)], axis=-1)
    return out, mask


def log_uniform_frame(h, w, seed, lo=-12.0, hi=6.0):
    """a seeded frame of log-uniform channels over 2^lo .. 2^hi"""
    rng = np.random.default_rng(seed)
    return np.exp2(rng.uniform(lo, hi, size=(h, w, 3)))


def edge_frame(n, seed):
    """n pixels (n, 3) that sit on the histogram's edges: exact powers of two and the values one ulp either side of them, 2^-24 and 2^24 and
    their neighbours, denormals, 0, negatives, NaN and both infinities, padded with log-uniform values.  Each special value v is placed as a
    grey pixel (v, v, v): its luminance is then within an ulp or two of v, on either side of the edge."""
    rng = np.random.default_rng(seed)
    special = []
    for k in (-25, -24, -23, -3, -1, 0, 1, 5, 23, 24, 25):
        p = math.ldexp(1.0, k)
        special += [p, np.nextafter(p, 0.0), np.nextafter(p, np.inf)]
    special += [5e-324, 2.2e-308, 1e-310, 0.0, -0.0, -1.0, -1e-30, np.nan, np.inf, -np.inf, 1e300, 0.18, 1.0 / 255.0, 254.5 / 255.0]
    special += [math.ldexp(1.0 + j / 8.0, e) for e in (-7, 0, 3) for j in range(8)]       # every sub-bin edge of three stops
    vals = np.exp2(rng.uniform(-26.0, 26.0, size=(n, 3)))
    idx = rng.permutation(n)[:min(n, len(special))]
    order = rng.permutation(len(special))[:len(idx)]
    for i, j in zip(idx, order):
        vals[i, :] = special[j]
    if n >= 64:
        vals[rng.integers(n), :] = (np.nan, 1.0, 1.0)          # a NaN in one channel only
        vals[rng.integers(n), :] = (-3.0, 0.5, 2.0)            # a negative beside values above and below 1
    return np.ascontiguousarray(vals)
