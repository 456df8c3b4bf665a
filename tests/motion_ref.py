"""numpy restatement of a motion's arithmetic (include/mcpt.h, motion blur): the time of a shutter step, the step of a sample and the blend
of two keyframes.  numpy's float64 has no fused multiply-add, so the blend has the bits of the library's kernel, which is compiled without
contraction."""
import numpy as np


def shutter_time(open, close, steps, j):
    """u_j = open + (close - open) * ((j + 0.5) / K), every operation rounded to fp64 as written"""
    o, c = np.float64(open), np.float64(close)
    return float(o + (c - o) * ((np.float64(j) + np.float64(0.5)) / np.float64(steps)))


def shutter_step(spp, steps, k):
    """sample k of an spp-sample frame belongs to step (k * K) // N"""
    return (int(k) * int(steps)) // int(spp)


def step_ranges(spp, steps):
    """[(first sample, count)] of the steps 0 .. K-1"""
    owner = [shutter_step(spp, steps, k) for k in range(spp)]
    return [(owner.index(j), owner.count(j)) for j in range(steps)]


def blend(x0, x1, u):
    """x(u) = (1 - u) * x0 + u * x1 per coordinate -- and x0 itself where x0 == x1: a coordinate that does not move keeps its bits"""
    x0, x1 = np.asarray(x0, dtype=np.float64), np.asarray(x1, dtype=np.float64)
    u = np.float64(u)
    with np.errstate(all="ignore"):
        mixed = (np.float64(1.0) - u) * x0 + u * x1
    return np.where(x0 == x1, x0, mixed)


def blend_camera(c0, c1, u):
    """the camera dicts (eye, look_at, up, fovy) blended coordinate by coordinate"""
    out = {k: blend(c0[k], c1[k], u) for k in ("eye", "look_at", "up")}
    out["fovy"] = float(blend(c0["fovy"], c1["fovy"], u))
    return out


def fold(x, n):
    """the frame's fold of samples x[..., k, :] of an n-sample frame: float32(float64(acc) + x / n) in k order"""
    acc = np.zeros(x.shape[:-2] + x.shape[-1:], dtype=np.float32)
    for k in range(x.shape[-2]):
        acc = (acc.astype(np.float64) + x[..., k, :] / n).astype(np.float32)
    return acc.astype(np.float64)
