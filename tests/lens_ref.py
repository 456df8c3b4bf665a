"""numpy restatement of the camera lens (include/mcpt.h, "camera lens"; csrc/camera.hpp: camera_ray) in fp64, in the library's operation
order: the camera frame of generateImg (pathTracing.cpp:276-294, scene_loader.cpp: camera_frame), the running-sum corners pos(i,j), the
Philox counter of the camera uniforms and the pinhole / thin-lens rays.  Vectorised over samples; no contraction (numpy has none)."""
import math

import numpy as np

LENS_JITTER, LENS_PER_SAMPLE = 1, 2
LENS_RNG_DEPTH = 0xFFFF
TWO_PI = 2.0 * math.pi


def _v(x):
    return [float(x[0]), float(x[1]), float(x[2])]


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _add(a, b):
    return [a[0] + b[0], a[1] + b[1], a[2] + b[2]]


def _mul(a, s):
    return [a[0] * s, a[1] * s, a[2] * s]


def _norm(a):
    return math.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])


def _normalized(a):
    d = _norm(a)
    return [a[0] / d, a[1] / d, a[2] / d]


def _cross(a, b):
    return [a[1] * b[2] - b[1] * a[2], b[0] * a[2] - a[0] * b[2], a[0] * b[1] - b[0] * a[1]]


class Camera:
    """generateImg's frame from a scene's camera (eye, look_at, up, fovy, width, height) and the image-plane point of every pixel."""

    def __init__(self, eye, look_at, up, fovy, width, height):
        pi = 3.1415926                                      # pathTracing.h:11 (the reference's pi, in the frame only)
        self.width, self.height = int(width), int(height)
        self.eye, self.look_at = _v(eye), _v(look_at)
        self.up = _normalized(_v(up))
        d = _sub(self.look_at, self.eye)
        self.l = _norm(d)
        dy = math.tan(float(fovy) / 2 / 180 * pi) * self.l
        dx = dy / self.height * self.width
        pdx, pdy = 2 * dx / self.width, 2 * dy / self.height
        self.xhat = _normalized(_cross(d, self.up))
        self.pdx = _mul(self.xhat, pdx)
        self.pdy = _mul(self.up, pdy)
        self.start = _add(_sub(self.look_at, _mul(self.xhat, dx)), _mul(self.up, dy))
        self._pos = None

    @classmethod
    def from_info(cls, info):
        """from mcpt_scene_info (montecarlopathtracing_amd.Scene.info)"""
        return cls(info.eye, info.look_at, info.up, info.fovy, info.width, info.height)

    @property
    def pos(self):
        """[H*W, 3]: pos(i,0) = start - pdy*i, pos(i,j+1) = pos(i,j) + pdx (pathTracing.cpp:297,326)"""
        if self._pos is None:
            i = np.arange(self.height, dtype=np.float64)
            out = np.empty((self.height, self.width, 3))
            row = np.stack([self.start[c] - self.pdy[c] * i for c in range(3)], axis=1)
            for j in range(self.width):
                out[:, j] = row
                row = row + np.array(self.pdx)
            self._pos = out.reshape(-1, 3)
        return self._pos


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays holding 32-bit words (dev_common.hpp: philox4x32_10)"""
    M = np.uint64(0xFFFFFFFF)
    c = [np.asarray(x, dtype=np.uint64) & M for x in (c0, c1, c2, c3)]
    k0 = np.uint64(k0) & M
    k1 = np.uint64(k1) & M
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & M
        hi1, lo1 = p1 >> np.uint64(32), p1 & M
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M
        k1 = (k1 + np.uint64(0xBB67AE85)) & M
    return c


def camera_uniforms(seed, pix, k):
    """u0..u3 of samples (pix, k): words 0..3 of the block with counter (pix, k, 0xFFFF << 16 | 0, 'MCPT'), key = seed, (w + 0.5) 2^-32"""
    pix = np.asarray(pix, dtype=np.uint64)
    k = np.asarray(k, dtype=np.uint64)
    w = philox4x32_10(pix, k, np.full(pix.shape, LENS_RNG_DEPTH << 16, dtype=np.uint64), np.full(pix.shape, 0x4D435054, dtype=np.uint64),
                      int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    return [(x.astype(np.float64) + 0.5) * 2.0 ** -32 for x in w]


def _nrm(a):
    d = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])
    return a / d[:, None]


def camera_ray(cam, seed, pix, k, aperture=0.0, focus_distance=0.0, jitter=False):
    """[n, 6] = origin, direction of the camera rays of samples (pix[i], k[i])"""
    pix = np.atleast_1d(np.asarray(pix, dtype=np.int64))
    k = np.atleast_1d(np.asarray(k, dtype=np.int64))
    q = cam.pos[pix].copy()
    eye = np.array(cam.eye)
    u0, u1, u2, u3 = camera_uniforms(seed, pix, k)
    if jitter:
        q = (q + np.array(cam.pdx)[None, :] * u0[:, None]) - np.array(cam.pdy)[None, :] * u1[:, None]
    if not aperture > 0.0:
        o = np.broadcast_to(eye, q.shape).copy()
        return np.concatenate([o, _nrm(q - eye[None, :])], axis=1)
    F = focus_distance if focus_distance > 0.0 else cam.l
    f = eye[None, :] + (q - eye[None, :]) * (F / cam.l)
    r = aperture * np.sqrt(u2)
    phi = TWO_PI * u3
    o = (eye[None, :] + np.array(cam.xhat)[None, :] * (r * np.cos(phi))[:, None]) + np.array(cam.up)[None, :] * (r * np.sin(phi))[:, None]
    return np.concatenate([o, _nrm(f - o)], axis=1)
