"""numpy restatement of the environment light (include/mcpt.h: environment light; csrc/environment.cpp, csrc/env.hpp): the fp64 tables,
the nearest-texel lookup, the draw of a direction and its pdf -- in the header's operation order, so that texel choices, pdfs and radiances
match the device bit for bit (row borders through math.cos, the C library's cosine, as the host's std::cos)."""
import math

import numpy as np

import lens_ref

PI = 3.141592653589793
TWO_PI = 6.283185307179586


class EnvRef:
    def __init__(self, rgb, scale=1.0):
        a = np.asarray(rgb, dtype=np.float64)
        if a.ndim == 1:
            a = a.reshape(1, 1, 3)
        self.tex = np.ascontiguousarray(a, dtype=np.float32)
        self.H, self.W = self.tex.shape[:2]
        self.scale = float(scale)
        H, W = self.H, self.W
        c = np.array([math.cos(PI * float(i) / float(H)) for i in range(H + 1)])
        c[0], c[H] = 1.0, -1.0
        self.c = c
        t = self.tex.astype(np.float64)
        self.lum = (0.2126 * t[..., 0] + 0.7152 * t[..., 1]) + 0.0722 * t[..., 2]
        self.omega = ((c[:-1] - c[1:]) * TWO_PI) / float(W)
        self.cond = np.zeros((H, W))
        self.marg = np.zeros(H)
        run = 0.0
        for i in range(H):
            row = 0.0
            for j in range(W):
                row += self.lum[i, j] * self.omega[i]
                self.cond[i, j] = row
            run += row
            self.marg[i] = run
        self.Z = run

    @property
    def active(self):
        return self.Z > 0.0

    def radiance(self, i, j):
        return self.scale * self.tex[i, j].astype(np.float64)

    def texel_of(self, d):
        """(row, column) of directions d (n, 3)"""
        d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
        phi = np.arctan2(d[:, 2], d[:, 0])
        phi = np.where(phi < 0.0, phi + TWO_PI, phi)
        j = np.minimum(self.W - 1, np.floor(phi * float(self.W) / TWO_PI).astype(np.int64))
        y = np.clip(d[:, 1], -1.0, 1.0)
        # the row with c[i+1] < y <= c[i]; the last row also takes y = -1
        i = np.array([min(int(np.argmax(self.c[1:] < yy)) if np.any(self.c[1:] < yy) else self.H - 1, self.H - 1) for yy in y])
        return i, j

    def eval(self, d):
        i, j = self.texel_of(d)
        return self.scale * self.tex[i, j].astype(np.float64)

    def pdf(self, i, j):
        """solid-angle pdf of a direction in texel (i, j)"""
        return self.lum[i, j] / self.Z

    def sample_u(self, u0, u1, u2, u3):
        """texel, direction, pdf and radiance of the draw from uniforms u0..u3 (arrays)"""
        u0, u1, u2, u3 = (np.asarray(u, dtype=np.float64) for u in (u0, u1, u2, u3))
        i = np.minimum(np.searchsorted(self.marg, u0 * self.Z, side="right"), self.H - 1)
        rowsum = self.cond[i, self.W - 1]
        j = np.array([min(int(np.searchsorted(self.cond[ii], r, side="right")), self.W - 1) for ii, r in zip(i, u1 * rowsum)], dtype=np.int64)
        ct = self.c[i] + (self.c[i + 1] - self.c[i]) * u2
        st = np.sqrt(np.maximum(0.0, 1.0 - ct * ct))
        phi = (TWO_PI * (j.astype(np.float64) + u3)) / float(self.W)
        d = np.stack([st * np.cos(phi), ct, st * np.sin(phi)], axis=1)
        pdf = self.lum[i, j] / self.Z
        rgb = self.scale * self.tex[i, j].astype(np.float64)
        return i, j, d, pdf, rgb


def vertex_uniforms(seed, pix, k, depth, nl):
    """u0..u3 of Philox block nl + 2 at vertex `depth` of samples (pix, k) (dev_common.hpp: uniform4)"""
    pix = np.asarray(pix, dtype=np.uint64)
    k = np.asarray(k, dtype=np.uint64)
    w = lens_ref.philox4x32_10(pix, k, np.full(pix.shape, (int(depth) << 16) | (int(nl) + 2), dtype=np.uint64),
                               np.full(pix.shape, 0x4D435054, dtype=np.uint64), int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    return [(x.astype(np.float64) + 0.5) * 2.0 ** -32 for x in w]
