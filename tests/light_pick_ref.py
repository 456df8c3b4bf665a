"""numpy restatement of MCPT_LIGHTS_ONE's light pick (include/mcpt.h: light sampling; csrc/light_sampling.cpp, csrc/vertex.hpp): the fp64
table in the header's operation order -- running sums left to right, pdf = w / Z, the factor 1.0 / pdf -- and the pick from slot 0 of
Philox block nl + 3, so that tables, picked lights and probabilities match the library bit for bit."""
import numpy as np

import lens_ref


def luminance(rgb):
    return (0.2126 * rgb[0] + 0.7152 * rgb[1]) + 0.0722 * rgb[2]


def default_weights(radiance, area):
    """luminance x area per light; all ones when every product is 0"""
    w = np.array([luminance([float(c) for c in r]) * float(a) for r, a in zip(radiance, area)], dtype=np.float64)
    w = np.where(np.isfinite(w) & (w >= 0.0), w, 0.0)
    return w if (w > 0.0).any() else np.ones_like(w)


class PickRef:
    def __init__(self, weights):
        w = np.asarray(weights, dtype=np.float64).reshape(-1)
        if not (np.isfinite(w).all() and (w >= 0.0).all() and (w > 0.0).any()):
            raise ValueError("weights: finite, >= 0, not all 0")
        self.w = w
        self.cdf = np.zeros_like(w)
        run = 0.0
        for l, x in enumerate(w):            # sequential, left to right (np.cumsum may sum pairwise)
            run = run + float(x)
            self.cdf[l] = run
        self.Z = run
        self.pdf = w / run
        self.inv = np.zeros_like(w)
        np.divide(1.0, self.pdf, out=self.inv, where=self.pdf > 0.0)
        self.last = int(np.nonzero(w > 0.0)[0][-1])

    @classmethod
    def of_scene(cls, scene, weights=None):
        if weights is not None:
            return cls(weights)
        lights = [scene.light(i) for i in range(scene.info.num_lights)]
        return cls(default_weights([l[1] for l in lights], [l[3] for l in lights]))

    def pick_u(self, u):
        """the smallest l with u * Z < cdf[l], clamped to the last light of non-zero weight"""
        x = np.asarray(u, dtype=np.float64) * self.Z
        return np.minimum(np.searchsorted(self.cdf, x, side="right"), self.last).astype(np.int32)

    def pick(self, seed, pix, k, depth):
        """(light, pdf) at vertex `depth` of camera samples (pix, k)"""
        l = self.pick_u(pick_uniform(seed, pix, k, depth, self.w.shape[0]))
        return l, self.pdf[l]


def pick_uniform(seed, pix, k, depth, nl):
    """slot 0 of Philox block nl + 3 at vertex `depth` of samples (pix, k) (dev_common.hpp: uniform1)"""
    pix = np.asarray(pix, dtype=np.uint64)
    k = np.asarray(k, dtype=np.uint64)
    w = lens_ref.philox4x32_10(pix, k, np.full(pix.shape, (int(depth) << 16) | (int(nl) + 3), dtype=np.uint64),
                               np.full(pix.shape, 0x4D435054, dtype=np.uint64), int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    return (w[0].astype(np.float64) + 0.5) * 2.0 ** -32


def path_pick_estimate(per_light, light, inv):
    """A second unbiased estimator of sum_l per_light[l], made in numpy alone: sample i keeps the one light light[i] for its whole path and
    divides by that light's probability -- per_light[light[i], i] * inv[light[i]].  per_light: (nl, n, 3), light: (n,), inv: (nl,)."""
    i = np.arange(light.shape[0])
    return per_light[light, i] * np.asarray(inv)[light][:, None]


def block_z(diff, block):
    """block means of per-sample differences (n, 3) and their standard errors: (means, sigmas), each (n // block, 3)"""
    n = diff.shape[0] // block * block
    d = diff[:n].reshape(-1, block, 3)
    return d.mean(axis=1), d.std(axis=1, ddof=1) / np.sqrt(block)
