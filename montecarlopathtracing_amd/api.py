"""Python face of libmcpt's C ABI, named after the reference's own functions and types
(render_scene / scene_data / BVH / ray_intersect / generateImg / imshow)."""
import ctypes as C
import math
import numbers

import numpy as np

from . import _lib
from ._lib import AdaptiveParams, CameraKey, DenoiseParams, DisplayInfo, DisplayParams, GuideParams, Environment, FastInfo, Lens, LightSampling, McptError, MotionInfo, Noise, QueryParams, ShParams, LightmapParams, LightmapDenoiseParams, VolumeGrid, VisibilityParams, VolumeVisibility, BakedSource, BakedOutputs, BakedFrameParams, BakedSpecular, BakedSpecularOutputs, ReflectionParams, ReflectionChain, OcclusionParams, OcclusionMap, PairParams, DirectLight, DirectParams, DirectMap, Shutter, RenderParams, RenderSceneOptions, SceneDesc, SceneInfo, Stats, UpdateInfo, check, lib


TRACE_FAST, TRACE_REFERENCE = 0, 1
RENDER_DEFAULT, RENDER_MEGAKERNEL = 0, 2
RENDER_KEEP_STATS, RENDER_PIPELINE = 4, 8
LOAD_STANDARD_OBJ, LOAD_MTLLIB, LOAD_MORTON_BOUNDS = 1, 2, 4
OUT_PNG_DEFLATE, OUT_PFM, OUT_ERROR_PFM, OUT_SPP_PFM, OUT_DENOISED, OUT_AOV_PFM = 1, 2, 4, 8, 16, 32
OUT_DENOISED_SAMPLES, OUT_SAMPLE_AOV_PFM = 64, 128
BUILD_HOST, BUILD_DEVICE, BUILD_DEVICE_FAST, BUILD_DEVICE_SAH = 0, 1, 2, 3
UPDATE_REFIT, UPDATE_REBUILD = 0, 1
# mcpt_fast_info.builder: which builder made the culling hierarchy a device walks
FAST_BUILT_HOST, FAST_BUILT_DEVICE_FAST, FAST_BUILT_DEVICE_PLOC, FAST_BUILT_PLOC_FELL_BACK = 0, 1, 2, 3
SCENE_DEFER_BUILD = 1
GATHER_PEER, GATHER_RCCL = 0, 1
LENS_JITTER, LENS_PER_SAMPLE = 1, 2
QUERY_RAY, QUERY_HEMISPHERE = 0, 1
_QUERY_KINDS = {"ray": QUERY_RAY, "hemisphere": QUERY_HEMISPHERE}
# mcpt.h: MCPT_LIGHTMAP_DENOISE_*
LIGHTMAP_DENOISE_ITERATIONS, LIGHTMAP_DENOISE_MAX_ITERATIONS = 5, 10
LIGHTMAP_DENOISE_SIGMA_L, LIGHTMAP_DENOISE_SIGMA_P = 2.0, 1.0
VOLUME_CLAMP_ZERO = 1
# mcpt.h: MCPT_BAKED_* -- the kinds of a baked source, the kinds of a sample, the flags of a baked call
BAKED_VOLUME, BAKED_LIGHTMAP = 1, 2
BAKED_MISS, BAKED_EMITTER, BAKED_SURFACE = 0, 1, 2
BAKED_FACE_VIEWER, BAKED_LIGHTING_ONLY = 1, 2


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def _dp(ptr):
    """a device pointer or stream given as an address (a torch tensor's data_ptr()) or as a ctypes pointer; None or 0: null"""
    if isinstance(ptr, C.c_void_p):
        return ptr
    return C.c_void_p(ptr) if ptr else None


def make_lens(aperture=0.0, focus_distance=0.0, jitter=False, per_sample=False):
    """An mcpt_lens: jitter = uniform over the pixel square, aperture > 0 = a thin lens of that radius focused at focus_distance
    (<= 0: at look_at), per_sample = a camera ray per sample even for the pinhole (mcpt.h: camera lens)."""
    return Lens((LENS_JITTER if jitter else 0) | (LENS_PER_SAMPLE if per_sample else 0), 0, float(aperture), float(focus_distance))


def make_environment(rgb, scale=1.0):
    """An mcpt_environment and the float32 texels it points to (keep both alive while it is used): rgb = an (H, W, 3) radiance map, top
    row first, or an (r, g, b) constant sky (a 1x1 map)."""
    a = np.asarray(rgb, dtype=np.float64)
    if a.ndim == 1:
        a = a.reshape(1, 1, 3)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("an environment is an (H, W, 3) array or an (r, g, b) triple")
    tex = np.ascontiguousarray(a, dtype=np.float32)
    e = Environment(tex.shape[1], tex.shape[0], _p(tex, C.c_float), float(scale), 0, 0)
    return e, tex


CURVE_CLAMP, CURVE_REINHARD, CURVE_FILMIC = 0, 1, 2
TRANSFER_LINEAR, TRANSFER_SRGB = 0, 1
DISPLAY_RGBA = 1
DISPLAY_BINS, DISPLAY_SLOTS = 384, 387
DISPLAY_ESTIMATE, DISPLAY_DENOISED, DISPLAY_DENOISED_GUIDED = 0, 1, 2
_CURVES = {"clamp": CURVE_CLAMP, "reinhard": CURVE_REINHARD, "filmic": CURVE_FILMIC}
_TRANSFERS = {"linear": TRANSFER_LINEAR, "srgb": TRANSFER_SRGB}
_SOURCES = {"estimate": DISPLAY_ESTIMATE, "denoised": DISPLAY_DENOISED, "denoised_guided": DISPLAY_DENOISED_GUIDED}


def make_display(exposure=0, auto_key=0, percentile=0, white=0, curve="clamp", transfer="linear", rgba=False):
    """An mcpt_display_params (mcpt.h: display transform).  exposure: a factor (0: 1.0); auto_key > 0: the exposure is scaled so that the
    frame's log-average luminance lands on that key (0.18 is the usual one); percentile (0: 0.99) picks the luminance that REINHARD's
    white (0: automatic) is taken from; curve "clamp", "reinhard" or "filmic"; transfer "linear" or "srgb"; rgba: four bytes per pixel,
    alpha 255.  Curve and transfer may be given as their MCPT_* numbers.  All defaults: imshow's bytes."""
    c = _CURVES[curve] if isinstance(curve, str) else int(curve)
    t = _TRANSFERS[transfer] if isinstance(transfer, str) else int(transfer)
    return DisplayParams(float(exposure), float(auto_key), float(percentile), float(white), c, t, DISPLAY_RGBA if rgba else 0, 0)


def _as_display(display):
    if display is None or isinstance(display, DisplayParams):
        return display
    return make_display(**display)


def _frame_pixels(img):
    img = np.ascontiguousarray(img, dtype=np.float64)
    if img.ndim < 1 or img.shape[-1] != 3:
        raise ValueError("a frame is an array of RGB triples")
    return img, img.size // 3


def display_host(img, **kw):
    """The display transform on the CPU (mcpt_display_host; usable without a GPU): img [..., 3] float64 and make_display's arguments ->
    (uint8 array [..., 3] or [..., 4], info dict)."""
    img, n = _frame_pixels(img)
    dp, info = make_display(**kw), DisplayInfo()
    out = np.zeros(img.shape[:-1] + (4 if dp.flags & DISPLAY_RGBA else 3,), dtype=np.uint8)
    check(lib().mcpt_display_host(_p(img, C.c_double), n, C.byref(dp), _p(out, C.c_uint8), C.byref(info)))
    return out, info.as_dict()


def display_exposure(slots, percentile=0.0):
    """(log_average, l_percentile) of a luminance histogram's 387 slots (mcpt_display_exposure; host only)"""
    slots = np.ascontiguousarray(slots, dtype=np.int64).reshape(-1)
    if slots.shape[0] != DISPLAY_SLOTS:
        raise ValueError("a luminance histogram has %d slots" % DISPLAY_SLOTS)
    la, lp = C.c_double(), C.c_double()
    check(lib().mcpt_display_exposure(slots.ctypes.data_as(C.POINTER(C.c_int64)), float(percentile), C.byref(la), C.byref(lp)))
    return la.value, lp.value


def _sh_args(sh, v, what):
    v = np.ascontiguousarray(v, dtype=np.float64)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError("%s must have shape (n, 3), not %r" % (what, v.shape))
    if sh is not None:
        sh = np.ascontiguousarray(sh, dtype=np.float64)
        if sh.shape != (v.shape[0], 9, 3):
            raise ValueError("sh must have shape (%d, 9, 3), not %r" % (v.shape[0], sh.shape))
    return sh, v


def sh_basis(dirs):
    """Y_0..8 of unit directions (n, 3), in mcpt.h's index order (mcpt_sh_basis): (n, 9)"""
    _, d = _sh_args(None, dirs, "dirs")
    y = np.zeros((d.shape[0], 9))
    check(lib().mcpt_sh_basis(_p(d, C.c_double), d.shape[0], _p(y, C.c_double)))
    return y


def sh_radiance(sh, dirs):
    """the radiance probe i's coefficients sh[i] (9, 3) give along the unit direction dirs[i] (mcpt_sh_radiance): (n, 3)"""
    sh, d = _sh_args(sh, dirs, "dirs")
    rgb = np.zeros((d.shape[0], 3))
    check(lib().mcpt_sh_radiance(_p(sh, C.c_double), _p(d, C.c_double), d.shape[0], _p(rgb, C.c_double)))
    return rgb


def sh_irradiance(sh, normals):
    """the irradiance probe i's coefficients sh[i] (9, 3) give a receiver of normal normals[i], any non-zero length (mcpt_sh_irradiance): (n, 3)"""
    sh, nrm = _sh_args(sh, normals, "normals")
    e = np.zeros((nrm.shape[0], 3))
    check(lib().mcpt_sh_irradiance(_p(sh, C.c_double), _p(nrm, C.c_double), nrm.shape[0], _p(e, C.c_double)))
    return e


def volume_grid(origin, spacing, counts, clamp_zero=False):
    """An mcpt_volume_grid (mcpt.h: irradiance volumes): probe (ix, iy, iz) sits at origin + (ix, iy, iz) * spacing; counts = (nx, ny, nz);
    spacing is a triple or one number for all axes; clamp_zero: the lookup returns max(E, 0).  The library judges the values."""
    origin = np.asarray(origin, dtype=np.float64).reshape(-1)
    spacing = np.asarray(spacing, dtype=np.float64).reshape(-1)
    if spacing.shape[0] == 1:
        spacing = np.repeat(spacing, 3)
    counts = tuple(counts)
    if origin.shape[0] != 3 or spacing.shape[0] != 3 or len(counts) != 3:
        raise ValueError("origin, spacing and counts are triples")
    for v in counts:
        if not isinstance(v, numbers.Integral) or not -2 ** 31 <= v < 2 ** 31:
            raise ValueError("counts must be 32-bit integers")
    return VolumeGrid((C.c_double * 3)(*origin), (C.c_double * 3)(*spacing), int(counts[0]), int(counts[1]), int(counts[2]),
                      VOLUME_CLAMP_ZERO if clamp_zero else 0, (C.c_int32 * 4)(0, 0, 0, 0))


def _grid_probes(grid):
    """the number of probes the arrays of `grid` must hold (0 for counts the library will refuse)"""
    if not isinstance(grid, VolumeGrid):
        raise ValueError("grid must be a VolumeGrid (volume_grid makes one)")
    n = max(grid.nx, 0) * max(grid.ny, 0) * max(grid.nz, 0)
    return n if n < 2 ** 31 else 0


def volume_points(grid):
    """The probe positions of a grid (mcpt_volume_points; no device): (nz * ny * nx, 3), probe (ix, iy, iz) at row (iz * ny + iy) * nx + ix"""
    p = np.zeros((_grid_probes(grid), 3))
    check(lib().mcpt_volume_points(C.byref(grid), _p(p, C.c_double)))
    return p


def _volume_args(grid, sh, points, normals, valid):
    probes = _grid_probes(grid)
    sh = np.ascontiguousarray(sh, dtype=np.float64)
    if sh.shape[-2:] != (9, 3) or sh.size != probes * 27:
        raise ValueError("sh must hold (9, 3) coefficients for each of the grid's %d probes, not %r" % (probes, sh.shape))
    points = np.asarray(points, dtype=np.float64)
    normals = np.asarray(normals, dtype=np.float64)
    if points.ndim != 2 or points.shape[1] != 3 or normals.shape != points.shape:
        raise ValueError("points and normals must both have shape (n, 3)")
    if valid is not None:
        valid = np.ascontiguousarray(valid)
        if valid.dtype.kind not in "biu" or valid.size != probes:
            raise ValueError("valid must hold one flag for each of the grid's %d probes" % probes)
        valid = np.ascontiguousarray(valid != 0, dtype=np.uint8)
    return sh, np.ascontiguousarray(np.concatenate([points, normals], axis=1)), valid


def volume_irradiance_host(grid, sh, points, normals, valid=None):
    """The irradiance volume's lookup on the CPU (mcpt_volume_irradiance_host; no device): sh [nz, ny, nx, 9, 3] (or [nprobes, 9, 3]) the
    probes' coefficients, receiver i at points[i] with normal normals[i] of any non-zero length, valid one flag per probe or None.
    Returns (E [n, 3], corners [n]): the trilinear blend of the eight probes around each point under the cosine lobe of its normal, and
    how many of the eight took part."""
    sh, q, valid = _volume_args(grid, sh, points, normals, valid)
    n = q.shape[0]
    E, corners = np.zeros((n, 3)), np.zeros(n, dtype=np.int32)
    check(lib().mcpt_volume_irradiance_host(C.byref(grid), _p(sh, C.c_double), _p(valid, C.c_uint8), _p(q, C.c_double), n, _p(E, C.c_double),
                                            _p(corners, C.c_int32)))
    return E, corners


def visibility_bin(dirs, res):
    """The octahedral bin of each direction dirs (n, 3), of any non-zero finite length, in a res x res map (mcpt_visibility_bin; no
    device): (n,) int32 in 0 .. res * res - 1, bin = by * res + bx."""
    d = np.ascontiguousarray(dirs, dtype=np.float64)
    if d.ndim != 2 or d.shape[1] != 3:
        raise ValueError("dirs must have shape (n, 3)")
    if not isinstance(res, numbers.Integral) or not -2 ** 31 <= res < 2 ** 31:
        raise ValueError("res must be a 32-bit integer")
    out = np.zeros(d.shape[0], dtype=np.int32)
    check(lib().mcpt_visibility_bin(_p(d, C.c_double), d.shape[0], int(res), _p(out, C.c_int32)))
    return out


def volume_visibility(res=8, max_distance=1.0, normal_bias=0.0, min_visibility=0.0):
    """An mcpt_volume_visibility (mcpt.h: probe visibility) for volume_irradiance_visible: res and max_distance are the bake's;
    normal_bias lifts a receiver off its surface along its normal before the probes' maps are asked; min_visibility is the factor's
    floor.  The library judges the values."""
    if not isinstance(res, numbers.Integral) or not -2 ** 31 <= res < 2 ** 31:
        raise ValueError("res must be a 32-bit integer")
    return VolumeVisibility(int(res), 0, float(max_distance), float(normal_bias), float(min_visibility), (C.c_int32 * 4)(0, 0, 0, 0))


def _visibility_moments(grid, vis, moments):
    if not isinstance(vis, VolumeVisibility):
        raise ValueError("vis must be a VolumeVisibility (volume_visibility makes one)")
    probes, bins = _grid_probes(grid), vis.res ** 2 if 1 <= vis.res <= 16 else 0
    moments = np.ascontiguousarray(moments, dtype=np.float64)
    if moments.shape[-1:] != (2,) or moments.size != probes * bins * 2:
        raise ValueError("moments must hold (%d, 2) values for each of the grid's %d probes, not %r" % (bins, probes, moments.shape))
    return moments


def volume_irradiance_visible_host(grid, sh, moments, points, normals, vis, valid=None):
    """The visibility-weighted lookup on the CPU (mcpt_volume_irradiance_visible_host; no device): volume_irradiance_host with every
    corner's weight multiplied by what its probe sees of the receiver -- moments [nz, ny, nx, res * res, 2] (or [nprobes, res * res, 2])
    from bake_volume_visibility, vis from volume_visibility.  Returns (E [n, 3], corners [n])."""
    sh, q, valid = _volume_args(grid, sh, points, normals, valid)
    moments = _visibility_moments(grid, vis, moments)
    n = q.shape[0]
    E, corners = np.zeros((n, 3)), np.zeros(n, dtype=np.int32)
    check(lib().mcpt_volume_irradiance_visible_host(C.byref(grid), _p(sh, C.c_double), _p(moments, C.c_double), _p(valid, C.c_uint8), C.byref(vis),
                                                    _p(q, C.c_double), n, _p(E, C.c_double), _p(corners, C.c_int32)))
    return E, corners


def _lightmap_args(E, uv, owner):
    E = np.ascontiguousarray(E, dtype=np.float64)
    if E.ndim != 3 or E.shape[2] != 3:
        raise ValueError("E must have shape (height, width, 3), not %r" % (E.shape,))
    uv = np.ascontiguousarray(uv, dtype=np.float64)
    if uv.ndim != 2 or uv.shape[1] != 2:
        raise ValueError("uv must have shape (n, 2), not %r" % (uv.shape,))
    if owner is not None:
        owner = np.ascontiguousarray(owner, dtype=np.int32)
        if owner.shape != E.shape[:2]:
            raise ValueError("owner must have shape (height, width) = %r, not %r" % (E.shape[:2], owner.shape))
    return E, uv, owner


def lightmap_irradiance_host(E, uv, owner=None):
    """A lightmap's lookup by chart coordinate on the CPU (mcpt_lightmap_irradiance_host; no device): E [height, width, 3] and owner
    [height, width] (or None) as bake_lightmap returns them, uv (n, 2) chart coordinates.  Returns (e [n, 3], taps [n]): the bilinear
    blend of the four texels around each coordinate -- texel x has its centre at (x + 0.5) / width, no flip, no wrap, the border's texels
    outside the map -- leaving out texels whose owner is -1, and how many of the four took part."""
    E, uv, owner = _lightmap_args(E, uv, owner)
    n = uv.shape[0]
    e, taps = np.zeros((n, 3)), np.zeros(n, dtype=np.int32)
    check(lib().mcpt_lightmap_irradiance_host(E.shape[1], E.shape[0], _p(E, C.c_double), _p(owner, C.c_int32), _p(uv, C.c_double), n,
                                              _p(e, C.c_double), _p(taps, C.c_int32)))
    return e, taps


class _Baked:
    """What lights the surfaces of a baked frame (mcpt_baked_source) with the arrays it points to; baked_volume and baked_lightmap make one"""

    def __init__(self, kind, **arrays):
        self.kind = kind
        self.__dict__.update(arrays)

    def struct(self):
        """the mcpt_baked_source of host pointers into this object's arrays (which must outlive it)"""
        s = BakedSource()
        s.kind = self.kind
        addr = lambda a: a.ctypes.data if a is not None else None
        if self.kind == BAKED_VOLUME:
            s.grid = C.pointer(self.grid)
            s.sh27, s.valid, s.moments = addr(self.sh), addr(self.valid), addr(self.moments)
            if self.vis is not None:
                s.visibility = C.pointer(self.vis)
        else:
            s.uv6, s.irradiance3, s.owner = addr(self.uv), addr(self.E), addr(self.owner)
            s.height, s.width = self.E.shape[:2]
        return s


def baked_volume(grid, sh, valid=None, moments=None, vis=None):
    """An irradiance volume as the source of Device.baked_radiance and Device.render_baked: grid, sh and valid as volume_irradiance takes
    them; with moments (and vis, from volume_visibility) the lookup is volume_irradiance_visible's."""
    probes = _grid_probes(grid)
    sh = np.ascontiguousarray(sh, dtype=np.float64)
    if sh.shape[-2:] != (9, 3) or sh.size != probes * 27:
        raise ValueError("sh must hold (9, 3) coefficients for each of the grid's %d probes, not %r" % (probes, sh.shape))
    if valid is not None:
        valid = np.ascontiguousarray(valid)
        if valid.dtype.kind not in "biu" or valid.size != probes:
            raise ValueError("valid must hold one flag for each of the grid's %d probes" % probes)
        valid = np.ascontiguousarray(valid != 0, dtype=np.uint8)
    if moments is not None:
        moments = _visibility_moments(grid, vis, moments)
    elif vis is not None:
        raise ValueError("vis without moments")
    return _Baked(BAKED_VOLUME, grid=grid, sh=sh, valid=valid, moments=moments, vis=vis)


def baked_lightmap(E, uv=None, owner=None):
    """A lightmap as the source of Device.baked_radiance and Device.render_baked: E [height, width, 3] and owner [height, width] (or
    None) as bake_lightmap returns them, uv (num_faces, 6) the chart it was baked under, None: the scene's own vt."""
    E, _, owner = _lightmap_args(E, np.zeros((0, 2)), owner)
    return _Baked(BAKED_LIGHTMAP, E=E, uv=_chart(uv) if uv is not None else None, owner=owner)


def _int32(**values):
    for name, v in values.items():
        if not isinstance(v, numbers.Integral) or not -2 ** 31 <= v < 2 ** 31:
            raise ValueError("%s must be a 32-bit integer" % name)


def reflection_chain(res, levels):
    """An mcpt_reflection_chain (mcpt.h: reflection probes) for prefilter_reflection and reflection_lookup: res is the source map's
    resolution, levels 1 to 8 pairs (level_res, ns) -- the level's resolution and the integer exponent of its Phong lobe, exponents
    strictly descending.  The library judges the values."""
    levels = [tuple(l) for l in levels]
    if len(levels) > 8 or any(len(l) != 2 for l in levels):
        raise ValueError("levels must be at most 8 pairs (level_res, ns)")
    _int32(res=res, **{"%s of level %d" % (name, i): v for i, l in enumerate(levels) for name, v in zip(("level_res", "ns"), l)})
    c = ReflectionChain()
    c.res, c.num_levels = int(res), len(levels)
    for i, (r, ns) in enumerate(levels):
        c.level_res[i], c.level_ns[i] = int(r), int(ns)
    return c


def reflection_texels(res):
    """The texels of a res x res octahedral map (mcpt_reflection_texels; no device): (d [res * res, 3], w [res * res]), the centre
    directions and the midpoint-rule solid angles, texel b = y * res + x."""
    _int32(res=res)
    n = int(res) ** 2 if 1 <= res <= 256 else 0             # (the library refuses any other res)
    d, w = np.zeros((n, 3)), np.zeros(n)
    check(lib().mcpt_reflection_texels(int(res), _p(d, C.c_double), _p(w, C.c_double)))
    return d, w


def _reflection_maps(chain_desc, radiance):
    if not isinstance(chain_desc, ReflectionChain):
        raise ValueError("the chain must be a ReflectionChain (reflection_chain makes one)")
    texels = chain_desc.res ** 2 if 1 <= chain_desc.res <= 256 else 0
    radiance = np.ascontiguousarray(radiance, dtype=np.float64)
    if radiance.ndim != 3 or radiance.shape[1:] != (texels, 3):
        raise ValueError("radiance must have shape (n, %d, 3), not %r" % (texels, radiance.shape))
    return radiance


def _reflection_receivers(chain_desc, chain, probe, dirs, ns):
    if not isinstance(chain_desc, ReflectionChain):
        raise ValueError("the chain must be a ReflectionChain (reflection_chain makes one)")
    chain = np.ascontiguousarray(chain, dtype=np.float64)
    if chain.ndim != 3 or chain.shape[1:] != (chain_desc.num_texels, 3):
        raise ValueError("chain must have shape (n, %d, 3), not %r" % (chain_desc.num_texels, chain.shape))
    dirs = np.ascontiguousarray(dirs, dtype=np.float64)
    if dirs.ndim != 2 or dirs.shape[1] != 3:
        raise ValueError("dirs must have shape (m, 3), not %r" % (dirs.shape,))
    m = dirs.shape[0]
    probe = np.asarray(probe)
    if probe.dtype.kind not in "iu" or probe.shape != (m,):
        raise ValueError("probe must be %d integers" % m)
    if probe.size and (int(probe.min()) < -2 ** 31 or int(probe.max()) >= 2 ** 31):
        raise ValueError("probe indices must fit 32 bits")
    ns = np.ascontiguousarray(np.broadcast_to(np.asarray(ns, dtype=np.float64), (m,)))
    return chain, np.ascontiguousarray(probe, dtype=np.int32), dirs, ns


def reflection_prefilter_host(chain_desc, radiance):
    """The prefilter on the CPU (mcpt_reflection_prefilter_host; no device): radiance [n, res * res, 3] as bake_reflection_probes
    returns it -> chain [n, T, 3], every level the map convolved with the level's Phong lobe, level l at texels
    sum(level_res[:l] ** 2) onwards."""
    radiance = _reflection_maps(chain_desc, radiance)
    chain = np.zeros((radiance.shape[0], chain_desc.num_texels, 3))
    check(lib().mcpt_reflection_prefilter_host(C.byref(chain_desc), _p(radiance, C.c_double), radiance.shape[0], _p(chain, C.c_double)))
    return chain


def reflection_lookup_host(chain_desc, chain, probe, dirs, ns):
    """The lookup on the CPU (mcpt_reflection_lookup_host; no device): for receiver q the radiance chain[probe[q]] holds for direction
    dirs[q] (any non-zero length) under a lobe of exponent ns[q] (a number or an array, finite and >= 0) -- bilinear inside a level
    across the octahedral seams, blended between the two levels whose exponents enclose ns[q].  Returns [m, 3]."""
    chain, probe, dirs, ns = _reflection_receivers(chain_desc, chain, probe, dirs, ns)
    out = np.zeros((dirs.shape[0], 3))
    check(lib().mcpt_reflection_lookup_host(C.byref(chain_desc), _p(chain, C.c_double), chain.shape[0], _p(probe, C.c_int32), _p(dirs, C.c_double),
                                            _p(ns, C.c_double), dirs.shape[0], _p(out, C.c_double)))
    return out


class _BakedReflection:
    """A reflection volume (mcpt_baked_specular) with the arrays it points to; baked_reflection makes one"""

    def __init__(self, grid, chain_desc, chain, valid, moments, vis):
        self.grid, self.chain_desc, self.chain, self.valid, self.moments, self.vis = grid, chain_desc, chain, valid, moments, vis

    def struct(self):
        """the mcpt_baked_specular of host pointers into this object's arrays (which must outlive it)"""
        s = BakedSpecular()
        s.grid, s.chain = C.pointer(self.grid), C.pointer(self.chain_desc)
        addr = lambda a: a.ctypes.data if a is not None else None
        s.chain_data, s.valid, s.moments = addr(self.chain), addr(self.valid), addr(self.moments)
        if self.vis is not None:
            s.visibility = C.pointer(self.vis)
        return s


def baked_reflection(grid, chain_desc, chain, valid=None, moments=None, vis=None):
    """A reflection volume -- the specular source of Device.baked_radiance_specular and Device.render_baked_specular, and what
    reflection_volume_lookup looks up: grid from volume_grid, chain_desc from reflection_chain (or prefilter_reflection), chain
    [nz, ny, nx, T, 3] (or [nprobes, T, 3]) the probes' chains in volume_points' order, valid one flag per probe or None; with moments
    (and vis, from volume_visibility) the corners are volume_irradiance_visible's."""
    probes = _grid_probes(grid)
    if not isinstance(chain_desc, ReflectionChain):
        raise ValueError("the chain must be a ReflectionChain (reflection_chain makes one)")
    chain = np.ascontiguousarray(chain, dtype=np.float64)
    if chain.shape[-2:] != (chain_desc.num_texels, 3) or chain.size != probes * chain_desc.num_texels * 3:
        raise ValueError("chain must hold (%d, 3) texels for each of the grid's %d probes, not %r" % (chain_desc.num_texels, probes, chain.shape))
    if valid is not None:
        valid = np.ascontiguousarray(valid)
        if valid.dtype.kind not in "biu" or valid.size != probes:
            raise ValueError("valid must hold one flag for each of the grid's %d probes" % probes)
        valid = np.ascontiguousarray(valid != 0, dtype=np.uint8)
    if moments is not None:
        moments = _visibility_moments(grid, vis, moments)
    elif vis is not None:
        raise ValueError("vis without moments")
    return _BakedReflection(grid, chain_desc, chain, valid, moments, vis)


def _volume_receivers(volume, points, normals, dirs, ns):
    if not isinstance(volume, _BakedReflection):
        raise ValueError("volume must come from baked_reflection")
    points, normals = np.asarray(points, dtype=np.float64), np.asarray(normals, dtype=np.float64)
    dirs = np.ascontiguousarray(dirs, dtype=np.float64)
    if points.ndim != 2 or points.shape[1] != 3 or normals.shape != points.shape or dirs.shape != points.shape:
        raise ValueError("points, normals and dirs must all have shape (m, 3)")
    ns = np.ascontiguousarray(np.broadcast_to(np.asarray(ns, dtype=np.float64), (points.shape[0],)))
    return np.ascontiguousarray(np.concatenate([points, normals], axis=1)), dirs, ns


def reflection_volume_lookup_host(volume, points, normals, dirs, ns):
    """A reflection volume's lookup on the CPU (mcpt_reflection_volume_lookup_host; no device): for receiver i at points[i] with normal
    normals[i] the radiance volume (from baked_reflection) holds for direction dirs[i] (any non-zero length) under a lobe of exponent
    ns[i] (a number or an array, finite and >= 0) -- reflection_lookup_host of each of the eight probes around the point, blended with
    volume_irradiance's weights (volume_irradiance_visible's when the volume has moments).  Returns (radiance [m, 3], corners [m])."""
    q, dirs, ns = _volume_receivers(volume, points, normals, dirs, ns)
    m = q.shape[0]
    out, corners = np.zeros((m, 3)), np.zeros(m, dtype=np.int32)
    v = volume
    check(lib().mcpt_reflection_volume_lookup_host(C.byref(v.grid), C.byref(v.chain_desc), _p(v.chain, C.c_double), _p(v.valid, C.c_uint8),
                                                   _p(v.moments, C.c_double), C.byref(v.vis) if v.vis is not None else None, _p(q, C.c_double),
                                                   _p(dirs, C.c_double), _p(ns, C.c_double), m, _p(out, C.c_double), _p(corners, C.c_int32)))
    return out, corners


def _baked_flags(face_viewer, lighting_only):
    return (BAKED_FACE_VIEWER if face_viewer else 0) | (BAKED_LIGHTING_ONLY if lighting_only else 0)


def _visibility_params(spp, res, max_distance, max_back_fraction, seed, sample_base, workspace_rays):
    for name, v in (("spp", spp), ("sample_base", sample_base), ("res", res)):
        if not isinstance(v, numbers.Integral) or not -2 ** 31 <= v < 2 ** 31:
            raise ValueError("%s must be a 32-bit integer" % name)
    if not isinstance(workspace_rays, numbers.Integral) or not -2 ** 63 <= workspace_rays < 2 ** 63:
        raise ValueError("workspace_rays must be a 64-bit integer")
    return VisibilityParams(int(spp), int(sample_base), int(seed), int(res), 0, float(max_distance), float(max_back_fraction), int(workspace_rays),
                            (C.c_int32 * 2)(0, 0))


OCCLUSION_HARD, OCCLUSION_LINEAR, OCCLUSION_SQUARE = 0, 1, 2
_FALLOFFS = {"hard": OCCLUSION_HARD, "linear": OCCLUSION_LINEAR, "square": OCCLUSION_SQUARE}


def _occlusion_params(spp, max_distance, falloff, seed, sample_base, workspace_rays):
    """mcpt_occlusion_params: falloff by name ("hard", "linear", "square") or by its MCPT_OCCLUSION_* number (the library judges a number)"""
    for name, v in (("spp", spp), ("sample_base", sample_base)):
        if not isinstance(v, numbers.Integral) or not -2 ** 31 <= v < 2 ** 31:
            raise ValueError("%s must be a 32-bit integer" % name)
    if not isinstance(workspace_rays, numbers.Integral) or not -2 ** 63 <= workspace_rays < 2 ** 63:
        raise ValueError("workspace_rays must be a 64-bit integer")
    if isinstance(falloff, str):
        if falloff not in _FALLOFFS:
            raise ValueError('falloff must be "hard", "linear" or "square"')
        falloff = _FALLOFFS[falloff]
    elif not isinstance(falloff, numbers.Integral) or not -2 ** 31 <= falloff < 2 ** 31:
        raise ValueError('falloff must be "hard", "linear", "square" or a 32-bit integer')
    return OcclusionParams(int(spp), int(sample_base), int(seed), int(falloff), 0, float(max_distance), int(workspace_rays), (C.c_int32 * 2)(0, 0))


def occlusion_fold_host(points, normals, rays, hit, t, face_normals, spp, max_distance, falloff="hard"):
    """The occlusion fold alone, on the CPU (mcpt_occlusion_fold_host; no device): points and normals (n, 3), and for the n * spp rays the
    caller traced -- sample j of entry i at i * spp + j -- rays (n * spp, 6), hit flags, distances t and the hit faces' normals
    (n * spp, 3).  Returns a dict: ao [n], stderr [n], bent [n, 3], hits [n], back [n]."""
    points = np.asarray(points, dtype=np.float64)
    normals = np.asarray(normals, dtype=np.float64)
    if points.ndim != 2 or points.shape[1] != 3 or normals.shape != points.shape:
        raise ValueError("points and normals must both have shape (n, 3)")
    op = _occlusion_params(spp, max_distance, falloff, 0, 0, 0)
    n = points.shape[0]
    m = n * max(int(spp), 0)
    q = np.ascontiguousarray(np.concatenate([points, normals], axis=1))
    rays = np.ascontiguousarray(rays, dtype=np.float64)
    t = np.ascontiguousarray(t, dtype=np.float64)
    face_normals = np.ascontiguousarray(face_normals, dtype=np.float64)
    hit = np.ascontiguousarray(np.asarray(hit) != 0, dtype=np.int32)
    if rays.shape != (m, 6) or t.shape != (m,) or hit.shape != (m,) or face_normals.shape != (m, 3):
        raise ValueError("rays, hit, t and face_normals must have shapes (%d, 6), (%d,), (%d,) and (%d, 3)" % (m, m, m, m))
    ao, err, bent = np.zeros(n), np.zeros(n), np.zeros((n, 3))
    hits, back = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    check(lib().mcpt_occlusion_fold_host(_p(q, C.c_double), _p(rays, C.c_double), _p(hit, C.c_int32), _p(t, C.c_double), _p(face_normals, C.c_double),
                                         n, C.byref(op), _p(ao, C.c_double), _p(err, C.c_double), _p(bent, C.c_double), _p(hits, C.c_int32),
                                         _p(back, C.c_int32)))
    return {"ao": ao, "stderr": err, "bent": bent, "hits": hits, "back": back}


def _pair_args(a, b, t0, t1):
    """the two point lists of a pair call as contiguous (n, 3) arrays and its mcpt_pair_params (the library judges t0 and t1)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 3 or b.ndim != 2 or b.shape[1] != 3:
        raise ValueError("a and b must have shapes (na, 3) and (nb, 3)")
    return a, b, PairParams(float(t0), float(t1), 0, 0)


def pair_rays(a, b, t0=0.0, t1=1.0):
    """The rays of a pair matrix, on the CPU (mcpt_pair_rays; no device): for points a (na, 3) and b (nb, 3) the ray of pair (i, j), at
    i * nb + j, has d = b - a and o = a + t0 * d, and every pair has the limit t1 - t0.  Returns (rays6 [na * nb, 6], tmax);
    Device.any_hit(rays6, tmax) reshaped to (na, nb) is Device.any_hit_pairs(a, b, t0, t1), bit for bit."""
    a, b, pp = _pair_args(a, b, t0, t1)
    na, nb = a.shape[0], b.shape[0]
    rays = np.zeros((na * nb, 6))
    tmax = C.c_double(pp.t1 - pp.t0)
    check(lib().mcpt_pair_rays(_p(a, C.c_double), na, _p(b, C.c_double), nb, C.byref(pp), _p(rays, C.c_double), C.byref(tmax)))
    return rays, tmax.value


LIGHT_POINT, LIGHT_SPOT, LIGHT_DIRECTIONAL, LIGHT_RECT = 0, 1, 2, 3
LIGHT_TWO_SIDED = 1


def _vec3(v, name):
    v = np.asarray(v, dtype=np.float64)
    if v.shape != (3,):
        raise ValueError("%s must have 3 components" % name)
    return (C.c_double * 3)(*v.tolist())


def _light(type_, flags=0, position=(0, 0, 0), direction=(0, 0, 0), u=(0, 0, 0), v=(0, 0, 0), color=(1, 1, 1), cos_inner=0.0, cos_outer=0.0, range=0.0):
    return DirectLight(int(type_), int(flags), _vec3(position, "position"), _vec3(direction, "direction"), _vec3(u, "u"), _vec3(v, "v"),
                       _vec3(color, "color"), float(cos_inner), float(cos_outer), float(range))


def point_light(position, color, range=0.0):
    """A point light for Device.direct_light (mcpt_direct_light, MCPT_LIGHT_POINT): color is its intensity, the irradiance it sends to a
    surface that faces it at distance 1; range > 0 cuts it off beyond that distance."""
    return _light(LIGHT_POINT, position=position, color=color, range=range)


def spot_light(position, direction, color, inner_degrees, outer_degrees, range=0.0):
    """A spot light (MCPT_LIGHT_SPOT): a point light that shines along `direction`, in full within inner_degrees of it and not at all
    beyond outer_degrees, a smoothstep of the cosine between them.  The half-angles become the record's cosines here."""
    return _light(LIGHT_SPOT, position=position, direction=direction, color=color, cos_inner=math.cos(math.radians(float(inner_degrees))),
                  cos_outer=math.cos(math.radians(float(outer_degrees))), range=range)


def directional_light(direction, color):
    """A directional light (MCPT_LIGHT_DIRECTIONAL): `direction` is the way the light travels, color the irradiance on a surface that
    faces it."""
    return _light(LIGHT_DIRECTIONAL, direction=direction, color=color)


def rect_light(corner, u, v, color, two_sided=False):
    """A rectangle light (MCPT_LIGHT_RECT): the parallelogram corner + s u + t v, 0 <= s, t <= 1, of emitted radiance `color`, shining
    toward cross(u, v) -- the library's cross -- or, two_sided, both ways."""
    return _light(LIGHT_RECT, flags=LIGHT_TWO_SIDED if two_sided else 0, position=corner, u=u, v=v, color=color)


def _lights(lights):
    """a sequence of DirectLight records as one contiguous ctypes array (None for an empty one) and its length"""
    lights = list(lights)
    for L in lights:
        if not isinstance(L, DirectLight):
            raise ValueError("lights must be DirectLight records (point_light, spot_light, directional_light, rect_light)")
    return ((DirectLight * len(lights))(*lights) if lights else None), len(lights)


def _direct_params(spp, bias, seed, sample_base):
    for name, v in (("spp", spp), ("sample_base", sample_base)):
        if not isinstance(v, numbers.Integral) or not -2 ** 31 <= v < 2 ** 31:
            raise ValueError("%s must be a 32-bit integer" % name)
    return DirectParams(int(spp), int(sample_base), int(seed), float(bias), 0, (C.c_int32 * 3)(0, 0, 0))


def direct_slots(lights, spp=1):
    """R, the shadow-ray slots of one receiver under `lights` (mcpt_direct_slots; no device): 1 per point, spot or directional light,
    spp per rectangle."""
    arr, nl = _lights(lights)
    if not isinstance(spp, numbers.Integral) or not -2 ** 31 <= spp < 2 ** 31:
        raise ValueError("spp must be a 32-bit integer")
    R = lib().mcpt_direct_slots(arr, nl, int(spp))
    if R < 0:
        check(int(R))
    return int(R)


def direct_fold_host(lights, g, occluded, n, spp=1):
    """The direct-light fold alone, on the CPU (mcpt_direct_fold_host; no device): g [n * R] the slots' factors as Device.direct_rays
    writes them (+0.0: a skipped slot) and occluded [n * R] their shadow rays' answers (Device.any_hit of those rays and limits).
    Returns what Device.direct_light returns, bit for bit."""
    arr, nl = _lights(lights)
    dp = _direct_params(spp, 0.0, 0, 0)
    R = direct_slots(lights, spp)
    n = int(n)
    g = np.ascontiguousarray(g, dtype=np.float64)
    occ = np.ascontiguousarray(np.asarray(occluded) != 0, dtype=np.uint8)
    if g.shape != (n * R,) or occ.shape != (n * R,):
        raise ValueError("g and occluded must have shape (%d,)" % (n * R))
    E, err, pl, vis = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, nl, 3)), np.zeros((n, nl))
    check(lib().mcpt_direct_fold_host(arr, nl, C.byref(dp), _p(g, C.c_double), _p(occ, C.c_uint8), n, _p(E, C.c_double), _p(err, C.c_double),
                                      _p(pl, C.c_double), _p(vis, C.c_double)))
    return {"irradiance": E, "stderr": err, "per_light": pl, "visibility": vis}


def _adaptive_params(rel_target, abs_target, min_spp):
    """mcpt_adaptive_params of the adaptive query calls: the targets as floats, min_spp a 32-bit integer (the library judges their values)"""
    if not isinstance(min_spp, numbers.Integral) or not -2 ** 31 <= min_spp < 2 ** 31:
        raise ValueError("min_spp must be a 32-bit integer")
    return AdaptiveParams(float(rel_target), float(abs_target), int(min_spp), 0)


def query_pass_boundaries(spp, min_spp):
    """The pass boundaries of an adaptive query call (mcpt_query_pass_boundaries): b_0 = min(min_spp, spp), doubling up to spp itself.
    Returns them as an int32 array; no device is needed."""
    for name, v in (("spp", spp), ("min_spp", min_spp)):
        if not isinstance(v, numbers.Integral) or not -2 ** 31 <= v < 2 ** 31:
            raise ValueError("%s must be a 32-bit integer" % name)
    n = lib().mcpt_query_pass_boundaries(int(spp), int(min_spp), None, 0)
    if n < 0:
        check(n)
    b = np.zeros(n, dtype=np.int32)
    got = lib().mcpt_query_pass_boundaries(int(spp), int(min_spp), _p(b, C.c_int32), n)
    if got < 0:
        check(got)
    return b


def _chart(uv, num_faces=None):
    """a UV chart as (num_faces, 6) float64 = (au, av, bu, bv, cu, cv) per face in .obj order"""
    uv = np.ascontiguousarray(uv, dtype=np.float64)
    if uv.ndim != 2 or uv.shape[1] != 6 or (num_faces is not None and uv.shape[0] != num_faces):
        raise ValueError("a chart must have shape (%s, 6), not %r" % ("num_faces" if num_faces is None else num_faces, uv.shape))
    return uv


def _map_size(width, height):
    for name, v in (("width", width), ("height", height)):
        if not isinstance(v, numbers.Integral) or not -2 ** 31 <= v < 2 ** 31:
            raise ValueError("%s must be a 32-bit integer" % name)
    return int(width), int(height)


def lightmap_raster(uv, width, height):
    """Coverage of a width x height lightmap by a UV chart, on the CPU (mcpt_lightmap_raster_host; no device, no scene): uv (num_faces, 6)
    -> owner [height, width] int32, the lowest face whose chart triangle covers the texel's centre, or -1."""
    uv = _chart(uv)
    width, height = _map_size(width, height)
    owner = np.zeros((max(height, 0), max(width, 0)), dtype=np.int32)
    check(lib().mcpt_lightmap_raster_host(_p(uv, C.c_double), uv.shape[0], width, height, _p(owner, C.c_int32)))
    return owner


def grid_atlas(num_faces, width, height, pad=1):
    """A trivial chart for a scene that has none, so that it can be baked: the map is cut into C x C square cells of s = min(width, height)
    // C texels, C = ceil(sqrt(num_faces)); face f gets the cell at column f % C, row f // C, and its corners in texel units are
    (x0 + pad, y0 + pad), (x0 + s - pad, y0 + pad), (x0 + pad, y0 + s - pad), divided by (width, height).  Not an unwrapper: every face
    is a right triangle in its own cell, whatever its shape.  ValueError when s < 2 * pad + 2.  Returns (num_faces, 6)."""
    num_faces, pad = int(num_faces), int(pad)
    if num_faces < 1 or pad < 0:
        raise ValueError("grid_atlas needs at least one face and pad >= 0")
    cells = math.isqrt(num_faces - 1) + 1                       # ceil(sqrt(num_faces)), in integers
    s = min(int(width), int(height)) // cells
    if s < 2 * pad + 2:
        raise ValueError("a %d x %d map gives %d faces cells of %d texels: at least %d are needed" % (width, height, num_faces, s, 2 * pad + 2))
    f = np.arange(num_faces)
    x0, y0 = (f % cells) * s, (f // cells) * s
    uv = np.stack([x0 + pad, y0 + pad, x0 + s - pad, y0 + pad, x0 + pad, y0 + s - pad], axis=1).astype(np.float64)
    uv[:, 0::2] /= float(width)
    uv[:, 1::2] /= float(height)
    return uv


def _as_lens(lens):
    if lens is None or isinstance(lens, Lens):
        return lens
    return make_lens(**lens)


def build_id():
    """hash of the sources libmcpt.so was compiled from (profiles/ files are stamped with it)"""
    return lib().mcpt_build_id().decode()


def hip_runtime_path():
    """which libamdhip64 this process has mapped (the torch wheel bundles a copy with the same soname: whichever is loaded first is
    the one libmcpt.so runs on)"""
    lib()
    found = []
    try:
        for ln in open("/proc/self/maps"):
            if "libamdhip64" in ln:
                f = ln.split()[-1]
                if f not in found:
                    found.append(f)
    except OSError:
        pass
    return ", ".join(found) if found else "unknown"


def hip_runtime_info():
    """(HIP_VERSION libmcpt.so was compiled against, the loaded runtime's version, the file that runtime came from)"""
    comp, run = C.c_int32(0), C.c_int32(0)
    path = C.create_string_buffer(512)
    check(lib().mcpt_hip_runtime_info(C.byref(comp), C.byref(run), path, 512))
    return comp.value, run.value, path.value.decode(errors="replace")


def hip_runtime_check(compiled, runtime, runtime_path=""):
    """the comparison mcpt_device_create makes (pure): (0 or MCPT_ERR_HIP, message)"""
    msg = C.create_string_buffer(1024)
    rc = lib().mcpt_hip_runtime_check(compiled, runtime, runtime_path.encode(), msg, 1024)
    return rc, msg.value.decode(errors="replace")


def allow_runtime_mismatch(allow=True):
    """explicit consent to run libmcpt.so's kernels on a HIP runtime of another release (a process that imported torch first)"""
    lib().mcpt_allow_runtime_mismatch(1 if allow else 0)


def device_count():
    return lib().mcpt_device_count()


LIGHTS_ALL, LIGHTS_ONE, LIGHTS_TREE = 0, 1, 2
# one node of the light tree of MCPT_LIGHTS_TREE (mcpt.h), 64 bytes; a leaf has left == right == ~light
LIGHT_NODE = np.dtype([("lo", "<f8", 3), ("hi", "<f8", 3), ("w", "<f8"), ("left", "<i4"), ("right", "<i4")])


def make_light_sampling(mode="all", weights=None):
    """An mcpt_light_sampling and the float64 weights it points to (keep both alive while it is used); (None, None) for "all" / None.
    mode: "all", "one", "tree", None, or a dict of these two arguments."""
    if isinstance(mode, dict):
        mode, weights = mode.get("mode", "one"), mode.get("weights")
    if mode is None or mode == "all":
        if weights is not None:
            raise ValueError('weights go with mode "one" or "tree"')
        return None, None
    if mode not in ("one", "tree"):
        raise ValueError('light sampling mode must be "all", "one" or "tree"')
    m = LIGHTS_TREE if mode == "tree" else LIGHTS_ONE
    if weights is None:
        return LightSampling(m, 0, None), None
    w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    return LightSampling(m, w.shape[0], _p(w, C.c_double)), w


class Scene:
    """scene_data::read_scene + Morton sort + BVH::BVH (MTPC/MTPC.cpp:38-45)."""

    def __init__(self, path, filename, width=None, height=None, load_flags=0):
        """load_flags: LOAD_STANDARD_OBJ | LOAD_MTLLIB | LOAD_MORTON_BOUNDS (opt-in; 0 = the reference's reader)."""
        self._h = C.c_void_p()
        check(lib().mcpt_scene_load_ex(path.encode(), filename.encode(), load_flags, C.byref(self._h)))
        if width is not None:
            self.set_resolution(width, height)

    @classmethod
    def from_arrays(cls, v, vn, material, material_rec, light_material, light_radiance, eye, look_at, up, fovy, width, height,
                    vt=None, material_names=None, defer_build=False):
        """scene_data from arrays (mcpt_scene_create): faces in .obj order, v/vn [n,9], vt [n,6] or None."""
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 9)
        vn = np.ascontiguousarray(vn, dtype=np.float64).reshape(-1, 9)
        n = v.shape[0]
        material = np.ascontiguousarray(material, dtype=np.int32)
        material_rec = np.ascontiguousarray(material_rec, dtype=np.float64).reshape(-1, 8)
        light_material = np.ascontiguousarray(light_material, dtype=np.int32)
        light_radiance = np.ascontiguousarray(light_radiance, dtype=np.float64).reshape(-1, 3)
        if vt is not None:
            vt = np.ascontiguousarray(vt, dtype=np.float64).reshape(-1, 6)
        d = SceneDesc()
        d.num_faces = n
        d.v, d.vn = _p(v, C.c_double), _p(vn, C.c_double)
        d.vt = _p(vt, C.c_double) if vt is not None else None
        d.material = _p(material, C.c_int32)
        d.num_materials = material_rec.shape[0]
        d.material_rec = _p(material_rec, C.c_double)
        if material_names is not None:
            arr = (C.c_char_p * len(material_names))(*[m.encode() for m in material_names])
            d.material_names = arr
        d.num_lights = light_material.shape[0]
        d.light_material = _p(light_material, C.c_int32)
        d.light_radiance = _p(light_radiance, C.c_double)
        d.eye = (C.c_double * 3)(*eye)
        d.look_at = (C.c_double * 3)(*look_at)
        d.up = (C.c_double * 3)(*up)
        d.fovy, d.width, d.height = fovy, width, height
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        check(lib().mcpt_scene_create(C.byref(d), SCENE_DEFER_BUILD if defer_build else 0, C.byref(self._h)))
        return self

    def close(self):
        if getattr(self, "_h", None):
            lib().mcpt_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown: module globals may already be gone
            pass

    def set_resolution(self, width, height):
        check(lib().mcpt_scene_set_resolution(self._h, width, height))

    @property
    def info(self):
        i = SceneInfo()
        check(lib().mcpt_scene_get_info(self._h, C.byref(i)))
        return i

    @property
    def width(self):
        return self.info.width

    @property
    def height(self):
        return self.info.height

    def faces(self):
        n = self.info.num_faces
        g = np.zeros((n, 27))
        m = np.zeros(n, dtype=np.int32)
        k = np.zeros(n, dtype=np.uint32)
        check(lib().mcpt_scene_get_faces(self._h, _p(g, C.c_double), _p(m, C.c_int32), _p(k, C.c_uint32)))
        return g, m, k

    def leaf_order(self):
        o = np.zeros(self.info.num_faces, dtype=np.int32)
        check(lib().mcpt_scene_get_leaf_order(self._h, _p(o, C.c_int32)))
        return o

    def bvh_nodes(self):
        nr = self.info.bvh.Nr
        box = np.zeros((nr, 6))
        lvl = np.zeros(nr, dtype=np.int32)
        leaf = np.zeros(nr, dtype=np.int32)
        check(lib().mcpt_scene_get_bvh_nodes(self._h, _p(box, C.c_double), _p(lvl, C.c_int32), _p(leaf, C.c_int32)))
        return box, lvl, leaf

    def find_index(self, i, l):
        return lib().mcpt_scene_find_index(self._h, i, l)

    def material(self, m):
        name = C.create_string_buffer(64)
        rec = np.zeros(8)
        fl = np.zeros(4, dtype=np.int32)
        check(lib().mcpt_scene_get_material(self._h, m, name, _p(rec, C.c_double), _p(fl, C.c_int32)))
        return name.value.decode(), rec, fl

    def light(self, i):
        name = C.create_string_buffer(64)
        rad = np.zeros(3)
        m = np.zeros(1, dtype=np.int32)
        a = np.zeros(1)
        check(lib().mcpt_scene_get_light(self._h, i, name, _p(rad, C.c_double), _p(m, C.c_int32), _p(a, C.c_double)))
        return name.value.decode(), rad, int(m[0]), float(a[0])

    def light_pick_table(self, weights=None):
        """The pick table of MCPT_LIGHTS_ONE for this scene's lights (mcpt_scene_light_pick_table; host only): the running sums cdf, the
        probabilities pdf and the factors 1.0 / pdf (0 for a light of weight 0) the kernels scale by.  weights: None (luminance x area) or
        one non-negative weight per light."""
        n = self.info.num_lights
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
            if w.shape[0] != n:
                raise ValueError("one weight per light of the scene")
        cdf, pdf = np.zeros(n), np.zeros(n)
        check(lib().mcpt_scene_light_pick_table(self._h, _p(w, C.c_double) if w is not None else None, _p(cdf, C.c_double), _p(pdf, C.c_double)))
        inv = np.zeros(n)
        np.divide(1.0, pdf, out=inv, where=pdf > 0)
        return cdf, pdf, inv

    def _light_weights(self, weights):
        if weights is None:
            return None
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if w.shape[0] != self.info.num_lights:
            raise ValueError("one weight per light of the scene")
        return w

    def light_tree(self, weights=None):
        """The light tree of MCPT_LIGHTS_TREE for this scene's lights, exactly as a device uploads it (mcpt_scene_light_tree; host only): a
        structured array of LIGHT_NODE records, root first.  weights: as light_pick_table."""
        w = self._light_weights(weights)
        wp = _p(w, C.c_double) if w is not None else None
        n = C.c_int32()
        check(lib().mcpt_scene_light_tree(self._h, wp, C.byref(n), None))
        nodes = np.zeros(n.value, dtype=LIGHT_NODE)
        check(lib().mcpt_scene_light_tree(self._h, wp, C.byref(n), nodes.ctypes.data_as(C.c_void_p)))
        return nodes

    def light_tree_pdf(self, p, pn, weights=None):
        """The probability with which MCPT_LIGHTS_TREE picks every light at the vertices p (n, 3) with normals pn (n, 3): (n, num_lights)
        (mcpt_scene_light_tree_pdf; host only, the device's arithmetic)."""
        w = self._light_weights(weights)
        p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
        pn = np.ascontiguousarray(pn, dtype=np.float64).reshape(-1, 3)
        if p.shape != pn.shape:
            raise ValueError("one normal per vertex")
        pdf = np.zeros((p.shape[0], self.info.num_lights))
        check(lib().mcpt_scene_light_tree_pdf(self._h, _p(w, C.c_double) if w is not None else None, _p(p, C.c_double), _p(pn, C.c_double),
                                              p.shape[0], _p(pdf, C.c_double)))
        return pdf

    def trace_engine(self):
        """'pool' or 'vote': the closest-hit engine a device created for this scene now would run (mcpt_scene_trace_engine)"""
        return "pool" if lib().mcpt_scene_trace_engine(self._h) == 1 else "vote"

    def fast_bvh_stats(self):
        n = np.zeros(1, dtype=np.int32)
        d = np.zeros(1, dtype=np.int32)
        ok = np.zeros(1, dtype=np.int32)
        order = np.zeros(self.info.num_faces, dtype=np.int32)
        check(lib().mcpt_scene_fast_bvh_stats(self._h, _p(n, C.c_int32), _p(d, C.c_int32), _p(order, C.c_int32), _p(ok, C.c_int32)))
        return int(n[0]), int(d[0]), order, bool(ok[0])

    def owned_pixels(self, rank=0, world=1, tile_w=0, tile_h=0):
        rp = RenderParams(1, 0, rank, world, tile_w, tile_h, 0)
        n = lib().mcpt_owned_pixels(self._h, C.byref(rp), None)
        if n < 0:
            check(int(n))
        out = np.zeros(n, dtype=np.int32)
        lib().mcpt_owned_pixels(self._h, C.byref(rp), _p(out, C.c_int32))
        return out


def _update_mode(mode):
    if mode in ("refit", UPDATE_REFIT):
        return UPDATE_REFIT
    if mode in ("rebuild", UPDATE_REBUILD):
        return UPDATE_REBUILD
    raise ValueError("mode must be 'refit' or 'rebuild'")


def _host_vertices(v, n_faces):
    """v as the [n_faces, 9] float64 array mcpt_device_update_vertices reads"""
    v = np.ascontiguousarray(v, dtype=np.float64)
    if v.size != n_faces * 9:
        raise ValueError("vertices: %d numbers given, the scene's %d faces need %d" % (v.size, n_faces, n_faces * 9))
    return v.reshape(n_faces, 9)


def _camera_args(eye, look_at, up):
    out = []
    for q in (eye, look_at, up):
        a = np.ascontiguousarray(q, dtype=np.float64).reshape(-1)
        if a.shape[0] != 3:
            raise ValueError("eye, look_at and up are 3-vectors")
        out.append(a)
    return out


def _shutter(shutter, steps):
    return Shutter(float(shutter[0]), float(shutter[1]), int(steps), 0)


def shutter_time(open, close, steps, j):
    """u_j of a shutter (mcpt_shutter_time; NaN for invalid arguments)"""
    return lib().mcpt_shutter_time(float(open), float(close), int(steps), int(j))


def shutter_step(spp, steps, k):
    """the step sample k of an spp-sample frame belongs to (mcpt_shutter_step; -1 for invalid arguments)"""
    return lib().mcpt_shutter_step(int(spp), int(steps), int(k))


class Device:
    """One MI355X holding a resident copy of a Scene."""

    def __init__(self, scene, ordinal=0, build=None):
        self.scene = scene
        self._h = C.c_void_p()
        if build is None:
            check(lib().mcpt_device_create(scene._h, ordinal, C.byref(self._h)))
        else:
            check(lib().mcpt_device_create_ex(scene._h, ordinal, build, C.byref(self._h)))
        i = scene.info
        self.width, self.height = i.width, i.height

    def close(self):
        if getattr(self, "_h", None):
            lib().mcpt_device_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # interpreter shutdown: module globals may already be gone
            pass

    def bvh_nodes(self):
        """(box6 [Nr,6], leaf_face [Nr]) read back from HBM."""
        nr = self.scene.info.bvh.Nr
        box = np.zeros((nr, 6))
        leaf = np.zeros(nr, dtype=np.int32)
        check(lib().mcpt_device_get_bvh_nodes(self._h, _p(box, C.c_double), _p(leaf, C.c_int32)))
        return box, leaf

    def leaf_order(self):
        o = np.zeros(self.scene.info.num_faces, dtype=np.int32)
        check(lib().mcpt_device_get_leaf_order(self._h, _p(o, C.c_int32)))
        return o

    def fast_hierarchy(self):
        """(FastInfo, nodes [n_nodes] uint8 records of 64 bytes, tri_faces [n_tris]): the culling hierarchy the fast walk walks, read
        back from HBM (mcpt_device_fast_hierarchy; tests/fast_bvh_ref.py decodes and checks it)."""
        info = FastInfo()
        check(lib().mcpt_device_fast_hierarchy(self._h, C.byref(info), None, None))
        nodes = np.zeros((info.n_nodes, 64), dtype=np.uint8)
        faces = np.zeros(info.n_tris, dtype=np.int32)
        check(lib().mcpt_device_fast_hierarchy(self._h, C.byref(info), nodes.ctypes.data_as(C.c_void_p), _p(faces, C.c_int32)))
        return info, nodes, faces

    def set_trace_mode(self, mode):
        """TRACE_FAST (default) or TRACE_REFERENCE: which walk answers closest-hit queries (same results)."""
        check(lib().mcpt_device_set_trace_mode(self._h, mode))

    def ray_intersect(self, rays, stats=None):
        """Batch of ray_intersect (MTPC/pathTracing.cpp:382): rays [n,6] -> face (.obj index or -1), t, p, pn."""
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        n = rays.shape[0]
        face = np.zeros(n, dtype=np.int32)
        t = np.zeros(n)
        p = np.zeros((n, 3))
        pn = np.zeros((n, 3))
        check(lib().mcpt_trace_closest(self._h, _p(rays, C.c_double), n, _p(face, C.c_int32), _p(t, C.c_double),
                                       _p(p, C.c_double), _p(pn, C.c_double), C.byref(stats) if stats is not None else None))
        return face, t, p, pn

    def generateImg(self, spp, seed=0, rank=0, world=1, tile_w=0, tile_h=0, flags=0, stats=None, img=None):
        """generateImg (MTPC/pathTracing.cpp:274): returns image::img as [H,W,3] float64."""
        if img is None:
            img = np.zeros((self.height, self.width, 3))
        rp = RenderParams(spp, seed, rank, world, tile_w, tile_h, flags)
        check(lib().mcpt_render(self._h, C.byref(rp), _p(img, C.c_double), C.byref(stats) if stats is not None else None))
        return img

    def render_device(self, d_img_ptr, spp, seed=0, rank=0, world=1, tile_w=0, tile_h=0, flags=0, stats=None, stream=None):
        """Same, into a caller-owned device buffer (e.g. a torch tensor's data_ptr()) on `stream`."""
        rp = RenderParams(spp, seed, rank, world, tile_w, tile_h, flags)
        check(lib().mcpt_render_device(self._h, C.byref(rp), C.c_void_p(d_img_ptr), C.byref(stats) if stats is not None else None,
                                       C.c_void_p(stream) if stream else None))

    def collect_stats(self, stats=None):
        """statistics of every RENDER_KEEP_STATS frame since the last call (waits for those frames)"""
        stats = stats if stats is not None else Stats()
        check(lib().mcpt_device_collect_stats(self._h, C.byref(stats)))
        return stats

    def sample_radiance(self, seed, pix, k):
        pix = np.ascontiguousarray(pix, dtype=np.int32)
        k = np.ascontiguousarray(k, dtype=np.int32)
        rgb = np.zeros((pix.shape[0], 3))
        check(lib().mcpt_sample_radiance(self._h, seed, _p(pix, C.c_int32), _p(k, C.c_int32), pix.shape[0], _p(rgb, C.c_double)))
        return rgb

    def set_lens(self, aperture=0.0, focus_distance=0.0, jitter=False, per_sample=False):
        """The camera lens of every later frame, sample_radiance, camera_rays and progressive handle created after it (mcpt_device_set_lens);
        no arguments: the reference's pinhole."""
        check(lib().mcpt_device_set_lens(self._h, C.byref(make_lens(aperture, focus_distance, jitter, per_sample))))

    def lens(self):
        """the device's lens as a dict of set_lens's arguments"""
        l = Lens()
        check(lib().mcpt_device_get_lens(self._h, C.byref(l)))
        return {"aperture": l.aperture, "focus_distance": l.focus_distance, "jitter": bool(l.flags & LENS_JITTER),
                "per_sample": bool(l.flags & LENS_PER_SAMPLE)}

    def camera_rays(self, seed, pix, k):
        """camera rays of samples (pix[i], k[i]) under the device's lens: (n, 6) = origin, direction"""
        pix = np.ascontiguousarray(pix, dtype=np.int32)
        k = np.ascontiguousarray(k, dtype=np.int32)
        rays = np.zeros((pix.shape[0], 6))
        check(lib().mcpt_camera_rays(self._h, seed, _p(pix, C.c_int32), _p(k, C.c_int32), pix.shape[0], _p(rays, C.c_double)))
        return rays

    @staticmethod
    def _query_list(q, ids, what="rays"):
        q = np.ascontiguousarray(q, dtype=np.float64)
        if q.ndim != 2 or q.shape[1] != 6:
            raise ValueError("%s must have shape (n, 6), not %r" % (what, q.shape))
        if ids is not None:
            ids = np.asarray(ids)
            if ids.dtype.kind not in "iu" or ids.shape != (q.shape[0],):
                raise ValueError("ids must be %d integers" % q.shape[0])
            if ids.size and (int(ids.min()) < -2 ** 31 or int(ids.max()) >= 2 ** 31):
                raise ValueError("ids must fit 32 bits")
            ids = np.ascontiguousarray(ids, dtype=np.int32)
        return q, ids

    def _query(self, q, ids, spp, seed, sample_base, kind, flags, stats):
        for name, v in (("spp", spp), ("sample_base", sample_base), ("flags", flags)):
            if not isinstance(v, numbers.Integral) or not -2 ** 31 <= v < 2 ** 31:
                raise ValueError("%s must be a 32-bit integer" % name)
        n = q.shape[0]
        mean, err, hits = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, dtype=np.int32)
        qp = QueryParams(int(spp), int(sample_base), int(seed), kind, int(flags), (C.c_int32 * 2)(0, 0))
        check(lib().mcpt_query_radiance(self._h, _p(q, C.c_double), _p(ids, C.c_int32), n, C.byref(qp), _p(mean, C.c_double),
                                        _p(err, C.c_double), _p(hits, C.c_int32), C.byref(stats) if stats is not None else None))
        return mean, err, hits

    def radiance(self, rays, spp, seed=0, ids=None, sample_base=0, flags=0, stats=None):
        """Path-traced radiance along the caller's rays (mcpt_query_radiance, MCPT_QUERY_RAY): rays (n, 6) = origin, unit direction;
        query i takes samples sample_base .. sample_base + spp - 1 under the RNG key (seed, ids[i] or i, sample).  Returns
        (mean [n,3], stderr [n,3], hits [n])."""
        q, ids = self._query_list(rays, ids)
        return self._query(q, ids, spp, seed, sample_base, QUERY_RAY, flags, stats)

    def irradiance(self, points, normals, spp, seed=0, ids=None, sample_base=0, flags=0, stats=None):
        """Irradiance at surface points (mcpt_query_radiance, MCPT_QUERY_HEMISPHERE): cosine-weighted directions about each normal, from
        0.01 off the point; E = pi * mean.  Returns (E [n,3], E_stderr [n,3], hits [n])."""
        points = np.asarray(points, dtype=np.float64)
        normals = np.asarray(normals, dtype=np.float64)
        if points.ndim != 2 or points.shape[1] != 3 or normals.shape != points.shape:
            raise ValueError("points and normals must both have shape (n, 3)")
        q, ids = self._query_list(np.concatenate([points, normals], axis=1), ids, "points and normals")
        mean, err, hits = self._query(q, ids, spp, seed, sample_base, QUERY_HEMISPHERE, flags, stats)
        return math.pi * mean, math.pi * err, hits

    def _query_adaptive(self, q, ids, spp, rel_target, abs_target, min_spp, seed, sample_base, kind, flags, stats):
        for name, v in (("spp", spp), ("sample_base", sample_base), ("flags", flags)):
            if not isinstance(v, numbers.Integral) or not -2 ** 31 <= v < 2 ** 31:
                raise ValueError("%s must be a 32-bit integer" % name)
        ap = _adaptive_params(rel_target, abs_target, min_spp)
        n = q.shape[0]
        mean, err = np.zeros((n, 3)), np.zeros((n, 3))
        hits, counts = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        qp = QueryParams(int(spp), int(sample_base), int(seed), kind, int(flags), (C.c_int32 * 2)(0, 0))
        check(lib().mcpt_query_radiance_adaptive(self._h, _p(q, C.c_double), _p(ids, C.c_int32), n, C.byref(qp), C.byref(ap), _p(mean, C.c_double),
                                                 _p(err, C.c_double), _p(hits, C.c_int32), _p(counts, C.c_int32),
                                                 C.byref(stats) if stats is not None else None))
        return mean, err, hits, counts

    def radiance_adaptive(self, rays, spp, rel_target, abs_target=0.0, min_spp=16, seed=0, ids=None, sample_base=0, flags=0, stats=None):
        """radiance() in passes (mcpt_query_radiance_adaptive): spp is the largest count a query may get; after each pass, whose boundaries
        double from min_spp (query_pass_boundaries), a query stops once its own error estimate meets the targets.  Query i is radiance()'s
        with spp = counts[i], bit for bit.  Returns (mean [n,3], stderr [n,3], hits [n], counts [n])."""
        q, ids = self._query_list(rays, ids)
        return self._query_adaptive(q, ids, spp, rel_target, abs_target, min_spp, seed, sample_base, QUERY_RAY, flags, stats)

    def irradiance_adaptive(self, points, normals, spp, rel_target, abs_target=0.0, min_spp=16, seed=0, ids=None, sample_base=0, flags=0, stats=None):
        """irradiance() in passes (mcpt_query_radiance_adaptive, MCPT_QUERY_HEMISPHERE); the targets apply to the query's mean, E / pi.
        Returns (E [n,3], E_stderr [n,3], hits [n], counts [n])."""
        points = np.asarray(points, dtype=np.float64)
        normals = np.asarray(normals, dtype=np.float64)
        if points.ndim != 2 or points.shape[1] != 3 or normals.shape != points.shape:
            raise ValueError("points and normals must both have shape (n, 3)")
        q, ids = self._query_list(np.concatenate([points, normals], axis=1), ids, "points and normals")
        mean, err, hits, counts = self._query_adaptive(q, ids, spp, rel_target, abs_target, min_spp, seed, sample_base, QUERY_HEMISPHERE, flags, stats)
        return math.pi * mean, math.pi * err, hits, counts

    def query_rays(self, q, seed, k, kind="ray", ids=None):
        """test seam (mcpt_query_rays): the ray of sample k[i] of query i, (n, 6) = origin, direction; kind is "ray" or "hemisphere" """
        if kind not in _QUERY_KINDS:
            raise ValueError('kind must be "ray" or "hemisphere"')
        q, ids = self._query_list(q, ids, "q")
        k = np.asarray(k)
        if k.dtype.kind not in "iu" or k.shape != (q.shape[0],):
            raise ValueError("k must be %d integers" % q.shape[0])
        k = np.ascontiguousarray(k, dtype=np.int32)
        rays = np.zeros((q.shape[0], 6))
        check(lib().mcpt_query_rays(self._h, _p(q, C.c_double), _p(ids, C.c_int32), q.shape[0], int(seed), _QUERY_KINDS[kind], _p(k, C.c_int32),
                                    _p(rays, C.c_double)))
        return rays

    @staticmethod
    def _probe_list(points, ids):
        p = np.ascontiguousarray(points, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError("points must have shape (n, 3), not %r" % (p.shape,))
        if ids is not None:
            ids = np.asarray(ids)
            if ids.dtype.kind not in "iu" or ids.shape != (p.shape[0],):
                raise ValueError("ids must be %d integers" % p.shape[0])
            if ids.size and (int(ids.min()) < -2 ** 31 or int(ids.max()) >= 2 ** 31):
                raise ValueError("ids must fit 32 bits")
            ids = np.ascontiguousarray(ids, dtype=np.int32)
        return p, ids

    def sh_probes(self, points, spp, seed=0, ids=None, sample_base=0, flags=0, stats=None):
        """Light probes (mcpt_query_sh): the incoming radiance of the whole sphere about each of points (n, 3), in free space, as nine
        spherical-harmonic coefficients per channel; probe i takes samples sample_base .. sample_base + spp - 1 under the RNG key
        (seed, ids[i] or i, sample).  Returns (sh [n,9,3], stderr [n,9,3], hits [n]); sh_radiance and sh_irradiance evaluate sh."""
        p, ids = self._probe_list(points, ids)
        for name, v in (("spp", spp), ("sample_base", sample_base), ("flags", flags)):
            if not isinstance(v, numbers.Integral) or not -2 ** 31 <= v < 2 ** 31:
                raise ValueError("%s must be a 32-bit integer" % name)
        n = p.shape[0]
        sh, err, hits = np.zeros((n, 9, 3)), np.zeros((n, 9, 3)), np.zeros(n, dtype=np.int32)
        sp = ShParams(int(spp), int(sample_base), int(seed), int(flags), (C.c_int32 * 3)(0, 0, 0))
        check(lib().mcpt_query_sh(self._h, _p(p, C.c_double), _p(ids, C.c_int32), n, C.byref(sp), _p(sh, C.c_double), _p(err, C.c_double),
                                  _p(hits, C.c_int32), C.byref(stats) if stats is not None else None))
        return sh, err, hits

    def sh_probe_rays(self, points, seed, k, ids=None):
        """test seam (mcpt_query_sh_rays): the ray of sample k[i] of probe i, (n, 6) = origin (the point itself), direction"""
        p, ids = self._probe_list(points, ids)
        k = np.asarray(k)
        if k.dtype.kind not in "iu" or k.shape != (p.shape[0],):
            raise ValueError("k must be %d integers" % p.shape[0])
        k = np.ascontiguousarray(k, dtype=np.int32)
        rays = np.zeros((p.shape[0], 6))
        check(lib().mcpt_query_sh_rays(self._h, _p(p, C.c_double), _p(ids, C.c_int32), p.shape[0], int(seed), _p(k, C.c_int32), _p(rays, C.c_double)))
        return rays

    def lightmap_texels(self, width, height, uv=None):
        """Coverage and texel list of a width x height lightmap on the device (mcpt_lightmap_texels): uv (num_faces, 6) or None for the
        scene's own vt.  Returns (owner [height, width], texels [n] ascending, q6 [n, 6] = position, normal of every covered texel)."""
        width, height = _map_size(width, height)
        uv = _chart(uv, self.scene.info.num_faces) if uv is not None else None
        owner = np.zeros((max(height, 0), max(width, 0)), dtype=np.int32)
        n = lib().mcpt_lightmap_texels(self._h, _p(uv, C.c_double), width, height, _p(owner, C.c_int32), None, None, 0)
        if n < 0:
            check(n)
        texels, q6 = np.zeros(n, dtype=np.int32), np.zeros((n, 6))
        if n > 0:
            got = lib().mcpt_lightmap_texels(self._h, _p(uv, C.c_double), width, height, None, _p(texels, C.c_int32), _p(q6, C.c_double), n)
            if got < 0:
                check(got)
        return owner, texels, q6

    def bake_lightmap(self, width, height, spp, uv=None, seed=0, sample_base=0, dilate=0, flags=0, stats=None):
        """A lightmap (mcpt_bake_lightmap): the irradiance at the surface points a chart maps its texels to -- uv (num_faces, 6), or None
        for the scene's own vt -- from spp hemisphere samples per covered texel, keyed (seed, texel index, sample); dilate rounds fill
        the gutters.  Returns (E [height, width, 3], E_stderr [height, width, 3], hits [height, width], owner [height, width]); owner is
        the face of a covered texel, -1 - r for a texel filled in round r, -1 otherwise."""
        width, height = _map_size(width, height)
        for name, v in (("spp", spp), ("sample_base", sample_base), ("flags", flags), ("dilate", dilate)):
            if not isinstance(v, numbers.Integral) or not -2 ** 31 <= v < 2 ** 31:
                raise ValueError("%s must be a 32-bit integer" % name)
        uv = _chart(uv, self.scene.info.num_faces) if uv is not None else None
        shape = (max(height, 0), max(width, 0))
        E, err = np.zeros(shape + (3,)), np.zeros(shape + (3,))
        hits, owner = np.zeros(shape, dtype=np.int32), np.zeros(shape, dtype=np.int32)
        lp = LightmapParams(width, height, int(spp), int(sample_base), int(seed), int(flags), int(dilate), (C.c_int32 * 2)(0, 0))
        check(lib().mcpt_bake_lightmap(self._h, _p(uv, C.c_double), C.byref(lp), _p(E, C.c_double), _p(err, C.c_double), _p(hits, C.c_int32),
                                       _p(owner, C.c_int32), C.byref(stats) if stats is not None else None))
        return E, err, hits, owner

    def bake_lightmap_adaptive(self, width, height, spp, rel_target, abs_target=0.0, min_spp=16, uv=None, seed=0, sample_base=0, dilate=0, flags=0,
                               stats=None):
        """bake_lightmap() whose texels stop on their own error estimate (mcpt_bake_lightmap_adaptive): the adaptive hemisphere query of
        the map's own texel list; spp is the largest count a texel may get and the targets apply to E / pi.  Returns (E, E_stderr, hits,
        owner, counts), each [height, width(, 3)]; counts is 0 where a texel is not covered or was only dilated."""
        width, height = _map_size(width, height)
        for name, v in (("spp", spp), ("sample_base", sample_base), ("flags", flags), ("dilate", dilate)):
            if not isinstance(v, numbers.Integral) or not -2 ** 31 <= v < 2 ** 31:
                raise ValueError("%s must be a 32-bit integer" % name)
        ap = _adaptive_params(rel_target, abs_target, min_spp)
        uv = _chart(uv, self.scene.info.num_faces) if uv is not None else None
        shape = (max(height, 0), max(width, 0))
        E, err = np.zeros(shape + (3,)), np.zeros(shape + (3,))
        hits, owner, counts = np.zeros(shape, dtype=np.int32), np.zeros(shape, dtype=np.int32), np.zeros(shape, dtype=np.int32)
        lp = LightmapParams(width, height, int(spp), int(sample_base), int(seed), int(flags), int(dilate), (C.c_int32 * 2)(0, 0))
        check(lib().mcpt_bake_lightmap_adaptive(self._h, _p(uv, C.c_double), C.byref(lp), C.byref(ap), _p(E, C.c_double), _p(err, C.c_double),
                                                _p(hits, C.c_int32), _p(owner, C.c_int32), _p(counts, C.c_int32),
                                                C.byref(stats) if stats is not None else None))
        return E, err, hits, owner, counts

    def denoise_lightmap(self, E, E_stderr, uv=None, iterations=LIGHTMAP_DENOISE_ITERATIONS, sigma_l=0.0, sigma_p=0.0, dilate=0):
        """A lightmap denoised (mcpt_lightmap_denoise): an edge-avoiding a-trous filter in UV space over the texels the chart covers -- uv
        (num_faces, 6), or None for the scene's own vt -- guided by every texel's world position, normal and footprint and by E_stderr;
        the size is E's, [height, width, 3].  iterations 0 .. 10 (0: no filtering), a sigma of 0 is its default, dilate rounds fill the
        gutters afterwards.  Returns (E_denoised [height, width, 3], owner [height, width]).  The result is biased towards the neighbours'
        values; a map whose E_stderr is 0 (spp = 1) comes back essentially unfiltered.  Bake the map passed here with dilate=0: the
        denoiser dilates after it filters, from the filtered texels, and never reads a texel that is not covered -- values an earlier
        dilation put there would only be overwritten."""
        E = np.ascontiguousarray(E, dtype=np.float64)
        E_stderr = np.ascontiguousarray(E_stderr, dtype=np.float64)
        if E.ndim != 3 or E.shape[2] != 3 or E_stderr.shape != E.shape:
            raise ValueError("E and E_stderr must both have shape (height, width, 3), not %r and %r" % (E.shape, E_stderr.shape))
        for name, v in (("iterations", iterations), ("dilate", dilate)):
            if not isinstance(v, numbers.Integral) or not -2 ** 31 <= v < 2 ** 31:
                raise ValueError("%s must be a 32-bit integer" % name)
        height, width = E.shape[:2]
        uv = _chart(uv, self.scene.info.num_faces) if uv is not None else None
        out, owner = np.zeros((height, width, 3)), np.zeros((height, width), dtype=np.int32)
        dp = LightmapDenoiseParams(width, height, int(iterations), int(dilate), float(sigma_l), float(sigma_p), (C.c_int32 * 2)(0, 0))
        check(lib().mcpt_lightmap_denoise(self._h, _p(uv, C.c_double), C.byref(dp), _p(E, C.c_double), _p(E_stderr, C.c_double),
                                          _p(out, C.c_double), _p(owner, C.c_int32)))
        return out, owner

    def bake_volume(self, grid, spp, seed=0, sample_base=0, flags=0, stats=None):
        """An irradiance volume (mcpt_bake_volume): sh_probes() of volume_points(grid), bit for bit, with the positions made on the GPU;
        probe P's RNG key id is P.  Returns (sh [nz, ny, nx, 9, 3], stderr [nz, ny, nx, 9, 3], hits [nz, ny, nx]); volume_irradiance
        looks the coefficients up."""
        for name, v in (("spp", spp), ("sample_base", sample_base), ("flags", flags)):
            if not isinstance(v, numbers.Integral) or not -2 ** 31 <= v < 2 ** 31:
                raise ValueError("%s must be a 32-bit integer" % name)
        shape = (max(grid.nz, 0), max(grid.ny, 0), max(grid.nx, 0)) if _grid_probes(grid) else (0, 0, 0)
        sh, err, hits = np.zeros(shape + (9, 3)), np.zeros(shape + (9, 3)), np.zeros(shape, dtype=np.int32)
        sp = ShParams(int(spp), int(sample_base), int(seed), int(flags), (C.c_int32 * 3)(0, 0, 0))
        check(lib().mcpt_bake_volume(self._h, C.byref(grid), C.byref(sp), _p(sh, C.c_double), _p(err, C.c_double), _p(hits, C.c_int32),
                                     C.byref(stats) if stats is not None else None))
        return sh, err, hits

    def volume_irradiance(self, grid, sh, points, normals, valid=None):
        """The irradiance volume's lookup on the GPU (mcpt_volume_irradiance): volume_irradiance_host's arguments and answers, bit for
        bit.  Returns (E [n, 3], corners [n])."""
        sh, q, valid = _volume_args(grid, sh, points, normals, valid)
        n = q.shape[0]
        E, corners = np.zeros((n, 3)), np.zeros(n, dtype=np.int32)
        check(lib().mcpt_volume_irradiance(self._h, C.byref(grid), _p(sh, C.c_double), _p(valid, C.c_uint8), _p(q, C.c_double), n,
                                           _p(E, C.c_double), _p(corners, C.c_int32)))
        return E, corners

    def probe_visibility(self, points, spp, res=8, max_distance=1.0, max_back_fraction=0.25, seed=0, ids=None, sample_base=0, workspace_rays=0,
                         stats=None):
        """What each of points (n, 3) sees (mcpt_query_visibility): the rays sh_probes() traces for the same seed, ids and sample range,
        folded into a res x res octahedral map of the mean and mean square of the distance to the nearest surface, clamped at
        max_distance, and into the count of hits from behind.  Returns (moments [n, res * res, 2] -- a bin without samples holds
        (-1, 0) --, hits [n], back [n], valid [n]); valid is 0 where more than max_back_fraction of the spp rays hit a back face: the
        probe sits inside geometry.  workspace_rays bounds the rays in flight (0: the library's default); it does not change the result."""
        p, ids = self._probe_list(points, ids)
        vp = _visibility_params(spp, res, max_distance, max_back_fraction, seed, sample_base, workspace_rays)
        n, bins = p.shape[0], int(res) ** 2 if 1 <= res <= 16 else 0      # (the library refuses any other res)
        moments, hits, back = np.zeros((n, bins, 2)), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        valid = np.zeros(n, dtype=np.uint8)
        check(lib().mcpt_query_visibility(self._h, _p(p, C.c_double), _p(ids, C.c_int32), n, C.byref(vp), _p(moments, C.c_double), _p(hits, C.c_int32),
                                          _p(back, C.c_int32), _p(valid, C.c_uint8), C.byref(stats) if stats is not None else None))
        return moments, hits, back, valid

    def bake_volume_visibility(self, grid, spp, res=8, max_distance=None, max_back_fraction=0.25, seed=0, sample_base=0, workspace_rays=0, stats=None):
        """probe_visibility() of volume_points(grid), bit for bit, with the positions made on the GPU (mcpt_bake_volume_visibility); probe
        P's RNG key id is P, so the rays are bake_volume()'s.  max_distance defaults to 1.5 x the cell diagonal.  Returns (moments
        [nz, ny, nx, res * res, 2], hits [nz, ny, nx], back [nz, ny, nx], valid [nz, ny, nx]): valid is volume_irradiance's mask, and
        volume_irradiance_visible takes the moments."""
        probes = _grid_probes(grid)
        if max_distance is None:
            max_distance = 1.5 * float(np.sqrt(sum(float(s) ** 2 for s in grid.spacing)))
        vp = _visibility_params(spp, res, max_distance, max_back_fraction, seed, sample_base, workspace_rays)
        shape = (max(grid.nz, 0), max(grid.ny, 0), max(grid.nx, 0)) if probes else (0, 0, 0)
        bins = int(res) ** 2 if 1 <= res <= 16 else 0
        moments, hits, back = np.zeros(shape + (bins, 2)), np.zeros(shape, dtype=np.int32), np.zeros(shape, dtype=np.int32)
        valid = np.zeros(shape, dtype=np.uint8)
        check(lib().mcpt_bake_volume_visibility(self._h, C.byref(grid), C.byref(vp), _p(moments, C.c_double), _p(hits, C.c_int32), _p(back, C.c_int32),
                                                _p(valid, C.c_uint8), C.byref(stats) if stats is not None else None))
        return moments, hits, back, valid

    def volume_irradiance_visible(self, grid, sh, moments, points, normals, vis, valid=None):
        """The visibility-weighted lookup on the GPU (mcpt_volume_irradiance_visible): volume_irradiance_visible_host's arguments and
        answers, bit for bit.  Returns (E [n, 3], corners [n])."""
        sh, q, valid = _volume_args(grid, sh, points, normals, valid)
        moments = _visibility_moments(grid, vis, moments)
        n = q.shape[0]
        E, corners = np.zeros((n, 3)), np.zeros(n, dtype=np.int32)
        check(lib().mcpt_volume_irradiance_visible(self._h, C.byref(grid), _p(sh, C.c_double), _p(moments, C.c_double), _p(valid, C.c_uint8), C.byref(vis),
                                                   _p(q, C.c_double), n, _p(E, C.c_double), _p(corners, C.c_int32)))
        return E, corners

    def occlusion(self, points, normals, spp, max_distance, falloff="hard", seed=0, ids=None, sample_base=0, workspace_rays=0, stats=None):
        """Ambient occlusion at surface points (mcpt_query_occlusion): the rays irradiance() traces for the same seed, ids and sample
        range, answered by their closest hit alone.  A hit nearer than max_distance closes its direction -- altogether ("hard"), or
        leaving t / max_distance ("linear") or its square ("square") open.  Returns a dict: ao [n] the open share of the cosine-weighted
        hemisphere, stderr [n], bent [n, 3] the unit mean open direction (the unit normal where nothing is open), hits [n] the near
        hits and back [n] those from behind a face.  workspace_rays bounds the rays in flight (0: the library's default); it does not
        change the result."""
        points = np.asarray(points, dtype=np.float64)
        normals = np.asarray(normals, dtype=np.float64)
        if points.ndim != 2 or points.shape[1] != 3 or normals.shape != points.shape:
            raise ValueError("points and normals must both have shape (n, 3)")
        q, ids = self._query_list(np.concatenate([points, normals], axis=1), ids, "points and normals")
        op = _occlusion_params(spp, max_distance, falloff, seed, sample_base, workspace_rays)
        n = q.shape[0]
        ao, err, bent = np.zeros(n), np.zeros(n), np.zeros((n, 3))
        hits, back = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        check(lib().mcpt_query_occlusion(self._h, _p(q, C.c_double), _p(ids, C.c_int32), n, C.byref(op), _p(ao, C.c_double), _p(err, C.c_double),
                                         _p(bent, C.c_double), _p(hits, C.c_int32), _p(back, C.c_int32), C.byref(stats) if stats is not None else None))
        return {"ao": ao, "stderr": err, "bent": bent, "hits": hits, "back": back}

    def bake_occlusion_lightmap(self, width, height, spp, max_distance, uv=None, falloff="hard", seed=0, sample_base=0, dilate=0, workspace_rays=0,
                                stats=None):
        """An occlusion map (mcpt_bake_occlusion_lightmap): occlusion() of lightmap_texels()' list with ids = texels, bit for bit, put
        back into the map; dilate rounds of the lightmap's rule fill the gutters of ao alone.  Returns a dict: ao [height, width],
        stderr [height, width], bent [height, width, 3], hits, back and owner [height, width]; owner is bake_lightmap()'s."""
        width, height = _map_size(width, height)
        if not isinstance(dilate, numbers.Integral) or not -2 ** 31 <= dilate < 2 ** 31:
            raise ValueError("dilate must be a 32-bit integer")
        op = _occlusion_params(spp, max_distance, falloff, seed, sample_base, workspace_rays)
        uv = _chart(uv, self.scene.info.num_faces) if uv is not None else None
        shape = (max(height, 0), max(width, 0))
        ao, err, bent = np.zeros(shape), np.zeros(shape), np.zeros(shape + (3,))
        hits, back, owner = np.zeros(shape, dtype=np.int32), np.zeros(shape, dtype=np.int32), np.zeros(shape, dtype=np.int32)
        om = OcclusionMap(width, height, int(dilate), 0)
        check(lib().mcpt_bake_occlusion_lightmap(self._h, _p(uv, C.c_double), C.byref(om), C.byref(op), _p(ao, C.c_double), _p(err, C.c_double),
                                                 _p(bent, C.c_double), _p(hits, C.c_int32), _p(back, C.c_int32), _p(owner, C.c_int32),
                                                 C.byref(stats) if stats is not None else None))
        return {"ao": ao, "stderr": err, "bent": bent, "hits": hits, "back": back, "owner": owner}

    def any_hit(self, rays, tmax=None, stats=None):
        """Is anything in the way of each ray before its limit (mcpt_trace_any): rays [n, 6] as ray_intersect() takes them, tmax [n] in
        each ray's own parameter, one number for all of them, or None for +inf ("does the ray hit anything").  Ray i is occluded iff
        ray_intersect() answers face >= 0 and t < tmax[i] for it -- exactly; a NaN or non-positive limit is never occluded -- but the
        walk stops at the first blocker and one byte per ray comes back.  Returns bool [n]."""
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        n = rays.shape[0]
        if tmax is not None:
            tmax = np.asarray(tmax, dtype=np.float64)
            if tmax.ndim == 0:
                tmax = np.full(n, float(tmax))
            tmax = np.ascontiguousarray(tmax)
            if tmax.shape != (n,):
                raise ValueError("tmax must be a number or have shape (%d,)" % n)
        occ = np.zeros(n, dtype=np.uint8)
        check(lib().mcpt_trace_any(self._h, _p(rays, C.c_double), _p(tmax, C.c_double), n, _p(occ, C.c_uint8),
                                   C.byref(stats) if stats is not None else None))
        return occ != 0

    def any_hit_pairs(self, a, b, t0=0.0, t1=1.0, packed=False, stats=None):
        """Point-pair visibility (mcpt_trace_any_pairs): for points a (na, 3) and b (nb, 3), is anything in the way of the part
        [t0, t1] of the segment a_i -> b_j -- any_hit() of pair_rays(a, b, t0, t1), bit for bit, with the rays formed on the GPU and one
        bit per pair coming back.  Points on surfaces want, for example, t0 = 1e-4 and t1 = 1 - 1e-4, so that neither point's own
        surface blocks.  Returns bool [na, nb], True where occluded; packed: the uint64 words [na, (nb + 63) // 64] as they are, pair
        (i, j) in bit j & 63 of word [i, j >> 6], padding bits 0."""
        a, b, pp = _pair_args(a, b, t0, t1)
        na, nb = a.shape[0], b.shape[0]
        W = (nb + 63) // 64
        bits = np.zeros((na, W), dtype=np.uint64)
        check(lib().mcpt_trace_any_pairs(self._h, _p(a, C.c_double), na, _p(b, C.c_double), nb, C.byref(pp), _p(bits, C.c_uint64),
                                         C.byref(stats) if stats is not None else None))
        if packed:
            return bits
        if na == 0 or nb == 0:
            return np.zeros((na, nb), dtype=bool)
        return np.unpackbits(bits.view(np.uint8).reshape(na, W * 8), axis=1, bitorder="little")[:, :nb].astype(bool)

    def any_hit_device(self, d_rays_ptr, n, d_occluded_ptr, d_tmax_ptr=None, stream=None):
        """any_hit() between caller-owned device buffers (e.g. torch tensors' data_ptr()) on `stream` (mcpt_trace_any_device): rays
        [n, 6] float64, tmax [n] float64 or None, occluded [n] uint8."""
        check(lib().mcpt_trace_any_device(self._h, _dp(d_rays_ptr), _dp(d_tmax_ptr), int(n), _dp(d_occluded_ptr), _dp(stream)))

    def any_hit_pairs_device(self, d_a_ptr, na, d_b_ptr, nb, d_bits_ptr, t0=0.0, t1=1.0, stream=None):
        """any_hit_pairs(packed=True) between caller-owned device buffers on `stream` (mcpt_trace_any_pairs_device): a [na, 3] and
        b [nb, 3] float64, bits [na, (nb + 63) // 64] uint64."""
        pp = PairParams(float(t0), float(t1), 0, 0)
        check(lib().mcpt_trace_any_pairs_device(self._h, _dp(d_a_ptr), int(na), _dp(d_b_ptr), int(nb), C.byref(pp), _dp(d_bits_ptr), _dp(stream)))

    def _direct_list(self, points, normals, ids):
        points = np.asarray(points, dtype=np.float64)
        normals = np.asarray(normals, dtype=np.float64)
        if points.ndim != 2 or points.shape[1] != 3 or normals.shape != points.shape:
            raise ValueError("points and normals must both have shape (n, 3)")
        return self._query_list(np.concatenate([points, normals], axis=1), ids, "points and normals")

    def direct_light(self, points, normals, lights, spp=1, bias=0.01, seed=0, ids=None, sample_base=0, stats=None):
        """Direct light from the caller's own lights at surface points (mcpt_query_direct): `lights` is a sequence of point_light,
        spot_light, directional_light and rect_light records; every shadow ray is formed and walked on the GPU and leaves the point by
        `bias` along itself; a rectangle takes spp samples, drawn from (seed, id, sample_base + j), the other lights one.  Returns a
        dict: irradiance [n, 3], stderr [n, 3] (the rectangles' sampling error), per_light [n, nl, 3] and visibility [n, nl], the share
        of a light's shadow rays that reached it (0 where none was shot) -- direct_fold_host() of any_hit() of direct_rays(), bit for
        bit."""
        q, ids = self._direct_list(points, normals, ids)
        arr, nl = _lights(lights)
        dp = _direct_params(spp, bias, seed, sample_base)
        n = q.shape[0]
        E, err, pl, vis = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, nl, 3)), np.zeros((n, nl))
        check(lib().mcpt_query_direct(self._h, _p(q, C.c_double), _p(ids, C.c_int32), n, arr, nl, C.byref(dp), _p(E, C.c_double), _p(err, C.c_double),
                                      _p(pl, C.c_double), _p(vis, C.c_double), C.byref(stats) if stats is not None else None))
        return {"irradiance": E, "stderr": err, "per_light": pl, "visibility": vis}

    def direct_rays(self, points, normals, lights, spp=1, bias=0.01, seed=0, ids=None, sample_base=0):
        """The shadow rays direct_light() forms, written out (mcpt_direct_rays, the test seam): per entry R = direct_slots(lights, spp)
        slots, the lights in order and a rectangle's samples in order.  Returns (rays [n * R, 6], tmax [n * R], g [n * R]); a skipped
        slot has a zero direction, tmax 0 and g +0.0."""
        q, ids = self._direct_list(points, normals, ids)
        arr, nl = _lights(lights)
        dp = _direct_params(spp, bias, seed, sample_base)
        n = q.shape[0]
        m = n * direct_slots(lights, spp)
        rays, tmax, g = np.zeros((m, 6)), np.zeros(m), np.zeros(m)
        check(lib().mcpt_direct_rays(self._h, _p(q, C.c_double), _p(ids, C.c_int32), n, arr, nl, C.byref(dp), _p(rays, C.c_double), _p(tmax, C.c_double),
                                     _p(g, C.c_double)))
        return rays, tmax, g

    def bake_direct_lightmap(self, width, height, lights, spp=1, uv=None, bias=0.01, seed=0, sample_base=0, dilate=0, stats=None):
        """A direct lightmap (mcpt_bake_direct_lightmap): direct_light() of lightmap_texels()' list with ids = texels, bit for bit, put
        back into the map; dilate rounds of the lightmap's rule fill the gutters of the irradiance alone.  Returns a dict: irradiance and
        stderr [height, width, 3], per_light [height, width, nl, 3], visibility [height, width, nl] and owner [height, width], which is
        bake_lightmap()'s."""
        width, height = _map_size(width, height)
        if not isinstance(dilate, numbers.Integral) or not -2 ** 31 <= dilate < 2 ** 31:
            raise ValueError("dilate must be a 32-bit integer")
        arr, nl = _lights(lights)
        dp = _direct_params(spp, bias, seed, sample_base)
        uv = _chart(uv, self.scene.info.num_faces) if uv is not None else None
        shape = (max(height, 0), max(width, 0))
        E, err, pl, vis = np.zeros(shape + (3,)), np.zeros(shape + (3,)), np.zeros(shape + (nl, 3)), np.zeros(shape + (nl,))
        owner = np.zeros(shape, dtype=np.int32)
        dm = DirectMap(width, height, int(dilate), 0)
        check(lib().mcpt_bake_direct_lightmap(self._h, _p(uv, C.c_double), C.byref(dm), arr, nl, C.byref(dp), _p(E, C.c_double), _p(err, C.c_double),
                                              _p(pl, C.c_double), _p(vis, C.c_double), _p(owner, C.c_int32),
                                              C.byref(stats) if stats is not None else None))
        return {"irradiance": E, "stderr": err, "per_light": pl, "visibility": vis, "owner": owner}

    def lightmap_irradiance(self, E, uv, owner=None):
        """A lightmap's lookup by chart coordinate on the GPU (mcpt_lightmap_irradiance): lightmap_irradiance_host's arguments and
        answers, bit for bit.  Returns (e [n, 3], taps [n])."""
        E, uv, owner = _lightmap_args(E, uv, owner)
        n = uv.shape[0]
        e, taps = np.zeros((n, 3)), np.zeros(n, dtype=np.int32)
        check(lib().mcpt_lightmap_irradiance(self._h, E.shape[1], E.shape[0], _p(E, C.c_double), _p(owner, C.c_int32), _p(uv, C.c_double), n,
                                             _p(e, C.c_double), _p(taps, C.c_int32)))
        return e, taps

    def lightmap_irradiance_device(self, width, height, d_E_ptr, d_uv_ptr, n, d_e_ptr, d_owner_ptr=None, d_taps_ptr=None, stream=None):
        """The same between caller-owned device buffers (e.g. torch tensors' data_ptr()) on `stream` (mcpt_lightmap_irradiance_device)."""
        check(lib().mcpt_lightmap_irradiance_device(self._h, int(width), int(height), _dp(d_E_ptr), _dp(d_owner_ptr),
                                                    _dp(d_uv_ptr), int(n), _dp(d_e_ptr), _dp(d_taps_ptr),
                                                    _dp(stream)))

    def _baked_source(self, source):
        if not isinstance(source, _Baked):
            raise ValueError("source must come from baked_volume or baked_lightmap")
        if source.kind == BAKED_LIGHTMAP and source.uv is not None:
            _chart(source.uv, self.scene.info.num_faces)
        return source.struct()

    def baked_radiance(self, rays, source, face_viewer=False, lighting_only=False, stats=None):
        """What the caller's rays (n, 6) = origin, direction see of a bake (mcpt_baked_radiance): every ray's closest hit, lit by `source`
        (baked_volume or baked_lightmap) as L = kd * E / pi; a miss shows the environment, an emitter its radiance.  face_viewer turns the
        shading normal towards the ray's origin; lighting_only leaves kd out.  Returns a dict: radiance [n, 3], kind [n] (BAKED_MISS,
        BAKED_EMITTER, BAKED_SURFACE), face [n] (.obj index, -1: a miss), q6 [n, 6] (hit point and the normal that went into the lookup),
        uv [n, 2] (the chart coordinate, lightmap sources), kd [n, 3], e [n, 3] (the irradiance looked up) and lit [n] (the corners or taps
        that took part).  Everything but radiance, kind and face is 0 where a ray is not a surface hit."""
        rays = np.ascontiguousarray(rays, dtype=np.float64)
        if rays.ndim != 2 or rays.shape[1] != 6:
            raise ValueError("rays must have shape (n, 6), not %r" % (rays.shape,))
        n = rays.shape[0]
        s = self._baked_source(source)
        out = {"radiance": np.zeros((n, 3)), "kind": np.zeros(n, dtype=np.int32), "face": np.zeros(n, dtype=np.int32), "q6": np.zeros((n, 6)),
               "uv": np.zeros((n, 2)), "kd": np.zeros((n, 3)), "e": np.zeros((n, 3)), "lit": np.zeros(n, dtype=np.int32)}
        o = BakedOutputs(*[out[k].ctypes.data for k in ("radiance", "kind", "face", "q6", "uv", "kd", "e", "lit")])
        check(lib().mcpt_baked_radiance(self._h, C.byref(s), _p(rays, C.c_double), n, _baked_flags(face_viewer, lighting_only), C.byref(o),
                                        C.byref(stats) if stats is not None else None))
        return out

    def baked_radiance_device(self, d_rays_ptr, n, source_struct, outputs_struct, face_viewer=False, lighting_only=False, stats=None, stream=None):
        """The same between caller-owned device buffers on `stream` (mcpt_baked_radiance_device): source_struct a BakedSource and
        outputs_struct a BakedOutputs of device pointers."""
        check(lib().mcpt_baked_radiance_device(self._h, C.byref(source_struct), _dp(d_rays_ptr), int(n), _baked_flags(face_viewer, lighting_only),
                                               C.byref(outputs_struct), C.byref(stats) if stats is not None else None,
                                               _dp(stream)))

    def render_baked(self, source, samples=1, seed=0, face_viewer=False, lighting_only=False, workspace_rays=0, stats=None):
        """A frame lit by a bake (mcpt_render_baked): for every pixel, `samples` camera rays of the device's lens -- camera_rays(seed,
        pixel, k) -- shaded as baked_radiance shades them and averaged in k order.  Returns {"image": [H, W, 3] in generateImg's layout,
        "counts": [H, W, 3] = (surface, emitter, miss) samples per pixel, "lit": [H, W] surface samples whose lookup found anything}.
        workspace_rays bounds the rays in flight (0: the library's default); it does not change the result."""
        if not isinstance(samples, numbers.Integral) or not -2 ** 31 <= samples < 2 ** 31:
            raise ValueError("samples must be a 32-bit integer")
        if not isinstance(workspace_rays, numbers.Integral) or not -2 ** 63 <= workspace_rays < 2 ** 63:
            raise ValueError("workspace_rays must be a 64-bit integer")
        s = self._baked_source(source)
        fp = BakedFrameParams(int(samples), _baked_flags(face_viewer, lighting_only), int(seed), int(workspace_rays), (C.c_int32 * 2)(0, 0))
        img = np.zeros((self.height, self.width, 3))
        counts, lit = np.zeros((self.height, self.width, 3), dtype=np.int32), np.zeros((self.height, self.width), dtype=np.int32)
        check(lib().mcpt_render_baked(self._h, C.byref(s), C.byref(fp), _p(img, C.c_double), _p(counts, C.c_int32), _p(lit, C.c_int32),
                                      C.byref(stats) if stats is not None else None))
        return {"image": img, "counts": counts, "lit": lit}

    def render_baked_device(self, source_struct, d_img_ptr, samples=1, seed=0, face_viewer=False, lighting_only=False, workspace_rays=0,
                            d_counts_ptr=None, d_lit_ptr=None, stats=None, stream=None):
        """The same into a caller-owned device buffer on `stream` (mcpt_render_baked_device): source_struct a BakedSource of device
        pointers.  Returns without waiting when stats is None."""
        fp = BakedFrameParams(int(samples), _baked_flags(face_viewer, lighting_only), int(seed), int(workspace_rays), (C.c_int32 * 2)(0, 0))
        check(lib().mcpt_render_baked_device(self._h, C.byref(source_struct), C.byref(fp), _dp(d_img_ptr),
                                             _dp(d_counts_ptr), _dp(d_lit_ptr),
                                             C.byref(stats) if stats is not None else None, _dp(stream)))

    def reflection_volume_lookup(self, volume, points, normals, dirs, ns):
        """A reflection volume's lookup on the GPU (mcpt_reflection_volume_lookup): reflection_volume_lookup_host's arguments and
        answers, bit for bit.  Returns (radiance [m, 3], corners [m])."""
        q, dirs, ns = _volume_receivers(volume, points, normals, dirs, ns)
        m = q.shape[0]
        out, corners = np.zeros((m, 3)), np.zeros(m, dtype=np.int32)
        v = volume
        check(lib().mcpt_reflection_volume_lookup(self._h, C.byref(v.grid), C.byref(v.chain_desc), _p(v.chain, C.c_double), _p(v.valid, C.c_uint8),
                                                  _p(v.moments, C.c_double), C.byref(v.vis) if v.vis is not None else None, _p(q, C.c_double),
                                                  _p(dirs, C.c_double), _p(ns, C.c_double), m, _p(out, C.c_double), _p(corners, C.c_int32)))
        return out, corners

    def reflection_volume_lookup_device(self, specular_struct, d_q6_ptr, d_dirs_ptr, d_ns_ptr, m, d_out_ptr, d_corners_ptr=None, stream=None):
        """The same between caller-owned device buffers on `stream` (mcpt_reflection_volume_lookup_device); never waits.  specular_struct: a
        BakedSpecular whose chain_data, valid and moments are device pointers."""
        s = specular_struct
        check(lib().mcpt_reflection_volume_lookup_device(self._h, s.grid, s.chain, _dp(s.chain_data), _dp(s.valid), _dp(s.moments), s.visibility,
                                                         _dp(d_q6_ptr), _dp(d_dirs_ptr), _dp(d_ns_ptr), int(m), _dp(d_out_ptr), _dp(d_corners_ptr),
                                                         _dp(stream)))

    @staticmethod
    def _baked_specular(specular):
        if not isinstance(specular, _BakedReflection):
            raise ValueError("specular must come from baked_reflection")
        return specular.struct()

    def baked_radiance_specular(self, rays, source, specular, face_viewer=False, lighting_only=False, stats=None):
        """baked_radiance with a specular term (mcpt_baked_radiance_specular): a surface hit whose material has a non-zero ks also shows
        ks * R, R the radiance the reflection volume `specular` (baked_reflection) holds at the hit along the mirror direction under the
        material's exponent Ns (R alone under lighting_only).  Returns baked_radiance's dict -- everything but radiance is the plain
        call's, bit for bit -- with spec [n, 3] = R, ks [n, 3], r [n, 3] (the mirror direction scaled by |n|^2), ns [n] and slit [n] (the
        probes that took part), all 0 where a ray has no specular term."""
        rays = np.ascontiguousarray(rays, dtype=np.float64)
        if rays.ndim != 2 or rays.shape[1] != 6:
            raise ValueError("rays must have shape (n, 6), not %r" % (rays.shape,))
        n = rays.shape[0]
        s, sp = self._baked_source(source), self._baked_specular(specular)
        out = {"radiance": np.zeros((n, 3)), "kind": np.zeros(n, dtype=np.int32), "face": np.zeros(n, dtype=np.int32), "q6": np.zeros((n, 6)),
               "uv": np.zeros((n, 2)), "kd": np.zeros((n, 3)), "e": np.zeros((n, 3)), "lit": np.zeros(n, dtype=np.int32),
               "spec": np.zeros((n, 3)), "ks": np.zeros((n, 3)), "r": np.zeros((n, 3)), "ns": np.zeros(n), "slit": np.zeros(n, dtype=np.int32)}
        o = BakedOutputs(*[out[k].ctypes.data for k in ("radiance", "kind", "face", "q6", "uv", "kd", "e", "lit")])
        so = BakedSpecularOutputs(*[out[k].ctypes.data for k in ("spec", "ks", "r", "ns", "slit")])
        check(lib().mcpt_baked_radiance_specular(self._h, C.byref(s), C.byref(sp), _p(rays, C.c_double), n, _baked_flags(face_viewer, lighting_only),
                                                 C.byref(o), C.byref(so), C.byref(stats) if stats is not None else None))
        return out

    def baked_radiance_specular_device(self, d_rays_ptr, n, source_struct, specular_struct, outputs_struct, specular_outputs_struct=None, face_viewer=False,
                                       lighting_only=False, stats=None, stream=None):
        """The same between caller-owned device buffers on `stream` (mcpt_baked_radiance_specular_device): source_struct a BakedSource,
        specular_struct a BakedSpecular, outputs_struct a BakedOutputs and specular_outputs_struct a BakedSpecularOutputs (or None) of
        device pointers."""
        check(lib().mcpt_baked_radiance_specular_device(self._h, C.byref(source_struct), C.byref(specular_struct), _dp(d_rays_ptr), int(n),
                                                        _baked_flags(face_viewer, lighting_only), C.byref(outputs_struct),
                                                        C.byref(specular_outputs_struct) if specular_outputs_struct is not None else None,
                                                        C.byref(stats) if stats is not None else None, _dp(stream)))

    def render_baked_specular(self, source, specular, samples=1, seed=0, face_viewer=False, lighting_only=False, workspace_rays=0, stats=None):
        """render_baked with every sample shaded as baked_radiance_specular shades it (mcpt_render_baked_specular).  Returns render_baked's
        dict with "slit": [H, W] the samples whose specular lookup found a probe."""
        if not isinstance(samples, numbers.Integral) or not -2 ** 31 <= samples < 2 ** 31:
            raise ValueError("samples must be a 32-bit integer")
        if not isinstance(workspace_rays, numbers.Integral) or not -2 ** 63 <= workspace_rays < 2 ** 63:
            raise ValueError("workspace_rays must be a 64-bit integer")
        s, sp = self._baked_source(source), self._baked_specular(specular)
        fp = BakedFrameParams(int(samples), _baked_flags(face_viewer, lighting_only), int(seed), int(workspace_rays), (C.c_int32 * 2)(0, 0))
        img = np.zeros((self.height, self.width, 3))
        counts, lit = np.zeros((self.height, self.width, 3), dtype=np.int32), np.zeros((self.height, self.width), dtype=np.int32)
        slit = np.zeros((self.height, self.width), dtype=np.int32)
        check(lib().mcpt_render_baked_specular(self._h, C.byref(s), C.byref(sp), C.byref(fp), _p(img, C.c_double), _p(counts, C.c_int32),
                                               _p(lit, C.c_int32), _p(slit, C.c_int32), C.byref(stats) if stats is not None else None))
        return {"image": img, "counts": counts, "lit": lit, "slit": slit}

    def render_baked_specular_device(self, source_struct, specular_struct, d_img_ptr, samples=1, seed=0, face_viewer=False, lighting_only=False,
                                     workspace_rays=0, d_counts_ptr=None, d_lit_ptr=None, d_slit_ptr=None, stats=None, stream=None):
        """The same into a caller-owned device buffer on `stream` (mcpt_render_baked_specular_device): source_struct a BakedSource and
        specular_struct a BakedSpecular of device pointers.  Returns without waiting when stats is None."""
        fp = BakedFrameParams(int(samples), _baked_flags(face_viewer, lighting_only), int(seed), int(workspace_rays), (C.c_int32 * 2)(0, 0))
        check(lib().mcpt_render_baked_specular_device(self._h, C.byref(source_struct), C.byref(specular_struct), C.byref(fp), _dp(d_img_ptr),
                                                      _dp(d_counts_ptr), _dp(d_lit_ptr), _dp(d_slit_ptr),
                                                      C.byref(stats) if stats is not None else None, _dp(stream)))

    def bake_reflection_volume(self, grid, res, spp, seed=0, sample_base=0, workspace_rays=0, flags=0, stats=None):
        """Reflection probes on every probe of a grid: bake_reflection_probes of volume_points(grid), bit for bit, reshaped.  Returns
        (radiance [nz, ny, nx, res * res, 3], stderr [nz, ny, nx, res * res, 3], hits [nz, ny, nx, res * res]); prefilter_reflection of
        the first, flattened to [nprobes, res * res, 3], gives the chain baked_reflection takes."""
        rad, err, hits = self.bake_reflection_probes(volume_points(grid), res, spp, seed=seed, sample_base=sample_base, workspace_rays=workspace_rays,
                                                     flags=flags, stats=stats)
        shape = (grid.nz, grid.ny, grid.nx)
        return rad.reshape(shape + rad.shape[1:]), err.reshape(shape + err.shape[1:]), hits.reshape(shape + hits.shape[1:])

    @staticmethod
    def _reflection_params(res, spp, seed, sample_base, workspace_rays, flags):
        _int32(res=res, spp=spp, sample_base=sample_base, flags=flags)
        if not isinstance(workspace_rays, numbers.Integral) or not -2 ** 63 <= workspace_rays < 2 ** 63:
            raise ValueError("workspace_rays must be a 64-bit integer")
        return ReflectionParams(int(spp), int(sample_base), int(seed), int(res), int(flags), int(workspace_rays), (C.c_int32 * 4)(0, 0, 0, 0))

    @staticmethod
    def _id_base(id_base, n):
        if id_base is None:
            return None
        id_base = np.asarray(id_base)
        if id_base.dtype.kind not in "iu" or id_base.shape != (n,):
            raise ValueError("id_base must be %d integers" % n)
        if id_base.size and (int(id_base.min()) < -2 ** 31 or int(id_base.max()) >= 2 ** 31):
            raise ValueError("id_base must fit 32 bits")
        return np.ascontiguousarray(id_base, dtype=np.int32)

    def bake_reflection_probes(self, points, res, spp, seed=0, sample_base=0, id_base=None, workspace_rays=0, flags=0, stats=None):
        """Reflection probes (mcpt_bake_reflection): for each of points (n, 3) a res x res octahedral map of the path-traced radiance
        arriving there, spp jittered rays per texel -- radiance() with spp = 1 over reflection_rays(), folded per texel, bit for bit.
        Sample j of texel b of probe i has the RNG id id_base[i] + b * spp + j (id_base None: i * res * res * spp) and the sample index
        sample_base.  Returns (radiance [n, res * res, 3], stderr [n, res * res, 3], hits [n, res * res]); prefilter_reflection takes
        the first.  workspace_rays bounds the rays in flight (0: the library's default); it does not change the result."""
        p, _ = self._probe_list(points, None)
        rp = self._reflection_params(res, spp, seed, sample_base, workspace_rays, flags)
        n, texels = p.shape[0], int(res) ** 2 if 1 <= res <= 256 else 0      # (the library refuses any other res)
        id_base = self._id_base(id_base, n)
        rad, err, hits = np.zeros((n, texels, 3)), np.zeros((n, texels, 3)), np.zeros((n, texels), dtype=np.int32)
        check(lib().mcpt_bake_reflection(self._h, _p(p, C.c_double), _p(id_base, C.c_int32), n, C.byref(rp), _p(rad, C.c_double), _p(err, C.c_double),
                                         _p(hits, C.c_int32), C.byref(stats) if stats is not None else None))
        return rad, err, hits

    def bake_reflection_probes_device(self, d_points_ptr, n, d_radiance_ptr, res, spp, seed=0, sample_base=0, d_id_base_ptr=None, workspace_rays=0, flags=0,
                                      d_stderr_ptr=None, d_hits_ptr=None, stats=None, stream=None):
        """The same between caller-owned device buffers on `stream` (mcpt_bake_reflection_device).  Returns without waiting when stats
        is None."""
        rp = self._reflection_params(res, spp, seed, sample_base, workspace_rays, flags)
        check(lib().mcpt_bake_reflection_device(self._h, _dp(d_points_ptr), _dp(d_id_base_ptr), int(n), C.byref(rp), _dp(d_radiance_ptr), _dp(d_stderr_ptr),
                                                _dp(d_hits_ptr), C.byref(stats) if stats is not None else None, _dp(stream)))

    def reflection_rays(self, points, res, spp, entries, seed=0, sample_base=0, id_base=None):
        """test seam (mcpt_reflection_rays): (rays [m, 6] = origin, direction, ids [m]) of the listed entries of
        bake_reflection_probes(points, res, spp, ...); entry (i * res * res + b) * spp + j is sample j of texel b of probe i."""
        p, _ = self._probe_list(points, None)
        rp = self._reflection_params(res, spp, seed, sample_base, 0, 0)
        id_base = self._id_base(id_base, p.shape[0])
        e = np.asarray(entries)
        if e.dtype.kind not in "iu" or e.ndim != 1:
            raise ValueError("entries must be a list of integers")
        e = np.ascontiguousarray(e, dtype=np.int64)
        rays, ids = np.zeros((e.shape[0], 6)), np.zeros(e.shape[0], dtype=np.int32)
        check(lib().mcpt_reflection_rays(self._h, _p(p, C.c_double), _p(id_base, C.c_int32), p.shape[0], C.byref(rp), _p(e, C.c_int64), e.shape[0],
                                         _p(rays, C.c_double), _p(ids, C.c_int32)))
        return rays, ids

    def prefilter_reflection(self, radiance, res, levels):
        """The prefilter on the GPU (mcpt_reflection_prefilter): radiance [n, res * res, 3] convolved with the Phong lobe of every
        (level_res, ns) of levels -- reflection_prefilter_host's answer, bit for bit.  Returns (chain_desc, chain [n, T, 3]) for
        reflection_lookup."""
        c = reflection_chain(res, levels)
        radiance = _reflection_maps(c, radiance)
        chain = np.zeros((radiance.shape[0], c.num_texels, 3))
        check(lib().mcpt_reflection_prefilter(self._h, C.byref(c), _p(radiance, C.c_double), radiance.shape[0], _p(chain, C.c_double)))
        return c, chain

    def prefilter_reflection_device(self, chain_desc, d_radiance_ptr, n, d_chain_ptr, stream=None):
        """The same between caller-owned device buffers on `stream` (mcpt_reflection_prefilter_device); never waits."""
        check(lib().mcpt_reflection_prefilter_device(self._h, C.byref(chain_desc), _dp(d_radiance_ptr), int(n), _dp(d_chain_ptr), _dp(stream)))

    def reflection_lookup(self, chain_desc, chain, probe, dirs, ns):
        """The lookup on the GPU (mcpt_reflection_lookup): reflection_lookup_host's arguments and answer, bit for bit."""
        chain, probe, dirs, ns = _reflection_receivers(chain_desc, chain, probe, dirs, ns)
        out = np.zeros((dirs.shape[0], 3))
        check(lib().mcpt_reflection_lookup(self._h, C.byref(chain_desc), _p(chain, C.c_double), chain.shape[0], _p(probe, C.c_int32), _p(dirs, C.c_double),
                                           _p(ns, C.c_double), dirs.shape[0], _p(out, C.c_double)))
        return out

    def reflection_lookup_device(self, chain_desc, d_chain_ptr, n, d_probe_ptr, d_dirs_ptr, d_ns_ptr, m, d_out_ptr, stream=None):
        """The same between caller-owned device buffers on `stream` (mcpt_reflection_lookup_device); never waits.  A probe index outside
        0 .. n - 1 gives +0.0."""
        check(lib().mcpt_reflection_lookup_device(self._h, C.byref(chain_desc), _dp(d_chain_ptr), int(n), _dp(d_probe_ptr), _dp(d_dirs_ptr), _dp(d_ns_ptr),
                                                  int(m), _dp(d_out_ptr), _dp(stream)))

    def set_environment(self, rgb=None, scale=1.0):
        """The environment light of every later frame, sample_radiance and progressive handle created after it (mcpt_device_set_environment):
        rgb = an (H, W, 3) lat-long radiance map (top row first) or an (r, g, b) constant sky; None clears it."""
        if rgb is None:
            check(lib().mcpt_device_set_environment(self._h, None))
            return
        e, tex = make_environment(rgb, scale)
        check(lib().mcpt_device_set_environment(self._h, C.byref(e)))
        del tex

    @property
    def environment(self):
        """the device's environment: None, or a dict of width, height, scale and Z (Z == 0: inactive)"""
        w, h, s, z = C.c_int32(), C.c_int32(), C.c_double(), C.c_double()
        check(lib().mcpt_device_get_environment(self._h, C.byref(w), C.byref(h), C.byref(s), C.byref(z)))
        if w.value == 0:
            return None
        return {"width": w.value, "height": h.value, "scale": s.value, "Z": z.value}

    def environment_eval(self, dirs):
        """Le(dirs[i]) under the device's (active) environment: (n, 3)"""
        dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
        rgb = np.zeros((dirs.shape[0], 3))
        check(lib().mcpt_environment_eval(self._h, _p(dirs, C.c_double), dirs.shape[0], _p(rgb, C.c_double)))
        return rgb

    def environment_sample(self, seed, pix, k, depth):
        """the environment's draw at vertex `depth` of camera samples (pix[i], k[i]): directions (n, 3), pdf (n,), radiance (n, 3)"""
        pix = np.ascontiguousarray(pix, dtype=np.int32)
        k = np.ascontiguousarray(k, dtype=np.int32)
        n = pix.shape[0]
        dirs, pdf, rgb = np.zeros((n, 3)), np.zeros(n), np.zeros((n, 3))
        check(lib().mcpt_environment_sample(self._h, seed, _p(pix, C.c_int32), _p(k, C.c_int32), int(depth), n, _p(dirs, C.c_double),
                                            _p(pdf, C.c_double), _p(rgb, C.c_double)))
        return dirs, pdf, rgb

    def set_light_sampling(self, mode="all", weights=None):
        """How every later frame, pass and sample_radiance samples the scene's lights (mcpt_device_set_light_sampling): "all" (or None) --
        every light at every vertex, the reference's loop -- or "one": one light per vertex, picked with probability weight / sum and
        divided by it -- or "tree": one light per vertex, picked by a descent of the light tree that weighs every node by its distance from
        the vertex and culls what lies below the vertex's horizon.  weights: None (luminance x area) or one non-negative weight per light;
        a light of weight 0 is never picked."""
        ls, keep = make_light_sampling(mode, weights)
        check(lib().mcpt_device_set_light_sampling(self._h, C.byref(ls) if ls is not None else None))
        del keep

    def light_sampling(self):
        """the device's light sampling: (mode, pdf) with mode "all", "one" or "tree" and pdf the pick probability of every light (1 under
        "all"; under "tree" the root's distribution -- a vertex's own comes from Scene.light_tree_pdf and light_pick_at)"""
        m = C.c_int32()
        pdf = np.zeros(self.scene.info.num_lights)
        check(lib().mcpt_device_get_light_sampling(self._h, C.byref(m), _p(pdf, C.c_double) if pdf.size else None))
        return {LIGHTS_ONE: "one", LIGHTS_TREE: "tree"}.get(m.value, "all"), pdf

    def light_pick(self, seed, pix, k, depth):
        """the light "one" picks at vertex `depth` of camera samples (pix[i], k[i]): indices (n,) int32, their probabilities (n,)"""
        pix = np.ascontiguousarray(pix, dtype=np.int32)
        k = np.ascontiguousarray(k, dtype=np.int32)
        n = pix.shape[0]
        light, pdf = np.zeros(n, dtype=np.int32), np.zeros(n)
        check(lib().mcpt_light_pick(self._h, seed, _p(pix, C.c_int32), _p(k, C.c_int32), int(depth), n, _p(light, C.c_int32), _p(pdf, C.c_double)))
        return light, pdf

    def light_pick_at(self, seed, pix, k, depth, p, pn):
        """the light "tree" picks at the vertices p[i] with normals pn[i] at `depth` of camera samples (pix[i], k[i]): indices (n,) int32 and
        the probabilities they were picked with (n,) (mcpt_light_pick_at: the path kernels' own device function)"""
        pix = np.ascontiguousarray(pix, dtype=np.int32)
        k = np.ascontiguousarray(k, dtype=np.int32)
        p = np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3)
        pn = np.ascontiguousarray(pn, dtype=np.float64).reshape(-1, 3)
        n = pix.shape[0]
        if k.shape[0] != n or p.shape[0] != n or pn.shape[0] != n:
            raise ValueError("one (pixel, sample, vertex, normal) per pick")
        light, pdf = np.zeros(n, dtype=np.int32), np.zeros(n)
        check(lib().mcpt_light_pick_at(self._h, seed, _p(pix, C.c_int32), _p(k, C.c_int32), int(depth), _p(p, C.c_double), _p(pn, C.c_double), n,
                                       _p(light, C.c_int32), _p(pdf, C.c_double)))
        return light, pdf

    def update_vertices(self, v, mode="refit", stream=None):
        """New positions for every face, in place (mcpt_device_update_vertices): v = [num_faces, 9] (v1 v2 v3 of every face, .obj order) as
        a numpy array, a torch tensor on this GPU (float64, contiguous) or a raw device pointer (int); mode "refit" keeps the culling
        hierarchy's topology and recomputes its boxes, "rebuild" builds it again.  The frame afterwards is that of a fresh device on the
        moved scene, bit for bit.  Returns the mcpt_update_info record as a dict."""
        n = self.scene.info.num_faces
        info = UpdateInfo()
        m = _update_mode(mode)
        if isinstance(v, numbers.Integral):
            v = int(v)
            check(lib().mcpt_device_update_vertices_device(self._h, C.c_void_p(v), m, C.byref(info), C.c_void_p(stream) if stream else None))
        elif hasattr(v, "data_ptr") and getattr(v, "is_cuda", False):
            if v.numel() != n * 9 or not v.is_contiguous() or str(v.dtype) != "torch.float64":
                raise ValueError("a device tensor of vertices must be contiguous float64 with %d elements" % (n * 9))
            check(lib().mcpt_device_update_vertices_device(self._h, C.c_void_p(v.data_ptr()), m, C.byref(info), C.c_void_p(stream) if stream else None))
        else:
            if hasattr(v, "detach"):
                v = v.detach().cpu().numpy()
            v = _host_vertices(v, n)
            check(lib().mcpt_device_update_vertices(self._h, _p(v, C.c_double), m, C.byref(info)))
        return info.as_dict()

    def vertices(self):
        """the positions the device holds now, [num_faces, 9] in .obj order (mcpt_device_get_vertices)"""
        v = np.zeros((self.scene.info.num_faces, 9))
        check(lib().mcpt_device_get_vertices(self._h, _p(v, C.c_double)))
        return v

    def set_camera(self, eye, look_at, up, fovy):
        """The camera of every later frame (mcpt_device_set_camera); width and height stay."""
        e, l, u = _camera_args(eye, look_at, up)
        check(lib().mcpt_device_set_camera(self._h, _p(e, C.c_double), _p(l, C.c_double), _p(u, C.c_double), float(fovy)))

    def camera(self):
        """the device's camera as a dict of eye, look_at, up (arrays) and fovy"""
        e, l, u, f = np.zeros(3), np.zeros(3), np.zeros(3), C.c_double()
        check(lib().mcpt_device_get_camera(self._h, _p(e, C.c_double), _p(l, C.c_double), _p(u, C.c_double), C.byref(f)))
        return {"eye": e, "look_at": l, "up": u, "fovy": f.value}

    def set_motion(self, v_end=None, camera_end=None, shutter=(0.0, 1.0), steps=1, stream=None):
        """A motion between what the device holds now (key 0) and key 1 (mcpt_device_set_motion): v_end as update_vertices takes the
        vertices (None: the geometry does not move), camera_end a dict of eye, look_at, up and fovy (None: the camera does not move),
        shutter = (open, close) within [0, 1] rendered in `steps` time steps.  generateImg, render_device and progressive frames then
        render the shutter frame; everything else keeps seeing key 0."""
        n = self.scene.info.num_faces
        sh = _shutter(shutter, steps)
        cam = None
        if camera_end is not None:
            e, l, u = _camera_args(camera_end["eye"], camera_end["look_at"], camera_end["up"])
            cam = CameraKey((C.c_double * 3)(*e), (C.c_double * 3)(*l), (C.c_double * 3)(*u), float(camera_end["fovy"]))
        cam = C.byref(cam) if cam is not None else None
        if isinstance(v_end, numbers.Integral):
            check(lib().mcpt_device_set_motion_device(self._h, C.c_void_p(int(v_end)), cam, C.byref(sh), C.c_void_p(stream) if stream else None))
        elif hasattr(v_end, "data_ptr") and getattr(v_end, "is_cuda", False):
            if v_end.numel() != n * 9 or not v_end.is_contiguous() or str(v_end.dtype) != "torch.float64":
                raise ValueError("a device tensor of vertices must be contiguous float64 with %d elements" % (n * 9))
            check(lib().mcpt_device_set_motion_device(self._h, C.c_void_p(v_end.data_ptr()), cam, C.byref(sh), C.c_void_p(stream) if stream else None))
        else:
            if v_end is not None:
                if hasattr(v_end, "detach"):
                    v_end = v_end.detach().cpu().numpy()
                v_end = _host_vertices(v_end, n)
            check(lib().mcpt_device_set_motion(self._h, _p(v_end, C.c_double) if v_end is not None else None, cam, C.byref(sh)))

    def clear_motion(self):
        """the device without a motion again, at key 0 (mcpt_device_clear_motion)"""
        check(lib().mcpt_device_clear_motion(self._h))

    @property
    def motion(self):
        """None, or the device's motion as a dict: shutter (open, close), steps, has_geometry, has_camera, camera_end"""
        sh, g, c, cam = Shutter(), C.c_int32(), C.c_int32(), CameraKey()
        check(lib().mcpt_device_get_motion(self._h, C.byref(sh), C.byref(g), C.byref(c), C.byref(cam)))
        if sh.steps == 0:
            return None
        return {"shutter": (sh.open, sh.close), "steps": sh.steps, "has_geometry": bool(g.value), "has_camera": bool(c.value),
                "camera_end": {"eye": np.array(cam.eye), "look_at": np.array(cam.look_at), "up": np.array(cam.up), "fovy": cam.fovy}}

    def motion_info(self):
        """what the steps of the last motion frame (or progressive pass) took: steps_run, ms_updates, max_cost_ratio"""
        info = MotionInfo()
        check(lib().mcpt_device_motion_info(self._h, C.byref(info)))
        return info.as_dict()

    def display(self, img, **kw):
        """The display transform of a frame on this GPU (mcpt_display): img [..., 3] float64 and make_display's arguments -> (uint8 array
        [..., 3] or [..., 4], info dict of the exposure and white used and of the histogram, when one was taken)."""
        img, n = _frame_pixels(img)
        dp, info = make_display(**kw), DisplayInfo()
        out = np.zeros(img.shape[:-1] + (4 if dp.flags & DISPLAY_RGBA else 3,), dtype=np.uint8)
        check(lib().mcpt_display(self._h, _p(img, C.c_double), n, C.byref(dp), _p(out, C.c_uint8), C.byref(info)))
        return out, info.as_dict()

    def display_device(self, d_img_ptr, n_pixels, d_out_ptr, stream=None, **kw):
        """The same between caller-owned device buffers (e.g. torch tensors' data_ptr()) on `stream` (mcpt_display_device): the info dict."""
        dp, info = make_display(**kw), DisplayInfo()
        check(lib().mcpt_display_device(self._h, C.c_void_p(d_img_ptr), int(n_pixels), C.byref(dp), C.c_void_p(d_out_ptr), C.byref(info),
                                        C.c_void_p(stream) if stream else None))
        return info.as_dict()

    def luminance_histogram(self, img):
        """the 387 slots of a frame's luminance histogram, counted on this GPU (mcpt_display_histogram): int64"""
        img, n = _frame_pixels(img)
        slots = np.zeros(DISPLAY_SLOTS, dtype=np.int64)
        check(lib().mcpt_display_histogram(self._h, _p(img, C.c_double), n, slots.ctypes.data_as(C.POINTER(C.c_int64))))
        return slots

    def progressive(self, spp, seed=0, rank=0, world=1, tile_w=0, tile_h=0, flags=0):
        """A frame of `spp` samples per pixel rendered in passes (mcpt_progressive_*): see Progressive."""
        return Progressive(self, spp, seed, rank, world, tile_w, tile_h, flags)

    def adaptive(self, spp, rel_target, abs_target=0.0, min_spp=16, seed=0, rank=0, world=1, tile_w=0, tile_h=0, flags=0):
        """An adaptive frame (mcpt_progressive_create_adaptive): a Progressive whose pixels stop on their own error estimate."""
        return Progressive(self, spp, seed, rank, world, tile_w, tile_h, flags, adaptive=AdaptiveParams(rel_target, abs_target, min_spp, 0))


class Progressive:
    """A progressive frame on a Device.  step(n) renders the next n samples of every owned pixel; at done == spp, image() is generateImg's
    frame bit for bit.  Before that, image() is the fp64 mean of the samples done (not the float fold) and stderr() its standard error.
    An adaptive frame (Device.adaptive) renders only the active pixels; image() and stderr() then use every pixel's own count
    (sample_counts())."""

    def __init__(self, device, spp, seed=0, rank=0, world=1, tile_w=0, tile_h=0, flags=0, adaptive=None):
        self.device, self.spp = device, spp
        self._h = C.c_void_p()
        rp = RenderParams(spp, seed, rank, world, tile_w, tile_h, flags)
        if adaptive is None:
            check(lib().mcpt_progressive_create(device._h, C.byref(rp), C.byref(self._h)))
        else:
            check(lib().mcpt_progressive_create_adaptive(device._h, C.byref(rp), C.byref(adaptive), C.byref(self._h)))

    def step(self, n, stats=None):
        check(lib().mcpt_progressive_step(self._h, n, C.byref(stats) if stats is not None else None))
        return self.done

    @property
    def done(self):
        rc = lib().mcpt_progressive_done(self._h)
        if rc < 0:
            check(rc)
        return rc

    @property
    def active(self):
        """pixels the next step renders (0: the frame is complete)"""
        n = lib().mcpt_progressive_active(self._h)
        if n < 0:
            check(n)
        return n

    def active_pixels(self):
        """the active pixel list, ascending, as int32"""
        out = np.zeros(self.active, dtype=np.int32)
        n = lib().mcpt_progressive_active_pixels(self._h, _p(out, C.c_int32))
        if n < 0:
            check(n)
        return out[:n]

    def sample_counts(self, counts=None):
        """the samples every owned pixel holds, as [H,W] int32 (pixels not owned: left as in counts, else 0)"""
        if counts is None:
            counts = np.zeros((self.device.height, self.device.width), dtype=np.int32)
        check(lib().mcpt_progressive_sample_counts(self._h, _p(counts, C.c_int32)))
        return counts

    def noise(self):
        """Noise: rel_error, abs_rms, sum_se2, sum_mean2, pixels (owned hit pixels), done, spp"""
        o = Noise()
        check(lib().mcpt_progressive_noise(self._h, C.byref(o)))
        return o

    def image(self, img=None):
        """the current estimate as [H,W,3] float64 (pixels not owned: left as in img, else 0)"""
        if img is None:
            img = np.zeros((self.device.height, self.device.width, 3))
        check(lib().mcpt_progressive_image(self._h, _p(img, C.c_double), None))
        return img

    def stderr(self, err=None):
        """the per-pixel, per-channel standard error of image() as [H,W,3] float64 (0 while done < 2)"""
        if err is None:
            err = np.zeros((self.device.height, self.device.width, 3))
        check(lib().mcpt_progressive_image(self._h, None, _p(err, C.c_double)))
        return err

    def aovs(self):
        """the first-hit AOVs of the owned pixels (mcpt_progressive_aovs): a dict of numpy arrays, material [H,W] int32 (-1: a miss),
        depth [H,W], normal [H,W,3] (not normalised) and albedo [H,W,3] float64.  Pixels not owned: material -1, the rest 0."""
        h, w = self.device.height, self.device.width
        out = {"material": np.full((h, w), -1, dtype=np.int32), "depth": np.zeros((h, w)), "normal": np.zeros((h, w, 3)),
               "albedo": np.zeros((h, w, 3))}
        check(lib().mcpt_progressive_aovs(self._h, _p(out["material"], C.c_int32), _p(out["depth"], C.c_double),
                                          _p(out["normal"], C.c_double), _p(out["albedo"], C.c_double)))
        return out

    def denoise(self, iterations=0, sigma_l=0.0, sigma_z=0.0, img=None):
        """the a-trous denoised estimate as [H,W,3] float64 (mcpt_progressive_denoise; pixels not owned: left as in img, else 0).  All
        three 0: the defaults; otherwise iterations is taken as given (0: the estimate) and a sigma of 0 is its default.  Biased, unlike
        image(); needs done >= 2."""
        if img is None:
            img = np.zeros((self.device.height, self.device.width, 3))
        dp = DenoiseParams(iterations, 0, sigma_l, sigma_z)
        check(lib().mcpt_progressive_denoise(self._h, C.byref(dp), _p(img, C.c_double)))
        return img

    def sample_aovs(self, samples=0):
        """the AOVs averaged over `samples` camera samples of every owned pixel under the handle's lens (mcpt_progressive_sample_aovs; 0:
        min(spp, 16)): a dict of numpy arrays, counts [H,W,3] int32 (surface, emitter and miss samples), depth [H,W], normal [H,W,3] (the
        mean unit normal, not renormalised) and albedo [H,W,3] float64.  Pixels not owned: 0."""
        h, w = self.device.height, self.device.width
        out = {"counts": np.zeros((h, w, 3), dtype=np.int32), "depth": np.zeros((h, w)), "normal": np.zeros((h, w, 3)),
               "albedo": np.zeros((h, w, 3))}
        check(lib().mcpt_progressive_sample_aovs(self._h, samples, _p(out["counts"], C.c_int32), _p(out["depth"], C.c_double),
                                                 _p(out["normal"], C.c_double), _p(out["albedo"], C.c_double)))
        return out

    def denoise_guided(self, iterations=0, sigma_l=0.0, sigma_z=0.0, samples=0, sigma_a=0.0, img=None):
        """denoise() guided by sample_aovs(samples) instead of the first-hit AOVs (mcpt_progressive_denoise_guided): the filter for frames
        under a lens.  iterations, sigma_l and sigma_z as in denoise(); samples and sigma_a of 0 are their defaults."""
        if img is None:
            img = np.zeros((self.device.height, self.device.width, 3))
        dp = DenoiseParams(iterations, 0, sigma_l, sigma_z)
        gp = GuideParams(samples, 0, sigma_a)
        check(lib().mcpt_progressive_denoise_guided(self._h, C.byref(dp), C.byref(gp), _p(img, C.c_double)))
        return img

    def display(self, source="estimate", out=None, **kw):
        """The frame's picture without the frame leaving the GPU (mcpt_progressive_display): source "estimate" (image()), "denoised"
        (denoise()) or "denoised_guided" (denoise_guided()), the filters with their defaults; make_display's arguments -> (uint8 [H,W,3] or
        [H,W,4], info dict).  Pixels not owned: left as in out, else 0."""
        dp, info = make_display(**kw), DisplayInfo()
        shape = (self.device.height, self.device.width, 4 if dp.flags & DISPLAY_RGBA else 3)
        if out is None:
            out = np.zeros(shape, dtype=np.uint8)
        if out.dtype != np.uint8 or out.shape != shape or not out.flags["C_CONTIGUOUS"]:
            raise ValueError("out must be a contiguous uint8 array of shape %r" % (shape,))
        check(lib().mcpt_progressive_display(self._h, _SOURCES[source] if isinstance(source, str) else int(source), C.byref(dp),
                                             _p(out, C.c_uint8), C.byref(info)))
        return out, info.as_dict()

    def close(self):
        if getattr(self, "_h", None):
            lib().mcpt_progressive_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def progressive_next_pass(spp, done, remaining_s=float("inf"), s_per_sample=0.0):
    """render_scene's pass schedule (mcpt_progressive_next_pass): samples of the next pass, 0 = stop"""
    return lib().mcpt_progressive_next_pass(spp, done, remaining_s, s_per_sample)


class MultiDevice:
    """generateImg on several GPUs of the node behind one call (mcpt_multi_*): one host thread per GPU inside the library, tiles
    dealt like rank/world, every rank's pixels gathered into devices[0]'s HBM (peer copies over xGMI, or RCCL)."""

    def __init__(self, scene, devices=None, build=BUILD_HOST, gather=GATHER_PEER):
        self.scene = scene
        self._h = C.c_void_p()
        if devices is None:
            arr, n = None, 0
        else:
            devices = np.ascontiguousarray(devices, dtype=np.int32)
            arr, n = _p(devices, C.c_int32), devices.shape[0]
        check(lib().mcpt_multi_create(scene._h, arr, n, build, gather, C.byref(self._h)))
        i = scene.info
        self.width, self.height = i.width, i.height

    @property
    def num_devices(self):
        return lib().mcpt_multi_num_devices(self._h)

    def set_lens(self, aperture=0.0, focus_distance=0.0, jitter=False, per_sample=False):
        """the same lens on every device of the group (Device.set_lens)"""
        check(lib().mcpt_multi_set_lens(self._h, C.byref(make_lens(aperture, focus_distance, jitter, per_sample))))

    def set_environment(self, rgb=None, scale=1.0):
        """the same environment on every device of the group (Device.set_environment)"""
        if rgb is None:
            check(lib().mcpt_multi_set_environment(self._h, None))
            return
        e, tex = make_environment(rgb, scale)
        check(lib().mcpt_multi_set_environment(self._h, C.byref(e)))
        del tex

    def set_light_sampling(self, mode="all", weights=None):
        """the same light sampling on every device of the group (Device.set_light_sampling)"""
        ls, keep = make_light_sampling(mode, weights)
        check(lib().mcpt_multi_set_light_sampling(self._h, C.byref(ls) if ls is not None else None))
        del keep

    def update_vertices(self, v, mode="refit"):
        """new positions on every device of the group (Device.update_vertices, host arrays); the info record of devices[0]"""
        v = _host_vertices(v, self.scene.info.num_faces)
        info = UpdateInfo()
        check(lib().mcpt_multi_update_vertices(self._h, _p(v, C.c_double), _update_mode(mode), C.byref(info)))
        return info.as_dict()

    def set_camera(self, eye, look_at, up, fovy):
        """the same camera on every device of the group (Device.set_camera)"""
        e, l, u = _camera_args(eye, look_at, up)
        check(lib().mcpt_multi_set_camera(self._h, _p(e, C.c_double), _p(l, C.c_double), _p(u, C.c_double), float(fovy)))

    def generateImg(self, spp, seed=0, tile_w=0, tile_h=0, flags=0, stats=None):
        img = np.zeros((self.height, self.width, 3))
        rp = RenderParams(spp, seed, 0, 1, tile_w, tile_h, flags)
        check(lib().mcpt_multi_render(self._h, C.byref(rp), _p(img, C.c_double), C.byref(stats) if stats is not None else None))
        return img

    def render_device(self, spp, seed=0, tile_w=0, tile_h=0, flags=0, stats=None):
        """The frame stays in devices[0]'s HBM; returns its device address (valid until the next call)."""
        rp = RenderParams(spp, seed, 0, 1, tile_w, tile_h, flags)
        d_img = C.c_void_p()
        check(lib().mcpt_multi_render_device(self._h, C.byref(rp), C.byref(d_img), C.byref(stats) if stats is not None else None))
        return d_img.value

    def collect_stats(self, stats=None):
        """statistics of every RENDER_KEEP_STATS frame since the last call, summed over the GPUs"""
        stats = stats if stats is not None else Stats()
        check(lib().mcpt_multi_collect_stats(self._h, C.byref(stats)))
        return stats

    def last_timing(self):
        """(render_ms per rank, gather_ms, ranks the RCCL communicator reports -- 0 with peer copies) of the last frame"""
        n = self.num_devices
        render_ms = np.zeros(n)
        gather_ms = C.c_double()
        comm = C.c_int32()
        check(lib().mcpt_multi_last_timing(self._h, _p(render_ms, C.c_double), C.byref(gather_ms), C.byref(comm)))
        return render_ms, gather_ms.value, comm.value

    def close(self):
        if getattr(self, "_h", None):
            lib().mcpt_multi_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def imshow_rgb8(img):
    """The 8-bit conversion of imshow (MTPC/MTPC.cpp:22-30)."""
    img = np.ascontiguousarray(img, dtype=np.float64)
    out = np.zeros(img.shape, dtype=np.uint8)
    check(lib().mcpt_quantize_rgb8(_p(img, C.c_double), img.size, _p(out, C.c_uint8)))
    return out


def png_bytes(rgb8):
    rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
    h, w, _ = rgb8.shape
    cap = 128 + h * (w * 3 + 6)
    out = np.zeros(cap, dtype=np.uint8)
    n = lib().mcpt_png_encode(_p(rgb8, C.c_uint8), w, h, _p(out, C.c_uint8), cap)
    if n < 0:
        check(int(n))
    return out[:n].tobytes()


def write_png(file, rgb8, deflate=False):
    rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
    h, w, _ = rgb8.shape
    check((lib().mcpt_write_png_deflate if deflate else lib().mcpt_write_png)(file.encode(), _p(rgb8, C.c_uint8), w, h))


def png_bytes_deflate(rgb8):
    """The same picture as a compressed PNG (per-row filters + deflate)."""
    rgb8 = np.ascontiguousarray(rgb8, dtype=np.uint8)
    h, w, _ = rgb8.shape
    cap = 1024 + h * (w * 3 + 1) * 2
    out = np.zeros(cap, dtype=np.uint8)
    n = lib().mcpt_png_encode_deflate(_p(rgb8, C.c_uint8), w, h, _p(out, C.c_uint8), cap)
    if n < 0:
        check(int(n))
    return out[:n].tobytes()


def read_pfm(file):
    """A colour PFM (as write_pfm writes it) -> float32 [H, W, 3], top row first."""
    w, h = C.c_int32(), C.c_int32()
    check(lib().mcpt_read_pfm(file.encode(), C.byref(w), C.byref(h), None, 0))
    out = np.zeros((h.value, w.value, 3), dtype=np.float32)
    check(lib().mcpt_read_pfm(file.encode(), C.byref(w), C.byref(h), _p(out, C.c_float), out.size))
    return out


def write_pfm(file, img):
    """Linear radiance [H,W,3] as a little-endian fp32 Portable Float Map."""
    img = np.ascontiguousarray(img, dtype=np.float64)
    h, w, _ = img.shape
    check(lib().mcpt_write_pfm(file.encode(), _p(img, C.c_double), w, h))


def checkpoint_save(file, scene, img, spp, seed, done):
    img = np.ascontiguousarray(img, dtype=np.float64)
    done = np.ascontiguousarray(done, dtype=np.uint8)
    check(lib().mcpt_checkpoint_save(file.encode(), scene._h, _p(img, C.c_double), spp, seed, done.shape[0], _p(done, C.c_uint8)))


def checkpoint_load(file, scene, spp, seed, parts):
    """(img [H,W,3], done [parts]) of a matching checkpoint; McptError (code ERR_IO / ERR_PARSE) otherwise."""
    i = scene.info
    img = np.zeros((i.height, i.width, 3))
    done = np.zeros(parts, dtype=np.uint8)
    check(lib().mcpt_checkpoint_load(file.encode(), scene._h, _p(img, C.c_double), spp, seed, parts, _p(done, C.c_uint8)))
    return img, done


def decode_jpeg(file):
    """8-bit BGR raster [rows, cols, 3] of a JPEG file, as cv::imread would hand it to Material::readinMap."""
    w = np.zeros(1, dtype=np.int32)
    h = np.zeros(1, dtype=np.int32)
    check(lib().mcpt_decode_jpeg(file.encode(), _p(w, C.c_int32), _p(h, C.c_int32), None, 0))
    out = np.zeros((int(h[0]), int(w[0]), 3), dtype=np.uint8)
    check(lib().mcpt_decode_jpeg(file.encode(), _p(w, C.c_int32), _p(h, C.c_int32), _p(out, C.c_uint8), out.size))
    return out


def morton_code(x, y, z):
    return lib().mcpt_morton_code(x, y, z)


def render_scene(path, filename, N_ray_per_pixel, seed=0, device=0, width=0, height=0, quiet=True, output_prefix=None, stats=None,
                 load_flags=0, output_flags=0, checkpoint=None, checkpoint_parts=0, devices=None, gather=GATHER_PEER, noise_target=0.0,
                 time_budget_s=0.0, adaptive_min_spp=0, abs_target=0.0, lens=None, environment=None, environment_scale=1.0, motion=None,
                 light_sampling=None, display=None):
    """render_scene(path, filename, N) of MTPC/MTPC.cpp:35; writes <prefix>-SPP<N>.png (default ../result/<filename>).
    devices: list of GPU ordinals, or -1 for every visible GPU (the frame is then rendered by mcpt_multi_*).
    noise_target / time_budget_s / OUT_ERROR_PFM: a progressive frame that may stop at k < N samples (<prefix>-SPP<k>.png).
    adaptive_min_spp > 0: an adaptive frame, noise_target and abs_target its per-pixel targets (OUT_SPP_PFM: the sample-count map).
    OUT_DENOISED / OUT_AOV_PFM: also the denoised frame (.denoised.png, .denoised.pfm with OUT_PFM) / the first-hit AOVs as .pfm files.
    OUT_DENOISED_SAMPLES / OUT_SAMPLE_AOV_PFM: the frame denoised under the sample AOVs' guidance (.denoised-samples.*) / the sample AOVs
    (.s-albedo.pfm, .s-normal.pfm, .s-depth.pfm, .coverage.pfm): the guides that follow a lens.
    lens: None (the pinhole), a Lens or a dict of Device.set_lens's arguments; rendered through mcpt_render_scene_lens.
    environment: None, or the path of a colour PFM lat-long map (environment_scale: its scale); rendered through mcpt_render_scene_env.
    motion: None, or a dict of end_obj and end_camera (file paths, either may be missing), shutter = (open, close) and steps: the shutter
    frame between the scene and those files (mcpt_render_scene_motion).
    light_sampling: None / "all", "one", "tree", or a dict of Device.set_light_sampling's arguments; rendered through mcpt_render_scene_lights (not
    together with motion).
    display: None (imshow's bytes), a DisplayParams or a dict of make_display's arguments: the .png and .denoised*.png go through the display
    transform, the PFMs stay linear; rendered through mcpt_render_scene_display (not together with motion)."""
    dev_arr, ndev = None, 0
    if devices == -1:
        ndev = -1
    elif devices is not None:
        keep = np.ascontiguousarray(devices, dtype=np.int32)
        dev_arr, ndev = _p(keep, C.c_int32), keep.shape[0]
    o = RenderSceneOptions(seed, device, width, height, int(quiet), output_prefix.encode() if output_prefix else None,
                           load_flags, output_flags, checkpoint.encode() if checkpoint else None, checkpoint_parts, 0,
                           ndev, gather, dev_arr, noise_target, time_budget_s, adaptive_min_spp, 0, abs_target)
    st = C.byref(stats) if stats is not None else None
    ls, keep_w = make_light_sampling(light_sampling)
    dp = _as_display(display)
    if dp is not None:
        if motion is not None:
            raise ValueError("display and motion do not go together in render_scene")
        check(lib().mcpt_render_scene_display(path.encode(), filename.encode(), N_ray_per_pixel, C.byref(o), C.sizeof(o),
                                              C.byref(_as_lens(lens)) if lens is not None else None,
                                              environment.encode() if environment is not None else None, float(environment_scale),
                                              C.byref(ls) if ls is not None else None, C.byref(dp), st))
        del keep_w
    elif ls is not None:
        if motion is not None:
            raise ValueError("light_sampling and motion do not go together in render_scene")
        check(lib().mcpt_render_scene_lights(path.encode(), filename.encode(), N_ray_per_pixel, C.byref(o), C.sizeof(o),
                                             C.byref(_as_lens(lens)) if lens is not None else None,
                                             environment.encode() if environment is not None else None, float(environment_scale), C.byref(ls), st))
        del keep_w
    elif motion is not None:
        sh = _shutter(motion.get("shutter", (0.0, 1.0)), motion.get("steps", 1))
        end_obj, end_camera = motion.get("end_obj"), motion.get("end_camera")
        check(lib().mcpt_render_scene_motion(path.encode(), filename.encode(), N_ray_per_pixel, C.byref(o), C.sizeof(o),
                                             C.byref(_as_lens(lens)) if lens is not None else None,
                                             environment.encode() if environment is not None else None, float(environment_scale),
                                             end_obj.encode() if end_obj else None, end_camera.encode() if end_camera else None, C.byref(sh), st))
    elif environment is not None:
        check(lib().mcpt_render_scene_env(path.encode(), filename.encode(), N_ray_per_pixel, C.byref(o), C.sizeof(o),
                                          C.byref(_as_lens(lens)) if lens is not None else None, environment.encode(), float(environment_scale), st))
    elif lens is None:
        check(lib().mcpt_render_scene_opts(path.encode(), filename.encode(), N_ray_per_pixel, C.byref(o), C.sizeof(o), st))
    else:
        check(lib().mcpt_render_scene_lens(path.encode(), filename.encode(), N_ray_per_pixel, C.byref(o), C.sizeof(o), C.byref(_as_lens(lens)), st))
    return True
