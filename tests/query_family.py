"""One observation of every read-out of a scene away from the camera -- radiance and irradiance queries, light probes, irradiance volumes,
probe visibility, reflection probes, lightmaps, adaptive queries and baked shading -- at the smallest sizes at which the kernels still meet
their edges (more than one workgroup, odd counts, several chunks), for tests that hold a device to another device bit for bit
(tests/test_gpu_update_queries.py).

observe(mcpt, dev, geom) runs the whole family and returns {member: tuple of arrays}; the query lists are derived deterministically from
geom, the vertex array [num_faces, 9] the device is meant to hold, and from nothing else -- so two devices that hold the same geometry are
asked the same questions whatever either was asked before.  observe(..., only=name, baked=earlier) runs ONE member and nothing else on the
device (the members that shade from a bake then take the bake from the earlier observation instead of baking)."""
import numpy as np

import anim_scenes as A

W, H = 64, 36
SEED = 0x5EED5EED1234
N_RAYS, RAY_SPP, RAY_BASE = 257, 3, 7
N_POINTS, POINT_SPP = 130, 5
N_PROBES, PROBE_SPP = 9, 65
COUNTS, VOLUME_SPP = (3, 2, 2), 33
N_VIS, VIS_SPP, VIS_RES, VIS_WORKSPACE = 13, 65, 4, 200          # 13 * 65 = 845 rays: five chunks of 200
GRID_VIS_SPP, GRID_VIS_RES = 64, 8
# cornell-box is wound so that from inside the room most hits count as back-face hits (65 % to 99 % of a probe's rays): under the default
# limit of 0.25 no probe of it would be valid and a bake would light nothing; under this one some are and some are not
BACK_FRACTION = 0.9
N_REFL, REFL_RES, REFL_SPP, REFL_WORKSPACE = 2, 5, 3, 23
MAP, MAP_SPP = 16, 4
ADAPTIVE_SPP, ADAPTIVE_MIN, ADAPTIVE_REL = 16, 4, 0.05
FRAME_SAMPLES = 2

# (baked_radiance and render_baked shade from what bake_volume, bake_volume_visibility and bake_lightmap returned: they come last)
MEMBERS = ("radiance", "radiance_reference", "radiance_megakernel", "irradiance", "sh_probes", "bake_volume", "probe_visibility",
           "bake_volume_visibility", "bake_reflection_probes", "bake_lightmap", "radiance_adaptive", "baked_radiance", "render_baked")
COUNTERS = ("samples", "rays_primary", "rays_shadow", "rays_bounce", "shade_calls")     # (node visits belong to the hierarchy, not the answer)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def differing(a, b):
    """the number of words in which two tuples of arrays differ, and the number of words"""
    return sum(int((bits(x) != bits(y)).sum()) for x, y in zip(a, b)), sum(bits(x).size for x in a)


def _unit(d):
    d = d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
    return d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]


def _fractions(n, seed):
    """n points of the unit cube's middle, the same for every geometry"""
    return 0.15 + 0.7 * np.random.default_rng(seed).random((n, 3))


def lists(mcpt, geom):
    """the query lists of a geometry: a dict of arrays made from geom alone"""
    geom = np.ascontiguousarray(geom, dtype=np.float64)
    p = geom.reshape(-1, 3)
    lo, hi = p.min(axis=0), p.max(axis=0)
    rng = np.random.default_rng(41)
    o = lo + (hi - lo) * (0.02 + 0.96 * rng.random((N_RAYS, 3)))
    d = _unit(rng.normal(size=(N_RAYS, 3)))
    d[::29] = np.roll(np.eye(3), 1, axis=1)[np.arange(d[::29].shape[0]) % 3]               # axis-parallel directions among them
    ids = rng.integers(0, 2 ** 31 - 1, size=N_RAYS, endpoint=True).astype(np.int32)
    ids[0] = 2 ** 31 - 1
    # surface points: centroids of faces that have an area, spread over the face list, 1e-3 off the face along its normal -- on either
    # side in turn: which side of a face is the open one depends on the scene's winding, and a point on the other side sees nothing
    nrm = A.face_normals(geom)
    length = np.sqrt((nrm * nrm).sum(axis=1))
    solid = np.flatnonzero(length > 1e-12 * max(float(length.max()), 1e-300))
    faces = solid[(np.arange(N_POINTS) * solid.size) // N_POINTS]
    n = nrm[faces] / length[faces][:, None] * np.where(np.arange(N_POINTS) % 2 == 0, 1.0, -1.0)[:, None]
    x = geom[faces].reshape(-1, 3, 3).mean(axis=1) + 1e-3 * n
    c = np.array(COUNTS)
    grid = mcpt.volume_grid(lo + 0.1 * (hi - lo), 0.8 * (hi - lo) / (c - 1), COUNTS)
    return {"rays": np.ascontiguousarray(np.concatenate([o, d], axis=1)), "ids": ids, "points": np.ascontiguousarray(x), "normals": np.ascontiguousarray(n),
            "point_ids": (np.arange(N_POINTS, dtype=np.int32) * 7919 + 3), "probes": lo + (hi - lo) * _fractions(N_PROBES, 42),
            "vis_probes": lo + (hi - lo) * _fractions(N_VIS, 43), "vis_distance": 0.5 * float(np.linalg.norm(hi - lo)),
            "refl_probes": lo + (hi - lo) * _fractions(N_REFL, 44), "grid": grid,
            "grid_distance": 1.5 * float(np.sqrt(sum(float(s) ** 2 for s in grid.spacing)))}


def _counters(st):
    return np.array([getattr(st, f) for f in COUNTERS], dtype=np.uint64)


def volume_source(mcpt, q, baked):
    """the visibility volume of an observation as a baked source"""
    vis = mcpt.volume_visibility(GRID_VIS_RES, q["grid_distance"], normal_bias=0.01 * q["grid_distance"])
    return mcpt.baked_volume(q["grid"], baked["bake_volume"][0], valid=baked["bake_volume_visibility"][3], moments=baked["bake_volume_visibility"][0], vis=vis)


def lightmap_source(mcpt, baked):
    E, _, _, owner = baked["bake_lightmap"][:4]
    return mcpt.baked_lightmap(E, uv=None, owner=owner)


def _baked_tuple(out):
    return tuple(out[k] for k in ("radiance", "kind", "face", "q6", "uv", "kd", "e", "lit"))


def run(mcpt, dev, q, name, baked=None):
    """one member on the device: a tuple of arrays (every float64 one is compared by its bits)"""
    st = mcpt.Stats()
    if name in ("radiance", "radiance_reference", "radiance_megakernel"):
        if name == "radiance_reference":
            dev.set_trace_mode(mcpt.TRACE_REFERENCE)
        try:
            out = dev.radiance(q["rays"], RAY_SPP, SEED, ids=q["ids"], sample_base=RAY_BASE,
                               flags=mcpt.RENDER_MEGAKERNEL if name == "radiance_megakernel" else 0, stats=st)
        finally:
            if name == "radiance_reference":
                dev.set_trace_mode(mcpt.TRACE_FAST)
    elif name == "irradiance":
        out = dev.irradiance(q["points"], q["normals"], POINT_SPP, SEED, ids=q["point_ids"], stats=st)
    elif name == "sh_probes":
        out = dev.sh_probes(q["probes"], PROBE_SPP, SEED, stats=st)
    elif name == "bake_volume":
        out = dev.bake_volume(q["grid"], VOLUME_SPP, seed=SEED, stats=st)
    elif name == "probe_visibility":
        out = dev.probe_visibility(q["vis_probes"], VIS_SPP, res=VIS_RES, max_distance=q["vis_distance"], max_back_fraction=BACK_FRACTION, seed=SEED,
                                   workspace_rays=VIS_WORKSPACE, stats=st)
    elif name == "bake_volume_visibility":
        out = dev.bake_volume_visibility(q["grid"], GRID_VIS_SPP, res=GRID_VIS_RES, max_distance=q["grid_distance"], max_back_fraction=BACK_FRACTION, seed=SEED,
                                         stats=st)
    elif name == "bake_reflection_probes":
        out = dev.bake_reflection_probes(q["refl_probes"], REFL_RES, REFL_SPP, seed=SEED, workspace_rays=REFL_WORKSPACE, stats=st)
    elif name == "bake_lightmap":
        out = dev.bake_lightmap(MAP, MAP, MAP_SPP, seed=SEED, stats=st)
    elif name == "radiance_adaptive":
        out = dev.radiance_adaptive(q["rays"], ADAPTIVE_SPP, ADAPTIVE_REL, min_spp=ADAPTIVE_MIN, seed=SEED, ids=q["ids"], stats=st)
    elif name == "baked_radiance":
        a = dev.baked_radiance(q["rays"], volume_source(mcpt, q, baked), face_viewer=True, stats=st)
        b = dev.baked_radiance(q["rays"], lightmap_source(mcpt, baked))
        return _baked_tuple(a) + _baked_tuple(b) + (_counters(st),)
    elif name == "render_baked":
        f = dev.render_baked(volume_source(mcpt, q, baked), samples=FRAME_SAMPLES, seed=SEED, face_viewer=True, stats=st)
        return (f["image"], f["counts"], f["lit"], _counters(st))
    else:
        raise KeyError(name)
    return tuple(out) + (_counters(st),)


def observe(mcpt, dev, geom, only=None, baked=None):
    q = lists(mcpt, geom)
    if only is not None:
        return {only: run(mcpt, dev, q, only, baked)}
    out = {}
    for name in MEMBERS:
        out[name] = run(mcpt, dev, q, name, out)
    return out


def assert_same(got, want, what):
    """key by key, bit for bit; the message counts the differing words"""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in got:
        assert len(got[k]) == len(want[k]), (what, k)
        for i, (x, y) in enumerate(zip(got[k], want[k])):
            assert bits(x).shape == bits(y).shape and bits(x).dtype == bits(y).dtype, (what, k, i)
            n = int((bits(x) != bits(y)).sum())
            assert n == 0, "%s: %s[%d] differs in %d of %d words" % (what, k, i, n, bits(x).size)


def unchanged(a, b):
    """the members of two observations that are equal in every word"""
    return sorted(k for k in a if differing(a[k], b[k])[0] == 0)
