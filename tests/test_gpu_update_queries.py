"""-m gpu: the read-outs of a scene away from the camera (tests/query_family.py: radiance and irradiance queries, light probes, irradiance
volumes, probe visibility, reflection probes, lightmaps, adaptive queries, baked shading) on a device whose geometry CHANGES.  include/mcpt.h
promises two things about them that their own suites, which run on devices whose geometry never changes, do not execute:

  after mcpt_device_update_vertices -- a refit or a rebuild -- every call answers as a device made fresh from the moved scene would: section
      "after an update" runs the whole family on a device BEFORE the update (so that every workspace, table and stored normal exists and was
      made for another geometry) and after it, and compares the second observation with a fresh device's on the moved files
      (tests/anim_scenes.py), key by key; then the radiance member against the CPU oracle's orc_ray_radiance loaded from the same files;
  under a motion everything that is not a motion frame sees key 0: section "under a motion" sends the geometry away with a motion frame before
      EVERY member, so that each entry point has to find its own way home, and interposes the members between the steps of a progressive
      handle, which then has to find its way back to its shutter step.

Every comparison is bit for bit (np.array_equal on the bit patterns; the messages count the differing words), except the oracle's, which keeps
the helpers, the relative bar and the flip allowance of tests/test_gpu_query_oracle.py as they are.

Measured on an MI355X on 2026-10-20 (the figures the tests print): 0 words differ in every comparison; mirrored, cornell-box's back-face
counts move at 13 of 13 probes and 11 of 12 grid probes (validity at 7 and 4), the probe inside the table from 17 to 127 of 256; the oracle
has 0 of 771 samples over 1e-9 in every row, largest relative error 1.0e-13 (glassroom, 33 on-surface paths).  A library built without
device_face_normals in update_geometry fails 61 of the 72 cases, one built without mcpt_query_visibility's motion_home exactly the four of
probe_visibility and bake_volume_visibility.  The file runs in 4.1 s (tests/test_gpu_update.py: 25.2 s)."""
import ctypes as C
import os

import numpy as np
import pytest

import anim_scenes as A
import env_scenes
import light_pick_ref as LP
import light_tree_ref as LT
import query_family as QF
import test_gpu_motion as TM
import test_gpu_query_oracle as TQ
import test_gpu_update as TU

pytestmark = pytest.mark.gpu

SIZE = (QF.W, QF.H)
BUILDS = TU.BUILDS
_clean_env = TU._clean_env                              # (autouse here as there: no engine knob of the caller's reaches a device)
_fresh = {}                                             # (scene, deformation, extra state, build) -> what a fresh device answers

# scene, deformation, extra state on both devices, build mode, update modes
ROWS = [("cornell-box", "rigid", None, "device_fast", ("refit", "rebuild")),
        ("cornell-box", "mirror", None, "host", ("refit", "rebuild")),
        ("cornell-box", "degenerate", None, "device_sah", ("refit",)),
        ("glassroom", "sine", "sky", "device", ("refit", "rebuild")),
        ("veach-mis", "lights", "tree", "device_fast", ("refit", "rebuild")),
        ("veach-mis", "lights", "one", "device_fast", ("refit",))]
CASES = [(name, what, extra, build, mode) for name, what, extra, build, modes in ROWS for mode in modes]
IDS = ["%s-%s-%s-%s" % (c[0], c[1], c[2] or "plain", c[4]) for c in CASES]
CHAIN = [("path1", "refit"), ("path2", "refit"), ("path3", "rebuild"), ("rigid", "refit")]


def dress(dev, extra):
    if extra == "sky":
        dev.set_environment(*env_scenes.SKIES["map"])
    elif extra in ("tree", "one"):
        dev.set_light_sampling(extra)
    return dev


def samples(dev, q):
    """the radiance member sample by sample: x [n, spp, 3] and hits [n, spp] of spp = 1 queries at the member's own sample indices"""
    x, hits = np.zeros((QF.N_RAYS, QF.RAY_SPP, 3)), np.zeros((QF.N_RAYS, QF.RAY_SPP), dtype=np.int32)
    for j in range(QF.RAY_SPP):
        x[:, j], err, hits[:, j] = dev.radiance(q["rays"], 1, QF.SEED, ids=q["ids"], sample_base=QF.RAY_BASE + j)
        assert not err.any()
    return x, hits


def geometry(mcpt, name, what, tmp_factory):
    return TU.base(mcpt, name, tmp_factory, size=SIZE)[1] if what is None else TU.deform(mcpt, name, what, tmp_factory)


def fresh(mcpt, name, what, extra, build, tmp_factory):
    """what a device made fresh from the scene's files -- moved by `what`, or as they are -- answers: the observation and the radiance
    member's samples, made once per module"""
    key = (name, what, extra, build)
    if key not in _fresh:
        v = geometry(mcpt, name, what, tmp_factory)
        if what is None:
            sc, dev = None, mcpt.Device(TU.base(mcpt, name, tmp_factory, size=SIZE)[0], 0, build=BUILDS[build])
        else:
            sc, dev = TU.fresh(mcpt, name, what, BUILDS[build], tmp_factory, size=SIZE)
            assert TU.same(sc.faces()[0][:, :9], v), "the moved files do not hold the moved vertices"
        dress(dev, extra)
        _fresh[key] = {"obs": QF.observe(mcpt, dev, v), "samples": samples(dev, QF.lists(mcpt, v))}
        dev.close()
        if sc is not None:
            sc.close()
    return _fresh[key]


def assert_changed(after, before, what):
    """the test could have failed: no member of the family answers the moved geometry as it answered the one before (none is allowed to)"""
    stayed = QF.unchanged(after, before)
    assert stayed == [], "%s: %s did not change with the geometry" % (what, stayed)


# ============================================================================================== after an update
@pytest.mark.parametrize("name,what,extra,build,mode", CASES, ids=IDS)
def test_updated_device_answers_as_a_fresh_one(mcpt, name, what, extra, build, mode, tmp_path_factory):
    """one row of the table: the family on the unmoved device, the update, the family again -- equal to the fresh device's of the moved files
    in every word, and different from the unmoved device's in every member"""
    sc, v, _, _ = TU.base(mcpt, name, tmp_path_factory, size=SIZE)
    dev = dress(mcpt.Device(sc, 0, build=BUILDS[build]), extra)
    before = QF.observe(mcpt, dev, v)
    QF.assert_same(before, fresh(mcpt, name, None, extra, build, tmp_path_factory)["obs"], "%s unmoved" % name)
    nv = geometry(mcpt, name, what, tmp_path_factory)
    info = dev.update_vertices(nv, mode=mode)
    assert info["mode"] == (0 if mode == "refit" else 1) and info["fast_enabled"] == 1
    after = QF.observe(mcpt, dev, nv)
    dev.close()
    QF.assert_same(after, fresh(mcpt, name, what, extra, build, tmp_path_factory)["obs"], "%s %s %s %s" % (name, what, extra, mode))
    assert_changed(after, before, "%s %s" % (name, what))
    for k in ("radiance", "irradiance", "sh_probes", "bake_volume", "bake_reflection_probes", "bake_lightmap", "baked_radiance", "render_baked"):
        assert after[k][0].max() > 0, k                                         # (light arrives: the bits compared are not all zero)
    print("valid probes: %d of %d and %d of %d; lit samples of the baked frame: %d" % (
        int(after["probe_visibility"][3].sum()), QF.N_VIS, int(after["bake_volume_visibility"][3].sum()), after["bake_volume_visibility"][3].size,
        int(after["render_baked"][2].sum())))
    if what == "mirror":
        # the fold counts back-face hits by the STORED normal of the hit triangle: the body turned inside out changes the counts
        for k in ("probe_visibility", "bake_volume_visibility"):
            a, b = after[k][2].reshape(-1), before[k][2].reshape(-1)
            assert (a != b).sum() >= 1, k
            print("%s: the back-face counts differ at %d of %d probes, validity at %d" % (k, int((a != b).sum()), a.size,
                                                                                           int((after[k][3] != before[k][3]).sum())))


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_a_probe_inside_the_mirrored_table_changes_its_validity(mcpt, mode, tmp_path_factory):
    """cornell-box's walls and table are wound so that from the room most hits count as back-face hits (the stored normal is
    (v1 - v2) x (v3 - v1)); at the point 22 %, 64 %, 81 % into the table's bounds 9 % of the sphere's directions do before the table is
    mirrored and 49 % after (the CPU oracle's closest hits of 8192 uniform directions), on either side of max_back_fraction = 0.25 by more
    than ten standard deviations of a count over 256 rays.  The update back to the first geometry brings the first answer back."""
    name = "cornell-box"
    sc, v, m, _ = TU.base(mcpt, name, tmp_path_factory, size=SIZE)
    nv = geometry(mcpt, name, "mirror", tmp_path_factory)
    table = np.flatnonzero((nv != v).any(axis=1))
    lo, hi = v[table].reshape(-1, 3).min(axis=0), v[table].reshape(-1, 3).max(axis=0)
    p = (lo + (hi - lo) * np.array([0.22, 0.64, 0.81])).reshape(1, 3)
    ask = lambda d: d.probe_visibility(p, 256, res=4, max_distance=1.0, seed=QF.SEED)
    dev = mcpt.Device(sc, 0)
    first = ask(dev)
    dev.update_vertices(nv, mode=mode)
    second = ask(dev)
    fsc, fdev = TU.fresh(mcpt, name, "mirror", None, tmp_path_factory, size=SIZE)
    assert QF.differing(second, ask(fdev))[0] == 0
    print("back-face hits of 256: %d before, %d mirrored" % (first[2][0], second[2][0]))
    assert first[2][0] < 64 < second[2][0] and (first[3][0], second[3][0]) == (1, 0)
    dev.update_vertices(v, mode=mode)
    assert QF.differing(ask(dev), first)[0] == 0
    for h in (fdev, fsc, dev):
        h.close()


@pytest.mark.parametrize("mode", ["refit", "rebuild"])
def test_a_mirrored_closed_body_turns_its_probes_valid(mcpt, mode):
    """tests/test_gpu_visibility.py's closed cube with outward faces in a closed room: by the winding alone every ray from inside the cube
    hits a back face and no ray from the room does.  Mirrored, the cube has inward faces: its inside is valid with no back-face hit at all,
    and a probe in the room counts exactly the rays that reach the cube."""
    import test_gpu_visibility as TV
    room, cube = TV._box((0, 0, 0), (3, 3, 3), inward=True), TV._box((1, 1, 1), (2, 2, 2), inward=False)
    sc = TV._scene(mcpt, [room, cube])
    v = np.ascontiguousarray(sc.faces()[0][:, :9])
    nv = A.mirror(v, np.arange(12, 24))
    outward = lambda x: (A.face_normals(x[12:]) * (x[12:].reshape(-1, 3, 3).mean(axis=1) - 1.5)).sum(axis=1)
    assert (outward(v) > 0).all() and (outward(nv) < 0).all() and np.array_equal(nv[:12], v[:12])
    rng =np.random.default_rng(8)
    inside = 1.05 + 0.9 * rng.random((33, 3))
    outside = 0.05 + 2.9 * rng.random((400, 3))
    outside = outside[((outside < 0.95) | (outside > 2.05)).any(axis=1)][:70]
    p = np.ascontiguousarray(np.concatenate([inside, outside]))
    spp = 96
    ask = lambda d: d.probe_visibility(p, spp, res=8, max_distance=1.0, seed=5, workspace_rays=1000)
    dev = mcpt.Device(sc, 0)
    m0, hits0, back0, valid0 = ask(dev)
    assert np.array_equal(back0[:33], np.full(33, spp)) and not valid0[:33].any() and not back0[33:].any() and valid0[33:].all()
    dev.update_vertices(nv, mode=mode)
    got = ask(dev)
    fsc = TV._scene(mcpt, [room, (nv[12:], cube[1])])
    assert TU.same(fsc.faces()[0][:, :9], nv)
    fdev = mcpt.Device(fsc, 0)
    want = ask(fdev)
    n, of = QF.differing(got, want)
    assert n == 0, "%d of %d words differ from the fresh device's" % (n, of)
    m1, hits1, back1, valid1 = got
    assert np.array_equal(hits1, np.full(p.shape[0], spp)) and not back1[:33].any() and valid1[:33].all()
    # from the room: a ray meets the cube's faces first or a wall; the faces now count as back faces.  What reaches the cube is what the
    # oracle-checked closest hits of the same device say: ray_intersect over sh_probe_rays, the rays the fold traces
    ids = np.repeat(np.arange(p.shape[0]), spp)
    rays = dev.sh_probe_rays(p[ids], 5, np.tile(np.arange(spp), p.shape[0]), ids=ids)
    face = dev.ray_intersect(rays)[0].reshape(p.shape[0], spp)
    assert (face[:33] >= 12).all()                                              # (from inside, the cube's own faces, now seen from their front)
    assert np.array_equal(back1[33:], (face[33:] >= 12).sum(axis=1).astype(np.int32)) and back1[33:].max() > 0
    for h in (fdev, fsc, dev, sc):
        h.close()


def test_a_chain_of_updates(mcpt, tmp_path_factory):
    """refit, refit, rebuild, refit on ONE device, the family after every link against the fresh device of that link's files"""
    name, build = "cornell-box", "device_fast"
    sc, v, _, _ = TU.base(mcpt, name, tmp_path_factory, size=SIZE)
    dev = mcpt.Device(sc, 0, build=BUILDS[build])
    last = QF.observe(mcpt, dev, v)
    for what, mode in CHAIN:
        nv = geometry(mcpt, name, what, tmp_path_factory)
        dev.update_vertices(nv, mode=mode)
        got = QF.observe(mcpt, dev, nv)
        QF.assert_same(got, fresh(mcpt, name, what, None, build, tmp_path_factory)["obs"], "chain: %s after %s" % (what, mode))
        assert_changed(got, last, "chain %s" % what)
        last = got
    dev.close()


# ---------------------------------------------------------------------------------------------- the oracle behind it
def oracle_samples(mcpt, oracle, name, what, extra, tmp_factory):
    """orc_ray_radiance of the radiance member's rays on the moved files, under the row's sky or light pick: x, hit, on [n, spp(, 3)]"""
    key = ("oracle", name, what, extra)
    if key not in _fresh:
        d, f = TU.moved_files(mcpt, name, what, tmp_factory)
        osc = oracle.OracleScene(d + f, texture_dir=d, width=SIZE[0], height=SIZE[1])
        sc = mcpt.Scene(d, f, width=SIZE[0], height=SIZE[1])
        if extra == "sky":
            assert osc.set_environment(*env_scenes.SKIES["map"]) > 0
        elif extra == "one":
            osc.set_light_pick(1, pick_ref=LP.PickRef.of_scene(sc))
        elif extra == "tree":
            osc.set_light_pick(2, tree_ref=LT.TreeRef.of_scene(sc))
        q = QF.lists(mcpt, geometry(mcpt, name, what, tmp_factory))
        x, hit, on = np.zeros((QF.N_RAYS, QF.RAY_SPP, 3)), np.zeros((QF.N_RAYS, QF.RAY_SPP), dtype=bool), np.zeros((QF.N_RAYS, QF.RAY_SPP), dtype=bool)
        for j in range(QF.RAY_SPP):
            x[:, j], hit[:, j], on[:, j] = osc.ray_radiance(QF.SEED, q["rays"], QF.RAY_BASE + j, ids=q["ids"])
        _fresh[key] = (x, hit, on)
        sc.close()
        osc.close()
    return _fresh[key]


@pytest.mark.parametrize("name,what,extra,build,mode", CASES, ids=IDS)
def test_the_oracle_agrees_after_the_update(mcpt, oracle, name, what, extra, build, mode, tmp_path_factory):
    """the radiance member's samples after the update against orc_ray_radiance on the moved files, through test_gpu_query_oracle's _check (hits
    exact, REL_TOL and the flip allowance of test_gpu_parity.py); the fresh device goes through the same check first, so that a failure of
    the second points at the update and not at the ray list"""
    x, hit, on = oracle_samples(mcpt, oracle, name, what, extra, tmp_path_factory)
    flat = lambda a: a.reshape((QF.N_RAYS * QF.RAY_SPP,) + a.shape[2:])
    f = fresh(mcpt, name, what, extra, build, tmp_path_factory)
    what_ = "%s %s %s" % (name, what, extra)
    TQ._check(what_ + ", the fresh device", "update", flat(f["samples"][0]), flat(f["samples"][1]), flat(x), flat(hit), flat(on))
    sc, v, _, _ = TU.base(mcpt, name, tmp_path_factory, size=SIZE)
    dev = dress(mcpt.Device(sc, 0, build=BUILDS[build]), extra)
    samples(dev, QF.lists(mcpt, v))
    nv = geometry(mcpt, name, what, tmp_path_factory)
    dev.update_vertices(nv, mode=mode)
    gx, ghits = samples(dev, QF.lists(mcpt, nv))
    dev.close()
    TQ._check(what_ + ", updated by a " + mode, "update", flat(gx), flat(ghits), flat(x), flat(hit), flat(on))
    assert QF.differing((gx, ghits), f["samples"])[0] == 0
    # the member itself is the fold of these samples (tests/query_cases.py: fold), to the bar of the samples
    mean, err = TQ.QC.fold(x)
    got = f["obs"]["radiance"]
    keep = (TQ._rel(f["samples"][0], x) <= TQ.TE.REL_TOL).all(axis=1)
    scale = np.maximum(np.abs(x).max(axis=(1, 2)), 1e-12)
    assert (np.abs(got[0] - mean).max(axis=1) / scale)[keep].max() <= TQ.TE.REL_TOL and (np.abs(got[1] - err).max(axis=1) / scale)[keep].max() <= TQ.TE.REL_TOL
    assert np.array_equal(got[2], hit.sum(axis=1).astype(np.int32)) and mean.max() > 0


# ============================================================================================== under a motion
N, STEPS, FRAME_SEED = 12, 3, 5


def _upload(hip_rt, a):
    a = np.ascontiguousarray(a)
    b = hip_rt.DeviceBuffer(max(a.nbytes, 8))
    hip_rt.check(hip_rt.hip().hipMemcpy(b.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes, 1))
    return b


def _download(stream, *pairs):
    for buf, out in pairs:
        buf.to_host_async(out, stream.h)
    stream.synchronize()


def plain(mcpt, dev, q, name, baked=None):
    """what is not a query but reads the geometry or the camera all the same"""
    if name == "ray_intersect":
        return tuple(dev.ray_intersect(q["rays"]))
    if name == "camera_rays":
        pix = np.arange(0, SIZE[0] * SIZE[1], 7, dtype=np.int32)
        return (dev.camera_rays(FRAME_SEED, pix, (pix % 3).astype(np.int32)),)
    if name == "vertices":
        return (dev.vertices(),)
    if name == "bvh_nodes":
        return tuple(dev.bvh_nodes())
    raise KeyError(name)


def device_form(mcpt, dev, q, name, baked):
    """the _device forms the binding exposes, between device buffers on a side stream: the arrays the host form of the same name returns"""
    import hip_rt
    from montecarlopathtracing_amd import _lib
    hip_rt.set_device(0)
    st = hip_rt.Stream()
    bufs = []

    def buf(nbytes):
        bufs.append(hip_rt.DeviceBuffer(nbytes))
        return bufs[-1]

    def up(a):
        bufs.append(_upload(hip_rt, a))
        return bufs[-1]
    try:
        if name == "bake_reflection_probes_device":
            n, T = QF.N_REFL, QF.REFL_RES ** 2
            d_p, d_rad, d_err, d_hits = up(q["refl_probes"]), buf(n * T * 24), buf(n * T * 24), buf(n * T * 4)
            dev.bake_reflection_probes_device(d_p.ptr, n, d_rad.ptr, QF.REFL_RES, QF.REFL_SPP, seed=QF.SEED, workspace_rays=QF.REFL_WORKSPACE,
                                              d_stderr_ptr=d_err.ptr, d_hits_ptr=d_hits.ptr, stream=st.h)
            rad, err, hits = np.zeros((n, T, 3)), np.zeros((n, T, 3)), np.zeros((n, T), dtype=np.int32)
            _download(st, (d_rad, rad), (d_err, err), (d_hits, hits))
            return rad, err, hits
        g = q["grid"]
        vis = mcpt.volume_visibility(QF.GRID_VIS_RES, q["grid_distance"], normal_bias=0.01 * q["grid_distance"])
        src = _lib.BakedSource()
        src.kind, src.grid, src.visibility = mcpt.BAKED_VOLUME, C.pointer(g), C.pointer(vis)
        src.sh27, src.moments = up(baked["bake_volume"][0]).ptr, up(baked["bake_volume_visibility"][0]).ptr
        src.valid = up(baked["bake_volume_visibility"][3]).ptr
        if name == "baked_radiance_device":
            n = QF.N_RAYS
            d_rays, d_rad, d_kind, d_face, d_lit = up(q["rays"]), buf(n * 24), buf(n * 4), buf(n * 4), buf(n * 4)
            o = _lib.BakedOutputs()
            o.radiance3, o.kind, o.face, o.lit = d_rad.ptr, d_kind.ptr, d_face.ptr, d_lit.ptr
            dev.baked_radiance_device(d_rays.ptr, n, src, o, face_viewer=True, stream=st.h)
            rad, kind, face, lit = np.zeros((n, 3)), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
            _download(st, (d_rad, rad), (d_kind, kind), (d_face, face), (d_lit, lit))
            return rad, kind, face, lit
        if name == "render_baked_device":
            w, h = SIZE
            d_img, d_counts, d_lit = buf(w * h * 24), buf(w * h * 12), buf(w * h * 4)
            dev.render_baked_device(src, d_img.ptr, samples=QF.FRAME_SAMPLES, seed=QF.SEED, face_viewer=True, d_counts_ptr=d_counts.ptr,
                                    d_lit_ptr=d_lit.ptr, stream=st.h)
            img, counts, lit = np.zeros((h, w, 3)), np.zeros((h, w, 3), dtype=np.int32), np.zeros((h, w), dtype=np.int32)
            _download(st, (d_img, img), (d_counts, counts), (d_lit, lit))
            return img, counts, lit
        raise KeyError(name)
    finally:
        st.synchronize()
        for b in bufs:
            b.free()
        st.destroy()


PLAIN = ("ray_intersect", "camera_rays", "vertices", "bvh_nodes")
# a device form and where the host form of F0 holds the same arrays
DEVICE_FORMS = {"bake_reflection_probes_device": lambda f: f["bake_reflection_probes"][:3],
                "baked_radiance_device": lambda f: tuple(f["baked_radiance"][i] for i in (0, 1, 2, 7)),
                "render_baked_device": lambda f: f["render_baked"][:3]}
ENTRIES = QF.MEMBERS + PLAIN + tuple(DEVICE_FORMS)


def call(mcpt, dev, q, name, F0):
    """one entry point alone on the device, and what F0 holds for it"""
    if name in QF.MEMBERS:
        return QF.run(mcpt, dev, q, name, F0), F0[name]
    if name in PLAIN:
        return plain(mcpt, dev, q, name), F0[name]
    return device_form(mcpt, dev, q, name, F0), DEVICE_FORMS[name](F0)


def assert_entry(got, want, what):
    assert len(got) == len(want), what
    n, of = QF.differing(got, want)
    assert n == 0, "%s: %d of %d words differ from key 0's answer" % (what, n, of)


class MotionWorld:
    """cornell-box, F0 = everything a device without a motion answers, and one device under a motion of the table and the camera"""

    def __init__(self, mcpt, tmp_factory, geometry_moves=True):
        self.sc, self.v0, _, _ = TU.base(mcpt, "cornell-box", tmp_factory, size=SIZE)
        self.v1 = geometry(mcpt, "cornell-box", "rigid", tmp_factory)
        i = self.sc.info
        cam = {"eye": np.array(i.eye), "look_at": np.array(i.look_at), "up": np.array(i.up), "fovy": float(i.fovy)}
        self.cam1 = TM.moved_camera(cam, self.v0)
        self.q = QF.lists(mcpt, self.v0)
        self.dev = mcpt.Device(self.sc, 0)
        self.F0 = QF.observe(mcpt, self.dev, self.v0)
        for name in PLAIN:
            self.F0[name] = plain(mcpt, self.dev, self.q, name)
        self.static = self.dev.generateImg(N, seed=FRAME_SEED)
        self.dev.set_motion(v_end=self.v1 if geometry_moves else None, camera_end=self.cam1, shutter=(0.0, 1.0), steps=STEPS)
        self.geometry_moves = geometry_moves

    def away(self):
        """a motion frame: the geometry is left at the last shutter step"""
        img = self.dev.generateImg(STEPS, seed=FRAME_SEED)
        info = self.dev.motion_info()
        assert info["steps_run"] == STEPS and (info["ms_updates"] > 0) == self.geometry_moves
        return img


def _world(mcpt, tmp_factory, geometry_moves):
    saved = {k: os.environ.pop(k) for k in TU.KNOBS if k in os.environ}
    try:
        return MotionWorld(mcpt, tmp_factory, geometry_moves)
    finally:
        os.environ.update(saved)


@pytest.fixture(scope="module")
def world(mcpt, tmp_path_factory):
    w = _world(mcpt, tmp_path_factory, True)
    yield w
    w.dev.close()


@pytest.fixture(scope="module")
def camera_world(mcpt, tmp_path_factory):
    w = _world(mcpt, tmp_path_factory, False)
    yield w
    w.dev.close()


def test_before_any_frame_a_motion_changes_nothing(mcpt, tmp_path_factory):
    """(a) set_motion alone: the family and the plain read-outs answer as before it"""
    w = _world(mcpt, tmp_path_factory, True)
    got = QF.observe(mcpt, w.dev, w.v0)
    for name in PLAIN:
        got[name] = plain(mcpt, w.dev, w.q, name)
    QF.assert_same(got, w.F0, "a motion set, no frame rendered")
    assert w.dev.motion_info()["steps_run"] == 0
    w.dev.close()


@pytest.mark.parametrize("name", ENTRIES)
def test_every_entry_point_finds_its_own_way_home(mcpt, world, name):
    """(b) a motion frame leaves the geometry at the last shutter step; the entry point called next, alone, answers from key 0"""
    world.away()
    got, want = call(mcpt, world.dev, world.q, name, world.F0)
    assert_entry(got, want, "%s after a motion frame" % name)


def test_the_motion_is_still_there(mcpt, world):
    """(c) after every entry point's return home: the same motion, the same motion frame, and a frame unlike the static one"""
    first = world.away()
    for name in ENTRIES:
        world.away()
        call(mcpt, world.dev, world.q, name, world.F0)
    m = world.dev.motion
    assert m["steps"] == STEPS and m["shutter"] == (0.0, 1.0) and m["has_geometry"] and m["has_camera"]
    assert TU.same(m["camera_end"]["eye"], world.cam1["eye"]) and m["camera_end"]["fovy"] == world.cam1["fovy"]
    assert TU.same(world.away(), first)
    blurred = world.dev.generateImg(N, seed=FRAME_SEED)
    assert not TU.same(blurred, world.static)
    call(mcpt, world.dev, world.q, "radiance", world.F0)
    assert TU.same(world.dev.generateImg(N, seed=FRAME_SEED), blurred)


@pytest.mark.parametrize("name", ENTRIES)
def test_a_progressive_handle_finds_its_shutter_step_again(mcpt, world, name):
    """(d) 12 samples in three passes of 4 -- one shutter step each -- with the entry point called between the passes: it answers from key 0
    and the handle's image and error estimate are those of an uninterrupted handle (which are the one-shot shutter frame's)"""
    dev = world.dev

    def handle(interrupted):
        pr = dev.progressive(N, seed=FRAME_SEED)
        for step in range(3):
            pr.step(4)
            if interrupted and step < 2:
                got, want = call(mcpt, dev, world.q, name, world.F0)
                assert_entry(got, want, "%s between passes %d and %d" % (name, step, step + 1))
        assert pr.done == N
        out = (pr.image(), pr.stderr())
        pr.close()
        return out
    if not hasattr(world, "uninterrupted"):
        world.uninterrupted = handle(False)
        assert TU.same(world.uninterrupted[0], dev.generateImg(N, seed=FRAME_SEED)) and world.uninterrupted[1].max() > 0
    n, of = QF.differing(handle(True), world.uninterrupted)
    assert n == 0, "%s between the passes: %d of %d words of the handle's image and error differ" % (name, n, of)


@pytest.mark.parametrize("name", ["radiance", "bake_reflection_probes", "camera_rays"])
def test_a_camera_only_motion(mcpt, camera_world, name):
    """(e) v_end = None: the frames blend the camera alone; the entry points answer under key 0's"""
    w = camera_world
    frame = w.away()
    got, want = call(mcpt, w.dev, w.q, name, w.F0)
    assert_entry(got, want, "%s after a camera-only motion frame" % name)
    assert TU.same(w.away(), frame) and not TU.same(w.dev.generateImg(N, seed=FRAME_SEED), w.static)


def test_an_update_clears_the_motion(mcpt, tmp_path_factory):
    """(f) new vertices are a new key 0: no motion any more, and the family answers as the fresh device of the new vertices"""
    w = _world(mcpt, tmp_path_factory, True)
    w.away()
    v2 = geometry(mcpt, "cornell-box", "path2", tmp_path_factory)
    w.dev.update_vertices(v2)
    assert w.dev.motion is None and w.dev.motion_info()["steps_run"] == 0
    # (the world's device has the default build mode: the hierarchy only culls, so the fresh device of the chain's build answers the same)
    QF.assert_same(QF.observe(mcpt, w.dev, v2), fresh(mcpt, "cornell-box", "path2", None, "device_fast", tmp_path_factory)["obs"],
                   "an update under a motion")
    w.dev.close()


def test_refused_updates_and_motions_change_nothing(mcpt, tmp_path_factory):
    """(g) what the library refuses -- the cases of test_gpu_update.py's and test_gpu_motion.py's refusal tests -- leaves the device, away at
    a shutter step or at home, answering as before, and the motion in place"""
    w = _world(mcpt, tmp_path_factory, True)
    dev = w.dev
    frame = w.away()
    v2 = geometry(mcpt, "cornell-box", "sine", tmp_path_factory)

    def refused(fn, code=-3):
        with pytest.raises(mcpt.McptError) as e:
            fn()
        assert e.value.code == code, e.value
    pr = dev.progressive(N, seed=FRAME_SEED)
    pr.step(4)                                                                  # (the geometry is at step 0 of the shutter)
    for mode in ("refit", "rebuild"):
        refused(lambda: dev.update_vertices(v2, mode=mode))
    refused(lambda: dev.set_camera([0, 0, 5], [0, 0, 0], [0, 1, 0], 40.0))
    refused(lambda: dev.set_motion(v_end=v2, steps=2))
    refused(dev.clear_motion)
    pr.close()
    with pytest.raises(mcpt.McptError):
        dev.update_vertices(np.int64(0))                                        # a null device pointer
    with pytest.raises(ValueError):
        dev.update_vertices(w.v0[:-1])
    with pytest.raises(ValueError):
        dev.update_vertices(w.v0, mode="other")
    with pytest.raises(ValueError):
        dev.set_motion(v_end=w.v0[:-1], steps=2)
    for eye, look, up, fovy in (([0, 0, 5], [0, 0, 5], [0, 1, 0], 40.0), ([0, 0, 5], [0, 0, 0], [0, 0, 1], 40.0),
                                ([0, 0, 5], [0, 0, 0], [0, 1, 0], 180.0), ([np.nan, 0, 5], [0, 0, 0], [0, 1, 0], 40.0)):
        refused(lambda: dev.set_camera(eye, look, up, fovy))
    refused(lambda: dev.set_motion(v_end=v2, shutter=(0.5, 0.25), steps=2))
    refused(lambda: dev.set_motion(v_end=v2, shutter=(0.0, 1.0), steps=0))
    refused(lambda: dev.set_motion(camera_end={"eye": [0, 0, 5], "look_at": [0, 0, 5], "up": [0, 1, 0], "fovy": 40.0}, steps=2))
    w.away()
    got = QF.observe(mcpt, dev, w.v0)
    for name in PLAIN:
        got[name] = plain(mcpt, dev, w.q, name)
    QF.assert_same(got, w.F0, "after the refusals")
    m = dev.motion
    assert m is not None and m["steps"] == STEPS and m["has_geometry"] and m["has_camera"] and TU.same(m["camera_end"]["eye"], w.cam1["eye"])
    assert TU.same(w.away(), frame)
    dev.close()
