"""-m gpu: the pool trace engine's refill reads slot flags first and fetches only the rays it takes (trace_pool.hpp, refill_window.hpp).

A refill of a sparse source (the wavefront's path state: bounce slots that Russian roulette emptied, shadow slots whose light is behind
the surface) looks at the flags of a window of up to 128 slots, hands the window's rays in slot order to the lanes that claimed a pool
slot, and each of those lanes loads the one ray it will walk.  Which ray goes to which lane changes nothing about a ray's walk, so every
case holds a frame of the pool engine bit for bit to the megakernel's (one lane per sample, no path state, no refill; pinned to the
oracle by test_gpu_parity.py), and cornell-box also to the CPU oracle by smoke()'s criterion.  64 x 48 frames unless a case says otherwise:

1. SPP 1, 3, 63, 64, 65, 192 (windows that straddle the runs of a pixel's samples; spp % 64 != 0: the first pass does not order bounce
   rays first, so empty slots sit anywhere in a window), with one light (cornell-box) and three (tests/light_scenes.py), hand-over to
   the finishing pass never, at depth 0 and at depth 1;
2. n_paths of 1, 63, 64, 65, 127, 128, 129 (small frames x SPP): windows and tickets that end inside the first or second half of a
   window, a plane shorter than a window, windows that run across the plane boundary;
3. the smallest chunk the launch knobs allow (64 slots per ticket): every window ends at its range's end;
4. an empty plane: a floor lit from below -- the only light is behind every surface, every shadow slot is empty (rays_shadow == 0) --
   must drain and the launch must end;
5. a full plane: glassroom (mirrors and glass: nearly every bounce slot holds a ray);
6. the work counters of one frame (SPP 65, every bounce through k_wf_trace_pool), recorded from the commit before the change by
   tests/make_pool_window_refill_golden.py into tests/golden/pool_window_refill_counts.json."""
import json
import os

import numpy as np
import pytest

import light_scenes
import make_pool_window_refill_golden as G
from conftest import SCENES, extra_scene_dir

pytestmark = pytest.mark.gpu

W, H, SEED = G.W, G.H, G.SEED
SPPS = (1, 3, 63, 64, 65, 192)
BIG = "1000000000"
# hand-over -> (knobs, trace launches before it or None)
HANDOVER = {"never": (G.WAVEFRONT, None), "depth0": ({"MCPT_FINISH_PATHS": BIG}, 0), "depth1": ({}, 1)}
# (n_paths, width, height, spp): every camera ray of these small cornell-box frames ends on a surface that is shaded (asserted)
# (5 x 13: 63 of the 65 pixels, the others look past the box; 8 x 8 and 3 x 3: all of them; the primes and 3 x 43 as one pixel's samples)
CROPS = [(1, 1, 1, 1), (63, 5, 13, 1), (63, 3, 3, 7), (64, 8, 8, 1), (65, 1, 1, 65), (127, 1, 1, 127), (128, 8, 8, 2), (129, 1, 1, 129)]
SMALL_CHUNK = dict(G.WAVEFRONT, MCPT_TRACE_MIN_CHUNK="64", MCPT_TRACE_MAX_CHUNK="64", MCPT_TRACE_BLOCK_RAYS="256")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def floor_lit_from_below():
    """a floor that faces up and a lamp under it that faces up too (synthetic.write_obj's dict): the light is behind every surface"""
    def quad(y, h):
        return np.array([[-h, y, -h, -h, y, h, h, y, h], [-h, y, -h, h, y, h, h, y, -h]], dtype=np.float64)
    v = np.vstack([quad(0.0, 6.0), quad(-3.0, 0.5)])
    e1, e2 = v[:, 3:6] - v[:, 0:3], v[:, 6:9] - v[:, 0:3]
    assert (np.cross(e1, e2)[:, 1] > 0).all()                    # counter-clockwise seen from above
    up = np.tile([0.0, 1.0, 0.0], (4, 3))
    rec = np.array([[0.7, 0.6, 0.5, 0, 0, 0, 1, 1], [0, 0, 0, 0, 0, 0, 1, 1]], dtype=np.float64)
    return dict(v=v, vn=up, material=np.array([0, 0, 1, 1], dtype=np.int32), material_rec=rec, material_names=["floor", "lamp"],
                light_material=np.array([1], dtype=np.int32), light_radiance=np.full((1, 3), 9.0),
                eye=[0.5, 5.0, 8.0], look_at=[0.0, 0.0, 0.0], up=[0.0, 1.0, 0.0], fovy=45.0, width=W, height=H)


class _World:
    def __init__(self, M, tmp):
        self.M, self.dir = M, str(tmp.mktemp("window_refill")) + os.sep
        self.scenes, self.megas = {}, {}

    def scene(self, key, width=W, height=H):
        k = (key, width, height)
        if k not in self.scenes:
            if key == "lights3":
                if not os.path.exists(self.dir + "lights3.obj"):
                    light_scenes.write(self.dir, "lights3", 3, W, H)
                sc = self.M.Scene(self.dir, "lights3", width=width, height=height)
            elif key == "below":
                from montecarlopathtracing_amd import synthetic
                synthetic.write_obj(floor_lit_from_below(), self.dir, "below")
                sc = self.M.Scene(self.dir, "below", width=width, height=height)
            else:
                sc = self.M.Scene(extra_scene_dir() if key == "glassroom" else SCENES, key, width=width, height=height)
            self.scenes[k] = sc
        return self.scenes[k]

    def mega(self, sc, spp):
        """the megakernel frame and the pixels whose camera ray hits something, once per (scene, spp)"""
        k = (id(sc), spp)
        if k not in self.megas:
            dev = G.pool_device(self.M, sc, G.WAVEFRONT)
            try:
                info = sc.info
                n = info.width * info.height
                rays = dev.camera_rays(SEED, np.arange(n, dtype=np.int32), np.zeros(n, dtype=np.int32))
                faces = dev.ray_intersect(rays)[0]
                self.megas[k] = (dev.generateImg(spp, seed=SEED, flags=self.M.RENDER_MEGAKERNEL), faces)
            finally:
                dev.close()
        return self.megas[k]

    def check(self, sc, spp, knobs, launches=None, what=""):
        """one frame on a fresh pool device under `knobs`, equal to the megakernel's bit for bit; returns its stats"""
        mega, _ = self.mega(sc, spp)
        dev = G.pool_device(self.M, sc, knobs)
        st = self.M.Stats()
        try:
            img = dev.generateImg(spp, seed=SEED, stats=st)
        finally:
            dev.close()
        print("%s spp %d %s: launches %d, shadow %d skipped %d bounce %d" % (what, spp, knobs, st.launches, st.rays_shadow, st.shadow_skipped, st.rays_bounce))
        assert np.array_equal(_bits(img), _bits(mega)), "%s spp %d: %d channels differ from the megakernel" % (what, spp, int((_bits(img) != _bits(mega)).sum()))
        if launches is not None:
            assert st.launches == launches, "the hand-over was not at depth %d: %d trace launches before it" % (launches, st.launches)
        return st

    def close(self):
        for sc in self.scenes.values():
            sc.close()


@pytest.fixture(scope="module")
def world(mcpt, tmp_path_factory):
    w = _World(mcpt, tmp_path_factory)
    yield w
    w.close()


# ------------------------------------------------------------------------------------------------------- 1: SPP, lights, hand-over
@pytest.mark.parametrize("handover", list(HANDOVER))
@pytest.mark.parametrize("key", ["cornell-box", "lights3"])
def test_sample_counts_lights_and_handover(world, key, handover):
    knobs, launches = HANDOVER[handover]
    sc = world.scene(key)
    for spp in SPPS:
        if handover == "depth1":
            # the first pass leaves hit pixels x spp paths less the few on emitters, the depth-1 pass at most 0.6 of them and what the
            # binomial adds: a threshold of 0.7 lies between (test_gpu_bounce_first.py's)
            hit = int((world.mega(sc, spp)[1] >= 0).sum())
            knobs = {"MCPT_FINISH_PATHS": str(max(1, int(0.7 * hit * spp)))}
        st = world.check(sc, spp, knobs, launches, "%s %s" % (key, handover))
        if launches is None:
            assert st.launches >= 3, st.launches


def test_cornell_box_against_the_oracle(world, mcpt, oracle):
    """the frame itself (not only the megakernel's) against the CPU oracle, by smoke()'s criterion"""
    sc = world.scene("cornell-box")
    osc = oracle.OracleScene(SCENES + "cornell-box", texture_dir=SCENES, width=W, height=H)
    try:
        for spp in (3, 65):
            ref = osc.render(spp, seed=SEED)
            dev = G.pool_device(mcpt, sc, G.WAVEFRONT)
            try:
                img = dev.generateImg(spp, seed=SEED)
            finally:
                dev.close()
            rel = np.abs(img - ref) / np.maximum(np.abs(ref), 1e-6)
            bad = int((rel > 1e-6).sum())
            print("spp %d: %d channels beyond 1e-6 of the oracle, max rel %.3e" % (spp, bad, rel.max()))
            assert bad <= 3
    finally:
        osc.close()


# ------------------------------------------------------------------------------------------------------- 2: path counts
@pytest.mark.parametrize("n_paths,w,h,spp", CROPS)
def test_path_counts_at_window_and_ticket_edges(world, n_paths, w, h, spp):
    sc = world.scene("cornell-box", w, h)
    _, faces = world.mega(sc, spp)
    _, mat, _ = sc.faces()
    lamps = {sc.light(i)[2] for i in range(sc.info.num_lights)}
    shaded = int(sum(1 for f in faces if f >= 0 and int(mat[f]) not in lamps))
    assert shaded * spp == n_paths, "%d x %d at SPP %d: %d pixels are shaded" % (w, h, spp, shaded)
    world.check(sc, spp, G.WAVEFRONT, None, "n_paths %d" % n_paths)
    world.check(sc, spp, SMALL_CHUNK, None, "n_paths %d, 64-slot tickets" % n_paths)


# ------------------------------------------------------------------------------------------------------- 3: smallest chunk
@pytest.mark.parametrize("key,spp", [("cornell-box", 3), ("cornell-box", 65), ("lights3", 3), ("lights3", 64)])
def test_smallest_chunk(world, key, spp):
    st = world.check(world.scene(key), spp, SMALL_CHUNK, None, "%s 64-slot tickets" % key)
    assert st.launches >= 3


# ------------------------------------------------------------------------------------------------------- 4: an empty plane
@pytest.mark.parametrize("knobs", [G.WAVEFRONT, SMALL_CHUNK], ids=["default-chunk", "64-slot-tickets"])
def test_a_plane_without_a_ray_drains(world, knobs):
    sc = world.scene("below")
    for spp in (3, 65):
        st = world.check(sc, spp, knobs, None, "floor lit from below")
        assert st.rays_shadow == 0 and st.shadow_skipped > 0 and st.rays_bounce > 0, (st.rays_shadow, st.shadow_skipped, st.rays_bounce)
        assert st.launches >= 1


# ------------------------------------------------------------------------------------------------------- 5: a full plane
def test_a_full_plane(world):
    sc = world.scene("glassroom")
    for spp in (3, 64):
        st = world.check(sc, spp, G.WAVEFRONT, None, "glassroom")
        assert st.rays_bounce > 0
    world.check(sc, 3, SMALL_CHUNK, None, "glassroom, 64-slot tickets")


# ------------------------------------------------------------------------------------------------------- 6: work counters
def test_work_counters_are_those_before_the_change(world, mcpt):
    """rays, node visits, triangle tests (of the run and of its dominant kernel) and the exact tests per ray the diagnostics print, as
    recorded from the commit before the change"""
    with open(G.GOLDEN) as f:
        golden = json.load(f)
    assert (golden["scene"], golden["width"], golden["height"], golden["spp"], golden["seed"]) == ("cornell-box", W, H, G.COUNT_SPP, SEED)
    sc = world.scene("cornell-box")
    img, c = G.counted_frame(mcpt, sc)
    print("build", mcpt.build_id(), "golden from", golden["recorded_from_build_id"])
    print(" counts", c)
    print(" golden", golden["counts"])
    assert np.array_equal(_bits(img), _bits(world.mega(sc, G.COUNT_SPP)[0]))
    assert c == golden["counts"]
    assert c["dom_rays"] == c["diag_rays"] > 0 and c["dom_node_visits"] > c["dom_rays"]
