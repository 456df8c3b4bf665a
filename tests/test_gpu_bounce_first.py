"""-m gpu: the path state's two savings (csrc/wave_rank.hpp, vertex.hpp first_vertex_throughput), held bit for bit to the megakernel.

With one shadow plane the first logic pass stores no throughput: whoever reads the T of a pixel's primary hit -- the depth-1 logic pass
(shade round, a specular chain that ends on an emitter, a bounce ray that leaves into the environment) and both finishing kernels
when they adopt at depth 0 -- forms it again from the pixel's PrimarySurface.  And every wave of a logic pass writes its vertices
with a bounce ray first, the first pass too when a pixel's run of spp positions is a whole number of waves.  Neither may change a bit
of a frame: the megakernel (one lane per sample, no path state at all; pinned to the oracle by test_gpu_parity.py) is the answer.

64 x 48 frames.  SPP 1, 3, 64, 65, 128, 192: a wave of the first pass inside one pixel's run (64, 128, 192: ranked) and across several
(1, 3, 65: in lane order), a partial last wave, several pixels per block.  Scenes:
- cornell-box: one light, the folded state (T not stored by the first pass, stored with the bounce ray afterwards);
- three lights (tests/light_scenes.py): the unfolded state (T and the bounce weight stored as before, positions ranked) -- and the
  same scene under pick modes "one" and "tree": one plane again, folded, with the pick's own kernels;
- the open scene under a sky map (tests/env_scenes.py) without a light (one plane, the environment's: folded, the escape of the
  resolve reads the first vertex's T) and with one (two planes); cornell-box under a constant sky.
Routes, each on a device of its own (the knobs are read when it is created): every bounce a logic pass (hand-over off) under the pool
and the voting engine; a two-block logic grid (each block's ring wraps, its rounds follow each other); the hand-over to the finishing
pass forced at depth 0 (MCPT_FINISH_PATHS = 10^9, test_gpu_trace_paths.py's) and at depth 1 (a threshold between the paths the first pass
leaves -- the samples of the pixels whose camera ray hits something, less the few on emitters -- and those the depth-1 pass leaves: Russian
roulette at 0.6 ends 40 % of them, so 70 % of the first pass's lies between), in the pool form and the lane form -- trace launches counted: none before a hand-over at depth 0, one before a hand-over at depth 1.
cornell-box runs every SPP on every route; the other scenes SPP 3, 64 and 65 (either side of the ranked first pass)."""
import os

import numpy as np
import pytest

import env_scenes
import light_scenes
from conftest import SCENES

pytestmark = pytest.mark.gpu

W, H, SEED = 64, 48, 7
SPPS = (1, 3, 64, 65, 128, 192)
SPPS_THIN = (3, 64, 65)
BIG = "1000000000"
KNOBS = ("MCPT_TRACE_ENGINE", "MCPT_FINISH_ENGINE", "MCPT_FINISH_PATHS", "MCPT_WORKSPACE_GB", "MCPT_LOGIC_GRID")
# route -> (knobs, depth of the hand-over or None)
ROUTES = {
    "wavefront-pool": ({"MCPT_TRACE_ENGINE": "pool", "MCPT_FINISH_PATHS": "0"}, None),
    "wavefront-vote": ({"MCPT_TRACE_ENGINE": "vote", "MCPT_FINISH_PATHS": "0"}, None),
    "logic-grid-2": ({"MCPT_LOGIC_GRID": "2", "MCPT_FINISH_PATHS": "0"}, None),
    "finish-pool-depth0": ({"MCPT_TRACE_ENGINE": "pool", "MCPT_FINISH_PATHS": BIG}, 0),
    "finish-lane-depth0": ({"MCPT_TRACE_ENGINE": "pool", "MCPT_FINISH_ENGINE": "lane", "MCPT_FINISH_PATHS": BIG}, 0),
    "finish-pool-depth1": ({"MCPT_TRACE_ENGINE": "pool"}, 1),
    "finish-lane-depth1": ({"MCPT_TRACE_ENGINE": "pool", "MCPT_FINISH_ENGINE": "lane"}, 1),
}
SCENE_KEYS = ["cornell-box", "lights3", "lights3-one", "lights3-tree", "open0-sky", "open1-sky", "cornell-box-sky"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class _World:
    def __init__(self, mcpt, directory):
        self.M, self.dir = mcpt, directory
        self.scenes, self.answers, self.hit_pixels = {}, {}, {}

    def scene(self, key):
        if key not in self.scenes:
            if key.startswith("cornell-box"):
                sc = self.M.Scene(SCENES, "cornell-box", width=W, height=H)
            elif key.startswith("lights3"):
                if not os.path.exists(self.dir + "lights3.obj"):
                    light_scenes.write(self.dir, "lights3", 3, W, H)
                sc = self.M.Scene(self.dir, "lights3", width=W, height=H)
            else:
                name = key.split("-")[0]
                env_scenes.open_scene(self.dir, name, int(name[4:]), W, H)
                sc = self.M.Scene(self.dir, name, width=W, height=H)
            self.scenes[key] = sc
        return self.scenes[key]

    def device(self, key, knobs):
        saved = {k: os.environ.pop(k, None) for k in KNOBS}
        try:
            os.environ.update(knobs)
            sc = self.scene(key)
            if "MCPT_TRACE_ENGINE" in knobs:
                assert sc.trace_engine() == knobs["MCPT_TRACE_ENGINE"]
            dev = self.M.Device(sc, 0)
        finally:
            for k, v in saved.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
        if key.endswith("-one"):
            dev.set_light_sampling("one")
        elif key.endswith("-tree"):
            dev.set_light_sampling("tree")
        elif key == "cornell-box-sky":
            dev.set_environment(*env_scenes.SKIES["constant"])
        elif key.endswith("-sky"):
            dev.set_environment(*env_scenes.SKIES["map"])
        return dev

    def answer(self, key, spp):
        """the megakernel frame, the counts of a run whose every bounce is a logic pass and the pixels whose camera ray hits something; once per
        (scene, spp)"""
        if (key, spp) not in self.answers:
            dev = self.device(key, {"MCPT_FINISH_PATHS": "0"})
            try:
                if key not in self.hit_pixels:
                    rays = dev.camera_rays(SEED, np.arange(W * H, dtype=np.int32), np.zeros(W * H, dtype=np.int32))
                    self.hit_pixels[key] = int((dev.ray_intersect(rays)[0] >= 0).sum())
                st = self.M.Stats()
                frame = dev.generateImg(spp, seed=SEED, stats=st)
                mega = dev.generateImg(spp, seed=SEED, flags=self.M.RENDER_MEGAKERNEL)
            finally:
                dev.close()
            assert np.array_equal(_bits(frame), _bits(mega)), "%s spp %d: %d channels differ from the megakernel" % (key, spp, int((_bits(frame) != _bits(mega)).sum()))
            self.answers[(key, spp)] = (mega, st, self.hit_pixels[key])
        return self.answers[(key, spp)]

    def close(self):
        for sc in self.scenes.values():
            sc.close()


@pytest.fixture(scope="module")
def world(mcpt, tmp_path_factory):
    w = _World(mcpt, str(tmp_path_factory.mktemp("bounce_first")) + os.sep)
    yield w
    w.close()


def _counts(st):
    return (st.rays_shadow + st.shadow_skipped, st.rays_bounce, st.shade_calls)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("key", SCENE_KEYS)
def test_frames_equal_the_megakernel(world, mcpt, key, route):
    knobs, handover = ROUTES[route]
    dev = None if handover == 1 else world.device(key, knobs)
    try:
        for spp in (SPPS if key == "cornell-box" else SPPS_THIN):
            mega, st0, hit_pixels = world.answer(key, spp)
            if handover == 1:
                # the first pass leaves hit_pixels * spp paths less the few on emitters; the depth-1 pass at most 0.6 of them and what the binomial adds
                dev = world.device(key, dict(knobs, MCPT_FINISH_PATHS=str(int(0.7 * hit_pixels * spp))))
            st = mcpt.Stats()
            img = dev.generateImg(spp, seed=SEED, stats=st)
            print("%s %s spp %d: launches %d, hit pixels %d, counts %s" % (key, route, spp, st.launches, hit_pixels, _counts(st)))
            if handover == 1:
                dev.close()
                dev = None
            assert np.array_equal(_bits(img), _bits(mega)), "%s %s spp %d: %d channels differ from the megakernel" % (
                key, route, spp, int((_bits(img) != _bits(mega)).sum()))
            assert _counts(st) == _counts(st0)
            if handover is not None:
                assert st.launches == handover, "the hand-over was not at depth %d: %d trace launches before it" % (handover, st.launches)
            else:
                assert st.launches >= 3, st.launches
    finally:
        if dev is not None:
            dev.close()
