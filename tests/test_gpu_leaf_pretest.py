"""-m gpu: the leaf step of the trace engines with the branch-free pre-test (csrc/pre_test.hpp) and the records of a round loaded
together (trace_persistent.hpp: leaf_survivors).  The arithmetic of the pre-test is the one it had, so the survivor masks, the exact
tests and every result bit are too.  64 x 48 frames:

1. cornell-box and veach-mis at SPP 1, 3 and 64, glassroom at SPP 3, through the pool engine and through the voting engine, and with
   the hand-over to k_wf_finish_pool at depth 0 (both scenes and glassroom) and at depth 1 (both scenes at SPP 3 and 64): each frame
   bit for bit the megakernel's (one lane per sample, the reference-shaped walk, no pre-test);
2. leaves of at most 1, 2, 3, 4 and 5 triangles (MCPT_FAST_LEAF): leaves that end on the first slot of a round, on the second, and in
   a third round -- on cornell-box through both engines and through k_wf_finish_pool (hand-over at depth 0), and, with leaves of one
   triangle, on a scene of five triangles: its last leaf is the last slot of the triangle array, so the slot past it is the padding;
3. rays, node visits, triangle tests, exact tests per ray and deferred rays of all of these, as recorded from the commit before the
   change by tests/make_leaf_pretest_golden.py into tests/golden/leaf_pretest_counts.json;
4. the self-check build (-DMCPT_PRE_CHECK: every rejected triangle goes through the exact test as well) on cornell-box and veach-mis
   at SPP 3: no rejected triangle is a candidate."""
import json

import numpy as np
import pytest

import make_leaf_pretest_golden as G
from conftest import ROOT, SCENES

pytestmark = pytest.mark.gpu

CASES = G.cases()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class _World:
    def __init__(self, M, tmp):
        self.M, self.scenes, self.megas = M, G.Scenes(M, tmp.mktemp("leaf_pretest")), {}
        with open(G.GOLDEN) as f:
            self.golden = json.load(f)
        assert (self.golden["width"], self.golden["height"], self.golden["seed"]) == (G.W, G.H, G.SEED)

    def mega(self, scene, spp):
        """the megakernel's frame, once per (scene, spp), on a device of the default leaf size"""
        if (scene, spp) not in self.megas:
            dev = G.device(self.M, self.scenes.get(scene), {})
            try:
                self.megas[scene, spp] = dev.generateImg(spp, seed=G.SEED, flags=self.M.RENDER_MEGAKERNEL)
            finally:
                dev.close()
        return self.megas[scene, spp]

    def frame(self, scene, spp, knobs):
        img, c = G.counted_frame(self.M, self.scenes.get(scene), spp, knobs)
        mega = self.mega(scene, spp)
        assert np.array_equal(_bits(img), _bits(mega)), "%s spp %d %s: %d channels differ from the megakernel" % (
            scene, spp, knobs, int((_bits(img) != _bits(mega)).sum()))
        return c


@pytest.fixture(scope="module")
def world(mcpt, tmp_path_factory):
    w = _World(mcpt, tmp_path_factory)
    yield w
    w.scenes.close()


@pytest.mark.parametrize("name", list(CASES))
def test_frame_and_counters_are_those_before_the_change(world, mcpt, name):
    scene, spp, knobs = CASES[name]
    c = world.frame(scene, spp, knobs)
    want = world.golden["counts"][name]
    print("build", mcpt.build_id(), "golden from", world.golden["recorded_from_build_id"])
    print(" counts", c)
    print(" golden", want)
    assert c == want
    handover = {G.BIG: 0, "DEPTH1": 1}.get(knobs["MCPT_FINISH_PATHS"])
    assert c["tri_tests"] > 0 and (handover == 0 or (c["diag_rays"] > 0 and c["dom_tri_tests"] > 0))
    if handover is not None:
        assert c["launches"] == handover, "the hand-over was not at depth %d: %d trace launches before it" % (handover, c["launches"])
    else:
        assert c["launches"] >= 1


def test_self_check_build_finds_no_wrongly_rejected_triangle():
    import selfcheck
    code = r'''
import sys
sys.path.insert(0, %r)
import montecarlopathtracing_amd as M
for name in ("cornell-box", "veach-mis"):
    sc = M.Scene(%r, name, width=64, height=48)
    for engine in ("pool", "vote"):
        import os
        os.environ["MCPT_TRACE_ENGINE"] = engine
        dev = M.Device(sc, 0)
        st = M.Stats()
        dev.generateImg(3, seed=17, stats=st)
        assert st.dom_rays > 0
        dev.close()
    sc.close()
print("done")
''' % (ROOT, SCENES)
    out = selfcheck.run(code, timeout=300)
    assert out.returncode == 0 and "done" in out.stdout, out.stderr[-3000:]
    assert "SELF-CHECK" not in out.stderr, selfcheck.pre_test_failures(out.stderr)[:6]
    shares = selfcheck.survivor_shares(out.stderr)
    assert len(shares) == 4 and max(shares) < 60.0, shares
