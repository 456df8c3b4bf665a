"""Records tests/golden/leaf_pretest_counts.json: the work counters of the trace engines on the cases of test_gpu_leaf_pretest.py, from a
build of the commit BEFORE the leaf pre-test became branch-free and a round's records were loaded together (select that build with
MCPT_LIB; its build id goes into the file).  The arithmetic of the pre-test and the walk did not change: every ray visits the same
nodes, tests the same triangles, sends the same ones on to the exact test, so the library under test must reproduce these numbers.

    MCPT_LIB=<parent build>/libmcpt.so python tests/make_leaf_pretest_golden.py [output.json]

Needs a GPU.  The cases and the way they are run are defined here and imported by the test, so both sides run the same thing.  Exact
tests and deferred rays are not part of mcpt_stats: they are taken from the lines MCPT_PRINT_DIAG prints (per ray, three decimals, with
the ray count of the trace launches beside them)."""
import contextlib
import json
import os
import re
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(HERE, "golden", "leaf_pretest_counts.json")
W, H, SEED = 64, 48, 17
KNOBS = ("MCPT_TRACE_ENGINE", "MCPT_FINISH_ENGINE", "MCPT_FINISH_PATHS", "MCPT_WORKSPACE_GB", "MCPT_LOGIC_GRID", "MCPT_SHORT_KERNEL",
         "MCPT_TEST_STACK_CAP", "MCPT_SLOW_LIST", "MCPT_TRACE_MIN_CHUNK", "MCPT_TRACE_MAX_CHUNK", "MCPT_TRACE_BLOCK_RAYS", "MCPT_PRINT_DIAG",
         "MCPT_FAST_LEAF", "MCPT_FAST_CT", "MCPT_PRE_TEST_MAX_TRIS")
BIG = "1000000000"
# route -> knobs: every bounce through the pool engine's or the voting engine's trace kernel; the hand-over to k_wf_finish_pool at
# depth 0 and at depth 1 (DEPTH1 stands for a threshold that depends on the frame: depth1_threshold)
ROUTES = {
    "pool": {"MCPT_TRACE_ENGINE": "pool", "MCPT_FINISH_PATHS": "0"},
    "vote": {"MCPT_TRACE_ENGINE": "vote", "MCPT_FINISH_PATHS": "0"},
    "depth0": {"MCPT_TRACE_ENGINE": "pool", "MCPT_FINISH_PATHS": BIG},
    "depth1": {"MCPT_TRACE_ENGINE": "pool", "MCPT_FINISH_PATHS": "DEPTH1"},
}
FRAMES = [("cornell-box", 1), ("cornell-box", 3), ("cornell-box", 64), ("veach-mis", 1), ("veach-mis", 3), ("veach-mis", 64), ("glassroom", 3)]
LEAVES = (1, 2, 3, 4, 5)
COUNTERS = ("rays_primary", "rays_shadow", "rays_bounce", "shadow_skipped", "shade_calls", "node_visits", "tri_tests",
            "dom_rays", "dom_node_visits", "dom_tri_tests", "launches")
DIAG = re.compile(r"k_wf_trace: (\d+) rays, ([0-9.]+) nodes, ([0-9.]+) triangles visited, ([0-9.]+) exact tests per ray")
DEFERRED = re.compile(r"rays deferred to the exact walk by k_wf_trace: (\d+) of (\d+)")


def five_triangles():
    """a floor, a lamp above it and one slanted triangle between them (synthetic.write_obj's dict): five triangles.  With leaves of one
    triangle the last leaf is the last slot of the triangle array, so the second slot of its round is the array's padding, whatever
    the builder does.  (With larger leaves the builder still splits these five the same way each time, so only leaf size 1 is run.)"""
    def quad(y, h, up):
        a, b, c, d = [-h, y, -h], [-h, y, h], [h, y, h], [h, y, -h]
        return np.array([a + b + c, a + c + d] if up else [a + c + b, a + d + c], dtype=np.float64)
    v = np.vstack([quad(0.0, 4.0, True), quad(3.0, 0.75, False), [[-1.5, 0.4, -1.0, 1.5, 0.9, -0.5, 0.0, 1.6, 1.2]]])
    n = np.cross(v[:, 3:6] - v[:, 0:3], v[:, 6:9] - v[:, 0:3])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    assert (n[:2, 1] > 0).all() and (n[2:4, 1] < 0).all()
    rec = np.array([[0.7, 0.6, 0.5, 0, 0, 0, 1, 1], [0, 0, 0, 0, 0, 0, 1, 1], [0.3, 0.6, 0.4, 0, 0, 0, 1, 1]], dtype=np.float64)
    return dict(v=v, vn=np.hstack([n, n, n]), material=np.array([0, 0, 1, 1, 2], dtype=np.int32), material_rec=rec,
                material_names=["floor", "lamp", "sheet"], light_material=np.array([1], dtype=np.int32), light_radiance=np.full((1, 3), 9.0),
                eye=[0.5, 2.2, 7.0], look_at=[0.0, 0.8, 0.0], up=[0.0, 1.0, 0.0], fovy=45.0, width=W, height=H)


def cases():
    """name -> (scene, spp, knobs)"""
    out = {}
    for scene, spp in FRAMES:
        for route in ("pool", "vote"):
            out["%s spp%d %s" % (scene, spp, route)] = (scene, spp, ROUTES[route])
    for scene, spp in (("cornell-box", 1), ("cornell-box", 3), ("cornell-box", 64), ("veach-mis", 3), ("veach-mis", 64), ("glassroom", 3)):
        out["%s spp%d depth0" % (scene, spp)] = (scene, spp, ROUTES["depth0"])
    for scene, spp in (("cornell-box", 3), ("cornell-box", 64), ("veach-mis", 3), ("veach-mis", 64)):
        out["%s spp%d depth1" % (scene, spp)] = (scene, spp, ROUTES["depth1"])
    # leaf sizes: through both engines, and through k_wf_finish_pool (compiled in another object, with other flags)
    for leaf in LEAVES:
        for route in ("pool", "vote", "depth0"):
            out["cornell-box spp3 %s leaf%d" % (route, leaf)] = ("cornell-box", 3, dict(ROUTES[route], MCPT_FAST_LEAF=str(leaf)))
    for route in ("pool", "vote", "depth0"):
        out["five spp3 %s leaf1" % route] = ("five", 3, dict(ROUTES[route], MCPT_FAST_LEAF="1"))
    return out


def device(M, sc, knobs):
    """a device created under `knobs` (read at creation), every other knob unset"""
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        os.environ.update(knobs)
        if "MCPT_TRACE_ENGINE" in knobs:
            assert sc.trace_engine() == knobs["MCPT_TRACE_ENGINE"]
        return M.Device(sc, 0)
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in old.items() if v is not None})


@contextlib.contextmanager
def captured_stderr(out):
    """what the library prints to file descriptor 2 inside the block is appended to the list `out` as one string"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        try:
            yield
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            f.seek(0)
            out.append(f.read().decode(errors="replace"))


def depth1_threshold(M, sc, spp):
    """The first pass leaves hit pixels x spp paths less the few on emitters, the depth-1 pass at most 0.6 of them and what the binomial
    adds: a threshold of 0.7 lies between (test_gpu_bounce_first.py's).  The test asserts that the hand-over was after one launch."""
    dev = device(M, sc, {})
    try:
        n = W * H
        rays = dev.camera_rays(SEED, np.arange(n, dtype=np.int32), np.zeros(n, dtype=np.int32))
        hit = int((dev.ray_intersect(rays)[0] >= 0).sum())
    finally:
        dev.close()
    return str(max(1, int(0.7 * hit * spp)))


def counted_frame(M, sc, spp, knobs):
    """one frame on a fresh device under `knobs`: (frame, counters)"""
    if knobs.get("MCPT_FINISH_PATHS") == "DEPTH1":
        knobs = dict(knobs, MCPT_FINISH_PATHS=depth1_threshold(M, sc, spp))
    dev = device(M, sc, dict(knobs, MCPT_PRINT_DIAG="1"))
    st = M.Stats()
    text = []
    try:
        with captured_stderr(text):
            img = dev.generateImg(spp, seed=SEED, stats=st)
    finally:
        dev.close()
    c = {n: int(getattr(st, n)) for n in COUNTERS}
    m, d = DIAG.search(text[0]), DEFERRED.search(text[0])
    assert m and d, "no k_wf_trace lines in the diagnostics:\n" + text[0]
    c["diag_rays"] = int(m.group(1))
    c["diag_nodes_per_ray"], c["diag_tris_per_ray"], c["diag_exact_per_ray"] = m.group(2), m.group(3), m.group(4)
    c["deferred_rays"] = int(d.group(1))
    return img, c


class Scenes:
    """the scenes of the cases, opened once"""
    def __init__(self, M, tmp_dir):
        self.M, self.dir, self.open = M, str(tmp_dir) + os.sep, {}

    def get(self, key):
        if key not in self.open:
            from conftest import SCENES, extra_scene_dir
            if key == "five":
                from montecarlopathtracing_amd import synthetic
                synthetic.write_obj(five_triangles(), self.dir, "five")
                self.open[key] = self.M.Scene(self.dir, "five", width=W, height=H)
            else:
                self.open[key] = self.M.Scene(extra_scene_dir() if key == "glassroom" else SCENES, key, width=W, height=H)
        return self.open[key]

    def close(self):
        for sc in self.open.values():
            sc.close()


def main(out):
    import montecarlopathtracing_amd as M
    scenes = Scenes(M, tempfile.mkdtemp(prefix="leaf_pretest"))
    counts = {}
    for name, (scene, spp, knobs) in cases().items():
        _, counts[name] = counted_frame(M, scenes.get(scene), spp, knobs)
        print(name, counts[name])
    scenes.close()
    doc = {"recorded_from_build_id": M.build_id(), "library": os.path.basename(os.environ.get("MCPT_LIB", "libmcpt.so")),
           "width": W, "height": H, "seed": SEED, "counts": counts}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, "from build", doc["recorded_from_build_id"])


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
