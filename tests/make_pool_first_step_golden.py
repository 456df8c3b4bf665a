"""Records tests/golden/pool_first_step_counts.json: the work counters of the pool trace engine on the cases of
test_gpu_pool_first_step.py, from a build of the commit BEFORE a ray's first node steps moved into the refill (select that build with
MCPT_LIB; its build id goes into the file).  The steps moved, the walk did not: every ray visits the same nodes and triangles in the
same order, so the library under test must reproduce these numbers exactly.

    MCPT_LIB=<parent build>/libmcpt.so python tests/make_pool_first_step_golden.py [output.json]

Needs a GPU.  The cases and the way they are run are defined here and imported by the test, so both sides run the same thing."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(HERE, "golden", "pool_first_step_counts.json")
W, H, SPP, SEED = 160, 90, 2, 3
N_RAYS = 8192
SCENE_NAMES = ("cornell-box", "glassroom", "veach-mis")
KNOBS = ("MCPT_TRACE_ENGINE", "MCPT_FINISH_ENGINE", "MCPT_FINISH_PATHS", "MCPT_SHORT_KERNEL", "MCPT_TEST_STACK_CAP", "MCPT_SLOW_LIST",
         "MCPT_PRE_TEST_MAX_TRIS", "MCPT_TRACE_MIN_CHUNK", "MCPT_TRACE_MAX_CHUNK", "MCPT_TRACE_BLOCK_RAYS", "MCPT_PRINT_DIAG")
# (1) the wavefront frame (every bounce through k_wf_trace_pool) and the default frame; (2) stack caps around the new boundary: after
# the root step a ray has 0..3 entries, and a node step refuses a ray with more than cap - 3
CONFIGS = {
    "wavefront": {"MCPT_FINISH_PATHS": "0"},
    "default": {},
    "cap4": {"MCPT_FINISH_PATHS": "0", "MCPT_TEST_STACK_CAP": "4"},
    "cap5": {"MCPT_FINISH_PATHS": "0", "MCPT_TEST_STACK_CAP": "5"},
    "cap6": {"MCPT_FINISH_PATHS": "0", "MCPT_TEST_STACK_CAP": "6"},
}
FRAME_COUNTERS = ("rays", "node_visits", "tri_tests", "dom_rays", "dom_node_visits", "dom_tri_tests")
RAY_COUNTERS = ("rays", "node_visits", "tri_tests")


def scene_dir(name):
    from conftest import SCENES, extra_scene_dir
    return extra_scene_dir() if name == "glassroom" else SCENES


def pool_device(M, sc, knobs):
    """a device of the pool engine created under `knobs` (read at creation), every other knob unset"""
    knobs = dict(knobs, MCPT_TRACE_ENGINE="pool")
    old = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(knobs)
        assert sc.trace_engine() == "pool"
        return M.Device(sc, 0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def counters(st, names):
    return {n: int(getattr(st, n)) for n in names}


def run_case(M, sc, rays, knobs):
    """ray_intersect of `rays` and one frame on a fresh pool device; returns (closest hits, frame, ray counters, frame counters)"""
    dev = pool_device(M, sc, knobs)
    sr, sf = M.Stats(), M.Stats()
    try:
        hits = dev.ray_intersect(rays, stats=sr)
        img = dev.generateImg(SPP, seed=SEED, stats=sf)
    finally:
        dev.close()
    return hits, img, counters(sr, RAY_COUNTERS), counters(sf, FRAME_COUNTERS)


def main(out):
    import montecarlopathtracing_amd as M
    import oracle_lib as O
    from conftest import make_rays
    counts = {}
    for name in SCENE_NAMES:
        base = scene_dir(name)
        osc = O.OracleScene(base + name, texture_dir=base, width=W, height=H)
        sc = M.Scene(base, name, width=W, height=H)
        rays = make_rays(osc, N_RAYS, seed=29)
        counts[name] = {}
        for cfg, knobs in CONFIGS.items():
            _, _, cr, cf = run_case(M, sc, rays, knobs)
            counts[name][cfg] = {"ray_intersect": cr, "frame": cf}
            print(name, cfg, cr, cf)
        sc.close()
        osc.close()
    doc = {"recorded_from_build_id": M.build_id(), "library": os.path.basename(os.environ.get("MCPT_LIB", "libmcpt.so")),
           "width": W, "height": H, "spp": SPP, "seed": SEED, "n_rays": N_RAYS, "ray_seed": 29, "counts": counts}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, "from build", doc["recorded_from_build_id"])


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
