"""Records tests/golden/pool_window_refill_counts.json: the work counters of the pool trace engine on one frame of
test_gpu_pool_window_refill.py, from a build of the commit BEFORE the refill read slot flags first (select that build with MCPT_LIB; its
build id goes into the file).  The refill hands the same rays to the engine, in another grouping: every ray still visits the same nodes
and triangles, so the library under test must reproduce these numbers exactly.

    MCPT_LIB=<parent build>/libmcpt.so python tests/make_pool_window_refill_golden.py [output.json]

Needs a GPU.  The frame and the way it is run are defined here and imported by the test, so both sides run the same thing.  The exact
tests per ray are not part of mcpt_stats: they are taken from the line MCPT_PRINT_DIAG prints (three decimals), with the dominant
kernel's ray count beside them."""
import contextlib
import json
import os
import re
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(HERE, "golden", "pool_window_refill_counts.json")
W, H, SEED = 64, 48, 11
COUNT_SPP = 65
KNOBS = ("MCPT_TRACE_ENGINE", "MCPT_FINISH_ENGINE", "MCPT_FINISH_PATHS", "MCPT_WORKSPACE_GB", "MCPT_LOGIC_GRID", "MCPT_SHORT_KERNEL",
         "MCPT_TEST_STACK_CAP", "MCPT_SLOW_LIST", "MCPT_TRACE_MIN_CHUNK", "MCPT_TRACE_MAX_CHUNK", "MCPT_TRACE_BLOCK_RAYS", "MCPT_PRINT_DIAG")
WAVEFRONT = {"MCPT_FINISH_PATHS": "0"}          # every bounce goes through k_wf_trace_pool
COUNTERS = ("rays_primary", "rays_shadow", "rays_bounce", "shadow_skipped", "shade_calls", "node_visits", "tri_tests",
            "dom_rays", "dom_node_visits", "dom_tri_tests")
DIAG = re.compile(r"k_wf_trace: (\d+) rays, ([0-9.]+) nodes, ([0-9.]+) triangles visited, ([0-9.]+) exact tests per ray")


def pool_device(M, sc, knobs):
    """a device of the pool engine created under `knobs` (read at creation), every other knob unset"""
    knobs = dict(knobs, MCPT_TRACE_ENGINE="pool")
    old = {k: os.environ.pop(k, None) for k in KNOBS}
    try:
        os.environ.update(knobs)
        assert sc.trace_engine() == "pool"
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


def counted_frame(M, sc):
    """the counted frame on a fresh pool device: (frame, counters)"""
    dev = pool_device(M, sc, dict(WAVEFRONT, MCPT_PRINT_DIAG="1"))
    st = M.Stats()
    text = []
    try:
        with captured_stderr(text):
            img = dev.generateImg(COUNT_SPP, seed=SEED, stats=st)
    finally:
        dev.close()
    m = DIAG.search(text[0])
    assert m, "no k_wf_trace line in the diagnostics:\n" + text[0]
    c = {n: int(getattr(st, n)) for n in COUNTERS}
    c["diag_rays"] = int(m.group(1))
    c["diag_nodes_per_ray"], c["diag_tris_per_ray"], c["diag_exact_per_ray"] = m.group(2), m.group(3), m.group(4)
    return img, c


def main(out):
    import montecarlopathtracing_amd as M
    from conftest import SCENES
    sc = M.Scene(SCENES, "cornell-box", width=W, height=H)
    _, c = counted_frame(M, sc)
    sc.close()
    doc = {"recorded_from_build_id": M.build_id(), "library": os.path.basename(os.environ.get("MCPT_LIB", "libmcpt.so")),
           "scene": "cornell-box", "width": W, "height": H, "spp": COUNT_SPP, "seed": SEED, "counts": c}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out, "from build", doc["recorded_from_build_id"], c)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else GOLDEN)
