"""-m gpu: the pool trace engine takes a ray's first node steps -- on the root and, where that is an inner node, on the nearest root child
-- in the refill step that loads the ray (trace_pool.hpp).

The root step is the node step's own arithmetic on a node that is the same in every lane; after it the ray holds up to three stack
entries and goes on to an inner node (the second step, unless the stack cap refuses it), a leaf, or the result class (a ray that misses
every root child).  Nothing about the walk changes, so every case asserts answers that do not depend on the engine, and the cases of
(1) and (2) also the work counters of the commit before the change, recorded by tests/make_pool_first_step_golden.py into
tests/golden/pool_first_step_counts.json:

1. answers: closest hits of make_rays() equal to the CPU oracle's bit for bit; the wavefront frame (MCPT_FINISH_PATHS=0) equal to the
   default frame and to the megakernel frame bit for bit -- cornell-box, glassroom (on-surface refraction rays), veach-mis (rays the fast
   walk may not take are deferred out of the same 64-slot fetch that starts other rays);
2. MCPT_TEST_STACK_CAP 4, 5, 6: after the root step a ray holds 0..3 entries, the second step is refused above 1, 2, 3 entries
   (the ray is filed as it is, and the node step hands it over);
3. tiny trees (1, 2, 4, 5, 17 triangles and a two-triangle lamp): a root with one leaf child, with leaf children only, the first inner
   child; rays that miss every root child (a miss straight from the refill), rays from outside into the scene, rays over one triangle;
4. ray_intersect batches of 1, 63, 64, 65, 129 rays, a quarter of them misses;
5. the counters of (1) and (2).

A device per case (knobs are read at creation), 160x90 at SPP 2; the oracle's answers and the reference frames are computed once per
scene and kept for the module."""
import json
import os

import numpy as np
import pytest

import make_pool_first_step_golden as G

pytestmark = pytest.mark.gpu

TINY = (1, 2, 4, 5, 17)
BATCHES = (1, 63, 64, 65, 129)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_hits(want, got, what):
    of, ot, op, opn = want
    gf, gt, gp, gpn = got
    assert np.array_equal(of, gf), "%s: %d of %d rays hit another face than the oracle's" % (what, int((of != gf).sum()), of.size)
    h = of >= 0
    for a, b in ((ot, gt), (op, gp), (opn, gpn)):
        assert np.array_equal(_bits(a[h]), _bits(b[h])), "%s: t / p / pn differ from the oracle's" % what


def tiny_geometry(n):
    """n small, slightly tilted triangles on a 5-wide grid in the plane y ~ 0, two units apart (no two share an x-z footprint), and a
    two-triangle lamp above them (synthetic.write_obj's dict)"""
    rng = np.random.default_rng(100 + n)
    i = np.arange(n)
    c = np.stack([2.0 * (i % 5), np.zeros(n), 2.0 * (i // 5)], axis=1)
    off = np.array([[-0.4, 0.0, -0.3], [0.4, 0.0, -0.3], [0.0, 0.0, 0.45]])
    v = c[:, None, :] + off[None, :, :] + rng.uniform(-0.05, 0.05, size=(n, 3, 3))
    # (counter-clockwise seen from above: the normals point up)
    v = v[:, [0, 2, 1], :].reshape(n, 9)
    mid = c.mean(axis=0)
    lamp = np.array([[-0.5, 3.0, -0.5, 0.5, 3.0, 0.5, 0.5, 3.0, -0.5], [-0.5, 3.0, -0.5, -0.5, 3.0, 0.5, 0.5, 3.0, 0.5]])
    lamp[:, 0::3] += mid[0]
    lamp[:, 2::3] += mid[2]
    v = np.vstack([v, lamp])
    e1, e2 = v[:, 3:6] - v[:, 0:3], v[:, 6:9] - v[:, 0:3]
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    mat = np.zeros(v.shape[0], dtype=np.int32)
    mat[n:] = 1
    rec = np.array([[0.6, 0.5, 0.4, 0, 0, 0, 1, 1], [0, 0, 0, 0, 0, 0, 1, 1]], dtype=np.float64)
    return dict(v=v, vn=np.tile(nrm, 3), material=mat, material_rec=rec, material_names=["grey", "lamp"],
                light_material=np.array([1], dtype=np.int32), light_radiance=np.full((1, 3), 12.0),
                eye=[mid[0] + 1.0, 6.0, mid[2] + 9.0], look_at=[mid[0], 0.0, mid[2]], up=[0.0, 1.0, 0.0], fovy=50.0, width=G.W, height=G.H)


def tiny_rays(g, osc, n_each, seed):
    """(away, inward, over): origins outside the scene's box pointing away from it (they miss the root's children), origins outside
    aimed at a point of a triangle, and origins just above one triangle pointing down at it, a little off the vertical (they enter the
    one root child that holds it)"""
    rng = np.random.default_rng(seed)
    box = osc.bvh_nodes()[0][0]
    hi, lo = box[:3], box[3:]
    mid, ext = 0.5 * (hi + lo), float(np.linalg.norm(hi - lo)) + 1.0
    u = rng.normal(size=(n_each, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    away = np.hstack([mid + 3.0 * ext * u, u])
    tri = g["v"][rng.integers(g["v"].shape[0], size=n_each)].reshape(n_each, 3, 3)
    bary = rng.dirichlet(np.ones(3), size=n_each)
    target = (tri * bary[:, :, None]).sum(axis=1)
    u2 = rng.normal(size=(n_each, 3))
    u2 /= np.linalg.norm(u2, axis=1, keepdims=True)
    o = mid + 3.0 * ext * u2
    d = target - o
    inward = np.hstack([o, d / np.linalg.norm(d, axis=1, keepdims=True)])
    n_small = g["v"].shape[0] - 2
    tri = g["v"][rng.integers(n_small, size=n_each)].reshape(n_each, 3, 3)
    cen = tri.mean(axis=1)
    d = np.array([0.0, -1.0, 0.0]) + rng.uniform(-2e-3, 2e-3, size=(n_each, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    over = np.hstack([cen - 0.25 * d, d])
    return [np.ascontiguousarray(a, dtype=np.float64) for a in (away, inward, over)]


class _World:
    def __init__(self, M, O, tmp):
        self.M, self.O, self.tmp = M, O, tmp
        self.scenes = {}
        with open(G.GOLDEN) as f:
            self.golden = json.load(f)

    def shipped(self, name):
        """oracle scene, library scene, rays and the oracle's closest hits, the default and the megakernel frame"""
        if name not in self.scenes:
            from conftest import make_rays
            base = G.scene_dir(name)
            osc = self.O.OracleScene(base + name, texture_dir=base, width=G.W, height=G.H)
            sc = self.M.Scene(base, name, width=G.W, height=G.H)
            rays = make_rays(osc, G.N_RAYS, seed=29)
            want = osc.trace_closest(rays)
            dev = G.pool_device(self.M, sc, {})
            try:
                frame = dev.generateImg(G.SPP, seed=G.SEED)
                mega = dev.generateImg(G.SPP, seed=G.SEED, flags=self.M.RENDER_MEGAKERNEL)
            finally:
                dev.close()
            assert np.array_equal(_bits(frame), _bits(mega))
            self.scenes[name] = dict(osc=osc, sc=sc, rays=rays, want=want, frame=frame, mega=mega, runs={})
        return self.scenes[name]

    def run(self, name, cfg):
        """the case (scene, configuration), run once: its answers are asserted here, its counters are returned"""
        s = self.shipped(name)
        if cfg not in s["runs"]:
            hits, img, cr, cf = G.run_case(self.M, s["sc"], s["rays"], G.CONFIGS[cfg])
            what = "%s %s" % (name, cfg)
            _same_hits(s["want"], hits, what)
            assert np.array_equal(_bits(img), _bits(s["frame"])), "%s: %d channels differ from the default frame" % (
                what, int((_bits(img) != _bits(s["frame"])).sum()))
            assert np.array_equal(_bits(img), _bits(s["mega"])), what
            s["runs"][cfg] = (cr, cf)
        return s["runs"][cfg]

    def tiny(self, n):
        key = "tiny%d" % n
        if key not in self.scenes:
            from montecarlopathtracing_amd import synthetic
            base = str(self.tmp.mktemp(key)) + os.sep
            g = tiny_geometry(n)
            synthetic.write_obj(g, base, key)
            osc = self.O.OracleScene(base + key, texture_dir=base, width=G.W, height=G.H)
            sc = self.M.Scene(base, key, width=G.W, height=G.H)
            self.scenes[key] = dict(osc=osc, sc=sc, g=g)
        return self.scenes[key]

    def close(self):
        for s in self.scenes.values():
            s["sc"].close()
            s["osc"].close()


@pytest.fixture(scope="module")
def world(mcpt, oracle, tmp_path_factory):
    w = _World(mcpt, oracle, tmp_path_factory)
    yield w
    w.close()


# ------------------------------------------------------------------------------------------------------- 1, 2: answers
@pytest.mark.parametrize("cfg", list(G.CONFIGS))
@pytest.mark.parametrize("name", G.SCENE_NAMES)
def test_answers(world, name, cfg):
    """closest hits equal to the oracle's, the frame equal to the default device's frame and to the megakernel frame, bit for bit"""
    if name == "veach-mis":
        assert int((world.shipped(name)["rays"][:, 3:] == 0).any(axis=1).sum()) > 100      # rays the fast walk may not take
    world.run(name, cfg)


# ------------------------------------------------------------------------------------------------------- 5: work counters
@pytest.mark.parametrize("cfg", list(G.CONFIGS))
@pytest.mark.parametrize("name", G.SCENE_NAMES)
def test_work_counters_are_those_before_the_step_moved(world, mcpt, name, cfg):
    """rays, node visits and triangle tests, of the run and of its dominant kernel, as recorded from the commit before the change"""
    cr, cf = world.run(name, cfg)
    want = world.golden["counts"][name][cfg]
    print(name, cfg, "build", mcpt.build_id(), "golden from", world.golden["recorded_from_build_id"])
    print(" ray_intersect", cr, "golden", want["ray_intersect"])
    print(" frame        ", cf, "golden", want["frame"])
    assert cr == want["ray_intersect"]
    assert cf == want["frame"]
    # (k_wf_trace_pool is the dominant kernel where every bounce goes through it; the default frame of this size is the finishing pass's)
    assert cf["node_visits"] > cf["rays"] > 0 and cr["node_visits"] > cr["rays"] > 0
    assert cfg == "default" or cf["dom_rays"] > 0


# ------------------------------------------------------------------------------------------------------- 3: tiny trees
@pytest.mark.parametrize("n", TINY)
def test_tiny_trees(world, n):
    """Scenes whose root has one leaf child, leaf children only, or its first inner child: misses straight from the refill, rays from
    outside into the scene, rays that enter the one root child over which they start; and make_rays()' mix."""
    from conftest import make_rays
    s = world.tiny(n)
    away, inward, over = tiny_rays(s["g"], s["osc"], 256, seed=n)
    rays = np.ascontiguousarray(np.vstack([away, inward, over, make_rays(s["osc"], 1024, seed=31)]))
    want = s["osc"].trace_closest(rays)
    of = want[0]
    assert (of[:256] < 0).all(), "rays pointing away from the scene must miss"
    assert (of[256:512] >= 0).sum() > 128 and (of[512:768] >= 0).sum() > 128, "rays aimed at triangles must mostly hit"
    assert (of < 0).sum() > 256 and (of >= 0).sum() > 256
    dev = G.pool_device(world.M, s["sc"], {})
    try:
        info = dev.fast_hierarchy()[0]
        print("tiny%d: %d nodes, %d triangle slots, stack need %d" % (n, info.n_nodes, info.n_tris, info.cw_stack_need))
        assert info.enabled == 1
        _same_hits(want, dev.ray_intersect(rays), "tiny%d" % n)
        # (the groups alone and in another order: every lane of a fetch misses, every lane of a fetch hits)
        for a, b in ((0, 256), (256, 512), (512, 768)):
            _same_hits([w[a:b] for w in want], dev.ray_intersect(np.ascontiguousarray(rays[a:b])), "tiny%d rays %d..%d" % (n, a, b))
        perm = np.random.default_rng(n).permutation(rays.shape[0])
        _same_hits([w[perm] for w in want], dev.ray_intersect(np.ascontiguousarray(rays[perm])), "tiny%d permuted" % n)
        img = dev.generateImg(G.SPP, seed=G.SEED)
        mega = dev.generateImg(G.SPP, seed=G.SEED, flags=world.M.RENDER_MEGAKERNEL)
        assert np.array_equal(_bits(img), _bits(mega))
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------------- 4: batch sizes
@pytest.mark.parametrize("n", BATCHES)
def test_batch_sizes_with_a_quarter_of_misses(world, n):
    """ray_intersect batches around the 64-slot fetch, a quarter of the rays missing the scene (a single ray: one that misses and one
    that hits), misses spread through the batch"""
    s = world.tiny(17)
    away, inward, _ = tiny_rays(s["g"], s["osc"], 256, seed=1000 + n)
    hits = inward[s["osc"].trace_closest(inward)[0] >= 0]
    assert (s["osc"].trace_closest(away)[0] < 0).all() and hits.shape[0] >= n
    dev = G.pool_device(world.M, s["sc"], {})
    try:
        for n_miss in ([0, 1] if n == 1 else [n // 4]):
            rays = np.vstack([away[:n_miss], hits[:n - n_miss]])
            rays = np.ascontiguousarray(rays[np.random.default_rng(n).permutation(n)])
            want = s["osc"].trace_closest(rays)
            assert int((want[0] < 0).sum()) == n_miss and rays.shape[0] == n
            _same_hits(want, dev.ray_intersect(rays), "batch of %d with %d misses" % (n, n_miss))
    finally:
        dev.close()
