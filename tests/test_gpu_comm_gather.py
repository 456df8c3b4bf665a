"""The one-process-per-GPU exchange (mcpt_comm_*, csrc/proc_comm.cpp; montecarlopathtracing_amd/procs.py) with MORE THAN ONE RANK, on one GPU.

RCCL refuses two ranks on one GPU, so the collective library is tests/fake_rccl.cpp, a stand-in that works within one process and that
libmcpt.so loads through MCPT_RCCL_LIBRARY; the ranks are threads of this process (ctypes releases the GIL, the library's error text is
thread-local), every one on ordinal 0.  Everything else is the product's code: the list preparation, the event hand-over from the render
stream, k_pack_pixels, the counts handed to ncclSend / ncclRecv, k_unpack_pixels, the error paths.  Expected frames come from a numpy
restatement of the partition written here (owner_map; held once to Scene.owned_pixels), never from mcpt_owned_pixels.  Every comparison is
bit for bit.

  (a) test_pattern_frames        every rank's frame holds doubles whose bits encode (rank, pixel, channel), in tests/guarded.py buffers:
                                 33 x 17 and 1 x 1 frames, worlds 2, 3 and 5, tiles 32 x 8 and 5 x 3, both fills, both alignments.  Rank 0's
                                 payload is the restatement's frame in every word, the other ranks' frames are their inputs, all bands intact
  (b) test_rendered_frames       procs.ProcessGroup, Device.render_device per rank on the rank's own stream and gather_frame behind it with no
                                 host synchronisation in between, twice: rank 0's frame is Device.generateImg of one device
  (c) test_lists_follow_the_frame one communicator, tile 5 x 3 then 32 x 8 on one frame, then one tile shape on a 5 x 3-pixel frame and on a
                                 33 x 17 one (small, then large: lists kept from the small frame index inside the large one)
  (d) test_allreduce             three ranks, n = 0 (barrier), 1 and 64, sum and max of integer-valued doubles
  (e) test_refusals_*            a rank on another id: gather and all-reduce return an error with a message on every rank inside the
                                 stand-in's bound (0.5 s here), the handles can be freed, a correct gather on fresh handles follows; ranks
                                 that disagree about the tile shape: the count mismatch is refused on both sides and nothing is copied
No case can wait without a bound: every wait for a peer in the stand-in has one, and a rank's thread that has not returned after 60 s fails
the case.  What this file cannot reach: real RCCL with more than one rank, two physical GPUs, the xGMI hop, peer access between ordinals.

24 cases; the whole file takes 3.4 s of wall time on an MI355X (pytest's own figure: 0.7 s of it the stand-in's compilation, 1.1 s the two
bounded waits of the first refusal case, which run to their bound of 0.5 s by design; every other case takes under 0.3 s).
"""
import ctypes as C
import math
import os
import threading
import time

import numpy as np
import pytest

import fake_rccl
from conftest import SCENES
from guarded import FILLS, Guarded
from hip_rt import DeviceBuffer, Stream, set_device
from montecarlopathtracing_amd._lib import RenderParams

pytestmark = pytest.mark.gpu

F64 = np.dtype(np.float64)
ALL = tuple((f, s) for f in FILLS for s in (0, 8))
ID_BYTES = 128
RANK_DEADLINE = 60.0                            # a rank's thread that has not returned by then fails the case (nothing here takes a second)
BOUND_MS = 500                                  # the stand-in's bound in the refusal cases


# ---- the partition, restated (include/mcpt.h, mcpt_render_params)

def owner_map(width, height, world, tile_w=0, tile_h=0):
    """[H, W]: the rank that owns each pixel.  Tile (tx, ty) belongs to rank (tx + shift * ty) mod world; a tile is tile_w x tile_h, 32 wide
    where tile_w <= 0 and 8 high where tile_h <= 0; shift is the first s >= max(1, world // 2) below world that is coprime to it, else 1."""
    tw, th = tile_w if tile_w > 0 else 32, tile_h if tile_h > 0 else 8
    shift = next((s for s in range(max(1, world // 2), world) if math.gcd(s, world) == 1), 1)
    ty, tx = np.arange(height)[:, None] // th, np.arange(width)[None, :] // tw
    return (tx + shift * ty) % world


def pattern(rank, width, height):
    """[H, W, 3] doubles (finite, all different) whose bits say which rank's frame, which pixel and which channel they came from"""
    pix = np.arange(width * height, dtype=np.uint64)[:, None]
    ch = np.arange(3, dtype=np.uint64)[None, :]
    return ((np.uint64(0x4000 + rank) << np.uint64(48)) | (pix << np.uint64(8)) | (ch + np.uint64(1))).view(np.float64).reshape(height, width, 3)


def gathered(width, height, world, tile_w, tile_h):
    """rank 0's frame after the gather of the pattern frames"""
    own = owner_map(width, height, world, tile_w, tile_h)
    out = pattern(0, width, height).copy()
    for r in range(1, world):
        out[own == r] = pattern(r, width, height)[own == r]
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64).reshape(-1)


def same_frame(got, want, width, what):
    bad = np.flatnonzero((bits(got) != bits(want)).reshape(-1, 3).any(axis=1))
    assert bad.size == 0, "%s: %d of %d pixels differ, the first (x, y): %s" % (
        what, bad.size, got.size // 3, ", ".join("(%d, %d)" % (p % width, p // width) for p in bad[:8]))


# ---- the ranks of this process

@pytest.fixture(scope="module")
def w(mcpt, tmp_path_factory):
    """the stand-in, built and named to the library; scenes by size"""
    so = fake_rccl.build(tmp_path_factory.mktemp("fake_rccl"))
    saved = {k: os.environ.get(k) for k in ("MCPT_RCCL_LIBRARY", fake_rccl.TIMEOUT_ENV)}
    os.environ["MCPT_RCCL_LIBRARY"] = so
    os.environ.pop(fake_rccl.TIMEOUT_ENV, None)
    ns = type("W", (), {})()
    ns.mcpt, ns.lib, ns.so, ns.scenes = mcpt, mcpt.lib(), so, {}
    # the library the knob names is the one that answers: its ids carry the stand-in's mark, and it is mapped into this process
    first = unique_id(ns)
    assert first[:8] == b"ccr_ekaf" and first != unique_id(ns), "the ids are not the stand-in's: MCPT_RCCL_LIBRARY was not honoured"
    assert so in open("/proc/self/maps").read()
    yield ns
    for sc in ns.scenes.values():
        sc.close()
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def scene(w, width, height):
    if (width, height) not in w.scenes:
        w.scenes[(width, height)] = w.mcpt.Scene(SCENES, "cornell-box", width=width, height=height)
    return w.scenes[(width, height)]


def unique_id(w):
    buf = (C.c_uint8 * ID_BYTES)()
    assert w.lib.mcpt_comm_unique_id(buf, ID_BYTES) == ID_BYTES, w.lib.mcpt_last_error()
    return bytes(buf)


def run_ranks(world, fn):
    """fn(rank) on one thread per rank -> [results]; a rank's exception is raised here, and so is a rank that does not return"""
    out, err = [None] * world, [None] * world

    def body(r):
        try:
            set_device(0)
            out[r] = fn(r)
        except BaseException as e:              # (raised below, in the test's thread)
            err[r] = e
    threads = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    end = time.monotonic() + RANK_DEADLINE
    for t in threads:
        t.join(max(0.0, end - time.monotonic()))
    late = [r for r, t in enumerate(threads) if t.is_alive()]
    assert not late, "ranks %s did not return within %.0f s" % (late, RANK_DEADLINE)
    for e in err:
        if e is not None:
            raise e
    return out


class Ranks:
    """mcpt_comm handles of `world` ranks on ordinal 0 (ids: one per rank, default the same for all) and a stream per rank"""

    def __init__(self, w, world, ids=None):
        self.w, self.world, self.h, self.streams = w, world, [], []
        ids = ids or [unique_id(w)] * world
        for r in range(world):
            h = C.c_void_p()
            rc = w.lib.mcpt_comm_create(0, r, world, (C.c_uint8 * ID_BYTES).from_buffer_copy(ids[r]), ID_BYTES, C.byref(h))
            assert rc == 0, (r, rc, w.lib.mcpt_last_error())
            assert w.lib.mcpt_comm_size(h) == world
            self.h.append(h)
            self.streams.append(Stream())

    def run(self, fn):
        return run_ranks(self.world, fn)

    def gather(self, sc, ptrs, tile, streams=True):
        """mcpt_comm_gather_frame on every rank -> [(return code, message, seconds)]"""
        lib = self.w.lib

        def one(r):
            rp = RenderParams(1, 0, r, self.world, tile[0], tile[1], 0)
            t0 = time.monotonic()
            rc = lib.mcpt_comm_gather_frame(self.h[r], sc._h, C.byref(rp), C.c_void_p(ptrs[r]), self.streams[r].h if streams else None)
            return rc, lib.mcpt_last_error().decode(errors="replace") if rc else "", time.monotonic() - t0
        return self.run(one)

    def allreduce(self, values, op):
        """mcpt_comm_allreduce on every rank, values[r] in place -> [(return code, message, seconds)]"""
        lib = self.w.lib

        def one(r):
            v = values[r]
            t0 = time.monotonic()
            rc = lib.mcpt_comm_allreduce(self.h[r], v.ctypes.data_as(C.POINTER(C.c_double)) if v is not None else None, 0 if v is None else v.size, op)
            return rc, lib.mcpt_last_error().decode(errors="replace") if rc else "", time.monotonic() - t0
        return self.run(one)

    def free(self):
        for h in self.h:
            self.w.lib.mcpt_comm_free(h)
        for s in self.streams:
            s.destroy()
        self.h, self.streams = [], []


def ok(results):
    assert [rc for rc, _, _ in results] == [0] * len(results), results


def bands_intact(g, what):
    """the bands of a buffer the call may write (rank 0's frame): Guarded.check without the hold to the upload"""
    sent, g.sent = g.sent, None
    try:
        g.check(what)
    finally:
        g.sent = sent


def gather_patterns(w, ranks, size, tile, fill, skew, what):
    """one gather of the pattern frames in guarded buffers, held to the restatement: rank 0's payload, the other ranks' inputs, every band"""
    width, height = size
    world = ranks.world
    bufs = [Guarded(pattern(r, width, height), F64, fill, skew) for r in range(world)]
    try:
        ok(ranks.gather(scene(w, width, height), [g.ptr for g in bufs], tile))
        same_frame(bufs[0].payload(), gathered(width, height, world, *tile), width, what + ": rank 0's frame")
        bands_intact(bufs[0], what + ": rank 0's frame")
        for r in range(1, world):
            bufs[r].check("%s: rank %d's frame" % (what, r))
    finally:
        for g in bufs:
            g.free()


# ---- the restatement against the library's list, once: a disagreement below then shows which side moved

def test_the_restated_partition_is_the_librarys(w):
    for size in ((33, 17), (1, 1), (5, 3), (64, 36)):
        sc = scene(w, *size)
        for world in (1, 2, 3, 5, 8):
            for tile in ((0, 0), (5, 3), (32, 8), (7, 2), (-1, 4)):
                own = owner_map(size[0], size[1], world, *tile).reshape(-1)
                for r in range(world):
                    assert np.array_equal(sc.owned_pixels(r, world, *tile), np.flatnonzero(own == r)), (size, world, tile, r)
    own = owner_map(33, 17, 5)
    assert sorted(np.bincount(own.reshape(-1), minlength=5)) == [8, 8, 32, 256, 257]           # (32 x 8 tiles: four ranks own one tile each)
    assert list(np.bincount(owner_map(1, 1, 5).reshape(-1), minlength=5)) == [1, 0, 0, 0, 0]


# ---- (a)

@pytest.mark.parametrize("tile", [(0, 0), (5, 3)], ids=["tiles32x8", "tiles5x3"])
@pytest.mark.parametrize("world", [2, 3, 5])
@pytest.mark.parametrize("size", [(33, 17), (1, 1)], ids=["33x17", "1x1"])
def test_pattern_frames(w, size, world, tile):
    ranks = Ranks(w, world)
    try:
        for fill, skew in ALL:                  # (the same handles: the second to fourth gather run on the lists the first one made)
            gather_patterns(w, ranks, size, tile, fill, skew, "%dx%d world %d tiles %s fill 0x%02X skew %d" % (size + (world, tile, fill, skew)))
    finally:
        ranks.free()


# ---- (b)

SPP, SEED = 3, 7


@pytest.fixture(scope="module")
def rendered(w):
    """cornell-box at 64 x 36: a device per rank (a device renders one frame at a time) and the frame of one device"""
    sc = scene(w, 64, 36)
    devs = [w.mcpt.Device(sc, 0) for _ in range(3)]
    want = devs[0].generateImg(SPP, seed=SEED)
    assert want.max() > 0
    yield sc, devs, want
    for d in devs:
        d.close()


@pytest.mark.parametrize("world", [2, 3])
def test_rendered_frames(w, rendered, tmp_path, world):
    from montecarlopathtracing_amd.procs import ProcessGroup
    sc, devs, want = rendered
    path = str(tmp_path / "rdzv")
    groups = [ProcessGroup(0, rank=r, world=world, rdzv_path=path) for r in range(world)]       # (rank 0 first: its record is there for the others)
    bufs = [DeviceBuffer(want.nbytes) for _ in range(world)]
    streams = [Stream() for _ in range(world)]
    try:
        assert [g.size() for g in groups] == [world] * world

        def one(r):
            devs[r].render_device(bufs[r].ptr.value, SPP, SEED, r, world, 0, 0, flags=0, stats=None, stream=streams[r].h.value)
            groups[r].gather_frame(sc, bufs[r].ptr.value, stream=streams[r].h.value)            # (nothing waits for the render but the event)
            groups[r].gather_frame(sc, bufs[r].ptr.value, stream=streams[r].h.value)
            got = np.full(want.shape, np.nan)
            bufs[r].to_host_async(got, streams[r].h)
            streams[r].synchronize()
            return got
        frames = run_ranks(world, one)
        same_frame(frames[0], want, 64, "world %d: rank 0's frame against generateImg" % world)
        own = owner_map(64, 36, world)
        for r in range(1, world):               # the other ranks' frames: their own pixels, and the zeros the buffer held
            same_frame(frames[r], np.where((own == r)[:, :, None], want, 0.0), 64, "world %d: rank %d's frame" % (world, r))
    finally:
        for g in groups:
            g.close()
        for b in bufs:
            b.free()
        for s in streams:
            s.destroy()


# ---- (c)

def test_lists_follow_the_frame(w):
    """The cached pixel lists belong to (frame width, frame height, tile_w, tile_h): a communicator is bound to no scene.  Under a key of
    the tile shape alone the fourth gather below ran on the lists of the 5 x 3-pixel frame (rank 2 owns nothing of it, rank 1 five pixels)
    and left rank 0's 33 x 17 frame wrong in 371 of its 561 pixels.  The order is small then large on purpose: kept lists of a LARGER frame
    would index outside the caller's buffer."""
    ranks = Ranks(w, 3)
    try:
        steps = (((33, 17), (5, 3)), ((33, 17), (32, 8)),           # one frame, two tile shapes
                 ((5, 3), (7, 2)), ((33, 17), (7, 2)))              # one tile shape (new to these handles), the small frame and then the large
        for i, (size, tile) in enumerate(steps):
            fill, skew = ALL[i]
            gather_patterns(w, ranks, size, tile, fill, skew, "step %d: %dx%d frame, tiles %s" % ((i + 1,) + size + (tile,)))
    finally:
        ranks.free()


# ---- (d)

@pytest.mark.parametrize("op", [0, 1], ids=["sum", "max"])
@pytest.mark.parametrize("n", [0, 1, 64])
def test_allreduce(w, n, op):
    ranks = Ranks(w, 3)
    try:
        # integer-valued doubles (exact in any order), a different rank the largest at different entries, negative entries among them
        sent = [np.array([((7 * r + 3 * i) % 11 - 4) * 1000.0 + r for i in range(n)]) for r in range(3)]
        want = (np.sum(sent, axis=0) if op == 0 else np.max(sent, axis=0)) if n else None
        values = [s.copy() if n else None for s in sent]
        for _ in range(2):                      # (twice on the same handles: the reduced values go in again)
            ok(ranks.allreduce(values, op))
            if n:
                for r in range(3):
                    assert np.array_equal(bits(values[r]), bits(want)), (r, values[r], want)
                want = want * 3 if op == 0 else want
        if n == 64 and op == 1:
            assert len({int(np.argmax([s[i] for s in sent])) for i in range(n)}) == 3
    finally:
        ranks.free()


# ---- (e)

@pytest.fixture
def short_bound():
    saved = os.environ.get(fake_rccl.TIMEOUT_ENV)
    os.environ[fake_rccl.TIMEOUT_ENV] = str(BOUND_MS)      # (read when a communicator is created)
    yield BOUND_MS / 1000.0
    if saved is None:
        del os.environ[fake_rccl.TIMEOUT_ENV]
    else:
        os.environ[fake_rccl.TIMEOUT_ENV] = saved


def test_refusals_a_rank_on_another_id(w, short_bound):
    """Ranks that took ids of different launches (a stale rendezvous record): with RCCL they wait in ncclCommInitRank for ever; the
    stand-in lets them be created and bounds their first operation.  Every rank gets an error and a message inside the bound -- rank 1
    too, whose send has a rank 0 to go to: its communicator never has all of its ranks."""
    ids = [unique_id(w)] * 2 + [unique_id(w)]
    ranks = Ranks(w, 3, ids)
    size, tile = (33, 17), (0, 0)
    bufs = [Guarded(pattern(r, *size), F64, 0xFF, 0) for r in range(3)]
    try:
        t0 = time.monotonic()
        res = ranks.gather(scene(w, *size), [g.ptr for g in bufs], tile)
        for r, (rc, msg, dt) in enumerate(res):
            assert rc != 0 and "fake_rccl" in msg and "ranks joined this id within %d ms" % BOUND_MS in msg, (r, rc, msg)
            assert "only %d of 3" % (1 if r == 2 else 2) in msg, (r, msg)
            assert short_bound * 0.9 <= dt < short_bound + 1.0, (r, dt)      # the wait ran to its bound and returned at it (1 s for a loaded host)
        for r in range(3):                      # nothing was copied anywhere
            bufs[r].check("refused gather: rank %d's frame" % r)
        res = ranks.allreduce([np.array([1.0 + r]) for r in range(3)], 0)
        for r, (rc, msg, dt) in enumerate(res):
            assert rc != 0 and "ranks joined this id" in msg and short_bound * 0.9 <= dt < short_bound + 1.0, (r, rc, msg, dt)
        assert time.monotonic() - t0 < 2 * short_bound + 2.0
    finally:
        ranks.free()                            # (the handles of a refused exchange can be freed)
        for g in bufs:
            g.free()
    fresh = Ranks(w, 3)
    try:
        gather_patterns(w, fresh, size, tile, 0xA5, 8, "fresh handles after the refusals")
        v = [np.array([float(r)]) for r in range(3)]
        ok(fresh.allreduce(v, 0))
        assert [x[0] for x in v] == [3.0] * 3
    finally:
        fresh.free()


def test_refusals_ranks_that_disagree_about_the_tiles(w, short_bound):
    """Rank 0 expects the pixels rank 1 owns under 32 x 8 tiles, rank 1 sends those it owns under 5 x 3: the counts differ, so the receive is
    an error on both sides at once and not a copy -- rank 0's frame keeps every word.  The same handles then gather correctly."""
    size = (33, 17)
    n0, n1 = int((owner_map(33, 17, 2) == 1).sum()), int((owner_map(33, 17, 2, 5, 3) == 1).sum())
    assert (n0, n1) == (265, 279)
    ranks = Ranks(w, 2)
    bufs = [Guarded(pattern(r, *size), F64, 0xA5, 0) for r in range(2)]
    lib = w.lib

    def one(r):
        rp = RenderParams(1, 0, r, 2, *((0, 0) if r == 0 else (5, 3)), 0)
        t0 = time.monotonic()
        rc = lib.mcpt_comm_gather_frame(ranks.h[r], scene(w, *size)._h, C.byref(rp), C.c_void_p(bufs[r].ptr), ranks.streams[r].h)
        return rc, lib.mcpt_last_error().decode(errors="replace"), time.monotonic() - t0
    try:
        scene(w, *size)
        res = ranks.run(one)
        assert res[0][0] != 0 and "receives %d elements" % (3 * n0) in res[0][1] and "which sends %d" % (3 * n1) in res[0][1], res[0]
        assert res[1][0] != 0 and "refused the send of rank 1 (%d elements" % (3 * n1) in res[1][1], res[1]
        assert max(dt for _, _, dt in res) < short_bound                        # (nobody waited for a bound)
        for r in range(2):
            bufs[r].check("mismatched gather: rank %d's frame" % r)
        gather_patterns(w, ranks, size, (5, 3), 0xFF, 8, "the same handles after the mismatch")
    finally:
        ranks.free()
        for g in bufs:
            g.free()
