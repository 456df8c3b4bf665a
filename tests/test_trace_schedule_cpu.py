"""Not gpu: the claim schedule both closest-hit engines share, restated operation for operation.

A wave of either engine takes a ticket from the queue head; ticket k < big_tickets is the slot range [k * chunk, (k + 1) * chunk), every
later ticket MCPT_TAIL_CHUNK slots (or chunk, if smaller), and a wave whose range starts at or past the total stops claiming.  Within its
range the wave fetches 64 slots at a time.  Restated here:
- the ticket -> [next, range_end) mapping and the 64-slot batches: make_ticket_schedule and ticket_range
  (csrc/trace_persistent.hpp:67-83), called from request (csrc/trace_persistent.hpp:217-230) and from the pool engine's refill
  (csrc/trace_pool.hpp:132 and 640-665);
- the chunk each launch passes in: wf_chunk (csrc/wavefront.hip:75-81, k_wf_trace and k_wf_trace_pool), persistent_chunk
  (csrc/wavefront.hip:235-243, the voting engine's closest-hit and primary launches) and the pool engine's closest-hit formula
  (csrc/kernels.hip:457-460);
- the chunk knobs: csrc/knobs.cpp:83-85 and init_launch_cfg (csrc/wavefront.hip:228-230).
Asserted: the tickets issued until a wave sees next >= total cover [0, total) exactly once and in order, for every total and chunk where
the mapping has an edge (1..300 slots, around 512, 4096 and 2^20, either side of seven eighths of a multiple of the chunk), and each
chunk formula stays a multiple of 64 within its bounds.  The GPU side of the same schedule (non-default chunk knobs, one block or many,
batches that straddle 64-slot fetches) is tests/test_gpu_trace_paths.py::test_launch_shapes."""
import pytest

TAIL_CHUNK = 256            # MCPT_TAIL_CHUNK (trace_persistent.hpp:37)
POOL_WAVES = 16             # MCPT_POOL_WAVES (trace_pool.hpp:45)
CHUNKS = [64, 128, 256, 320, 2048, 1 << 24]


def _c_div(a, b):
    """C++ integer division of non-negative long longs"""
    assert a >= 0 and b > 0
    return a // b


def ticket_range(ticket, total, chunk):
    """[next, range_end) of one ticket (ticket_range, trace_persistent.hpp:77-83)"""
    small = chunk if chunk < TAIL_CHUNK else TAIL_CHUNK
    big_tickets = _c_div(total - _c_div(total, 8), chunk)
    size = chunk if ticket < big_tickets else small
    nxt = ticket * chunk if ticket < big_tickets else big_tickets * chunk + (ticket - big_tickets) * small
    range_end = nxt + size if nxt + size < total else total
    return nxt, range_end


def batches(total, chunk):
    """every 64-slot fetch of the launch, in ticket order: (ticket, reg_base, reg_count)"""
    out = []
    ticket = 0
    while True:
        nxt, range_end = ticket_range(ticket, total, chunk)
        if nxt >= total:
            return out, ticket
        while nxt < range_end:                  # request(): reg_count = min(range_end - next, 64)
            avail = range_end - nxt
            reg_count = avail if avail < 64 else 64
            out.append((ticket, nxt, reg_count))
            nxt += reg_count
        ticket += 1


def wf_chunk(total, grid, block, min_chunk, max_chunk):
    waves = grid * (block >> 6)
    c = _c_div(total, waves * 4)
    c = _c_div(c, 64) * 64
    return min_chunk if c < min_chunk else (max_chunk if c > max_chunk else c)


def persistent_chunk(total, grid_blocks):
    waves = grid_blocks * 4
    c = _c_div(total, waves * 4)
    c = _c_div(c, 64) * 64
    if c < 64:
        c = 64
    if c > 2048:
        c = 2048
    return c


def pool_closest_chunk(total, gp, min_chunk, max_chunk):
    c = _c_div(total, gp * POOL_WAVES * 4)
    c = _c_div(c, 64) * 64
    return min_chunk if c < min_chunk else (max_chunk if c > max_chunk else c)


def chunk_knobs(min_env, max_env):
    """knobs.cpp:83-85 (env_ll: outside 64..2^24 the default) then init_launch_cfg's rounding"""
    def env_ll(v, dflt):
        return dflt if v is None or v < 64 or v > (1 << 24) else v
    lo = env_ll(min_env, 256) // 64 * 64
    hi = env_ll(max_env, 2048) // 64 * 64
    if hi < lo:
        hi = lo
    lo2 = lo // 64 * 64 if lo >= 64 else 256
    hi2 = hi // 64 * 64 if hi >= 64 else 2048
    if hi2 < lo2:
        hi2 = lo2
    return lo2, hi2


def _totals(chunk):
    t = set(range(1, 301)) | {511, 512, 513, 4095, 4096, 4097, (1 << 20) - 1, 1 << 20, (1 << 20) + 1}
    # seven eighths: the totals at which big_tickets steps up (total - total / 8 crosses a multiple of the chunk), and their neighbours
    for k in (1, 2, 3, 17):
        for total in range(max(1, (8 * k * chunk) // 7 - 3), (8 * k * chunk) // 7 + 10):
            if total <= (1 << 21):
                t.add(total)
    return sorted(t)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_tickets_cover_every_slot_once_in_order(chunk):
    for total in _totals(chunk):
        out, n_tickets = batches(total, chunk)
        expect = 0
        last_ticket = -1
        for ticket, base, count in out:
            assert base == expect, (total, chunk, ticket, base, expect)      # contiguous: no slot twice, none skipped, in order
            assert 1 <= count <= 64
            assert ticket >= last_ticket
            last_ticket = ticket
            expect = base + count
        assert expect == total, (total, chunk, expect)
        # every ticket before the last one issued held at least one slot; the first ticket past the end is the only empty one
        assert n_tickets == len({b[0] for b in out})
        big = (total - total // 8) // chunk
        small = min(chunk, TAIL_CHUNK)
        assert n_tickets == big + -(-(total - big * chunk) // small)
        # the big tickets end at or before seven eighths of the total: the last eighth always goes out in tail tickets
        assert big * chunk <= total - total // 8


def test_tail_tickets_and_batches_at_the_edges():
    # one slot: one ticket of one slot (a big ticket only when chunk divides total - total / 8 = 1: never, chunk >= 64)
    assert batches(1, 64)[0] == [(0, 0, 1)]
    # 65 slots of chunk 64: 65 - 8 = 57 < 64, no big ticket; tail tickets of 64: [0, 64), [64, 65)
    assert batches(65, 64)[0] == [(0, 0, 64), (1, 64, 1)]
    # 74 slots: 74 - 9 = 65 -> one big ticket of 64, then tail tickets of 64: [64, 74)
    assert batches(74, 64)[0] == [(0, 0, 64), (1, 64, 10)]
    # chunk 320 and 4097 slots: 4097 - 512 = 3585 -> 11 big tickets (3520 slots), then tail tickets of 256
    out, n = batches(4097, 320)
    assert ticket_range(10, 4097, 320) == (3200, 3520) and ticket_range(11, 4097, 320) == (3520, 3776)
    assert ticket_range(13, 4097, 320) == (4032, 4097) and ticket_range(14, 4097, 320)[0] >= 4097 and n == 14
    # a chunk of 2^24 never makes a big ticket below 2^24 * 8 / 7 slots: every claim is a tail ticket
    assert all(ticket_range(k, 1 << 20, 1 << 24)[1] - ticket_range(k, 1 << 20, 1 << 24)[0] == TAIL_CHUNK for k in range(4096))
    # a range that is not a multiple of 64 ends in a partial batch; the batch after it starts the next ticket
    out, _ = batches(300, 128)
    assert [c for _, _, c in out] == [64, 64, 64, 64, 44]


@pytest.mark.parametrize("knobs", [(None, None), (64, 64), (1 << 24, 1 << 24), (100, 90), (63, 1 << 25), (320, 200), (4096, 2048)])
def test_chunk_formulas_stay_within_their_bounds(knobs):
    lo, hi = chunk_knobs(*knobs)
    assert lo % 64 == 0 and hi % 64 == 0 and 64 <= lo <= hi <= (1 << 24)
    totals = [1, 63, 64, 65, 4095, 4097, 57600, 115200, (1 << 20) + 1, 3 * (1 << 22), 1 << 32]
    for total in totals:
        for grid in (1, 2, 7, 256, 1024, 3072):
            for block in (256, POOL_WAVES * 64):            # k_wf_trace, k_wf_trace_pool
                c = wf_chunk(total, grid, block, lo, hi)
                assert c % 64 == 0 and lo <= c <= hi, (knobs, total, grid, block, c)
            c = persistent_chunk(total, grid)
            assert c % 64 == 0 and 64 <= c <= 2048, (total, grid, c)
            c = pool_closest_chunk(total, grid, lo, hi)
            assert c % 64 == 0 and lo <= c <= hi, (knobs, total, grid, c)
    if knobs == (None, None):
        assert (lo, hi) == (256, 2048)
    if knobs == (64, 64):
        assert (lo, hi) == (64, 64)
    if knobs == (100, 90):          # 100 -> 64, 90 -> 64: rounded down to 64 each
        assert (lo, hi) == (64, 64)
    if knobs == (63, 1 << 25):      # both out of range: the defaults
        assert (lo, hi) == (256, 2048)
    if knobs == (320, 200):         # max below min: raised to min
        assert (lo, hi) == (320, 320)
    # persistent_chunk ignores the knobs: the voting engine's closest-hit and primary launches
    assert persistent_chunk(57600, 1024) == 64 and persistent_chunk(1 << 30, 1024) == 2048 and persistent_chunk(1 << 20, 256) == 256


def test_default_launches_take_big_tickets():
    """What the defaults do with a frame's worth of rays: the chunk lands between the bounds and the first seven eighths go out in big
    tickets (the schedule the GPU tests run most of the time)."""
    lo, hi = chunk_knobs(None, None)
    total = 160 * 90 * 4 * 2                # a small frame's bounce launch: paths x (lights + 1)
    grid = min(-(-total // 2048), 256 * 4)  # launch_wf_trace: a block per MCPT_TRACE_BLOCK_RAYS rays, at most the resident grid
    c = wf_chunk(total, grid, 256, lo, hi)
    assert grid == 57 and c == 256
    big = (total - total // 8) // c
    assert big > 0 and big * c <= total - total // 8
