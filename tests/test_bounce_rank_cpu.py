"""Not gpu: bounce_first_rank (csrc/wave_rank.hpp), the function by which a wave of k_wf_logic orders its 64 vertices within its 64 output
positions -- those with a bounce ray first.  The header is compiled by the host compiler into a stand-alone program
(tests/bounce_rank_main.cpp) that prints the 64 ranks of every mask it is given.  For the masks 0, all ones, every single bit, the two
alternating patterns and 1 000 seeded random masks (of every density: a random mask and-ed / or-ed with others):
- the ranks are a permutation of 0 .. 63 (no two vertices on one position, no position of the run left out);
- every set lane ranks below every clear lane (the words only a bounce ray needs fill the head of the run);
- lane order is kept inside both groups (a lane that takes no part in the ballot -- the tail of a partial wave, a clear bit above every
  lane that does -- therefore ranks above every lane that does)."""
import os
import subprocess

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "montecarlopathtracing_amd", "csrc")
ALL = (1 << 64) - 1


def _masks():
    m = [0, ALL] + [1 << b for b in range(64)] + [0x5555555555555555, 0xAAAAAAAAAAAAAAAA]
    rng = np.random.default_rng(20)
    r = [int(x) for x in rng.integers(0, 1 << 63, size=3000, dtype=np.uint64) * 2 + rng.integers(0, 2, size=3000, dtype=np.uint64)]
    for i in range(1000):
        a, b, c = r[3 * i], r[3 * i + 1], r[3 * i + 2]
        m.append((a, a & b, a | b, a & b & c, a | b | c)[i % 5])       # densities 1/2, 1/4, 3/4, 1/8, 7/8
    return m


def test_bounce_rays_first_in_lane_order(tmp_path):
    exe = str(tmp_path / "bounce_rank")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "bounce_rank_main.cpp")])
    masks = _masks()
    assert len(masks) == 2 + 64 + 2 + 1000
    out = subprocess.run([exe], input="".join("%x\n" % m for m in masks), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stderr == ""
    ranks = np.array([[int(x) for x in line.split()] for line in out.stdout.splitlines()])
    assert ranks.shape == (len(masks), 64)
    for m, rk in zip(masks, ranks):
        assert sorted(rk) == list(range(64)), hex(m)
        has = [l for l in range(64) if (m >> l) & 1]
        no = [l for l in range(64) if not (m >> l) & 1]
        # set lanes take ranks 0 .. popcount - 1 in lane order, clear lanes the rest in lane order: both orders kept, every set lane
        # below every clear one
        assert [rk[l] for l in has] == list(range(len(has))), hex(m)
        assert [rk[l] for l in no] == list(range(len(has), 64)), hex(m)
