"""csrc/chunks.hpp without a GPU: the chunk plan of the calls that work through a workspace of rays (probe visibility, reflection probes,
baked frames, baked radiance) against a restatement, at the edges of its arguments, under the address and undefined-behaviour sanitizers in
a stand-alone program (tests/chunks_sanitize_main.cpp)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "montecarlopathtracing_amd", "csrc")
DEFAULT = 2 ** 22


def plan(ws, item, n):
    """items per chunk: the budget in whole items, at least one, at most n"""
    return min(n, max(1, (ws or DEFAULT) // item))


def walk(per, n):
    """(chunks, the sum of their counts, the last one's count) of the callers' loop"""
    chunks = -(-n // per)
    return chunks, n, n - (chunks - 1) * per


# The chunk counts the GPU tests assert through stats.launches, as those tests state them: (workspace_rays, rays_per_item, n, chunks).
def _asserted_on_the_gpu():
    out = []
    # tests/test_gpu_visibility.py::test_a_grid_bake_is_its_parts: grids of 1, 7 and 60 probes, per = min(n, max(1, (ws or 2^22) // spp))
    for n in (1, 7, 60):
        for spp in (1, 63, 64, 65):
            for ws in (0, spp, 2 * spp + 1):
                per = min(n, max(1, (ws or 2 ** 22) // spp))
                out.append((ws, spp, n, -(-n // per)))
    # tests/test_gpu_baked.py::test_a_frame_is_the_fold_of_baked_radiance_over_the_camera_rays: 64 x 36 pixels of G samples
    n = 64 * 36
    for G in (1, 3, 16):
        per = (2 * G + 1) // G
        out += [(0, G, n, 1), (G, G, n, n), (2 * G + 1, G, n, (n + per - 1) // per)]
    # tests/test_gpu_baked.py::_check_radiance: baked radiance along a caller's rays, one ray an item under the default budget, is one
    # chunk whatever the list's length there (st.launches == 1)
    out += [(0, 1, n, 1) for n in (1, 257, 64 * 36 * 16)]
    # tests/test_gpu_reflection.py::test_chunking_does_not_change_a_bake: 3 probes of 5 x 5 texels, 3 samples each
    out += [(1, 3, 75, 75), (3, 3, 75, 75), (4, 3, 75, 75), (74, 3, 75, 4), (75 * 3, 3, 75, 1), (10 ** 12, 3, 75, 1)]
    return out


def _edges():
    out = []
    for item in (1, 5, 65, 2 ** 31 - 1):
        for n in (1, 2, 7, 2 ** 31 - 1):
            for ws in (0, 1, item - 1, item, 2 * item + 1, 2 ** 62):
                out.append((ws, item, n))
    out += [(2 ** 62, 2 ** 62, 2 ** 62), (0, 2 ** 62, 1), (2 ** 62, 1, 2 ** 62), (DEFAULT, 1, DEFAULT + 1), (DEFAULT - 1, 1, DEFAULT)]
    return out


def test_the_restatement_by_hand():
    assert plan(0, 1, 10 ** 9) == 2 ** 22 and plan(0, 64, 10 ** 9) == 65536 and plan(0, 2 ** 31 - 1, 5) == 1
    assert plan(200, 65, 13) == 3 and walk(3, 13) == (5, 13, 1)                 # tests/query_family.py: five chunks of 200 rays
    assert plan(7, 8, 3) == 1 and plan(8, 8, 3) == 1 and plan(17, 8, 3) == 2 and plan(2 ** 62, 8, 3) == 3
    assert walk(2, 3) == (2, 3, 1) and walk(3, 3) == (1, 3, 3) and walk(1, 3) == (3, 3, 1)


def test_the_chunk_plan_under_address_and_undefined_sanitizers(tmp_path):
    """A stand-alone program, not the library: nothing loaded into this process is instrumented."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "chunks_sanitize")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I", CSRC,
                           "-o", exe, os.path.join(ROOT, "tests", "chunks_sanitize_main.cpp")])
    asserted = _asserted_on_the_gpu()
    triples = [t[:3] for t in asserted] + _edges()
    out = subprocess.run([exe], input="".join("%d %d %d\n" % t for t in triples), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    got = [tuple(int(v) for v in l.split()) for l in out.stdout.splitlines()]
    assert len(got) == len(triples)
    walked = 0
    for (ws, item, n), g in zip(triples, got):
        per = plan(ws, item, n)
        assert 1 <= per <= n and g[:2] == (per, per * item), (ws, item, n, g)
        if n // per <= 2 ** 20:
            assert g[2:] == walk(per, n), (ws, item, n, g)
            walked += 1
        else:
            assert g[2:] == (-1, -1, -1), (ws, item, n, g)
    assert walked > len(triples) // 2
    for (ws, item, n, chunks), g in zip(asserted, got):
        assert g[2] == chunks, (ws, item, n, chunks, g)
