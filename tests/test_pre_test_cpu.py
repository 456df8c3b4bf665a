"""Not gpu: csrc/pre_test.hpp, the arithmetic of the trace engines' conservative fp32 pre-test of a leaf triangle in its branch-free
form (five rejection comparisons and `clear` evaluated unconditionally and combined with | and &).  The header is compiled by the host
compiler into a stand-alone program (tests/pre_test_main.cpp) that carries the short-circuit form it replaced, verbatim, as the model,
and compares the two input for input: the same bool, and the eight debug words bit for bit (where a word is NaN,
NaN in both: the sign and payload of a NaN result are the host compiler's choice of operand order).

- random: 1.2 million seeded (record, ray, limit, margin) tuples around cornell-box's extents: triangles with edges of 0.003 to 2,
  rays aimed at the triangle's plane with weights in [-0.1, 1.1], away from it, or anywhere; half of them without a limit, one
  triangle in 97 with the pre-test switched off.  Each answer occurs in at least a tenth of the cases.
- edges: a1 = +inf; eta4 = +inf; limit = +inf and 0; margin = +inf; det = 0, -0, +-denormal and +-the smallest normal; NaN, -NaN, +inf
  and -inf in each of the 21 input positions, one at a time, on six base cases (inside, and rejected by each comparison alone); a
  triangle seen edge-on, |det| through the 81 floats around 2^-9 X; each of the five comparisons, the limit and the margin through the
  81 floats around its bound, for det > 0 and det < 0 -- the answer changes exactly once in every such sweep.

-O2 -ffp-contract=off, as the issue of the change asks; the same program built with -fsanitize=address,undefined runs both modes."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "montecarlopathtracing_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "pre_test_main.cpp")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I", CSRC]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pre_test") / "pre_test")
    subprocess.check_call(["g++", "-O2"] + FLAGS + ["-o", out, MAIN])
    return out


def _run(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    return out.stdout


def test_random_tuples_against_the_short_circuit_form(exe):
    out = _run(exe, "random")
    cases, rejected = int(out.split()[2]), int(out.split()[3])
    assert out.startswith("ok random ") and cases >= 10 ** 6
    assert cases // 10 < rejected < cases - cases // 10


def test_edge_inputs_against_the_short_circuit_form(exe):
    out = _run(exe, "edges")
    # 6 base cases x (5 switches + 8 determinants + 21 positions x 4 values) + 2 + 5 x 2 + 2 sweeps of 81
    assert out.startswith("ok edges ") and int(out.split()[2]) >= 6 + 6 * (5 + 8 + 21 * 4) + 14 * 81


def test_under_the_host_sanitizers(tmp_path):
    exe = str(tmp_path / "pre_test_san")
    subprocess.check_call(["g++", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + FLAGS + ["-o", exe, MAIN])
    assert _run(exe, "random", "200000").startswith("ok random ")
    assert _run(exe, "edges").startswith("ok edges ")
