"""The self-check build of the library for the tests that run it: where it is, how a child process runs under it, and how the three
texts it prints on stderr (MCPT_PRINT_DIAG) are read."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def variant_lib(name="chk", flags="-DMCPT_PRE_CHECK"):
    """csrc/variants/libmcpt_<name>.so, brought up to date by the Makefile (build() has made it: nothing is compiled when it is fresh)"""
    subprocess.check_call(["bash", os.path.join(ROOT, "tools", "build_variant.sh"), name, flags], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "montecarlopathtracing_amd", "csrc", "variants", "libmcpt_%s.so" % name)


def run(code, *argv, timeout):
    """`code` in a fresh Python under the self-check build, diagnostics on, no hand-over to the finishing kernel: the completed process"""
    env = dict(os.environ, MCPT_LIB=variant_lib(), MCPT_PRINT_DIAG="1", MCPT_FINISH_PATHS="0")
    return subprocess.run([sys.executable, "-c", code] + [str(a) for a in argv], capture_output=True, text=True, timeout=timeout, env=env)


def pre_test_failures(stderr):
    """the lines of a failed pre-test self-check: the count and what the pre-test saw of the first offender ([]: none failed)"""
    return [ln for ln in stderr.splitlines() if "PRE-TEST SELF-CHECK" in ln or ln.startswith("  first") or ln.startswith("  ray")]


def survivor_shares(stderr):
    """per frame, the percentage of the visited triangles that survived the pre-test"""
    return [float(x) for x in re.findall(r"\(([0-9.]+) % of the visited triangles survive the pre-test\)", stderr)]


def kernarg_checks(stderr):
    """per frame, (a, b) of `KERNARG CHECK: a of b trace launches`"""
    return [(int(a), int(b)) for a, b in re.findall(r"KERNARG CHECK: (\d+) of (\d+) trace launches", stderr)]
