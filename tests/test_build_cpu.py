"""The build recipe (csrc/Makefile) after build(): nothing left to do, header dependencies that follow the #include lines, one recipe for
the product and the variants, and a rebuild when a variant's flags change.  make's question and dry-run modes only: nothing is compiled,
no source is touched."""
import collections
import glob
import os
import re
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "montecarlopathtracing_amd", "csrc")
CHK = ("VARIANT=chk", "EXTRA=-DMCPT_PRE_CHECK")


def _make(*args):
    return subprocess.run(["make", "-C", CSRC, "--no-print-directory"] + list(args), capture_output=True, text=True)


def _sources():
    """the library's sources as the Makefile picks them: every *.hip and *.cpp but the generated build id and the mtpc executable"""
    names = [os.path.basename(f) for pat in ("*.hip", "*.cpp") for f in glob.glob(os.path.join(CSRC, pat))]
    return sorted(n for n in names if n not in ("build_id.cpp", "mtpc_main.cpp"))


def _objects(text):
    """the objects the compile commands of a dry run write (-c -o <object>), without their directory"""
    return sorted(os.path.basename(o) for o in re.findall(r" -c -o (\S+\.o) ", text))


def _includes(path, seen):
    """every file `path` includes through #include "..." lines, transitively (a scanner of its own: it does not ask the compiler)"""
    for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), re.M):
        f = os.path.normpath(os.path.join(os.path.dirname(path), inc))
        if f not in seen:
            seen.add(f)
            _includes(f, seen)
    return seen


def test_nothing_is_left_to_do_after_build():
    for args in (("all",), CHK):
        out = _make("-q", *args)
        assert out.returncode == 0, (args, out.stdout, out.stderr, _make("-n", *args).stdout[-2000:])


def test_a_changed_header_rebuilds_exactly_its_includers():
    headers = sorted(glob.glob(os.path.join(CSRC, "*.hpp"))) + [os.path.join(ROOT, "include", "mcpt.h")]
    assert len(headers) > 20
    includers = {h: set() for h in headers}
    for src in _sources() + ["mtpc_main.cpp"]:
        for f in _includes(os.path.join(CSRC, src), set()):
            if f in includers:
                includers[f].add(src)
    assert "kernels.hip" in includers[os.path.join(CSRC, "accel_build.hpp")] and "wavefront.hip" in includers[os.path.join(ROOT, "include", "mcpt.h")]
    for h in headers:
        out = _make("-n", "-W", os.path.relpath(h, CSRC), "all")
        assert out.returncode == 0, out.stderr
        # the build id is a hash of every source: it is made again whatever changed
        want = sorted(os.path.splitext(s)[0] + ".o" for s in includers[h] if s != "mtpc_main.cpp") + ["build_id.o"]
        assert _objects(out.stdout) == sorted(want), (os.path.basename(h), _objects(out.stdout), sorted(want))
        assert out.stdout.count(" -shared ") == 1 and out.stdout.count(" -o mtpc ") == 1      # the library, and the executable linked against it


def _normalised(text, out_dir, lib, extra):
    lines = []
    for ln in text.splitlines():
        if " -o mtpc " in ln:
            continue                            # the product's executable: the one thing a variant does not have
        ln = ln.replace(out_dir + "/", "O/").replace(lib, "LIB")
        ln = re.sub(r"O/flags\.[0-9a-f]+", "O/flags.X", ln)
        ln = re.sub(r'return "[0-9a-f]{16}"', 'return "ID"', ln)
        ln = re.sub(r"^(@?)mkdir -p \S+$", r"\1mkdir -p O", ln).replace("rm -f %s/flags.*" % out_dir, "rm -f O/flags.*")
        lines.append(" ".join(w for w in ln.split() if w != extra))
    return collections.Counter(lines)


def test_product_and_variant_are_built_by_the_same_commands():
    prod, var = _make("-n", "-B", "all"), _make("-n", "-B", *CHK)
    assert prod.returncode == 0 and var.returncode == 0, (prod.stderr, var.stderr)
    a = _normalised(prod.stdout, "obj", "libmcpt.so", None)
    b = _normalised(var.stdout, "variants/obj_chk", "variants/libmcpt_chk.so", "-DMCPT_PRE_CHECK")
    assert a == b, (sorted((a - b).elements()), sorted((b - a).elements()))
    assert sum(" -shared -o LIB " in ln and ln.endswith(" -ldl") for ln in a) == 1
    assert _objects(prod.stdout) == sorted(os.path.splitext(s)[0] + ".o" for s in _sources() + ["build_id.cpp"])
    assert all(" -DMCPT_PRE_CHECK " in ln for ln in var.stdout.splitlines() if " -c -o " in ln)
    logic = [ln for ln in prod.stdout.splitlines() if " -c -o " in ln and "disable-machine-licm" in ln]
    assert len(logic) == 1 and " wavefront_logic.hip" in logic[0]


def test_other_flags_rebuild_every_object_of_a_variant():
    assert _make("-q", *CHK).returncode == 0
    out = _make("-n", "VARIANT=chk", "EXTRA=-DOTHER")
    assert out.returncode == 0, out.stderr
    assert _objects(out.stdout) == sorted(os.path.splitext(s)[0] + ".o" for s in _sources() + ["build_id.cpp"])
    assert _make("-q", *CHK).returncode == 0        # (the dry run changed nothing)
