"""The build pipeline itself (mimi_amd/build.py; no GPU): what libmimi_hip.so holds is what csrc holds, and it has passed the
lint gate.  The build runs on a tiny tree -- two one-kernel sources, a header each, a shared header, and an .inc one source
includes through a macro as tensor_p3.hip includes its generated loop -- with the module's paths, source list and gate
pointed at it (the functions read them when called).  An object is compiled again exactly when a file its depfile names is
newer; a kernel the gate refuses leaves no object, so that a second build cannot link it; isa_lint.assembly() of a source of
the library reads the assembly kept from that object's compilation and writes nothing."""
import os
import shutil
import subprocess
import time

import pytest

from mimi_amd import build, isa_lint
from _hazard import HAZARD, PAD_STATEMENT, SAFE_STATEMENT

pytestmark = pytest.mark.skipif(not os.path.exists(build.HIPCC), reason="no hipcc: nothing to compile")

HAZARD_PAD = '#define A_PAD asm volatile("s_nop 0");\n'          # 1 wait state where 19 are needed
SAFE_PAD = "#define A_PAD %s\n" % SAFE_STATEMENT
A_HIP = '#include "shared.hpp"\n#include "a.hpp"\n#ifndef A_INC\n#define A_INC "a_loop.inc"\n#endif\n#include A_INC\n' + \
    HAZARD.replace(PAD_STATEMENT, "A_PAD")
# two instantiations of one kernel: the first waits for the matrix instruction's result, the second as b.hpp says
B_HIP = r"""
#include "shared.hpp"
#include "b.hpp"
typedef double d4 __attribute__((ext_vector_type(4)));
template <int ID, bool SAFE> __global__ void twin_kernel(const double* a, const double* b, double* out) {
  d4 c;
  const double x = a[threadIdx.x], y = b[threadIdx.x];
  asm volatile("s_nop 1\n\tv_mfma_f64_16x16x4_f64 %0, %1, %2, 0" : "=&v"(c) : "v"(x), "v"(y));
  if (SAFE) asm volatile("s_nop 15\n\ts_nop 2"); else asm volatile("s_nop 0");
  double s;
  asm volatile("v_add_f64 %0, %1, %2" : "=v"(s) : "v"(c[0]), "v"(c[1]));
  out[threadIdx.x] = s * SHARED_ONE;
}
template __global__ void twin_kernel<0, true>(const double*, const double*, double*);
template __global__ void twin_kernel<1, B_SECOND_SAFE>(const double*, const double*, double*);
"""


class Tree:
    def __init__(self, root):
        self.csrc, self.libdir = os.path.join(root, "csrc"), os.path.join(root, "lib")
        self.obj, self.lib = os.path.join(self.libdir, "obj"), os.path.join(self.libdir, "libtiny.so")
        os.makedirs(self.csrc)
        for name, text in (("shared.hpp", "#pragma once\n#include <hip/hip_runtime.h>\n#define SHARED_ONE 1.0\n"),
                           ("a.hpp", SAFE_PAD), ("a_loop.inc", "#define A_LOOP 1\n"), ("a.hip", A_HIP),
                           ("b.hpp", "#define B_SECOND_SAFE true\n"), ("b.hip", B_HIP)):
            self.write(name, text)

    def write(self, name, text):
        with open(os.path.join(self.csrc, name), "w") as f:
            f.write(text)
        self.touch(name)

    def touch(self, name):
        # (the clock itself, not the file system's stamp of "now": that one lags by a tick, and a file touched within
        # the tick in which the library was written would not be newer than it)
        now = time.time_ns()
        os.utime(os.path.join(self.csrc, name), ns=(now, now))

    def mtimes(self):
        return {f: os.stat(p).st_mtime_ns for f, p in (("a", os.path.join(self.obj, "a.o")), ("b", os.path.join(self.obj, "b.o")),
                                                       ("lib", self.lib))}


@pytest.fixture
def tree(tmp_path, monkeypatch):
    t = Tree(str(tmp_path))
    for name, value in (("CSRC", t.csrc), ("LIBDIR", t.libdir), ("LIB", t.lib), ("SOURCES", ["a.hip", "b.hip"]), ("LINT_GATE", {})):
        monkeypatch.setattr(build, name, value)
    monkeypatch.delenv("MIMI_HIP_BUILD_NO_LINT", raising=False)
    return t


@pytest.mark.parametrize("touched, recompiled, kept", [("a_loop.inc", "a", "b"),        # (1) included through a macro
                                                       ("b.hpp", "b", "a")])            # (2) a header of one source
def test_a_touched_file_recompiles_only_the_objects_that_include_it(tree, touched, recompiled, kept):
    assert build.build() == tree.lib
    before = tree.mtimes()
    tree.touch(touched)
    build.build()
    after = tree.mtimes()
    assert after[recompiled] > before[recompiled] and after[kept] == before[kept] and after["lib"] > before["lib"]


def test_a_kernel_the_gate_refuses_leaves_no_object_for_the_next_build_to_link(tree, monkeypatch):
    monkeypatch.setattr(build, "LINT_GATE", {"a.hip": {"hazard_kernel": False}})
    tree.write("a.hpp", HAZARD_PAD)
    for _ in range(2):                                   # (the second build is the retry, or the job's second rank)
        with pytest.raises(RuntimeError, match="hazard_kernel fails the ISA hazard lint"):
            build.build()
        assert not os.path.exists(tree.lib) and not os.path.exists(os.path.join(tree.obj, "a.o"))
    tree.write("a.hpp", SAFE_PAD)
    assert build.build() == tree.lib and os.path.exists(tree.lib)


def test_an_object_compiled_with_the_lint_off_is_not_linked_by_a_build_with_the_lint_on(tree, monkeypatch):
    monkeypatch.setattr(build, "LINT_GATE", {"a.hip": {"hazard_kernel": False}})
    tree.write("a.hpp", HAZARD_PAD)
    monkeypatch.setenv("MIMI_HIP_BUILD_NO_LINT", "1")
    assert build.build() == tree.lib
    monkeypatch.delenv("MIMI_HIP_BUILD_NO_LINT")
    unlinted = os.stat(tree.lib).st_mtime_ns
    # the link has to run again, and nothing of a.hip was touched: for the other source's sake, then for want of a library
    tree.touch("b.hpp")
    with pytest.raises(RuntimeError, match="hazard_kernel fails the ISA hazard lint"):
        build.build()
    assert os.stat(tree.lib).st_mtime_ns == unlinted
    os.remove(tree.lib)
    with pytest.raises(RuntimeError, match="hazard_kernel fails the ISA hazard lint"):
        build.build()
    assert not os.path.exists(tree.lib)


def test_a_gate_entry_lints_every_kernel_it_matches_and_must_match_one(tree, monkeypatch):
    monkeypatch.setattr(build, "LINT_GATE", {"b.hip": {"twin_kernel": False, "renamed_kernel": False}})
    with pytest.raises(RuntimeError, match="renamed_kernel matches no kernel"):
        build.build()
    monkeypatch.setattr(build, "LINT_GATE", {"b.hip": {"twin_kernel": False}})
    assert build.build() == tree.lib                     # both instantiations wait
    tree.write("b.hpp", "#define B_SECOND_SAFE false\n")
    with pytest.raises(RuntimeError, match=r"twin_kernelILi1ELb0EE\w+ fails the ISA hazard lint"):
        build.build()


def test_a_current_library_is_used_as_it_is_without_objects_and_without_a_compiler(tree, monkeypatch):
    build.build()
    before = tree.mtimes()

    def started(*args, **kwargs):
        raise AssertionError(f"build() started a process: {args}")
    monkeypatch.setattr(subprocess, "Popen", started)
    assert build.build() == tree.lib and tree.mtimes() == before
    shutil.rmtree(tree.obj)                              # (what a machine gets that is sent the library without its objects)
    assert build.build() == tree.lib and os.stat(tree.lib).st_mtime_ns == before["lib"]
    assert not os.path.exists(tree.obj)


def test_assembly_of_a_library_source_is_the_object_s_own_and_is_never_written_by_reading_it(tree):
    build.build()
    shipped = os.path.join(tree.obj, "a.lint.s")
    with open(shipped) as f:
        text, stamp = f.read(), os.stat(shipped).st_mtime_ns
    assert "hazard_kernel" in text and isa_lint.assembly("a.hip") == text
    with open(shipped) as f:
        assert f.read() == text and os.stat(shipped).st_mtime_ns == stamp
    # another compilation of the same source goes elsewhere
    assert "hazard_kernel" in isa_lint.assembly("a.hip", extra_flags=["-DA_OTHER"])
    assert os.stat(shipped).st_mtime_ns == stamp
    # a stale object is compiled again, object and assembly together
    before = tree.mtimes()
    tree.touch("a.hpp")
    assert "hazard_kernel" in isa_lint.assembly("a.hip")
    after = tree.mtimes()
    assert after["a"] > before["a"] and os.stat(shipped).st_mtime_ns > stamp and after["b"] == before["b"]


def test_a_copied_tree_follows_its_own_files_not_those_of_the_tree_it_was_copied_from(tree, tmp_path, monkeypatch):
    """the depfiles hold the absolute names of the tree the objects were compiled in: in a copy of that tree (objects and
    all) an object whose depfile names the ORIGINAL's files is compiled again, and then follows the copy's"""
    build.build()
    copy = str(tmp_path / "copy")
    shutil.copytree(tree.csrc, os.path.join(copy, "csrc"), copy_function=shutil.copy2)
    shutil.copytree(tree.libdir, os.path.join(copy, "lib"), copy_function=shutil.copy2)
    csrc, obj = os.path.join(copy, "csrc"), os.path.join(copy, "lib", "obj")
    before = os.stat(os.path.join(obj, "a.o")).st_mtime_ns
    assert os.path.realpath(os.path.join(tree.csrc, "a.hip")) in {os.path.realpath(d) for d in build.read_depfile(os.path.join(obj, "a.d"), csrc)}
    build.compile_object("a.hip", obj, csrc)
    deps = {os.path.realpath(d) for d in build.read_depfile(os.path.join(obj, "a.d"), csrc)}
    assert os.stat(os.path.join(obj, "a.o")).st_mtime_ns > before
    assert {os.path.realpath(os.path.join(csrc, f)) for f in ("a.hip", "a.hpp", "shared.hpp", "a_loop.inc")} <= deps
    assert not any(d.startswith(os.path.realpath(tree.csrc) + os.sep) for d in deps)
    # and is current from then on
    again = os.stat(os.path.join(obj, "a.o")).st_mtime_ns
    build.compile_object("a.hip", obj, csrc)
    assert os.stat(os.path.join(obj, "a.o")).st_mtime_ns == again


def test_the_depfile_is_read_as_make_reads_it(tmp_path):
    d = tmp_path / "x.d"
    d.write_text("/tmp/o/x.o: /src/x.hip \\\n  common.hpp ../../include/mimi\\ hip.h \\\n  /opt/a$$b.h\n")
    assert build.read_depfile(str(d), "/src") == ["/src/x.hip", "/src/common.hpp", "/src/../../include/mimi hip.h", "/opt/a$b.h"]


def test_the_degree3_object_depends_on_its_generated_loop_and_on_every_header_it_includes():
    """on the real tree: lib/obj/tensor_p3.d names tp3_contract_loop.inc (included through T3_LOOP_INC) and every file of csrc
    that tensor_p3.hip includes, directly or through another"""
    import re
    build.build()
    isa_lint.assembly("tensor_p3.hip")                   # (the object is there and current, whatever the library came from)
    deps = {os.path.realpath(p) for p in build.read_depfile(os.path.join(build.LIBDIR, "obj", "tensor_p3.d"), build.CSRC)}
    included, todo = set(), ["tensor_p3.hip"]
    while todo:
        with open(os.path.join(build.CSRC, todo.pop())) as f:
            for name in re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M):
                path = os.path.realpath(os.path.join(build.CSRC, name))
                if path not in included and os.path.exists(path):
                    included.add(path)
                    todo.append(name)
    assert len(included) >= 3 and os.path.realpath(os.path.join(build.CSRC, "common.hpp")) in included
    assert os.path.realpath(os.path.join(build.CSRC, "tp3_contract_loop.inc")) in deps
    assert included <= deps, sorted(included - deps)
