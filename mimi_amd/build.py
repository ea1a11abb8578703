"""In-tree build of libmimi_hip.so for gfx950 (hipcc cross-compiles without a GPU), and variant libraries from the same code:

    python -m mimi_amd.build [-- flags]                          the library of the package, every source compiled again
    python -m mimi_amd.build --out PATH [--rev REV] [-- flags]   another library (same-box A/B runs: MIMI_HIP_LIBRARY=PATH) from the
                                                                 working tree or a git revision; lib/ is untouched
"""
import contextlib
import os
import re
import shutil
import subprocess
import sys
import tempfile
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libmimi_hip.so")
SOURCES = ["domain.hip", "tensor_p3.hip", "contact.hip", "krylov.hip", "exchange.hip", "pressure.hip", "fold.hip", "surface.hip", "explicit.hip"]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# the one flag list: objects take it without -shared, the link whole, isa_lint's device-only compiles without -shared / -fPIC
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-munsafe-fp-atomics",
         "-Wno-unused-result"]

# kernels whose inline-asm matrix / DPP instructions nothing in the compiler pads: linted at the disassembly level (isa_lint.py)
# as part of the build -- same compiler, same flags, the very assembly that goes into the object (a compiler
# bump or an unrelated edit must not ship a stale-result hazard because a test was not run).  Part of a kernel's mangled name ->
# may it keep registers in scratch memory (the point kernels' asm instructions are ordinary vector ones: no hazard there).
# Every kernel an entry matches is linted: a finding fails the build, and so does a spilled register where the entry says False.
LINT_GATE = {"tensor_p3.hip": {"tp3_contract_kernel": False, "tp3_contract_asm_kernel": False, "tp3_point_kernelILi0ELi0": True,
                               "tp3_point_kernelILi0ELi1": True, "tp3_point_kernelILi0ELi2": True},
             "domain.hip": {"tensor_residual_col_kernel": False}}


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    deps.append(os.path.join(os.path.dirname(HERE), "include", "mimi_hip.h"))
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False, extra_flags=()):
    """Compile every HIP source of the package into mimi_amd/lib/libmimi_hip.so."""
    if not force and not _stale():
        return LIB
    os.makedirs(LIBDIR, exist_ok=True)
    # one builder at a time (the ranks of a multi-GPU job all come through here at once); whoever waited finds it done
    import fcntl
    with open(os.path.join(LIBDIR, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and not _stale():
                return LIB
            # lib/obj holds linted objects of the plain flags only, so that no later build can link another kind: those are
            # compiled, all of them, into a directory that ends with the call
            keep = not extra_flags and os.environ.get("MIMI_HIP_BUILD_NO_LINT") != "1"
            return _link(CSRC, SOURCES, LIB, os.path.join(LIBDIR, "obj") if keep else None, force, verbose, extra_flags)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def variant(out, rev=None, extra_flags=(), verbose=False):
    """Every source of the working tree, or of git revision `rev` (by its own SOURCES list), into the library `out`.  The
    working tree's kernels pass the lint gate as in build(); a revision's do not: their gate is that revision's."""
    if not rev:
        return _link(CSRC, SOURCES, os.path.abspath(out), None, True, verbose, extra_flags)
    import runpy
    with tempfile.TemporaryDirectory() as work:
        tar = subprocess.run(["git", "-C", os.path.dirname(HERE), "archive", rev, "mimi_amd/build.py", "mimi_amd/csrc", "include"],
                             stdout=subprocess.PIPE, check=True)
        subprocess.run(["tar", "-x", "-C", work], input=tar.stdout, check=True)
        sources = runpy.run_path(os.path.join(work, "mimi_amd", "build.py"))["SOURCES"]
        return _link(os.path.join(work, "mimi_amd", "csrc"), sources, os.path.abspath(out), None, True, verbose, extra_flags, lint=False)


def _link(csrc, sources, out, objdir, force, verbose, extra_flags=(), lint=True):
    """objdir None: a temporary one"""
    gate = lint_gate(verbose) if lint and os.environ.get("MIMI_HIP_BUILD_NO_LINT") != "1" else None
    with (contextlib.nullcontext(objdir) if objdir else tempfile.TemporaryDirectory()) as objdir:
        # one translation unit per source, compiled side by side
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=len(sources)) as pool:
            objs = list(pool.map(lambda s: compile_object(s, objdir, csrc, extra_flags, force, gate, verbose), sources))
        cmd = [HIPCC] + FLAGS + ["-o", out + ".tmp"] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=csrc)
    os.replace(out + ".tmp", out)
    return out


def read_depfile(depfile, cwd):
    """the prerequisites of the make rule the compiler wrote (-MD): a backslash at the end of a line continues it, `\\ ` is a
    space inside a name, `$$` a dollar; names are relative to the directory the compiler ran in"""
    with open(depfile) as f:
        rule = f.read().replace("\\\n", " ")
    names = re.findall(r"(?:\\.|\S)+", re.split(r":\s", rule, maxsplit=1)[1])
    return [os.path.join(cwd, re.sub(r"\\(.)", r"\1", n).replace("$$", "$")) for n in names]


def compile_object(src, objdir, csrc=None, extra_flags=(), force=False, gate=None, verbose=False):
    """<csrc>/<src> -> <objdir>/<stem>.o, beside it <stem>.d (what it was compiled from) and <stem>.lint.s: with
    -save-temps=obj the device assembly that IS assembled into the object stays -- what the hazard lint and the tests read
    is the shipped code, not a second compilation of it.  The object is current while it is newer than every file the
    depfile names and this source is one of them.  Otherwise everything is compiled under temporary names and `gate(src, assembly file)` runs before any
    of it gets its name: a source the gate refuses leaves no object behind."""
    csrc = csrc or CSRC
    stem = os.path.join(objdir, src[:-len(".hip")])
    with contextlib.suppress(OSError):            # (a file that is missing: the object, its depfile, something it was compiled from)
        t = os.path.getmtime(stem + ".o")
        deps = read_depfile(stem + ".d", csrc)
        # (a depfile that does not name this very source was written in another tree, of which this one is a copy: its
        # files are not the ones this object has to follow)
        own = os.path.realpath(os.path.join(csrc, src)) in {os.path.realpath(d) for d in deps}
        if not force and own and os.path.exists(stem + ".lint.s") and all(os.path.getmtime(d) < t for d in deps):
            return stem + ".o"
    os.makedirs(objdir, exist_ok=True)
    with tempfile.TemporaryDirectory(prefix=src + ".", dir=objdir) as tmp:
        t = os.path.join(tmp, os.path.basename(stem))
        cmd = ([HIPCC] + [f for f in FLAGS if f != "-shared"] + ["-save-temps=obj", "-c", os.path.join(csrc, src), "-o", t + ".o",
                                                                 "-MD", "-MF", t + ".d"] + list(extra_flags))
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=csrc)
        asm = t + "-hip-amdgcn-amd-amdhsa-gfx950.s"
        if gate:
            gate(src, asm)
        for a, b in ((asm, stem + ".lint.s"), (t + ".d", stem + ".d"), (t + ".o", stem + ".o")):     # (the object last)
            os.replace(a, b)
    return stem + ".o"


def lint_gate(verbose):
    """the hazard lint of one build, as compile_object's `gate`; calibrated once, by the first gated source that gets there"""
    from . import isa_lint
    lock, need = threading.Lock(), []

    def gate(src, asm_file):
        if src not in LINT_GATE:
            return
        with lock:
            if not need:
                need.append(isa_lint.calibrate())
        with open(asm_file) as f:
            asm = f.read()
        spills = isa_lint.spill_counts(asm)
        for entry, may_spill in LINT_GATE[src].items():
            kernels = [n for n in spills if entry in n]
            if not kernels:
                raise RuntimeError(f"{src}: the lint gate's entry {entry} matches no kernel")
            for kernel in kernels:
                bad, stats = isa_lint.lint_kernel(isa_lint.parse_kernel(asm, kernel), need[0], asm_only=True)
                if verbose:
                    print(f"lint {kernel}: {len(bad)} findings, {stats['mfma_from_asm']} asm matrix instructions, "
                          f"nearest reads {stats['nearest_valu_read']} / {stats['nearest_mem']}, spills {spills[kernel]}", flush=True)
                if bad or (spills[kernel] and not may_spill):
                    lines = "\n".join(f"  {what}: {dist} < {req}\n    {a}\n    {b}" for a, b, dist, req, what in bad[:10])
                    raise RuntimeError(f"{src}: {kernel} fails the ISA hazard lint ({len(bad)} findings, "
                                       f"{spills[kernel]} spilled registers)\n{lines}")
    return gate


if __name__ == "__main__":
    import argparse
    argv, flags = sys.argv[1:], []
    if "--" in argv:
        argv, flags = argv[:argv.index("--")], argv[argv.index("--") + 1:]
    ap = argparse.ArgumentParser(prog="python -m mimi_amd.build", epilog="behind `--`: extra hipcc flags")
    ap.add_argument("--out", help="build this library instead of the package's, through a temporary object directory")
    ap.add_argument("--rev", help="with --out: the sources of this git revision instead of the working tree's")
    args = ap.parse_args(argv)
    if args.rev and not args.out:
        ap.error("--rev needs --out")
    print(variant(args.out, args.rev, flags, True) if args.out else build(True, True, flags))
