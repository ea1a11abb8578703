#!/usr/bin/env python3
"""usage: scratch/isa_diff.py REV [source...]   (default sources: domain.hip tensor_p3.hip)

Device code of a refactor against its parent: compiles the named sources of mimi_amd/csrc device-only for gfx950 with the
build's flags (isa_lint.ASM_FLAGS), once from `git archive REV` and once from the working tree, and reports per kernel
symbol whether the instruction stream (isa_lint.parse_kernel; local labels renumbered, since they carry the position of
the function in the file) and the resource block (the .amdhsa_kernel directives and isa_lint.kernel_resources) are
identical, and which kernels exist on one side only.  Exit status 0 = same symbols, every kernel identical.
Cost on a CPU box: domain.hip is 153 kernels and 74 s per side; the sides and sources compile side by side."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mimi_amd import isa_lint  # noqa: E402


def compile_side(tree, source, out):
    src = os.path.join(tree, "mimi_amd", "csrc", source)
    run = subprocess.run([isa_lint.HIPCC] + isa_lint.ASM_FLAGS + ["-o", out, src], cwd=os.path.dirname(src),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if run.returncode != 0:
        raise RuntimeError(f"hipcc -S {src} failed:\n{run.stderr[-4000:]}")
    with open(out) as f:
        return f.read()


def kernels_of(asm):
    """{symbol: (instruction texts, resource block)}"""
    res = isa_lint.kernel_resources(asm)
    out = {}
    for name in res:
        stream = [re.sub(r"\.LBB\d+_", ".LBB_", i.text) for i in isa_lint.parse_kernel(asm, name)]
        m = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(name), asm, re.S)
        out[name] = (stream, (m.group(1) if m else "", sorted(res[name].items())))
    return out


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    rev, sources = sys.argv[1], sys.argv[2:] or ["domain.hip", "tensor_p3.hip"]
    bad = 0
    with tempfile.TemporaryDirectory() as work:
        old = os.path.join(work, "old")
        os.makedirs(old)
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "mimi_amd/csrc", "include"], stdout=subprocess.PIPE, check=True)
        subprocess.run(["tar", "-x", "-C", old], input=tar.stdout, check=True)
        jobs = [(side, tree, s) for s in sources for side, tree in (("old", old), ("new", ROOT))]
        with ThreadPoolExecutor(max_workers=len(jobs)) as pool:
            asms = list(pool.map(lambda j: compile_side(j[1], j[2], os.path.join(work, f"{j[0]}_{j[2]}.s")), jobs))
        for k, s in enumerate(sources):
            a, b = kernels_of(asms[2 * k]), kernels_of(asms[2 * k + 1])
            only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
            diff_i = sorted(n for n in set(a) & set(b) if a[n][0] != b[n][0])
            diff_r = sorted(n for n in set(a) & set(b) if a[n][1] != b[n][1])
            print(f"{s}: {len(a)} kernels at {rev}, {len(b)} in the working tree; {len(set(a) & set(b)) - len(set(diff_i) | set(diff_r))} identical")
            for n in only_a:
                print(f"  only at {rev}: {n}")
            for n in only_b:
                print(f"  only in the working tree: {n}")
            for n in diff_i:
                print(f"  instruction stream differs: {n} ({len(a[n][0])} -> {len(b[n][0])} instructions)")
            for n in diff_r:
                print(f"  resource block differs: {n}")
            # what decides a changed kernel's occupancy, before -> after (workgroups of 256 threads; dynamic LDS is the launcher's)
            for n in sorted(set(diff_i) | set(diff_r) | set(only_a) | set(only_b)):
                for side, k in ((rev, a.get(n)), ("working tree", b.get(n))):
                    if k:
                        res = dict(k[1][1])
                        sgpr = re.search(r"\.amdhsa_next_free_sgpr (\d+)", k[1][0])
                        print(f"    {n} at {side}: {len(k[0])} instructions, {res} sgpr {sgpr.group(1) if sgpr else '?'}, "
                              f"{isa_lint.waves_per_simd(res, 256):g} waves per SIMD")
            bad += len(only_a) + len(only_b) + len(diff_i) + len(diff_r)
    print("IDENTICAL" if not bad else f"DIFFERENT ({bad} findings)")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
