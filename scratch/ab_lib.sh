#!/bin/bash
# usage: scratch/ab_lib.sh NAME [GIT_REV|-] [extra hipcc flags...]  ->  scratch/lib_NAME.so: every source of
# mimi_amd.build.SOURCES, of the working tree (no revision, or "-") or of GIT_REV, compiled with the build's flags plus the
# extra ones, for same-box A/B runs (MIMI_HIP_LIBRARY=scratch/lib_NAME.so python bench.py ...).  The library of a revision
# is built where the git history is and travels as the git-ignored scratch/lib_NAME.so.
set -e
name=$1; rev=$2; shift; shift || true
root=$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)
work=$(mktemp -d); trap 'rm -rf "$work"' EXIT
tree=$root
if [ -n "$rev" ] && [ "$rev" != "-" ]; then
  git -C "$root" archive "$rev" mimi_amd/build.py mimi_amd/csrc include | tar -x -C "$work"
  tree=$work
fi
sources=$(python3 -c "import runpy, sys; print(' '.join(runpy.run_path(sys.argv[1])['SOURCES']))" "$tree/mimi_amd/build.py")
cd "$tree/mimi_amd/csrc"
pids=()
for s in $sources; do
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics -Wno-unused-result "$@" -c "$s" -o "$work/${s%.hip}.o" & pids+=($!)
done
for p in "${pids[@]}"; do wait "$p"; done
hipcc --offload-arch=gfx950 -shared -fPIC -o "$root/scratch/lib_$name.so" $(for s in $sources; do echo "$work/${s%.hip}.o"; done)
echo scratch/lib_$name.so
