#!/bin/sh
# usage: scripts/device_asm.sh <outdir>    (no GPU needed; JOBS=n compiles n files at a time)
# Writes the gfx950 device assembly of every object of the csrc Makefile, compiled with that object's own
# flags, to <outdir>/<name>.s.  A refactor that leaves the kernels alone leaves every file identical under cmp
# (-cuid: the compilation unit id is otherwise a hash of the source's path, which differs between two checkouts).
set -eu
mkdir -p "$1" && out=$(cd "$1" && pwd)
cd "$(dirname "$0")/../node2vec_amd/csrc"
make -s -n -B | grep -e ' -c [a-z0-9_]*\.hip ' |
    sed -E "s/ -MMD -MP -MF [^ ]+ -MT [^ ]+//; s# -c ([a-z0-9_]+)\.hip -o [^ ]+# --offload-device-only -S -cuid=\1 \1.hip -o $out/\1.s#" |
    xargs -d '\n' -P "${JOBS:-8}" -n 1 sh -c
ls "$out"/*.s | wc -l
