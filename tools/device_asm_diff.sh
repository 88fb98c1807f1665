#!/bin/bash
# tools/device_asm_diff.sh [BASE_REV]: proves that a host-side change left the kernels alone.  For every object of the
# Makefile's OBJS that comes from a .hip file it emits the gfx950 device assembly (the Makefile's own compile line with
# -c replaced by -S --cuda-device-only) at BASE_REV (default HEAD) and in the working tree, then diffs the two after
# dropping only the lines that name the source file or the compiler.  CPU only (hipcc cross-compiles).
# Exit status 0: no device code differs.
set -euo pipefail
BASE=${1:-HEAD}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
WORK=$(mktemp -d)
trap 'git -C "$ROOT" worktree remove --force "$WORK/base" 2>/dev/null || true; rm -rf "$WORK"' EXIT
git -C "$ROOT" worktree add --detach "$WORK/base" "$BASE" >/dev/null

emit() {  # emit <tree> <outdir>: one .s per .hip object, in parallel
    mkdir -p "$2"
    make -C "$1/lut_renderer_amd/csrc" -n -B all | grep -- ' -c [a-z0-9_]*\.hip -o build/' |
        sed -E "s# -c ([a-z0-9_]+\.hip) -o build/([a-z0-9_]+)\.o# -w -S --cuda-device-only \1 -o $2/\2.s#" |
        (cd "$1/lut_renderer_amd/csrc" && xargs -P "${JOBS:-8}" -d '\n' -n 1 sh -c)
    # drop the lines that only name the source file or the compiler; the compilation unit id (__hip_cuid_<hash of the
    # source path>) names the file too and is made anonymous
    sed -i -E '/^\s*\.(file|ident)\b/d; /^\s*- *(clang|Clang)/d; /\.amdgcn\.(producer|ident)/d; s/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g' "$2"/*.s
}

emit "$WORK/base" "$WORK/a"
emit "$ROOT" "$WORK/b"
na=$(ls "$WORK/a" | wc -l); nb=$(ls "$WORK/b" | wc -l)
if diff -r "$WORK/a" "$WORK/b" >"$WORK/diff.txt"; then
    echo "device assembly identical: $nb objects (base $BASE has $na)"
else
    head -50 "$WORK/diff.txt"
    echo "device assembly DIFFERS against $BASE" >&2
    exit 1
fi
