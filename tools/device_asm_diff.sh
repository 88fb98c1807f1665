#!/bin/bash
# tools/device_asm_diff.sh [--usage] [BASE_REV]: proves that a host-side change left the kernels alone.  For every object of the
# Makefile's OBJS that comes from a .hip file it emits the gfx950 device assembly (the Makefile's own compile line with
# -c replaced by -S --cuda-device-only) at BASE_REV (default HEAD) and in the working tree, then diffs the two after
# dropping only the lines that name the source file or the compiler.  CPU only (hipcc cross-compiles).
# Exit status 0: no device code differs.
# --usage: for a change that is meant to move device code.  Where assembly differs it lists the objects, reads each kernel's
# (NumVgprs, NumAgprs, ScratchSize, Occupancy, LDS bytes, codeLenInByte) from the compiler's own trailer on both sides and prints,
# per object, how many kernels changed and how far VGPRs and code length moved, then each kernel whose other figures changed.
# Exit status 0 unless a kernel lost occupancy, gained scratch or AGPRs where the base has none, changed its LDS size, or exists
# on one side only.
set -euo pipefail
USAGE=0
if [ "${1:-}" = "--usage" ]; then USAGE=1; shift; fi
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

usage() {  # usage <dir>: "object:kernel vgprs agprs scratch occupancy lds codelen" per kernel, sorted by that key as join wants it
    awk '$1 == ".amdhsa_kernel" { k = $2 }
         $1 == ";" && $2 == "codeLenInByte" { len = $4 }
         $1 == ";" && $2 == "NumVgprs:" { v = $3 }
         $1 == ";" && $2 == "NumAgprs:" { a = $3 }
         $1 == ";" && $2 == "ScratchSize:" { s = $3 }
         $1 == ";" && $2 == "LDSByteSize:" { l = $3 }
         $1 == ";" && $2 == "Occupancy:" { o = FILENAME; sub(/.*\//, "", o); sub(/\.s$/, "", o); print o ":" k, v, a, s, $3, l, len }' "$1"/*.s |
        LC_ALL=C sort
}

usage_diff() {  # usage_diff <dir a> <dir b>: one line per object whose assembly differs (VGPR and code length moves, recorded),
    # then every kernel whose occupancy, scratch, AGPRs or LDS changed (gated)
    for f in "$2"/*.s; do cmp -s "$1/$(basename "$f")" "$f" || echo "assembly differs: $(basename "$f" .s)"; done
    LC_ALL=C join -a 1 -a 2 -e - -o 0,1.2,1.3,1.4,1.5,1.6,1.7,2.2,2.3,2.4,2.5,2.6,2.7 <(usage "$1") <(usage "$2") |
        awk 'function mm(k, d) { if (!(k in lo) || d < lo[k]) lo[k] = d; if (!(k in hi) || d > hi[k]) hi[k] = d }
             { n++; same = 1; for (i = 2; i <= 7; i++) if ($i != $(i + 6)) same = 0
               if (same) next
               c++; split($1, p, ":"); o = p[1]; cnt[o]++; mm(o " v", $8 - $2); mm(o " len", $13 - $7)
               if ($3 == $9 && $4 == $10 && $5 == $11 && $6 == $12) next
               k = p[2]; sub(/^_ZN4lutr[0-9]+/, "", k); sub(/EEEv.*/, "", k)
               line = sprintf("%s %s  vgprs %s -> %s  agprs %s -> %s  scratch %s -> %s  occupancy %s -> %s  lds %s -> %s", o, k, $2, $8, $3, $9, $4, $10, $5, $11, $6, $12)
               if ($2 == "-" || $8 == "-" || $11 + 0 < $5 + 0 || ($4 == 0 && $10 != 0) || ($3 == 0 && $9 != 0) || $6 != $12) { bad++; line = line "  FAILS a condition" }
               gated[++g] = line }
             END { print "per object: kernels whose usage changed, VGPR delta min .. max, code length delta min .. max (bytes)"
                   for (o in cnt) printf "%s  %d  vgprs %+d .. %+d  len %+d .. %+d\n", o, cnt[o], lo[o " v"], hi[o " v"], lo[o " len"], hi[o " len"] | "sort"
                   close("sort")
                   print "kernels whose occupancy, scratch, AGPRs or LDS changed, base -> tree:"
                   for (i = 1; i <= g; i++) print gated[i]
                   printf "%d kernels, %d changed, %d fail a condition\n", n, c, bad; exit bad > 0 }'
}

emit "$WORK/base" "$WORK/a"
emit "$ROOT" "$WORK/b"
na=$(ls "$WORK/a" | wc -l); nb=$(ls "$WORK/b" | wc -l)
if diff -r "$WORK/a" "$WORK/b" >"$WORK/diff.txt"; then
    echo "device assembly identical: $nb objects (base $BASE has $na)"
elif [ "$USAGE" = 1 ]; then
    usage_diff "$WORK/a" "$WORK/b"
else
    head -50 "$WORK/diff.txt"
    echo "device assembly DIFFERS against $BASE" >&2
    exit 1
fi
