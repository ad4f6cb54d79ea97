#!/bin/bash
# isa_diff.sh <file.hip> [rev] -- is the device code of a source file what it was at <rev> (default HEAD)?
# Compiles the file from the work tree and from `git show <rev>` (with that revision's csrc/ and include/ beside
# it, in a temporary directory), each with its own Makefile's CXXFLAGS plus --cuda-device-only -S, and diffs the
# assembly: instructions, kernel names and the metadata blocks (registers, scratch, LDS).  Dropped before the
# diff: .file / .loc / .ident, comment-only lines and the per-file __hip_cuid_<hash> symbol.  Prints the diff and
# exits 1 if anything is left: the check behind "object unchanged".  Needs git and hipcc, no GPU.
# Files the Makefile builds with more than CXXFLAGS (PRELOAD, -DCWN_LAYER_W8) take them in ISA_DIFF_FLAGS.
set -euo pipefail
[ $# -ge 1 ] || { echo "usage: $0 <file.hip> [rev]" >&2; exit 2; }
ROOT=$(git -C "$(dirname "$0")" rev-parse --show-toplevel)
SRC=$(realpath --relative-to="$ROOT" "$1")
REV=${2:-HEAD}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT

mkdir "$TMP/rev"
git -C "$ROOT" archive "$REV" cwn_amd/csrc include | tar -x -C "$TMP/rev"

# device assembly of <tree>/$SRC, cleaned, on stdout
isa() {
    local flags
    flags=$(make -s -C "$1/cwn_amd/csrc" --eval 'isa-diff-flags: ; @echo $(CXXFLAGS)' isa-diff-flags)
    # shellcheck disable=SC2086
    (cd "$1" && "$HIPCC" $flags ${ISA_DIFF_FLAGS:-} --cuda-device-only -S "$SRC" -o "$2")
    grep -v -E '^[[:space:]]*(;|\.file[[:space:]]|\.loc[[:space:]]|\.ident[[:space:]])|__hip_cuid_' "$2"
}

isa "$ROOT" "$TMP/work.s" > "$TMP/work.clean"
isa "$TMP/rev" "$TMP/rev.s" > "$TMP/rev.clean"
if diff "$TMP/rev.clean" "$TMP/work.clean"; then
    echo "$SRC: device assembly identical to $REV ($(grep -c '^[[:space:]]*\.amdhsa_kernel ' "$TMP/work.clean") kernels, $(wc -l < "$TMP/work.clean") lines)"
else
    echo "$SRC: device assembly differs from $REV" >&2
    exit 1
fi
