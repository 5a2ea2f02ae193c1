#!/bin/bash
# Device assembly of the working tree against a git revision, file by file; needs hipcc, no GPU:  bash tools/asm_diff.sh [REV] [OUTDIR]
# Every csrc/*.hip of REV (default HEAD) and of the working tree is compiled with build.py's flags plus --cuda-device-only -S and the two
# .s files are compared whole (cmp: nothing filtered); of the compiler's diagnostics, the warning and error messages without their line numbers.  Both sides are compiled at the SAME staging
# path, input and output: clang derives the __hip_cuid_<hash> symbol from its command line.  Prints one row per file; exit status 1 if
# any file differs.  The assembly stays in OUTDIR/{base,new} (default: a new temporary directory, printed).
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
REV=${1:-HEAD}
OUT=${2:-$(mktemp -d)}
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS=$(python -c "import context_attentive_ir_amd.build as b; print(' '.join(b.FLAGS))") || exit 1
P=context_attentive_ir_amd/csrc
S=$OUT/stage
mkdir -p "$OUT" && echo "assembly in $OUT"
compile_side() {        # $1 = base | new; the sources are staged under $S already
    mkdir -p "$OUT/$1" "$S/out"
    (cd "$S/$P" && ls *.hip | xargs -P "${JOBS:-8}" -I{} sh -c \
        "b=\$(basename {} .hip); $HIPCC $FLAGS --cuda-device-only -S {} -o $S/out/\$b.s 2> $S/out/\$b.log; mv $S/out/\$b.s $S/out/\$b.log $OUT/$1/")
}
rm -rf "$S" && mkdir -p "$S" && git archive "$REV" $P include | tar -x -C "$S" && compile_side base || exit 1
rm -rf "$S" && mkdir -p "$S/$P" && cp $P/*.hip $P/*.hpp "$S/$P/" && cp -r include "$S/include" && compile_side new || exit 1
rm -rf "$S"
msgs() { grep -E 'warning:|error:' "$1" | sed -E 's/^[^ ]+:[0-9]+:[0-9]+: //'; }
rc=0
printf '| %-18s | %-9s | %-11s |\n' file assembly diagnostics
for f in $(cd "$OUT" && ls base/*.s new/*.s | xargs -n1 basename | sort -u); do
    a=identical; w=identical
    cmp -s "$OUT/base/$f" "$OUT/new/$f" || { a="DIFFERS"; rc=1; }
    [ "$(msgs "$OUT/base/${f%.s}.log")" = "$(msgs "$OUT/new/${f%.s}.log")" ] || { w="DIFFER"; rc=1; }
    printf '| %-18s | %-9s | %-11s |\n' "${f%.s}.hip" "$a" "$w"
done
exit $rc
