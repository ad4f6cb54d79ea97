#!/bin/bash
# Kernels per optimisation step of the forms tools/bench_static_width.py times, counted exactly: every form runs twice under
# rocprofv3 --kernel-trace --stats, 2 and 6 epochs long, and the difference of the two dispatch counts over the difference of the
# step counts is the step's own (warm-up, capture and the one-off launches cancel).
#   bash tools/bench_static_width_kernels.sh [tree]      ->  stdout and $OUT_DIR/static_width_kernels[_tree].txt (OUT_DIR: /tmp)
# `tree`: the root of another checkout of this project with a built library (the hidden-128 step of the parent commit).
export TMPDIR=/tmp
R=$PWD
T=$(cd "${1:-$R}" && pwd)
OUT_DIR=${OUT_DIR:-/tmp}
OUT=$OUT_DIR/static_width_kernels${1:+_$(basename $1)}.txt
mkdir -p $OUT_DIR
: > $OUT
count() {   # form hidden epochs -> "dispatches" on stdout, per-kernel counts in /tmp/bswk_$3.txt
  rm -rf /tmp/bswk
  ( cd /tmp && timeout -k 10 280 rocprofv3 --kernel-trace --stats -d /tmp/bswk -- python $T/tools/bench_static_width.py --count $1 --hidden $2 --epochs $3 > /tmp/bswk.log 2>&1 ) || { tail -20 /tmp/bswk.log >&2; return 1; }
  python - "$(ls /tmp/bswk/*/*results.db | head -1)" $3 <<'PY'
import sqlite3, sys
rows = sqlite3.connect(sys.argv[1]).cursor().execute('select name, count(*) from kernels group by name').fetchall()
with open(f'/tmp/bswk_{sys.argv[2]}.txt', 'w') as f:
    for k, c in sorted(rows):
        f.write(f'{c}\t{k}\n')
print(sum(c for _, c in rows))
PY
}
FORMS=${FORMS:-"static:48 static:16 per_batch:48 static:128"}
for fh in $FORMS; do
  f=${fh%%:*}; h=${fh##*:}
  a=$(count $f $h 2) || exit 1
  b=$(count $f $h 6) || exit 1
  python - $f $h $a $b >> $OUT <<'PY'
import sys
f, h, a, b = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
steps = 4 * 16
print(f'{f} hidden {h}: {(b - a) / steps:.2f} kernels per step ({a} dispatches in 2 epochs, {b} in 6, 16 steps per epoch)')
ka = {l.split("\t")[1].strip(): int(l.split("\t")[0]) for l in open('/tmp/bswk_2.txt')}
kb = {l.split("\t")[1].strip(): int(l.split("\t")[0]) for l in open('/tmp/bswk_6.txt')}
for k in sorted(kb):
    d = (kb[k] - ka.get(k, 0)) / steps
    if d:
        print(f'    {d:7.3f}  {k[:110]}')
PY
done
cat $OUT
