"""The median duration of each of the three rank kernels per problem size, from a rocprofv3 kernel trace:

    rocprofv3 --kernel-trace --stats -d DIR -o rank -- python tools/bench_eval.py --rank 4113 32901
    python tools/rank_trace_summary.py DIR/rank_results.db 4113 32901          (or a *_kernel_trace.csv)

bench_eval.py --rank runs the sizes one after the other with the same number of calls each, so the launches of a kernel in
time order fall into as many equal runs as there are sizes."""
import csv
import sqlite3
import statistics
import sys

KERNELS = ('rank_compact_kernel', 'rank_count_kernel', 'rank_finish_kernel')


def launches(path):
    """(kernel name, start ns, end ns) of every dispatch."""
    if path.endswith('.db'):
        return sqlite3.connect(path).execute('select name, start, end from kernels').fetchall()
    with open(path) as f:
        return [(r['Kernel_Name'], int(r['Start_Timestamp']), int(r['End_Timestamp'])) for r in csv.DictReader(f)]


def main(path, sizes):
    per = {k: [] for k in KERNELS}
    for name, start, end in launches(path):
        for k in KERNELS:
            if k in name:
                per[k].append((start, (end - start) / 1e3))
    for name, rows in per.items():
        rows.sort()
        m = len(rows) // len(sizes)
        for i, n in enumerate(sizes):
            us = [d for _, d in rows[i * m:(i + 1) * m]]
            if us:
                print(f'{name} n = {n}: {len(us)} launches, median {statistics.median(us):.1f} us, min {min(us):.1f}, max {max(us):.1f}')


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2:] or ['4113', '32901'])
