"""cwn_amd/csrc/cwn_group.h on the host: the block-start filler and the descriptor search agree with each other on
every pattern of empty and non-empty groups, the filler refuses a grid at INT32_MAX and not below, and the three
row-count readers return what their definitions say.  A stand-alone C++ program includes the header, prints, and the
expected values are worked out here.  No library call, no GPU."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX, INT64_MIN, INT64_MAX = 2**31 - 1, -2**63, 2**63 - 1
MAX = 8
CAPS = (0, 1, 33)

PROBE = r'''
#include <stdio.h>
#include <stdint.h>
#include <inttypes.h>
#include "cwn_group.h"

constexpr int MAX = 8;

// one line per pattern: the counts, what push said, the table, the total, the group of every block below the total
template <typename T> void patterns(const char* tag) {
    const int64_t vals[3] = {0, 1, 3};
    for (int n = 1; n <= 4; ++n) {
        int combos = 1;
        for (int i = 0; i < n; ++i) combos *= 3;
        for (int c = 0; c < combos; ++c) {
            T start[MAX + 1];
            for (int i = 0; i <= MAX; ++i) start[i] = (T)-7;
            cwn::BlockFill fill(start);
            printf("%s %d |", tag, n);
            int q = c;
            bool ok = true;
            for (int i = 0; i < n; ++i, q /= 3) {
                printf(" %" PRId64, vals[q % 3]);
                ok = fill.push(i, vals[q % 3]) && ok;
            }
            const int64_t total = fill.close(n);
            printf(" | %d | %" PRId64 " |", ok ? 1 : 0, total);
            for (int i = 0; i <= MAX; ++i) printf(" %" PRId64, (int64_t)start[i]);
            printf(" |");
            for (int64_t b = 0; b < total; ++b) printf(" %d", cwn::group_of<MAX>(start, n, (T)b));
            printf("\n");
        }
    }
}

int main(void) {
    patterns<int32_t>("P32");
    patterns<int64_t>("P64");
    {   // the grid bound: a total of INT32_MAX - 1 is accepted, INT32_MAX is not -- in one push, and reached by a second
        int32_t s[MAX + 1];
        cwn::BlockFill a(s);
        printf("O below %d\n", a.push(0, (int64_t)INT32_MAX - 1) ? 1 : 0);
        const bool reach = a.push(1, 1);
        printf("O reach %d %" PRId64 "\n", reach ? 1 : 0, a.close(2));
        cwn::BlockFill b(s);
        printf("O at %d\n", b.push(0, (int64_t)INT32_MAX) ? 1 : 0);
        cwn::BlockFill c(s);
        printf("O split %d", c.push(0, 1 << 30) ? 1 : 0);
        printf(" %d", c.push(1, (1 << 30) - 2) ? 1 : 0);
        printf(" %d\n", c.push(2, 1) ? 1 : 0);
    }
    const int64_t caps[3] = {0, 1, 33};
    for (int64_t cap : caps) {
        const int64_t counts[8] = {INT64_MIN, -1, 0, 1, cap - 1, cap, cap + 1, INT64_MAX};
        for (int64_t m : counts)
            printf("R %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", cap, m, cwn::rows_vouched(&m, cap),
                   cwn::rows_capped(&m, cap), cwn::rows_clamped(&m, cap));
        printf("N %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", cap, cwn::rows_vouched(nullptr, cap),
               cwn::rows_capped(nullptr, cap), cwn::rows_clamped(nullptr, cap));
    }
    return 0;
}
'''


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp('group_host')
    src, exe = d / 'probe.cpp', d / 'probe'
    src.write_text(PROBE)
    subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'cwn_amd', 'csrc'), str(src), '-o', str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    return [l.split() for l in out]


def test_filler_and_search_agree_on_every_pattern_of_empty_groups(probe):
    for tag in ('P32', 'P64'):
        seen = set()
        for l in (l for l in probe if l[0] == tag):
            n = int(l[1])
            parts = ' '.join(l[2:]).split('|')[1:]
            counts, (ok, ), (total, ), start, groups = ([int(x) for x in p.split()] for p in parts)
            seen.add(tuple(counts))
            assert len(counts) == n and ok == 1 and total == sum(counts), l
            assert start[:n] == [sum(counts[:i]) for i in range(n)], l
            assert start[n:] == [total] * (MAX + 1 - n), l        # start[n .. MAX]: the total
            # block b belongs to the group whose range [start, start + count) holds it: never an empty one
            want = [i for i, c in enumerate(counts) for _ in range(c)]
            assert groups == want, l
            assert all(counts[g] > 0 for g in groups), l
        assert seen == {c for n in range(1, 5) for c in itertools.product((0, 1, 3), repeat=n)}, tag


def test_filler_refuses_a_grid_at_int32_max_and_not_below(probe):
    got = {l[1]: [int(x) for x in l[2:]] for l in probe if l[0] == 'O'}
    assert got['below'] == [1]                            # INT32_MAX - 1 workgroups: accepted
    assert got['reach'] == [0, INT32_MAX]                 # one more: refused (today's blocks >= INT32_MAX)
    assert got['at'] == [0]
    assert got['split'] == [1, 1, 0]                      # 2^30, then 2^31 - 2, then INT32_MAX


def test_row_count_readers_are_their_definitions(probe):
    rows = {(int(l[1]), int(l[2])): tuple(int(x) for x in l[3:]) for l in probe if l[0] == 'R'}
    want = {(cap, m) for cap in CAPS for m in (INT64_MIN, -1, 0, 1, cap - 1, cap, cap + 1, INT64_MAX)}
    assert set(rows) == want
    for (cap, m), (vouched, capped, clamped) in rows.items():
        assert vouched == m, (cap, m)
        assert capped == min(m, cap), (cap, m)
        assert clamped == max(0, min(m, cap)), (cap, m)
    null = {int(l[1]): tuple(int(x) for x in l[2:]) for l in probe if l[0] == 'N'}
    assert null == {cap: (cap, cap, cap) for cap in CAPS}     # no device count: the capacity
