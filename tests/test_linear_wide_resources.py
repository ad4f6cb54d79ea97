"""Build-time facts about the kernels of csrc/cwn_linear_wide.hip, read from the built library's code object the way
tests/test_linear_stats_resources.py reads its kernel (no GPU): both weight layouts exist once, under a name of their own,
without a spill or scratch, in workgroups of 256, with the static LDS the file's header comment and the C header state."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from kernel_resources import kernels, short, READELF      # noqa: E402

LIB = os.path.join(ROOT, 'cwn_amd', 'libcwn_hip.so')
SRC = os.path.join(ROOT, 'cwn_amd', 'csrc', 'cwn_linear_wide.hip')
HEADER = os.path.join(ROOT, 'include', 'cwn_hip.h')


@pytest.fixture(scope='module')
def table():
    assert os.path.exists(LIB), 'the library has not been built'
    if not os.path.exists(READELF):
        pytest.skip('llvm-readelf missing')
    return kernels(LIB)


def _stated_lds():
    """(natural, transposed) bytes the header comment of the source file states, checked against the layouts it names."""
    m = re.search(r'// LDS \(static\): natural W \((\d+) \+ (\d+)\) x (\d+) floats = (\d+) B; transposed W (\d+) x (\d+) \+ (\d+) x (\d+) '
                  r'floats = (\d+) B', open(SRC).read())
    assert m, 'the header comment of cwn_linear_wide.hip states no LDS figures'
    wn, xr, kc, nat, kc2, rs, xr2, kc3, tr = (int(g) for g in m.groups())
    assert (wn + xr) * kc * 4 == nat and (kc2 * rs + xr2 * kc3) * 4 == tr
    return nat, tr


def test_header_comment_states_the_lds_of_its_layouts():
    src = open(SRC).read()
    const = lambda name: int(re.search(rf'constexpr int {name} = (\d+);', src).group(1))
    bn, bm, kc = const('kBN'), const('kBM'), const('kKC')
    assert (bn, bm, kc) == (128, 32, 64)
    nat, tr = _stated_lds()
    assert nat == (bn + bm) * kc * 4 and tr == (kc * (bn + 4) + bm * kc) * 4
    budget = int(re.search(r'#define CWN_LINEAR_WIDE_LDS_BYTES (\d+)', open(HEADER).read()).group(1))
    assert max(nat, tr) == budget <= 64 * 1024


def test_both_kernels_exist_once_and_neither_spills_nor_uses_scratch(table):
    mine = {n: v for n, v in table.items() if 'linear_wide_f32_kernel' in n}
    assert len(mine) == 2, sorted(mine)
    nat, tr = _stated_lds()
    lds = set()
    for name, v in mine.items():
        assert 'gemm_kernel' not in name and not short(name).startswith('gemm_kernel<'), name
        assert v['vgpr_spill_count'] == v['sgpr_spill_count'] == v['private_segment_fixed_size'] == 0, (name, v)
        assert v['max_flat_workgroup_size'] == 256, (name, v)
        lds.add(v['group_segment_fixed_size'])
    assert lds == {nat, tr}, (lds, nat, tr)
