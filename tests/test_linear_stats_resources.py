"""Build-time facts about the kernel of csrc/cwn_linear_stats.hip, read from the built library's code object the way
tests/test_chain_f32_resources.py reads its kernel (no GPU): the kernel exists once, under a name of its own, without a spill or
scratch, in workgroups of 256, with the static LDS the file's header comment states."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from kernel_resources import kernels, short, READELF      # noqa: E402

LIB = os.path.join(ROOT, 'cwn_amd', 'libcwn_hip.so')
SRC = os.path.join(ROOT, 'cwn_amd', 'csrc', 'cwn_linear_stats.hip')


@pytest.fixture(scope='module')
def table():
    assert os.path.exists(LIB), 'the library has not been built'
    if not os.path.exists(READELF):
        pytest.skip('llvm-readelf missing')
    return kernels(LIB)


def _stated_lds() -> int:
    """The bytes the header comment of the source file states, checked against the layout it names."""
    m = re.search(r'// LDS \(static\): linear_stats_f32 \((\d+) \+ (\d+)\) rows x (\d+) floats = (\d+) B\.', open(SRC).read())
    assert m, 'the header comment of cwn_linear_stats.hip states no LDS figure'
    w_rows, x_rows, k, nbytes = (int(g) for g in m.groups())
    assert (w_rows + x_rows) * k * 4 == nbytes
    return nbytes


def test_header_comment_states_the_lds_of_its_layout():
    """A chunk of W (every column of the widest product: 128 rows) and one of X (one 32-row statistics band), 64 floats of K each."""
    src = open(SRC).read()
    bn = int(re.search(r'constexpr int kBN = (\d+);', src).group(1))
    bm = int(re.search(r'constexpr int kBM = (\d+);', src).group(1))
    kc = int(re.search(r'constexpr int kKC = (\d+);', src).group(1))
    assert (bn, bm) == (128, 32)
    assert _stated_lds() == (bn + bm) * kc * 4


def test_kernel_exists_once_under_its_own_name_and_neither_spills_nor_uses_scratch(table):
    mine = {n: v for n, v in table.items() if 'linear_stats_f32_kernel' in n}
    assert len(mine) == 1, sorted(mine)
    (name, v), = mine.items()
    assert 'gemm_kernel' not in name and not short(name).startswith('gemm_kernel<'), name     # (tests/test_kernel_resources.py lists those)
    assert v['vgpr_spill_count'] == v['sgpr_spill_count'] == v['private_segment_fixed_size'] == 0, (name, v)
    assert v['max_flat_workgroup_size'] == 256, (name, v)
    assert v['group_segment_fixed_size'] == _stated_lds() <= 64 * 1024, (name, v)
