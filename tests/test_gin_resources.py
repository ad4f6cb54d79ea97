"""Build-time facts about the kernel of csrc/cwn_gin.hip, read from the built library's code object the way
tests/test_agnostic_resources.py reads its kernels (no GPU): the kernel exists once, without a spill or scratch, in
workgroups of 256, with the static LDS the file's header comment states."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from kernel_resources import kernels, READELF      # noqa: E402

LIB = os.path.join(ROOT, 'cwn_amd', 'libcwn_hip.so')
SRC = os.path.join(ROOT, 'cwn_amd', 'csrc', 'cwn_gin.hip')
HEADER = os.path.join(ROOT, 'include', 'cwn_hip.h')


@pytest.fixture(scope='module')
def table():
    assert os.path.exists(LIB), 'the library has not been built'
    if not os.path.exists(READELF):
        pytest.skip('llvm-readelf missing')
    return kernels(LIB)


def _stated_lds() -> int:
    """The float32 bytes the header comment of the source file states, checked against the layout it names."""
    m = re.search(r'// LDS \(static\): gin_layer \((\d+) x (\d+) x (\d+)\) elements = (\d+) B in float32', open(SRC).read())
    assert m, 'the header comment of cwn_gin.hip states no LDS figure'
    panels, rows, pitch, nbytes = (int(g) for g in m.groups())
    assert panels * rows * pitch * 4 == nbytes
    return nbytes


def test_header_comment_states_the_lds_of_its_layout():
    """Two panels (s and h) of CWN_GIN_TM rows at a pitch of CWN_GIN_MAX_WIDTH + 4 floats."""
    header = open(HEADER).read()
    tm = int(re.search(r'#define CWN_GIN_TM (\d+)', header).group(1))
    width = int(re.search(r'#define CWN_GIN_MAX_WIDTH (\d+)', header).group(1))
    assert _stated_lds() == 2 * tm * (width + 4) * 4


def test_gin_kernel_exists_once_and_neither_spills_nor_uses_scratch(table):
    mine = {n: v for n, v in table.items() if 'gin_layer_kernel' in n}
    assert len(mine) == 1, sorted(mine)
    (name, v), = mine.items()
    assert v['vgpr_spill_count'] == v['sgpr_spill_count'] == v['private_segment_fixed_size'] == 0, (name, v)
    assert v['max_flat_workgroup_size'] == 256, (name, v)
    assert v['group_segment_fixed_size'] == _stated_lds() <= 64 * 1024, (name, v)
    assert v['vgpr_count'] <= 128, (name, v)            # four waves of a workgroup per SIMD at the least
