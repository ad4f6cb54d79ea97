"""Build-time facts about the kernel of csrc/cwn_chain_f32.hip, read from the built library's code object the way
tests/test_gin_resources.py reads its kernel (no GPU): the kernel exists once, under a name of its own, without a spill or
scratch, in workgroups of 256, with the static LDS the file's header comment states."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from kernel_resources import kernels, short, READELF      # noqa: E402

LIB = os.path.join(ROOT, 'cwn_amd', 'libcwn_hip.so')
SRC = os.path.join(ROOT, 'cwn_amd', 'csrc', 'cwn_chain_f32.hip')
HEADER = os.path.join(ROOT, 'include', 'cwn_hip.h')


@pytest.fixture(scope='module')
def table():
    assert os.path.exists(LIB), 'the library has not been built'
    if not os.path.exists(READELF):
        pytest.skip('llvm-readelf missing')
    return kernels(LIB)


def _stated_lds() -> int:
    """The float32 bytes the header comment of the source file states, checked against the layout it names."""
    m = re.search(r'// LDS \(static\): update_chain_f32 \((\d+) x (\d+) x (\d+)\) elements = (\d+) B in float32', open(SRC).read())
    assert m, 'the header comment of cwn_chain_f32.hip states no LDS figure'
    panels, rows, pitch, nbytes = (int(g) for g in m.groups())
    assert panels * rows * pitch * 4 == nbytes
    return nbytes


def test_header_comment_states_the_lds_of_its_layout():
    """Three panels (up, boundary, hidden) of CWN_CHAIN_F32_TM rows at a pitch of CWN_CHAIN_F32_MAX_WIDTH + 4 floats."""
    header = open(HEADER).read()
    tm = int(re.search(r'#define CWN_CHAIN_F32_TM (\d+)', header).group(1))
    width = int(re.search(r'#define CWN_CHAIN_F32_MAX_WIDTH (\d+)', header).group(1))
    assert _stated_lds() == 3 * tm * (width + 4) * 4


def test_chain_kernel_exists_once_and_neither_spills_nor_uses_scratch(table):
    mine = {n: v for n, v in table.items() if 'update_chain_f32_kernel' in n}
    assert len(mine) == 1, sorted(mine)
    (name, v), = mine.items()
    assert not short(name).startswith(('layer_kernel<', 'update_mlp_kernel<')), name      # (tests/test_kernel_resources.py counts those)
    assert v['vgpr_spill_count'] == v['sgpr_spill_count'] == v['private_segment_fixed_size'] == 0, (name, v)
    assert v['max_flat_workgroup_size'] == 256, (name, v)
    assert v['group_segment_fixed_size'] == _stated_lds() <= 64 * 1024, (name, v)
    assert v['vgpr_count'] <= 128, (name, v)            # four waves of a workgroup per SIMD at the least
