"""Build-time facts about the kernel of csrc/cwn_gine.hip, read from the built library's code object the way
tests/test_gin_resources.py reads its kernel (no GPU): the kernel exists once, without a spill or scratch, in workgroups
of 256, within 128 VGPRs, with the static LDS the file's header comment states -- and the GIN kernel it shares
csrc/cwn_gin_tile.h with is still the one kernel with the LDS it had."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from kernel_resources import kernels, READELF      # noqa: E402

LIB = os.path.join(ROOT, 'cwn_amd', 'libcwn_hip.so')
CSRC = os.path.join(ROOT, 'cwn_amd', 'csrc')
HEADER = os.path.join(ROOT, 'include', 'cwn_hip.h')


@pytest.fixture(scope='module')
def table():
    assert os.path.exists(LIB), 'the library has not been built'
    if not os.path.exists(READELF):
        pytest.skip('llvm-readelf missing')
    return kernels(LIB)


def _stated_lds() -> int:
    """The float32 bytes the header comment of the source file states, checked against the layout it names."""
    m = re.search(r'// LDS \(static\): gine_layer \((\d+) x (\d+) x (\d+)\) elements = (\d+) B in float32',
                  open(os.path.join(CSRC, 'cwn_gine.hip')).read())
    assert m, 'the header comment of cwn_gine.hip states no LDS figure'
    panels, rows, pitch, nbytes = (int(g) for g in m.groups())
    assert panels * rows * pitch * 4 == nbytes
    return nbytes


def test_header_comment_states_the_lds_of_its_layout():
    """Two panels (s and h) of CWN_GIN_TM rows at a pitch of CWN_GIN_MAX_WIDTH + 4 floats: the GIN kernel's geometry."""
    header = open(HEADER).read()
    tm = int(re.search(r'#define CWN_GIN_TM (\d+)', header).group(1))
    width = int(re.search(r'#define CWN_GIN_MAX_WIDTH (\d+)', header).group(1))
    assert _stated_lds() == 2 * tm * (width + 4) * 4


def test_the_shared_code_is_written_once():
    """product, epilogue, the panel constants and the checks live in cwn_gin_tile.h; both kernels include it and define none."""
    tile = open(os.path.join(CSRC, 'cwn_gin_tile.h')).read()
    for name in ('void product(', 'float epilogue(', 'constexpr int kLdp', 'bool gin_overlaps(', 'int gin_check('):
        assert name in tile, name
        for f in ('cwn_gin.hip', 'cwn_gine.hip'):
            src = open(os.path.join(CSRC, f)).read()
            assert name not in src and '#include "cwn_gin_tile.h"' in src, (f, name)
    assert '// LDS (static): gin_layer (' in open(os.path.join(CSRC, 'cwn_gin.hip')).read()


def test_gine_kernel_exists_once_and_neither_spills_nor_uses_scratch(table):
    mine = {n: v for n, v in table.items() if 'gine_layer_kernel' in n}
    assert len(mine) == 1, sorted(mine)
    (name, v), = mine.items()
    assert v['vgpr_spill_count'] == v['sgpr_spill_count'] == v['private_segment_fixed_size'] == 0, (name, v)
    assert v['max_flat_workgroup_size'] == 256, (name, v)
    assert v['group_segment_fixed_size'] == _stated_lds() <= 64 * 1024, (name, v)
    assert v['vgpr_count'] <= 128, (name, v)            # four waves of a workgroup per SIMD at the least


def test_gin_kernel_is_still_one_kernel_with_its_lds(table):
    gin = {n: v for n, v in table.items() if 'gin_layer_kernel' in n}
    assert len(gin) == 1, sorted(gin)
    (name, v), = gin.items()
    assert v['group_segment_fixed_size'] == 33792 and v['max_flat_workgroup_size'] == 256, (name, v)
    assert v['vgpr_spill_count'] == v['sgpr_spill_count'] == v['private_segment_fixed_size'] == 0, (name, v)
