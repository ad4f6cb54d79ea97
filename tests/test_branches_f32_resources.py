"""Build-time facts about the kernel of csrc/cwn_branches_f32.hip, read from the built library's code object the way
tests/test_chain_f32_resources.py reads its kernel (no GPU): the kernel exists once, under a name of its own, without a spill
or scratch, in workgroups of 256, with the static LDS the file's header comment states -- two panels, whatever the number of
branches -- and the kernel of the two-branch chain is still the one it was."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from kernel_resources import kernels, short, READELF      # noqa: E402

LIB = os.path.join(ROOT, 'cwn_amd', 'libcwn_hip.so')
SRC = os.path.join(ROOT, 'cwn_amd', 'csrc', 'cwn_branches_f32.hip')
HEADER = os.path.join(ROOT, 'include', 'cwn_hip.h')


@pytest.fixture(scope='module')
def table():
    assert os.path.exists(LIB), 'the library has not been built'
    if not os.path.exists(READELF):
        pytest.skip('llvm-readelf missing')
    return kernels(LIB)


def _stated_lds() -> int:
    """The float32 bytes the header comment of the source file states, checked against the layout it names."""
    m = re.search(r'// LDS \(static\): update_branches_f32 \((\d+) x (\d+) x (\d+)\) elements = (\d+) B in float32', open(SRC).read())
    assert m, 'the header comment of cwn_branches_f32.hip states no LDS figure'
    panels, rows, pitch, nbytes = (int(g) for g in m.groups())
    assert panels * rows * pitch * 4 == nbytes
    return nbytes


def test_header_comment_states_the_lds_of_its_layout():
    """Two panels (the branch at work and its hidden activation) of CWN_BRANCHES_F32_TM rows at a pitch of
    CWN_BRANCHES_F32_MAX_WIDTH + 4 floats: LDS does not grow with the number of branches."""
    header = open(HEADER).read()
    tm = int(re.search(r'#define CWN_BRANCHES_F32_TM (\d+)', header).group(1))
    width = int(re.search(r'#define CWN_BRANCHES_F32_MAX_WIDTH (\d+)', header).group(1))
    assert _stated_lds() == 2 * tm * (width + 4) * 4 == 33792


def test_the_tile_code_is_shared_with_the_chain():
    """Both files include csrc/cwn_chain_tile.h and neither defines the product of its own."""
    for name in ('cwn_branches_f32.hip', 'cwn_chain_f32.hip'):
        text = open(os.path.join(ROOT, 'cwn_amd', 'csrc', name)).read()
        assert '#include "cwn_chain_tile.h"' in text and 'void product(' not in text, name
    assert 'cwn_chain_tile.h' in open(os.path.join(ROOT, 'cwn_amd', 'csrc', 'Makefile')).read()       # a header every object follows


def test_branches_kernel_exists_once_and_neither_spills_nor_uses_scratch(table):
    mine = {n: v for n, v in table.items() if 'update_branches_f32_kernel' in n}
    assert len(mine) == 1, sorted(mine)
    (name, v), = mine.items()
    assert not short(name).startswith(('layer_kernel<', 'update_mlp_kernel<')), name      # (tests/test_kernel_resources.py counts those)
    assert v['vgpr_spill_count'] == v['sgpr_spill_count'] == v['private_segment_fixed_size'] == 0, (name, v)
    assert v['max_flat_workgroup_size'] == 256, (name, v)
    assert v['group_segment_fixed_size'] == _stated_lds() <= 64 * 1024, (name, v)
    assert v['vgpr_count'] <= 128, (name, v)            # four waves of a workgroup per SIMD at the least


def test_the_chain_kernel_is_still_there_once(table):
    """tests/test_chain_f32_resources.py counts matches of this substring: the new kernel's name does not contain it."""
    assert len([n for n in table if 'update_chain_f32_kernel' in n]) == 1
    assert not any('update_chain_f32_kernel' in n for n in table if 'update_branches_f32_kernel' in n)
