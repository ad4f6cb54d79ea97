"""Build-time facts about the kernels of csrc/cwn_aggregate_act_bwd.hip, read from the built library's code object the way
tests/test_act_message_resources.py reads the forward's (no GPU): both element types, both addressing forms, and in each
of them every (vector width, activation) form -- they are dispatched inside the kernel -- without a spill or scratch."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from kernel_resources import kernels, READELF      # noqa: E402

LIB = os.path.join(ROOT, 'cwn_amd', 'libcwn_hip.so')

# (vgpr_count, sgpr_count) each kernel took as a text of its own, by <element type, 32-bit row offsets> as the mangled name
# spells them: the body shared with the other direction (csrc/cwn_aggregate_act_body.h) costs no register
PINNED = {'IfLb0': (95, 76), 'IfLb1': (95, 74), 'IdLb0': (110, 102), 'IdLb1': (96, 99)}


@pytest.fixture(scope='module')
def table():
    assert os.path.exists(LIB), 'the library has not been built'
    if not os.path.exists(READELF):
        pytest.skip('llvm-readelf missing')
    return kernels(LIB)


def test_act_message_bwd_kernels_neither_spill_nor_use_scratch(table):
    mine = {n: v for n, v in table.items() if 'aggregate_act_bwd_kernel' in n}
    # <float | double> x <64-bit | 32-bit row offsets>
    assert len(mine) == 4 and sum('IfLb' in n for n in mine) == 2 and sum('IdLb' in n for n in mine) == 2, sorted(mine)
    for name, v in mine.items():
        assert v['vgpr_spill_count'] == v['sgpr_spill_count'] == v['private_segment_fixed_size'] == 0, (name, v)
        assert v['max_flat_workgroup_size'] == 256, (name, v)
        # the long-row partials: 256 lanes x 16 bytes
        assert v['group_segment_fixed_size'] == 256 * 16, (name, v)
        assert v['vgpr_count'] <= 128, (name, v)        # four waves of a workgroup per SIMD at the least
        vgpr, sgpr = PINNED[re.search(r'kernel(I[fd]Lb[01])E', name).group(1)]
        assert v['vgpr_count'] <= vgpr and v['sgpr_count'] <= sgpr, (name, v)


def test_the_forward_kernels_are_still_their_own(table):
    """The backward is a translation unit of its own: the forward's four kernels are there under their names, untouched by it."""
    assert sum('aggregate_act_kernel' in n for n in table) == 4
