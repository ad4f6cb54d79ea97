"""Build-time facts about the kernels of csrc/cwn_agnostic.hip, read from the built library's code object the way
tests/test_act_message_resources.py reads its kernels (no GPU): both kernels in both element types, without a spill or
scratch, workgroups of 256, and the LDS the file's header comment states."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from kernel_resources import kernels, READELF      # noqa: E402

LIB = os.path.join(ROOT, 'cwn_amd', 'libcwn_hip.so')
SRC = os.path.join(ROOT, 'cwn_amd', 'csrc', 'cwn_agnostic.hip')


@pytest.fixture(scope='module')
def table():
    assert os.path.exists(LIB), 'the library has not been built'
    if not os.path.exists(READELF):
        pytest.skip('llvm-readelf missing')
    return kernels(LIB)


def _stated_lds():
    """{kernel: (float32 bytes, float64 bytes)} from the header comment of the source file."""
    text = open(SRC).read()
    out = {}
    for kernel, word in (('embed_pool_kernel', 'embed_pool'), ('agnostic_head_kernel', 'head')):
        m = re.search(rf'// (?:LDS \(static\):)?\s*{word} \([^)]*\) elements = (\d+) B in float32, (\d+) B in float64', text)
        assert m, word
        out[kernel] = (int(m.group(1)), int(m.group(2)))
    return out


def test_header_comment_states_the_lds_of_its_layout():
    """The stated figures are those of the layout the comment describes: a 64 x 129 block of W and 256 partials; a 256 x 33
    tile, 8 x 32 elements of P and 1024 sums."""
    assert _stated_lds() == {'embed_pool_kernel': ((64 * 129 + 256) * 4, (64 * 129 + 256) * 8),
                             'agnostic_head_kernel': ((256 * 33 + 8 * 32 + 1024) * 4, (256 * 33 + 8 * 32 + 1024) * 8)}


@pytest.mark.parametrize('kernel', ['embed_pool_kernel', 'agnostic_head_kernel'])
def test_agnostic_kernels_neither_spill_nor_use_scratch(table, kernel):
    mine = {n: v for n, v in table.items() if kernel in n}
    f32 = [n for n in mine if f'{kernel}IfE' in n]
    f64 = [n for n in mine if f'{kernel}IdE' in n]
    assert len(mine) == 2 and len(f32) == 1 and len(f64) == 1, sorted(mine)
    lds = _stated_lds()[kernel]
    for name, v in mine.items():
        assert v['vgpr_spill_count'] == v['sgpr_spill_count'] == v['private_segment_fixed_size'] == 0, (name, v)
        assert v['max_flat_workgroup_size'] == 256, (name, v)
        assert v['group_segment_fixed_size'] == lds[0 if name in f32 else 1], (name, v)
        assert v['vgpr_count'] <= 128, (name, v)        # four waves of a workgroup per SIMD at the least
