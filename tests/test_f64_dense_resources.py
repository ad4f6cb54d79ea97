"""Build-time facts about the two kernels of csrc/cwn_dense_f64.hip, read from the built library's code object the way
tests/test_kernel_resources.py reads the others (no GPU): neither spills, both keep their static LDS below the 64 KiB a
kernel may declare -- far inside the 160 KiB of a CU, the bound the five 64-wide matrices of a layer (192 KiB) would break
if they were staged together -- and several workgroups share a CU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from kernel_resources import kernels, READELF      # noqa: E402

LIB = os.path.join(ROOT, 'cwn_amd', 'libcwn_hip.so')
CU_LDS = 160 * 1024


@pytest.fixture(scope='module')
def table():
    assert os.path.exists(LIB), 'the library has not been built'
    if not os.path.exists(READELF):
        pytest.skip('llvm-readelf missing')
    return kernels(LIB)


@pytest.mark.parametrize('kernel,lds', [('update_chain_f64_kernel', (2 * 16 * 64 + 64 * 65) * 8),
                                        ('linear_many_f64_kernel', (16 * 128 + 32 * 129) * 8)])
def test_dense_f64_kernels_keep_registers_and_lds(table, kernel, lds):
    mine = {n: v for n, v in table.items() if kernel in n}
    assert len(mine) == 1, sorted(mine)
    (name, v), = mine.items()
    assert v['vgpr_spill_count'] == v['sgpr_spill_count'] == v['private_segment_fixed_size'] == 0, (name, v)
    assert v['max_flat_workgroup_size'] == 256, (name, v)
    assert v['group_segment_fixed_size'] == lds, (name, v)              # what the file's header says it stages
    assert v['group_segment_fixed_size'] <= CU_LDS // 3                 # three workgroups per CU
    assert v['vgpr_count'] <= 128, (name, v)                            # 4 waves per workgroup: no register limit on those three
