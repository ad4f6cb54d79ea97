"""packed.PackedCochains without a GPU: the segment tables of a batch of cochains (`cochain_tables`: numpy in, numpy out)
against CochainBatch.from_cochain_list, what the packing refuses, the loader's index lists, and the bookkeeping of the
edge-flow readout head in the library (header, exports, ABI, the model switch's default)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from cwn_amd import _ffi, packed
from cwn_amd.complex import Cochain, CochainBatch
from cwn_amd.synthetic import edge_flows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flows():
    """Six small flow cochains; number 2 has no upper adjacency, number 4 has no cells."""
    cs = edge_flows(6, side=6, seed=5)
    c = cs[2]
    cs[2] = Cochain(dim=1, x=c.x, lower_index=c.lower_index, lower_orient=c.lower_orient, y=c.y)
    z = torch.zeros(2, 0, dtype=torch.long)
    cs[4] = Cochain(dim=1, x=torch.zeros(0, 1), upper_index=z, lower_index=z.clone(), upper_orient=torch.zeros(0),
                    lower_orient=torch.zeros(0), y=torch.tensor([1]))
    return cs


@pytest.mark.parametrize('idx', [[0, 1, 2, 3, 4, 5], [5, 3, 0, 1, 4, 2], [3], [1, 1, 5, 1], [2], [4], [2, 4, 2], [4, 0]])
def test_tables_agree_with_the_host_collate(idx):
    cs = _flows()
    meta = packed.cochain_meta(cs)
    t = packed.cochain_tables(meta, idx)
    ref = CochainBatch.from_cochain_list([cs[i] for i in idx])
    assert t['slices'] == ref.__slices__
    assert t['ptr'].tolist() == ref.ptr
    assert t['num_cells_list'] == ref.__num_cells_list__
    assert t['num_cells'] == ref.num_cells and t['num_cells_up'] == ref.__num_cells_up__ and t['num_cells_down'] == ref.__num_cells_down__
    # the running cell offset: what the host collate added to every cochain's index values
    for key in ('upper_index', 'lower_index'):
        for s, i in enumerate(idx):
            if cs[i][key] is None or cs[i][key].size(1) == 0:
                continue
            lo, hi = t['slices'][key][s], t['slices'][key][s + 1]
            assert torch.equal(getattr(ref, key)[:, lo:hi] - int(t['cell_off'][s]), cs[i][key])
    assert t['seg'].tolist() == [0] + np.cumsum([cs[i].num_cells for i in idx]).tolist()
    assert torch.equal(ref.batch, torch.repeat_interleave(torch.arange(len(idx)), torch.tensor(np.diff(t['seg']))))
    assert t['present']['upper_index'] == any(cs[i].upper_index is not None for i in idx)


def test_a_cochain_without_cells_keeps_no_segment():
    cs = edge_flows(2, side=6, seed=1) + [Cochain(dim=1, y=torch.tensor([0]))]
    t = packed.cochain_tables(packed.cochain_meta(cs), [0, 2, 1])
    ref = CochainBatch.from_cochain_list([cs[i] for i in (0, 2, 1)])
    assert t['ptr'].tolist() == ref.ptr and len(ref.ptr) == 3
    assert t['num_cells_list'] == ref.__num_cells_list__ == [cs[0].num_cells, None, cs[1].num_cells]
    assert t['seg'].tolist() == [0, cs[0].num_cells, cs[0].num_cells, 2 * cs[0].num_cells]


@pytest.mark.parametrize('key,value', [('shared_boundaries', torch.zeros(4, dtype=torch.long)),
                                       ('shared_coboundaries', torch.zeros(4, dtype=torch.long)),
                                       ('boundary_index', torch.zeros(2, 4, dtype=torch.long)),
                                       ('mask', torch.zeros(83, dtype=torch.bool))])
def test_refused_keys_are_named(key, value):
    cs = edge_flows(3, side=6, seed=2)
    setattr(cs[1], key, value)
    with pytest.raises(ValueError, match=f'cochain 1 carries {key}'):
        packed.PackedCochains(cs, 'cpu', with_csr=False)


def test_other_refusals():
    cs = edge_flows(3, side=6, seed=2)
    cs[2].upper_orient = cs[2].upper_orient[:-1]
    with pytest.raises(ValueError, match='cochain 2: upper_orient has .* entries, upper_index has .* columns'):
        packed.cochain_meta(cs)
    cs = edge_flows(3, side=6, seed=2)
    cs[0].lower_index = None
    with pytest.raises(ValueError, match='cochain 0: lower_orient has .* entries, lower_index has 0 columns'):
        packed.cochain_meta(cs)
    cs = edge_flows(2, side=6, seed=2) + [Cochain(dim=0, x=torch.zeros(3, 1))]
    with pytest.raises(ValueError, match='cochain 2 has dim 0, cochain 0 has dim 1'):
        packed.cochain_meta(cs)
    cs = edge_flows(2, side=6, seed=2)
    cs[1].x = cs[1].x.double()
    with pytest.raises(TypeError, match='torch.float64'):
        packed.cochain_meta(cs)
    cs = edge_flows(2, side=6, seed=2)
    cs[1].x = torch.cat([cs[1].x, cs[1].x], 1)
    with pytest.raises(ValueError, match='cochain 1: x is'):
        packed.cochain_meta(cs)
    meta = packed.cochain_meta(edge_flows(2, side=6, seed=2))
    with pytest.raises(IndexError):
        packed.cochain_tables(meta, [0, 2])
    with pytest.raises(ValueError):
        packed.cochain_tables(meta, [])


def test_loader_index_lists():
    pc = packed.PackedCochains(edge_flows(7, side=6, seed=3), 'cpu', with_csr=False)
    plain = pc.batch_indices(3)
    assert [b.tolist() for b in plain] == [[0, 1, 2], [3, 4, 5], [6]]
    assert [b.tolist() for b in pc.batch_indices(3, drop_last=True)] == [[0, 1, 2], [3, 4, 5]]
    e0, e0b, e1 = (np.concatenate(pc.batch_indices(3, shuffle=True, seed=11, epoch=e)) for e in (0, 0, 1))
    assert sorted(e0.tolist()) == sorted(e1.tolist()) == list(range(7))
    assert e0.tolist() == e0b.tolist() and e0.tolist() != e1.tolist()


def test_library_declares_the_flow_head():
    header = open(os.path.join(ROOT, 'include', 'cwn_hip.h')).read()
    names = ('cwn_flow_head_f32', 'cwn_flow_head_bwd_f32', 'cwn_flow_head_workspace_floats')
    for name in names:
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert name in _ffi.EXPORTS
    section = header[header.index('The edge-flow readout head'):header.index('cwn_flow_head_bwd_f32(')]
    assert 'NO m_dev' in section and 'no static batch reaches' in section
    assert int(re.search(r'#define CWN_ABI_VERSION (\d+)', header).group(1)) == _ffi.ABI_VERSION == 24
    for macro, value in (('CWN_FLOW_HEAD_MAX_WIDTH', _ffi.FLOW_HEAD_MAX_WIDTH), ('CWN_FLOW_HEAD_MAX_OUT', _ffi.FLOW_HEAD_MAX_OUT),
                         ('CWN_FLOW_HEAD_CHUNK', _ffi.FLOW_HEAD_CHUNK)):
        assert int(re.search(r'#define ' + macro + r' (\d+)', header).group(1)) == value
    lib = _ffi.lib()
    for name in names:
        assert hasattr(lib, name)
    # the workspace: one row of K floats per slot, N / CHUNK + C slots
    assert lib.cwn_flow_head_workspace_floats(1000, 7, 64) == (1000 // 128 + 7) * 64
    assert lib.cwn_flow_head_workspace_floats(0, 3, 5) == 15
    # every check precedes the first HIP call: the argument errors come back without a device
    f = lib.cwn_flow_head_f32
    assert f(None, 4, 8, None, 1, None, None, None, None, None, 2, None, None, 129, 8, 2, 1, 0, None, 0, None) == 1     # K
    assert f(None, 4, 8, None, 1, None, None, None, None, None, 2, None, None, 8, 8, 65, 1, 0, None, 0, None) == 1      # O
    assert f(None, 4, 8, None, 1, None, None, None, None, None, 2, None, None, 8, 8, 2, 2, 0, None, 0, None) == 1       # abs flag
    assert f(None, 4, 8, None, 1, None, None, None, None, None, 2, None, None, 8, 8, 2, 1, 0, None, 0, None) == 1       # x NULL
    assert f(None, 0, 8, None, 0, None, None, None, None, None, 2, None, None, 8, 8, 2, 1, 0, None, 0, None) == 0       # nothing to do
    assert f(None, 2 ** 31, 8, None, 1, None, None, None, None, None, 2, None, None, 8, 8, 2, 1, 0, None, 0, None) == 2
    b = lib.cwn_flow_head_bwd_f32
    assert b(None, 2, None, None, 4, 8, None, 1, None, None, None, 8, None, 8, 129, 2, 1, 0, None, 0, None) == 1        # H
    assert b(None, 2, None, None, 0, 8, None, 0, None, None, None, 8, None, 8, 8, 2, 1, 0, None, 0, None) == 0


def test_switch_is_off_by_default():
    env = {k: v for k, v in os.environ.items() if k != 'CWN_FUSED_FLOW_HEAD'}
    code = 'from cwn_amd import models; print(models.FUSED_FLOW_HEAD)'
    assert subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, check=True, capture_output=True, text=True).stdout.strip() == 'False'
    env['CWN_FUSED_FLOW_HEAD'] = '1'
    assert subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, check=True, capture_output=True, text=True).stdout.strip() == 'True'
