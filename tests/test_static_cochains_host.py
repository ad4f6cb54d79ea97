"""The static batch of cochains without a GPU: the counted head's and the table launch's bookkeeping in the library (header,
exports, ABI, argument checks before the first HIP call), the stacked epoch tables against `cochain_tables` batch by batch,
the capacity arithmetic with its ValueError, and every construction-time refusal of StaticCochainBatch /
StaticCochainForward / StaticCochainTrainStep."""
import os
import re

import numpy as np
import pytest
import torch

from cwn_amd import _ffi, layers, models, packed, static_cochains, static_graph
from cwn_amd.complex import Cochain
from cwn_amd.synthetic import edge_flows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('cwn_flow_head_dev_f32', 'cwn_flow_head_bwd_dev_f32', 'cwn_table_advance')


def _flows():
    """Cochains of three meshes; number 2 has no upper adjacency, number 4 has no cells."""
    cs = edge_flows(3, side=6, seed=5) + edge_flows(2, side=4, seed=6, holes=False) + edge_flows(2, side=9, seed=7)
    c = cs[2]
    cs[2] = Cochain(dim=1, x=c.x, lower_index=c.lower_index, lower_orient=c.lower_orient, y=c.y)
    z = torch.zeros(2, 0, dtype=torch.long)
    cs[4] = Cochain(dim=1, x=torch.zeros(0, 1), upper_index=z, lower_index=z.clone(), upper_orient=torch.zeros(0),
                    lower_orient=torch.zeros(0), y=torch.tensor([1]))
    return cs


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'cwn_hip.h')).read()
    lib = _ffi.lib()
    for name in NEW:
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert name in _ffi.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None, name
    assert int(re.search(r'#define CWN_ABI_VERSION (\d+)', header).group(1)) == _ffi.ABI_VERSION == 24
    # the counted section states the count contract; the host-count section still says what it said
    section = header[header.index('The counted form of that head'):header.index('cwn_flow_head_bwd_dev_f32(')]
    for words in ('CAPACITIES', 'c_dev', 'n_dev', 'clamped', 'NEVER WRITTEN', 'ZEROS', 'SAME BITS', 'm_dev = c_dev'):
        assert words in section, words
    old = header[header.index('The edge-flow readout head'):header.index('cwn_flow_head_bwd_f32(')]
    assert 'NO m_dev' in old and 'no static batch reaches' in old
    # the counted forms take the host-count arguments with the two device words in front of the workspace
    assert len(lib.cwn_flow_head_dev_f32.argtypes) == len(lib.cwn_flow_head_f32.argtypes) + 2
    assert len(lib.cwn_flow_head_bwd_dev_f32.argtypes) == len(lib.cwn_flow_head_bwd_f32.argtypes) + 2


def test_argument_checks_precede_the_first_hip_call():
    lib = _ffi.lib()
    BAD, TOO_LARGE, ALIGN = 1, 2, 5                       # CWN_ERR_BAD_ARG, CWN_ERR_TOO_LARGE, CWN_ERR_ALIGN
    f = lib.cwn_flow_head_dev_f32
    #        x    N  ldx ptr   C  W1    b1    W2    b2    out  ldo pool  h     K   H  O  abs mean n_dev c_dev ws  n  stream
    assert f(None, 4, 8, None, 1, None, None, None, None, None, 2, None, None, 129, 8, 2, 1, 0, None, None, None, 0, None) == BAD   # K
    assert f(None, 4, 8, None, 1, None, None, None, None, None, 2, None, None, 8, 8, 65, 1, 0, None, None, None, 0, None) == BAD    # O
    assert f(None, 4, 8, None, 1, None, None, None, None, None, 2, None, None, 8, 8, 2, 1, 2, None, None, None, 0, None) == BAD     # mean flag
    assert f(None, 4, 8, None, 1, None, None, None, None, None, 2, None, None, 8, 8, 2, 1, 0, None, None, None, 0, None) == BAD     # x NULL
    assert f(None, 0, 8, None, 0, None, None, None, None, None, 2, None, None, 8, 8, 2, 1, 0, None, None, None, 0, None) == 0       # nothing to do
    assert f(None, 2 ** 31, 8, None, 1, None, None, None, None, None, 2, None, None, 8, 8, 2, 1, 0, None, None, None, 0, None) == TOO_LARGE
    # every pointer given and aligned but c_dev: the counted form needs the cochain count
    p = 4096
    assert f(p, 4, 8, p, 1, p, None, p, None, p, 2, None, None, 8, 8, 2, 1, 0, None, None, p, 64, None) == BAD
    assert f(p, 4, 8, p, 1, p, None, p, None, p, 2, None, None, 8, 8, 2, 1, 0, None, p + 4, p, 64, None) == ALIGN                  # c_dev off 8
    assert f(p, 4, 8, p, 1, p, None, p, None, p, 2, None, None, 8, 8, 2, 1, 0, p + 4, p, p, 64, None) == ALIGN                     # n_dev off 8
    assert f(p + 2, 4, 8, p, 1, p, None, p, None, p, 2, None, None, 8, 8, 2, 1, 0, None, p, p, 64, None) == ALIGN                  # x off 4
    b = lib.cwn_flow_head_bwd_dev_f32
    #        g    ldg h     x    N  ldx ptr   C  W1    W2    dx  lddx dh    K  H    O  abs mean n_dev c_dev ws  n  stream
    assert b(None, 2, None, None, 4, 8, None, 1, None, None, None, 8, None, 8, 129, 2, 1, 0, None, None, None, 0, None) == BAD      # H
    assert b(None, 2, None, None, 0, 8, None, 0, None, None, None, 8, None, 8, 8, 2, 1, 0, None, None, None, 0, None) == 0
    assert b(p, 2, p, p, 4, 8, p, 1, p, p, None, 8, None, 8, 8, 2, 1, 0, None, None, p, 64, None) == BAD                           # c_dev NULL
    assert b(p, 2, p, p, 4, 8, p, 1, p, p, None, 8, None, 8, 8, 2, 1, 0, None, p + 4, p, 64, None) == ALIGN
    assert b(p, 2, p, p, 4, 8, p, 1, p, p, p, 8, None, 8, 8, 2, 1, 0, None, p, p, 64, None) == BAD                                 # dx is x
    a = lib.cwn_table_advance
    assert a(None, 1, 8, p, p, None) == BAD and a(p, 0, 8, p, p, None) == BAD and a(p, 1, 0, p, p, None) == BAD
    assert a(p, 1, 8, p + 4, p, None) == ALIGN and a(p, 1, 2 ** 31, p, p, None) == TOO_LARGE


@pytest.mark.parametrize('B', [4, 7])
def test_stacked_epoch_tables_equal_cochain_tables_batch_by_batch(B):
    cs = _flows()
    meta = packed.cochain_meta(cs)
    batches = [[0, 1, 2, 3], [6, 5, 4], [3], [2, 4], [4], [1, 1, 5, 1]]
    lay = packed.cochain_epoch_layout(meta, B)
    tab = packed.cochain_epoch_tables(meta, batches, B)
    assert tab.dtype == np.int64 and tab.shape == (len(batches), lay['len']) and lay['len'] % 2 == 0
    row0 = np.cumsum(meta['n_cells']) - meta['n_cells']
    for r, idx in zip(tab, batches):
        t = packed.cochain_tables(meta, idx)
        b, n = t['B'], t['num_cells']
        for key in meta['keys']:
            dst = r[lay['dst_' + key]:lay['dst_' + key] + B + 1]
            assert dst[:b + 1].tolist() == t['dst'][key].tolist() and (dst[b + 1:] == t['dst'][key][-1]).all(), key
            src = r[lay['src_' + key]:lay['src_' + key] + B]
            assert src[:b].tolist() == t['src'][key].tolist() and (src[b:] == 0).all(), key
        for o in (lay['cell_off'], lay['cell_off'] + B):
            assert r[o:o + b].tolist() == t['cell_off'].tolist()
        seg = r[lay['seg']:lay['seg'] + B + 1]
        assert seg[:b + 1].tolist() == t['seg'].tolist() and (seg[b + 1:] == n).all()         # absent cochains: empty segments
        assert r[lay['row0']:lay['row0'] + b].tolist() == row0[np.asarray(idx)].tolist()
        assert r[lay['one_dst']:lay['one_dst'] + B + 1].tolist() == [0] + [1] * B
        assert (r[lay['zero_src']:lay['zero_src'] + B] == 0).all()
        counts = dict(zip(packed.EPOCH_COUNTS, r[lay['counts']:lay['counts'] + 4].tolist()))
        assert counts == {'rows': n, 'upper_index': t['slices']['upper_index'][-1], 'lower_index': t['slices']['lower_index'][-1],
                          'cochains': b}
        assert (r[lay['counts'] + 4:] == 0).all()
    with pytest.raises(ValueError, match='exceed the capacity 2'):
        packed.cochain_epoch_tables(meta, [[0, 1, 2]], 2)


def test_capacity_arithmetic_and_its_value_error():
    cs = _flows()
    meta = packed.cochain_meta(cs)
    n = np.sort(meta['n_cells'])
    up = np.sort(meta['length'][meta['keys'].index('upper_index')])
    lo = np.sort(meta['length'][meta['keys'].index('lower_index')])
    caps = static_cochains.capacities(meta, 3)
    assert caps == {'rows': int(n[-3:].sum()), 'upper_index': int(up[-3:].sum()), 'lower_index': int(lo[-3:].sum())}
    # more cochains per batch than the dataset has: everything; distinct from one another and from the batch size
    caps = static_cochains.capacities(meta, 40)
    assert caps['rows'] == int(n.sum()) and len({40, *caps.values()}) == 4
    caps = static_cochains.capacities(meta, 2, {'rows': 3000, 'upper_index': 3000, 'lower_index': 3000})
    assert caps == {'rows': 3000, 'upper_index': 3001, 'lower_index': 3002}
    assert static_cochains.capacities(meta, int(n[-1]), {'rows': int(n[-1])})['rows'] == int(n[-1]) + 1      # ... and from the batch size
    with pytest.raises(ValueError, match=r"caps\['rows'\] = 10 is below the largest cochain"):
        static_cochains.capacities(meta, 2, {'rows': 10})
    with pytest.raises(ValueError, match='unknown entries'):
        static_cochains.capacities(meta, 2, {'cells': 10})
    caps = static_cochains.capacities(meta, 2)
    static_cochains.check_capacity(meta, [[5, 6], [0, 4], [2]], 2, caps)
    tight = dict(caps, lower_index=int(lo[-1]))
    with pytest.raises(ValueError, match=r"batch 1: \d+ entries of 'lower_index' exceed the capacity"):
        static_cochains.check_capacity(meta, [[0, 4], [5, 6]], 2, tight)
    with pytest.raises(ValueError, match=r'batch 0: \d+ rows exceed the capacity'):
        static_cochains.check_capacity(meta, [[5, 6]], 2, dict(caps, rows=int(n[-1])))
    with pytest.raises(ValueError, match='batch 1: 1 .. 2 cochains'):
        static_cochains.check_capacity(meta, [[0], [0, 1, 2]], 2, caps)
    with pytest.raises(IndexError):
        static_cochains.check_capacity(meta, [[0, 7]], 2, caps)


def test_static_cochain_batch_refusals():
    cs = edge_flows(3, side=6, seed=2)
    with pytest.raises(ValueError, match='with_csr=True'):
        static_cochains.StaticCochainBatch(packed.PackedCochains(cs, 'cpu', with_csr=False), 2)
    pc = packed.PackedCochains.__new__(packed.PackedCochains)          # (a packed dataset that claims its plans, on the host)
    pc.with_csr, pc.device = True, torch.device('cpu')
    with pytest.raises(_ffi.CwnError, match='on the GPU'):
        static_cochains.StaticCochainBatch(pc, 2)
    pc.device = torch.device('cuda:0')
    with pytest.raises(ValueError, match='1 .. 64 slots'):
        static_cochains.StaticCochainBatch(pc, 2, slots=65)
    with pytest.raises(ValueError, match='1 .. 64 slots'):
        static_cochains.StaticCochainBatch(pc, 2, slots=0)
    with pytest.raises(TypeError, match='PackedCochains'):
        static_cochains.StaticCochainBatch(object(), 2)


def _refused(model, match, training=False):
    for who in ('StaticCochainForward',) + (('StaticCochainTrainStep',) if training else ()):
        with pytest.raises(NotImplementedError, match=match):
            static_graph.refuse_unsupported_flow_model(model, who, training=who.endswith('TrainStep'))


def test_model_refusals_name_the_layer_or_option():
    ok = models.EdgeOrient(1, 2, 2, 8)
    static_graph.refuse_unsupported_flow_model(ok, 'x', training=True)
    static_graph.refuse_unsupported_flow_model(models.EdgeMPNN(1, 2, 2, 8, readout='mean'), 'x', training=True)
    m = models.EdgeOrient(1, 2, 2, 8)
    m.convs[1].update_up_nn = torch.nn.Linear(8, 8, bias=True)
    _refused(m, r'convs\.1\.update_up_nn is a Linear with a bias', training=True)
    m = models.EdgeOrient(1, 2, 2, 8)
    m.convs[0].update_nn = torch.nn.Sequential(torch.nn.Linear(1, 8, bias=False))
    _refused(m, r'convs\.0\.update_nn is a user callable \(Sequential\)', training=True)
    m = models.EdgeOrient(1, 2, 2, 8)
    m.convs[1].aggr_down = 'mean'
    _refused(m, r"convs\.1 reduces with aggr_down='mean'", training=True)
    _refused(models.EdgeOrient(1, 2, 2, 8).double(), 'float64', training=True)
    with pytest.raises(NotImplementedError, match='dropout_rate = 0.5'):
        static_graph.refuse_unsupported_flow_model(models.EdgeOrient(1, 2, 2, 8, dropout_rate=0.5), 'StaticCochainTrainStep', training=True)
    m = models.EdgeOrient(1, 2, 2, 8)
    m.readout = 'max'
    _refused(m, "readout 'max'", training=True)
    _refused(models.EdgeOrient(1, 2, 2, 132), 'beyond the layer launch', training=True)
    _refused(models.EdgeOrient(1, 65, 2, 8), r'beyond the counted head.s limits \(128 / 64\)', training=True)
    m = models.EdgeOrient(1, 2, 1, 8)
    m.lin1 = torch.nn.Linear(8, 130)
    m.lin2 = torch.nn.Linear(130, 2)
    _refused(m, r'beyond the counted head.s limits', training=True)
    _refused(models.SparseCIN(1, 2, 2, 8), 'SparseCIN is not served', training=True)

    class Mine(layers.OrientedConv):
        def message_up(self, up_x_j, up_attr):
            return up_x_j

    m = models.EdgeOrient(1, 2, 2, 8)
    c = m.convs[0]
    m.convs[0] = Mine(1, 1, 1, c.update_up_nn, c.update_down_nn, c.update_nn, c.act_fn)
    _refused(m, r'convs\.0 \(Mine\) is not a plain OrientedConv', training=True)


def test_include_partial_and_active_dropout_are_refused_by_the_counted_route():
    """The counted head has no per-cell output and no dropout: a model that reaches it with either says so (the step drivers
    refuse active dropout at construction; include_partial is a per-call argument)."""
    class Data:
        num_cochains, ptr_dev, head_counts = 2, None, (None, None)
    m = models.EdgeOrient(1, 2, 1, 8)
    with pytest.raises(NotImplementedError, match='include_partial'):
        models._edge_readout(m, Data(), torch.zeros(3, 8), True)
    m = models.EdgeOrient(1, 2, 1, 8, dropout_rate=0.5).train()
    with pytest.raises(NotImplementedError, match='active dropout'):
        models._edge_readout(m, Data(), torch.zeros(3, 8), False)
    assert models.FUSED_FLOW_HEAD is (os.environ.get('CWN_FUSED_FLOW_HEAD') == '1')      # the switch is not touched
