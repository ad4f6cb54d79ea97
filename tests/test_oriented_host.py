"""Host-side checks of the fused OrientedConv layer (csrc/cwn_oriented.hip) and of what rides on it -- no GPU needed:
the C ABI (symbols, ABI number, every argument check of cwn_oriented_layer_f32 / cwn_oriented_dz_f32: they all precede the
first HIP call), the EdgeMPNN mirror's structure, the dispatch's refusal of CPU tensors and biased maps, and the synthetic
edge-flow construction.

EdgeMPNN has no reference fixture and this project computes nothing on the CPU (a CPU tensor is a CwnError: "no CPU
fallback"), so its forward is compared with a float64 restatement of mp/models.py:589-612 where it runs -- on the device,
tests/test_gpu_oriented.py::test_edge_mpnn_against_float64_restatement.  Here: its state_dict keys, its layers, and that a CPU
batch is refused exactly as every other model of the package refuses it."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from cwn_amd import _ffi, layers, models, ops, synthetic
from cwn_amd.complex import CochainBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, ALIGN = 0, 1, 5


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'cwn_hip.h')).read()
    lib = _ffi.lib()
    for name in ('cwn_oriented_layer_f32', 'cwn_oriented_dz_f32'):
        assert re.search(rf'\bint {name}\s*\(', header), name
        assert name in _ffi.EXPORTS
        assert hasattr(lib, name)
    assert lib.cwn_abi_version() == _ffi.ABI_VERSION == 24
    assert int(re.search(r'#define CWN_ABI_VERSION (\d+)', header).group(1)) == 24
    acts = re.search(r'enum \{ CWN_ACT_ID = 0, CWN_ACT_RELU = 1, CWN_ACT_ELU = 2[^,]*, CWN_ACT_TANH = 3, CWN_ACT_SIGMOID = 4 \}', header)
    assert acts is not None
    assert (_ffi.ACT_ID, _ffi.ACT_RELU, _ffi.ACT_ELU, _ffi.ACT_TANH, _ffi.ACT_SIGMOID) == (0, 1, 2, 3, 4)
    assert ops.ACTS == {'id': 0, 'relu': 1, 'elu': 2, 'tanh': 3, 'sigmoid': 4}
    m = re.search(r'#define CWN_ORIENTED_TM\(w\) \(\(w\) <= (\d+) \? (\d+) : (\d+)\)', header)
    for w in (1, 16, 17, 128):
        assert _ffi.oriented_tm(w) == (int(m.group(2)) if w <= int(m.group(1)) else int(m.group(3)))


def test_descriptor_layout_matches_the_header(tmp_path):
    """cwn_oriented_desc field by field against the ctypes mirror, through a probe compiled with the host C compiler."""
    import subprocess
    st = _ffi.OrientedDesc
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cwn_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(cwn_oriented_desc));']
    lines += [f'printf("{f} %zu\\n", offsetof(cwn_oriented_desc, {f}));' for f, _ in st._fields_]
    lines += ['return 0; }']
    src, exe = tmp_path / 'probe.c', tmp_path / 'probe'
    src.write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got['size']) == C.sizeof(st)
    for f, _ in st._fields_:
        assert int(got[f]) == getattr(st, f).offset, f


def _desc(**kw):
    """A descriptor that passes every check (the pointers are made-up, aligned addresses: a call that passed the checks
    would launch, so every test below breaks exactly one thing)."""
    P = 0x10000
    d = dict(x=P, up_rowptr=2 * P, up_col=3 * P, up_perm=4 * P, up_orient=5 * P, w_up=6 * P, dn_rowptr=7 * P, dn_col=8 * P,
             dn_perm=9 * P, dn_orient=10 * P, w_dn=11 * P, w_self=12 * P, out=13 * P, agg_out=14 * P, n=10, ldx=8, ldout=12,
             w=8, H=12, act=0, w_trans=0, m_dev=None)
    d.update(kw)
    return _ffi.OrientedDesc(**d)


def _call(d):
    return _ffi.lib().cwn_oriented_layer_f32(C.byref(d), None)


BAD = {
    'w=0': dict(w=0), 'w=129': dict(w=129, ldx=129), 'H=0': dict(H=0), 'H=129': dict(H=129, ldout=129), 'n<0': dict(n=-1),
    'x NULL': dict(x=None), 'out NULL': dict(out=None), 'ldx<w': dict(ldx=7), 'ldout<H': dict(ldout=11),
    'act=-1': dict(act=-1), 'act=5': dict(act=5),
    'up: weight without plan': dict(up_rowptr=None), 'up: plan without weight': dict(w_up=None),
    'dn: weight without plan': dict(dn_rowptr=None), 'dn: plan without weight': dict(w_dn=None),
    'up: plan without col': dict(up_col=None), 'dn: orient without perm': dict(dn_perm=None),
    'out aliases x': dict(out=0x10000), 'out aliases agg_out': dict(agg_out=13 * 0x10000),
}


@pytest.mark.parametrize('case', sorted(BAD))
def test_bad_arguments_are_refused_before_any_hip_call(case):
    assert _call(_desc(**BAD[case])) == BAD_ARG, case


def test_null_descriptor_and_misaligned_pointers():
    assert _ffi.lib().cwn_oriented_layer_f32(None, None) == BAD_ARG
    for field in ('x', 'out', 'agg_out', 'w_self', 'w_up', 'w_dn', 'up_orient', 'dn_col', 'up_rowptr'):
        assert _call(_desc(**{field: 0x10000 * 20 + 2})) == ALIGN, field
    assert _call(_desc(m_dev=0x10000 * 20 + 4)) == ALIGN
    # the argument checks come first: a bad width wins over a misaligned pointer
    assert _call(_desc(w=0, x=0x10002)) == BAD_ARG


def test_empty_launches_are_ok_without_a_device():
    """n == 0 returns before the first HIP call, with or without buffers."""
    assert _call(_desc(n=0)) == OK
    assert _call(_desc(n=0, x=None, out=None, agg_out=None)) == OK
    # absent streams and an absent self map are legal shapes of the descriptor
    assert _call(_desc(n=0, up_rowptr=None, up_col=None, up_perm=None, up_orient=None, w_up=None)) == OK
    assert _call(_desc(n=0, w_self=None, up_orient=None, up_perm=None)) == OK


def test_dz_argument_checks():
    fn = _ffi.lib().cwn_oriented_dz_f32
    P = 0x10000
    good = [P, 2 * P, 3 * P, 10, 12, 12, 12, 12, 1, None, None]

    def call(**kw):
        names = ('dout', 'out', 'dz', 'n', 'H', 'lddout', 'ldout', 'lddz', 'act', 'm_dev', 'stream')
        a = dict(zip(names, good))
        a.update(kw)
        return fn(*[a[k] for k in names])

    assert call(n=0) == OK
    for kw in (dict(H=0), dict(H=129), dict(n=-1), dict(act=5), dict(act=-1), dict(dout=None), dict(out=None), dict(dz=None),
               dict(lddout=11), dict(ldout=11), dict(lddz=11)):
        assert call(**kw) == BAD_ARG, kw
    assert call(dz=3 * P + 2) == ALIGN
    assert call(m_dev=P + 4) == ALIGN


# ---- EdgeMPNN ---------------------------------------------------------------------------------------------------------------
def test_edge_mpnn_mirrors_the_reference_structure():
    m = models.EdgeMPNN(8, 3, 2, 12)
    assert list(m.state_dict().keys()) == [
        'convs.0.update_down_nn.weight', 'convs.0.update_nn.weight',
        'convs.1.update_down_nn.weight', 'convs.1.update_nn.weight',
        'lin1.weight', 'lin1.bias', 'lin2.weight', 'lin2.bias']
    assert m.fully_invar is True and m.nonlinearity == 'relu' and m.max_dim == 1
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes['convs.0.update_nn.weight'] == (12, 8) and shapes['convs.1.update_down_nn.weight'] == (12, 12)
    assert shapes['lin1.weight'] == (12, 12) and shapes['lin2.weight'] == (3, 12)
    for conv in m.convs:
        assert isinstance(conv, layers.OrientedConv) and conv.orient is False
        assert type(conv.update_up_nn) is layers.ZeroUpdate and not list(conv.update_up_nn.parameters())
        assert conv.act_fn is torch.nn.functional.relu
    assert all(c.orient for c in models.EdgeMPNN(8, 3, 2, 12, fully_invar=False, nonlinearity='tanh').convs)
    import inspect
    assert list(inspect.signature(models.EdgeMPNN.__init__).parameters) == [
        'self', 'num_input_features', 'num_classes', 'num_layers', 'hidden', 'dropout_rate', 'jump_mode', 'nonlinearity',
        'readout', 'fully_invar']
    m.reset_parameters()
    assert repr(m) == 'EdgeMPNN'
    assert layers.ZeroUpdate()(torch.ones(3, 2)) == 0


def _cpu_batch():
    return CochainBatch.from_cochain_list(synthetic.edge_flows(2, 6, 0))


def test_cpu_tensors_and_biased_maps_take_the_present_path():
    """The fused dispatch declines CPU tensors, a Linear with a bias, a user callable, float64 and reduce != add; what then
    runs is today's path, whose answer to a CPU tensor is today's: CwnError (the package computes on the GPU only)."""
    data = _cpu_batch()
    lin = lambda bias=False: torch.nn.Linear(1, 4, bias=bias)
    conv = layers.OrientedConv(1, 1, 1, lin(), lin(), lin(), layers.identity)
    assert layers.FUSED_ORIENTED is True
    assert conv.fused_operands(data.x) is None                          # CPU
    with pytest.raises(_ffi.CwnError, match='GPU only'):
        conv(data)
    assert ops.oriented_layer_applies(data.x, [conv.update_nn.weight]) is False
    with pytest.raises(_ffi.CwnError, match='GPU only'):               # the op itself: an error, never a fallback
        ops.oriented_layer(data.x, None, None, None, None, conv.update_nn.weight, None, None, 'id')
    with pytest.raises(_ffi.CwnError, match='GPU only'):
        models.EdgeMPNN(1, 2, 2, 4)(_cpu_batch())
    with pytest.raises(_ffi.CwnError, match='GPU only'):
        models.EdgeOrient(1, 2, 2, 4)(_cpu_batch())

    # ... and a biased Linear is refused whatever the device (tests/test_gpu_oriented.py walks the dispatch on the GPU)
    biased = layers.OrientedConv(1, 1, 1, lin(True), lin(True), lin(True), layers.identity)
    assert biased.fused_operands(data.x) is None
    with pytest.raises(_ffi.CwnError, match='GPU only'):
        biased(data)
    # the 'id' nonlinearity is one recognisable function object and still the identity
    f = models.get_nonlinearity('id', return_module=False)
    assert f is layers.identity and f is models.get_nonlinearity('id', return_module=False)
    t = torch.randn(3)
    assert f(t) is t


# ---- synthetic.edge_flows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('side', [6, 9])
def test_edge_flow_mesh_is_a_complex_with_two_holes(side):
    m = synthetic.edge_flow_mesh(side)
    B1, B2 = m['B1'].astype(np.int64), m['B2'].astype(np.int64)
    assert not (B1 @ B2).any()                                           # the boundary of a boundary
    assert (np.abs(B1).sum(0) == 2).all() and (B1.sum(0) == 0).all() and (np.abs(B2).sum(0) == 3).all()
    V, E, T = len(m['points']), len(m['edges']), len(m['triangles'])
    assert V - E + T == 1 - 2                                            # Euler characteristic of a disc with two holes
    full = synthetic.edge_flow_mesh(side, holes=False)
    assert len(full['points']) - len(full['edges']) + len(full['triangles']) == 1


def test_edge_flows_layout_signs_and_determinism():
    cs = synthetic.edge_flows(6, 6, seed=3)
    again = synthetic.edge_flows(6, 6, seed=3)
    other = synthetic.edge_flows(6, 6, seed=4)
    assert [int(c.y) for c in cs] == [0, 0, 0, 1, 1, 1]
    differs = False
    for a, b, o in zip(cs, again, other):
        for k in ('x', 'upper_index', 'lower_index', 'upper_orient', 'lower_orient', 'y'):
            assert torch.equal(getattr(a, k), getattr(b, k)), k
        differs = differs or not torch.equal(a.x, o.x) or not torch.equal(a.lower_orient, o.lower_orient)
    assert differs
    E = cs[0].x.size(0)
    for c in cs:
        assert c.dim == 1 and tuple(c.x.shape) == (E, 1) and c.x.dtype == torch.float32
        assert set(c.x.unique().tolist()) <= {-1.0, 0.0, 1.0} and int(c.x.abs().sum()) >= 5        # a path crosses the square
        for index, orient in ((c.lower_index, c.lower_orient), (c.upper_index, c.upper_orient)):
            assert index.dtype == torch.long and orient.dtype == torch.float32 and orient.numel() == index.size(1)
            assert bool(((orient == 1) | (orient == -1)).all())
            # both directions of a pair are stored consecutively and carry the same sign
            assert torch.equal(index[:, 0::2], index[:, 1::2].flip(0))
            assert torch.equal(orient[0::2], orient[1::2])
            assert bool((index[0, 0::2] > index[1, 0::2]).all()) and int(index.max()) < E


def test_edge_flows_adjacency_is_the_sign_pattern_of_the_boundary_products():
    """lower: off-diagonal signs of (B1 T)^T (B1 T), upper: of (T B2)(T B2)^T -- recomputed here entry by entry."""
    m = synthetic.edge_flow_mesh(6)
    E = len(m['edges'])
    t = np.random.default_rng(11).integers(0, 2, E) * 2 - 1
    c = synthetic.edge_flows(2, 6, seed=5, flip=t)[1]
    B1, B2 = m['B1'].astype(np.int64) * t[None, :], m['B2'].astype(np.int64) * t[:, None]
    for A, index, orient in ((B1.T @ B1, c.lower_index, c.lower_orient), (B2 @ B2.T, c.upper_index, c.upper_orient)):
        off = A - np.diag(np.diag(A))
        assert index.size(1) == np.count_nonzero(off)
        assert np.array_equal(off[index[0].numpy(), index[1].numpy()], orient.numpy().astype(np.int64))


def test_flipping_edge_orientations_transforms_features_and_signs():
    """x -> T x and orient_ij -> t_i t_j orient_ij, the indices and the labels unchanged."""
    m = synthetic.edge_flow_mesh(6)
    E = len(m['edges'])
    t = torch.from_numpy(np.random.default_rng(7).integers(0, 2, E) * 2 - 1).float()
    base = synthetic.edge_flows(4, 6, seed=9, flip=np.ones(E))
    flipped = synthetic.edge_flows(4, 6, seed=9, flip=t.numpy())
    assert bool((t == -1).any()) and bool((t == 1).any())
    for a, b in zip(base, flipped):
        assert torch.equal(b.x, a.x * t[:, None]) and torch.equal(a.y, b.y)
        for k in ('lower', 'upper'):
            ia, ib = getattr(a, f'{k}_index'), getattr(b, f'{k}_index')
            assert torch.equal(ia, ib)
            assert torch.equal(getattr(b, f'{k}_orient'), getattr(a, f'{k}_orient') * t[ia[0]] * t[ia[1]])
