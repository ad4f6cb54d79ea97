"""Host-side checks of the molecular graph baseline (csrc/cwn_gine.hip, ops.gine_layer, layers.GINEConv, models.EmbedGIN) --
no GPU needed: the C ABI (symbol, ABI number, descriptor layout, every argument check of cwn_gine_layer_f32: they all
precede the first HIP call), the op's refusals, EmbedGIN's state_dict keys and shapes against a literal list written down
from the reference's constructor (mp/molec_models.py:514-552, mp/layers.py:500-506), the model on the CPU against the float64
restatement of tests/_gine.py, and the reference's own property (mp/test_molec_models.py:119-164): batched equals
unbatched.  The bar where values are compared is tests/_product.gate: max|delta| <= 1e-5 * max(1, |ref|_inf)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest
import torch

from cwn_amd import _ffi, layers, models, ops
from cwn_amd.cell_mp import IndexedRows
from cwn_amd.complex import ComplexBatch
from tests import _gin, _gine
from tests import test_gin_host as gin_host
from tests._product import dummy_complex, gate, list_names

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, TOO_LARGE, ALIGN = 0, 1, 2, 5
P = gin_host.P


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_new_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'cwn_hip.h')).read()
    lib = _ffi.lib()
    assert re.search(r'\bint cwn_gine_layer_f32\s*\(', header)
    assert 'cwn_gine_layer_f32' in _ffi.EXPORTS and hasattr(lib, 'cwn_gine_layer_f32')
    assert lib.cwn_abi_version() == _ffi.ABI_VERSION == 24
    assert int(re.search(r'#define CWN_ABI_VERSION (\d+)', header).group(1)) == 24
    section = header[header.index('GINEConv as one launch'):header.index('int cwn_gine_layer_f32')]
    assert 'NO m_dev' in section and 'no static batch reaches this launch' in section
    makefile = open(os.path.join(ROOT, 'cwn_amd', 'csrc', 'Makefile')).read()
    assert 'cwn_gine.hip' in makefile and 'cwn_gin_tile.h' in makefile
    assert callable(_ffi.gine_layer)


def test_descriptor_layout_matches_the_header(tmp_path):
    """cwn_gine_desc field by field against the ctypes mirror -- the embedded cwn_gin_desc's fields included -- through a probe
    compiled with the host C compiler."""
    st = _ffi.GineDesc
    assert [f for f, _ in st._fields_] == ['g', 'e', 'eidx', 'lde', 'n_e'] and dict(st._fields_)['g'] is _ffi.GinDesc
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cwn_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(cwn_gine_desc));']
    lines += [f'printf("{f} %zu\\n", offsetof(cwn_gine_desc, {f}));' for f, _ in st._fields_]
    lines += [f'printf("g.{f} %zu\\n", offsetof(cwn_gine_desc, g.{f}));' for f, _ in _ffi.GinDesc._fields_]
    lines += ['return 0; }']
    src, exe = tmp_path / 'probe.c', tmp_path / 'probe'
    src.write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got['size']) == C.sizeof(st)
    for f, _ in st._fields_:
        assert int(got[f]) == getattr(st, f).offset, f
    for f, _ in _ffi.GinDesc._fields_:
        assert int(got[f'g.{f}']) == st.g.offset + getattr(_ffi.GinDesc, f).offset, f


def _desc(e=20 * P, eidx=21 * P, lde=8, n_e=4, **kw):
    """A descriptor that passes every check (tests/test_gin_host.py::_desc for `g`, made-up aligned addresses for the edge
    operand): every case below breaks exactly one thing."""
    return _ffi.GineDesc(g=gin_host._desc(**kw), e=e, eidx=eidx, lde=lde, n_e=n_e)


def _call(d):
    return _ffi.lib().cwn_gine_layer_f32(C.byref(d), None)


@pytest.mark.parametrize('case', sorted(gin_host.BAD))
def test_inherited_bad_arguments_are_refused_before_any_hip_call(case):
    assert _call(_desc(**gin_host.BAD[case])) == BAD_ARG, case


BAD_EDGE = {'e NULL with rowptr': dict(e=None), 'eidx NULL with rowptr': dict(eidx=None), 'lde < w': dict(lde=7),
            'n_e < 0': dict(n_e=-1)}


@pytest.mark.parametrize('case', sorted(BAD_EDGE))
def test_bad_edge_operands_are_refused_before_any_hip_call(case):
    assert _call(_desc(**BAD_EDGE[case])) == BAD_ARG, case


def test_null_descriptor_misaligned_pointers_and_too_many_tiles():
    assert _ffi.lib().cwn_gine_layer_f32(None, None) == BAD_ARG
    for field in ('x', 'rowptr', 'col', 'eps_dev', 'W1', 'b1', 'scale1', 'shift1', 'W2', 'b2', 'scale2', 'shift2', 'out'):
        assert _call(_desc(**{field: 40 * P + 2})) == ALIGN, field
    for field in ('e', 'eidx'):
        assert _call(_desc(**{field: 40 * P + 2})) == ALIGN, field
    assert _call(_desc(w=0, e=40 * P + 2)) == BAD_ARG           # the argument checks of `g` come first
    assert _call(_desc(n=_ffi.GIN_TM * (2 ** 31 - 1), x=0x10, out=0x7f0000000000)) == TOO_LARGE


def test_empty_launches_and_legal_shapes_are_ok_without_a_device():
    """n == 0 returns before the first HIP call; without a rowptr the edge operand may be absent."""
    assert _call(_desc(n=0)) == OK
    assert _call(_desc(n=0, x=None, out=None, W1=None, W2=None)) == OK
    assert _call(_desc(n=0, rowptr=None, col=None, e=None, eidx=None, lde=0, n_e=0)) == OK
    assert _call(_desc(n=0, rowptr=None, col=None, eps_dev=None, b1=None, scale1=None, shift1=None, b2=None, scale2=None,
                       shift2=None, e=None, eidx=None)) == OK
    assert _call(_desc(n=0, ldx=32, ldout=32, out=P + 4 * 8)) == OK


# ---- the op ---------------------------------------------------------------------------------------------------------------------
def test_op_refuses_cpu_tensors_and_other_dtypes():
    x, e = torch.randn(4, 3), torch.randn(2, 3)
    st = [(torch.randn(5, 3), None, None, None), (torch.randn(5, 5), None, None, None)]
    assert ops.gine_layer_applies(x, e, st) is False
    with pytest.raises(TypeError, match='gine_layer: x must be a float32 tensor on the GPU'):
        ops.gine_layer(x, None, None, None, st, 'relu')
    with pytest.raises(TypeError, match='gine_layer: x must be float32 .got torch.float64.'):
        ops.gine_layer(x.double(), None, None, None, st, 'relu')
    with pytest.raises(TypeError, match='gine_layer: edge must be a float32 tensor on the GPU .got torch.float32 on cpu.'):
        ops.gine_layer(x, None, e, None, st, 'relu')
    with pytest.raises(TypeError, match='gine_layer: edge must be float32 .got torch.float16.'):
        ops.gine_layer(x, None, e.half(), None, st, 'relu')
    with pytest.raises(ValueError, match='edge_mode'):
        ops.gine_layer(x, None, None, None, st, 'relu', edge_mode='col')
    assert list(inspect.signature(ops.gine_layer).parameters) == ['x', 'adj', 'edge', 'eps', 'stages', 'act', 'act_post', 'out',
                                                                  'edge_mode']


# ---- layers.GINEConv on the CPU ---------------------------------------------------------------------------------------------------
def _net(w, H):
    return torch.nn.Sequential(torch.nn.Linear(w, H), torch.nn.Identity(), torch.nn.ReLU(),
                               torch.nn.Linear(H, H), torch.nn.Identity(), torch.nn.ReLU())


def test_gine_conv_state_signature_and_cpu_routes():
    assert list(inspect.signature(layers.GINEConv.__init__).parameters) == ['self', 'nn', 'eps', 'train_eps']
    assert list(inspect.signature(layers.GINEConv.forward).parameters) == ['self', 'x', 'edge_index', 'edge_attr', 'out', 'act_post']
    for trained in (False, True):
        conv = layers.GINEConv(torch.nn.Sequential(torch.nn.Linear(3, 4)), eps=0.25, train_eps=trained)
        assert torch.equal(conv.state_dict()['eps'], torch.tensor([0.25]))
        assert isinstance(conv.eps, torch.nn.Parameter) is trained
        with torch.no_grad():
            conv.eps.fill_(2.0)
        conv.reset_parameters()
        assert float(conv.eps.detach()) == 0.25
    torch.manual_seed(3)
    conv = layers.GINEConv(_net(3, 4), eps=0.3).eval()
    x, cells = torch.randn(6, 3), torch.randn(2, 3)
    idx = torch.tensor([[0, 1, 2, 5], [1, 0, 1, 1]])
    shared = torch.tensor([0, 0, 1, 1])
    st = [(conv.nn[0].weight, conv.nn[0].bias, None, None), (conv.nn[3].weight, conv.nn[3].bias, None, None)]
    assert conv.last_route is None
    for on in (True, False):
        old, layers.FUSED_GINE = layers.FUSED_GINE, on
        try:
            with torch.no_grad():
                assert conv.fused_stages(x, cells) is None
                lazy = conv(x, idx, IndexedRows(cells, shared))
                dense = conv(x, idx, cells[shared])
                narrow = conv(x, idx, cells[shared][:, :1])            # an edge width of 1 broadcasts, as in torch_geometric
                alone = conv(x, None, None)
        finally:
            layers.FUSED_GINE = old
        assert conv.last_route == 'generic'
        gate(lazy, _gine.gine_formula64(x, idx, cells, shared, 0.3, st, 'relu'), 'GINEConv on the CPU, IndexedRows')
        gate(dense, _gine.gine_formula64(x, idx, cells[shared], 'perm', 0.3, st, 'relu'), 'GINEConv on the CPU, dense')
        gate(narrow, _gine.gine_formula64(x, idx, cells[shared][:, :1].expand(4, 3), 'perm', 0.3, st, 'relu'), 'edge width 1')
        gate(alone, _gin.gin_formula64(x, None, 0.3, st, 'relu'), 'no edges')
    assert layers.FUSED_GINE_DEFAULT in (True, False) and isinstance(layers.FUSED_GINE, bool)


# ---- models.EmbedGIN: structure ----------------------------------------------------------------------------------------------------
ATOMS, BONDS, OUT, LAYERS, HID = 32, 12, 3, 3, 8      # (the dummy complexes' bond features reach 9)


def _expected(embed_edge, embed_dim):
    """Written down from mp/molec_models.py:514-552: the two embeddings registered on the model AND inside init_conv (an
    EmbedVEWithReduce keeps them as v_embed_layer / e_embed_layer, mp/layers.py:504-505; InitReduceConv has no state),
    num_layers GINEConv over Linear(layer_dim, hidden), BN, act, Linear(hidden, hidden), BN, act, then lin1 and lin2."""
    E = HID if embed_dim is None else embed_dim
    keys = {'v_embed_init.weight': (ATOMS, E), 'init_conv.v_embed_layer.weight': (ATOMS, E)}
    if embed_edge:
        keys.update({'e_embed_init.weight': (BONDS, E), 'init_conv.e_embed_layer.weight': (BONDS, E)})
    for i in range(LAYERS):
        keys.update(gin_host._conv_keys(f'convs.{i}', E if i == 0 else HID, HID))
    keys.update({'lin1.weight': (HID, HID), 'lin1.bias': (HID,), 'lin2.weight': (OUT, HID), 'lin2.bias': (OUT,)})
    return keys


@pytest.mark.parametrize('embed_edge', [False, True])
@pytest.mark.parametrize('embed_dim', [None, 12])
def test_state_dict_keys_and_shapes_are_the_references(embed_edge, embed_dim):
    m = models.EmbedGIN(ATOMS, BONDS, OUT, LAYERS, HID, embed_edge=embed_edge, embed_dim=embed_dim)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == _expected(embed_edge, embed_dim)
    assert m.state_dict()['v_embed_init.weight'].data_ptr() == m.state_dict()['init_conv.v_embed_layer.weight'].data_ptr()
    assert m.max_dim == 1 and (m.e_embed_init is not None) is embed_edge
    assert isinstance(m.reduce_init, layers.InitReduceConv) and isinstance(m.init_conv, layers.EmbedVEWithReduce)
    assert m.init_conv.init_reduce is m.reduce_init
    for conv in m.convs:
        assert isinstance(conv, layers.GINEConv) and tuple(conv.eps.shape) == (1,) and not isinstance(conv.eps, torch.nn.Parameter)
    assert repr(m) == 'EmbedGIN'
    m.reset_parameters()


def test_constructor_signature_is_the_references():
    want = ['self', 'atom_types', 'bond_types', 'out_size', 'num_layers', 'hidden', 'dropout_rate', 'nonlinearity', 'readout',
            'train_eps', 'apply_dropout_before', 'init_reduce', 'embed_edge', 'embed_dim']
    sig = inspect.signature(models.EmbedGIN.__init__)
    assert list(sig.parameters) == want
    defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(dropout_rate=0.5, nonlinearity='relu', readout='sum', train_eps=False, apply_dropout_before='lin2',
                            init_reduce='sum', embed_edge=False, embed_dim=None)
    m = models.EmbedGIN(ATOMS, BONDS, OUT, 2, HID, train_eps=True)
    assert all(isinstance(c.eps, torch.nn.Parameter) for c in m.convs)
    with pytest.raises(NotImplementedError):
        models.EmbedGIN(ATOMS, BONDS, OUT, 2, HID, readout='max')


# ---- models.EmbedGIN on the CPU against the float64 restatement ---------------------------------------------------------------------
MIXED = ['house', 'fullstop', 'kite', 'colon', 'molecular', 'bridged']          # 'fullstop' and 'colon' have no edges
_BATCHES = {}


def cpu_batch(names, edge_features: bool):
    """The dummy complexes `names` collated up to dimension 1 (built once per case); edge_features False: cochains[1].x is
    None, as the reference's test sets it, and the edges start from the reduction of their vertices."""
    key = (tuple(names), edge_features)
    if key not in _BATCHES:
        b = ComplexBatch.from_complex_list([dummy_complex(n) for n in names], max_dim=1)
        if not edge_features and 1 in b.cochains:
            b.cochains[1].x = None
        _BATCHES[key] = b
    return _BATCHES[key]


def fresh(batch):
    """EmbedGIN.forward replaces the batch's features by their embeddings (data.set_xs, as the reference does): every
    forward gets a copy."""
    import copy
    return copy.deepcopy(batch)


def make_model(act='relu', readout='sum', train_eps=False, embed_edge=False, seed=0, **kw):
    torch.manual_seed(seed)
    m = models.EmbedGIN(ATOMS, BONDS, OUT, LAYERS, HID, nonlinearity=act, readout=readout, train_eps=train_eps,
                        embed_edge=embed_edge, **kw)
    return _gin.randomise(m, seed + 1).eval()


@pytest.mark.parametrize('act', ['relu', 'elu', 'tanh', 'sigmoid', 'id'])
@pytest.mark.parametrize('readout,train_eps,embed_edge', [('sum', False, False), ('mean', True, True)])
def test_embed_gin_on_the_cpu_against_the_float64_restatement(act, readout, train_eps, embed_edge):
    model = make_model(act, readout, train_eps, embed_edge, seed=5)
    batch = cpu_batch(MIXED, edge_features=embed_edge)
    ref = _gine.embed_gin64_of(_gin.state64(model), batch, act=act, readout=readout)
    assert tuple(ref.shape) == (len(MIXED), OUT) and float(ref.abs().max()) > 1e-3
    with torch.no_grad():
        out = model(fresh(batch))
    gate(out, ref, f'EmbedGIN {act} {readout} train_eps={train_eps} embed_edge={embed_edge}')
    assert all(c.last_route == 'generic' for c in model.convs)
    if train_eps:
        assert all(float(c.eps.detach()) != 0.0 for c in model.convs)


@pytest.mark.parametrize('init_reduce', ['mean', 'max'])
def test_embed_gin_other_init_reduces_and_a_complex_without_edges(init_reduce):
    model = make_model(seed=7, init_reduce=init_reduce)
    batch = cpu_batch(MIXED, edge_features=False)
    with torch.no_grad():
        gate(model(fresh(batch)), _gine.embed_gin64_of(_gin.state64(model), batch, init_reduce=init_reduce), init_reduce)
        alone = ComplexBatch.from_complex_list([dummy_complex('fullstop')], max_dim=1)
        gate(model(fresh(alone)), _gine.embed_gin64_of(_gin.state64(model), alone, init_reduce=init_reduce), 'no edges at all')


def test_batched_equals_unbatched_as_in_the_references_test():
    """mp/test_molec_models.py:119-164: EmbedGIN(32, 4, 3, num_layers=3, hidden=5).eval() on the testing list (which holds
    complexes without edges), cochains[1].x and cochains[2].x None, batch sizes 2 .. len(list): batched == unbatched within
    atol 1e-6."""
    names = list_names('testing')
    assert 'fullstop' in names
    torch.manual_seed(0)
    model = models.EmbedGIN(atom_types=32, bond_types=4, out_size=3, num_layers=3, hidden=5).eval()

    def run(group):
        b = ComplexBatch.from_complex_list([dummy_complex(n) for n in group], max_dim=1)
        for d in (1, 2):
            if d in b.cochains:
                b.cochains[d].x = None
        with torch.no_grad():
            return model(b)
    unbatched = torch.cat([run([n]) for n in names])
    assert tuple(unbatched.shape) == (len(names), 3)
    for bs in range(2, len(names) + 1):
        batched = torch.cat([run(names[i:i + bs]) for i in range(0, len(names), bs)])
        assert torch.allclose(unbatched, batched, atol=1e-6), bs


def test_training_mode_on_the_cpu_is_differentiable_at_every_dropout_position():
    for pos in ('lin1', 'final_readout', 'lin2'):
        torch.manual_seed(1)
        model = models.EmbedGIN(ATOMS, BONDS, OUT, 2, HID, train_eps=True, apply_dropout_before=pos, dropout_rate=0.2).train()
        out = model(fresh(cpu_batch(MIXED, edge_features=False)))
        out.square().sum().backward()
        for k, p in model.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), (pos, k)
