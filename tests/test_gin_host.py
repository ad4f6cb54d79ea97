"""Host-side checks of the graph baselines (csrc/cwn_gin.hip, layers.GINConv, models.GIN0 / GIN / GIN0WithJK / GINWithJK /
RingGIN) -- no GPU needed: the C ABI (symbol, ABI number, descriptor layout, every argument check of cwn_gin_layer_f32: they
all precede the first HIP call), the models' state_dict keys and shapes against literal lists written down from the
reference's constructors (mp/graph_models.py, mp/ring_exp_models.py:76-108), the models on the CPU against the float64
restatement of tests/_gin.py, and the receptive field of RingGIN on the ring-transfer data.  The bar where values are
compared is tests/_product.gate: max|delta| <= 1e-5 * max(1, |ref|_inf)."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import pytest
import torch

from cwn_amd import _ffi, layers, models, ops, synthetic
from cwn_amd.complex import ComplexBatch
from tests import _gin
from tests._product import gate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, TOO_LARGE, ALIGN = 0, 1, 2, 5


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_new_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'cwn_hip.h')).read()
    lib = _ffi.lib()
    assert re.search(r'\bint cwn_gin_layer_f32\s*\(', header)
    assert 'cwn_gin_layer_f32' in _ffi.EXPORTS and hasattr(lib, 'cwn_gin_layer_f32')
    assert lib.cwn_abi_version() == _ffi.ABI_VERSION == 24
    assert int(re.search(r'#define CWN_ABI_VERSION (\d+)', header).group(1)) == 24
    assert int(re.search(r'#define CWN_GIN_MAX_WIDTH (\d+)', header).group(1)) == _ffi.GIN_MAX_WIDTH == 128
    assert int(re.search(r'#define CWN_GIN_TM (\d+)', header).group(1)) == _ffi.GIN_TM
    section = header[header.index('GINConv as one launch'):header.index('int cwn_gin_layer_f32')]
    assert 'NO m_dev' in section and 'no static batch reaches this launch' in section
    assert 'cwn_gin.hip' in open(os.path.join(ROOT, 'cwn_amd', 'csrc', 'Makefile')).read()


def test_descriptor_layout_matches_the_header(tmp_path):
    """cwn_gin_desc field by field against the ctypes mirror, through a probe compiled with the host C compiler."""
    st = _ffi.GinDesc
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cwn_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(cwn_gin_desc));']
    lines += [f'printf("{f} %zu\\n", offsetof(cwn_gin_desc, {f}));' for f, _ in st._fields_]
    lines += ['return 0; }']
    src, exe = tmp_path / 'probe.c', tmp_path / 'probe'
    src.write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got['size']) == C.sizeof(st)
    for f, _ in st._fields_:
        assert int(got[f]) == getattr(st, f).offset, f


P = 0x100000


def _desc(**kw):
    """A descriptor that passes every check (made-up, aligned addresses far apart: a call that passed the checks would launch,
    so every case below breaks exactly one thing)."""
    d = dict(x=P, rowptr=2 * P, col=3 * P, eps_dev=4 * P, W1=5 * P, b1=6 * P, scale1=7 * P, shift1=8 * P, W2=9 * P, b2=10 * P,
             scale2=11 * P, shift2=12 * P, out=13 * P, n=10, ldx=8, ldout=12, w=8, H=12, act=1, act_post=0)
    d.update(kw)
    return _ffi.GinDesc(**d)


def _call(d):
    return _ffi.lib().cwn_gin_layer_f32(C.byref(d), None)


BAD = {
    'w=0': dict(w=0), 'w=129': dict(w=129, ldx=129), 'H=0': dict(H=0), 'H=129': dict(H=129, ldout=129), 'n<0': dict(n=-1),
    'act=-1': dict(act=-1), 'act=5': dict(act=5), 'act_post=-1': dict(act_post=-1), 'act_post=5': dict(act_post=5),
    'ldx<w': dict(ldx=7), 'ldout<H': dict(ldout=11), 'x NULL': dict(x=None), 'out NULL': dict(out=None),
    'W1 NULL': dict(W1=None), 'W2 NULL': dict(W2=None), 'rowptr without col': dict(col=None),
    'out aliases x': dict(out=P),
    # two column slices of one [n, 32] buffer: x in columns [0, 8), out in [4, 16) -- they meet; and out in front of x
    'slices that meet': dict(ldx=32, ldout=32, out=P + 4 * 4),
    'slices that meet from below': dict(ldx=32, ldout=32, x=P + 4 * 8, out=P),
}


@pytest.mark.parametrize('case', sorted(BAD))
def test_bad_arguments_are_refused_before_any_hip_call(case):
    assert _call(_desc(**BAD[case])) == BAD_ARG, case


def test_null_descriptor_misaligned_pointers_and_too_many_tiles():
    assert _ffi.lib().cwn_gin_layer_f32(None, None) == BAD_ARG
    for field in ('x', 'rowptr', 'col', 'eps_dev', 'W1', 'b1', 'scale1', 'shift1', 'W2', 'b2', 'scale2', 'shift2', 'out'):
        assert _call(_desc(**{field: 40 * P + 2})) == ALIGN, field
    assert _call(_desc(w=0, x=P + 2)) == BAD_ARG           # the argument checks come first
    assert _call(_desc(n=_ffi.GIN_TM * (2 ** 31 - 1), x=0x10, out=0x7f0000000000)) == TOO_LARGE


def test_empty_launches_and_legal_shapes_are_ok_without_a_device():
    """n == 0 returns before the first HIP call, with or without buffers; absent operands are legal shapes."""
    assert _call(_desc(n=0)) == OK
    assert _call(_desc(n=0, x=None, out=None, W1=None, W2=None)) == OK
    assert _call(_desc(n=0, rowptr=None, col=None, eps_dev=None, b1=None, scale1=None, shift1=None, b2=None, scale2=None,
                       shift2=None)) == OK
    # two column slices of one buffer that do not overlap pass the alias check (n = 0: nothing is launched)
    assert _call(_desc(n=0, ldx=32, ldout=32, out=P + 4 * 8)) == OK


def test_op_refuses_cpu_tensors_other_dtypes_and_recording_autograd():
    x = torch.randn(4, 3)
    st = [(torch.randn(5, 3), None, None, None), (torch.randn(5, 5), None, None, None)]
    assert ops.gin_layer_applies(x, st) is False
    with pytest.raises(TypeError, match='float32 tensor on the GPU'):
        ops.gin_layer(x, None, None, st, 'relu')
    with pytest.raises(TypeError, match='float64'):
        ops.gin_layer(x.double(), None, None, st, 'relu')


# ---- the models' structure -----------------------------------------------------------------------------------------------------
def _conv_keys(prefix, k_in, H, norm=True):
    """The state of one GINConv over Linear(k_in, H), BN(H), act, Linear(H, H), BN(H), act: torch_geometric's `eps`, the
    Sequential's entries 0, 1, 3, 4 (2 and 5 are the activations)."""
    keys = {f'{prefix}.eps': (1,)}
    for lin, bn, k in ((0, 1, k_in), (3, 4, H)):
        keys[f'{prefix}.nn.{lin}.weight'], keys[f'{prefix}.nn.{lin}.bias'] = (H, k), (H,)
        if norm:
            keys.update({f'{prefix}.nn.{bn}.weight': (H,), f'{prefix}.nn.{bn}.bias': (H,), f'{prefix}.nn.{bn}.running_mean': (H,),
                         f'{prefix}.nn.{bn}.running_var': (H,), f'{prefix}.nn.{bn}.num_batches_tracked': ()})
    return keys


F_IN, LAYERS, HID, CLASSES = 5, 3, 16, 4


def _expected(name, mode=None, norm=True):
    keys = _conv_keys('conv1', F_IN, HID, norm)
    for i in range(LAYERS - 1):
        keys.update(_conv_keys(f'convs.{i}', HID, HID, norm))
    if name == 'RingGIN':
        keys.update({'init_linear.weight': (F_IN, F_IN), 'init_linear.bias': (F_IN,), 'lin1.weight': (CLASSES, HID),
                     'lin1.bias': (CLASSES,)})
    else:
        keys.update({'lin1.weight': (HID, LAYERS * HID if mode == 'cat' else HID), 'lin1.bias': (HID,),
                     'lin2.weight': (CLASSES, HID), 'lin2.bias': (CLASSES,)})
    return keys


MODELS = [('GIN0', None), ('GIN', None), ('GIN0WithJK', 'cat'), ('GIN0WithJK', 'max'), ('GINWithJK', 'cat'), ('GINWithJK', 'max'),
          ('RingGIN', None)]


def _make(name, mode=None, **kw):
    cls = getattr(models, name)
    if mode is not None:
        kw['mode'] = mode
    return cls(F_IN, LAYERS, HID, CLASSES, **kw)


@pytest.mark.parametrize('name,mode', MODELS)
def test_state_dict_keys_and_shapes_are_the_references(name, mode):
    m = _make(name, mode)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == _expected(name, mode)
    trained = name in ('GIN', 'GINWithJK')
    for conv in [m.conv1] + list(m.convs):
        assert isinstance(conv, layers.GINConv) and tuple(conv.eps.shape) == (1,) and conv.initial_eps == 0.
        assert isinstance(conv.eps, torch.nn.Parameter) is trained
        assert ('eps' in dict(conv.named_parameters())) is trained and ('eps' in dict(conv.named_buffers())) is not trained
    assert repr(m) == name
    m.reset_parameters()
    if mode is not None:
        assert isinstance(m.jump, models.JumpingKnowledge) and not list(m.jump.parameters())


def test_constructor_signatures_are_the_references():
    import inspect
    plain = ['self', 'num_features', 'num_layers', 'hidden', 'num_classes', 'readout', 'dropout_rate', 'nonlinearity']
    jk = plain[:5] + ['mode'] + plain[5:]
    for name, want in (('GIN0', plain), ('GIN', plain), ('GIN0WithJK', jk), ('GINWithJK', jk),
                       ('RingGIN', ['self', 'num_features', 'num_layers', 'hidden', 'num_classes', 'nonlinearity', 'graph_norm'])):
        assert list(inspect.signature(getattr(models, name).__init__).parameters) == want, name
    assert list(inspect.signature(layers.GINConv.__init__).parameters) == ['self', 'nn', 'eps', 'train_eps']
    assert models.RingGIN(5, 2, 8, 5, graph_norm='id').state_dict().keys() == _expected_ring_id().keys()


def _expected_ring_id():
    keys = _conv_keys('conv1', 5, 8, norm=False)
    keys.update(_conv_keys('convs.0', 8, 8, norm=False))
    keys.update({'init_linear.weight': 0, 'init_linear.bias': 0, 'lin1.weight': 0, 'lin1.bias': 0})
    return keys


def test_gin_conv_state_and_reset():
    for trained in (False, True):
        conv = layers.GINConv(torch.nn.Sequential(torch.nn.Linear(3, 4)), eps=0.25, train_eps=trained)
        assert torch.equal(conv.state_dict()['eps'], torch.tensor([0.25]))
        with torch.no_grad():
            conv.eps.fill_(2.0)
        w = conv.nn[0].weight.clone()
        conv.reset_parameters()
        assert float(conv.eps.detach()) == 0.25 and not torch.equal(conv.nn[0].weight, w)


def test_jumping_knowledge_lstm_is_not_implemented():
    for name in ('GIN0WithJK', 'GINWithJK'):
        with pytest.raises(NotImplementedError):
            _make(name, 'lstm')
    with pytest.raises(NotImplementedError):
        models.JumpingKnowledge('lstm')


# ---- the models on the CPU against the float64 restatement -------------------------------------------------------------------------
def _ring_batch(nodes=10, samples=10):
    return ComplexBatch.from_complex_list(synthetic.ring_transfer(nodes, samples), max_dim=2)


def _namespace(batch):
    v = batch.nodes
    return SimpleNamespace(x=v.x.clone(), edge_index=v.upper_index.clone(), batch=v.batch.clone(), mask=v.mask.clone())


_RING = {}


def _ring(nodes=10, samples=10):
    """(collated batch, the same graph as a plain namespace), built once."""
    if (nodes, samples) not in _RING:
        b = _ring_batch(nodes, samples)
        _RING[(nodes, samples)] = (b, _namespace(b))
    return _RING[(nodes, samples)]


def reference64(name, mode, model, ns, act, readout='sum'):
    st = _gin.state64(model)
    if name == 'RingGIN':
        return _gin.ring_gin64(st, ns.x, ns.edge_index, ns.mask, act)
    return _gin.gin_model64(st, ns.x, ns.edge_index, ns.batch, int(ns.batch.max()) + 1, act, readout, mode)


@pytest.mark.parametrize('name,mode', MODELS)
def test_models_on_the_cpu_against_the_float64_restatement(name, mode):
    """ring_transfer(10, 10) collated, and a SimpleNamespace carrying the same graph: eval() inside the gate of the restatement."""
    torch.manual_seed(11)
    act = 'tanh' if name == 'RingGIN' else 'relu'
    kw = dict(nonlinearity=act) if name == 'RingGIN' else dict(nonlinearity=act, readout='mean' if mode == 'max' else 'sum')
    model = _gin.randomise(_make(name, mode, **kw), 3).eval()
    batch, ns = _ring()
    ref = reference64(name, mode, model, ns, act, kw.get('readout', 'sum'))
    assert float(ref.abs().max()) > 1e-3
    with torch.no_grad():
        for data in (batch, ns):
            x0 = ns.x.clone()
            out = model(data)
            gate(out, ref, f'{name}[{mode}] on {type(data).__name__}')
            assert torch.equal(ns.x, x0) and torch.equal(batch.nodes.x, x0)       # the inputs are left alone
    for conv in [model.conv1] + list(model.convs):
        assert conv.last_route == 'generic'


def test_a_graph_without_edges_and_a_single_complex():
    torch.manual_seed(2)
    model = _gin.randomise(models.GIN(5, 2, 8, 3), 1).eval()
    one = synthetic.ring_transfer(6, 5)[2]
    v = one.nodes
    with torch.no_grad():
        gate(model(one), _gin.gin_model64(_gin.state64(model), v.x, v.upper_index, torch.zeros(6, dtype=torch.long), 1), 'one complex')
        ns = SimpleNamespace(x=v.x, edge_index=None, batch=torch.zeros(6, dtype=torch.long))
        gate(model(ns), _gin.gin_model64(_gin.state64(model), v.x, None, ns.batch, 1), 'no edges')


# ---- the receptive field ------------------------------------------------------------------------------------------------------------
def receptive_field(device, fused=None, batched=False):
    """RingGIN(5 features, L layers, hidden 16, 5 classes, tanh).eval() on ring_transfer(10, 5): the five complexes differ at the
    source vertex alone, 5 hops from the target.  -> {L: predictions [5, 5]} for L = 4, 5.

    batched=False runs the five complexes one at a time: the five forwards then have identical shapes and the target is the same
    row in each, so `torch.equal` below does not lean on a BLAS giving a row the same bits wherever it stands in a matrix (torch's
    CPU GEMM does not promise that, and on one host it did not deliver it: the collated batch differed in the last bit there).
    batched=True collates the five into one batch: for routes that do promise it (the fused launch: an output row is a function
    of its own row's entries and the weights alone, include/cwn_hip.h)."""
    out = {}
    for L in (4, 5):
        torch.manual_seed(20 + L)
        model = _gin.randomise(models.RingGIN(num_features=5, num_layers=L, hidden=16, num_classes=5, nonlinearity='tanh'), L)
        model = model.to(device).eval()
        ring = synthetic.ring_transfer(10, 5)
        groups = [ring] if batched else [[c] for c in ring]
        with torch.no_grad():
            out[L] = torch.cat([model(ComplexBatch.from_complex_list(g, max_dim=2).to(device)) for g in groups])
        assert all(c.last_route == (fused or 'generic') for c in [model.conv1] + list(model.convs))
    return out


def check_receptive_field(out):
    four, five = out[4], out[5]
    assert tuple(four.shape) == tuple(five.shape) == (5, 5)
    for i in range(1, 5):
        assert torch.equal(four[i], four[0]), 'four layers cannot see a source five hops away'
    spread = float((five - five[0]).abs().max())
    assert spread > 1e-5 * max(1.0, float(five.abs().max())), spread


def test_receptive_field_on_the_cpu():
    check_receptive_field(receptive_field(torch.device('cpu')))


def test_routing_on_cpu_tensors_is_generic():
    conv = layers.GINConv(torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Identity(), torch.nn.ReLU(),
                                              torch.nn.Linear(4, 4), torch.nn.Identity(), torch.nn.ReLU())).eval()
    x = torch.randn(6, 3)
    idx = torch.tensor([[0, 1, 2, 5], [1, 0, 1, 1]])
    assert conv.last_route is None
    for on in (True, False):
        old, layers.FUSED_GIN = layers.FUSED_GIN, on
        try:
            with torch.no_grad():
                assert conv.fused_stages(x) is None
                y = conv(x, idx)
        finally:
            layers.FUSED_GIN = old
        assert conv.last_route == 'generic'
        st = [(conv.nn[0].weight, conv.nn[0].bias, None, None), (conv.nn[3].weight, conv.nn[3].bias, None, None)]
        gate(y, _gin.gin_formula64(x, idx, 0.0, st, 'relu'), 'GINConv on the CPU')
    assert layers.FUSED_GIN_DEFAULT in (True, False) and isinstance(layers.FUSED_GIN, bool)
