"""Host-side checks of the message-passing-agnostic baseline (csrc/cwn_agnostic.hip) and of what rides on it -- no GPU needed:
the four entry points in the header, the library and the binding at ABI 24, the descriptors' layouts, every argument check of
the two launchers (they all precede the first HIP call), the MessagePassingAgnostic mirror's state_dict against the
reference-made fixture (tests/golden/mp_agnostic.npz, tools/gen_golden_agnostic.py) and its CPU forward in both dtypes."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from cwn_amd import _ffi, models, ops
from cwn_amd.models import MessagePassingAgnostic
from tests._golden import load, T, state_dict
from tests._product import dummy_batch, gate
from tests._agnostic import CASES, CONFIGS, DTYPES, TOL, case_batch, fixture_model, G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, TOO_LARGE, ALIGN = 0, 1, 2, 5
POOL = ('cwn_embed_pool_f32', 'cwn_embed_pool_f64')
HEAD = ('cwn_agnostic_head_f32', 'cwn_agnostic_head_f64')
P0 = 0x10000


def test_symbols_are_declared_exported_and_bound_at_abi_24():
    header = open(os.path.join(ROOT, 'include', 'cwn_hip.h')).read()
    lib = _ffi.lib()
    for name in POOL + HEAD:
        assert re.search(rf'\bint {name}\s*\(', header), name
        assert name in _ffi.EXPORTS
        assert hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    assert lib.cwn_abi_version() == _ffi.ABI_VERSION == 24
    assert int(re.search(r'#define CWN_ABI_VERSION (\d+)', header).group(1)) == 24
    for macro, value in (('CWN_EMBED_POOL_MAX_K', _ffi.EMBED_POOL_MAX_K), ('CWN_AGNOSTIC_MAX_WIDTH', _ffi.AGNOSTIC_MAX_WIDTH),
                         ('CWN_EMBED_POOL_CHUNK', _ffi.EMBED_POOL_CHUNK), ('CWN_MAX_DESCS', _ffi.MAX_DESCS)):
        assert int(re.search(rf'#define {macro} (\d+)', header).group(1)) == value, macro
    assert (_ffi.EMBED_POOL_MAX_K, _ffi.AGNOSTIC_MAX_WIDTH) == (128, 1024)
    # row counts are host counts, and the header says so
    section = header[header.index('The message-passing-agnostic baseline'):header.index('int cwn_agnostic_head_f64')]
    assert 'NO m_dev' in section and 'no static batch reaches this launch' in section
    assert 'm_dev' not in [f for f, _ in _ffi.EmbedPoolDesc._fields_ + _ffi.AgnosticHeadDesc._fields_]


@pytest.mark.parametrize('ctype,struct', [('cwn_embed_pool_desc', 'EmbedPoolDesc'), ('cwn_embed_pool_desc_f64', 'EmbedPoolDescF64'),
                                          ('cwn_agnostic_head_desc', 'AgnosticHeadDesc'),
                                          ('cwn_agnostic_head_desc_f64', 'AgnosticHeadDescF64')])
def test_descriptor_layout_matches_the_header(tmp_path, ctype, struct):
    """Field by field against the ctypes mirror, through a probe compiled with the host C compiler."""
    st = getattr(_ffi, struct)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cwn_hip.h"', 'int main(void) {',
             f'printf("size %zu\\n", sizeof({ctype}));']
    lines += [f'printf("{f} %zu\\n", offsetof({ctype}, {f}));' for f, _ in st._fields_]
    lines += ['return 0; }']
    src, exe = tmp_path / 'probe.c', tmp_path / 'probe'
    src.write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got['size']) == C.sizeof(st)
    for f, _ in st._fields_:
        assert int(got[f]) == getattr(st, f).offset, f


def _pool(**kw):
    """A descriptor that passes every check (made-up, aligned addresses: a call that passed the checks would launch, so every
    test below breaks exactly one thing -- or sets C = 0, which launches nothing)."""
    d = dict(x=P0, cell_ptr=2 * P0, W=3 * P0, bias=4 * P0, out=5 * P0, N=10, C=3, ldx=8, ldw=8, ldo=32, K=8, H=32, act=2, mean=0)
    d.update(kw)
    return _ffi.EmbedPoolDesc(**d)


def _call_pool(name, descs, n=None):
    arr = (_ffi.EmbedPoolDesc * max(len(descs), 1))(*descs)
    return getattr(_ffi.lib(), name)(arr, len(descs) if n is None else n, None)


POOL_BAD = {
    'K=0': dict(K=0), 'K=129': dict(K=129, ldx=129, ldw=129), 'H=0': dict(H=0), 'H=1025': dict(H=1025, ldo=1025),
    'ldx<K': dict(ldx=7), 'ldw<K': dict(ldw=7), 'ldo<H': dict(ldo=31), 'act=-1': dict(act=-1), 'act=5': dict(act=5),
    'mean=2': dict(mean=2), 'N<0': dict(N=-1), 'C<0': dict(C=-1), 'x NULL': dict(x=None), 'W NULL': dict(W=None),
    'cell_ptr NULL': dict(cell_ptr=None), 'out NULL': dict(out=None),
}


@pytest.mark.parametrize('name', POOL)
@pytest.mark.parametrize('case', sorted(POOL_BAD))
def test_embed_pool_bad_arguments_are_refused_before_any_hip_call(name, case):
    assert _call_pool(name, [_pool(**POOL_BAD[case])]) == BAD_ARG, case
    # ... wherever the bad descriptor stands among good ones that would not launch anything themselves
    assert _call_pool(name, [_pool(C=0), _pool(**POOL_BAD[case])]) == BAD_ARG, case


@pytest.mark.parametrize('name', POOL)
def test_embed_pool_counts_sizes_and_alignment(name):
    fn = getattr(_ffi.lib(), name)
    assert fn(None, 0, None) == OK                                       # n = 0 is legal, with or without an array
    assert _call_pool(name, [_pool()], n=0) == OK
    assert fn(None, 1, None) == BAD_ARG
    assert _call_pool(name, [_pool()], n=-1) == BAD_ARG
    assert _call_pool(name, [_pool(C=0)] * 9) == BAD_ARG                 # n > CWN_MAX_DESCS
    assert _call_pool(name, [_pool(C=0)] * 8) == OK                      # eight descriptors without a complex launch nothing
    assert _call_pool(name, [_pool(C=0, K=128, ldx=128, ldw=128, H=1024, ldo=1024)]) == OK     # the limits themselves
    assert _call_pool(name, [_pool(C=0, N=0, x=None, W=None, bias=None, cell_ptr=None, out=None)]) == OK
    assert _call_pool(name, [_pool(C=0, bias=None)]) == OK
    assert _call_pool(name, [_pool(C=2 ** 31 - 1)]) == TOO_LARGE
    assert _call_pool(name, [_pool(N=2 ** 40)]) == TOO_LARGE
    assert _call_pool(name, [_pool(C=2 ** 27, H=1024, ldo=1024)]) == TOO_LARGE     # the grid: C x 16 column blocks
    elem = 4 if name.endswith('f32') else 8
    for field in ('x', 'W', 'bias', 'out'):
        assert _call_pool(name, [_pool(C=0, **{field: 20 * P0 + elem // 2})]) == ALIGN, field
    assert _call_pool(name, [_pool(C=0, cell_ptr=20 * P0 + 4)]) == ALIGN
    # the argument checks come first: a bad activation wins over a misaligned pointer
    assert _call_pool(name, [_pool(act=7, out=P0 + 1)]) == BAD_ARG


def _head(**kw):
    d = dict(W1=2 * P0, b1=3 * P0, W2=4 * P0, b2=5 * P0, out=6 * P0, C=3, ldw1=32, ldw2=32, ldo=8, D=3, H=32, O=8, act=2)
    ps = kw.pop('P', [10 * P0, None, 12 * P0])
    ldp = kw.pop('ldp', [32] * len(ps))
    d.update(kw)
    D = _ffi.AgnosticHeadDesc(**d)
    for i, (p, ld) in enumerate(zip(ps, ldp)):
        D.P[i], D.ldp[i] = p, ld
    return D


def _call_head(name, D):
    return getattr(_ffi.lib(), name)(C.byref(D), None)


HEAD_BAD = {
    'D=0': dict(D=0), 'D=9': dict(D=9), 'H=0': dict(H=0), 'H=1025': dict(H=1025, ldw1=1025, ldw2=1025, ldp=[1025] * 3),
    'O=0': dict(O=0), 'O=1025': dict(O=1025, ldo=1025), 'act=-1': dict(act=-1), 'act=5': dict(act=5), 'C<0': dict(C=-1),
    'ldw1<H': dict(ldw1=31), 'ldw2<H': dict(ldw2=31), 'ldo<O': dict(ldo=7), 'ldp<H': dict(ldp=[32, 32, 31]),
    'W1 NULL': dict(W1=None), 'W2 NULL': dict(W2=None), 'out NULL': dict(out=None),
}


@pytest.mark.parametrize('name', HEAD)
@pytest.mark.parametrize('case', sorted(HEAD_BAD))
def test_head_bad_arguments_are_refused_before_any_hip_call(name, case):
    assert _call_head(name, _head(**HEAD_BAD[case])) == BAD_ARG, case


@pytest.mark.parametrize('name', HEAD)
def test_head_counts_sizes_and_alignment(name):
    assert getattr(_ffi.lib(), name)(None, None) == BAD_ARG
    assert _call_head(name, _head(C=0)) == OK                            # no complex: nothing is launched
    assert _call_head(name, _head(C=0, D=8, P=[None] * 8)) == OK         # every dimension absent, the most dimensions
    assert _call_head(name, _head(C=0, H=1024, O=1024, ldw1=1024, ldw2=1024, ldo=1024, ldp=[1024] * 3)) == OK
    assert _call_head(name, _head(C=0, b1=None, b2=None)) == OK
    assert _call_head(name, _head(C=0, ldp=[32, 0, 32])) == OK           # the stride of a NULL matrix is not looked at
    assert _call_head(name, _head(C=2 ** 31 - 1)) == TOO_LARGE
    assert _call_head(name, _head(C=2 ** 40)) == TOO_LARGE
    elem = 4 if name.endswith('f32') else 8
    for field in ('W1', 'b1', 'W2', 'b2', 'out'):
        assert _call_head(name, _head(C=0, **{field: 20 * P0 + elem // 2})) == ALIGN, field
    assert _call_head(name, _head(C=0, P=[10 * P0, None, 12 * P0 + elem // 2])) == ALIGN
    assert _call_head(name, _head(act=7, out=P0 + 1)) == BAD_ARG


def test_ops_refuse_other_dtypes_and_devices_by_name():
    """The dtype rule is checked before the device: reachable without a GPU."""
    x, w, b = torch.zeros(4, 3), torch.zeros(8, 3), torch.zeros(8)
    ptr = torch.tensor([0, 4])
    for bad in (torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match=str(bad)):
            ops.embed_pool([x.to(bad)], [ptr], 1, [w.to(bad)], [b.to(bad)], 'elu')
        with pytest.raises(TypeError, match=str(bad)):
            ops.agnostic_head([torch.zeros(1, 8, dtype=bad)], torch.zeros(8, 8, dtype=bad), None, torch.zeros(2, 8, dtype=bad), None, 'elu')
    with pytest.raises(TypeError, match='torch.float64'):
        ops.embed_pool([x], [ptr], 1, [w.double()], [b], 'elu')
    with pytest.raises(TypeError, match='torch.float64'):
        ops.agnostic_head([torch.zeros(1, 8)], torch.zeros(8, 8), None, torch.zeros(2, 8).double(), None, 'elu')
    with pytest.raises(TypeError, match='on the GPU'):
        ops.embed_pool([x], [ptr], 1, [w], [b], 'elu')


def test_switch():
    env = os.environ.get('CWN_FUSED_AGNOSTIC')
    assert models.FUSED_AGNOSTIC == {'0': False, '1': True}.get(env, models.FUSED_AGNOSTIC_DEFAULT)
    assert models.FUSED_AGNOSTIC_DEFAULT <= {torch.float32, torch.float64}


def test_mirror_has_the_reference_state_dict():
    g = load(G)
    state = state_dict(g, 'state')
    model = MessagePassingAgnostic(1, 8, 32, dropout_rate=0.5, max_dim=2, nonlinearity='elu', readout='sum')
    mine = model.state_dict()
    assert sorted(mine) == [str(k) for k in g['state_keys']] == sorted(state)
    assert sorted(mine) == sorted([f'lin0s.{d}.{p}' for d in range(3) for p in ('weight', 'bias')]
                                  + [f'{l}.{p}' for l in ('lin1', 'lin2') for p in ('weight', 'bias')])
    for k, v in mine.items():
        assert tuple(v.shape) == tuple(state[k].shape), k
    model.double().load_state_dict(state)                               # strict
    assert repr(model) == 'MessagePassingAgnostic'
    assert (model.max_dim, model.dropout_rate, model.readout_type) == (2, 0.5, 'sum') and model.act is torch.nn.functional.elu
    before = model.lin1.weight.detach().clone()
    model.reset_parameters()
    assert not torch.equal(before, model.lin1.weight)
    with pytest.raises(NotImplementedError):
        MessagePassingAgnostic(1, 8, 32, nonlinearity='gelu')


@pytest.mark.parametrize('case', CASES)
def test_case_batches_are_the_fixtures(case):
    """The product-side batch of every case has the rows the reference's collate produced."""
    g = load(G)
    b = case_batch(case, torch.float64)
    assert b.dimension == int(g[f'{case}/dimension'])
    for d in range(b.dimension + 1):
        assert np.array_equal(b.cochains[d].x.numpy(), g[f'{case}/batch/{d}/x']), d
        assert np.array_equal(b.cochains[d].batch.numpy(), g[f'{case}/batch/{d}/batch']), d
    if case == 'dummy_no2':
        assert b.dimension == 1                                         # one dimension fewer than the model has
    if case == 'dummy_mixed':
        two = set(b.cochains[2].batch.tolist())
        assert two and two < set(range(b.num_complexes))                # some complexes have 2-cells, some have none


@pytest.mark.parametrize('tag', sorted(DTYPES))
@pytest.mark.parametrize('case', CASES)
def test_cpu_forward_reproduces_the_fixture(case, tag):
    """Pooled rows (the input of lin1) and logits on the CPU, in both dtypes, every configuration."""
    g = load(G)
    dtype = DTYPES[tag]
    for act, readout in CONFIGS:
        model = fixture_model(act, readout, dtype)
        seen = []
        hook = model.lin1.register_forward_hook(lambda mod, inp, res: seen.append(inp[0]))
        with torch.no_grad():
            out = model(case_batch(case, dtype))
        hook.remove()
        assert model.last_route == 'torch' and out.dtype == dtype
        key = f'{case}/{act}/{readout}/{tag}'
        gate(seen[0], T(g[f'{key}/pooled']), f'{key}: pooled rows', tol=TOL[dtype])
        gate(out, T(g[f'{key}/out']), f'{key}: logits', tol=TOL[dtype])


def test_cpu_training_path_is_differentiable():
    model = fixture_model('elu', 'mean', torch.float64).train()
    torch.manual_seed(0)
    out = model(case_batch('dummy_mixed', torch.float64))
    out.square().sum().backward()
    assert model.last_route == 'torch'
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    with pytest.raises(NotImplementedError):
        MessagePassingAgnostic(1, 8, 32, readout='max')(dummy_batch(['house', 'kite']))


def test_generator_check_passes():
    """tools/gen_golden_agnostic.py --check: the committed fixture regenerates bit for bit from the reference (where the
    reference tree is present: it is read on the machine that writes fixtures, never on the GPU box)."""
    ref = re.search(r"^REF = '([^']+)'", open(os.path.join(ROOT, 'oracle', 'gen_golden.py')).read(), re.M).group(1)
    if not os.path.isdir(ref):
        pytest.skip('the reference tree is not on this machine')
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_golden_agnostic.py'), '--check'], capture_output=True,
                         text=True, cwd=ROOT)
    assert run.returncode == 0, run.stdout + run.stderr
    assert 'regenerate bit-exactly' in run.stdout
