"""Host-side checks of the activated coboundary message (csrc/cwn_aggregate_act.hip) and of what rides on it -- no GPU
needed: the two entry points in the header, the library and the binding at ABI 24, the descriptor's layout, every argument
check of the launcher (they all precede the first HIP call), Stream(act=...)'s own rules, and which message networks
SparseCINCochainConv._up_kind() sends that way."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from cwn_amd import _ffi, layers, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, TOO_LARGE, ALIGN = 0, 1, 2, 5
NAMES = ('cwn_aggregate_act_f32', 'cwn_aggregate_act_f64')


def test_symbols_are_declared_exported_and_bound_at_abi_24():
    header = open(os.path.join(ROOT, 'include', 'cwn_hip.h')).read()
    lib = _ffi.lib()
    for name in NAMES:
        assert re.search(rf'\bint {name}\s*\(', header), name
        assert name in _ffi.EXPORTS
        assert hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    assert lib.cwn_abi_version() == _ffi.ABI_VERSION == 24
    assert int(re.search(r'#define CWN_ABI_VERSION (\d+)', header).group(1)) == 24
    assert ops.ACT_CODES == {'id': 0, 'relu': 1, 'elu': 2, 'tanh': 3, 'sigmoid': 4}
    # no new message code and no new field of the shared descriptor
    assert re.search(r'CWN_MSG_A_TIMES_2RELU = 6 \};', header)
    assert [f for f, _ in _ffi.AggDesc._fields_][-3:] == ['self_x2', 'eps2', 'm_dev'] and len(_ffi.AggDesc._fields_) == 21


@pytest.mark.parametrize('ctype,struct', [('cwn_agg_act_desc', 'AggActDesc'), ('cwn_agg_act_desc_f64', 'AggActDescF64')])
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
    assert 'm_dev' not in got and 'msg_op' not in got and 'reduce' not in got and 'b_width' not in got


def _desc(**kw):
    """A descriptor that passes every check (made-up, aligned addresses: a call that passed the checks would launch, so
    every test below breaks exactly one thing)."""
    P = 0x10000
    d = dict(rowptr=P, ia=2 * P, ib=3 * P, A=4 * P, B=5 * P, self_x=6 * P, eps=7 * P, out=8 * P, long_rows=9 * P, n_long=10 * P,
             n_dst=10, F=8, act=2, long_cap=1, flags=1)
    d.update(kw)
    return _ffi.AggActDesc(**d)


def _call(name, descs, n=None):
    arr = (_ffi.AggActDesc * max(len(descs), 1))(*descs)
    return getattr(_ffi.lib(), name)(arr, len(descs) if n is None else n, None)


BAD = {
    'act=-1': dict(act=-1), 'act=5': dict(act=5), 'F=0': dict(F=0), 'F<0': dict(F=-3), 'n_dst<0': dict(n_dst=-1),
    'out NULL': dict(out=None), 'ia NULL': dict(ia=None), 'ib NULL': dict(ib=None), 'A NULL': dict(A=None), 'B NULL': dict(B=None),
}


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('case', sorted(BAD))
def test_bad_arguments_are_refused_before_any_hip_call(name, case):
    assert _call(name, [_desc(**BAD[case])]) == BAD_ARG, case
    # ... wherever the bad descriptor stands among good ones that would not launch anything themselves
    assert _call(name, [_desc(n_dst=0), _desc(**BAD[case])]) == BAD_ARG, case


@pytest.mark.parametrize('name', NAMES)
def test_counts_sizes_and_alignment(name):
    fn = getattr(_ffi.lib(), name)
    assert fn(None, 0, None) == OK                                       # n = 0 is legal, with or without an array
    assert _call(name, [_desc()], n=0) == OK
    assert fn(None, 1, None) == BAD_ARG
    assert _call(name, [_desc()], n=-1) == BAD_ARG
    assert _call(name, [_desc(n_dst=0)] * 9) == BAD_ARG                  # n > CWN_MAX_DESCS
    assert _call(name, [_desc(n_dst=0)] * 8) == OK                       # eight empty descriptors launch nothing
    assert _call(name, [_desc(n_dst=0, out=None, rowptr=None, ia=None, ib=None, A=None, B=None, self_x=None, eps=None)]) == OK
    assert _call(name, [_desc(n_dst=2 ** 31 - 1)]) == TOO_LARGE
    assert _call(name, [_desc(n_dst=2 ** 40)]) == TOO_LARGE
    elem = 4 if name.endswith('f32') else 8
    for field in ('A', 'B', 'self_x', 'out', 'eps'):
        assert _call(name, [_desc(**{field: 0x10000 * 20 + elem // 2})]) == ALIGN, field
    # an absent adjacency does not look at the gathered operands
    assert _call(name, [_desc(n_dst=0, rowptr=None, A=0x30001, B=0x30003, ia=None, ib=None)]) == OK
    # the argument checks come first: a bad activation wins over a misaligned pointer
    assert _call(name, [_desc(act=7, out=0x10001)]) == BAD_ARG


class _Adj:
    """What Stream.validate reads of an Adjacency."""
    n_val, n_aux, n_entries, n_dst, aux = 5, 4, 6, 3, object()


def _stream(**kw):
    d = dict(adj=_Adj(), n_dst=3, width=4, A=torch.zeros(5, 4), B=torch.zeros(4, 4), msg_op=ops.MSG_A_PLUS_B, act='elu')
    d.update(kw)
    return ops.Stream(**d)


def test_stream_act_rules(monkeypatch):
    monkeypatch.setattr(_ffi, 'require_gpu', lambda t, name: None)          # the rules, not the device check
    assert ops.Stream(adj=None, n_dst=3, width=4).act is None
    _stream().validate()
    _stream(act=_ffi.ACT_TANH).validate()
    _stream(B=torch.zeros(6, 4), ib_mode='perm').validate()
    for bad in (dict(msg_op=ops.MSG_RELU_A_PLUS_B), dict(msg_op=ops.MSG_A, B=None), dict(msg_op=ops.MSG_A_TIMES_B),
                dict(reduce='mean'), dict(reduce='max'), dict(B=torch.zeros(4, 1)), dict(B=None),
                dict(act='gelu'), dict(act=5)):
        with pytest.raises(ValueError):
            _stream(**bad).validate()
    with pytest.raises(TypeError):
        _stream(A=torch.zeros(5, 4, dtype=torch.bfloat16), B=torch.zeros(4, 4, dtype=torch.bfloat16)).validate()
    with pytest.raises(TypeError):
        _stream(A=torch.zeros(5, 4, dtype=torch.float16), B=torch.zeros(4, 4, dtype=torch.float16)).validate()
    # the scalar attribute stays legal where there is no activation
    _stream(act=None, B=torch.zeros(4, 1)).validate()


def _level(act_module, **kw):
    H = 4
    msg = torch.nn.Sequential(layers.Catter(), torch.nn.Linear(2 * H, H), act_module)
    conv = layers.SparseCINConv(H, H, H, None, None, None, None, hidden=H, layer_dim=H, act_module=torch.nn.ReLU,
                                use_coboundaries=True, max_dim=0, **kw)
    lvl = conv.mp_levels[0]
    lvl.msg_up_nn = msg
    return lvl


def test_up_kind(monkeypatch):
    env = os.environ.get('CWN_FUSED_ACT_MESSAGE')
    assert layers.FUSED_ACT_MESSAGE == {'0': False, '1': True}.get(env, layers.FUSED_ACT_MESSAGE_DEFAULT)
    assert layers.FUSED_ACT_MESSAGE_DEFAULT <= {torch.float32, torch.float64}
    # per dtype: a set of dtypes turns the route on for those alone
    with torch.no_grad():
        monkeypatch.setattr(layers, 'FUSED_ACT_MESSAGE', {torch.float64})
        assert _level(torch.nn.ELU())._up_kind() == 'custom'
        assert _level(torch.nn.ELU()).double()._up_kind() == 'cat_linear_act'
        monkeypatch.setattr(layers, 'FUSED_ACT_MESSAGE', frozenset())
        assert _level(torch.nn.ELU()).double()._up_kind() == 'custom'
    monkeypatch.setattr(layers, 'FUSED_ACT_MESSAGE', True)
    acts = [torch.nn.ELU(), torch.nn.Tanh(), torch.nn.Sigmoid(), torch.nn.Identity()]
    with torch.no_grad():
        for act in acts:
            assert _level(act)._up_kind() == 'cat_linear_act', act
        assert _level(torch.nn.ReLU())._up_kind() == 'cat_linear_relu'
        assert _level(torch.nn.ELU(alpha=0.5))._up_kind() == 'custom'            # the kernel's ELU has alpha = 1
        assert _level(torch.nn.GELU())._up_kind() == 'custom'
        lvl = _level(torch.nn.ELU())
        lvl.msg_up_nn = layers.FirstOf()
        assert lvl._up_kind() == 'first'
        with _ffi.dynamic_rows({7: 1234}):                                       # a static batch: no device-side row count here
            assert _level(torch.nn.ELU())._up_kind() == 'custom'
    # a recording autograd keeps the path it had
    assert torch.is_grad_enabled()
    for act in acts:
        assert _level(act)._up_kind() == 'custom'
    assert _level(torch.nn.ReLU())._up_kind() == 'cat_linear_relu'
    monkeypatch.setattr(layers, 'FUSED_ACT_MESSAGE', False)
    with torch.no_grad():
        for act in acts:
            assert _level(act)._up_kind() == 'custom'
        assert _level(torch.nn.ReLU())._up_kind() == 'cat_linear_relu'


def test_custom_networks_have_no_products_and_no_stream(monkeypatch):
    """gemm_specs() / _up_stream() of a level whose kind is 'custom' return [] / None: the caller's `is None` branches."""
    from cwn_amd.cell_mp import CochainMessagePassingParams
    monkeypatch.setattr(layers, 'FUSED_ACT_MESSAGE', False)
    lvl = _level(torch.nn.ELU())
    x = torch.zeros(3, 4)
    idx = torch.tensor([[0, 1], [1, 0]])
    with torch.no_grad():
        assert lvl.gemm_specs(CochainMessagePassingParams(x, idx, up_attr=torch.zeros(2, 4))) == []
        assert lvl._up_stream(None, x, torch.zeros(2, 4)) is None
        monkeypatch.setattr(layers, 'FUSED_ACT_MESSAGE', True)
        specs = lvl.gemm_specs(CochainMessagePassingParams(x, idx, up_attr=torch.zeros(2, 4)))
        assert len(specs) == 2 and specs[0].W is lvl.msg_up_nn[1].weight and specs[1].w_col0 == 4
    assert lvl.gemm_specs(CochainMessagePassingParams(x, idx, up_attr=torch.zeros(2, 4))) == []      # recording: as before
