"""Host-side checks of the activated message's backward (csrc/cwn_aggregate_act_bwd.hip) and of what rides on it -- no GPU
needed: the two entry points in the header, the library and the binding at ABI 24, the descriptor's layout, every argument
check of the launcher (they all precede the first HIP call), the switch's default, and which message networks
SparseCINCochainConv._up_kind() sends that way with the switch off and on."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

from cwn_amd import _ffi, layers, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, TOO_LARGE, ALIGN = 0, 1, 2, 5
NAMES = ('cwn_aggregate_act_bwd_f32', 'cwn_aggregate_act_bwd_f64')


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
    assert callable(_ffi.aggregate_act_bwd)
    # additive: the forward's descriptor is what it was
    assert [f for f, _ in _ffi.AggActDesc._fields_] == ['rowptr', 'ia', 'ib', 'A', 'B', 'self_x', 'eps', 'out', 'long_rows',
                                                         'n_long', 'n_dst', 'F', 'act', 'long_cap', 'flags']


@pytest.mark.parametrize('ctype,struct', [('cwn_agg_act_bwd_desc', 'AggActBwdDesc'), ('cwn_agg_act_bwd_desc_f64', 'AggActBwdDescF64')])
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
    assert [f for f, _ in st._fields_] == ['rowptr', 'ig', 'iq', 'g', 'P', 'Q', 'out', 'long_rows', 'n_long', 'n_dst', 'F', 'act',
                                           'long_cap', 'flags']
    # no self term, no device-side row count
    assert not {'m_dev', 'self_x', 'eps', 'msg_op', 'reduce'} & set(got)


def _desc(**kw):
    """A descriptor that passes every check (made-up, aligned addresses: a call that passed the checks would launch, so
    every test below breaks exactly one thing)."""
    P = 0x10000
    d = dict(rowptr=P, ig=2 * P, iq=3 * P, g=4 * P, P=5 * P, Q=6 * P, out=8 * P, long_rows=9 * P, n_long=10 * P,
             n_dst=10, F=8, act=2, long_cap=1, flags=1)
    d.update(kw)
    return _ffi.AggActBwdDesc(**d)


def _call(name, descs, n=None):
    arr = (_ffi.AggActBwdDesc * max(len(descs), 1))(*descs)
    return getattr(_ffi.lib(), name)(arr, len(descs) if n is None else n, None)


BAD = {
    'act=-1': dict(act=-1), 'act=5': dict(act=5), 'F=0': dict(F=0), 'F<0': dict(F=-3), 'n_dst<0': dict(n_dst=-1),
    'out NULL': dict(out=None), 'ig NULL': dict(ig=None), 'iq NULL': dict(iq=None), 'g NULL': dict(g=None), 'P NULL': dict(P=None),
    'Q NULL': dict(Q=None),
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
    assert _call(name, [_desc(n_dst=0, out=None, rowptr=None, ig=None, iq=None, g=None, P=None, Q=None)]) == OK
    assert _call(name, [_desc(n_dst=2 ** 31 - 1)]) == TOO_LARGE
    assert _call(name, [_desc(n_dst=2 ** 40)]) == TOO_LARGE
    elem = 4 if name.endswith('f32') else 8
    for field in ('g', 'P', 'Q', 'out'):
        assert _call(name, [_desc(**{field: 0x10000 * 20 + elem // 2})]) == ALIGN, field
    # an absent plan does not look at the operands
    assert _call(name, [_desc(n_dst=0, rowptr=None, g=0x30001, P=0x30003, Q=0x30005, ig=None, iq=None)]) == OK
    # the argument checks come first: a bad activation wins over a misaligned pointer
    assert _call(name, [_desc(act=7, out=0x10001)]) == BAD_ARG
    # ... and the codes are the forward's for the same faults
    fwd = getattr(_ffi.lib(), name.replace('_bwd', ''))
    assert fwd(None, 1, None) == BAD_ARG and fwd((_ffi.AggActDesc * 1)(_ffi.AggActDesc(n_dst=2 ** 31 - 1, F=8, out=64)), 1, None) == TOO_LARGE


def test_switch_default_follows_the_environment():
    assert ops.ACT_MESSAGE_BACKWARD is (os.environ.get('CWN_ACT_MESSAGE_BACKWARD') == '1')
    if 'CWN_ACT_MESSAGE_BACKWARD' not in os.environ:
        assert ops.ACT_MESSAGE_BACKWARD is False


def _level(act_module, **kw):
    H = 4
    msg = torch.nn.Sequential(layers.Catter(), torch.nn.Linear(2 * H, H), act_module)
    conv = layers.SparseCINConv(H, H, H, None, None, None, None, hidden=H, layer_dim=H, act_module=torch.nn.ReLU,
                                use_coboundaries=True, max_dim=0, **kw)
    lvl = conv.mp_levels[0]
    lvl.msg_up_nn = msg
    return lvl


ACT_MODULES = [torch.nn.ELU, torch.nn.Tanh, torch.nn.Sigmoid, torch.nn.Identity]


def test_up_kind_with_the_switch_off_is_todays_table(monkeypatch):
    monkeypatch.setattr(ops, 'ACT_MESSAGE_BACKWARD', False)
    monkeypatch.setattr(layers, 'FUSED_ACT_MESSAGE', True)
    assert torch.is_grad_enabled()
    for act in ACT_MODULES:
        assert _level(act())._up_kind() == 'custom', act                         # a recording autograd keeps the path it had
        with torch.no_grad():
            assert _level(act())._up_kind() == 'cat_linear_act', act
    assert _level(torch.nn.ReLU())._up_kind() == 'cat_linear_relu'
    with torch.no_grad():
        assert _level(torch.nn.ReLU())._up_kind() == 'cat_linear_relu'
        assert _level(torch.nn.ELU(alpha=0.5))._up_kind() == 'custom'
        assert _level(torch.nn.GELU())._up_kind() == 'custom'
        with _ffi.dynamic_rows({7: 1234}):
            assert _level(torch.nn.ELU())._up_kind() == 'custom'
        monkeypatch.setattr(layers, 'FUSED_ACT_MESSAGE', {torch.float64})
        assert _level(torch.nn.ELU())._up_kind() == 'custom'
        assert _level(torch.nn.ELU()).double()._up_kind() == 'cat_linear_act'
        monkeypatch.setattr(layers, 'FUSED_ACT_MESSAGE', False)
        assert _level(torch.nn.ELU()).double()._up_kind() == 'custom'
    lvl = _level(torch.nn.ELU())
    lvl.msg_up_nn = layers.FirstOf()
    assert lvl._up_kind() == 'first'


def test_up_kind_with_the_switch_on(monkeypatch):
    monkeypatch.setattr(ops, 'ACT_MESSAGE_BACKWARD', True)
    monkeypatch.setattr(layers, 'FUSED_ACT_MESSAGE', True)
    assert torch.is_grad_enabled()
    for act in ACT_MODULES:
        assert _level(act())._up_kind() == 'cat_linear_act', act                 # under a recording autograd too
        assert _level(act()).double()._up_kind() == 'cat_linear_act', act
        with torch.no_grad():
            assert _level(act())._up_kind() == 'cat_linear_act', act
    assert _level(torch.nn.ReLU())._up_kind() == 'cat_linear_relu'               # unchanged
    assert _level(torch.nn.ELU(alpha=0.5))._up_kind() == 'custom'                # the kernels' ELU has alpha = 1
    assert _level(torch.nn.GELU())._up_kind() == 'custom'
    with _ffi.dynamic_rows({7: 1234}):                                           # a static batch: no device-side row count
        assert _level(torch.nn.ELU())._up_kind() == 'custom'
    lvl = _level(torch.nn.ELU())
    lvl.msg_up_nn = layers.FirstOf()
    assert lvl._up_kind() == 'first'
    # FUSED_ACT_MESSAGE still decides per dtype
    monkeypatch.setattr(layers, 'FUSED_ACT_MESSAGE', {torch.float64})
    assert _level(torch.nn.ELU())._up_kind() == 'custom'
    assert _level(torch.nn.ELU()).double()._up_kind() == 'cat_linear_act'
    monkeypatch.setattr(layers, 'FUSED_ACT_MESSAGE', frozenset())
    assert _level(torch.nn.ELU()).double()._up_kind() == 'custom'
    monkeypatch.setattr(layers, 'FUSED_ACT_MESSAGE', False)
    assert _level(torch.nn.Tanh())._up_kind() == 'custom'


def test_products_under_a_recording_autograd_follow_the_switch(monkeypatch):
    """gemm_specs() of an ELU level under grad: [] with the switch off (as before), the two products with it on."""
    from cwn_amd.cell_mp import CochainMessagePassingParams
    monkeypatch.setattr(layers, 'FUSED_ACT_MESSAGE', True)
    lvl = _level(torch.nn.ELU())
    x, idx = torch.zeros(3, 4), torch.tensor([[0, 1], [1, 0]])
    monkeypatch.setattr(ops, 'ACT_MESSAGE_BACKWARD', False)
    assert lvl.gemm_specs(CochainMessagePassingParams(x, idx, up_attr=torch.zeros(2, 4))) == []
    monkeypatch.setattr(ops, 'ACT_MESSAGE_BACKWARD', True)
    specs = lvl.gemm_specs(CochainMessagePassingParams(x, idx, up_attr=torch.zeros(2, 4)))
    assert len(specs) == 2 and specs[0].W is lvl.msg_up_nn[1].weight and specs[1].w_col0 == 4
