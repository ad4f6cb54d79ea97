"""cwn_linear_wide_f32 without a GPU (csrc/cwn_linear_wide.hip behind ops.linear_wide and dense_ln.run): the symbol is declared,
exported and bound under ABI 24, the descriptor's ctypes layout is the header's, the launcher refuses every malformed
descriptor before anything is launched and takes empty launches without a device, ops.linear_wide names a wrong dtype or
device, and dense_ln.run hands the op exactly the two-branch combine products beyond the grouped GEMM's K."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest
import torch
from torch.nn import LayerNorm as LN, ReLU

from cwn_amd import _ffi, dense_ln, ops
from cwn_amd.layers import CINppConv, SparseCINConv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, ALIGN = 0, 1, 5
P = 0x100000


def test_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'cwn_hip.h')).read()
    lib = _ffi.lib()
    assert re.search(r'\bint cwn_linear_wide_f32\s*\(const cwn_linear_wide_desc\* descs_host, int n, cwn_stream_t stream\)', header)
    assert 'cwn_linear_wide_f32' in _ffi.EXPORTS and hasattr(lib, 'cwn_linear_wide_f32')
    assert lib.cwn_linear_wide_f32.argtypes[0]._type_ is _ffi.LinearWideDesc
    assert lib.cwn_abi_version() == _ffi.ABI_VERSION == 24
    assert int(re.search(r'#define CWN_ABI_VERSION (\d+)', header).group(1)) == 24
    assert int(re.search(r'#define CWN_LINEAR_WIDE_MAX_N (\d+)', header).group(1)) == _ffi.LINEAR_WIDE_MAX_N == 256
    assert int(re.search(r'#define CWN_LINEAR_WIDE_MAX_K (\d+)', header).group(1)) == _ffi.LINEAR_WIDE_MAX_K == 512
    section = header[header.index('A wide Linear product under a row count'):header.index('int cwn_linear_wide_f32')]
    for said in ('m_dev', 'w_trans', 'NaN', 'ascending', "row's bits", 'CWN_ERR_BAD_ARG', 'CWN_ERR_ALIGN', 'without a device'):
        assert said in section, said
    assert 'cwn_linear_wide.hip' in open(os.path.join(ROOT, 'cwn_amd', 'csrc', 'Makefile')).read()


def test_descriptor_layout_matches_the_header():
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cwn_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(cwn_linear_wide_desc));']
    for fname, _ in _ffi.LinearWideDesc._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(cwn_linear_wide_desc, {fname}));')
    lines.append('return 0; }')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, 'probe.c'), os.path.join(d, 'probe')
        open(src, 'w').write('\n'.join(lines))
        subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), src, '-o', exe], check=True)
        got = dict(l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got['size']) == ctypes.sizeof(_ffi.LinearWideDesc)
    for fname, _ in _ffi.LinearWideDesc._fields_:
        assert int(got[fname]) == getattr(_ffi.LinearWideDesc, fname).offset, fname
    # ... and no existing struct moved: the ABI stays at 24
    header = open(os.path.join(ROOT, 'include', 'cwn_hip.h')).read()
    assert header.count('typedef struct cwn_linear_wide_desc') == 1


def _desc(**kw):
    """A descriptor that passes every check (made-up, aligned addresses far apart: a call that passed the checks with rows
    would launch, so every case below breaks exactly one thing or has no rows)."""
    d = _ffi.LinearWideDesc(X=P, X2=2 * P, W=3 * P, bias=4 * P, Y=5 * P, m_dev=6 * P, M=70, ldx=161, ldx2=163, ldw=325, ldy=167,
                            N=160, K=160, K2=157, w_trans=0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(*ds, n=None):
    arr = (_ffi.LinearWideDesc * max(len(ds), 1))(*ds)
    return _ffi.lib().cwn_linear_wide_f32(arr if ds else None, len(ds) if n is None else n, None)


BAD = {
    'N = 0': dict(N=0),
    'N = 257': dict(N=257, ldy=257),
    'K = 0': dict(K=0),
    'K2 < 0': dict(K2=-1),
    'K + K2 = 513': dict(K=356, ldx=356, ldw=513),
    'X2 without K2': dict(K2=0),
    'K2 without X2': dict(X2=None),
    'M < 0': dict(M=-1),
    'ldx < K': dict(ldx=159),
    'ldx2 < K2': dict(ldx2=156),
    'ldw < K + K2': dict(ldw=316),
    'ldw < N, transposed': dict(w_trans=1, ldw=159),
    'ldy < N': dict(ldy=159),
    'X NULL with rows': dict(X=None),
    'W NULL with rows': dict(W=None),
    'Y NULL with rows': dict(Y=None),
}


@pytest.mark.parametrize('case', sorted(BAD))
def test_malformed_descriptors_are_refused_before_any_launch(case):
    assert _call(_desc(M=0)) == OK
    assert _call(_desc(**BAD[case])) == BAD_ARG, case
    assert _call(_desc(M=0), _desc(**BAD[case])) == BAD_ARG, case           # ... wherever it stands in the launch


def test_descriptor_counts_layouts_alignment_and_empty_launches():
    lib = _ffi.lib()
    assert _call(n=-1) == BAD_ARG
    assert _call(n=_ffi.MAX_DESCS + 1) == BAD_ARG
    assert lib.cwn_linear_wide_f32(None, 1, None) == BAD_ARG
    assert lib.cwn_linear_wide_f32(None, 0, None) == OK                    # nothing to do, no device touched
    assert _call(*[_desc(M=0) for _ in range(_ffi.MAX_DESCS)]) == OK
    assert _call(_desc(M=0, X=None, W=None, Y=None, bias=None, m_dev=None)) == OK     # (operands are required with rows only)
    assert _call(_desc(M=0, w_trans=1), _desc(M=0, w_trans=1)) == OK
    assert _call(_desc(M=0), _desc(M=0, w_trans=1)) == BAD_ARG             # one weight layout per launch
    for name in ('X', 'X2', 'W', 'bias', 'Y'):
        assert _call(_desc(M=0, **{name: getattr(_desc(), name) + 2})) == ALIGN, name
    assert _call(_desc(M=0, m_dev=6 * P + 4)) == ALIGN
    assert _call(_desc(M=0, X=P + 4, W=3 * P + 12)) == OK                  # 4 bytes is all a float pointer needs


F16, F32, F64 = torch.float16, torch.float32, torch.float64
_HINT = ': cwn_linear_wide_f32 computes in fp32 only (float64 products run on torch.nn.functional.linear)'
z = lambda *s, dtype=F32: torch.zeros(*s, dtype=dtype)
MESSAGES = {
    'X.float64': (lambda: ops.linear_wide(z(3, 4, dtype=F64), None, z(2, 4), None), 'linear_wide: X must be float32 (got torch.float64)' + _HINT),
    'X2.float16': (lambda: ops.linear_wide(z(3, 4), z(3, 4, dtype=F16), z(2, 8), None), 'linear_wide: X2 must be float32 (got torch.float16)' + _HINT),
    'weight.list': (lambda: ops.linear_wide(z(3, 4), None, [[0.0] * 4] * 2, None), 'linear_wide: weight must be float32 (got list)' + _HINT),
    'bias.float64': (lambda: ops.linear_wide(z(3, 4), None, z(2, 4), z(2, dtype=F64)), 'linear_wide: bias must be float32 (got torch.float64)' + _HINT),
    'X.cpu': (lambda: ops.linear_wide(z(3, 4), None, z(2, 4), None), 'linear_wide: X must be a float32 tensor on the GPU (got torch.float32 on cpu)'),
}


@pytest.mark.parametrize('case', sorted(MESSAGES))
def test_operand_checks_name_the_dtype_or_the_device(case):
    call, message = MESSAGES[case]
    with pytest.raises(TypeError) as got:
        call()
    assert str(got.value) == message


def test_limits_of_the_op_are_the_entry_points():
    assert ops.linear_wide_applies(160, 160, 160) and ops.linear_wide_applies(256, 256, 256) and ops.linear_wide_applies(1, 0, 1)
    assert not ops.linear_wide_applies(256, 257, 160) and not ops.linear_wide_applies(160, 160, 257)
    assert not ops.linear_wide_applies(0, 4, 4) and not ops.linear_wide_applies(4, -1, 4)


# ---- the dispatch of dense_ln.run, with every op stubbed --------------------------------------------------------------------
def _conv(cls=SparseCINConv, hidden=32, **kw):
    args = (hidden, hidden, hidden) + (None,) * (4 if cls is SparseCINConv else 6)
    return cls(*args, max_dim=2, hidden=hidden, act_module=ReLU, layer_dim=hidden, graph_norm=LN, use_coboundaries=True, **kw)


def _run_stubbed(conv, monkeypatch, rows=5):
    """dense_ln.run over zeros on the CPU: the products and the LayerNorm launches are replaced by shape-correct stubs that
    record who was asked for the combine product."""
    nb = 2 if isinstance(conv, SparseCINConv) and not isinstance(conv, CINppConv) else len(
        [n for n in (conv.mp_levels[0].update_up_nn, conv.mp_levels[0].update_boundaries_nn, conv.mp_levels[0].update_down_nn,
                     conv.mp_levels[0].update_coboundaries_nn) if n is not None])
    chains, combine = conv._ln_chains([[None] * nb] * 3, [None] * (3 * nb), 0)
    assert dense_ln.supported(chains, combine)
    calls = []

    def gemm_many(gemms):
        calls.append(('gemm_many', [(g.X.size(1), 0 if g.X2 is None else g.X2.size(1), g.W.size(0)) for g in gemms]))
        return [torch.zeros(g.X.size(0), g.W.size(0)) for g in gemms]

    def linear_wide(X, X2, weight, bias):
        calls.append(('linear_wide', [(X.size(1), X2.size(1), weight.size(0))]))
        return torch.zeros(X.size(0), weight.size(0))

    def linear(x, w, b):
        calls.append(('torch', [(x.size(1), 0, w.size(0))]))
        return torch.zeros(x.size(0), w.size(0))

    monkeypatch.setattr(ops, 'gemm_many', gemm_many)
    monkeypatch.setattr(ops, 'linear_wide', linear_wide)
    monkeypatch.setattr(ops, 'layer_norm_act_many', lambda zs, norms, relu=True: list(zs))
    monkeypatch.setattr(torch.nn.functional, 'linear', linear)
    width = conv.mp_levels[0].up_msg_size
    outs = dense_ln.run(chains, combine, [torch.zeros(rows, width) for _ in range(3 * nb)])
    assert [tuple(o.shape) for o in outs] == [(rows, width)] * 3
    return calls


def test_width_160_takes_the_op(monkeypatch):
    calls = _run_stubbed(_conv(hidden=160), monkeypatch)
    assert [c[0] for c in calls] == ['gemm_many', 'gemm_many', 'linear_wide', 'linear_wide', 'linear_wide'], calls
    assert all(c[1] == [(160, 160, 160)] for c in calls[2:])


def test_width_128_takes_what_it_took(monkeypatch):
    calls = _run_stubbed(_conv(hidden=128), monkeypatch)
    assert [c[0] for c in calls] == ['gemm_many', 'gemm_many', 'gemm_many'], calls
    assert calls[2][1] == [(128, 128, 128)] * 3                             # K + K2 = 256 = GEMM_MAX_K: the grouped GEMM


@pytest.mark.parametrize('kw', [dict(), dict(coboundary_stream=True)])
def test_three_and_four_branches_take_what_they_took(kw, monkeypatch):
    calls = _run_stubbed(_conv(CINppConv, hidden=160, **kw), monkeypatch)
    nb = 4 if kw else 3
    assert [c[0] for c in calls] == ['gemm_many', 'gemm_many', 'torch', 'torch', 'torch'], calls
    assert all(c[1] == [(nb * 160, 0, 160)] for c in calls[2:])


def test_beyond_the_new_limits_stays_on_the_torch_branch(monkeypatch):
    monkeypatch.setattr(_ffi, 'LINEAR_WIDE_MAX_K', 256)                     # (as if 320 were beyond the op)
    calls = _run_stubbed(_conv(hidden=160), monkeypatch)
    assert [c[0] for c in calls][2:] == ['torch'] * 3, calls
