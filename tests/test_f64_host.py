"""The float64 aggregate / gather entry points without a GPU: exported and declared, the descriptor's layout, argument
validation before any launch, and the dtype rules of cwn_amd.ops that need no device."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from cwn_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, ALIGN = 1, 5            # CWN_ERR_BAD_ARG, CWN_ERR_ALIGN


def test_f64_symbols_are_exported_and_declared():
    hdr = open(os.path.join(ROOT, 'include', 'cwn_hip.h')).read()
    lib = _ffi.lib()
    for name in ('cwn_aggregate_f64', 'cwn_gather_rows_f64'):
        assert name in _ffi.EXPORTS
        assert re.search(r'\bint %s\(' % name, hdr), name
        assert getattr(lib, name).restype is ctypes.c_int
    assert _ffi.ABI_VERSION == 24 == lib.cwn_abi_version()          # additive: nothing that existed changed layout


def test_f64_descriptor_layout_matches_the_ctypes_mirror(tmp_path):
    """cwn_agg_desc_f64 has the layout of cwn_agg_desc: the one ctypes AggDesc serves both."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cwn_hip.h"', 'int main(void) {']
    for cname in ('cwn_agg_desc_f64', 'cwn_agg_desc'):
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in _ffi.AggDesc._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['return 0; }']
    src = tmp_path / 'probe.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname in ('cwn_agg_desc_f64', 'cwn_agg_desc'):
        assert int(got[cname]) == ctypes.sizeof(_ffi.AggDesc), cname
        for fname, _ in _ffi.AggDesc._fields_:
            assert int(got[f'{cname}.{fname}']) == getattr(_ffi.AggDesc, fname).offset, (cname, fname)
    # ... and the element type really is double
    hdr = open(os.path.join(ROOT, 'include', 'cwn_hip.h')).read()
    body = re.search(r'typedef struct cwn_agg_desc_f64 \{(.*?)\} cwn_agg_desc_f64;', hdr, re.S).group(1)
    assert 'float' not in body and body.count('double') == 8


def _desc(**kw):
    base = dict(n_dst=4, F=8, msg_op=0, reduce=0, out=0x1000, self_x=0x2000)         # absent adjacency: zeros + self term
    base.update(kw)
    return (_ffi.AggDesc * 1)(_ffi.AggDesc(**base))


def _check_refusals(agg, gat, off):
    """The descriptors and gather arguments both element types refuse (one validity rule: csrc/cwn_aggregate_body.h);
    `off` is a byte offset that breaks the type's alignment."""
    assert agg(None, 1, None) == BAD_ARG
    assert agg(_desc(), 0, None) == BAD_ARG
    nine = (_ffi.AggDesc * 9)(*[_ffi.AggDesc(n_dst=4, F=8, out=0x1000) for _ in range(9)])
    assert agg(nine, 9, None) == BAD_ARG
    assert agg(_desc(F=0), 1, None) == BAD_ARG
    assert agg(_desc(n_dst=-1), 1, None) == BAD_ARG
    assert agg(_desc(out=None), 1, None) == BAD_ARG
    assert agg(_desc(msg_op=7), 1, None) == BAD_ARG and agg(_desc(reduce=3), 1, None) == BAD_ARG
    for op in (3, 4, 5, 6):                  # CWN_MSG_RELU_A_PLUS_B and above: add only
        for red in (1, 2):
            assert agg(_desc(msg_op=op, reduce=red), 1, None) == BAD_ARG, (op, red)
    # an adjacency without its operands
    assert agg(_desc(rowptr=0x3000), 1, None) == BAD_ARG
    assert agg(_desc(rowptr=0x3000, ia=0x4000, A=0x5000, msg_op=1), 1, None) == BAD_ARG
    assert agg(_desc(rowptr=0x3000, ia=0x4000, A=0x5000, msg_op=4, ib=0x6000, B=0x7000, b_width=8), 1, None) == BAD_ARG
    assert agg(_desc(out=0x1000 + off), 1, None) == ALIGN
    assert agg(_desc(self_x=0x2000 + off), 1, None) == ALIGN
    assert agg(_desc(n_dst=0), 1, None) == 0                # nothing to do
    assert gat(None, 0, 0, None, 0, None, None) == BAD_ARG
    assert gat(None, 5, 4, None, 3, None, None) == BAD_ARG
    assert gat(0x1000, 5, 4, 0x2000, -1, 0x3000, None) == BAD_ARG
    assert gat(0x1000 + off, 5, 4, 0x2000, 3, 0x3000, None) == ALIGN
    assert gat(0x1000, 5, 4, 0x2000, 3, 0x3000 + off, None) == ALIGN
    assert gat(None, 5, 4, None, 0, None, None) == 0        # an empty index


def test_f64_bad_arguments_are_refused_before_any_launch():
    lib = _ffi.lib()
    # doubles lie on 8 bytes: a pointer that is only 4-byte aligned
    _check_refusals(lib.cwn_aggregate_f64, lib.cwn_gather_rows_f64, off=4)
    assert lib.cwn_aggregate_f64(_desc(eps=0x2004), 1, None) == ALIGN


def test_f32_bad_arguments_are_refused_before_any_launch():
    lib = _ffi.lib()
    # floats lie on 4 bytes; the f32 entry does not look at eps
    _check_refusals(lib.cwn_aggregate_f32, lib.cwn_gather_rows_f32, off=2)


def test_small_operand_flag_follows_the_element_size():
    """CWN_AGG_SMALL_OPERANDS vouches for BYTE offsets below 2^32: half as many float64 elements as float32."""
    from cwn_amd import ops

    class Rows:                      # a stand-in with the size of a large operand
        def __init__(self, numel, dtype): self.n, self.dtype = numel, dtype
        def numel(self): return self.n
        def size(self, d): return 8
        def data_ptr(self): return 0x1000
    n = (1 << 29) + 8                # 4 GiB + 64 B of doubles, 2 GiB of floats
    out32, out64 = torch.zeros(4, 8), torch.zeros(4, 8, dtype=torch.float64)
    assert ops.AggSpec(adj=None, n_dst=4, F=8, A=Rows(n, torch.float32), out=out32).desc().flags == ops.AGG_SMALL_OPERANDS
    assert ops.AggSpec(adj=None, n_dst=4, F=8, A=Rows(n, torch.float64), out=out64).desc().flags == 0
    assert ops.AggSpec(adj=None, n_dst=4, F=8, A=Rows(n // 2, torch.float64), out=out64).desc().flags == ops.AGG_SMALL_OPERANDS


def test_spec_dtype_comes_from_its_operands():
    from cwn_amd import ops
    x32, x64 = torch.zeros(4, 8), torch.zeros(4, 8, dtype=torch.float64)
    assert ops.AggSpec(adj=None, n_dst=4, F=8, self_x=x64).resolve_dtype() == torch.float64        # adj=None: from self_x
    assert ops.AggSpec(adj=None, n_dst=4, F=8, self_x=x32).resolve_dtype() == torch.float32
    assert ops.AggSpec(adj=None, n_dst=4, F=8).resolve_dtype() == torch.float32
    assert ops.AggSpec(adj=None, n_dst=4, F=8, dtype=torch.float64).resolve_dtype() == torch.float64
    with pytest.raises(TypeError, match='float32.*float64|float64.*float32'):
        ops.AggSpec(adj=None, n_dst=4, F=8, A=x32, self_x=x64).resolve_dtype()
    assert ops.zeros_rows(2, 3, 'cpu', torch.float64).dtype == torch.float64
    assert ops.zeros_rows(2, 3, 'cpu').dtype == torch.float32


def test_float32_only_machinery_names_the_dtype():
    from cwn_amd import ops
    model = torch.nn.Linear(3, 3).double()
    with pytest.raises(TypeError, match='float64'):
        ops.require_float32_model(model, 'StaticForward')
    ops.require_float32_model(torch.nn.Linear(3, 3), 'StaticForward')
    # the flat optimizer hands raw pointers to float32 kernels: double parameters are refused before anything is re-homed
    from cwn_amd.dist import FlatGradBucket
    from cwn_amd.train import FlatAdam
    w = model.weight
    with pytest.raises(TypeError, match='float64'):
        FlatAdam(FlatGradBucket(model.parameters()))
    assert model.weight is w and model.weight.grad is None and model.weight.dtype == torch.float64
