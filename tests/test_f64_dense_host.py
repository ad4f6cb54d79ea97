"""The float64 dense path without a GPU (csrc/cwn_dense_f64.hip behind ops.linear_many_f64 / ops.update_chain_f64): the
launchers refuse every malformed descriptor before anything is launched, the ctypes records have the header's layout,
the predicate and SparseCINConv._dense_f64 decline what the launch does not take, and the ops refuse other operands by
naming the dtype."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from cwn_amd import _ffi, layers, ops
from cwn_amd.layers import SparseCINConv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, ALIGN = 1, 5
F64 = torch.float64


def _buf(n=64 * 128):
    return (ctypes.c_double * n)()


def test_records_match_the_header(tmp_path):
    structs = {'cwn_linear_desc_f64': _ffi.LinearDescF64, 'cwn_chain_desc_f64': _ffi.ChainDescF64}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cwn_hip.h"', 'int main(void) {']
    for cname, st in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in st._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    for macro in ('CWN_LINEAR_F64_MAX_DESCS', 'CWN_LINEAR_F64_MAX_WIDTH', 'CWN_CHAIN_F64_MAX_DIMS', 'CWN_CHAIN_F64_MAX_WIDTH',
                  'CWN_DENSE_F64_TILE_ROWS'):
        lines.append(f'printf("{macro} %d\\n", {macro});')
    lines += ['return 0; }']
    src = tmp_path / 'probe.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, st in structs.items():
        assert int(got[cname]) == ctypes.sizeof(st), cname
        for fname, _ in st._fields_:
            assert int(got[f'{cname}.{fname}']) == getattr(st, fname).offset, (cname, fname)
    assert (_ffi.LINEAR_F64_MAX_DESCS, _ffi.LINEAR_F64_MAX_WIDTH, _ffi.CHAIN_F64_MAX_DIMS, _ffi.CHAIN_F64_MAX_WIDTH,
            _ffi.DENSE_F64_TILE_ROWS) == tuple(int(got[m]) for m in ('CWN_LINEAR_F64_MAX_DESCS', 'CWN_LINEAR_F64_MAX_WIDTH',
                                                                      'CWN_CHAIN_F64_MAX_DIMS', 'CWN_CHAIN_F64_MAX_WIDTH',
                                                                      'CWN_DENSE_F64_TILE_ROWS'))
    hdr = open(os.path.join(ROOT, 'include', 'cwn_hip.h')).read()
    acts = re.search(r'enum \{ CWN_ACT_ID = 0, CWN_ACT_RELU = 1, CWN_ACT_ELU = 2[^}]*CWN_ACT_TANH = 3, CWN_ACT_SIGMOID = 4 \}', hdr)
    assert acts and ops.ACT_CODES == {'id': 0, 'relu': 1, 'elu': 2, 'tanh': 3, 'sigmoid': 4}


def _linear(keep, **kw):
    x, w, b, y = (_buf() for _ in range(4))
    keep += [x, w, b, y]
    f = dict(X=ctypes.addressof(x), W=ctypes.addressof(w), bias=ctypes.addressof(b), Y=ctypes.addressof(y), M=5, ldx=16, ldw=16,
             ldy=16, K=16, N=16, act=_ffi.ACT_ELU)
    f.update(kw)
    return _ffi.LinearDescF64(**f)


def test_linear_many_refuses_malformed_descriptors():
    """Everything is checked on the host before the first HIP call: these calls never reach a device (there is none here)."""
    fn = _ffi.lib().cwn_linear_many_f64
    keep = []
    arr = lambda *ds: (_ffi.LinearDescF64 * len(ds))(*ds)
    assert fn(None, 1, None) == BAD_ARG
    assert fn(arr(_linear(keep)), 0, None) == BAD_ARG
    assert fn(arr(_linear(keep)), -1, None) == BAD_ARG
    assert fn(arr(*[_linear(keep, M=0) for _ in range(17)]), 17, None) == BAD_ARG
    for bad in (dict(M=-1), dict(K=0), dict(K=129, ldx=129, ldw=129), dict(N=0), dict(N=129, ldy=129), dict(act=5), dict(act=-1),
                dict(X=None), dict(W=None), dict(Y=None), dict(ldx=15), dict(ldw=15), dict(ldy=15)):
        assert fn(arr(_linear(keep, **bad)), 1, None) == BAD_ARG, bad
        assert fn(arr(_linear(keep, M=0), _linear(keep, **bad)), 2, None) == BAD_ARG, bad       # ... wherever it stands
    d = _linear(keep)
    d.X += 4
    assert fn(arr(d), 1, None) == ALIGN
    # M = 0 is legal, writes nothing, and does not look at the pointers; widths are still checked
    assert fn(arr(_linear(keep, M=0, X=None, W=None, Y=None, bias=None)), 1, None) == 0
    assert fn(arr(*[_linear(keep, M=0) for _ in range(16)]), 16, None) == 0
    assert fn(arr(_linear(keep, M=0, K=200)), 1, None) == BAD_ARG


def _chain(keep, edits=None, **kw):
    bufs = [_buf() for _ in range(23)]
    keep += bufs
    a = [ctypes.addressof(b) for b in bufs]
    d = _ffi.ChainDescF64(in_up=a[0], in_b=a[1], out=a[2], n=7, ld_up=16, ld_b=16, ld_out=16, F=16, H=16, act=_ffi.ACT_RELU)
    for s in range(5):
        d.W[s], d.bias[s], d.scale[s], d.shift[s] = a[3 + s], a[8 + s], a[13 + s], a[18 + s]
    for k, v in {**kw, **(edits or {})}.items():
        if isinstance(k, tuple):
            getattr(d, k[0])[k[1]] = v
        else:
            setattr(d, k, v)
    return d


def test_update_chain_refuses_malformed_descriptors():
    fn = _ffi.lib().cwn_update_chain_f64
    keep = []
    arr = lambda *ds: (_ffi.ChainDescF64 * len(ds))(*ds)
    assert fn(None, 1, None) == BAD_ARG
    for n_dims in (0, -1, 5):
        assert fn(arr(*[_chain(keep, n=0) for _ in range(5)]), n_dims, None) == BAD_ARG, n_dims
    bads = [dict(n=-1), dict(F=0), dict(F=65, ld_up=65, ld_b=65), dict(H=0), dict(H=65, ld_out=65), dict(act=5), dict(act=-2),
            dict(in_up=None), dict(in_b=None), dict(out=None), dict(ld_up=15), dict(ld_b=15), dict(ld_out=15),
            {('W', 0): None}, {('W', 4): None}, {('scale', 2): None}, {('shift', 3): None}]
    for bad in bads:
        assert fn(arr(_chain(keep, bad)), 1, None) == BAD_ARG, bad
        assert fn(arr(_chain(keep, n=0), _chain(keep, n=0), _chain(keep, bad)), 3, None) == BAD_ARG, bad
    d = _chain(keep)
    d.W[1] += 4
    assert fn(arr(d), 1, None) == ALIGN
    # empty dimensions: legal, nothing launched; biases and affines are optional
    empty = _chain(keep, n=0, in_up=None, in_b=None, out=None)
    assert fn(arr(empty), 1, None) == 0
    assert fn(arr(*[_chain(keep, n=0) for _ in range(4)]), 4, None) == 0
    assert fn(arr(_chain(keep, {('bias', 0): None, ('scale', 0): None, ('shift', 0): None}, n=0, F=1, H=64)), 1, None) == 0
    assert fn(arr(_chain(keep, {('scale', 0): None}, n=0)), 1, None) == BAD_ARG               # scale without shift, even when empty


# ---- the predicate and the layer's declines, on CPU tensors ------------------------------------------------------------
def _conv(hidden=16, layer_dim=16, norm=torch.nn.Identity, act=torch.nn.ELU, dtype=F64, **kw):
    conv = SparseCINConv(layer_dim, layer_dim, layer_dim, None, None, kw.pop('up_nn', None), kw.pop('b_nn', None), max_dim=2,
                         hidden=hidden, act_module=act, layer_dim=layer_dim, graph_norm=norm, use_coboundaries=True, **kw)
    return conv.to(dtype).eval()


def _chain_dim(F=16, H=16, n=5, dtype=F64, **kw):
    t = lambda *s: torch.zeros(*s, dtype=dtype)
    f = dict(in_up=t(n, F), in_b=t(n, F), weights=[t(H, F), t(H, H), t(H, F), t(H, H), t(H, 2 * H)], biases=[t(H)] * 5,
             folds=[(None, None)] * 5, act='elu')
    f.update(kw)
    return ops.ChainDim(**f)


def test_predicate_declines_what_the_launch_does_not_take():
    class OnGpu(torch.Tensor):           # a float64 CPU tensor that says it is on the GPU: the predicate's other checks
        @property
        def is_cuda(self):
            return True

    def gpu(d):
        as_gpu = lambda t: None if t is None else t.as_subclass(OnGpu)
        return ops.ChainDim(in_up=as_gpu(d.in_up), in_b=as_gpu(d.in_b), weights=[as_gpu(w) for w in d.weights],
                            biases=[as_gpu(b) for b in d.biases], folds=[(as_gpu(s), as_gpu(t)) for s, t in d.folds], act=d.act,
                            out=as_gpu(d.out))
    ok = ops.update_chain_f64_applies
    assert ok([gpu(_chain_dim())]) and ok([gpu(_chain_dim(1, 64)), gpu(_chain_dim(64, 64, n=0)), gpu(_chain_dim(5, 3))])
    assert not ok([_chain_dim()])                                            # CPU tensors
    assert not ok([]) and not ok([gpu(_chain_dim())] * 5)
    assert not ok([gpu(_chain_dim(65, 16))]) and not ok([gpu(_chain_dim(16, 65))])        # width 65
    assert not ok([gpu(_chain_dim(dtype=torch.float32))])                                 # float32
    assert not ok([gpu(_chain_dim(act='gelu'))])
    assert not ok([gpu(_chain_dim(in_b=torch.zeros(4, 16, dtype=F64)))])                  # row counts differ
    assert not ok([gpu(_chain_dim(folds=[(torch.zeros(16, dtype=F64), None)] + [(None, None)] * 4))])
    assert not ok([gpu(_chain_dim(out=torch.zeros(4, 16, dtype=F64)))])                   # fewer rows than n
    w = _chain_dim().weights
    w[4] = torch.zeros(16, 64, dtype=F64)[:, :32]                                         # combine weight not contiguous
    assert not ok([gpu(_chain_dim(weights=w))])


def test_ops_refuse_other_operands_by_naming_the_dtype():
    x, w = torch.zeros(3, 4), torch.zeros(2, 4)
    with pytest.raises(TypeError, match='float32'):
        ops.linear_many_f64([(x, w, None, 'id')])
    with pytest.raises(TypeError, match='float16'):
        ops.linear_many_f64([(x.half(), w.double(), None, 'id')])
    with pytest.raises(TypeError, match=r'float64.*cpu'):
        ops.linear_many_f64([(x.double(), w.double(), None, 'id')])                   # float64, but not on the GPU
    with pytest.raises(TypeError, match='float32'):
        ops.update_chain_f64([_chain_dim(dtype=torch.float32)])
    with pytest.raises(TypeError, match=r'float64.*cpu'):
        ops.update_chain_f64([_chain_dim()])
    with pytest.raises(ValueError, match='activation'):
        ops._act_code('gelu')


def test_dense_f64_declines_on_the_layer(monkeypatch):
    """SparseCINConv._dense_f64 returns None -- the caller then runs the torch modules exactly as before -- for width 65,
    LayerNorm, a training-mode BatchNorm, a passed-in Sequential, float32, a recording autograd and the switch; and its
    structural half accepts the stock networks with each of the five activations."""
    called = []
    monkeypatch.setattr(ops, 'update_chain_f64', lambda dims: called.append(dims) or ['launched'] * len(dims))
    monkeypatch.setattr(ops, 'update_chain_f64_applies', lambda dims: True)

    class OnGpu(torch.Tensor):
        @property
        def is_cuda(self):
            return True

    def outs(width=16, dtype=F64, n_dims=3):
        return [torch.zeros(4, width, dtype=dtype).as_subclass(OnGpu) for _ in range(2 * n_dims)]
    plans = [['stream'] * 2] * 3
    with torch.no_grad():
        for act in (torch.nn.ReLU, torch.nn.ELU, torch.nn.Tanh, torch.nn.Sigmoid, torch.nn.Identity):
            assert _conv(act=act)._dense_f64(plans, outs()) == ['launched'] * 3
        bn = _conv(norm=torch.nn.BatchNorm1d)
        assert bn._dense_f64(plans, outs()) == ['launched'] * 3                   # eval-mode BatchNorm folds
        assert all(s is not None and s.dtype == F64 for s, _ in called[-1][0].folds)
        n_ok = len(called)
        assert _conv(hidden=65)._dense_f64(plans, outs()) is None                 # width 65
        assert _conv(hidden=16, layer_dim=65)._dense_f64(plans, outs(65)) is None
        assert _conv(norm=torch.nn.LayerNorm)._dense_f64(plans, outs()) is None
        assert bn.train()._dense_f64(plans, outs()) is None                       # batch statistics are no fixed affine
        custom = torch.nn.Sequential(torch.nn.Linear(16, 16), torch.nn.ELU()).double()
        assert _conv(up_nn=custom)._dense_f64(plans, outs()) is None              # a passed-in network
        assert _conv(dtype=torch.float32)._dense_f64(plans, outs(dtype=torch.float32)) is None
        assert _conv()._dense_f64(plans, [torch.zeros(4, 16, dtype=F64)] * 6) is None          # CPU features
        assert _conv()._dense_f64([None] + plans[1:], outs(n_dims=2)) is None     # an unfused dimension without its parameters
        from cwn_amd.layers import CINppConv
        pp = CINppConv(16, 16, 16, None, None, None, None, None, None, max_dim=2, hidden=16, act_module=torch.nn.ELU, layer_dim=16,
                       graph_norm=torch.nn.Identity, use_coboundaries=True).double().eval()
        assert pp._dense_f64(plans, outs()) is None
        monkeypatch.setattr(layers, 'FUSED_F64_DENSE', False)
        assert _conv()._dense_f64(plans, outs()) is None
        monkeypatch.setattr(layers, 'FUSED_F64_DENSE', True)
    assert _conv()._dense_f64(plans, outs()) is None                              # autograd is recording
    assert len(called) == n_ok


def test_the_switch_follows_the_environment():
    env = dict(os.environ, CWN_FUSED_F64_DENSE='0')
    out = subprocess.run([os.sys.executable, '-c', 'from cwn_amd import layers; print(layers.FUSED_F64_DENSE)'], cwd=ROOT, env=env,
                         capture_output=True, text=True, check=True).stdout
    assert out.strip() == 'False'
