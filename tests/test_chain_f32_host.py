"""The float32 update chain without a GPU (csrc/cwn_chain_f32.hip behind ops.update_chain_f32 and
SparseCINConv._dense_chain_f32): the symbol is declared, bound and exported under ABI 24, the ctypes record has the header's
layout, the launcher refuses every malformed descriptor before anything is launched, the predicate and the op refuse other
operands (naming the dtype), the layer's route declines what it must on CPU tensors, and the switch reads its regimes."""
import ctypes
import os
import re
import subprocess
from types import SimpleNamespace

import pytest
import torch

from cwn_amd import _ffi, layers, ops
from cwn_amd.layers import CINppConv, SparseCINConv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, TOO_LARGE, ALIGN = 0, 1, 2, 5
F32 = torch.float32


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_new_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'cwn_hip.h')).read()
    lib = _ffi.lib()
    assert re.search(r'\bint cwn_update_chain_f32\s*\(const cwn_chain_desc_f32\* descs_host, int n, cwn_stream_t stream\)', header)
    assert 'cwn_update_chain_f32' in _ffi.EXPORTS and hasattr(lib, 'cwn_update_chain_f32')
    assert lib.cwn_abi_version() == _ffi.ABI_VERSION == 24
    assert int(re.search(r'#define CWN_ABI_VERSION (\d+)', header).group(1)) == 24
    section = header[header.index('The float32 update chain'):header.index('int cwn_update_chain_f32')]
    for said in ('m_dev', 'CLAMPED', 'never written', 'All checks precede the first HIP call', 'CIN++', 'training',
                 'widths above 128', 'compiled torch binding', 'float64'):
        assert said in section, said
    assert 'cwn_chain_f32.hip' in open(os.path.join(ROOT, 'cwn_amd', 'csrc', 'Makefile')).read()


def test_record_matches_the_header(tmp_path):
    """cwn_chain_desc_f32 field by field against the ctypes mirror, through a probe compiled with the host C compiler."""
    st, cname = _ffi.ChainDescF32, 'cwn_chain_desc_f32'
    macros = ('CWN_CHAIN_F32_MAX_DIMS', 'CWN_CHAIN_F32_MAX_WIDTH', 'CWN_CHAIN_F32_TM')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cwn_hip.h"', 'int main(void) {',
             f'printf("size %zu\\n", sizeof({cname}));']
    lines += [f'printf("{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in st._fields_]
    lines += [f'printf("{m} %d\\n", {m});' for m in macros]
    lines += ['return 0; }']
    src, exe = tmp_path / 'probe.c', tmp_path / 'probe'
    src.write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got['size']) == ctypes.sizeof(st)
    assert [f for f, _ in st._fields_] == ['in_up', 'in_b', 'out', 'W', 'bias', 'scale', 'shift', 'n', 'ld_up', 'ld_b', 'ld_out',
                                           'F', 'H', 'act', 'reserved', 'm_dev']
    for f, _ in st._fields_:
        assert int(got[f]) == getattr(st, f).offset, f
    assert (_ffi.CHAIN_F32_MAX_DIMS, _ffi.CHAIN_F32_MAX_WIDTH, _ffi.CHAIN_F32_TM) == tuple(int(got[m]) for m in macros) == (4, 128, 32)


P = 0x100000


def _desc(edits=None, **kw):
    """A descriptor that passes every check (made-up, aligned addresses far apart: a call that passed the checks with rows
    would launch, so every case below breaks exactly one thing or has no rows)."""
    d = _ffi.ChainDescF32(in_up=P, in_b=2 * P, out=3 * P, n=7, ld_up=12, ld_b=12, ld_out=20, F=12, H=20, act=_ffi.ACT_TANH,
                          m_dev=30 * P)
    for s in range(5):
        d.W[s], d.bias[s], d.scale[s], d.shift[s] = (4 + s) * P, (9 + s) * P, (14 + s) * P, (19 + s) * P
    for k, v in {**kw, **(edits or {})}.items():
        if isinstance(k, tuple):
            getattr(d, k[0])[k[1]] = v
        else:
            setattr(d, k, v)
    return d


def _call(*ds, n=None):
    return _ffi.lib().cwn_update_chain_f32((_ffi.ChainDescF32 * len(ds))(*ds), len(ds) if n is None else n, None)


BAD = {
    'n<0': dict(n=-1), 'F=0': dict(F=0), 'F=129': dict(F=129, ld_up=129, ld_b=129), 'H=0': dict(H=0), 'H=129': dict(H=129, ld_out=129),
    'act=-1': dict(act=-1), 'act=5': dict(act=5), 'in_up NULL': dict(in_up=None), 'in_b NULL': dict(in_b=None),
    'out NULL': dict(out=None), 'ld_up<F': dict(ld_up=11), 'ld_b<F': dict(ld_b=11), 'ld_out<H': dict(ld_out=19),
    'W[0] NULL': {('W', 0): None}, 'W[1] NULL': {('W', 1): None}, 'W[2] NULL': {('W', 2): None}, 'W[3] NULL': {('W', 3): None},
    'W[4] NULL': {('W', 4): None},
}


@pytest.mark.parametrize('case', sorted(BAD))
def test_bad_arguments_are_refused_before_any_hip_call(case):
    assert _call(_desc(BAD[case])) == BAD_ARG, case
    assert _call(_desc(n=0), _desc(n=0), _desc(BAD[case])) == BAD_ARG, case               # ... wherever it stands


def test_null_descriptors_counts_misaligned_pointers_and_too_many_tiles():
    assert _ffi.lib().cwn_update_chain_f32(None, 1, None) == BAD_ARG
    for n_dims in (0, -1, 5):
        assert _call(*[_desc(n=0) for _ in range(5)], n=n_dims) == BAD_ARG, n_dims
    for field in ('in_up', 'in_b', 'out'):
        assert _call(_desc(**{field: 40 * P + 2})) == ALIGN, field
    for field in ('W', 'bias', 'scale', 'shift'):
        for s in range(5):
            assert _call(_desc({(field, s): 40 * P + 2})) == ALIGN, (field, s)
    assert _call(_desc(m_dev=40 * P + 4)) == ALIGN                         # the device count is an int64
    assert _call(_desc(F=0, in_up=P + 2)) == BAD_ARG                       # the argument checks come first
    assert _call(_desc(n=_ffi.CHAIN_F32_TM * (2 ** 31 - 1))) == TOO_LARGE
    assert _call(_desc(n=_ffi.CHAIN_F32_TM * 2 ** 30), _desc(n=_ffi.CHAIN_F32_TM * 2 ** 30)) == TOO_LARGE      # ... in sum


def test_empty_launches_and_legal_shapes_are_ok_without_a_device():
    """Dimensions without rows return before the first HIP call and none of their pointers is looked at; every per-stage
    vector is optional on its own; the widths are checked even then."""
    assert _call(_desc(n=0)) == OK
    assert _call(*[_desc(n=0) for _ in range(4)]) == OK
    assert _call(_desc(n=0, in_up=None, in_b=None, out=None, m_dev=None)) == OK
    assert _call(_desc({('W', 2): None, ('bias', 0): 3, ('scale', 1): None, ('shift', 4): None}, n=0, in_up=2)) == OK
    for F, H in ((1, 128), (128, 1), (3, 5), (128, 128)):
        assert _call(_desc(n=0, F=F, H=H)) == OK
    assert _call(_desc(n=0, F=200)) == BAD_ARG
    assert _call(_desc(n=0, act=7)) == BAD_ARG


# ---- the predicate and the op ---------------------------------------------------------------------------------------------
class OnGpu(torch.Tensor):               # a CPU tensor that says it is on the GPU: reaches the checks behind the device's
    @property
    def is_cuda(self):
        return True


def _chain_dim(F=16, H=16, n=5, dtype=F32, **kw):
    t = lambda *s: torch.zeros(*s, dtype=dtype)
    f = dict(in_up=t(n, F), in_b=t(n, F), weights=[t(H, F), t(H, H), t(H, F), t(H, H), t(H, 2 * H)], biases=[t(H)] * 5,
             folds=[(None, None)] * 5, act='elu')
    f.update(kw)
    return ops.ChainDim(**f)


def _gpu(d):
    as_gpu = lambda t: None if t is None else t.as_subclass(OnGpu)
    return ops.ChainDim(in_up=as_gpu(d.in_up), in_b=as_gpu(d.in_b), weights=[as_gpu(w) for w in d.weights],
                        biases=[as_gpu(b) for b in d.biases], folds=[(as_gpu(s), as_gpu(t)) for s, t in d.folds], act=d.act,
                        out=as_gpu(d.out))


def test_predicate_declines_what_the_launch_does_not_take():
    ok = ops.update_chain_f32_applies
    assert ok([_gpu(_chain_dim())]) and ok([_gpu(_chain_dim(1, 128)), _gpu(_chain_dim(128, 128, n=0)), _gpu(_chain_dim(5, 3))])
    assert ok([_gpu(_chain_dim(48, 48, act=a)) for a in ('relu', 'tanh', 'sigmoid', 'id')])
    assert not ok([_chain_dim()])                                            # CPU tensors
    assert not ok([]) and not ok([_gpu(_chain_dim())] * 5)
    assert not ok([_gpu(_chain_dim(129, 16))]) and not ok([_gpu(_chain_dim(16, 129))])      # width 129
    assert not ok([_gpu(_chain_dim(dtype=torch.float64))])
    assert not ok([_gpu(_chain_dim(act='gelu'))])
    assert not ok([_gpu(_chain_dim(in_b=torch.zeros(4, 16)))])                              # row counts differ
    assert not ok([_gpu(_chain_dim(biases=[torch.zeros(15)] * 5))])
    assert not ok([_gpu(_chain_dim(out=torch.zeros(4, 16)))])                               # fewer rows than n
    assert ok([_gpu(_chain_dim(out=torch.zeros(9, 40)[:, :16]))])                           # a row-strided view with room
    assert ok([_gpu(_chain_dim(in_up=torch.zeros(5, 40)[:, 8:24]))])
    assert not ok([_gpu(_chain_dim(in_up=torch.zeros(16, 5).t()))])                         # rows not contiguous
    # a stage's scale and shift are optional on their own here (the float64 launch wants both or neither)
    half = [(torch.zeros(16), None), (None, torch.zeros(16))] + [(None, None)] * 3
    assert ok([_gpu(_chain_dim(folds=half))])
    assert not ops.update_chain_f64_applies([_gpu(_chain_dim(folds=[(s if s is None else s.double(), t if t is None else t.double())
                                                                     for s, t in half], dtype=torch.float64))])
    w = _chain_dim().weights
    w[4] = torch.zeros(16, 64)[:, :32]                                                      # combine weight not contiguous
    assert not ok([_gpu(_chain_dim(weights=w))])


def test_op_refuses_other_operands_by_naming_the_dtype():
    with pytest.raises(TypeError, match='float64'):
        ops.update_chain_f32([_chain_dim(dtype=torch.float64)])
    with pytest.raises(TypeError, match='float16'):
        ops.update_chain_f32([_gpu(_chain_dim(in_b=torch.zeros(5, 16, dtype=torch.float16)))])
    with pytest.raises(TypeError, match=r'float32.*cpu'):
        ops.update_chain_f32([_chain_dim()])                                                # float32, but not on the GPU
    with pytest.raises(TypeError, match='contiguous rows'):
        ops.update_chain_f32([_gpu(_chain_dim(in_up=torch.zeros(16, 5).t()))])
    with pytest.raises(ValueError, match='five-stage shapes'):
        ops.update_chain_f32([_gpu(_chain_dim(129, 16))])
    with pytest.raises(ValueError, match='five-stage shapes'):
        ops.update_chain_f32([_gpu(_chain_dim(in_b=torch.zeros(4, 16)))])
    with pytest.raises(ValueError, match='five-stage shapes'):
        ops.update_chain_f32([_gpu(_chain_dim())] * 5)


# ---- the route on the layer, on CPU tensors -------------------------------------------------------------------------------
def _conv(hidden=48, layer_dim=None, norm=torch.nn.Identity, act=torch.nn.ELU, dtype=F32, **kw):
    layer_dim = hidden if layer_dim is None else layer_dim
    conv = SparseCINConv(layer_dim, layer_dim, layer_dim, None, None, kw.pop('up_nn', None), kw.pop('b_nn', None), max_dim=2,
                         hidden=hidden, act_module=act, layer_dim=layer_dim, graph_norm=norm, use_coboundaries=True, **kw)
    return conv.to(dtype).eval()


def _outs(width=48, dtype=F32, n_dims=3):
    return [torch.zeros(4, width, dtype=dtype).as_subclass(OnGpu) for _ in range(2 * n_dims)]


PLANS = [['stream'] * 2] * 3


@pytest.fixture
def launched(monkeypatch):
    """The dimensions every prepared launch was built from; its run is replaced (there is no device here), its validity check
    is the real one."""
    built = []

    class Launch(ops.ChainLaunch):
        def __init__(self, dims, sources):
            super().__init__(dims, sources)
            built.append(dims)

        def run(self, ins):
            assert len(ins) == self.n and all(len(pair) == 2 for pair in ins)
            return ['launched'] * self.n
    monkeypatch.setattr(ops, 'ChainLaunch', Launch)
    monkeypatch.setattr(ops, 'update_chain_f32_applies', lambda dims: True)
    monkeypatch.setattr(layers, 'FUSED_CHAIN_F32', layers.CHAIN_F32_REGIMES)
    return built


def test_route_takes_the_stock_networks_of_its_regime(launched):
    with torch.no_grad():
        for act in (torch.nn.ELU, torch.nn.Tanh, torch.nn.Sigmoid, torch.nn.Identity):
            for hidden in (16, 48, 64, 128):
                assert _conv(hidden, act=act)._dense_chain_f32(PLANS, _outs(hidden)) == ['launched'] * 3
        assert [d.act for d in launched[-1]] == ['id'] * 3
        assert _conv(act=torch.nn.ReLU)._dense_chain_f32(PLANS, _outs()) is None                # ReLU is not the 'act' regime
        for hidden in (16, 48, 100):
            assert _conv(hidden, act=torch.nn.ReLU)._dense_chain_f32(PLANS, _outs(hidden), regime='relu_width') == ['launched'] * 3
        assert _conv(64, layer_dim=100, act=torch.nn.ReLU)._dense_chain_f32(PLANS, _outs(100), regime='relu_width') == ['launched'] * 3
        n_ok = len(launched)
        for hidden in (64, 128):             # ReLU at 64 / 128 never takes the chain, a narrower first layer included
            assert _conv(hidden, act=torch.nn.ReLU)._dense_chain_f32(PLANS, _outs(hidden), regime='relu_width') is None
        assert _conv(64, layer_dim=16, act=torch.nn.ReLU)._dense_chain_f32(PLANS, _outs(16), regime='relu_width') is None
        assert _conv(act=torch.nn.ELU)._dense_chain_f32(PLANS, _outs(), regime='relu_width') is None
        bn = _conv(norm=torch.nn.BatchNorm1d)
        assert bn._dense_chain_f32(PLANS, _outs()) == ['launched'] * 3                          # eval-mode BatchNorm folds
        assert all(s is not None and s.dtype == F32 and t is not None for s, t in launched[-1][0].folds)
        dims = launched[-1]
        lvl = bn.mp_levels[1]
        assert [w is m.weight for w, m in zip(dims[1].weights, (lvl.update_up_nn[0], lvl.update_up_nn[3], lvl.update_boundaries_nn[0],
                                                                lvl.update_boundaries_nn[3], lvl.combine_nn[0]))] == [True] * 5
        assert len(launched) == n_ok + 1
        # from a later dimension on (start_to_process): the active dimensions only
        assert _conv()._dense_chain_f32([None] + PLANS[1:], _outs(n_dims=2), 1) == ['launched'] * 2


def test_route_declines_on_the_layer(launched, monkeypatch):
    """None -- the caller goes on exactly as before -- for a width above 128, LayerNorm, a training-mode BatchNorm, a passed-in
    network, float64 and CPU features, CIN++, an unfused dimension without its parameters (or in the ReLU regime), a recording
    autograd and the switch."""
    with torch.no_grad():
        assert _conv(129)._dense_chain_f32(PLANS, _outs(129)) is None
        assert _conv(16, layer_dim=129)._dense_chain_f32(PLANS, _outs(129)) is None
        assert _conv(norm=torch.nn.LayerNorm)._dense_chain_f32(PLANS, _outs()) is None
        assert _conv(norm=torch.nn.BatchNorm1d).train()._dense_chain_f32(PLANS, _outs()) is None
        custom = torch.nn.Sequential(torch.nn.Linear(48, 48), torch.nn.ELU())
        assert _conv(up_nn=custom)._dense_chain_f32(PLANS, _outs()) is None
        assert _conv(dtype=torch.float64)._dense_chain_f32(PLANS, _outs(dtype=torch.float64)) is None
        assert _conv()._dense_chain_f32(PLANS, [torch.zeros(4, 48)] * 6) is None               # CPU features
        assert _conv()._dense_chain_f32(PLANS, _outs(n_dims=2)) is None                         # not two matrices per dimension
        assert _conv()._dense_chain_f32([None] + PLANS[1:], _outs(n_dims=2)) is None            # unfused, no parameters
        params = [SimpleNamespace(x=torch.zeros(4, 48)) for _ in range(3)]                      # ... whose features are on the CPU
        assert _conv()._dense_chain_f32([None] + PLANS[1:], _outs(n_dims=2), 0, params) is None
        assert _conv(act=torch.nn.ReLU)._dense_chain_f32([None] + PLANS[1:], _outs(n_dims=2), 0, params, regime='relu_width') is None
        pp = CINppConv(48, 48, 48, None, None, None, None, None, None, max_dim=2, hidden=48, act_module=torch.nn.ELU, layer_dim=48,
                       graph_norm=torch.nn.Identity, use_coboundaries=True).eval()
        assert pp._dense_chain_f32(PLANS, _outs()) is None
        assert pp._dense_chain_f32([['stream'] * 3] * 3, _outs() + _outs(n_dims=1)) is None
        for off in (frozenset(), False, frozenset({'relu_width'})):
            monkeypatch.setattr(layers, 'FUSED_CHAIN_F32', off)
            assert _conv()._dense_chain_f32(PLANS, _outs()) is None
        monkeypatch.setattr(layers, 'FUSED_CHAIN_F32', frozenset({'act'}))
        assert _conv()._dense_chain_f32(PLANS, _outs()) == ['launched'] * 3
        assert _conv(act=torch.nn.ReLU)._dense_chain_f32(PLANS, _outs(), regime='relu_width') is None
        monkeypatch.setattr(layers, 'FUSED_CHAIN_F32', True)
        assert _conv(act=torch.nn.ReLU)._dense_chain_f32(PLANS, _outs(), regime='relu_width') == ['launched'] * 3
        n_ok = len(launched)
    assert _conv()._dense_chain_f32(PLANS, _outs()) is None                                     # autograd is recording
    assert len(launched) == n_ok == 2


def test_route_touches_no_level_before_it_declines(launched):
    """CPU tensors and CINppConv are refused before any level is looked at (tests/test_dense_dispatch_host.py hands the
    dispatch fake plans and CPU zeros)."""
    class Untouchable:
        def __getitem__(self, d):
            raise AssertionError('a level was looked at')
    params = [SimpleNamespace(x=torch.zeros(2, 48)) for _ in range(3)]
    with torch.no_grad():
        conv = _conv()
        conv.__dict__['mp_levels'] = Untouchable()
        conv._modules.pop('mp_levels')
        for plans, n_outs in ((PLANS, 6), ([[None] * 2] * 3, 6), ([None] + PLANS[1:], 4)):
            assert conv._dense_chain_f32(plans, [torch.zeros(2, 48)] * n_outs, 0, params) is None
            assert conv._dense_chain_f32(plans, [torch.zeros(2, 48)] * n_outs, 0, params, regime='relu_width') is None


def test_launch_is_prepared_once_per_layer_and_follows_its_sources(launched):
    """ops.ChainLaunch is built on the first call and again only when a tensor it was derived from is written in place or
    moved, or the module tree changes; a training-mode BatchNorm declines without being remembered."""
    with torch.no_grad():
        conv = _conv(norm=torch.nn.BatchNorm1d)
        for _ in range(3):
            assert conv._dense_chain_f32(PLANS, _outs()) == ['launched'] * 3
        assert len(launched) == 1
        assert conv._dense_chain_f32(PLANS, _outs(), regime='relu_width') is None               # the other regime: read once, declined
        assert conv._dense_chain_f32(PLANS, _outs()) == ['launched'] * 3 and len(launched) == 1
        conv.mp_levels[1].combine_nn[0].bias.add_(1.0)
        assert conv._dense_chain_f32(PLANS, _outs()) == ['launched'] * 3 and len(launched) == 2
        conv.mp_levels[2].update_up_nn[1].running_var.mul_(2.0)
        assert conv._dense_chain_f32(PLANS, _outs()) == ['launched'] * 3 and len(launched) == 3
        scale = launched[-1][2].folds[0][0]
        bn = conv.mp_levels[2].update_up_nn[1]
        assert torch.allclose(scale, bn.weight * torch.rsqrt(bn.running_var + bn.eps))
        conv.mp_levels[0].update_up_nn[2] = torch.nn.Tanh()                                      # mixed activations in a network
        assert conv._dense_chain_f32(PLANS, _outs()) is None and len(launched) == 3
        conv.mp_levels[0].update_up_nn[2] = torch.nn.ELU()
        assert conv._dense_chain_f32(PLANS, _outs()) == ['launched'] * 3 and len(launched) == 4
        assert conv.train()._dense_chain_f32(PLANS, _outs()) is None
        assert conv.eval()._dense_chain_f32(PLANS, _outs()) == ['launched'] * 3
        assert conv._dense_chain_f32([None] + PLANS[1:], _outs(n_dims=2), 1) == ['launched'] * 2 and len(launched[-1]) == 2


# ---- the switch -----------------------------------------------------------------------------------------------------------
def test_the_switch_reads_its_regimes():
    both = frozenset({'relu_width', 'act'})
    assert layers.CHAIN_F32_REGIMES == both
    assert layers._chain_f32_switch('1') == both and layers._chain_f32_switch('0') == frozenset()
    assert layers._chain_f32_switch(None) is layers.FUSED_CHAIN_F32_DEFAULT <= both
    assert isinstance(layers.FUSED_CHAIN_F32_DEFAULT, frozenset)


def test_the_switch_follows_the_environment(value='0', want=()):
    """One child process: CWN_FUSED_CHAIN_F32=0 is read at import (what '1' and an unset variable give: `_chain_f32_switch`)."""
    env = {k: v for k, v in os.environ.items() if k != 'CWN_FUSED_CHAIN_F32'}
    if value is not None:
        env['CWN_FUSED_CHAIN_F32'] = value
    code = ('from cwn_amd import layers; print(sorted(layers.FUSED_CHAIN_F32)); print(sorted(layers.FUSED_CHAIN_F32_DEFAULT)); '
            'print([layers._chain_f32_on(r) for r in ("relu_width", "act")])')
    out = subprocess.run([os.sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True, check=True).stdout
    got, default, on = (eval(l) for l in out.strip().splitlines())
    assert got == list(want) and set(default) <= {'relu_width', 'act'}
    assert on == [r in got for r in ('relu_width', 'act')]
