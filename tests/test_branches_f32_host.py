"""The float32 update branches without a GPU (csrc/cwn_branches_f32.hip behind ops.update_branches_f32 and
CINppConv._dense_branches_f32): the symbol is declared, bound and exported under ABI 24, the ctypes record has the header's
layout, the launcher refuses every malformed descriptor before anything is launched, the predicate and the op refuse other
operands (naming the dtype), the layer's route declines what it must on CPU tensors, the switch reads its regimes, and
CINppCochainConv.forward_unfused is finish(*aggregate_unfused(...)) and still the formula it was."""
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
    assert re.search(r'\bint cwn_update_branches_f32\s*\(const cwn_branches_desc_f32\* descs_host, int n_dims, cwn_stream_t stream\)',
                     header)
    assert 'cwn_update_branches_f32' in _ffi.EXPORTS and hasattr(lib, 'cwn_update_branches_f32')
    assert lib.cwn_update_branches_f32.argtypes[0]._type_ is _ffi.BranchesDescF32
    assert lib.cwn_abi_version() == _ffi.ABI_VERSION == 24
    assert int(re.search(r'#define CWN_ABI_VERSION (\d+)', header).group(1)) == 24
    section = header[header.index('The float32 update branches'):header.index('int cwn_update_branches_f32')]
    for said in ('m_dev', 'CLAMPED', 'never written', 'All checks precede the first HIP call', 'OPERAND WINDOWS', 'training',
                 'widths above 128', 'compiled torch binding', 'float64', 'LayerNorm', 'feed_down_attr'):
        assert said in section, said
    assert 'cwn_branches_f32.hip' in open(os.path.join(ROOT, 'cwn_amd', 'csrc', 'Makefile')).read()
    # the section of the two-branch chain keeps its wording (tests/test_chain_f32_host.py reads it)
    assert header.index('The float32 update chain') < header.index('The float32 update branches')


def test_record_matches_the_header(tmp_path):
    """cwn_branches_desc_f32 field by field against the ctypes mirror, through a probe compiled with the host C compiler."""
    st, cname = _ffi.BranchesDescF32, 'cwn_branches_desc_f32'
    macros = ('CWN_BRANCHES_F32_MAX_DIMS', 'CWN_BRANCHES_F32_MAX_WIDTH', 'CWN_BRANCHES_F32_TM', 'CWN_BRANCHES_F32_MIN_BRANCHES',
              'CWN_BRANCHES_F32_MAX_BRANCHES', 'CWN_BRANCHES_F32_STAGES')
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cwn_hip.h"', 'int main(void) {',
             f'printf("size %zu\\n", sizeof({cname}));']
    lines += [f'printf("{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in st._fields_]
    lines += [f'printf("{m} %d\\n", {m});' for m in macros]
    lines += ['return 0; }']
    src, exe = tmp_path / 'probe.c', tmp_path / 'probe'
    src.write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got['size']) == ctypes.sizeof(st) == 400
    assert 4 * ctypes.sizeof(st) + 6 * 4 < 4096                      # the by-value launch record: four of them and the block table
    assert [f for f, _ in st._fields_] == ['ins', 'out', 'W', 'bias', 'scale', 'shift', 'n', 'ld_in', 'ld_out', 'F', 'H', 'act', 'nb',
                                           'm_dev']
    for f, _ in st._fields_:
        assert int(got[f]) == getattr(st, f).offset, f
    consts = (_ffi.BRANCHES_F32_MAX_DIMS, _ffi.BRANCHES_F32_MAX_WIDTH, _ffi.BRANCHES_F32_TM, _ffi.BRANCHES_F32_MIN_BRANCHES,
              _ffi.BRANCHES_F32_MAX_BRANCHES, _ffi.BRANCHES_F32_STAGES)
    assert consts == tuple(int(got[m]) for m in macros) == (4, 128, 32, 3, 4, 9)
    assert len(st().ins) == len(st().ld_in) == 4 and len(st().W) == len(st().bias) == len(st().scale) == len(st().shift) == 9


P = 0x100000


def _desc(edits=None, **kw):
    """A descriptor that passes every check (made-up, aligned addresses far apart: a call that passed the checks with rows
    would launch, so every case below breaks exactly one thing or has no rows)."""
    nb = {**kw, **(edits or {})}.get('nb', 3)
    d = _ffi.BranchesDescF32(out=3 * P, n=7, ld_out=20, F=12, H=20, act=_ffi.ACT_TANH, nb=nb, m_dev=60 * P)
    for k in range(4):
        d.ins[k], d.ld_in[k] = (50 + k) * P, 12
    for s in range(9):
        d.W[s], d.bias[s], d.scale[s], d.shift[s] = (4 + s) * P, (14 + s) * P, (24 + s) * P, (34 + s) * P
    for k, v in {**kw, **(edits or {})}.items():
        if isinstance(k, tuple):
            getattr(d, k[0])[k[1]] = v
        else:
            setattr(d, k, v)
    return d


def _call(*ds, n=None):
    return _ffi.lib().cwn_update_branches_f32((_ffi.BranchesDescF32 * len(ds))(*ds), len(ds) if n is None else n, None)


BAD = {
    'n<0': dict(n=-1), 'F=0': dict(F=0), 'F=129': {'F': 129, **{('ld_in', k): 129 for k in range(4)}}, 'H=0': dict(H=0),
    'H=129': dict(H=129, ld_out=129), 'act=-1': dict(act=-1), 'act=5': dict(act=5), 'nb=2': dict(nb=2), 'nb=5': dict(nb=5),
    'out NULL': dict(out=None), 'ld_out<H': dict(ld_out=19),
    **{f'ins[{k}] NULL': {('ins', k): None} for k in range(3)}, **{f'ld_in[{k}]<F': {('ld_in', k): 11} for k in range(3)},
    **{f'W[{s}] NULL': {('W', s): None} for s in range(7)},
    'ins[3] NULL, nb=4': {'nb': 4, ('ins', 3): None}, 'ld_in[3]<F, nb=4': {'nb': 4, ('ld_in', 3): 11},
    'W[7] NULL, nb=4': {'nb': 4, ('W', 7): None}, 'W[8] NULL, nb=4': {'nb': 4, ('W', 8): None},
}


@pytest.mark.parametrize('case', sorted(BAD))
def test_bad_arguments_are_refused_before_any_hip_call(case):
    assert _call(_desc(BAD[case])) == BAD_ARG, case
    assert _call(_desc(n=0), _desc(n=0, nb=4), _desc(BAD[case])) == BAD_ARG, case          # ... wherever it stands


def test_null_descriptors_counts_misaligned_pointers_and_too_many_tiles():
    assert _ffi.lib().cwn_update_branches_f32(None, 1, None) == BAD_ARG
    for n_dims in (0, -1, 5):
        assert _call(*[_desc(n=0) for _ in range(5)], n=n_dims) == BAD_ARG, n_dims
    assert _call(_desc(out=70 * P + 2)) == ALIGN
    for nb in (3, 4):
        for k in range(nb):
            assert _call(_desc({('ins', k): 70 * P + 2}, nb=nb)) == ALIGN, (nb, k)
        for field in ('W', 'bias', 'scale', 'shift'):
            for s in range(2 * nb + 1):
                assert _call(_desc({(field, s): 70 * P + 2}, nb=nb)) == ALIGN, (field, s, nb)
    assert _call(_desc(m_dev=70 * P + 4)) == ALIGN                         # the device count is an int64
    assert _call(_desc(F=0, out=P + 2)) == BAD_ARG                         # the argument checks come first
    assert _call(_desc(n=_ffi.BRANCHES_F32_TM * (2 ** 31 - 1))) == TOO_LARGE
    assert _call(_desc(n=_ffi.BRANCHES_F32_TM * 2 ** 30), _desc(n=_ffi.BRANCHES_F32_TM * 2 ** 30)) == TOO_LARGE      # ... in sum


def test_empty_launches_and_legal_shapes_are_ok_without_a_device():
    """Dimensions without rows return before the first HIP call and none of their pointers is looked at; every per-stage
    vector is optional on its own; the widths, the activation and the branch count are checked even then."""
    assert _call(_desc(n=0)) == OK
    assert _call(*[_desc(n=0, nb=3 + i % 2) for i in range(4)]) == OK
    assert _call(_desc({('ins', k): None for k in range(4)}, n=0, out=None, m_dev=None)) == OK
    assert _call(_desc({('W', 2): None, ('bias', 0): 3, ('scale', 1): None, ('shift', 6): None, ('ins', 0): 2}, n=0)) == OK
    for F, H in ((1, 128), (128, 1), (3, 5), (128, 128)):
        assert _call(_desc(n=0, F=F, H=H)) == OK
    assert _call(_desc(n=0, F=200)) == BAD_ARG
    assert _call(_desc(n=0, act=7)) == BAD_ARG
    assert _call(_desc(n=0, nb=2)) == BAD_ARG


# ---- the predicate and the op ---------------------------------------------------------------------------------------------
class OnGpu(torch.Tensor):               # a CPU tensor that says it is on the GPU: reaches the checks behind the device's
    @property
    def is_cuda(self):
        return True


def _branch_dim(F=16, H=16, n=5, nb=3, dtype=F32, **kw):
    t = lambda *s: torch.zeros(*s, dtype=dtype)
    f = dict(ins=[t(n, F) for _ in range(nb)], weights=[t(H, F), t(H, H)] * nb + [t(H, nb * H)], biases=[t(H)] * (2 * nb + 1),
             folds=[(None, None)] * (2 * nb + 1), act='elu')
    f.update(kw)
    return ops.BranchDim(**f)


def _gpu(d):
    as_gpu = lambda t: None if t is None else t.as_subclass(OnGpu)
    return ops.BranchDim(ins=[as_gpu(x) for x in d.ins], weights=[as_gpu(w) for w in d.weights], biases=[as_gpu(b) for b in d.biases],
                         folds=[(as_gpu(s), as_gpu(t)) for s, t in d.folds], act=d.act, out=as_gpu(d.out))


def test_predicate_declines_what_the_launch_does_not_take():
    ok = ops.update_branches_f32_applies
    assert ok([_gpu(_branch_dim())]) and ok([_gpu(_branch_dim(1, 128)), _gpu(_branch_dim(128, 128, n=0, nb=4)), _gpu(_branch_dim(5, 3))])
    assert ok([_gpu(_branch_dim(48, 48, nb=4, act=a)) for a in ('relu', 'tanh', 'sigmoid', 'id')])
    assert not ok([_branch_dim()])                                           # CPU tensors
    assert not ok([]) and not ok([_gpu(_branch_dim())] * 5)
    assert not ok([_gpu(_branch_dim(129, 16))]) and not ok([_gpu(_branch_dim(16, 129))])    # width 129
    assert not ok([_gpu(_branch_dim(dtype=torch.float64))])
    assert not ok([_gpu(_branch_dim(act='gelu'))])
    two = _branch_dim()
    two.ins = two.ins[:2]
    assert not ok([_gpu(two)])                                                              # two inputs for three branches
    t = lambda *s: torch.zeros(*s)
    assert not ok([_gpu(ops.BranchDim(ins=[t(5, 16)] * 2, weights=[t(16, 16)] * 4 + [t(16, 32)], biases=[None] * 5,
                                      folds=[(None, None)] * 5))])                          # two branches: the chain's
    assert not ok([_gpu(ops.BranchDim(ins=[t(5, 16)] * 5, weights=[t(16, 16)] * 10 + [t(16, 80)], biases=[None] * 11,
                                      folds=[(None, None)] * 11))])                         # five
    assert not ok([_gpu(_branch_dim(ins=[t(5, 16), t(4, 16), t(5, 16)]))])                  # row counts differ
    assert not ok([_gpu(_branch_dim(biases=[t(15)] * 7))])
    assert not ok([_gpu(_branch_dim(out=t(4, 16)))])                                        # fewer rows than n
    assert ok([_gpu(_branch_dim(out=t(9, 40)[:, :16]))])                                    # a row-strided view with room
    assert ok([_gpu(_branch_dim(ins=[t(5, 40)[:, 8:24], t(5, 16), t(5, 17)[:, 1:]]))])
    assert not ok([_gpu(_branch_dim(ins=[t(16, 5).t(), t(5, 16), t(5, 16)]))])              # rows not contiguous
    half = [(t(16), None), (None, t(16))] + [(None, None)] * 5                              # scale and shift: each on its own
    assert ok([_gpu(_branch_dim(folds=half))])
    w = _branch_dim().weights
    w[6] = t(16, 96)[:, :48]                                                                # combine weight not contiguous
    assert not ok([_gpu(_branch_dim(weights=w))])
    w = _branch_dim(nb=4).weights
    w[8] = t(16, 48)                                                                        # a 3H-wide combine for four branches
    assert not ok([_gpu(_branch_dim(nb=4, weights=w))])


def test_op_refuses_other_operands_by_naming_the_dtype():
    t = lambda *s, **k: torch.zeros(*s, **k)
    with pytest.raises(TypeError, match='float64'):
        ops.update_branches_f32([_branch_dim(dtype=torch.float64)])
    with pytest.raises(TypeError, match='float16'):
        ops.update_branches_f32([_gpu(_branch_dim(ins=[t(5, 16), t(5, 16, dtype=torch.float16), t(5, 16)]))])
    with pytest.raises(TypeError, match=r'float32.*cpu'):
        ops.update_branches_f32([_branch_dim()])                                            # float32, but not on the GPU
    with pytest.raises(TypeError, match='contiguous rows'):
        ops.update_branches_f32([_gpu(_branch_dim(ins=[t(16, 5).t(), t(5, 16), t(5, 16)]))])
    with pytest.raises(ValueError, match='3 or 4 branches'):
        ops.update_branches_f32([_gpu(_branch_dim(129, 16))])
    with pytest.raises(ValueError, match='3 or 4 branches'):
        ops.update_branches_f32([_gpu(_branch_dim(ins=[t(5, 16), t(4, 16), t(5, 16)]))])
    with pytest.raises(ValueError, match='3 or 4 branches'):
        ops.update_branches_f32([_gpu(_branch_dim())] * 5)


# ---- the route on the layer, on CPU tensors -------------------------------------------------------------------------------
def _conv(hidden=48, layer_dim=None, norm=torch.nn.Identity, act=torch.nn.ELU, dtype=F32, cob=False, **kw):
    layer_dim = hidden if layer_dim is None else layer_dim
    conv = CINppConv(layer_dim, layer_dim, layer_dim, None, None, None, kw.pop('up_nn', None), None, None, max_dim=2, hidden=hidden,
                     act_module=act, layer_dim=layer_dim, graph_norm=norm, use_coboundaries=True, coboundary_stream=cob, **kw)
    return conv.to(dtype).eval()


def _outs(width=48, dtype=F32, n_dims=3, nb=3):
    return [torch.zeros(4, width, dtype=dtype).as_subclass(OnGpu) for _ in range(nb * n_dims)]


PLANS = [['stream'] * 3] * 3
PLANS4 = [['stream'] * 4] * 3
RELU = torch.nn.ReLU


@pytest.fixture
def launched(monkeypatch):
    """The dimensions every prepared launch was built from; its run is replaced (there is no device here), its validity check
    is the real one."""
    built = []

    class Launch(ops.BranchesLaunch):
        def __init__(self, dims, sources):
            super().__init__(dims, sources)
            built.append(dims)

        def run(self, ins):
            assert len(ins) == self.n and [len(xs) for xs in ins] == [nb for _, _, nb in self.shapes]
            return ['launched'] * self.n
    monkeypatch.setattr(ops, 'BranchesLaunch', Launch)
    monkeypatch.setattr(ops, 'update_branches_f32_applies', lambda dims: True)
    monkeypatch.setattr(layers, 'FUSED_BRANCHES_F32', layers.BRANCHES_F32_REGIMES)
    return built


def test_route_takes_the_stock_networks_of_its_regime(launched):
    with torch.no_grad():
        for act in (torch.nn.ELU, torch.nn.Tanh, torch.nn.Sigmoid, torch.nn.Identity):
            for hidden in (16, 48, 64, 128):
                assert _conv(hidden, act=act)._dense_branches_f32(PLANS, _outs(hidden)) == ['launched'] * 3
        assert [d.act for d in launched[-1]] == ['id'] * 3 and [len(d.ins) for d in launched[-1]] == [3] * 3
        assert _conv(64, cob=True)._dense_branches_f32(PLANS4, _outs(64, nb=4)) == ['launched'] * 3
        assert [len(d.ins) for d in launched[-1]] == [4] * 3 and [len(d.weights) for d in launched[-1]] == [9] * 3
        assert tuple(launched[-1][0].weights[8].shape) == (64, 256)
        assert _conv(act=RELU)._dense_branches_f32(PLANS, _outs()) is None                      # ReLU is not the 'act' regime
        for hidden in (16, 48, 100):
            assert _conv(hidden, act=RELU)._dense_branches_f32(PLANS, _outs(hidden), regime='relu_width') == ['launched'] * 3
        # a first layer with F != H, and four branches at 64 / 128: not cwn_update_mlp3_f32's
        assert _conv(64, layer_dim=100, act=RELU)._dense_branches_f32(PLANS, _outs(100), regime='relu_width') == ['launched'] * 3
        assert _conv(64, layer_dim=16, act=RELU)._dense_branches_f32(PLANS, _outs(16), regime='relu_width') == ['launched'] * 3
        for hidden in (64, 128):
            assert _conv(hidden, act=RELU, cob=True)._dense_branches_f32(PLANS4, _outs(hidden, nb=4), regime='relu_width') == ['launched'] * 3
        n_ok = len(launched)
        for hidden in (64, 128):             # three ReLU branches at 64 / 128 with (F, F) first layers keep cwn_update_mlp3_f32
            assert _conv(hidden, act=RELU)._dense_branches_f32(PLANS, _outs(hidden), regime='relu_width') is None
        assert _conv(act=torch.nn.ELU)._dense_branches_f32(PLANS, _outs(), regime='relu_width') is None
        bn = _conv(norm=torch.nn.BatchNorm1d)
        assert bn._dense_branches_f32(PLANS, _outs()) == ['launched'] * 3                       # eval-mode BatchNorm folds
        assert all(s is not None and s.dtype == F32 and t is not None for s, t in launched[-1][0].folds)
        dims, lvl = launched[-1], bn.mp_levels[1]
        order = (lvl.update_up_nn[0], lvl.update_up_nn[3], lvl.update_down_nn[0], lvl.update_down_nn[3], lvl.update_boundaries_nn[0],
                 lvl.update_boundaries_nn[3], lvl.combine_nn[0])
        assert [w is m.weight for w, m in zip(dims[1].weights, order)] == [True] * 7            # the order of torch.cat
        assert len(launched) == n_ok + 1
        # the blocked propagate's three outputs per dimension, and from a later dimension on (start_to_process)
        assert _conv()._dense_branches_f32(['blocked'] * 3, _outs()) == ['launched'] * 3
        assert _conv()._dense_branches_f32([None] + PLANS[1:], _outs(n_dims=2), 1) == ['launched'] * 2


def test_route_declines_on_the_layer(launched, monkeypatch):
    """None -- the caller goes on exactly as before -- for a width above 128, LayerNorm, a training-mode BatchNorm, a passed-in
    network of another form, float64 and CPU features, more than 4 dimensions, a SparseCINConv, an unfused dimension without
    its parameters, in the ReLU regime or under a static batch, a recording autograd and the switch."""
    with torch.no_grad():
        assert _conv(129)._dense_branches_f32(PLANS, _outs(129)) is None
        assert _conv(16, layer_dim=129)._dense_branches_f32(PLANS, _outs(129)) is None
        assert _conv(norm=torch.nn.LayerNorm)._dense_branches_f32(PLANS, _outs()) is None
        assert _conv(norm=torch.nn.BatchNorm1d).train()._dense_branches_f32(PLANS, _outs()) is None
        custom = torch.nn.Sequential(torch.nn.Linear(48, 48), torch.nn.ELU())
        assert _conv(up_nn=custom)._dense_branches_f32(PLANS, _outs()) is None
        assert _conv(dtype=torch.float64)._dense_branches_f32(PLANS, _outs(dtype=torch.float64)) is None
        assert _conv(dtype=torch.float64)._dense_branches_f32(PLANS, _outs()) is None          # float64 networks
        assert _conv()._dense_branches_f32(PLANS, [torch.zeros(4, 48)] * 9) is None            # CPU features
        assert _conv()._dense_branches_f32(PLANS, _outs(n_dims=2)) is None                      # not three matrices per dimension
        assert _conv()._dense_branches_f32(PLANS4, _outs()) is None
        five = CINppConv(48, 48, 48, None, None, None, None, None, None, max_dim=4, hidden=48, act_module=torch.nn.ELU, layer_dim=48,
                         graph_norm=torch.nn.Identity, use_coboundaries=True).eval()
        assert five._dense_branches_f32([['stream'] * 3] * 5, _outs(n_dims=5)) is None          # five dimensions
        plain = SparseCINConv(48, 48, 48, None, None, None, None, max_dim=2, hidden=48, act_module=torch.nn.ELU, layer_dim=48,
                              graph_norm=torch.nn.Identity, use_coboundaries=True).eval()
        assert plain._dense_branches_f32(PLANS, _outs()) is None
        assert plain._dense_branches_f32([['stream'] * 2] * 3, _outs(nb=2)) is None
        # an unfused dimension: its parameters are needed, its features on the GPU, the regime 'act', no static batch
        assert _conv()._dense_branches_f32([None] + PLANS[1:], _outs(n_dims=2)) is None
        params = [SimpleNamespace(x=torch.zeros(4, 48)) for _ in range(3)]                      # ... whose features are on the CPU
        assert _conv()._dense_branches_f32([None] + PLANS[1:], _outs(n_dims=2), 0, params) is None
        gparams = [SimpleNamespace(x=torch.zeros(4, 48).as_subclass(OnGpu)) for _ in range(3)]
        assert _conv(act=RELU)._dense_branches_f32([None] + PLANS[1:], _outs(n_dims=2), 0, gparams, regime='relu_width') is None
        conv = _conv()
        for lvl in conv.mp_levels:
            lvl.aggregate_unfused = lambda cochain: tuple(_outs(n_dims=1))
        assert conv._dense_branches_f32([None] + PLANS[1:], _outs(n_dims=2), 0, gparams) == ['launched'] * 3
        with _ffi.dynamic_rows({4: 64}):
            assert conv._dense_branches_f32([None] + PLANS[1:], _outs(n_dims=2), 0, gparams) is None   # a static batch
            assert conv._dense_branches_f32(PLANS, _outs()) == ['launched'] * 3
        for off in (frozenset(), False, frozenset({'relu_width'})):
            monkeypatch.setattr(layers, 'FUSED_BRANCHES_F32', off)
            assert _conv()._dense_branches_f32(PLANS, _outs()) is None
        monkeypatch.setattr(layers, 'FUSED_BRANCHES_F32', frozenset({'act'}))
        assert _conv()._dense_branches_f32(PLANS, _outs()) == ['launched'] * 3
        assert _conv(act=RELU)._dense_branches_f32(PLANS, _outs(), regime='relu_width') is None
        monkeypatch.setattr(layers, 'FUSED_BRANCHES_F32', True)
        assert _conv(act=RELU)._dense_branches_f32(PLANS, _outs(), regime='relu_width') == ['launched'] * 3
        n_ok = len(launched)
    assert _conv()._dense_branches_f32(PLANS, _outs()) is None                                  # autograd is recording
    assert len(launched) == n_ok == 3


def test_route_touches_no_level_before_it_declines(launched):
    """CPU tensors are refused before any level is looked at (tests/test_dense_dispatch_host.py hands the dispatch fake plans
    and CPU zeros)."""
    class Untouchable:
        def __getitem__(self, d):
            raise AssertionError('a level was looked at')
    params = [SimpleNamespace(x=torch.zeros(2, 48)) for _ in range(3)]
    with torch.no_grad():
        conv = _conv()
        conv.__dict__['mp_levels'] = Untouchable()
        conv._modules.pop('mp_levels')
        for plans, n_outs in ((PLANS, 9), (['blocked'] * 3, 9), ([None] + PLANS[1:], 6)):
            assert conv._dense_branches_f32(plans, [torch.zeros(2, 48)] * n_outs, 0, params) is None
            assert conv._dense_branches_f32(plans, [torch.zeros(2, 48)] * n_outs, 0, params, regime='relu_width') is None


def test_launch_is_prepared_once_per_layer_and_follows_its_sources(launched):
    """ops.BranchesLaunch is built on the first call and again only when a tensor it was derived from is written in place or
    moved, or the module tree changes; a training-mode BatchNorm declines without being remembered."""
    with torch.no_grad():
        conv = _conv(norm=torch.nn.BatchNorm1d, cob=True)
        for _ in range(3):
            assert conv._dense_branches_f32(PLANS4, _outs(nb=4)) == ['launched'] * 3
        assert len(launched) == 1
        assert conv._dense_branches_f32(PLANS4, _outs(nb=4), regime='relu_width') is None       # the other regime: read once, declined
        assert conv._dense_branches_f32(PLANS4, _outs(nb=4)) == ['launched'] * 3 and len(launched) == 1
        conv.mp_levels[1].combine_nn[0].bias.add_(1.0)
        assert conv._dense_branches_f32(PLANS4, _outs(nb=4)) == ['launched'] * 3 and len(launched) == 2
        conv.mp_levels[2].update_coboundaries_nn[1].running_var.mul_(2.0)                        # the fourth branch's norm
        assert conv._dense_branches_f32(PLANS4, _outs(nb=4)) == ['launched'] * 3 and len(launched) == 3
        scale = launched[-1][2].folds[6][0]
        bn = conv.mp_levels[2].update_coboundaries_nn[1]
        assert torch.allclose(scale, bn.weight * torch.rsqrt(bn.running_var + bn.eps))
        conv.mp_levels[0].update_down_nn[2] = torch.nn.Tanh()                                    # mixed activations in a network
        assert conv._dense_branches_f32(PLANS4, _outs(nb=4)) is None and len(launched) == 3
        conv.mp_levels[0].update_down_nn[2] = torch.nn.ELU()
        assert conv._dense_branches_f32(PLANS4, _outs(nb=4)) == ['launched'] * 3 and len(launched) == 4
        assert conv.train()._dense_branches_f32(PLANS4, _outs(nb=4)) is None
        assert conv.eval()._dense_branches_f32(PLANS4, _outs(nb=4)) == ['launched'] * 3
        assert conv._dense_branches_f32([None] + PLANS4[1:], _outs(n_dims=2, nb=4), 1) == ['launched'] * 2 and len(launched[-1]) == 2


# ---- the switch -----------------------------------------------------------------------------------------------------------
def test_the_switch_reads_its_regimes():
    both = frozenset({'relu_width', 'act'})
    assert layers.BRANCHES_F32_REGIMES == both
    assert layers._branches_f32_switch('1') == both and layers._branches_f32_switch('0') == frozenset()
    assert layers._branches_f32_switch(None) is layers.FUSED_BRANCHES_F32_DEFAULT <= both
    assert isinstance(layers.FUSED_BRANCHES_F32_DEFAULT, frozenset)


@pytest.mark.parametrize('value', ['0', '1', None])
def test_the_switch_follows_the_environment(value):
    """A child process: CWN_FUSED_BRANCHES_F32 is read at import; unset gives the default; FUSED_CHAIN_F32 is another switch."""
    env = {k: v for k, v in os.environ.items() if k != 'CWN_FUSED_BRANCHES_F32'}
    if value is not None:
        env['CWN_FUSED_BRANCHES_F32'] = value
    code = ('from cwn_amd import layers; print(sorted(layers.FUSED_BRANCHES_F32)); print(sorted(layers.FUSED_BRANCHES_F32_DEFAULT)); '
            'print([layers._branches_f32_on(r) for r in ("relu_width", "act")]); print(sorted(layers.FUSED_CHAIN_F32))')
    out = subprocess.run([os.sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True, check=True).stdout
    got, default, on, chain = (eval(l) for l in out.strip().splitlines())
    want = {'0': [], '1': ['act', 'relu_width'], None: default}[value]
    assert got == want and set(default) <= {'relu_width', 'act'}
    assert on == [r in got for r in ('relu_width', 'act')]
    assert chain == sorted(layers.FUSED_CHAIN_F32)


# ---- CINppCochainConv.forward_unfused = finish(*aggregate_unfused(...)) -------------------------------------------------------
def _sum_to(index, src, n):
    """out[i] = sum of src[j] over the entries (j, i) of a [2, E] index, on the CPU."""
    out = torch.zeros(n, src.size(1), dtype=src.dtype)
    return out.index_add_(0, index[1], src[index[0]])


@pytest.mark.parametrize('cob,cob_index', [(False, False), (True, True), (True, False)],
                         ids=['three-streams', 'four-streams', 'four-streams-no-coboundary-index'])
def test_forward_unfused_is_finish_of_aggregate_unfused_and_the_formula_it_was(monkeypatch, cob, cob_index):
    """A small complex on the CPU: 6 edges with upper and boundary adjacencies, 3 rings above them.  propagate() and
    propagate_coboundary() aggregate on the device, so here they are replaced by the same sums on torch's index_add_ -- the
    split under test is everything around them: the self terms with eps1 .. eps4, the zeros of an absent co-boundary index,
    the order of the branches in torch.cat."""
    torch.manual_seed(3)
    n, H = 6, 8
    conv = CINppConv(H, H, H, None, None, None, None, None, None, max_dim=2, hidden=H, act_module=torch.nn.Tanh, layer_dim=H,
                     graph_norm=torch.nn.Identity, use_coboundaries=False, coboundary_stream=cob, train_eps=True).eval()
    lvl = conv.mp_levels[1]
    with torch.no_grad():
        for k, eps in enumerate([lvl.eps1, lvl.eps2, lvl.eps3] + ([lvl.eps4] if cob else [])):
            eps.fill_(0.1 * (k + 1))
    x, b_attr, c_attr = torch.randn(n, H), torch.randn(5, H), torch.randn(3, H)
    up = torch.tensor([[0, 1, 1, 2, 4, 5], [1, 0, 2, 1, 5, 4]])
    bnd = torch.tensor([[0, 1, 1, 2, 3, 4, 4, 0], [0, 0, 1, 1, 2, 3, 5, 5]])
    cobi = torch.tensor([[0, 1, 2, 2, 1], [0, 0, 1, 3, 5]])                  # (ring, edge) pairs as (source, destination)
    cochain = SimpleNamespace(x=x, up_index=up, down_index=None, boundary_index=bnd, kwargs=dict(up_attr=None, boundary_attr=b_attr),
                              coboundary_index=cobi if cob_index else None, coboundary_attr=c_attr if cob_index else None)
    calls = []

    def propagate(up_index, down_index, boundary_index, **kw):
        calls.append(sorted(kw))
        assert down_index is None and kw['x'] is x
        return _sum_to(up_index, x, n), torch.zeros(n, H), _sum_to(boundary_index, kw['boundary_attr'], n)
    monkeypatch.setattr(lvl, 'propagate', propagate)
    monkeypatch.setattr(lvl, 'propagate_coboundary', lambda index, attr, n_cells: _sum_to(index, attr, n_cells))
    monkeypatch.setattr(ops, 'zeros_rows', lambda rows, width, device, dtype: torch.zeros(rows, width, dtype=dtype))
    with torch.no_grad():
        parts = lvl.aggregate_unfused(cochain)
        assert len(parts) == (4 if cob else 3) and all(p.shape == (n, H) for p in parts)
        got = lvl.forward_unfused(cochain)
        assert torch.equal(got, lvl.finish(*parts))
        # the formula of forward_unfused before the split (mp/layers.py:243-260 + the fourth stream), restated
        out_up = _sum_to(up, x, n) + (1 + lvl.eps1) * x
        out_down = torch.zeros(n, H) + (1 + lvl.eps2) * x
        out_b = _sum_to(bnd, b_attr, n) + (1 + lvl.eps3) * x
        want = [lvl.update_up_nn(out_up), lvl.update_down_nn(out_down), lvl.update_boundaries_nn(out_b)]
        if cob:
            out_cob = _sum_to(cobi, c_attr, n) if cob_index else torch.zeros(n, H)
            want.append(lvl.update_coboundaries_nn(out_cob + (1 + lvl.eps4) * x))
        assert torch.equal(got, lvl.combine_nn(torch.cat(want, dim=-1)))
        for p, w in zip(parts, (out_up, out_down, out_b)):
            assert torch.equal(p, w)
    assert calls and all(c == ['boundary_attr', 'up_attr', 'x'] for c in calls)           # no down_attr without feed_down_attr
