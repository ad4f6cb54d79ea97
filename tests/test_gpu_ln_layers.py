"""Layers and models built with graph_norm='ln' on the grouped GEMM + LayerNorm launches (cwn_amd/dense_ln.py): against the
same layer / model after copy.deepcopy(...).double() on the same inputs (the float64 path: cwn_aggregate_f64 and the torch
modules), with tests/_product.gate as the bound; launch counts; the switch; captured training steps and static batches."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch.nn import BatchNorm1d as BN, LayerNorm as LN

from tests._product import dummy_batch, gate, list_names

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda:0')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _no_device_side_errors():
    yield
    from cwn_amd import csr
    csr.check_errors(DEV)


@pytest.fixture
def ln_launches(monkeypatch):
    """Counts the forward LayerNorm launches: [descriptors of call 1, ...]."""
    from cwn_amd import _ffi
    calls = []
    real = _ffi.layer_norm_act
    monkeypatch.setattr(_ffi, 'layer_norm_act', lambda descs, dev: (calls.append(len(descs)), real(descs, dev))[1])
    return calls


def _batches(F, dtype, which):
    """The mol dummy complexes / a ZINC-like batch of 8 with random features of width F in `dtype`, on the device."""
    from cwn_amd.synthetic import zinc_like_batch
    b = dummy_batch(list_names('mol'), max_dim=2) if which == 'dummy' else zinc_like_batch(8, seed=5)
    g = torch.Generator().manual_seed(7)
    for d in range(3):
        b.cochains[d].x = torch.randn(b.cochains[d].num_cells, F, generator=g).to(dtype)
    return b.to(DEV).prepare(backward=True)


def _conv(cls, F, norm=LN):
    from cwn_amd.layers import SparseCINConv
    torch.manual_seed(0)
    args = (F, F, F) + (None,) * (4 if cls is SparseCINConv else 6)
    conv = cls(*args, max_dim=2, hidden=F, act_module=torch.nn.ReLU, layer_dim=F, graph_norm=norm, use_coboundaries=True)
    with torch.no_grad():           # (a LayerNorm's affine starts as the identity: make it count)
        for m in conv.modules():
            if isinstance(m, (LN, BN)):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0.0, 0.3)
    return conv.to(DEV)


def _run(conv, b, train):
    """(outputs, gradients of the features, gradients of the parameters by name)."""
    params = b.get_all_cochain_params(max_dim=2, include_down_features=False)
    if not train:
        with torch.no_grad():
            return list(conv.eval()(*params)), None, None
    conv.train()
    conv.zero_grad(set_to_none=True)
    xs = [b.cochains[d].x.requires_grad_(True) for d in range(3)]
    for x in xs:
        x.grad = None
    outs = list(conv(*params))
    g = torch.Generator().manual_seed(3)
    torch.autograd.backward(outs, [torch.randn(o.shape, generator=g).to(o) for o in outs])
    return outs, [x.grad for x in xs], {n: p.grad for n, p in conv.named_parameters()}


def _layer_against_float64(cls, F, which, ln_launches):
    conv = _conv(cls, F)
    conv64 = copy.deepcopy(conv).double()
    b32, b64 = _batches(F, torch.float32, which), _batches(F, torch.float64, which)
    for train in (False, True):
        del ln_launches[:]
        outs, gx, gp = _run(conv, b32, train)
        # three stages (two of the update networks, one of the combine network), each ONE launch over every dimension and branch
        assert len(ln_launches) == 3, ln_launches
        ref, rx, rp = _run(conv64, b64, train)
        what = f'{cls.__name__} LN width {F} on {which} ({"training" if train else "eval"})'
        for d, (o, r) in enumerate(zip(outs, ref)):
            assert o.dtype == torch.float32 and r.dtype == torch.float64
            gate(o, r, f'{what}: output dim {d}')
        if train:
            for d, (a, r) in enumerate(zip(gx, rx)):
                gate(a, r, f'{what}: gradient of the features dim {d}')
            n_grads = 0
            for name, r in rp.items():
                if r is None:
                    assert gp[name] is None or float(gp[name].abs().max()) == 0.0, name
                    continue
                gate(gp[name], r, f'{what}: gradient of {name}')
                n_grads += 1
            assert n_grads >= 15 * 4


@pytest.mark.parametrize('which', ['dummy', 'zinc8'])
@pytest.mark.parametrize('F', [64, 160])
def test_sparse_cin_conv_with_layer_norm_against_float64(F, which, ln_launches):
    from cwn_amd.layers import SparseCINConv
    _layer_against_float64(SparseCINConv, F, which, ln_launches)


@pytest.mark.parametrize('which', ['dummy', 'zinc8'])
def test_cinpp_conv_with_layer_norm_against_float64(which, ln_launches):
    from cwn_amd.layers import CINppConv
    _layer_against_float64(CINppConv, 64, which, ln_launches)


@pytest.mark.parametrize('F', [64, 160])
def test_switch_off_is_the_torch_modules_bit_for_bit(F, ln_launches, monkeypatch):
    from cwn_amd import dense_ln
    from cwn_amd.layers import SparseCINConv
    conv = _conv(SparseCINConv, F)
    b = _batches(F, torch.float32, 'zinc8')
    monkeypatch.setattr(dense_ln, 'FUSED_LN', False)
    for train in (False, True):
        outs, gx, gp = _run(conv, b, train)
        assert ln_launches == []
        # the layer before this path existed: the aggregated streams through update_up_nn / update_boundaries_nn / combine_nn
        params = b.get_all_cochain_params(max_dim=2, include_down_features=False)
        with torch.set_grad_enabled(train):
            plans, streams = conv.propagate_all(*params)
            want = [conv.mp_levels[d].finish(streams[2 * d], streams[2 * d + 1]) for d in range(3)]
        for d, (o, w) in enumerate(zip(outs, want)):
            assert torch.equal(o, w), (train, d)
    monkeypatch.setattr(dense_ln, 'FUSED_LN', True)
    outs, _, _ = _run(conv, b, False)
    assert len(ln_launches) == 3
    for o, w in zip(outs, want):
        gate(o, w.double(), f'width {F}: grouped launches vs the torch modules in float32')


def test_batch_norm_layers_launch_no_layer_norm(ln_launches):
    from cwn_amd import _ffi
    from cwn_amd.layers import SparseCINConv
    conv = _conv(SparseCINConv, 64, norm=BN)
    b = _batches(64, torch.float32, 'zinc8')
    bwd = []
    real = _ffi.layer_norm_bwd
    _ffi.layer_norm_bwd = lambda descs, dev: (bwd.append(len(descs)), real(descs, dev))[1]
    try:
        for train in (False, True):
            outs, _, _ = _run(conv, b, train)
            assert all(torch.isfinite(o).all() for o in outs)
    finally:
        _ffi.layer_norm_bwd = real
    assert ln_launches == [] and bwd == []


# ---- the model of exp/scripts/cwn-csl.sh --------------------------------------------------------------------------------
def _csl_model(seed=0):
    from cwn_amd.models import EmbedSparseCIN
    torch.manual_seed(seed)
    model = EmbedSparseCIN(1, 1, 10, 3, 160, dropout_rate=0.0, max_dim=2, jump_mode=None, nonlinearity='relu', readout='mean',
                           final_readout='sum', apply_dropout_before='lin2', init_reduce='sum', embed_edge=True,
                           use_coboundaries=True, graph_norm='ln')
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, LN):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0.0, 0.3)
    return model.to(DEV)


def _csl_batch():
    from cwn_amd.complex import ComplexBatch
    from cwn_amd.synthetic import csl_graphs
    return ComplexBatch.from_complex_list(csl_graphs(12, seed=0, max_ring=8), max_dim=2).to(DEV)


def test_csl_model_forward_and_gradients_against_float64(ln_launches):
    model = _csl_model()
    model64 = copy.deepcopy(model).double()
    res = []
    for m in (model, model64):
        b = _csl_batch().prepare(backward=True)
        m.train()
        m.zero_grad(set_to_none=True)
        out = m(b)
        loss = torch.nn.functional.cross_entropy(out, b.y.view(-1))
        loss.backward()
        res.append((out, loss, {n: p.grad for n, p in m.named_parameters()}))
    assert len(ln_launches) == 3 * 3           # three layers, three stages each
    (out, loss, gp), (ref, rloss, rp) = res
    assert out.dtype == torch.float32 and ref.dtype == torch.float64
    gate(out, ref, 'CSL model (3 layers, width 160, ln, mean readout): logits')
    gate(loss.view(1), rloss.view(1), 'CSL model: cross-entropy')
    n = 0
    for name, r in rp.items():
        if r is None:
            continue
        gate(gp[name], r, f'CSL model: gradient of {name}')
        n += 1
    assert n > 100
    with torch.no_grad():
        gate(model.eval()(_csl_batch()), model64.eval()(_csl_batch()), 'CSL model: eval logits')


def test_csl_captured_training_step_equals_the_eager_step(ln_launches):
    """One TrainStep(use_graph=True) step against the eager step of the same model from the same state, with the bars
    tests/test_gpu_train_full.py has for the BatchNorm configurations: the loss within the gate, every gradient within
    2 x 1e-5 of max(1, |ref|_inf), the whole gradient within 2e-6 in relative L2, the parameters after Adam within 2e-3 lr."""
    from cwn_amd.train import TrainStep
    lr = 5e-4
    m1, m2 = _csl_model(), _csl_model()
    m2.load_state_dict(m1.state_dict())
    graph = TrainStep(m1, [_csl_batch()], task_type='classification', lr=lr, use_graph=True)
    eager = TrainStep(m2, [_csl_batch()], task_type='classification', lr=lr, use_graph=False)
    l1, l2 = graph.step(0), eager.step(0)
    torch.cuda.synchronize()
    assert len(ln_launches) >= 2 * 9           # (the LayerNorm launches were captured, not skipped)
    gate(l1.detach().view(1), l2.detach().view(1), 'CSL TrainStep: loss, captured vs eager')
    worst, d2, n2 = 0.0, 0.0, 0.0
    for (name, p), (_, q) in zip(m1.named_parameters(), m2.named_parameters()):
        if q.grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        g, r = p.grad.detach().double(), q.grad.detach().double()
        worst = max(worst, float((g - r).abs().max()) / max(1.0, float(r.abs().max())))
        d2, n2 = d2 + float(((g - r) ** 2).sum()), n2 + float((r ** 2).sum())
        assert float((p.detach() - q.detach()).abs().max()) <= 2e-3 * lr, name
    rel = (d2 / n2) ** 0.5
    print(f'[gate] CSL TrainStep: gradients captured vs eager: worst max|delta| / max(1, |ref|_inf) = {worst:.3e}, relative L2 = {rel:.3e}')
    assert worst <= 2e-5 and rel <= 2e-6, (worst, rel)
    assert torch.isfinite(graph.step(0)).all()          # a replay


def test_static_forward_with_layer_norm_equals_the_collated_batch(ln_launches):
    """A graph captured once over capacity-sized buffers: the LayerNorm launches take the device-side row counts, and rows
    beyond a slot's count do not reach the predictions."""
    from cwn_amd.models import EmbedSparseCIN
    from cwn_amd.packed import PackedComplexes
    from cwn_amd.static_batch import StaticBatch
    from cwn_amd.static_graph import StaticForward
    from cwn_amd.synthetic import zinc_like_complexes
    pool = zinc_like_complexes(60, seed=3, max_ring=6, n_lo=9, n_hi=28)
    p = PackedComplexes(pool, DEV, max_dim=2, with_csr=True)
    torch.manual_seed(0)
    model = EmbedSparseCIN(28, 4, 1, 2, 64, dropout_rate=0.0, max_dim=2, jump_mode=None, nonlinearity='relu', readout='sum',
                           final_readout='sum', init_reduce='sum', embed_edge=True, use_coboundaries=True, graph_norm='ln').to(DEV).eval()
    B = 24
    sf = StaticForward(model, StaticBatch(p, B))
    rng = np.random.default_rng(2)
    perm = rng.permutation(len(pool))
    with torch.no_grad():
        for idx in (perm[:B], perm[B:B + 7], perm[B + 7:B + 8], perm[B + 8:2 * B + 8]):
            got = sf.run(idx)[:len(idx)].clone()
            want = model(p.collate(idx))
            assert torch.isfinite(got).all()
            gate(got, want.double(), f'StaticForward with LayerNorm, {len(idx)} of {B} complexes')
    assert len(ln_launches) >= 6


def test_train_csl_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'train_csl.py'), '--epochs', '2', '--graphs', '30'],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('epoch ')]
    assert len(lines) == 2 and 'done: ' in out.stdout, out.stdout
    for l in lines:
        loss = float(l.split('train loss ')[1].split(',')[0])
        assert np.isfinite(loss), l
