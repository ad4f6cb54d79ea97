"""Captured training steps for graph_norm='ln' models over a static batch (StaticTrainStep / StaticBatch(mode='csr')), up to the
reference's CSL configuration (width 160: the 320-wide combine product on csrc/cwn_linear_wide.hip).

The comparison and its bars are the ones tests/test_gpu_linear_stats.py applies to the same static-against-eager comparison
for BatchNorm (_steps_against_per_batch_steps): StaticTrainStep.step_on against TrainStep(use_graph=False) on
packed.collate(idx) from ONE state per step; the loss within 1e-5 * max(1, |ref|), the whole gradient within 2e-5 in relative
L2.  Here every single gradient (max|delta| <= 2e-5 * max(1, |ref|_inf), the per-gradient bar of
tests/test_gpu_ln_layers.py's captured step) and the parameters after Adam (relative L2 2e-5) are held to them as well.
Every figure is printed before it is asserted."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cwn_amd import _ffi, dense_ln, ops

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda', 0)
B = 12
LN = torch.nn.LayerNorm


def _randomise_norms(model):
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, LN):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0.0, 0.3)
    return model


def _csl_model(seed=0):
    from tests.test_gpu_ln_layers import _csl_model as make          # width 160, 3 layers, readout='mean'
    return make(seed)


def _zinc_model(hidden=48, seed=4):
    from cwn_amd.models import EmbedSparseCIN
    torch.manual_seed(seed)
    return _randomise_norms(EmbedSparseCIN(28, 4, 1, 2, hidden, dropout_rate=0.0, max_dim=2, embed_edge=True, use_coboundaries=True,
                                           graph_norm='ln')).to(DEV)


@functools.lru_cache(maxsize=None)
def _csl():
    from cwn_amd.packed import PackedComplexes
    from cwn_amd.synthetic import csl_graphs
    pool = csl_graphs(30, seed=0, max_ring=8)
    return pool, PackedComplexes(pool, DEV, max_dim=2, with_csr=True)


@functools.lru_cache(maxsize=None)
def _zinc():
    from cwn_amd.packed import PackedComplexes
    from cwn_amd.synthetic import zinc_like_complexes
    pool = zinc_like_complexes(60, n_lo=9, n_hi=28)
    return pool, PackedComplexes(pool, DEV, max_dim=2, with_csr=True)


def _sequence(n, seed=13):
    """12, then 5, then 1, then 12 complexes: from the second step on stale rows of a larger batch lie behind a smaller one."""
    perm = np.random.default_rng(seed).permutation(n)
    return [perm[:12], perm[12:17], perm[17:18], perm[18:30]]


def _static_against_collated(make, p, task, batches, lr=5e-4, mode='csr'):
    from cwn_amd import csr
    from cwn_amd.static_batch import StaticBatch
    from cwn_amd.static_graph import StaticTrainStep
    from cwn_amd.train import TrainStep
    m1, m2 = make(), make()
    m2.load_state_dict(m1.state_dict())
    sb = StaticBatch(p, B, slots=1, mode=mode)
    sb.set_batch(batches[0])
    st = StaticTrainStep(m1, sb, task_type=task, lr=lr)
    ref = TrainStep(m2, [p.collate(idx) for idx in batches], task_type=task, lr=lr, use_graph=False)
    for j, idx in enumerate(batches):
        l1 = st.step_on([idx])[0].clone()
        l2 = ref.step(j)
        torch.cuda.synchronize()
        g1, g2 = st.bucket.flat, ref.bucket.flat
        rel = float((g1 - g2).norm() / g2.norm())
        rel_p = float((st.opt.flat_p - ref.opt.flat_p).norm() / ref.opt.flat_p.norm())
        worst, who = 0.0, None
        for (name, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
            if b.grad is None:
                continue
            assert torch.isfinite(a.grad).all(), (j, name)
            w = float((a.grad - b.grad).abs().max()) / max(1.0, float(b.grad.abs().max()))
            if w > worst:
                worst, who = w, name
        print(f'[static ln] step {j} ({len(idx)} complexes): loss {float(l1):.6f} vs {float(l2):.6f}; whole gradient relative L2 '
              f'{rel:.2e}; worst gradient max|delta| / max(1, |ref|_inf) {worst:.2e} ({who}); parameters after Adam relative L2 '
              f'{rel_p:.2e}')
        assert abs(float(l1) - float(l2)) <= 1e-5 * max(1.0, abs(float(l2))), (j, float(l1), float(l2))
        assert rel < 2e-5, (j, rel)
        assert worst <= 2e-5, (j, who, worst)
        assert rel_p < 2e-5, (j, rel_p)
        ref.opt.flat_p.copy_(st.opt.flat_p)
        ref.opt.exp_avg.copy_(st.opt.exp_avg)
        ref.opt.exp_avg_sq.copy_(st.opt.exp_avg_sq)
    csr.check_errors(DEV)
    assert len(st._graphs) == 1
    return st, m1


class _Spy:
    """Counts the calls of entry points of the library (the ctypes functions the wrappers look up on every call)."""

    def __init__(self, monkeypatch, *names):
        self.n = {k: 0 for k in names}
        L = _ffi.lib()
        for k in names:
            monkeypatch.setattr(L, k, self._wrap(k, getattr(L, k)), raising=True)

    def _wrap(self, k, fn):
        def call(*a):
            self.n[k] += 1
            return fn(*a)
        return call


def test_csl_model_at_width_160_static_against_collated_eager(monkeypatch):
    """The model of exp/scripts/cwn-csl.sh on csl_graphs, batches of 12, 5, 1 and 12 through ONE captured graph.  Without
    ops.linear_wide the combine product Linear(320 -> 160) is torch.cat + linear, whose backward sums dW / db over the
    capacity rows of the slot -- rows cwn_layernorm_bwd_f32 never wrote.  Measured on the commit before: the first step (a full
    batch) agrees, the step on 5 complexes behind it has a whole-gradient relative L2 distance of 2.85e+02, the worst single
    gradient convs.1.mp_levels.0.combine_nn.0.bias."""
    spy = _Spy(monkeypatch, 'cwn_linear_wide_f32')
    pool, p = _csl()
    _static_against_collated(_csl_model, p, 'classification', _sequence(len(pool)))
    print('[static ln] launches recorded:', spy.n)
    assert spy.n['cwn_linear_wide_f32'] > 0


def test_zinc_like_model_at_width_48_static_against_collated_eager(monkeypatch):
    """An ln EmbedSparseCIN at hidden 48: the combine on the grouped GEMM, as before."""
    spy = _Spy(monkeypatch, 'cwn_linear_wide_f32')
    pool, p = _zinc()
    _static_against_collated(lambda: _zinc_model(48), p, 'regression', _sequence(len(pool)))
    assert spy.n['cwn_linear_wide_f32'] == 0, spy.n


@pytest.mark.parametrize('hidden', [64, 128])
def test_blocked_mode_at_64_and_128_static_against_collated_eager(hidden):
    """mode='blocked' (the complex-blocked layer launches) with LayerNorm at its two widths: count-correct as it stood, served."""
    pool, p = _zinc()
    _static_against_collated(lambda: _zinc_model(hidden), p, 'regression', _sequence(len(pool))[:3], mode='blocked')


def test_routed_train_step_runs_an_epoch_with_layer_norm():
    from cwn_amd import csr
    from cwn_amd.static_graph import RoutedTrainStep, StaticRouter
    pool, p = _zinc()
    step = RoutedTrainStep(_zinc_model(64), StaticRouter(p, batch_size=B, slots=2), task_type='regression', lr=5e-4)
    perm = np.random.default_rng(2).permutation(len(pool))
    batches = [perm[:12], perm[12:24], perm[24:29]]
    losses = [float(l) for l in step.run_epoch(batches)]
    csr.check_errors(DEV)
    print('[static ln] RoutedTrainStep losses:', losses)
    assert len(losses) == 3 and all(np.isfinite(l) for l in losses) and int(step.opt.t) == 3


@functools.lru_cache(maxsize=None)
def _raw(width=7):
    """Ring-lifted molecules with `width` raw float features on every cell (what SparseCIN takes as given)."""
    from cwn_amd.packed import PackedComplexes
    from cwn_amd.synthetic import random_molecule, ring_lift
    rng, g = np.random.default_rng(5), torch.Generator().manual_seed(5)
    rand = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32)
    pool = []
    for _ in range(30):
        n, bonds = random_molecule(rng, 9, 28)
        cx = ring_lift(n, bonds, rand(n, width), rand(len(bonds), width), max_k=6, y=rand(1))
        if cx.dimension >= 2:
            cx.cochains[2].x = rand(cx.cochains[2].num_cells, width)
        pool.append(cx)
    return pool, PackedComplexes(pool, DEV, max_dim=2, with_csr=True)


@functools.lru_cache(maxsize=None)
def _molhiv():
    from cwn_amd.packed import PackedComplexes
    from cwn_amd.synthetic import molhiv_like_complexes
    pool = molhiv_like_complexes(30, 7, 6, n_lo=9, n_hi=28)
    g = torch.Generator().manual_seed(0)
    for c in pool:
        c.y = torch.randn(1, 1, generator=g)
    return pool, PackedComplexes(pool, DEV, max_dim=2, with_csr=True)


@pytest.mark.parametrize('kind', ['SparseCIN', 'OGBEmbedSparseCIN', 'EmbedSparseCINNoRings'])
def test_the_other_model_classes_with_layer_norm_static_against_collated_eager(kind):
    """SparseCIN over 7 raw features (a first layer 7 -> 64), OGBEmbedSparseCIN (the OGB encoders, mean readout) and
    EmbedSparseCINNoRings (vertices and edges only) with graph_norm='ln' at hidden 64, over StaticBatch(mode='csr')."""
    from cwn_amd.models import EmbedSparseCINNoRings, OGBEmbedSparseCIN, SparseCIN

    def make():
        torch.manual_seed(4)
        if kind == 'SparseCIN':
            m = SparseCIN(7, 1, 2, 64, dropout_rate=0.0, max_dim=2, graph_norm='ln')
        elif kind == 'OGBEmbedSparseCIN':
            m = OGBEmbedSparseCIN(1, 2, 64, dropout_rate=0.0, max_dim=2, readout='mean', final_readout='sum', init_reduce='sum',
                                  embed_edge=True, use_coboundaries=True, graph_norm='ln')
        else:
            m = EmbedSparseCINNoRings(28, 4, 1, 2, 64, dropout_rate=0.0, embed_edge=True, use_coboundaries=True, graph_norm='ln')
        return _randomise_norms(m).to(DEV)

    pool, p = {'SparseCIN': _raw, 'OGBEmbedSparseCIN': _molhiv, 'EmbedSparseCINNoRings': _zinc}[kind]()
    _static_against_collated(make, p, 'regression', _sequence(len(pool), seed=17)[:3])


def test_eager_layer_norm_model_at_a_width_that_is_no_multiple_of_4_against_float64(monkeypatch):
    """hidden 6: cwn_gemm_f32 refuses X2 behind a K that is no multiple of 4 (the combine of such a layer used to end in
    'bad argument'); the combine takes cwn_linear_wide_f32, forward and backward, within the gate of float64."""
    import copy
    from tests._product import gate
    spy = _Spy(monkeypatch, 'cwn_linear_wide_f32')
    pool, p = _zinc()
    model = _zinc_model(6)
    model64 = copy.deepcopy(model).double()
    idx = np.arange(12)
    res = []
    for m in (model, model64):
        b = p.collate(idx).prepare(backward=True)
        m.train()
        m.zero_grad(set_to_none=True)
        out = m(b)
        out.square().mean().backward()
        res.append((out, {n: q.grad for n, q in m.named_parameters()}))
    (out, gp), (ref, rp) = res
    assert out.dtype == torch.float32 and ref.dtype == torch.float64 and spy.n['cwn_linear_wide_f32'] > 0
    gate(out, ref, 'ln EmbedSparseCIN at hidden 6: predictions')
    for name, r in rp.items():
        if r is not None:
            gate(gp[name], r, f'ln EmbedSparseCIN at hidden 6: gradient of {name}')


def test_two_replays_of_one_batch_from_one_state_give_equal_losses():
    from cwn_amd.static_batch import StaticBatch
    from cwn_amd.static_graph import StaticTrainStep
    pool, p = _csl()
    batches = _sequence(len(pool))
    sb = StaticBatch(p, B, slots=1, mode='csr')
    sb.set_batch(batches[0])
    st = StaticTrainStep(_csl_model(), sb, task_type='classification', lr=5e-4)
    st.step_on([batches[0]])                                       # a larger batch first: its rows stay behind the next one
    state = st.state_dict()
    losses = []
    for _ in range(2):
        st.load_state_dict(state)                                  # (in place: the captured graph stays valid)
        losses.append(float(st.step_on([batches[1]])[0]))
    print('[static ln] the same batch from the same state, twice:', losses)
    assert losses[0] == losses[1] and np.isfinite(losses[0])


def test_run_epoch_over_a_shuffled_split_with_a_short_tail():
    from cwn_amd.packed import PackedLoader
    from cwn_amd.static_batch import StaticBatch
    from cwn_amd.static_graph import StaticTrainStep
    pool, p = _csl()
    st = StaticTrainStep(_csl_model(), StaticBatch(p, B, slots=2, mode='csr'), task_type='classification', lr=5e-4)
    loader = PackedLoader(p, batch_size=B, shuffle=True, indices=np.arange(29), seed=3)      # 12 + 12 + 5
    loader.set_epoch(0)
    batches = loader.batches()
    assert [len(b) for b in batches] == [12, 12, 5]
    losses = [float(l) for l in st.run_epoch(batches)]
    print('[static ln] run_epoch losses:', losses)
    assert len(losses) == 3 and all(np.isfinite(l) for l in losses)
    assert int(st.opt.t) == 3


class _Static:
    def __init__(self, mode):
        self.mode = mode


def test_what_no_counted_launch_serves_is_refused_at_construction(monkeypatch):
    from cwn_amd.models import EmbedCINpp, EmbedSparseCIN, SparseCIN
    from cwn_amd.static_graph import refuse_unsupported_layers
    kw = dict(dropout_rate=0.0, max_dim=2, embed_edge=True, use_coboundaries=True, graph_norm='ln')
    for width in (4, 48, 64, 128, 160, 256):
        refuse_unsupported_layers(EmbedSparseCIN(28, 4, 1, 2, width, **kw), 'StaticTrainStep', _Static('csr'), training=True)
    for width in (64, 128):                     # mode 'blocked' is count-correct with LayerNorm at its two widths: served
        refuse_unsupported_layers(EmbedSparseCIN(28, 4, 1, 2, width, **kw), 'StaticTrainStep', _Static('blocked'), training=True)
    with pytest.raises(NotImplementedError, match=r"\[160\].*mode='csr'"):     # ... and other widths stay refused there
        refuse_unsupported_layers(EmbedSparseCIN(28, 4, 1, 2, 160, **kw), 'StaticTrainStep', _Static('blocked'), training=True)
    refuse_unsupported_layers(SparseCIN(7, 3, 2, 160, max_dim=2, dropout_rate=0.0, graph_norm='ln'), 'StaticTrainStep',
                              _Static('csr'), training=True)
    with pytest.raises(NotImplementedError, match=r'SparseCINConv\(width 260\) with LayerNorm.*capacity rows'):
        refuse_unsupported_layers(EmbedSparseCIN(28, 4, 1, 2, 260, **kw), 'StaticTrainStep', _Static('csr'), training=True)
    with pytest.raises(NotImplementedError, match=r'SparseCINConv\(width 6\) with LayerNorm.*no multiple of 4'):
        refuse_unsupported_layers(EmbedSparseCIN(28, 4, 1, 2, 6, **kw), 'StaticTrainStep', _Static('csr'), training=True)
    pp = EmbedCINpp(28, 4, 1, 2, 64, **kw)
    with pytest.raises(NotImplementedError, match=r'CINppConv\(width 64\) with LayerNorm.*capacity rows'):
        refuse_unsupported_layers(pp, 'StaticTrainStep', _Static('csr'), training=True)
    refuse_unsupported_layers(pp, 'StaticForward', _Static('csr'), training=False)          # inference: nothing is summed over rows
    monkeypatch.setattr(dense_ln, 'FUSED_LN', False)
    with pytest.raises(NotImplementedError, match=r'SparseCINConv\(width 160\) with LayerNorm.*CWN_FUSED_LN=0'):
        refuse_unsupported_layers(EmbedSparseCIN(28, 4, 1, 2, 160, **kw), 'StaticTrainStep', _Static('csr'), training=True)


def test_train_csl_example_static_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'train_csl.py'), '--static', '--epochs', '2', '--graphs', '30'],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('epoch ')]
    assert len(lines) == 2 and 'done: ' in out.stdout, out.stdout
    for l in lines:
        loss = float(l.split('train loss ')[1].split(',')[0])
        assert np.isfinite(loss), l
