"""Learning-rate schedules and checkpoints of captured training steps: cwn_adam_dev_f32 reads Adam's hyperparameters from a
device record that FlatAdam rewrites (stream-ordered) when a scheduler of exp/run_exp.py:343-408 moves the param group, so a
replayed graph follows the schedule without a re-capture; TrainStep / FlatAdam checkpoints resume bit for bit and move to and
from torch.optim.Adam."""
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


def _adam_launch(name, p, g, m, v, t, active, lr, b1, b2, eps, wd, hyper=None):
    from cwn_amd import _ffi
    L = _ffi.lib()
    if name == 'cwn_adam_f32':
        code = L.cwn_adam_f32(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), lr, b1, b2, eps, wd,
                              t.data_ptr(), _ffi.ptr(active), _ffi.stream_ptr(DEV))
    else:
        hyper.copy_(torch.tensor([lr, b1, b2, eps, wd, 0, 0, 0], dtype=torch.float32))
        code = L.cwn_adam_dev_f32(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), hyper.data_ptr(),
                                  t.data_ptr(), _ffi.ptr(active), _ffi.stream_ptr(DEV))
    _ffi.check(code, name)


@pytest.mark.parametrize('n', [1, 7, 4096 + 3])
@pytest.mark.parametrize('active', [None, 0, 1])
def test_device_record_adam_is_bitwise_the_argument_form(n, active):
    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen).to(DEV)
    act = None if active is None else torch.tensor([active], dtype=torch.int64, device=DEV)
    outs = {}
    for name in ('cwn_adam_f32', 'cwn_adam_dev_f32'):
        p, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        t = torch.zeros(1, dtype=torch.int32, device=DEV)
        hyper = torch.zeros(8, dtype=torch.float32, device=DEV)
        g2 = torch.Generator().manual_seed(n + 1)
        for it, (lr, wd) in enumerate([(1e-3, 0.0), (3e-3, 0.01), (7e-4, 0.0)]):
            g = (torch.randn(n, generator=g2) * 10.0 ** (it - 1)).to(DEV)
            t.add_(1)
            _adam_launch(name, p, g, m, v, t, act, lr, 0.9, 0.999, 1e-8, wd, hyper)
        torch.cuda.synchronize()
        outs[name] = (p, m, v)
    for a, b in zip(outs['cwn_adam_f32'], outs['cwn_adam_dev_f32']):
        assert torch.equal(a, b)
    if active == 0:
        assert torch.equal(outs['cwn_adam_dev_f32'][0], p0)
    else:
        assert not torch.equal(outs['cwn_adam_dev_f32'][0], p0)


def test_captured_adam_follows_the_record_rewritten_between_replays():
    from cwn_amd.dist import FlatGradBucket
    from cwn_amd.train import FlatAdam
    torch.manual_seed(0)
    shapes = [(128, 256), (128,), (7, 3), (1,), (64, 64)]
    pa = [torch.nn.Parameter(torch.randn(*s, device=DEV)) for s in shapes]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    ref = torch.optim.Adam(pb, lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.01)
    opt = FlatAdam(FlatGradBucket(pa), lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.01)
    opt.sync()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    assert int(opt.t) == 0                       # (captured, not run)
    g = torch.Generator().manual_seed(1)
    for it, lr in enumerate([3e-3, 1e-3, 1e-3, 2.5e-4, 4e-3]):
        grads = [torch.randn(*s, generator=g).to(DEV) * (10.0 ** (it - 2)) for s in shapes]
        for p, q, gr in zip(pa, pb, grads):
            p.grad.copy_(gr)
            q.grad = gr.clone()
        opt.param_groups[0]['lr'] = lr
        ref.param_groups[0]['lr'] = lr
        opt.sync()
        graph.replay()
        ref.step()
        torch.cuda.synchronize()
        assert float(opt.hyper[0]) == torch.tensor(lr, dtype=torch.float32).item()
        for p, q in zip(pa, pb):
            torch.testing.assert_close(p.data, q.data, rtol=2e-5, atol=2e-6)
    assert int(opt.t) == 5


def _setup(kind, seed=3):
    from cwn_amd.complex import ComplexBatch
    from cwn_amd.models import EmbedSparseCIN, OGBEmbedSparseCIN
    from cwn_amd.synthetic import molhiv_like_complexes, zinc_like_complexes
    torch.manual_seed(seed)
    if kind == 'zinc':
        model = EmbedSparseCIN(28, 4, 1, 3, 64, dropout_rate=0.0, max_dim=2, jump_mode=None, nonlinearity='relu', readout='sum',
                               train_eps=False, final_hidden_multiplier=2, final_readout='sum', init_reduce='sum', embed_edge=True,
                               use_coboundaries=True, graph_norm='bn')
        bs = [ComplexBatch.from_complex_list(zinc_like_complexes(48, 70 + i, 6), max_dim=2) for i in range(2)]
        task = 'regression'
    else:
        model = OGBEmbedSparseCIN(1, 2, 64, dropout_rate=0.5, max_dim=2, readout='mean', final_readout='sum', init_reduce='sum',
                                  embed_edge=True, use_coboundaries=True, graph_norm='bn')
        bs = [ComplexBatch.from_complex_list(molhiv_like_complexes(64, 80 + i, 6), max_dim=2) for i in range(2)]
        task = 'bin_classification'
    return model.to(DEV), [b.to(DEV) for b in bs], task


def _no_scheduler_warning(caught):
    """Neither "lr_scheduler.step() before optimizer.step()" nor "optimizer.step() has been overridden"."""
    bad = [str(w.message) for w in caught if 'lr_scheduler' in str(w.message) or 'optimizer.step()' in str(w.message)]
    assert not bad, bad


def _flat(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()]).clone()


def test_step_lr_through_a_captured_train_step_equals_the_eager_loop():
    import warnings
    from cwn_amd import ops
    from cwn_amd.train import TrainStep
    state0 = {k: v.clone() for k, v in _setup('zinc')[0].state_dict().items()}

    def run(use_graph, gamma):
        model, bs, task = _setup('zinc')
        model.load_state_dict(state0)
        ts = TrainStep(model, bs, task_type=task, lr=1e-3, use_graph=use_graph)
        sched = torch.optim.lr_scheduler.StepLR(ts.opt, step_size=1, gamma=gamma)
        lrs, graphs = [], None
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter('always')
            for i in range(4):
                lrs.append(ts.opt.param_groups[0]['lr'])
                ts.step(i % len(bs))
                sched.step()
                if i == 1 and use_graph:
                    graphs = {k: id(v[0][0]) for k, v in ts._graphs.items()}
        _no_scheduler_warning(caught)
        torch.cuda.synchronize()
        if use_graph:
            assert graphs == {k: id(v[0][0]) for k, v in ts._graphs.items()}     # the graphs of the first capture, kept
        return _flat(model), lrs, int(ts.opt.t)

    ops.deterministic(True)
    try:
        eager, lrs_e, te = run(False, 0.5)
        graph, lrs_g, tg = run(True, 0.5)
        const, _, _ = run(True, 1.0)
    finally:
        ops.deterministic(False)
    assert lrs_e == lrs_g == [1e-3, 5e-4, 2.5e-4, 1.25e-4] and te == tg == 4
    assert torch.equal(eager, graph), float((eager - graph).abs().max())
    assert not torch.equal(graph, const)
    print(f'[StepLR] max |scheduled - constant lr| after 4 steps: {float((graph - const).abs().max()):.3e}')


def _lr_ratio(d_got, d_want, lr):
    """The scale between two parameter updates of one epoch from the same state: the median over the parameters whose update
    is a sizeable fraction of lr (Adam's early steps are ~lr per parameter; a parameter whose gradient is summation noise may
    flip sign between two forms of the same arithmetic, which the median ignores)."""
    sel = d_want.abs() > 0.2 * lr
    assert int(sel.sum()) > 100
    return float((d_got[sel] / d_want[sel]).median())


def _plateau_epochs(step_obj, owners, ref, run_epoch, ref_epoch, min_lr):
    """exp/run_exp.py's loop on a forced plateau: ReduceLROnPlateau(mode='min', factor=0.5, patience=0) fed a constant
    validation metric halves lr from the second epoch on; the loop stops once lr < min_lr.  Each epoch is pinned on an
    eager replica (TrainStep over the collated batches) started from the same checkpoint: its update scales like the lr the
    scheduler set, i.e. the lr the captured kernel read."""
    import warnings
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(step_obj.opt, mode='min', factor=0.5, patience=0)
    lrs, graphs = [], None
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        while step_obj.opt.param_groups[0]['lr'] >= min_lr:
            lr = step_obj.opt.param_groups[0]['lr']
            lrs.append(lr)
            ref.load_state_dict(step_obj.state_dict())
            assert ref.opt.param_groups[0]['lr'] == lr
            p0 = step_obj.opt.flat_p.clone()
            run_epoch()
            ref_epoch()
            torch.cuda.synchronize()
            r = _lr_ratio(step_obj.opt.flat_p - p0, ref.opt.flat_p - p0, lr)
            print(f'[plateau] epoch {len(lrs)}: lr {lr:.3e}, update scale vs the eager replica {r:.4f}')
            assert abs(r - 1.0) < 0.05, (len(lrs), lr, r)
            now = {(j, k): id(v[0]) for j, ts in enumerate(owners) for k, v in ts._graphs.items()}
            if graphs is None:
                graphs = now
            assert graphs == now                        # no re-capture
            sched.step(1.0)
            assert len(lrs) < 10
    _no_scheduler_warning(caught)
    return lrs


def test_reduce_lr_on_plateau_through_static_and_routed_epochs():
    from cwn_amd.models import OGBEmbedSparseCIN
    from cwn_amd.packed import PackedComplexes
    from cwn_amd.static_batch import StaticBatch
    from cwn_amd.static_graph import RoutedTrainStep, StaticRouter, StaticTrainStep
    from cwn_amd.synthetic import molhiv_like_complexes, zinc_like_complexes
    from cwn_amd.train import TrainStep
    # StaticTrainStep.run_epoch, two slots: three batches = a two-slot replay and a one-slot tail replay per epoch
    pool = zinc_like_complexes(220, seed=3, max_ring=6, n_lo=9, n_hi=28)
    p = PackedComplexes(pool, DEV, max_dim=2, with_csr=True)
    B = 40
    perm = np.random.default_rng(21).permutation(len(pool))
    epoch = [perm[k * B:(k + 1) * B] for k in range(3)]
    m1, m2 = _setup('zinc', seed=6)[0], _setup('zinc', seed=6)[0]
    sb = StaticBatch(p, B, slots=2)
    sb.reserve_epoch(4)
    sb.set_epoch(epoch)
    st = StaticTrainStep(m1, sb, lr=1e-3)
    ref = TrainStep(m2, [p.collate(idx) for idx in epoch], lr=1e-3, use_graph=False)
    lrs = _plateau_epochs(st, [st], ref, lambda: st.run_epoch(epoch, keep_losses=False),
                          lambda: [ref.step(j) for j in range(len(epoch))], 2e-4)
    assert lrs == [1e-3, 1e-3, 5e-4, 2.5e-4]
    assert int(st.opt.t) == 4 * len(epoch)
    # RoutedTrainStep: both static batches' graphs share the one optimizer (and its record)
    pool = molhiv_like_complexes(300, seed=7, max_ring=6, tail=0.02)
    p = PackedComplexes(pool, DEV, max_dim=2, with_csr=True)
    B = 32
    perm = np.random.default_rng(5).permutation(len(pool))
    epoch = [perm[k * B:(k + 1) * B] for k in range(9)]

    def mk():
        torch.manual_seed(4)
        return OGBEmbedSparseCIN(1, 2, 64, dropout_rate=0.0, max_dim=2, readout='mean', final_readout='sum', init_reduce='sum',
                                 embed_edge=True, use_coboundaries=True, graph_norm='bn').to(DEV)
    router = StaticRouter(p, B, slots=2)
    rt = RoutedTrainStep(mk(), router, task_type='bin_classification', lr=1e-3)
    a, b = router.split(epoch)
    assert a and b
    ref = TrainStep(mk(), [p.collate(epoch[k]) for k in a + b], task_type='bin_classification', lr=1e-3, use_graph=False)
    lrs = _plateau_epochs(rt, [rt.ta, rt.tb], ref, lambda: rt.run_epoch(epoch, keep_losses=False),
                          lambda: [ref.step(j) for j in range(len(epoch))], 4e-4)
    assert lrs == [1e-3, 1e-3, 5e-4]
    assert int(rt.opt.t) == 3 * len(epoch)


def test_resume_from_a_checkpoint_bit_for_bit_with_dropout():
    from cwn_amd import ops
    from cwn_amd.train import TrainStep
    N, k = 5, 2
    state0 = {kk: v.clone() for kk, v in _setup('molhiv_dropout')[0].state_dict().items()}

    def fresh():
        model, bs, task = _setup('molhiv_dropout')
        model.load_state_dict(state0)
        return model, TrainStep(model, bs, task_type=task, lr=1e-3, use_graph=True)

    def snapshot(model, ts):
        torch.cuda.synchronize()
        return ([t.detach().clone() for t in model.parameters()] + [t.detach().clone() for t in model.buffers()]
                + [t.clone() for t in ts.opt.state_tensors()] + [ops.dropout_state(DEV).clone()])

    def same(a, b):
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), (i, x.shape)

    ops.deterministic(True)
    try:
        ops.dropout_seed(11, DEV)
        model, ts = fresh()
        for i in range(N):
            ts.step(i % 2)
        straight = snapshot(model, ts)
        # k steps, checkpoint through torch.save, a NEW model and step object, N - k steps
        ops.dropout_seed(11, DEV)
        model, ts = fresh()
        for i in range(k):
            ts.step(i % 2)
        buf = io.BytesIO()
        torch.save(ts.state_dict(), buf)
        ck = torch.load(io.BytesIO(buf.getvalue()), weights_only=False)
        assert set(ck) == {'model', 'optimizer', 'dropout'} and ck['dropout'] is not None
        assert int(ck['dropout'][0]) == 11
        ops.dropout_seed(99, DEV)                          # (whatever the device stream holds: the checkpoint's wins)
        model2, ts2 = fresh()
        ts2.load_state_dict(ck)
        for i in range(k, N):
            ts2.step(i % 2)
        same(snapshot(model2, ts2), straight)
        # ... and in place: rewind the captured step object of the second run to the checkpoint, its graphs kept
        graphs = dict(ts2._graphs)
        ts2.load_state_dict(ck)
        for i in range(k, N):
            ts2.step(i % 2)
        same(snapshot(model2, ts2), straight)
        assert ts2._graphs == graphs
    finally:
        ops.deterministic(False)


def test_a_torch_adam_run_continues_on_the_flat_optimizer():
    from cwn_amd.train import TrainStep
    model, bs, task = _setup('zinc', seed=8)
    # k steps with torch.optim.Adam (gradients through the same eager step)
    topt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=0.01)
    warm = TrainStep(model, bs, task_type=task, optimizer=topt, use_graph=False)
    for i in range(3):
        warm.step(i % 2)
    torch.cuda.synchronize()
    twin = _setup('zinc', seed=8)[0]
    twin.load_state_dict(model.state_dict())
    topt2 = torch.optim.Adam(twin.parameters(), lr=1e-3, weight_decay=0.01)
    topt2.load_state_dict(topt.state_dict())
    # ... continued on a captured TrainStep: FlatAdam takes torch's state; torch's Adam continues on the twin with the
    # gradients the captured step computed
    ts = TrainStep(model, bs, task_type=task, lr=5.0, use_graph=True)
    ts.opt.load_state_dict(topt.state_dict())
    assert int(ts.opt.t) == 3 and ts.opt.param_groups[0]['lr'] == 1e-3 and ts.opt.param_groups[0]['weight_decay'] == 0.01
    for i in range(3, 7):
        ts.step(i % 2)
        torch.cuda.synchronize()
        for p, q in zip(model.parameters(), twin.parameters()):
            q.grad = p.grad.detach().clone()
        topt2.step()
        for p, q in zip(model.parameters(), twin.parameters()):
            torch.testing.assert_close(p.data, q.data, rtol=2e-5, atol=2e-6)
    assert int(ts.opt.t) == 7
    back = ts.opt.state_dict()
    want = topt2.state_dict()
    for i, st in want['state'].items():
        assert float(back['state'][i]['step']) == float(st['step'])
        torch.testing.assert_close(back['state'][i]['exp_avg'], st['exp_avg'], rtol=2e-5, atol=2e-6)
