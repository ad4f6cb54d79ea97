"""The captured edge-flow path on the device: the counted readout head under a capacity, StaticCochainForward and
StaticCochainTrainStep over a deliberately NON-UNIFORM dataset of cochains (all cochains of one `edge_flows` call share one
mesh, which would hide every count bug), against the eager forward / autograd step on PackedCochains.collate(idx) with the
fused head on.  Float comparisons use tests/_product.gate: max|delta| <= 1e-5 * max(1, |ref|_inf); where the launches and
their operands are the same, torch.equal.

The dataset: thirteen cochains on the meshes edge_flow_mesh(side) for side in {3, 4, 6, 9}, with and without holes -- 16,
33, 83, 85, 202 and 208 edges: above and below the head's 128-row chunk, five of the six sizes no multiple of the layer's
32-row tile.  The generator cannot make a cochain without upper adjacency (every mesh it cuts has triangles), so cochain 0
-- on the smallest mesh -- has its upper adjacency taken away by hand.  Batches of 4 with a tail batch of 1."""
import copy

import numpy as np
import pytest
import torch

from cwn_amd import _ffi, evaluate, models, ops, packed, static_cochains, static_graph
from cwn_amd.complex import Cochain
from cwn_amd.dist import FlatGradBucket
from cwn_amd.synthetic import edge_flows
from cwn_amd.train import FlatAdam, fused_loss
from tests._product import gate

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CHUNK = _ffi.FLOW_HEAD_CHUNK
CONFIGS = [('orient', 8, 'sum'), ('orient', 64, 'mean'), ('mpnn', 64, 'sum'), ('mpnn', 8, 'mean')]
_CACHE = {}


def _data():
    if 'data' not in _CACHE:
        cs = []
        for side, holes, n, seed in ((3, False, 2, 1), (4, True, 2, 2), (6, True, 2, 3), (6, False, 2, 4), (9, True, 2, 5),
                                     (9, False, 3, 6)):
            cs += edge_flows(n, side, seed, holes=holes)
        c = cs[0]
        cs[0] = Cochain(dim=1, x=c.x, lower_index=c.lower_index, lower_orient=c.lower_orient, y=c.y)
        sizes = [c.num_cells for c in cs]
        assert len(cs) == 13 and max(sizes) > CHUNK > min(sizes) and any(n % 32 for n in sizes)
        _CACHE['data'] = (cs, packed.PackedCochains(cs, DEV))
    return _CACHE['data']


def _epoch(e: int):
    """Four batches of 4 and 4 and 4 and 1, shuffled per epoch; the tail is never cochain 0 alone (a batch none of whose
    cochains has an upper adjacency has no `upper_index` on the eager path either: OrientedConv refuses it there)."""
    order = np.random.default_rng(100 + e).permutation(13)
    if order[-1] == 0:
        order[[0, -1]] = order[[-1, 0]]
    return [order[lo:lo + 4] for lo in range(0, 13, 4)]


def _model(kind, hidden, readout, seed=0):
    torch.manual_seed(seed)
    if kind == 'orient':
        return models.EdgeOrient(1, 2, 2, hidden, nonlinearity='tanh', readout=readout).to(DEV)
    return models.EdgeMPNN(1, 2, 2, hidden, nonlinearity='relu', readout=readout).to(DEV)


class _fused_head:
    def __enter__(self):
        self.prev, models.FUSED_FLOW_HEAD = models.FUSED_FLOW_HEAD, True

    def __exit__(self, *exc):
        models.FUSED_FLOW_HEAD = self.prev
        return False


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. the counted head on its own ----------------------------------------------------------------------------------------------
SENTINEL = 0x7fc12345                                                  # the bits of a NaN with a payload
ROWS = [(0, []), (2, [0, 0]), (1, [1]), (1, [CHUNK - 1]), (1, [CHUNK]), (2, [CHUNK + 1, 3]), (5, [CHUNK, 1, 0, CHUNK + 1, 42])]


@pytest.mark.parametrize('K,H,O,take_abs,mean', [(8, 16, 2, True, False), (6, 5, 3, False, True), (64, 64, 2, True, True)])
def test_counted_head_equals_the_host_count_launch_on_the_trimmed_tensors(K, H, O, take_abs, mean):
    n_cap, c_cap = 2 * CHUNK + 44, 5                                   # the last case fills the capacity exactly
    g = torch.Generator().manual_seed(K)
    w1, b1 = torch.randn(H, K, generator=g).to(DEV), torch.randn(H, generator=g).to(DEV)
    w2, b2 = torch.randn(O, H, generator=g).to(DEV), torch.randn(O, generator=g).to(DEV)
    for c, rows in ROWS:
        n = sum(rows)
        for explicit_n in (False, True):
            x = torch.full((n_cap, K), float('nan'))
            x[:n] = torch.randn(n, K, generator=g)
            x = x.to(DEV)
            ptr = torch.full((c_cap + 1,), n, dtype=torch.long)
            ptr[:c + 1] = torch.tensor([0] + np.cumsum(rows).tolist(), dtype=torch.long)
            if explicit_n:
                ptr[c + 1:] = -7                                       # entries behind the live ones are never read
            ptr = ptr.to(DEV)
            n_dev = torch.tensor([n], dtype=torch.long, device=DEV) if explicit_n else None
            c_dev = torch.tensor([c], dtype=torch.long, device=DEV)
            gout = torch.full((c_cap, O), float('nan'))
            gout[:c] = torch.randn(c, O, generator=g)
            gout = gout.to(DEV)
            out, pooled, h = _ffi.flow_head_counted(x, ptr, n_dev, c_dev, w1, b1, w2, b2, take_abs, mean, keep=True)
            dx = torch.full((n_cap, K), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
            dh = _ffi.flow_head_counted_bwd(gout, h, x, ptr, n_dev, c_dev, w1, w2, take_abs, mean, dx)
            what = (K, c, rows, explicit_n)
            # absent cochains: zeros; padding rows of dx: the sentinel, bit for bit
            for t in (out, pooled, h, dh):
                assert not t[c:].any() and torch.isfinite(t[c:]).all(), what
            assert bool((_bits(dx[n:]) == SENTINEL).all()), what
            if c == 0:
                continue
            xt, pt = x[:n].contiguous(), ptr[:c + 1].contiguous()
            ro, rp, rh = _ffi.flow_head(xt, pt, w1, b1, w2, b2, take_abs, mean, keep=True)
            rdx, rdh = _ffi.flow_head_bwd(gout[:c].contiguous(), rh, xt, pt, w1, w2, take_abs, mean, True)
            for got, ref, name in ((out, ro, 'out'), (pooled, rp, 'pooled'), (h, rh, 'h'), (dh, rdh, 'dh')):
                assert torch.equal(got[:c], ref), (what, name)
            assert torch.equal(dx[:n], rdx), what
    # the op: autograd under a capacity against the host-count op on the trimmed tensors (weight gradients under the count)
    c, rows = ROWS[-1]
    n = sum(rows)
    x = torch.full((n_cap, K), float('nan'))
    x[:n] = torch.randn(n, K, generator=g)
    x = x.to(DEV).requires_grad_(True)
    ptr = torch.tensor([0] + np.cumsum(rows).tolist(), dtype=torch.long, device=DEV)
    params = [t.clone().requires_grad_(True) for t in (w1, b1, w2, b2)]
    c_dev = torch.tensor([c - 1], dtype=torch.long, device=DEV)         # one cochain fewer than the capacity of `ptr`
    out = ops.flow_head_counted(x, ptr, c_dev, params[0], params[1], params[2], params[3], abs=take_abs, mean=mean)
    seed = torch.randn(c, O, generator=g).to(DEV)
    seed[c - 1] = float('nan')                                          # the absent cochain's gradient row may hold anything
    got = torch.autograd.grad(out, params, seed)
    xr = x.detach()[:n - rows[-1]].clone().requires_grad_(True)
    ref_p = [t.detach().clone().requires_grad_(True) for t in params]
    ref = ops.flow_head(xr, ptr[:c].contiguous(), ref_p[0], ref_p[1], ref_p[2], ref_p[3], abs=take_abs, mean=mean)
    assert torch.equal(out[:c - 1], ref)
    want = torch.autograd.grad(ref, ref_p, seed[:c - 1].contiguous())
    for a, b, name in zip(got, want, ('dW1', 'db1', 'dW2', 'db2')):
        gate(a, b.double(), f'counted head {name} K={K}')


# ---- 2. the captured forward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,hidden,readout', CONFIGS)
def test_forward_over_poisoned_buffers_equals_the_eager_forward(kind, hidden, readout):
    cs, pc = _data()
    model = _model(kind, hidden, readout).eval()
    sb = static_cochains.StaticCochainBatch(pc, 4, slots=2)
    sb.poison()
    fwd = static_graph.StaticCochainForward(model, sb)
    for e in (0, 1):
        batches = _epoch(e)
        preds = fwd.run_epoch(batches)
        assert [p.size(0) for p in preds] == [4, 4, 4, 1]
        assert e > 0 or model.last_head_route == 'counted'             # (epoch 1 is replays alone: no Python runs)
        with torch.no_grad(), _fused_head():
            for idx, p in zip(batches, preds):
                ref = model(pc.collate(idx))
                assert model.last_head_route == 'fused'
                assert torch.equal(p, ref), (kind, hidden, readout, e, idx.tolist())
    assert set(fwd._graphs) == {2}                                     # one captured sequence served both epochs
    tail = cs[int(batches[-1][0])]
    assert sb.sizes() == {'rows': tail.num_cells, 'upper_index': int(tail.upper_index.size(1)),
                          'lower_index': int(tail.lower_index.size(1)), 'cochains': 1}
    most = max(sum(cs[int(i)].num_cells for i in idx) for e in (0, 1) for idx in _epoch(e))
    assert torch.isnan(sb.bufs['x'][most:]).all()                      # rows no batch reached are still poison


# ---- 3. / 4. the captured training step ----------------------------------------------------------------------------------------------
LR = 1e-2


def _eager_steps(kind, hidden, readout, batches, det):
    """The eager collated steps from the same initial parameters with the same FlatAdam settings: per step the loss and the
    gradients, and the parameters behind every step.  Computed once per configuration and shared."""
    key = ('eager', kind, hidden, readout, det)
    if key not in _CACHE:
        _, pc = _data()
        ref = _model(kind, hidden, readout).train()
        bucket = FlatGradBucket(ref.parameters())
        opt = FlatAdam(bucket, lr=LR)
        losses, grads, params = [], [], []
        with _fused_head():
            for idx in batches:
                bucket.zero_()
                b = pc.collate(idx)
                loss = fused_loss('classification', ref(b), b.y.view(-1))
                loss.backward()
                assert ref.last_head_route == 'fused'
                losses.append(loss.detach().clone())
                grads.append([p.grad.clone() for p in ref.parameters()])
                opt.step()
                params.append([p.detach().clone() for p in ref.parameters()])
        _CACHE[key] = (losses, grads, params)
    return _CACHE[key]


def _static_step(kind, hidden, readout, slots):
    _, pc = _data()
    model = _model(kind, hidden, readout)
    sb = static_cochains.StaticCochainBatch(pc, 4, slots=slots)
    sb.poison()
    return model, sb, static_graph.StaticCochainTrainStep(model, sb, 'classification', lr=LR)


@pytest.mark.parametrize('kind,hidden,readout', CONFIGS)
def test_train_step_against_the_eager_collated_step(kind, hidden, readout):
    batches = _epoch(0)
    ref_losses, ref_grads, ref_params = _eager_steps(kind, hidden, readout, batches, False)
    model, sb, step = _static_step(kind, hidden, readout, 2)
    sb.set_epoch(batches)
    losses = [l.clone() for l in step.step(n_slots=1)]                  # ONE step: the bucket holds its gradients
    for (name, p), g in zip(model.named_parameters(), ref_grads[0]):
        gate(p.grad, g.double(), f'{kind} {hidden} {readout}: gradient of {name} after one step')
    losses += [l.clone() for l in step.step()]                          # two more
    for (name, p), r in zip(model.named_parameters(), ref_params[2]):
        gate(p, r.double(), f'{kind} {hidden} {readout}: {name} after three steps')
    for k, (l, r) in enumerate(zip(losses, ref_losses[:3])):
        gate(l, r.double(), f'{kind} {hidden} {readout}: loss of step {k}')
    assert step.opt.param_groups[0]['lr'] == LR and int(step.opt.t.item()) == 3
    # a state_dict round trip followed by one more step equals the uninterrupted run
    state = step.state_dict()
    last = step.step(n_slots=1)[0].clone()
    after = [p.detach().clone() for p in model.parameters()]
    gate(last, ref_losses[3].double(), 'loss of the tail batch')
    step.step(n_slots=1)                                                # (a step past the epoch: an empty batch changes nothing)
    assert all(torch.equal(p, a) for p, a in zip(model.parameters(), after)) and int(step.opt.t.item()) == 4
    step.load_state_dict(state)
    assert int(step.opt.t.item()) == 3
    sb.rewind(3)
    again = step.step(n_slots=1)[0].clone()
    gate(again, last.double(), 'loss after the round trip')
    for (name, p), a in zip(model.named_parameters(), after):
        gate(p, a.double(), f'{name} after the state_dict round trip')
    assert not any(torch.isnan(p).any() for p in model.parameters())


def test_train_step_has_the_eager_bits_under_deterministic_sums():
    kind, hidden, readout = CONFIGS[1]
    batches = _epoch(1)
    ops.deterministic(True)
    try:
        ref_losses, ref_grads, ref_params = _eager_steps(kind, hidden, readout, batches, True)
        model, sb, step = _static_step(kind, hidden, readout, 1)
        sb.set_epoch(batches)
        loss = step.step()[0]
        assert torch.equal(loss, ref_losses[0])
        for (name, p), g in zip(model.named_parameters(), ref_grads[0]):
            assert torch.equal(p.grad, g), name
    finally:
        ops.deterministic(False)


def test_short_epoch_takes_the_shorter_captured_sequence():
    kind, hidden, readout = CONFIGS[0]
    batches = _epoch(0)
    ref_losses, _, ref_params = _eager_steps(kind, hidden, readout, batches, False)
    model, sb, step = _static_step(kind, hidden, readout, 3)
    losses = step.run_epoch(batches)                                    # 4 batches, 3 slots: one full replay and a one-step tail
    assert ('seq', 0, 1, 2) in step._graphs and ('seq', 0) in step._graphs and step.slots_for(1) == 1 and step.slots_for(2) == 2
    assert len(losses) == 4 and all(torch.isfinite(l) for l in losses)
    assert not any(torch.isnan(p).any() for p in model.parameters())
    for (name, p), r in zip(model.named_parameters(), ref_params[3]):
        gate(p, r.double(), f'{name} after an epoch of 3 + 1 steps')
    for k, (l, r) in enumerate(zip(losses, ref_losses)):
        gate(l, r.double(), f'loss of step {k}')


# ---- 5. evaluation -------------------------------------------------------------------------------------------------------------------
def test_evaluate_takes_the_static_forward():
    _, pc = _data()
    model = _model('orient', 64, 'sum', seed=3)
    sb = static_cochains.StaticCochainBatch(pc, 4, slots=3)
    sb.poison()
    batches = _epoch(2)
    ev = evaluate.Evaluator('accuracy')
    fwd = static_graph.StaticCochainForward(model, sb)
    for scale in (1.0, 1.5):               # the second pass: new parameter VALUES, the same captured graphs
        with torch.no_grad():
            model.lin2.weight.mul_(scale)
            model.convs[0].update_nn.weight.mul_(scale)
        acc, loss = evaluate.evaluate(fwd, batches, ev, 'classification')
        with _fused_head():
            acc_ref, loss_ref = evaluate.evaluate(packed.CochainForward(model, pc), batches, ev, 'classification')
        assert acc == acc_ref and 0.0 <= acc <= 1.0
        assert abs(loss - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref)), (loss, loss_ref)
    assert sorted(fwd._graphs) == [1, 3]   # (4 batches at 3 slots: the full sequence and the one-step tail, captured once each)


def test_a_batch_beyond_a_capacity_is_refused_by_name():
    _, pc = _data()
    sb = static_cochains.StaticCochainBatch(pc, 4, caps={'rows': 500})
    with pytest.raises(ValueError, match=r'batch 1: \d+ rows exceed the capacity 500'):
        sb.set_epoch([[0, 1, 2, 3], [9, 10, 11, 12]])
    with pytest.raises(ValueError, match='1 .. 4 cochains'):
        sb.set_epoch([[0, 1, 2, 3, 4]])
