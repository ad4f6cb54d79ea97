"""The edge-flow readout head on the device (csrc/cwn_flow_head.hip, ops.flow_head) against a float64 evaluation on the CPU of

    pooled[c] = sum over the rows of cochain c of f(x[r])  (f = |.| or identity; / max(rows, 1) for 'mean')
    out[c]    = W2 relu(W1 pooled[c] + b1) + b2

forward, batch invariance (torch.equal), backward against float64 autograd of the formula, the non-finite contract, the
operand checks, and the route through models.EdgeOrient / EdgeMPNN.  The bar is tests/_product.gate: max|delta| <= 1e-5 *
max(1, |ref|_inf).  Row counts sit around the chunk (CWN_FLOW_HEAD_CHUNK = 128 rows): 0, 1, 127, 128, 129, 257, 5."""
import numpy as np
import pytest
import torch

from cwn_amd import _ffi, models, ops, packed
from cwn_amd.complex import CochainBatch
from cwn_amd.synthetic import edge_flows
from tests._product import gate, gate_nonfinite

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
ROWS = [0, 1, 127, 128, 129, 257, 5]
TOL = 1e-5


def _ptr(rows):
    return torch.tensor([0] + np.cumsum(rows).tolist(), dtype=torch.long)


def _x(n: int, K: int, seed: int) -> torch.Tensor:
    """Values of both signs, about a third of them exactly zero (what a ReLU layer hands the head)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, K, generator=g)
    x[torch.rand(n, K, generator=g) < 0.33] = 0.0
    return x


def _weights(K: int, O: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    H = K
    return (torch.randn(H, K, generator=g) / max(K, 4) ** 0.5, torch.randn(H, generator=g) * 0.1,
            torch.randn(O, H, generator=g) / max(H, 4) ** 0.5, torch.randn(O, generator=g) * 0.1)


def _formula64(x, ptr, w1, b1, w2, b2, take_abs, mean):
    """The head in float64 on the CPU, differentiable."""
    x64 = x.double()
    f = x64.abs() if take_abs else x64
    rows = (ptr[1:] - ptr[:-1])
    seg = torch.repeat_interleave(torch.arange(rows.numel()), rows)
    pooled = torch.zeros(rows.numel(), x.size(1), dtype=torch.float64).index_add(0, seg, f)
    if mean:
        pooled = pooled / rows.clamp(min=1).double()[:, None]
    h = pooled @ w1.double().t() + b1.double()
    return torch.relu(h) @ w2.double().t() + b2.double()


def _dev(*ts):
    return [t.to(DEV) for t in ts]


@pytest.mark.parametrize('mean', [False, True])
@pytest.mark.parametrize('C', [1, 65])
@pytest.mark.parametrize('K,O', [(1, 1), (12, 2), (16, 5), (64, 2), (128, 5)])
def test_forward_against_float64(K, O, C, mean):
    rows = [129] if C == 1 else (ROWS * 10)[:C]
    ptr = _ptr(rows)
    x = _x(int(ptr[-1]), K, seed=K + C)
    w = _weights(K, O, seed=3 * K + O)
    # a row stride that is no multiple of 4: element loads; NaN beside the window (a zero there would hide a load that strays)
    wide = torch.full((x.size(0), K + 3), float('nan'), device=DEV)
    wide[:, :K] = x.to(DEV)
    outs = {}
    for take_abs in (True, False):
        ref = _formula64(x, ptr, *w, take_abs, mean)
        got = ops.flow_head(x.to(DEV), ptr.to(DEV), *_dev(*w), abs=take_abs, mean=mean)
        gate(got, ref, f'K {K} O {O} C {C} mean {mean} abs {take_abs}')
        strided = ops.flow_head(wide[:, :K], ptr.to(DEV), *_dev(*w), abs=take_abs, mean=mean, n_cochains=C)
        assert torch.equal(strided, got)                             # 16-byte and element loads add in the same order
        outs[take_abs] = ref
    # the two variants are far apart on this input: a missing |.| would show
    assert float((outs[True] - outs[False]).abs().max()) > 100 * TOL * max(1.0, float(outs[True].abs().max()))


@pytest.mark.parametrize('K', [12, 64])
def test_batch_invariance(K):
    """A cochain's prediction has the same bits alone, at any place of two differently ordered batches, and on a second run."""
    rows = ROWS + [300]
    xs = [_x(n, K, seed=100 + i) for i, n in enumerate(rows)]
    w = _dev(*_weights(K, 3, seed=K))

    def run(order):
        ptr = _ptr([rows[i] for i in order]).to(DEV)
        return ops.flow_head(torch.cat([xs[i] for i in order]).to(DEV), ptr, *w, abs=True, mean=True)
    a_order, b_order = list(range(len(rows))), [7, 3, 0, 5, 1, 6, 2, 4]
    a, b = run(a_order), run(b_order)
    assert torch.equal(a, run(a_order))
    for i in range(len(rows)):
        alone = run([i])
        assert torch.equal(alone[0], a[a_order.index(i)]) and torch.equal(alone[0], b[b_order.index(i)]), i
    assert torch.isfinite(a).all() and float(a.abs().max()) > 1e-3


@pytest.mark.parametrize('take_abs,mean', [(True, False), (True, True), (False, False)])
@pytest.mark.parametrize('K,O', [(1, 1), (12, 2), (64, 5), (128, 2)])
def test_backward_against_float64_autograd(K, O, take_abs, mean):
    ptr = _ptr(ROWS)
    x = _x(int(ptr[-1]), K, seed=7 * K)
    w = _weights(K, O, seed=K + O)
    g = torch.randn(len(ROWS), O, generator=torch.Generator().manual_seed(5))
    leaves64 = [t.double().requires_grad_(True) for t in (x,) + w]
    _formula64(leaves64[0], ptr, *leaves64[1:], take_abs, mean).backward(g.double())
    leaves = [t.to(DEV).requires_grad_(True) for t in (x,) + w]
    out = ops.flow_head(leaves[0], ptr.to(DEV), *leaves[1:], abs=take_abs, mean=mean)
    out.backward(g.to(DEV))
    for name, got, ref in zip(('dx', 'dW1', 'db1', 'dW2', 'db2'), leaves, leaves64):
        assert got.grad is not None and got.grad.shape == ref.grad.shape, name
        gate(got.grad, ref.grad, f'K {K} O {O} abs {take_abs} mean {mean}: {name}')
    dx = leaves[0].grad.cpu()
    if take_abs:
        assert bool((x == 0).any()) and bool((dx[x == 0] == 0).all())           # sgn(0) = 0, exactly
    # every row written: row by row against the reference (dx comes out of torch.empty)
    for c in range(len(ROWS)):
        lo, hi = int(ptr[c]), int(ptr[c + 1])
        if hi > lo:
            gate(dx[lo:hi], leaves64[0].grad[lo:hi], f'dx rows of cochain {c}')


def test_backward_writes_every_row_of_a_sentinel_buffer():
    """The entry point itself over a dx the caller filled with a sentinel: no row keeps it."""
    K, H, O = 16, 16, 2
    ptr = _ptr(ROWS).to(DEV)
    N, Cn = int(ptr[-1]), len(ROWS)
    x = _x(N, K, seed=1).to(DEV)
    w1, _, w2, _ = _dev(*_weights(K, O, seed=2))
    g, h = torch.randn(Cn, O, device=DEV), torch.randn(Cn, H, device=DEV)
    dx = torch.full((N, K), 12345.0, device=DEV)
    dh = torch.empty(Cn, H, device=DEV)
    ws = torch.empty(int(_ffi.lib().cwn_flow_head_workspace_floats(N, Cn, K)), device=DEV)
    _ffi.check(_ffi.lib().cwn_flow_head_bwd_f32(g.data_ptr(), O, h.data_ptr(), x.data_ptr(), N, K, ptr.data_ptr(), Cn, w1.data_ptr(),
                                                w2.data_ptr(), dx.data_ptr(), K, dh.data_ptr(), K, H, O, 1, 0, ws.data_ptr(), ws.numel(),
                                                _ffi.stream_ptr(DEV)), 'cwn_flow_head_bwd_f32')
    assert not bool((dx == 12345.0).any())
    dh64 = (g.double().cpu() @ w2.double().cpu()) * (h.cpu() > 0)
    gate(dh, dh64, 'dh')
    dp = dh64 @ w1.double().cpu()
    seg = torch.repeat_interleave(torch.arange(Cn), torch.tensor(ROWS))
    gate(dx, torch.sign(x.double().cpu()) * dp[seg], 'dx')


@pytest.mark.parametrize('poison', [float('nan'), float('inf')])
@pytest.mark.parametrize('mean', [False, True])
def test_nonfinite_stays_in_its_cochain(poison, mean):
    K, O = 16, 5
    ptr = _ptr(ROWS)
    x = _x(int(ptr[-1]), K, seed=9)
    w = _weights(K, O, seed=4)
    clean = ops.flow_head(x.to(DEV), ptr.to(DEV), *_dev(*w), abs=True, mean=mean)
    bad = 5                                                           # the cochain of 257 rows: several chunks
    x[int(ptr[bad]) + 200, 3] = poison
    ref = _formula64(x, ptr, *w, True, mean)
    got = ops.flow_head(x.to(DEV), ptr.to(DEV), *_dev(*w), abs=True, mean=mean)
    gate_nonfinite(got, ref, f'poison {poison} mean {mean}')
    assert not bool(torch.isfinite(got[bad]).all())
    keep = [c for c in range(len(ROWS)) if c != bad]
    assert torch.equal(got[keep], clean[keep])


def test_operand_checks_precede_any_launch():
    K, O = 8, 2
    ptr = _ptr([3, 4]).to(DEV)
    x = _x(7, K, seed=0).to(DEV)
    w = _dev(*_weights(K, O, seed=0))
    with pytest.raises(TypeError, match='flow_head: x must be float32 .got torch.float64.'):
        ops.flow_head(x.double(), ptr, *w)
    with pytest.raises(TypeError, match='flow_head: lin1_w must be float32 .got torch.float64.'):
        ops.flow_head(x, ptr, w[0].double(), *w[1:])
    with pytest.raises(TypeError, match='flow_head: x must be a float32 tensor on the GPU .got torch.float32 on cpu.'):
        ops.flow_head(x.cpu(), ptr, *w)
    with pytest.raises(TypeError, match='flow_head: lin2_b must be a float32 tensor on the GPU'):
        ops.flow_head(x, ptr, w[0], w[1], w[2], w[3].cpu())
    with pytest.raises(TypeError, match='flow_head: ptr_dev must be an int64 tensor on the GPU'):
        ops.flow_head(x, ptr.cpu(), *w)
    with pytest.raises(TypeError, match='flow_head: lin1_w must be a 2-D float32 tensor with contiguous rows'):
        ops.flow_head(x, ptr, w[0].t(), *w[1:])
    with pytest.raises(TypeError, match='flow_head: lin2_w must be a contiguous 2-D float32 tensor'):
        ops.flow_head(x, ptr, w[0], w[1], torch.zeros(O, 2 * K, device=DEV)[:, :K], w[3])
    with pytest.raises(ValueError, match='ptr_dev holds C . 1 row offsets .3 entries'):
        ops.flow_head(x, torch.zeros(4, dtype=torch.long, device=DEV), *w, n_cochains=2)
    with pytest.raises(ValueError, match='ptr_dev holds'):
        ops.flow_head(x, torch.zeros(0, dtype=torch.long, device=DEV), *w)
    big = _dev(*_weights(129, O, seed=0))
    with pytest.raises(ValueError, match='1 <= K, H <= 128'):
        ops.flow_head(torch.zeros(7, 129, device=DEV), ptr, *big)
    wide = _dev(*_weights(K, 65, seed=0))
    with pytest.raises(ValueError, match='1 <= O <= 64'):
        ops.flow_head(x, ptr, *wide)
    assert not ops.flow_head_applies(x.double(), ptr, *w) and not ops.flow_head_applies(x.cpu(), ptr, *w)
    assert not ops.flow_head_applies(x, ptr, *wide) and ops.flow_head_applies(x, ptr, *w)


# ---- through the models ---------------------------------------------------------------------------------------------------
_FLOWS = {}


def _flows(flip=None):
    key = None if flip is None else tuple(flip.tolist())
    if key not in _FLOWS:
        cs = edge_flows(4, side=6, seed=2, flip=flip)
        _FLOWS[key] = (cs, packed.PackedCochains(cs, DEV))
    return _FLOWS[key]


class _switch:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.prev, models.FUSED_FLOW_HEAD = models.FUSED_FLOW_HEAD, self.on

    def __exit__(self, *exc):
        models.FUSED_FLOW_HEAD = self.prev
        return False


MODELS = [('orient', 'id', False, 'sum'), ('orient', 'tanh', False, 'sum'), ('orient', 'relu', False, 'sum'),
          ('orient', 'id', True, 'sum'), ('orient', 'tanh', True, 'sum'), ('orient', 'relu', True, 'sum'),
          ('mpnn', 'relu', True, 'sum'), ('mpnn', 'relu', False, 'sum'), ('orient', 'tanh', False, 'mean'), ('mpnn', 'relu', True, 'mean')]


@pytest.mark.parametrize('kind,act,invar,readout', MODELS)
def test_models_fused_head_matches_the_generic_route(kind, act, invar, readout):
    _, pc = _flows()
    torch.manual_seed(3)
    cls = models.EdgeOrient if kind == 'orient' else models.EdgeMPNN
    model = cls(1, 2, 3, 16, nonlinearity=act, readout=readout, fully_invar=invar).to(DEV)
    idx = [2, 0, 3, 1]
    for training in (False, True):
        model.train(training)
        res = {}
        for on in (False, True):
            model.zero_grad(set_to_none=True)
            with _switch(on), torch.set_grad_enabled(training):
                y = model(pc.collate(idx))
                if training:
                    y.square().sum().backward()
            assert model.last_head_route == ('fused' if on else 'generic')
            res[on] = (y.detach(), {k: p.grad.clone() for k, p in model.named_parameters()} if training else {})
        gate(res[True][0], res[False][0].double(), f'{kind} {act} invar {invar} {readout} training {training}: predictions')
        for k, gref in res[False][1].items():
            gate(res[True][1][k], gref.double(), f'{kind} {act} invar {invar} {readout}: grad {k}')
        assert float(res[False][0].abs().max()) > 1e-4


def test_the_generic_route_keeps_what_the_head_does_not_take():
    cs, pc = _flows()
    idx = [0, 1, 2, 3]
    model = models.EdgeOrient(1, 2, 2, 16, nonlinearity='tanh').to(DEV).eval()
    with torch.no_grad():
        with _switch(False):
            model(pc.collate(idx))
            assert model.last_head_route == 'generic'
        with _switch(True):
            model(pc.collate(idx))
            assert model.last_head_route == 'fused'
            y, cells = model(pc.collate(idx), include_partial=True)
            assert model.last_head_route == 'generic' and cells.shape == (pc.collate(idx).num_cells, 16)
            model(CochainBatch.from_cochain_list([cs[i] for i in idx]).to(DEV))
            assert model.last_head_route == 'generic'                 # a host-collated batch: no ptr_dev
            drop = models.EdgeOrient(1, 2, 2, 16, dropout_rate=0.5, nonlinearity='tanh').to(DEV).train()
            drop(pc.collate(idx))
            assert drop.last_head_route == 'generic'                  # active dropout
            drop.eval()
            drop(pc.collate(idx))
            assert drop.last_head_route == 'fused'
            dbl = models.EdgeOrient(1, 2, 2, 16, nonlinearity='tanh').to(DEV).double().eval()
            b = pc.collate(idx)
            b.x = b.x.double()
            b.upper_orient, b.lower_orient = b.upper_orient.double(), b.lower_orient.double()
            dbl(b)
            assert dbl.last_head_route == 'generic'                   # float64


@pytest.mark.parametrize('act', ['id', 'tanh'])
def test_orientation_equivariance_through_the_fused_head(act):
    """On edge_flows(4, side=6) under a random change of edge orientations the predictions do not move, inside the gate."""
    _, base = _flows()
    E = base.meta['n_cells'][0]
    t = np.random.default_rng(3).integers(0, 2, int(E)) * 2 - 1
    _, flipped = _flows(t)
    torch.manual_seed(1)
    model = models.EdgeOrient(1, 2, 4, 16, nonlinearity=act).to(DEV).eval()
    with _switch(True), torch.no_grad():
        y0 = model(base.collate([0, 1, 2, 3]))
        y1 = model(flipped.collate([0, 1, 2, 3]))
        assert model.last_head_route == 'fused'
    gate(y1, y0.double(), f'{act}: predictions under a change of orientation')
    assert float(y0.abs().max()) > 1e-3
