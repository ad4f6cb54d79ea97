"""The float64 dense path on the GPU (csrc/cwn_dense_f64.hip): ops.linear_many_f64 and ops.update_chain_f64 against the
same torch.nn modules / torch.nn.functional.linear evaluated in float64 on the CPU through the project's float64 gate
(tests/_product.gate, tol 1e-11: max|delta| <= 1e-11 * max(1, |ref|_inf)), the row independence of both kernels bit for
bit, whole double models with the route on against the route off, and which route a model takes."""
import copy

import numpy as np
import pytest
import torch
from torch.nn import BatchNorm1d, Identity, Linear, Sequential

from tests._product import gate

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F64 = torch.float64
TOL = 1e-11
ACTS = {'id': torch.nn.Identity, 'relu': torch.nn.ReLU, 'elu': torch.nn.ELU, 'tanh': torch.nn.Tanh, 'sigmoid': torch.nn.Sigmoid}


@pytest.fixture(scope='module', autouse=True)
def _native_loaded():
    from cwn_amd import _ffi
    assert _ffi.lib().cwn_target_arch() == b'gfx950'
    assert torch.cuda.is_available()


@pytest.fixture(autouse=True)
def _no_device_side_errors():
    yield
    from cwn_amd import csr
    csr.check_errors(torch.device(DEV))


def _tile():
    from cwn_amd import _ffi
    return _ffi.DENSE_F64_TILE_ROWS


# ------------------------------------------------------------------------------------------------
# 1. linear_many_f64 against torch.nn.functional.linear
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', list(ACTS))
def test_linear_many_every_shape_against_f_linear(act):
    """M in {0, 1, 33} x K in {1, 2, 16, 48, 64, 128} x N in {1, 16, 64, 128}, with and without bias: 144 products, 16 per
    launch (products of different shapes share every launch)."""
    from cwn_amd import ops
    g = torch.Generator().manual_seed(len(act))
    items, refs, tags = [], [], []
    fn = ACTS[act]()
    for M in (0, 1, 33):
        for K in (1, 2, 16, 48, 64, 128):
            for N in (1, 16, 64, 128):
                for has_bias in (True, False):
                    x, w = torch.randn(M, K, generator=g, dtype=F64), torch.randn(N, K, generator=g, dtype=F64)
                    b = torch.randn(N, generator=g, dtype=F64) if has_bias else None
                    refs.append(fn(torch.nn.functional.linear(x, w, b)))
                    items.append((x.to(DEV), w.to(DEV), None if b is None else b.to(DEV), act))
                    tags.append((M, K, N, has_bias))
    outs = ops.linear_many_f64(items)
    assert len(outs) == len(refs)
    worst = 0.0
    for y, r, tag in zip(outs, refs, tags):
        assert y.dtype == F64 and y.shape == r.shape, tag
        assert bool(torch.isfinite(y).all()), tag
        if r.numel():
            err = float((y.cpu() - r).abs().max())
            scale = max(1.0, float(r.abs().max()))
            worst = max(worst, err / scale)
            assert err <= TOL * scale, (act, tag, err, scale)
    print(f'[gate] linear_many_f64 {act}: 144 products, worst max|delta| / max(1, |ref|_inf) = {worst:.3e} (bound {TOL:g})')


def test_linear_many_one_product_seven_products_and_weight_slices():
    from cwn_amd import ops
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    # one product
    x, w, b = r(33, 48), r(16, 48), r(16)
    y, = ops.linear_many_f64([(x.to(DEV), w.to(DEV), b.to(DEV), 'elu')])
    gate(y, torch.nn.functional.elu(torch.nn.functional.linear(x, w, b)), 'linear_many_f64, one product', tol=TOL)
    # seven of different shapes, acts and bias, one of them empty, one with a code for its activation; every x a strided view
    shapes = [(33, 16, 16, 'relu', True), (1, 128, 128, 'tanh', False), (0, 5, 7, 'elu', True), (17, 1, 64, 'sigmoid', True),
              (40, 64, 1, None, False), (16, 2, 33, 2, True), (65, 100, 100, 'id', True)]
    items, refs = [], []
    for M, K, N, act, hb in shapes:
        wide, w, b = r(M, K + 3), r(N, K), (r(N) if hb else None)
        wide[:, 0] = wide[:, K + 1:] = float('nan')                  # (beside the window: nothing of it reaches a result)
        x, xd = wide[:, 1:K + 1], wide.to(DEV)[:, 1:K + 1]          # x is a view with a row stride of K + 3
        assert M < 2 or xd.stride(0) == K + 3
        name = {None: 'id', 2: 'elu'}.get(act, act)
        refs.append(ACTS[name]()(torch.nn.functional.linear(x, w, b)))
        items.append((xd, w.to(DEV), None if b is None else b.to(DEV), act))
    outs = ops.linear_many_f64(items)
    for i, (y, ref) in enumerate(zip(outs, refs)):
        assert y.shape == ref.shape
        gate(y, ref, f'linear_many_f64, product {i} of 7 {shapes[i]}', tol=TOL)
    # the message weight [F, 2F] as its two column slices (ldw = 2F)
    for F in (1, 16, 64):
        W, bias, xa, xb = r(F, 2 * F), r(F), r(37, F), r(21, F)
        Wd = W.to(DEV)
        assert F == 1 or not Wd[:, F:].is_contiguous()
        y1, y2 = ops.linear_many_f64([(xa.to(DEV), Wd[:, :F], bias.to(DEV), None), (xb.to(DEV), Wd[:, F:], None, None)])
        gate(y1, torch.nn.functional.linear(xa, W[:, :F], bias), f'message product Y1, F = {F}', tol=TOL)
        gate(y2, torch.nn.functional.linear(xb, W[:, F:]), f'message product Y2, F = {F}', tol=TOL)


# ------------------------------------------------------------------------------------------------
# 2. update_chain_f64 against the layer's own three Sequentials
# ------------------------------------------------------------------------------------------------
def _networks(F, H, norm, act, seed):
    """update_up_nn, update_boundaries_nn, combine_nn as SparseCINConv builds them, in double, eval mode; BatchNorm with
    non-trivial running statistics and affine."""
    from cwn_amd.layers import _update_mlp
    torch.manual_seed(seed)
    nets = [_update_mlp(F, H, norm, ACTS[act]), _update_mlp(F, H, norm, ACTS[act]),
            Sequential(Linear(2 * H, H), norm(H), ACTS[act]())]
    g = torch.Generator().manual_seed(seed + 1)
    for net in nets:
        net.double().eval()
        for m in net:
            if isinstance(m, BatchNorm1d):
                with torch.no_grad():
                    m.running_mean.copy_(torch.randn(H, generator=g, dtype=F64))
                    m.running_var.copy_(torch.rand(H, generator=g, dtype=F64) + 0.5)
                    m.weight.copy_(torch.randn(H, generator=g, dtype=F64))
                    m.bias.copy_(torch.randn(H, generator=g, dtype=F64))
    return nets


def _chain_dim(nets_dev, in_up, in_b, act, out=None):
    from cwn_amd import layers, ops
    up, bd, cb = nets_dev
    stages = [(up[0], up[1]), (up[3], up[4]), (bd[0], bd[1]), (bd[3], bd[4]), (cb[0], cb[1])]
    folds = [layers._fold_norm(norm, lin.out_features) for lin, norm in stages]
    assert all(f is not None for f in folds)
    return ops.ChainDim(in_up=in_up, in_b=in_b, weights=[lin.weight for lin, _ in stages], biases=[lin.bias for lin, _ in stages],
                        folds=folds, act=act, out=out)


def _reference(nets, in_up, in_b):
    with torch.no_grad():
        return nets[2](torch.cat([nets[0](in_up), nets[1](in_b)], dim=-1))


@pytest.mark.parametrize('norm', [Identity, BatchNorm1d], ids=['id', 'bn'])
@pytest.mark.parametrize('F,H', [(1, 16), (5, 16), (16, 16), (48, 48), (64, 64), (16, 64)])
def test_update_chain_against_the_sequentials(F, H, norm):
    """Every activation; launches of 1, 2 and 3 dimensions with rows from {0, 1, R-1, R, R+1, 3R+7} (a middle dimension
    empty); outputs into NaN-filled buffers with three spare rows: live rows finite and within the gate, spare rows NaN."""
    from cwn_amd import ops
    R = _tile()
    launches = [(3 * R + 7,), (1, R - 1), (R, 0, R + 1), (0,), (R + 1, 3 * R + 7, 1)]
    g = torch.Generator().manual_seed(F * 100 + H)
    worst = 0.0
    with torch.no_grad():
        for act in ACTS:
            nets = [_networks(F, H, norm, act, seed=d + len(act)) for d in range(3)]
            nets_dev = [[copy.deepcopy(n).to(DEV) for n in nd] for nd in nets]
            for rows in launches:
                dims, refs, bufs = [], [], []
                for d, n in enumerate(rows):
                    in_up, in_b = torch.randn(n, F, generator=g, dtype=F64), torch.randn(n, F, generator=g, dtype=F64)
                    refs.append(_reference(nets[d], in_up, in_b))
                    bufs.append(torch.full((n + 3, H), float('nan'), dtype=F64, device=DEV))
                    dims.append(_chain_dim(nets_dev[d], in_up.to(DEV), in_b.to(DEV), act, out=bufs[-1]))
                assert ops.update_chain_f64_applies(dims)
                outs = ops.update_chain_f64(dims)
                for d, (n, y, ref, buf) in enumerate(zip(rows, outs, refs, bufs)):
                    tag = (act, rows, d)
                    assert y.shape == (n, H) and (n == 0 or y.data_ptr() == buf.data_ptr()), tag   # (an empty tensor has no address)
                    host = buf.cpu()
                    assert bool(torch.isnan(host[n:]).all()), tag                       # spare rows untouched
                    assert bool(torch.isfinite(host[:n]).all()), tag
                    if n:
                        err = float((host[:n] - ref).abs().max())
                        scale = max(1.0, float(ref.abs().max()))
                        worst = max(worst, err / scale)
                        assert err <= TOL * scale, (tag, err, scale)
    print(f'[gate] update_chain_f64 F {F} H {H} {norm.__name__}: worst max|delta| / max(1, |ref|_inf) = {worst:.3e} (bound {TOL:g})')


def test_update_chain_allocates_its_outputs_and_takes_strided_inputs():
    from cwn_amd import ops
    F, H, n = 5, 16, 40
    nets = _networks(F, H, BatchNorm1d, 'elu', seed=3)
    nets_dev = [copy.deepcopy(m).to(DEV) for m in nets]
    g = torch.Generator().manual_seed(4)
    wide_up, wide_b = torch.randn(n, F + 4, generator=g, dtype=F64), torch.randn(n, F + 2, generator=g, dtype=F64)
    wide_up[:, :2] = wide_up[:, 2 + F:] = wide_b[:, F:] = float('nan')      # (beside the windows: nothing of it reaches a result)
    in_up, in_b = wide_up.to(DEV)[:, 2:2 + F], wide_b.to(DEV)[:, :F]
    assert in_up.stride(0) == F + 4 and in_b.stride(0) == F + 2
    with torch.no_grad():
        y, = ops.update_chain_f64([_chain_dim(nets_dev, in_up, in_b, 'elu')])
    assert y.shape == (n, H) and y.is_contiguous()
    gate(y, _reference(nets, wide_up[:, 2:2 + F], wide_b[:, :F]), 'update_chain_f64, strided inputs, own output', tol=TOL)


def test_operands_without_contiguous_rows_are_refused_with_their_whole_message():
    """The shape / stride clause of the operand check (the dtype and device clauses: tests/test_operand_messages_host.py), the
    messages as literals recorded before the ops shared one checker.  Nothing is launched."""
    from cwn_amd import ops
    z = lambda *s: torch.zeros(*s, dtype=F64, device=DEV)
    x, w, b = z(4, 3), z(2, 3), z(2)
    F, H, n = 3, 4, 5
    chain = lambda **over: [ops.ChainDim(**{**dict(
        in_up=z(n, F), in_b=z(n, F), weights=[z(H, F), z(H, H), z(H, F), z(H, H), z(H, 2 * H)], biases=[z(H) for _ in range(5)],
        folds=[(z(H), z(H)) for _ in range(5)], act='relu'), **over})]
    cases = [
        (lambda: ops.linear_many_f64([(z(3, 4).t(), w, b, 'id')]),
         'x[0] must be a 2-D float64 tensor with contiguous rows (got torch.float64, shape (4, 3), strides (1, 4))'),
        (lambda: ops.linear_many_f64([(x, z(3), b, 'id')]),
         'weight[0] must be a 2-D float64 tensor with contiguous rows (got torch.float64, shape (3,), strides (1,))'),
        (lambda: ops.update_chain_f64(chain(in_b=z(F, n).t())),
         'dims[0].in_b must be a 2-D float64 tensor with contiguous rows (got torch.float64, shape (5, 3), strides (1, 5))'),
        (lambda: ops.update_chain_f64(chain(weights=[z(H, F), z(H), z(H, F), z(H, H), z(H, 2 * H)])),
         'dims[0].weights[1] must be a 2-D float64 tensor with contiguous rows (got torch.float64, shape (4,), strides (1,))'),
    ]
    for call, message in cases:
        with pytest.raises(TypeError) as got:
            call()
        assert type(got.value) is TypeError and str(got.value) == message
    assert not ops.update_chain_f64_applies(chain(in_b=z(F, n).t()))


# ------------------------------------------------------------------------------------------------
# 3. row independence, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,H,norm,act', [(16, 16, Identity, 'elu'), (64, 64, BatchNorm1d, 'tanh'), (5, 48, Identity, 'sigmoid')])
def test_update_chain_row_independence(F, H, norm, act):
    """Identical input rows at 0, R-1, R and the last row give bit-identical output rows, equal to the output of a 1-row
    launch of that row -- alone, and as the second dimension of a 3-dimension launch."""
    from cwn_amd import ops
    R = _tile()
    n = 3 * R + 7
    marked = [0, R - 1, R, n - 1]
    nets_dev = [[m.to(DEV) for m in _networks(F, H, norm, act, seed=20 + d)] for d in range(3)]
    g = torch.Generator().manual_seed(F + H)
    in_up, in_b = torch.randn(n, F, generator=g, dtype=F64), torch.randn(n, F, generator=g, dtype=F64)
    in_up[marked], in_b[marked] = in_up[0].clone(), in_b[0].clone()
    in_up, in_b = in_up.to(DEV), in_b.to(DEV)
    other = lambda rows: (torch.randn(rows, F, generator=g, dtype=F64).to(DEV), torch.randn(rows, F, generator=g, dtype=F64).to(DEV))
    with torch.no_grad():
        one, = ops.update_chain_f64([_chain_dim(nets_dev[1], in_up[:1].clone(), in_b[:1].clone(), act)])
        alone, = ops.update_chain_f64([_chain_dim(nets_dev[1], in_up, in_b, act)])
        _, second, _ = ops.update_chain_f64([_chain_dim(nets_dev[0], *other(R + 5), act), _chain_dim(nets_dev[1], in_up, in_b, act),
                                             _chain_dim(nets_dev[2], *other(2), act)])
    assert one.shape == (1, H) and bool(torch.isfinite(one).all()) and float(one.abs().max()) > 0
    for name, y in (('alone', alone), ('second of three', second)):
        for r in marked:
            assert torch.equal(y[r], one[0]), (name, r)
    assert torch.equal(alone, second)


def test_linear_many_row_independence():
    from cwn_amd import ops
    R = _tile()
    g = torch.Generator().manual_seed(1)
    for K, N in ((16, 16), (100, 128), (3, 33)):
        n = 3 * R + 7
        marked = [0, R - 1, R, n - 1]
        x, w, b = torch.randn(n, K, generator=g, dtype=F64), torch.randn(N, K, generator=g, dtype=F64).to(DEV), torch.randn(N, generator=g, dtype=F64).to(DEV)
        x[marked] = x[0].clone()
        x = x.to(DEV)
        z = torch.randn(R + 3, 7, generator=g, dtype=F64).to(DEV)
        wz = torch.randn(5, 7, generator=g, dtype=F64).to(DEV)
        one, = ops.linear_many_f64([(x[:1].clone(), w, b, 'elu')])
        alone, = ops.linear_many_f64([(x, w, b, 'elu')])
        _, second, _ = ops.linear_many_f64([(z, wz, None, 'id'), (x, w, b, 'elu'), (z, wz, None, 'relu')])
        for y in (alone, second):
            for r in marked:
                assert torch.equal(y[r], one[0]), (K, N, r)
        assert torch.equal(alone, second)


# ------------------------------------------------------------------------------------------------
# 4. whole models: the route on against the route off; the reference's isomorphism criterion on the new route
# ------------------------------------------------------------------------------------------------
def _sr_batch(graphs=None, dtype=F64):
    """rook, Shrikhande and two random molecules, ring-lifted (rings up to 6), constant features."""
    from cwn_amd.complex import ComplexBatch
    from cwn_amd.synthetic import rook_4x4, shrikhande, random_molecule, sr_lift
    if graphs is None:
        rng = np.random.default_rng(3)
        graphs = [rook_4x4(), shrikhande(), random_molecule(rng), random_molecule(rng)]
    return ComplexBatch.from_complex_list([sr_lift(n, bonds, dtype=dtype) for n, bonds in graphs], max_dim=2)


def _model(hidden=16, layers=3, nonlinearity='elu', norm='id', dtype=F64, seed=0):
    from cwn_amd.models import SparseCIN
    torch.manual_seed(seed)
    m = SparseCIN(num_input_features=1, num_classes=16, num_layers=layers, hidden=hidden, dropout_rate=0.0, max_dim=2,
                  use_coboundaries=True, nonlinearity=nonlinearity, graph_norm=norm, readout='sum', final_readout='sum',
                  readout_dims=(0, 1, 2)).to(dtype)
    g = torch.Generator().manual_seed(seed + 1)
    for mod in m.modules():
        if isinstance(mod, BatchNorm1d):                # non-trivial running statistics and affine
            with torch.no_grad():
                mod.running_mean.copy_(torch.randn(mod.num_features, generator=g).to(dtype) * 0.1)
                mod.running_var.copy_((torch.rand(mod.num_features, generator=g) + 0.5).to(dtype))
                mod.weight.copy_((torch.rand(mod.num_features, generator=g) + 0.5).to(dtype))
                mod.bias.copy_(torch.randn(mod.num_features, generator=g).to(dtype) * 0.1)
    return m.to(DEV).eval()


class _Spy:
    """Counts the calls of ops.update_chain_f64 / ops.linear_many_f64 and passes them on."""

    def __init__(self, monkeypatch):
        from cwn_amd import ops
        self.chain, self.linear = 0, 0
        chain, linear = ops.update_chain_f64, ops.linear_many_f64

        def chain_spy(dims):
            self.chain += 1
            return chain(dims)

        def linear_spy(items):
            self.linear += 1
            return linear(items)
        monkeypatch.setattr(ops, 'update_chain_f64', chain_spy)
        monkeypatch.setattr(ops, 'linear_many_f64', linear_spy)


@pytest.mark.parametrize('hidden,nonlinearity,norm', [(16, 'elu', 'id'), (64, 'relu', 'bn')], ids=['sr-h16-elu-id', 'h64-relu-bn'])
def test_model_with_the_route_on_matches_the_route_off(monkeypatch, hidden, nonlinearity, norm):
    from cwn_amd import layers
    model = _model(hidden, 3, nonlinearity, norm)
    batch = _sr_batch().to(DEV)
    spy = _Spy(monkeypatch)
    with torch.no_grad():
        monkeypatch.setattr(layers, 'FUSED_F64_DENSE', False)
        y_off, res_off = model(_sr_batch().to(DEV), include_partial=True)
        assert spy.chain == 0 and spy.linear == 0
        monkeypatch.setattr(layers, 'FUSED_F64_DENSE', True)
        y_on, res_on = model(batch, include_partial=True)
    # one chain launch per layer; the head's lin1s and lin2; a ReLU model's message products too (two dimensions per layer)
    assert spy.chain == 3 and spy.linear == 2 + (6 if nonlinearity == 'relu' else 0)
    assert y_on.dtype == F64 and bool(torch.isfinite(y_on).all())
    for k, v in res_off.items():
        gate(res_on[k], v, f'SparseCIN h{hidden} {nonlinearity} {norm}: route on vs off, {k}', tol=TOL)
    gate(y_on, y_off, f'SparseCIN h{hidden} {nonlinearity} {norm}: route on vs off, prediction', tol=TOL)


def test_sr_criterion_holds_on_the_new_route(monkeypatch):
    """exp/test_sr.py:81-102 through the float64 launches: relabelled copies of a graph, each lifted on its own, land within
    0.01 of each other (torch.pdist); the rook's graph and the Shrikhande graph are told apart."""
    from cwn_amd.synthetic import rook_4x4, shrikhande, relabel
    model = _model(16, 3, 'elu', 'id', seed=0)
    spy = _Spy(monkeypatch)
    rng = np.random.default_rng(43)
    embs = []
    for graph in (rook_4x4(), shrikhande()):
        copies = [graph] + [relabel(*graph, rng.permutation(16)) for _ in range(3)]
        with torch.no_grad():
            out = model(_sr_batch(copies).to(DEV))
        dist = torch.pdist(out, p=2)
        print(f'[sr] pdist over the 4 copies: max {float(dist.max()):.3e}   max|embedding| {float(out.abs().max()):.4g}')
        assert float(dist.max()) <= 0.01
        embs.append(out[0])
    assert spy.chain == 6
    apart = float((embs[0] - embs[1]).norm())
    print(f'[sr] rook vs Shrikhande: {apart:.4g}')
    assert apart > 0.01


# ------------------------------------------------------------------------------------------------
# 5. the route is taken, or declined
# ------------------------------------------------------------------------------------------------
def test_route_taken_once_per_layer_and_declined_otherwise(monkeypatch):
    from cwn_amd import layers
    spy = _Spy(monkeypatch)
    batch = _sr_batch().to(DEV)
    with torch.no_grad():
        _model(16, 3)(batch)
    assert spy.chain == 3 and spy.linear == 2                       # one per layer; lin1s, lin2
    spy.chain = spy.linear = 0
    # autograd recording with trainable parameters
    model = _model(16, 2)
    assert torch.is_grad_enabled() and all(p.requires_grad for p in model.parameters())
    out = model(_sr_batch().to(DEV))
    assert out.requires_grad and spy.chain == 0 and spy.linear == 0
    with torch.no_grad():
        _model(256, 2)(_sr_batch().to(DEV))                          # hidden 256: dgemm
        assert spy.chain == 0
        _model(16, 2, norm='ln')(_sr_batch().to(DEV))                # LayerNorm
        assert spy.chain == 0
        spy.linear = 0                                               # (the heads of those two may take their launches)
        _model(16, 2, dtype=torch.float32)(_sr_batch(dtype=torch.float32).to(DEV))
        assert spy.chain == 0 and spy.linear == 0
        monkeypatch.setattr(layers, 'FUSED_F64_DENSE', False)
        _model(16, 2)(_sr_batch().to(DEV))
        assert spy.chain == 0 and spy.linear == 0
