"""tests/golden/cell_options.npz and tests/golden/gin_family.npz on the device: the reference's own models at non-ReLU
nonlinearities, graph_norm 'ln' / 'id', jump_mode 'max', and the graph baselines (tools/gen_golden_options.py) -- an
independent yardstick for what the route-on / route-off tests of tests/test_gpu_chain_f32.py, test_gpu_act_message.py,
test_gpu_f64_dense.py, test_gpu_gin.py and test_gpu_gine.py compare with the product itself.

Every case runs in float32 against the reference's FLOAT64 outputs (prediction and every stored per-layer tensor) within the
project's gate 1e-5 * max(1, |ref|_inf) -- the generator made sure that the reference's own float32 run sits within half of it
-- and in float64 within 1e-11 * max(1, |ref|_inf); each with the fused routes on and off, and the launches that the routes are
made of counted, so that a silent fall-back does not pass for coverage.  Reads tests/golden/ alone."""
import numpy as np
import pytest
import torch

from tests import _options as X
from tests._gin import ACT64
from tests._product import gate

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
TOL = {F32: 1e-5, F64: 1e-11}


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


class _Launches:
    """Counts, and passes on: the C entry point of the float32 chain, ops.update_chain_f64, ops.run_aggregate_act and the
    forward LayerNorm launch."""

    def __init__(self, monkeypatch):
        from cwn_amd import _ffi, ops
        self.reset()
        L = _ffi.lib()

        def chain32(arr, n, s, fn=L.cwn_update_chain_f32):
            self.chain32 += 1
            return fn(arr, n, s)

        def chain64(dims, fn=ops.update_chain_f64):
            self.chain64 += 1
            return fn(dims)

        def act(specs, device, fn=ops.run_aggregate_act):
            self.act += 1
            return fn(specs, device)

        def ln(descs, dev, fn=_ffi.layer_norm_act):
            self.ln += 1
            return fn(descs, dev)
        monkeypatch.setattr(L, 'cwn_update_chain_f32', chain32)
        monkeypatch.setattr(ops, 'update_chain_f64', chain64)
        monkeypatch.setattr(ops, 'run_aggregate_act', act)
        monkeypatch.setattr(_ffi, 'layer_norm_act', ln)

    def reset(self):
        self.chain32 = self.chain64 = self.act = self.ln = 0

    def counts(self):
        return dict(chain32=self.chain32, chain64=self.chain64, act=self.act, ln=self.ln)


def _switch(monkeypatch, on: bool):
    from cwn_amd import dense_ln, layers, ops
    monkeypatch.setattr(layers, 'FUSED_CHAIN_F32', True if on else frozenset())
    monkeypatch.setattr(layers, 'FUSED_ACT_MESSAGE', on)
    monkeypatch.setattr(layers, 'FUSED_F64_DENSE', on)
    monkeypatch.setattr(layers, 'FUSED_GIN', on)
    monkeypatch.setattr(layers, 'FUSED_GINE', on)
    monkeypatch.setattr(dense_ln, 'FUSED_LN', on)
    monkeypatch.setattr(ops, 'FUSED_ENDS', on)


# ------------------------------------------------------------------------------------------------
# 1. the cell-complex models
# ------------------------------------------------------------------------------------------------
# The launches a 2-layer model makes with every route on: the float32 chain (SparseCINConv with BatchNorm / Identity: regime
# 'act' for elu / tanh / sigmoid / id, 'relu_width' for ReLU at 16), the float64 chain (the same layers up to width 64), the
# activated coboundary message (act(Linear(cat)) other than ReLU, one launch per layer), the LayerNorm launch (ReLU networks:
# three stages per layer, at any width).
EXPECTED = {
    'elu_bn_cob': dict(chain32=2, chain64=2, act=2, ln=0),
    'tanh_ln_cat': dict(chain32=0, chain64=0, act=2, ln=0),
    'sigmoid_id': dict(chain32=2, chain64=2, act=0, ln=0),
    'id_bn': dict(chain32=2, chain64=2, act=2, ln=0),
    'sr_elu_bn_64': dict(chain32=2, chain64=2, act=2, ln=0),
    'cinpp_elu': dict(chain32=0, chain64=0, act=2, ln=0),
    'ogb_tanh': dict(chain32=2, chain64=2, act=2, ln=0),
    'norings_elu': dict(chain32=2, chain64=2, act=2, ln=0),
    'relu_ln_48': dict(chain32=0, chain64=0, act=0, ln=6),
    'relu_ln_10': dict(chain32=0, chain64=0, act=0, ln=6),       # (at 10 only the combine PRODUCT leaves the grouped GEMM: dense_ln.counted)
    'jk_max': dict(chain32=2, chain64=2, act=0, ln=0),
}


def _cell_forward(case, dtype):
    c = X.cfg(X.CELL, case)
    model = X.product_model(X.CELL, case, dtype).to(DEV)
    with torch.no_grad():
        y, res = model(X.product_batch(X.CELL, c['inputs'], dtype).to(DEV), include_partial=True)
    return y, res


def _check_cell(case, dtype, y, res, what):
    ref = X.partials(X.CELL, case)
    assert y.dtype == dtype and ref and set(ref) <= set(res), set(ref) - set(res)
    for k, v in ref.items():
        gate(res[k], v, f'{case} {what} {k}', tol=TOL[dtype])
    gate(y, X.out64(X.CELL, case), f'{case} {what} out', tol=TOL[dtype])


@pytest.mark.parametrize('case', X.CELL_CASES)
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_cell_model_matches_the_reference(monkeypatch, case, dtype):
    spy = _Launches(monkeypatch)
    _switch(monkeypatch, False)
    y, res = _cell_forward(case, dtype)
    assert spy.counts() == dict(chain32=0, chain64=0, act=0, ln=0), spy.counts()
    _check_cell(case, dtype, y, res, f'{dtype} routes off')
    _switch(monkeypatch, True)
    y, res = _cell_forward(case, dtype)
    want = dict(EXPECTED[case], chain32=0, ln=0) if dtype == F64 else dict(EXPECTED[case], chain64=0)
    print(f'[routes] {case} {dtype}: {spy.counts()}')
    assert spy.counts() == want, (spy.counts(), want)
    _check_cell(case, dtype, y, res, f'{dtype} routes on')


def test_sr_case_through_a_static_batch(monkeypatch):
    """Case 5 through StaticForward over a 'csr' static batch, every switch on.  A static batch declines the two launches of an
    ELU model -- the activated message and the float32 chain have no device-side row count (layers._up_kind,
    SparseCINConv._dense_chain_f32) -- so what it captures is the route those switches leave: the counts say so.  The replay
    equals the same forward as ordinary launches (StaticForward.eager) and the eager forward on the collated batch with the
    two launches off bit for bit; replay, that forward and the eager forward with the launches ON (another summation order:
    its distance from the replay is printed) each sit inside the gate against the reference."""
    from cwn_amd import csr
    from cwn_amd.packed import PackedComplexes
    from cwn_amd.static_batch import StaticBatch
    from cwn_amd.static_graph import StaticForward
    ref = X.out64(X.CELL, 'sr_elu_bn_64')
    spy = _Launches(monkeypatch)
    _switch(monkeypatch, True)
    pool = X.sr_complexes()
    p = PackedComplexes(pool, DEV, max_dim=2, with_csr=True)
    model = X.product_model(X.CELL, 'sr_elu_bn_64').to(DEV)
    idx = np.arange(len(pool))
    sb = StaticBatch(p, len(pool), slots=1, mode='csr')
    sf = StaticForward(model, sb)
    assert sb.fits([idx]).all()
    sb.set_epoch([idx])
    with torch.no_grad():
        out = sf.replay()[0][:len(idx)].clone()
        assert spy.counts() == dict(chain32=0, chain64=0, act=0, ln=0), spy.counts()
        sb.set_epoch([idx])
        plain = sf.eager()[0][:len(idx)].clone()
        assert spy.counts() == dict(chain32=0, chain64=0, act=0, ln=0), spy.counts()
        on = model(p.collate(idx))
        assert spy.counts() == dict(chain32=2, chain64=0, act=2, ln=0), spy.counts()
        _switch(monkeypatch, False)
        off = model(p.collate(idx))
    torch.cuda.synchronize()
    csr.check_errors(DEV)
    gate(out, ref, 'sr_elu_bn_64 static replay')
    gate(off, ref, 'sr_elu_bn_64 eager forward on the collated batch, launches off')
    gate(on, ref, 'sr_elu_bn_64 eager forward on the collated batch, launches on')
    print(f'[static] replay vs the eager forward with the launches on: max|delta| = {float((out - on).abs().max()):.3e}')
    assert torch.equal(out, plain), float((out - plain).abs().max())
    assert torch.equal(out, off), float((out - off).abs().max())


# ------------------------------------------------------------------------------------------------
# 2. the graph baselines
# ------------------------------------------------------------------------------------------------
def _graph_forward(model, data):
    seen = {}
    convs = ([model.conv1] if hasattr(model, 'conv1') else []) + list(model.convs)
    hooks = X.hook_layers(convs, seen)
    with torch.no_grad():
        y = model(data)
    for h in hooks:
        h.remove()
    return y, {k: v.clone() for k, v in seen.items()}, [c.last_route for c in convs]


def _check_graph(case, dtype, make_data, folds: bool, monkeypatch):
    c = X.cfg(X.GIN, case)
    ref = X.partials(X.GIN, case)
    if c['cls'] == 'RingGIN':                # act(conv1(x)) (mp/ring_exp_models.py:121) is applied inside the product's conv1
        ref = dict(ref, layer0=ACT64[c['kw']['nonlinearity']](ref['layer0']))
    model = X.product_model(X.GIN, case, dtype).to(DEV)
    for on in (False, True):
        _switch(monkeypatch, on)
        y, seen, routes = _graph_forward(model, make_data())
        want = 'fused' if on and dtype == F32 and folds else 'generic'
        print(f'[routes] {case} {dtype} switch {on}: {routes}')
        assert routes == [want] * len(routes) and len(routes) == len(ref), (routes, want)
        assert y.dtype == dtype and set(seen) == set(ref)
        for k, v in ref.items():
            gate(seen[k], v, f'{case} {dtype} switch {on} {k}', tol=TOL[dtype])
        gate(y, X.out64(X.GIN, case), f'{case} {dtype} switch {on} out', tol=TOL[dtype])


@pytest.mark.parametrize('case', X.GIN_CASES + X.RING_CASES)
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_graph_model_matches_the_reference(monkeypatch, case, dtype):
    folds = X.cfg(X.GIN, case)['kw'].get('graph_norm', 'bn') != 'ln'        # LayerNorm is no fixed affine: the generic route
    _check_graph(case, dtype, lambda: X.graph_data(case, dtype, DEV), folds, monkeypatch)


@pytest.mark.parametrize('case', X.EGIN_CASES)
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_embed_gin_matches_the_reference(monkeypatch, case, dtype):
    kind = X.cfg(X.GIN, case)['inputs']
    _check_graph(case, dtype, lambda: X.product_batch(X.GIN, kind).to(DEV), True, monkeypatch)


# ------------------------------------------------------------------------------------------------
# 3. training: one forward and backward against the reference's float64 autograd
# ------------------------------------------------------------------------------------------------
def _check_training(fixture, case, run):
    """The metric and bound of tests/test_gpu_parity.py::test_model_training_gradients_match_float64_oracle_autograd: the output
    within gate()'s 1e-5, every parameter gradient within gate(tol=2e-5)."""
    ref_out, cot, grads, _ = X.training(fixture, case)
    model = X.product_model(fixture, case).to(DEV).train()
    out = run(model)
    (out * cot.float().to(DEV)).sum().backward()
    gate(out.detach(), ref_out, f'{case} training output vs the reference float64')
    params = dict(model.named_parameters())
    assert set(grads) <= set(params)
    worst = 0.0
    for name, p in params.items():
        if name not in grads:            # a parameter the loss does not reach
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        assert p.grad is not None, name
        worst = max(worst, gate(p.grad, grads[name], f'{case} grad {name}', tol=2e-5))
    print(f'[gate] {case} training gradients vs the reference float64 autograd: worst max|delta| = {worst:.3e}')


def test_cell_model_training_gradients_match_the_reference():
    _check_training(X.CELL, 'elu_bn_cob', lambda m: m(X.product_batch(X.CELL, 'mol').to(DEV)))


def test_gin_training_gradients_match_the_reference():
    _check_training(X.GIN, 'gin_elu', lambda m: m(X.graph_data('gin_elu', F32, DEV)))
