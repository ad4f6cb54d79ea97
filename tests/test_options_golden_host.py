"""tests/golden/cell_options.npz and tests/golden/gin_family.npz on the CPU: the reference's own models at non-ReLU
nonlinearities, graph_norm 'ln' / 'id', jump_mode 'max', and the graph baselines (tools/gen_golden_options.py).

  * the oracle, with its `act` argument, in float64 against every cell-model case;
  * the restatements tests/_gin.py and tests/_gine.py -- the yardsticks of the GPU tests of the graph baselines -- from the
    stored states against the reference's outputs;
  * the product's CPU paths of the graph baselines: the stored state loaded strictly, float32 against `out32`, float64 against
    `out64`, and the training gradients of GIN (elu);
  * the generator's --check.

Gates are the project's (tests/_product.gate): float64 1e-11 * max(1, |ref|_inf), float32 1e-5 * max(1, |ref|_inf)."""
import os
import re
import subprocess
import sys

import pytest
import torch

from oracle import cwn_oracle as O
from tests import _gin, _gine, _options as X
from tests._golden import load, T, dummy_complex, state_dict
from tests._product import gate, to_double

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
TOL64 = 1e-11


# ------------------------------------------------------------------------------------------------
# 1. the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', X.CELL_CASES)
def test_oracle_reproduces_the_reference_in_float64(case):
    c = X.cfg(X.CELL, case)
    y, partial = O.sparse_cin_model_forward(to_double(X.state(X.CELL, case)), X.oracle_cx(X.CELL, c['inputs']), **X.oracle_kwargs(c))
    ref = X.partials(X.CELL, case)
    assert ref and set(ref) <= set(partial), set(ref) - set(partial)
    if c['cls'] != 'EmbedSparseCINNoRings':              # (its forward has no include_partial: the layers' outputs alone)
        assert set(ref) == set(partial)
    for k, v in ref.items():
        assert partial[k].dtype == F64
        gate(partial[k], v, f'oracle {case} {k}', tol=TOL64)
    gate(y, X.out64(X.CELL, case), f'oracle {case} out', tol=TOL64)


def test_oracle_act_table_is_the_settings_of_the_cases():
    """Every entry of the oracle's table is exercised by a case, and a wrong entry would show: with another activation the
    oracle misses the fixture."""
    used = {X.cfg(X.CELL, case)['kw']['nonlinearity'] for case in X.CELL_CASES}
    assert used == set(O.ACTS) == {'relu', 'elu', 'tanh', 'sigmoid', 'id'}
    c = X.cfg(X.CELL, 'elu_bn_cob')
    kw = dict(X.oracle_kwargs(c), act='relu')
    y, _ = O.sparse_cin_model_forward(to_double(X.state(X.CELL, 'elu_bn_cob')), X.oracle_cx(X.CELL, 'mol'), **kw)
    assert float((y - X.out64(X.CELL, 'elu_bn_cob')).abs().max()) > 1e-3


def test_oracle_defaults_are_relu_bit_for_bit():
    """The default arguments are the ReLU oracle: on the existing ReLU fixtures the call without `act` equals the call with
    act='relu' bit for bit, layer functions included, and still reproduces the reference's outputs."""
    names = [str(n) for n in load('dummy_complexes.npz')['lists/mol']]
    for fixture, tag, kw in (('embed_sparse_cin.npz', 'h32_l4', {}), ('embed_cinpp.npz', 'h16_l2', dict(conv='cinpp'))):
        g = load(fixture)
        L = int(g[f'{tag}/meta'][1])
        st = state_dict(g, f'{tag}/state')
        for mode in ('eval', 'train'):
            outs = []
            for extra in ({}, dict(act='relu')):
                cx = O.batch_complexes([dummy_complex(n) for n in names], max_dim=2)
                cx['cochains'][0]['x'], cx['cochains'][1]['x'], cx['cochains'][2]['x'] = T(g[f'{tag}/v_types']), T(g[f'{tag}/e_types']), None
                outs.append(O.sparse_cin_model_forward(st, cx, L, training=(mode == 'train'), **kw, **extra))
            assert torch.equal(outs[0][0], outs[1][0])
            for k, v in outs[0][1].items():
                assert torch.equal(v, outs[1][1][k]), k
                torch.testing.assert_close(v, T(g[f'{tag}/{mode}/{k}']), rtol=1e-4, atol=1e-4)
    g = load('sparse_cin_conv.npz')
    from tests._golden import params_dict
    p = {k[len('mp_levels.1.'):]: v for k, v in state_dict(g, 'mol_cob_bn/state').items() if k.startswith('mp_levels.1.')}
    prm = params_dict(load('batching.npz'), 'mol/params_nodown/1')
    F = int(g['mol_cob_bn/meta'][0])
    prm['x'] = T(g['mol_cob_bn/x/1'])
    prm['up_attr'] = T(g['mol_cob_bn/x/2'])[O.batch_complexes([dummy_complex(n) for n in names])['cochains'][1]['shared_coboundaries']]
    prm['boundary_attr'] = T(g['mol_cob_bn/x/0'])
    assert prm['x'].size(1) == F
    a, b = O.sparse_cin_cochain_conv(p, prm, True), O.sparse_cin_cochain_conv(p, prm, True, act='relu')
    assert torch.equal(a, b)
    torch.testing.assert_close(a, T(g['mol_cob_bn/eval/1']), rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------------------------------------
# 2. the restatements of tests/_gin.py and tests/_gine.py
# ------------------------------------------------------------------------------------------------
def _graph64(case):
    d = X.graph_data(case, F64)
    return d, 5


@pytest.mark.parametrize('case', X.GIN_CASES)
def test_gin_restatement_reproduces_the_reference(case):
    c = X.cfg(X.GIN, case)
    d, size = _graph64(case)
    st = to_double(X.state(X.GIN, case))
    kw = dict(act=c['kw']['nonlinearity'], readout=c['kw']['readout'], jump=c['kw'].get('mode'))
    y, cells = _gin.gin_model64(st, d.x, d.edge_index, d.batch, size, partial=True, **kw)
    gate(y, X.out64(X.GIN, case), f'_gin.gin_model64 {case} out', tol=TOL64)
    ref = X.partials(X.GIN, case)
    L = c['args'][1]
    assert set(ref) == {f'layer{i}' for i in range(L)}
    x = d.x
    for i, prefix in enumerate(['conv1'] + [f'convs.{j}' for j in range(L - 1)]):
        x = _gin.conv64(st, prefix, x, d.edge_index, kw['act'])
        gate(x, ref[f'layer{i}'], f'_gin.conv64 {case} layer {i}', tol=TOL64)
    if kw['jump'] is None:
        gate(cells, ref[f'layer{L - 1}'], f'_gin.gin_model64 {case} cells', tol=TOL64)


@pytest.mark.parametrize('case', X.RING_CASES)
def test_ring_gin_restatement_reproduces_the_reference(case):
    c = X.cfg(X.GIN, case)
    d, _ = _graph64(case)
    st = to_double(X.state(X.GIN, case))
    assert ('conv1.nn.1.running_mean' in st) == (c['kw']['graph_norm'] == 'bn')
    y = _gin.ring_gin64(st, d.x, d.edge_index, d.mask, act=c['kw']['nonlinearity'])
    gate(y, X.out64(X.GIN, case), f'_gin.ring_gin64 {case} out', tol=TOL64)


def _egin_args(case):
    c = X.cfg(X.GIN, case)
    cx = X.oracle_cx(X.GIN, c['inputs'])
    v = cx['cochains'][0]
    e = cx['cochains'][1] if len(cx['cochains']) > 1 and v['upper_index'] is not None else None
    args = (v['x'], None if e is None else e['x'], None if e is None else e['boundary_index'], 0 if e is None else e['num_cells'],
            v['upper_index'], None if e is None else v['shared_coboundaries'], v['batch'], int(v['batch'].max()) + 1)
    kw = dict(act=c['kw']['nonlinearity'], readout=c['kw']['readout'], init_reduce=c['kw']['init_reduce'])
    return c, args, kw


@pytest.mark.parametrize('case', X.EGIN_CASES)
def test_embed_gin_restatement_reproduces_the_reference(case):
    c, args, kw = _egin_args(case)
    assert (args[4] is None) == (case == 'egin_nodes_only') and (args[1] is None) == (case in ('egin_noedge', 'egin_nodes_only'))
    y, cells = _gine.embed_gin64(to_double(X.state(X.GIN, case)), *args, partial=True, **kw)
    gate(y, X.out64(X.GIN, case), f'_gine.embed_gin64 {case} out', tol=TOL64)
    ref = X.partials(X.GIN, case)
    gate(cells, ref[f'layer{len(ref) - 1}'], f'_gine.embed_gin64 {case} cells', tol=TOL64)


# ------------------------------------------------------------------------------------------------
# 3. the product on the CPU
# ------------------------------------------------------------------------------------------------
def _product_layers(model, run, ring=False):
    seen = {}
    hooks = X.hook_layers(([model.conv1] if hasattr(model, 'conv1') else []) + list(model.convs), seen)
    with torch.no_grad():
        y = run(model)
    for h in hooks:
        h.remove()
    return y, seen


def _check_product(case, run, ring_act=None):
    ref = X.partials(X.GIN, case)
    if ring_act is not None:                 # RingGIN's first layer applies the activation once more (act(conv1), :121) inside
        ref = dict(ref, layer0=_gin.ACT64[ring_act](ref['layer0']))       # the product's conv1: the hook sees it applied
    m32 = X.product_model(X.GIN, case)
    y, seen = _product_layers(m32, lambda m: run(m, F32))
    assert y.dtype == F32
    gate(y, X.out32(X.GIN, case), f'{case} CPU float32 vs the reference float32', tol=1e-5)
    gate(y, X.out64(X.GIN, case), f'{case} CPU float32 vs the reference float64', tol=1e-5)
    for k, v in ref.items():
        gate(seen[k], v, f'{case} CPU float32 {k}', tol=1e-5)
    m64 = X.product_model(X.GIN, case, F64)
    y, seen = _product_layers(m64, lambda m: run(m, F64))
    assert y.dtype == F64 and set(seen) == set(ref)
    gate(y, X.out64(X.GIN, case), f'{case} CPU float64', tol=TOL64)
    for k, v in ref.items():
        gate(seen[k], v, f'{case} CPU float64 {k}', tol=TOL64)


@pytest.mark.parametrize('case', X.GIN_CASES + X.RING_CASES)
def test_product_graph_models_on_the_cpu(case):
    c = X.cfg(X.GIN, case)
    _check_product(case, lambda m, dtype: m(X.graph_data(case, dtype)), ring_act=c['kw']['nonlinearity'] if c['cls'] == 'RingGIN' else None)


@pytest.mark.parametrize('case', X.EGIN_CASES)
def test_product_embed_gin_on_the_cpu(case):
    kind = X.cfg(X.GIN, case)['inputs']
    _check_product(case, lambda m, dtype: m(X.product_batch(X.GIN, kind)))


def test_product_gin_training_gradients_on_the_cpu():
    """GIN (elu) in train() mode in float64: the output, and every parameter's gradient for loss = (out * c).sum() with the stored
    cotangent, within 1e-11 of the stored gradient's max-norm.  The bias of a Linear that feeds a train-mode BatchNorm (`nn.0.bias`,
    `nn.3.bias`) has the exact gradient 0 -- the norm subtracts the batch mean -- and what the reference stored for it is its own
    float64 summation noise (about 1e-17): a bound relative to that noise would compare two roundings.  Those gradients are held
    to 1e-11 of the max-norm of the same Linear's WEIGHT gradient, the sum of the same dz rows against O(1) inputs."""
    ref_out, cot, grads, _ = X.training(X.GIN, 'gin_elu')
    model = X.product_model(X.GIN, 'gin_elu', F64).train()
    out = model(X.graph_data('gin_elu', F64))
    (out * cot).sum().backward()
    gate(out, ref_out, 'gin_elu CPU float64 training output', tol=TOL64)
    params = dict(model.named_parameters())
    assert set(grads) == {k for k, p in params.items() if p.grad is not None} == set(params)
    for k, r in grads.items():
        err, scale = float((params[k].grad - r).abs().max()), float(r.abs().max())
        if re.search(r'\.nn\.[03]\.bias$', k):
            assert scale < 1e-13, (k, scale)                            # noise around an exact zero, as said above
            scale = float(grads[k[:-len('bias')] + 'weight'].abs().max())
        print(f'[grad] gin_elu {k}: max|delta| = {err:.3e}  scale = {scale:.3g}')
        assert err <= TOL64 * scale, (k, err, scale)


# ------------------------------------------------------------------------------------------------
# 4. the generator
# ------------------------------------------------------------------------------------------------
def test_generator_check_passes():
    """tools/gen_golden_options.py --check: both committed fixtures regenerate byte for byte from the reference (where the
    reference tree is present: it is read on the machine that writes fixtures, never on the GPU box)."""
    ref = re.search(r"^REF = '([^']+)'", open(os.path.join(ROOT, 'oracle', 'gen_golden.py')).read(), re.M).group(1)
    if not os.path.isdir(ref):
        pytest.skip('the reference tree is not on this machine')
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_golden_options.py'), '--check'], capture_output=True,
                         text=True, cwd=ROOT)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.count('regenerate bit-exactly') == 2


def test_fixture_files_stay_under_the_size_limit():
    from tests._golden import GOLD, parts
    for name in (X.CELL, X.GIN):
        for part in parts(name):
            assert os.path.getsize(os.path.join(GOLD, part)) < (1 << 20), part
