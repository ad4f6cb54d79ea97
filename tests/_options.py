"""Loaders for tests/golden/cell_options.npz and tests/golden/gin_family.npz (tools/gen_golden_options.py: the reference's own
models at the options no other fixture covers).  Reads tests/golden/ alone."""
import json
from types import SimpleNamespace

import numpy as np
import torch

from tests._golden import load, T, complex_dict, state_dict

CELL, GIN = 'cell_options.npz', 'gin_family.npz'
CELL_CASES = ('elu_bn_cob', 'tanh_ln_cat', 'sigmoid_id', 'id_bn', 'sr_elu_bn_64', 'cinpp_elu', 'ogb_tanh', 'norings_elu',
              'relu_ln_48', 'relu_ln_10', 'jk_max')
GIN_CASES = ('gin0_relu', 'gin_elu', 'gin0jk_cat_tanh', 'ginjk_max_sigmoid', 'gin0_id_64')
RING_CASES = ('ring_bn', 'ring_ln')
EGIN_CASES = ('egin_edge', 'egin_noedge', 'egin_dim12', 'egin_nodes_only', 'egin_lin1')
INDEX_KEYS = ('upper_index', 'lower_index', 'shared_boundaries', 'shared_coboundaries', 'boundary_index')


def cfg(fixture, case):
    return json.loads(str(load(fixture)[f'{case}/cfg']))


def state(fixture, case):
    return state_dict(load(fixture), f'{case}/state')


def partials(fixture, case):
    g, pre = load(fixture), f'{case}/p64/'
    return {k[len(pre):]: T(v) for k, v in g.items() if k.startswith(pre)}


def out64(fixture, case):
    return T(load(fixture)[f'{case}/out64'])


def out32(fixture, case):
    return T(load(fixture)[f'{case}/out32'])


def training(fixture, case):
    """-> (out, cotangent, {parameter: gradient}, {parameter: the reference's own float32 deviation}) of the float64 training run."""
    g, pre = load(fixture), f'train/{case}/'
    grads = {k[len(pre) + 5:]: T(v) for k, v in g.items() if k.startswith(pre + 'grad/')}
    own = {k[len(pre) + 11:]: float(v) for k, v in g.items() if k.startswith(pre + 'grad32_err/')}
    return T(g[pre + 'out']), T(g[pre + 'cotangent']), grads, own


def product_model(fixture, case, dtype=torch.float32):
    """The product's class of the case's name with the case's settings and the stored state, loaded strictly; eval mode."""
    from cwn_amd import models
    c = cfg(fixture, case)
    model = getattr(models, c['cls'])(*c['args'], **c['kw'])
    model.load_state_dict(state(fixture, case), strict=True)
    return model.to(dtype).eval()


def oracle_cx(fixture, kind, dtype=torch.float64):
    """The stored batch as the oracle's dict (floating features in `dtype`, integer features as they are)."""
    cx = complex_dict(load(fixture), f'inputs/{kind}')
    for c in cx['cochains']:
        if c['x'] is not None and c['x'].is_floating_point():
            c['x'] = c['x'].to(dtype)
    return cx


def oracle_kwargs(c):
    """cwn_oracle.sparse_cin_model_forward's arguments (after state and complex) for a case's settings."""
    kw, cls = c['kw'], c['cls']
    out = dict(num_layers=c['args'][{'SparseCIN': 2, 'OGBEmbedSparseCIN': 1}.get(cls, 3)],
               use_coboundaries=kw['use_coboundaries'], readout=kw['readout'], final_readout=kw['final_readout'],
               norm=kw['graph_norm'], jump_mode=kw.get('jump_mode'), act=kw['nonlinearity'],
               embed={'SparseCIN': None, 'OGBEmbedSparseCIN': 'ogb'}.get(cls, 'zinc'),
               init_reduce_mode={'sum': 'add'}.get(kw.get('init_reduce', 'sum'), kw.get('init_reduce')),
               conv='cinpp' if cls == 'EmbedCINpp' else 'sparse_cin')
    if cls == 'EmbedSparseCINNoRings':
        out.update(max_dim=1, readout_dims=(0, 1), drop_edge_up=True)
    return out


def _same_layout(batch, fixture, kind):
    g = load(fixture)
    for d in range(batch.dimension + 1):
        for k in INDEX_KEYS + ('batch',):
            key, have = f'inputs/{kind}/{d}/{k}', batch.cochains[d][k] if k != 'batch' else batch.cochains[d].batch
            assert (key in g) == (have is not None), key
            if have is not None:
                assert torch.equal(have.cpu(), T(g[key])), key


def sr_complexes(fixture=CELL):
    """The four SR(16,6,2,2) lifts of the case 'sr_elu_bn_64' in this project's containers (the generator's recipe: the rook's
    graph, a relabelled copy, the Shrikhande graph, a relabelled copy, rings up to 6) with the stored float32 features."""
    from cwn_amd import synthetic
    g = load(fixture)
    rng = np.random.default_rng(43)
    out = []
    for graph in (synthetic.rook_4x4(), synthetic.shrikhande()):
        out += [synthetic.sr_lift(*graph, max_k=6), synthetic.sr_lift(*synthetic.relabel(*graph, rng.permutation(16)), max_k=6)]
    offs = [0, 0, 0]
    for cx in out:
        for d in range(3):
            n = cx.cochains[d].num_cells
            cx.cochains[d].x = T(g[f'inputs/sr/{d}/x'])[offs[d]:offs[d] + n].clone()
            offs[d] += n
    assert offs == [g[f'inputs/sr/{d}/x'].shape[0] for d in range(3)]
    return out


def product_batch(fixture, kind, dtype=torch.float32):
    """The stored batch in this project's containers (CPU), its index layout checked against the stored one."""
    from cwn_amd.complex import ComplexBatch
    from tests._product import dummy_batch
    g = load(fixture)
    if kind == 'sr':
        b = ComplexBatch.from_complex_list(sr_complexes(fixture), max_dim=2)
        b.set_xs([b.cochains[d].x.to(dtype) for d in range(3)])
    else:
        b = dummy_batch([str(n) for n in g[f'inputs/{"mol" if kind in ("ogb", "mol_noedge") else kind}/names']], max_dim=2)
        for d in range(b.dimension + 1):
            key = f'inputs/{kind}/{d}/x'
            b.cochains[d]._x = T(g[key]).clone() if key in g else None
    _same_layout(b, fixture, kind)
    return b


def graph_data(case, dtype=torch.float32, device=None):
    """What a graph model of gin_family.npz is handed: x, edge_index, batch, mask."""
    g = load(GIN)
    w = cfg(GIN, case)['args'][0]
    mv = (lambda t: t) if device is None else (lambda t: t.to(device))
    return SimpleNamespace(x=mv(T(g[f'graph/x/{w}']).to(dtype)), edge_index=mv(T(g['graph/edge_index'])),
                           batch=mv(T(g['graph/batch'])), mask=mv(T(g['graph/mask'])))


def hook_layers(modules, seen):
    """Forward hooks recording every module's output tensor under 'layer{c}'; returns the handles."""
    def make(c):
        def hook(mod, inp, res):
            seen[f'layer{c}'] = res
        return hook
    return [m.register_forward_hook(make(c)) for c, m in enumerate(modules)]
