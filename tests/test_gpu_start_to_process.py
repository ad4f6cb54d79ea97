"""A conv layer called with start_to_process > 0 (mp/layers.py:333-342, :418-427): the dimensions below it hand their input
back untouched, the others are the layer evaluated in float64 on the CPU (the oracle over the layer's own state) -- through
the one `forward` that SparseCINConv and CINppConv share, in inference and (SparseCINConv) in training mode with BatchNorm.

Not asserted: bit equality with the start_to_process=0 call.  It does not hold (dimension 1 differs by one float32 ulp, 2.4e-7):
from 0 the propagate step is the blocked launch, from 1 the grouped GEMM + aggregation launches."""
import pytest
import torch

from tests._product import gate, to_double

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = 64


def _batch():
    """Three small ring-lifted molecules-like complexes: a few dozen cells per dimension."""
    from cwn_amd.complex import ComplexBatch
    from cwn_amd.synthetic import zinc_like_complexes
    b = ComplexBatch.from_complex_list(zinc_like_complexes(3, 5, 6), max_dim=2)
    g = torch.Generator().manual_seed(7)
    for d in range(3):
        b.cochains[d].x = torch.randn(b.cochains[d].num_cells, F, generator=g)
    assert all(b.cochains[d].num_cells >= 2 for d in range(3))
    return b


def _conv(cls, seed):
    from cwn_amd.layers import SparseCINConv
    torch.manual_seed(seed)
    args = (F, F, F) + (None,) * (4 if cls is SparseCINConv else 6)
    conv = cls(*args, max_dim=2, hidden=F, eps=0.25, act_module=torch.nn.ReLU, layer_dim=F, use_coboundaries=True)
    with torch.no_grad():                # BatchNorm with statistics and an affine of its own: a skipped norm would show
        for m in conv.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.normal_(0.0, 0.3)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0.0, 0.2)
    return conv


KEYS = ('x', 'upper_index', 'lower_index', 'shared_boundaries', 'shared_coboundaries', 'boundary_index', 'y', 'batch')


def _reference(conv, b, which, start, train):
    """The layer in float64 on the CPU: the oracle's forward over the layer's own state (taken before any forward: a
    training-mode one moves the running statistics)."""
    from oracle import cwn_oracle as O
    cochains = [{k: b.cochains[d][k] for k in KEYS} for d in range(3)]
    for c in cochains:
        c['x'] = c['x'].double()
    params = O.all_cochain_params({'dimension': 2, 'y': None, 'cochains': cochains}, 2, include_down_features=False)
    state = to_double({k: v.detach().clone() for k, v in conv.state_dict().items()})
    return O.sparse_cin_conv(state, params, True, training=train, start_to_process=start,
                             conv='cinpp' if which == 'cinpp' else 'sparse_cin')


@pytest.mark.parametrize('which,train', [('cin', False), ('cinpp', False), ('cin', True)])
def test_start_to_process_one(which, train):
    from cwn_amd.layers import CINppConv, SparseCINConv
    conv = _conv(SparseCINConv if which == 'cin' else CINppConv, seed=11).train(train)
    b = _batch()
    want = _reference(conv, b, which, 1, train)
    conv, b = conv.to(DEV), b.to(DEV)
    params = b.get_all_cochain_params(max_dim=2, include_down_features=False)
    with torch.set_grad_enabled(train):
        got = conv(*params, start_to_process=1)
    assert len(got) == len(want) == 3 and got[0] is params[0].x
    for d in (1, 2):
        assert got[d].dtype == torch.float32 and got[d].shape == (params[d].x.size(0), F)
        gate(got[d], want[d], f'{which} {"training" if train else "eval"} start_to_process=1 dim {d} vs float64 on the CPU')
