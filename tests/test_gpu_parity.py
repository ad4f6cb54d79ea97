"""Parity of the HIP path (through the C ABI) against the CPU oracle, the golden vectors produced
by the live reference and the hand-computed expectations of the reference's tests.

Tolerances: integer structures (CSR) bit-exact; fp32 features |delta| <= 1e-5 (north star), and
exact equality wherever the arithmetic is exact (integer-valued features) or the summation order
is provably the oracle's (add-reduce over the stable CSR order)."""
import copy

import numpy as np
import pytest
import torch

from oracle import cwn_oracle as O
from tests._golden import load, T, dummy_complex as o_complex, params_dict, state_dict
from tests._product import dummy_complex, dummy_batch, list_names, gate, to_double

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _grad_scale(name: str, ref) -> float:
    """Scale of the absolute tolerance for a parameter gradient compared between two float32 implementations.  Two kinds of
    gradient are pure rounding noise relative to their own value: the eps scalars (ONE number = a sum of ~1e5 O(1) products
    that cancel) and the bias of a Linear that feeds a BatchNorm(train) (the column sums of dz, zero in exact arithmetic:
    what is left is the summation noise of M rows, different for every summation order -- atomics, bands, torch)."""
    if name.endswith(('eps', 'eps1', 'eps2', 'eps3', 'eps4')):
        return 40.0
    s = max(1.0, float(ref.abs().max()))
    import re
    if re.search(r'(update_\w+_nn\.(0|3)|combine_nn\.0)\.bias$', name):
        return 10.0 * s
    return s
NAMES = ['house', 'bridged', 'fullstop', 'colon', 'square', 'square_dot', 'kite', 'pyramid',
         'filled_square', 'molecular']


@pytest.fixture(scope='module', autouse=True)
def _native_loaded():
    from cwn_amd import _ffi
    assert _ffi.lib().cwn_target_arch() == b'gfx950'
    assert torch.cuda.is_available()


def cpu(t):
    return None if t is None else t.detach().cpu()


def run_base(prm, **ctor):
    from cwn_amd.cell_mp import CochainMessagePassing
    w = prm.x.size(1)
    ctor = dict(dict(up_msg_size=w, down_msg_size=w), **ctor)
    cmp = CochainMessagePassing(**ctor)
    return cmp.propagate(prm.up_index, prm.down_index, prm.boundary_index, x=prm.x,
                         up_attr=prm.kwargs['up_attr'], down_attr=prm.kwargs['down_attr'],
                         boundary_attr=prm.kwargs['boundary_attr'])


# ------------------------------------------------------------------------------------------------
# CSR plans: integer, bit-exact
# ------------------------------------------------------------------------------------------------
def _check_adj(adj, index, n_dst, aux=None):
    rowptr, col, perm = O.csr_from_coo(index.cpu(), n_dst)
    assert torch.equal(cpu(adj.rowptr), rowptr)
    assert torch.equal(cpu(adj.col), col)
    assert torch.equal(cpu(adj.perm), perm)
    if aux is not None:
        assert torch.equal(cpu(adj.aux), aux.cpu()[perm.long()].int())
    # rows longer than CWN_LONG_ROW are listed (any order) for the whole-workgroup reduction
    from cwn_amd.csr import LONG_ROW
    deg = (rowptr[1:] - rowptr[:-1]).long()
    want = torch.nonzero(deg > LONG_ROW).flatten()
    assert torch.equal(cpu(adj.long_row_list()).sort().values, want)


def test_csr_build_on_every_batched_index():
    from cwn_amd.csr import Adjacency
    b = dummy_batch(list_names('testing'), max_dim=2, device=DEV)
    for d in range(3):
        c = b.cochains[d]
        n = c.num_cells
        for index, aux, n_src, n_aux in (
                (c.upper_index, c.shared_coboundaries, n, c.num_cells_up),
                (c.lower_index, c.shared_boundaries, n, c.num_cells_down),
                (c.boundary_index, None, c.num_cells_down, 0)):
            if index is None:
                continue
            adj = Adjacency.from_index(index, n, n_src, aux, n_aux or 0)
            _check_adj(adj, index, n, aux)
            # transposes used by backward
            _check_adj(adj.t_src, index.flip(0), n_src, aux)
            if aux is not None:
                _check_adj(adj.t_aux, torch.stack([index[1], aux]), n_aux, index[0])


@pytest.mark.parametrize('E,n_dst,n_src', [(0, 5, 5), (1, 1, 1), (1000, 7, 300), (50_000, 20_000, 9_000),
                                           (300_000, 100_000, 100_000)])
def test_csr_build_random(E, n_dst, n_src):
    from cwn_amd.csr import Adjacency
    g = torch.Generator().manual_seed(E + n_dst)
    index = torch.stack([torch.randint(0, n_src, (E,), generator=g),
                         torch.randint(0, n_dst, (E,), generator=g)])
    aux = torch.randint(0, 17, (E,), generator=g)
    adj = Adjacency.from_index(index.to(DEV), n_dst, n_src, aux.to(DEV), 17)
    _check_adj(adj, index, n_dst, aux)


def test_csr_build_hub_rows_and_batched_call():
    """Skewed segments (REDDIT-like hubs) and several descriptors in one call."""
    from cwn_amd.csr import Adjacency, build_many
    g = torch.Generator().manual_seed(3)
    n = 4000
    dst = torch.cat([torch.full((6000,), 17), torch.full((3000,), 3999), torch.randint(0, n, (20_000,), generator=g)])
    dst = dst[torch.randperm(dst.numel(), generator=g)]
    src = torch.randint(0, n, (dst.numel(),), generator=g)
    idx = torch.stack([src, dst])
    adjs = [Adjacency.from_index(idx.to(DEV), n, n, build=False)]
    others = []
    for k in range(19):   # > CWN_CSR_MAX_DESCS descriptors -> two C-ABI calls
        e = 100 * (k + 1)
        i2 = torch.stack([torch.randint(0, 50, (e,), generator=g), torch.randint(0, 60, (e,), generator=g)])
        others.append(i2)
        adjs.append(Adjacency.from_index(i2.to(DEV), 60, 50, build=False))
    build_many(adjs)
    _check_adj(adjs[0], idx, n)
    for a, i2 in zip(adjs[1:], others):
        _check_adj(a, i2, 60)


def test_csr_out_of_range_raises_index_error():
    from cwn_amd.csr import Adjacency
    bad = torch.tensor([[0, 1, 7], [1, 0, 2]], device=DEV)
    with pytest.raises(IndexError, match='source index'):
        Adjacency.from_index(bad, 3, 3)
    bad = torch.tensor([[0, 1, 2], [1, 0, 9]], device=DEV)
    with pytest.raises(IndexError, match='destination index'):
        Adjacency.from_index(bad, 3, 3)


# ------------------------------------------------------------------------------------------------
# K1 gather
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [1, 2, 3, 4, 8, 64, 127, 128, 130, 512])
def test_gather_rows_exact(F):
    from cwn_amd import ops
    g = torch.Generator().manual_seed(F)
    src = torch.randn(777, F, generator=g)
    idx = torch.randint(0, 777, (5001,), generator=g)
    out = ops.gather_rows(src.to(DEV), idx.to(DEV))
    assert torch.equal(cpu(out), O.lift(src, idx))


def test_gather_rows_unaligned_view_and_empty():
    from cwn_amd import ops
    src = torch.randn(50, 9, device=DEV)[:, 1:]          # non-contiguous view -> made contiguous
    idx = torch.tensor([3, 3, 49, 0], device=DEV)
    assert torch.equal(cpu(ops.gather_rows(src, idx)), cpu(src)[cpu(idx)])
    assert ops.gather_rows(torch.randn(5, 4, device=DEV), torch.empty(0, dtype=torch.long, device=DEV)).shape == (0, 4)


# ------------------------------------------------------------------------------------------------
# propagate: known answers of the reference's tests, on the GPU
# ------------------------------------------------------------------------------------------------
def test_house_known_answers_gpu():
    """mp/test_cell_mp.py:13-88."""
    h = dummy_complex('house', DEV)
    up, down, bnd = run_base(h.get_cochain_params(dim=1))
    assert cpu(up).flatten().tolist() == [0, 0, 11, 0, 9, 8]
    assert cpu(down).flatten().tolist() == [6, 10, 17, 9, 13, 10]
    assert cpu(bnd).flatten().tolist() == [3, 5, 7, 5, 9, 8]
    up, down, bnd = run_base(h.get_cochain_params(dim=0))
    assert cpu(up).flatten().tolist() == [6, 4, 11, 9, 7]
    assert torch.equal(cpu(down), torch.zeros(5, 1)) and torch.equal(cpu(bnd), torch.zeros(5, 1))
    up, down, bnd = run_base(h.get_cochain_params(dim=2))
    assert torch.equal(cpu(up), torch.zeros(1, 1)) and torch.equal(cpu(down), torch.zeros(1, 1))
    assert cpu(bnd).flatten().tolist() == [14]


def test_two_triangles_and_isolated_gpu():
    """mp/test_cell_mp.py:91-176."""
    from cwn_amd.cell_mp import CochainMessagePassing
    cmp = CochainMessagePassing(up_msg_size=1, down_msg_size=1)
    x = torch.tensor([[32.], [17.]], device=DEV)
    down_index = torch.tensor([[0, 1], [1, 0]], device=DEV)
    up, down, _ = cmp.propagate(None, down_index, None, x=x, down_attr=torch.tensor([[1], [1]], device=DEV))
    assert cpu(up + down).flatten().tolist() == [17, 32]
    sd = dummy_complex('square_dot', DEV).get_cochain_params(dim=0)
    up, down, _ = cmp.propagate(up_index=sd.up_index, down_index=None, boundary_index=None, x=sd.x, up_attr=None)
    assert cpu(up)[4].item() == 0 and all(cpu(up)[i].item() != 0 for i in range(4))
    assert torch.equal(cpu(down), torch.zeros(5, 1))
    for name in ('fullstop', 'colon'):
        p = dummy_complex(name, DEV).get_cochain_params(dim=0)
        up, _, _ = cmp.propagate(up_index=p.up_index, down_index=None, boundary_index=None, x=p.x, up_attr=None)
        assert torch.equal(cpu(up), torch.zeros_like(cpu(p.x)))
    empty = torch.empty(2, 0, dtype=torch.long, device=DEV)
    up, _, _ = cmp.propagate(up_index=empty, down_index=None, boundary_index=None, x=x, up_attr=None)
    assert torch.equal(cpu(up), torch.zeros(2, 1))


def test_bridged_multiplicity_gpu():
    """mp/test_cell_mp.py:179-247: shared (co)boundaries count with multiplicity."""
    b = dummy_complex('bridged', DEV)
    up, _, _ = run_base(b.get_cochain_params(dim=1))
    assert cpu(up).flatten().tolist() == [24, 22, 20, 18, 22, 20]
    _, down, bnd = run_base(b.get_cochain_params(dim=2))
    assert cpu(down).flatten().tolist() == [10, 8, 6] and cpu(bnd).flatten().tolist() == [16, 16, 10]


@pytest.mark.parametrize('name', NAMES)
def test_propagate_every_complex_exact(name):
    g = load('propagate_known_answer.npz')
    cx = dummy_complex(name, DEV)
    for d in range(cx.dimension + 1):
        up, down, bnd = run_base(cx.get_cochain_params(dim=d))
        assert torch.equal(cpu(up), T(g[f'{name}/{d}/up']))
        assert torch.equal(cpu(down), T(g[f'{name}/{d}/down']))
        assert torch.equal(cpu(bnd), T(g[f'{name}/{d}/boundary']))


@pytest.mark.parametrize('lazy', [True, False])
@pytest.mark.parametrize('name', NAMES)
def test_dummy_layer_exact(name, lazy):
    """mp/test_layers.py:11-69 and every other complex; fused x_j + attr with lazy and with
    materialised (reference-style) attributes."""
    from cwn_amd.layers import DummyCellularMessagePassing
    g = load('propagate_known_answer.npz')
    cx = dummy_complex(name, DEV)
    cx.lazy_attrs = lazy
    prms = [cx.get_cochain_params(dim=d) for d in range(min(cx.dimension, 2) + 1)]
    for ub in (0, 1):
        for ud in (0, 1):
            outs = DummyCellularMessagePassing(use_boundary_msg=bool(ub), use_down_msg=bool(ud)).forward(*prms)
            for d, o in enumerate(outs):
                assert torch.equal(cpu(o), T(g[f'{name}/dummy_b{ub}_d{ud}/{d}'])), (ub, ud, d)


@pytest.mark.parametrize('F', [1, 3, 8, 64, 128])
def test_propagate_random_golden_gpu(F):
    """Batched testing list, random features, all reductions; golden = the live reference."""
    g = load('propagate_random.npz')
    b = dummy_batch(list_names('testing'), max_dim=2, device=DEV)
    for d in range(3):
        b.cochains[d].x = T(g[f'F{F}/{d}/params/x']).to(DEV)
    prms = b.get_all_cochain_params(max_dim=2)
    for d, prm in enumerate(prms):
        for aggr in ('add', 'mean', 'max'):
            up, down, bnd = run_base(prm, aggr_up=aggr, aggr_down=aggr, aggr_boundary=aggr)
            for got, key in ((up, 'up'), (down, 'down'), (bnd, 'boundary')):
                ref = T(g[f'F{F}/{d}/{aggr}/{key}'])
                torch.testing.assert_close(cpu(got), ref, rtol=0, atol=1e-5)
                if aggr != 'mean':   # same summation order as the sequential CPU scatter
                    assert torch.equal(cpu(got), ref), (d, aggr, key)
        _, down, bnd = run_base(prm, up_msg_size=F, down_msg_size=5, boundary_msg_size=7,
                                use_down_msg=False, use_boundary_msg=False)
        assert list(down.shape) == g[f'F{F}/{d}/flags_off/down_shape'].tolist()
        assert list(bnd.shape) == g[f'F{F}/{d}/flags_off/boundary_shape'].tolist()
        assert not down.any() and not bnd.any()
    from cwn_amd.layers import DummyCellularMessagePassing
    outs = DummyCellularMessagePassing(input_dim=F, use_boundary_msg=True, use_down_msg=True).forward(*prms)
    for d, o in enumerate(outs):
        torch.testing.assert_close(cpu(o), T(g[f'F{F}/dummy/{d}']), rtol=0, atol=1e-5)


# ------------------------------------------------------------------------------------------------
# generic hook path + gradients
# ------------------------------------------------------------------------------------------------
def test_custom_hooks_match_oracle_and_autograd():
    from cwn_amd.cell_mp import CochainMessagePassing

    class Custom(CochainMessagePassing):
        def message_up(self, up_x_j, up_x_i, up_attr):
            return torch.tanh(up_x_j - up_x_i) * up_attr

        def message_boundary(self, boundary_x_j):
            return boundary_x_j ** 2

    g = load('propagate_random.npz')
    F = 8
    b = dummy_batch(list_names('testing'), max_dim=2, device=DEV)
    xs = [T(g[f'F{F}/{d}/params/x']) for d in range(3)]
    for d in range(3):
        b.cochains[d].x = xs[d].to(DEV).requires_grad_(True)
    prm = b.get_cochain_params(dim=1)
    layer = Custom(F, F)
    up, down, bnd = layer.propagate(prm.up_index, prm.down_index, prm.boundary_index, x=prm.x,
                                    up_attr=prm.kwargs['up_attr'], down_attr=prm.kwargs['down_attr'],
                                    boundary_attr=prm.kwargs['boundary_attr'])
    w = torch.randn(3, *up.shape, generator=torch.Generator().manual_seed(0))
    ((up * w[0].to(DEV)).sum() + (down * w[1].to(DEV)).sum() + (bnd * w[2].to(DEV)).sum()).backward()

    oxs = [x.clone().requires_grad_(True) for x in xs]
    ocx = O.batch_complexes([o_complex(n) for n in list_names('testing')], max_dim=2)
    for d in range(3):
        ocx['cochains'][d]['x'] = oxs[d]
    op = O.cochain_params(ocx, 1)
    idx = op['up_index']
    oup, odown, obnd = O.propagate(
        op['x'], op['up_index'], op['down_index'], op['boundary_index'], up_attr=op['up_attr'],
        down_attr=op['down_attr'], boundary_attr=op['boundary_attr'],
        message_up=lambda xj, a: torch.tanh(xj - op['x'].index_select(0, idx[1])) * a,
        message_boundary=lambda xj: xj ** 2, up_msg_size=F, down_msg_size=F)
    ((oup * w[0]).sum() + (odown * w[1]).sum() + (obnd * w[2]).sum()).backward()
    for got, ref in ((up, oup), (down, odown), (bnd, obnd)):
        torch.testing.assert_close(cpu(got), ref.detach(), rtol=1e-5, atol=1e-5)
    for d in range(3):
        torch.testing.assert_close(cpu(b.cochains[d].x.grad), oxs[d].grad, rtol=1e-5, atol=1e-5)


def test_identity_path_gradients_all_reductions():
    from cwn_amd.cell_mp import CochainMessagePassing
    g = load('propagate_random.npz')
    F = 8
    names = list_names('testing')
    for aggr in ('add', 'mean'):
        b = dummy_batch(names, max_dim=2, device=DEV)
        xs = [T(g[f'F{F}/{d}/params/x']) for d in range(3)]
        for d in range(3):
            b.cochains[d].x = xs[d].to(DEV).requires_grad_(True)
        prm = b.get_cochain_params(dim=1)
        layer = CochainMessagePassing(F, F, aggr_up=aggr, aggr_down=aggr, aggr_boundary=aggr)
        outs = layer.propagate(prm.up_index, prm.down_index, prm.boundary_index, x=prm.x,
                               up_attr=prm.kwargs['up_attr'], down_attr=prm.kwargs['down_attr'],
                               boundary_attr=prm.kwargs['boundary_attr'])
        w = torch.randn(3, *outs[0].shape, generator=torch.Generator().manual_seed(1))
        sum((o * w[k].to(DEV)).sum() for k, o in enumerate(outs)).backward()
        oxs = [x.clone().requires_grad_(True) for x in xs]
        ocx = O.batch_complexes([o_complex(n) for n in names], max_dim=2)
        for d in range(3):
            ocx['cochains'][d]['x'] = oxs[d]
        op = O.cochain_params(ocx, 1)
        oouts = O.propagate(op['x'], op['up_index'], op['down_index'], op['boundary_index'],
                            up_attr=op['up_attr'], down_attr=op['down_attr'],
                            boundary_attr=op['boundary_attr'], aggr_up=aggr, aggr_down=aggr,
                            aggr_boundary=aggr, up_msg_size=F, down_msg_size=F)
        sum((o * w[k]).sum() for k, o in enumerate(oouts)).backward()
        for d in (0, 1):
            torch.testing.assert_close(cpu(b.cochains[d].x.grad), oxs[d].grad, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------
# layers against the live-reference golden vectors (its state_dict loaded unchanged)
# ------------------------------------------------------------------------------------------------
def _sparse_cin(tag, g):
    from cwn_amd.layers import SparseCINConv
    from cwn_amd.models import get_graph_norm
    F, H, cob, bn = g[f'{tag}/meta'].tolist()
    conv = SparseCINConv(up_msg_size=F, down_msg_size=F, boundary_msg_size=F, passed_msg_up_nn=None,
                         passed_msg_boundaries_nn=None, passed_update_up_nn=None,
                         passed_update_boundaries_nn=None, train_eps=True, max_dim=2, hidden=H,
                         act_module=torch.nn.ReLU, layer_dim=F,
                         graph_norm=get_graph_norm('bn' if bn else 'id'), use_coboundaries=bool(cob))
    conv.load_state_dict(state_dict(g, f'{tag}/state'))
    return conv.to(DEV)


@pytest.mark.parametrize('tag', ['mol_cob_bn', 'mol_nocob_bn', 'test_cob_id', 'mol_cob_bn_64'])
def test_sparse_cin_conv_forward_golden(tag):
    g = load('sparse_cin_conv.npz')
    conv = _sparse_cin(tag, g)
    names = [str(n) for n in g[f'{tag}/names']]
    for mode in ('eval', 'train'):
        conv.load_state_dict(state_dict(g, f'{tag}/state'))   # train mode updates running stats
        conv.train(mode == 'train')
        b = dummy_batch(names, max_dim=2, device=DEV)
        for d in range(3):
            b.cochains[d].x = T(g[f'{tag}/x/{d}']).to(DEV)
        b.prepare()
        with torch.no_grad():
            outs = conv(*b.get_all_cochain_params(max_dim=2, include_down_features=False))
        for d, o in enumerate(outs):
            torch.testing.assert_close(cpu(o), T(g[f'{tag}/{mode}/{d}']), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('lazy', [True, False])
def test_sparse_cin_conv_unfused_paths_agree(lazy):
    """forward_unfused (propagate + fused hooks, reference's sequence) == batched forward; and the
    dense-attribute form (reference-style up_attr tensors) == the lazy form."""
    g = load('sparse_cin_conv.npz')
    tag = 'mol_cob_bn'
    conv = _sparse_cin(tag, g).eval()
    b = dummy_batch([str(n) for n in g[f'{tag}/names']], max_dim=2, device=DEV)
    b.lazy_attrs = lazy
    for d in range(3):
        b.cochains[d].x = T(g[f'{tag}/x/{d}']).to(DEV)
    prms = b.get_all_cochain_params(max_dim=2, include_down_features=False)
    with torch.no_grad():
        for d, prm in enumerate(prms):
            o = conv.mp_levels[d].forward_unfused(prm)
            torch.testing.assert_close(cpu(o), T(g[f'{tag}/eval/{d}']), rtol=1e-5, atol=1e-5)
            o = conv.mp_levels[d].forward(prm)
            torch.testing.assert_close(cpu(o), T(g[f'{tag}/eval/{d}']), rtol=1e-5, atol=1e-5)


def test_sparse_cin_conv_custom_message_net_generic_path():
    """An unrecognised message network (lambda, tanh) runs through gather -> hook -> reduce."""
    from cwn_amd.layers import SparseCINCochainConv
    g = load('sparse_cin_conv.npz')
    tag = 'mol_cob_bn'
    F = int(g[f'{tag}/meta'][0])
    b = dummy_batch([str(n) for n in g[f'{tag}/names']], max_dim=2, device=DEV)
    for d in range(3):
        b.cochains[d].x = T(g[f'{tag}/x/{d}']).to(DEV)
    lvl = SparseCINCochainConv(1, F, F, F, msg_up_nn=lambda xs: torch.tanh(xs[0] * xs[1]),
                               msg_boundaries_nn=lambda x: 2 * x, update_up_nn=torch.nn.Identity(),
                               update_boundaries_nn=torch.nn.Identity(),
                               combine_nn=torch.nn.Identity(), eps=0.5).to(DEV)
    prm = b.get_cochain_params(dim=1, include_down_features=False)
    out = lvl(prm)
    ocx = O.batch_complexes([o_complex(str(n)) for n in g[f'{tag}/names']], max_dim=2)
    for d in range(3):
        ocx['cochains'][d]['x'] = T(g[f'{tag}/x/{d}'])
    op = O.cochain_params(ocx, 1, include_down_features=False)
    up, _, bnd = O.propagate(op['x'], op['up_index'], None, op['boundary_index'], up_attr=op['up_attr'],
                             boundary_attr=op['boundary_attr'],
                             message_up=lambda xj, a: torch.tanh(xj * a),
                             message_boundary=lambda xj: 2 * xj, use_down_msg=False,
                             up_msg_size=F, down_msg_size=F, boundary_msg_size=F)
    ref = torch.cat([up + 1.5 * op['x'], bnd + 1.5 * op['x']], dim=-1)
    torch.testing.assert_close(cpu(out), ref, rtol=1e-5, atol=1e-5)


def test_sparse_cin_conv_backward_golden():
    """Gradients w.r.t. inputs and every parameter equal the reference's (train mode, BN)."""
    g = load('sparse_cin_conv.npz')
    tag = 'mol_cob_bn'
    conv = _sparse_cin(tag, g).train()
    b = dummy_batch([str(n) for n in g[f'{tag}/names']], max_dim=2, device=DEV)
    xs = [T(g[f'{tag}/x/{d}']).to(DEV).requires_grad_(True) for d in range(3)]
    for d in range(3):
        b.cochains[d].x = xs[d]
    b.prepare(backward=True)
    outs = conv(*b.get_all_cochain_params(max_dim=2, include_down_features=False))
    sum((o * T(g[f'{tag}/train_w/{d}']).to(DEV)).sum() for d, o in enumerate(outs)).backward()
    for d, o in enumerate(outs):
        torch.testing.assert_close(cpu(o), T(g[f'{tag}/train/{d}']), rtol=1e-5, atol=1e-5)
    for d in range(3):
        torch.testing.assert_close(cpu(xs[d].grad), T(g[f'{tag}/train_gx/{d}']), rtol=1e-4, atol=2e-5)
    pre = f'{tag}/train_grad/'
    params = dict(conv.named_parameters())
    n = 0
    for k, v in g.items():
        if k.startswith(pre):
            torch.testing.assert_close(cpu(params[k[len(pre):]].grad), T(v), rtol=1e-4, atol=5e-5)
            n += 1
    assert n > 20


def test_cin_conv_and_oriented_messages_golden():
    from cwn_amd.layers import CINConv, OrientedConv
    g = load('cin_conv.npz')
    F = 8
    msg_up = torch.nn.Sequential(torch.nn.Linear(2 * F, F), torch.nn.ReLU())
    msg_down = torch.nn.Sequential(torch.nn.Linear(2 * F, F), torch.nn.ReLU())
    upd = torch.nn.Sequential(torch.nn.Linear(F, 12), torch.nn.ReLU())
    conv = CINConv(F, F, msg_up, msg_down, upd, eps=0.1, train_eps=False, max_dim=2)
    conv.load_state_dict(state_dict(g, 'cin/state'))
    conv = conv.to(DEV)
    b = dummy_batch(list_names('testing'), max_dim=2, device=DEV)
    for d in range(3):
        b.cochains[d].x = T(g[f'cin/x/{d}']).to(DEV)
    prm = b.get_cochain_params(dim=1)
    with torch.no_grad():
        out = conv.mp_levels[1].forward(prm)
    torch.testing.assert_close(cpu(out), T(g['cin/out/1']), rtol=1e-5, atol=1e-5)
    oc = OrientedConv(1, F, F, update_up_nn=None, update_down_nn=None, update_nn=None, act_fn=None)
    up, down, _ = oc.propagate(prm.up_index, prm.down_index, None, x=prm.x,
                               up_attr=T(g['orient/up_orient']).to(DEV).view(-1, 1),
                               down_attr=T(g['orient/down_orient']).to(DEV).view(-1, 1))
    torch.testing.assert_close(cpu(up), T(g['orient/up']), rtol=0, atol=1e-6)
    torch.testing.assert_close(cpu(down), T(g['orient/down']), rtol=0, atol=1e-6)


@pytest.mark.parametrize('norm,lazy', [('bn', True), ('bn', False), ('none', True), ('bn_eval', True)])
def test_cin_conv_fused_training_matches_the_per_entry_path(norm, lazy):
    """CINCochainConv._fused_training (round 4; mp/layers.py:62-124 with the message networks of
    mp/models.py:40-47, Linear -> ReLU -> BatchNorm in TRAINING mode: statistics over the ENTRIES of each adjacency) against
    the generic path -- gather, the torch network per entry, segmented reduce -- on a ZINC-like batch with upper AND lower
    adjacencies: outputs, input gradients, every parameter gradient, the running statistics and batch counters.  `lazy`:
    the attributes as IndexedRows (gathered through the shared-cell index) or materialised per entry."""
    from cwn_amd import layers
    from cwn_amd.layers import CINConv
    from cwn_amd.synthetic import zinc_like_batch
    F = 64
    torch.manual_seed(7)

    def msg():
        mods = [torch.nn.Linear(2 * F, F), torch.nn.ReLU()]
        if norm != 'none':
            mods.append(torch.nn.BatchNorm1d(F))
        return torch.nn.Sequential(*mods)
    upd = torch.nn.Sequential(torch.nn.Linear(F, F), torch.nn.ReLU(), torch.nn.BatchNorm1d(F))
    conv = CINConv(F, F, msg(), msg(), upd, eps=0.1, train_eps=True, max_dim=2).to(DEV).train()
    if norm == 'bn_eval':
        for lvl in conv.mp_levels:
            for net in (lvl.msg_up_nn, lvl.msg_down_nn):
                net[2].eval()
                net[2].running_mean.uniform_(-0.2, 0.2)
                net[2].running_var.uniform_(0.5, 1.5)
    state0 = {k: v.clone() for k, v in conv.state_dict().items()}
    b = zinc_like_batch(12, seed=4, device=DEV)
    g = torch.Generator().manual_seed(2)
    xs0 = [torch.randn(b.cochains[d].num_cells, F, generator=g).to(DEV) for d in range(3)]
    ws = [torch.randn(b.cochains[d].num_cells, F, generator=g).to(DEV) for d in range(3)]
    taken = []
    orig = layers.CINCochainConv._fused_training
    layers.CINCochainConv._fused_training = lambda self, c: (lambda r: (taken.append(r is not None), r)[1])(orig(self, c))

    def run(fused):
        layers.FUSED_CIN_TRAINING = fused
        conv.load_state_dict(state0)
        conv.zero_grad(set_to_none=True)
        xin = [x.clone().requires_grad_() for x in xs0]
        b.set_xs(xin)
        params = b.get_all_cochain_params(max_dim=2, include_down_features=True)
        if not lazy:
            for prm in params:
                for key in ('up_attr', 'down_attr'):
                    a = prm.kwargs.get(key)
                    if a is not None and hasattr(a, 'tensor'):        # cell_mp.IndexedRows -> one row per entry
                        prm.kwargs[key] = a.tensor()
        out = conv(*params)
        sum((o * w).sum() for o, w in zip(out, ws)).backward()
        return ([o.detach().clone() for o in out], [x.grad.clone() for x in xin],
                {n: p.grad.clone() for n, p in conv.named_parameters() if p.grad is not None},
                {n: t.clone() for n, t in conv.named_buffers()})

    try:
        taken.clear()
        got = run(True)
        assert taken and all(taken), f'the fused training path was not taken: {taken}'
        want = run(False)
    finally:
        layers.FUSED_CIN_TRAINING = True
        layers.CINCochainConv._fused_training = orig
    for d, (a, r) in enumerate(zip(got[0], want[0])):
        torch.testing.assert_close(a, r, rtol=1e-4, atol=2e-5 * max(1.0, float(r.abs().max())), msg=lambda m, d=d: f'out[{d}]: {m}')
    for d, (a, r) in enumerate(zip(got[1], want[1])):
        torch.testing.assert_close(a, r, rtol=1e-4, atol=5e-5 * max(1.0, float(r.abs().max())), msg=lambda m, d=d: f'dx[{d}]: {m}')
    assert got[2].keys() == want[2].keys()
    for n_, r in want[2].items():
        sc = 40.0 if n_.endswith('eps') else max(1.0, float(r.abs().max()))
        torch.testing.assert_close(got[2][n_], r, rtol=1e-4, atol=5e-5 * sc, msg=lambda m, n_=n_: f'{n_}: {m}')
    for n_, t in want[3].items():
        if t.dtype.is_floating_point:
            torch.testing.assert_close(got[3][n_], t, rtol=1e-5, atol=1e-6, msg=lambda m, n_=n_: f'{n_}: {m}')
        else:
            assert torch.equal(got[3][n_], t), n_


def test_edge_cin_conv_and_full_oriented_conv_golden_gpu():
    """Round 3: `EdgeCINConv` with EdgeCIN0's networks and call (mp/layers.py:127-150,
    mp/models.py:311-341, 388-390) and a FULL `OrientedConv.forward` (mp/layers.py:441-452: propagate with the
    orientation messages, three update networks, activation) against the reference's own outputs."""
    from cwn_amd.complex import Cochain
    from cwn_amd.layers import EdgeCINConv, OrientedConv
    g = load('edge_oriented.npz')
    F, Hd = 8, 12

    def msg_net(k):
        return torch.nn.Sequential(torch.nn.Linear(k, F), torch.nn.ReLU(), torch.nn.BatchNorm1d(F))

    def upd_net():
        return torch.nn.Sequential(torch.nn.Linear(F, Hd), torch.nn.ReLU(), torch.nn.Linear(Hd, Hd), torch.nn.ReLU(),
                                   torch.nn.BatchNorm1d(Hd))
    conv = EdgeCINConv(F, F, msg_net(2 * F), msg_net(2 * F), msg_net(2 * F), upd_net(), upd_net(), eps=0.2, train_eps=False)
    conv.load_state_dict(state_dict(g, 'edge_cin/state'))
    conv = conv.to(DEV).eval()
    b = dummy_batch(list_names('testing'), max_dim=2, device=DEV)
    for d in range(3):
        b.cochains[d].x = T(g[f'edge_cin/x/{d}']).to(DEV)
    for grad in (False, True):                  # the fused inference form and the generic (autograd) path
        with torch.set_grad_enabled(grad):
            outs = conv(*b.get_all_cochain_params(max_dim=1, include_top_features=True))
        assert len(outs) == 2
        for d, o in enumerate(outs):
            gate(o, T(g[f'edge_cin/out/{d}']), f'EdgeCINConv out[{d}] (grad={grad})')
    oc = OrientedConv(1, F, F, update_up_nn=torch.nn.Linear(F, Hd), update_down_nn=torch.nn.Linear(F, Hd),
                      update_nn=torch.nn.Linear(F, Hd), act_fn=torch.tanh)
    oc.load_state_dict(state_dict(g, 'oriented/state'))
    oc = oc.to(DEV)
    c = Cochain(dim=1, x=T(g['oriented/x']), upper_index=T(g['oriented/upper_index']), lower_index=T(g['oriented/lower_index']),
                upper_orient=T(g['oriented/upper_orient']), lower_orient=T(g['oriented/lower_orient']))
    for k in ('x', 'upper_index', 'lower_index', 'upper_orient', 'lower_orient'):
        setattr(c, k, getattr(c, k).to(DEV))
    with torch.no_grad():
        y = oc(c)
    gate(y, T(g['oriented/out']), 'OrientedConv.forward')
    # both adjacencies in ONE aggregation launch / one autograd node (OrientedConv.propagate_both, round 4) against
    # propagate() -- a launch per adjacency: outputs, input and parameter gradients, with and without orientations
    x0, w = c.x.detach().clone(), torch.randn(c.x.size(0), Hd, generator=torch.Generator().manual_seed(2)).to(DEV)
    for orient in (True, False):
        oc.orient = orient
        res = []
        for one_launch in (True, False):
            oc.zero_grad(set_to_none=True)
            c.x = x0.clone().requires_grad_(True)
            if not one_launch:
                oc.propagate_both = lambda cochain: None
            try:
                y = oc(c)
            finally:
                oc.__dict__.pop('propagate_both', None)
            (y * w).sum().backward()
            res.append((y.detach(), c.x.grad.clone(), {n: p.grad.clone() for n, p in oc.named_parameters()}))
        assert oc.propagate_both(c) is not None
        torch.testing.assert_close(res[0][0], res[1][0], rtol=1e-6, atol=1e-6)
        torch.testing.assert_close(res[0][1], res[1][1], rtol=1e-5, atol=1e-5)
        for n in res[1][2]:
            torch.testing.assert_close(res[0][2][n], res[1][2][n], rtol=1e-5, atol=1e-5, msg=n)
    oc.orient = True


def test_init_reduce_known_answer_gpu():
    """mp/test_layers.py:135-149."""
    from cwn_amd.layers import InitReduceConv
    h = dummy_complex('house', DEV)
    p = [h.get_cochain_params(dim=d) for d in range(3)]
    conv = InitReduceConv(reduce='add')
    assert cpu(conv(p[0].x, p[1].boundary_index)).flatten().tolist() == [3, 5, 7, 5, 9, 8]
    assert cpu(conv(p[1].x, p[2].boundary_index)).flatten().tolist() == [14]


@pytest.mark.parametrize('tag', ['h16_l2', 'h32_l4'])
def test_embed_sparse_cin_whole_stack_golden(tag):
    """The reference model's state_dict on the engine: every layer output and the prediction."""
    from cwn_amd.models import EmbedSparseCIN
    g = load('embed_sparse_cin.npz')
    H, L = g[f'{tag}/meta'].tolist()
    model = EmbedSparseCIN(28, 4, 1, L, H, dropout_rate=0.0, max_dim=2, jump_mode=None,
                           nonlinearity='relu', readout='sum', train_eps=False,
                           final_hidden_multiplier=2, final_readout='sum', apply_dropout_before='lin2',
                           init_reduce='sum', embed_edge=True, use_coboundaries=True, graph_norm='bn')
    names = list_names('mol')
    for mode in ('eval', 'train'):
        model.load_state_dict(state_dict(g, f'{tag}/state'))
        model = model.to(DEV).train(mode == 'train')
        b = dummy_batch(names, max_dim=2)
        b.cochains[0].x = T(g[f'{tag}/v_types'])
        b.cochains[1].x = T(g[f'{tag}/e_types'])
        b.cochains[2]._x = None
        b = b.to(DEV)
        with torch.no_grad():
            y, res = model(b, include_partial=True)
        for k, v in res.items():
            gate(v, T(g[f'{tag}/{mode}/{k}']), f'{tag} {mode} {k}')
        gate(y, T(g[f'{tag}/{mode}/out']), f'{tag} {mode} out')


@pytest.mark.parametrize('tag', ['h16_l2', 'h64_l2'])
def test_embed_cinpp_whole_stack_golden(tag):
    """EmbedCINpp (mp/molec_models.py:167-199: EmbedSparseCIN with CINppConv layers, mp/layers.py:216-260, 344-427) with the
    REFERENCE's state_dict against the reference's own outputs (oracle/gen_golden.py cinpp): every layer output and the
    prediction, eval and training mode -- and in training mode once more with autograd recording, where at hidden 64 the
    update networks of all three streams run on the stage kernels (dense_train, a plan without combine stages)."""
    from cwn_amd.models import EmbedCINpp
    g = load('embed_cinpp.npz')
    H, L = g[f'{tag}/meta'].tolist()
    model = EmbedCINpp(28, 4, 1, L, H, dropout_rate=0.0, max_dim=2, jump_mode=None, nonlinearity='relu', readout='sum',
                       train_eps=True, final_hidden_multiplier=2, final_readout='sum', apply_dropout_before='lin2',
                       init_reduce='sum', embed_edge=True, use_coboundaries=True, graph_norm='bn')
    names = list_names('mol')
    for mode, grad in (('eval', False), ('train', False), ('train', True)):
        model.load_state_dict(state_dict(g, f'{tag}/state'))
        model = model.to(DEV).train(mode == 'train')
        b = dummy_batch(names, max_dim=2)
        b.cochains[0].x = T(g[f'{tag}/v_types'])
        b.cochains[1].x = T(g[f'{tag}/e_types'])
        b.cochains[2]._x = None
        b = b.to(DEV)
        taken = []
        if grad:
            from cwn_amd import dense_train as DT
            orig = DT.dense_train
            def record(plan, outs):
                res = orig(plan, outs)                      # (a refused plan raises: not recorded)
                taken.append((plan.nb, plan.cb is not None))
                return res
            DT.dense_train = record
        try:
            with torch.set_grad_enabled(grad):
                y, res = model(b, include_partial=True)
        finally:
            if grad:
                DT.dense_train = orig
        if grad:
            # per layer: dimensions 0 - 1 and dimension 2, three chains each; at 64 the combine stage rides in the same node
            # (cwn_dense_stage_ex_f32), at 16 it stays a torch module
            assert taken == [(3, H == 64)] * (2 * L), taken
        for k, v in res.items():
            gate(v, T(g[f'{tag}/{mode}/{k}']), f'{tag} {mode} grad={grad} {k}')
        gate(y, T(g[f'{tag}/{mode}/out']), f'{tag} {mode} grad={grad} out')


def test_plain_cinpp_golden():
    """CINpp (mp/models.py:259-284: the SparseCIN stack over CINppConv layers, features as given, messages = the first
    operand, JK cat) with the reference's state_dict against the reference's outputs, eval and training mode (with and without
    autograd recording)."""
    from cwn_amd.models import CINpp
    g = load('embed_cinpp.npz')
    model = CINpp(1, 2, 2, 16, dropout_rate=0.0, max_dim=2, jump_mode='cat', nonlinearity='relu', readout='sum', train_eps=True,
                  use_coboundaries=False, graph_norm='bn', final_readout='sum')
    for mode, grad in (('eval', False), ('train', False), ('train', True)):
        model.load_state_dict(state_dict(g, 'plain/state'))
        model = model.to(DEV).train(mode == 'train')
        b = dummy_batch(list_names('testing'), max_dim=2)
        for d in range(3):
            b.cochains[d].x = T(g[f'plain/x/{d}'])
        with torch.set_grad_enabled(grad):
            y, res = model(b.to(DEV), include_partial=True)
        for k, v in res.items():
            gate(v, T(g[f'plain/{mode}/{k}']), f'CINpp {mode} grad={grad} {k}')
        gate(y, T(g[f'plain/{mode}/out']), f'CINpp {mode} grad={grad} out')


@pytest.mark.parametrize('tag', ['cin0', 'edge', 'edge_notop'])
def test_cin0_and_edge_cin0_golden(tag):
    """CIN0 / EdgeCIN0 (mp/models.py:12-109, 286-420: the dense-CIN stacks over CINConv / EdgeCINConv) with the REFERENCE's
    state_dict against the reference's own predictions (oracle/gen_golden.py cin0): eval, training mode (BatchNorm over the
    adjacency entries), and training mode with autograd recording -- the fused per-entry training form of the layers."""
    from cwn_amd.models import CIN0, EdgeCIN0
    g = load('cin0_models.npz')
    F = 8
    if tag == 'cin0':
        model = CIN0(F, 3, 2, 12, dropout_rate=0.0, max_dim=2, jump_mode='cat', nonlinearity='relu', readout='sum')
    elif tag == 'edge':
        model = EdgeCIN0(F, 3, 3, 12, dropout_rate=0.0, jump_mode=None, nonlinearity='relu', include_top_features=True,
                         update_top_features=True, readout='mean')
    else:
        model = EdgeCIN0(F, 3, 2, 12, dropout_rate=0.0, jump_mode=None, nonlinearity='relu', include_top_features=False,
                         readout='sum')
    for mode, grad in (('eval', False), ('train', False), ('train', True)):
        model.load_state_dict(state_dict(g, f'{tag}/state'))
        model = model.to(DEV).train(mode == 'train')
        b = dummy_batch(list_names('testing'), max_dim=2)
        for d in range(3):
            b.cochains[d].x = T(g[f'{tag}/x/{d}'])
        with torch.set_grad_enabled(grad):
            y = model(b.to(DEV))
        gate(y, T(g[f'{tag}/{mode}/out']), f'{tag} {mode} grad={grad}')


def test_dummy_and_edge_orient_models_golden():
    """Dummy (mp/models.py:422-473) and EdgeOrient (:476-546: OrientedConv layers on a CochainBatch of edges with random
    orientations; the equivariant form with |.| behind the layers and the fully invariant form with |.| in front) with the
    reference's state_dict against the reference's outputs -- predictions and the per-edge values."""
    from cwn_amd.complex import Cochain, CochainBatch
    from cwn_amd.models import Dummy, EdgeOrient
    g = load('cin0_models.npz')
    model = Dummy(1, 3, 2, max_dim=2, readout='sum')
    model.load_state_dict(state_dict(g, 'dummy/state'))
    b = dummy_batch(list_names('testing'), max_dim=2)
    for d in range(3):
        b.cochains[d].x = T(g[f'dummy/x/{d}'])
    with torch.no_grad():
        gate(model.to(DEV)(b.to(DEV)), T(g['dummy/out']), 'Dummy')
    keys = ('x', 'upper_index', 'lower_index', 'upper_orient', 'lower_orient')
    for tag, invar, act in (('orient', False, 'id'), ('orient_invar', True, 'relu')):
        model = EdgeOrient(8, 2, 2, 12, dropout_rate=0.0, nonlinearity=act, readout='sum', fully_invar=invar)
        model.load_state_dict(state_dict(g, f'{tag}/state'))
        model = model.to(DEV).eval()
        edges = [Cochain(dim=1, **{k: T(g[f'orient/edges/{i}/{k}']) for k in keys}) for i in range(int(g['orient/n']))]
        data = CochainBatch.from_cochain_list(edges)
        for k in keys + ('batch',):
            setattr(data, k, getattr(data, k).to(DEV))
        for grad in (False, True):
            data.x = torch.cat([e.x for e in edges]).to(DEV)
            with torch.set_grad_enabled(grad):
                y, cells = model(data, include_partial=True)
            gate(cells, T(g[f'{tag}/cells']), f'EdgeOrient[{tag}] per-edge values (grad={grad})')
            gate(y, T(g[f'{tag}/out']), f'EdgeOrient[{tag}] prediction (grad={grad})')


def test_embed_sparse_cin_no_rings_golden():
    """EmbedSparseCINNoRings (mp/molec_models.py:386-503) with the reference's state_dict against the reference's predictions:
    eval, training mode, training mode with autograd recording."""
    from cwn_amd.models import EmbedSparseCINNoRings
    g = load('no_rings.npz')
    model = EmbedSparseCINNoRings(28, 4, 1, 2, 16, dropout_rate=0.0, nonlinearity='relu', readout='sum', train_eps=False,
                                  final_hidden_multiplier=2, final_readout='sum', init_reduce='sum', embed_edge=True,
                                  use_coboundaries=True, graph_norm='bn')
    for mode, grad in (('eval', False), ('train', False), ('train', True)):
        model.load_state_dict(state_dict(g, 'state'))
        model = model.to(DEV).train(mode == 'train')
        b = dummy_batch(list_names('mol'), max_dim=2)
        b.cochains[0].x, b.cochains[1].x = T(g['v_types']), T(g['e_types'])
        b.cochains[2]._x = None
        with torch.set_grad_enabled(grad):
            y = model(b.to(DEV))
        gate(y, T(g[f'{mode}/out']), f'EmbedSparseCINNoRings {mode} grad={grad}')


def test_ogb_embed_cinpp_golden():
    """OGBEmbedCINpp (mp/molec_models.py:355-384) with the reference's state_dict against the reference's outputs."""
    from cwn_amd.models import OGBEmbedCINpp
    g = load('embed_cinpp.npz')
    model = OGBEmbedCINpp(1, 2, 16, dropout_rate=0.0, indropout_rate=0.0, max_dim=2, jump_mode=None, nonlinearity='relu',
                          readout='mean', final_readout='sum', init_reduce='sum', embed_edge=True, use_coboundaries=True,
                          graph_norm='bn')
    model.load_state_dict(state_dict(g, 'ogb/state'))
    model = model.to(DEV).eval()
    b = dummy_batch(list_names('mol'), max_dim=2)
    b.cochains[0].x, b.cochains[1].x = T(g['ogb/v_feats']), T(g['ogb/e_feats'])
    b.cochains[2]._x = None
    with torch.no_grad():
        y, res = model(b.to(DEV), include_partial=True)
    for k, v in res.items():
        gate(v, T(g[f'ogb/{k}']), f'OGBEmbedCINpp {k}')
    gate(y, T(g['ogb/out']), 'OGBEmbedCINpp out')


# ------------------------------------------------------------------------------------------------
# BASELINE-size properties (ZINC-like batch of 128, F = 128): size-independent checks
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def zinc128():
    from cwn_amd.synthetic import zinc_like_batch
    b = zinc_like_batch(128, seed=0, max_ring=6, device=DEV)
    g = torch.Generator().manual_seed(0)
    for d in range(3):
        b.cochains[d].x = torch.randn(b.cochains[d].num_cells, 128, generator=g).to(DEV)
    return b.prepare(backward=True)


def test_full_size_matches_oracle(zinc128):
    """At this size the oracle still runs in well under a second: direct comparison."""
    b = zinc128
    for d in range(3):
        prm = b.get_cochain_params(dim=d, include_down_features=False)
        up, down, bnd = run_base(prm)
        oup, odown, obnd = O.propagate(
            cpu(prm.x), cpu(prm.up_index), None, cpu(prm.boundary_index),
            boundary_attr=cpu(prm.kwargs['boundary_attr']), up_msg_size=128, down_msg_size=128)
        assert torch.equal(cpu(up), oup) and torch.equal(cpu(bnd), obnd) and not down.any()


def test_full_size_linearity_and_checksum(zinc128):
    from cwn_amd import ops
    from cwn_amd.csr import cached_adjacency
    b = zinc128
    c = b.cochains[1]
    adj = cached_adjacency(c.upper_index, c.num_cells, c.num_cells, c.shared_coboundaries, c.num_cells_up)
    x, y = c.x, torch.randn_like(c.x)
    lhs = ops.aggregate(adj, c.num_cells, 2.0 * x - 3.0 * y)
    rhs = 2.0 * ops.aggregate(adj, c.num_cells, x) - 3.0 * ops.aggregate(adj, c.num_cells, y)
    torch.testing.assert_close(lhs, rhs, rtol=1e-5, atol=1e-4)
    # checksum of checksums: column sums of the output == out-degree-weighted column sums of x
    outdeg = torch.bincount(c.upper_index[0], minlength=c.num_cells).double()
    want = (outdeg.unsqueeze(1) * x.double()).sum(0)
    got = ops.aggregate(adj, c.num_cells, x).double().sum(0)
    torch.testing.assert_close(got, want, rtol=1e-6, atol=1e-3)
    # entry-order independence: shuffling the COO entries changes nothing for integer features
    perm = torch.randperm(c.upper_index.size(1), device=DEV)
    xi = torch.randint(-8, 8, x.shape, device=DEV).float()
    adj2 = cached_adjacency(c.upper_index[:, perm].contiguous(), c.num_cells, c.num_cells)
    assert torch.equal(ops.aggregate(adj, c.num_cells, xi), ops.aggregate(adj2, c.num_cells, xi))


def test_full_size_transpose_identity(zinc128):
    """<agg(x), w> == <x, agg^T(w)>: the backward kernel is the adjoint of the forward one."""
    from cwn_amd import ops
    from cwn_amd.csr import cached_adjacency
    b = zinc128
    c = b.cochains[2]
    adj = cached_adjacency(c.boundary_index, c.num_cells, c.num_cells_down)
    x = b.cochains[1].x.clone().requires_grad_(True)
    w = torch.randn(c.num_cells, 128, device=DEV)
    out = ops.aggregate(adj, c.num_cells, x)
    (out * w).sum().backward()
    ref = torch.zeros_like(x).index_add_(0, c.boundary_index[0], w[c.boundary_index[1]])
    torch.testing.assert_close(x.grad, ref, rtol=1e-5, atol=1e-5)


def test_sparse_cin_layer_full_size_vs_oracle(zinc128):
    """One SparseCIN layer (coboundary messages, BN train mode) at the BASELINE size."""
    from cwn_amd.layers import SparseCINConv
    b = zinc128
    torch.manual_seed(0)
    conv = SparseCINConv(128, 128, 128, None, None, None, None, max_dim=2, hidden=128,
                         act_module=torch.nn.ReLU, layer_dim=128, use_coboundaries=True).to(DEV).train()
    state = {k: v.detach().cpu() for k, v in conv.state_dict().items()}
    with torch.no_grad():
        outs = conv(*b.get_all_cochain_params(max_dim=2, include_down_features=False))
    ocx = {'dimension': 2, 'y': None, 'cochains': []}
    for d in range(3):
        c = b.cochains[d]
        ocx['cochains'].append({k: cpu(c[k]) for k in ('x', 'upper_index', 'lower_index',
                                'shared_boundaries', 'shared_coboundaries', 'boundary_index', 'y', 'batch')})
    for c in ocx['cochains']:
        c['x'] = c['x'].double()
    oouts = O.sparse_cin_conv(to_double(state), O.all_cochain_params(ocx, 2, include_down_features=False), True,
                              training=True)
    for d, (o, r) in enumerate(zip(outs, oouts)):
        gate(o, r, f'ZINC-128 SparseCIN layer (BN train mode) dim {d} vs float64 oracle')


# ------------------------------------------------------------------------------------------------
# grouped fp32-MFMA GEMM (dense parts) against torch matmul in float64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,N,K', [(1, 1, 1), (33, 128, 128), (3341, 128, 128), (100, 64, 64), (77, 130, 24),
                                   (50, 16, 10), (5, 256, 128), (0, 128, 128), (1000, 128, 256),
                                   # narrow layers: the 64 x 64 tile shapes (K <= 64 / 128 / 256)
                                   (1000, 64, 128), (257, 64, 200), (5000, 40, 64), (63, 3, 7), (4097, 64, 64)])
def test_gemm_matches_float64(M, N, K):
    from cwn_amd import ops
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    X = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    ref = (X.double() @ W.double().t() + b.double())
    Y, Yr = ops.run_gemm([ops.Gemm(X=X.to(DEV), W=W.to(DEV), bias=b.to(DEV)),
                          ops.Gemm(X=X.to(DEV), W=W.to(DEV), bias=b.to(DEV), relu=True)], DEV)
    torch.testing.assert_close(cpu(Y).double(), ref, rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(cpu(Yr).double(), ref.clamp(min=0), rtol=1e-5, atol=2e-5)


def test_gemm_grouped_concat_affine_stats():
    """Several GEMMs in one launch; weight column slices (ldw > K); K-concatenation; input affine +
    ReLU prologue; output affine epilogue; BatchNorm column statistics."""
    from cwn_amd import ops
    g = torch.Generator().manual_seed(5)
    F = 128
    Wfull = (torch.randn(F, 2 * F, generator=g) / 16).to(DEV)
    bias = torch.randn(F, generator=g).to(DEV)
    X0, X1 = torch.randn(3165, F, generator=g).to(DEV), torch.randn(304, F, generator=g).to(DEV)
    Xa, Xb = torch.randn(500, F, generator=g).to(DEV), torch.randn(500, F, generator=g).to(DEV)
    isc, ish = torch.rand(F, generator=g).to(DEV) + 0.5, torch.randn(F, generator=g).to(DEV)
    osc, osh = torch.rand(F, generator=g).to(DEV) + 0.5, torch.randn(F, generator=g).to(DEV)
    stats = torch.empty(2, ops.stat_rows(500), F, device=DEV, dtype=torch.float64)
    outs = ops.run_gemm([
        ops.Gemm(X=X0, W=Wfull[:, :F], bias=bias),
        ops.Gemm(X=X1, W=Wfull[:, F:]),
        ops.Gemm(X=Xa, X2=Xb, W=Wfull, bias=bias, relu=True, out_scale=osc, out_shift=osh),
        ops.Gemm(X=Xa, W=Wfull[:, :F], bias=bias, in_scale=isc, in_shift=ish, in_relu=True,
                 col_stats=stats),
    ], DEV)
    d = lambda t: t.double()
    refs = [d(X0) @ d(Wfull[:, :F]).t() + d(bias), d(X1) @ d(Wfull[:, F:]).t(),
            ((d(torch.cat([Xa, Xb], 1)) @ d(Wfull).t() + d(bias)) * d(osc) + d(osh)).clamp(min=0),
            (d(Xa) * d(isc) + d(ish)).clamp(min=0) @ d(Wfull[:, :F]).t() + d(bias)]
    for o, r in zip(outs, refs):
        torch.testing.assert_close(d(o), r, rtol=1e-5, atol=3e-5)
    torch.testing.assert_close(d(stats[0].sum(0)), refs[3].sum(0), rtol=1e-6, atol=1e-3)
    torch.testing.assert_close(d(stats[1].sum(0)), (refs[3] ** 2).sum(0), rtol=1e-6, atol=1e-3)


def test_gemm_transpose_detecting_identity():
    """A = I with an asymmetric B: a swapped output layout cannot pass."""
    from cwn_amd import ops
    W = torch.arange(48 * 32, dtype=torch.float32).view(48, 32).to(DEV)     # N=48, K=32
    X = torch.eye(32, device=DEV)
    Y, = ops.run_gemm([ops.Gemm(X=X, W=W)], DEV)
    assert torch.equal(Y, W.t())


def test_gemm_autograd_matches_linear():
    from cwn_amd import ops
    g = torch.Generator().manual_seed(9)
    lin = torch.nn.Linear(256, 128).to(DEV)
    Xa = torch.randn(700, 128, generator=g).to(DEV).requires_grad_(True)
    Xb = torch.randn(300, 128, generator=g).to(DEV).requires_grad_(True)
    y1, y2 = ops.gemm_many([ops.Gemm(X=Xa, W=lin.weight[:, :128], bias=lin.bias, relu=True),
                            ops.Gemm(X=Xb, W=lin.weight[:, 128:])])
    w1, w2 = torch.randn_like(y1), torch.randn_like(y2)
    ((y1 * w1).sum() + (y2 * w2).sum()).backward()
    got = [Xa.grad.clone(), Xb.grad.clone(), lin.weight.grad.clone(), lin.bias.grad.clone()]
    for t in (Xa, Xb, lin.weight, lin.bias):
        t.grad = None
    r1 = torch.relu(torch.nn.functional.linear(Xa, lin.weight[:, :128], lin.bias))
    r2 = torch.nn.functional.linear(Xb, lin.weight[:, 128:])
    ((r1 * w1).sum() + (r2 * w2).sum()).backward()
    for a, b in zip(got, [Xa.grad, Xb.grad, lin.weight.grad, lin.bias.grad]):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4)


def test_csr_small_path_with_hub_row():
    """Single-launch LDS path (fits 150 KiB) with one row holding half of the entries."""
    from cwn_amd.csr import Adjacency
    g = torch.Generator().manual_seed(11)
    n = 100
    dst = torch.cat([torch.full((3000,), 42), torch.randint(0, n, (3000,), generator=g)])
    dst = dst[torch.randperm(dst.numel(), generator=g)]
    src = torch.randint(0, 77, (dst.numel(),), generator=g)
    aux = torch.randint(0, 9, (dst.numel(),), generator=g)
    idx = torch.stack([src, dst])
    adj = Adjacency.from_index(idx.to(DEV), n, 77, aux.to(DEV), 9)
    _check_adj(adj, idx, n, aux)
    _check_adj(adj.t_src, idx.flip(0), 77, aux)


def test_overlapped_plan_build_and_deferred_index_check():
    """Plans built on the side stream give the same results; index errors surface in check_errors."""
    from cwn_amd import csr
    g = load('sparse_cin_conv.npz')
    tag = 'mol_cob_bn'
    conv = _sparse_cin(tag, g).eval()
    b = dummy_batch([str(n) for n in g[f'{tag}/names']], max_dim=2, device=DEV)
    for d in range(3):
        b.cochains[d].x = T(g[f'{tag}/x/{d}']).to(DEV)
    csr._cache.clear()
    b.prepare(overlap=True)
    with torch.no_grad():
        outs = conv(*b.get_all_cochain_params(max_dim=2, include_down_features=False))
    for d, o in enumerate(outs):
        torch.testing.assert_close(cpu(o), T(g[f'{tag}/eval/{d}']), rtol=1e-5, atol=1e-5)
    csr.check_errors(DEV)
    bad = torch.tensor([[0, 1, 7], [1, 0, 2]], device=DEV)
    adj = csr.Adjacency.from_index(bad, 3, 3, build=False)
    csr.build_many([adj], overlap=True)
    with pytest.raises(IndexError, match='source index'):
        csr.check_errors(DEV)


def test_fused_dense_eval_path_is_taken_and_matches_modules():
    """Eval + no_grad: update / combine MLPs run as grouped MFMA GEMMs with folded BatchNorm; the
    result equals the torch-module path (grad enabled) and the golden vectors."""
    g = load('sparse_cin_conv.npz')
    for tag in ('mol_cob_bn_64', 'test_cob_id'):
        conv = _sparse_cin(tag, g).eval()
        b = dummy_batch([str(n) for n in g[f'{tag}/names']], max_dim=2, device=DEV)
        for d in range(3):
            b.cochains[d].x = T(g[f'{tag}/x/{d}']).to(DEV)
        prms = b.get_all_cochain_params(max_dim=2, include_down_features=False)
        with torch.no_grad():
            plans, outs = conv.propagate_all(*prms)
            assert conv._dense_eval(plans, outs, 0) is not None
            fused = conv(*prms)
        modules = conv(*prms)            # grad enabled -> torch modules
        for d in range(3):
            torch.testing.assert_close(fused[d], modules[d].detach(), rtol=1e-5, atol=1e-5)
            torch.testing.assert_close(cpu(fused[d]), T(g[f'{tag}/eval/{d}']), rtol=1e-5, atol=1e-5)
        conv.train()
        with torch.no_grad():
            plans, outs = conv.propagate_all(*prms)
            took = conv._dense_eval(plans, outs, 0)
        assert (took is None) == (tag == 'mol_cob_bn_64')    # BN in training mode is not folded


# ------------------------------------------------------------------------------------------------
# BASELINE configs 3 (molhiv-like) and 5 (REDDIT-like clique complexes)
# ------------------------------------------------------------------------------------------------
def _oracle_cx(b):
    return {'dimension': b.dimension, 'y': None, 'num_complexes': b.num_complexes, 'cochains': [
        {k: cpu(b.cochains[d][k]) for k in ('x', 'upper_index', 'lower_index', 'shared_boundaries',
                                            'shared_coboundaries', 'boundary_index', 'y', 'batch')}
        for d in range(b.dimension + 1)]}


def test_extra_models_golden_gpu():
    """SparseCIN (F = 1 inputs, JK cat, no norm) and OGBEmbedSparseCIN (mean readout) with the
    reference's state_dicts, against the reference's outputs."""
    from cwn_amd.models import SparseCIN, OGBEmbedSparseCIN
    g = load('sparse_cin_models.npz')
    model = SparseCIN(1, 2, 3, 16, dropout_rate=0.0, max_dim=2, jump_mode='cat', readout='sum',
                      use_coboundaries=False, graph_norm='id')
    model.load_state_dict(state_dict(g, 'reddit/state'))
    model = model.to(DEV).eval()
    b = dummy_batch(list_names('testing'), max_dim=2, device=DEV)
    for d in range(3):
        b.cochains[d].x = T(g[f'reddit/x/{d}']).to(DEV)
    for grad in (False, True):       # fused dense path (no_grad) and module path
        b2 = dummy_batch(list_names('testing'), max_dim=2, device=DEV)
        for d in range(3):
            b2.cochains[d].x = T(g[f'reddit/x/{d}']).to(DEV)
        with torch.set_grad_enabled(grad):
            y, res = model(b2, include_partial=True)
        for k, v in res.items():
            gate(v, T(g[f'reddit/{k}']), f'SparseCIN fixture {k} (grad={grad})')
    model = OGBEmbedSparseCIN(1, 2, 16, dropout_rate=0.0, max_dim=2, readout='mean', init_reduce='sum',
                              embed_edge=True, use_coboundaries=True, graph_norm='bn')
    model.load_state_dict(state_dict(g, 'molhiv/state'))
    model = model.to(DEV).eval()
    b = dummy_batch(list_names('mol'), max_dim=2)
    b.cochains[0]._x, b.cochains[1]._x, b.cochains[2]._x = T(g['molhiv/v_feats']), T(g['molhiv/e_feats']), None
    b = b.to(DEV)
    with torch.no_grad():
        y, res = model(b, include_partial=True)
    for k, v in res.items():
        gate(v, T(g[f'molhiv/{k}']), f'OGBEmbedSparseCIN fixture {k}')


def test_molhiv_like_full_size_vs_oracle():
    """BASELINE config 3: ogbg-molhiv-like ring-lift, OGBEmbedSparseCIN hidden 64, 2 layers,
    readout mean (exp/scripts/cwn-molhiv.sh), batch 512."""
    from cwn_amd.complex import ComplexBatch
    from cwn_amd.models import OGBEmbedSparseCIN
    from cwn_amd.synthetic import molhiv_like_complexes
    torch.manual_seed(0)
    model = OGBEmbedSparseCIN(1, 2, 64, dropout_rate=0.0, max_dim=2, readout='mean', final_readout='sum',
                              init_reduce='sum', embed_edge=True, use_coboundaries=True, graph_norm='bn').eval()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    b = ComplexBatch.from_complex_list(molhiv_like_complexes(512, seed=3), max_dim=2)
    ref, rpart = O.sparse_cin_model_forward(to_double(state), _oracle_cx(b), 2, readout='mean', embed='ogb')
    model = model.to(DEV)
    with torch.no_grad():
        y, res = model(b.to(DEV), include_partial=True)
    for k, v in rpart.items():
        gate(res[k], v, f'molhiv-512 {k} vs float64 oracle')
    gate(y, ref, 'molhiv-512 prediction vs float64 oracle')


def test_jumping_knowledge_max_vs_oracle():
    """mp/models.py:51, 92-99 with jump_mode='max' (torch_geometric's JumpingKnowledge('max'): elementwise
    maximum over the layers' outputs, per dimension).  The oracle restates the published one-liner; the reference's own
    EmbedSparseCIN with jump_mode='max' is the case 'jk_max' of tests/golden/cell_options.npz (tests/test_gpu_options_golden.py)."""
    from cwn_amd.models import SparseCIN
    torch.manual_seed(3)
    model = SparseCIN(1, 2, 3, 16, dropout_rate=0.0, max_dim=2, jump_mode='max', readout='sum',
                      use_coboundaries=True, graph_norm='id').eval()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    b = dummy_batch(list_names('testing'), max_dim=2)
    g = torch.Generator().manual_seed(5)
    for d in range(3):
        b.cochains[d].x = torch.randn(b.cochains[d].num_cells, 1, generator=g)
    ocx = _oracle_cx(b)
    for c in ocx['cochains']:
        c['x'] = c['x'].double()
    ref, rpart = O.sparse_cin_model_forward(to_double(state), ocx, 3, use_coboundaries=True, norm='id',
                                            jump_mode='max', embed=None)
    model = model.to(DEV)
    with torch.no_grad():
        y, res = model(b.to(DEV), include_partial=True)
    for k, v in rpart.items():
        gate(res[k], v, f'JK-max {k} vs float64 oracle')
    gate(y, ref, 'JK-max prediction vs float64 oracle')
    with pytest.raises(NotImplementedError):
        SparseCIN(1, 2, 3, 16, jump_mode='lstm')


@pytest.mark.parametrize('readout', ['sum', 'mean'])
def test_reddit_like_full_size_vs_oracle(readout):
    """BASELINE config 5: REDDIT-like clique complexes (hubs of degree >= 100: skewed segments,
    F = 1 inputs), SparseCIN hidden 64, 4 layers, no coboundaries, norm id, JK cat, batch 32.
    `readout='mean'` is the NORMALISED variant: with `sum` the pooled rows are sums over thousands of
    cells (|ref|_inf 30 .. 80) and two of them pass the relative gate only (1.2e-5 absolute); pooled as means every compared
    tensor is O(1) and the north star's ABSOLUTE 1e-5 is asserted -- scale, not arithmetic, is what exceeded it."""
    from cwn_amd.complex import ComplexBatch
    from cwn_amd.models import SparseCIN
    from cwn_amd.synthetic import reddit_like_complexes, batch_stats
    torch.manual_seed(0)
    model = SparseCIN(1, 2, 4, 64, dropout_rate=0.0, max_dim=2, jump_mode='cat', readout=readout,
                      use_coboundaries=False, graph_norm='id').eval()
    with torch.no_grad():            # keep activations O(1) without a norm layer (degrees reach 300)
        for p in model.parameters():
            p.mul_(0.3)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    b = ComplexBatch.from_complex_list(reddit_like_complexes(32, seed=1), max_dim=2)
    st = batch_stats(b)
    assert st['cells'] > 30_000
    ocx = _oracle_cx(b)
    for c in ocx['cochains']:
        c['x'] = c['x'].double()
    ref, rpart = O.sparse_cin_model_forward(to_double(state), ocx, 4, use_coboundaries=False, norm='id',
                                            jump_mode='cat', embed=None, readout=readout)
    # the propagate outputs of the first layer are integer-valued (all-ones features): exact
    prm = b.to(DEV).get_cochain_params(dim=0, include_down_features=False)
    up, _, _ = run_base(prm)
    deg = torch.bincount(cpu(prm.up_index)[1], minlength=prm.x.size(0)).float().unsqueeze(1)
    assert torch.equal(cpu(up), deg) and deg.max() >= 100
    model = model.to(DEV)
    with torch.no_grad():
        y, res = model(b, include_partial=True)
    worst = 0.0
    for k, v in rpart.items():
        worst = max(worst, gate(res[k], v, f'REDDIT-32 (readout {readout}) {k} vs float64 oracle'))
    worst = max(worst, gate(y, ref, f'REDDIT-32 (readout {readout}) prediction vs float64 oracle'))
    if readout == 'mean':
        assert worst <= 1e-5, worst           # the absolute bar, on every compared tensor


# ------------------------------------------------------------------------------------------------
# device-side collate: bit-exact against the reference's batching layouts
# ------------------------------------------------------------------------------------------------
def _assert_batch_equal(got, ref_cochains, dimension):
    assert got.dimension == dimension
    for d in range(dimension + 1):
        for k in ('x', 'upper_index', 'lower_index', 'shared_boundaries', 'shared_coboundaries',
                  'boundary_index', 'y', 'batch'):
            a, r = got.cochains[d][k], ref_cochains[d][k]
            assert (a is None) == (r is None), (d, k)
            if a is not None:
                assert a.dtype == r.dtype and torch.equal(cpu(a), cpu(r)), (d, k)


@pytest.mark.parametrize('lname', ['testing', 'testing3', 'mol', 'pair', 'nodes_only'])
def test_device_collate_matches_reference_layout(lname):
    from cwn_amd.packed import PackedComplexes
    from tests._golden import complex_dict
    g = load('batching.npz')
    names = [str(n) for n in g[f'{lname}/names']]
    md = int(g[f'{lname}/max_dim'])
    packed = PackedComplexes([dummy_complex(n) for n in names], DEV, max_dim=md)
    b = packed.collate(range(len(names)))
    ref = complex_dict(g, f'{lname}/batch')
    _assert_batch_equal(b, ref['cochains'], ref['dimension'])
    assert torch.equal(cpu(b.y), ref['y']) and b.num_complexes == len(names)
    for d in range(ref['dimension'] + 1):
        assert b.cochains[d].num_cells == ref['cochains'][d]['num_cells']


def test_device_collate_subsets_and_forward():
    """Arbitrary index subsets equal the CPU container collate; the result feeds the engine."""
    from cwn_amd.blockplan import BlockPlan
    from cwn_amd.complex import ComplexBatch
    from cwn_amd.packed import PackedComplexes
    from cwn_amd.synthetic import zinc_like_complexes
    cxs = zinc_like_complexes(40, seed=9)
    packed = PackedComplexes(cxs, DEV, max_dim=2)
    gsel = torch.Generator().manual_seed(0)
    for _ in range(3):
        idx = torch.randperm(40, generator=gsel)[:17].tolist()
        got = packed.collate(idx)
        ref = ComplexBatch.from_complex_list([cxs[i] for i in idx], max_dim=2)
        _assert_batch_equal(got, ref.cochains, ref.dimension)
        assert torch.equal(cpu(got.y), ref.y)
        # the per-complex tables travel too, so the blocked layer kernel serves device-collated batches
        pg, pr = got.block_plan(), BlockPlan.from_batch(ref)
        assert pg is not None and pr is not None and pg.C == pr.C == 17
        for d in range(3):
            assert np.array_equal(pg.cells[d], pr.cells[d])
            for a, b_ in ((pg.up_ptr[d], pr.up_ptr[d]), (pg.b_ptr[d], pr.b_ptr[d])):
                assert (a is None) == (b_ is None) and (a is None or np.array_equal(a, b_))
    from cwn_amd.models import EmbedSparseCIN
    torch.manual_seed(0)
    model = EmbedSparseCIN(28, 4, 1, 2, 64, dropout_rate=0.0, embed_edge=True, use_coboundaries=True).to(DEV).eval()
    with torch.no_grad():
        y1 = model(packed.collate(idx))
        y2 = model(ComplexBatch.from_complex_list([cxs[i] for i in idx], max_dim=2).to(DEV))
    assert torch.equal(y1, y2)


def test_cinpp_quirk_lower_stream_is_always_zero():
    """CINppCochainConv inherits use_down_msg=False from SparseCINCochainConv
    (mp/layers.py:167-168, 223-226) and its forward never passes down_attr (:243-247), so the lower
    stream is zeros whether or not a lower index is supplied."""
    from cwn_amd.layers import CINppConv
    torch.manual_seed(0)
    F = 8
    conv = CINppConv(F, F, F, None, None, None, None, None, None, max_dim=2, hidden=F,
                     act_module=torch.nn.ReLU, layer_dim=F, use_coboundaries=True).to(DEV).eval()
    b = dummy_batch(list_names('mol'), max_dim=2, device=DEV)
    g = torch.Generator().manual_seed(4)
    for d in range(3):
        b.cochains[d].x = torch.randn(b.cochains[d].num_cells, F, generator=g).to(DEV)
    with torch.no_grad():
        outs = conv(*b.get_all_cochain_params(max_dim=2, include_down_features=False))
        assert all(torch.isfinite(o).all() for o in outs) and outs[1].shape == (b.cochains[1].num_cells, F)
        prm = b.get_cochain_params(dim=1, include_down_features=False)
        _, down, _ = conv.mp_levels[1].propagate(prm.up_index, prm.down_index, prm.boundary_index, x=prm.x,
                                                 up_attr=prm.kwargs['up_attr'],
                                                 boundary_attr=prm.kwargs['boundary_attr'])
        assert not down.any()
        outs2 = conv(*b.get_all_cochain_params(max_dim=2, include_down_features=True))
        for o, o2 in zip(outs, outs2):
            assert torch.equal(o, o2)
        assert conv.mp_levels[1].use_down_msg is False


# ------------------------------------------------------------------------------------------------
# long rows (hubs): whole-workgroup reduction path of cwn_aggregate_f32
# ------------------------------------------------------------------------------------------------
def _hub_index(g, n_dst, n_src, n_aux):
    # rows 5 and n_dst-1 are hubs (1500 / 700 / 65 / 64 entries: both sides of CWN_LONG_ROW), the rest sparse
    dst = torch.cat([torch.full((1500,), 5), torch.full((700,), n_dst - 1), torch.full((65,), 9),
                     torch.full((64,), 10), torch.randint(0, n_dst, (4000,), generator=g)])
    dst = dst[torch.randperm(dst.numel(), generator=g)]
    src = torch.randint(0, n_src, (dst.numel(),), generator=g)
    aux = torch.randint(0, n_aux, (dst.numel(),), generator=g)
    return torch.stack([src, dst]), aux


@pytest.mark.parametrize('F', [1, 3, 8, 64, 128, 130, 512])
@pytest.mark.parametrize('reduce', ['add', 'mean', 'max'])
def test_long_rows_identity_message_exact_on_integers(F, reduce):
    """Integer-valued features: any summation order gives the same fp32 result, so the chunked
    hub reduction must equal the oracle's sequential scatter bit for bit."""
    from cwn_amd import ops
    from cwn_amd.csr import Adjacency
    g = torch.Generator().manual_seed(F * 7 + len(reduce))
    n_dst, n_src = 300, 211
    idx, aux = _hub_index(g, n_dst, n_src, 50)
    x = torch.randint(-8, 9, (n_src, F), generator=g).float()
    sx = torch.randint(-3, 4, (n_dst, F), generator=g).float()
    adj = Adjacency.from_index(idx.to(DEV), n_dst, n_src, aux.to(DEV), 50)
    assert adj.long_row_list().numel() >= 3
    got = ops.aggregate(adj, n_dst, x.to(DEV), reduce=reduce, self_x=sx.to(DEV))
    want = O.scatter_rows(x[idx[0]], idx[1], n_dst, reduce) + sx
    if reduce == 'mean':
        torch.testing.assert_close(cpu(got), want, rtol=1e-6, atol=1e-6)
    else:
        assert torch.equal(cpu(got), want)


@pytest.mark.parametrize('F', [4, 64, 128])
@pytest.mark.parametrize('op', ['plus', 'times', 'relu_plus'])
def test_long_rows_two_operand_messages_and_backward(F, op):
    from cwn_amd import ops
    from cwn_amd.csr import Adjacency
    g = torch.Generator().manual_seed(F + len(op))
    n_dst = n_src = 257
    n_aux = 91
    idx, aux = _hub_index(g, n_dst, n_src, n_aux)
    x = torch.randn(n_src, F, generator=g, dtype=torch.float64)
    ua = torch.randn(n_aux, F, generator=g, dtype=torch.float64)
    msg_op = {'plus': ops.MSG_A_PLUS_B, 'times': ops.MSG_A_TIMES_B, 'relu_plus': ops.MSG_RELU_A_PLUS_B}[op]

    def ref(xr, ur):
        a, b = xr[idx[0]], ur[aux]
        m = a + b if op == 'plus' else (a * b if op == 'times' else torch.relu(a + b))
        return torch.zeros(n_dst, F, dtype=m.dtype).index_add_(0, idx[1], m)

    xr, ur = x.clone().requires_grad_(), ua.clone().requires_grad_()
    want = ref(xr, ur)
    w = torch.randn(n_dst, F, generator=g, dtype=torch.float64)
    (want * w).sum().backward()
    adj = Adjacency.from_index(idx.to(DEV), n_dst, n_src, aux.to(DEV), n_aux)
    # (the multiplicative attribute has no fused gradient: ops.py routes trainable ones elsewhere)
    xg, ug = x.float().to(DEV).requires_grad_(), ua.float().to(DEV).requires_grad_(op != 'times')
    got = ops.aggregate(adj, n_dst, xg, msg_op=msg_op, B=ug)
    (got * w.float().to(DEV)).sum().backward()
    # the transposed plans have hubs of their own only where a SOURCE is popular; here the
    # destination hubs make long rows in forward, and t_aux (91 rows, ~70 entries each) in backward
    assert adj.t_aux.long_row_list().numel() > 0
    scale = float(want.detach().abs().max())
    torch.testing.assert_close(cpu(got).double(), want.detach(), rtol=1e-5, atol=1e-5 * scale)
    torch.testing.assert_close(cpu(xg.grad).double(), xr.grad, rtol=1e-5, atol=1e-5 * float(xr.grad.abs().max()))
    if op != 'times':
        torch.testing.assert_close(cpu(ug.grad).double(), ur.grad, rtol=1e-5,
                                   atol=1e-5 * float(ur.grad.abs().max()))


@pytest.mark.parametrize('F', [1, 3, 8, 64, 128, 130])
@pytest.mark.parametrize('op', ['id', 'plus', 'times', 'relu_plus'])
def test_wide_and_small_addressing_are_bit_identical(F, op):
    """cwn_aggregate_f32 has two addressing variants (32-bit byte offsets when the caller sets
    CWN_AGG_SMALL_OPERANDS, 64-bit otherwise): same arithmetic, same order -- forward and the
    backward kernels (transposed plans, ReLU mask form) must agree bit for bit."""
    from cwn_amd import ops
    from cwn_amd.csr import Adjacency
    g = torch.Generator().manual_seed(11 * F + len(op))
    n_dst, n_src, n_aux = 300, 211, 50
    idx, aux = _hub_index(g, n_dst, n_src, n_aux)
    x = torch.randn(n_src, F, generator=g)
    ua = torch.randn(n_aux, F, generator=g)
    sx = torch.randn(n_dst, F, generator=g)
    eps = torch.tensor([0.25])
    w = torch.randn(n_dst, F, generator=g).to(DEV)
    msg_op = {'id': ops.MSG_A, 'plus': ops.MSG_A_PLUS_B, 'times': ops.MSG_A_TIMES_B,
              'relu_plus': ops.MSG_RELU_A_PLUS_B}[op]
    res = []
    for small in (True, False):
        ops.ALLOW_SMALL_OPERANDS = small
        try:
            adj = Adjacency.from_index(idx.to(DEV), n_dst, n_src, aux.to(DEV), n_aux)
            xg = x.to(DEV).requires_grad_()
            ug = ua.to(DEV).requires_grad_(op in ('plus', 'relu_plus'))
            sg = sx.to(DEV).requires_grad_()
            got = ops.aggregate(adj, n_dst, xg, msg_op=msg_op, B=None if op == 'id' else ug,
                                self_x=sg, eps=eps.to(DEV))
            (got * w).sum().backward()
            res.append([got.detach(), xg.grad, sg.grad] + ([ug.grad] if ug.requires_grad else []))
        finally:
            ops.ALLOW_SMALL_OPERANDS = True
    for a, b in zip(*res):
        assert torch.equal(a, b)
    a, b = x[idx[0]], ua[aux]
    m = a if op == 'id' else (a + b if op == 'plus' else (a * b if op == 'times' else torch.relu(a + b)))
    want = torch.zeros(n_dst, F).index_add_(0, idx[1], m) + 1.25 * sx
    torch.testing.assert_close(cpu(res[0][0]), want, rtol=1e-5, atol=1e-5 * float(want.abs().max()))


def test_long_rows_are_deterministic():
    from cwn_amd import ops
    from cwn_amd.csr import Adjacency
    g = torch.Generator().manual_seed(5)
    idx, aux = _hub_index(g, 300, 211, 50)
    x = torch.randn(211, 64, generator=g).to(DEV)
    outs = []
    for _ in range(3):
        adj = Adjacency.from_index(idx.to(DEV), 300, 211)     # the long-row LIST order may differ
        outs.append(ops.aggregate(adj, 300, x))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


# ------------------------------------------------------------------------------------------------
# cwn_gemm_f32 on the bf16 matrix pipe (exact three-way split of both operands)
# ------------------------------------------------------------------------------------------------
def _both_gemm_paths(make):
    """Run the same launch with the split path allowed and forbidden."""
    from cwn_amd import _ffi, ops
    outs = []
    prev = ops.set_gemm_exact(False)
    try:
        for exact in (False, True):
            ops.set_gemm_exact(exact)
            outs.append([y.clone() for y in ops.run_gemm(make(), DEV)])
    finally:
        ops.set_gemm_exact(prev)
    return outs


@pytest.mark.parametrize('M', [1, 63, 64, 65, 3341, 20000])
def test_gemm_split_path_has_fp32_accuracy(M):
    """N = K = 128 launches run as six bf16 MFMAs per product on exactly-split operands: the
    error against float64 must be at the level of the fp32-MFMA kernel (a few 1e-7 of |x|.|w|;
    plain bf16 would be 4e-3), with bias, BatchNorm-eval affine, ReLU, a column slice of a wider
    weight and several GEMMs in one launch.
    (A tolerance cannot tell whether all six terms are there: tests/test_gpu_split_terms.py pins each term and plane.)"""
    from cwn_amd import ops
    g = torch.Generator().manual_seed(M)
    W2 = (torch.randn(128, 256, generator=g) / 16).to(DEV)          # [N, 2F]: two column halves
    X = [torch.randn(m, 128, generator=g).to(DEV) for m in (M, max(M // 3, 1), M + 5)]
    b = torch.randn(128, generator=g).to(DEV)
    sc, sh = (torch.rand(128, generator=g) + 0.5).to(DEV), torch.randn(128, generator=g).to(DEV)

    def make():
        return [ops.Gemm(X=X[0], W=W2[:, :128], bias=b),
                ops.Gemm(X=X[1], W=W2[:, 128:]),
                ops.Gemm(X=X[2], W=W2[:, :128], bias=b, out_scale=sc, out_shift=sh, relu=True)]

    split, exact = _both_gemm_paths(make)
    for i, (ys, ye) in enumerate(zip(split, exact)):
        Wd = (W2[:, :128] if i != 1 else W2[:, 128:]).double()
        ref = X[i].double() @ Wd.t()
        bound = X[i].double().abs() @ Wd.abs().t() + 1.0
        if i != 1:
            ref = ref + b.double()
        if i == 2:
            ref = torch.relu(ref * sc.double() + sh.double())
            bound = bound * sc.double()
        for y in (ys, ye):
            assert float(((y.double() - ref).abs() / bound).max()) < 2e-6
    if M >= 64:
        assert not torch.equal(split[0], exact[0])       # the two kernels really differ


@pytest.mark.parametrize('M', [1, 64, 3341, 20000])
def test_gemm_split_packed_weight_is_bit_identical(M):
    """cwn_gemm_pack_weights_f32 + CWN_GEMM_W_PACKED: the stationary operand split once per weight version
    instead of in every workgroup -- the same numbers in the same MFMA order, so the results are the
    fp32-weight launch's bit for bit (bias, BatchNorm-eval affine, ReLU, several GEMMs per launch); a packed
    weight in a launch that does not run on the split path is an argument error, and the Python layer
    falls back to the fp32 weight there.
    (Packed = unpacked links two kernels to each other; tests/test_gpu_split_terms.py pins the packed planes to the integers.)"""
    import ctypes as C
    from cwn_amd import _ffi, ops
    g = torch.Generator().manual_seed(100 + M)
    Ws = [torch.nn.Parameter((torch.randn(128, 128, generator=g) / 16).to(DEV)) for _ in range(2)]
    X = [torch.randn(m, 128, generator=g).to(DEV) for m in (M, M + 7)]
    b = torch.randn(128, generator=g).to(DEV)
    sc, sh = (torch.rand(128, generator=g) + 0.5).to(DEV), torch.randn(128, generator=g).to(DEV)

    def make(packed):
        pk = [ops.pack_gemm_weight(w) if packed else None for w in Ws]
        return [ops.Gemm(X=X[0], W=Ws[0], bias=b, relu=True, out_scale=sc, out_shift=sh, w_packed=pk[0]),
                ops.Gemm(X=X[1], W=Ws[1], w_packed=pk[1])]

    with torch.no_grad():
        plain = ops.run_gemm(make(False), DEV)
        packed = ops.run_gemm(make(True), DEV)
        assert ops.pack_gemm_weight(Ws[0]) is ops.pack_gemm_weight(Ws[0])          # cached per version
        for a, c in zip(plain, packed):
            assert torch.equal(a, c)
        # a new weight version is packed again
        old = ops.pack_gemm_weight(Ws[0])
        Ws[0].mul_(2.0)
        assert ops.pack_gemm_weight(Ws[0]) is not old
        assert torch.equal(ops.run_gemm(make(True), DEV)[0], ops.run_gemm(make(False), DEV)[0])
        # exact launches take the fp32 weight (the Python layer does not pass the packed one) ...
        ex = make(True)
        for gm in ex:
            gm.exact = True
        exact = ops.run_gemm(ex, DEV)
        assert float((exact[1] - packed[1]).abs().max()) < 1e-4
        # ... and the C ABI refuses a packed weight outside the split path
        Y = torch.empty(M + 7, 128, device=DEV)
        d = make(True)[1].desc(Y, packed=True)
        d.flags |= _ffi.GEMM_EXACT
        arr = (_ffi.GemmDesc * 1)(d)
        assert _ffi.lib().cwn_gemm_f32(arr, 1, _ffi.stream_ptr(torch.device(DEV))) != 0
    assert ops.pack_gemm_weight(torch.nn.Parameter(torch.zeros(64, 128, device=DEV))) is None
    assert _ffi.lib().cwn_gemm_packed_weight_bytes() == 128 * 128 * 6


@pytest.mark.parametrize('F', [128, 64])
@pytest.mark.parametrize('rows', [(3165, 3341, 304), (1, 33, 0), (64, 31, 32), (65, 129, 63), (9001, 11000, 1203)])
def test_fused_update_mlp_vs_float64_and_three_launch_path(rows, F):
    """cwn_update_mlp_f32 (csrc/cwn_mlp.hip): update_up_nn, update_boundaries_nn and combine_nn of every
    dimension (mp/layers.py:193-199, :303-325) in one launch, against the same networks evaluated in float64
    on the CPU (north-star gate) and against the three grouped GEMM launches it replaces."""
    from cwn_amd import layers
    from cwn_amd.layers import SparseCINConv
    torch.manual_seed(sum(rows) + F)
    conv = SparseCINConv(F, F, F, None, None, None, None, max_dim=2, hidden=F, act_module=torch.nn.ReLU,
                         layer_dim=F, use_coboundaries=True, graph_norm=torch.nn.BatchNorm1d).eval()
    with torch.no_grad():                                # non-trivial BatchNorm statistics and affine
        for name, buf in conv.named_buffers():
            if name.endswith('running_mean'):
                buf.copy_(torch.randn_like(buf) * 0.2)
            elif name.endswith('running_var'):
                buf.copy_(torch.rand_like(buf) + 0.5)
        for m in conv.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.copy_(torch.rand_like(m.weight) + 0.5)
                m.bias.copy_(torch.randn_like(m.bias) * 0.1)
    g = torch.Generator().manual_seed(1)
    outs = []
    for n in rows:
        outs += [torch.randn(n, F, generator=g) * 2, torch.randn(n, F, generator=g) * 2]
    ref = []
    conv64 = copy.deepcopy(conv).double()
    with torch.no_grad():
        for d in range(3):
            lvl = conv64.mp_levels[d]
            if rows[d] == 0:
                ref.append(torch.zeros(0, F, dtype=torch.float64))
                continue
            hu = lvl.update_up_nn(outs[2 * d].double())
            hb = lvl.update_boundaries_nn(outs[2 * d + 1].double())
            ref.append(lvl.combine_nn(torch.cat([hu, hb], dim=-1)))
    conv = conv.to(DEV)
    dev_outs = [o.to(DEV) for o in outs]
    plans = ['blocked'] * 3

    def run(fused):
        prev = layers.FUSED_UPDATE_MLP
        layers.FUSED_UPDATE_MLP = fused
        try:
            with torch.no_grad():
                return conv._dense_eval(plans, dev_outs)
        finally:
            layers.FUSED_UPDATE_MLP = prev

    got, three = run(True), run(False)
    assert got is not None and three is not None
    for d in range(3):
        assert got[d].shape == (rows[d], F)
        gate(got[d], ref[d], f'fused update MLP dim {d} ({rows[d]} rows) vs float64')
        gate(three[d], ref[d], f'three-launch update MLP dim {d} vs float64')
    if sum(-(-r // (4096 // F)) for r in rows) > 256:
        # round 5: a launch of more workgroups than the chip has CUs runs the sequential schedule, two workgroups per CU
        # (csrc/cwn_mlp.hip: Shape<F, 2, true>); the same rows in pieces of one round each run the alternating one -- per row
        # the same arithmetic
        pieces = []
        with torch.no_grad():
            for d in range(3):
                parts = []
                for lo in range(0, rows[d], 4096):
                    sub = [torch.zeros(0, F, device=DEV)] * 6
                    sub[2 * d], sub[2 * d + 1] = dev_outs[2 * d][lo:lo + 4096], dev_outs[2 * d + 1][lo:lo + 4096]
                    parts.append(conv._dense_eval(plans, sub)[d])
                pieces.append(torch.cat(parts))
        assert all(torch.equal(a, b) for a, b in zip(got, pieces))
        print(f'[gate] fused update MLP, {sum(rows)} rows at width {F}: the two-per-CU schedule bit-identical to the alternating one')


@pytest.mark.parametrize('F', [64, 128])
@pytest.mark.parametrize('w_in', [1, 3, 20])
@pytest.mark.parametrize('rows', [(3165, 7000, 304), (70, 0, 3)])
def test_fused_update_mlp_over_narrow_inputs(rows, w_in, F):
    """The first layer of a model over raw features (REDDIT-BINARY: one constant feature, mp/models.py:112-260; exp/scripts/
    mpsn-redditb.sh): update networks Linear(w_in -> F) ... with w_in < F.  cwn_update_mlp_f32 takes the narrow rows as they are
    (cwn_mlp_dim.in_width; the first weights zero-padded once per version) -- against float64 and against the grouped launches
    it replaces (three generic GEMM launches, 84 us of a 0.34 ms REDDIT-32 forward)."""
    from cwn_amd import layers
    from cwn_amd.layers import SparseCINConv
    torch.manual_seed(sum(rows) + F + w_in)
    conv = SparseCINConv(w_in, w_in, w_in, None, None, None, None, max_dim=2, hidden=F, act_module=torch.nn.ReLU,
                         layer_dim=w_in, use_coboundaries=False, graph_norm=torch.nn.Identity).eval()
    g = torch.Generator().manual_seed(1)
    outs = []
    for n in rows:
        outs += [torch.randn(n, w_in, generator=g) * 2, torch.randn(n, w_in, generator=g) * 2]
    conv64 = copy.deepcopy(conv).double()
    ref = []
    with torch.no_grad():
        for d in range(3):
            lvl = conv64.mp_levels[d]
            if rows[d] == 0:
                ref.append(torch.zeros(0, F, dtype=torch.float64))
                continue
            ref.append(lvl.combine_nn(torch.cat([lvl.update_up_nn(outs[2 * d].double()), lvl.update_boundaries_nn(outs[2 * d + 1].double())], dim=-1)))
    conv = conv.to(DEV)
    dev_outs = [o.to(DEV) for o in outs]

    def run(fused):
        prev = layers.FUSED_UPDATE_MLP
        layers.FUSED_UPDATE_MLP = fused
        try:
            with torch.no_grad():
                return conv._dense_eval(['blocked'] * 3, dev_outs)
        finally:
            layers.FUSED_UPDATE_MLP = prev
    three, got, again = run(False), run(True), run(True)
    assert conv in layers._MLP_CACHE and layers._MLP_CACHE[conv][0].w_in == [w_in] * 3       # the one-launch form served it
    for d in range(3):
        assert got[d].shape == (rows[d], F) and torch.equal(got[d], again[d])
        gate(got[d], ref[d], f'fused update MLP over {w_in}-wide inputs, width {F}, dim {d} ({rows[d]} rows) vs float64')
        gate(three[d], ref[d], f'three-launch form, dim {d} vs float64')
    # a strided view (columns of a wider matrix) is taken as it is
    wide = [torch.randn(n, w_in + 5, generator=g).to(DEV) for n in rows for _ in range(2)]
    with torch.no_grad():
        a = conv._dense_eval(['blocked'] * 3, [w[:, 2:2 + w_in] for w in wide])
        b = conv._dense_eval(['blocked'] * 3, [w[:, 2:2 + w_in].contiguous() for w in wide])
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    # the first weight written in place: the padded form follows
    with torch.no_grad():
        conv.mp_levels[1].update_up_nn[0].weight.mul_(2.0)
        c = conv._dense_eval(['blocked'] * 3, dev_outs)
    assert not torch.equal(c[1], got[1]) or rows[1] == 0
    layers._MLP_CACHE.pop(conv, None)
    with torch.no_grad():
        assert all(torch.equal(u, v) for u, v in zip(c, conv._dense_eval(['blocked'] * 3, dev_outs)))


def test_gemm_split_path_identity_is_exact_and_fallbacks_are_untouched():
    from cwn_amd import ops
    g = torch.Generator().manual_seed(3)
    W = (torch.randn(128, 128, generator=g) / 16).to(DEV)
    eye = torch.eye(128, device=DEV)
    split, exact = _both_gemm_paths(lambda: [ops.Gemm(X=eye, W=W)])
    # 1.0 splits into (1, 0, 0) and w = hi + mid + lo exactly: an asymmetric W comes back transposed, bit for bit
    assert torch.equal(split[0], W.t()) and torch.equal(exact[0], W.t())
    assert ops.gemm_uses_split([ops.Gemm(X=eye, W=W)], DEV)
    # launches the split kernel does not serve (K != 128, K-concat, prologue) are the exact kernel's either way
    X64, W64 = torch.randn(300, 64, generator=g).to(DEV), torch.randn(128, 64, generator=g).to(DEV)
    X, X2 = torch.randn(300, 128, generator=g).to(DEV), torch.randn(300, 128, generator=g).to(DEV)
    Wc = torch.randn(128, 256, generator=g).to(DEV)
    s1 = torch.rand(128, generator=g).to(DEV)
    for make in (lambda: [ops.Gemm(X=X64, W=W64)],
                 lambda: [ops.Gemm(X=X, X2=X2, W=Wc)],
                 lambda: [ops.Gemm(X=X, W=W, in_scale=s1, in_shift=s1, in_relu=1)]):
        assert not ops.gemm_uses_split(make(), DEV)
        a, b_ = _both_gemm_paths(make)
        assert torch.equal(a[0], b_[0])


def test_gemm_narrow_grouped_concat_affine_stats():
    """The 64 x 64 tile shape with every fused piece: K-concatenation, input affine + ReLU, output
    affine, column statistics, row strides (molhiv-like hidden 64)."""
    from cwn_amd import ops
    g = torch.Generator().manual_seed(123)
    M, H = 777, 64
    Xfull = torch.randn(M, 2 * H, generator=g)
    X = Xfull[:, :H]                                         # ldx = 128
    X2 = torch.randn(M, H, generator=g)
    W = torch.randn(H, 2 * H, generator=g) / (2 * H) ** 0.5
    b = torch.randn(H, generator=g)
    isc, ish = torch.rand(H, generator=g) + 0.5, torch.randn(H, generator=g)
    osc, osh = torch.rand(H, generator=g) + 0.5, torch.randn(H, generator=g)
    Xd, X2d = Xfull.to(DEV)[:, :H], X2.to(DEV)
    assert Xd.stride(0) == 2 * H
    stats = torch.empty(2, ops.stat_rows(M), H, device=DEV, dtype=torch.float64)
    gm = [ops.Gemm(X=Xd, X2=X2d, W=W.to(DEV), bias=b.to(DEV), in_scale=isc.to(DEV), in_shift=ish.to(DEV),
                   in_relu=True, out_scale=osc.to(DEV), out_shift=osh.to(DEV), relu=True, col_stats=stats),
          ops.Gemm(X=X2d, W=W[:40, :H].to(DEV), bias=None)]
    Y, Y2 = ops.run_gemm(gm, DEV)
    xin = torch.cat([torch.relu(X.double() * isc.double() + ish.double()), X2.double()], 1)
    pre = xin @ W.double().t() + b.double()
    ref = torch.relu(pre * osc.double() + osh.double())
    torch.testing.assert_close(cpu(Y).double(), ref, rtol=1e-5, atol=3e-5)
    torch.testing.assert_close(cpu(stats[0].sum(0)), pre.sum(0), rtol=1e-6, atol=1e-3)
    torch.testing.assert_close(cpu(stats[1].sum(0)), (pre * pre).sum(0), rtol=1e-6, atol=1e-3)
    torch.testing.assert_close(cpu(Y2).double(), X2.double() @ W[:40, :H].double().t(), rtol=1e-5, atol=2e-5)


# ------------------------------------------------------------------------------------------------
# training-mode dense path: transposed-weight GEMM, weight-gradient GEMM, BatchNorm pieces, and
# the whole SparseCINConv layer forward + backward against the torch modules
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,N,K', [(1, 1, 1), (100, 128, 128), (3341, 128, 256), (77, 40, 24), (513, 64, 64),
                                   (1000, 256, 128)])
def test_gemm_transposed_weight_matches_float64(M, N, K):
    """dX = dY @ W with W in Linear layout [K_in_of_this_product = rows, N = cols]."""
    from cwn_amd import ops
    g = torch.Generator().manual_seed(M + 3 * N + 7 * K)
    X = torch.randn(M, K, generator=g)
    Wt = torch.randn(K, N, generator=g) / K ** 0.5
    Y, = ops.run_gemm([ops.Gemm(X=X.to(DEV), W=Wt.to(DEV), w_trans=True)], DEV)
    torch.testing.assert_close(cpu(Y).double(), X.double() @ Wt.double(), rtol=1e-5, atol=2e-5)


@pytest.mark.parametrize('M,N,K,K2', [(1, 1, 1, 0), (300, 128, 128, 0), (3341, 128, 128, 128), (77, 40, 24, 0),
                                      (1025, 64, 64, 64), (257, 130, 36, 12), (5000, 128, 128, 0)])
def test_gemm_tn_weight_gradient(M, N, K, K2):
    from cwn_amd import _ffi
    g = torch.Generator().manual_seed(M + N + K + K2)
    dZ = torch.randn(M, N, generator=g)
    X = torch.randn(M, K, generator=g)
    X2 = torch.randn(M, K2, generator=g) if K2 else None
    sc, sh = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g)
    dZd, Xd, X2d, scd, shd = dZ.to(DEV), X.to(DEV), None if X2 is None else X2.to(DEV), sc.to(DEV), sh.to(DEV)
    dW = torch.zeros(N, K + K2, device=DEV)
    db = torch.zeros(N, device=DEV)
    _ffi.gemm_tn([_ffi.GemmTnDesc(dZ=dZd.data_ptr(), X=Xd.data_ptr(), X2=_ffi.ptr(X2d), in_scale=scd.data_ptr(),
                                  in_shift=shd.data_ptr(), in_scale2=None, in_shift2=None, dW=dW.data_ptr(),
                                  db=db.data_ptr(), M=M, lddz=N, ldx=K, ldx2=K2, lddw=K + K2, N=N, K=K, K2=K2,
                                  in_relu=1)], DEV)
    A = torch.relu(X.double() * sc.double() + sh.double())
    if X2 is not None:
        A = torch.cat([A, X2.double()], 1)
    ref = dZ.double().t() @ A
    tol = 2e-5 * max(1.0, float(ref.abs().max()))
    torch.testing.assert_close(cpu(dW).double(), ref, rtol=1e-5, atol=tol)
    torch.testing.assert_close(cpu(db).double(), dZ.double().sum(0), rtol=1e-5, atol=tol)
    # the workspace form sums the row bands in a fixed order: bit-reproducible, and it ACCUMULATES
    dW.zero_(); db.zero_()
    _ffi.DETERMINISTIC_TN = True
    first = None
    desc = lambda: [_ffi.GemmTnDesc(dZ=dZd.data_ptr(), X=Xd.data_ptr(), X2=_ffi.ptr(X2d), in_scale=scd.data_ptr(),
                                    in_shift=shd.data_ptr(), in_scale2=None, in_shift2=None, dW=dW.data_ptr(),
                                    db=db.data_ptr(), M=M, lddz=N, ldx=K, ldx2=K2, lddw=K + K2, N=N, K=K, K2=K2,
                                    in_relu=1)]
    try:
        _ffi.gemm_tn(desc(), DEV)
        first = dW.clone()
        _ffi.gemm_tn(desc(), DEV)
    finally:
        _ffi.DETERMINISTIC_TN = False
    assert torch.equal(dW, 2 * first)
    torch.testing.assert_close(cpu(first).double(), ref, rtol=1e-5, atol=tol)


@pytest.mark.parametrize('M,N', [(2, 4), (777, 128), (3341, 64), (100, 30), (5000, 256)])
def test_batchnorm_relu_pieces_match_torch(M, N):
    """statistics (GEMM epilogue) -> finalize -> act, and reduce -> apply, against
    torch.nn.BatchNorm1d(train) + ReLU autograd; running statistics included."""
    from cwn_amd import _ffi, ops
    from cwn_amd.dense_train import _norm_desc
    g = torch.Generator().manual_seed(M + N)
    K = 32
    X = torch.randn(M, K, generator=g)
    lin = torch.nn.Linear(K, N)
    bn = torch.nn.BatchNorm1d(N)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(N, K, generator=g) / K ** 0.5)
        lin.bias.copy_(torch.randn(N, generator=g) * 3)          # large mean relative to the spread
        bn.weight.copy_(torch.rand(N, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(N, generator=g))
    ref_bn = torch.nn.BatchNorm1d(N)
    ref_bn.load_state_dict(bn.state_dict())
    Xr = X.clone().double()
    lin64, bn64 = torch.nn.Linear(K, N).double(), ref_bn.double()
    lin64.load_state_dict({k: v.double() for k, v in lin.state_dict().items()})
    z_ref = lin64(Xr).detach().requires_grad_()
    h_ref = torch.relu(bn64(z_ref))
    dH = torch.randn(M, N, generator=g)
    h_ref.backward(dH.double())

    stats = torch.empty(2, ops.stat_rows(M), N, dtype=torch.float64, device=DEV)
    Z, = ops.run_gemm([ops.Gemm(X=X.to(DEV), W=lin.weight.detach().to(DEV), bias=lin.bias.detach().to(DEV),
                                col_stats=stats)], DEV)
    aff = torch.empty(4, N, device=DEV)
    rm, rv = bn.running_mean.clone().to(DEV), bn.running_var.clone().to(DEV)
    gam, bet = bn.weight.detach().to(DEV), bn.bias.detach().to(DEV)
    _ffi.bn_finalize([_ffi.BnDesc(col_sum=stats[0].data_ptr(), col_sumsq=stats[1].data_ptr(), gamma=gam.data_ptr(),
                                  beta=bet.data_ptr(), running_mean=rm.data_ptr(), running_var=rv.data_ptr(),
                                  scale=aff[0].data_ptr(), shift=aff[1].data_ptr(), mean=aff[2].data_ptr(),
                                  rstd=aff[3].data_ptr(), M=M, N=N, eps=bn.eps, momentum=bn.momentum)], DEV)
    H = torch.empty(M, N, device=DEV)
    _ffi.norm_act([_norm_desc(Z, out=H, aff=aff)], DEV)
    torch.testing.assert_close(cpu(H).double(), h_ref.detach(), rtol=1e-5, atol=2e-5)
    torch.testing.assert_close(cpu(rm).double(), bn64.running_mean, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(cpu(rv).double(), bn64.running_var, rtol=1e-5, atol=1e-6)
    s12 = torch.zeros(2, N, device=DEV)
    dHd = dH.to(DEV)
    dZ = torch.empty(M, N, device=DEV)
    _ffi.norm_bwd_reduce([_norm_desc(Z, dy=dHd, aff=aff, s12=s12)], DEV)
    _ffi.norm_bwd_apply([_norm_desc(Z, dy=dHd, out=dZ, aff=aff, s12=s12)], DEV)
    scale = float(z_ref.grad.abs().max())
    torch.testing.assert_close(cpu(dZ).double(), z_ref.grad, rtol=1e-4, atol=2e-5 * max(scale, 1.0))
    torch.testing.assert_close(cpu(s12[1]).double(), bn64.weight.grad, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(cpu(s12[0]).double(), bn64.bias.grad, rtol=1e-4, atol=1e-4)
    # the same in ONE launch (cwn_norm_bwd_f32), sums written / added to what the targets hold; twice: bit-reproducible
    if M <= _ffi.NORM_BWD_FUSED_MAX_ROWS and N % 4 == 0:
        t12 = torch.full((2, N), 3.0, device=DEV)
        dZ2 = torch.empty(M, N, device=DEV)
        _ffi.norm_bwd([_norm_desc(Z, dy=dHd, out=dZ2, aff=aff, s12=t12)], DEV, accumulate=False)
        torch.testing.assert_close(cpu(dZ2).double(), z_ref.grad, rtol=1e-4, atol=2e-5 * max(scale, 1.0))
        torch.testing.assert_close(cpu(t12[1]).double(), bn64.weight.grad, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(cpu(t12[0]).double(), bn64.bias.grad, rtol=1e-4, atol=1e-4)
        first, dZ3 = t12.clone(), torch.empty(M, N, device=DEV)
        _ffi.norm_bwd([_norm_desc(Z, dy=dHd, out=dZ3, aff=aff, s12=t12)], DEV, accumulate=True)
        assert torch.equal(t12, 2 * first) and torch.equal(dZ3, dZ2)
        # identity normalisation: the ReLU mask only, sums untouched
        dZ4 = torch.empty(M, N, device=DEV)
        _ffi.norm_bwd([_norm_desc(Z, dy=dHd, out=dZ4, aff=None)], DEV, accumulate=False)
        assert torch.equal(dZ4, dHd * (Z > 0))
    else:
        with pytest.raises(_ffi.CwnError):
            _ffi.norm_bwd([_norm_desc(Z, dy=dHd, out=torch.empty(M, N, device=DEV), aff=aff, s12=s12)], DEV, accumulate=False)


def _train_layer_pair(graph_norm, hidden, use_cob, seed=0):
    """Two identical SparseCINConv layers in train mode: one takes the fused training path, the
    other the torch modules (FUSED_DENSE_TRAINING off)."""
    from cwn_amd import layers
    kw = dict(passed_msg_up_nn=None, passed_msg_boundaries_nn=None, passed_update_up_nn=None,
              passed_update_boundaries_nn=None, train_eps=True, max_dim=2, hidden=hidden,
              act_module=torch.nn.ReLU, layer_dim=hidden, graph_norm=graph_norm, use_coboundaries=use_cob)
    torch.manual_seed(seed)
    a = layers.SparseCINConv(hidden, hidden, hidden, **kw).to(DEV).train()
    b = layers.SparseCINConv(hidden, hidden, hidden, **kw).to(DEV).train()
    b.load_state_dict(a.state_dict())
    return a, b


@pytest.mark.parametrize('into_grad', [False, True])
def test_one_launch_batchnorm_backward_gives_the_same_gradients(into_grad):
    """dense_train.FUSED_NORM_BACKWARD (cwn_norm_bwd_f32, the bit-reproducible form) against reduce + apply: same layer,
    same inputs; with `into_grad` the sums are added straight into gamma.grad / beta.grad (pre-filled with ones)."""
    from cwn_amd import dense_train as DT, ops
    from cwn_amd.synthetic import zinc_like_batch
    a, bl = _train_layer_pair(torch.nn.BatchNorm1d, 128, True, seed=3)
    b = zinc_like_batch(8, seed=2, device=DEV)
    g = torch.Generator().manual_seed(0)
    xs = [torch.randn(b.cochains[d].num_cells, 128, generator=g).to(DEV) for d in range(3)]
    ws = [torch.randn(b.cochains[d].num_cells, 128, generator=g).to(DEV) for d in range(3)]

    def run(conv, fused):
        DT.FUSED_NORM_BACKWARD = fused
        try:
            if into_grad:
                for p in conv.parameters():
                    p.grad = torch.ones_like(p)
            xin = [x.clone().requires_grad_() for x in xs]
            b.set_xs(xin)
            out = conv(*b.get_all_cochain_params(max_dim=2, include_down_features=False))
            with ops.accumulate_into_grad(into_grad):
                sum((o * w).sum() for o, w in zip(out, ws)).backward()
        finally:
            DT.FUSED_NORM_BACKWARD = False
        return xin

    xa, xb = run(a, True), run(bl, False)
    for u, v in zip(xa, xb):
        torch.testing.assert_close(u.grad, v.grad, rtol=1e-4, atol=1e-4 * max(1.0, float(v.grad.abs().max())))
    for (n, p), q in zip(a.named_parameters(), bl.parameters()):
        if q.grad is None:
            assert p.grad is None, n
            continue
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-4, atol=1e-4 * max(1.0, float(q.grad.abs().max())), msg=n)


@pytest.mark.parametrize('norm,hidden,use_cob', [('bn', 128, True), ('bn', 64, False), ('id', 32, True)])
def test_fused_training_layer_matches_torch_modules(norm, hidden, use_cob):
    from cwn_amd import layers
    from cwn_amd.synthetic import zinc_like_batch
    gn = torch.nn.BatchNorm1d if norm == 'bn' else torch.nn.Identity
    fused, plain = _train_layer_pair(gn, hidden, use_cob)
    b = zinc_like_batch(6, seed=5, device=DEV)     # small: fewer chances of a pre-activation at the kink
    state0 = {k: v.clone() for k, v in plain.state_dict().items()}

    def run(conv, fused_on):
        layers.FUSED_DENSE_TRAINING = fused_on
        try:
            xin = [x.clone().requires_grad_() for x in xs]
            b.set_xs(xin)
            params = b.get_all_cochain_params(max_dim=2, include_down_features=False)
            out = conv(*params)
            sum((o * w).sum() for o, w in zip(out, ws)).backward()
        finally:
            layers.FUSED_DENSE_TRAINING = True
        return out, xin

    # ReLU is not differentiable at 0: a pre-activation within rounding distance of 0 may land on
    # either side in the two implementations and legitimately changes a gradient by O(1).  Pick
    # inputs whose pre-activations (in the torch-module run) all stay clear of the kink.
    near = []
    hooks = [m.register_forward_hook(lambda mod, inp, out: near.append(float(inp[0].detach().abs().min())))
             for m in plain.modules() if isinstance(m, torch.nn.ReLU)]
    for seed in range(1, 40):
        g = torch.Generator().manual_seed(seed)
        xs = [torch.randn(b.cochains[d].num_cells, hidden, generator=g).to(DEV) for d in range(3)]
        ws = [torch.randn(b.cochains[d].num_cells, hidden, generator=g).to(DEV) for d in range(3)]
        near.clear()
        plain.load_state_dict(state0)
        plain.zero_grad(set_to_none=True)
        out_p, xin_p = run(plain, False)
        if min(near) > 6e-6:       # the two paths' pre-activations agree to ~3e-6
            break
    else:
        pytest.skip('no kink-free input found')
    for h in hooks:
        h.remove()

    called = []
    from cwn_amd import dense_train as DT
    orig = DT.dense_train
    DT.dense_train = lambda *a, **k: (called.append(1), orig(*a, **k))[1]
    try:
        out_f, xin_f = run(fused, True)
    finally:
        DT.dense_train = orig
    assert called, 'the fused training path was not taken'
    for of, op in zip(out_f, out_p):
        torch.testing.assert_close(of, op, rtol=1e-4, atol=2e-5)
    for xf, xp in zip(xin_f, xin_p):
        s = max(1.0, float(xp.grad.abs().max()))
        torch.testing.assert_close(xf.grad, xp.grad, rtol=1e-4, atol=3e-5 * s)
    pf, pp = dict(fused.named_parameters()), dict(plain.named_parameters())
    for name, p in pp.items():
        if p.grad is None:
            assert pf[name].grad is None or float(pf[name].grad.abs().max()) == 0.0, name
            continue
        s = _grad_scale(name, p.grad)
        torch.testing.assert_close(pf[name].grad, p.grad, rtol=1e-4, atol=5e-5 * s, msg=lambda m, n=name: f'{n}: {m}')
    bf, bp = dict(fused.named_buffers()), dict(plain.named_buffers())
    for name, t in bp.items():
        if t.dtype.is_floating_point:
            torch.testing.assert_close(bf[name], t, rtol=1e-5, atol=1e-6, msg=lambda m, n=name: f'{n}: {m}')
        else:
            assert torch.equal(bf[name], t), name


@pytest.mark.parametrize('hidden', [128, 64])
def test_live_batchnorm_matches_the_finalize_launches(hidden):
    """cwn_bn_live / cwn_bn_bwd_live (round 4): the stage launches sum the statistics (forward) and the reduce half of the
    BatchNorm backward into slots and the consuming launches take them in their prologue -- no cwn_bn_finalize_f32 launch, a
    cwn_norm_bwd_reduce_f32 launch for the combine stages only -- against the same layer with CWN_LIVE_BN off (per-band partials + finalize): outputs,
    input gradients, parameter gradients, running statistics and batch counters, inside a step arena and outside one; a
    batch with an empty dimension (no 2-cells) included."""
    from cwn_amd import _ffi, dense_train as DT, layers, ops
    from cwn_amd.synthetic import zinc_like_batch
    fused, _ = _train_layer_pair(torch.nn.BatchNorm1d, hidden, True)
    state0 = {k: v.clone() for k, v in fused.state_dict().items()}
    calls, reduced = [], []
    orig, orig_red = _ffi.bn_finalize, _ffi.norm_bwd_reduce
    _ffi.bn_finalize = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    _ffi.norm_bwd_reduce = lambda descs, *a, **k: (reduced.append(len(descs)), orig_red(descs, *a, **k))[1]

    def run(b, live, arena):
        fused.load_state_dict(state0)
        fused.zero_grad(set_to_none=True)
        ops.weights_changed()
        # (the model's forward packs the blocks of every update / combine Linear for cwn_dense_stage_f32: models.py)
        ops.pack_stage_weights_many([lin.weight for lvl in fused.mp_levels
                                     for net in (lvl.update_up_nn, lvl.update_boundaries_nn, lvl.combine_nn)
                                     for lin, _ in layers._mlp_stages(net)])
        DT.LIVE_BN = DT.LIVE_BN_BWD = live
        g = torch.Generator().manual_seed(3)
        xin = [(torch.randn(b.cochains[d].num_cells, hidden, generator=g).to(DEV)).requires_grad_() for d in range(3)]
        ws = [torch.randn(b.cochains[d].num_cells, hidden, generator=g).to(DEV) for d in range(3)]
        b.set_xs(xin)
        params = b.get_all_cochain_params(max_dim=2, include_down_features=False)
        ctx = ops.step_arena(DEV) if arena else contextlib.nullcontext()
        with ctx:
            out = fused(*params)
            sum((o * w).sum() for o, w in zip(out, ws)).backward()
        torch.cuda.synchronize()
        return ([o.detach().clone() for o in out], [x.grad.clone() for x in xin],
                {n: p.grad.clone() for n, p in fused.named_parameters() if p.grad is not None},
                {n: t.clone() for n, t in fused.named_buffers()})

    import contextlib
    try:
        for b in (zinc_like_batch(24, seed=5, device=DEV), zinc_like_batch(3, seed=8, device=DEV)):
            calls.clear()
            reduced.clear()
            ref = run(b, False, False)
            assert calls, 'the finalize form did not launch cwn_bn_finalize_f32'
            assert sum(reduced) == 15, reduced          # every BatchNorm of the layer: 5 per dimension
            for arena in (False, True, True):           # (twice inside the arena: the second step starts from its fill)
                calls.clear()
                reduced.clear()
                got = run(b, True, arena)
                assert not calls, 'live BatchNorm still launched cwn_bn_finalize_f32'
                assert sum(reduced) == 3, reduced       # the combine stages only (their dy comes from autograd)
                for a, r in zip(got[0] + got[1], ref[0] + ref[1]):
                    torch.testing.assert_close(a, r, rtol=2e-5, atol=2e-5 * max(1.0, float(r.abs().max())))
                assert got[2].keys() == ref[2].keys()
                for n in ref[2]:
                    torch.testing.assert_close(got[2][n], ref[2][n], rtol=1e-4, atol=5e-5 * _grad_scale(n, ref[2][n]), msg=n)
                for n, t in ref[3].items():
                    if t.dtype.is_floating_point:
                        torch.testing.assert_close(got[3][n], t, rtol=1e-6, atol=1e-7, msg=n)
                    else:
                        assert torch.equal(got[3][n], t), n
    finally:
        _ffi.bn_finalize, _ffi.norm_bwd_reduce = orig, orig_red
        DT.LIVE_BN = DT.LIVE_BN_BWD = True


def test_training_accumulates_into_existing_grads():
    """With .grad buffers allocated (FlatGradBucket), the weight-gradient kernels add into them
    directly; two backward passes must equal twice one pass, and must match autograd's own
    accumulation (ACCUMULATE_INTO_GRAD off)."""
    from cwn_amd import layers, ops
    from cwn_amd.dist import FlatGradBucket
    from cwn_amd.synthetic import zinc_like_batch
    fused, other = _train_layer_pair(torch.nn.BatchNorm1d, 64, True, seed=3)
    b = zinc_like_batch(8, seed=2, device=DEV)
    g = torch.Generator().manual_seed(0)
    xs = [torch.randn(b.cochains[d].num_cells, 64, generator=g).to(DEV) for d in range(3)]
    ws = [torch.randn(b.cochains[d].num_cells, 64, generator=g).to(DEV) for d in range(3)]

    def backward_once(conv):
        b.set_xs([x.clone() for x in xs])
        params = b.get_all_cochain_params(max_dim=2, include_down_features=False)
        sum((o * w).sum() for o, w in zip(conv(*params), ws)).backward()

    bucket = FlatGradBucket(fused.parameters())
    state = {k: v.clone() for k, v in fused.state_dict().items()}
    # (the weight-gradient launches of a block run when it ENDS -- _ffi.flush_tn: the buffers are complete behind it)
    with ops.accumulate_into_grad():
        backward_once(fused)
    once = bucket.flat.clone()
    assert float(once.abs().max()) > 0
    fused.load_state_dict(state)          # same running statistics / parameters for the second pass
    with ops.accumulate_into_grad():
        backward_once(fused)
    torch.testing.assert_close(bucket.flat, 2 * once, rtol=1e-5, atol=1e-5 * float(once.abs().max()))
    # autograd's own accumulation (the default: grad hooks fire, torch.autograd.grad works)
    assert not ops.ACCUMULATE_INTO_GRAD
    bucket2 = FlatGradBucket(other.parameters())
    backward_once(other)
    torch.testing.assert_close(bucket2.flat, once, rtol=1e-4, atol=2e-5 * float(once.abs().max()))


# ------------------------------------------------------------------------------------------------
# the whole optimisation step (cwn_amd/train.py)
# ------------------------------------------------------------------------------------------------
def _train_setup(seed=0, hidden=32, nb=2):
    from cwn_amd.models import EmbedSparseCIN
    from cwn_amd.synthetic import zinc_like_batch
    torch.manual_seed(seed)
    model = EmbedSparseCIN(28, 4, 1, 2, hidden, dropout_rate=0.0, embed_edge=True, use_coboundaries=True).to(DEV)
    batches = [zinc_like_batch(16, seed=10 + i, device=DEV) for i in range(nb)]
    return model, batches


def test_train_step_graph_replay_matches_eager():
    """Three optimisation steps replayed from hipGraphs leave the model where three eager steps
    leave it (same kernels, same order; fp32 atomics in the weight gradients allow ~1e-6)."""
    from cwn_amd.train import TrainStep
    m1, b1 = _train_setup()
    m2, b2 = _train_setup()
    m2.load_state_dict(m1.state_dict())
    eager = TrainStep(m1, b1, use_graph=False)
    graph = TrainStep(m2, b2, use_graph=True)
    for i in range(3):
        le = eager.step(i % 2)
        lg = graph.step(i % 2)
        torch.testing.assert_close(lg, le, rtol=2e-3, atol=1e-4)
    torch.cuda.synchronize()
    worst = 0.0
    for (n, p), (_, q) in zip(m1.state_dict().items(), m2.state_dict().items()):
        if p.dtype.is_floating_point:
            worst = max(worst, float((p - q).abs().max()) / max(1.0, float(p.abs().max())))
    # Adam's first steps move every weight by ~lr = 1e-3 whatever the size of its gradient: an element whose
    # gradient is at the level of the fp32-atomic summation noise can take opposite signs in the two runs,
    # every step -- 2 * lr * steps is the bound that follows, not a tolerance on the kernels (5e-3 failed
    # once in ~15 runs)
    print(f'[train] graph replay vs eager after 3 steps: worst relative parameter distance {worst:.3e}')
    assert worst < 2 * 1e-3 * 3 * 1.1, worst


def test_train_step_learns_and_keeps_grads_in_the_bucket():
    from cwn_amd.train import TrainStep
    model, batches = _train_setup(seed=1)
    ts = TrainStep(model, batches, lr=3e-3, use_graph=True)
    first = [float(ts.step(i)) for i in range(2)]
    for i in range(60):
        ts.step(i % 2)
    last = [float(ts.step(i)) for i in range(2)]
    assert sum(last) < 0.7 * sum(first), (first, last)
    # every gradient is a view into the one flat buffer (what the DP all-reduce sends)
    lo, hi = ts.bucket.flat.data_ptr(), ts.bucket.flat.data_ptr() + 4 * ts.bucket.flat.numel()
    for p in model.parameters():
        assert p.grad is not None and lo <= p.grad.data_ptr() < hi
    assert torch.isfinite(ts.bucket.flat).all()


def test_model_training_forward_backward_matches_torch_modules():
    """Whole EmbedSparseCIN in train mode: fused dense path on vs off, loss and flat gradient."""
    from cwn_amd import layers
    from cwn_amd.dist import FlatGradBucket
    m1, b = _train_setup(seed=2, hidden=32, nb=1)
    m2, _ = _train_setup(seed=2, hidden=32, nb=1)
    m2.load_state_dict(m1.state_dict())
    b = b[0]
    x0 = [None if b.cochains[d].x is None else b.cochains[d].x.clone() for d in range(3)]

    def run(model, fused_on):
        layers.FUSED_DENSE_TRAINING = fused_on
        try:
            for d in range(3):
                b.cochains[d]._x = x0[d]
            model.train()
            bucket = FlatGradBucket(model.parameters())
            loss = (model(b) - b.y.view(-1, 1)).abs().mean()
            loss.backward()
            for d in range(3):
                b.cochains[d]._x = x0[d]
            return float(loss.detach()), bucket.flat.clone()
        finally:
            layers.FUSED_DENSE_TRAINING = True

    l1, g1 = run(m1, True)
    l2, g2 = run(m2, False)
    assert abs(l1 - l2) < 1e-5 * max(1.0, abs(l2))
    # relative L2 distance of the whole gradient: robust to an isolated ReLU-kink tie
    rel = float((g1 - g2).norm() / g2.norm())
    assert rel < 2e-3, rel


def test_model_training_gradients_match_float64_oracle_autograd():
    """An independent pin of the fused training path (BatchNorm statistics in the GEMM epilogue, MFMA weight
    gradients, aggregation backward, embedding backward): every parameter gradient of a train-mode
    EmbedSparseCIN step against torch autograd run over the ORACLE's forward in float64 on the CPU --
    not against torch modules on the same GPU."""
    model, bs = _train_setup(seed=6, hidden=32, nb=1)
    b = bs[0]
    model.train()
    state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    ocx = _oracle_cx(b)
    leaves = {k: v.double().requires_grad_(True) for k, v in state.items() if v.is_floating_point() and 'running' not in k}
    ostate = dict(to_double(state))
    ostate.update(leaves)
    ref_out, _ = O.sparse_cin_model_forward(ostate, ocx, 2, use_coboundaries=True, training=True, norm='bn', embed='zinc')
    y = cpu(b.y).double().view(-1, 1)
    ref_loss = (ref_out - y).abs().mean()
    ref_loss.backward()
    x0 = [None if b.cochains[d].x is None else b.cochains[d].x.clone() for d in range(3)]
    loss = (model(b) - b.y.view(-1, 1)).abs().mean()
    loss.backward()
    for d in range(3):
        b.cochains[d]._x = x0[d]
    gate(loss.detach().view(1), ref_loss.detach().view(1), 'train-mode loss vs float64 oracle')
    worst = 0.0
    for name, p in model.named_parameters():
        r = leaves[name].grad
        if r is None:            # a parameter the loss does not reach (e.g. an unused embedding row table)
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        assert p.grad is not None, name
        worst = max(worst, gate(p.grad, r, f'grad {name}', tol=2e-5))
    print(f'[gate] training gradients vs float64 oracle autograd: worst max|delta| = {worst:.3e}')


def test_train_step_two_graph_form_used_under_data_parallelism():
    """World size > 1 splits the step into graph(forward + backward) -> all-reduce -> graph(Adam).
    Exercised here on one GPU by forcing the form (the collective is a no-op without a process
    group); the result must equal the single-graph step."""
    from cwn_amd.train import TrainStep
    m1, b1 = _train_setup(seed=4)
    m2, b2 = _train_setup(seed=4)
    m2.load_state_dict(m1.state_dict())
    one = TrainStep(m1, b1, use_graph=True)
    two = TrainStep(m2, b2, use_graph=True)
    two.world = 2
    for i in range(4):
        la, lb = one.step(i % 2), two.step(i % 2)
        torch.testing.assert_close(lb, la, rtol=2e-3, atol=1e-4)
    assert two._graphs[0][1] is not None and one._graphs[0][1] is None


def test_train_step_staged_backward_matches_the_monolithic_step():
    """Data parallelism cuts the backward behind the message-passing layers (one hipGraph per piece, the
    all-reduce of a piece's gradients issued while the next piece runs).  On one GPU the collectives are no-ops,
    so the staged step must equal the single-graph step: stages read off the autograd graph, every chunk of the
    gradient bucket untouched until its piece has run, gradients equal up to the fp32-atomic summation noise."""
    from cwn_amd.models import EmbedSparseCIN
    from cwn_amd.synthetic import zinc_like_batch
    from cwn_amd.train import TrainStep

    def setup():
        torch.manual_seed(5)
        m = EmbedSparseCIN(28, 4, 1, 4, 32, dropout_rate=0.0, embed_edge=True, use_coboundaries=True).to(DEV)
        return m, [zinc_like_batch(16, seed=30 + i, device=DEV) for i in range(2)]
    m1, b1 = setup()
    m2, b2 = setup()
    m2.load_state_dict(m1.state_dict())
    one = TrainStep(m1, b1, use_graph=True)
    cut = TrainStep(m2, b2, use_graph=True, stages=4)
    assert one.n_stages == 1 and cut.n_stages == 4 and len(cut.bucket.chunks) == 4
    names = {id(p): n for n, p in m2.named_parameters()}
    for j, ps in enumerate(cut.stage_params):
        got = {names[id(p)].split('.')[0] + '.' + names[id(p)].split('.')[1] for p in ps if names[id(p)].startswith('convs')}
        # a layer's parameters ride with the layer, reached or not (the reference constructs unused networks too:
        # lower-adjacency messages, the top dimension's coboundary message)
        assert got == {f'convs.{3 - j}'}, (j, got)
    assert any(names[id(p)].startswith('lin2') for p in cut.stage_params[0])
    assert any('embed' in names[id(p)] for p in cut.stage_params[3])
    # buffers untouched by the probe forward
    for (n, a), (_, b) in zip(m1.named_buffers(), m2.named_buffers()):
        assert torch.equal(a, b), n
    # eager pieces: a chunk is written by its own piece only
    for j in range(4):
        cut._forward_backward(0, [j])
        assert cut.bucket.chunk(j).any()
        assert not any(cut.bucket.chunk(c).any() for c in range(j + 1, 4)), j
    one._forward_backward(0)
    # whole-gradient distances: a bias in front of a BatchNorm has a true gradient of zero and a computed one of
    # summation noise, so per-parameter ratios mean nothing
    ga = torch.cat([p.grad.flatten() for p in m1.parameters()])
    gb = torch.cat([q.grad.flatten() for q in m2.parameters()])
    rel, top = float((ga - gb).norm() / ga.norm()), float((ga - gb).abs().max() / ga.abs().max())
    print(f'[train] staged vs monolithic backward: relative L2 distance {rel:.3e}, max|delta| / max|g| {top:.3e}')
    assert rel < 1e-5 and top < 1e-5, (rel, top)
    for (n, a), (_, b) in zip(m1.named_buffers(), m2.named_buffers()):
        a.copy_(b)
    for i in range(4):
        la, lb = one.step(i % 2), cut.step(i % 2)
        torch.testing.assert_close(lb, la, rtol=2e-3, atol=1e-4)
    torch.cuda.synchronize()
    pieces, g2, _ = cut._graphs[0]
    assert len(pieces) == 4 and g2 is not None
    worst = 0.0
    for (n, p), (_, q) in zip(m1.state_dict().items(), m2.state_dict().items()):
        if p.dtype.is_floating_point:
            worst = max(worst, float((p - q).abs().max()) / max(1.0, float(p.abs().max())))
    print(f'[train] staged graphs vs single graph after 4 steps: worst relative parameter distance {worst:.3e}')
    assert worst < 2 * 1e-3 * 4 * 1.1, worst     # the Adam sign-flip bound of test_train_step_graph_replay_matches_eager
    # a network with jumping knowledge cannot be cut: one stage, same result as ever
    torch.manual_seed(5)
    mj = EmbedSparseCIN(28, 4, 1, 3, 32, dropout_rate=0.0, embed_edge=True, use_coboundaries=True, jump_mode='cat').to(DEV)
    tj = TrainStep(mj, b1, use_graph=False, stages=3)
    assert tj.n_stages == 1 and tj.staged is None
    assert torch.isfinite(tj.step(0))


def test_two_rank_train_step_reduces_inside_the_backward():
    """Two ranks sharing this box's GPU over gloo (tools/train_2rank_check.py compare): the staged step --
    backward in pieces, each piece's gradients all-reduced while the next one runs -- leaves both ranks with the
    same model as the step with one all-reduce behind the backward, replayed from hipGraphs and eagerly."""
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, LAYERS='3')
    env.pop('CWN_TRAIN_STAGES', None)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
           '--master-addr', '127.0.0.1', '--master-port', str(port),
           os.path.join(root, 'tools', 'train_2rank_check.py'), 'compare']
    out = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        print(out.stdout[-3000:], out.stderr[-6000:])
    assert out.returncode == 0, [l for l in out.stderr.splitlines() if 'Error' in l or 'error' in l][-5:]
    # (two processes print to one pipe: their lines can arrive glued together)
    assert out.stdout.count('compare OK rank') == 2, out.stdout[-2000:]
    print('[train] ' + ' | '.join(l for l in out.stdout.splitlines() if 'compare OK' in l))


def test_eval_after_training_sees_the_trained_weights():
    """Packed weights, folded BatchNorm and prepared launches are cached per tensor version -- but the training
    kernels (cwn_adam_f32, the BatchNorm-statistics epilogue) write through raw pointers, and a replayed hipGraph
    runs no Python at all.  eval -> train (graph replays) -> eval must equal a freshly built model holding the
    trained state (mp/molec_models.py:90-160 evaluated after exp/train_utils.py:57-75)."""
    from cwn_amd.models import EmbedSparseCIN
    from cwn_amd.synthetic import zinc_like_batch
    from cwn_amd.train import TrainStep

    def build():
        return EmbedSparseCIN(28, 4, 1, 2, 64, dropout_rate=0.0, embed_edge=True, use_coboundaries=True).to(DEV)
    torch.manual_seed(8)
    model = build()
    fresh_batch = lambda: zinc_like_batch(16, seed=77, device=DEV)
    with torch.no_grad():
        y0 = model.eval()(fresh_batch())                  # fills every cache with the initial state
    for use_graph in (True, False):
        ts = TrainStep(model, [zinc_like_batch(16, seed=78, device=DEV)], lr=1e-2, use_graph=use_graph)
        for _ in range(3):
            ts.step(0)
        with torch.no_grad():
            y1 = model.eval()(fresh_batch())
            ref = build()
            ref.load_state_dict(model.state_dict())
            y2 = ref.eval()(fresh_batch())
        assert torch.equal(y1, y2), (use_graph, float((y1 - y2).abs().max()))
        assert float((y1 - y0).abs().max()) > 1e-3       # and the training did move the output
        y0 = y1


def test_several_steps_behind_one_replay_take_the_same_steps():
    """TrainStep.steps(seq): one captured graph for a sequence of batches -- the trained state equals the one the same
    steps reach one replay at a time (weight gradients use fp32 atomics: equal up to their summation order) and the
    losses come back per step."""
    from cwn_amd.models import EmbedSparseCIN
    from cwn_amd.synthetic import zinc_like_batch
    from cwn_amd.train import TrainStep

    def run(many):
        torch.manual_seed(4)
        model = EmbedSparseCIN(28, 4, 1, 2, 64, dropout_rate=0.0, embed_edge=True, use_coboundaries=True).to(DEV)
        ts = TrainStep(model, [zinc_like_batch(12, seed=90 + i, device=DEV) for i in range(3)], lr=1e-3, use_graph=True)
        seq = [0, 1, 2, 1]
        losses = []
        for _ in range(1):          # (one round: the weight gradients' fp32 atomics make later steps drift apart by design)
            if many:
                losses += [float(l) for l in ts.steps(seq)]
            else:
                for i in seq:
                    losses.append(float(ts.step(i)))
        with torch.no_grad():
            y = model.eval()(zinc_like_batch(9, seed=5, device=DEV))
        return losses, {k: v.detach().clone() for k, v in model.state_dict().items()}, y

    la, sa, ya = run(True)
    lb, sb, yb = run(False)
    assert len(la) == len(lb) == 4
    for a, b in zip(la, lb):
        assert abs(a - b) <= 1e-3 * max(1.0, abs(b)), (la, lb)
    # (parameter by parameter the two runs may differ by 2 lr after any step: a Linear bias in front of a BatchNorm has a
    # zero gradient up to rounding, and Adam normalises that noise to full-size steps -- which the network's output does
    # not see, nor do the normalised activations, while running_mean follows the bias; compared are the integer state and
    # the per-step training losses, which agree to 1e-3: observed 1e-6 ... 1e-4, growing with the step)
    for k in sb:
        if not sb[k].dtype.is_floating_point:
            assert torch.equal(sa[k], sb[k]), k
    assert torch.isfinite(ya).all() and torch.isfinite(yb).all()


def test_flat_adam_matches_torch_adam():
    from cwn_amd.dist import FlatGradBucket
    from cwn_amd.train import FlatAdam
    torch.manual_seed(0)
    shapes = [(128, 256), (128,), (7, 3), (1,), (64, 64)]
    pa = [torch.nn.Parameter(torch.randn(*s, device=DEV)) for s in shapes]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    ref = torch.optim.Adam(pb, lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.01)
    bucket = FlatGradBucket(pa)
    opt = FlatAdam(bucket, lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.01)
    g = torch.Generator().manual_seed(1)
    for it in range(5):
        grads = [torch.randn(*s, generator=g).to(DEV) * (10.0 ** (it - 2)) for s in shapes]
        for p, q, gr in zip(pa, pb, grads):
            p.grad.copy_(gr)
            q.grad = gr.clone()
        opt.step()
        ref.step()
        for p, q in zip(pa, pb):
            torch.testing.assert_close(p.data, q.data, rtol=2e-5, atol=2e-6)
    # parameters are views of one buffer, modules see the updates
    lo, hi = opt.flat_p.data_ptr(), opt.flat_p.data_ptr() + 4 * opt.flat_p.numel()
    assert all(lo <= p.data_ptr() < hi for p in pa)


@pytest.mark.parametrize('F', [1, 2, 3, 4, 8, 16])
@pytest.mark.parametrize('op', ['id', 'plus'])
def test_narrow_feature_medium_rows_entry_parallel(F, op):
    """Narrow features: rows with 17..64 entries are folded by several lanes (entry slots) and
    combined by a fixed tree -- equal to the sequential sum up to fp32 re-association, exact on
    integers, deterministic; rows up to 16 entries stay bit-identical to index_add_."""
    from cwn_amd import ops
    from cwn_amd.csr import Adjacency
    g = torch.Generator().manual_seed(F * 3 + len(op))
    n_dst, n_src, n_aux = 400, 300, 50
    deg = torch.randint(0, 65, (n_dst,), generator=g)
    deg[::7] = torch.randint(0, 17, (deg[::7].numel(),), generator=g)       # some short rows
    dst = torch.repeat_interleave(torch.arange(n_dst), deg)
    dst = dst[torch.randperm(dst.numel(), generator=g)]
    src = torch.randint(0, n_src, (dst.numel(),), generator=g)
    aux = torch.randint(0, n_aux, (dst.numel(),), generator=g)
    idx = torch.stack([src, dst])
    x = torch.randn(n_src, F, generator=g)
    ua = torch.randn(n_aux, F, generator=g)
    adj = Adjacency.from_index(idx.to(DEV), n_dst, n_src, aux.to(DEV), n_aux)
    kw = {} if op == 'id' else dict(msg_op=ops.MSG_A_PLUS_B, B=ua.to(DEV))
    got = ops.aggregate(adj, n_dst, x.to(DEV), **kw)
    msg = x[src] if op == 'id' else x[src] + ua[aux]
    ref64 = torch.zeros(n_dst, F, dtype=torch.float64).index_add_(0, dst, msg.double())
    torch.testing.assert_close(cpu(got).double(), ref64, rtol=1e-5, atol=1e-5)
    seq = torch.zeros(n_dst, F).index_add_(0, dst, msg)
    short = deg <= 16
    assert torch.equal(cpu(got)[short], seq[short])              # sequential order kept
    assert torch.equal(got, ops.aggregate(adj, n_dst, x.to(DEV), **kw))   # deterministic
    xi = torch.randint(-5, 6, (n_src, F), generator=g).float()
    goti = ops.aggregate(adj, n_dst, xi.to(DEV))
    assert torch.equal(cpu(goti), torch.zeros(n_dst, F).index_add_(0, dst, xi[src]))
    for red in ('mean', 'max'):
        gr = ops.aggregate(adj, n_dst, xi.to(DEV), reduce=red)
        assert torch.equal(cpu(gr), O.scatter_rows(xi[src], dst, n_dst, red)) or red == 'mean'
        torch.testing.assert_close(cpu(gr), O.scatter_rows(xi[src], dst, n_dst, red), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize('dims,N,H', [((28,), 3165, 64), ((4,), 3165, 64), ((119, 5, 12, 12, 10, 6, 6, 2, 2), 3165, 64),
                                      ((5, 6, 2), 3165, 64), ((28,), 3341, 128), ((4,), 70, 128), ((60,), 1000, 256),
                                      ((70,), 500, 128), ((28,), 333, 96)])
def test_embedding_sum_matches_torch_embedding(dims, N, H):
    """Forward bit-identical to the sum of torch.nn.Embedding outputs (same order); backward equal
    to embedding_backward up to fp32 re-association of the very long table rows (one small table at width 64 / 128 / 256:
    the ballot kernel; everything else: the table-in-LDS kernel)."""
    from cwn_amd import ops
    g = torch.Generator().manual_seed(sum(dims) + N + H)
    tables = [torch.randn(d, H, generator=g).to(DEV).requires_grad_() for d in dims]
    ref_tables = [t.detach().clone().requires_grad_() for t in tables]
    idx = torch.stack([torch.randint(0, d, (N,), generator=g) for d in dims], 1).to(DEV)
    out = ops.embedding_sum(tables, idx if len(dims) > 1 else idx[:, 0])
    ref = sum(torch.nn.functional.embedding(idx[:, c], ref_tables[c]) for c in range(len(dims)))
    assert torch.equal(out, ref)
    w = torch.randn(N, H, generator=g).to(DEV)
    (out * w).sum().backward()
    (ref * w).sum().backward()
    for t, r in zip(tables, ref_tables):
        torch.testing.assert_close(t.grad, r.grad, rtol=1e-4, atol=1e-4 * max(1.0, float(r.grad.abs().max())))
    with pytest.raises(IndexError):
        bad = idx.clone()
        bad[3, 0] = dims[0]
        ops.embedding_sum(tables, bad if len(dims) > 1 else bad[:, 0])


def test_randomised_kernel_cross_check():
    """tools/fuzz_kernels.py: random shapes / degree distributions / option combinations of the
    aggregation (forward + backward), GEMM and weight-gradient GEMM kernels vs float64 torch."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'tools', 'fuzz_kernels.py'), '30', '11'],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize('with_bn', [True, False])
def test_cin_conv_fused_inference_matches_generic_path(with_bn):
    """CINConv (mp/layers.py:62-124) with the message networks of mp/models.py:40-47
    (Linear -> ReLU -> BatchNorm): the fused inference path (per-cell GEMMs + one aggregation + the
    degree-weighted BatchNorm shift) against the generic gather -> network -> scatter path."""
    from cwn_amd.layers import CINConv
    from cwn_amd.synthetic import zinc_like_batch
    torch.manual_seed(0)
    F = 64
    def net():
        mods = [torch.nn.Linear(2 * F, F), torch.nn.ReLU()]
        if with_bn:
            bn = torch.nn.BatchNorm1d(F)
            with torch.no_grad():
                bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 2.0)
                bn.weight.uniform_(0.5, 1.5); bn.bias.normal_()
            mods.append(bn)
        return torch.nn.Sequential(*mods)
    upd = torch.nn.Sequential(torch.nn.Linear(F, F), torch.nn.ReLU(), torch.nn.Linear(F, F), torch.nn.ReLU(),
                              torch.nn.BatchNorm1d(F))
    conv = CINConv(F, F, net(), net(), upd, eps=0.1, train_eps=False, max_dim=2).to(DEV).eval()
    b = zinc_like_batch(32, seed=3, device=DEV, include_down_adj=True)
    g = torch.Generator().manual_seed(2)
    xs = [torch.randn(b.cochains[d].num_cells, F, generator=g).to(DEV) for d in range(3)]
    b.set_xs(xs)
    params = b.get_all_cochain_params(max_dim=2, include_down_features=True)
    called = []
    lvl = conv.mp_levels[1]
    orig = type(lvl)._fused_finish
    type(lvl)._fused_finish = lambda self, p, o: (called.append(1), orig(self, p, o))[1]
    try:
        with torch.no_grad():
            fused = conv(*params)
            single = conv.mp_levels[1].forward(params[1])        # the per-dimension entry point
    finally:
        type(lvl)._fused_finish = orig
    assert len(called) == 4
    torch.testing.assert_close(single, fused[1], rtol=1e-6, atol=1e-6)
    b.set_xs([x.clone().requires_grad_() for x in xs])           # gradients wanted -> generic path
    params = b.get_all_cochain_params(max_dim=2, include_down_features=True)
    generic = conv(*params)
    for d, (f, gnr) in enumerate(zip(fused, generic)):
        torch.testing.assert_close(f, gnr.detach(), rtol=1e-4, atol=1e-4, msg=lambda m, d=d: f'dim {d}: {m}')


# ------------------------------------------------------------------------------------------------
# BASELINE config 2 end to end at full size: 4-layer hidden-128 EmbedSparseCIN, batch 128, eval forward
# (the path bench.py times as secondary.full_forward) against the oracle evaluated in float64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', ['blocked+split', 'csr+split', 'csr+exact'])
def test_config2_eval_forward_full_size_vs_float64_oracle(path):
    """mp/molec_models.py:90-160 on a ZINC-like batch of 128: every layer output, the pooled vectors and
    the prediction, gate 1e-5 * max(1, |ref|_inf).  'blocked': the complex-blocked layer kernel;
    'csr': grouped GEMM + CSR aggregation; 'split' / 'exact': the dense arithmetic of the N = K = 128
    launches (three-way bf16 split on the matrix pipe, or fp32 MFMA)."""
    from cwn_amd import layers, ops
    from cwn_amd.complex import ComplexBatch
    from cwn_amd.models import EmbedSparseCIN
    from cwn_amd.synthetic import zinc_like_complexes
    torch.manual_seed(0)
    model = EmbedSparseCIN(28, 4, 1, 4, 128, dropout_rate=0.0, max_dim=2, jump_mode=None, nonlinearity='relu',
                           readout='sum', train_eps=False, final_hidden_multiplier=2, final_readout='sum',
                           init_reduce='sum', embed_edge=True, use_coboundaries=True, graph_norm='bn').eval()
    with torch.no_grad():       # running statistics of a trained model are not (0, 1): make BatchNorm do work
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.uniform_(-0.2, 0.2)
                m.running_var.uniform_(0.5, 1.5)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    b = ComplexBatch.from_complex_list(zinc_like_complexes(128, 0, 6), max_dim=2)
    ref, rpart = O.sparse_cin_model_forward(to_double(state), _oracle_cx(b), 4)
    model = model.to(DEV)
    prev_b, prev_e = layers.BLOCKED_LAYER, ops.set_gemm_exact(path.endswith('exact'))
    layers.BLOCKED_LAYER = path.startswith('blocked')
    try:
        with torch.no_grad():
            y, res = model(b.to(DEV), include_partial=True)
        assert (model.convs[0].blocked_reason is None) == path.startswith('blocked'), model.convs[0].blocked_reason
    finally:
        layers.BLOCKED_LAYER = prev_b
        ops.set_gemm_exact(prev_e)
    for k, v in rpart.items():
        gate(res[k], v, f'config 2 [{path}] {k}')
    gate(y, ref, f'config 2 [{path}] prediction')


def _fp32_own_deviation_check(tag, keys, prod, ref32s, ref64, slack=2.0):
    """The product's deviation from the float64 oracle against the fp32 references' OWN deviation from it (the
    reference-generated golden where there is one, and the oracle evaluated in fp32 on the CPU)."""
    from tests._product import deviation
    worst = 0.0
    for k in keys:
        e_prod = deviation(prod[k], ref64[k])
        e_ref = max(deviation(r[k], ref64[k]) for r in ref32s)
        scale = max(1.0, float(ref64[k].abs().max())) if ref64[k].numel() else 1.0
        floor = 2.0 ** -23 * scale               # one fp32 ulp of the largest value: nothing in fp32 can promise less
        print(f'[fp32-own] {tag} {k}: product {e_prod:.3e}  fp32 reference {e_ref:.3e}  (|ref|_inf {scale:.3g})')
        assert e_prod <= slack * max(e_ref, floor), (tag, k, e_prod, e_ref)
        worst = max(worst, e_prod / max(e_ref, floor))
    return worst


@pytest.mark.parametrize('mode', ['eval', 'train'])
def test_product_rounding_vs_the_fp32_references_own_h32_l4(mode):
    """the gate is 1e-5 * max(1, |ref|_inf); the deep cases sit at 1-2e-5 ABSOLUTE
    against the reference-generated fp32 golden.  That excess is fp32 depth, not the product: against the oracle
    evaluated in FLOAT64 the product deviates no more than twice what the reference's own fp32 outputs (the golden)
    and the fp32 oracle deviate -- every layer output, pooled vector and the prediction of the 4-layer model."""
    from cwn_amd.models import EmbedSparseCIN
    tag = 'h32_l4'
    g = load('embed_sparse_cin.npz')
    H, L = g[f'{tag}/meta'].tolist()
    names = list_names('mol')
    state = state_dict(g, f'{tag}/state')
    ocx = O.batch_complexes([o_complex(n) for n in names], max_dim=2)
    ocx['cochains'][0]['x'], ocx['cochains'][1]['x'], ocx['cochains'][2]['x'] = T(g[f'{tag}/v_types']), T(g[f'{tag}/e_types']), None
    outs = {}
    for name, st in (('f32', state), ('f64', to_double(state))):
        y, part = O.embed_sparse_cin_forward({k: v.clone() for k, v in st.items()}, ocx, L, training=(mode == 'train'))
        outs[name] = dict(part, out=y)
    golden = {k: T(g[f'{tag}/{mode}/{k}']) for k in outs['f64']}
    model = EmbedSparseCIN(28, 4, 1, L, H, dropout_rate=0.0, max_dim=2, jump_mode=None, nonlinearity='relu', readout='sum',
                           train_eps=False, final_hidden_multiplier=2, final_readout='sum', apply_dropout_before='lin2',
                           init_reduce='sum', embed_edge=True, use_coboundaries=True, graph_norm='bn')
    model.load_state_dict(state)
    model = model.to(DEV).train(mode == 'train')
    b = dummy_batch(names, max_dim=2)
    b.cochains[0].x, b.cochains[1].x = T(g[f'{tag}/v_types']), T(g[f'{tag}/e_types'])
    b.cochains[2]._x = None
    with torch.no_grad():
        y, res = model(b.to(DEV), include_partial=True)
    prod = dict(res, out=y)
    _fp32_own_deviation_check(f'{tag} {mode}', list(outs['f64']), prod, [golden, outs['f32']], outs['f64'])


def test_product_rounding_vs_the_fp32_oracles_own_reddit32():
    """The same statement at BASELINE config 5's full size (REDDIT-like, 32 complexes with hubs of degree >= 100,
    pooled sums of ~76 where round 2 observed 5e-4 absolute): product vs float64 <= 2 x (fp32 oracle vs float64)."""
    from cwn_amd.complex import ComplexBatch
    from cwn_amd.models import SparseCIN
    from cwn_amd.synthetic import reddit_like_complexes
    torch.manual_seed(0)
    model = SparseCIN(1, 2, 4, 64, dropout_rate=0.0, max_dim=2, jump_mode='cat', readout='sum', use_coboundaries=False,
                      graph_norm='id').eval()
    with torch.no_grad():
        for p_ in model.parameters():
            p_.mul_(0.3)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    b = ComplexBatch.from_complex_list(reddit_like_complexes(32, 0), max_dim=2)
    kw = dict(use_coboundaries=False, norm='id', jump_mode='cat', embed=None)
    outs = {}
    for name, st in (('f32', state), ('f64', to_double(state))):
        cx = _oracle_cx(b)
        if name == 'f64':
            for c in cx['cochains']:
                c['x'] = c['x'].double()
        y, part = O.sparse_cin_model_forward(st, cx, 4, **kw)
        outs[name] = dict(part, out=y)
    model = model.to(DEV)
    with torch.no_grad():
        y, res = model(b.to(DEV), include_partial=True)
    _fp32_own_deviation_check('REDDIT-32', list(outs['f64']), dict(res, out=y), [outs['f32']], outs['f64'])


def test_sparse_cin_backward_with_materialised_up_attr():
    """up_attr as a dense [E, F] tensor (Complex.lazy_attrs = False, or a reference-style
    CochainMessagePassingParams) runs the fused coboundary message with a per-ENTRY B operand; its
    backward must mask with THAT entry's pre-activation.  Gradients of x, up_attr and the message
    Linear against CPU autograd of the reference formulation, with and without prepare()."""
    from cwn_amd.complex import Complex
    from cwn_amd.layers import SparseCINConv
    from cwn_amd.synthetic import zinc_like_batch
    F = 16
    for prepared in (False, True):
        torch.manual_seed(0)
        conv = SparseCINConv(F, F, F, None, None, None, None, max_dim=2, hidden=F, act_module=torch.nn.ReLU,
                             layer_dim=F, use_coboundaries=True, graph_norm=torch.nn.Identity).train()
        state = {k: v.clone() for k, v in conv.state_dict().items()}
        b = zinc_like_batch(6, seed=4, max_ring=6)
        g = torch.Generator().manual_seed(1)
        xs = [torch.randn(b.cochains[d].num_cells, F, generator=g) for d in range(3)]
        # CPU reference: the oracle's layer with autograd
        ocx = {'dimension': 2, 'y': None, 'cochains': []}
        xs_ref = [x.clone().double().requires_grad_(True) for x in xs]
        for d in range(3):
            c = b.cochains[d]
            ocx['cochains'].append(dict({k: c[k] for k in ('upper_index', 'lower_index', 'shared_boundaries',
                                                           'shared_coboundaries', 'boundary_index', 'y', 'batch')},
                                        x=xs_ref[d]))
        pstate = {k: torch.nn.Parameter(v.double()) if v.is_floating_point() else v for k, v in state.items()}
        oouts = O.sparse_cin_conv(pstate, O.all_cochain_params(ocx, 2, include_down_features=False), True,
                                  training=True, norm='id')
        sum((o * (i + 1)).sum() for i, o in enumerate(oouts)).backward()
        # product: dense attributes
        prev = Complex.lazy_attrs
        Complex.lazy_attrs = False
        try:
            conv = conv.to(DEV)
            bd = zinc_like_batch(6, seed=4, max_ring=6, device=DEV)
            if prepared:
                bd.prepare(backward=True)
            xd = [x.clone().to(DEV).requires_grad_(True) for x in xs]
            bd.set_xs(xd)
            params = bd.get_all_cochain_params(max_dim=2, include_down_features=False)
            assert torch.is_tensor(params[0].kwargs['up_attr'])          # dense, one row per entry
            outs = conv(*params)
            sum((o * (i + 1)).sum() for i, o in enumerate(outs)).backward()
        finally:
            Complex.lazy_attrs = prev
        for d in range(3):
            gate(outs[d], oouts[d], f'dense up_attr (prepared={prepared}) out[{d}]')
            gate(xd[d].grad, xs_ref[d].grad, f'dense up_attr (prepared={prepared}) dL/dx[{d}]', tol=2e-5)
        for k, p_ in conv.named_parameters():
            if p_.grad is not None and pstate[k].grad is not None:
                gate(p_.grad, pstate[k].grad, f'dense up_attr (prepared={prepared}) dL/d{k}', tol=2e-5)


@pytest.mark.parametrize('ia_mode', ['col', 'perm'])
def test_reduce_max_backward_matches_cpu_autograd(ia_mode):
    """reduce='max' (mp/cell_mp.py:104-105 -> torch_scatter.scatter(reduce='max'), :439): forward
    against scatter_reduce_('amax'), backward against its CPU autograd on tie-free data, and the
    arg-max rule on ties (the FIRST entry that attains the maximum takes the gradient)."""
    from cwn_amd import ops
    from cwn_amd.csr import Adjacency
    g = torch.Generator().manual_seed(0)
    n_src, n_dst, E, F = 40, 25, 300, 12
    idx = torch.stack([torch.randint(0, n_src, (E,), generator=g), torch.randint(0, n_dst - 3, (E,), generator=g)])
    rows = E if ia_mode == 'perm' else n_src
    x = torch.randn(rows, F, generator=g)
    w = torch.randn(n_dst, F, generator=g)
    xr = x.clone().double().requires_grad_(True)
    msg = xr if ia_mode == 'perm' else xr[idx[0]]
    ref = torch.zeros(n_dst, F, dtype=torch.float64).scatter_reduce(0, idx[1].unsqueeze(1).expand(-1, F), msg,
                                                                    'amax', include_self=False)
    (ref * w.double()).sum().backward()
    adj = Adjacency.from_index(idx.to(DEV), n_dst, n_src)
    xd = x.clone().to(DEV).requires_grad_(True)
    out = ops.aggregate(adj, n_dst, xd, reduce='max', ia_mode=ia_mode)
    (out * w.to(DEV)).sum().backward()
    assert torch.equal(cpu(out).double(), ref.detach())
    gate(xd.grad, xr.grad, f'max backward ({ia_mode})')
    # ties: two entries of one row carry the same maximal value -> the first one gets the gradient
    idx2 = torch.tensor([[0, 1, 2], [0, 0, 0]])
    a = torch.tensor([[5.0], [5.0], [1.0]], device=DEV, requires_grad=True)
    adj2 = Adjacency.from_index(idx2.to(DEV), 1, 3)
    ops.aggregate(adj2, 1, a, reduce='max').sum().backward()
    assert cpu(a.grad).flatten().tolist() == [1.0, 0.0, 0.0]


# ------------------------------------------------------------------------------------------------
# the co-boundary stream and CIN++ with a real lower stream (engine extensions; the
# reference has neither -- mp/cell_mp.py:44 TODO, mp/layers.py:244-247 -- so PARITY IS UNPINNED:
# property tests only)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['house', 'bridged', 'molecular', 'filled_square'])
def test_coboundary_stream_exact_on_integers_and_adjoint_to_the_boundary_stream(name):
    from cwn_amd.cell_mp import CochainMessagePassing
    cx = dummy_complex(name, device=DEV)
    g = torch.Generator().manual_seed(3)
    F = 8
    for d in range(cx.dimension):
        c, up = cx.cochains[d], cx.cochains[d + 1]
        if up.boundary_index is None:
            continue
        n, n_up = c.num_cells, up.num_cells
        v = torch.randint(-4, 5, (n_up, F), generator=g).float().to(DEV)      # on the cofaces
        mp_ = CochainMessagePassing(F, F)
        out = mp_.propagate_coboundary(up.boundary_index, v, n)
        # direct restatement: every (boundary cell, coface) pair of boundary_index sends v[coface] to the cell
        bi = cpu(up.boundary_index)
        want = torch.zeros(n, F).index_add_(0, bi[0], cpu(v)[bi[1]])
        assert torch.equal(cpu(out), want), (name, d)
        # adjoint of the boundary stream of dimension d+1:  <cob(v), w> == <v, bnd(w)>
        w = torch.randint(-4, 5, (n, F), generator=g).float().to(DEV)         # on this dimension's cells
        _, _, bnd = mp_.propagate(None, None, up.boundary_index, x=v, boundary_attr=w)
        assert float((out * w).sum()) == float((v * bnd).sum())
        # differentiable: d/dv <cob(v), w> = bnd(w)
        vv = v.clone().requires_grad_(True)
        (mp_.propagate_coboundary(up.boundary_index, vv, n) * w).sum().backward()
        assert torch.equal(vv.grad, bnd)


def test_cinpp_with_a_real_lower_stream_and_coboundary_stream():
    """feed_down_attr=True: the lower stream equals the oracle's propagate with down_attr and the
    layer's own msg_down_nn; coboundary_stream=True: a fourth stream, zero on the top dimension,
    equal to the transposed boundary aggregation elsewhere; the default layer keeps the quirk."""
    from cwn_amd.layers import CINppConv
    torch.manual_seed(0)
    F = 8
    b = dummy_batch(list_names('mol'), max_dim=2, device=DEV)
    g = torch.Generator().manual_seed(4)
    for d in range(3):
        b.cochains[d].x = torch.randn(b.cochains[d].num_cells, F, generator=g).to(DEV)
    conv = CINppConv(F, F, F, None, None, None, None, None, None, max_dim=2, hidden=F, act_module=torch.nn.ReLU,
                     layer_dim=F, use_coboundaries=True, feed_down_attr=True, coboundary_stream=True).to(DEV).eval()
    assert conv.mp_levels[1].use_down_msg and conv.mp_levels[1].combine_nn[0].in_features == 4 * F
    params = b.get_all_cochain_params(max_dim=2, include_down_features=True)
    with torch.no_grad():
        outs = conv(*params)
        assert all(torch.isfinite(o).all() for o in outs)
        lvl, prm = conv.mp_levels[1], params[1]
        _, down, _ = lvl.propagate(prm.up_index, prm.down_index, prm.boundary_index, x=prm.x,
                                   up_attr=prm.kwargs['up_attr'], down_attr=prm.kwargs['down_attr'],
                                   boundary_attr=prm.kwargs['boundary_attr'])
    W, bias = cpu(lvl.msg_down_nn[1].weight).double(), cpu(lvl.msg_down_nn[1].bias).double()
    x = cpu(prm.x).double()
    down_attr = cpu(b.cochains[0].x).double()[cpu(b.cochains[1].shared_boundaries)]
    _, odown, _ = O.propagate(x, None, cpu(prm.down_index), None, down_attr=down_attr,
                              message_down=lambda xj, a: torch.relu(torch.cat([xj, a], -1) @ W.t() + bias),
                              up_msg_size=F, down_msg_size=F)
    assert down.abs().max() > 0
    gate(down, odown, 'CIN++ lower stream with down_attr vs the oracle propagate (float64)')
    # the fourth stream of dimension 0: sum over incident edges of the edge features
    with torch.no_grad():
        cob0 = conv.mp_levels[0].propagate_coboundary(params[0].coboundary_index, params[0].coboundary_attr,
                                                      params[0].x.size(0))
    bi = cpu(b.cochains[1].boundary_index)
    want = torch.zeros(b.cochains[0].num_cells, F, dtype=torch.float64).index_add_(0, bi[0], cpu(b.cochains[1].x).double()[bi[1]])
    gate(cob0, want, 'co-boundary stream of the vertices')
    assert params[2].coboundary_index is None        # nothing above the top dimension


@pytest.mark.parametrize('proper', [False, True])
@pytest.mark.parametrize('F', [8, 64])
def test_cinpp_fused_streams_match_the_hook_path(F, proper):
    """CINppConv's three streams (four with coboundary_stream) of ALL dimensions -- the coboundary and
    the lower message as ReLU(Y1[j] + Y2[shared cell]), the self terms (1 + eps1 / eps2 / eps3 / eps4) x folded in -- in
    one grouped GEMM + ONE aggregation launch, one autograd node in training, against the reference's own sequence
    (`forward_unfused`: propagate() + the message hooks, mp/layers.py:243-260): outputs, input and parameter gradients,
    running statistics, eval and training mode (training at width 64: the update networks of all streams through
    dense_train's stage launches, a plan without combine stages).  Width 64 on a batch that carries its per-complex tables is the case SparseCINConv's blocked
    two-stream kernel would otherwise claim."""
    from cwn_amd.complex import ComplexBatch
    from cwn_amd.layers import CINppConv
    from cwn_amd.synthetic import zinc_like_complexes
    torch.manual_seed(3)
    if proper:           # the reference's test complexes: they carry lower adjacencies and shared boundaries
        b = dummy_batch(list_names('mol') + list_names('mol'), max_dim=2, device=DEV)
    else:
        b = ComplexBatch.from_complex_list(zinc_like_complexes(12, 5, 6), max_dim=2).to(DEV)
    g = torch.Generator().manual_seed(1)
    conv = CINppConv(F, F, F, None, None, None, None, None, None, max_dim=2, hidden=F, act_module=torch.nn.ReLU,
                     layer_dim=F, use_coboundaries=True, train_eps=True, feed_down_attr=proper,
                     coboundary_stream=proper).to(DEV)
    with torch.no_grad():
        for k, lvl in enumerate(conv.mp_levels):             # distinct eps per stream: a mix-up shows
            for j, name in enumerate(('eps1', 'eps2', 'eps3') + (('eps4',) if proper else ())):
                getattr(lvl, name).fill_(0.1 * (j + 1) + 0.01 * k)
    xs = [torch.randn(b.cochains[d].num_cells, F, generator=g).to(DEV) for d in range(3)]
    ws = [torch.randn(b.cochains[d].num_cells, F, generator=g).to(DEV) for d in range(3)]

    def run(fused, train):
        conv.train(train)
        conv.zero_grad(set_to_none=True)
        for d in range(3):
            b.cochains[d].x = xs[d].clone().requires_grad_(True)
        params = b.get_all_cochain_params(max_dim=2, include_down_features=proper)
        outs = conv(*params) if fused else [conv.mp_levels[d].forward_unfused(params[d]) for d in range(3)]
        sum((o * w).sum() for o, w in zip(outs, ws)).backward()
        return ([o.detach() for o in outs], [b.cochains[d].x.grad for d in range(3)],
                {n: p.grad.clone() for n, p in conv.named_parameters() if p.grad is not None},
                {n: t.clone().float() for n, t in conv.named_buffers() if 'running' in n or 'num_batches' in n})

    def close(a, r, what, mult=1.0):
        tol = mult * 2e-5 * max(1.0, float(r.abs().max()))
        assert float((a - r).abs().max()) <= tol, (what, float((a - r).abs().max()), tol)

    for train in (False, True):
        if train:
            for m in conv.modules():                          # both runs start from the same running statistics
                if isinstance(m, torch.nn.BatchNorm1d):
                    m.reset_running_stats()
        o1, gx1, gp1, st1 = run(True, train)
        # (round 6: at widths 64 / 128 the default layer now takes the blocked launches -- tests/test_gpu_cinpp_blocked.py; here
        #  the fused STREAMS are what is compared with the hooks, whichever launch serves them)
        if train:
            for m in conv.modules():
                if isinstance(m, torch.nn.BatchNorm1d):
                    m.reset_running_stats()
        o0, gx0, gp0, st0 = run(False, train)
        for n in st0:                                         # running statistics and batch counters (training: one update each)
            close(st1[n], st0[n], f'buffer {n} train={train}')
        for d in range(3):
            close(o1[d], o0[d], f'output dim {d} train={train}')
            close(gx1[d], gx0[d], f'input gradient dim {d} train={train}')
        assert set(gp1) == set(gp0)
        for n in gp0:
            close(gp1[n], gp0[n], f'gradient of {n} train={train}', mult=2.5 * _grad_scale(n, gp0[n]) / max(1.0, float(gp0[n].abs().max())))
    # inference (no autograd): the update networks as grouped launches with the eval-mode BatchNorm folded in
    conv.eval()
    for d in range(3):
        b.cochains[d].x = xs[d]
    params = b.get_all_cochain_params(max_dim=2, include_down_features=proper)
    taken, orig = [], conv._dense_eval
    conv._dense_eval = lambda *a, **k: (taken.append(orig(*a, **k)) or taken[-1])
    with torch.no_grad():
        got = conv(*params)
        want = [conv.mp_levels[d].forward_unfused(params[d]) for d in range(3)]
    conv._dense_eval = orig
    assert taken and taken[0] is not None, 'the grouped inference path of the update networks was not taken'
    for d in range(3):
        close(got[d], want[d], f'inference output dim {d}')
    # the lower stream of the proper form is live; the quirk's is the self term alone
    lvl = conv.mp_levels[1]
    params = b.get_all_cochain_params(max_dim=2, include_down_features=proper)
    with torch.no_grad():
        sts = lvl.streams(params[1])
    assert sts is not None and len(sts) == (4 if proper else 3)
    assert (sts[1].adj is not None) == proper


@pytest.mark.parametrize('world,with_train', [(2, False), (8, True)])
def test_bench_multi_rank_control_flow_on_one_gpu(tmp_path, world, with_train):
    """bench.py launched the way the driver launches it for N > 1 (torch.distributed.run, one process per
    rank), with all ranks sharing this box's single GPU over gloo (CWN_BENCH_SHARE_GPU=1): barriers,
    the max-over-ranks time, the all-reduced cell count and the rank-0-only legs all run.  At world 8 (the node the
    scaling run uses: VERDICT r2 item 6) the data-parallel training leg runs too -- eight shards, one flat gradient
    bucket, the weighted-mean all-reduce inside the backward -- so that a first real 8-GPU run has RCCL itself as its
    only unknown."""
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    import tempfile
    detail = os.path.join(tempfile.mkdtemp(prefix='cwn_bench_'), 'detail.json')     # (the stdout line is the slim one)
    env = dict(os.environ, CWN_BENCH_SHARE_GPU='1', CWN_BENCH_MIN_REGION_S='0.005', CWN_BENCH_DETAIL=detail,
               CWN_BENCH_SKIP='concurrent,full,eager' + ('' if with_train else ',train'))
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world),
           '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.join(root, 'bench.py'),
           '--gpus', str(world), '--steps', '8', '--warmup', '2', '--full', '--no-cpu', '--kernel-reps', '4', '--num-batches', '2']
    out = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]            # rank 0 prints ONE line
    d = json.loads(lines[0])
    assert d['n_gpus'] == world and d['steps'] == 8 and d['warmup'] == 2 and d['scaling'] == 'weak'
    assert d['value'] > 0 and d['unit'] == 'cells/s' and d['cpu_baseline'] is None
    # whole-job value: all ranks' cells over the slowest rank's time
    assert abs(d['value'] - world * d['config']['cells_per_batch'] * d['config']['layers'] / (d['ms_per_step'] * 1e-3)) \
        < 0.2 * d['value']
    assert d['roofline'] is not None and 0 < d['roofline']['frac'] < 1
    assert d['timing']['rounds'] >= 1 and d['timing']['timed_steps'] == d['timing']['rounds'] * 8
    assert len(lines[0]) < 6144 and d['multi_gpu']['rccl_ranks'] == world
    if with_train:
        assert d['secondary']['train_step_ms'] > 0
        with open(detail) as fh:
            tr = json.load(fh)['secondary']['train_step']
        assert tr is not None and 'skipped' not in tr and tr['ms_per_step'] > 0 and tr['backward_pieces'] >= 1, tr


@pytest.mark.parametrize('E,n_dst,n_src', [(60, 9, 11), (300_000, 5000, 7000)])
def test_both_csr_build_paths_treat_bad_indices_alike(E, n_dst, n_src):
    """the one-launch LDS path (small inputs) and the general path must produce the SAME
    integers on out-of-range input: every bad index is reported, an entry with a bad destination is
    dropped, a bad source / shared index is clamped into range."""
    from cwn_amd import csr
    from cwn_amd.csr import Adjacency, build_many
    g = torch.Generator().manual_seed(E)
    key = torch.randint(0, n_dst, (E,), generator=g)
    val = torch.randint(0, n_src, (E,), generator=g)
    aux = torch.randint(0, 13, (E,), generator=g)
    key[[3, E // 2]] = torch.tensor([n_dst + 5, -2])          # bad destinations: dropped
    val[[5, E - 1]] = torch.tensor([n_src + 9, -7])           # bad sources: clamped to n_src - 1 / 0
    aux[7] = 99                                               # bad shared index: clamped to 12
    adj = Adjacency(key.to(DEV), val.to(DEV), n_dst, n_src, aux.to(DEV), 13)
    build_many([adj], validate=False)
    with pytest.raises(IndexError, match='destination index, source index, shared'):
        csr.check_errors(DEV)
    keep = (key >= 0) & (key < n_dst)
    ids = torch.nonzero(keep).flatten()
    order = ids[torch.argsort(key[ids], stable=True)]
    want_rowptr = torch.zeros(n_dst + 1, dtype=torch.int64)
    want_rowptr[1:] = torch.bincount(key[ids], minlength=n_dst).cumsum(0)
    n_ok = int(want_rowptr[-1])
    assert torch.equal(cpu(adj.rowptr).long(), want_rowptr)
    assert torch.equal(cpu(adj.perm)[:n_ok].long(), order)
    assert torch.equal(cpu(adj.col)[:n_ok].long(), val[order].clamp(0, n_src - 1))
    assert torch.equal(cpu(adj.aux)[:n_ok].long(), aux[order].clamp(0, 12))


@pytest.mark.parametrize('M,K,N,affine,relu', [(1, 128, 128, True, 1), (33, 128, 128, True, 1), (3341, 128, 128, True, 1),
                                               (500, 128, 128, False, 1), (777, 64, 64, True, 1), (65, 64, 64, True, 0),
                                               (2000, 128, 128, True, 0), (500, 128, 64, True, 1), (300, 64, 128, True, 1)])
def test_gemm_with_batchnorm_backward_prologue(M, K, N, affine, relu):
    """cwn_gemm_bnb: the transposed-weight GEMM whose input is the BatchNorm / ReLU backward of dy, formed in the prologue,
    against cwn_norm_bwd_apply_f32 + the plain GEMM (same arithmetic up to the grouping of the per-column constants) and
    against float64; dz written once, the sums handed on to acc1 / acc2 by exactly one workgroup; a second descriptor over
    the same input (dz = NULL) multiplies the same dz."""
    from cwn_amd import _ffi, ops
    from cwn_amd.dense_train import _norm_desc
    g = torch.Generator().manual_seed(M + 3 * K + 7 * N + affine + 2 * relu)
    dy = torch.randn(M, K, generator=g).to(DEV)
    z = (torch.randn(M, K, generator=g) * 2 + 0.5).to(DEV)
    W = (torch.randn(K, N, generator=g) / K ** 0.5).to(DEV)          # w_trans layout: [K, N]
    aff = None
    s12 = torch.zeros(2, K, device=DEV)
    if affine:
        aff = torch.stack([torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g), torch.randn(K, generator=g) * 0.3 + 0.5,
                           torch.rand(K, generator=g) + 0.5]).to(DEV)      # scale, shift, mean, rstd
        _ffi.norm_bwd_reduce([_norm_desc(z, dy=dy, aff=aff, s12=s12, relu=bool(relu))], DEV)
    # reference: apply launch + plain GEMM, and float64
    dz_ref = torch.empty(M, K, device=DEV)
    _ffi.norm_bwd_apply([_norm_desc(z, dy=dy, out=dz_ref, aff=aff, s12=s12 if affine else None, relu=bool(relu))], DEV)
    y_ref, = ops.run_gemm([ops.Gemm(X=dz_ref, W=W, w_trans=True)], DEV)
    z64, dy64 = cpu(z).double(), cpu(dy).double()
    if affine:
        sc, sh, mu, rs = (cpu(aff[r]).double() for r in range(4))
        yv = z64 * sc + sh
        dyh = dy64 * (yv > 0) if relu else dy64
        xhat = (z64 - mu) * rs
        dz64 = sc * (dyh - cpu(s12[0]).double() / M - xhat * cpu(s12[1]).double() / M)
    else:
        dz64 = dy64 * (z64 > 0) if relu else dy64
    y64 = dz64 @ cpu(W).double()
    # the fused form, two descriptors over the same input (the halves of a combine weight in the training step)
    W = torch.cat([W, W.flip(1)], 1).contiguous()                     # [K, 2N]: the second product uses another weight
    y64 = torch.cat([y64, y64.flip(1)], 1)
    y_ref = torch.cat([y_ref, y_ref.flip(1)], 1)
    h = N
    dz = torch.full((M, K), float('nan'), device=DEV)
    acc = torch.ones(2, K, device=DEV)
    out = torch.empty(M, 2 * N, device=DEV)
    b = _ffi.GemmBnb(z=z.data_ptr(), dz=dz.data_ptr(), ldz=z.stride(0), lddz=dz.stride(0), relu=relu)
    if affine:
        b.scale, b.shift, b.mean, b.rstd = (aff[r].data_ptr() for r in range(4))
        b.s1, b.s2, b.acc1, b.acc2 = s12[0].data_ptr(), s12[1].data_ptr(), acc[0].data_ptr(), acc[1].data_ptr()
    b2 = _ffi.GemmBnb.from_buffer_copy(b)
    b2.dz, b2.acc1, b2.acc2 = None, None, None
    ops.run_gemm([ops.Gemm(X=dy, W=W[:, :h], w_trans=True, out=out[:, :h], bnb=b),
                  ops.Gemm(X=dy, W=W[:, h:], w_trans=True, out=out[:, h:], bnb=b2)], DEV)
    scale = max(1.0, float(dz64.abs().max()))
    torch.testing.assert_close(cpu(dz).double(), dz64, rtol=1e-5, atol=2e-5 * scale)
    torch.testing.assert_close(cpu(dz), cpu(dz_ref), rtol=1e-5, atol=1e-5 * scale)
    torch.testing.assert_close(cpu(out).double(), y64, rtol=1e-5, atol=3e-5 * max(1.0, float(y64.abs().max())))
    torch.testing.assert_close(cpu(out), cpu(y_ref), rtol=1e-5, atol=2e-5 * max(1.0, float(y64.abs().max())))
    if affine:
        assert torch.equal(acc, 1.0 + s12)          # added once (the first workgroup of the FIRST descriptor), exactly
    else:
        assert torch.equal(acc, torch.ones_like(acc))
    # misuse is refused before anything is launched
    with pytest.raises(_ffi.CwnError):
        ops.run_gemm([ops.Gemm(X=dy, W=W.t().contiguous(), bnb=b)], DEV)           # not a transposed-weight launch


@pytest.mark.parametrize('M,N,K', [(1, 128, 128), (3341, 128, 128), (515, 64, 64), (100, 40, 24), (48 * 7 + 5, 128, 128)])
def test_gemm_add_out_adds_onto_what_the_output_holds(M, N, K):
    from cwn_amd import ops
    g = torch.Generator().manual_seed(M + N + K)
    X = torch.randn(M, K, generator=g).to(DEV)
    Wt = (torch.randn(K, N, generator=g) / K ** 0.5).to(DEV)
    base = torch.randn(M, N, generator=g).to(DEV)
    plain, = ops.run_gemm([ops.Gemm(X=X, W=Wt, w_trans=True)], DEV)
    out = base.clone()
    ops.run_gemm([ops.Gemm(X=X, W=Wt, w_trans=True, out=out, add_out=True)], DEV)
    assert torch.equal(out, base + plain)


@pytest.mark.gpu
@pytest.mark.parametrize('F,Ms', [(128, (3165, 3341, 304)), (128, (1, 33)), (64, (700, 65, 2)),
                                  (128, (3165, 3341, 304, 3165, 3341, 299)), (64, (9000, 8999))])     # (the last two: the large row tile)
def test_dense_stage_kernel_vs_grouped_gemm(F, Ms):
    """cwn_dense_stage_f32 (csrc/cwn_stage.hip: one stage of the update / combine networks in training mode on the bf16-split
    path with pre-packed weights) against the grouped cwn_gemm_f32 launch it replaces and a float64 product: the rows of Z
    within the gate, the per-band column statistics (fp64 partials of what each path wrote) to 1e-6 of the band's scale;
    both forms (F -> F with one prologue, 2F -> F on the K-concatenation with two), a launch of several products, row
    counts that end inside a band and inside a workgroup."""
    from cwn_amd import ops
    g = torch.Generator().manual_seed(F + len(Ms))
    rn = lambda *s: torch.randn(*s, generator=g).to(DEV)
    lins = [torch.nn.Linear(F, F).to(DEV) for _ in Ms] + [torch.nn.Linear(2 * F, F).to(DEV) for _ in Ms]
    ops.pack_stage_weights_many([l.weight for l in lins])

    def make(form):
        gemms = []
        for k, M in enumerate(Ms):
            X, X2 = rn(M, F), rn(M, F)
            sc, sh, sc2, sh2 = rn(F).abs() + 0.5, rn(F), rn(F).abs() + 0.5, rn(F)
            stats = torch.zeros(2, ops.stat_rows(M), F, dtype=torch.float64, device=DEV)
            if form == 'single':
                lin = lins[k]
                gemms.append(ops.Gemm(X=X, W=lin.weight, bias=lin.bias.detach(), in_scale=sc if k % 2 == 0 else None,
                                      in_shift=sh if k % 2 == 0 else None, in_relu=1 if k != 1 else 0, col_stats=stats))
            else:
                lin = lins[len(Ms) + k]
                gemms.append(ops.Gemm(X=X, X2=X2, W=lin.weight, bias=lin.bias.detach() if k else None, in_scale=sc, in_shift=sh,
                                      in_scale2=sc2, in_shift2=sh2, in_relu=3, col_stats=stats))
        return gemms

    for form in ('single', 'cat'):
        gemms = make(form)
        got = ops.run_stage(gemms, DEV)
        assert got is not None, 'the stage kernel refused a launch it is written for'
        got_stats = [gm.col_stats.clone() for gm in gemms]
        for gm in gemms:
            gm.col_stats.zero_()
        with torch.no_grad():
            ref = ops.run_gemm(gemms, DEV)
        for k, gm in enumerate(gemms):
            x = gm.X.double()
            if gm.in_scale is not None:
                x = x * gm.in_scale.double() + gm.in_shift.double()
            if gm.in_relu & 1:
                x = x.relu()
            if gm.X2 is not None:
                x2 = (gm.X2.double() * gm.in_scale2.double() + gm.in_shift2.double()).relu()
                x = torch.cat([x, x2], 1)
            z = x @ gm.W.detach().double().t() + (gm.bias.double() if gm.bias is not None else 0.0)
            scale = float(z.abs().max())
            assert (got[k].double() - z).abs().max() <= 1e-5 * max(1.0, scale), (form, k)
            assert (ref[k].double() - z).abs().max() <= 1e-5 * max(1.0, scale), (form, k)
            M = z.size(0)
            pad = (-M) % 32
            zp = torch.cat([z, z.new_zeros(pad, F)]).view(-1, 32, F)
            want = torch.stack([zp.sum(1), (zp * zp).sum(1)])
            tol = 1e-6 * max(1.0, float(want.abs().max()))
            assert (got_stats[k] - want).abs().max() <= 32 * 1e-6 * max(1.0, scale * scale), (form, k)
            assert (gm.col_stats - want).abs().max() <= 32 * 1e-6 * max(1.0, scale * scale), (form, k)
            del tol
    # a block that was not packed by the latest call: the launch is refused (the caller runs cwn_gemm_f32)
    ops.pack_stage_weights_many([lins[0].weight])
    assert ops.run_stage(make('cat'), DEV) is None


@pytest.mark.gpu
@pytest.mark.parametrize('F,Ms,blocks', [(128, (3165, 3341, 304), 3), (128, (1, 33, 700), 4), (64, (700, 65, 2, 129), 3),
                                         (64, (9000, 63), 4), (128, (2968, 6381, 612, 40), 4)])
def test_dense_stage_ex_kernel_vs_float64(F, Ms, blocks):
    """cwn_dense_stage_ex_f32 (round 4, ABI 19): Z = prologue([X | X2 | X3 (| X4)]) W^T + b with W [F, 3F] / [F, 4F] -- the
    combine network of a CIN++ layer (mp/layers.py:260, 408-410) -- against the float64 product: the first two blocks with the
    scale / shift prologues of cwn_dense_stage_f32, the extra blocks with ReLU or nothing in front, a LIVE BatchNorm record on
    an extra block (its affine derived in the kernel from slot sums, written to `aff`; running statistics updated once), the
    per-band column statistics, several products per launch, row counts that end inside a band and inside a workgroup; a launch
    without extras falls through to the two-block kernel."""
    from cwn_amd import ops, _ffi
    g = torch.Generator().manual_seed(31 * F + sum(Ms) + blocks)
    rn = lambda *s: torch.randn(*s, generator=g).to(DEV)
    lins = [torch.nn.Linear(blocks * F, F).to(DEV) for _ in Ms]
    ops.pack_stage_weights_many([l.weight for l in lins])
    gemms, refs, keep = [], [], []
    for k, M in enumerate(Ms):
        Xs = [rn(M, F) for _ in range(blocks)]
        sc, sh, sc2, sh2 = rn(F).abs() + 0.5, rn(F), rn(F).abs() + 0.5, rn(F)
        stats = torch.zeros(2, ops.stat_rows(M), F, dtype=torch.float64, device=DEV)
        more, pro = [], []
        for j in range(2, blocks):
            relu = (j + k) % 2 == 0
            live = (j == 2 and k % 2 == 0)
            if live:
                # a BatchNorm(train) in front of this block: slot sums of the block's own values (as the producing launch leaves them)
                x64 = Xs[j].double()
                slots = torch.zeros(_ffi.BN_SLOTS, 2, F, dtype=torch.float64, device=DEV)
                parts = x64.chunk(_ffi.BN_SLOTS) if M >= _ffi.BN_SLOTS else [x64]
                for q, part in enumerate(parts):
                    slots[q, 0], slots[q, 1] = part.sum(0), (part * part).sum(0)
                gamma, beta = rn(F).abs() + 0.5, rn(F)
                rm, rv, nbt = torch.zeros(F, device=DEV), torch.ones(F, device=DEV), torch.zeros((), dtype=torch.long, device=DEV)
                aff = torch.full((4, F), float('nan'), device=DEV)
                rec = _ffi.BnLive(slots=slots.data_ptr(), gamma=gamma.data_ptr(), beta=beta.data_ptr(), running_mean=rm.data_ptr(),
                                  running_var=rv.data_ptr(), num_batches_tracked=nbt.data_ptr(), aff=aff.data_ptr(), eps=1e-5,
                                  momentum=0.1)
                mean, var = x64.mean(0), x64.var(0, unbiased=False)
                scale = gamma.double() / torch.sqrt(var + 1e-5)
                pro.append((scale, beta.double() - mean * scale, relu))
                keep += [slots, gamma, beta, rm, rv, nbt, aff]
                refs.append((k, aff, scale, mean, var, rm, rv, nbt, M))
                more.append((Xs[j], relu, rec))
            else:
                pro.append((None, None, relu))
                more.append((Xs[j], relu, None))
        lin = lins[k]
        gemms.append(ops.Gemm(X=Xs[0], X2=Xs[1], W=lin.weight, bias=lin.bias.detach() if k != 1 else None, in_scale=sc, in_shift=sh,
                              in_scale2=sc2, in_shift2=sh2, in_relu=3 if k != 2 else 1, col_stats=stats, more=tuple(more)))
        x = [(Xs[0].double() * sc.double() + sh.double()).relu()]
        x2 = Xs[1].double() * sc2.double() + sh2.double()
        x.append(x2.relu() if k != 2 else x2)
        for j in range(2, blocks):
            a, b_, relu = pro[j - 2]
            xe = Xs[j].double() if a is None else Xs[j].double() * a + b_
            x.append(xe.relu() if relu else xe)
        z = torch.cat(x, 1) @ lin.weight.detach().double().t() + (lin.bias.detach().double() if k != 1 else 0.0)
        keep.append((Xs, z, stats))
    got = ops.run_stage(gemms, DEV)
    assert got is not None, 'the stage kernel refused a launch it is written for'
    torch.cuda.synchronize()
    zs = [t[1] for t in keep if isinstance(t, tuple)]
    for k, (gm, z) in enumerate(zip(gemms, zs)):
        scale = max(1.0, float(z.abs().max()))
        assert (got[k].double() - z).abs().max() <= 1e-5 * scale, (k, float((got[k].double() - z).abs().max()), scale)
        M = z.size(0)
        zp = torch.cat([z, z.new_zeros((-M) % 32, F)]).view(-1, 32, F)
        want = torch.stack([zp.sum(1), (zp * zp).sum(1)])
        assert (gm.col_stats - want).abs().max() <= 32 * 1e-6 * scale * scale, k
    for k, aff, scale, mean, var, rm, rv, nbt, M in refs:
        torch.testing.assert_close(aff[0].double(), scale, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(aff[2].double(), mean, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(rm.double(), 0.1 * mean, rtol=1e-5, atol=1e-6)
        unb = var * (M / max(M - 1, 1))
        torch.testing.assert_close(rv.double(), 0.9 + 0.1 * unb, rtol=1e-5, atol=1e-6)
        assert int(nbt) == 1
    # without extra blocks the same call runs the two-block kernel
    two = [ops.Gemm(X=gm.X, X2=gm.X2, W=torch.nn.Parameter(gm.W.detach()[:, :2 * F].contiguous()), in_relu=3) for gm in gemms]
    ops.pack_stage_weights_many([t.W for t in two])
    res = ops.run_stage(two, DEV)
    assert res is not None
    for t, r in zip(two, res):
        z = torch.cat([t.X.double().relu(), t.X2.double().relu()], 1) @ t.W.detach().double().t()
        assert (r.double() - z).abs().max() <= 1e-5 * max(1.0, float(z.abs().max()))


@pytest.mark.gpu
def test_packing_many_stage_blocks_equals_one_by_one():
    from cwn_amd import ops
    torch.manual_seed(3)
    ws = [torch.nn.Parameter(torch.randn(F, c * F, device=DEV)) for F, c in ((128, 1), (64, 2), (128, 2), (128, 1), (64, 1))]
    ops.pack_stage_weights_many(ws)
    for w in ws:
        F = w.size(0)
        one = ops.pack_mlp_weight(torch.nn.Parameter(w.detach().clone()))
        for h, c0 in enumerate(range(0, w.size(1), F)):
            assert torch.equal(ops.packed_stage_block(w, c0), one[h]), (tuple(w.shape), c0)


@pytest.mark.gpu
@pytest.mark.parametrize('F,Ms', [(128, (3165, 3341, 304)), (128, (1, 33)), (64, (700, 65, 2)),
                                  (128, (3165, 3341, 304, 3165, 3341, 299)), (64, (9000, 8999))])     # (the last two: the large row tile)
def test_dense_stage_backward_kernel_vs_float64(F, Ms):
    """cwn_dense_stage_bwd_f32: dz = BatchNorm(train) + ReLU backward of dy (given the column sums), written out, and dX = dz W
    -- one output for a Linear(F -> F), the two halves for a Linear(2F -> F) -- against the formulas in float64; the sums
    handed on to beta.grad / gamma.grad once; a stage without a norm (dz = dy where z > 0)."""
    from cwn_amd import ops, _ffi
    g = torch.Generator().manual_seed(7 * F + len(Ms))
    rn = lambda *s: torch.randn(*s, generator=g).to(DEV)
    for wide in (False, True):
        lins = [torch.nn.Linear(2 * F if wide else F, F).to(DEV) for _ in Ms]
        ops.pack_stage_weights_many([l.weight for l in lins])
        entries, refs, keep = [], [], []
        for k, M in enumerate(Ms):
            dy, z = rn(M, F), rn(M, F)
            with_norm = k != 1
            aff = torch.stack([rn(F).abs() + 0.5, rn(F), rn(F) * 0.1, rn(F).abs() + 0.5])      # scale, shift, mean, rstd
            s12 = torch.stack([rn(F), rn(F)]) * M ** 0.5
            acc = torch.stack([rn(F), rn(F)])
            acc0 = acc.clone()
            dz = torch.empty(M, F, device=DEV)
            b = _ffi.GemmBnb(z=z.data_ptr(), dz=dz.data_ptr(), ldz=F, lddz=F, relu=1)
            if with_norm:
                b.scale, b.shift, b.mean, b.rstd = (aff[r].data_ptr() for r in range(4))
                b.s1, b.s2 = s12[0].data_ptr(), s12[1].data_ptr()
                b.acc1, b.acc2 = acc[0].data_ptr(), acc[1].data_ptr()
            out = torch.full((M, 2 * F if wide else F), float('nan'), device=DEV)
            W = lins[k].weight
            entries.append((dy, b, W, out[:, :F], out[:, F:] if wide else None))
            keep += [dy, z, aff, s12, acc, dz, out]
            D = lambda t: t.double()
            if with_norm:
                sc, sh, mu, rs = (D(aff[r]) for r in range(4))
                dyh = D(dy) * ((D(z) * sc + sh) > 0)
                want_dz = sc * dyh - sc * D(s12[0]) / M - sc * rs * D(s12[1]) / M * (D(z) - mu)
            else:
                want_dz = D(dy) * (D(z) > 0)
            refs.append((dz, want_dz, out, want_dz @ D(W.detach()), acc, acc0, s12 if with_norm else None))
        assert ops.run_stage_bwd(entries, DEV), 'the backward stage kernel refused a launch it is written for'
        for k, (dz, want_dz, out, want_dx, acc, acc0, s12) in enumerate(refs):
            assert (dz.double() - want_dz).abs().max() <= 1e-5 * max(1.0, float(want_dz.abs().max())), (wide, k)
            assert (out.double() - want_dx).abs().max() <= 1e-5 * max(1.0, float(want_dx.abs().max())), (wide, k)
            if s12 is not None:
                torch.testing.assert_close(acc, acc0 + s12, rtol=1e-6, atol=1e-6)
            else:
                assert torch.equal(acc, acc0)
