"""packed.PackedCochains on the device: `collate(idx)` against CochainBatch.from_cochain_list(...).to(device) field for field
(torch.equal), one cwn_collate launch per batch, the attached plans against csr.Adjacency.from_index on the collated index,
no cwn_csr_build in an EdgeOrient training step on a collated batch, and the loader.  Float comparisons use
tests/_product.gate: max|delta| <= 1e-5 * max(1, |ref|_inf)."""
import numpy as np
import pytest
import torch

from cwn_amd import _ffi, csr, models, packed
from cwn_amd.complex import Cochain, CochainBatch
from cwn_amd.synthetic import edge_flows
from tests._product import gate

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
FIELDS = ('x', 'y', 'batch', 'upper_index', 'lower_index', 'upper_orient', 'lower_orient')


def _dataset(kind: str):
    cs = edge_flows(6, side=6, seed=5)
    if kind == 'no_upper':
        c = cs[2]
        cs[2] = Cochain(dim=1, x=c.x, lower_index=c.lower_index, lower_orient=c.lower_orient, y=c.y)
    if kind == 'no_cells':
        z = torch.zeros(2, 0, dtype=torch.long)
        cs[4] = Cochain(dim=1, x=torch.zeros(0, 1), upper_index=z, lower_index=z.clone(), upper_orient=torch.zeros(0),
                        lower_orient=torch.zeros(0), y=torch.tensor([1]))
    if kind == 'long_row':
        # a hand-made cochain: row 3 has 70 lower neighbours (> CWN_LONG_ROW), the others a few
        g = torch.Generator().manual_seed(0)
        n = 90
        dst = torch.cat([torch.full((70,), 3), torch.randint(0, n, (150,), generator=g)])
        src = torch.randint(0, n, (220,), generator=g)
        p = torch.randperm(220, generator=g)
        low = torch.stack([src[p], dst[p]])
        up = torch.stack([torch.randint(0, n, (40,), generator=g), torch.randint(0, n, (40,), generator=g)])
        cs[1] = Cochain(dim=1, x=torch.randn(n, 1, generator=g), upper_index=up, lower_index=low,
                        upper_orient=torch.randn(40, generator=g), lower_orient=torch.randn(220, generator=g), y=torch.tensor([0]))
    return cs


_PACKED = {}


def _packed(kind: str):
    if kind not in _PACKED:
        cs = _dataset(kind)
        _PACKED[kind] = (cs, packed.PackedCochains(cs, DEV))
    return _PACKED[kind]


def _assert_same_batch(got: CochainBatch, ref: CochainBatch, what):
    for f in FIELDS:
        a, b = getattr(got, f), getattr(ref, f)
        assert (a is None) == (b is None), (what, f)
        if a is not None:
            assert a.dtype == b.dtype and a.device == b.device and torch.equal(a, b), (what, f)
    assert got.ptr == ref.ptr and got.num_cochains == ref.num_cochains and got.num_cells == ref.num_cells, what
    assert got.__slices__ == ref.__slices__ and got.__num_cells_list__ == ref.__num_cells_list__, what
    assert got.__num_cells_up__ == ref.__num_cells_up__ and got.__num_cells_down__ == ref.__num_cells_down__, what
    seg = [0] + np.cumsum([n or 0 for n in ref.__num_cells_list__]).tolist()
    assert got.ptr_dev.dtype == torch.long and got.ptr_dev.is_cuda and got.ptr_dev.tolist() == seg, what


CASES = [('plain', [0, 1, 2, 3, 4, 5]), ('plain', [4, 2, 5, 0, 3, 1]), ('plain', [3]), ('plain', [1, 4, 1, 1]),
         ('no_upper', [0, 1, 2, 3, 4, 5]), ('no_upper', [2]), ('no_upper', [2, 5, 2]),
         ('no_cells', [5, 4, 3, 2, 1, 0]), ('no_cells', [4]), ('no_cells', [4, 0]), ('long_row', [0, 1, 2, 1])]


@pytest.mark.parametrize('kind,idx', CASES)
def test_collate_equals_the_host_collate(kind, idx):
    cs, pc = _packed(kind)
    ref = CochainBatch.from_cochain_list([cs[i] for i in idx]).to(DEV)
    _assert_same_batch(pc.collate(idx), ref, (kind, idx))
    if 'y' in ref.keys:
        assert torch.equal(pc.labels(idx), ref.y)


class _Calls:
    """Counts cwn_collate / cwn_csr_build / cwn_csr_long_rows calls by wrapping the loaded library's functions."""
    NAMES = ('cwn_collate', 'cwn_csr_build', 'cwn_csr_long_rows')

    def __enter__(self):
        self.n = dict.fromkeys(self.NAMES, 0)
        self._lib = _ffi.lib()

        class Proxy:
            def __getattr__(p, name):
                fn = getattr(self._lib, name)
                if name not in self.NAMES:
                    return fn

                def counted(*a):
                    self.n[name] += 1
                    return fn(*a)
                return counted
        self._prev, _ffi._lib = _ffi._lib, Proxy()
        return self

    def __exit__(self, *exc):
        _ffi._lib = self._prev
        return False


def test_a_collate_is_one_launch():
    _, pc = _packed('plain')
    with _Calls() as c:
        pc.collate([2, 0, 5])
    assert c.n == {'cwn_collate': 1, 'cwn_csr_build': 0, 'cwn_csr_long_rows': 0}
    _, pl = _packed('long_row')
    assert pl.has_long_rows and not pc.has_long_rows
    with _Calls() as c:
        pl.collate([1, 0])
    assert c.n == {'cwn_collate': 1, 'cwn_csr_build': 0, 'cwn_csr_long_rows': 1}


@pytest.mark.parametrize('kind,idx', [('plain', [4, 2, 5, 0]), ('no_upper', [1, 2, 0]), ('no_cells', [4, 0, 4, 3]), ('long_row', [0, 1, 2, 1])])
def test_attached_plans_equal_a_build_on_the_collated_index(kind, idx):
    _, pc = _packed(kind)
    b = pc.collate(idx)
    n = b.num_cells
    for key in ('upper_index', 'lower_index'):
        index = getattr(b, key)
        got = csr.cached_adjacency(index, n, n, build=False)          # what OrientedConv._plans is handed: built by the collate
        assert got.built and got._t_src is not None and got._t_src.built
        ref = csr.Adjacency.from_index(index.clone(), n, n)
        for g, r, what in ((got, ref, key), (got.t_src, ref.t_src, key + '^T')):
            assert g.n_dst == r.n_dst == n and g.n_entries == r.n_entries
            for f in ('rowptr', 'col', 'perm'):
                assert torch.equal(getattr(g, f), getattr(r, f)), (kind, what, f)
            assert sorted(g.long_row_list().tolist()) == sorted(r.long_row_list().tolist()), (kind, what)
            if kind == 'long_row' and key == 'lower_index' and g is got:
                assert len(r.long_row_list()) == 2                    # (cochain 1 twice in the batch: the case says something)


def test_training_step_builds_no_csr_and_matches_the_host_batch():
    cs, pc = _packed('plain')
    idx = [3, 0, 5, 1]
    torch.manual_seed(0)
    model = models.EdgeOrient(1, 2, 3, 16, nonlinearity='tanh').to(DEV).train()
    host = CochainBatch.from_cochain_list([cs[i] for i in idx]).to(DEV)
    model(host).square().sum().backward()
    y_ref = model(CochainBatch.from_cochain_list([cs[i] for i in idx]).to(DEV)).detach()
    g_ref = {k: p.grad.clone() for k, p in model.named_parameters()}
    prev = models.FUSED_FLOW_HEAD
    try:
        models.FUSED_FLOW_HEAD = False                      # same launches, same operands: the same bits
        assert torch.equal(model(pc.collate(idx)).detach(), y_ref) and model.last_head_route == 'generic'
        models.FUSED_FLOW_HEAD = True
        model.zero_grad(set_to_none=True)
        batch = pc.collate(idx)
        with _Calls() as c:
            y = model(batch)
            y.square().sum().backward()
        assert model.last_head_route == 'fused'
        assert c.n['cwn_csr_build'] == 0, c.n
    finally:
        models.FUSED_FLOW_HEAD = prev
    gate(y, y_ref.double(), 'predictions: packed batch + fused head against the host batch')
    for k, p in model.named_parameters():
        gate(p.grad, g_ref[k].double(), f'grad {k}')


def test_loader_visits_every_cochain_once_per_epoch():
    cs, pc = _packed('plain')
    pc.epoch = 0
    orders = []
    for _ in range(2):
        ys, sizes = [], []
        for b in pc.batches(4, shuffle=True, seed=7):
            assert b.x.is_cuda and b.ptr_dev.numel() == b.num_cochains + 1
            sizes.append(b.num_cochains)
            ys.append(b.y)
        assert sizes == [4, 2]
        orders.append(np.concatenate(pc.batch_indices(4, shuffle=True, seed=7, epoch=pc.epoch - 1)))
        assert sorted(orders[-1].tolist()) == list(range(6))
        assert torch.equal(torch.cat(ys), pc.labels(orders[-1]))
    assert orders[0].tolist() != orders[1].tolist()
    again = np.concatenate(pc.batch_indices(4, shuffle=True, seed=7, epoch=0))
    assert again.tolist() == orders[0].tolist()
    assert [b.num_cochains for b in pc.batches(4, drop_last=True)] == [4]


def test_evaluate_takes_a_packed_cochain_dataset():
    """evaluate.evaluate over packed.CochainForward: the labels by `labels(idx)`, the metric and the mean loss of the eager pass."""
    from cwn_amd import evaluate
    cs, pc = _packed('plain')
    torch.manual_seed(2)
    model = models.EdgeOrient(1, 2, 2, 16, nonlinearity='tanh').to(DEV)
    batches = pc.batch_indices(4)
    acc, loss = evaluate.evaluate(packed.CochainForward(model, pc), batches, evaluate.Evaluator('accuracy'), 'classification')
    with torch.no_grad():
        preds = [model(CochainBatch.from_cochain_list([cs[i] for i in idx]).to(DEV)) for idx in batches]
    y = torch.cat([c.y for c in cs]).to(DEV)
    assert acc == float((torch.cat(preds).argmax(1) == y).sum()) / len(cs)
    want = np.mean([float(torch.nn.functional.cross_entropy(p.double(), y[idx[0]:idx[-1] + 1])) for p, idx in zip(preds, batches)])
    assert abs(loss - want) <= 1e-5 * max(1.0, abs(want)), (loss, want)
