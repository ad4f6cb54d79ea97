"""The graph baselines on static batches: EmbedGIN (with and without edge embeddings), GIN0 over float features and RingGIN
through StaticBatch(mode='csr') + StaticForward -- batches the captured graph has never seen, every GINConv / GINEConv as ONE
counted launch (layers.FUSED_GIN_STATIC: last_route 'fused_counted'), the pooled head as one ops.head launch over the slot's
`ptr` table, RingGIN's through ops.target_head.

About 35 small complexes, one of them a lone atom (no edge at all), batches of 8 in two slots: an epoch is four full batches
and a tail of three, and two epochs with different permutations run through ONE StaticForward.  The first batch of the first
epoch holds the eight largest complexes, so every later batch leaves stale rows of it behind its counts.

What is asserted: the replays equal StaticForward.eager() bit for bit; every batch's predictions pass tests/_product.gate --
max|delta| <= 1e-5 * max(1, |ref|_inf) -- against a float64 CPU copy of the model on the host-collated batch (plain torch on
the CPU; the pooled head sums in another order than a collated eager forward does, so equality of bits with that route is not
asked for); with layers.FUSED_GIN_STATIC off the same predictions pass the same gate on the generic route; and everything a
static batch does not serve is refused at construction, by model and reason."""
import copy

import numpy as np
import pytest
import torch

from cwn_amd import csr, layers, models, synthetic
from cwn_amd.complex import ComplexBatch
from tests import _gin
from tests._product import gate

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
B, S, N = 8, 2, 35
ATOMS, BONDS = 12, 4


@pytest.fixture
def routes_on():
    old = layers.FUSED_GIN, layers.FUSED_GINE, layers.FUSED_GIN_STATIC
    layers.FUSED_GIN = layers.FUSED_GINE = layers.FUSED_GIN_STATIC = True
    yield
    layers.FUSED_GIN, layers.FUSED_GINE, layers.FUSED_GIN_STATIC = old


# ---- the datasets (built once) -------------------------------------------------------------------------------------------------------
_POOLS = {}


def _molecules(kind: str):
    """N - 1 small molecule-like ring lifts and a lone atom.  'types+edges': integer atom and bond types as [n, 1] floats
    (EmbedGIN with embed_edge); 'types': atom types, edges without features (EmbedGIN without); 'floats': three float features per
    vertex (GIN0)."""
    rng = np.random.default_rng(17)
    out = []
    for i in range(N):
        n, bonds = synthetic.random_molecule(rng, 6, 14) if i != 20 else (1, [])
        if kind == 'floats':
            vx = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32))
        else:
            vx = torch.from_numpy(rng.integers(0, ATOMS, size=(n, 1))).float()
        ex = torch.from_numpy(rng.integers(0, BONDS, size=(len(bonds), 1))).float() if kind == 'types+edges' and bonds else None
        y = torch.from_numpy(rng.standard_normal(1).astype(np.float32))
        out.append(synthetic.ring_lift(n, bonds, vx, ex, max_k=6, y=y))
    return out


def _rings():
    return synthetic.ring_transfer(6, 10) + synthetic.ring_transfer(10, 15) + synthetic.ring_transfer(4, N - 25)


def _pool(kind: str):
    """(complexes, PackedComplexes on the device, max_dim of the host collate)."""
    from cwn_amd.packed import PackedComplexes
    if kind not in _POOLS:
        if kind == 'rings':
            cxs = _rings()
            _POOLS[kind] = (cxs, PackedComplexes(cxs, DEV, with_csr=True), 2)
        else:
            cxs = _molecules(kind)
            assert cxs[20].nodes.upper_index is None and cxs[20].nodes.num_cells == 1      # the complex without edges
            _POOLS[kind] = (cxs, PackedComplexes(cxs, DEV, max_dim=1, with_csr=True), 1)
    return _POOLS[kind]


def _epochs(cxs):
    """Two permutations of the dataset cut into four batches of B and a tail of three; the first batch of the first epoch is
    the B largest complexes."""
    size = np.array([c.nodes.num_cells for c in cxs])
    rng = np.random.default_rng(3)
    big = np.argsort(-size, kind='stable')[:B]
    rest = rng.permutation(np.setdiff1d(np.arange(len(cxs)), big))
    first = np.concatenate([big, rest])
    second = rng.permutation(len(cxs))
    assert not np.array_equal(first, second)
    cut = lambda perm: [perm[lo:lo + B] for lo in range(0, len(perm), B)]
    epochs = [cut(first), cut(second)]
    assert [len(b) for b in epochs[0]] == [B, B, B, B, 3]
    return epochs


def _model(case: str):
    torch.manual_seed(4)
    if case == 'embed_gin_edges':
        m = models.EmbedGIN(ATOMS, BONDS, 3, num_layers=2, hidden=16, embed_edge=True, train_eps=True, readout='sum')
    elif case == 'embed_gin':
        m = models.EmbedGIN(ATOMS, BONDS, 3, num_layers=2, hidden=16, embed_edge=False, readout='mean')
    elif case == 'gin0':
        m = models.GIN0(3, 2, 16, 4, readout='sum')
    else:
        m = models.RingGIN(5, 3, 16, 5)
    return _gin.randomise(m, 6).eval()


CASES = {'embed_gin_edges': 'types+edges', 'embed_gin': 'types', 'gin0': 'floats', 'ring_gin': 'rings'}


def _convs(model):
    return [m for m in model.modules() if isinstance(m, (layers.GINConv, layers.GINEConv))]


_REFS = {}


def _references(case):
    """Per epoch and batch the float64 CPU model on the host-collated batch, computed once per case."""
    if case not in _REFS:
        cxs, _, max_dim = _pool(CASES[case])
        model64 = copy.deepcopy(_model(case)).double().eval()
        refs = []
        with torch.no_grad():
            for epoch in _epochs(cxs):
                refs.append([])
                for idx in epoch:
                    b = ComplexBatch.from_complex_list([copy.deepcopy(cxs[i]) for i in idx], max_dim=max_dim)
                    if not case.startswith('embed_gin'):
                        b.cochains[0].x = b.cochains[0].x.double()
                    refs[-1].append(model64(b))
                    assert all(c.last_route == 'generic' for c in _convs(model64))
        assert max(float(r.abs().max()) for e in refs for r in e) > 1e-3
        _REFS[case] = refs
    return _REFS[case]


def _run(case, counted: bool):
    """Both epochs through ONE StaticForward: (per epoch the per-batch predictions, the model, the StaticForward)."""
    from cwn_amd.static_batch import StaticBatch
    from cwn_amd.static_graph import StaticForward
    cxs, packed, _ = _pool(CASES[case])
    model = _model(case).to(DEV)
    layers.FUSED_GIN_STATIC = counted
    sb = StaticBatch(packed, B, slots=S, mode='csr')
    sf = StaticForward(model, sb)
    got = []
    for epoch in _epochs(cxs):
        assert sb.fits(epoch).all()
        got.append(sf.run_epoch(epoch))
        assert all(c.last_route == ('fused_counted' if counted else 'generic') for c in _convs(model)), [c.last_route for c in _convs(model)]
    # the last epoch's first S batches again, as ordinary launches: what a replay must reproduce bit for bit
    last = _epochs(cxs)[-1]
    sb.set_epoch(last)
    eager = [o.clone() for o in sf.eager()]
    for j in range(S):
        assert torch.equal(eager[j][:len(last[j])], got[-1][j]), (case, j)
    torch.cuda.synchronize()
    csr.check_errors(DEV)
    return got


@pytest.mark.parametrize('case', sorted(CASES))
def test_counted_route_on_unseen_batches_against_the_float64_cpu_model(routes_on, case):
    got, refs = _run(case, counted=True), _references(case)
    for e, (ge, re_) in enumerate(zip(got, refs)):
        assert len(ge) == len(re_) == 5
        for j, (g, r) in enumerate(zip(ge, re_)):
            gate(g, r, f'{case} counted, epoch {e} batch {j}')


@pytest.mark.parametrize('case', sorted(CASES))
def test_generic_route_on_unseen_batches_against_the_float64_cpu_model(routes_on, case):
    """layers.FUSED_GIN_STATIC off: one aggregation launch and the torch modules per layer, the same head -- the same gate.
    (The readout of the pooled models goes through the slot's `ptr` table, which every fill rewrites; a plan keyed on the
    slot's `batch` vector would be the first batch's.)"""
    got, refs = _run(case, counted=False), _references(case)
    for e, (ge, re_) in enumerate(zip(got, refs)):
        for j, (g, r) in enumerate(zip(ge, re_)):
            gate(g, r, f'{case} generic, epoch {e} batch {j}')


# ---- what is refused -----------------------------------------------------------------------------------------------------------------
def _custom_nn():
    m = models.EmbedGIN(ATOMS, BONDS, 3, num_layers=2, hidden=16)
    m.convs[1].nn = torch.nn.Sequential(torch.nn.Linear(16, 16), torch.nn.ReLU())
    return m


REFUSED = {
    'blocked': (lambda: models.GIN0(3, 2, 16, 4), 'floats', 'blocked', r"GIN0 .*mode='csr'"),
    'jk cat': (lambda: models.GIN0WithJK(3, 2, 16, 4, mode='cat'), 'floats', 'csr', 'GIN0WithJK .*JumpingKnowledge'),
    'jk max': (lambda: models.GINWithJK(3, 2, 16, 4, mode='max'), 'floats', 'csr', 'GINWithJK .*JumpingKnowledge'),
    'tanh head': (lambda: models.GIN(3, 2, 16, 4, nonlinearity='tanh'), 'floats', 'csr', "GIN .*'tanh'.*ReLU"),
    'elu head': (lambda: models.EmbedGIN(ATOMS, BONDS, 3, 2, 16, nonlinearity='elu'), 'types', 'csr', "EmbedGIN .*'elu'.*ReLU"),
    'width 6': (lambda: models.GIN0(3, 2, 6, 4), 'floats', 'csr', 'GIN0 .*width 6 is no multiple of 4'),
    'width 10': (lambda: models.EmbedGIN(ATOMS, BONDS, 3, 2, 10), 'types', 'csr', 'EmbedGIN .*width 10 is no multiple of 4'),
    'layernorm': (lambda: models.RingGIN(5, 3, 16, 5, graph_norm='ln'), 'rings', 'csr', 'RingGIN .*conv1 does not fold'),
    'custom nn': (_custom_nn, 'types', 'csr', r'EmbedGIN .*convs\.1 does not fold'),
    'float64': (lambda: models.GIN0(3, 2, 16, 4).double(), 'floats', 'csr', 'GIN0 .*float64'),
}


@pytest.mark.parametrize('name', sorted(REFUSED))
def test_static_forward_refuses_what_it_does_not_serve_by_model_and_reason(name):
    from cwn_amd.static_batch import StaticBatch
    from cwn_amd.static_graph import StaticForward
    make, kind, mode, reason = REFUSED[name]
    sb = StaticBatch(_pool(kind)[1], B, slots=1, mode=mode)
    with pytest.raises(NotImplementedError, match='StaticForward: ' + reason):
        StaticForward(make().to(DEV).eval(), sb)


@pytest.mark.parametrize('case', sorted(CASES))
def test_static_train_step_refuses_the_gin_family_by_name(case):
    from cwn_amd.static_batch import StaticBatch
    from cwn_amd.static_graph import StaticTrainStep
    sb = StaticBatch(_pool(CASES[case])[1], B, slots=1, mode='csr')
    model = _model(case).to(DEV).train()
    with pytest.raises(NotImplementedError, match=f'StaticTrainStep: {type(model).__name__} .*inference only'):
        StaticTrainStep(model, sb)
