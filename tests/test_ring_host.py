"""Host-side checks of the ring-transfer experiment -- no GPU needed: the generator against the reference-made fixture
(tests/golden/ring_sparse_cin.npz, written by tools/gen_golden_ring.py from the reference's own RingSparseCIN and collate),
the `mask` key and the target rows through Cochain / CochainBatch / PackedComplexes, the C ABI of the target-cell head
(csrc/cwn_target_head.hip: every argument check precedes the first HIP call), and the RingSparseCIN mirror's state_dict."""
import os
import re

import numpy as np
import pytest
import torch

from cwn_amd import _ffi, models, ops, synthetic
from cwn_amd.complex import Cochain, Complex, ComplexBatch
from cwn_amd.packed import PackedComplexes
from tests._golden import load, state_dict, T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, ALIGN = 0, 1, 5
G = 'ring_sparse_cin.npz'
INDEX_KEYS = ('upper_index', 'shared_coboundaries', 'boundary_index')


def case_complexes(name):
    r = {n: synthetic.ring_transfer(n, 5, 5) for n in (4, 10, 30)}
    return {'ring4': r[4], 'ring10': r[10], 'ring30': r[30], 'mixed': [r[10][1], r[30][3], r[30][0], r[10][4]]}[name]


CASES = ('ring4', 'ring10', 'ring30', 'mixed')


@pytest.mark.parametrize('name', CASES)
def test_generator_reproduces_the_fixture_graphs_and_batches(name):
    """The fixture's per-graph arrays were written from synthetic.ring_transfer itself (tools/gen_golden_ring.py): for x, y and the
    lift this pins the generator against a change, not against the reference's own lift.  Reference-made, and compared here: the
    batched index tensors, `batch`, y and the collated `mask` (the reference's data/complex.py over those arrays)."""
    g = load(G)
    cxs = case_complexes(name)
    for i, cx in enumerate(cxs):
        assert np.array_equal(cx.nodes.x.numpy(), g[f'{name}/graphs/{i}/x'])
        assert np.array_equal(cx.y.numpy(), g[f'{name}/graphs/{i}/y'])
        assert cx.nodes.num_cells == int(g[f'{name}/graphs/{i}/nodes'])
        assert not cx.edges.x.any() and not cx.two_cells.x.any()
        assert cx.nodes.mask.dtype == torch.bool and cx.nodes.mask.nonzero().flatten().tolist() == [0]
    b = ComplexBatch.from_complex_list(cxs)
    for d in range(3):
        c = b.cochains[d]
        assert np.array_equal(c.x.numpy(), g[f'{name}/batch/{d}/x'])
        assert np.array_equal(c.batch.numpy(), g[f'{name}/batch/{d}/batch'])
        for k in INDEX_KEYS:
            key = f'{name}/batch/{d}/{k}'
            assert (c[k] is not None) == (key in g), key
            if c[k] is not None:
                assert np.array_equal(c[k].numpy(), g[key]), key
    assert np.array_equal(b.y.numpy(), g[f'{name}/batch/y'])
    # the extra key, batched as the reference's collate batches it, and the rows it marks
    want = g[f'{name}/batch/0/mask']
    assert b.nodes.mask.dtype == torch.bool and np.array_equal(b.nodes.mask.numpy(), want)
    assert 'mask' in b.nodes.keys and 'mask' in b.nodes
    rows = b.target_rows(0)
    assert rows.dtype == torch.int32 and np.array_equal(rows.numpy(), np.nonzero(want)[0])
    assert b.target_rows(1) is None and b.target_rows(5) is None


def test_samples_are_labelled_in_class_order():
    cxs = synthetic.ring_transfer(6, 10, 5)
    assert [int(c.y) for c in cxs] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4]
    for c in cxs:
        x = c.nodes.x
        assert x.shape == (6, 5) and not x[0].any() and x[3].tolist() == [float(k == int(c.y)) for k in range(5)]
        assert bool((x[[1, 2, 4, 5]] == 1).all())
    with pytest.raises(ValueError):
        synthetic.ring_transfer(6, 7, 5)
    with pytest.raises(ValueError):
        synthetic.ring_transfer(2, 5, 5)


@pytest.mark.parametrize('n', [3, 4, 7, 10, 30])
def test_ring_lift_of_an_n_ring(n):
    """One two-cell with n boundary edges; every ordered pair of distinct edges is upper adjacent through it: n (n - 1)."""
    cx = synthetic.ring_transfer(n, 5, 5)[2]
    assert cx.dimension == 2 and cx.nodes.num_cells == n and cx.edges.num_cells == n and cx.two_cells.num_cells == 1
    assert cx.two_cells.boundary_index.shape == (2, n) and sorted(cx.two_cells.boundary_index[0].tolist()) == list(range(n))
    assert cx.edges.upper_index.shape == (2, n * (n - 1)) and not cx.edges.shared_coboundaries.any()
    assert cx.nodes.upper_index.shape == (2, 2 * n)
    assert cx.edges.lower_index is None and cx.two_cells.lower_index is None


def test_mask_moves_with_the_cochain_and_is_cloned():
    c = synthetic.ring_transfer(5, 5, 5)[0].nodes
    d = c.clone()
    d.mask[1] = True
    assert c.mask.tolist() == [True, False, False, False, False]
    moved = d.to('cpu', dtype=None) if False else d.to('cpu')
    assert moved.mask.tolist() == [True, True, False, False, False]
    plain = Cochain(dim=0, x=torch.zeros(3, 2))
    assert plain.mask is None and 'mask' not in plain.keys


def _two_marks():
    cxs = synthetic.ring_transfer(5, 5, 5)
    bad = cxs[2]
    m = bad.nodes.mask.clone()
    m[3] = True
    two = Complex(Cochain(dim=0, x=bad.nodes.x, upper_index=bad.nodes.upper_index, shared_coboundaries=bad.nodes.shared_coboundaries,
                          num_cells=5, num_cells_up=5, mask=m), bad.edges, bad.two_cells, y=bad.y, dimension=2)
    return [cxs[0], two, cxs[1]]


def test_a_complex_with_two_marked_cells():
    """The batch keeps the mask and has no target rows (the model then takes x[mask] literally); a packed dataset, which carries
    one row per complex, refuses it."""
    cxs = _two_marks()
    b = ComplexBatch.from_complex_list(cxs)
    assert b.nodes.mask.nonzero().flatten().tolist() == [0, 5, 8, 10]
    assert b.target_rows(0) is None
    none = ComplexBatch.from_complex_list([Complex(Cochain(dim=0, x=torch.zeros(3, 2), mask=torch.zeros(3, dtype=torch.bool)))])
    assert none.target_rows(0) is None
    with pytest.raises(ValueError, match='exactly one cell'):
        PackedComplexes(cxs, 'cpu')
    # a batch of complexes without masks carries neither
    plain = ComplexBatch.from_complex_list(synthetic.zinc_like_complexes(3, seed=0))
    assert plain.nodes.mask is None and plain.target_rows(0) is None and 'mask' not in plain.nodes.keys


def test_packed_dataset_carries_the_local_target_index():
    cxs = case_complexes('mixed')
    for cx, t in zip(cxs, (0, 7, 29, 3)):                # (marks other than vertex 0: first, middle, last)
        m = torch.zeros(cx.nodes.num_cells, dtype=torch.bool)
        m[t] = True
        cx.nodes.mask = m
    packed = PackedComplexes(cxs, 'cpu', with_csr=True)
    pk = packed.keys[0]['target']
    assert pk.data.dtype == torch.int32 and pk.data.tolist() == [0, 7, 29, 3]
    assert pk.op == _ffi.COLLATE_ADD32 and pk.length.tolist() == [1, 1, 1, 1] and pk.start.tolist() == [0, 1, 2, 3]
    assert PackedComplexes._ADD_ROW['target'] == 0       # + the complex's first vertex row
    assert packed.key_index(0, 'target') >= 0
    # = what the host collate computes
    order = [2, 0, 3, 1]
    b = ComplexBatch.from_complex_list([cxs[i] for i in order])
    first = np.concatenate([[0], np.cumsum([cxs[i].nodes.num_cells for i in order])[:-1]])
    assert b.target_rows(0).tolist() == (first + pk.data.numpy()[order]).tolist()
    assert b.target_rows(0).tolist() == b.nodes.mask.nonzero().flatten().tolist()


def test_from_arrays_refuses_a_target_outside_its_complex():
    cxs = synthetic.ring_transfer(6, 5, 5)
    packed = PackedComplexes(cxs, 'cpu')
    keys = [{k: (pk.data if k != 'x' else pk.data.reshape(-1, pk.width), pk.length, pk.has) for k, pk in packed.keys[d].items()
             if k != 'target'} for d in range(3)]
    args = ('cpu', 2, packed.dims, packed.n_cells, packed.has_cells, packed.n_up, packed.n_down)
    keys[0]['target'] = torch.tensor([0, 5, 2, 1, 0])
    ok = PackedComplexes.from_arrays(*args, keys)
    assert ok.keys[0]['target'].data.tolist() == [0, 5, 2, 1, 0]
    for bad in ([0, 6, 2, 1, 0], [0, 1, -1, 1, 0]):
        keys[0]['target'] = torch.tensor(bad)
        with pytest.raises(IndexError, match='outside its complex'):
            PackedComplexes.from_arrays(*args, keys)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'cwn_hip.h')).read()
    lib = _ffi.lib()
    for name in ('cwn_target_head_f32', 'cwn_target_head_bwd_f32', 'cwn_target_head_bwd_workspace_bytes'):
        assert re.search(rf'\b(int|size_t) {name}\s*\(', header), name
        assert name in _ffi.EXPORTS
        assert hasattr(lib, name)
    assert 'mp/ring_exp_models.py:61-64' in header
    assert lib.cwn_abi_version() == _ffi.ABI_VERSION == 24
    assert int(re.search(r'#define CWN_ABI_VERSION (\d+)', header).group(1)) == 24
    assert _ffi.TARGET_HEAD_MAX_H == int(re.search(r'#define CWN_TARGET_HEAD_MAX_H (\d+)', header).group(1)) == 512
    assert _ffi.TARGET_HEAD_MAX_K == int(re.search(r'#define CWN_TARGET_HEAD_MAX_K (\d+)', header).group(1)) == 64


P = 0x10000
FWD = ('x', 'N', 'ldx', 'target_row', 'C', 'W', 'bias', 'out', 'ldout', 'H', 'K', 'err', 'm_dev', 'stream')
FWD_GOOD = dict(x=P, N=100, ldx=64, target_row=2 * P, C=0, W=3 * P, bias=4 * P, out=5 * P, ldout=5, H=64, K=5, err=6 * P, m_dev=None,
                stream=None)
BWD = ('dl', 'lddl', 'x', 'N', 'ldx', 'target_row', 'C', 'W', 'dx', 'lddx', 'dW', 'db', 'H', 'K', 'ws', 'ws_bytes', 'm_dev', 'stream')
BWD_GOOD = dict(dl=P, lddl=5, x=2 * P, N=0, ldx=64, target_row=3 * P, C=0, W=4 * P, dx=None, lddx=64, dW=None, db=None, H=64, K=5,
                ws=None, ws_bytes=0, m_dev=None, stream=None)


def fwd(**kw):
    a = dict(FWD_GOOD, **kw)
    return _ffi.lib().cwn_target_head_f32(*[a[k] for k in FWD])


def bwd(**kw):
    a = dict(BWD_GOOD, **kw)
    return _ffi.lib().cwn_target_head_bwd_f32(*[a[k] for k in BWD])


def test_forward_argument_checks_precede_any_hip_call():
    assert fwd() == OK                                    # C == 0: nothing is launched
    assert fwd(bias=None, err=None, x=None, out=None, target_row=None) == OK
    for kw in (dict(H=0), dict(H=2), dict(H=62, ldx=64), dict(H=516, ldx=516), dict(K=0), dict(K=65, ldout=65), dict(N=-1), dict(C=-1),
               dict(W=None), dict(ldx=60), dict(ldout=4), dict(C=3, out=None), dict(C=3, target_row=None), dict(C=3, x=None)):
        assert fwd(**kw) == BAD_ARG, kw
    for kw in (dict(x=P + 4), dict(W=3 * P + 8), dict(ldx=66), dict(out=5 * P + 2), dict(target_row=2 * P + 2), dict(m_dev=P + 4),
               dict(bias=4 * P + 1)):
        assert fwd(**kw) == ALIGN, kw
    assert fwd(H=0, x=P + 4) == BAD_ARG                   # the shape checks come first
    assert fwd(H=512, ldx=512, K=64, ldout=64) == OK      # the widest served shape
    assert _ffi.target_head_served(64, 5) and _ffi.target_head_served(512, 64) and _ffi.target_head_served(4, 1)
    assert not any(_ffi.target_head_served(h, k) for h, k in ((5, 5), (516, 5), (64, 0), (64, 65), (0, 1)))


def test_backward_argument_checks_precede_any_hip_call():
    assert bwd() == OK                                    # neither gradient asked for: nothing is launched
    for kw in (dict(H=30), dict(K=65), dict(N=-1), dict(lddl=4), dict(dx=5 * P, lddx=60), dict(dx=5 * P, W=None), dict(db=6 * P),
               dict(dW=5 * P, ldx=60), dict(dx=2 * P), dict(dx=P), dict(C=2, dl=None), dict(C=2, target_row=None)):
        assert bwd(**kw) == BAD_ARG, kw
    ws = _ffi.lib().cwn_target_head_bwd_workspace_bytes
    assert ws(64, 64, 5) == 0 and ws(0, 64, 5) == 0 and ws(65, 64, 5) == 2 * (5 * 64 + 8) * 4 and ws(130, 160, 10) == 3 * (1600 + 12) * 4
    WORKSPACE = 3
    assert bwd(C=65, dW=5 * P, ws=None) == WORKSPACE and bwd(C=65, dW=5 * P, ws=7 * P, ws_bytes=ws(65, 64, 5) - 1) == WORKSPACE
    assert bwd(C=65, dW=5 * P, ws=7 * P + 4, ws_bytes=1 << 20) == ALIGN
    assert bwd(C=65, dx=None, dW=None, ws=None) == OK    # (no weight gradient: no workspace)
    for kw in (dict(dx=5 * P + 4), dict(dx=5 * P, lddx=66), dict(dW=5 * P + 8), dict(W=4 * P + 4), dict(m_dev=P + 4),
               dict(dW=5 * P, x=2 * P + 4), dict(dW=5 * P, ldx=66, H=64), dict(db=6 * P + 2, dW=5 * P)):
        assert bwd(**kw) == ALIGN, kw


# ---- the model and the op -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cob', [True, False])
def test_ring_sparse_cin_state_dict_matches_the_fixture(cob):
    g = load(G)
    st = state_dict(g, 'state')
    m = models.RingSparseCIN(5, 5, 3, 64, use_coboundaries=cob)
    ours = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert sorted(ours) == [str(k) for k in g[f'state_keys/cob{int(cob)}']]
    assert all(tuple(st[k].shape) == shape for k, shape in ours.items())
    m.load_state_dict({k: st[k] for k in ours})          # strict
    assert m.init_layer.in_features == m.init_layer.out_features == 5 and m.lin1.out_features == 5 and len(m.convs) == 3
    assert m.max_dim == 2 and m.nonlinearity == 'relu' and m.graph_norm is torch.nn.Identity
    assert repr(m) == 'RingSparseCIN'
    m.reset_parameters()


def test_target_head_refuses_cpu_tensors_and_has_its_switch():
    x, w = torch.zeros(4, 8), torch.zeros(3, 8)
    with pytest.raises(_ffi.CwnError):
        ops.target_head(x, torch.zeros(2, dtype=torch.int32), w)
    assert isinstance(ops.FUSED_TARGET_HEAD, bool)
    assert not ops.target_head_applies(x, torch.zeros(2, dtype=torch.int32), w, None)      # (CPU-shaped misuse: never the launch)
    src = open(os.path.join(ROOT, 'cwn_amd', 'ops.py')).read()
    assert "os.environ.get('CWN_FUSED_TARGET_HEAD') != '0'" in src
