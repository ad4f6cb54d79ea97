"""The float64 path on the GPU: cwn_aggregate_f64 / cwn_gather_rows_f64 (csrc/cwn_aggregate_f64.hip) bit-exact against
float64 CPU references, torch.autograd.gradcheck over the hand-written backward rules of cwn_amd.ops (the first check of
them that needs no oracle), whole models in double against the float64 oracle, and the strongly-regular-graph configuration
(exp/test_sr.py of the reference: SparseCIN, ELU, no norm, sum readouts, float64 by default)."""
import copy

import numpy as np
import pytest
import torch

from oracle import cwn_oracle as O
from tests._golden import load, T, dummy_complex as o_complex, state_dict
from tests._product import dummy_complex, dummy_batch, list_names, gate, to_double

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F64 = torch.float64


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


def cpu(t):
    return None if t is None else t.detach().cpu()


# ------------------------------------------------------------------------------------------------
# 1. aggregate, exact
# ------------------------------------------------------------------------------------------------
N_DST, N_SRC, N_AUX = 37, 29, 23
WIDTHS = [1, 3, 8, 14, 16, 64, 127, 128, 130, 192]       # one lane per row, VEC 1, narrow, first non-narrow, a wave per row, two chunks


def _coo(lens, seed):
    """A shuffled COO index with the given entries per destination row (+ a shared-cell index)."""
    g = torch.Generator().manual_seed(seed)
    dst = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens))
    dst = dst[torch.randperm(dst.numel(), generator=g)]
    src = torch.randint(0, N_SRC, (dst.numel(),), generator=g)
    aux = torch.randint(0, N_AUX, (dst.numel(),), generator=g)
    return torch.stack([src, dst]), aux


# the edges of the 4-way unroll, one row above kSplitRow (16), one above CWN_LONG_ROW (64) -- all among the first 20 rows
LENS = [0, 1, 3, 4, 5, 17, 70] + [2, 6, 0, 3, 1, 5, 4, 2, 0, 6, 3, 1, 2, 5, 0, 4, 6, 1, 3, 2, 0, 5, 4, 1, 6, 2, 3, 0, 1, 4]
assert len(LENS) == N_DST


@pytest.fixture(scope='module')
def plan():
    from cwn_amd.csr import Adjacency
    idx, aux = _coo(LENS, 1234)
    adj = Adjacency.from_index(idx.to(DEV), N_DST, N_SRC, aux.to(DEV), N_AUX)
    assert adj.long_row_list().tolist() == [6]            # the 70-entry row goes to the whole-workgroup pass
    short = copy.copy(adj)                                # the same plan without its long-row list: one lane group walks the row
    short.long_rows = short.n_long = None
    return idx, aux, adj, short


def _ints(g, *shape, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def _message(op, a, b, pre):
    from cwn_amd import ops
    return {ops.MSG_A: lambda: a, ops.MSG_A_PLUS_B: lambda: a + b, ops.MSG_A_TIMES_B: lambda: a * b,
            ops.MSG_RELU_A_PLUS_B: lambda: torch.relu(a + b), ops.MSG_A_MASK_RELU: lambda: a * ((pre + b) > 0),
            ops.MSG_RELU_A_PLUS_B_SQ: lambda: torch.relu(a + b) ** 2,
            ops.MSG_A_TIMES_2RELU: lambda: 2 * a * torch.relu(pre + b)}[op]()


def _run(adj, op, red, A, B, pre, sx, eps):
    """One descriptor through the public stream API, or (the two backward-only messages) through a raw spec."""
    from cwn_amd import ops, _ffi
    d = lambda t: None if t is None else t.to(DEV)
    if op in (ops.MSG_A_MASK_RELU, ops.MSG_A_TIMES_2RELU):
        spec = ops.AggSpec(adj=adj, n_dst=N_DST, F=A.size(1), A=d(A), ia=adj.col, B=d(B), ib=adj.aux, msg_op=op,
                           reduce=_ffi.REDUCE[red], self_x=d(sx), eps=d(eps), self_pre=d(pre))
        return ops.run_aggregate([spec], torch.device(DEV))[0]
    return ops.aggregate(adj, N_DST, d(A), msg_op=op, B=None if op == ops.MSG_A else d(B), reduce=red, self_x=d(sx), eps=d(eps))


@pytest.mark.parametrize('F', WIDTHS)
def test_aggregate_every_message_and_reduce_exact(plan, F):
    """Integer-valued doubles in [-8, 8]: every sum and product is exact, so every message form x legal reduce equals the
    float64 CPU evaluation of the formula bit for bit -- with and without the long-row list, and with A an 8-byte-aligned
    view (one double per lane)."""
    from cwn_amd import ops
    idx, aux, adj, short = plan
    g = torch.Generator().manual_seed(F)
    A, B, B1 = _ints(g, N_SRC, F), _ints(g, N_AUX, F), _ints(g, N_AUX, 1)
    pre, sx = _ints(g, N_DST, F), _ints(g, N_DST, F, lo=-3, hi=3)
    eps = torch.tensor([0.25], dtype=F64)
    flat = torch.zeros(N_SRC * F + 1, dtype=F64, device=DEV)
    flat[1:] = A.flatten().to(DEV)
    A_view = flat[1:].view(N_SRC, F)                      # contiguous, 8 bytes off the allocation's 16-byte alignment
    assert A_view.is_contiguous() and A_view.data_ptr() % 16 == 8
    for op in range(7):
        for red in (('add', 'mean', 'max') if op < ops.MSG_RELU_A_PLUS_B else ('add',)):
            for Bm in ((B, B1) if op == ops.MSG_A_TIMES_B else (B,)):
                m = _message(op, A[idx[0]], Bm[aux], pre[idx[1]])
                want = O.scatter_rows(m, idx[1], N_DST, red) + 1.25 * sx
                for which, a_op, p in (('long rows', A, adj), ('lane groups only', A, short), ('8-byte view', A_view, adj)):
                    got = _run(p, op, red, a_op, Bm, pre, sx, eps)
                    assert got.dtype == F64
                    assert torch.equal(cpu(got), want), (F, op, red, which, int(Bm.size(1)))
    # an absent adjacency: zeros + the self term
    got = ops.aggregate(None, N_DST, None, self_x=sx.to(DEV), eps=eps.to(DEV), width=F)
    assert got.dtype == F64 and torch.equal(cpu(got), 1.25 * sx)


def test_aggregate_per_entry_operands_exact(plan):
    """ia_mode / ib_mode 'perm': one operand row per ENTRY (the output of a message hook, a materialised up_attr)."""
    from cwn_amd import ops
    idx, aux, adj, _ = plan
    g = torch.Generator().manual_seed(5)
    E, F = idx.size(1), 16
    A, B = _ints(g, E, F), _ints(g, E, F)
    for op in (ops.MSG_A, ops.MSG_A_PLUS_B, ops.MSG_A_TIMES_B, ops.MSG_RELU_A_PLUS_B, ops.MSG_RELU_A_PLUS_B_SQ):
        want = O.scatter_rows(_message(op, A, B, None), idx[1], N_DST, 'add')
        got = ops.aggregate(adj, N_DST, A.to(DEV), msg_op=op, B=None if op == ops.MSG_A else B.to(DEV), ia_mode='perm', ib_mode='perm')
        assert torch.equal(cpu(got), want), op


def test_aggregate_many_takes_two_launches_beyond_eight_streams(plan):
    from cwn_amd import ops
    idx, aux, adj, _ = plan
    g = torch.Generator().manual_seed(9)
    streams, want = [], []
    for k, F in enumerate([1, 3, 8, 14, 16, 64, 127, 128, 130, 16]):
        A, B = _ints(g, N_SRC, F), _ints(g, N_AUX, F)
        op = (ops.MSG_A, ops.MSG_A_PLUS_B, ops.MSG_RELU_A_PLUS_B)[k % 3]
        red = ('add', 'mean', 'max')[k % 3] if op != ops.MSG_RELU_A_PLUS_B else 'add'
        streams.append(ops.Stream(adj=adj, n_dst=N_DST, width=F, A=A.to(DEV), B=None if op == ops.MSG_A else B.to(DEV),
                                  msg_op=op, reduce=red))
        want.append(O.scatter_rows(_message(op, A[idx[0]], B[aux], None), idx[1], N_DST, red))
    assert len(streams) > 8
    for k, (got, ref) in enumerate(zip(ops.aggregate_many(streams), want)):
        assert got.dtype == F64 and torch.equal(cpu(got), ref), k


def test_one_call_mixes_a_float32_and_a_float64_stream(plan):
    from cwn_amd import ops
    idx, aux, adj, _ = plan
    g = torch.Generator().manual_seed(10)
    A = _ints(g, N_SRC, 16)
    o32, o64 = ops.aggregate_many([ops.Stream(adj=adj, n_dst=N_DST, width=16, A=A.float().to(DEV)),
                                   ops.Stream(adj=adj, n_dst=N_DST, width=16, A=(A * 3).to(DEV))])
    want = O.scatter_rows(A[idx[0]], idx[1], N_DST, 'add')
    assert o32.dtype == torch.float32 and o64.dtype == F64
    assert torch.equal(cpu(o32), want.float()) and torch.equal(cpu(o64), 3 * want)


def test_device_side_row_count_leaves_the_rows_past_it_untouched(plan):
    """m_dev: n_dst is the capacity, *m_dev the rows that exist; rows past it keep what the output held."""
    from cwn_amd import ops, _ffi
    idx, aux, adj, _ = plan
    g = torch.Generator().manual_seed(11)
    live = 20
    for F in (3, 16, 130):
        A, sx = _ints(g, N_SRC, F), _ints(g, N_DST, F)
        want = O.scatter_rows(A[idx[0]], idx[1], N_DST, 'add') + sx
        out = torch.full((N_DST, F), -77.0, dtype=F64, device=DEV)
        n = torch.tensor([live], dtype=torch.int64, device=DEV)
        spec = ops.AggSpec(adj=adj, n_dst=N_DST, F=F, A=A.to(DEV), ia=adj.col, self_x=sx.to(DEV), out=out)
        with _ffi.dynamic_rows({N_DST: n.data_ptr()}):
            ops.run_aggregate([spec], torch.device(DEV))
        assert torch.equal(cpu(out)[:live], want[:live]), F
        assert bool((cpu(out)[live:] == -77.0).all()), F


@pytest.mark.parametrize('F,lens', [(F, 'wide') for F in (16, 64, 127, 128, 130)] + [(F, 'narrow') for F in (1, 3, 8, 14)])
def test_real_valued_add_is_bit_identical_to_a_sequential_index_add(F, lens):
    """The project's bar: 'add' sums in entry order -- bit-identical to a sequential float64 index_add_ on rows the lane
    group walks alone: up to CWN_LONG_ROW entries, and up to kSplitRow = 16 for widths with fewer than 8 feature lanes
    (F <= 14), whose longer rows take the entry-parallel fold."""
    from cwn_amd import ops
    from cwn_amd.csr import Adjacency
    rows = [0, 1, 3, 4, 5, 17, 64, 33] if lens == 'wide' else [0, 1, 3, 4, 5, 16, 15, 9]
    rows = rows + [2, 6, 1, 5] * 7 + [3]
    assert len(rows) == N_DST
    idx, aux = _coo(rows, 77 + F)
    g = torch.Generator().manual_seed(F)
    A = torch.randn(N_SRC, F, generator=g, dtype=F64)
    sx = torch.randn(N_DST, F, generator=g, dtype=F64)
    adj = Adjacency.from_index(idx.to(DEV), N_DST, N_SRC, aux.to(DEV), N_AUX)
    got = ops.aggregate(adj, N_DST, A.to(DEV))
    want = torch.zeros(N_DST, F, dtype=F64).index_add_(0, idx[1], A[idx[0]])
    assert torch.equal(cpu(got), want)
    got = ops.aggregate(adj, N_DST, A.to(DEV), self_x=sx.to(DEV))
    assert torch.equal(cpu(got), want + 1.0 * sx)


# ------------------------------------------------------------------------------------------------
# 2. gather
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [1, 2, 3, 4, 8, 64, 127, 128, 130, 512])
def test_gather_rows_exact_in_double(F):
    from cwn_amd import ops
    g = torch.Generator().manual_seed(F)
    src = torch.randn(777, F, generator=g, dtype=F64)
    idx = torch.randint(0, 777, (5001,), generator=g)
    out = ops.gather_rows(src.to(DEV), idx.to(DEV))
    assert out.dtype == F64 and torch.equal(cpu(out), O.lift(src, idx))


def test_gather_rows_unaligned_view_and_empty_in_double():
    from cwn_amd import ops
    src = torch.randn(50, 9, device=DEV, dtype=F64)[:, 1:]          # non-contiguous view -> made contiguous
    idx = torch.tensor([3, 3, 49, 0], device=DEV)
    assert torch.equal(cpu(ops.gather_rows(src, idx)), cpu(src)[cpu(idx)])
    flat = torch.randn(50 * 8 + 1, device=DEV, dtype=F64)
    view = flat[1:].view(50, 8)                                     # contiguous, 8-byte aligned only: one double per lane
    assert view.data_ptr() % 16 == 8
    assert torch.equal(cpu(ops.gather_rows(view, idx)), cpu(view)[cpu(idx)])
    out = ops.gather_rows(torch.randn(5, 4, device=DEV, dtype=F64), torch.empty(0, dtype=torch.long, device=DEV))
    assert out.shape == (0, 4) and out.dtype == F64


# ------------------------------------------------------------------------------------------------
# 3. propagate on the dummy complexes
# ------------------------------------------------------------------------------------------------
def run_base(prm, **ctor):
    from cwn_amd.cell_mp import CochainMessagePassing
    w = prm.x.size(1)
    cmp = CochainMessagePassing(**dict(dict(up_msg_size=w, down_msg_size=w), **ctor))
    return cmp.propagate(prm.up_index, prm.down_index, prm.boundary_index, x=prm.x, up_attr=prm.kwargs['up_attr'],
                         down_attr=prm.kwargs['down_attr'], boundary_attr=prm.kwargs['boundary_attr'])


def _double_features(cx):
    for d in range(cx.dimension + 1):
        if cx.cochains[d].x is not None:
            cx.cochains[d].x = cx.cochains[d].x.double()
    return cx


ALL_NAMES = sorted(k[:-len('/dimension')] for k in load('dummy_complexes.npz') if k.endswith('/dimension'))


@pytest.mark.parametrize('name', ALL_NAMES)
def test_propagate_every_dummy_complex_in_double(name):
    cx = _double_features(dummy_complex(name, DEV))
    ocx = o_complex(name)
    for c in ocx['cochains']:
        c['x'] = None if c['x'] is None else c['x'].double()
    for d in range(cx.dimension + 1):
        if cx.cochains[d].x is None:
            continue
        op = O.cochain_params(ocx, d)
        w = op['x'].size(1)
        ref = O.propagate(op['x'], op['up_index'], op['down_index'], op['boundary_index'], up_attr=op['up_attr'],
                          down_attr=op['down_attr'], boundary_attr=op['boundary_attr'], up_msg_size=w, down_msg_size=w)
        for got, want, key in zip(run_base(cx.get_cochain_params(dim=d)), ref, ('up', 'down', 'boundary')):
            assert got.dtype == F64 and want.dtype == F64
            assert torch.equal(cpu(got), want), (name, d, key)


def test_house_known_answers_in_double():
    """mp/test_cell_mp.py:13-88."""
    h = _double_features(dummy_complex('house', DEV))
    up, down, bnd = run_base(h.get_cochain_params(dim=1))
    assert up.dtype == down.dtype == bnd.dtype == F64
    assert cpu(up).flatten().tolist() == [0, 0, 11, 0, 9, 8]
    assert cpu(down).flatten().tolist() == [6, 10, 17, 9, 13, 10]
    assert cpu(bnd).flatten().tolist() == [3, 5, 7, 5, 9, 8]
    up, down, bnd = run_base(h.get_cochain_params(dim=0))
    assert cpu(up).flatten().tolist() == [6, 4, 11, 9, 7]
    z = torch.zeros(5, 1, dtype=F64)
    assert torch.equal(cpu(down), z) and torch.equal(cpu(bnd), z)        # (absent streams: zero rows of the features' dtype)
    up, down, bnd = run_base(h.get_cochain_params(dim=2))
    z = torch.zeros(1, 1, dtype=F64)
    assert torch.equal(cpu(up), z) and torch.equal(cpu(down), z)
    assert cpu(bnd).flatten().tolist() == [14]


# ------------------------------------------------------------------------------------------------
# 4. gradcheck: the hand-written backward rules against finite differences
# ------------------------------------------------------------------------------------------------
G_DST, G_SRC, G_AUX, G_E, G_F = 6, 5, 4, 13, 3


@pytest.fixture(scope='module')
def gplan():
    from cwn_amd.csr import Adjacency
    g = torch.Generator().manual_seed(21)
    dst = torch.tensor([0, 0, 0, 0, 1, 2, 2, 2, 4, 4, 5, 5, 5])[torch.randperm(G_E, generator=g)]     # row 3 is empty
    src = torch.randint(0, G_SRC, (G_E,), generator=g)
    aux = torch.randint(0, G_AUX, (G_E,), generator=g)
    idx = torch.stack([src, dst])
    return idx, aux, Adjacency.from_index(idx.to(DEV), G_DST, G_SRC, aux.to(DEV), G_AUX)


def _distinct(g, rows):
    """[rows, G_F] doubles that are pairwise at least 0.05 apart: no ties under max, far more than gradcheck's 1e-6 step."""
    v = torch.randperm(rows * G_F, generator=g).to(F64) * 0.05 - 0.4
    return v.view(rows, G_F)


MODES = {'col': ('col', 'aux'), 'perm': ('perm', 'perm'), 'perm_aux': ('perm', 'aux'), 'col_perm': ('col', 'perm')}


def _away_from_zero(idx, aux, ia, ib, seed):
    """A (per source cell for ia 'col', per entry for 'perm') and B (per shared cell for ib 'aux', per entry for 'perm') with
    every pre-activation A + B at least 0.1 from the kink."""
    for s in range(seed, seed + 5000):
        g = torch.Generator().manual_seed(s)
        A = torch.randn(G_SRC if ia == 'col' else G_E, G_F, generator=g, dtype=F64)
        B = torch.randn(G_AUX if ib == 'aux' else G_E, G_F, generator=g, dtype=F64)
        pre = (A[idx[0]] if ia == 'col' else A) + (B[aux] if ib == 'aux' else B)
        if float(pre.abs().min()) >= 0.1 and bool((pre > 0).any()) and bool((pre < 0).any()):
            return A, B
    raise AssertionError('no operands found')


CASES = [('a', 'add'), ('a', 'mean'), ('a', 'max'), ('plus', 'add'), ('plus', 'mean'), ('times', 'add'), ('relu', 'add'), ('relu_sq', 'add')]


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('msg,red', CASES)
def test_gradcheck_aggregate(gplan, msg, red, mode):
    """torch.autograd.gradcheck with torch's defaults for double (eps 1e-6, atol 1e-5, rtol 1e-3) over ops.aggregate_many:
    gradients w.r.t. A, B, self_x and eps (A only for the multiplicative message, whose attribute has no fused gradient)."""
    from cwn_amd import ops
    idx, aux, adj = gplan
    op = {'a': ops.MSG_A, 'plus': ops.MSG_A_PLUS_B, 'times': ops.MSG_A_TIMES_B, 'relu': ops.MSG_RELU_A_PLUS_B,
          'relu_sq': ops.MSG_RELU_A_PLUS_B_SQ}[msg]
    g = torch.Generator().manual_seed(31)
    ia, ib = MODES[mode]
    if msg in ('relu', 'relu_sq'):
        A, B = _away_from_zero(idx, aux, ia, ib, 100)
    else:
        A = _distinct(g, G_SRC if ia == 'col' else G_E)
        B = torch.randn(G_AUX if ib == 'aux' else G_E, G_F, generator=g, dtype=F64)
    sx = torch.randn(G_DST, G_F, generator=g, dtype=F64)
    eps = torch.tensor([0.3], dtype=F64)
    A, sx, eps = (t.to(DEV).requires_grad_(True) for t in (A, sx, eps))
    B = B.to(DEV).requires_grad_(msg != 'times')
    modes = dict(ia_mode=ia, ib_mode=ib)

    def fn(A, B, sx, eps):
        return ops.aggregate_many([ops.Stream(adj=adj, n_dst=G_DST, width=G_F, A=A, B=None if op == ops.MSG_A else B, msg_op=op,
                                              reduce=red, self_x=sx, eps=eps, **modes)])[0]
    if op == ops.MSG_A:                    # (one operand: B is not an input)
        assert torch.autograd.gradcheck(lambda A, sx, eps: fn(A, None, sx, eps), (A, sx, eps))
    else:
        assert torch.autograd.gradcheck(fn, (A, B, sx, eps))


def test_gradcheck_gather_rows():
    from cwn_amd import ops
    g = torch.Generator().manual_seed(41)
    src = torch.randn(7, G_F, generator=g, dtype=F64).to(DEV).requires_grad_(True)
    idx = torch.tensor([3, 3, 6, 0, 1, 3, 5], device=DEV)          # row 2 and 4 are never read, row 3 three times
    assert torch.autograd.gradcheck(lambda s: ops.gather_rows(s, idx), (src,))


def test_gradcheck_propagate_with_a_custom_message_hook():
    from cwn_amd.cell_mp import CochainMessagePassing

    class Custom(CochainMessagePassing):
        def message_up(self, up_x_j, up_x_i, up_attr):
            return torch.tanh(up_x_j - up_x_i) * up_attr

        def message_boundary(self, boundary_x_j):
            return boundary_x_j ** 2

    h = dummy_complex('house', DEV)
    prm = h.get_cochain_params(dim=1)
    g = torch.Generator().manual_seed(51)
    E = prm.up_index.size(1)
    x = torch.randn(prm.x.size(0), G_F, generator=g, dtype=F64).to(DEV).requires_grad_(True)
    attr = torch.randn(E, G_F, generator=g, dtype=F64).to(DEV).requires_grad_(True)
    bx = torch.randn(h.cochains[0].num_cells, G_F, generator=g, dtype=F64).to(DEV).requires_grad_(True)
    layer = Custom(G_F, G_F)

    def fn(x, attr, bx):
        return layer.propagate(prm.up_index, prm.down_index, prm.boundary_index, x=x, up_attr=attr,
                               down_attr=None, boundary_attr=bx)
    assert torch.autograd.gradcheck(fn, (x, attr, bx))


# ------------------------------------------------------------------------------------------------
# 5. whole model against the float64 oracle
# ------------------------------------------------------------------------------------------------
def _oracle_cx(b):
    return {'dimension': b.dimension, 'y': None, 'num_complexes': b.num_complexes, 'cochains': [
        {k: cpu(b.cochains[d][k]) for k in ('x', 'upper_index', 'lower_index', 'shared_boundaries',
                                            'shared_coboundaries', 'boundary_index', 'y', 'batch')}
        for d in range(b.dimension + 1)]}


def _sr_batch(dtype=F64, graphs=None):
    """rook, Shrikhande and two random molecules, ring-lifted (rings up to 6), constant features."""
    from cwn_amd.complex import ComplexBatch
    from cwn_amd.synthetic import rook_4x4, shrikhande, random_molecule, sr_lift
    if graphs is None:
        rng = np.random.default_rng(3)
        graphs = [rook_4x4(), shrikhande(), random_molecule(rng), random_molecule(rng)]
    return ComplexBatch.from_complex_list([sr_lift(n, bonds, dtype=dtype) for n, bonds in graphs], max_dim=2)


@pytest.fixture(scope='module')
def sr_ref():
    """The batch's oracle form, computed once and shared (read-only)."""
    return _oracle_cx(_sr_batch())


@pytest.mark.parametrize('jump', [None, 'cat'])
@pytest.mark.parametrize('norm', ['id', 'bn'])
@pytest.mark.parametrize('hidden,layers', [(16, 3), (64, 2)])
def test_sparse_cin_in_double_vs_float64_oracle(sr_ref, hidden, layers, norm, jump):
    """SparseCIN.double() on double features against the oracle in float64 through the 1e-11 gate: well above what fp64
    re-association can leave (about K * 2^-53 per product), three orders below one accidental float32 intermediate (>= 6e-8).
    The same state in float32 still passes the project's 1e-5 gate: both dtypes run one model."""
    from cwn_amd.models import SparseCIN
    torch.manual_seed(hidden + layers)
    model = SparseCIN(1, 3, layers, hidden, dropout_rate=0.0, max_dim=2, jump_mode=jump, nonlinearity='relu', readout='sum',
                      use_coboundaries=True, graph_norm=norm).eval()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    ref, rpart = O.sparse_cin_model_forward(to_double(state), sr_ref, layers, use_coboundaries=True, norm=norm,
                                            jump_mode=jump, embed=None)
    for dtype, tol in ((F64, 1e-11), (torch.float32, 1e-5)):
        m = copy.deepcopy(model).to(dtype).to(DEV)
        b = _sr_batch(dtype).to(DEV)
        with torch.no_grad():
            y, res = m(b, include_partial=True)
        assert y.dtype == dtype
        worst = 0.0
        for k, v in rpart.items():
            assert res[k].dtype == dtype, k
            worst = max(worst, gate(res[k], v, f'SparseCIN {dtype} h{hidden} l{layers} {norm} jump={jump} {k}', tol=tol) /
                        max(1.0, float(v.abs().max())))
        worst = max(worst, gate(y, ref, f'SparseCIN {dtype} h{hidden} l{layers} {norm} jump={jump} prediction', tol=tol) /
                    max(1.0, float(ref.abs().max())))
        print(f'[gate] SparseCIN {dtype} h{hidden} l{layers} {norm} jump={jump}: worst relative deviation {worst:.3e}')


# ------------------------------------------------------------------------------------------------
# 6. the strongly-regular-graph configuration
# ------------------------------------------------------------------------------------------------
def _sr_model(layers, nonlinearity='elu'):
    from cwn_amd.models import SparseCIN
    return SparseCIN(num_input_features=1, num_classes=16, num_layers=layers, hidden=16, dropout_rate=0.0, max_dim=2,
                     use_coboundaries=True, nonlinearity=nonlinearity, graph_norm='id', readout='sum', final_readout='sum',
                     readout_dims=(0, 1, 2))


def test_sr_isomorphic_copies_land_within_the_reference_eps():
    """exp/test_sr.py:81-102: an untrained SparseCIN (ELU, no norm, hidden 16, 5 layers, sum readouts, coboundaries) under
    torch.set_default_dtype(float64) embeds a graph and its vertex-relabelled copies, each lifted on its own, within 0.01 of
    each other (torch.pdist, p = 2), with max |embedding| < 5e8."""
    from cwn_amd.synthetic import rook_4x4, shrikhande, relabel
    prev = torch.get_default_dtype()
    torch.set_default_dtype(F64)
    try:
        torch.manual_seed(0)
        model = _sr_model(5).to(DEV).eval()
        assert all(p.dtype == F64 for p in model.parameters())
        rng = np.random.default_rng(43)
        embs = []
        for graph in (rook_4x4(), shrikhande()):
            copies = [graph] + [relabel(*graph, rng.permutation(16)) for _ in range(3)]
            with torch.no_grad():
                out = model(_sr_batch(graphs=copies).to(DEV))
            assert out.dtype == F64 and out.shape == (4, 16)
            dist = torch.pdist(out, p=2)
            apex = float(out.abs().max())
            print(f'[sr] pdist over the 4 copies: max {float(dist.max()):.3e}   max|embedding| {apex:.4g}')
            assert float(dist.max()) <= 0.01
            assert apex < 5e8
            embs.append(out[0])
        print(f'[sr] rook vs Shrikhande: {float((embs[0] - embs[1]).norm()):.4g}')
    finally:
        torch.set_default_dtype(prev)


def test_sr_model_float32_follows_float64_at_two_layers():
    prev = torch.get_default_dtype()
    torch.set_default_dtype(F64)
    try:
        torch.manual_seed(1)
        model = _sr_model(2).eval()
    finally:
        torch.set_default_dtype(prev)
    with torch.no_grad():
        y64 = copy.deepcopy(model).to(DEV)(_sr_batch().to(DEV))
        y32 = copy.deepcopy(model).float().to(DEV)(_sr_batch(torch.float32).to(DEV))
    assert y64.dtype == F64 and y32.dtype == torch.float32
    gate(y32, y64, 'SR configuration, 2 layers: float32 run vs float64 run', tol=1e-5)


def test_sr_training_step_in_double_matches_oracle_autograd(sr_ref):
    """Forward, L1 loss to zeros, backward and one torch.optim.Adam step in float64 (relu / id, hidden 16, 2 layers): every
    parameter the loss reaches gets a finite float64 gradient equal to CPU autograd over the ORACLE's forward to
    1e-10 * max(1, |ref|_inf).  (The message network of the top dimension has no upper adjacency to run on: the loss does
    not reach it, here or in the oracle.)"""
    torch.manual_seed(2)
    model = _sr_model(2, 'relu').double().train()
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    leaves = {k: v.clone().requires_grad_(True) for k, v in state.items() if k in dict(model.named_parameters())}
    ostate = dict(state)
    ostate.update(leaves)
    ref_out, _ = O.sparse_cin_model_forward(ostate, sr_ref, 2, use_coboundaries=True, training=True, norm='id', embed=None)
    ref_loss = torch.nn.functional.l1_loss(ref_out, torch.zeros_like(ref_out))
    ref_loss.backward()
    model = model.to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    out = model(_sr_batch().to(DEV))
    loss = torch.nn.functional.l1_loss(out, torch.zeros_like(out))
    loss.backward()
    assert out.dtype == F64
    gate(loss.detach().view(1), ref_loss.detach().view(1), 'float64 training loss vs oracle', tol=1e-11)
    # the only parameters without a gradient: the message network of the top dimension, in every layer
    top = {f'convs.{l}.mp_levels.2.msg_up_nn.1.{w}' for l in range(2) for w in ('weight', 'bias')}
    assert {k for k, v in leaves.items() if v.grad is None} == top
    for name, p in model.named_parameters():
        if name in top:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        assert p.grad is not None and p.grad.dtype == F64 and bool(torch.isfinite(p.grad).all()), name
        gate(p.grad, leaves[name].grad, f'float64 grad {name}', tol=1e-10)
    before = [p.detach().clone() for p in model.parameters()]
    opt.step()
    assert all(bool(torch.isfinite(p).all()) and p.dtype == F64 for p in model.parameters())
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))


# ------------------------------------------------------------------------------------------------
# 7. the other layers and models
# ------------------------------------------------------------------------------------------------
def test_cin0_dummy_and_edge_orient_in_double_follow_their_float32_runs():
    from cwn_amd.complex import Cochain, CochainBatch
    from cwn_amd.models import CIN0, Dummy, EdgeOrient
    g = load('cin0_models.npz')

    def both(make, batch_of, tag):
        outs = []
        for dtype in (torch.float32, F64):
            model = make().to(dtype).to(DEV).eval()
            with torch.no_grad():
                y = model(batch_of(dtype))
            y = y[0] if isinstance(y, tuple) else y
            assert y.dtype == dtype, tag
            outs.append(y)
        gate(outs[0], outs[1], f'{tag}: float32 run vs float64 run', tol=1e-5)
        return outs[1]

    def complex_batch(tag):
        def make(dtype):
            b = dummy_batch(list_names('testing'), max_dim=2)
            for d in range(3):
                b.cochains[d].x = T(g[f'{tag}/x/{d}']).to(dtype)
            return b.to(DEV)
        return make

    def cin0():
        m = CIN0(8, 3, 2, 12, dropout_rate=0.0, max_dim=2, jump_mode='cat', nonlinearity='relu', readout='sum')
        m.load_state_dict(state_dict(g, 'cin0/state'))
        return m
    y = both(cin0, complex_batch('cin0'), 'CIN0')
    gate(y, T(g['cin0/eval/out']), 'CIN0 in double vs the reference fixture')

    def dummy():
        m = Dummy(1, 3, 2, max_dim=2, readout='sum')
        m.load_state_dict(state_dict(g, 'dummy/state'))
        return m
    y = both(dummy, complex_batch('dummy'), 'Dummy')
    gate(y, T(g['dummy/out']), 'Dummy in double vs the reference fixture')

    keys = ('x', 'upper_index', 'lower_index', 'upper_orient', 'lower_orient')
    edges = [Cochain(dim=1, **{k: T(g[f'orient/edges/{i}/{k}']) for k in keys}) for i in range(int(g['orient/n']))]

    def edge_batch(dtype):
        data = CochainBatch.from_cochain_list(edges)
        for k in keys + ('batch',):
            setattr(data, k, getattr(data, k).to(DEV))
        data.x = torch.cat([e.x for e in edges]).to(dtype).to(DEV)
        return data

    def orient():
        m = EdgeOrient(8, 2, 2, 12, dropout_rate=0.0, nonlinearity='id', readout='sum', fully_invar=False)
        m.load_state_dict(state_dict(g, 'orient/state'))
        return m
    y = both(orient, edge_batch, 'EdgeOrient')
    gate(y, T(g['orient/out']), 'EdgeOrient in double vs the reference fixture')


def test_cinpp_and_edge_cin0_in_double_follow_their_float32_runs():
    """The CIN++ layer with a real lower stream and the co-boundary stream (four fused streams; ReLU(Linear(cat)) messages up
    and down through torch products + the float64 aggregate), the CINpp model, and EdgeCIN0: double against float32."""
    from cwn_amd.layers import CINppConv
    from cwn_amd.models import CINpp, EdgeCIN0
    F = 8
    torch.manual_seed(0)
    conv = CINppConv(F, F, F, None, None, None, None, None, None, max_dim=2, hidden=F, act_module=torch.nn.ReLU,
                     layer_dim=F, use_coboundaries=True, feed_down_attr=True, coboundary_stream=True).eval()
    g = torch.Generator().manual_seed(4)
    base = dummy_batch(list_names('mol'), max_dim=2)
    xs = [torch.randn(base.cochains[d].num_cells, F, generator=g) for d in range(3)]
    outs = {}
    for dtype in (torch.float32, F64):
        b = dummy_batch(list_names('mol'), max_dim=2)
        for d in range(3):
            b.cochains[d].x = xs[d].to(dtype)
        b = b.to(DEV)
        with torch.no_grad():
            outs[dtype] = copy.deepcopy(conv).to(dtype).to(DEV)(*b.get_all_cochain_params(max_dim=2, include_down_features=True))
        assert all(o.dtype == dtype for o in outs[dtype])
    for d, (o32, o64) in enumerate(zip(outs[torch.float32], outs[F64])):
        gate(o32, o64, f'CINppConv (lower + co-boundary streams) dim {d}: float32 run vs float64 run', tol=1e-5)
    # with autograd recording: the same layer through the training-side branches
    b = dummy_batch(list_names('mol'), max_dim=2)
    for d in range(3):
        b.cochains[d].x = xs[d].double()
    b = b.to(DEV)
    m64 = copy.deepcopy(conv).double().to(DEV)
    og = m64(*b.get_all_cochain_params(max_dim=2, include_down_features=True))
    for d, (o, o64) in enumerate(zip(og, outs[F64])):
        gate(o, o64, f'CINppConv in double, autograd on vs off, dim {d}', tol=1e-11)
    sum(o.sum() for o in og).backward()
    assert all(p.grad is None or (p.grad.dtype == F64 and bool(torch.isfinite(p.grad).all())) for p in m64.parameters())
    assert sum(p.grad is not None for p in m64.parameters()) > 20

    torch.manual_seed(1)
    model = CINpp(F, 3, 2, 16, dropout_rate=0.0, max_dim=2, nonlinearity='relu', readout='sum', use_coboundaries=True,
                  graph_norm='bn').eval()
    ys = []
    for dtype in (torch.float32, F64):
        b = dummy_batch(list_names('mol'), max_dim=2)
        for d in range(3):
            b.cochains[d].x = xs[d].to(dtype)
        with torch.no_grad():
            ys.append(copy.deepcopy(model).to(dtype).to(DEV)(b.to(DEV)))
        assert ys[-1].dtype == dtype
    gate(ys[0], ys[1], 'CINpp model: float32 run vs float64 run', tol=1e-5)

    gg = load('cin0_models.npz')
    edge = EdgeCIN0(8, 3, 3, 12, dropout_rate=0.0, jump_mode=None, nonlinearity='relu', include_top_features=True,
                    update_top_features=True, readout='mean')
    edge.load_state_dict(state_dict(gg, 'edge/state'))
    b = dummy_batch(list_names('testing'), max_dim=2)
    for d in range(3):
        b.cochains[d].x = T(gg[f'edge/x/{d}']).double()
    with torch.no_grad():
        y = edge.double().to(DEV).eval()(b.to(DEV))
    assert y.dtype == F64
    gate(y, T(gg['edge/eval/out']), 'EdgeCIN0 in double vs the reference fixture')


def test_init_reduce_and_coboundary_stream_in_double():
    from cwn_amd.cell_mp import CochainMessagePassing
    from cwn_amd.layers import InitReduceConv
    h = _double_features(dummy_complex('house', DEV))
    p = [h.get_cochain_params(dim=d) for d in range(3)]
    out = InitReduceConv(reduce='add')(p[0].x, p[1].boundary_index)          # mp/test_layers.py:135-149
    assert out.dtype == F64 and cpu(out).flatten().tolist() == [3, 5, 7, 5, 9, 8]
    assert cpu(InitReduceConv(reduce='add')(p[1].x, p[2].boundary_index)).flatten().tolist() == [14]
    g = torch.Generator().manual_seed(7)
    vx = torch.randn(p[0].x.size(0), 5, generator=g, dtype=F64)
    for red in ('add', 'mean', 'max', 'min'):
        got = InitReduceConv(reduce=red)(vx.to(DEV), p[1].boundary_index, p[1].x.size(0))
        want = O.init_reduce(vx, cpu(p[1].boundary_index), red)
        assert got.dtype == F64
        if red == 'mean':
            torch.testing.assert_close(cpu(got), want, rtol=0, atol=1e-15)
        else:
            assert torch.equal(cpu(got), want), red
    # the co-boundary stream: exact on integers, adjoint to the boundary stream of the next dimension
    for name in ('house', 'bridged'):
        cx = dummy_complex(name, device=DEV)
        for d in range(cx.dimension):
            c, up = cx.cochains[d], cx.cochains[d + 1]
            n, n_up = c.num_cells, up.num_cells
            v = torch.randint(-4, 5, (n_up, 8), generator=g).to(F64).to(DEV)
            mp_ = CochainMessagePassing(8, 8)
            out = mp_.propagate_coboundary(up.boundary_index, v, n)
            bi = cpu(up.boundary_index)
            assert out.dtype == F64
            assert torch.equal(cpu(out), torch.zeros(n, 8, dtype=F64).index_add_(0, bi[0], cpu(v)[bi[1]])), (name, d)
            w = torch.randint(-4, 5, (n, 8), generator=g).to(F64).to(DEV)
            _, _, bnd = mp_.propagate(None, None, up.boundary_index, x=v, boundary_attr=w)
            assert float((out * w).sum()) == float((v * bnd).sum())


# ------------------------------------------------------------------------------------------------
# 8. refusals
# ------------------------------------------------------------------------------------------------
def test_mixed_and_half_operands_are_type_errors(plan):
    from cwn_amd import ops
    idx, aux, adj, _ = plan
    A = torch.zeros(N_SRC, 4, device=DEV)
    with pytest.raises(TypeError, match=r'float32.*float64|float64.*float32'):
        ops.aggregate(adj, N_DST, A.double(), msg_op=ops.MSG_A_PLUS_B, B=torch.zeros(N_AUX, 4, device=DEV))
    with pytest.raises(TypeError, match=r'float32.*float64|float64.*float32'):
        ops.aggregate(adj, N_DST, A, self_x=torch.zeros(N_DST, 4, device=DEV, dtype=F64))
    for bad in (torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match='float32 or float64'):
            ops.aggregate(adj, N_DST, A.to(bad))
        with pytest.raises(TypeError, match='float32 or float64'):
            ops.gather_rows(A.to(bad), torch.zeros(3, dtype=torch.long, device=DEV))
    # eps is a device scalar and follows the stream's dtype
    out = ops.aggregate(adj, N_DST, A.double() + 1, self_x=torch.ones(N_DST, 4, device=DEV, dtype=F64),
                        eps=torch.tensor([0.5], device=DEV))
    assert out.dtype == F64


def test_float32_only_machinery_refuses_a_double_model():
    """StaticForward / TrainStep (FlatAdam, captured graphs, the blocked launches) stay float32: a float64 model or batch is a
    TypeError that names the dtype, not a wrong result."""
    from cwn_amd.static_graph import StaticForward
    from cwn_amd.train import TrainStep
    model = _sr_model(2, 'relu').double().to(DEV)
    with pytest.raises(TypeError, match='float64'):
        StaticForward(model, None)                          # (refused on the model alone, before the batch is looked at)
    with pytest.raises(TypeError, match='float64'):
        TrainStep(model, [_sr_batch().to(DEV)])
    with pytest.raises(TypeError, match='float64'):
        TrainStep(_sr_model(2, 'relu').to(DEV), [_sr_batch().to(DEV)])
