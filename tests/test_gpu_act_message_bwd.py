"""The backward of the activated coboundary message on the device: cwn_aggregate_act_bwd_f32 / _f64
(csrc/cwn_aggregate_act_bwd.hip) behind ops.ACT_MESSAGE_BACKWARD, against the same computation in float64 torch on the CPU
(index_add_ over the entries, torch autograd for the gradients), exactly where the sums are integers, bit for bit against the
streams that exist, and under the models that take the route.

Gates are the project's own (tests/_product.gate): 1e-5 * max(1, |ref|_inf) in float32 and 1e-11 in float64.

One hand-built adjacency serves the kernel tests: 40 destination rows, 24 source cells, 20 shared cells, 529 entries in
shuffled order, its three index columns drawn so that EACH keying -- the destination rows, the source rows of t_src and the
shared-cell rows of t_aux -- has rows of 0, 1, 16, 17, 64, 65 and 300 entries: the lengths at which the fold changes path
(the entry-slot split above 16 on narrow widths, the whole-workgroup pass above CWN_LONG_ROW = 64)."""
import copy

import numpy as np
import pytest
import torch

from tests._product import gate, gate_nonfinite
from tests.test_gpu_act_message import _model_f32
from tests.test_gpu_f64_dense import _model, _sr_batch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
TOL = {F32: 1e-5, F64: 1e-11}
ACTS = ('id', 'relu', 'elu', 'tanh', 'sigmoid')
ACT_FN = {'id': lambda t: t, 'relu': torch.relu, 'elu': torch.nn.functional.elu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}
N_DST, N_SRC, N_COB = 40, 24, 20
SPECIAL = (0, 1, 16, 17, 64, 65, 300)              # rows 0..6 of every keying
N_ENTRIES = sum(SPECIAL) + 66


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


@pytest.fixture
def switch_on(monkeypatch):
    from cwn_amd import layers, ops
    monkeypatch.setattr(ops, 'ACT_MESSAGE_BACKWARD', True)
    monkeypatch.setattr(layers, 'FUSED_ACT_MESSAGE', True)


def _lengths(n, total=N_ENTRIES, special=SPECIAL):
    """`special` and then the remaining entries spread evenly over the remaining rows."""
    rest, k = total - sum(special), n - len(special)
    return list(special) + [rest // k + (1 if i < rest % k else 0) for i in range(k)]


class _Graph:
    """Explicit (dst, src, cob) columns of an adjacency, its plan, and the CPU reference of a stream over it."""

    def __init__(self, dst, src, cob, n_dst=N_DST, n_src=N_SRC, n_cob=N_COB):
        from cwn_amd.csr import Adjacency
        self.dst, self.src, self.cob = (torch.as_tensor(np.asarray(t)).long() for t in (dst, src, cob))
        self.n_dst, self.n_src, self.n_cob = n_dst, n_src, n_cob
        self.adj = Adjacency.from_index(torch.stack([self.src, self.dst]).to(DEV), n_dst, n_src,
                                        aux_index=self.cob.to(DEV), n_aux=n_cob)

    @classmethod
    def with_lengths(cls, seed, dst_len, src_len, cob_len, **kw):
        rng = np.random.default_rng(seed)
        cols = [rng.permutation(np.repeat(np.arange(len(l)), l)) for l in (dst_len, src_len, cob_len)]
        return cls(*cols, n_dst=len(dst_len), n_src=len(src_len), n_cob=len(cob_len), **kw)

    def only_sources(self, rows):
        """The entries whose source is in `rows`, in their order, the sources renumbered 0, 1, ...: (graph, entry numbers)."""
        new = {int(r): i for i, r in enumerate(rows)}
        keep = torch.tensor([e for e in range(self.src.numel()) if int(self.src[e]) in new], dtype=torch.long)
        src = torch.tensor([new[int(s)] for s in self.src[keep]], dtype=torch.long)
        return _Graph(self.dst[keep], src, self.cob[keep], self.n_dst, len(rows), self.n_cob), keep

    def reference(self, o, ib, act, g, with_self=True):
        """out = index_add_(act(A[src] + B[cob])) + (1 + eps) self_x in float64 on the CPU and, by torch autograd, the
        gradients of (A, B, self_x, eps) for the output gradient `g`."""
        A, self_x, eps = (o[k].detach().cpu().double().requires_grad_() for k in ('A', 'self_x', 'eps'))
        B = o['B_aux' if ib == 'aux' else 'B_perm'].detach().cpu().double().requires_grad_()
        msg = ACT_FN[act](A[self.src] + (B[self.cob] if ib == 'aux' else B))
        out = torch.zeros(self.n_dst, A.size(1), dtype=F64).index_add_(0, self.dst, msg)
        if with_self:
            out = out + (1.0 + eps) * self_x
        out.backward(g.detach().cpu().double())
        return out.detach(), [A.grad, B.grad] + ([self_x.grad, eps.grad] if with_self else [])


@pytest.fixture(scope='module')
def graph():
    g = _Graph.with_lengths(7, _lengths(N_DST), _lengths(N_SRC), _lengths(N_COB))
    for col, n in ((g.dst, N_DST), (g.src, N_SRC), (g.cob, N_COB)):
        assert torch.bincount(col, minlength=n)[:7].tolist() == list(SPECIAL) and col.numel() == N_ENTRIES
    return g


@pytest.fixture(scope='module')
def short_graph():
    """Every row of every keying has at most 16 entries: summed sequentially in CSR order by every kernel."""
    mk = lambda n, head: head + _lengths(n - len(head), 160 - sum(head), ())
    g = _Graph.with_lengths(12, mk(37, [0, 1, 16, 15]), mk(23, [16, 0, 1, 13]), mk(19, [1, 16, 0, 14]))
    for t in (g.adj.t_src, g.adj.t_aux, g.adj):
        assert int((t.rowptr[1:] - t.rowptr[:-1]).max()) == 16
    return g


def _operands(g, F, dtype, seed, integer_g=False):
    gen = torch.Generator().manual_seed(seed)
    mk = lambda n: torch.randn(n, F, generator=gen, dtype=F64).to(dtype).to(DEV)
    o = dict(A=mk(g.n_src), B_aux=mk(g.n_cob), B_perm=mk(g.dst.numel()), self_x=mk(g.n_dst),
             eps=torch.tensor([0.25], dtype=dtype, device=DEV), g=mk(g.n_dst))
    if integer_g:
        o['g'] = torch.randint(-4, 5, (g.n_dst, F), generator=gen).to(dtype).to(DEV)
    return o


def _leaves(o, ib, with_self=True):
    """Fresh leaf tensors (A, B, self_x, eps) of one stream."""
    keys = ('A', 'B_aux' if ib == 'aux' else 'B_perm') + (('self_x', 'eps') if with_self else ())
    return [o[k].detach().clone().requires_grad_() for k in keys]


def _stream(g, leaves, ib, act, F, **kw):
    from cwn_amd import ops
    A, B = leaves[:2]
    self_x, eps = (leaves[2], leaves[3]) if len(leaves) == 4 else (None, None)
    if act is None:
        return ops.Stream(adj=g.adj, n_dst=g.n_dst, width=F, A=A, B=B, ib_mode=ib, self_x=self_x, eps=eps, **kw)
    return ops.Stream(adj=g.adj, n_dst=g.n_dst, width=F, A=A, B=B, msg_op=ops.MSG_A_PLUS_B, ib_mode=ib, act=act, self_x=self_x,
                      eps=eps, **kw)


def _grads(g, o, cases, F, with_self=True):
    """[(out, [dA, dB, (dself, deps)])] of the activated streams `cases` = [(act, ib)] run in ONE aggregate_many call and
    one backward with the output gradient o['g'] for each."""
    from cwn_amd import ops
    leaves = [_leaves(o, ib, with_self) for _, ib in cases]
    outs = ops.aggregate_many([_stream(g, lv, ib, act, F) for lv, (act, ib) in zip(leaves, cases)])
    torch.autograd.backward(outs, [o['g']] * len(outs))
    return [(out.detach(), [t.grad for t in lv]) for out, lv in zip(outs, leaves)]


# ------------------------------------------------------------------------------------------------
# 1. against the CPU
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [1, 3, 6, 16, 64, 128, 200, 260])
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_gradients_against_cpu_autograd(graph, switch_on, dtype, F):
    o = _operands(graph, F, dtype, seed=F)
    cases = [(act, ib) for act in ACTS for ib in ('aux', 'perm')]
    for (act, ib), (out, grads) in zip(cases, _grads(graph, o, cases, F)):
        ref_out, ref = graph.reference(o, ib, act, o['g'])
        gate(out, ref_out, f'forward {dtype} F={F} {act} ib={ib}', tol=TOL[dtype])
        for name, got, want in zip(('dA', 'dB', 'dself_x', 'deps'), grads, ref):
            assert got is not None and got.dtype == dtype and got.shape == want.shape, (name, act, ib)
            gate(got, want, f'{name} {dtype} F={F} {act} ib={ib}', tol=TOL[dtype])


@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_an_activated_stream_next_to_a_plain_one(graph, switch_on, dtype):
    from cwn_amd import ops
    F = 6
    o = _operands(graph, F, dtype, seed=31)
    act_leaves = _leaves(o, 'aux')
    plain = [o['A'].detach().clone().requires_grad_(), None, o['self_x'].detach().clone().requires_grad_(),
             o['eps'].detach().clone().requires_grad_()]
    outs = ops.aggregate_many([ops.Stream(adj=graph.adj, n_dst=N_DST, width=F, A=plain[0], self_x=plain[2], eps=plain[3]),
                               _stream(graph, act_leaves, 'aux', 'elu', F)])
    torch.autograd.backward(outs, [o['g'], o['g']])
    _, ref = graph.reference(o, 'aux', 'elu', o['g'])
    for name, got, want in zip(('dA', 'dB', 'dself_x', 'deps'), [t.grad for t in act_leaves], ref):
        gate(got, want, f'activated stream beside a plain one: {name} {dtype}', tol=TOL[dtype])
    g64 = o['g'].cpu().double()
    dA = torch.zeros(N_SRC, F, dtype=F64).index_add_(0, graph.src, g64[graph.dst])
    gate(plain[0].grad, dA, f'plain MSG_A stream beside an activated one: dA {dtype}', tol=TOL[dtype])
    gate(plain[2].grad, 1.25 * g64, f'plain stream: dself_x {dtype}', tol=TOL[dtype])
    gate(plain[3].grad, (g64 * o['self_x'].cpu().double()).sum().reshape(1), f'plain stream: deps {dtype}', tol=TOL[dtype])


# ------------------------------------------------------------------------------------------------
# 2. exact: integer-valued g, act' in {0, 1} -- every partial sum is an integer
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [4, 64])
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_integer_gradients_are_exact_on_every_row_kind(graph, switch_on, dtype, F):
    o = _operands(graph, F, dtype, seed=40 + F, integer_g=True)
    cases = [(act, ib) for act in ('id', 'relu') for ib in ('aux', 'perm')]
    for (act, ib), (_, grads) in zip(cases, _grads(graph, o, cases, F, with_self=False)):
        _, ref = graph.reference(o, ib, act, o['g'], with_self=False)
        for name, got, want in zip(('dA', 'dB'), grads, ref):
            assert bool((want == want.round()).all())                    # integers ...
            if name == 'dA' or ib == 'aux':
                assert float(want.abs().max()) > 8                       # ... and sums of many
            assert torch.equal(got.cpu().double(), want), (name, act, ib, float((got.cpu().double() - want).abs().max()))


# ------------------------------------------------------------------------------------------------
# 3. bit for bit against the streams that exist; two runs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [16, 64])
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_relu_and_id_gradients_equal_the_existing_streams_bitwise(short_graph, switch_on, dtype, F):
    from cwn_amd import ops
    g = short_graph
    o = _operands(g, F, dtype, seed=3)
    for ib in ('aux', 'perm'):
        for act, op in (('relu', ops.MSG_RELU_A_PLUS_B), ('id', ops.MSG_A_PLUS_B)):
            (_, new), = _grads(g, o, [(act, ib)], F, with_self=False)
            old = _leaves(o, ib, with_self=False)
            out = ops.aggregate_many([_stream(g, old, ib, None, F, msg_op=op)])[0]
            out.backward(o['g'])
            assert torch.equal(new[0], old[0].grad), (act, ib, 'dA')
            assert torch.equal(new[1], old[1].grad), (act, ib, 'dB')


@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_two_runs_give_the_same_bits(graph, switch_on, dtype):
    F = 16
    o = _operands(graph, F, dtype, seed=8)
    cases = [(act, ib) for act in ACTS for ib in ('aux', 'perm')]
    one, two = _grads(graph, o, cases, F), _grads(graph, o, cases, F)
    for (act, ib), (_, a), (_, b) in zip(cases, one, two):
        for x, y in zip(a, b):
            assert torch.equal(x, y), (act, ib)


# ------------------------------------------------------------------------------------------------
# 4. a row's bits are its own
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [3, 64])
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_a_source_rows_gradient_does_not_depend_on_the_rest_of_the_launch(graph, switch_on, monkeypatch, dtype, F):
    """The source cells with 300, 65, 17, 1 and 0 entries: dA of those rows on the sub-adjacency that holds only their
    entries (in the same order) against the same rows inside the full graph, whose backward launch also carries seven
    descriptors of other widths and activations."""
    from cwn_amd import _ffi, ops
    rows = [SPECIAL.index(n) for n in (300, 65, 17, 1, 0)]
    sub, keep = graph.only_sources(rows)
    o = _operands(graph, F, dtype, seed=50 + F)
    o_sub = dict(o, A=o['A'][rows].contiguous(), B_perm=o['B_perm'][keep.to(DEV)].contiguous())
    others = [(_operands(graph, w, dtype, seed=w), act, ib) for w, act, ib in ((7, 'tanh', 'aux'), (200, 'sigmoid', 'aux'), (12, 'id', 'aux'))]
    seen = []
    real = _ffi.aggregate_act_bwd

    def spy(descs, device, dt=torch.float32):
        seen.append(len(descs))
        return real(descs, device, dt)
    monkeypatch.setattr(_ffi, 'aggregate_act_bwd', spy)
    for ib in ('aux', 'perm'):
        (_, alone), = _grads(sub, o_sub, [('elu', ib)], F, with_self=False)
        # the full graph: this stream (dA, and dB when B is per shared cell) + three streams of other widths (dA, dB each)
        lv = _leaves(o, ib, with_self=False)
        olv = [_leaves(oo, oib, with_self=False) for oo, _, oib in others]
        outs = ops.aggregate_many([_stream(graph, lv, ib, 'elu', F)] +
                                  [_stream(graph, l, oib, oact, int(oo['A'].size(1))) for l, (oo, oact, oib) in zip(olv, others)])
        torch.autograd.backward(outs, [o['g']] + [oo['g'] for oo, _, _ in others])
        assert seen[-1] == (8 if ib == 'aux' else 7), seen               # ONE call for all of them
        assert torch.equal(lv[0].grad[rows], alone[0]), ib
        assert not bool(lv[0].grad[rows[-1]].any())                      # the source nobody reads: zeros


# ------------------------------------------------------------------------------------------------
# 5. gradcheck
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ib', ['aux', 'perm'])
@pytest.mark.parametrize('act', ACTS)
def test_gradcheck(switch_on, act, ib):
    from cwn_amd import ops
    g = _Graph([0, 0, 1, 2, 2, 2, 4, 5, 5, 2], [0, 1, 1, 2, 0, 3, 3, 1, 2, 0], [0, 1, 2, 0, 1, 2, 0, 1, 2, 2], n_dst=6, n_src=4, n_cob=3)
    F = 3
    gen = torch.Generator().manual_seed(5)
    rnd = lambda n: torch.rand(n, F, generator=gen, dtype=F64)
    n_b = 3 if ib == 'aux' else 10
    A = 0.2 + 0.8 * rnd(4)                                   # in [0.2, 1]
    if act == 'relu':                                        # pre-activations at least 0.3 from the kink
        sign = torch.where(torch.arange(n_b).unsqueeze(1) % 2 == 0, 1.0, -1.0).double()
        B = torch.where(sign > 0, 0.2 + 0.8 * rnd(n_b), -1.3 - rnd(n_b))
    else:
        B = 2 * rnd(n_b) - 1
    ins = [t.to(DEV).requires_grad_() for t in (A, B, 2 * rnd(6) - 1, torch.tensor([0.25], dtype=F64))]

    def fn(A, B, self_x, eps):
        return ops.aggregate_many([ops.Stream(adj=g.adj, n_dst=6, width=F, A=A, B=B, msg_op=ops.MSG_A_PLUS_B, ib_mode=ib, act=act,
                                              self_x=self_x, eps=eps)])[0]
    assert torch.autograd.gradcheck(fn, ins)


# ------------------------------------------------------------------------------------------------
# 6. non-finite values
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_nonfinite_gradients_are_where_torch_puts_them(graph, switch_on, dtype, act):
    """A NaN row and a +Inf row in g, a NaN row in A: each gradient is non-finite exactly where float64 torch makes it so."""
    F = 6
    o = _operands(graph, F, dtype, seed=60)
    o['g'][5] = float('nan')
    o['g'][9] = float('inf')
    o['A'][8] = float('nan')
    for ib in ('aux', 'perm'):
        (_, grads), = _grads(graph, o, [(act, ib)], F)
        _, ref = graph.reference(o, ib, act, o['g'])
        for name, got, want in zip(('dA', 'dB', 'dself_x'), grads, ref):
            gate_nonfinite(got, want, f'{name} {dtype} {act} ib={ib}', tol=TOL[dtype])
        assert not bool(torch.isfinite(ref[3]).any()) and not bool(torch.isfinite(grads[3]).any())       # eps: one scalar


# ------------------------------------------------------------------------------------------------
# 7. models
# ------------------------------------------------------------------------------------------------
class _Launches:
    """Counts the descriptors handed to _ffi.aggregate_act / _ffi.aggregate_act_bwd and the calls of _ffi.gather_rows."""

    def __init__(self, monkeypatch):
        from cwn_amd import _ffi
        self.fwd = self.bwd = self.gathers = 0
        fwd, bwd, gather = _ffi.aggregate_act, _ffi.aggregate_act_bwd, _ffi.gather_rows

        def fwd_spy(descs, device, dtype=torch.float32):
            self.fwd += len(descs)
            return fwd(descs, device, dtype)

        def bwd_spy(descs, device, dtype=torch.float32):
            self.bwd += len(descs)
            return bwd(descs, device, dtype)

        def gather_spy(*a, **kw):
            self.gathers += 1
            return gather(*a, **kw)
        monkeypatch.setattr(_ffi, 'aggregate_act', fwd_spy)
        monkeypatch.setattr(_ffi, 'aggregate_act_bwd', bwd_spy)
        monkeypatch.setattr(_ffi, 'gather_rows', gather_spy)

    def reset(self):
        self.fwd = self.bwd = self.gathers = 0


def _zinc_batch():
    from cwn_amd.synthetic import zinc_like_batch
    b = zinc_like_batch(8, seed=2).to(DEV)
    # SparseCIN takes features as given: rings without any get ones
    b.set_xs([c.x if c.x is not None else torch.ones(c.num_cells, 1, device=DEV) for c in (b.cochains[d] for d in range(3))])
    return b


def _loss_and_grads(model, batch):
    """MSE of the prediction against a fixed target; (loss, {name: grad} with the vertex features' as 'x0')."""
    x0 = batch.cochains[0].x.detach().clone().requires_grad_()
    batch.set_xs([x0] + [batch.cochains[d].x for d in range(1, batch.dimension + 1)])
    model.zero_grad(set_to_none=True)
    out = model(batch)
    target = torch.linspace(-1, 1, out.numel(), dtype=out.dtype, device=out.device).reshape(out.shape)
    loss = torch.nn.functional.mse_loss(out, target)
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    grads['x0'] = x0.grad.detach().clone()
    return loss.detach(), grads


MODELS = {
    'f64-elu': (lambda: _model(16, 2, 'elu', 'id'), lambda: _sr_batch().to(DEV), F64),
    'f64-tanh': (lambda: _model(16, 2, 'tanh', 'id'), lambda: _sr_batch().to(DEV), F64),
    'f64-sigmoid': (lambda: _model(16, 2, 'sigmoid', 'id'), lambda: _sr_batch().to(DEV), F64),
    'f64-id': (lambda: _model(16, 2, 'id', 'id'), lambda: _sr_batch().to(DEV), F64),
    'f32-h16-elu': (lambda: _model_f32('SparseCIN', 16, 'elu'), _zinc_batch, F32),
    'f32-h64-elu': (lambda: _model_f32('SparseCIN', 64, 'elu'), _zinc_batch, F32),
    'f32-h16-tanh': (lambda: _model_f32('SparseCIN', 16, 'tanh'), _zinc_batch, F32),
    'f32-cinpp-elu': (lambda: _model_f32('CINpp', 16, 'elu'), _zinc_batch, F32),
}


@pytest.mark.parametrize('which', sorted(MODELS))
def test_model_gradients_route_on_against_off(monkeypatch, which):
    from cwn_amd import layers, ops
    make_model, make_batch, dtype = MODELS[which]
    model = make_model()
    spy = _Launches(monkeypatch)
    monkeypatch.setattr(layers, 'FUSED_ACT_MESSAGE', True)
    monkeypatch.setattr(ops, 'ACT_MESSAGE_BACKWARD', False)
    loss_off, off = _loss_and_grads(model, make_batch())
    assert spy.fwd == 0 and spy.bwd == 0 and spy.gathers > 0             # the generic propagate: row gathers, neither kernel
    spy.reset()
    monkeypatch.setattr(ops, 'ACT_MESSAGE_BACKWARD', True)
    loss_on, on = _loss_and_grads(model, make_batch())
    # two layers, two dimensions with an upper adjacency each: a forward descriptor each, dA and dB behind it
    assert spy.fwd >= 4 and spy.bwd >= 4, (spy.fwd, spy.bwd)
    assert spy.gathers == 0                                              # no row gather for the up stream (nor elsewhere)
    gate(loss_on, loss_off, f'{which}: loss, route on vs off', tol=TOL[dtype])
    assert set(on) == set(off) and any('msg_up_nn' in k for k in on)
    for k in sorted(off):
        gate(on[k], off[k], f'{which}: d{k}, route on vs off', tol=TOL[dtype])


@pytest.mark.parametrize('which', ['f64-elu', 'f32-h16-elu'])
def test_three_adam_steps_lower_the_loss_on_both_routes(monkeypatch, which):
    from cwn_amd import layers, ops
    make_model, make_batch, dtype = MODELS[which]
    monkeypatch.setattr(layers, 'FUSED_ACT_MESSAGE', True)
    first = make_model()
    losses = {}
    for on in (False, True):
        monkeypatch.setattr(ops, 'ACT_MESSAGE_BACKWARD', on)
        model = copy.deepcopy(first)
        # (sum readouts over hundreds of cells: a step of 2e-5 per weight moves the prediction by about a tenth of its error)
        opt = torch.optim.Adam(model.parameters(), lr=2e-5)
        batch = make_batch()
        x0 = [batch.cochains[d].x for d in range(batch.dimension + 1)]

        def forward():
            batch.set_xs(x0)                                             # (the model's layers write their outputs into the batch)
            return model(batch)
        with torch.no_grad():
            out0 = forward()
        target = out0 + torch.linspace(-1, 1, out0.numel(), dtype=out0.dtype, device=out0.device).reshape(out0.shape)
        trace = []
        for _ in range(4):                                               # the loss before each of three steps, and after the last
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.mse_loss(forward(), target)
            trace.append(loss.detach())
            if len(trace) < 4:
                loss.backward()
                opt.step()
        losses[on] = torch.stack(trace)
        print(f'[adam] {which} switch {"on" if on else "off"}: {[float(v) for v in trace]}')
        assert float(trace[-1]) < float(trace[0])
    gate(losses[True], losses[False], f'{which}: losses over three Adam steps, route on vs off', tol=TOL[dtype])


# ------------------------------------------------------------------------------------------------
# 8. off means off
# ------------------------------------------------------------------------------------------------
def test_default_is_off():
    import os
    from cwn_amd import ops
    assert ops.ACT_MESSAGE_BACKWARD is (os.environ.get('CWN_ACT_MESSAGE_BACKWARD') == '1')


@pytest.mark.parametrize('which', ['f64-elu', 'f32-h16-elu', 'f32-cinpp-elu'])
def test_switch_off_records_autograd_without_either_kernel(monkeypatch, which):
    from cwn_amd import layers, ops
    make_model, make_batch, _ = MODELS[which]
    monkeypatch.setattr(ops, 'ACT_MESSAGE_BACKWARD', False)
    monkeypatch.setattr(layers, 'FUSED_ACT_MESSAGE', True)
    spy = _Launches(monkeypatch)
    model = make_model()
    out = model(make_batch())
    assert out.requires_grad
    out.sum().backward()
    assert spy.fwd == 0 and spy.bwd == 0
    assert model.convs[0].mp_levels[0].msg_up_nn[1].weight.grad is not None


def test_switch_off_refuses_the_gradient(graph, monkeypatch):
    from cwn_amd import ops
    monkeypatch.setattr(ops, 'ACT_MESSAGE_BACKWARD', False)
    o = _operands(graph, 6, F32, seed=6)
    with pytest.raises(NotImplementedError, match='inference only'):
        ops.aggregate_many([_stream(graph, _leaves(o, 'aux'), 'aux', 'elu', 6)])
