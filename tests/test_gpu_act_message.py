"""The activated coboundary message on the device: cwn_aggregate_act_f32 / _f64 (csrc/cwn_aggregate_act.hip) against a CPU
reference, bit for bit against the streams that exist, and under the models that take it (layers.FUSED_ACT_MESSAGE).

Gates are the project's own (tests/_product.gate): float64 1e-11 * max(1, |ref|_inf) as tests/test_gpu_f64_dense.py, float32
1e-5 * max(1, |ref|_inf), the README's bar."""
import numpy as np
import pytest
import torch

from tests._product import gate
from tests.test_gpu_f64_dense import _model, _sr_batch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
TOL = {F32: 1e-5, F64: 1e-11}
ACTS = ('id', 'relu', 'elu', 'tanh', 'sigmoid')
ACT_FN = {'id': lambda t: t, 'relu': torch.relu, 'elu': torch.nn.functional.elu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}
N_DST, N_SRC, N_COB = 37, 23, 19
LENGTHS = (0, 1, 16, 17, 64, 65, 300)              # rows 0..6; the other 30 rows are short and random


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


class _Graph:
    """One hand-built adjacency: entries in shuffled order (so that the plan's permutation is not the identity), its plan,
    and the CPU copies the reference reads."""

    def __init__(self, lengths, seed, n_src=N_SRC, n_cob=N_COB, rows=None):
        from cwn_amd.csr import Adjacency
        rng = np.random.default_rng(seed)
        self.lengths = list(lengths)
        dst = np.repeat(np.arange(len(lengths)), lengths)
        order = rng.permutation(dst.size)
        self.dst = torch.from_numpy(dst[order]).long()
        self.src = torch.from_numpy(rng.integers(0, n_src, dst.size)).long()
        self.cob = torch.from_numpy(rng.integers(0, n_cob, dst.size)).long()
        self.n_dst = len(lengths)
        if rows is not None:                        # the entries of `rows` of another graph, in its order, as rows 0, 1, ...
            g, rows = rows
            keep = [torch.nonzero(g.dst == r).flatten() for r in rows]
            self.dst = torch.cat([torch.full_like(k, i) for i, k in enumerate(keep)])
            self.src, self.cob = torch.cat([g.src[k] for k in keep]), torch.cat([g.cob[k] for k in keep])
            self.entries = torch.cat(keep)          # their entry numbers in `g` (a per-entry B is cut by them)
        self.adj = Adjacency.from_index(torch.stack([self.src, self.dst]).to(DEV), self.n_dst, n_src,
                                        aux_index=self.cob.to(DEV), n_aux=n_cob)

    def reference(self, A, B, ib, act, self_x, eps):
        """index_add_ of act(A[src] + B[cob]) plus the self term, in float64 on the CPU."""
        A, B = A.detach().cpu().double(), B.detach().cpu().double()
        msg = ACT_FN[act](A[self.src] + (B[self.cob] if ib == 'aux' else B))
        out = torch.zeros(self.n_dst, A.size(1), dtype=F64).index_add_(0, self.dst, msg)
        if self_x is not None:
            out = out + (1.0 + (0.0 if eps is None else float(eps))) * self_x.detach().cpu().double()
        return out


@pytest.fixture(scope='module')
def graph():
    rng = np.random.default_rng(5)
    return _Graph(list(LENGTHS) + [int(v) for v in rng.integers(0, 12, N_DST - len(LENGTHS))], seed=6)


def _operands(g, F, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    mk = lambda n: torch.randn(n, F, generator=gen, dtype=F64).to(dtype).to(DEV)
    return dict(A=mk(N_SRC), B_aux=mk(N_COB), B_perm=mk(g.dst.numel()), self_x=mk(g.n_dst),
                eps=torch.tensor([0.25], dtype=dtype, device=DEV))


def _stream(g, ops_, ib, act, with_self, F, **kw):
    from cwn_amd import ops
    return ops.Stream(adj=g.adj, n_dst=g.n_dst, width=F, A=ops_['A'], B=ops_['B_aux'] if ib == 'aux' else ops_['B_perm'],
                      msg_op=ops.MSG_A_PLUS_B, ib_mode=ib, act=act, self_x=ops_['self_x'] if with_self else None,
                      eps=ops_['eps'] if with_self else None, **kw)


# ------------------------------------------------------------------------------------------------
# 1. the kernel against a CPU reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [1, 3, 16, 64, 128, 200, 12, 260])
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_kernel_against_cpu_reference(graph, dtype, F):
    """The widths of the issue, and two at which the code takes another path: 12 (float64: eight feature lanes of a
    16-lane group, the other eight lanes a second entry slot) and 260 (float32: more columns than one pass of 64 lanes x 4,
    the feature-chunk loop, which float64 enters at 200)."""
    from cwn_amd import ops
    o = _operands(graph, F, dtype, seed=F)
    cases = [(act, ib, ws) for act in ACTS for ib in ('aux', 'perm') for ws in (False, True)]
    # all twenty through aggregate_many: eight descriptors per launch
    outs = ops.aggregate_many([_stream(graph, o, ib, act, ws, F) for act, ib, ws in cases])
    for (act, ib, ws), out in zip(cases, outs):
        assert out.dtype == dtype and tuple(out.shape) == (N_DST, F)
        ref = graph.reference(o['A'], o['B_aux'] if ib == 'aux' else o['B_perm'], ib, act, o['self_x'] if ws else None,
                              o['eps'] if ws else None)
        gate(out, ref, f'aggregate_act {dtype} F={F} {act} ib={ib} self={ws}', tol=TOL[dtype])


# ------------------------------------------------------------------------------------------------
# 2. bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [16, 64])
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_relu_and_id_equal_the_existing_streams_bitwise(dtype, F):
    """Rows of at most 16 entries are summed sequentially in CSR order by both kernels."""
    from cwn_amd import ops
    rng = np.random.default_rng(11)
    g = _Graph([0, 1, 16, 15, 7] + [int(v) for v in rng.integers(0, 17, 32)], seed=12)
    o = _operands(g, F, dtype, seed=3)
    for ib in ('aux', 'perm'):
        B = o['B_aux'] if ib == 'aux' else o['B_perm']
        for act, op in (('relu', ops.MSG_RELU_A_PLUS_B), ('id', ops.MSG_A_PLUS_B)):
            new, again = ops.aggregate_many([_stream(g, o, ib, act, True, F), _stream(g, o, ib, act, True, F)])
            old = ops.aggregate(g.adj, g.n_dst, o['A'], msg_op=op, B=B, ib_mode=ib, self_x=o['self_x'], eps=o['eps'])
            assert torch.equal(new, old), (act, ib)
            assert torch.equal(new, again)
            bare = ops.aggregate_many([_stream(g, o, ib, act, False, F)])[0]
            assert torch.equal(bare, ops.aggregate(g.adj, g.n_dst, o['A'], msg_op=op, B=B, ib_mode=ib)), (act, ib)


@pytest.mark.parametrize('F', [1, 16, 64])
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_two_runs_and_a_rows_place_do_not_change_its_bits(graph, dtype, F):
    """The rows with 300, 17 and 1 entries: alone in a 3-row launch, inside the 37-row launch, and as the second of three
    descriptors of other widths and activations."""
    from cwn_amd import ops
    rows = [LENGTHS.index(300), LENGTHS.index(17), LENGTHS.index(1)]
    small = _Graph([300, 17, 1], seed=0, rows=(graph, rows))
    o = _operands(graph, F, dtype, seed=21)
    o3 = dict(o, B_perm=o['B_perm'][small.entries.to(DEV)].contiguous(), self_x=o['self_x'][rows].contiguous())
    for ib in ('aux', 'perm'):
        whole = ops.aggregate_many([_stream(graph, o, ib, 'elu', True, F)])[0]
        assert torch.equal(whole, ops.aggregate_many([_stream(graph, o, ib, 'elu', True, F)])[0])
        alone = ops.aggregate_many([_stream(small, o3, ib, 'elu', True, F)])[0]
        assert torch.equal(alone, whole[rows]), ib
        oa, ob = _operands(graph, 7, dtype, seed=1), _operands(graph, 200, dtype, seed=2)
        second = ops.aggregate_many([_stream(graph, oa, 'aux', 'tanh', False, 7), _stream(small, o3, ib, 'elu', True, F),
                                     _stream(graph, ob, 'perm', 'sigmoid', True, 200)])[1]
        assert torch.equal(second, alone), ib


# ------------------------------------------------------------------------------------------------
# 3. launches: eight descriptors in one, nine in two; the shapes without an adjacency
# ------------------------------------------------------------------------------------------------
class _Launches:
    """Counts the calls of the two C entry points and of ops.run_aggregate_act / ops.run_aggregate, and passes them on."""

    def __init__(self, monkeypatch):
        from cwn_amd import _ffi, ops
        self.c, self.act, self.plain, self.plain_ops = 0, 0, 0, []
        L = _ffi.lib()
        for name in ('cwn_aggregate_act_f32', 'cwn_aggregate_act_f64'):
            def spy(arr, n, s, fn=getattr(L, name)):
                self.c += 1
                assert 1 <= n <= 8
                return fn(arr, n, s)
            monkeypatch.setattr(L, name, spy)
        run_act, run = ops.run_aggregate_act, ops.run_aggregate

        def act_spy(specs, device):
            self.act += 1
            return run_act(specs, device)

        def plain_spy(specs, device):
            self.plain += 1
            self.plain_ops += [s.msg_op for s in specs]
            return run(specs, device)
        monkeypatch.setattr(ops, 'run_aggregate_act', act_spy)
        monkeypatch.setattr(ops, 'run_aggregate', plain_spy)

    def reset(self):
        self.c, self.act, self.plain, self.plain_ops = 0, 0, 0, []


@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_eight_descriptors_one_launch_nine_two_and_absent_adjacencies(graph, monkeypatch, dtype):
    from cwn_amd import ops
    from cwn_amd.csr import Adjacency
    F = 5
    o = _operands(graph, F, dtype, seed=9)
    spy = _Launches(monkeypatch)
    empty = Adjacency.from_index(torch.zeros(2, 0, dtype=torch.long, device=DEV), N_DST, N_SRC,
                                 aux_index=torch.zeros(0, dtype=torch.long, device=DEV), n_aux=N_COB)
    zero_rows = torch.zeros(0, F, dtype=dtype, device=DEV)

    def streams():
        mk = lambda **kw: ops.Stream(**{**dict(adj=None, n_dst=N_DST, width=F, msg_op=ops.MSG_A_PLUS_B, act='elu', dtype=dtype), **kw})
        return [_stream(graph, o, 'aux', 'elu', True, F),
                mk(adj=empty, A=o['A'], B=o['B_aux'], self_x=o['self_x'], eps=o['eps']),       # an adjacency without entries
                mk(self_x=o['self_x'], eps=o['eps']),                                           # rowptr = NULL, self term
                mk(),                                                                           # rowptr = NULL, nothing: zeros
                mk(n_dst=0, self_x=zero_rows),                                                  # no rows
                _stream(graph, o, 'perm', 'tanh', False, F), _stream(graph, o, 'aux', 'sigmoid', True, F),
                _stream(graph, o, 'perm', 'id', True, F), _stream(graph, o, 'aux', 'relu', False, F)]
    outs = ops.aggregate_many(streams())            # nine streams, eight of them with rows: eight descriptors
    assert spy.c == 1 and spy.act == 1 and spy.plain == 0
    self_term = 1.25 * o['self_x'].double().cpu()
    gate(outs[1], self_term, 'empty adjacency', tol=TOL[dtype])
    gate(outs[2], self_term, 'absent adjacency, self term', tol=TOL[dtype])
    assert outs[3].dtype == dtype and tuple(outs[3].shape) == (N_DST, F) and not bool(outs[3].any())
    assert tuple(outs[4].shape) == (0, F)
    gate(outs[0], graph.reference(o['A'], o['B_aux'], 'aux', 'elu', o['self_x'], o['eps']), 'first of eight', tol=TOL[dtype])
    gate(outs[7], graph.reference(o['A'], o['B_perm'], 'perm', 'id', o['self_x'], o['eps']), 'eighth of nine streams', tol=TOL[dtype])
    spy.reset()
    nine = ops.aggregate_many(streams() + [_stream(graph, o, 'aux', 'relu', True, F)])
    assert spy.c == 2 and spy.act == 1
    for a, b in zip(nine, outs):
        assert torch.equal(a, b)
    gate(nine[9], graph.reference(o['A'], o['B_aux'], 'aux', 'relu', o['self_x'], o['eps']), 'the ninth', tol=TOL[dtype])
    # streams with and without an activation in one call: one launch each, outputs in stream order
    spy.reset()
    mixed = ops.aggregate_many([ops.Stream(adj=graph.adj, n_dst=N_DST, width=F, A=o['A'], self_x=o['self_x'], eps=o['eps']),
                                _stream(graph, o, 'aux', 'elu', True, F),
                                ops.Stream(adj=None, n_dst=N_DST, width=F, self_x=o['self_x'], eps=o['eps'])])
    assert spy.act == 1 and spy.plain == 1 and spy.c == 1
    assert torch.equal(mixed[1], outs[0])
    gate(mixed[2], self_term, 'plain stream next to an activated one', tol=TOL[dtype])
    plain_ref = torch.zeros(N_DST, F, dtype=F64).index_add_(0, graph.dst, o['A'].double().cpu()[graph.src]) + self_term
    gate(mixed[0], plain_ref, 'plain gathered stream next to an activated one', tol=TOL[dtype])


def test_gradients_and_half_types_are_refused(graph):
    from cwn_amd import ops
    o = _operands(graph, 4, F32, seed=2)
    o['A'] = o['A'].requires_grad_()
    with pytest.raises(NotImplementedError, match='inference only'):
        ops.aggregate_many([_stream(graph, o, 'aux', 'elu', True, 4)])
    with torch.no_grad():
        ops.aggregate_many([_stream(graph, o, 'aux', 'elu', True, 4)])
    for dt in (torch.float16, torch.bfloat16):
        h = {k: v.detach().to(dt) for k, v in o.items()}
        with pytest.raises(TypeError):
            ops.aggregate_many([_stream(graph, h, 'aux', 'elu', True, 4)])


# ------------------------------------------------------------------------------------------------
# 4. float64 models
# ------------------------------------------------------------------------------------------------
def _on_off(monkeypatch, model, make_batch, tol, what):
    """model on a fresh batch with the route on and off; every include_partial entry and the prediction within the gate."""
    from cwn_amd import layers
    spy = _Launches(monkeypatch)
    with torch.no_grad():
        monkeypatch.setattr(layers, 'FUSED_ACT_MESSAGE', False)
        y_off, res_off = model(make_batch(), include_partial=True)
        assert spy.act == 0 and spy.c == 0
        spy.reset()
        monkeypatch.setattr(layers, 'FUSED_ACT_MESSAGE', True)
        y_on, res_on = model(make_batch(), include_partial=True)
    assert bool(torch.isfinite(y_on).all())
    for k, v in res_off.items():
        gate(res_on[k], v, f'{what}: route on vs off, {k}', tol=tol)
    gate(y_on, y_off, f'{what}: route on vs off, prediction', tol=tol)
    return spy


def test_sr_model_f64_route_on_matches_off_and_launches_once_per_layer(monkeypatch):
    spy = _on_off(monkeypatch, _model(16, 3, 'elu', 'id'), lambda: _sr_batch().to(DEV), 1e-11, 'SR SparseCIN f64 h16 elu')
    # every layer has two dimensions with an upper adjacency: their two streams in ONE launch per layer
    assert spy.act == 3 and spy.c == 3
    assert 3 not in spy.plain_ops                                    # no ReLU stream anywhere


@pytest.mark.parametrize('nonlinearity', ['tanh', 'sigmoid', 'id'])
def test_other_activations_f64_hidden_64_with_eval_batchnorm(monkeypatch, nonlinearity):
    spy = _on_off(monkeypatch, _model(64, 2, nonlinearity, 'bn'), lambda: _sr_batch().to(DEV), 1e-11,
                  f'SparseCIN f64 h64 {nonlinearity} bn')
    assert spy.act == 2 and spy.c == 2


def test_route_declined_f64(monkeypatch):
    from cwn_amd import layers, ops
    spy = _Launches(monkeypatch)
    monkeypatch.setattr(layers, 'FUSED_ACT_MESSAGE', True)
    # a recording autograd with trainable parameters: the path it had, and a gradient
    model = _model(16, 2, 'elu', 'id')
    assert torch.is_grad_enabled() and all(p.requires_grad for p in model.parameters())
    out = model(_sr_batch().to(DEV))
    assert out.requires_grad and spy.act == 0 and spy.c == 0
    out.sum().backward()
    assert model.convs[0].mp_levels[0].msg_up_nn[1].weight.grad is not None
    with torch.no_grad():
        # a message network of another form
        custom = _model(16, 2, 'elu', 'id')
        for conv in custom.convs:
            for lvl in conv.mp_levels:
                lvl.msg_up_nn[2] = torch.nn.Softplus()
        custom(_sr_batch().to(DEV))
        assert spy.act == 0 and spy.c == 0
        # ReLU keeps its own stream
        spy.reset()
        _model(16, 2, 'relu', 'id')(_sr_batch().to(DEV))
        assert spy.act == 0 and spy.c == 0 and spy.plain_ops.count(ops.MSG_RELU_A_PLUS_B) == 4


def test_sr_criterion_holds_on_the_route(monkeypatch):
    """exp/test_sr.py:81-102: relabelled copies of a graph, each lifted on its own, within 0.01 of each other (torch.pdist);
    the rook's graph and the Shrikhande graph more than 0.01 apart; no embedding beyond 5e8."""
    from cwn_amd import layers
    from cwn_amd.synthetic import rook_4x4, shrikhande, relabel
    monkeypatch.setattr(layers, 'FUSED_ACT_MESSAGE', True)
    model = _model(16, 3, 'elu', 'id', seed=0)
    spy = _Launches(monkeypatch)
    rng = np.random.default_rng(43)
    embs = []
    for g in (rook_4x4(), shrikhande()):
        copies = [g] + [relabel(*g, rng.permutation(16)) for _ in range(3)]
        with torch.no_grad():
            out = model(_sr_batch(copies).to(DEV))
        dist = torch.pdist(out, p=2)
        print(f'[sr] pdist over the 4 copies: max {float(dist.max()):.3e}   max|embedding| {float(out.abs().max()):.4g}')
        assert float(dist.max()) <= 0.01
        assert float(out.abs().max()) < 5e8
        embs.append(out[0])
    assert spy.act == 6
    apart = float((embs[0] - embs[1]).norm())
    print(f'[sr] rook vs Shrikhande: {apart:.4g}')
    assert apart > 0.01


# ------------------------------------------------------------------------------------------------
# 5. float32 models
# ------------------------------------------------------------------------------------------------
def _model_f32(kind, hidden, nonlinearity, layers_=2, seed=0):
    from cwn_amd import models
    torch.manual_seed(seed)
    m = getattr(models, kind)(num_input_features=1, num_classes=4, num_layers=layers_, hidden=hidden, dropout_rate=0.0, max_dim=2,
                              use_coboundaries=True, nonlinearity=nonlinearity, graph_norm='bn', readout='sum',
                              final_readout='sum', readout_dims=(0, 1, 2))
    return m.to(DEV).eval()


@pytest.mark.parametrize('nonlinearity', ['elu', 'tanh', 'sigmoid', 'id'])
@pytest.mark.parametrize('hidden', [16, 64])
@pytest.mark.parametrize('kind', ['SparseCIN', 'CINpp'])
def test_f32_models_route_on_matches_off(monkeypatch, kind, hidden, nonlinearity):
    model = _model_f32(kind, hidden, nonlinearity)
    spy = _on_off(monkeypatch, model, lambda: _sr_batch(dtype=F32).to(DEV), 1e-5, f'{kind} f32 h{hidden} {nonlinearity}')
    assert spy.act == 2 and spy.c == 2
    if hidden == 64:
        # the blocked launch declines the model as it did
        assert 'message network is not ReLU(Linear(cat))' in model.convs[1].blocked_reason


# ------------------------------------------------------------------------------------------------
# 6. hub rows: a REDDIT-like complex, rows beyond CWN_LONG_ROW through the whole-workgroup pass
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_hub_complex_route_on_matches_off(monkeypatch, dtype):
    from cwn_amd import models
    from cwn_amd.complex import ComplexBatch
    from cwn_amd.synthetic import reddit_like_complexes
    cs = reddit_like_complexes(2, seed=1, n_lo=150, n_hi=220)

    def batch():
        b = ComplexBatch.from_complex_list(cs, max_dim=2).to(DEV)
        b.set_xs([b.cochains[d].x.to(dtype) for d in range(b.dimension + 1)])
        return b
    b = batch()
    up = b.cochains[0].upper_index
    assert int(torch.bincount(up[1]).max()) > 64                     # a hub: a long row of the vertices' upper adjacency
    torch.manual_seed(0)
    model = models.SparseCIN(num_input_features=1, num_classes=2, num_layers=2, hidden=16, dropout_rate=0.0, max_dim=2,
                             use_coboundaries=True, nonlinearity='elu', graph_norm='id', readout='sum', final_readout='sum',
                             readout_dims=(0, 1, 2)).to(dtype).to(DEV).eval()
    spy = _on_off(monkeypatch, model, batch, TOL[dtype], f'REDDIT-like hub complex {dtype}')
    assert spy.act == 2
