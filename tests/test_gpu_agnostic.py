"""The message-passing-agnostic baseline on the device: cwn_embed_pool_* and cwn_agnostic_head_* (csrc/cwn_agnostic.hip)
against a float64 CPU evaluation, the invariance contract of include/cwn_hip.h bit for bit, and MessagePassingAgnostic
with the route on (models.FUSED_AGNOSTIC) against the reference-made fixture, against the route off, and as the control of
the strongly-regular-graph experiment.

Gates are the project's own (tests/_product.gate): float64 1e-11 * max(1, |ref|_inf) as tests/test_gpu_f64_dense.py, float32
1e-5 * max(1, |ref|_inf), the README's bar."""
import numpy as np
import pytest
import torch

from tests._golden import load, T
from tests._product import gate
from tests._agnostic import CASES, CONFIGS, DTYPES, TOL, case_batch, fixture_model, sr_complexes, G

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
ACTS = ('id', 'relu', 'elu', 'tanh', 'sigmoid')
ACT_FN = {'id': lambda t: t, 'relu': torch.relu, 'elu': torch.nn.functional.elu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}


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


def _chunk():
    from cwn_amd import _ffi
    return _ffi.EMBED_POOL_CHUNK


def _row_counts():
    """The rows per complex at which the kernel's order of summation changes shape."""
    c = _chunk()
    return [0, 1, c - 1, c, c + 1, 4 * c + 1]


class _Dim:
    """One descriptor's operands: CPU masters in the dtype under test (so the reference sees the rounded inputs), x a
    column slice of a wider matrix (ldx > K), W a column slice that does not start at column 0 (ldw > K)."""

    def __init__(self, dtype, rows, K, H, act, mean=False, bias=True, seed=0):
        g = torch.Generator().manual_seed(1000 * K + H + seed)
        self.rows, self.K, self.H, self.act, self.mean = list(rows), K, H, act, mean
        N = sum(rows)
        self.x_full = torch.randn(N, K + 3, generator=g, dtype=F64).to(dtype)
        self.w_full = (torch.randn(H, K + 2, generator=g, dtype=F64) / K ** 0.5).to(dtype)
        # (NaN beside both windows: a load that strays and is not discarded shows in the result)
        self.x_full[:, K:] = self.w_full[:, 0] = self.w_full[:, K + 1:] = float('nan')
        self.b = torch.randn(H, generator=g, dtype=F64).to(dtype) if bias else None
        self.ptr = torch.tensor(np.concatenate([[0], np.cumsum(rows)]).astype(np.int64))

    def device_operands(self):
        x = self.x_full.to(DEV)[:, :self.K]
        w = self.w_full.to(DEV)[:, 1:1 + self.K]
        if x.size(0) > 1:
            assert x.stride(0) > self.K
        if w.size(0) > 1:
            assert w.stride(0) > self.K
        return x, self.ptr.to(DEV), w, None if self.b is None else self.b.to(DEV)

    def reference(self):
        """sum (mean) over the rows of every complex of act(x @ W.T + b), in float64 on the CPU."""
        x, w = self.x_full[:, :self.K].double(), self.w_full[:, 1:1 + self.K].double()
        y = x @ w.t()
        if self.b is not None:
            y = y + self.b.double()
        y = ACT_FN[self.act](y)
        out = torch.zeros(len(self.rows), self.H, dtype=F64)
        for c in range(len(self.rows)):
            lo, hi = int(self.ptr[c]), int(self.ptr[c + 1])
            out[c] = y[lo:hi].sum(0)
            if self.mean:
                out[c] /= max(hi - lo, 1)
        return out


def _launch(dims, act=None, mean=None):
    """One call of ops.embed_pool over `dims` (they share act and mean: arguments of the call)."""
    from cwn_amd import ops
    operands = [d.device_operands() for d in dims]
    return ops.embed_pool([o[0] for o in operands], [o[1] for o in operands], len(dims[0].rows), [o[2] for o in operands],
                          [o[3] for o in operands], dims[0].act if act is None else act, mean=dims[0].mean if mean is None else mean)


def _check(dtype, dims, what):
    outs = _launch(dims)
    assert len(outs) == len(dims)
    for i, (d, out) in enumerate(zip(dims, outs)):
        assert out.dtype == dtype and tuple(out.shape) == (len(d.rows), d.H)
        gate(out, d.reference(), f'{what}, descriptor {i}: K = {d.K}, H = {d.H}, {d.act}, mean = {d.mean}', tol=TOL[dtype])
    return outs


@pytest.mark.parametrize('dtype', [F32, F64])
@pytest.mark.parametrize('K', [1, 3, 33, 128])
def test_embed_pool_widths(dtype, K):
    """Every K with every H; three descriptors in one launch, then one: rows per complex around the chunk boundaries."""
    rows = _row_counts()
    shuffled = [rows[i] for i in (5, 0, 3, 1, 4, 2)]
    _check(dtype, [_Dim(dtype, rows, K, 1, 'elu'), _Dim(dtype, shuffled, K, 16, 'elu'), _Dim(dtype, rows, K, 65, 'elu')],
           f'embed_pool {dtype}')
    _check(dtype, [_Dim(dtype, shuffled, K, 256, 'elu', bias=False)], f'embed_pool {dtype}, no bias')


@pytest.mark.parametrize('dtype', [F32, F64])
@pytest.mark.parametrize('mean', [False, True])
@pytest.mark.parametrize('act', ACTS)
def test_embed_pool_activations_and_readouts(dtype, act, mean):
    """All five activations, sum and mean, bias present and absent; the second descriptor has no row at all (N == 0)."""
    rows = _row_counts()
    outs = _check(dtype, [_Dim(dtype, rows, 3, 65, act, mean=mean), _Dim(dtype, [0] * len(rows), 3, 16, act, mean=mean),
                          _Dim(dtype, rows[::-1], 33, 16, act, mean=mean, bias=False)], f'embed_pool {dtype}')
    assert not outs[1].any()                                 # no row in that dimension: zero rows, mean included
    assert not outs[0][0].any() and not outs[2][-1].any()    # the complex without a row


@pytest.mark.parametrize('dtype', [F32, F64])
def test_embed_pool_no_complex_and_one_complex(dtype):
    out, = _launch([_Dim(dtype, [], 3, 16, 'tanh')])
    assert tuple(out.shape) == (0, 16)
    for n in _row_counts():
        _check(dtype, [_Dim(dtype, [n], 3, 65, 'tanh', seed=n)], f'embed_pool {dtype}, C = 1 with {n} rows')


def _head_reference(pooled, w1, b1, w2, b2, act):
    s = 0
    for p in pooled:
        z = (p.double() @ w1.double().t()) if p is not None else torch.zeros(1, w1.size(0), dtype=F64)
        if b1 is not None:
            z = z + b1.double()
        s = s + ACT_FN[act](z)                                # an absent dimension contributes act(b1)
    out = s @ w2.double().t()
    return out + b2.double() if b2 is not None else out


@pytest.mark.parametrize('dtype', [F32, F64])
@pytest.mark.parametrize('H,O,D,absent,bias,act', [(1, 1, 1, None, True, 'elu'), (17, 16, 3, 1, True, 'elu'), (256, 16, 3, None, True, 'elu'),
                                                  (256, 1, 1, None, False, 'tanh'), (17, 1, 3, 0, True, 'sigmoid'),
                                                  (300, 260, 2, None, True, 'relu'), (256, 16, 3, 2, False, 'id')])
def test_agnostic_head(dtype, H, O, D, absent, bias, act):
    """Both products against float64 on the CPU; H = 300 / O = 260 take a second block of output columns."""
    from cwn_amd import ops
    g = torch.Generator().manual_seed(H * 7 + O)
    C = 5
    pooled = [None if d == absent else torch.randn(C, H, generator=g, dtype=F64).to(dtype) for d in range(D)]
    w1 = (torch.randn(H, H, generator=g, dtype=F64) / H ** 0.5).to(dtype)
    w2 = (torch.randn(O, H, generator=g, dtype=F64) / H ** 0.5).to(dtype)
    b1 = torch.randn(H, generator=g, dtype=F64).to(dtype) if bias else None
    b2 = torch.randn(O, generator=g, dtype=F64).to(dtype) if bias else None
    dev = lambda t: None if t is None else t.to(DEV)
    out = ops.agnostic_head([dev(p) for p in pooled], dev(w1), dev(b1), dev(w2), dev(b2), act, n_complexes=C)
    assert out.dtype == dtype and tuple(out.shape) == (C, O)
    ref = _head_reference(pooled, w1, b1, w2, b2, act)
    gate(out, ref.expand(C, O), f'agnostic_head {dtype}: H = {H}, O = {O}, D = {D}, absent {absent}, {act}', tol=TOL[dtype])
    # one complex alone gives the bits it has in the batch
    alone = ops.agnostic_head([None if p is None else dev(p[3:4]) for p in pooled], dev(w1), dev(b1), dev(w2), dev(b2), act,
                              n_complexes=1)
    assert torch.equal(alone[0], out[3])


def test_agnostic_head_with_every_dimension_absent():
    """Nothing but NULL matrices: D * act(b1) through lin2, for the number of complexes the caller names."""
    from cwn_amd import ops
    g = torch.Generator().manual_seed(5)
    w1, b1, w2, b2 = (torch.randn(*s, generator=g, dtype=F64) for s in ((17, 17), (17,), (4, 17), (4,)))
    out = ops.agnostic_head([None, None], w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV), 'elu', n_complexes=3)
    ref = (2 * torch.nn.functional.elu(b1)) @ w2.t() + b2
    gate(out, ref.expand(3, 4), 'agnostic_head: absent dimensions only', tol=TOL[F64])


# ---- the invariance contract ---------------------------------------------------------------------------------------------

def _forward_ops(dtype, complexes, second=True, H=256, O=16):
    """embed_pool + agnostic_head over a batch given as a list of per-complex (x0 [n0, K], x1 [n1, K]) -> (pooled, logits)."""
    from cwn_amd import ops
    g = torch.Generator().manual_seed(77)
    K = complexes[0][0].size(1)
    ws = [(torch.randn(H, K, generator=g, dtype=F64) / K ** 0.5).to(dtype).to(DEV) for _ in range(2)]
    bs = [torch.randn(H, generator=g, dtype=F64).to(dtype).to(DEV) for _ in range(2)]
    w1 = (torch.randn(H, H, generator=g, dtype=F64) / H ** 0.5).to(dtype).to(DEV)
    w2 = (torch.randn(O, H, generator=g, dtype=F64) / H ** 0.5).to(dtype).to(DEV)
    b1, b2 = torch.randn(H, generator=g, dtype=F64).to(dtype).to(DEV), torch.randn(O, generator=g, dtype=F64).to(dtype).to(DEV)
    nd = 2 if second else 1
    xs = [torch.cat([c[d] for c in complexes]).to(DEV) for d in range(nd)]
    ptrs = [torch.tensor(np.concatenate([[0], np.cumsum([c[d].size(0) for c in complexes])]).astype(np.int64)).to(DEV)
            for d in range(nd)]
    pooled = ops.embed_pool(xs, ptrs, len(complexes), ws[:nd], bs[:nd], 'elu')
    logits = ops.agnostic_head(pooled + [None] * (2 - nd), w1, b1, w2, b2, 'elu')
    return pooled, logits


@pytest.mark.parametrize('dtype', [F32, F64])
def test_a_complex_has_the_same_bits_wherever_it_stands(dtype):
    c = _chunk()
    g = torch.Generator().manual_seed(3)
    make = lambda n0, n1: (torch.randn(n0, 3, generator=g, dtype=F64).to(dtype), torch.randn(n1, 3, generator=g, dtype=F64).to(dtype))
    target = make(4 * c + 1, c + 1)
    others = [make(1, 0), make(c, 4 * c + 1), make(c - 1, c), make(2 * c + 3, 1)]
    alone_p, alone_y = _forward_ops(dtype, [target])
    again_p, again_y = _forward_ops(dtype, [target])
    assert torch.equal(alone_y, again_y) and all(torch.equal(a, b) for a, b in zip(alone_p, again_p))      # two runs
    assert bool(torch.isfinite(alone_y).all()) and float(alone_y.abs().max()) > 0
    for place in (0, 2, 4):                                   # first, in the middle, last of five
        batch = list(others)
        batch.insert(place, target)
        pooled, y = _forward_ops(dtype, batch)
        for d in range(2):
            assert torch.equal(pooled[d][place], alone_p[d][0]), (place, d)
        assert torch.equal(y[place], alone_y[0]), place
        # ... and the rest of the launch: without the second descriptor, dimension 0 has the same bits
        pooled1, _ = _forward_ops(dtype, batch, second=False)
        assert torch.equal(pooled1[0], pooled[0]), place


# ---- the model -----------------------------------------------------------------------------------------------------------

class _Spy:
    """Counts the calls of the two launches."""

    def __init__(self, monkeypatch):
        from cwn_amd import ops
        self.n = 0
        for name in ('embed_pool', 'agnostic_head'):
            monkeypatch.setattr(ops, name, self._wrap(getattr(ops, name)))

    def _wrap(self, fn):
        def counted(*a, **kw):
            self.n += 1
            return fn(*a, **kw)
        return counted


@pytest.mark.parametrize('tag', sorted(DTYPES))
@pytest.mark.parametrize('case', CASES)
def test_model_matches_the_fixture_and_the_unfused_route(monkeypatch, case, tag):
    """Every configuration of the fixture with the route on -- 'dummy_no2' has one dimension fewer than the model, 'dummy_mixed'
    complexes without 2-cells -- and the same batch with the route off."""
    from cwn_amd import models
    g, dtype = load(G), DTYPES[tag]
    spy = _Spy(monkeypatch)
    for act, readout in CONFIGS:
        model = fixture_model(act, readout, dtype, device=DEV)
        with torch.no_grad():
            monkeypatch.setattr(models, 'FUSED_AGNOSTIC', True)
            on = model(case_batch(case, dtype, device=DEV))
            assert model.last_route == 'fused' and spy.n == 2
            monkeypatch.setattr(models, 'FUSED_AGNOSTIC', False)
            off = model(case_batch(case, dtype, device=DEV))
            assert model.last_route == 'torch' and spy.n == 2
            monkeypatch.setattr(models, 'FUSED_AGNOSTIC', {torch.float16})          # a set of dtypes: not this one
            model(case_batch(case, dtype, device=DEV))
            assert model.last_route == 'torch' and spy.n == 2
        spy.n = 0
        key = f'{case}/{act}/{readout}/{tag}'
        assert on.dtype == dtype
        gate(on, T(g[f'{key}/out']), f'{key}: route on vs the fixture', tol=TOL[dtype])
        gate(off, T(g[f'{key}/out']), f'{key}: route off vs the fixture', tol=TOL[dtype])
        gate(on, off, f'{key}: route on vs off', tol=TOL[dtype])


@pytest.mark.parametrize('tag', sorted(DTYPES))
def test_pooled_rows_match_the_fixture(tag):
    """ops.embed_pool on the fixture's batches against the reference's pooled rows (the input of its lin1)."""
    from cwn_amd import ops
    g, dtype = load(G), DTYPES[tag]
    for case in CASES:
        for act, readout in CONFIGS:
            model = fixture_model(act, readout, dtype, device=DEV)
            b = case_batch(case, dtype, device=DEV)
            plan = b.block_plan()
            n = b.dimension + 1
            pooled = ops.embed_pool([b.cochains[d].x for d in range(n)], [plan.cell_ptr_device(d, torch.device(DEV)) for d in range(n)],
                                    plan.C, [model.lin0s[d].weight for d in range(n)], [model.lin0s[d].bias for d in range(n)], act,
                                    mean=readout == 'mean')
            want = T(g[f'{case}/{act}/{readout}/{tag}/pooled'])
            for d in range(n):
                gate(pooled[d], want[d], f'{case}/{act}/{readout}/{tag}: pooled rows of dimension {d}', tol=TOL[dtype])
            assert not want[n:].any()


@pytest.mark.parametrize('tag', sorted(DTYPES))
def test_training_and_autograd_keep_the_unfused_route(monkeypatch, tag):
    """With autograd on, or in training mode with dropout, no new kernel is launched; the backward through the unfused path
    matches float64 autograd on the CPU."""
    from cwn_amd import models
    dtype = DTYPES[tag]
    monkeypatch.setattr(models, 'FUSED_AGNOSTIC', True)
    spy = _Spy(monkeypatch)
    model = fixture_model('elu', 'sum', dtype, device=DEV)
    assert model.dropout_rate > 0
    model.train()
    with torch.no_grad():
        model(case_batch('dummy_mixed', dtype, device=DEV))               # training mode with dropout, no autograd
    assert model.last_route == 'torch' and spy.n == 0
    model.eval()
    out = model(case_batch('dummy_mixed', dtype, device=DEV))             # eval mode, autograd on
    assert model.last_route == 'torch' and spy.n == 0 and out.requires_grad
    out.square().sum().backward()
    ref = fixture_model('elu', 'sum', F64)
    x64 = case_batch('dummy_mixed', dtype)
    for d in range(x64.dimension + 1):
        x64.cochains[d].x = x64.cochains[d].x.double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in model.state_dict().items()})
    out64 = ref(x64)
    out64.square().sum().backward()
    gate(out, out64, f'{tag}: unfused forward under autograd', tol=TOL[dtype])
    for (name, p), q in zip(model.named_parameters(), ref.parameters()):
        gate(p.grad, q.grad, f'{tag}: gradient of {name}', tol=TOL[dtype])
    with torch.no_grad():
        model(case_batch('dummy_mixed', dtype, device=DEV))               # eval mode, no autograd: the two launches
    assert model.last_route == 'fused' and spy.n == 2


def test_widths_beyond_the_limits_keep_the_unfused_route(monkeypatch):
    """128 input features are the widest the launch takes; a model with 129 runs the torch modules, with the same result."""
    from cwn_amd import models
    from cwn_amd.models import MessagePassingAgnostic
    monkeypatch.setattr(models, 'FUSED_AGNOSTIC', True)
    spy = _Spy(monkeypatch)
    for K, route in ((128, 'fused'), (129, 'torch')):
        torch.manual_seed(K)
        model = MessagePassingAgnostic(K, 4, 8, dropout_rate=0.0, max_dim=2, nonlinearity='tanh', readout='mean').to(DEV).eval()
        g = torch.Generator().manual_seed(K)

        def batch():
            b = case_batch('dummy_mixed', F32)
            for d in range(b.dimension + 1):
                b.cochains[d].x = torch.randn(b.cochains[d].x.size(0), K, generator=g)
            return b.to(DEV)
        b = batch()
        with torch.no_grad():
            out = model(b)
            assert model.last_route == route and spy.n == (2 if route == 'fused' else 0)
            monkeypatch.setattr(models, 'FUSED_AGNOSTIC', False)
            gate(out, model(b), f'K = {K}: {route} route against the torch modules', tol=TOL[F32])
            monkeypatch.setattr(models, 'FUSED_AGNOSTIC', True)
        spy.n = 0


# ---- the control of the strongly-regular-graph experiment ----------------------------------------------------------------------

def _sr_embeddings(dtype, max_k):
    from cwn_amd.complex import ComplexBatch
    from cwn_amd.models import MessagePassingAgnostic
    torch.manual_seed(0)
    model = MessagePassingAgnostic(1, 16, 256, dropout_rate=0.0, max_dim=2, nonlinearity='elu', readout='sum').to(dtype).to(DEV).eval()
    batch = ComplexBatch.from_complex_list(sr_complexes(max_k, dtype), max_dim=2).to(DEV)     # rook, rook', Shrikhande, Shrikhande'
    with torch.no_grad():
        emb = model(batch)
    assert model.last_route == 'fused' and emb.dtype == dtype and tuple(emb.shape) == (4, 16)
    return emb


@pytest.mark.parametrize('dtype', [F32, F64])
def test_sr_control_cannot_separate_the_graphs_at_rings_of_three(monkeypatch, dtype):
    """At max_k = 3 both graphs lift to 16 / 48 / 32 cells with identical features: identical rows and counts give identical
    bits under the invariance contract, for the two graphs and their relabelled copies alike."""
    from cwn_amd import models
    monkeypatch.setattr(models, 'FUSED_AGNOSTIC', True)
    emb = _sr_embeddings(dtype, 3)
    assert bool(torch.isfinite(emb).all()) and float(emb.abs().max()) > 0
    assert torch.equal(emb[0], emb[2])
    assert torch.equal(emb[0], emb[1]) and torch.equal(emb[2], emb[3])


def test_sr_control_at_rings_of_six(monkeypatch):
    """At max_k = 6 the 2-cell counts differ (164 against 204): relabelled copies within the reference's 0.01, the two graphs
    further apart (a float64 evaluation on the CPU gives <= 3e-13 and >= 57); the 'isomorphism' Evaluator agrees."""
    from cwn_amd import models
    from cwn_amd.evaluate import Evaluator
    monkeypatch.setattr(models, 'FUSED_AGNOSTIC', True)
    emb = _sr_embeddings(F64, 6)
    same = [float(torch.pdist(emb[[0, 1]])), float(torch.pdist(emb[[2, 3]]))]
    apart = float(torch.pdist(emb[[0, 2]]))
    print(f'[sr control] relabelled copies {same[0]:.3e}, {same[1]:.3e}; rook vs Shrikhande {apart:.3e}')
    assert max(same) < 0.01 and apart > 0.01
    ev = Evaluator('isomorphism')
    assert ev.eval({'y_pred': emb[[0, 2]], 'y_true': None}) == 0.0          # no pair mistaken for isomorphic
    assert ev.eval({'y_pred': emb[[0, 1]], 'y_true': None}) == 1.0          # the copies are (the failure share counts them)
    assert ev.eval({'y_pred': emb, 'y_true': None}) == pytest.approx(2 / 6)


# ---- dtypes --------------------------------------------------------------------------------------------------------------

def test_other_dtypes_are_a_type_error_that_names_the_dtype():
    from cwn_amd import ops
    ptr = torch.tensor([0, 4], device=DEV)
    z = lambda *s, dtype=F32: torch.zeros(*s, dtype=dtype, device=DEV)
    for bad in (torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match=str(bad)):
            ops.embed_pool([z(4, 3, dtype=bad)], [ptr], 1, [z(8, 3, dtype=bad)], [z(8, dtype=bad)], 'elu')
        with pytest.raises(TypeError, match=str(bad)):
            ops.agnostic_head([z(1, 8, dtype=bad)], z(8, 8, dtype=bad), None, z(2, 8, dtype=bad), None, 'elu')
    with pytest.raises(TypeError, match='torch.float64'):
        ops.embed_pool([z(4, 3)], [ptr], 1, [z(8, 3)], [z(8, dtype=F64)], 'elu')
    with pytest.raises(TypeError, match='torch.float32'):
        ops.agnostic_head([z(1, 8, dtype=F64)], z(8, 8, dtype=F64), z(8), z(2, 8, dtype=F64), None, 'elu')
    with pytest.raises(ValueError):
        ops.embed_pool([z(4, 3)], [ptr], 1, [z(8, 3)], [z(8)], 'gelu')


@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_operands_without_contiguous_rows_are_refused_with_their_whole_message(dtype):
    """The shape / stride clause of the operand check (the dtype and device clauses: tests/test_operand_messages_host.py), the
    messages as literals recorded before the ops shared one checker.  Nothing is launched."""
    from cwn_amd import ops
    ptr = torch.tensor([0, 4], device=DEV)
    z = lambda *s: torch.zeros(*s, dtype=dtype, device=DEV)
    kind = {F32: 'torch.float32', F64: 'torch.float64'}[dtype]        # (these messages print the dtype as torch does)
    embed = lambda x, w: ops.embed_pool([x], [ptr], 1, [w], [z(8)], 'elu')
    head = lambda p, w2: ops.agnostic_head([p], z(3, 3), z(3), w2, None, 'elu')
    cases = [
        (lambda: embed(z(3, 4).t(), z(8, 3)),
         f'embed_pool: xs[0] must be a 2-D {kind} tensor with contiguous rows (shape (4, 3), strides (1, 4))'),
        (lambda: embed(z(4, 3), z(3)),
         f'embed_pool: weights[0] must be a 2-D {kind} tensor with contiguous rows (shape (3,), strides (1,))'),
        (lambda: head(z(3, 4).t(), z(2, 3)),
         f'agnostic_head: pooled[0] must be a 2-D {kind} tensor with contiguous rows (shape (4, 3), strides (1, 4))'),
        (lambda: head(z(4, 3), z(3)),
         f'agnostic_head: lin2_w must be a 2-D {kind} tensor with contiguous rows (shape (3,), strides (1,))'),
    ]
    for call, message in cases:
        with pytest.raises(TypeError) as got:
            call()
        assert type(got.value) is TypeError and str(got.value) == message
