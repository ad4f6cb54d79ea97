"""The ring-transfer experiment on the device: the target-cell head (csrc/cwn_target_head.hip: cwn_target_head_f32 /
cwn_target_head_bwd_f32, ops.target_head), the RingSparseCIN mirror against the reference-made fixture
(tests/golden/ring_sparse_cin.npz), the `mask` key / target rows through the collate launch and the static batches, and three
training steps against float64 autograd of a plain-torch restatement (below) of mp/ring_exp_models.py:47-70.

Everything is gated by tests/_product.py::gate (max|got - ref| <= 1e-5 max(1, |ref|_inf)) against float64 unless a test says
otherwise (bit equality, or the training-step bar of test_gpu_train_full.py)."""
import numpy as np
import pytest
import torch

from cwn_amd import _cext, _ffi, models, ops, synthetic
from cwn_amd.complex import ComplexBatch
from oracle import cwn_oracle as O
from tests._golden import load, state_dict
from tests._product import gate, to_double

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
G = 'ring_sparse_cin.npz'
NAN = float('nan')
SENT = -9.0
CASES = ('ring4', 'ring10', 'ring30', 'mixed')


# ---- operands of the kernel tests ------------------------------------------------------------------------------------------------
def _targets(C, seed):
    """C complexes of 1 .. 9 cells (the first one and every fifth: ONE cell), the target at the first, a middle or the last cell
    of its complex in turn.  -> (total rows, global target rows [C])."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(2, 10, size=C)
    sizes[::5] = 1
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    local = np.array([(0, s // 2, s - 1)[c % 3] for c, s in enumerate(sizes)])
    return int(sizes.sum()), (first + local).astype(np.int32)


def _operands(H, K, C, seed, bias=True):
    g = torch.Generator().manual_seed(seed)
    N, rows = _targets(C, seed)
    x = torch.full((N, H + 8), NAN)                      # a strided x whose every non-target row (and pad column) is NaN
    x[torch.from_numpy(rows).long(), :H] = torch.randn(C, H, generator=g)
    W = torch.randn(K, H, generator=g)
    b = torch.randn(K, generator=g) if bias else None
    gout = torch.randn(C, K, generator=g)
    return x, torch.from_numpy(rows), W, b, gout


def _reference(x, rows, W, b, gout):
    H = W.size(1)
    xt = x[rows.long(), :H].double()
    out = xt @ W.double().t() + (b.double() if b is not None else 0.0)
    dx_rows = gout.double() @ W.double()
    return out, dx_rows, gout.double().t() @ xt, gout.double().sum(0)


def _workspace(C, H, K):
    """NaN-poisoned, of the size the library asks for (+ 16 bytes so that it is never empty)."""
    n = int(_ffi.lib().cwn_target_head_bwd_workspace_bytes(C, H, K))
    assert n == (0 if C <= 64 else -(-C // 64) * (K * H + (K + 3) // 4 * 4) * 4)
    return torch.full(((n + 16) // 4,), NAN, device=DEV).view(torch.uint8)[:max(n, 16)]


# ... and the kernel's other forms: (256, 32) W staged in LDS (16 .. 64 KiB); (320, 17) and (512, 64) the second 16-byte load per
# lane (H > 256) and classes beyond 16 per dW thread; (512, 64) W beyond 64 KiB, read through L2
WIDE = [(256, 32), (320, 17), (512, 64)]
SHAPES = [(H, K) for H in (4, 64, 128, 160) for K in (1, 5, 10)] + WIDE


@pytest.mark.parametrize('H,K', SHAPES)
def test_target_head_forward_and_backward_against_float64(H, K):
    for C in (1, 5, 130):
        x, rows, W, b, gout = _operands(H, K, C, seed=100 * H + 10 * K + C, bias=(K != 10))
        want, want_dx, want_dW, want_db = _reference(x, rows, W, b, gout)
        xd = x.to(DEV)[:, :H].requires_grad_(True)
        assert xd.stride(0) == H + 8
        Wd = W.to(DEV).requires_grad_(True)
        bd = None if b is None else b.to(DEV).requires_grad_(True)
        rd = rows.to(DEV)
        assert ops.FUSED_TARGET_HEAD and ops.target_head_applies(xd, rd, Wd, bd)
        out = ops.target_head(xd, rd, Wd, bd)
        what = f'H={H} K={K} C={C}'
        gate(out, want, f'target head forward {what}')
        with torch.no_grad():                            # the inference call (no autograd node) is the same launch
            assert torch.equal(ops.target_head(xd, rd, Wd, bd), out)
        out.backward(gout.to(DEV))
        dx = xd.grad
        on = torch.zeros(x.size(0), dtype=torch.bool)
        on[rows.long()] = True
        assert torch.equal(dx[~on.to(DEV)], torch.zeros(int((~on).sum()), H, device=DEV)), what
        gate(dx[rows.long().to(DEV)], want_dx, f'target head dx {what}')
        gate(Wd.grad, want_dW, f'target head dW {what}')
        if bd is not None:
            gate(bd.grad, want_db, f'target head db {what}')


@pytest.mark.parametrize('H,K,C', [(64, 5, 130), (160, 10, 130), (4, 1, 1), (128, 5, 5), (64, 5, 64), (64, 5, 65), (4, 2, 4200),
                                   (256, 32, 130), (320, 17, 5), (512, 64, 70)])
def test_backward_writes_every_row_of_dx_once_and_is_reproducible(H, K, C):
    """dx into a NaN-poisoned buffer: exactly zero off the target rows (no separate fill, nothing left over); two runs equal bit
    for bit (dW / db are summed in complex order, without atomics)."""
    x, rows, W, b, gout = _operands(H, K, C, seed=7 + H + C)
    _, want_dx, want_dW, want_db = _reference(x, rows, W, b, gout)
    xd, rd, Wd, gd = x.to(DEV)[:, :H], rows.to(DEV), W.to(DEV), gout.to(DEV)
    N = x.size(0)
    runs = []
    for _ in range(2):
        dx = torch.full((N, H + 4), NAN, device=DEV)[:, :H]
        dW, db = torch.full((K, H), NAN, device=DEV), torch.full((K,), NAN, device=DEV)
        ws = _workspace(C, H, K)
        _ffi.check(_ffi.lib().cwn_target_head_bwd_f32(gd.data_ptr(), K, xd.data_ptr(), N, xd.stride(0), rd.data_ptr(), C, Wd.data_ptr(),
                                                      dx.data_ptr(), dx.stride(0), dW.data_ptr(), db.data_ptr(), H, K, ws.data_ptr(),
                                                      ws.numel(), None, _ffi.stream_ptr(DEV)), 'cwn_target_head_bwd_f32')
        runs.append((dx.clone(), dW, db))
    on = torch.zeros(N, dtype=torch.bool, device=DEV)
    on[rd.long()] = True
    dx, dW, db = runs[0]
    assert torch.equal(dx[~on], torch.zeros(int((~on).sum()), H, device=DEV))
    gate(dx[rd.long()], want_dx, 'dx on the target rows')
    gate(dW, want_dW, 'dW')
    gate(db, want_db, 'db')
    for a, c in zip(runs[0], runs[1]):
        assert torch.equal(a, c)


@pytest.mark.parametrize('H,K', [(64, 5)] + WIDE)
@pytest.mark.parametrize('live', [0, 1, 130])
def test_row_count_contract(live, H, K):
    """include/cwn_hip.h, "DEVICE-SIDE ROW COUNTS": C is the capacity, the live number of complexes sits in device memory.  Rows
    of out at or past it are untouched; their target rows (garbage here) and rows of dlogits (NaN) enter nothing: the results
    are bit-identical to the launch a caller without a device-side count issues (C = live)."""
    CAP = 130
    x, rows, W, b, gout = _operands(H, K, CAP, seed=31)
    N = x.size(0)
    x = torch.nan_to_num(x[:, :H], nan=0.5).contiguous()      # (rows of x that a padding target could name hold numbers)
    rows_pad, g_pad = rows.clone(), gout.clone()
    rows_pad[live:] = torch.tensor([N + 5, -3, 0, 1 << 30] * CAP)[:CAP - live].int()
    g_pad[live:] = NAN
    xd, Wd, bd = x.to(DEV), W.to(DEV), b.to(DEV)
    count = torch.tensor([live, 77, 77], dtype=torch.int64, device=DEV)

    def run(rows_, g_, C, m_dev):
        out = torch.full((CAP, K), SENT, device=DEV)
        dx = torch.full((N, H), NAN, device=DEV)
        dW, db = torch.full((K, H), NAN, device=DEV), torch.full((K,), NAN, device=DEV)
        rd, gd = rows_.to(DEV), g_.to(DEV)
        L, s = _ffi.lib(), _ffi.stream_ptr(DEV)
        _ffi.check(L.cwn_target_head_f32(xd.data_ptr(), N, H, rd.data_ptr(), C, Wd.data_ptr(), bd.data_ptr(), out.data_ptr(), K, H, K,
                                         None, m_dev, s), 'fwd')
        ws = _workspace(C, H, K)
        _ffi.check(L.cwn_target_head_bwd_f32(gd.data_ptr(), K, xd.data_ptr(), N, H, rd.data_ptr(), C, Wd.data_ptr(), dx.data_ptr(), H,
                                             dW.data_ptr(), db.data_ptr(), H, K, ws.data_ptr(), ws.numel(), m_dev, s), 'bwd')
        torch.cuda.synchronize()
        return out, dx, dW, db

    out, dx, dW, db = run(rows_pad, g_pad, CAP, count.data_ptr())
    assert bool((out[live:] == SENT).all()), 'a row of out at or beyond the live count was written'
    want = _reference(x, rows[:live], W, b, gout[:live])
    gate(out[:live], want[0], f'live {live}: out')
    ref_out, ref_dx, ref_dW, ref_db = run(rows[:live].clone(), gout[:live].clone(), live, None)
    assert torch.equal(out[:live], ref_out[:live])
    assert torch.equal(dx, ref_dx) and torch.equal(dW, ref_dW) and torch.equal(db, ref_db)
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dW).all())
    if live == 0:
        assert not dx.any() and not dW.any() and not db.any()
    # ... and through the op, whose wrappers take the count from _ffi.dynamic_rows by the capacity
    with _ffi.dynamic_rows({CAP: count.data_ptr()}):
        got = ops.target_head(xd, rows_pad.clamp(0, N - 1).to(DEV), Wd, bd)
    assert torch.equal(got[:live], out[:live])


def test_unserved_shapes_and_the_switch_take_the_former_form():
    """H % 4 != 0, H > 512, K > 64, float64 and CWN_FUSED_TARGET_HEAD=0: gather_rows + linear on the same rows, inside the gate."""
    for H, K, dtype in ((6, 3, torch.float32), (516, 3, torch.float32), (8, 65, torch.float32), (64, 5, torch.float64)):
        x, rows, W, b, gout = _operands(H, K, 5, seed=H + K)
        x = torch.nan_to_num(x[:, :H], nan=0.0).contiguous()
        want = _reference(x, rows, W, b, gout)[0]
        args = (x.to(DEV, dtype), rows.to(DEV), W.to(DEV, dtype), b.to(DEV, dtype))
        assert not ops.target_head_applies(*args)
        gate(ops.target_head(*args), want, f'former form H={H} K={K} {dtype}')
    x, rows, W, b, gout = _operands(64, 5, 5, seed=3)
    args = (torch.nan_to_num(x[:, :64], nan=0.0).contiguous().to(DEV), rows.to(DEV), W.to(DEV), b.to(DEV))
    fused = ops.target_head(*args)
    ops.FUSED_TARGET_HEAD = False
    try:
        former = ops.target_head(*args)
    finally:
        ops.FUSED_TARGET_HEAD = True
    gate(fused, former, 'fused vs former form')
    with pytest.raises(IndexError):
        from cwn_amd import csr
        bad = rows.clone()
        bad[2] = 10 ** 6
        ops.target_head(args[0], bad.to(DEV), args[2], args[3])
        csr.check_errors(DEV)


# ---- the model --------------------------------------------------------------------------------------------------------------------
def case_complexes(name):
    r = {n: synthetic.ring_transfer(n, 5, 5) for n in (4, 10, 30)}
    return {'ring4': r[4], 'ring10': r[10], 'ring30': r[30], 'mixed': [r[10][1], r[30][3], r[30][0], r[10][4]]}[name]


def _model(cob, seed=None, train=False):
    m = models.RingSparseCIN(5, 5, 3, 64, use_coboundaries=cob)
    if seed is None:
        st = state_dict(load(G), 'state')
        m.load_state_dict({k: st[k] for k in m.state_dict()})
    else:
        torch.manual_seed(seed)
        m.reset_parameters()
    return (m.train() if train else m.eval()).to(DEV)


@pytest.mark.parametrize('cob', [True, False])
@pytest.mark.parametrize('name', CASES)
def test_ring_sparse_cin_against_the_reference_fixture(name, cob):
    g = load(G)
    tag = f'cob{int(cob)}'
    outs = {}
    for binding in ('ctypes', 'compiled'):
        with _cext.binding(binding):
            model = _model(cob)
            b = ComplexBatch.from_complex_list(case_complexes(name)).to(DEV)
            assert b.target_rows(0).is_cuda and b.nodes.mask.is_cuda
            with torch.no_grad():
                out, res = model(b, include_partial=True)
        gate(out, torch.from_numpy(g[f'{name}/{tag}/out']), f'{name} {tag} {binding}: logits')
        for c in range(3):
            for k in range(3):
                gate(res[f'layer{c}_{k}'], torch.from_numpy(g[f'{name}/{tag}/layer{c}_{k}']), f'{name} {tag} {binding}: layer{c}_{k}')
        assert res['out'] is out and out.shape == (len(case_complexes(name)), 5)
        outs[binding] = out
    model = _model(cob)
    ops.FUSED_TARGET_HEAD = False
    try:
        with torch.no_grad():
            former = model(ComplexBatch.from_complex_list(case_complexes(name)).to(DEV))
    finally:
        ops.FUSED_TARGET_HEAD = True
    gate(outs['ctypes'], former, f'{name} {tag}: fused head vs CWN_FUSED_TARGET_HEAD=0')
    gate(former, outs['ctypes'], f'{name} {tag}: CWN_FUSED_TARGET_HEAD=0 vs fused head')
    gate(former, torch.from_numpy(g[f'{name}/{tag}/out']), f'{name} {tag}: former form vs the fixture')


def test_a_batch_without_target_rows_takes_the_mask_literally():
    cxs = case_complexes('ring10')
    model = _model(True)
    b = ComplexBatch.from_complex_list(cxs).to(DEV)
    with torch.no_grad():
        want = model(b)
    b2 = ComplexBatch.from_complex_list(cxs).to(DEV)
    b2.nodes.target = None
    assert b2.target_rows(0) is None
    with torch.no_grad():
        got = model(b2)
    gate(got, want, 'x[mask] literally vs the target head')


@pytest.mark.parametrize('cob', [True, False])
def test_batched_forward_equals_per_complex_forwards(cob):
    model = _model(cob)
    cxs = case_complexes('mixed') + case_complexes('ring4')[:2]

    def forward(group):
        b = ComplexBatch.from_complex_list(group).to(DEV)
        with torch.no_grad():
            return model(b, include_partial=True)
    out, res = forward(cxs)
    singles = [forward([cx]) for cx in cxs]
    assert float((out - torch.cat([s[0] for s in singles])).abs().max()) == 0.0
    for key in res:
        if key != 'out':
            assert float((res[key] - torch.cat([s[1][key] for s in singles])).abs().max()) == 0.0, key


# ---- packed datasets and static batches ---------------------------------------------------------------------------------------------
def _dataset():
    """Rings of 10, 30 and 4 vertices with marks other than vertex 0 on some, labels attached."""
    cxs = synthetic.ring_transfer(10, 20, 5) + synthetic.ring_transfer(30, 10, 5) + synthetic.ring_transfer(4, 10, 5)
    for i, cx in enumerate(cxs):
        if i % 3 == 1:
            m = torch.zeros(cx.nodes.num_cells, dtype=torch.bool)
            m[(i * 7) % cx.nodes.num_cells] = True
            cx.nodes.mask = m
    return cxs


def _batches(n, sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.choice(n, size=s, replace=False) for s in sizes]


def test_collate_launch_carries_target_rows_and_mask():
    from cwn_amd.packed import PackedComplexes
    cxs = _dataset()
    p = PackedComplexes(cxs, DEV, with_csr=True)
    for idx in _batches(len(cxs), [16, 1, 7], 5):
        got = p.collate(idx)
        want = ComplexBatch.from_complex_list([cxs[i] for i in idx])
        assert got.target_rows(0).dtype == torch.int32 and got.target_rows(0).is_cuda
        assert torch.equal(got.target_rows(0).cpu(), want.target_rows(0))
        assert torch.equal(got.nodes.mask.cpu(), want.nodes.mask)
        assert torch.equal(got.target_rows(0).cpu().long(), want.nodes.mask.nonzero().flatten())
        assert torch.equal(got.y.cpu(), want.y)


@pytest.mark.parametrize('mode', ['blocked', 'csr'])
def test_static_slots_hold_the_target_rows_in_both_modes(mode):
    """The fill's collate launch writes a slot's target rows (local index + the complex's first vertex row) like any other key."""
    from cwn_amd.packed import PackedComplexes
    from cwn_amd.static_batch import StaticBatch
    cxs = _dataset()
    p = PackedComplexes(cxs, DEV, with_csr=True)
    B = 16
    sb = StaticBatch(p, B, mode=mode)
    rows = sb.slots[0].batch.target_rows(0)
    assert rows.shape == (B,) and rows.dtype == torch.int32
    for idx in _batches(len(cxs), [B, 5, 1], 4):
        sb.set_batch(idx)
        sb.fill()
        torch.cuda.synchronize()
        assert torch.equal(rows[:len(idx)], p.collate(idx).target_rows(0))


def test_static_forward_on_unseen_ring_batches_equals_the_collated_forward():
    """StaticForward over a packed ring dataset (mode 'csr' with items=True: the 5-wide first layer takes the streaming launches, the 64-wide
    layers the complex-blocked ones, as on a collated batch): batches it has never seen, one captured graph, bit-identical to
    model(packed.collate(idx)); the output is one row per complex."""
    from cwn_amd import csr
    from cwn_amd.packed import PackedComplexes
    from cwn_amd.static_batch import StaticBatch
    from cwn_amd.static_graph import StaticForward
    cxs = _dataset()
    p = PackedComplexes(cxs, DEV, with_csr=True)
    model = _model(True)
    B = 16
    sb = StaticBatch(p, B, mode='csr', items=True)
    sf = StaticForward(model, sb)
    graphs = set()
    with torch.no_grad():
        for idx in _batches(len(cxs), [B, B, 5, 1, B], 9):
            got = sf.run(idx).clone()
            graphs.add(id(sf.graph))
            want = model(p.collate(idx))
            assert got.shape == want.shape == (len(idx), 5)
            assert torch.equal(got, want), float((got - want).abs().max())
    assert len(graphs) == 1
    csr.check_errors(DEV)


def test_static_train_step_equals_the_eager_step_under_deterministic():
    from cwn_amd import csr
    from cwn_amd.packed import PackedComplexes
    from cwn_amd.static_batch import StaticBatch
    from cwn_amd.static_graph import StaticTrainStep
    from cwn_amd.train import TrainStep
    cxs = _dataset()
    p = PackedComplexes(cxs, DEV, with_csr=True)
    m1, m2 = _model(True, seed=3, train=True), _model(True, seed=3, train=True)
    m2.load_state_dict(m1.state_dict())
    B = 16
    idx = _batches(len(cxs), [11], 21)[0]
    ops.deterministic(True)
    try:
        sb = StaticBatch(p, B, mode='csr', items=True)
        sb.set_batch(idx)
        st = StaticTrainStep(m1, sb, task_type='classification', lr=1e-3)
        ref = TrainStep(m2, [p.collate(idx)], task_type='classification', lr=1e-3, use_graph=False)
        l1 = st.step_on([idx])[0].clone()
        l2 = ref.step(0)
        torch.cuda.synchronize()
        print(f'[static ring step] loss {float(l1):.9f} vs {float(l2):.9f}; flat gradient max|delta| = '
              f'{float((st.bucket.flat - ref.bucket.flat).abs().max()):.3e} of |g|_inf {float(ref.bucket.flat.abs().max()):.3e}')
        for (name, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
            if a.grad is not None and b.grad is not None and not torch.equal(a.grad, b.grad):
                print(f'[static ring step]   {name}: max|delta| = {float((a.grad - b.grad).abs().max()):.3e}')
        assert torch.equal(l1.view(-1), l2.detach().view(-1)), (float(l1), float(l2))
        assert torch.equal(st.bucket.flat, ref.bucket.flat), float((st.bucket.flat - ref.bucket.flat).abs().max())
        assert torch.equal(st.opt.flat_p, ref.opt.flat_p)
    finally:
        ops.deterministic(False)
    csr.check_errors(DEV)


# ---- training against float64 autograd of a plain-torch restatement ------------------------------------------------------------------
def ring_forward(state, cx, num_layers, use_coboundaries):
    """mp/ring_exp_models.py:47-70 in plain torch over the oracle's complex dict: init_layer on the vertex features, L x
    SparseCINConv (graph_norm 'id'), lin1 on the marked rows."""
    mask = cx['mask']
    cx = {'dimension': cx['dimension'], 'y': None, 'num_complexes': cx.get('num_complexes'), 'cochains': [dict(c) for c in cx['cochains']]}
    cx['cochains'][0]['x'] = cx['cochains'][0]['x'] @ state['init_layer.weight'].t() + state['init_layer.bias']
    xs = None
    for l in range(num_layers):
        params = O.all_cochain_params(cx, max_dim=2, include_down_features=False)
        pre = f'convs.{l}.'
        xs = O.sparse_cin_conv({k[len(pre):]: v for k, v in state.items() if k.startswith(pre)}, params, use_coboundaries, True, 'id')
        for d, x in enumerate(xs):
            cx['cochains'][d]['x'] = x
    return xs[0][mask] @ state['lin1.weight'].t() + state['lin1.bias']


def _oracle_cx(b, dtype):
    cpu = lambda t: None if t is None else t.detach().cpu()
    cx = {'dimension': b.dimension, 'y': None, 'num_complexes': b.num_complexes, 'mask': cpu(b.nodes.mask), 'cochains': [
        {k: cpu(b.cochains[d][k]) for k in ('x', 'upper_index', 'lower_index', 'shared_boundaries', 'shared_coboundaries',
                                            'boundary_index', 'y', 'batch')} for d in range(b.dimension + 1)]}
    for c in cx['cochains']:
        c['x'] = c['x'].to(dtype)
    return cx


@pytest.mark.parametrize('ring,n_steps', [(10, 3), (30, 1)])
def test_three_training_steps_against_float64_autograd(ring, n_steps):
    """Ring 10, batch 8, cross-entropy, three steps of the captured TrainStep (and one step at ring 30: 870 upper entries on the
    edges of every complex, a two-cell of 30 edges): the loss and every parameter gradient of each step
    against float64 autograd of `ring_forward` from the model's state before that step.  The bar is test_gpu_train_full.py's: the
    gate where the fp32 restatement meets it, else no further from float64 than twice what the fp32 restatement is."""
    from cwn_amd.train import TrainStep
    cxs = synthetic.ring_transfer(ring, 10, 5)[1:9]
    model = _model(True, seed=11, train=True)
    b = ComplexBatch.from_complex_list(cxs).to(DEV)
    y = b.y.detach().cpu()
    ts = TrainStep(model, [b], task_type='classification', lr=1e-3, use_graph=True)
    for step in range(n_steps):
        state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        grads = {}
        for dtype in (torch.float64, torch.float32):
            leaves = {k: v.to(dtype).requires_grad_(True) for k, v in state.items() if v.is_floating_point()}
            b_in = ComplexBatch.from_complex_list(cxs)
            out = ring_forward(leaves, _oracle_cx(b_in, dtype), 3, True)
            loss = torch.nn.functional.cross_entropy(out, y)
            loss.backward()
            grads[dtype] = (loss.detach(), {k: v.grad for k, v in leaves.items()})
        ref_loss, ref = grads[torch.float64]
        loss32, ref32 = grads[torch.float32]
        got_loss = ts.step(0)
        torch.cuda.synchronize()
        d_loss, d_loss32 = abs(float(got_loss) - float(ref_loss)), abs(float(loss32) - float(ref_loss))
        print(f'[gate] ring step {step}: loss {float(got_loss):.7f} vs float64 {float(ref_loss):.7f}: |delta| = {d_loss:.3e} '
              f'(fp32 restatement: {d_loss32:.3e})')
        assert d_loss <= 2.0 * max(d_loss32, 1e-5 * max(1.0, abs(float(ref_loss))))
        worst, worst32, d2, d2_32, n2 = 0.0, 0.0, 0.0, 0.0, 0.0
        for name, p in model.named_parameters():
            r = ref[name]
            if r is None:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
                continue
            g, r32 = p.grad.detach().cpu().double(), ref32[name].double()
            scale = max(1.0, float(r.abs().max()))
            worst, worst32 = max(worst, float((g - r).abs().max()) / scale), max(worst32, float((r32 - r).abs().max()) / scale)
            d2, d2_32, n2 = d2 + float(((g - r) ** 2).sum()), d2_32 + float(((r32 - r) ** 2).sum()), n2 + float((r ** 2).sum())
        rel, rel32 = (d2 / n2) ** 0.5, (d2_32 / n2) ** 0.5
        print(f'[gate] ring step {step}: gradients vs float64: worst max|delta| / max(1, |ref|_inf) = {worst:.3e} (fp32 restatement '
              f'{worst32:.3e}); relative L2 distance {rel:.3e} (fp32 restatement {rel32:.3e})')
        assert worst <= 2.0 * max(worst32, 1e-5), (step, worst, worst32)
        assert rel <= 2.0 * max(rel32, 1e-6), (step, rel, rel32)
