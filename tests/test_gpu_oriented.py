"""OrientedConv as one launch (csrc/cwn_oriented.hip) on the device: the entry point against a float64 evaluation of

    out = act( x W^T + (A_up o_up x) W_up^T + (A_dn o_dn x) W_dn^T )

the device-side row-count contract in the form of tests/test_gpu_row_counts.py, autograd against float64 CPU autograd, the
EdgeOrient fixtures of the reference, EdgeMPNN against a float64 restatement, the orientation property on synthetic flows
and the proof of which launches a model makes.  The bar everywhere is tests/_product.gate: max|delta| <= 1e-5 * max(1, |ref|_inf).

Shapes: widths (1,64) (3,5) (8,12) (12,12) (64,64) (128,128) -- both tile heights (w <= 16: 128 rows, else 32), vector and
scalar weight loads, masked edge columns, K not a multiple of 16; row counts 0, 1 and around 64 and 130: one tile, a partial
tile, several tiles.  The plans hold empty rows and rows of exactly CWN_LONG_ROW, CWN_LONG_ROW + 1 and 300 entries."""
import ctypes as C

import numpy as np
import pytest
import torch

from cwn_amd import _ffi, csr, layers, models, ops, synthetic
from cwn_amd.complex import Cochain, CochainBatch
from tests._golden import load, T, state_dict
from tests._product import gate

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
ACTS = ('id', 'relu', 'elu', 'tanh', 'sigmoid')
ACT64 = {'id': lambda z: z, 'relu': torch.relu, 'elu': torch.nn.functional.elu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}
WIDTHS = ((1, 64), (3, 5), (8, 12), (12, 12), (64, 64), (128, 128))
ROWS = (0, 1, 63, 64, 65, 130)
LONG = csr.LONG_ROW


def _index(n: int, seed: int, long_rows: bool = True) -> torch.Tensor:
    """A COO index [2, E] over n rows in shuffled entry order: most rows 0 .. 5 entries (a third of them empty), and -- as far
    as n has the rows -- one row of exactly LONG_ROW entries, one of LONG_ROW + 1, one of 300."""
    g = torch.Generator().manual_seed(seed)
    if n == 0:
        return torch.zeros(2, 0, dtype=torch.long)
    deg = torch.randint(0, 6, (n,), generator=g)
    deg[torch.rand(n, generator=g) < 0.33] = 0
    if long_rows:
        for r, d in zip(torch.randperm(n, generator=g)[:3].tolist(), (LONG, LONG + 1, 300)):
            deg[r] = d
    dst = torch.repeat_interleave(torch.arange(n), deg)
    src = torch.randint(0, n, (int(deg.sum()),), generator=g)
    p = torch.randperm(dst.numel(), generator=g)
    return torch.stack([src[p], dst[p]])


_PLANS = {}


def _plan(n: int, which: str):
    """(index on the CPU, built Adjacency) of the up / down stream of the n-row case, shared by every test that needs it."""
    key = (n, which)
    if key not in _PLANS:
        idx = _index(n, 1000 * n + (7 if which == 'up' else 13))
        _PLANS[key] = (idx, csr.Adjacency.from_index(idx.to(DEV), n, n))
    return _PLANS[key]


def _orient(kind, E: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    if kind is None:
        return None
    if kind == 'pm1':
        return (torch.randint(0, 2, (E,), generator=g) * 2 - 1).float()
    return torch.randn(E, generator=g)


def _agg64(x64, idx, orient):
    m = x64[idx[0]] if orient is None else x64[idx[0]] * orient.double()[:, None]
    return torch.zeros_like(x64).index_add_(0, idx[1], m)


def _formula64(x, up, dn, w_self, w_up, w_dn, act):
    """The plain formula in float64 on the CPU.  up / dn: (index, orient or None) or None."""
    x64 = x.double()
    n = x.size(0)
    H = next(t.size(0) for t in (w_self, w_up, w_dn) if t is not None)
    z = torch.zeros(n, H, dtype=torch.float64)
    if w_self is not None:
        z = z + x64 @ w_self.double().t()
    if up is not None and w_up is not None:
        z = z + _agg64(x64, *up) @ w_up.double().t()
    if dn is not None and w_dn is not None:
        z = z + _agg64(x64, *dn) @ w_dn.double().t()
    return ACT64[act](z)


def _raw(x, up, dn, w_self, w_up, w_dn, act, H, agg=False, out=None, agg_out=None, n=None, rowptrs=None):
    """One cwn_oriented_layer_f32 call on device tensors.  up / dn: (Adjacency, orient on the device or None) or None."""
    n = x.size(0) if n is None else n
    w = x.size(1)
    out = torch.empty(n, H, device=DEV) if out is None else out
    if agg and agg_out is None:
        agg_out = torch.empty(n, 2 * w, device=DEV)
    d = _ffi.OrientedDesc(x=x.data_ptr(), w_self=_ffi.ptr(w_self), out=out.data_ptr(), agg_out=_ffi.ptr(agg_out), n=n, ldx=w,
                          ldout=H, w=w, H=H, act=ops.ACTS[act], w_trans=0)
    for name, st, wt in (('up', up, w_up), ('dn', dn, w_dn)):
        if st is None:
            continue
        adj, o = st
        rp = adj.rowptr if rowptrs is None else rowptrs[name]
        setattr(d, name + '_rowptr', rp.data_ptr())
        setattr(d, name + '_col', adj.col.data_ptr() if adj.n_entries else rp.data_ptr())
        setattr(d, name + '_perm', adj.perm.data_ptr() if adj.n_entries else rp.data_ptr())
        setattr(d, name + '_orient', _ffi.ptr(o))
        setattr(d, 'w_' + name, wt.data_ptr())
    _ffi.oriented_layer(d, DEV)
    return out, agg_out


#          streams     orient   act        agg_out
CONFIGS = (('both', 'pm1', 'id', True),
           ('both', 'float', 'relu', False),
           ('both', None, 'elu', True),
           ('no_up', 'pm1', 'tanh', True),
           ('none', None, 'sigmoid', False),
           ('no_self', 'float', 'tanh', True),
           ('both', 'float', 'sigmoid', True))


@pytest.mark.parametrize('n', ROWS)
@pytest.mark.parametrize('w,H', WIDTHS)
def test_entry_point_against_float64(w, H, n):
    """Every configuration of CONFIGS at one (w, H, n): out inside the gate of the float64 formula; agg_out's halves bit-identical
    to cwn_aggregate_f32 (CWN_MSG_A_TIMES_B, ib = perm; CWN_MSG_A without orient) on rows of at most CWN_LONG_ROW entries and
    inside the gate on the longer ones; an absent stream's half zeros; two runs torch.equal."""
    g = torch.Generator().manual_seed(w * 1000 + H * 10 + n)
    x = torch.randn(n, w, generator=g)
    ws = [torch.randn(H, w, generator=g) / (3 * w) ** 0.5 for _ in range(3)]
    xd, wd = x.to(DEV), [t.to(DEV) for t in ws]
    if n == 0:                                  # nothing to launch, and nothing launched: CWN_OK, an empty result
        out, _ = _raw(xd, None, None, wd[0], None, None, 'relu', H, agg=True)
        assert tuple(out.shape) == (0, H)
        assert tuple(ops.oriented_layer(xd, None, None, None, None, wd[0], wd[1], wd[2], 'tanh').shape) == (0, H)
        return
    (iu, au), (il, al) = _plan(n, 'up'), _plan(n, 'dn')
    for streams, okind, act, agg in CONFIGS:
        ou, ol = _orient(okind, iu.size(1), 5), _orient(okind, il.size(1), 6)
        up = None if streams in ('no_up', 'none') else (au, None if ou is None else ou.to(DEV))
        dn = None if streams == 'none' else (al, None if ol is None else ol.to(DEV))
        w_self = None if streams == 'no_self' else wd[0]
        what = f'w={w} H={H} n={n} {streams} orient={okind} {act} agg_out={agg}'
        out, ag = _raw(xd, up, dn, w_self, wd[1], wd[2], act, H, agg=agg)
        ref = _formula64(x, None if up is None else (iu, ou), None if dn is None else (il, ol),
                         None if w_self is None else ws[0], ws[1], ws[2], act)
        gate(out, ref, what)
        out2, ag2 = _raw(xd, up, dn, w_self, wd[1], wd[2], act, H, agg=agg)
        assert torch.equal(out, out2), what + ': two runs differ'
        if not agg:
            continue
        assert torch.equal(ag, ag2)
        for half, st, idx, o in ((0, up, iu, ou), (1, dn, il, ol)):
            got = ag[:, half * w:(half + 1) * w]
            if st is None:
                assert not bool(got.any()), what + ': the half of an absent stream is not zero'
                continue
            adj = st[0]
            spec = ops.AggSpec(adj=adj, n_dst=n, F=w, A=xd, ia=adj.col)
            if o is not None:
                spec.B, spec.ib, spec.msg_op = st[1].view(-1, 1), adj.perm, ops.MSG_A_TIMES_B
            ref_agg, = ops.run_aggregate([spec], DEV)
            short = ((adj.rowptr[1:] - adj.rowptr[:-1]) <= LONG)
            assert torch.equal(got[short], ref_agg[short]), what + f': agg_out half {half} is not cwn_aggregate_f32 bit for bit'
            gate(got, _agg64(x.double(), idx, o), what + f' agg_out half {half}')


class _NoEntries:
    """The plan of an adjacency over no rows."""
    n_entries = 0

    def __init__(self):
        self.rowptr = torch.zeros(1, dtype=torch.int32, device=DEV)


# ---- the device-side row count ----------------------------------------------------------------------------------------------------
CAP = 200
SENT = -9.0
NAN = float('nan')


@pytest.mark.parametrize('w,H,act', [(8, 12, 'tanh'), (64, 64, 'relu')])
def test_row_count_contract(w, H, act):
    """cwn_oriented_layer_f32 under the "DEVICE-SIDE ROW COUNTS" contract of include/cwn_hip.h, in the form of
    tests/test_gpu_row_counts.py: capacity 200, live counts 0, 1, 63, 64, 65, 199, 200 and one below / at / above both tile
    heights of the kernel (32 and 128 rows); the padding rows of x hold NaN, the padding rowptr entries garbage, out and agg_out
    the sentinel.  (a) live rows inside the gate of the float64 formula over the live rows; (b) bit-identical to the launch
    with n = live, m_dev = NULL on copies; (c) rows at or beyond the count hold the sentinel bit for bit; (d) a count of 0
    writes nothing."""
    tm = _ffi.oriented_tm(w)
    assert tm in (32, 128)
    lives = sorted({0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 199, 200})
    g = torch.Generator().manual_seed(w + H)
    X = torch.randn(CAP, w, generator=g)
    ws = [torch.randn(H, w, generator=g) / (3 * w) ** 0.5 for _ in range(3)]
    wd = [t.to(DEV) for t in ws]
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    for live in lives:
        iu, il = _index(live, 31 * live + 1, long_rows=live > 100), _index(live, 31 * live + 2, long_rows=False)
        if live == 0:                           # no rows, no entries: a row pointer of one zero
            au = al = _NoEntries()
        else:
            au, al = csr.Adjacency.from_index(iu.to(DEV), live, live), csr.Adjacency.from_index(il.to(DEV), live, live)
        ou, ol = _orient('pm1', iu.size(1), live), _orient('float', il.size(1), live + 1)
        up, dn = (au, ou.to(DEV)), (al, ol.to(DEV))
        # capacity-sized operands: NaN rows, garbage row pointers, sentinel outputs
        xd = X.clone()
        xd[live:] = NAN
        xd = xd.to(DEV)
        junk = torch.full((CAP - live,), 0x7ffffff0, dtype=torch.int32, device=DEV)
        rps = {'up': torch.cat([au.rowptr, junk]), 'dn': torch.cat([al.rowptr, junk])}
        out = torch.full((CAP, H), SENT, device=DEV)
        agg = torch.full((CAP, 2 * w), SENT, device=DEV)
        count.fill_(live)
        with _ffi.dynamic_rows({CAP: count.data_ptr()}):
            _raw(xd, up, dn, wd[0], wd[1], wd[2], act, H, out=out, agg_out=agg, n=CAP, rowptrs=rps)
        what = f'w={w} H={H} live={live}'
        assert bool((out[live:] == SENT).all()) and bool((agg[live:] == SENT).all()), what + ': a row beyond the count was written'  # (c), (d)
        assert not bool(torch.isnan(out[:live]).any()) and not bool(torch.isnan(agg[:live]).any()), what
        if live == 0:
            continue
        ref = _formula64(X[:live], (iu, ou), (il, ol), ws[0], ws[1], ws[2], act)
        gate(out[:live], ref, what)                                                             # (a)
        o2, a2 = _raw(X[:live].contiguous().to(DEV), up, dn, wd[0], wd[1], wd[2], act, H, agg=True)
        assert torch.equal(out[:live], o2) and torch.equal(agg[:live], a2), what + ': differs from the launch over the live rows'  # (b)


def test_dz_row_count_and_formulas():
    """cwn_oriented_dz_f32: act' as a function of out for the five activations against float64, rows beyond the count untouched."""
    g = torch.Generator().manual_seed(3)
    z = torch.randn(CAP, 12, generator=g)
    dout = torch.randn(CAP, 12, generator=g)
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    for act in ACTS:
        out = ACT64[act](z.double())
        z64 = z.double().requires_grad_(True)
        ref, = torch.autograd.grad(ACT64[act](z64), z64, dout.double())
        for live in (0, 1, 65, 200):
            dz = torch.full((CAP, 12), SENT, device=DEV)
            count.fill_(live)
            o = out.float()
            o[live:] = NAN
            dd, od = dout.to(DEV), o.to(DEV)
            rc = _ffi.lib().cwn_oriented_dz_f32(dd.data_ptr(), od.data_ptr(), dz.data_ptr(), CAP, 12, 12, 12, 12,
                                                ops.ACTS[act], count.data_ptr(), _ffi.stream_ptr(DEV))
            assert rc == 0
            assert bool((dz[live:] == SENT).all())
            gate(dz[:live], ref[:live], f'dz {act} live={live}')


# ---- autograd ---------------------------------------------------------------------------------------------------------------------
def _autograd_case(w, H, act, x_grad=True, n=130):
    g = torch.Generator().manual_seed(w + 7 * H)
    x = torch.randn(n, w, generator=g)
    ws = [torch.randn(H, w, generator=g) / (3 * w) ** 0.5 for _ in range(3)]
    G = torch.randn(n, H, generator=g)
    (iu, au), (il, al) = _plan(n, 'up'), _plan(n, 'dn')
    ou, ol = _orient('pm1', iu.size(1), 1), _orient('float', il.size(1), 2)
    return x, ws, G, (iu, au, ou), (il, al, ol)


def _device_grads(x, ws, G, up, dn, act, x_grad=True):
    xd = x.to(DEV).requires_grad_(x_grad)
    wd = [t.to(DEV).requires_grad_(True) for t in ws]
    out = ops.oriented_layer(xd, up[1], up[2].to(DEV), dn[1], dn[2].to(DEV), wd[0], wd[1], wd[2], act)
    (out * G.to(DEV)).sum().backward()
    return out.detach(), xd.grad, [t.grad for t in wd]


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('w,H', [(8, 12), (64, 64)])
def test_autograd_against_float64(w, H, act):
    """Gradients of ops.oriented_layer w.r.t. x and the three weights against float64 CPU autograd of the formula (n = 130,
    plans with empty, 64-, 65- and 300-entry rows)."""
    x, ws, G, up, dn = _autograd_case(w, H, act)
    out, dx, dws = _device_grads(x, ws, G, up, dn, act)
    x64 = x.double().requires_grad_(True)
    w64 = [t.double().requires_grad_(True) for t in ws]
    z = x64 @ w64[0].t()
    for (idx, _, o), W in ((up, w64[1]), (dn, w64[2])):
        z = z + torch.zeros(x.size(0), w, dtype=torch.float64).index_add_(0, idx[1], x64[idx[0]] * o.double()[:, None]) @ W.t()
    ref = ACT64[act](z)
    (ref * G.double()).sum().backward()
    gate(out, ref, f'forward {act} {w}x{H}')
    gate(dx, x64.grad, f'dx {act} {w}x{H}')
    for k, name in enumerate(('w_self', 'w_up', 'w_dn')):
        gate(dws[k], w64[k].grad, f'd{name} {act} {w}x{H}')


def test_autograd_without_input_gradient_and_absent_streams():
    """x.requires_grad = False: no data launch, the weight gradients unchanged; a weight whose stream has no entries gets zeros;
    EdgeMPNN's shape (w_up None) has no upper gradient at all."""
    x, ws, G, up, dn = _autograd_case(8, 12, 'tanh')
    _, dx, dws = _device_grads(x, ws, G, up, dn, 'tanh', x_grad=True)
    _, dx0, dws0 = _device_grads(x, ws, G, up, dn, 'tanh', x_grad=False)
    assert dx is not None and dx0 is None
    for a, b in zip(dws, dws0):
        assert torch.equal(a, b)
    xd = x.to(DEV).requires_grad_(True)
    wd = [t.to(DEV).requires_grad_(True) for t in ws]
    empty = csr.Adjacency.from_index(torch.zeros(2, 0, dtype=torch.long, device=DEV), x.size(0), x.size(0), build=False)
    out = ops.oriented_layer(xd, empty, torch.zeros(0, device=DEV), dn[1], dn[2].to(DEV), wd[0], wd[1], wd[2], 'relu')
    out.sum().backward()
    assert wd[1].grad is not None and not bool(wd[1].grad.any()) and bool(wd[2].grad.any())
    gate(out, _formula64(x, None, (dn[0], dn[2]), ws[0], None, ws[2], 'relu'), 'empty upper adjacency')
    xd.grad = None
    out = ops.oriented_layer(xd, up[1], None, dn[1], None, wd[0], None, wd[2], 'relu')
    gate(out, _formula64(x, None, (dn[0], None), ws[0], None, ws[2], 'relu'), 'no upper map, no orientation')
    out.sum().backward()
    assert xd.grad is not None


def test_deterministic_backward_is_bit_reproducible():
    x, ws, G, up, dn = _autograd_case(64, 64, 'tanh')
    ops.deterministic(True)
    try:
        a = _device_grads(x, ws, G, up, dn, 'tanh')
        b = _device_grads(x, ws, G, up, dn, 'tanh')
    finally:
        ops.deterministic(False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for p, q in zip(a[2], b[2]):
        assert torch.equal(p, q)


# ---- models -------------------------------------------------------------------------------------------------------------------------
KEYS = ('x', 'upper_index', 'lower_index', 'upper_orient', 'lower_orient')


def _to_dev(data):
    for k in KEYS + ('batch',):
        setattr(data, k, getattr(data, k).to(DEV))
    return data


class _Counter:
    """Counts the calls of two entry points by wrapping the _ffi functions that issue them."""

    def __enter__(self):
        self.fused = self.aggregate = 0
        self._o, self._a = _ffi.oriented_layer, _ffi.aggregate

        def oriented(*a, **k):
            self.fused += 1
            return self._o(*a, **k)

        def aggregate(descs, device, dtype=torch.float32):
            self.aggregate += 1
            return self._a(descs, device, dtype)
        _ffi.oriented_layer, _ffi.aggregate = oriented, aggregate
        return self

    def __exit__(self, *exc):
        _ffi.oriented_layer, _ffi.aggregate = self._o, self._a
        return False


@pytest.mark.parametrize('tag,invar,act', [('orient', False, 'id'), ('orient_invar', True, 'relu')])
def test_edge_orient_fixture_on_the_fused_layer(tag, invar, act):
    """EdgeOrient with the reference's state_dict (tests/golden/cin0_models.npz: F 8, hidden 12, 2 layers, five complexes, some
    without upper adjacency): per-edge values and predictions against the reference's, in eval and with autograd recording,
    and against the same model with layers.FUSED_ORIENTED = False; the fused launch is what ran."""
    g = load('cin0_models.npz')
    model = models.EdgeOrient(8, 2, 2, 12, dropout_rate=0.0, nonlinearity=act, readout='sum', fully_invar=invar)
    model.load_state_dict(state_dict(g, f'{tag}/state'))
    model = model.to(DEV).eval()
    edges = [Cochain(dim=1, **{k: T(g[f'orient/edges/{i}/{k}']) for k in KEYS}) for i in range(int(g['orient/n']))]
    data = _to_dev(CochainBatch.from_cochain_list(edges))
    for grad in (False, True):
        res = {}
        for fused in (True, False):
            layers.FUSED_ORIENTED = fused
            try:
                data.x = torch.cat([e.x for e in edges]).to(DEV)
                with _Counter() as c, torch.set_grad_enabled(grad):
                    y, cells = model(data, include_partial=True)
            finally:
                layers.FUSED_ORIENTED = True
            assert c.fused == (2 if fused else 0)
            res[fused] = (y, cells)
            gate(cells, T(g[f'{tag}/cells']), f'EdgeOrient[{tag}] cells fused={fused} grad={grad}')
            gate(y, T(g[f'{tag}/out']), f'EdgeOrient[{tag}] out fused={fused} grad={grad}')
        gate(res[True][1], res[False][1].double(), f'EdgeOrient[{tag}] cells, fused against unfused grad={grad}')
        gate(res[True][0], res[False][0].double(), f'EdgeOrient[{tag}] out, fused against unfused grad={grad}')
        if grad:
            res[True][0].sum().backward()
            assert all(p.grad is not None for p in model.parameters())
            model.zero_grad()


def test_biased_layer_is_declined_and_matches_the_fixture():
    """OrientedConv.forward of tests/golden/edge_oriented.npz: its three maps carry biases, so the dispatch declines the layer
    (as it declines a user callable, float64 and a reduce other than add) and the result is the fixture's."""
    g = load('edge_oriented.npz')
    F, Hd = 8, 12
    oc = layers.OrientedConv(1, F, F, update_up_nn=torch.nn.Linear(F, Hd), update_down_nn=torch.nn.Linear(F, Hd),
                             update_nn=torch.nn.Linear(F, Hd), act_fn=torch.tanh)
    oc.load_state_dict(state_dict(g, 'oriented/state'))
    oc = oc.to(DEV)
    c = Cochain(dim=1, **{k: T(g[f'oriented/{k}']).to(DEV) for k in KEYS})
    assert oc.fused_operands(c.x) is None
    with _Counter() as cnt, torch.no_grad():
        y = oc(c)
    assert cnt.fused == 0 and cnt.aggregate == 1
    gate(y, T(g['oriented/out']), 'OrientedConv.forward with biases (declined)')
    # the same layer without its biases is taken, and is the formula
    free = layers.OrientedConv(1, F, F, update_up_nn=torch.nn.Linear(F, Hd, bias=False), update_down_nn=torch.nn.Linear(F, Hd, bias=False),
                               update_nn=torch.nn.Linear(F, Hd, bias=False), act_fn=torch.tanh).to(DEV)
    w = free.fused_operands(c.x)
    assert w is not None and w[3] == 'tanh' and w[0] is free.update_nn.weight and w[1] is free.update_up_nn.weight
    with _Counter() as cnt, torch.no_grad():
        y = free(c)
    assert cnt.fused == 1 and cnt.aggregate == 0
    ref = _formula64(c.x.cpu(), (c.upper_index.cpu(), c.upper_orient.cpu()), (c.lower_index.cpu(), c.lower_orient.cpu()),
                     free.update_nn.weight.detach().cpu(), free.update_up_nn.weight.detach().cpu(),
                     free.update_down_nn.weight.detach().cpu(), 'tanh')
    gate(y, ref, 'OrientedConv.forward without biases (fused)')
    for name in ACTS:
        free.act_fn = models.get_nonlinearity(name, return_module=False)
        assert free.fused_operands(c.x)[3] == name
    free.act_fn = lambda t: t
    assert free.fused_operands(c.x) is None                     # a user callable
    free.act_fn = torch.tanh
    assert free.fused_operands(c.x.double()) is None            # float64
    free.aggr_down = 'mean'
    assert free.fused_operands(c.x) is None                     # reduce != add
    free.aggr_down = 'add'
    free.update_up_nn = torch.nn.Sequential(torch.nn.Linear(F, Hd, bias=False)).to(DEV)
    assert free.fused_operands(c.x) is None                     # not a Linear
    free.update_up_nn = layers.ZeroUpdate()
    assert free.fused_operands(c.x)[1] is None


def _edge_mpnn64(state, data, num_layers, fully_invar, act):
    """mp/models.py:589-612 restated in float64 on the CPU (sum readout, no dropout): OrientedConv layers without the upper
    map, messages x_j (times the orientation unless fully_invar), then |.|, pooling per complex, lin1 -> ReLU -> lin2."""
    x = data.x.detach().cpu().double()
    idx, o = data.lower_index.cpu(), data.lower_orient.cpu().double()
    if fully_invar:
        x = x.abs()
    for i in range(num_layers):
        m = x[idx[0]] if fully_invar else x[idx[0]] * o[:, None]
        down = torch.zeros_like(x).index_add_(0, idx[1], m)
        x = ACT64[act](x @ state[f'convs.{i}.update_nn.weight'].t() + down @ state[f'convs.{i}.update_down_nn.weight'].t())
    cells = x
    if not fully_invar:
        x = x.abs()
    batch = data.batch.cpu()
    pooled = torch.zeros(int(batch.max()) + 1, x.size(1), dtype=torch.float64).index_add_(0, batch, x)
    h = torch.relu(pooled @ state['lin1.weight'].t() + state['lin1.bias'])
    return h @ state['lin2.weight'].t() + state['lin2.bias'], cells


@pytest.mark.parametrize('invar', [True, False])
def test_edge_mpnn_against_float64_restatement(invar):
    """EdgeMPNN has no reference fixture: its layer is the OrientedConv the EdgeOrient fixtures pin, and the model is compared
    here with a float64 restatement of mp/models.py:589-612 -- 3 layers, hidden 16, relu: predictions, per-edge values and every
    parameter gradient; L fused launches and no aggregation launch but the readout's."""
    torch.manual_seed(5)
    model = models.EdgeMPNN(1, 2, 3, 16, nonlinearity='relu', fully_invar=invar).to(DEV)
    data = _to_dev(CochainBatch.from_cochain_list(synthetic.edge_flows(4, 6, seed=2)))
    x0 = data.x.clone()
    with _Counter() as c:
        y, cells = model(data, include_partial=True)
    assert c.fused == 3 and c.aggregate == 1
    y.square().sum().backward()
    st = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    data.x = x0
    y64, cells64 = _edge_mpnn64(st, data, 3, invar, 'relu')
    y64.square().sum().backward()
    gate(cells, cells64, f'EdgeMPNN cells fully_invar={invar}')
    gate(y, y64, f'EdgeMPNN out fully_invar={invar}')
    for k, p in model.named_parameters():
        gate(p.grad, st[k].grad, f'EdgeMPNN d{k} fully_invar={invar}')


def _flows(t=None, seed=4):
    m = synthetic.edge_flow_mesh(6)
    E = len(m['edges'])
    cs = synthetic.edge_flows(4, 6, seed=seed, flip=np.ones(E) if t is None else t)
    return _to_dev(CochainBatch.from_cochain_list(cs)), E


@pytest.mark.parametrize('act', ['id', 'tanh'])
def test_orientation_equivariance_on_the_device(act):
    """On edge_flows(4, side=6): under a random change of edge orientations T the per-edge outputs of EdgeOrient (odd
    activations: id, tanh) become T . cells and the predictions do not move, inside the gate; with relu (not odd) and
    fully_invar=False the per-edge equivariance fails by far more than the gate -- the test can see a difference."""
    torch.manual_seed(1)
    base, E = _flows()
    t = np.random.default_rng(3).integers(0, 2, E) * 2 - 1
    flipped, _ = _flows(t)
    tt = torch.from_numpy(np.tile(t, 4)).to(DEV).float()[:, None]
    model = models.EdgeOrient(1, 2, 4, 16, nonlinearity=act).to(DEV).eval()
    with _Counter() as c, torch.no_grad():
        y0, c0 = model(base, include_partial=True)
        y1, c1 = model(flipped, include_partial=True)
    assert c.fused == 8
    gate(c1, (c0 * tt).double(), f'{act}: cells under T')
    gate(y1, y0.double(), f'{act}: predictions under T')
    assert float(c0.abs().max()) > 1e-3
    relu = models.EdgeOrient(1, 2, 4, 16, nonlinearity='relu', fully_invar=False).to(DEV).eval()
    base, _ = _flows()
    flipped, _ = _flows(t)
    with torch.no_grad():
        _, r0 = relu(base, include_partial=True)
        _, r1 = relu(flipped, include_partial=True)
    err = float((r1 - r0 * tt).abs().max())
    assert err > 100 * 1e-5 * max(1.0, float(r0.abs().max())), err


def test_dispatch_proof():
    """With the switch on an L-layer EdgeOrient eval forward makes L calls of cwn_oriented_layer_f32 and no cwn_aggregate_f32 call
    for its layers (the one aggregation left is the readout's pooling); with the switch off none of the new calls."""
    L = 3
    model = models.EdgeOrient(1, 2, L, 16, nonlinearity='tanh').to(DEV).eval()
    for fused in (True, False):
        data, _ = _flows()
        layers.FUSED_ORIENTED = fused
        try:
            with _Counter() as c, torch.no_grad():
                model(data)
        finally:
            layers.FUSED_ORIENTED = True
        assert (c.fused, c.aggregate) == ((L, 1) if fused else (0, L + 1)), (fused, c.fused, c.aggregate)
        data, _ = _flows()                      # the layers alone: no aggregation launch at all when fused
        layers.FUSED_ORIENTED = fused
        try:
            with _Counter() as c, torch.no_grad():
                for conv in model.convs:
                    data.x = conv(data)
        finally:
            layers.FUSED_ORIENTED = True
        assert (c.fused, c.aggregate) == ((L, 0) if fused else (0, L))
