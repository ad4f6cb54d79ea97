"""The molecular graph baseline on the device: cwn_gine_layer_f32 (csrc/cwn_gine.hip) against a float64 evaluation of

    s = sum_p relu(x[col[p]] + e[eidx[p]]) + (1 + eps) x,   h = act((s W1^T + b1) scale1 + shift1),
    out = act_post(act((h W2^T + b2) scale2 + shift2))

with both forms of eidx (the plan's shared-cell index into a few edge rows, and its perm into one row per entry), rows without
entries, strided operands inside wider buffers, bit-reproducibility, non-finite values, the two routes of layers.GINEConv,
the generic route's gradients against float64 CPU autograd, and models.EmbedGIN against the float64 restatement of
tests/_gine.py.  The bar everywhere is tests/_product.gate: max|delta| <= 1e-5 * max(1, |ref|_inf).

Shapes and plans are those of tests/test_gpu_gin.py: widths (1,64) (3,5) (5,64) (12,12) (64,64) (100,128) (128,128), rows 0, 1,
one below / at / above CWN_GIN_TM and 130, plans with empty rows and rows of exactly CWN_LONG_ROW, CWN_LONG_ROW + 1 and 300
entries; the edge rows are n_e = max(1, n // 2).

Input scale.  x and e are drawn at tests/test_gpu_gin.py's XSCALE = 1/64.  The formula evaluated in float32 on the CPU, the
row's messages added in CSR order, no kernel, at (w, H, n) = (100, 128, 32) over the eight settings the entry-point test runs,
eps 0.37, the edge rows read through the shared-cell index: the largest distance from float64 is 4.7e-7 of max(1, |ref|_inf)
(ELU with biases and norms: 3.3e-6 at |ref|_inf = 7.03; behind the saturating tanh 4.4e-7 at |ref|_inf = 1) against the
gate's 1e-5 -- the number format's own error is a factor of 21 inside the gate."""
import itertools

import pytest
import torch

from cwn_amd import _ffi, csr, layers, models, ops, synthetic
from cwn_amd.cell_mp import IndexedRows
from cwn_amd.complex import ComplexBatch
from tests import _gin, _gine
from tests import test_gine_host as host
from tests._product import gate, gate_nonfinite
from tests.test_gpu_gin import XSCALE, WIDTHS, ROWS, ACTS, EPS, TM, _operands, _pick

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
# the settings of one (w, H, n): (act, bias, norm) -- all five activations at one setting, ReLU at all four
SETTINGS = [(a, True, True) for a in ACTS] + [('relu', b, s) for b, s in ((False, False), (True, False), (False, True))]


@pytest.fixture
def fused_on():
    old, layers.FUSED_GINE = layers.FUSED_GINE, True
    yield
    layers.FUSED_GINE = old


_PLANS = {}


def _plan(n: int):
    """(index [2, E], shared-cell index [E], n_e, edge rows [n_e, 128] -- all on the CPU -- and the built Adjacency, which
    carries the shared-cell index) of the n-row case, shared by every test that needs it."""
    if n not in _PLANS:
        idx = _gin.index_like_oriented(n, 1000 * n + 7, csr.LONG_ROW)
        g = torch.Generator().manual_seed(77 + n)
        n_e = max(1, n // 2)
        shared = torch.randint(0, n_e, (idx.size(1),), generator=g)
        cells = XSCALE * torch.randn(n_e, 128, generator=g)
        adj = csr.Adjacency.from_index(idx.to(DEV), n, n, shared.to(DEV), n_e) if n else None
        _PLANS[n] = (idx, shared, n_e, cells, adj)
    return _PLANS[n]


def _edge(n, w, mode):
    """(edge matrix on the CPU, the eidx_mode argument of tests/_gine.py) of the n-row plan at width w in the form `mode`."""
    idx, shared, _, cells, _ = _plan(n)
    cells = cells[:, :w].contiguous()
    return (cells, shared) if mode == 'aux' else (cells[shared], 'perm')


def _raw(x, adj, e, mode, eps_dev, stages, act, act_post, out=None):
    """One cwn_gine_layer_f32 call on device tensors (x, e and out may be column slices)."""
    n, w = x.shape
    H = stages[0][0].size(0)
    out = torch.empty(n, H, device=DEV) if out is None else out
    g = _ffi.GinDesc(x=x.data_ptr(), eps_dev=_ffi.ptr(eps_dev), out=out.data_ptr(), n=n, ldx=x.stride(0) if n > 1 else w,
                     ldout=out.stride(0) if n > 1 else H, w=w, H=H, act=ops.ACT_CODES[act], act_post=ops.ACT_CODES[act_post])
    (g.W1, g.b1, g.scale1, g.shift1), (g.W2, g.b2, g.scale2, g.shift2) = [[_ffi.ptr(t) for t in s] for s in stages]
    d = _ffi.GineDesc(g=g)
    if adj is not None and adj.n_entries:
        d.g.rowptr, d.g.col = adj.rowptr.data_ptr(), adj.col.data_ptr()
        d.e, d.lde, d.n_e = e.data_ptr(), (e.stride(0) if e.size(0) > 1 else w), e.size(0)
        d.eidx = (adj.aux if mode == 'aux' else adj.perm).data_ptr()
    _ffi.gine_layer(d, DEV)
    return out


def _dev(stages):
    return [tuple(t.to(DEV) for t in s) for s in stages]


@pytest.mark.parametrize('n', ROWS)
@pytest.mark.parametrize('w,H', WIDTHS)
def test_entry_point_against_float64(w, H, n):
    """At one (w, H, n): both forms of eidx x the eight settings x eps_dev (NULL, 0.37), each inside the gate of the float64
    formula; one setting more with act_post."""
    x, stages = _operands(w, H, n, w * 1000 + H * 10 + n)
    idx, _, _, _, adj = _plan(n)
    xd, sd = x.to(DEV), _dev(stages)
    eps_dev = torch.tensor([EPS], device=DEV)
    for mode in ('aux', 'perm'):
        e, how = _edge(n, w, mode)
        ed = e.to(DEV)
        for (act, bias, norm), eps in itertools.product(SETTINGS + [('elu+post', True, True)], (None, EPS)):
            act, post = (act[:-5], act[:-5]) if act.endswith('+post') else (act, 'id')
            out = _raw(xd, adj, ed, mode, None if eps is None else eps_dev, _pick(sd, bias, norm), act, post)
            assert tuple(out.shape) == (n, H)
            if n == 0:                              # nothing to launch, and nothing launched: CWN_OK, an empty result
                continue
            ref = _gine.gine_formula64(x, idx, e, how, eps or 0.0, _pick(stages, bias, norm), act, post)
            gate(out, ref, f'w={w} H={H} n={n} {mode} act={act} post={post} norm={norm} bias={bias} eps={eps}')


def test_rows_without_entries_equal_the_no_plan_launch_and_no_plan_means_the_self_term():
    x, stages = _operands(12, 12, 70, 5)
    idx, _, _, _, adj = _plan(70)
    deg = torch.bincount(idx[1], minlength=70)
    assert int((deg == 0).sum()) > 5
    e, _ = _edge(70, 12, 'aux')
    xd, sd = x.to(DEV), _dev(stages)
    eps_dev = torch.tensor([EPS], device=DEV)
    out = _raw(xd, adj, e.to(DEV), 'aux', eps_dev, sd, 'tanh', 'id')
    alone = _raw(xd, None, None, 'aux', eps_dev, sd, 'tanh', 'id')          # rowptr NULL, e and eidx NULL
    gate(alone, _gin.gin_formula64(x, None, EPS, stages, 'tanh'), 'no plan: nn((1 + eps) x)')
    assert torch.equal(out[deg == 0], alone[deg == 0])
    assert not torch.equal(out[deg > 0], alone[deg > 0])


@pytest.mark.parametrize('mode', ['aux', 'perm'])
@pytest.mark.parametrize('w,H,x0,o0,e0,n', [(64, 64, 0, 64, 4, 130), (12, 20, 3, 17, 1, 70), (100, 128, 128, 0, 0, 33),
                                            (5, 7, 9, 1, 2, 1)])
def test_strided_operands_inside_wider_buffers(w, H, x0, o0, e0, n, mode):
    """x and out are column slices of one buffer, e a column slice of another (16-byte aligned and not): the output inside
    the gate, every element outside the out slice untouched bit for bit, the edge buffer untouched."""
    width = max(x0 + w, o0 + H) + 5
    x, stages = _operands(w, H, n, 77 + w)
    idx, _, _, _, adj = _plan(n)
    e, how = _edge(n, w, mode)
    buf = torch.full((n, width), float('nan'), device=DEV)      # (NaN around the x and e slices: a load that strays shows in out)
    buf[:, x0:x0 + w] = x.to(DEV)
    ebuf = torch.full((e.size(0), e0 + w + 3), float('nan'), device=DEV)
    ebuf[:, e0:e0 + w] = e.to(DEV)
    before, ebefore = buf.clone(), ebuf.clone()
    sd = _dev(stages)
    out = _raw(buf[:, x0:x0 + w], adj, ebuf[:, e0:e0 + w], mode, None, sd, 'relu', 'id', out=buf[:, o0:o0 + H])
    assert not torch.isnan(out).any(), 'a NaN beside the x or e slice reached the output'
    gate(out, _gine.gine_formula64(x, idx, e, how, 0.0, stages, 'relu'), f'strided {w}x{H} {mode}')
    keep = torch.ones(width, dtype=torch.bool, device=DEV)
    keep[o0:o0 + H] = False
    assert torch.equal(buf[:, keep].view(torch.int32), before[:, keep].view(torch.int32)), 'an element outside the slice was written'
    assert torch.equal(ebuf.view(torch.int32), ebefore.view(torch.int32))
    # the op does the same through its `out` argument
    buf2 = before.clone()
    with torch.no_grad():
        got = ops.gine_layer(buf2[:, x0:x0 + w], adj, ebuf[:, e0:e0 + w], None, sd, 'relu', out=buf2[:, o0:o0 + H], edge_mode=mode)
    assert got.data_ptr() == buf2.data_ptr() + 4 * o0 and torch.equal(buf2.view(torch.int32), buf.view(torch.int32))


@pytest.mark.parametrize('w,H', [(5, 64), (128, 128)])
def test_two_launches_are_bit_identical(w, H):
    x, stages = _operands(w, H, 130, 9)
    adj = _plan(130)[4]
    xd, sd = x.to(DEV), _dev(stages)
    eps_dev = torch.tensor([EPS], device=DEV)
    for mode in ('aux', 'perm'):
        ed = _edge(130, w, mode)[0].to(DEV)
        a = _raw(xd, adj, ed, mode, eps_dev, sd, 'elu', 'elu')
        b = _raw(xd, adj, ed, mode, eps_dev, sd, 'elu', 'elu')
        assert torch.equal(a, b)
    assert torch.equal(a, _raw(xd, adj, _edge(130, w, 'aux')[0].to(DEV), 'aux', eps_dev, sd, 'elu', 'elu'))     # one code path


POISON = {'nan': float('nan'), '+inf': float('inf'), '-inf': float('-inf')}


@pytest.mark.parametrize('act', ['relu', 'elu'])
def test_non_finite_values(act):
    """One live NaN / +Inf / -Inf in x -- in a row that an entry lists as its source, which is also a self row -- and in e:
    the output's NaN and +-Inf masks are the float64 formula's (tests/_product.gate_nonfinite), a -Inf message (ReLU -> 0)
    leaves its row finite, and every row the formula does not change keeps the bits of the clean launch."""
    n, w, H = 70, 64, 64
    x, stages = _operands(w, H, n, 5)
    idx, shared, n_e, _, adj = _plan(n)
    e, _ = _edge(n, w, 'aux')
    sd = _dev(stages)
    eps_dev = torch.tensor([0.37], device=DEV)
    clean = _raw(x.to(DEV), adj, e.to(DEV), 'aux', eps_dev, sd, act, act)
    clean_ref = _gine.gine_formula64(x, idx, e, shared, 0.37, stages, act, act)
    # a source row that is listed by ANOTHER row, and an edge row that some entry reads
    p = next(p for p in range(idx.size(1)) if int(idx[0][p]) != int(idx[1][p]))
    s, c = int(idx[0][p]), int(shared[p])
    seen = dict.fromkeys(POISON, False)
    for poison, v in POISON.items():
        for place, xp, ep in ((f'x[{s}, 3]', _put(x, (s, 3), v), e), (f'e[{c}, 3]', x, _put(e, (c, 3), v))):
            out = _raw(xp.to(DEV), adj, ep.to(DEV), 'aux', eps_dev, sd, act, act)
            ref = _gine.gine_formula64(xp, idx, ep, shared, 0.37, stages, act, act)
            touched = ~(ref == clean_ref).all(dim=1)                       # (NaN != NaN: a poisoned row counts as touched)
            assert bool(touched.any()) and not bool(touched.all())
            if bool(torch.isfinite(ref).all()):
                gate(out, ref, f'gine_layer {act}, {poison} at {place} (finite reference)')
            else:
                gate_nonfinite(out, ref, f'gine_layer {act}, {poison} at {place}')
                seen[poison] = True
            assert torch.equal(out[~touched.to(DEV)], clean[~touched.to(DEV)]), 'a row the poison does not reach changed'
            if poison == '-inf' and place.startswith('e['):
                # the message relu(x_j - Inf) is 0 and nothing else reads e: every row stays finite
                assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(out).all())
    assert seen['nan'] and seen['+inf'], seen


def _put(t, index, value):
    t = t.clone()
    t[index] = value
    return t


def test_op_checks_on_device_operands():
    x, stages = _operands(8, 8, 10, 1)
    sd = _dev(stages)
    idx = _plan(10)[0]
    shared, n_e = _plan(10)[1], _plan(10)[2]
    adj = _plan(10)[4]
    e, _ = _edge(10, 8, 'aux')
    xd, ed = x.to(DEV), e.to(DEV)
    with pytest.raises(RuntimeError, match='inference only'):
        ops.gine_layer(xd.clone().requires_grad_(True), adj, ed, None, sd, 'relu')
    with pytest.raises(RuntimeError, match='inference only'):
        ops.gine_layer(xd, adj, ed.clone().requires_grad_(True), None, sd, 'relu')
    with torch.no_grad():
        y = ops.gine_layer(xd, adj, ed, 0.37, sd, 'relu')                       # a Python eps becomes a device float
        z = ops.gine_layer(xd, adj, ed[shared.to(DEV)], torch.tensor([EPS], device=DEV), sd, 'relu', edge_mode='perm')
        plain = csr.Adjacency.from_index(idx.to(DEV), 10, 10, build=False)       # no shared-cell index, not yet built
        zp = ops.gine_layer(xd, plain, ed[shared.to(DEV)], torch.tensor([EPS], device=DEV), sd, 'relu', edge_mode='perm')
        none = ops.gine_layer(xd, None, None, 0.37, sd, 'relu')
        with pytest.raises(ValueError, match="needs an adjacency built with a shared-cell index"):
            ops.gine_layer(xd, plain, ed, None, sd, 'relu')
        with pytest.raises(ValueError, match='edge has 3 rows'):
            ops.gine_layer(xd, adj, ed[:3], None, sd, 'relu')
        with pytest.raises(ValueError, match='edge has 5 rows'):
            ops.gine_layer(xd, adj, ed, None, sd, 'relu', edge_mode='perm')
        with pytest.raises(ValueError, match='its width must be that of x'):
            ops.gine_layer(xd, adj, ed[:, :4].contiguous(), None, sd, 'relu')
        with pytest.raises(ValueError, match='edge is None'):
            ops.gine_layer(xd, adj, None, None, sd, 'relu')
        with pytest.raises(TypeError, match='float64'):
            ops.gine_layer(xd.double(), adj, ed, None, sd, 'relu')
        with pytest.raises(ValueError):
            ops.gine_layer(xd, adj, ed, None, sd, 'relu', out=torch.empty(10, 9, device=DEV))
    gate(y, _gine.gine_formula64(x, idx, e, shared, 0.37, stages, 'relu'), 'python eps')
    gate(z, _gine.gine_formula64(x, idx, e, shared, EPS, stages, 'relu'), 'perm')
    assert torch.equal(z, zp)
    gate(none, _gin.gin_formula64(x, None, 0.37, stages, 'relu'), 'no adjacency')
    assert n_e == 5
    old = dict(_ffi.DYN_ROWS)
    _ffi.DYN_ROWS[10] = 0
    try:
        with torch.no_grad(), pytest.raises(RuntimeError, match='dynamic_rows'):
            ops.gine_layer(xd, adj, ed, None, sd, 'relu')
    finally:
        _ffi.DYN_ROWS.clear()
        _ffi.DYN_ROWS.update(old)


# ---- layers.GINEConv -------------------------------------------------------------------------------------------------------------
def _conv(w, H, act='relu', norm='bn', train_eps=True, seed=0):
    torch.manual_seed(seed)
    net = models._gin_network(w, H, models.get_graph_norm(norm), models.get_nonlinearity(act, return_module=True))
    conv = layers.GINEConv(net, eps=0.2, train_eps=train_eps)
    return _gin.randomise(conv, seed + 1).to(DEV).eval()


class _Counter:
    """Counts the calls of two entry points by wrapping the _ffi functions that issue them."""

    def __enter__(self):
        self.fused = self.aggregate = 0
        self._g, self._a = _ffi.gine_layer, _ffi.aggregate

        def gine(*a, **k):
            self.fused += 1
            return self._g(*a, **k)

        def aggregate(descs, device, dtype=torch.float32):
            self.aggregate += 1
            return self._a(descs, device, dtype)
        _ffi.gine_layer, _ffi.aggregate = gine, aggregate
        return self

    def __exit__(self, *exc):
        _ffi.gine_layer, _ffi.aggregate = self._g, self._a
        return False


@pytest.mark.parametrize('w,H,act', [(12, 16, 'tanh'), (64, 64, 'relu'), (5, 128, 'elu')])
def test_gine_conv_fused_against_generic(fused_on, w, H, act):
    """Both routes, with the edge features as IndexedRows and as a dense [E, w] tensor: each inside the gate of float64, and
    of each other; the fused route is one cwn_gine_layer_f32 call, the generic route one aggregation call."""
    conv = _conv(w, H, act)
    idx, shared, n_e, _, _ = _plan(130)
    e, _ = _edge(130, w, 'aux')
    x = XSCALE * torch.randn(130, w, generator=torch.Generator().manual_seed(1))
    xd, idxd, ed, sharedd = x.to(DEV), idx.to(DEV), e.to(DEV), shared.to(DEV)
    holder = torch.nn.ModuleDict({'c': conv})
    ref = _gine.conv64(_gin.state64(holder), 'c', x.double(), idx, e.double(), shared, act)
    for name, attr in (('IndexedRows', IndexedRows(ed, sharedd)), ('dense', ed[sharedd])):
        with torch.no_grad():
            layers.FUSED_GINE = True
            with _Counter() as c:
                a = conv(xd, idxd, attr)
            assert conv.last_route == 'fused' and (c.fused, c.aggregate) == (1, 0)
            layers.FUSED_GINE = False
            with _Counter() as c:
                b = conv(xd, idxd, attr)
            assert conv.last_route == 'generic' and (c.fused, c.aggregate) == (0, 1)
        gate(a, ref, f'fused against float64, {name}')
        gate(b, ref, f'generic against float64, {name}')
        gate(a, b.double(), f'fused against generic, {name}')


def test_gine_conv_routes(fused_on):
    idx, shared = _plan(70)[0].to(DEV), _plan(70)[1].to(DEV)
    x = XSCALE * torch.randn(70, 12, device=DEV)
    attr = IndexedRows(_edge(70, 12, 'aux')[0].to(DEV), shared)
    conv = _conv(12, 16)
    with torch.no_grad():
        conv(x, idx, attr)
        assert conv.last_route == 'fused'
        conv(x, None, None)                                 # a graph without edges
        assert conv.last_route == 'fused'
    with torch.enable_grad():
        conv(x, idx, attr)
        assert conv.last_route == 'generic'
    with torch.no_grad():
        conv.train()
        conv(x, idx, attr)
        assert conv.last_route == 'generic'                 # BatchNorm on batch statistics does not fold
        conv.eval()
        ln = _conv(12, 16, norm='ln')
        ln(x, idx, attr)
        assert ln.last_route == 'generic'
        idn = _conv(12, 16, norm='id')
        idn(x, idx, attr)
        assert idn.last_route == 'fused'
        dbl = _conv(12, 16).double()
        y = dbl(x.double(), idx, IndexedRows(attr.src.double(), shared))
        assert dbl.last_route == 'generic' and y.dtype == torch.float64
        narrow = conv(x, idx, attr.tensor()[:, :1].contiguous())         # an edge width of 1: the formula in plain torch
        assert conv.last_route == 'generic' and tuple(narrow.shape) == (70, 16)
        cpu = _conv(12, 16).cpu()
        cpu(x.cpu(), idx.cpu(), IndexedRows(attr.src.cpu(), shared.cpu()))
        assert cpu.last_route == 'generic'
        wide = _conv(12, 136)
        wide(x, idx, attr)
        assert wide.last_route == 'generic'
        layers.FUSED_GINE = False
        conv(x, idx, attr)
        assert conv.last_route == 'generic'


@pytest.mark.parametrize('lazy', [True, False], ids=['IndexedRows', 'dense'])
@pytest.mark.parametrize('w,H,act', [(12, 16, 'tanh'), (64, 64, 'relu')])
def test_generic_route_gradients_against_float64(w, H, act, lazy):
    """x, the edge features, every weight and the trained eps: the GPU's generic route (ops.aggregate + the torch modules)
    under autograd against float64 CPU autograd of the restatement (eval-mode BatchNorm)."""
    conv = _conv(w, H, act, train_eps=True)
    idx, shared, _, _, _ = _plan(130)
    g = torch.Generator().manual_seed(4)
    x, G = XSCALE * torch.randn(130, w, generator=g), torch.randn(130, H, generator=g)
    e = _edge(130, w, 'aux' if lazy else 'perm')[0]
    xd, ed = x.to(DEV).requires_grad_(True), e.to(DEV).requires_grad_(True)
    y = conv(xd, idx.to(DEV), IndexedRows(ed, shared.to(DEV)) if lazy else ed)
    assert conv.last_route == 'generic'
    (y * G.to(DEV)).sum().backward()
    holder = torch.nn.ModuleDict({'c': conv})
    st = _gin.state64(holder)
    names = [k for k, _ in holder.named_parameters()]
    assert 'c.eps' in names
    for k in names:
        st[k].requires_grad_(True)
    x64, e64 = x.double().requires_grad_(True), e.double().requires_grad_(True)
    ref = _gine.conv64(st, 'c', x64, idx, e64, shared if lazy else 'perm', act)
    (ref * G.double()).sum().backward()
    gate(y, ref, 'forward')
    gate(xd.grad, x64.grad, 'dx')
    gate(ed.grad, e64.grad, 'de')
    for k, p in holder.named_parameters():
        gate(p.grad, st[k].grad, f'd{k}')


# ---- models.EmbedGIN -----------------------------------------------------------------------------------------------------------------
_MOLS = {}


def _molecules():
    """8 synthetic molecules collated up to dimension 1, on the CPU (built once)."""
    if 'b' not in _MOLS:
        _MOLS['b'] = ComplexBatch.from_complex_list(synthetic.zinc_like_complexes(8, seed=3), max_dim=1)
    return _MOLS['b']


@pytest.mark.parametrize('case', ['molecules', 'dummy', 'dummy_no_edge_features', 'fullstop'])
def test_embed_gin_on_the_device_against_the_float64_restatement(fused_on, case):
    """eval(), fused and generic: inside the gate of the restatement; L fused launches and the readout's aggregation alone,
    then no fused launch and L + 1 aggregations (a complex without any edge: the layers' self terms)."""
    batch = {'molecules': _molecules, 'dummy': lambda: host.cpu_batch(host.MIXED, True),
             'dummy_no_edge_features': lambda: host.cpu_batch(host.MIXED, False),
             'fullstop': lambda: host.cpu_batch(['fullstop'], False)}[case]()
    model = host.make_model('relu', 'mean' if case == 'dummy' else 'sum', train_eps=True,
                            embed_edge=case in ('molecules', 'dummy'), seed=9)
    ref = _gine.embed_gin64_of(_gin.state64(model), batch, readout=model.readout)
    assert float(ref.abs().max()) > 1e-3
    model = model.to(DEV)
    for fused in (True, False):
        layers.FUSED_GINE = fused
        with _Counter() as c, torch.no_grad():
            out = model(host.fresh(batch).to(DEV))
        assert all(conv.last_route == ('fused' if fused else 'generic') for conv in model.convs)
        assert c.fused == (host.LAYERS if fused else 0)
        gate(out, ref, f'EmbedGIN on {case}, {"fused" if fused else "generic"}')


def test_one_optimisation_step_of_embed_gin_moves_every_parameter():
    torch.manual_seed(0)
    model = models.EmbedGIN(28, 4, 1, num_layers=2, hidden=16, train_eps=True, embed_edge=True, dropout_rate=0.1).to(DEV).train()
    batch = host.fresh(_molecules()).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    loss = torch.nn.functional.mse_loss(model(batch).view(-1), batch.y.view(-1).float())
    loss.backward()
    opt.step()
    assert bool(torch.isfinite(loss))
    assert all(c.last_route == 'generic' for c in model.convs)
    for k, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        assert not torch.equal(p.detach(), before[k]), f'{k} did not move'
