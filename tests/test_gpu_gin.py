"""The graph baselines on the device: cwn_gin_layer_f32 (csrc/cwn_gin.hip) against a float64 evaluation of

    s = A x + (1 + eps) x,   h = act((s W1^T + b1) scale1 + shift1),   out = act_post(act((h W2^T + b2) scale2 + shift2))

strided operands inside one buffer, bit-reproducibility, the two routes of layers.GINConv, the generic route's gradients
against float64 CPU autograd, and the five models against the float64 restatement of tests/_gin.py with the proof of which
launches they make.  The bar everywhere is tests/_product.gate: max|delta| <= 1e-5 * max(1, |ref|_inf).

Shapes: widths (1,64) (3,5) (5,64) (12,12) (64,64) (100,128) (128,128) -- vector and scalar weight loads, masked edge columns,
K not a multiple of 16, the widest panel; rows 0, 1, one below / at / above CWN_GIN_TM and 130: nothing, a partial tile, a full
tile, several tiles.  The plans hold empty rows and rows of exactly CWN_LONG_ROW, CWN_LONG_ROW + 1 and 300 entries.

Input scale.  The sum s is specified in CSR order, and float32's own rounding in such a sum of 300 terms is about 3e-7 of |s|.
With unit-variance x the 300-entry row reaches |s| = 185 at n = 32 (its sources are 32 rows, drawn with repetition), and a plain
float32 evaluation of the formula in the same order on the CPU -- exact fma chains, no kernel -- is then 1.07e-5 away from float64
behind a saturating activation (|ref|_inf = 1) at (w, H, n) = (100, 128, 32), tanh, scale / shift, no bias; the launch measured
1.10e-5 there.  So the features are drawn at XSCALE = 1/64: |s| stays within a few units and the number format's own error an
order of magnitude below the bar, which is left where it is."""
import itertools
from types import SimpleNamespace

import pytest
import torch

from cwn_amd import _ffi, csr, layers, models, ops, synthetic
from cwn_amd.complex import ComplexBatch
from tests import _gin
from tests import test_gin_host as host
from tests._product import gate

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
ACTS = ('id', 'relu', 'elu', 'tanh', 'sigmoid')
WIDTHS = ((1, 64), (3, 5), (5, 64), (12, 12), (64, 64), (100, 128), (128, 128))
TM = _ffi.GIN_TM
ROWS = (0, 1, TM - 1, TM, TM + 1, 130)
EPS = 0.37
XSCALE = 1.0 / 64          # see "Input scale" above


@pytest.fixture
def fused_on():
    old, layers.FUSED_GIN = layers.FUSED_GIN, True
    yield
    layers.FUSED_GIN = old


_PLANS = {}


def _plan(n: int):
    """(index on the CPU, built Adjacency) of the n-row case, shared by every test that needs it."""
    if n not in _PLANS:
        idx = _gin.index_like_oriented(n, 1000 * n + 7, csr.LONG_ROW)
        _PLANS[n] = (idx, csr.Adjacency.from_index(idx.to(DEV), n, n) if n else None)
    return _PLANS[n]


def _operands(w, H, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = XSCALE * torch.randn(n, w, generator=g)
    stages = []
    for k in (w, H):
        stages.append((torch.randn(H, k, generator=g) / k ** 0.5, 0.3 * torch.randn(H, generator=g),
                       1.0 + 0.3 * torch.randn(H, generator=g), 0.3 * torch.randn(H, generator=g)))
    return x, stages


def _pick(stages, bias: bool, norm: bool):
    return [(W, b if bias else None, sc if norm else None, sh if norm else None) for W, b, sc, sh in stages]


def _raw(x, adj, eps_dev, stages, act, act_post, out=None):
    """One cwn_gin_layer_f32 call on device tensors (x and out may be column slices)."""
    n, w = x.shape
    H = stages[0][0].size(0)
    out = torch.empty(n, H, device=DEV) if out is None else out
    d = _ffi.GinDesc(x=x.data_ptr(), eps_dev=_ffi.ptr(eps_dev), out=out.data_ptr(), n=n, ldx=x.stride(0) if n > 1 else w,
                     ldout=out.stride(0) if n > 1 else H, w=w, H=H, act=ops.ACT_CODES[act], act_post=ops.ACT_CODES[act_post])
    (d.W1, d.b1, d.scale1, d.shift1), (d.W2, d.b2, d.scale2, d.shift2) = [[_ffi.ptr(t) for t in s] for s in stages]
    if adj is not None and adj.n_entries:
        d.rowptr, d.col = adj.rowptr.data_ptr(), adj.col.data_ptr()
    _ffi.gin_layer(d, DEV)
    return out


@pytest.mark.parametrize('n', ROWS)
@pytest.mark.parametrize('w,H', WIDTHS)
def test_entry_point_against_float64(w, H, n):
    """At one (w, H, n): the five activations x act_post (id, the same activation) x with / without scale and shift x with /
    without biases x eps_dev (NULL, 0.37), each inside the gate of the float64 formula."""
    x, stages = _operands(w, H, n, w * 1000 + H * 10 + n)
    idx, adj = _plan(n)
    xd = x.to(DEV)
    sd = [tuple(t.to(DEV) for t in s) for s in stages]
    eps_dev = torch.tensor([EPS], device=DEV)
    for act, same, norm, bias, eps in itertools.product(ACTS, (False, True), (False, True), (False, True), (None, EPS)):
        post = act if same else 'id'
        out = _raw(xd, adj, None if eps is None else eps_dev, _pick(sd, bias, norm), act, post)
        assert tuple(out.shape) == (n, H)
        if n == 0:                              # nothing to launch, and nothing launched: CWN_OK, an empty result
            continue
        ref = _gin.gin_formula64(x, idx, eps or 0.0, _pick(stages, bias, norm), act, post)
        gate(out, ref, f'w={w} H={H} n={n} act={act} post={post} norm={norm} bias={bias} eps={eps}')


def test_rows_without_entries_get_the_self_term_and_no_plan_means_no_edges():
    x, stages = _operands(12, 12, 70, 5)
    idx, adj = _plan(70)
    deg = torch.bincount(idx[1], minlength=70)
    assert int((deg == 0).sum()) > 5
    xd, sd = x.to(DEV), [tuple(t.to(DEV) for t in s) for s in stages]
    eps_dev = torch.tensor([EPS], device=DEV)
    out = _raw(xd, adj, eps_dev, sd, 'tanh', 'id')
    alone = _raw(xd, None, eps_dev, sd, 'tanh', 'id')
    gate(alone, _gin.gin_formula64(x, None, EPS, stages, 'tanh'), 'no plan')
    assert torch.equal(out[deg == 0], alone[deg == 0])


@pytest.mark.parametrize('w,H,x0,o0,n', [(64, 64, 0, 64, 130), (12, 20, 3, 17, 70), (100, 128, 128, 0, 33), (5, 7, 9, 1, 1)])
def test_strided_operands_inside_one_buffer(w, H, x0, o0, n):
    """x is a column slice of a wider buffer and out another slice of the same buffer (16-byte aligned and not): the output inside
    the gate, every element outside the out slice untouched bit for bit."""
    width = max(x0 + w, o0 + H) + 5
    x, stages = _operands(w, H, n, 77 + w)
    idx, adj = _plan(n)
    buf = torch.full((n, width), float('nan'), device=DEV)      # (NaN around the x slice: a load that strays shows in out)
    buf[:, x0:x0 + w] = x.to(DEV)
    before = buf.clone()
    sd = [tuple(t.to(DEV) for t in s) for s in stages]
    out = _raw(buf[:, x0:x0 + w], adj, None, sd, 'relu', 'id', out=buf[:, o0:o0 + H])
    assert not torch.isnan(out).any(), 'a NaN beside the x slice reached the output'
    gate(out, _gin.gin_formula64(x, idx, 0.0, stages, 'relu'), f'strided {w}x{H}')
    keep = torch.ones(width, dtype=torch.bool, device=DEV)
    keep[o0:o0 + H] = False
    assert torch.equal(buf[:, keep].view(torch.int32), before[:, keep].view(torch.int32)), 'an element outside the slice was written'
    # the op does the same through its `out` argument
    buf2 = before.clone()
    with torch.no_grad():
        got = ops.gin_layer(buf2[:, x0:x0 + w], adj, None, sd, 'relu', out=buf2[:, o0:o0 + H])
    assert got.data_ptr() == buf2.data_ptr() + 4 * o0 and torch.equal(buf2.view(torch.int32), buf.view(torch.int32))


@pytest.mark.parametrize('w,H', [(5, 64), (128, 128)])
def test_two_launches_are_bit_identical(w, H):
    x, stages = _operands(w, H, 130, 9)
    _, adj = _plan(130)
    xd, sd = x.to(DEV), [tuple(t.to(DEV) for t in s) for s in stages]
    eps_dev = torch.tensor([EPS], device=DEV)
    a = _raw(xd, adj, eps_dev, sd, 'elu', 'elu')
    b = _raw(xd, adj, eps_dev, sd, 'elu', 'elu')
    assert torch.equal(a, b)


def test_op_raises_under_a_recording_autograd_and_on_other_dtypes():
    x, stages = _operands(8, 8, 10, 1)
    sd = [tuple(t.to(DEV) for t in s) for s in stages]
    xd = x.to(DEV).requires_grad_(True)
    with pytest.raises(RuntimeError, match='inference only'):
        ops.gin_layer(xd, None, None, sd, 'relu')
    with torch.no_grad():
        y = ops.gin_layer(xd, None, 0.37, sd, 'relu')       # an unbuilt plan is built, a Python eps becomes a device float
        adj = csr.Adjacency.from_index(_plan(10)[0].to(DEV), 10, 10, build=False)
        z = ops.gin_layer(xd, adj, torch.tensor([EPS], device=DEV), sd, 'relu')
    gate(y, _gin.gin_formula64(x, None, 0.37, stages, 'relu'), 'python eps')
    gate(z, _gin.gin_formula64(x, _plan(10)[0], EPS, stages, 'relu'), 'unbuilt plan')
    with pytest.raises(TypeError, match='float64'):
        ops.gin_layer(x.to(DEV).double(), None, None, sd, 'relu')
    with pytest.raises(ValueError):
        ops.gin_layer(x.to(DEV), None, None, sd, 'relu', out=torch.empty(10, 9, device=DEV))


def test_operands_without_contiguous_rows_are_refused_with_their_whole_message():
    """The shape / stride clause of the operand check (the dtype and device clauses: tests/test_operand_messages_host.py), the
    messages as literals recorded before the ops shared one checker.  Nothing is launched."""
    z = lambda *s: torch.zeros(*s, device=DEV)
    gin = lambda x, W1=None, b1=None: ops.gin_layer(x, None, None, [(z(5, 3) if W1 is None else W1, b1, None, None),
                                                                    (z(5, 5), None, None, None)], 'relu')
    cases = [
        (lambda: gin(z(3, 4).t()), 'gin_layer: x must be a 2-D float32 tensor with contiguous rows (shape (4, 3), strides (1, 4))'),
        (lambda: gin(z(4, 3), W1=z(3)), 'gin_layer: W1 must be a 2-D float32 tensor with contiguous rows (shape (3,), strides (1,))'),
        (lambda: gin(z(4, 3), b1=z(5, 1)),
         'gin_layer: b1 must be a 1-D float32 tensor with contiguous rows (shape (5, 1), strides (1, 1))'),
    ]
    for call, message in cases:
        with pytest.raises(TypeError) as got:
            call()
        assert type(got.value) is TypeError and str(got.value) == message
    assert not ops.gin_layer_applies(z(3, 4).t(), [(z(5, 3), None, None, None), (z(5, 5), None, None, None)])


# ---- layers.GINConv -------------------------------------------------------------------------------------------------------------
def _conv(w, H, act='relu', norm='bn', train_eps=True, seed=0):
    torch.manual_seed(seed)
    net = models._gin_network(w, H, models.get_graph_norm(norm), models.get_nonlinearity(act, return_module=True))
    conv = layers.GINConv(net, eps=0.2, train_eps=train_eps)
    return _gin.randomise(conv, seed + 1).to(DEV).eval()


@pytest.mark.parametrize('w,H,act', [(12, 16, 'tanh'), (64, 64, 'relu'), (5, 128, 'elu')])
def test_gin_conv_fused_against_generic(fused_on, w, H, act):
    conv = _conv(w, H, act)
    idx, adj = _plan(130)
    x = XSCALE * torch.randn(130, w, generator=torch.Generator().manual_seed(1))
    xd, idxd = x.to(DEV), idx.to(DEV)
    with torch.no_grad():
        a = conv(xd, idxd)
        assert conv.last_route == 'fused'
        layers.FUSED_GIN = False
        b = conv(xd, idxd)
        assert conv.last_route == 'generic'
    holder = torch.nn.ModuleDict({'c': conv})
    ref = _gin.conv64(_gin.state64(holder), 'c', x.double(), idx, act)
    gate(a, ref, 'fused against float64')
    gate(b, ref, 'generic against float64')
    gate(a, b.double(), 'fused against generic')


def test_gin_conv_routes(fused_on):
    idx = _plan(70)[0].to(DEV)
    x = XSCALE * torch.randn(70, 12, device=DEV)
    conv = _conv(12, 16)
    with torch.no_grad():
        conv(x, idx)
        assert conv.last_route == 'fused'
        conv(x, None)                                       # a graph without edges
        assert conv.last_route == 'fused'
    with torch.enable_grad():
        conv(x, idx)
        assert conv.last_route == 'generic'
    with torch.no_grad():
        conv.train()
        conv(x, idx)
        assert conv.last_route == 'generic'                 # BatchNorm on batch statistics does not fold
        conv.eval()
        ln = _conv(12, 16, norm='ln')
        ln(x, idx)
        assert ln.last_route == 'generic'
        idn = _conv(12, 16, norm='id')
        idn(x, idx)
        assert idn.last_route == 'fused'
        dbl = _conv(12, 16).double()
        y = dbl(x.double(), idx)
        assert dbl.last_route == 'generic' and y.dtype == torch.float64
        custom = layers.GINConv(torch.nn.Linear(12, 16)).to(DEV).eval()
        custom(x, idx)
        assert custom.last_route == 'generic'
        wide = _conv(12, 136)
        wide(x, idx)
        assert wide.last_route == 'generic'
        layers.FUSED_GIN = False
        conv(x, idx)
        assert conv.last_route == 'generic'


@pytest.mark.parametrize('w,H,act', [(12, 16, 'tanh'), (64, 64, 'relu')])
def test_generic_route_gradients_against_float64(w, H, act):
    """x, every weight and the trained eps: the GPU's generic route (ops.aggregate + the torch modules) under autograd against
    float64 CPU autograd of the restatement (eval-mode BatchNorm)."""
    conv = _conv(w, H, act, train_eps=True)
    idx, _ = _plan(130)
    g = torch.Generator().manual_seed(4)
    x, G = XSCALE * torch.randn(130, w, generator=g), torch.randn(130, H, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    y = conv(xd, idx.to(DEV))
    assert conv.last_route == 'generic'
    (y * G.to(DEV)).sum().backward()
    holder = torch.nn.ModuleDict({'c': conv})
    st = _gin.state64(holder)
    names = [k for k, _ in holder.named_parameters()]
    assert 'c.eps' in names
    for k in names:
        st[k].requires_grad_(True)
    x64 = x.double().requires_grad_(True)
    ref = _gin.conv64(st, 'c', x64, idx, act)
    (ref * G.double()).sum().backward()
    gate(y, ref, 'forward')
    gate(xd.grad, x64.grad, 'dx')
    for k, p in holder.named_parameters():
        gate(p.grad, st[k].grad, f'd{k}')


# ---- models -------------------------------------------------------------------------------------------------------------------------
class _Counter:
    """Counts the calls of two entry points by wrapping the _ffi functions that issue them."""

    def __enter__(self):
        self.fused = self.aggregate = 0
        self._g, self._a = _ffi.gin_layer, _ffi.aggregate

        def gin(*a, **k):
            self.fused += 1
            return self._g(*a, **k)

        def aggregate(descs, device, dtype=torch.float32):
            self.aggregate += 1
            return self._a(descs, device, dtype)
        _ffi.gin_layer, _ffi.aggregate = gin, aggregate
        return self

    def __exit__(self, *exc):
        _ffi.gin_layer, _ffi.aggregate = self._g, self._a
        return False


def _on_device(ns):
    return SimpleNamespace(**{k: v.to(DEV) for k, v in vars(ns).items()})


@pytest.mark.parametrize('name,mode', host.MODELS)
def test_models_on_the_device_against_the_float64_restatement(fused_on, name, mode):
    """eval() on ring_transfer(10, 10), collated and as a plain namespace: inside the gate of the restatement; L fused launches
    and no aggregation launch but the readout's (none at all for RingGIN); with the switch off no fused launch."""
    torch.manual_seed(11)
    act = 'tanh' if name == 'RingGIN' else 'relu'
    kw = dict(nonlinearity=act) if name == 'RingGIN' else dict(nonlinearity=act, readout='mean' if mode == 'max' else 'sum')
    model = _gin.randomise(host._make(name, mode, **kw), 3).eval()
    _, ns = host._ring()
    ref = host.reference64(name, mode, model, ns, act, kw.get('readout', 'sum'))
    model = model.to(DEV)
    readout = 0 if name == 'RingGIN' else 1
    for data in (host._ring_batch().to(DEV), _on_device(ns)):
        with _Counter() as c, torch.no_grad():
            out = model(data)
        assert (c.fused, c.aggregate) == (host.LAYERS, readout), (c.fused, c.aggregate)
        gate(out, ref, f'{name}[{mode}] fused on {type(data).__name__}')
    layers.FUSED_GIN = False
    with _Counter() as c, torch.no_grad():
        out = model(host._ring_batch().to(DEV))
    assert (c.fused, c.aggregate) == (0, host.LAYERS + readout)
    gate(out, ref, f'{name}[{mode}] generic')


@pytest.mark.parametrize('name', ['GIN0WithJK', 'GINWithJK'])
def test_jumping_knowledge_cat_is_one_buffer(fused_on, name, monkeypatch):
    """Layer l writes columns [l H, (l + 1) H) of one [n, L H] buffer and layer l + 1 reads them in place: no torch.cat."""
    model = _gin.randomise(host._make(name, 'cat'), 5).to(DEV).eval()
    seen = []
    for conv in [model.conv1] + list(model.convs):
        conv.register_forward_hook(lambda m, args, out: seen.append((args[0], out)))
    batch = host._ring_batch().to(DEV)
    L, H = host.LAYERS, host.HID
    made = []                                   # the shape of everything torch.cat makes during the forward
    real = torch.cat

    def cat(*a, **k):
        r = real(*a, **k)
        made.append(tuple(r.shape))
        return r
    monkeypatch.setattr(torch, 'cat', cat)
    with torch.no_grad():
        model(batch)
    monkeypatch.setattr(torch, 'cat', real)
    assert (100, L * H) not in made and len(seen) == L, made
    base = seen[0][1].data_ptr()
    for l, (xin, out) in enumerate(seen):
        assert out.data_ptr() == base + 4 * l * H and tuple(out.shape) == (100, H) and out.stride() == (L * H, 1)
        if l:
            assert xin.data_ptr() == seen[l - 1][1].data_ptr() and xin.stride() == (L * H, 1)


def test_receptive_field_on_the_device(fused_on):
    """The fused launch on the collated batch and one complex at a time; the generic route (rocBLAS behind the modules) one
    complex at a time -- see tests/test_gin_host.py::receptive_field."""
    host.check_receptive_field(host.receptive_field(DEV, fused='fused', batched=True))
    host.check_receptive_field(host.receptive_field(DEV, fused='fused'))
    layers.FUSED_GIN = False
    host.check_receptive_field(host.receptive_field(DEV))


def test_one_optimisation_step_of_ring_gin_moves_every_parameter():
    torch.manual_seed(0)
    model = models.RingGIN(num_features=5, num_layers=5, hidden=16, num_classes=5).to(DEV).train()
    batch = host._ring_batch(10, 10).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    loss = torch.nn.functional.cross_entropy(model(batch), batch.y.view(-1))
    loss.backward()
    opt.step()
    assert bool(torch.isfinite(loss))
    assert all(c.last_route == 'generic' for c in [model.conv1] + list(model.convs))
    for k, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        assert not torch.equal(p.detach(), before[k]), f'{k} did not move'
