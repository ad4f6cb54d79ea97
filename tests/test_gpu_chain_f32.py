"""The float32 update chain on the device: cwn_update_chain_f32 (csrc/cwn_chain_f32.hip) behind ops.update_chain_f32 against
float64 torch on the CPU, bit for bit against itself (a row alone, a second launch, a device-side row count), with
non-finite inputs, and under the layers and models that take it (layers.FUSED_CHAIN_F32).

The bar is the project's own (tests/_product.gate): max|delta| <= 1e-5 * max(1, |ref|_inf).  The operands are the ones the
bar was checked with on plain float32 torch (worst 0.13 of the bound, tanh at 128 x 128): inputs 2 randn, weights
randn / sqrt(K), biases and shifts 0.3 randn, scales 1 + 0.3 randn."""
import copy
import math

import pytest
import torch

from tests._product import gate, gate_nonfinite

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
F32, F64 = torch.float32, torch.float64
ACTS = ('id', 'relu', 'elu', 'tanh', 'sigmoid')
ACT_FN = {'id': lambda t: t, 'relu': torch.relu, 'elu': torch.nn.functional.elu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}
# scalar and vector weight loads, K not a multiple of 16, a combine K of 10 / 96 / 256, the widest panel
WIDTHS = [(1, 16), (3, 5), (5, 48), (12, 12), (48, 48), (64, 64), (100, 128), (128, 128)]
SENT = -9.0
CAP = 200
LIVES = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128, 129, 199, 200)     # tests/test_gpu_row_counts.py


@pytest.fixture(scope='module', autouse=True)
def _native_loaded():
    from cwn_amd import _ffi
    assert _ffi.lib().cwn_target_arch() == b'gfx950'
    assert torch.cuda.is_available()


class _Net:
    """The five stages of one dimension: float32 values held on the CPU (the float64 reference reads exactly them) and on
    the device.  bias / scale / shift: which of the per-stage vectors exist."""

    def __init__(self, F, H, seed, bias=True, scale=True, shift=True):
        g = torch.Generator().manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=g)
        self.F, self.H = F, H
        self.W = [r(H, K) / math.sqrt(K) for K in (F, H, F, H, 2 * H)]
        self.b = [0.3 * r(H) if bias else None for _ in range(5)]
        self.scale = [1 + 0.3 * r(H) if scale else None for _ in range(5)]
        self.shift = [0.3 * r(H) if shift else None for _ in range(5)]
        dev = lambda ts: [None if t is None else t.to(DEV) for t in ts]
        self.dW, self.db, self.dscale, self.dshift = dev(self.W), dev(self.b), dev(self.scale), dev(self.shift)

    def inputs(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        return 2 * torch.randn(n, self.F, generator=g), 2 * torch.randn(n, self.F, generator=g)

    def dim(self, in_up, in_b, act, out=None):
        from cwn_amd import ops
        return ops.ChainDim(in_up=in_up, in_b=in_b, weights=self.dW, biases=self.db, folds=list(zip(self.dscale, self.dshift)),
                            act=act, out=out)

    def reference(self, in_up, in_b, act):
        """float64 torch on the CPU."""
        def stage(x, s):
            z = x @ self.W[s].double().t()
            for t, op in ((self.b[s], torch.add), (self.scale[s], torch.mul), (self.shift[s], torch.add)):
                if t is not None:
                    z = op(z, t.double())
            return ACT_FN[act](z)
        u = stage(stage(in_up.double(), 0), 1)
        b = stage(stage(in_b.double(), 2), 3)
        return stage(torch.cat([u, b], dim=-1), 4)


VARIANTS = [dict(), dict(bias=False, scale=False, shift=False), dict(scale=False, shift=False), dict(bias=False),
            dict(shift=False), dict(scale=False)]


# ------------------------------------------------------------------------------------------------
# 1. the entry point against float64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,H', WIDTHS)
def test_update_chain_against_float64(F, H):
    """Every activation; launches of 1, 3 and 4 dimensions with rows from {0, 1, 31, 32, 33, 130} (a zero-row dimension among
    them), the dimensions with and without bias and with and without scale / shift; outputs into sentinel-filled buffers
    with three spare rows: live rows within the gate, spare rows untouched."""
    from cwn_amd import ops
    launches = [(130,), (1, 0, 33), (31, 32, 0, 130), (0,)]
    nets = [_Net(F, H, seed=100 * F + H + v, **kw) for v, kw in enumerate(VARIANTS)]
    k = 0
    for a, act in enumerate(ACTS):
        for rows in launches:
            dims, refs, bufs = [], [], []
            for d, n in enumerate(rows):
                net = nets[k % len(nets)]
                k += 1
                in_up, in_b = net.inputs(n, seed=7 * n + d + a)
                refs.append(net.reference(in_up, in_b, act))
                bufs.append(torch.full((n + 3, H), SENT, device=DEV))
                dims.append(net.dim(in_up.to(DEV), in_b.to(DEV), act, out=bufs[-1]))
            assert ops.update_chain_f32_applies(dims)
            outs = ops.update_chain_f32(dims)
            for d, (n, y, ref, buf) in enumerate(zip(rows, outs, refs, bufs)):
                assert y.dtype == F32 and y.shape == (n, H) and (n == 0 or y.data_ptr() == buf.data_ptr()), (act, rows, d)
                assert bool((buf[n:] == SENT).all()), (act, rows, d)                        # spare rows untouched
                gate(buf[:n], ref, f'update_chain_f32 F {F} H {H} {act} rows {rows} dim {d}')


def test_update_chain_allocates_its_outputs_and_takes_strided_operands():
    """Row-strided inputs (column slices of wider buffers, one of them off 16 bytes), `out` as a row-strided view of a wider
    buffer whose other columns stay as they were, and an output of the op's own."""
    from cwn_amd import ops
    for F, H in ((5, 48), (48, 48), (100, 128)):
        net, n = _Net(F, H, seed=3), 70
        g = torch.Generator().manual_seed(4)
        wide_up, wide_b = 2 * torch.randn(n, F + 9, generator=g), 2 * torch.randn(n, F + 4, generator=g)
        wide_up[:, :3] = wide_up[:, 3 + F:] = wide_b[:, F:] = float('nan')     # (beside the windows: nothing of it reaches a result)
        in_up, in_b = wide_up.to(DEV)[:, 3:3 + F], wide_b.to(DEV)[:, :F]
        assert in_up.stride(0) == F + 9 and in_b.stride(0) == F + 4
        ref = net.reference(wide_up[:, 3:3 + F], wide_b[:, :F], 'elu')
        y, = ops.update_chain_f32([net.dim(in_up, in_b, 'elu')])
        assert y.shape == (n, H) and y.is_contiguous()
        gate(y, ref, f'update_chain_f32 F {F} H {H}: strided inputs, own output')
        for off in (4, 1):                                                        # 16-byte stores, and scalar ones
            wide_out = torch.full((n + 2, H + 8), SENT, device=DEV)
            view = wide_out[:, off:off + H]
            z, = ops.update_chain_f32([net.dim(in_up, in_b, 'elu', out=view)])
            assert z.data_ptr() == view.data_ptr() and z.stride(0) == H + 8
            assert torch.equal(z, y)
            keep = torch.ones_like(wide_out, dtype=torch.bool)
            keep[:n, off:off + H] = False
            assert bool((wide_out[keep] == SENT).all())


# ------------------------------------------------------------------------------------------------
# 2. row independence and reproducibility, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,H,act', [(48, 48, 'relu'), (100, 128, 'tanh')])
def test_a_row_has_the_same_bits_alone_and_in_any_batch(F, H, act):
    from cwn_amd import ops
    net, n = _Net(F, H, seed=11), 130
    in_up, in_b = (t.to(DEV) for t in net.inputs(n, seed=12))
    batch, = ops.update_chain_f32([net.dim(in_up, in_b, act)])
    again, = ops.update_chain_f32([net.dim(in_up, in_b, act)])
    assert torch.equal(batch, again)                                              # two launches on the same operands
    alone = torch.cat([ops.update_chain_f32([net.dim(in_up[r:r + 1], in_b[r:r + 1], act)])[0] for r in range(n)])
    assert torch.equal(batch, alone)
    other = _Net(5, 16, seed=13)
    o_up, o_b = (t.to(DEV) for t in other.inputs(37, seed=14))
    _, _, third = ops.update_chain_f32([other.dim(o_up, o_b, 'elu'), other.dim(o_up[:0], o_b[:0], 'elu'), net.dim(in_up, in_b, act)])
    assert torch.equal(batch, third)                                              # ... in another slot of a wider launch
    gate(batch, net.reference(in_up.cpu(), in_b.cpu(), act), f'update_chain_f32 F {F} H {H} {act}, 130 rows')


# ------------------------------------------------------------------------------------------------
# 3. the device-side row count
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,H', [(48, 48), (100, 128)])
def test_device_side_row_count(F, H):
    """include/cwn_hip.h, "DEVICE-SIDE ROW COUNTS": capacity-sized operands whose rows at or beyond the count hold NaN, the
    count in a device int64.  Live rows are within the gate and bit-identical to the same call with n = live and no
    m_dev; rows at or beyond the count keep the sentinel; a count of 0 writes nothing; a count beyond the capacity
    behaves as the capacity."""
    from cwn_amd import _ffi, ops
    net = _Net(F, H, seed=21)
    in_up, in_b = net.inputs(CAP, seed=22)
    ref = net.reference(in_up, in_b, 'elu')
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    for live in LIVES + (CAP + 50,):
        rows = min(live, CAP)
        up, b = in_up.clone(), in_b.clone()
        up[rows:], b[rows:] = float('nan'), float('nan')
        up, b = up.to(DEV), b.to(DEV)
        out = torch.full((CAP + 4, H), SENT, device=DEV)
        count.fill_(live)
        with _ffi.dynamic_rows({CAP: count.data_ptr()}):
            y, = ops.update_chain_f32([net.dim(up, b, 'elu', out=out)])
        assert y.shape == (CAP, H)
        assert bool((out[rows:] == SENT).all()), f'a row at or beyond the live count {live} was written'
        static, = ops.update_chain_f32([net.dim(up[:rows], b[:rows], 'elu')])
        assert torch.equal(out[:rows], static), live
        gate(out[:rows], ref[:rows], f'update_chain_f32 F {F} H {H}, {live} live rows of {CAP}')
    # a capacity that is not a key of the mapping: a host count, as without the context
    count.fill_(3)
    with _ffi.dynamic_rows({CAP + 1: count.data_ptr()}):
        y, = ops.update_chain_f32([net.dim(in_up.to(DEV), in_b.to(DEV), 'elu')])
    gate(y, ref, 'update_chain_f32 under a mapping without its capacity')


# ------------------------------------------------------------------------------------------------
# 4. non-finite inputs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', ['relu', 'tanh'])
@pytest.mark.parametrize('F,H', [(12, 12), (48, 48)])
def test_non_finite_inputs_come_out_where_float64_torch_puts_them(F, H, act):
    """A NaN, a +Inf and a -Inf in single input rows (one of them in the boundary input, one in the second tile): non-finite
    outputs exactly in the rows where float64 torch has them, every other row within the gate."""
    from cwn_amd import ops
    net, n = _Net(F, H, seed=31), 70
    in_up, in_b = net.inputs(n, seed=32)
    in_up[3, F // 2], in_b[40, 0], in_up[66, F - 1] = float('nan'), float('inf'), float('-inf')
    ref = net.reference(in_up, in_b, act)
    y, = ops.update_chain_f32([net.dim(in_up.to(DEV), in_b.to(DEV), act)])
    gate_nonfinite(y, ref, f'update_chain_f32 F {F} H {H} {act}: NaN / +Inf / -Inf input rows')
    clean = [r for r in range(n) if r not in (3, 40, 66)]
    assert bool(torch.isfinite(y[clean]).all()) and bool(torch.isnan(y[3]).all())


# ------------------------------------------------------------------------------------------------
# 5. layers and models
# ------------------------------------------------------------------------------------------------
class _Spy:
    """Counts the calls of the C entry point and passes them on."""

    def __init__(self, monkeypatch):
        from cwn_amd import _ffi
        self.calls = 0
        L = _ffi.lib()

        def spy(arr, n, s, fn=L.cwn_update_chain_f32):
            self.calls += 1
            assert 1 <= n <= 4
            return fn(arr, n, s)
        monkeypatch.setattr(L, 'cwn_update_chain_f32', spy)


def _model(hidden, nonlinearity, layers_=2, norm='bn', dtype=F32):
    from tests.test_gpu_f64_dense import _model as sr_model
    return sr_model(hidden, layers_, nonlinearity, norm, dtype=dtype)


def _batch(dtype=F32):
    from tests.test_gpu_f64_dense import _sr_batch
    return _sr_batch(dtype=dtype).to(DEV)


def _double(module):
    return copy.deepcopy(module).double()


CONFIGS = [(48, 'relu', 'relu_width'), (16, 'elu', 'act'), (64, 'elu', 'act')]


@pytest.mark.parametrize('hidden,nonlinearity,regime', CONFIGS, ids=[f'h{h}-{a}' for h, a, _ in CONFIGS])
def test_layer_route_on_matches_off_and_float64(monkeypatch, hidden, nonlinearity, regime):
    """One SparseCINConv (eval-mode BatchNorm with non-trivial statistics) over random features: the route on against the
    route off and each against the same layer in float64; the entry point is called once when on, never when off."""
    from cwn_amd import layers
    conv = _model(hidden, nonlinearity).convs[1]
    batch, batch64 = _batch(), _batch(F64)
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(batch.cochains[d].num_cells, hidden, generator=g) for d in range(3)]
    spy = _Spy(monkeypatch)

    def run(c, b, dtype):
        b.set_xs([x.to(dtype).to(DEV) for x in xs])
        return c(*b.get_all_cochain_params(max_dim=2, include_down_features=False))
    with torch.no_grad():
        monkeypatch.setattr(layers, 'FUSED_CHAIN_F32', frozenset())
        off = run(conv, batch, F32)
        assert spy.calls == 0
        monkeypatch.setattr(layers, 'FUSED_CHAIN_F32', frozenset({regime}))
        on = run(conv, batch, F32)
        assert spy.calls == 1
        ref = run(_double(conv), batch64, F64)
    for d in range(3):
        assert on[d].dtype == F32 and on[d].shape == off[d].shape
        gate(on[d], ref[d], f'SparseCINConv h{hidden} {nonlinearity}: route on vs float64, dim {d}')
        gate(off[d], ref[d], f'SparseCINConv h{hidden} {nonlinearity}: route off vs float64, dim {d}')
        gate(on[d], off[d], f'SparseCINConv h{hidden} {nonlinearity}: route on vs off, dim {d}')


@pytest.mark.parametrize('hidden,nonlinearity,regime', CONFIGS, ids=[f'h{h}-{a}' for h, a, _ in CONFIGS])
def test_model_route_on_matches_off_and_float64(monkeypatch, hidden, nonlinearity, regime):
    """A 2-layer SparseCIN: one call of the entry point per layer when the regime is on, none when it is off or when only the
    other regime is on."""
    from cwn_amd import layers
    model = _model(hidden, nonlinearity)
    spy = _Spy(monkeypatch)
    other = ({'relu_width', 'act'} - {regime}).pop()
    with torch.no_grad():
        monkeypatch.setattr(layers, 'FUSED_CHAIN_F32', frozenset())
        off = model(_batch())
        monkeypatch.setattr(layers, 'FUSED_CHAIN_F32', frozenset({other}))
        model(_batch())
        assert spy.calls == 0
        monkeypatch.setattr(layers, 'FUSED_CHAIN_F32', frozenset({regime}))
        on = model(_batch())
        assert spy.calls == 2
        monkeypatch.setattr(layers, 'FUSED_CHAIN_F32', True)
        assert torch.equal(model(_batch()), on) and spy.calls == 4
        ref = _double(model)(_batch(F64))
    gate(on, ref, f'SparseCIN h{hidden} {nonlinearity}: route on vs float64')
    gate(off, ref, f'SparseCIN h{hidden} {nonlinearity}: route off vs float64')
    gate(on, off, f'SparseCIN h{hidden} {nonlinearity}: route on vs off')


def test_route_declined(monkeypatch):
    """Never for CINppConv layers, under a recording autograd, for ReLU at 64 (cwn_update_mlp_f32's), for LayerNorm or a
    float64 model."""
    from cwn_amd import layers
    from cwn_amd.models import CINpp
    monkeypatch.setattr(layers, 'FUSED_CHAIN_F32', True)
    spy = _Spy(monkeypatch)
    torch.manual_seed(0)
    for nonlinearity in ('relu', 'elu'):
        pp = CINpp(num_input_features=1, num_classes=4, num_layers=2, hidden=48, dropout_rate=0.0, max_dim=2, use_coboundaries=True,
                   nonlinearity=nonlinearity, graph_norm='bn', readout='sum', final_readout='sum').to(DEV).eval()
        with torch.no_grad():
            pp(_batch())
    assert spy.calls == 0
    model = _model(48, 'elu')
    assert torch.is_grad_enabled() and all(p.requires_grad for p in model.parameters())
    out = model(_batch())
    assert out.requires_grad and spy.calls == 0
    with torch.no_grad():
        _model(64, 'relu')(_batch())
        _model(48, 'relu', norm='ln')(_batch())
        _model(16, 'elu', dtype=F64)(_batch(F64))
        assert spy.calls == 0
        _model(48, 'relu')(_batch())
        assert spy.calls == 2


# ------------------------------------------------------------------------------------------------
# 6. a static batch: the row counts live on the device
# ------------------------------------------------------------------------------------------------
def test_static_forward_replay_equals_the_eager_route(monkeypatch):
    """The hidden-48 EmbedSparseCIN through StaticForward over a StaticBatch in mode 'csr' (which serves that model with the
    route off as well): with the route on, the replay over batches of 20, 7 and 1 complexes equals the eager route-on
    forward on the collated batches bit for bit -- the launch reads every dimension's row count from the device."""
    import numpy as np
    from cwn_amd import csr, layers
    from cwn_amd.models import EmbedSparseCIN
    from cwn_amd.packed import PackedComplexes
    from cwn_amd.static_batch import StaticBatch
    from cwn_amd.static_graph import StaticForward
    from cwn_amd.synthetic import zinc_like_complexes
    monkeypatch.setattr(layers, 'FUSED_CHAIN_F32', frozenset({'relu_width'}))
    spy = _Spy(monkeypatch)
    pool = zinc_like_complexes(40, seed=5, max_ring=6)
    p = PackedComplexes(pool, DEV, max_dim=2, with_csr=True)
    torch.manual_seed(0)
    model = EmbedSparseCIN(28, 4, 1, 2, 48, dropout_rate=0.0, embed_edge=True, use_coboundaries=True).to(DEV).eval()
    perm = np.random.default_rng(1).permutation(40)
    epoch = [perm[:20], perm[20:27], perm[27:28]]
    sb = StaticBatch(p, 20, slots=1, mode='csr')
    sf = StaticForward(model, sb)
    assert sb.fits(epoch).all()
    sb.set_epoch(epoch)
    with torch.no_grad():
        for idx in epoch:
            out = sf.replay()[0][:len(idx)].clone()
            captured = spy.calls
            assert captured >= 2                                                  # two layers, inside the captured forward
            want = model(p.collate(idx))
            assert spy.calls == captured + 2
            assert torch.equal(out, want), (len(idx), float((out - want).abs().max()))
    torch.cuda.synchronize()
    csr.check_errors(DEV)
