"""The float32 update branches on the device: cwn_update_branches_f32 (csrc/cwn_branches_f32.hip) behind
ops.update_branches_f32 against float64 torch on the CPU, bit for bit against itself (a row alone, a second launch, another
slot, a device-side row count), through operand windows, with non-finite inputs, and under the CIN++ layers and models that
take it (layers.FUSED_BRANCHES_F32).

The bar is the project's own (tests/_product.gate): max|delta| <= 1e-5 * max(1, |ref|_inf), with the yardstick and operands
of tests/test_gpu_chain_f32.py: float64 torch on the CPU, inputs 2 randn, weights randn / sqrt(K), biases and shifts
0.3 randn, scales 1 + 0.3 randn.  Plain float32 torch stays within 0.19 of that bound on these operands over every width
below x 3 and 4 branches x the five activations (worst: tanh at 100 -> 128)."""
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
# scalar and vector weight loads, K not a multiple of 16, a combine K of 15 .. 512, the widest panel
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
    """The 2 nb + 1 stages of one dimension: float32 values held on the CPU (the float64 reference reads exactly them) and on
    the device.  bias / scale / shift: which of the per-stage vectors exist."""

    def __init__(self, F, H, nb, seed, bias=True, scale=True, shift=True):
        g = torch.Generator().manual_seed(seed)
        r = lambda *s: torch.randn(*s, generator=g)
        self.F, self.H, self.nb = F, H, nb
        n_st = 2 * nb + 1
        self.W = [r(H, K) / math.sqrt(K) for K in [F, H] * nb + [nb * H]]
        self.b = [0.3 * r(H) if bias else None for _ in range(n_st)]
        self.scale = [1 + 0.3 * r(H) if scale else None for _ in range(n_st)]
        self.shift = [0.3 * r(H) if shift else None for _ in range(n_st)]
        dev = lambda ts: [None if t is None else t.to(DEV) for t in ts]
        self.dW, self.db, self.dscale, self.dshift = dev(self.W), dev(self.b), dev(self.scale), dev(self.shift)

    def inputs(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        return [2 * torch.randn(n, self.F, generator=g) for _ in range(self.nb)]

    def dim(self, ins, act, out=None):
        from cwn_amd import ops
        return ops.BranchDim(ins=list(ins), weights=self.dW, biases=self.db, folds=list(zip(self.dscale, self.dshift)), act=act, out=out)

    def reference(self, ins, act):
        """float64 torch on the CPU."""
        def stage(x, s):
            z = x @ self.W[s].double().t()
            for t, op in ((self.b[s], torch.add), (self.scale[s], torch.mul), (self.shift[s], torch.add)):
                if t is not None:
                    z = op(z, t.double())
            return ACT_FN[act](z)
        hs = [stage(stage(x.double(), 2 * k), 2 * k + 1) for k, x in enumerate(ins)]
        return stage(torch.cat(hs, dim=-1), 2 * self.nb)


def _dev(ts):
    return [t.to(DEV) for t in ts]


VARIANTS = [dict(), dict(bias=False, scale=False, shift=False), dict(scale=False, shift=False), dict(bias=False),
            dict(shift=False), dict(scale=False)]


# ------------------------------------------------------------------------------------------------
# 1. the entry point against float64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,H', WIDTHS)
def test_update_branches_against_float64(F, H):
    """Every activation; launches of 1, 3 and 4 dimensions with rows from {0, 1, 31, 32, 33, 130} (a zero-row dimension among
    them), three and four branches mixed inside one launch, the dimensions with each of the six bias / scale / shift
    variants; outputs into sentinel-filled buffers with three spare rows: live rows within the gate, spare rows untouched."""
    from cwn_amd import ops
    launches = [(130,), (1, 0, 33), (31, 32, 0, 130), (0,)]
    nets = {nb: [_Net(F, H, nb, seed=100 * F + H + 10 * nb + v, **kw) for v, kw in enumerate(VARIANTS)] for nb in (3, 4)}
    k = 0
    for a, act in enumerate(ACTS):
        for rows in launches:
            dims, refs, bufs = [], [], []
            for d, n in enumerate(rows):
                net = nets[3 + (k + a) % 2][k % len(VARIANTS)]
                k += 1
                ins = net.inputs(n, seed=7 * n + d + a)
                refs.append(net.reference(ins, act))
                bufs.append(torch.full((n + 3, H), SENT, device=DEV))
                dims.append(net.dim(_dev(ins), act, out=bufs[-1]))
            assert ops.update_branches_f32_applies(dims)
            outs = ops.update_branches_f32(dims)
            for d, (n, y, ref, buf) in enumerate(zip(rows, outs, refs, bufs)):
                assert y.dtype == F32 and y.shape == (n, H) and (n == 0 or y.data_ptr() == buf.data_ptr()), (act, rows, d)
                assert bool((buf[n:] == SENT).all()), (act, rows, d)                        # spare rows untouched
                gate(buf[:n], ref, f'update_branches_f32 F {F} H {H} nb {len(dims[d].ins)} {act} rows {rows} dim {d}')
    assert k >= 2 * len(VARIANTS)            # every variant with three and with four branches


# ------------------------------------------------------------------------------------------------
# 2. operand windows
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nb', [3, 4])
def test_update_branches_allocates_its_outputs_and_takes_strided_operands(nb):
    """Row-strided inputs (column slices of wider buffers, one of them off 16 bytes, NaN beside the windows), `out` as a
    row-strided view of a wider buffer at column offsets 4 (16-byte stores) and 1 (scalar stores): equal bits to the
    contiguous launch, the other columns stay as they were."""
    from cwn_amd import ops
    for F, H in ((5, 48), (48, 48), (100, 128)):
        net, n = _Net(F, H, nb, seed=3), 70
        g = torch.Generator().manual_seed(4)
        pads = [(3, 6), (0, 4), (8, 0), (1, 2)][:nb]                              # columns before and behind each window
        wides = [2 * torch.randn(n, lo + F + hi, generator=g) for lo, hi in pads]
        for w, (lo, hi) in zip(wides, pads):
            w[:, :lo] = float('nan')
            w[:, lo + F:] = float('nan')                                          # (beside the windows: nothing of it reaches a result)
        ins = [w.to(DEV)[:, lo:lo + F] for w, (lo, hi) in zip(wides, pads)]
        assert [x.stride(0) for x in ins] == [lo + F + hi for lo, hi in pads] and ins[0].data_ptr() % 16 != 0
        cpu_ins = [w[:, lo:lo + F] for w, (lo, hi) in zip(wides, pads)]
        ref = net.reference(cpu_ins, 'elu')
        y, = ops.update_branches_f32([net.dim(ins, 'elu')])
        assert y.shape == (n, H) and y.is_contiguous()
        gate(y, ref, f'update_branches_f32 F {F} H {H} nb {nb}: strided inputs, own output')
        packed, = ops.update_branches_f32([net.dim([x.contiguous() for x in ins], 'elu')])
        assert torch.equal(packed, y)                                             # a window or the matrix itself: the same bits
        for off in (4, 1):
            wide_out = torch.full((n + 2, H + 8), SENT, device=DEV)
            view = wide_out[:, off:off + H]
            z, = ops.update_branches_f32([net.dim(ins, 'elu', out=view)])
            assert z.data_ptr() == view.data_ptr() and z.stride(0) == H + 8
            assert torch.equal(z, y)
            keep = torch.ones_like(wide_out, dtype=torch.bool)
            keep[:n, off:off + H] = False
            assert bool((wide_out[keep] == SENT).all())


# ------------------------------------------------------------------------------------------------
# 3. row independence and reproducibility, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,H,act,nb', [(48, 48, 'relu', 3), (100, 128, 'tanh', 4)])
def test_a_row_has_the_same_bits_alone_and_in_any_batch(F, H, act, nb):
    from cwn_amd import ops
    net, n = _Net(F, H, nb, seed=11), 130
    ins = _dev(net.inputs(n, seed=12))
    batch, = ops.update_branches_f32([net.dim(ins, act)])
    again, = ops.update_branches_f32([net.dim(ins, act)])
    assert torch.equal(batch, again)                                              # two launches on the same operands
    alone = torch.cat([ops.update_branches_f32([net.dim([x[r:r + 1] for x in ins], act)])[0] for r in range(n)])
    assert torch.equal(batch, alone)
    other = _Net(5, 16, 7 - nb, seed=13)                                          # (the other branch count beside it)
    o_ins = _dev(other.inputs(37, seed=14))
    _, _, third = ops.update_branches_f32([other.dim(o_ins, 'elu'), other.dim([x[:0] for x in o_ins], 'elu'), net.dim(ins, act)])
    assert torch.equal(batch, third)                                              # ... in another slot of a wider launch
    gate(batch, net.reference([x.cpu() for x in ins], act), f'update_branches_f32 F {F} H {H} nb {nb} {act}, 130 rows')


# ------------------------------------------------------------------------------------------------
# 4. the device-side row count
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,H,nb', [(48, 48, 3), (100, 128, 4)])
def test_device_side_row_count(F, H, nb):
    """include/cwn_hip.h, "DEVICE-SIDE ROW COUNTS": capacity-sized operands whose rows at or beyond the count hold NaN, the
    count in a device int64.  Live rows are within the gate and bit-identical to the same call with n = live and no
    m_dev; rows at or beyond the count keep the sentinel; a count of 0 writes nothing; a count beyond the capacity
    behaves as the capacity."""
    from cwn_amd import _ffi, ops
    net = _Net(F, H, nb, seed=21)
    ins = net.inputs(CAP, seed=22)
    ref = net.reference(ins, 'elu')
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    for live in LIVES + (CAP + 50,):
        rows = min(live, CAP)
        xs = [x.clone() for x in ins]
        for x in xs:
            x[rows:] = float('nan')
        xs = _dev(xs)
        out = torch.full((CAP + 4, H), SENT, device=DEV)
        count.fill_(live)
        with _ffi.dynamic_rows({CAP: count.data_ptr()}):
            y, = ops.update_branches_f32([net.dim(xs, 'elu', out=out)])
        assert y.shape == (CAP, H)
        assert bool((out[rows:] == SENT).all()), f'a row at or beyond the live count {live} was written'
        static, = ops.update_branches_f32([net.dim([x[:rows] for x in xs], 'elu')])
        assert torch.equal(out[:rows], static), live
        gate(out[:rows], ref[:rows], f'update_branches_f32 F {F} H {H} nb {nb}, {live} live rows of {CAP}')
    # a capacity that is not a key of the mapping: a host count, as without the context
    count.fill_(3)
    with _ffi.dynamic_rows({CAP + 1: count.data_ptr()}):
        y, = ops.update_branches_f32([net.dim(_dev(ins), 'elu')])
    gate(y, ref, 'update_branches_f32 under a mapping without its capacity')


# ------------------------------------------------------------------------------------------------
# 5. non-finite inputs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', ['relu', 'tanh'])
@pytest.mark.parametrize('F,H,nb', [(12, 12, 3), (48, 48, 4)])
def test_non_finite_inputs_come_out_where_float64_torch_puts_them(F, H, nb, act):
    """A NaN, a +Inf and a -Inf in single input rows of different branches (the +Inf in the last branch, the -Inf in the
    third row tile, the +Inf in the second): non-finite outputs exactly where float64 torch has them, every other row finite
    and within the gate."""
    from cwn_amd import ops
    net, n = _Net(F, H, nb, seed=31), 70
    ins = net.inputs(n, seed=32)
    ins[0][3, F // 2], ins[nb - 1][40, 0], ins[1][66, F - 1] = float('nan'), float('inf'), float('-inf')
    ref = net.reference(ins, act)
    y, = ops.update_branches_f32([net.dim(_dev(ins), act)])
    gate_nonfinite(y, ref, f'update_branches_f32 F {F} H {H} nb {nb} {act}: NaN / +Inf / -Inf input rows')
    clean = [r for r in range(n) if r not in (3, 40, 66)]
    assert bool(torch.isfinite(y[clean]).all()) and bool(torch.isnan(y[3]).all())


# ------------------------------------------------------------------------------------------------
# 6. layers and models
# ------------------------------------------------------------------------------------------------
class _Spy:
    """Counts the calls of the C entry points (the new one, and cwn_update_mlp3_f32 / cwn_update_chain_f32 beside it) and
    passes them on."""

    def __init__(self, monkeypatch):
        from cwn_amd import _ffi
        self.calls = self.mlp3 = self.chain = 0
        L = _ffi.lib()

        def spy(arr, n, s, fn=L.cwn_update_branches_f32):
            self.calls += 1
            assert 1 <= n <= 4
            return fn(arr, n, s)

        def mlp3(*a, fn=L.cwn_update_mlp3_f32):
            self.mlp3 += 1
            return fn(*a)

        def chain(*a, fn=L.cwn_update_chain_f32):
            self.chain += 1
            return fn(*a)
        monkeypatch.setattr(L, 'cwn_update_branches_f32', spy)
        monkeypatch.setattr(L, 'cwn_update_mlp3_f32', mlp3)
        monkeypatch.setattr(L, 'cwn_update_chain_f32', chain)


def _stats(module, dtype=F32, seed=1):
    """Non-trivial running statistics and affine for every BatchNorm."""
    g = torch.Generator().manual_seed(seed)
    for mod in module.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            with torch.no_grad():
                mod.running_mean.copy_(torch.randn(mod.num_features, generator=g).to(dtype) * 0.1)
                mod.running_var.copy_((torch.rand(mod.num_features, generator=g) + 0.5).to(dtype))
                mod.weight.copy_((torch.rand(mod.num_features, generator=g) + 0.5).to(dtype))
                mod.bias.copy_(torch.randn(mod.num_features, generator=g).to(dtype) * 0.1)
    return module


def _model(hidden, nonlinearity, layers_=2, norm='bn', dtype=F32, cls=None):
    from cwn_amd.models import CINpp, SparseCIN
    torch.manual_seed(0)
    m = (cls or CINpp)(num_input_features=1, num_classes=16, num_layers=layers_, hidden=hidden, dropout_rate=0.0, max_dim=2,
                       use_coboundaries=True, nonlinearity=nonlinearity, graph_norm=norm, readout='sum', final_readout='sum',
                       readout_dims=(0, 1, 2)).to(dtype)
    return _stats(m, dtype).to(DEV).eval()


def _batch(dtype=F32):
    from tests.test_gpu_f64_dense import _sr_batch
    return _sr_batch(dtype=dtype).to(DEV)


def _double(module):
    return copy.deepcopy(module).double()


CONFIGS = [(48, 'relu', 'relu_width'), (16, 'elu', 'act')]


@pytest.mark.parametrize('hidden,nonlinearity,regime', CONFIGS, ids=[f'h{h}-{a}' for h, a, _ in CONFIGS])
def test_model_route_on_matches_off_and_float64(monkeypatch, hidden, nonlinearity, regime):
    """A 2-layer CINpp (eval-mode BatchNorm with non-trivial statistics; the first layer reads the raw feature, F = 1): one
    call of the entry point per layer when the regime is on, none when it is off or when only the other regime is on."""
    from cwn_amd import layers
    model = _model(hidden, nonlinearity)
    spy = _Spy(monkeypatch)
    other = ({'relu_width', 'act'} - {regime}).pop()
    with torch.no_grad():
        monkeypatch.setattr(layers, 'FUSED_BRANCHES_F32', frozenset())
        off = model(_batch())
        monkeypatch.setattr(layers, 'FUSED_BRANCHES_F32', frozenset({other}))
        model(_batch())
        assert spy.calls == 0
        monkeypatch.setattr(layers, 'FUSED_BRANCHES_F32', frozenset({regime}))
        on = model(_batch())
        assert spy.calls == 2
        monkeypatch.setattr(layers, 'FUSED_BRANCHES_F32', True)
        assert torch.equal(model(_batch()), on) and spy.calls == 4
        ref = _double(model)(_batch(F64))
    assert spy.mlp3 == spy.chain == 0
    gate(on, ref, f'CINpp h{hidden} {nonlinearity}: route on vs float64')
    gate(off, ref, f'CINpp h{hidden} {nonlinearity}: route off vs float64')
    gate(on, off, f'CINpp h{hidden} {nonlinearity}: route on vs off')


def test_four_stream_layer_route_on_matches_off_and_float64(monkeypatch):
    """One CINppConv(coboundary_stream=True) at 64 with ReLU and eval-mode BatchNorm with non-trivial statistics, over random
    features: four branches are not cwn_update_mlp3_f32's at any width.  The route on against the route off and each against
    the same layer in float64; the entry point is called once when on, never when off or with only 'act' on."""
    from cwn_amd import layers
    from cwn_amd.layers import CINppConv
    F = 64
    torch.manual_seed(0)
    conv = _stats(CINppConv(F, F, F, None, None, None, None, None, None, max_dim=2, hidden=F, act_module=torch.nn.ReLU, layer_dim=F,
                            use_coboundaries=True, coboundary_stream=True)).to(DEV).eval()
    assert conv.mp_levels[1].combine_nn[0].in_features == 4 * F
    batch, batch64 = _batch(), _batch(F64)
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(batch.cochains[d].num_cells, F, generator=g) for d in range(3)]
    spy = _Spy(monkeypatch)

    def run(c, b, dtype):
        b.set_xs([x.to(dtype).to(DEV) for x in xs])
        return c(*b.get_all_cochain_params(max_dim=2, include_down_features=False))
    with torch.no_grad():
        monkeypatch.setattr(layers, 'FUSED_BRANCHES_F32', frozenset())
        off = run(conv, batch, F32)
        monkeypatch.setattr(layers, 'FUSED_BRANCHES_F32', frozenset({'act'}))
        run(conv, batch, F32)
        assert spy.calls == 0
        monkeypatch.setattr(layers, 'FUSED_BRANCHES_F32', frozenset({'relu_width'}))
        on = run(conv, batch, F32)
        assert spy.calls == 1 and spy.mlp3 == 0
        ref = run(_double(conv), batch64, F64)
    for d in range(3):
        assert on[d].dtype == F32 and on[d].shape == off[d].shape
        gate(on[d], ref[d], f'CINppConv 4 streams h64 relu: route on vs float64, dim {d}')
        gate(off[d], ref[d], f'CINppConv 4 streams h64 relu: route off vs float64, dim {d}')
        gate(on[d], off[d], f'CINppConv 4 streams h64 relu: route on vs off, dim {d}')


def test_route_declined(monkeypatch):
    """ReLU at 64 with three branches stays with cwn_update_mlp3_f32; never under a recording autograd, for LayerNorm, a
    float64 model or a SparseCIN."""
    from cwn_amd import layers
    from cwn_amd.models import SparseCIN
    monkeypatch.setattr(layers, 'FUSED_BRANCHES_F32', True)
    spy = _Spy(monkeypatch)
    from cwn_amd.models import CINpp
    torch.manual_seed(0)
    wide = CINpp(num_input_features=64, num_classes=4, num_layers=2, hidden=64, dropout_rate=0.0, max_dim=2, use_coboundaries=True,
                 nonlinearity='relu', graph_norm='bn', readout='sum', final_readout='sum').to(DEV).eval()
    b = _batch()
    g = torch.Generator().manual_seed(2)
    b.set_xs([torch.randn(b.cochains[d].num_cells, 64, generator=g).to(DEV) for d in range(3)])
    with torch.no_grad():
        wide(b)
    assert spy.calls == 0 and spy.mlp3 == 2                                       # (F, F) first layers at 64: both layers
    model = _model(48, 'elu')
    assert torch.is_grad_enabled() and all(p.requires_grad for p in model.parameters())
    out = model(_batch())
    assert out.requires_grad and spy.calls == 0
    with torch.no_grad():
        _model(48, 'relu', norm='ln')(_batch())
        _model(16, 'elu', dtype=F64)(_batch(F64))
        _model(48, 'relu', cls=SparseCIN)(_batch())
        _model(16, 'elu', cls=SparseCIN)(_batch())
        assert spy.calls == 0
        _model(48, 'relu')(_batch())
        assert spy.calls == 2


# ------------------------------------------------------------------------------------------------
# 7. the reference's own EmbedCINpp with ELU
# ------------------------------------------------------------------------------------------------
def test_reference_fixture_cinpp_elu(monkeypatch):
    """Case `cinpp_elu` of tests/golden/cell_options.npz (tests/_options.py): the reference's float64 prediction and every
    stored partial, in float32 with the 'act' regime on, within the float32 tolerance of tests/test_gpu_options_golden.py; the
    entry point is called once per layer."""
    from cwn_amd import csr, layers
    from tests import _options as X
    from tests.test_gpu_options_golden import TOL
    case = 'cinpp_elu'
    monkeypatch.setattr(layers, 'FUSED_BRANCHES_F32', frozenset({'act'}))
    spy = _Spy(monkeypatch)
    c = X.cfg(X.CELL, case)
    model = X.product_model(X.CELL, case, F32).to(DEV)
    n_layers = len(model.convs)
    with torch.no_grad():
        y, res = model(X.product_batch(X.CELL, c['inputs'], F32).to(DEV), include_partial=True)
    assert spy.calls == n_layers >= 1 and spy.mlp3 == spy.chain == 0
    ref = X.partials(X.CELL, case)
    assert y.dtype == F32 and ref and set(ref) <= set(res), set(ref) - set(res)
    for k, v in ref.items():
        gate(res[k], v, f'{case} branches on {k}', tol=TOL[F32])
    gate(y, X.out64(X.CELL, case), f'{case} branches on out', tol=TOL[F32])
    csr.check_errors(DEV)


# ------------------------------------------------------------------------------------------------
# 8. a static batch: the row counts live on the device
# ------------------------------------------------------------------------------------------------
def test_static_forward_replay_equals_the_eager_route(monkeypatch):
    """The hidden-48 EmbedCINpp through StaticForward over a StaticBatch in mode 'csr': with the route on, the replay over
    batches of 20, 7 and 1 complexes equals the eager route-on forward on the collated batches bit for bit -- the launch
    reads every dimension's row count from the device."""
    import numpy as np
    from cwn_amd import csr, layers
    from cwn_amd.models import EmbedCINpp
    from cwn_amd.packed import PackedComplexes
    from cwn_amd.static_batch import StaticBatch
    from cwn_amd.static_graph import StaticForward
    from cwn_amd.synthetic import zinc_like_complexes
    monkeypatch.setattr(layers, 'FUSED_BRANCHES_F32', frozenset({'relu_width'}))
    spy = _Spy(monkeypatch)
    pool = zinc_like_complexes(40, seed=5, max_ring=6)
    p = PackedComplexes(pool, DEV, max_dim=2, with_csr=True)
    torch.manual_seed(0)
    model = EmbedCINpp(28, 4, 1, 2, 48, dropout_rate=0.0, embed_edge=True, use_coboundaries=True).to(DEV).eval()
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
