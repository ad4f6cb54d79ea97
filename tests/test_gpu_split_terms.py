"""Every term and every plane of the bf16 three-way split (csrc/cwn_split.h), at every site that writes the split out.

The inputs are tests/_split_probe.py's: integer operands of three classes (A: three-piece X, one-piece W; B: the mirror
image; C: two pieces each) for which every kept piece product is exercised, every dropped one is exactly zero and every partial
sum is an integer below 2^24 -- so each kernel must return the integer product under torch.equal, whatever its accumulation
order, and once more with a power of two on every row / column (the exponents of all three planes).  A lost term, a plane
under another contraction index, a packed chunk at the wrong plane offset give other integers; tests/test_split_probe_host.py
proves that on the CPU model.  Each test first asserts that the split path served the launch.

Sites: cwn_gemm_f32 (split form: fp32 and packed weight, MULTI), cwn_gemm_tn_f32 (split form: atomic and ordered),
cwn_dense_stage_f32 / _ex_f32 / _bwd_f32, cwn_update_mlp_f32 (both schedules), cwn_update_mlp3_f32, the blocked layer forward
(16-wave, two-per-CU, big item) and its two backwards."""
import copy

import pytest
import torch

from tests import _split_probe as P
from tests.test_gpu_blocked import _batch, _conv, _oracle_scope, _propagate_reference_backward, _run, cpu

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = [('A', False), ('B', False), ('C', False), ('A', True)]         # (class, power-of-two scales)
IDS = ['A', 'B', 'C', 'A-scaled']


def _same(got, ref, what):
    """torch.equal against the exact reference; the share of wrong elements is printed first."""
    g = cpu(got).double()
    ref = ref.double()
    assert g.shape == ref.shape, (what, g.shape, ref.shape)
    bad = int((g != ref).sum())
    print(f'[split terms] {what}: {bad} of {ref.numel()} elements differ from the exact answer')
    assert torch.equal(g, ref), what


# ------------------------------------------------------------------------------------------------
# cwn_gemm_f32, split form
# ------------------------------------------------------------------------------------------------
def _gemm_both(make):
    """The launch on the split kernel (asserted) and on the exact fp32-MFMA kernel."""
    from cwn_amd import ops
    prev = ops.set_gemm_exact(False)
    try:
        assert ops.gemm_uses_split(make(), DEV), 'the launch would not run on the split kernel'
        with torch.no_grad():
            split = ops.run_gemm(make(), DEV)
            ops.set_gemm_exact(True)
            assert not ops.gemm_uses_split(make(), DEV)
            exact = ops.run_gemm(make(), DEV)
    finally:
        ops.set_gemm_exact(prev)
    return split, exact


@pytest.mark.parametrize('cls,scaled', CASES, ids=IDS)
def test_gemm_split_terms(cls, scaled):
    """N = K = 128, M = 256 (four 64-row tiles, every row position): fp32 weight (in-kernel split8 of W) and packed weight
    (pack_gemm_weights_kernel), plain and with an integer bias + ReLU."""
    from cwn_amd import ops
    p = P.make_case(cls, 256, 128, 128, seed=1, scaled=scaled)
    X, W = p.X.to(DEV), torch.nn.Parameter(p.W.to(DEV))
    bias = P.draw('one', (128,), torch.Generator().manual_seed(11))
    assert p.top + 3 < P.EXACT_LIMIT
    variants = [(None, False)] if scaled else [(None, False), (bias, True)]       # (a bias has one scale per column only)
    for packed in (False, True):
        for bi, relu in variants:
            ref = p.ref if bi is None else torch.relu(p.ref + bi.double())
            make = lambda: [ops.Gemm(X=X, W=W, bias=None if bi is None else bi.float().to(DEV), relu=relu,
                                     w_packed=ops.pack_gemm_weight(W) if packed else None)]
            if packed:
                assert ops.pack_gemm_weight(W) is not None
            split, exact = _gemm_both(make)
            _same(split[0], ref, f'gemm class {cls} scaled={scaled} packed={packed} bias={bi is not None}')
            _same(exact[0], ref, f'exact kernel, class {cls} scaled={scaled}')
            assert torch.equal(split[0], exact[0])


@pytest.mark.parametrize('cls', ['A', 'B', 'C'])
def test_gemm_split_terms_multi(cls):
    """Three descriptors of 172 row tiles each: more tiles (516) than resident workgroups, the MULTI form.  The first and
    the last 256 rows of each carry the probe, the rows between are zero."""
    from cwn_amd import ops
    M = 11008
    ps = [P.make_case(cls, 512, 128, 128, seed=20 + i) for i in range(3)]
    Xs, refs = [], []
    for p in ps:
        X, ref = torch.zeros(M, 128), torch.zeros(M, 128, dtype=torch.float64)
        X[:256], X[-256:] = p.X[:256], p.X[256:]
        ref[:256], ref[-256:] = p.ref[:256], p.ref[256:]
        Xs.append(X.to(DEV))
        refs.append(ref)
    Ws = [torch.nn.Parameter(p.W.to(DEV)) for p in ps]
    bias = P.draw('one', (128,), torch.Generator().manual_seed(12))
    refs[0] = torch.relu(refs[0] + bias.double())
    for packed in (False, True):
        make = lambda: [ops.Gemm(X=Xs[i], W=Ws[i], bias=bias.float().to(DEV) if i == 0 else None, relu=i == 0,
                                 w_packed=ops.pack_gemm_weight(Ws[i]) if packed else None) for i in range(3)]
        split, exact = _gemm_both(make)
        for i in range(3):
            _same(split[i], refs[i], f'MULTI gemm class {cls} packed={packed} descriptor {i}')
            assert torch.equal(split[i], exact[i])


# ------------------------------------------------------------------------------------------------
# cwn_gemm_tn_f32, split form
# ------------------------------------------------------------------------------------------------
def _tn(p, K, K2, in_relu, ordered):
    from cwn_amd import _ffi
    M, N = p.dZ.shape
    dZ, X = p.dZ.to(DEV), p.X[:, :K].contiguous().to(DEV)
    X2 = p.X[:, K:].contiguous().to(DEV) if K2 else None
    sc, sh = (torch.ones(K, device=DEV), torch.zeros(K, device=DEV)) if in_relu else (None, None)
    dW, db = torch.zeros(N, K + K2, device=DEV), torch.zeros(N, device=DEV)
    desc = _ffi.GemmTnDesc(dZ=dZ.data_ptr(), X=X.data_ptr(), X2=_ffi.ptr(X2), in_scale=_ffi.ptr(sc), in_shift=_ffi.ptr(sh),
                           in_scale2=None, in_shift2=None, dW=dW.data_ptr(), db=db.data_ptr(), M=M, lddz=N, ldx=K, ldx2=K2,
                           lddw=K + K2, N=N, K=K, K2=K2, in_relu=in_relu)
    assert _ffi.gemm_tn_would_split([desc]), 'the launch would not run on the split kernel'
    prev = _ffi.DETERMINISTIC_TN
    _ffi.DETERMINISTIC_TN = ordered
    try:
        _ffi.gemm_tn([desc], DEV)
    finally:
        _ffi.DETERMINISTIC_TN = prev
    torch.cuda.synchronize()
    return dW, db


@pytest.mark.parametrize('K2', [0, 128])
@pytest.mark.parametrize('cls,scaled', CASES, ids=IDS)
def test_gemm_tn_split_terms(cls, scaled, K2):
    """dW = dZ^T [X | X2] over M = 1024 rows, N = K = 128: dZ has one non-zero per row, eight per column in different 32-row
    chunks and ring slots; the atomic and the ordered (workspace) form, without and with the ReLU + scale 1 / shift 0
    prologue on X; db = the column sums of dZ."""
    p = P.make_tn_case(cls, 1024, 128, 128 + K2, seed=3, scaled=scaled)
    for ordered in (False, True):
        for in_relu in (0, 1):
            dW, db = _tn(p, 128, K2, in_relu, ordered)
            what = f'gemm_tn class {cls} scaled={scaled} K2={K2} ordered={ordered} in_relu={in_relu}'
            _same(dW, p.ref(relu_cols=128 if in_relu else 0), what)
            _same(db, p.ref_db(), what + ' db')


@pytest.mark.parametrize('cls', ['A', 'B', 'C'])
def test_gemm_tn_split_terms_over_several_bands(cls):
    """M = 5000 (beyond the longest band, and no multiple of a chunk): the 1024 live rows scattered over the bands."""
    M = 5000
    live = torch.randperm(M, generator=torch.Generator().manual_seed(5))[:1024].sort().values
    p = P.make_tn_case(cls, M, 128, 128, live=live, seed=4)
    for ordered in (False, True):
        dW, db = _tn(p, 128, 0, 0, ordered)
        _same(dW, p.ref(), f'gemm_tn over bands, class {cls} ordered={ordered}')
        _same(db, p.ref_db(), f'gemm_tn over bands, class {cls} ordered={ordered} db')


# ------------------------------------------------------------------------------------------------
# the stage kernels (cwn_tile.h + cwn_stage.hip)
# ------------------------------------------------------------------------------------------------
def _stage_rows(F):
    """2048 / F + 1 rows (one workgroup and one row), and more workgroups than the chip has CUs plus a partial one."""
    return (2048 // F + 1, 256 * (4096 // F) + 37)


@pytest.mark.parametrize('F', [64, 128])
@pytest.mark.parametrize('cls,scaled', CASES, ids=IDS)
def test_stage_forward_split_terms(cls, scaled, F):
    """cwn_dense_stage_f32 (F -> F, 2F -> F) and cwn_dense_stage_ex_f32 (3F, 4F -> F) on weights packed by
    pack_stage_weights_many, both row counts in one launch; prologues off, and scale 1 / shift 0 / ReLU on every block."""
    from cwn_amd import ops
    bias = P.draw('one', (F,), torch.Generator().manual_seed(13))
    for blocks in (1, 2, 3, 4):
        ps = [P.make_case(cls, M, F, blocks * F, seed=30 + blocks + 10 * k, scaled=scaled) for k, M in enumerate(_stage_rows(F))]
        Ws = [torch.nn.Parameter(p.W.to(DEV)) for p in ps]
        ops.pack_stage_weights_many(Ws)
        one, zero = torch.ones(F, device=DEV), torch.zeros(F, device=DEV)
        for pro in (False, True):
            gemms, refs = [], []
            for k, (p, W) in enumerate(zip(ps, Ws)):
                Xb = [p.X[:, j * F:(j + 1) * F].contiguous().to(DEV) for j in range(blocks)]
                with_bias = k == 1 and not scaled
                gemms.append(ops.Gemm(X=Xb[0], X2=Xb[1] if blocks > 1 else None, W=W,
                                      bias=bias.float().to(DEV) if with_bias else None,
                                      in_scale=one if pro else None, in_shift=zero if pro else None,
                                      in_scale2=one if pro and blocks > 1 else None, in_shift2=zero if pro and blocks > 1 else None,
                                      in_relu=(3 if blocks > 1 else 1) if pro else 0,
                                      more=tuple((x, pro, None) for x in Xb[2:])))
                ref = p.scaled_like_ref((p.Xi.clamp(min=0) if pro else p.Xi) @ p.Wi.t())
                refs.append(ref + bias.double() if with_bias else ref)
                assert p.top + 3 < P.EXACT_LIMIT
            got = ops.run_stage(gemms, DEV)
            assert got is not None, 'the stage kernel refused a launch it is written for'
            for k, ref in enumerate(refs):
                _same(got[k], ref, f'stage F={F} blocks={blocks} prologue={pro} class {cls} scaled={scaled} rows={ref.size(0)}')


@pytest.mark.parametrize('F', [64, 128])
@pytest.mark.parametrize('cls,scaled', CASES, ids=IDS)
def test_stage_backward_split_terms(cls, scaled, F):
    """cwn_dense_stage_bwd_f32 without a norm and z > 0 everywhere: dz = dy bit for bit, dX = dz W on the transposed packed
    blocks, for a Linear(F -> F) and the two halves of a Linear(2F -> F)."""
    from cwn_amd import ops, _ffi
    for wide in (False, True):
        n_in = 2 * F if wide else F
        ps = [P.make_case(cls, M, n_in, F, seed=50 + wide + 10 * k, scaled=scaled) for k, M in enumerate(_stage_rows(F))]
        Ws = [torch.nn.Parameter(p.W.t().contiguous().to(DEV)) for p in ps]          # Linear layout [F, n_in]; dX = dz W
        ops.pack_stage_weights_many(Ws)
        entries, keep = [], []
        for p, W in zip(ps, Ws):
            M = p.X.size(0)
            dy, z = p.X.to(DEV), torch.ones(M, F, device=DEV)
            dz = torch.full((M, F), float('nan'), device=DEV)
            out = torch.full((M, n_in), float('nan'), device=DEV)
            b = _ffi.GemmBnb(z=z.data_ptr(), dz=dz.data_ptr(), ldz=F, lddz=F, relu=1)
            entries.append((dy, b, W, out[:, :F], out[:, F:] if wide else None))
            keep.append((dy, z, dz, out))
        assert ops.run_stage_bwd(entries, DEV), 'the backward stage kernel refused a launch it is written for'
        for p, (dy, z, dz, out) in zip(ps, keep):
            what = f'stage backward F={F} wide={wide} class {cls} scaled={scaled} rows={dy.size(0)}'
            assert torch.equal(dz, dy), what
            _same(out, p.ref, what)


# ------------------------------------------------------------------------------------------------
# cwn_update_mlp_f32 and cwn_update_mlp3_f32: the probe in one Linear, the identity in all others
# ------------------------------------------------------------------------------------------------
def _linears(seq):
    return [m for m in seq if isinstance(m, torch.nn.Linear)]


def _mlp_terms(conv, nets, F, cls, scaled, rows, run, what):
    """Every Linear of the chain takes its turn (dimension d is one Linear ahead of dimension d - 1).  The other Linears are
    the identity -- which splits to (1, 0, 0), so they hand the probed product on bit for bit -- and the combine selects the
    probed branch ([.. I ..] among zero blocks) unless it is the probed Linear itself; biases are zero.  What enters a second
    stage or the combine has been through a ReLU: the reference takes it too."""
    nb = len(nets)
    n_lin = 2 * nb + 1
    eye = torch.eye(F)
    for t in range(n_lin):
        outs, refs = [], []
        with torch.no_grad():
            for d, M in enumerate(rows):
                lvl = conv.mp_levels[d]
                lins = [lin for name in nets for lin in _linears(getattr(lvl, name))]
                cb, = _linears(lvl.combine_nn)
                assert len(lins) == 2 * nb and tuple(cb.weight.shape) == (F, nb * F)
                for lin in lins + [cb]:
                    lin.bias.zero_()
                for lin in lins:
                    lin.weight.copy_(eye)
                k = (t + d) % n_lin
                if k < 2 * nb:
                    br, stage = divmod(k, 2)
                    p = P.make_case(cls, M, F, F, seed=70 + 7 * t + d, scaled=scaled, p_neg=0.25)
                    lins[k].weight.copy_(p.W)
                    sel = torch.zeros(F, nb * F)
                    sel[:, br * F:(br + 1) * F] = eye
                    cb.weight.copy_(sel)
                    outs += [p.X.to(DEV) for _ in range(nb)]
                    pre = p.Xi if stage == 0 else p.Xi.clamp(min=0)
                else:
                    p = P.make_case(cls, M, F, nb * F, seed=70 + 7 * t + d, scaled=scaled, p_neg=0.25)
                    cb.weight.copy_(p.W)
                    outs += [p.X[:, j * F:(j + 1) * F].contiguous().to(DEV) for j in range(nb)]
                    pre = p.Xi.clamp(min=0)
                ref = (pre @ p.Wi.t()).clamp(min=0)
                assert int((ref > 0).sum()) * 2 >= ref.numel(), 'fewer than half of the outputs survive the ReLU'
                refs.append(p.scaled_like_ref(ref))
        got = run(outs)
        assert got is not None
        for d in range(len(rows)):
            _same(got[d], refs[d], f'{what} F={F} class {cls} scaled={scaled} turn {t} dim {d} (Linear {(t + d) % n_lin}, {rows[d]} rows)')


def _mlp_rows(F, schedule):
    """'alternating': one round of workgroups (4096 / F rows each); 'sequential': more workgroups than the chip has CUs."""
    TM = 4096 // F
    return (TM + 1, 2 * TM + 3, 5) if schedule == 'alternating' else (90 * TM + 1,) * 3


@pytest.mark.parametrize('schedule', ['alternating', 'sequential'])
@pytest.mark.parametrize('F', [64, 128])
@pytest.mark.parametrize('cls,scaled', CASES, ids=IDS)
def test_update_mlp_split_terms(cls, scaled, F, schedule):
    """cwn_update_mlp_f32 through SparseCINConv._dense_eval: both schedules (at F = 64 the three-buffer one is the swizzled
    layout), every one of the five Linears."""
    from cwn_amd import layers
    from cwn_amd.layers import SparseCINConv
    torch.manual_seed(0)
    conv = SparseCINConv(F, F, F, None, None, None, None, max_dim=2, hidden=F, act_module=torch.nn.ReLU, layer_dim=F,
                         use_coboundaries=True, graph_norm=torch.nn.Identity).eval().to(DEV)

    def run(outs):
        with torch.no_grad():
            got = conv._dense_eval(['blocked'] * 3, outs)
        assert conv in layers._MLP_CACHE, 'cwn_update_mlp_f32 did not serve the launch'
        return got

    assert layers.FUSED_UPDATE_MLP
    _mlp_terms(conv, ['update_up_nn', 'update_boundaries_nn'], F, cls, scaled, _mlp_rows(F, schedule), run, f'update_mlp ({schedule})')
    layers._MLP_CACHE.pop(conv, None)


@pytest.mark.parametrize('F', [64, 128])
@pytest.mark.parametrize('cls,scaled', CASES, ids=IDS)
def test_update_mlp3_split_terms(cls, scaled, F):
    """cwn_update_mlp3_f32 through CINppConv._dense_eval: every one of the seven Linears."""
    from cwn_amd import ops
    from cwn_amd.layers import CINppConv
    torch.manual_seed(0)
    conv = CINppConv(F, F, F, None, None, None, None, None, None, max_dim=2, hidden=F, act_module=torch.nn.ReLU, layer_dim=F,
                     use_coboundaries=True, graph_norm=torch.nn.Identity).eval().to(DEV)
    calls, orig = [], ops.update_mlp3

    def run(outs):
        ops.update_mlp3 = lambda dims: (calls.append(len(dims)), orig(dims))[1]
        try:
            with torch.no_grad():
                return conv._dense_eval(['blocked'] * 3, outs, 0)
        finally:
            ops.update_mlp3 = orig

    TM = 4096 // F
    _mlp_terms(conv, ['update_up_nn', 'update_down_nn', 'update_boundaries_nn'], F, cls, scaled, (TM + 1, 2 * TM + 3, 5), run,
               'update_mlp3')
    assert calls == [3] * 7, 'cwn_update_mlp3_f32 did not serve every launch'


# ------------------------------------------------------------------------------------------------
# the blocked layer: forward
# ------------------------------------------------------------------------------------------------
def _abs_conv(conv, big_bias=False):
    """A float64 twin whose message weights are |hi| + |mid| + |lo| of the original's (and |bias|): run on the same sums of the
    features / gradients, the references give the sum of the absolute terms of everything they compute."""
    twin = copy.deepcopy(conv).double().cpu()
    with torch.no_grad():
        for d, lvl in enumerate(twin.mp_levels):
            lin, src = lvl.msg_up_nn[1], conv.mp_levels[d].msg_up_nn[1]
            lin.weight.copy_(P.pieces_abs(cpu(src.weight)))
            lin.bias.copy_(cpu(src.bias).double().abs())
            if big_bias:
                lin.bias.fill_(1e30)            # (every message positive: the backward's ReLU mask is all ones)
    return twin


def _no_dropped_terms(x, w, what):
    """One factor of each dropped product (wm*xl, wl*xm, wl*xl) is zero throughout."""
    (_, xm, xl), (_, wm, wl) = P.split(x), P.split(w)
    assert not (bool(wm.any()) and bool(xl.any())) and not (bool(wl.any()) and bool(xm.any())) \
        and not (bool(wl.any()) and bool(xl.any())), what


def _layer_case(b, conv, F, cls, scaled, seed):
    """Features and message weights of class `cls` into the batch and the layer; returns the exact outputs (float64).
    At most 2 non-zero features per row -- 1 on edges and rings: an edge of two fused hexagons sums ten messages -- and values
    below 768 in class C.  Asserted from the reference: the absolute terms of every
    reduced output (which bound Y1, Y2, their sum and every partial reduce) sum to < 2^24.
    The scaled form multiplies features and bias by 2^-20 (one scale: the self term and the messages add up)."""
    px, pw = P.CLASS_POOLS[cls]
    cap = P.LAYER_CAP_C if cls == 'C' else 0
    nnz = (2, 1, 1)
    a = -20 if scaled else 0
    gen = torch.Generator().manual_seed(seed)
    xi = [P.sparse_rows(px, b.cochains[d].num_cells, F, nnz[d], gen, cap=cap) for d in range(3)]
    with torch.no_grad():
        for d, lvl in enumerate(conv.mp_levels):
            lin = lvl.msg_up_nn[1]
            Wi = P.draw(pw, (F, 2 * F), gen, cap=cap)
            lin.weight.copy_(Wi.float())
            lin.bias.copy_(P.draw('one', (F,), gen).float())
            for x in xi:
                _no_dropped_terms(x.float(), Wi.float(), f'layer class {cls}')
    # the budget, on the unscaled integers
    for d in range(3):
        b.cochains[d].x = P.pieces_abs(xi[d])
    top = max(float(o.max()) for pair in _oracle_scope(_abs_conv(conv), b) for o in pair)
    assert top < P.EXACT_LIMIT, f'layer class {cls}: absolute terms sum to {top:.0f} >= 2^24'
    with torch.no_grad():
        for d, lvl in enumerate(conv.mp_levels):
            b.cochains[d].x = torch.ldexp(xi[d].float(), torch.tensor(a)).to(conv.mp_levels[0].eps1.device)
            lvl.msg_up_nn[1].bias.mul_(2.0 ** a)
    ref = _oracle_scope(conv, b, dtype=torch.float64)
    for up, bnd in ref:
        assert torch.equal(up.float().double(), up) and torch.equal(bnd.float().double(), bnd)
    return ref


def _run_variant(conv, b, variant, big=False):
    from cwn_amd import layers
    keep = (layers.LAYER_VARIANT, layers.BIG_ITEMS)
    try:
        layers.LAYER_VARIANT = variant
        if big:
            layers.BIG_ITEMS = 'always'
        layers._BLOCKED_CACHE.clear()
        b.block_plan().forget_csr()
        outs = _run(conv, b, blocked=True)                  # (asserts plans[0] == 'blocked')
        with torch.no_grad():
            table = conv._blocked_args(b.get_all_cochain_params(max_dim=2, include_down_features=False), 0)[2]
    finally:
        layers.LAYER_VARIANT, layers.BIG_ITEMS = keep
        layers._BLOCKED_CACHE.clear()
    return outs, table


@pytest.mark.parametrize('F', [64, 128])
@pytest.mark.parametrize('cls,scaled', CASES, ids=IDS)
def test_blocked_layer_split_terms(cls, scaled, F):
    """cwn_layer_fused_f32 on a ZINC-like batch of 50, eps = 0, in the 16-wave and the two-per-CU form."""
    b = _batch('zinc', 50, F, seed=5)
    conv = _conv(F, seed=6)
    ref = _layer_case(b, conv, F, cls, scaled, seed=100 + F)
    for variant in ('0', '1'):
        outs, table = _run_variant(conv, b, variant)
        assert table.variant == int(variant) and not table.n_big
        for d in range(3):
            _same(outs[2 * d], ref[d][0], f'blocked layer F={F} variant {variant} class {cls} scaled={scaled} out_up[{d}]')
            _same(outs[2 * d + 1], ref[d][1], f'blocked layer F={F} variant {variant} class {cls} scaled={scaled} out_b[{d}]')


@pytest.mark.parametrize('cls', ['A', 'B', 'C'])
def test_blocked_layer_split_terms_big_item(cls):
    """A batch with complexes beyond one workgroup's LDS at F = 128: their workgroups stream them (BIG records)."""
    F = 128
    b = _batch('molhiv', 40, F, seed=12)
    conv = _conv(F, seed=13)
    ref = _layer_case(b, conv, F, cls, False, seed=300)
    outs, table = _run_variant(conv, b, '0', big=True)
    assert table.variant == 0 and table.n_big > 0
    for d in range(3):
        _same(outs[2 * d], ref[d][0], f'blocked layer with big items, class {cls} out_up[{d}]')
        _same(outs[2 * d + 1], ref[d][1], f'blocked layer with big items, class {cls} out_b[{d}]')


# ------------------------------------------------------------------------------------------------
# the blocked layer: backward (atomic and owner form)
# ------------------------------------------------------------------------------------------------
def _backward_case(b, conv, F, cls, scaled, seed):
    """Output gradients from the class's X pool (one non-zero per row; on the edges' upper output every fourth row only: a
    ring's gY2 sums thirty entries), message weights from its W pool, forward features from `one` -- so the forward products
    are exact and the kernel's ReLU mask is the reference's.  Returns (gs, dx, gY1, gY2) with the exact float64 references;
    asserts from them that no dropped term exists and, with an all-ones mask, that the absolute terms of dx, gY1, gY2 sum to
    < 2^24."""
    px, pw = P.CLASS_POOLS[cls]
    cap = P.LAYER_CAP_C if cls == 'C' else 0
    a = -20 if scaled else 0
    gen = torch.Generator().manual_seed(seed)
    dev = conv.mp_levels[0].eps1.device
    rows = [b.cochains[d].num_cells for d in range(3)]
    with torch.no_grad():
        for d, lvl in enumerate(conv.mp_levels):
            b.cochains[d].x = P.sparse_rows('one', rows[d], F, 2, gen).float().to(dev)
            lin = lvl.msg_up_nn[1]
            lin.weight.copy_(P.draw(pw, (F, 2 * F), gen, cap=cap).float())
            lin.bias.copy_(P.draw('one', (F,), gen).float())
    gi = []
    for d in range(3):
        for up in (True, False):
            g = P.sparse_rows(px, rows[d], F, 1, gen, cap=cap)
            if up and d == 1:
                g[torch.arange(rows[d]) % 4 != 0] = 0
            gi.append(g)
    top = _propagate_reference_backward(_abs_conv(conv, big_bias=True), b, [P.pieces_abs(g) for g in gi], F)
    worst = max(float(t.max()) for part in top for t in part if t is not None)
    assert worst < P.EXACT_LIMIT, f'backward class {cls}: absolute terms sum to {worst:.0f} >= 2^24'
    dx, gy1, gy2 = _propagate_reference_backward(conv, b, [g.double() for g in gi], F)
    for d in range(2):                      # the products of the backward: gY1[d] W[:, :F] and gY2[d + 1] W[:, F:]
        W = cpu(conv.mp_levels[d].msg_up_nn[1].weight)
        for gy in (gy1[d], gy2[d + 1]):
            if gy is not None:
                assert float(gy.abs().max()) < P.EXACT_LIMIT
                _no_dropped_terms(gy.float(), W, f'backward class {cls} dim {d}')
    s = 2.0 ** a
    scale = lambda ts: [None if t is None else t * s for t in ts]
    return [(g.float() * s).to(dev) for g in gi], scale(dx), scale(gy1), scale(gy2)


@pytest.mark.parametrize('form', ['atomic', 'own'])
@pytest.mark.parametrize('F', [64, 128])
@pytest.mark.parametrize('cls,scaled', CASES, ids=IDS)
def test_blocked_backward_split_terms(cls, scaled, F, form):
    """cwn_layer_bwd_f32 and cwn_layer_bwd_own_f32, driven as test_blocked_backward_launch_vs_float64_autograd drives them:
    dx, gY1 and gY2 equal the float64 autograd of the plain restatement exactly."""
    from cwn_amd import csr, layers, ops
    b = _batch('zinc', 40, F, seed=31)
    conv = _conv(F, seed=32).train()
    gs, dx_ref, gy1_ref, gy2_ref = _backward_case(b, conv, F, cls, scaled, seed=400 + F)
    keep = layers.LAYER_VARIANT
    try:
        layers.LAYER_VARIANT = '0'                     # (the atomic form runs over the 16-wave table)
        args = conv._blocked_args(b.get_all_cochain_params(max_dim=2, include_down_features=False), 0, training=True)
    finally:
        layers.LAYER_VARIANT = keep
    assert not isinstance(args, str), args
    dims, plan, table, key = args
    assert table.variant == 0 and not table.n_big
    bwd_table = None
    if form == 'own':
        bwd_table = plan.bwd_items(F, [D.up_index is not None and D.up_index.size(1) > 0 for D in dims], [D.b_index is not None for D in dims])
        assert bwd_table is not None
    rows = [int(D.x.size(0)) for D in dims]
    ys_of = [[None, None] for _ in range(3)]
    for d in range(2):
        assert dims[d].up_index is not None and dims[d].up_index.size(1)
        ys_of[d][0] = torch.empty(rows[d], F, device=DEV)
        ys_of[d + 1][1] = torch.empty(rows[d + 1], F, device=DEV)
    ops.LayerLaunch(dims, table).run([D.x for D in dims], 0, ys=[tuple(p) for p in ys_of])
    ws = [conv.mp_levels[d].msg_up_nn[1].weight for d in range(2)]
    ops.pack_layer_weights_many(ws, transposed=True)
    wt_of = [ops.packed_layer_weight_t(ws[0]), ops.packed_layer_weight_t(ws[1]), None]
    before = list(ops.BLOCKED_BACKWARD_LAUNCHES)
    got = ops.layer_backward(dims, table, [tuple(p) for p in ys_of], [(gs[2 * d], gs[2 * d + 1]) for d in range(3)], wt_of,
                             bwd_table=bwd_table)
    assert got is not None
    which = 1 if form == 'own' else 0
    assert ops.BLOCKED_BACKWARD_LAUNCHES[which] == before[which] + 1, f'the {form} form did not run'
    csr.check_errors(DEV)
    dxs, gys = got
    what = f'blocked backward ({form}) F={F} class {cls} scaled={scaled}'
    for d in range(3):
        _same(dxs[d], dx_ref[d], f'{what} dx[{d}]')
        if gy1_ref[d] is not None:
            _same(gys[d][0], gy1_ref[d], f'{what} gY1[{d}]')
        if gy2_ref[d] is not None:
            _same(gys[d][1], gy2_ref[d], f'{what} gY2[{d}]')
