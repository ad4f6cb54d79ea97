"""The non-finite contract of the HIP kernels ("Non-finite values"): a live NaN / Inf comes out where the same
operation in plain torch, in float64 on the CPU, puts one -- and nowhere else.

Every case poisons ONE value (an element of row 0, an element of the last, partial row tile, the last column of an operand,
a bias or a weight entry, one source row of an aggregation, one cell of one complex) and hands the kernel's output and the
float64 reference to tests/_product.gate_nonfinite:
  (a) wherever the reference is non-finite the output is;
  (b) wherever the output is non-finite the reference is (a poison does not leak into another row / complex);
  (c) the entries finite in both are inside the project's gate, 1e-5 * max(1, |ref|_inf) in float32 and 1e-11 in float64;
  (d) the reference itself has a non-finite entry (and, for a row- or complex-local operation, a finite one).
The reference is never a product path: torch.relu, F.batch_norm, F.layer_norm, index_add_ / scatter_reduce_('amax'), matmul,
the float64 restatements of tests/_gin.py and tests/test_gpu_oriented.py, and the oracle for whole layers and models.

Poisons.  NaN is the main one and runs under (a) - (d) everywhere.  +Inf and -Inf run as a second parameter: (a), (c) and (d)
always; (b) only off the bf16-split kernels (cwn_gemm_split, cwn_gemm_tn's split form, the tile header of update_mlp /
update_mlp3 / the dense stage, the blocked layer kernel): there an Inf operand is split into NaN pieces (the documented limit
of csrc/cwn_split.h), so a relu(-Inf) that the reference maps to 0 may legitimately come out NaN.  Where the operation itself
maps an Inf to a finite value everywhere (relu(-Inf) = 0, tanh(Inf) = 1, a -Inf under a max beside finite values) the
reference of that tensor is finite and the plain gate applies to it (on the split kernels: (c) on the entries finite in
both); every test still requires, for every poison, that at least one of its tensors had a non-finite reference -- it flips the
sign of a scale so that a -Inf survives a ReLU prologue -- except for the pairs it names, where the mathematics leaves none.

Shapes: M = 70 rows (one row tile and a partial one), widths 64 and 128, N = 40 / K = 24 for the exact GEMM as well;
aggregations over the hub index of tests/test_gpu_parity.py (rows on both sides of CWN_LONG_ROW); layers and models on
batches of 4 - 8 ZINC-like complexes at width 64 / 128."""
import copy
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as Fn

from oracle import cwn_oracle as O
from tests._product import gate, gate_nonfinite, to_double

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
TOL = {F32: 1e-5, F64: 1e-11}
POISON = {'nan': float('nan'), '+inf': float('inf'), '-inf': float('-inf')}
POISONS = tuple(POISON)
ACT64 = {'id': lambda t: t, 'relu': torch.relu, 'elu': Fn.elu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid}


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


def cpu64(t):
    return t.detach().cpu().double()


def _finite_scale(r) -> float:
    r = cpu64(r)
    f = torch.isfinite(r)
    return max(1.0, float(r[f].abs().max())) if bool(f.any()) else 1.0


def _check(got, ref, what, poison, *, split=False, tol=1e-5, local=True) -> bool:
    """gate_nonfinite under the rules of the module docstring; a reference without a non-finite entry (the operation mapped
    the poison to a finite value, or this tensor is another complex's / dimension's) is held to the plain gate.  Returns
    whether the reference had a non-finite entry: every test requires that of at least one of its tensors."""
    r = cpu64(ref)
    if bool(torch.isfinite(r).all()):
        if split and poison != 'nan':
            # an Inf through a bf16-split kernel may come out NaN where the reference is finite: (b) is not asked, the entries
            # finite in both are still held to (c)
            gate_nonfinite(got, r, what + ' (finite reference, split kernel)', tol=tol, exact_mask=False, require_nonfinite=False)
        else:
            gate(got, r, what + ' (finite reference)', tol=tol)
        return False
    gate_nonfinite(got, r, what, tol=tol, exact_mask=(poison == 'nan' or not split), local=local)
    return True


def _put(t, index, value):
    t = t.clone()
    t[index] = value
    return t


# ------------------------------------------------------------------------------------------------
# 1. the grouped GEMM: ReLU epilogue, affine + ReLU prologue, column statistics -> BatchNorm -> ReLU
# ------------------------------------------------------------------------------------------------
def _run_gemm(path, make):
    """(outputs, served by the split kernel?) of one grouped launch with the split path allowed ('split') or not ('exact')."""
    from cwn_amd import ops
    prev = ops.set_gemm_exact(path == 'exact')
    try:
        split = ops.gemm_uses_split(make(), DEV)
        outs = ops.run_gemm(make(), DEV)
    finally:
        ops.set_gemm_exact(prev)
    assert not (path == 'exact' and split)
    return outs, split


GEMM_SHAPES = [('exact', 70, 128, 128), ('split', 70, 128, 128), ('exact', 70, 64, 64), ('split', 70, 64, 64), ('exact', 70, 40, 24)]


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('path,M,N,K', GEMM_SHAPES)
def test_gemm_relu_epilogue(path, M, N, K, poison):
    """relu(X W^T + b) of cwn_gemm_f32 (csrc/cwn_gemm.hip, exact) and its bf16-split form (csrc/cwn_gemm_split.hip): the
    poison in X (row 0; row 69, last column), in W (last column) and in the bias (last entry)."""
    from cwn_amd import ops
    v = POISON[poison]
    g = torch.Generator().manual_seed(M + N + K)
    X, W, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    cases = {'X[0, 3]': (_put(X, (0, 3), v), W, b), f'X[{M - 1}, {K - 1}]': (_put(X, (M - 1, K - 1), v), W, b),
             f'W[5, {K - 1}]': (X, _put(W, (5, K - 1), v), b), f'b[{N - 1}]': (X, W, _put(b, N - 1, v))}
    seen = False
    for place, (Xp, Wp, bp) in cases.items():
        ref = torch.relu(Xp.double() @ Wp.double().t() + bp.double())
        (got,), split = _run_gemm(path, lambda: [ops.Gemm(X=Xp.to(DEV), W=Wp.to(DEV), bias=bp.to(DEV), relu=True)])
        # (under the default policy the split kernel serves N = K = 128 and nothing else: the 64-wide launch of the 'split'
        #  parameter is the exact kernel reached without the CWN_GEMM_EXACT flag)
        assert split == (path == 'split' and N == K == 128), (path, N, K, split)
        seen |= _check(got, ref, f'gemm[{path}] {M}x{N}x{K} relu, {poison} at {place}', poison, split=split)
    assert seen


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('path,F', [('exact', 128), ('split', 128), ('exact', 64), ('split', 64)])
def test_gemm_prologue_statistics_batchnorm_relu(path, F, poison):
    """Z = relu(X * in_scale + in_shift) W^T + b with the per-band column statistics of its epilogue, then cwn_bn_finalize_f32
    and cwn_norm_act_f32 (csrc/cwn_norm.hip): a poisoned row makes its band's sums non-finite and the BatchNorm + ReLU output
    non-finite in every column that F.batch_norm(training=True) poisons; a poisoned bias entry does so for exactly its column."""
    from cwn_amd import _ffi, ops
    from cwn_amd.dense_train import _norm_desc
    v = POISON[poison]
    M = 70
    g = torch.Generator().manual_seed(F + 1)
    X, W, b = torch.randn(M, F, generator=g), torch.randn(F, F, generator=g) / F ** 0.5, torch.randn(F, generator=g)
    isc, ish = torch.rand(F, generator=g) + 0.5, torch.randn(F, generator=g)
    gam, bet = torch.rand(F, generator=g) + 0.5, torch.randn(F, generator=g)
    flip = lambda col: _put(isc, col, -isc[col]) if poison == '-inf' else isc      # (-Inf survives the prologue's ReLU)
    cases = {'X[0, 3]': (_put(X, (0, 3), v), b, flip(3), ish, False),
             f'X[{M - 1}, {F - 1}]': (_put(X, (M - 1, F - 1), v), b, flip(F - 1), ish, False),
             f'in_shift[{F - 1}]': (X, b, isc, _put(ish, F - 1, v), False),
             f'b[{F - 1}]': (X, _put(b, F - 1, v), isc, ish, True)}
    seen = False
    for place, (Xp, bp, sc, sh, local) in cases.items():
        what = f'gemm[{path}] F={F}, {poison} at {place}'
        Zr = torch.relu(Xp.double() * sc.double() + sh.double()) @ W.double().t() + bp.double()
        stats = torch.empty(2, ops.stat_rows(M), F, dtype=F64, device=DEV)
        (Z,), split = _run_gemm(path, lambda: [ops.Gemm(X=Xp.to(DEV), W=W.to(DEV), bias=bp.to(DEV), in_scale=sc.to(DEV),
                                                        in_shift=sh.to(DEV), in_relu=1, col_stats=stats)])
        assert not split        # (a prologue or statistics keep a launch on the exact kernel under either policy)
        if not _check(Z, Zr, what + ': Z', poison, split=split, local=local):
            continue                                          # (relu(-Inf + shift) = 0: nothing non-finite to follow)
        seen = True
        zs = _finite_scale(Zr)
        zp = torch.cat([Zr, Zr.new_zeros((-M) % 32, F)]).view(-1, 32, F)
        want = [zp.sum(1), (zp * zp).sum(1)]
        # a band sums 32 entries each within the gate e = 1e-5 zs of Z: 32 e, and 32 (2 zs e + e^2) for the squares
        for k, bound in ((0, 32 * 1e-5 * zs), (1, 32 * 2.1e-5 * zs * zs)):
            _check(stats[k], want[k], what + f': band {"sums" if k == 0 else "sums of squares"}', poison, split=split,
                   tol=bound / _finite_scale(want[k]), local=local)
        aff = torch.empty(4, F, device=DEV)
        rm, rv = torch.zeros(F, device=DEV), torch.ones(F, device=DEV)
        gd, bd = gam.to(DEV), bet.to(DEV)
        _ffi.bn_finalize([_ffi.BnDesc(col_sum=stats[0].data_ptr(), col_sumsq=stats[1].data_ptr(), gamma=gd.data_ptr(),
                                      beta=bd.data_ptr(), running_mean=rm.data_ptr(), running_var=rv.data_ptr(),
                                      scale=aff[0].data_ptr(), shift=aff[1].data_ptr(), mean=aff[2].data_ptr(),
                                      rstd=aff[3].data_ptr(), M=M, N=F, eps=1e-5, momentum=0.1)], DEV)
        H = torch.empty(M, F, device=DEV)
        _ffi.norm_act([_norm_desc(Z, out=H, aff=aff)], DEV)
        Hr = torch.relu(Fn.batch_norm(Zr, None, None, gam.double(), bet.double(), True, 0.1, 1e-5))
        # (the statistics mix a column's rows: an Inf entry poisons its whole column with NaN in the reference as well, so
        #  the masks are compared exactly on the split path too once Z itself is non-finite there)
        _check(H, Hr, what + ': relu(batch_norm(Z))', poison, split=False, local=local)
    assert seen


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('M,N,K', [(70, 128, 128), (70, 64, 64), (70, 40, 24)])
def test_gemm_tn_input_relu(M, N, K, poison):
    """dW = dZ^T relu(X * in_scale + in_shift), db = column sums of dZ (csrc/cwn_gemm_tn.hip; the library says which
    kernel serves a launch -- its bf16-split one at N = 128, the fp32-MFMA one at the narrower shapes, both of which the test
    requires to be covered): a poisoned X row gives the non-finite dW entries of the reference."""
    from cwn_amd import _ffi
    v = POISON[poison]
    g = torch.Generator().manual_seed(M + N + K + 7)
    dZ, X = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
    sc, sh = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g)
    flip = lambda col: _put(sc, col, -sc[col]) if poison == '-inf' else sc
    cases = {'X[0, 3]': (dZ, _put(X, (0, 3), v), flip(3), sh), f'X[{M - 1}, {K - 1}]': (dZ, _put(X, (M - 1, K - 1), v), flip(K - 1), sh),
             f'dZ[{M - 1}, {N - 1}]': (_put(dZ, (M - 1, N - 1), v), X, sc, sh), f'in_shift[{K - 1}]': (dZ, X, sc, _put(sh, K - 1, v))}
    seen = False
    for place, (dZp, Xp, scp, shp) in cases.items():
        dZd, Xd, scd, shd = dZp.to(DEV), Xp.to(DEV), scp.to(DEV), shp.to(DEV)
        dW, db = torch.zeros(N, K, device=DEV), torch.zeros(N, device=DEV)
        descs = [_ffi.GemmTnDesc(dZ=dZd.data_ptr(), X=Xd.data_ptr(), X2=None, in_scale=scd.data_ptr(), in_shift=shd.data_ptr(),
                                 in_scale2=None, in_shift2=None, dW=dW.data_ptr(), db=db.data_ptr(), M=M, lddz=N, ldx=K,
                                 ldx2=0, lddw=K, N=N, K=K, K2=0, in_relu=1)]
        split = _ffi.gemm_tn_would_split(descs)
        assert split == (N == 128), 'the shapes of this test no longer cover both kernels of cwn_gemm_tn_f32'
        _ffi.gemm_tn(descs, DEV)
        ref = dZp.double().t() @ torch.relu(Xp.double() * scp.double() + shp.double())
        what = f'gemm_tn {M}x{N}x{K}, {poison} at {place}'
        seen |= _check(dW, ref, what + ': dW', poison, split=split)
        _check(db, dZp.double().sum(0), what + ': db', poison, split=split)
    assert seen


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('N', [64, 128])
def test_norm_act(N, poison):
    """relu(z * scale + shift) of cwn_norm_act_f32: the poison in z and in the affine."""
    from cwn_amd import _ffi
    from cwn_amd.dense_train import _norm_desc
    v = POISON[poison]
    M = 70
    g = torch.Generator().manual_seed(N)
    z, aff = torch.randn(M, N, generator=g), torch.randn(4, N, generator=g)
    cases = {'z[0, 3]': (_put(z, (0, 3), v), aff), f'z[{M - 1}, {N - 1}]': (_put(z, (M - 1, N - 1), v), aff),
             f'scale[{N - 1}]': (z, _put(aff, (0, N - 1), v)), 'shift[5]': (z, _put(aff, (1, 5), v))}
    seen = False
    for place, (zp, ap) in cases.items():
        zd, ad = zp.to(DEV), ap.to(DEV)
        out = torch.empty(M, N, device=DEV)
        _ffi.norm_act([_norm_desc(zd, out=out, aff=ad)], DEV)
        ref = torch.relu(zp.double() * ap[0].double() + ap[1].double())
        seen |= _check(out, ref, f'norm_act N={N}, {poison} at {place}', poison)
    assert seen


@pytest.mark.parametrize('poison', POISONS)
def test_layer_norm_act_many(poison):
    """relu(LayerNorm(z)) of two matrices in one launch (csrc/cwn_layernorm.hip): a poisoned element gives a non-finite row,
    exactly that row; a poisoned weight entry exactly its column."""
    from cwn_amd import ops
    v = POISON[poison]
    g = torch.Generator().manual_seed(3)
    zs = [torch.randn(70, 64, generator=g), torch.randn(33, 128, generator=g)]
    norms = [torch.nn.LayerNorm(64), torch.nn.LayerNorm(128)]
    with torch.no_grad():
        for n in norms:
            n.weight.copy_(torch.rand(n.weight.shape, generator=g) + 0.5)
            n.bias.copy_(torch.randn(n.bias.shape, generator=g))
    cases = {'z0[0, 3]': (0, 'z', (0, 3)), 'z0[69, 63]': (0, 'z', (69, 63)), 'z1[32, 127]': (1, 'z', (32, 127)), 'weight0[5]': (0, 'w', 5)}
    seen = False
    for place, (k, which, index) in cases.items():
        zp, np_ = [z.clone() for z in zs], copy.deepcopy(norms)
        with torch.no_grad():
            (zp[k] if which == 'z' else np_[k].weight)[index] = v
        with torch.no_grad():
            outs = ops.layer_norm_act_many([z.to(DEV) for z in zp], [n.to(DEV) for n in copy.deepcopy(np_)], relu=True)
        for j in range(2):
            ref = torch.relu(Fn.layer_norm(zp[j].double(), (zp[j].size(1),), np_[j].weight.detach().double(), np_[j].bias.detach().double(), np_[j].eps))
            seen |= _check(outs[j], ref, f'layer_norm_act_many, {poison} at {place}: matrix {j}', poison)
    assert seen


# ------------------------------------------------------------------------------------------------
# 2. the fused dense networks of a layer: update_mlp, update_mlp3, the training stage kernel (all on the bf16 split)
# ------------------------------------------------------------------------------------------------
def _randomise_bn(conv, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in conv.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.copy_(0.2 * torch.randn(m.num_features, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
                m.weight.copy_(0.5 + torch.rand(m.num_features, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.num_features, generator=g))


def _dense_eval_counted(conv, outs, name):
    """conv._dense_eval on `outs`, with the launches of ops.<name> counted (update_mlp also runs as a prepared
    ops.MlpLaunch): (outputs, [did the call launch?, ...])."""
    from cwn_amd import ops
    calls = []
    targets = [(ops, name)] + ([(ops.MlpLaunch, 'run')] if name == 'update_mlp' else [])
    origs = [getattr(o, a) for o, a in targets]

    def counted(fn):
        def call(*a, **kw):
            res = fn(*a, **kw)
            calls.append(res is not None)
            return res
        return call

    for (o, a), fn in zip(targets, origs):
        setattr(o, a, counted(fn))
    try:
        ops.weights_changed()
        with torch.no_grad():
            got = conv._dense_eval(['blocked'] * 3, outs, 0)
    finally:
        for (o, a), fn in zip(targets, origs):
            setattr(o, a, fn)
    return got, calls


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('F', [64, 128])
def test_update_mlp(F, poison):
    """cwn_update_mlp_f32 (csrc/cwn_mlp.hip, epilogue in csrc/cwn_tile.h): update_up_nn, update_boundaries_nn and combine_nn
    of three dimensions in one launch against the same torch modules in float64; the poison in an input (row 0 of one
    network, the last row and column of the other) and in the first weight of a network."""
    from cwn_amd.layers import SparseCINConv
    v = POISON[poison]
    rows = (70, 33, 5)
    for place in ('up input [0, 3] of dim 0', f'boundary input [69, {F - 1}] of dim 0', f'update_up_nn[0].weight[5, {F - 1}] of dim 1'):
        torch.manual_seed(F)
        conv = SparseCINConv(F, F, F, None, None, None, None, max_dim=2, hidden=F, act_module=torch.nn.ReLU, layer_dim=F,
                             use_coboundaries=True, graph_norm=torch.nn.BatchNorm1d).eval()
        _randomise_bn(conv, 1)
        g = torch.Generator().manual_seed(2)
        outs = [torch.randn(n, F, generator=g) for n in rows for _ in range(2)]
        with torch.no_grad():
            if place.startswith('up input'):
                outs[0][0, 3] = v
            elif place.startswith('boundary input'):
                outs[1][69, F - 1] = v
            else:
                conv.mp_levels[1].update_up_nn[0].weight[5, F - 1] = v
        conv64 = copy.deepcopy(conv).double()
        with torch.no_grad():
            ref = [lvl.combine_nn(torch.cat([lvl.update_up_nn(outs[2 * d].double()), lvl.update_boundaries_nn(outs[2 * d + 1].double())], -1))
                   for d, lvl in enumerate(conv64.mp_levels)]
        got, calls = _dense_eval_counted(conv.to(DEV), [o.to(DEV) for o in outs], 'update_mlp')
        assert any(calls), 'the fused launch was not taken'
        seen = False
        for d in range(3):
            seen |= _check(got[d], ref[d], f'update_mlp F={F}, {poison} at {place}: dim {d}', poison, split=True,
                           local='weight' not in place)
        assert seen


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('F', [64, 128])
def test_update_mlp3(F, poison):
    """cwn_update_mlp3_f32 (csrc/cwn_mlp3.hip): the three update networks and the 3F-wide combine of a CIN++ layer."""
    from cwn_amd.layers import CINppConv
    v = POISON[poison]
    rows = (70, 33, 5)
    for place in ('up input [0, 3] of dim 0', f'down input [69, {F - 1}] of dim 0', f'update_up_nn[0].weight[5, {F - 1}] of dim 1'):
        torch.manual_seed(F + 1)
        conv = CINppConv(F, F, F, None, None, None, None, None, None, max_dim=2, hidden=F, eps=0.0, train_eps=True,
                         act_module=torch.nn.ReLU, layer_dim=F, use_coboundaries=True).eval()
        _randomise_bn(conv, 3)
        g = torch.Generator().manual_seed(4)
        outs = [torch.randn(n, F, generator=g) for n in rows for _ in range(3)]
        with torch.no_grad():
            if place.startswith('up input'):
                outs[0][0, 3] = v
            elif place.startswith('down input'):
                outs[1][69, F - 1] = v
            else:
                conv.mp_levels[1].update_up_nn[0].weight[5, F - 1] = v
        conv64 = copy.deepcopy(conv).double()
        with torch.no_grad():
            ref = [lvl.combine_nn(torch.cat([lvl.update_up_nn(outs[3 * d].double()), lvl.update_down_nn(outs[3 * d + 1].double()),
                                             lvl.update_boundaries_nn(outs[3 * d + 2].double())], -1))
                   for d, lvl in enumerate(conv64.mp_levels)]
        got, calls = _dense_eval_counted(conv.to(DEV), [o.to(DEV) for o in outs], 'update_mlp3')
        assert any(calls), 'the fused launch was not taken'
        seen = False
        for d in range(3):
            seen |= _check(got[d], ref[d], f'update_mlp3 F={F}, {poison} at {place}: dim {d}', poison, split=True,
                           local='weight' not in place)
        assert seen


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('F', [64, 128])
def test_dense_stage(F, poison):
    """cwn_dense_stage_f32 (csrc/cwn_stage.hip): Z = relu(X * in_scale + in_shift) W^T + b of a training stage, with its band
    statistics; the poison in X and in the (packed) weight."""
    from cwn_amd import ops
    v = POISON[poison]
    M = 70
    g = torch.Generator().manual_seed(F + 5)
    X, W, b = torch.randn(M, F, generator=g), torch.randn(F, F, generator=g) / F ** 0.5, torch.randn(F, generator=g)
    sc, sh = torch.rand(F, generator=g) + 0.5, torch.randn(F, generator=g)
    flip = lambda col: _put(sc, col, -sc[col]) if poison == '-inf' else sc
    cases = {'X[0, 3]': (_put(X, (0, 3), v), W, flip(3)), f'X[{M - 1}, {F - 1}]': (_put(X, (M - 1, F - 1), v), W, flip(F - 1)),
             f'W[5, {F - 1}]': (X, _put(W, (5, F - 1), v), sc)}
    seen = False
    for place, (Xp, Wp, scp) in cases.items():
        Wd = Wp.to(DEV)
        ops.pack_stage_weights_many([Wd])
        stats = torch.zeros(2, ops.stat_rows(M), F, dtype=F64, device=DEV)
        got = ops.run_stage([ops.Gemm(X=Xp.to(DEV), W=Wd, bias=b.to(DEV), in_scale=scp.to(DEV), in_shift=sh.to(DEV), in_relu=1,
                                      col_stats=stats)], DEV)
        assert got is not None, 'the stage kernel refused a launch it is written for'
        Zr = torch.relu(Xp.double() * scp.double() + sh.double()) @ Wp.double().t() + b.double()
        what = f'dense stage F={F}, {poison} at {place}'
        seen |= _check(got[0], Zr, what + ': Z', poison, split=True)
        zp = torch.cat([Zr, Zr.new_zeros((-M) % 32, F)]).view(-1, 32, F)
        _check(stats[0], zp.sum(1), what + ': band sums', poison, split=True, tol=32 * 1e-5 * _finite_scale(Zr) / _finite_scale(zp.sum(1)))
    assert seen


# ------------------------------------------------------------------------------------------------
# 3. aggregation: reductions, ReLU messages, activated messages
# ------------------------------------------------------------------------------------------------
N_DST, N_SRC, N_AUX, SRC, LONELY = 300, 211, 50, 17, 7
_HUB = {}


def _hub():
    """The hub index of tests/test_gpu_parity.py (rows of 1500, 700, 65 and 64 entries among short ones) with row LONELY
    listing source SRC and nothing else (a max over -Inf alone): (index, aux, Adjacency), built once."""
    if not _HUB:
        from cwn_amd.csr import Adjacency
        from tests.test_gpu_parity import _hub_index
        idx, aux = _hub_index(torch.Generator().manual_seed(11), N_DST, N_SRC, N_AUX)
        keep = idx[1] != LONELY
        idx = torch.cat([idx[:, keep], torch.tensor([[SRC] * 3, [LONELY] * 3])], 1)
        aux = torch.cat([aux[keep], torch.tensor([1, 2, 3])])
        adj = Adjacency.from_index(idx.to(DEV), N_DST, N_SRC, aux.to(DEV), N_AUX)
        assert adj.long_row_list().numel() >= 3
        lists = torch.zeros(N_DST, dtype=torch.bool)
        lists[idx[1][idx[0] == SRC]] = True
        deg = torch.bincount(idx[1], minlength=N_DST)
        # the poisoned source is listed by long rows and by short ones, and not by every row
        assert bool(lists[5]) and bool((lists & (deg <= 16)).any()) and bool((~lists).any())
        _HUB['v'] = (idx, aux, adj)
    return _HUB['v']


def _scatter64(msg, dst, n_dst, reduce):
    out = torch.zeros(n_dst, msg.size(1), dtype=F64)
    if reduce == 'max':
        return out.scatter_reduce_(0, dst.unsqueeze(1).expand_as(msg), msg, 'amax', include_self=False)
    out.index_add_(0, dst, msg)
    if reduce == 'mean':
        out = out / torch.bincount(dst, minlength=n_dst).clamp(min=1).double().unsqueeze(1)
    return out


@pytest.mark.parametrize('F', [3, 64, 128])
@pytest.mark.parametrize('reduce', ['add', 'mean', 'max'])
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_aggregate_reductions(dtype, reduce, F):
    """cwn_aggregate_f32 / _f64 (csrc/cwn_aggregate_body.h), messages A and A + B under add, mean and max: a poisoned source row
    reaches exactly the destinations that list it -- short rows, rows beyond CWN_LONG_ROW (the whole-workgroup pass) and, at
    F = 3, the entry-parallel fold -- as index_add_ / scatter_reduce_('amax') say; a row of -Inf alone has the maximum -Inf."""
    from cwn_amd import ops
    idx, aux, adj = _hub()
    g = torch.Generator().manual_seed(F + len(reduce))
    x = torch.randn(N_SRC, F, generator=g, dtype=F64).to(dtype)
    ua = torch.randn(N_AUX, F, generator=g, dtype=F64).to(dtype)
    sx = torch.randn(N_DST, F, generator=g, dtype=F64).to(dtype)
    for poison, v in POISON.items():
        xp = x.clone()
        xp[SRC] = v
        for op, name in ((ops.MSG_A, 'A'), (ops.MSG_A_PLUS_B, 'A + B')):
            got = ops.aggregate(adj, N_DST, xp.to(DEV), msg_op=op, reduce=reduce, B=ua.to(DEV) if op != ops.MSG_A else None,
                                self_x=sx.to(DEV))
            msg = xp.double()[idx[0]] + (ua.double()[aux] if op != ops.MSG_A else 0.0)
            ref = _scatter64(msg, idx[1], N_DST, reduce) + sx.double()
            assert got.dtype == dtype
            assert _check(got, ref, f'aggregate {dtype} {reduce} F={F} message {name}, source row {SRC} = {poison}', poison, tol=TOL[dtype])


@pytest.mark.parametrize('F', [64, 128])
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_aggregate_relu_messages(dtype, F):
    """The four ReLU messages of cwn_aggregate_*: relu(a + b), relu(a + b)^2, 2 a relu(pre + b) and (pre + b <= 0 ? 0 : a),
    summed; the poison in a source row of A and in one element of B.  The last is ReLU's gradient as torch's threshold_backward
    states it: the gradient a passes unless pre + b <= 0.  These four are served under reduce = add alone: with mean or max the
    launchers refuse the descriptor on the host (check_desc in csrc/cwn_aggregate_body.h, CWN_ERR_BAD_ARG) before anything is
    launched, in both precisions -- there is no ReLU message under mean or max to poison, and the test pins that."""
    from cwn_amd import _ffi, ops
    _, _, adj = _hub()
    col, auxc = adj.col.cpu().long(), adj.aux.cpu().long()
    dst = torch.repeat_interleave(torch.arange(N_DST), torch.diff(adj.rowptr.cpu().long()))
    g = torch.Generator().manual_seed(F + 13)
    A = torch.randn(N_SRC, F, generator=g, dtype=F64).to(dtype)
    B = torch.randn(N_AUX, F, generator=g, dtype=F64).to(dtype)
    pre = torch.randn(N_DST, F, generator=g, dtype=F64).to(dtype)
    forms = {ops.MSG_RELU_A_PLUS_B: lambda a, b, p: torch.relu(a + b),
             ops.MSG_RELU_A_PLUS_B_SQ: lambda a, b, p: torch.relu(a + b) ** 2,
             ops.MSG_A_TIMES_2RELU: lambda a, b, p: 2.0 * a * torch.relu(p + b),
             ops.MSG_A_MASK_RELU: lambda a, b, p: torch.where(p + b <= 0, torch.zeros_like(a), a)}      # (threshold_backward)
    for poison, v in POISON.items():
        seen = {op: False for op in forms}
        for place in ('A', 'B'):
            Ap, Bp = (_put(A, SRC, v), B) if place == 'A' else (A, _put(B, (3, 5), v))
            specs = [ops.AggSpec(adj, N_DST, F, A=Ap.to(DEV), ia=adj.col, B=Bp.to(DEV), ib=adj.aux, msg_op=op, self_pre=pre.to(DEV))
                     for op in forms]
            outs = ops.run_aggregate(specs, DEV)
            for (op, form), out in zip(forms.items(), outs):
                msg = form(Ap.double()[col], Bp.double()[auxc], pre.double()[dst])
                ref = torch.zeros(N_DST, F, dtype=F64).index_add_(0, dst, msg)
                seen[op] |= _check(out, ref, f'aggregate {dtype} F={F} message op {op}, {poison} in {place}', poison, tol=TOL[dtype])
        # (relu(-Inf + b) = 0 and its square are finite: -Inf shows in the two forms that multiply by a)
        assert all(seen[op] for op in forms if poison != '-inf' or op in (ops.MSG_A_TIMES_2RELU, ops.MSG_A_MASK_RELU)), (poison, seen)
    for op in forms:
        for reduce in (1, 2):                                 # CWN_REDUCE_MEAN, CWN_REDUCE_MAX
            with pytest.raises(_ffi.CwnError, match='aggregate'):
                ops.run_aggregate([ops.AggSpec(adj, N_DST, F, A=A.to(DEV), ia=adj.col, B=B.to(DEV), ib=adj.aux, msg_op=op, reduce=reduce,
                                               self_pre=pre.to(DEV))], DEV)


@pytest.mark.parametrize('act', ['relu', 'elu', 'tanh', 'sigmoid'])
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_aggregate_act(dtype, act):
    """sum_p act(A[src_p] + B[cob_p]) + (1 + eps) x of cwn_aggregate_act_f32 / _f64, rows of 0 .. 300 entries."""
    from cwn_amd import ops
    from tests.test_gpu_act_message import LENGTHS, N_COB, _Graph
    F = 64
    gr = _Graph(list(LENGTHS) + [3, 5, 0, 9, 2, 11, 1, 4], seed=21)
    g = torch.Generator().manual_seed(F + len(act))
    mk = lambda n: torch.randn(n, F, generator=g, dtype=F64).to(dtype)
    A, B, sx = mk(23), mk(N_COB), mk(gr.n_dst)
    eps = torch.tensor([0.25], dtype=dtype, device=DEV)
    seen = dict.fromkeys(POISON, False)
    for poison, v in POISON.items():
        Ap = _put(A, 4, v)
        out, = ops.aggregate_many([ops.Stream(adj=gr.adj, n_dst=gr.n_dst, width=F, A=Ap.to(DEV), B=B.to(DEV), msg_op=ops.MSG_A_PLUS_B,
                                              ib_mode='aux', act=act, self_x=sx.to(DEV), eps=eps)])
        msg = ACT64[act](Ap.double()[gr.src] + B.double()[gr.cob])
        ref = torch.zeros(gr.n_dst, F, dtype=F64).index_add_(0, gr.dst, msg) + 1.25 * sx.double()
        seen[poison] |= _check(out, ref, f'aggregate_act {dtype} {act}, source row 4 = {poison}', poison, tol=TOL[dtype])
    # finite by the mathematics: relu(-Inf) = 0, elu(-Inf) = -1, tanh(+-Inf) = +-1, sigmoid(+-Inf) = 1 / 0
    finite = {('relu', '-inf'), ('elu', '-inf'), ('tanh', '+inf'), ('tanh', '-inf'), ('sigmoid', '+inf'), ('sigmoid', '-inf')}
    assert all(seen[p] or (act, p) in finite for p in POISON), seen


# ------------------------------------------------------------------------------------------------
# 4. the blocked layer kernel and the two-kernel routes it replaces
# ------------------------------------------------------------------------------------------------
def _layer_batch(form, F):
    from cwn_amd.complex import ComplexBatch
    from cwn_amd.synthetic import zinc_like_complexes
    from tests.test_gpu_blocked import _batch
    if form != 'big':
        return _batch('zinc', 4, F, seed=51), 1
    lo, hi = (70, 90) if F == 128 else (130, 200)
    cxs = zinc_like_complexes(3, 41, 6) + zinc_like_complexes(1, 42, 6, n_lo=lo, n_hi=hi)
    b = ComplexBatch.from_complex_list(cxs, max_dim=2).to(DEV)
    g = torch.Generator().manual_seed(43)
    for d in range(3):
        b.cochains[d].x = torch.randn(b.cochains[d].num_cells, F, generator=g).to(DEV)
    return b, 3


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('form', ['16-wave', 'two-per-cu', 'big'])
@pytest.mark.parametrize('F', [64, 128])
def test_blocked_layer(F, form, poison):
    """cwn_layer_fused_f32 (csrc/cwn_layer.hip) in its 16-wave and two-per-CU forms and with a BIG record, on four complexes
    with one vertex feature of one complex poisoned: the rows of that complex which the oracle's propagate + self terms give
    non-finite are non-finite, no row of another complex is, and the two-kernel routes (grouped GEMM on the split / on fp32
    MFMA + the CSR aggregation) agree under the same mask."""
    from cwn_amd import csr, layers, ops
    from tests.test_gpu_blocked import _conv, _oracle_scope, _run
    b, c = _layer_batch(form, F)
    batch0 = b.cochains[0].batch.cpu()
    row = int(torch.nonzero(batch0 == c).flatten()[1])
    b.cochains[0].x = _put(b.cochains[0].x, (row, 3), POISON[poison])
    conv = _conv(F, seed=52, eps=0.25)
    ref = _oracle_scope(conv, b)
    for d in range(3):                      # the reference itself keeps the poison inside its complex
        bad = ~torch.isfinite(torch.stack(ref[d])).all(-1).all(0)
        assert bool((b.cochains[d].batch.cpu()[bad] == c).all())
    keep_v, keep_b = layers.LAYER_VARIANT, layers.BIG_ITEMS
    try:
        layers.LAYER_VARIANT = '1' if form == 'two-per-cu' else '0'
        if form == 'big':
            layers.BIG_ITEMS = 'always'
        layers._BLOCKED_CACHE.clear()
        b.block_plan().forget_csr()
        with torch.no_grad():
            table = conv._blocked_args(b.get_all_cochain_params(max_dim=2, include_down_features=False), 0)[2]
        assert table.variant == int(layers.LAYER_VARIANT) and (table.n_big >= 1) == (form == 'big'), (table.variant, table.n_big)
        outs = {'blocked': _run(conv, b, blocked=True)}
    finally:
        layers.LAYER_VARIANT, layers.BIG_ITEMS = keep_v, keep_b
        layers._BLOCKED_CACHE.clear()
    for exact in (False, True):
        prev = ops.set_gemm_exact(exact)
        try:
            csr._cache.clear()
            outs['csr+exact' if exact else 'csr+split'] = _run(conv, b, blocked=False)
        finally:
            ops.set_gemm_exact(prev)
    for route, got in outs.items():
        seen = False
        for d in range(3):
            for k, name in ((0, 'out_up'), (1, 'out_b')):
                seen |= _check(got[2 * d + k], ref[d][k], f'layer [{route}, {form}] F={F} {name}[{d}], {poison} in complex {c}', poison,
                               split=route != 'csr+exact')
        assert seen


# ------------------------------------------------------------------------------------------------
# 5. the baseline launches: GIN layer, oriented layer, embed_pool, agnostic_head
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', ['relu', 'elu'])
def test_gin_layer(act):
    from tests import _gin
    from tests.test_gpu_gin import _operands, _plan, _raw
    x, stages = _operands(64, 64, 70, 5)
    idx, adj = _plan(70)
    sd = [tuple(t.to(DEV) for t in s) for s in stages]
    eps_dev = torch.tensor([0.37], device=DEV)
    s = int(idx[0][0])                                       # a row that some entry lists
    seen = dict.fromkeys(POISON, False)
    for poison, v in POISON.items():
        cases = {f'x[{s}, 3]': (_put(x, (s, 3), v), stages, sd)}
        W1 = _put(stages[0][0], (5, 63), v)
        st_w = [(W1,) + tuple(stages[0][1:]), stages[1]]
        cases['W1[5, 63]'] = (x, st_w, [tuple(t.to(DEV) for t in q) for q in st_w])
        for place, (xp, st, std) in cases.items():
            out = _raw(xp.to(DEV), adj, eps_dev, std, act, act)
            ref = _gin.gin_formula64(xp, idx, 0.37, st, act, act)
            seen[poison] |= _check(out, ref, f'gin_layer {act}, {poison} at {place}', poison, local='x[' in place)
    assert all(seen.values()), seen          # (an Inf meets weights of both signs: +Inf survives relu and elu either way)


@pytest.mark.parametrize('act', ['relu', 'tanh'])
def test_oriented_layer(act):
    from tests.test_gpu_oriented import _formula64, _plan, _raw
    n, w, H = 70, 64, 64
    g = torch.Generator().manual_seed(31)
    x = torch.randn(n, w, generator=g)
    ws = [torch.randn(H, w, generator=g) / (3 * w) ** 0.5 for _ in range(3)]
    (iu, au), (il, al) = _plan(n, 'up'), _plan(n, 'dn')
    wd = [t.to(DEV) for t in ws]
    s = int(iu[0][0])
    seen = dict.fromkeys(POISON, False)
    for poison, v in POISON.items():
        xp = _put(x, (s, 3), v)
        out, _ = _raw(xp.to(DEV), (au, None), (al, None), wd[0], wd[1], wd[2], act, H)
        ref = _formula64(xp, (iu, None), (il, None), ws[0], ws[1], ws[2], act)
        seen[poison] |= _check(out, ref, f'oriented_layer {act}, x[{s}, 3] = {poison}', poison)
    assert all(seen[p] or (act == 'tanh' and p != 'nan') for p in POISON), seen          # (tanh(+-Inf) = +-1)


@pytest.mark.parametrize('act', ['relu', 'sigmoid'])
@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_embed_pool_and_agnostic_head(dtype, act):
    """ops.embed_pool (sum over a complex's rows of act(x W^T + b)) and ops.agnostic_head (sum_d act(pooled_d W1^T + b1) W2^T + b2):
    a poisoned cell poisons its complex's pooled row and prediction, and no other."""
    from cwn_amd import ops
    g = torch.Generator().manual_seed(41)
    sizes = [9, 70, 1, 33, 5]
    C, K, H, Oc = len(sizes), 33, 64, 3
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.tensor(sizes).cumsum(0)])
    mk = lambda *s: torch.randn(*s, generator=g, dtype=F64).to(dtype)
    x, w0, b0 = mk(sum(sizes), K), mk(H, K) / K ** 0.5, mk(H)
    w1, b1, w2, b2 = mk(H, H) / H ** 0.5, mk(H), mk(Oc, H) / H ** 0.5, mk(Oc)
    dev = lambda t: t.to(DEV)
    seen = dict.fromkeys(POISON, False)
    for poison, v in POISON.items():
        xp = _put(x, (int(ptr[1]) + 69, K - 1), v)              # the last row of complex 1, last column
        pooled, = ops.embed_pool([dev(xp)], [dev(ptr)], C, [dev(w0)], [dev(b0)], act)
        y = ACT64[act](xp.double() @ w0.double().t() + b0.double())
        pref = torch.stack([y[int(ptr[c]):int(ptr[c + 1])].sum(0) for c in range(C)])
        what = f'{dtype} {act}, {poison} in complex 1'
        hit = _check(pooled, pref, 'embed_pool ' + what, poison, tol=TOL[dtype])
        seen[poison] |= hit
        # the head on the REFERENCE's pooled rows, rounded to the dtype: its own contract, whatever embed_pool gave
        pin = pref.to(dtype)
        out = ops.agnostic_head([dev(pin)], dev(w1), dev(b1), dev(w2), dev(b2), act, n_complexes=C)
        oref = ACT64[act](pin.double() @ w1.double().t() + b1.double()) @ w2.double().t() + b2.double()
        if hit:
            assert _check(out, oref, 'agnostic_head ' + what, poison, tol=TOL[dtype]) or (act == 'sigmoid' and poison != 'nan')
    assert all(seen[p] or (act == 'sigmoid' and p != 'nan') for p in POISON), seen       # (sigmoid(+-Inf) = 1 / 0)


# ------------------------------------------------------------------------------------------------
# 6. the head
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('mean', [False, True], ids=['sum', 'mean'])
@pytest.mark.parametrize('train', [False, True], ids=['head', 'head_train'])
def test_head(train, mean, poison):
    """cwn_head_f32 through ops.head and ops.head_train: pool, relu(lin1) per dimension, their sum, lin2.  A poisoned cell of one
    complex gives that complex a non-finite pooled row and prediction and leaves the others finite; both readouts."""
    from cwn_amd import ops
    g = torch.Generator().manual_seed(61)
    C, K, H2 = 5, 64, 128
    sizes = [torch.tensor([9, 70, 1, 33, 5]), torch.tensor([12, 75, 0, 30, 4]), torch.tensor([1, 11, 0, 3, 0])]
    ptrs = [torch.cat([torch.zeros(1, dtype=torch.long), s.cumsum(0)]) for s in sizes]
    xs = [torch.randn(int(s.sum()), K, generator=g) for s in sizes]
    xs[1] = _put(xs[1], (int(ptrs[1][1]) + 74, 5), POISON[poison])         # the last edge of complex 1
    lin1 = [torch.nn.Linear(K, H2) for _ in range(3)]
    lin2 = torch.nn.Linear(H2, 2)
    pooled = []
    for d in range(3):
        p = torch.stack([xs[d].double()[int(ptrs[d][c]):int(ptrs[d][c + 1])].sum(0) for c in range(C)])
        pooled.append(p / sizes[d].clamp(min=1).double().unsqueeze(1) if mean else p)
    l64 = [copy.deepcopy(l).double() for l in lin1 + [lin2]]
    with torch.no_grad():
        ref = l64[3](sum(torch.relu(l64[d](pooled[d])) for d in range(3)))
    lin1, lin2 = [l.to(DEV) for l in lin1], lin2.to(DEV)
    args = ([x.to(DEV) for x in xs], [p.to(DEV) for p in ptrs], C, [l.weight for l in lin1], [l.bias for l in lin1], lin2.weight, lin2.bias)
    if train:
        out, got_pooled = ops.head_train(*args, mean_readout=mean)
    else:
        with torch.no_grad():
            out, got_pooled = ops.head(*args, mean_readout=mean, want_pooled=True)
    what = f'{"head_train" if train else "head"} [{"mean" if mean else "sum"}], {poison} in complex 1'
    assert _check(got_pooled[1], pooled[1], what + ': pooled edges', poison)
    _check(got_pooled[0], pooled[0], what + ': pooled vertices', poison)
    assert _check(out, ref, what + ': prediction', poison)
    assert bool(torch.isfinite(out[[0, 2, 3, 4]]).all()) and not bool(torch.isfinite(out[1]).any())


# ------------------------------------------------------------------------------------------------
# 7. the loss launches: the maxima inside log-softmax and BCE are followed by a subtraction that keeps the NaN
# ------------------------------------------------------------------------------------------------
def _loss_operands(task):
    g = torch.Generator().manual_seed(71)
    if task == 'classification':
        return torch.randn(8, 5, generator=g), torch.randint(0, 5, (8,), generator=g)
    return torch.randn(8, 3, generator=g), torch.randint(0, 2, (8, 3), generator=g).float()


def _loss64(task, pred, y):
    if task == 'classification':
        return Fn.cross_entropy(pred.double(), y)
    return Fn.binary_cross_entropy_with_logits(pred.double(), y.double())


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('task', ['classification', 'bin_classification'])
def test_training_loss(task, poison):
    """cwn_loss_cols_f32 (csrc/cwn_norm.hip) through train.fused_loss."""
    from cwn_amd.train import fused_loss
    pred, y = _loss_operands(task)
    pred = _put(pred, (1, 2), POISON[poison])
    loss = fused_loss(task, pred.to(DEV), y.to(DEV))
    assert loss is not None
    seen = _check(loss.view(1), _loss64(task, pred, y).view(1), f'fused {task} loss, {poison} in a prediction', poison, local=False)
    assert seen or (task, poison) == ('classification', '-inf')         # (softmax gives a -Inf logit the weight 0: a finite loss)


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('task', ['classification', 'bin_classification'])
def test_evaluation_loss_segments(task, poison):
    """cwn_loss_segments_f32 (csrc/cwn_metrics.hip) through evaluate.loss_segments: the segment that holds the poison, only."""
    from cwn_amd.evaluate import loss_segments
    pred, y = _loss_operands(task)
    pred = _put(pred, (1, 2), POISON[poison])
    ptr = torch.tensor([0, 3, 8])
    out = loss_segments(task, pred.to(DEV).contiguous(), y.to(DEV), ptr.to(DEV))
    ref = torch.stack([_loss64(task, pred[lo:hi], y[lo:hi]) for lo, hi in ((0, 3), (3, 8))])
    seen = _check(out, ref, f'{task} loss per segment, {poison} in segment 0', poison)
    assert seen or (task, poison) == ('classification', '-inf')


# ------------------------------------------------------------------------------------------------
# 8. models
# ------------------------------------------------------------------------------------------------
H = 64


def _cin_model(seed, norm='bn'):
    from cwn_amd.models import SparseCIN
    torch.manual_seed(seed)
    model = SparseCIN(H, 1, 2, H, dropout_rate=0.0, max_dim=2, jump_mode=None, nonlinearity='relu', readout='sum', train_eps=False,
                      final_hidden_multiplier=2, use_coboundaries=True, final_readout='sum', graph_norm=norm).eval()
    _randomise_bn(model, seed + 1)
    return model


def _cin_batch(seed, n=6):
    """n ZINC-like complexes with float features of width H on the CPU (the models overwrite a batch's features: every
    forward takes a fresh copy on the device)."""
    from cwn_amd.synthetic import zinc_like_batch
    b = zinc_like_batch(n, seed=seed, max_ring=6)
    g = torch.Generator().manual_seed(seed + 3)
    for d in range(3):
        b.cochains[d].x = torch.randn(b.cochains[d].num_cells, H, generator=g)
    return b


def _poison_cell(b, c, v):
    """One feature of the second vertex of complex c."""
    row = int(torch.nonzero(b.cochains[0].batch == c).flatten()[1])
    b.cochains[0].x = _put(b.cochains[0].x, (row, 3), v)
    return b


def _cx64(b):
    cx = {'dimension': b.dimension, 'y': None, 'num_complexes': b.num_complexes, 'cochains': [
        {k: (None if b.cochains[d][k] is None else b.cochains[d][k].detach().cpu())
         for k in ('x', 'upper_index', 'lower_index', 'shared_boundaries', 'shared_coboundaries', 'boundary_index', 'y', 'batch')}
        for d in range(b.dimension + 1)]}
    for c in cx['cochains']:
        c['x'] = c['x'].double()
    return cx


def _fresh(b):
    return copy.deepcopy(b).to(DEV)


ROUTES = ['blocked+split', 'csr+split', 'csr+exact']


def _forward(model, b, route):
    from cwn_amd import layers, ops
    prev_b, prev_e = layers.BLOCKED_LAYER, ops.set_gemm_exact(route.endswith('exact'))
    layers.BLOCKED_LAYER = route.startswith('blocked')
    try:
        with torch.no_grad():
            y, res = model(_fresh(b), include_partial=True)
        assert (model.convs[0].blocked_reason is None) == route.startswith('blocked'), model.convs[0].blocked_reason
    finally:
        layers.BLOCKED_LAYER = prev_b
        ops.set_gemm_exact(prev_e)
    return y, res


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('route', ROUTES)
def test_model_eval_one_poisoned_feature(route, poison):
    """SparseCIN (2 layers, hidden 64, BatchNorm in eval) on six complexes, one input feature of complex 2 poisoned: every layer
    output and the prediction against the oracle in float64 -- non-finite for that complex only -- on the three routes of
    tests/test_gpu_parity.py::test_config2_eval_forward_full_size_vs_float64_oracle."""
    model = _cin_model(81)
    b = _poison_cell(_cin_batch(82), 2, POISON[poison])
    ref, rpart = O.sparse_cin_model_forward(to_double(model.state_dict()), _cx64(b), 2, embed=None)
    assert not bool(torch.isfinite(ref[2]).any()) and bool(torch.isfinite(ref[[0, 1, 3, 4, 5]]).all())
    y, res = _forward(model.to(DEV), b, route)
    split = route != 'csr+exact'
    for k, r in rpart.items():
        _check(res[k], r, f'SparseCIN [{route}] {k}, {poison} in complex 2', poison, split=split)
    assert _check(y, ref, f'SparseCIN [{route}] prediction, {poison} in complex 2', poison, split=split)


@pytest.mark.parametrize('route', ROUTES)
def test_model_eval_one_nan_weight(route):
    """The same model with one NaN entry in a first-layer weight: every prediction is NaN."""
    model = _cin_model(83)
    with torch.no_grad():
        model.convs[0].mp_levels[0].update_up_nn[0].weight[3, 5] = float('nan')
    b = _cin_batch(84)
    ref, _ = O.sparse_cin_model_forward(to_double(model.state_dict()), _cx64(b), 2, embed=None)
    assert not bool(torch.isfinite(ref).any())
    y, _ = _forward(model.to(DEV), b, route)
    _check(y, ref, f'SparseCIN [{route}] prediction with a NaN weight', 'nan', local=False)


def test_training_step_with_a_nan_feature():
    """One optimisation step (BatchNorm in training mode) on a batch with one NaN feature, captured in a graph and eagerly: the
    returned loss is NaN, every parameter gradient is non-finite wherever float64 CPU autograd over the oracle's forward has a
    non-finite gradient, and the two forms of the step give the same mask."""
    from cwn_amd.train import TrainStep
    b = _poison_cell(_cin_batch(85, n=8), 3, float('nan'))
    model = _cin_model(86)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    leaves = {k: v.double().requires_grad_(True) for k, v in state.items() if v.is_floating_point() and 'running' not in k}
    ostate = dict(to_double(state))
    ostate.update(leaves)
    ref_out, _ = O.sparse_cin_model_forward(ostate, _cx64(b), 2, embed=None, training=True, norm='bn')
    ref_loss = (ref_out - b.y.double().view(-1, 1)).abs().mean()
    ref_loss.backward()
    assert not bool(torch.isfinite(ref_loss))
    masks = {}
    for form in ('captured', 'eager'):
        m = copy.deepcopy(model).to(DEV)
        ts = TrainStep(m, [_fresh(b)], use_graph=form == 'captured')
        loss = ts.step(0)
        torch.cuda.synchronize()
        assert not bool(torch.isfinite(loss)), (form, float(loss))
        masks[form] = {}
        n_bad, finite = 0, []
        for name, p in m.named_parameters():
            r = leaves[name].grad
            if r is None:
                continue
            assert p.grad is not None, name
            bad_ref, bad_got = ~torch.isfinite(r), ~torch.isfinite(p.grad.detach().cpu())
            n_bad += int(bad_ref.sum())
            missed = int((bad_ref & ~bad_got).sum())
            print(f'[gate_nonfinite] training step ({form}) grad {name}: ref non-finite {int(bad_ref.sum())} of {r.numel()}, '
                  f'got non-finite {int(bad_got.sum())}, finite where ref is not: {missed}')
            if missed:
                finite.append((name, missed, float(p.grad.detach().abs().nan_to_num(nan=-1.0).max())))
            masks[form][name] = bad_got
        assert n_bad > 0
        assert not finite, f'{form} step: gradients finite where float64 autograd has none: {finite}'
    for name in masks['eager']:
        assert torch.equal(masks['eager'][name], masks['captured'][name]), name


def test_evaluator_refuses_the_nan_prediction_of_a_fused_forward():
    """evaluate.infer over the fused inference path hands the NaN prediction on, and the Evaluator raises the ValueError that
    INTEGRATION.md promises instead of scoring it."""
    from cwn_amd import evaluate
    model = _cin_model(87).to(DEV)
    b = _poison_cell(_cin_batch(88), 2, float('nan'))
    pred = evaluate.infer((model, [_fresh(b)]))
    assert model.convs[0].blocked_reason is None, model.convs[0].blocked_reason
    bad = ~torch.isfinite(pred.cpu()).view(-1)
    assert bad.tolist() == [False, False, True, False, False, False]
    y = torch.tensor([0., 1., 1., 0., 1., 0.]).view(-1, 1)
    with pytest.raises(ValueError, match='NaN or infinity'):
        evaluate.Evaluator('ogbg-molhiv').eval({'y_true': y, 'y_pred': pred})
    assert evaluate.Evaluator('ogbg-molhiv').eval({'y_true': y[~bad], 'y_pred': pred[~bad.to(pred.device)]}) >= 0.0


def test_layer_norm_model_with_a_nan_feature():
    """SparseCIN with graph_norm='ln' (the LayerNorm launches)."""
    model = _cin_model(89, norm='ln')
    b = _poison_cell(_cin_batch(90), 4, float('nan'))
    ref, rpart = O.sparse_cin_model_forward(to_double(model.state_dict()), _cx64(b), 2, embed=None, norm='ln')
    with torch.no_grad():
        y, res = model.to(DEV)(_fresh(b), include_partial=True)
    for k, r in rpart.items():
        _check(res[k], r, f'SparseCIN ln {k}, NaN in complex 4', 'nan')
    assert _check(y, ref, 'SparseCIN ln prediction, NaN in complex 4', 'nan')


def test_gin_model_with_a_nan_feature():
    """GIN0 on the fused GIN launches against the float64 restatement of tests/_gin.py."""
    from cwn_amd import layers
    from tests import _gin
    from tests import test_gin_host as host
    torch.manual_seed(11)
    model = _gin.randomise(host._make('GIN0', None, nonlinearity='relu', readout='sum'), 3).eval()
    _, ns0 = host._ring()
    ns = SimpleNamespace(x=ns0.x.clone(), edge_index=ns0.edge_index.clone(), batch=ns0.batch.clone(), mask=ns0.mask.clone())
    row = int(torch.nonzero(ns.batch == 5).flatten()[0])
    ns.x[row, 0] = float('nan')
    ref = host.reference64('GIN0', None, model, ns, 'relu', 'sum')
    model = model.to(DEV)
    old, layers.FUSED_GIN = layers.FUSED_GIN, True
    try:
        with torch.no_grad():
            out = model(SimpleNamespace(**{k: t.to(DEV) for k, t in vars(ns).items()}))
    finally:
        layers.FUSED_GIN = old
    assert _check(out, ref, 'GIN0, NaN in graph 5', 'nan')


def test_agnostic_model_with_a_nan_feature():
    """MessagePassingAgnostic on its two launches against its formula in float64."""
    from tests._agnostic import case_batch, fixture_model
    model = fixture_model('relu', 'sum', F32)
    b = case_batch('dummy_mixed', F32)
    row = int(torch.nonzero(b.cochains[0].batch == 1).flatten()[0])
    b.cochains[0].x = _put(b.cochains[0].x, (row, 0), float('nan'))
    st = {k: t.detach().double() for k, t in model.state_dict().items()}
    C = b.num_complexes
    hs = []
    for d in range(3):
        if d <= b.dimension and b.cochains[d].x is not None:
            h = torch.relu(b.cochains[d].x.double() @ st[f'lin0s.{d}.weight'].t() + st[f'lin0s.{d}.bias'])
            pooled = torch.zeros(C, h.size(1), dtype=F64).index_add_(0, b.cochains[d].batch, h)
        else:
            pooled = torch.zeros(C, st['lin1.weight'].size(1), dtype=F64)
        hs.append(torch.relu(pooled @ st['lin1.weight'].t() + st['lin1.bias']))
    ref = sum(hs) @ st['lin2.weight'].t() + st['lin2.bias']
    model = model.to(DEV)
    with torch.no_grad():
        out = model(_fresh(b))
    assert model.last_route == 'fused'
    assert _check(out, ref, 'MessagePassingAgnostic, NaN in complex 1', 'nan')
