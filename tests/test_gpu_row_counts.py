"""The device-side row-count contract of include/cwn_hip.h ("DEVICE-SIDE ROW COUNTS") on every f32 entry point that carries a
count: with `m_dev` / `n_dev` given, the host row count is only the CAPACITY of the buffers, and

    "Rows in [*m_dev, capacity) are never written and never enter a reduction."

Every test here puts one kernel at the live counts where hand-written live-row logic goes wrong -- 0, 1, the capacity, and one
below / at / one above every tile height in use (16 / 32 / 48 / 64 / 96 / 128) -- over capacity-sized operands whose padding
rows hold NaN (inputs) and a sentinel (outputs), and asserts per live count
  (a) the rows below the count, and every reduction output, against a float64 reference evaluated on the CPU from the live
      rows only, inside tests/_product.gate: 1e-5 * max(1, |ref|_inf);
  (b) row-wise kernels: bit-identical to the same entry point called with M = live, m_dev = NULL, on a copy of the live rows;
  (c) every output row at or beyond the count still holds the sentinel, bit for bit;
  (d) a count of 0 is harmless: zero reductions, accumulated targets left as they were, nothing NaN.
NaN is the poison on purpose: a kernel may LOAD padding rows into a tile, but must discard them by selection -- a product
with zero would pass NaN on.  (cwn_layernorm_*, cwn_aggregate_f64 and the cross-entropy form of cwn_loss_cols_f32 have
their contract tests in test_gpu_layernorm.py, test_gpu_f64.py and test_gpu_static_csr.py.)"""
import ctypes as C

import pytest
import torch

from cwn_amd import _ffi, ops
from tests._product import gate

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CAP = 200                      # a few tiles of every tile height in use
SENT = -9.0
LIVES = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128, 129, 199, 200)
NAN = float('nan')
_COUNT = {}


def _count(live: int) -> torch.Tensor:
    """THE device int64 the launches of this module read their row count from, rewritten between launches."""
    if 'n' not in _COUNT:
        _COUNT['n'] = torch.zeros(3, dtype=torch.int64, device=DEV)
    _COUNT['n'].fill_(int(live))
    return _COUNT['n']


def _launch(live, ins, outs, fn, cap=CAP, dynamic=True, pad=None):
    """One launch of the sweep.  `ins`: name -> CPU tensor [cap, ...]; `outs`: name -> the shape behind the row dimension (a
    float32 row output) or a CPU tensor handed over as it is (a reduction target, a pre-filled output).
    dynamic: capacity-sized operands, input rows >= live hold NaN (`pad[name]` for index inputs), row outputs the sentinel,
    `live` in a device int64, fn(I, O) run inside _ffi.dynamic_rows({cap: its address}).
    not dynamic: the same launch as a caller without a device-side count issues it -- M = live, copies of the live rows."""
    rows = cap if dynamic else live
    I, O = {}, {}
    for name, t in ins.items():
        d = t[:rows].clone()
        if dynamic:
            d[live:] = (pad or {}).get(name, NAN)
        I[name] = d.to(DEV)
    for name, spec in outs.items():
        if isinstance(spec, torch.Tensor):
            O[name] = (spec if dynamic or spec.size(0) != cap else spec[:rows]).clone().to(DEV)
        else:
            O[name] = torch.full((rows,) + tuple(spec), SENT, dtype=torch.float32, device=DEV)
    if dynamic:
        with _ffi.dynamic_rows({cap: _count(live).data_ptr()}):
            fn(I, O)
    else:
        fn(I, O)
    return I, O


def _untouched(t, live, what):
    """(c): rows >= live hold the sentinel, bit for bit (a NaN written there fails too)."""
    assert bool((t[live:] == SENT).all()), f'{what}: a row at or beyond the live count {live} was written'


def _rand(g, *shape):
    return torch.randn(*shape, generator=g)


def _stream():
    return _ffi.stream_ptr(DEV)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. cwn_gemm_f32
# ------------------------------------------------------------------------------------------------------------------------------
GEMM_CASES = {
    # name: (N, K, K2, w_trans, add_out, packed, relu, runs on the bf16-split kernel)
    'exact_40x24': (40, 24, 0, False, False, False, True, False),
    'exact_64x64': (64, 64, 0, False, False, False, False, False),
    'split_128': (128, 128, 0, False, False, False, True, True),
    'split_128_packed': (128, 128, 0, False, False, True, False, True),
    'w_trans_40x24': (40, 24, 0, True, False, False, False, False),
    'w_trans_128': (128, 128, 0, True, False, False, False, False),
    'concat_x2': (64, 24, 12, False, False, False, True, False),
    'add_out_40x24': (40, 24, 0, False, True, False, False, False),
    'add_out_128': (128, 128, 0, False, True, False, False, False),
}


@pytest.mark.parametrize('case', sorted(GEMM_CASES))
def test_gemm_device_side_row_count(case):
    """cwn_gemm_f32 (csrc/cwn_gemm.hip, csrc/cwn_gemm_split.hip): "the workgroups walk the row tiles below *m_dev only" and "rows
    in [*m_dev, capacity) are never written" -- the exact kernel on its 64 x 64 (N = 40, K = 24; 64 x 64; K-concatenation with
    X2) and 32 x 128 (transposed weight at 128) tiles, the bf16-split kernel with the fp32 and the CWN_GEMM_W_PACKED weight,
    w_trans, and CWN_GEMM_ADD_OUT, where the padding rows of a pre-filled Y stay as they were.  Live counts: LIVES.
    FOUND by this test: both kernels bounded their STORES by the capacity -- the last live tile wrote its rows beyond the count
    (NaN from NaN padding, and with ADD_OUT onto rows the contract says are not touched) at every live % tile != 0; the
    stores are now bounded by the count."""
    N, K, K2, w_trans, add_out, packed, relu, split = GEMM_CASES[case]
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    X, X2 = _rand(g, CAP, K), (_rand(g, CAP, K2) if K2 else None)
    Wc = _rand(g, K + K2, N) / (K + K2) ** 0.5 if w_trans else _rand(g, N, K + K2) / (K + K2) ** 0.5
    W = torch.nn.Parameter(Wc.to(DEV))
    bias, Y0 = _rand(g, N), _rand(g, CAP, N)
    bd = bias.to(DEV)
    pk = ops.pack_gemm_weight(W) if packed else None
    assert not packed or pk is not None
    ins = {'X': X} if X2 is None else {'X': X, 'X2': X2}
    outs = {'Y': Y0 if add_out else (N,)}

    def run(I, O):
        gm = ops.Gemm(X=I['X'], X2=I.get('X2'), W=W.detach(), bias=bd, relu=relu, w_trans=w_trans, out=O['Y'], add_out=add_out,
                      w_packed=pk)
        assert ops.gemm_uses_split([gm], DEV) == split
        assert gm.desc(O['Y']).m_dev == _ffi.dyn(I['X'].size(0))
        ops.run_gemm([gm], DEV)

    for live in LIVES:
        _, O = _launch(live, ins, outs, run)
        x = X[:live].double() if X2 is None else torch.cat([X[:live], X2[:live]], 1).double()
        ref = x @ (Wc.double() if w_trans else Wc.double().t()) + bias.double()
        ref = ref.relu() if relu else ref
        ref = ref + Y0[:live].double() if add_out else ref
        Y = O['Y']
        assert not torch.isnan(Y[:live]).any()
        gate(Y[:live], ref, f'gemm {case} live={live}')
        if add_out:
            assert torch.equal(Y[live:].cpu(), Y0[live:]), f'gemm {case} live={live}: ADD_OUT touched a padding row'
        else:
            _untouched(Y, live, f'gemm {case} Y')
        if live:
            _, S = _launch(live, ins, outs, run, dynamic=False)
            assert torch.equal(Y[:live], S['Y']), f'gemm {case} live={live}: not the bits of the M = live call'


def test_gemm_refuses_a_row_count_with_statistics_or_the_batchnorm_prologue():
    """cwn_gemm_desc.m_dev: "Not with col_sum / col_sumsq or bnb (CWN_ERR_BAD_ARG)" -- the C ABI refuses, and ops.Gemm.desc
    raises inside _ffi.dynamic_rows instead of dropping the count (a statistic over the capacity rows of a static batch)."""
    g = torch.Generator().manual_seed(1)
    X, W = _rand(g, CAP, 64).to(DEV), _rand(g, 64, 64).to(DEV)
    Y = torch.empty(CAP, 64, device=DEV)
    stats = torch.zeros(2, ops.stat_rows(CAP), 64, dtype=torch.float64, device=DEV)
    z, dz = torch.zeros(CAP, 64, device=DEV), torch.empty(CAP, 64, device=DEV)
    bnb = _ffi.GemmBnb(z=z.data_ptr(), dz=dz.data_ptr(), ldz=64, lddz=64, relu=1)
    for gm in (ops.Gemm(X=X, W=W, col_stats=stats), ops.Gemm(X=X, W=W, w_trans=True, bnb=bnb)):
        d = gm.desc(Y)
        assert d.m_dev is None
        ops.run_gemm([gm], DEV)                                   # (without a count: served)
        d.m_dev = _count(17).data_ptr()
        rc = _ffi.lib().cwn_gemm_f32((_ffi.GemmDesc * 1)(d), 1, _stream())
        assert rc == 1, rc                                        # CWN_ERR_BAD_ARG
        with _ffi.dynamic_rows({CAP: _count(17).data_ptr()}):
            with pytest.raises(RuntimeError, match='CWN_STAGE_KERNEL'):
                gm.desc(Y)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------------
# 2. cwn_gemm_tn_f32
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('deterministic', [False, True])
@pytest.mark.parametrize('N,K,K2', [(128, 128, 0), (128, 128, 128), (64, 64, 0), (64, 64, 64), (40, 24, 0), (40, 24, 12)])
def test_gemm_tn_device_side_row_count(N, K, K2, deterministic):
    """cwn_gemm_tn_f32 (csrc/cwn_gemm_tn.hip): m_dev = "actual rows of the reduction (M = capacity: grid, workspace layout)" --
    dW / db take the live rows only, with the in_relu prologue in front of X (relu(NaN * scale + shift) of a padding row must
    not reach dW), with and without X2; the bf16-split form (128 x 128) and the fp32 form (64 x 64, 40 x 24); the atomic
    form ADDS onto what the targets hold (a count of 0 leaves them as they were), the workspace form (DETERMINISTIC_TN) run twice
    into the same targets doubles them bit for bit.  Live counts: LIVES."""
    g = torch.Generator().manual_seed(N + K + K2 + deterministic)
    dZ, X, X2 = _rand(g, CAP, N), _rand(g, CAP, K), (_rand(g, CAP, K2) if K2 else None)
    sc, sh = torch.rand(K, generator=g) + 0.5, _rand(g, K)
    scd, shd = sc.to(DEV), sh.to(DEV)
    start = 0.0 if deterministic else 0.5
    ins = {'dZ': dZ, 'X': X} if X2 is None else {'dZ': dZ, 'X': X, 'X2': X2}
    outs = {'dW': torch.full((N, K + K2), start), 'db': torch.full((N,), start)}

    def run(I, O):
        rows = I['X'].size(0)
        x2 = I.get('X2')
        desc = lambda: [_ffi.GemmTnDesc(dZ=I['dZ'].data_ptr(), X=I['X'].data_ptr(), X2=_ffi.ptr(x2), in_scale=scd.data_ptr(),
                                        in_shift=shd.data_ptr(), in_scale2=None, in_shift2=None, dW=O['dW'].data_ptr(),
                                        db=O['db'].data_ptr(), M=rows, lddz=N, ldx=K, ldx2=K2, lddw=K + K2, N=N, K=K, K2=K2,
                                        in_relu=1)]
        if not deterministic:
            return _ffi.gemm_tn(desc(), DEV)
        _ffi.DETERMINISTIC_TN = True
        try:
            _ffi.gemm_tn(desc(), DEV)
            O['first'] = O['dW'].clone(), O['db'].clone()
            _ffi.gemm_tn(desc(), DEV)
        finally:
            _ffi.DETERMINISTIC_TN = False

    for live in LIVES:
        _, O = _launch(live, ins, outs, run)
        A = torch.relu(X[:live].double() * sc.double() + sh.double())
        if X2 is not None:
            A = torch.cat([A, X2[:live].double()], 1)
        ref_w, ref_b = dZ[:live].double().t() @ A, dZ[:live].double().sum(0)
        what = f'gemm_tn {N}x{K}+{K2} det={deterministic} live={live}'
        if deterministic:
            assert torch.equal(O['dW'], 2 * O['first'][0]) and torch.equal(O['db'], 2 * O['first'][1]), what
            dW, db = O['first']
        else:
            dW, db = O['dW'], O['db']
        gate(dW, ref_w + start, what + ' dW')
        gate(db, ref_b + start, what + ' db')
        if live == 0:
            assert bool((dW == start).all()) and bool((db == start).all()), what


# ------------------------------------------------------------------------------------------------------------------------------
# 3. cwn_dense_stage_f32 / cwn_dense_stage_ex_f32 / cwn_dense_stage_bwd_f32     4. the BatchNorm(train) pieces behind them
# ------------------------------------------------------------------------------------------------------------------------------
EPS, MOM = 1e-5, 0.1


def _stage_weight(g, F, blocks):
    W = torch.nn.Parameter((_rand(g, F, blocks * F) / (blocks * F) ** 0.5).to(DEV))
    ops.pack_stage_weights_many([W])
    return W


def _stage_launch(I, O, W, F, bias, pro, stat_slots=None, extra_relu=None):
    """cwn_dense_stage_f32 (or _ex with a third block) over X (, X2 (, X3)) of I into O['Y'] and the band statistics O['cs'] /
    O['cq'] (or `stat_slots`), the descriptor as ops.run_stage builds it."""
    X, X2, X3 = I['X'], I.get('X2'), I.get('X3')
    rows = X.size(0)
    sc, sh, sc2, sh2 = pro
    d = _ffi.StageDesc(X=X.data_ptr(), X2=_ffi.ptr(X2), w_packed=ops.packed_stage_block(W, 0).data_ptr(),
                       w2_packed=None if X2 is None else ops.packed_stage_block(W, F).data_ptr(), bias=_ffi.ptr(bias),
                       in_scale=_ffi.ptr(sc), in_shift=_ffi.ptr(sh), in_scale2=_ffi.ptr(sc2), in_shift2=_ffi.ptr(sh2),
                       Y=O['Y'].data_ptr(), col_sum=None if stat_slots is not None else O['cs'].data_ptr(),
                       col_sumsq=None if stat_slots is not None else O['cq'].data_ptr(), M=rows, ldx=F, ldx2=0 if X2 is None else F,
                       ldy=F, in_relu=1 if X2 is None else 3, m_dev=_ffi.dyn(rows), stat_slots=_ffi.ptr(stat_slots))
    arr = (_ffi.StageDesc * 1)(d)
    if X3 is None:
        _ffi.check(_ffi.lib().cwn_dense_stage_f32(arr, 1, F, _stream()), 'cwn_dense_stage_f32')
    else:
        ex = (_ffi.StageExtra * 2)()
        ex[0].X, ex[0].w_packed, ex[0].ldx, ex[0].relu = X3.data_ptr(), ops.packed_stage_block(W, 2 * F).data_ptr(), F, int(extra_relu)
        _ffi.check(_ffi.lib().cwn_dense_stage_ex_f32(arr, ex, 1, F, _stream()), 'cwn_dense_stage_ex_f32')


def _stage_ref(X, X2, X3, W, bias, pro, live, extra_relu):
    sc, sh, sc2, sh2 = [None if t is None else t.double() for t in pro]
    x = [(X[:live].double() * sc + sh).relu()]
    if X2 is not None:
        x.append((X2[:live].double() * sc2 + sh2).relu())
    if X3 is not None:
        x.append(X3[:live].double().relu() if extra_relu else X3[:live].double())
    return torch.cat(x, 1) @ W.double().t() + bias.double()


def _band_sums(z, F):
    zp = torch.cat([z, z.new_zeros((-z.size(0)) % 32, F)]).view(-1, 32, F)
    return zp.sum(1), (zp * zp).sum(1)


@pytest.mark.parametrize('F', [64, 128])
@pytest.mark.parametrize('form', ['single', 'cat', 'ex'])
def test_dense_stage_device_side_row_count(F, form):
    """cwn_dense_stage_f32 / cwn_dense_stage_ex_f32 (csrc/cwn_stage.hip): m_dev = "actual rows (M = capacity; col_sum / col_sumsq
    hold CWN_STAT_ROWS(M) bands, the first CWN_STAT_ROWS(*m_dev) are written)" -- Y of the live rows, the per-band statistics
    of the live rows only (the band the count ends in sums its live rows, not the NaN behind them), the bands beyond left as
    they were; F -> F, 2F -> F and the 3F -> F form with an extra block.  Live counts: LIVES."""
    g = torch.Generator().manual_seed(F + len(form))
    blocks = {'single': 1, 'cat': 2, 'ex': 3}[form]
    W = _stage_weight(g, F, blocks)
    Wc = W.detach().cpu()
    bias = _rand(g, F)
    pro = [torch.rand(F, generator=g) + 0.5, _rand(g, F), torch.rand(F, generator=g) + 0.5, _rand(g, F)]
    if blocks == 1:
        pro[2] = pro[3] = None
    bd, prod = bias.to(DEV), [None if t is None else t.to(DEV) for t in pro]
    ins = {name: _rand(g, CAP, F) for name in ('X', 'X2', 'X3')[:blocks]}
    bands = ops.stat_rows(CAP)
    outs = {'Y': (F,), 'cs': torch.full((bands, F), SENT, dtype=torch.float64), 'cq': torch.full((bands, F), SENT, dtype=torch.float64)}
    run = lambda I, O: _stage_launch(I, O, W, F, bd, prod, extra_relu=True)
    for live in LIVES:
        _, O = _launch(live, ins, outs, run)
        what = f'stage {form} F={F} live={live}'
        ref = _stage_ref(ins['X'], ins.get('X2'), ins.get('X3'), Wc, bias, pro, live, True)
        gate(O['Y'][:live], ref, what + ' Y')
        _untouched(O['Y'], live, what + ' Y')
        nb = ops.stat_rows(live)
        s, q = _band_sums(ref, F)
        gate(O['cs'][:nb], s, what + ' col_sum')
        gate(O['cq'][:nb], q, what + ' col_sumsq')
        _untouched(O['cs'], nb, what + ' col_sum bands')
        _untouched(O['cq'], nb, what + ' col_sumsq bands')
        if live:
            souts = dict(outs, cs=torch.full((nb, F), SENT, dtype=torch.float64), cq=torch.full((nb, F), SENT, dtype=torch.float64))
            _, S = _launch(live, ins, souts, run, dynamic=False)
            assert torch.equal(O['Y'][:live], S['Y']) and torch.equal(O['cs'][:nb], S['cs']) and torch.equal(O['cq'][:nb], S['cq']), what


def _bn_reference(z, gamma, beta, dy, rm0, rv0):
    """BatchNorm1d(train) + ReLU in float64 over the rows of z: (h, dz, dgamma, dbeta, running_mean, running_var, mean, var).
    torch.nn.BatchNorm1d and its autograd from two rows on; one row (torch refuses it) by the same formulas: biased variance 0,
    the running variance takes it as it is (cwn_bn_finalize_f32: "Mv > 1 ? unbiased : var")."""
    M, N = z.shape
    z = z.double()
    if M >= 2:
        bn = torch.nn.BatchNorm1d(N, eps=EPS, momentum=MOM).double()
        with torch.no_grad():
            bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rm0), bn.running_var.copy_(rv0)
        zz = z.clone().requires_grad_(True)
        h = torch.relu(bn(zz))
        h.backward(dy.double())
        return (h.detach(), zz.grad, bn.weight.grad, bn.bias.grad, bn.running_mean.clone(), bn.running_var.clone(), z.mean(0),
                z.var(0, unbiased=False))
    mean, var = z.mean(0), torch.zeros(N, dtype=torch.float64)
    h = torch.relu(beta.double()).expand(M, N)
    dyh = dy.double() * (beta.double() > 0)
    return (h, torch.zeros(M, N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64), dyh.sum(0),
            (1 - MOM) * rm0.double() + MOM * mean, (1 - MOM) * rv0.double() + MOM * var, mean, var)


def _one_row_out(out, z, aff, what):
    """A batch of ONE row is outside what the reference defines (torch.nn.BatchNorm1d refuses to train on it) and outside what fp32
    can hold to the gate: its variance is 0, rstd = eps^-1/2 = 316, and out = z * scale + shift cancels |z| * 316 * gamma ~ 1e3
    down to beta.  The constants (mean, rstd, running statistics) are still gated against float64; the activation is held to
    float64 of ITS OWN operation on the constants it was handed, within what the number format allows: one rounding of the
    product and one of the sum, each at most 2^-24 of max(|z * scale|, |shift|) -- 2^-23 * max(|z * scale|, |shift|)."""
    a = aff.detach().cpu().double()
    ref = torch.relu(z.double() * a[0] + a[1])
    bound = 2.0 ** -23 * max(float((z.double() * a[0]).abs().max()), float(a[1].abs().max()))
    err = float((out.detach().cpu().double() - ref).abs().max())
    print(f'[one row] {what}: max|delta| = {err:.3e}  bound 2^-23 max(|z scale|, |shift|) = {bound:.3e}')
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize('F', [64, 128])
def test_batchnorm_pieces_device_side_row_count(F):
    """cwn_bn_finalize_f32, cwn_norm_act_f32, cwn_norm_bwd_reduce_f32, cwn_norm_bwd_apply_f32 and cwn_norm_bwd_f32
    (csrc/cwn_norm.hip), fed by the band statistics a cwn_dense_stage_f32 launch left under the same count: "the first
    CWN_STAT_ROWS(*m_dev) [bands] are summed" and divided by *m_dev, "*m_dev < 1: ... the running statistics are left alone";
    out / dz of the live rows, s1 / s2 (d beta, d gamma) over the live rows, against torch.nn.BatchNorm1d(train) + ReLU and
    its autograd in float64 on the live rows of the kernel's own z, running statistics and batch counter included.
    Live counts: LIVES (the activation of a ONE-row batch: _one_row_out)."""
    g = torch.Generator().manual_seed(7 * F)
    W = _stage_weight(g, F, 1)
    bias = (_rand(g, F) * 2).to(DEV)
    pro = [(torch.rand(F, generator=g) + 0.5).to(DEV), _rand(g, F).to(DEV), None, None]
    gamma, beta = torch.rand(F, generator=g) + 0.5, _rand(g, F)
    rm0, rv0 = _rand(g, F), torch.rand(F, generator=g) + 0.5
    gd, bd = gamma.to(DEV), beta.to(DEV)
    X, dY = _rand(g, CAP, F), _rand(g, CAP, F)
    bands = ops.stat_rows(CAP)
    outs = {'Y': (F,), 'cs': torch.full((bands, F), SENT, dtype=torch.float64), 'cq': torch.full((bands, F), SENT, dtype=torch.float64),
            'H': (F,), 'dz': (F,), 'dz2': (F,), 'aff': torch.full((4, F), SENT), 'rm': rm0, 'rv': rv0,
            'nbt': torch.full((1,), 5, dtype=torch.int64), 's12': torch.zeros(2, F), 'bwd_sums': torch.full((2, F), SENT),
            'acc': torch.full((2, F), 0.25), 't12': torch.full((2, F), SENT), 'u12': torch.full((2, F), 2.5)}

    def run(I, O):
        from cwn_amd.dense_train import _norm_desc
        _stage_launch(I, O, W, F, bias, pro)
        rows = I['X'].size(0)
        if _ffi.dyn(rows) is not None:
            O['Y'][live:] = NAN                                           # the padding rows of z: poison for what follows
        aff = O['aff']
        _ffi.bn_finalize([_ffi.BnDesc(col_sum=O['cs'].data_ptr(), col_sumsq=O['cq'].data_ptr(), gamma=gd.data_ptr(), beta=bd.data_ptr(),
                                      running_mean=O['rm'].data_ptr(), running_var=O['rv'].data_ptr(), scale=aff[0].data_ptr(),
                                      shift=aff[1].data_ptr(), mean=aff[2].data_ptr(), rstd=aff[3].data_ptr(), M=rows, N=F, eps=EPS,
                                      momentum=MOM, num_batches_tracked=O['nbt'].data_ptr(), bwd_sums=O['bwd_sums'].data_ptr())], DEV)
        _ffi.norm_act([_norm_desc(O['Y'], out=O['H'], aff=aff)], DEV)
        _ffi.norm_bwd_reduce([_norm_desc(O['Y'], dy=I['dY'], aff=aff, s12=O['s12'])], DEV)
        d = _norm_desc(O['Y'], dy=I['dY'], out=O['dz'], aff=aff, s12=O['s12'])
        d.acc1, d.acc2 = O['acc'][0].data_ptr(), O['acc'][1].data_ptr()
        _ffi.norm_bwd_apply([d], DEV)
        _ffi.norm_bwd([_norm_desc(O['Y'], dy=I['dY'], out=O['dz2'], aff=aff, s12=O['t12'])], DEV, accumulate=False)
        _ffi.norm_bwd([_norm_desc(O['Y'], dy=I['dY'], out=O['dz2'], aff=aff, s12=O['u12'])], DEV, accumulate=True)

    for live in LIVES:
        _, O = _launch(live, {'X': X, 'dY': dY}, outs, run)
        what = f'batchnorm F={F} live={live}'
        for name in ('H', 'dz', 'dz2'):
            _untouched(O[name], live, f'{what} {name}')
        for name in ('aff', 's12', 'acc', 't12', 'u12', 'rm', 'rv'):
            assert torch.isfinite(O[name]).all(), (what, name)
        assert bool((O['bwd_sums'] == 0).all()), what                    # (cleared for the backward, whatever the count)
        if live == 0:
            assert torch.equal(O['rm'].cpu(), rm0) and torch.equal(O['rv'].cpu(), rv0) and int(O['nbt']) == 5, what
            assert bool((O['s12'] == 0).all()) and bool((O['acc'] == 0.25).all()) and bool((O['u12'] == 2.5).all()), what
            assert bool((O['t12'] == 0).all()), what
            continue
        z = O['Y'][:live].cpu()
        h, dz, dgamma, dbeta, rm, rv, mean, var = _bn_reference(z, gamma, beta, dY[:live], rm0, rv0)
        gate(O['aff'][2], mean, what + ' mean')
        gate(O['aff'][3], 1.0 / torch.sqrt(var + EPS), what + ' rstd')
        gate(O['rm'], rm, what + ' running_mean')
        gate(O['rv'], rv, what + ' running_var')
        assert int(O['nbt']) == 6, what
        if live == 1:
            _one_row_out(O['H'][:1], z, O['aff'], what + ' out')
        else:
            gate(O['H'][:live], h, what + ' out')
        gate(O['s12'][0], dbeta, what + ' s1')
        gate(O['s12'][1], dgamma, what + ' s2')
        gate(O['acc'], torch.stack([dbeta, dgamma]) + 0.25, what + ' acc1 / acc2')
        gate(O['dz'][:live], dz, what + ' dz (reduce + apply)')
        gate(O['t12'], torch.stack([dbeta, dgamma]), what + ' s1 / s2 (one launch)')
        gate(O['u12'], torch.stack([dbeta, dgamma]) + 2.5, what + ' s1 / s2 (one launch, accumulate)')
        gate(O['dz2'][:live], dz, what + ' dz (one launch)')
        # row-wise: the activation is the M = live call's, bit for bit (the statistics are band sums in band order in both)
        souts = dict(outs, cs=torch.full((ops.stat_rows(live), F), SENT, dtype=torch.float64),
                     cq=torch.full((ops.stat_rows(live), F), SENT, dtype=torch.float64))
        _, S = _launch(live, {'X': X, 'dY': dY}, souts, run, dynamic=False)
        assert torch.equal(O['H'][:live], S['H']) and torch.equal(O['aff'], S['aff']), what


@pytest.mark.parametrize('F', [64, 128])
def test_stage_statistics_in_slots_device_side_row_count(F):
    """cwn_stage_desc.stat_slots + cwn_bn_live: the statistics of Y as slot sums, the affine derived by the consumer
    (cwn_norm_act_f32 with cwn_norm_desc.bn) -- sums over the live rows only, divided by *m_dev, the running statistics and the
    batch counter updated once, and left alone at a count of 0.  Live counts: LIVES (the activation of a ONE-row batch: _one_row_out)."""
    g = torch.Generator().manual_seed(11 * F)
    W = _stage_weight(g, F, 2)
    bias = (_rand(g, F) * 2).to(DEV)
    pro = [(torch.rand(F, generator=g) + 0.5).to(DEV) if k % 2 == 0 else _rand(g, F).to(DEV) for k in range(4)]
    gamma, beta = torch.rand(F, generator=g) + 0.5, _rand(g, F)
    rm0, rv0 = _rand(g, F), torch.rand(F, generator=g) + 0.5
    gd, bd = gamma.to(DEV), beta.to(DEV)
    ins = {'X': _rand(g, CAP, F), 'X2': _rand(g, CAP, F)}
    outs = {'Y': (F,), 'H': (F,), 'slots': torch.zeros(_ffi.BN_SLOTS, 2, F, dtype=torch.float64), 'aff': torch.full((4, F), SENT),
            'rm': rm0, 'rv': rv0, 'nbt': torch.full((1,), 5, dtype=torch.int64)}

    def run(I, O):
        from cwn_amd.dense_train import _norm_desc
        _stage_launch(I, O, W, F, bias, pro, stat_slots=O['slots'])
        d = _norm_desc(O['Y'], out=O['H'], aff=None)
        d.bn = _ffi.BnLive(slots=O['slots'].data_ptr(), gamma=gd.data_ptr(), beta=bd.data_ptr(), running_mean=O['rm'].data_ptr(),
                           running_var=O['rv'].data_ptr(), num_batches_tracked=O['nbt'].data_ptr(), aff=O['aff'].data_ptr(),
                           eps=EPS, momentum=MOM)
        _ffi.norm_act([d], DEV)

    for live in LIVES:
        _, O = _launch(live, ins, outs, run)
        what = f'stage slots F={F} live={live}'
        _untouched(O['Y'], live, what + ' Y')
        _untouched(O['H'], live, what + ' H')
        assert torch.isfinite(O['slots']).all() and torch.isfinite(O['rm']).all() and torch.isfinite(O['rv']).all(), what
        if live == 0:
            assert bool((O['slots'] == 0).all()), what
            assert torch.equal(O['rm'].cpu(), rm0) and torch.equal(O['rv'].cpu(), rv0) and int(O['nbt']) == 5, what
            continue
        z = O['Y'][:live].cpu()
        gate(O['slots'].sum(0), torch.stack([z.double().sum(0), (z.double() ** 2).sum(0)]), what + ' slot sums')
        h, _, _, _, rm, rv, mean, var = _bn_reference(z, gamma, beta, torch.zeros(live, F), rm0, rv0)
        gate(O['aff'][2], mean, what + ' mean')
        gate(O['aff'][3], 1.0 / torch.sqrt(var + EPS), what + ' rstd')
        if live == 1:
            _one_row_out(O['H'][:1], z, O['aff'], what + ' out')
        else:
            gate(O['H'][:live], h, what + ' out')
        gate(O['rm'], rm, what + ' running_mean')
        gate(O['rv'], rv, what + ' running_var')
        assert int(O['nbt']) == 6, what


@pytest.mark.parametrize('F', [64, 128])
@pytest.mark.parametrize('wide', [False, True])
def test_dense_stage_backward_device_side_row_count(F, wide):
    """cwn_dense_stage_bwd_f32 (csrc/cwn_stage.hip): m_dev = "actual rows (M = capacity)" -- dz = scale * (dyh - s1 / M - xhat *
    s2 / M) with M the COUNT, dz and dX (dX2) of the live rows only, s1 / s2 handed on to acc1 / acc2 once; against the autograd of
    BatchNorm1d(train) + ReLU + Linear in float64 on the live rows.  Live counts: LIVES."""
    g = torch.Generator().manual_seed(13 * F + wide)
    W = _stage_weight(g, F, 2 if wide else 1)
    Wc = W.detach().cpu().double()
    gamma, beta = torch.rand(F, generator=g) + 0.5, _rand(g, F)
    ins = {'dy': _rand(g, CAP, F), 'z': _rand(g, CAP, F) * 2 + 0.5}
    outs = {'dz': (F,), 'dx': (F,), 'dx2': (F,), 'acc': torch.full((2, F), 0.25)}

    for live in LIVES:
        what = f'stage bwd F={F} wide={wide} live={live}'
        if live:
            _, dz, dgamma, dbeta, _, _, mean, var = _bn_reference(ins['z'][:live], gamma, beta, ins['dy'][:live], torch.zeros(F), torch.ones(F))
        else:
            dz, dgamma, dbeta, mean, var = torch.zeros(0, F).double(), torch.zeros(F), torch.zeros(F), torch.zeros(F), torch.zeros(F)
        rstd = 1.0 / torch.sqrt(var.double() + EPS)
        scale = gamma.double() * rstd
        aff = torch.stack([scale, beta.double() - mean.double() * scale, mean.double(), rstd]).float().to(DEV)
        s12 = torch.stack([dbeta, dgamma]).float().to(DEV)

        def run(I, O):
            rows = I['dy'].size(0)
            d = _ffi.StageBwdDesc(dy=I['dy'].data_ptr(), z=I['z'].data_ptr(), dz=O['dz'].data_ptr(), scale=aff[0].data_ptr(),
                                  shift=aff[1].data_ptr(), mean=aff[2].data_ptr(), rstd=aff[3].data_ptr(), s1=s12[0].data_ptr(),
                                  s2=s12[1].data_ptr(), acc1=O['acc'][0].data_ptr(), acc2=O['acc'][1].data_ptr(),
                                  wt_packed=ops.packed_stage_block(W, 0, transposed=True).data_ptr(),
                                  wt2_packed=ops.packed_stage_block(W, F, transposed=True).data_ptr() if wide else None,
                                  dx=O['dx'].data_ptr(), dx2=O['dx2'].data_ptr() if wide else None, M=rows, lddy=F, ldz=F, lddz=F,
                                  lddx=F, lddx2=F if wide else 0, relu=1, m_dev=_ffi.dyn(rows))
            _ffi.check(_ffi.lib().cwn_dense_stage_bwd_f32((_ffi.StageBwdDesc * 1)(d), 1, F, _stream()), 'cwn_dense_stage_bwd_f32')

        _, O = _launch(live, ins, outs, run)
        for name in ('dz', 'dx', 'dx2'):
            _untouched(O[name], live if (wide or name != 'dx2') else 0, f'{what} {name}')
        gate(O['acc'], torch.stack([dbeta, dgamma]).double() + 0.25, what + ' acc1 / acc2')
        if live == 0:
            assert bool((O['acc'] == 0.25).all()), what
            continue
        # (the reference of the row outputs: the formula on the fp32 constants the kernel was handed)
        gate(O['dz'][:live], dz, what + ' dz')
        dx = dz @ Wc
        gate(O['dx'][:live], dx[:, :F], what + ' dx')
        if wide:
            gate(O['dx2'][:live], dx[:, F:], what + ' dx2')
        _, S = _launch(live, ins, outs, run, dynamic=False)
        assert torch.equal(O['dz'][:live], S['dz']) and torch.equal(O['dx'][:live], S['dx']), what
        assert not wide or torch.equal(O['dx2'][:live], S['dx2']), what


# ------------------------------------------------------------------------------------------------------------------------------
# 5. cwn_update_mlp_f32 / cwn_update_mlp3_f32 (inference)
# ------------------------------------------------------------------------------------------------------------------------------
def _mlp_net(g, F, w_in, branches):
    """Linear layers + folded-norm (scale, shift) pairs in the launch's stage order: per branch Linear(w_in -> F), Linear(F -> F),
    then the combine Linear(branches * F -> F)."""
    lins, folds = [], []
    shapes = [(F, w_in), (F, F)] * branches + [(F, branches * F)]
    for k, (o, i) in enumerate(shapes):
        lin = torch.nn.Linear(i, o)
        with torch.no_grad():
            lin.weight.copy_(_rand(g, o, i) / i ** 0.5)
            lin.bias.copy_(_rand(g, o) * 0.5)
        lins.append(lin.to(DEV))
        folds.append((None, None) if k == 1 else ((torch.rand(o, generator=g) + 0.5).to(DEV), (_rand(g, o) * 0.3).to(DEV)))
    return lins, folds


def _mlp_ref(xs, lins, folds, live):
    def stage(k, x):
        y = x @ lins[k].weight.detach().cpu().double().t() + lins[k].bias.detach().cpu().double()
        if folds[k][0] is not None:
            y = y * folds[k][0].cpu().double() + folds[k][1].cpu().double()
        return y.relu()
    hs = [stage(2 * b + 1, stage(2 * b, x[:live].double())) for b, x in enumerate(xs)]
    return stage(len(lins) - 1, torch.cat(hs, 1))


@pytest.mark.parametrize('F', [64, 128])
@pytest.mark.parametrize('w_in', [None, 20])
def test_update_mlp_device_side_row_count(F, w_in):
    """cwn_update_mlp_f32 (csrc/cwn_mlp.hip): cwn_mlp_dim.m_dev = "actual rows (M = capacity)" -- y of the live rows through all
    five Linear layers, the rows beyond left as they were; F-wide inputs and narrow ones (in_width = 20: the rows are staged
    element-wise and zero-padded).  Live counts: LIVES."""
    g = torch.Generator().manual_seed(3 * F + (w_in or 0))
    wi = w_in or F
    lins, folds = _mlp_net(g, F, wi, 2)
    ins = {'xu': _rand(g, CAP, wi) * 2, 'xb': _rand(g, CAP, wi) * 2}
    packed = []
    for k, l in enumerate(lins[:4]):
        packed += list(ops.pack_mlp_weight(ops._mlp_first_weight(l.weight, F) if k in (0, 2) else l.weight))
    packed += list(ops.pack_mlp_weight(lins[4].weight))

    def run(I, O):
        rows = I['xu'].size(0)
        arr = (_ffi.MlpDim * 1)()
        a = arr[0]
        a.x_up, a.x_b, a.y, a.M = I['xu'].data_ptr(), I['xb'].data_ptr(), O['y'].data_ptr(), rows
        a.ldx_up = a.ldx_b = wi
        a.ldy, a.in_width, a.m_dev = F, (wi if wi < F else 0), _ffi.dyn(rows)
        for k, pk in enumerate(packed):
            a.w_packed[k] = pk.data_ptr()
        for k, (lin, (sc, sh)) in enumerate(zip(lins, folds)):
            a.bias[k], a.scale[k], a.shift[k] = lin.bias.data_ptr(), _ffi.ptr(sc), _ffi.ptr(sh)
        _ffi.check(_ffi.lib().cwn_update_mlp_f32(arr, 1, F, _stream()), 'cwn_update_mlp_f32')

    for live in LIVES:
        _, O = _launch(live, ins, {'y': (F,)}, run)
        what = f'update_mlp F={F} w_in={w_in} live={live}'
        gate(O['y'][:live], _mlp_ref([ins['xu'], ins['xb']], lins, folds, live), what)
        _untouched(O['y'], live, what)
        if live:
            _, S = _launch(live, ins, {'y': (F,)}, run, dynamic=False)
            assert torch.equal(O['y'][:live], S['y']), what


@pytest.mark.parametrize('F', [64, 128])
def test_update_mlp3_device_side_row_count(F):
    """cwn_update_mlp3_f32 (csrc/cwn_mlp3.hip): cwn_mlp3_dim.m_dev = "actual rows (M = capacity)" -- the three update networks
    and the 3F-wide combine of a CIN++ layer on the live rows only.  Live counts: LIVES."""
    g = torch.Generator().manual_seed(5 * F)
    lins, folds = _mlp_net(g, F, F, 3)
    ins = {f'x{k}': _rand(g, CAP, F) * 2 for k in range(3)}
    wc = ops.pack_mlp_weight(lins[6].weight)
    packed = []
    for k in range(3):
        packed += [ops.pack_mlp_weight(lins[2 * k].weight)[0], ops.pack_mlp_weight(lins[2 * k + 1].weight)[0], wc[k]]

    def run(I, O):
        rows = I['x0'].size(0)
        arr = (_ffi.Mlp3Dim * 1)()
        a = arr[0]
        for k in range(3):
            a.x[k], a.ldx[k] = I[f'x{k}'].data_ptr(), F
        a.y, a.M, a.ldy, a.m_dev = O['y'].data_ptr(), rows, F, _ffi.dyn(rows)
        for k, pk in enumerate(packed):
            a.w_packed[k] = pk.data_ptr()
        for k, (lin, (sc, sh)) in enumerate(zip(lins, folds)):
            a.bias[k], a.scale[k], a.shift[k] = lin.bias.data_ptr(), _ffi.ptr(sc), _ffi.ptr(sh)
        _ffi.check(_ffi.lib().cwn_update_mlp3_f32(arr, 1, F, _stream()), 'cwn_update_mlp3_f32')

    for live in LIVES:
        _, O = _launch(live, ins, {'y': (F,)}, run)
        what = f'update_mlp3 F={F} live={live}'
        gate(O['y'][:live], _mlp_ref([ins['x0'], ins['x1'], ins['x2']], lins, folds, live), what)
        _untouched(O['y'], live, what)
        if live:
            _, S = _launch(live, ins, {'y': (F,)}, run, dynamic=False)
            assert torch.equal(O['y'][:live], S['y']), what


# ------------------------------------------------------------------------------------------------------------------------------
# 6. cwn_aggregate_f32 (+ cwn_csr_long_rows)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [3, 16, 64, 130])
def test_aggregate_f32_device_side_row_count(F):
    """cwn_aggregate_f32 (csrc/cwn_aggregate.hip), the f32 mirror of test_gpu_f64.py: cwn_agg_desc.m_dev = "the ACTUAL number of
    destination rows (n_dst is then the capacity)" -- add / mean / max with both self terms ((1 + eps) x + (1 + eps2) x2, NaN in their
    padding rows), over a plan with one row longer than CWN_LONG_ROW (row 40) whose long-row list cwn_csr_long_rows rewrites
    under the same count ("rows r < *m_dev ... go to sub-list 0"): the hub row is walked by the whole-workgroup pass when it
    exists and left alone when it does not.  Integer-valued features: every sum is exact, so equality is the bar.
    Live counts: LIVES."""
    from cwn_amd.csr import Adjacency, check_errors
    n_src = 57
    g = torch.Generator().manual_seed(F)
    lens = [int(v) for v in torch.randint(0, 7, (CAP,), generator=g)]
    lens[40], lens[0], lens[199] = 70, 0, 5
    dst = torch.repeat_interleave(torch.arange(CAP), torch.tensor(lens))
    dst = dst[torch.randperm(dst.numel(), generator=g)]
    src = torch.randint(0, n_src, (dst.numel(),), generator=g)
    adj = Adjacency.from_index(torch.stack([src, dst]).to(DEV), CAP, n_src)
    assert adj.long_row_list().tolist() == [40]
    A = torch.randint(-8, 9, (n_src, F), generator=g).float()
    sx, sx2 = torch.randint(-3, 4, (CAP, F), generator=g).float(), torch.randint(-3, 4, (CAP, F), generator=g).float()
    Ad, eps = A.to(DEV), torch.tensor([0.25], device=DEV)
    m = A[src].double()
    cnt = torch.zeros(CAP, dtype=torch.float64).index_add_(0, dst, torch.ones(dst.numel(), dtype=torch.float64))
    add = torch.zeros(CAP, F, dtype=torch.float64).index_add_(0, dst, m)
    mx = torch.full((CAP, F), float('-inf'), dtype=torch.float64).scatter_reduce(0, dst[:, None].expand(-1, F), m, 'amax')
    want = {'add': add, 'mean': add / cnt.clamp(min=1)[:, None], 'max': torch.where(cnt[:, None] > 0, mx, torch.zeros_like(mx))}
    for red in ('add', 'mean', 'max'):
        def run(I, O):
            rows = I['sx'].size(0)
            lr = _ffi.LongRowsDesc(rowptr=adj.rowptr.data_ptr(), n_rows=CAP, m_dev=_ffi.dyn(rows), long_rows=adj.long_rows.data_ptr(),
                                   n_long=adj.n_long.data_ptr(), long_cap=adj.long_cap)
            _ffi.check(_ffi.lib().cwn_csr_long_rows((_ffi.LongRowsDesc * 1)(lr), 1, _stream()), 'cwn_csr_long_rows')
            spec = ops.AggSpec(adj=adj, n_dst=CAP, F=F, A=Ad, ia=adj.col, reduce=_ffi.REDUCE[red], self_x=I['sx'], eps=eps, self_x2=I['sx2'],
                               eps2=eps, out=O['out'])
            ops.run_aggregate([spec], DEV)

        for live in LIVES:
            _, O = _launch(live, {'sx': sx, 'sx2': sx2}, {'out': (F,)}, run)
            what = f'aggregate F={F} {red} live={live}'
            assert int(adj.n_long[0]) == (1 if live > 40 else 0), what
            ref = (want[red] + 1.25 * sx.double() + 1.25 * sx2.double())[:live]
            gate(O['out'][:live], ref, what)
            if red != 'mean':
                assert torch.equal(O['out'][:live].cpu().double(), ref), what
            _untouched(O['out'], live, what)
    check_errors(DEV)


# ------------------------------------------------------------------------------------------------------------------------------
# 7. cwn_dropout_f32
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [64, 7])
def test_dropout_device_side_row_count(N):
    """cwn_dropout_f32 (csrc/cwn_norm.hip): "m_dev (or NULL): the rows that exist (M = capacity)" -- the 16-byte form (N = 64) and
    the element-wise one (N = 7).  The multiplier of element e = row * N + column is a function of (seed, step, site, e), not
    of the capacity: the live rows are the M = live call's bit for bit, and tests/_philox_ref's multipliers times x.
    Live counts: LIVES."""
    from tests._philox_ref import multipliers
    g = torch.Generator().manual_seed(N)
    x = _rand(g, CAP, N)
    seed, step, site, p = 1234567, 3, 5, 0.5
    state = torch.tensor([seed, step], dtype=torch.int64, device=DEV)
    rec = _ffi.Dropout(state=state.data_ptr(), p=p, site=site)
    mult = torch.as_tensor(multipliers((CAP, N), p, seed, step, site)).reshape(CAP, N).double()

    def run(I, O):
        rows = I['x'].size(0)
        _ffi.check(_ffi.lib().cwn_dropout_f32(I['x'].data_ptr(), O['out'].data_ptr(), rows, N, N, N, C.byref(rec), _ffi.dyn(rows),
                                              _stream()), 'cwn_dropout_f32')

    for live in LIVES:
        _, O = _launch(live, {'x': x}, {'out': (N,)}, run)
        what = f'dropout N={N} live={live}'
        gate(O['out'][:live], x[:live].double() * mult[:live], what)
        _untouched(O['out'], live, what)
        if live:
            _, S = _launch(live, {'x': x}, {'out': (N,)}, run, dynamic=False)
            assert torch.equal(O['out'][:live], S['out']), what


# ------------------------------------------------------------------------------------------------------------------------------
# 8. cwn_loss_f32
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', [0, 1, 2])
def test_loss_device_side_element_count(kind):
    """cwn_loss_f32, L1 / MSE / BCE-with-logits: "n_dev: the ACTUAL number of elements (n is then the capacity: grad[i] = 0 for
    i >= *n_dev)"; "a target that is NaN is a NULL label: it contributes no loss and no gradient and does not count in the mean"
    -- a NaN target among the live elements (index 5), NaN predictions and targets in the padding; the mean of nothing (a count
    of 0) is NaN, its gradient zero.  Live counts: LIVES."""
    g = torch.Generator().manual_seed(kind)
    pred = _rand(g, CAP) * 2
    y = (torch.rand(CAP, generator=g) > 0.5).float() if kind == 2 else _rand(g, CAP)
    y[5] = NAN
    crit = [torch.nn.L1Loss(), torch.nn.MSELoss(), torch.nn.BCEWithLogitsLoss()][kind]

    def run(I, O):
        n = I['pred'].size(0)
        _ffi.check(_ffi.lib().cwn_loss_f32(kind, I['pred'].data_ptr(), I['y'].data_ptr(), n, O['loss'].data_ptr(), O['grad'].data_ptr(),
                                           _ffi.dyn(n), _stream()), 'cwn_loss_f32')

    for live in LIVES:
        _, O = _launch(live, {'pred': pred, 'y': y}, {'loss': torch.full((1,), SENT), 'grad': ()}, run)
        what = f'loss kind={kind} live={live}'
        assert bool((O['grad'][live:] == 0).all()), what              # (the documented exception to "never written")
        if live == 0:
            assert torch.isnan(O['loss']).all(), what
            continue
        keep = ~torch.isnan(y[:live])
        p64 = pred[:live][keep].double().requires_grad_(True)
        ref = crit(p64, y[:live][keep].double())
        ref.backward()
        gref = torch.zeros(live, dtype=torch.float64)
        gref[keep] = p64.grad
        gate(O['loss'], ref.detach().reshape(1), what + ' loss')
        gate(O['grad'][:live], gref, what + ' grad')


# ------------------------------------------------------------------------------------------------------------------------------
# 9. cwn_embedding_bwd_f32 / cwn_embed_front_f32 / cwn_embed_front_bwd_f32
# ------------------------------------------------------------------------------------------------------------------------------
BAD_INDEX = 10 ** 6            # what the padding rows of an index input hold: far outside every table


@pytest.mark.parametrize('H,sizes,f32', [(64, (28,), False), (128, (9, 5, 4), False), (32, (9, 5, 4), True)])
def test_embedding_backward_device_side_row_count(H, sizes, f32):
    """cwn_embedding_bwd_f32 (csrc/cwn_norm.hip): "n_dev: the actual number of rows (n_rows = capacity)" -- dW takes the live rows
    only; the padding rows hold NaN gradients and an index far outside the table, which is neither looked up nor reported.  The
    banded form (H = 64 / 128, one table and three) and the table-in-LDS form (H = 32), int64 and float32 indices; dW is added to
    (a count of 0 leaves it as it was).  Live counts: LIVES."""
    from cwn_amd.csr import check_errors
    g = torch.Generator().manual_seed(H + len(sizes))
    V, cols = sum(sizes), len(sizes)
    idx = torch.stack([torch.randint(0, s, (CAP,), generator=g) for s in sizes], 1)
    gr = _rand(g, CAP, H)
    off = None if cols == 1 else torch.tensor([sum(sizes[:c]) for c in range(cols)], dtype=torch.int64, device=DEV)
    size = None if cols == 1 else torch.tensor(sizes, dtype=torch.int64, device=DEV)
    src = idx.float() if f32 else idx

    def run(I, O):
        n = I['g'].size(0)
        _ffi.check(_ffi.lib().cwn_embedding_bwd_f32(I['g'].data_ptr(), I['src'].data_ptr(), _ffi.ptr(off), _ffi.ptr(size),
                                                    O['dW'].data_ptr(), n, cols, H, V, int(f32), _ffi.dyn(n), _stream()),
                   'cwn_embedding_bwd_f32')

    for live in LIVES:
        _, O = _launch(live, {'g': gr, 'src': src}, {'dW': torch.full((V, H), 0.5)}, run, pad={'src': BAD_INDEX})
        what = f'embedding bwd H={H} tables={sizes} live={live}'
        ref = torch.full((V, H), 0.5, dtype=torch.float64)
        for c in range(cols):
            ref.index_add_(0, idx[:live, c] + sum(sizes[:c]), gr[:live].double())
        gate(O['dW'], ref, what)
        if live == 0:
            assert bool((O['dW'] == 0.5).all()), what
    check_errors(DEV)


def _prefix_closed_csr(n, fan):
    """A CSR over n rows whose row r lists r // k for k = fan, fan - 1, ... 2 and r itself: every entry of a row below a count
    lies below the count too, as in a collated batch, whatever the count."""
    col = torch.stack([torch.arange(n) // k for k in range(fan, 1, -1)] + [torch.arange(n)], 1).reshape(-1)
    return (torch.arange(n + 1) * fan).to(torch.int32).to(DEV), col.to(torch.int32).to(DEV), col.view(n, fan)


@pytest.mark.parametrize('H', [64, 32])
def test_embed_front_device_side_cell_counts(H):
    """cwn_embed_front_f32 (csrc/cwn_ends.hip): "n_dev: device int64 [3] = the ACTUAL n0, n1, n2 (the arguments are then
    capacities)" -- x0 / x1 / x2 of the cells that exist, the rows beyond left as they were; the padding rows of the vertex and
    edge features hold an index far outside their table, which is neither looked up nor raises the error word.  All three
    counts sweep LIVES together (capacity 200 each)."""
    from cwn_amd.csr import _err_flag, check_errors
    g = torch.Generator().manual_seed(H)
    Vv, Ve = 28, 4
    Wv, We = _rand(g, Vv, H), _rand(g, Ve, H)
    Wvd, Wed = Wv.to(DEV), We.to(DEV)
    ids0, ids1 = torch.randint(0, Vv, (CAP, 1), generator=g), torch.randint(0, Ve, (CAP, 1), generator=g)
    rp1, c1, b1 = _prefix_closed_csr(CAP, 2)            # an edge's two boundary vertices
    rp2, c2, b2 = _prefix_closed_csr(CAP, 3)            # a ring's three boundary edges
    check_errors(DEV)

    def run(I, O):
        n = I['ids0'].size(0)
        tv = _ffi.EmbedTable(W=Wvd.data_ptr(), src=I['ids0'].data_ptr(), col_off=None, col_size=None, V=Vv, cols=1, src_is_f32=0)
        te = _ffi.EmbedTable(W=Wed.data_ptr(), src=I['ids1'].data_ptr(), col_off=None, col_size=None, V=Ve, cols=1, src_is_f32=0)
        counts = _COUNT['n'].data_ptr() if _ffi.dyn(n) is not None else None
        _ffi.check(_ffi.lib().cwn_embed_front_f32(C.byref(tv), n, O['x0'].data_ptr(), C.byref(te), n, O['x1'].data_ptr(), rp1.data_ptr(),
                                                  c1.data_ptr(), 2 * n, n, O['x2'].data_ptr(), rp2.data_ptr(), c2.data_ptr(), 3 * n, H, 1,
                                                  _err_flag(DEV).data_ptr(), counts, _stream()), 'cwn_embed_front_f32')

    for live in LIVES:
        outs = {'x0': (H,), 'x1': (H,), 'x2': (H,)}
        _, O = _launch(live, {'ids0': ids0, 'ids1': ids1}, outs, run, pad={'ids0': BAD_INDEX, 'ids1': BAD_INDEX})
        what = f'embed front H={H} live={live}'
        x0 = Wv.double()[ids0[:live, 0]]
        red1 = x0[b1[:live].long()].sum(1) if live else x0
        x2 = 0.5 * red1[b2[:live].long()].sum(1) if live else x0
        gate(O['x0'][:live], x0, what + ' x0')
        gate(O['x1'][:live], We.double()[ids1[:live, 0]], what + ' x1')
        gate(O['x2'][:live], x2, what + ' x2')
        for name in outs:
            _untouched(O[name], live, f'{what} {name}')
        if live:
            _, S = _launch(live, {'ids0': ids0, 'ids1': ids1}, outs, run, dynamic=False)
            assert all(torch.equal(O[k][:live], S[k]) for k in outs), what
    check_errors(DEV)                                   # no out-of-range index was looked up


@pytest.mark.parametrize('H', [64, 128])
@pytest.mark.parametrize('edge_table', [True, False])
def test_embed_front_backward_device_side_cell_counts(H, edge_table):
    """cwn_embed_front_bwd_f32 (csrc/cwn_ends.hip): cwn_front_bwd.n0_dev / n1_dev = "actual rows" -- dWv / dWe take the vertices /
    edges that exist only (their gradients NaN and their features far outside the tables in the padding rows); with and
    without an edge table (g1 then flows into the vertices); the tables are added to (a count of 0 leaves them as they
    were).  Both counts sweep LIVES together."""
    g = torch.Generator().manual_seed(H + edge_table)
    Vv, Ve = 28, 4
    vs, es = torch.randint(0, Vv, (CAP,), generator=g), torch.randint(0, Ve, (CAP,), generator=g)
    rp1, c1, t1 = _prefix_closed_csr(CAP, 2)            # per vertex its edges
    rp2, c2, t2 = _prefix_closed_csr(CAP, 3)            # per edge its rings
    ins = {'g0': _rand(g, CAP, H), 'g1': _rand(g, CAP, H), 'g2': _rand(g, CAP, H), 'vs': vs, 'es': es}
    outs = {'dWv': torch.full((Vv, H), 0.5), 'dWe': torch.full((Ve, H), 0.5)}

    def run(I, O):
        n = I['g0'].size(0)
        a = _ffi.FrontBwd(g0=I['g0'].data_ptr(), g1=I['g1'].data_ptr(), g2=I['g2'].data_ptr(), rowptr1=rp1.data_ptr(), col1=c1.data_ptr(),
                          rowptr2=rp2.data_ptr(), col2=c2.data_ptr(), v_src=I['vs'].data_ptr(), e_src=I['es'].data_ptr() if edge_table else None,
                          dWv=O['dWv'].data_ptr(), dWe=O['dWe'].data_ptr() if edge_table else None, n0=n, n1=n, n0_dev=_ffi.dyn(n),
                          n1_dev=_ffi.dyn(n), H=H, Vv=Vv, Ve=Ve if edge_table else 0, src_f32=0, halve=1)
        _ffi.check(_ffi.lib().cwn_embed_front_bwd_f32(C.byref(a), _stream()), 'cwn_embed_front_bwd_f32')

    for live in LIVES:
        _, O = _launch(live, ins, outs, run, pad={'vs': BAD_INDEX, 'es': BAD_INDEX})
        what = f'embed front bwd H={H} edge_table={edge_table} live={live}'
        g0, g1, g2 = (ins[k][:live].double() for k in ('g0', 'g1', 'g2'))
        te = 0.5 * g2[t2[:live].long()].sum(1) if live else g0
        if not edge_table:
            te = te + g1
        dv = g0 + te[t1[:live].long()].sum(1) if live else g0
        gate(O['dWv'], torch.full((Vv, H), 0.5, dtype=torch.float64).index_add_(0, vs[:live], dv), what + ' dWv')
        if edge_table:
            gate(O['dWe'], torch.full((Ve, H), 0.5, dtype=torch.float64).index_add_(0, es[:live], g1), what + ' dWe')
        else:
            assert bool((O['dWe'] == 0.5).all()), what
        if live == 0:
            assert bool((O['dWv'] == 0.5).all()) and bool((O['dWe'] == 0.5).all()), what
