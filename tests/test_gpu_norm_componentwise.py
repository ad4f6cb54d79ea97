"""The normalisation launches under GRADED columns, held entry by entry (tests/_bounds.py, tests/_norm_cases.py;
tests/test_bounds_host.py proves on the CPU that these checks can fail).

The componentwise gate of tests/test_gpu_componentwise.py stops at the dense products.  Here the batch statistics and
everything that divides by them get it: z has column spreads 2^((11n mod 25) - 12) and column means 2^(5n mod 13) = 1 ... 4096
spreads (negative in every third column), gamma in [0.5, 1.5), beta ~ randn, dy ~ randn with columns graded like z's, and
  (R) |got - v| <= 2 * 2^-24 * c against the Tracked float64 reference, sums bounded order-free (rows * sum |v|);
  (E) the same ratio with one step per sum, within MARGIN = 8 x that of float32 torch on the CPU (F.batch_norm(training=True),
      F.layer_norm, float32 autograd) on the same operands;
  (equivariance) where every sum has a fixed order: the backward is linear in dy (bits of the ungraded launch times the
      grades), and with eps = 0 train-mode BatchNorm does not see a power-of-two grade of a column of z.
An entry whose ReLU sign float32 and float64 may dispute (|y| <= 4 * 2^-24 * c) keeps its forward gate; its incoming gradient
is zero, and every case asserts that such entries are at most 1% of the matrix.  At M = 1 a third qualify: that backward runs
without ReLU.  Every launch is a C entry point called directly, or asserted through the `ops` wrapper's own refusal
(ops.run_stage / run_stage_bwd return None / False instead of falling back), so nothing passes on torch.
Rows: tests/_windows.ROWS + 300 (several 64-row bands per workgroup chain; more 32-row stage tiles than CWN_BN_SLOTS), and the
smallest count that reaches a further path (4100: the second trip of bn_finalize_kernel's band loop; 600 and 4096:
norm_bwd_fused_kernel with two rows per thread and at its limit).  Section 8 runs a whole dense_train plan and holds every stage
from what the plan itself stored and handed on, since a Tracked chain across several BatchNorms bounds nothing."""
import math

import pytest
import torch

from cwn_amd import _ffi, ops
from cwn_amd.dense_train import _norm_desc
from tests import _bounds as B
from tests import _norm_cases as NC
from tests._windows import ROWS

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
MS = ROWS + (300,)
NAN = float('nan')
SENT = -9.0


def _form(what, form):
    print(f'[cw] {what}: served by {form}')


def _capped(c):
    assert c.share() <= NC.DISPUTED_CAP, f'{c.what}: more than 1% of the ReLU signs are disputed'


# ------------------------------------------------------------------------------------------------------------------------------
# 1. band statistics of cwn_gemm_f32 (col_stats), cwn_linear_stats_f32 and cwn_dense_stage_f32 (bands and slots)
# ------------------------------------------------------------------------------------------------------------------------------
def _exact_sums(y, band):
    """[2, bands, N] float64: the correctly rounded sums of y and y^2 over bands of `band` rows (math.fsum; a float32 squared is
    exact in float64)."""
    y = y.detach().cpu().double()
    M, N = y.shape
    nb = (M + band - 1) // band
    out = torch.zeros(2, nb, N, dtype=torch.float64)
    cols = y.t().tolist()
    for n, col in enumerate(cols):
        for b in range(nb):
            part = col[b * band:(b + 1) * band]
            out[0, b, n] = math.fsum(part)
            out[1, b, n] = math.fsum(v * v for v in part)
    return out


def _hold_sums(got, y, band, what):
    """|delta| <= band * 2^-53 * sum |y| (sum y^2) against the float64 sums of the Y the same launch stored."""
    ref = _exact_sums(y, band)
    rows = min(band, y.size(0))
    for k, name in enumerate(('sum', 'sum of squares')):
        r = B.ratio(got[k], B.Tracked(ref[k], ref[k].abs() if k else _exact_sums(y.abs(), band)[0]), f'{what} {name}', unit=rows * B.UNIT64)
        assert r <= 1.0, f'{what} {name}: {r:.3g} of {rows} * 2^-53 * sum |terms|'


def _stat_operands(g, M, K, N, rows):
    """X ~ randn / sqrt(K) (rows graded in the second variant), weight rows graded by grade_cols, bias = +-grade_ratio * grade_cols."""
    X = torch.randn(M, K, generator=g) / K ** 0.5
    if rows:
        X = X * B.grade_rows(M)[:, None]
    W = torch.randn(N, K, generator=g) * B.grade_cols(N)[:, None]
    return X, W, B.grade_ratio(N) * B.grade_cols(N)


@pytest.mark.parametrize('rows', [False, True], ids=['cols', 'rows'])
@pytest.mark.parametrize('K,N', [(64, 64), (128, 128), (24, 100), (13, 30)])
def test_gemm_band_statistics(K, N, rows):
    """cwn_gemm_f32 with col_stats and cwn_linear_stats_f32 on the same descriptor: one float64 partial per 32-row band."""
    g = torch.Generator().manual_seed(K * N + rows)
    for M in MS:
        X, W, b = _stat_operands(g, M, K, N, rows)
        for mine in (False, True):
            Y = torch.full((M, N), SENT, device=DEV)
            cs = torch.full((2, ops.stat_rows(M), N), SENT, dtype=torch.float64, device=DEV)
            gm = ops.Gemm(X=X.to(DEV), W=W.to(DEV), bias=b.to(DEV), col_stats=cs, out=Y, exact=True)
            what = f'{"linear_stats" if mine else "gemm"} statistics K={K} N={N} M={M}{" rows" if rows else ""}'
            if mine:
                _ffi.linear_stats([gm.desc(Y)], DEV)
                _form(what, 'cwn_linear_stats_f32 (called directly)')
            else:
                assert not ops.gemm_uses_split([gm], DEV)
                ops.run_gemm([gm], DEV)
                _form(what, 'cwn_gemm_f32, the exact kernel (ops.run_gemm has no other route)')
            _hold_sums(cs, Y, 32, what)


@pytest.mark.parametrize('K,N', [(48, 48), (37, 100)])
def test_linear_stats_bands_behind_the_count_are_untouched(K, N):
    g = torch.Generator().manual_seed(K + N)
    for M in MS:
        cap = M + 70
        X, W, b = _stat_operands(g, cap, K, N, False)
        X[M:] = NAN
        Y = torch.full((cap, N), SENT, device=DEV)
        cs = torch.full((2, ops.stat_rows(cap), N), SENT, dtype=torch.float64, device=DEV)
        count = torch.tensor([M], dtype=torch.int64, device=DEV)
        with _ffi.dynamic_rows({cap: count.data_ptr()}):
            res = ops.run_linear_stats([ops.Gemm(X=X.to(DEV), W=W.to(DEV), bias=b.to(DEV), col_stats=cs, out=Y)], DEV)
        assert res is not None, 'cwn_linear_stats_f32 refused a launch it is written for'
        nb = ops.stat_rows(M)
        what = f'linear_stats under a count K={K} N={N} M={M} of {cap}'
        assert bool((cs[:, nb:] == SENT).all()) and bool((Y[M:] == SENT).all()), what
        _hold_sums(cs[:, :nb], Y[:M], 32, what)


def _stage_weight(g, F, blocks=1, grade=True):
    W = torch.randn(F, blocks * F, generator=g) / (blocks * F) ** 0.5
    if grade:
        W = W * B.grade_cols(F)[:, None]
    P = torch.nn.Parameter(W.to(DEV))
    ops.pack_stage_weights_many([P])
    return P, W


@pytest.mark.parametrize('rows', [False, True], ids=['cols', 'rows'])
@pytest.mark.parametrize('F', [64, 128])
def test_stage_band_and_slot_statistics(F, rows):
    """cwn_dense_stage_f32: col_sum / col_sumsq bands, and the same sums in CWN_BN_SLOTS slots (float64 atomics, no order:
    M * 2^-53 * sum |terms|); the slotted total equals the band total to that bound; under a device-side count the bands behind
    it keep what they held."""
    g = torch.Generator().manual_seed(F + rows)
    for M in MS:
        cap = M + 70
        X, _, b = _stat_operands(g, cap, F, F, rows)
        X = X * F ** 0.5                                     # (the stage's prologue is a ReLU: keep the scale of a Linear's input)
        P, _ = _stage_weight(g, F)
        what = f'stage statistics F={F} M={M}{" rows" if rows else ""}'
        Xd, bd = X[:M].contiguous().to(DEV), b.to(DEV)
        cs = torch.full((2, ops.stat_rows(M), F), SENT, dtype=torch.float64, device=DEV)
        Y, = _run_stage([ops.Gemm(X=Xd, W=P, bias=bd, in_relu=1, col_stats=cs)])
        _form(what, 'cwn_dense_stage_f32 (ops.run_stage took the launch)')
        _hold_sums(cs, Y, 32, what + ' bands')
        slots = torch.zeros(_ffi.BN_SLOTS, 2, F, dtype=torch.float64, device=DEV)
        Y2, = _run_stage([ops.Gemm(X=Xd, W=P, bias=bd, in_relu=1, stat_slots=slots)])
        assert torch.equal(Y2, Y), what + ': Y depends on where the statistics go'
        total = slots.sum(0)
        _hold_sums(total[:, None], Y, M, what + ' slots')
        band_total = cs.sum(1)
        for k, name in enumerate(('sum', 'sum of squares')):
            bound = M * B.UNIT64 * (Y.double().abs() ** (k + 1)).sum(0)
            worst = float(((total[k] - band_total[k]).abs() / bound.clamp(min=1e-300)).max())
            print(f'[cw] {what}: slotted total against band total, {name}: {worst:.3g} of M * 2^-53 * sum |terms|')
            # (slots within M * 2^-53 * sum |terms| of the exact sum, bands within 32 * 2^-53 * sum |terms|: the triangle inequality)
            assert worst <= (M + 32) / M, what
        # a count below the capacity: the bands behind it are untouched
        Xc = X.clone()
        Xc[M:] = NAN
        csc = torch.full((2, ops.stat_rows(cap), F), SENT, dtype=torch.float64, device=DEV)
        count = torch.tensor([M], dtype=torch.int64, device=DEV)
        with _ffi.dynamic_rows({cap: count.data_ptr()}):
            Yc, = _run_stage([ops.Gemm(X=Xc.to(DEV), W=P, bias=bd, in_relu=1, col_stats=csc)])
        nb = ops.stat_rows(M)
        assert bool((csc[:, nb:] == SENT).all()), what + ': a band behind the count was written'
        assert torch.equal(Yc[:M], Y) and torch.equal(csc[:, :nb], cs), what + ': the live bands depend on the count'


def _run_stage(gemms):
    with torch.no_grad():
        got = ops.run_stage(gemms, DEV)
    assert got is not None, 'the stage kernel refused a launch it is written for'
    torch.cuda.synchronize()
    return got


# ------------------------------------------------------------------------------------------------------------------------------
# 2. cwn_bn_finalize_f32     3. cwn_norm_act_f32, with the finalize launch's constants and with a live record
# ------------------------------------------------------------------------------------------------------------------------------
FWD = ('out', 'mean', 'rstd', 'running_mean', 'running_var')


def _finalize(c, z=None, stats=None):
    """cwn_bn_finalize_f32 over `stats` ([2, bands, N] float64 on the device, as a producing launch left them), or over the
    float64 band sums of z (c.z) taken on the host: the affine rows and the running statistics."""
    N = c.N
    stats = c.band_sums(z).to(DEV) if stats is None else stats
    aff = torch.full((4, N), NAN, device=DEV)
    rm, rv, nbt = c.rm0.to(DEV), c.rv0.to(DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    gam, bet = c.gamma.to(DEV), c.beta.to(DEV)
    _ffi.bn_finalize([_ffi.BnDesc(col_sum=stats[0].data_ptr(), col_sumsq=stats[1].data_ptr(), gamma=gam.data_ptr(), beta=bet.data_ptr(),
                                  running_mean=rm.data_ptr(), running_var=rv.data_ptr(), scale=aff[0].data_ptr(), shift=aff[1].data_ptr(),
                                  mean=aff[2].data_ptr(), rstd=aff[3].data_ptr(), M=c.M, N=N, eps=c.eps, momentum=NC.MOM,
                                  num_batches_tracked=nbt.data_ptr())], DEV)
    torch.cuda.synchronize()
    assert int(nbt) == 1
    return dict(aff=aff, scale=aff[0], shift=aff[1], mean=aff[2], rstd=aff[3], running_mean=rm, running_var=rv)


def _slots(z):
    """[BN_SLOTS, 2, N] float64: the sums of z and z^2 as a producing launch leaves them, row chunks in the slots."""
    z = z.double()
    slots = torch.zeros(_ffi.BN_SLOTS, 2, z.size(1), dtype=torch.float64)
    for q, part in enumerate(z.chunk(_ffi.BN_SLOTS) if z.size(0) >= _ffi.BN_SLOTS else [z]):
        slots[q, 0], slots[q, 1] = part.sum(0), (part * part).sum(0)
    return slots


def _live_record(c, z=None):
    N = c.N
    keep = dict(slots=_slots(c.z if z is None else z).to(DEV), gamma=c.gamma.to(DEV), beta=c.beta.to(DEV), running_mean=c.rm0.to(DEV),
                running_var=c.rv0.to(DEV), nbt=torch.zeros(1, dtype=torch.int64, device=DEV), aff=torch.full((4, N), NAN, device=DEV))
    rec = _ffi.BnLive(slots=keep['slots'].data_ptr(), gamma=keep['gamma'].data_ptr(), beta=keep['beta'].data_ptr(),
                      running_mean=keep['running_mean'].data_ptr(), running_var=keep['running_var'].data_ptr(),
                      num_batches_tracked=keep['nbt'].data_ptr(), aff=keep['aff'].data_ptr(), eps=c.eps, momentum=NC.MOM)
    return rec, keep


def _act(c, aff=None, live=None, z=None):
    zd = (c.z if z is None else z).to(DEV)
    H = torch.full((c.M, c.N), NAN, device=DEV)
    d = _norm_desc(zd, out=H, aff=aff, relu=c.relu)
    if live is not None:
        d.bn = live
    _ffi.norm_act([d], DEV)
    torch.cuda.synchronize()
    return H


@pytest.mark.parametrize('rows', [False, True], ids=['cols', 'rows'])
@pytest.mark.parametrize('N', [64, 128, 100, 30])
def test_finalize_and_norm_act(N, rows):
    """cwn_bn_finalize_f32 -> cwn_norm_act_f32, and cwn_norm_act_f32 with a live record on the same sums: mean, rstd, scale,
    shift, the running statistics and out.  4100 rows: the second trip of the finalize kernel's band loop."""
    for M in MS + (4100,):
        c = NC.BnCase(M, N, rows=rows, relu=M > 1)
        if M > 1:
            _capped(c)
        cpu = c.cpu32()
        fin = _finalize(c)
        fin['out'] = _act(c, aff=fin['aff'])
        what = f'finalize + norm_act {c.what}'
        _form(what, 'cwn_bn_finalize_f32 and cwn_norm_act_f32 (called directly)')
        NC.hold(fin, c.fwd, cpu, FWD, what)
        NC.hold(fin, c.fwd, None, ('scale', 'shift'), what)
        if cpu is not None:
            far = B.grade_ratio(N).abs() == 4096
            ref, k, t = c.fwd(B.FMA)['out'].v[:, far], fin['out'].cpu().double()[:, far], cpu['out'].double()[:, far]
            print(f'[cw] {c.what}: out in the columns with |mean| / spread = 4096, max |delta|: kernel against float64 '
                  f'{float((k - ref).abs().max()):.3e}, F.batch_norm float32 against float64 {float((t - ref).abs().max()):.3e}, '
                  f'kernel against F.batch_norm float32 {float((k - t).abs().max()):.3e}')
        rec, keep = _live_record(c)
        liv = dict(out=_act(c, live=rec), scale=keep['aff'][0], shift=keep['aff'][1], mean=keep['aff'][2], rstd=keep['aff'][3],
                   running_mean=keep['running_mean'], running_var=keep['running_var'])
        assert int(keep['nbt']) == 1
        what = f'live norm_act {c.what}'
        _form(what, 'cwn_norm_act_f32 with a cwn_bn_live record (called directly)')
        NC.hold(liv, lambda s: c.fwd(s, 3), cpu, FWD, what)
        NC.hold(liv, c.fwd, None, ('scale', 'shift'), what)
        for name in ('out', 'scale', 'shift', 'mean', 'rstd', 'running_mean', 'running_var'):
            a, b = fin[name].cpu(), liv[name].cpu()
            ulp = (a.view(torch.int32) - b.view(torch.int32)).abs().max()
            print(f'[cw] {c.what}: live against finalize form, {name}: at most {int(ulp)} ulp apart')


@pytest.mark.parametrize('N', [64, 100, 30])
def test_batchnorm_with_eps_zero_does_not_see_a_column_grade(N):
    """eps = 0 at the C ABI: out on z and on z times grade_cols, bit for bit -- the finalize form and the live form; (R) and
    (E) against the Tracked reference with the float32 twin in torch's place (F.batch_norm refuses eps = 0)."""
    for M in MS[1:]:
        c = NC.BnCase(M, N, eps=0.0)
        plain = c.z / c.gc[None, :]
        twin = B.bn_forward_twin(c.z, c.gamma, c.beta, 0.0, c.rm0, c.rv0, NC.MOM)
        twin['out'] = torch.relu(twin['out'])
        for live in (False, True):
            what = f'eps = 0, {"live" if live else "finalize"} form, {c.what}'
            outs = []
            for z in (c.z, plain):
                if live:
                    rec, keep = _live_record(c, z)
                    outs.append(_act(c, live=rec, z=z))
                else:
                    outs.append(_act(c, aff=_finalize(c, z)['aff'], z=z))
            NC.hold(dict(out=outs[0]), c.fwd, twin, ('out',), what)
            bad = int((outs[0] != outs[1]).sum())
            print(f'[cw] {what}: {bad} of {outs[0].numel()} outputs change under the column grades')
            assert torch.equal(outs[0], outs[1]), what


def test_gemm_to_norm_act_with_eps_zero_and_graded_weight_rows():
    """The chain that makes z itself: cwn_gemm_f32 (col_stats) -> cwn_bn_finalize_f32 -> cwn_norm_act_f32 with eps = 0, with and
    without grade_cols on the weight rows and the bias: the same out, bit for bit."""
    g = torch.Generator().manual_seed(5)
    K, N = 64, 64
    for M in MS[1:]:
        c = NC.BnCase(M, N, eps=0.0)
        X, W, b = _stat_operands(g, M, K, N, False)
        outs = []
        for Wv, bv in ((W, b), (W / c.gc[:, None], b / c.gc)):
            cs = torch.zeros(2, ops.stat_rows(M), N, dtype=torch.float64, device=DEV)
            Z, = ops.run_gemm([ops.Gemm(X=X.to(DEV), W=Wv.to(DEV), bias=bv.to(DEV), col_stats=cs, exact=True)], DEV)
            c.z = Z.cpu()
            outs.append(_act(c, aff=_finalize(c)['aff']))
        assert torch.equal(outs[0], outs[1]), f'M={M}: out changes under a power-of-two grade of the weight rows'


@pytest.mark.parametrize('producer', ['gemm', 'linear_stats', 'stage_bands', 'stage_slots'])
def test_statistics_epilogue_to_norm_act(producer):
    """The launches chained as a training step chains them: the producing launch stores z and its float64 statistics, and
    cwn_bn_finalize_f32 + cwn_norm_act_f32 (bands) or cwn_norm_act_f32 with the live record (slots) normalise that z.  The
    reference takes the stored z as its input, so a statistics epilogue that accumulates in float32 fails here."""
    g = torch.Generator().manual_seed(len(producer))
    F = 64
    for M in MS:
        X, W, b = _stat_operands(g, M, F, F, False)
        Xd, bd = X.to(DEV), b.to(DEV)
        slots = torch.zeros(_ffi.BN_SLOTS, 2, F, dtype=torch.float64, device=DEV)
        cs = torch.full((2, ops.stat_rows(M), F), SENT, dtype=torch.float64, device=DEV)
        if producer.startswith('stage'):
            P, _ = _stage_weight(g, F)
            Z, = _run_stage([ops.Gemm(X=Xd * F ** 0.5, W=P, bias=bd, in_relu=1, **(dict(stat_slots=slots) if producer == 'stage_slots'
                                                                                  else dict(col_stats=cs)))])
        else:
            Z = torch.full((M, F), NAN, device=DEV)
            gm = ops.Gemm(X=Xd, W=W.to(DEV), bias=bd, col_stats=cs, out=Z, exact=True)
            if producer == 'gemm':
                ops.run_gemm([gm], DEV)
            else:
                _ffi.linear_stats([gm.desc(Z)], DEV)
        c = NC.BnCase(M, F, z=Z)             # (one row: torch refuses it, (R) alone; the forward stays gated under ReLU)
        if M > 1:
            _capped(c)
        what = f'{producer} -> norm_act {c.what}'
        if producer == 'stage_slots':
            rec, keep = _live_record(c)
            rec.slots = slots.data_ptr()
            got = dict(out=_act(c, live=rec), mean=keep['aff'][2], rstd=keep['aff'][3], running_mean=keep['running_mean'],
                       running_var=keep['running_var'])
            NC.hold(got, lambda s: c.fwd(s, 3), c.cpu32(), FWD, what)
        else:
            got = _finalize(c, stats=cs)
            got['out'] = _act(c, aff=got['aff'])
            NC.hold(got, c.fwd, c.cpu32(), FWD, what)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the next stage's prologue of cwn_dense_stage_f32 with a live input BatchNorm
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [64, 128])
def test_stage_prologue_with_a_live_batchnorm(F):
    """Y = relu(BatchNorm(z)) W^T + b, the affine derived in the consuming stage's prologue from slot sums: (R) with the
    split's 6 K steps on top of the affine's c."""
    g = torch.Generator().manual_seed(3 * F)
    for M in MS:                                  # (one row included: nothing but (R) is asked here, and ReLU is 1-Lipschitz)
        c = NC.BnCase(M, F)
        P, W = _stage_weight(g, F, grade=False)
        b = torch.randn(F, generator=g)
        rec, keep = _live_record(c)
        Y, = _run_stage([ops.Gemm(X=c.z.to(DEV), W=P, bias=b.to(DEV), in_bn=rec, in_relu=1)])
        what = f'stage with a live input BatchNorm F={F} M={M}'
        _form(what, 'cwn_dense_stage_f32 (ops.run_stage took the launch)')
        r = B.ratio(Y, B.linear(c.fwd(B.FMA)['out'], W, b, B.SPLIT(F)), what + ' (R)')
        assert r <= B.RIGOROUS, r
        liv = dict(scale=keep['aff'][0], shift=keep['aff'][1], mean=keep['aff'][2], rstd=keep['aff'][3],
                   running_mean=keep['running_mean'], running_var=keep['running_var'])
        NC.hold(liv, lambda s: c.fwd(s, 3), None, ('scale', 'shift', 'mean', 'rstd', 'running_mean', 'running_var'), what)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. cwn_norm_bwd_reduce_f32 + cwn_norm_bwd_apply_f32, cwn_norm_bwd_f32, cwn_gemm_f32 with the bnb prologue
# ------------------------------------------------------------------------------------------------------------------------------
BWD = ('dz', 's1', 's2')


def _in_slot_order(parts):
    """The CWN_BN_SLOTS float32 slot rows added as the consuming launch adds them: from zero, slot 0 first."""
    total = torch.zeros_like(parts[0])
    for q in range(_ffi.BN_SLOTS):
        total = total + parts[q]
    return total


def _start(c, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2, c.N, generator=g) * c.gc[None, :]


def _with_acc(ref, start):
    ref = dict(ref)
    ref['acc1'], ref['acc2'] = B.add(B.inp(start[0]), ref['s1']), B.add(B.inp(start[1]), ref['s2'])
    return ref


def _cpu_acc(cpu, start):
    return None if cpu is None else dict(cpu, acc1=start[0] + cpu['s1'], acc2=start[1] + cpu['s2'])


def _reduce_apply(c, aff, dy):
    zd, dyd = c.z.to(DEV), dy.to(DEV)
    s12, acc = torch.zeros(2, c.N, device=DEV), _start(c).to(DEV)
    dz = torch.full((c.M, c.N), NAN, device=DEV)
    _ffi.norm_bwd_reduce([_norm_desc(zd, dy=dyd, aff=aff, s12=s12, relu=c.relu)], DEV)
    d = _norm_desc(zd, dy=dyd, out=dz, aff=aff, s12=s12, relu=c.relu)
    d.acc1, d.acc2 = acc[0].data_ptr(), acc[1].data_ptr()
    _ffi.norm_bwd_apply([d], DEV)
    torch.cuda.synchronize()
    return dict(dz=dz, s1=s12[0], s2=s12[1], acc1=acc[0], acc2=acc[1])


def _fused(c, aff, dy, accumulate):
    zd, dyd = c.z.to(DEV), dy.to(DEV)
    s12 = _start(c).to(DEV) if accumulate else torch.full((2, c.N), NAN, device=DEV)
    dz = torch.full((c.M, c.N), NAN, device=DEV)
    _ffi.norm_bwd([_norm_desc(zd, dy=dyd, out=dz, aff=aff, s12=s12, relu=c.relu)], DEV, accumulate=accumulate)
    torch.cuda.synchronize()
    return dict(dz=dz, s1=s12[0], s2=s12[1], acc1=s12[0], acc2=s12[1])


@pytest.mark.parametrize('rows', [False, True], ids=['cols', 'rows'])
@pytest.mark.parametrize('N', [64, 128, 100, 30])
def test_backward_reduce_and_apply(N, rows):
    """cwn_norm_bwd_reduce_f32 (atomics between the 64-row bands) + cwn_norm_bwd_apply_f32, fed by cwn_bn_finalize_f32: dz, s1,
    s2 and what the apply launch adds to acc1 / acc2."""
    for M in MS:
        c = NC.BnCase(M, N, rows=rows, relu=M > 1)
        if M > 1:
            _capped(c)
        got = _reduce_apply(c, _finalize(c)['aff'], c.dy)
        what = f'reduce + apply {c.what}'
        _form(what, 'cwn_norm_bwd_reduce_f32 and cwn_norm_bwd_apply_f32 (called directly)')
        start = _start(c)
        NC.hold(got, lambda s: _with_acc(c.bwd(s), start), _cpu_acc(c.cpu32(), start), BWD + ('acc1', 'acc2'), what)


@pytest.mark.parametrize('accumulate', [False, True], ids=['write', 'accumulate'])
@pytest.mark.parametrize('N', [64, 128, 100])
def test_backward_in_one_launch(N, accumulate):
    """cwn_norm_bwd_f32: column-owning workgroups, every sum in a fixed order.  600 rows: a thread owns two; 4096: the limit.
    Linear in dy: on the column-graded dy, dz, s1 and s2 are the bits of the launch on the ungraded dy times the grades."""
    for M in MS + (600, _ffi.NORM_BWD_FUSED_MAX_ROWS):
        c = NC.BnCase(M, N, relu=M > 1)
        if M > 1:
            _capped(c)
        aff = _finalize(c)['aff']
        got = _fused(c, aff, c.dy, accumulate)
        what = f'one-launch backward {"accumulate" if accumulate else "write"} {c.what}'
        _form(what, 'cwn_norm_bwd_f32 (called directly)')
        start = _start(c)
        if accumulate:
            NC.hold(got, lambda s: _with_acc(c.bwd(s), start), _cpu_acc(c.cpu32(), start), ('dz', 'acc1', 'acc2'), what)
        else:
            NC.hold(got, c.bwd, c.cpu32(), BWD, what)
            plain = _fused(c, aff, c.dy_plain, False)
            B.equivariant(got['dz'], plain['dz'], None, c.gc, what + ' dz')
            B.equivariant(got['s1'][None], plain['s1'][None], None, c.gc, what + ' s1')
            B.equivariant(got['s2'][None], plain['s2'][None], None, c.gc, what + ' s2')


@pytest.mark.parametrize('N,K', [(64, 64), (128, 128), (128, 64)])
def test_backward_as_the_prologue_of_the_input_gradient_gemm(N, K):
    """cwn_gemm_f32 with the bnb extension: dz = scale dyh + c0 + c1 (z - mean) formed on the way into LDS and stored, dx = dz W,
    s1 / s2 handed on to acc1 / acc2.  The sums come from cwn_norm_bwd_reduce_f32."""
    g = torch.Generator().manual_seed(N + K)
    for M in MS:
        c = NC.BnCase(M, N, relu=M > 1)
        if M > 1:
            _capped(c)
        W = torch.randn(N, K, generator=g) / N ** 0.5
        aff = _finalize(c)['aff']
        zd, dyd, Wd = c.z.to(DEV), c.dy.to(DEV), W.to(DEV)
        s12, acc = torch.zeros(2, N, device=DEV), _start(c).to(DEV)
        _ffi.norm_bwd_reduce([_norm_desc(zd, dy=dyd, aff=aff, s12=s12, relu=c.relu)], DEV)
        dz = torch.full((M, N), NAN, device=DEV)
        b = _ffi.GemmBnb(z=zd.data_ptr(), dz=dz.data_ptr(), ldz=N, lddz=N, relu=int(c.relu), scale=aff[0].data_ptr(),
                         shift=aff[1].data_ptr(), mean=aff[2].data_ptr(), rstd=aff[3].data_ptr(), s1=s12[0].data_ptr(),
                         s2=s12[1].data_ptr(), acc1=acc[0].data_ptr(), acc2=acc[1].data_ptr())
        gm = ops.Gemm(X=dyd, W=Wd, w_trans=True, bnb=b)
        split = ops.gemm_uses_split([gm], DEV)
        with torch.no_grad():
            dx, = ops.run_gemm([gm], DEV)
        torch.cuda.synchronize()
        what = f'bnb prologue N={N} K={K} {c.what}'
        _form(what, f'cwn_gemm_f32 with cwn_gemm_bnb, the {"bf16-split" if split else "exact"} kernel')
        start, cpu = _start(c), c.cpu32()
        got = dict(dz=dz, s1=s12[0], s2=s12[1], acc1=acc[0], acc2=acc[1], dx=dx)
        steps = B.SPLIT if split else B.FMA

        def ref_of(s):
            r = _with_acc(c.bwd(s, 'stage'), start)
            r['dx'] = B.linear(r['dz'], W.t(), None, (steps if s is B.FMA else s)(N))
            return r
        cpu = None if cpu is None else dict(_cpu_acc(cpu, start), dx=cpu['dz'] @ W)
        NC.hold(got, ref_of, cpu, BWD + ('acc1', 'acc2', 'dx'), what)


# ------------------------------------------------------------------------------------------------------------------------------
# 6. cwn_dense_stage_bwd_f32 with a norm: constants from s1 / s2 and from the slots of a live producer
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('slots', [False, True], ids=['s1s2', 'slots'])
@pytest.mark.parametrize('wide', [False, True], ids=['F', '2F'])
@pytest.mark.parametrize('F', [64, 128])
def test_stage_backward_with_a_norm(F, wide, slots):
    """dz = scale dyh + a0 + a1 (z - mean) and dx (dx2) = dz W on the split path; s1 / s2 read from memory, or summed in slot
    order from the CWN_BN_SLOTS float32 partials a live producer left (and stored, and handed on to acc1 / acc2)."""
    g = torch.Generator().manual_seed(7 * F + wide)
    n_in = 2 * F if wide else F
    for M in MS:
        c = NC.BnCase(M, F, relu=M > 1)
        if M > 1:
            _capped(c)
        W = torch.randn(F, n_in, generator=g) / F ** 0.5
        P = torch.nn.Parameter(W.to(DEV))
        ops.pack_stage_weights_many([P])
        aff = _finalize(c)['aff']
        zd, dyd = c.z.to(DEV), c.dy.to(DEV)
        a = aff.cpu()
        # the partial sums of dyh and dyh xhat over row chunks, as float32 (a producer's epilogue: the settled mask, float32 xhat)
        xhat = (c.z - a[2]) * a[3]
        parts = torch.zeros(_ffi.BN_SLOTS, 2, F)
        for q, (p1, p2) in enumerate(zip(c.dyh.chunk(_ffi.BN_SLOTS), (c.dyh * xhat).chunk(_ffi.BN_SLOTS))):
            parts[q, 0], parts[q, 1] = p1.double().sum(0).float(), p2.double().sum(0).float()
        s12 = (torch.full((2, F), NAN) if slots else parts.sum(0)).to(DEV)
        acc = _start(c).to(DEV)
        dz, out = torch.full((M, F), NAN, device=DEV), torch.full((M, n_in), NAN, device=DEV)
        b = _ffi.GemmBnb(z=zd.data_ptr(), dz=dz.data_ptr(), ldz=F, lddz=F, relu=int(c.relu), scale=aff[0].data_ptr(),
                         shift=aff[1].data_ptr(), mean=aff[2].data_ptr(), rstd=aff[3].data_ptr(), s1=s12[0].data_ptr(),
                         s2=s12[1].data_ptr(), acc1=acc[0].data_ptr(), acc2=acc[1].data_ptr())
        sl = parts.to(DEV) if slots else None
        ok = ops.run_stage_bwd([(dyd, b, P, out[:, :F], out[:, F:] if wide else None)], DEV, live=[(sl, None, None)])
        assert ok, 'the backward stage kernel refused a launch it is written for'
        torch.cuda.synchronize()
        what = f'stage backward with a norm F={F} n_in={n_in} {"slots" if slots else "s1 / s2"} {c.what}'
        _form(what, 'cwn_dense_stage_bwd_f32 (ops.run_stage_bwd took the launch)')
        start, cpu = _start(c), c.cpu32()
        got = dict(dz=dz, s1=s12[0], s2=s12[1], acc1=acc[0], acc2=acc[1], dx=out)

        def ref_of(s):
            r = _with_acc(c.bwd(s, 'stage'), start)
            r['dx'] = B.linear(r['dz'], W.t(), None, (B.SPLIT if s is B.FMA else s)(F))
            return r
        cpu = None if cpu is None else dict(_cpu_acc(cpu, start), dx=cpu['dz'] @ W)
        # (without slots s1 / s2 are this test's own operands, which the launch only reads: nothing to hold)
        NC.hold(got, ref_of, cpu, (BWD if slots else ('dz',)) + ('acc1', 'acc2'), what)
        r = B.ratio(out, ref_of(B.FMA)['dx'], what + ' dx (R)')
        assert r <= B.RIGOROUS, r
        if slots:          # the stored sums are the slots added in slot order
            want = _in_slot_order(parts)
            assert torch.equal(s12.cpu(), want), what + ': s1 / s2 are not the slots summed in slot order'


@pytest.mark.parametrize('F', [64, 128])
def test_stage_backward_as_a_live_producer(F):
    """cwn_dense_stage_bwd_f32 with out_bn: besides dz and dx, the launch leaves the reduce of the stage that RECEIVES dx as its
    dy -- sum dx [y' > 0] and sum dx [y' > 0] xhat' over its rows, float32 atomics into CWN_BN_SLOTS slot rows.  The receiving
    stage's z' and constants are inputs here (exact float32 vectors), z' moved to its column mean wherever the sign of
    y' = z' scale' + shift' could be disputed, so the mask is settled; the slots are summed in slot order and held to (R) with
    the 6 K steps of dx = dz W under the order-free bound of the sums."""
    g = torch.Generator().manual_seed(11 * F)
    for M in MS:
        c = NC.BnCase(M, F, relu=M > 1)
        if M > 1:
            _capped(c)
        W = torch.randn(F, F, generator=g) / F ** 0.5
        P = torch.nn.Parameter(W.to(DEV))
        ops.pack_stage_weights_many([P])
        aff = _finalize(c)['aff']
        zd, dyd = c.z.to(DEV), c.dy.to(DEV)
        s12 = torch.zeros(2, F, device=DEV)
        _ffi.norm_bwd_reduce([_norm_desc(zd, dy=dyd, aff=aff, s12=s12, relu=c.relu)], DEV)
        # the receiving stage
        r = NC.BnCase(max(M, 33), F, seed=5)             # (one row: the first of 33, under their constants -- inputs either way)
        t = B.bn_forward_twin(r.z, r.gamma, r.beta, NC.EPS, r.rm0, r.rv0, NC.MOM)
        aff2 = torch.stack([t['scale'], t['shift'], t['mean'], t['rstd']])
        y2_of = lambda z: B.add(B.mul(B.inp(z), B.inp(aff2[0])), B.inp(aff2[1]))
        z2 = r.z[:M]
        z2 = torch.where(B.sign_disputed(y2_of(z2)), aff2[2][None, :].expand(M, F), z2).contiguous()
        y2 = y2_of(z2)
        assert not bool(B.sign_disputed(y2).any()), 'the receiving stage still has a disputed ReLU sign'
        mask2 = (y2.v > 0).double()
        slots2 = torch.zeros(_ffi.BN_SLOTS, 2, F, device=DEV)
        z2d, aff2d = z2.to(DEV), aff2.to(DEV)
        live = _ffi.BnBwdLive(z=z2d.data_ptr(), aff=aff2d.data_ptr(), slots=slots2.data_ptr(), ldz=F)
        dz, dx = torch.full((M, F), NAN, device=DEV), torch.full((M, F), NAN, device=DEV)
        b = _ffi.GemmBnb(z=zd.data_ptr(), dz=dz.data_ptr(), ldz=F, lddz=F, relu=int(c.relu), scale=aff[0].data_ptr(),
                         shift=aff[1].data_ptr(), mean=aff[2].data_ptr(), rstd=aff[3].data_ptr(), s1=s12[0].data_ptr(), s2=s12[1].data_ptr())
        assert ops.run_stage_bwd([(dyd, b, P, dx, None)], DEV, live=[(None, live, None)]), 'the backward stage kernel refused the launch'
        torch.cuda.synchronize()
        what = f'stage backward as a live producer F={F} {c.what}'
        _form(what, 'cwn_dense_stage_bwd_f32 with out_bn (ops.run_stage_bwd took the launch)')
        p = slots2.cpu()
        got = _in_slot_order(p)
        dx_t = B.linear(c.bwd(B.FMA, 'stage')['dz'], W.t(), None, B.SPLIT(F))
        assert B.ratio(dx, dx_t, what + ' dx (R)') <= B.RIGOROUS
        dyh2 = B.Tracked(dx_t.v * mask2, dx_t.c * mask2)
        xhat2 = B.mul(B.sub(B.inp(z2), B.inp(aff2[2])), B.inp(aff2[3]))
        for k, (name, ref) in enumerate((('s1', B.col_sum(dyh2, B.FMA)), ('s2', B.col_sum(B.mul(dyh2, xhat2), B.FMA)))):
            rr = B.ratio(got[k], ref, f'{what} slot sums {name} (R)')
            assert rr <= B.RIGOROUS, (name, rr)

# ------------------------------------------------------------------------------------------------------------------------------
# 7. cwn_layernorm_act_f32 / cwn_layernorm_bwd_f32, the 16-byte and the element-wise form
# ------------------------------------------------------------------------------------------------------------------------------
LN = ('out', 'mean', 'rstd', 'dz', 'dgamma', 'dbeta')


def _ld(t):
    return t.stride(0) if t.size(0) > 1 else t.size(1)


def _window(t, col0):
    """t as the columns [col0, col0 + N) of a wider matrix (col0 = 1: only 4-byte aligned, the element-wise form)."""
    if not col0:
        return t.to(DEV)
    wide = torch.full((t.size(0), t.size(1) + 4 + (-t.size(1)) % 4), NAN, device=DEV)
    w = wide[:, col0:col0 + t.size(1)]
    w.copy_(t)
    return w


def _layernorm(c, dy, col0):
    M, N = c.M, c.N
    z, dyd = _window(c.z, col0), _window(dy, col0)
    out, dz = _window(torch.full((M, N), NAN), col0), _window(torch.full((M, N), NAN), col0)
    gam, bet = c.gamma.to(DEV), c.beta.to(DEV)
    mean, rstd = torch.full((M,), NAN, device=DEV), torch.full((M,), NAN, device=DEV)
    dgamma, dbeta = torch.full((N,), NAN, device=DEV), torch.full((N,), NAN, device=DEV)
    _ffi.layer_norm_act([_ffi.LnDesc(z=z.data_ptr(), gamma=gam.data_ptr(), beta=bet.data_ptr(), out=out.data_ptr(), mean=mean.data_ptr(),
                                     rstd=rstd.data_ptr(), M=M, ldz=_ld(z), ldout=_ld(out), N=N, relu=int(c.relu), eps=NC.EPS)], DEV)
    _ffi.layer_norm_bwd([_ffi.LnDesc(z=z.data_ptr(), gamma=gam.data_ptr(), out=out.data_ptr(), mean=mean.data_ptr(), rstd=rstd.data_ptr(),
                                     dy=dyd.data_ptr(), dz=dz.data_ptr(), dgamma=dgamma.data_ptr(), dbeta=dbeta.data_ptr(), M=M,
                                     ldz=_ld(z), ldout=_ld(out), lddy=_ld(dyd), lddz=_ld(dz), N=N, relu=int(c.relu), eps=NC.EPS)], DEV)
    torch.cuda.synchronize()
    return dict(out=out, mean=mean, rstd=rstd, dz=dz, dgamma=dgamma, dbeta=dbeta)


@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'id'])
@pytest.mark.parametrize('col0', [0, 1], ids=['vec16', 'elementwise'])
@pytest.mark.parametrize('N', [3, 100, 160, 260])
def test_layernorm(N, col0, relu):
    """Rows graded by grade_rows and standing grade_ratio spreads off zero, gamma, beta and dy graded by grade_cols: out, the
    row statistics, dz, dgamma and dbeta.  The rows are independent and the backward is linear in dy: with the ROWS of dy graded
    by powers of two, dz is the bits of the ungraded launch times the grades."""
    for M in MS:
        c = NC.LnCase(M, N, relu=relu)
        _capped(c)
        got = _layernorm(c, c.dy, col0)
        what = f'{c.what} {"element-wise" if col0 or N % 4 else "16-byte"} form'
        _form(what, 'cwn_layernorm_act_f32 and cwn_layernorm_bwd_f32 (called directly)')
        NC.hold(got, lambda s: {**c.fwd(s), **c.bwd(s)}, c.torch32(), LN, what)
        gr = B.grade_rows(M)
        graded = _layernorm(c, c.dy * gr[:, None], col0)
        B.equivariant(graded['dz'], got['dz'], gr, None, what + ' dz under row grades of dy')


# ------------------------------------------------------------------------------------------------------------------------------
# 8. one dense_train plan, stage by stage: every BatchNorm from its own record, forward and backward
# ------------------------------------------------------------------------------------------------------------------------------
def _plan(g, F, Ms):
    """Three dimensions x two branches x two Linear(F, F) -> BatchNorm -> ReLU stages and a combine stage over 2F; weight rows
    and biases graded as in section 1; every BatchNorm with its own gamma, beta and running buffers, all away from their defaults,
    so that a stage that met another stage's record is off by orders of magnitude."""
    from cwn_amd import dense_train as DT
    gc, bias = B.grade_cols(F), B.grade_ratio(F) * B.grade_cols(F)

    def stage(k_in):
        lin, bn = torch.nn.Linear(k_in, F), torch.nn.BatchNorm1d(F, eps=NC.EPS, momentum=NC.MOM)
        with torch.no_grad():
            lin.weight.copy_(torch.randn(F, k_in, generator=g) / k_in ** 0.5 * gc[:, None])
            lin.bias.copy_(bias * (torch.randint(0, 2, (F,), generator=g) * 2.0 - 1))
            bn.weight.copy_(torch.rand(F, generator=g) + 0.5)
            bn.bias.copy_(torch.randn(F, generator=g))
            bn.running_mean.copy_(torch.randn(F, generator=g) * gc)
            bn.running_var.copy_((torch.rand(F, generator=g) + 0.5) * gc ** 2)
        return DT.Stage(lin.to(DEV), bn.to(DEV).train())

    chains = [[[stage(F), stage(F)] for _ in range(2)] for _ in Ms]
    plan = DT._Plan(chains, [stage(2 * F) for _ in Ms], 0.0)
    assert DT.supported(list(plan.stages()))
    ops.pack_stage_weights_many([st.lin.weight for st in plan.stages()])
    return plan


@pytest.mark.parametrize('live_bwd', [True, False], ids=['slot_reduce', 'reduce_launches'])
@pytest.mark.parametrize('live', [True, False], ids=['live', 'finalize'])
@pytest.mark.parametrize('F', [64, 128])
def test_dense_train_plan_stage_by_stage(F, live, live_bwd, monkeypatch):
    """dense_train.dense_train forward and backward under LIVE_BN x LIVE_BN_BWD.  A Tracked chain from X to the output
    compounds through every BatchNorm until it bounds nothing, so each of the fifteen stages is held on its own, from what it
    was actually handed: the z the plan stored for the backward, its own gamma, beta and running buffers, and the dy it received
    (captured where the weight-gradient launch is given dz and dy).  Forward: the stage's affine rows, running statistics and its
    consumer's output (the next stage's z, or the plan's output).  Backward: dz, s1 and s2 (beta.grad, gamma.grad), dx from the
    stored dz (the next stage's dy, or X.grad), dW and db.  The plan's dH is zero where the last ReLU's sign is disputed; an
    inner stage cannot be given that, so there a disputed entry of dyh carries an allowance of |dy| (BnCase.bwd_handed)."""
    from cwn_amd import dense_train as DT
    g = torch.Generator().manual_seed(F + 2 * live + live_bwd)
    monkeypatch.setattr(DT, 'LIVE_BN', live)
    monkeypatch.setattr(DT, 'LIVE_BN_BWD', live_bwd)
    calls = dict(finalize=0, reduce=0, stage_bwd=0, tn=0)
    handed = []                                  # per weight-gradient launch: (the dz list, the dy list), combine stage first

    def counted(mod, name, key, after=None):
        real = getattr(mod, name)

        def wrapper(*a, **kw):
            res = real(*a, **kw)
            calls[key] += 1 if res is None else int(bool(res))
            if after is not None:
                after(*a, **kw)
            return res
        monkeypatch.setattr(mod, name, wrapper)

    def keep_handed(descs, dev, keep=None, deferrable=False):
        flat = lambda ts: [t.detach().clone() for x in ts for t in (x if isinstance(x, (list, tuple)) else [x])]
        handed.append((flat(keep[0]), flat(keep[4])))
    counted(_ffi, 'bn_finalize', 'finalize')
    counted(_ffi, 'norm_bwd_reduce', 'reduce')
    counted(ops, 'run_stage_bwd', 'stage_bwd')
    counted(_ffi, 'gemm_tn', 'tn', after=keep_handed)

    Ms = MS[1:]                                  # (torch.nn.BatchNorm1d, and with it a plan, takes no batch of one row)
    plan = _plan(g, F, Ms)
    stages = list(plan.stages())
    before = {id(st): tuple(t.detach().cpu().clone() for t in (st.norm.weight, st.norm.bias, st.norm.running_mean, st.norm.running_var))
              for st in stages}
    xs = [torch.randn(M, F, generator=g).to(DEV).requires_grad_(True) for M in Ms for _ in range(2)]
    H = DT.dense_train(plan, xs)
    node = H[0].grad_fn
    saved = [t.detach() for t in node.saved_tensors]
    nd, o = len(Ms), 2 * len(Ms)
    Z = [[[saved[o + 4 * i + 2 * br + s] for s in range(2)] for br in range(2)] for i in range(nd)]
    Z3 = saved[o + 4 * nd: o + 5 * nd]
    aff_of = {k: v.detach().cpu().clone() for k, v in node.aff_of.items()}
    torch.cuda.synchronize()
    assert (calls['finalize'] == 0) == live, f'LIVE_BN = {live}: cwn_bn_finalize_f32 was launched {calls["finalize"]} times'
    tag = f'dense_train F={F} {"live" if live else "finalize"} / {"slot reduce" if live_bwd else "reduce launches"}'
    _form(tag, ('live records' if live else 'cwn_bn_finalize_f32 launches') + ' forward')
    cpu = lambda t: t.detach().cpu()

    def case(st, z, M, relu=True):
        c = NC.BnCase(M, F, z=z, module=before[id(st)], relu=relu)
        _capped(c)
        return c

    def hold_forward(st, c, what):
        a = aff_of[id(st)]
        got = dict(scale=a[0], shift=a[1], mean=a[2], rstd=a[3], running_mean=st.norm.running_mean, running_var=st.norm.running_var)
        NC.hold(got, lambda s: c.fwd(s, 3 if live else 1), None, tuple(got), what)
        assert int(st.norm.num_batches_tracked) == 1, what

    cases = {}
    for i, M in enumerate(Ms):
        outs = []
        for br in range(2):
            for s, st in enumerate(plan.chains[i][br]):
                what = f'{tag} M={M} branch {br} stage {s}'
                c = cases[id(st)] = case(st, Z[i][br][s], M)
                hold_forward(st, c, what)
                if s == 0:
                    nxt = plan.chains[i][br][1]
                    ref = B.linear(c.fwd(B.FMA)['out'], cpu(nxt.lin.weight), cpu(nxt.lin.bias), B.SPLIT(F))
                    assert B.ratio(Z[i][br][1], ref, what + ': the next stage\'s z (R)') <= B.RIGOROUS
                else:
                    outs.append(c.fwd(B.FMA)['out'])
        st, what = plan.cb[i], f'{tag} M={M} combine'
        ref = B.linear(B.cat(outs), cpu(st.lin.weight), cpu(st.lin.bias), B.SPLIT(2 * F))
        assert B.ratio(Z3[i], ref, what + ': z of the combine stage (R)') <= B.RIGOROUS
        c = cases[id(st)] = case(st, Z3[i], M)
        hold_forward(st, c, what)
        assert B.ratio(H[i], c.fwd(B.FMA)['out'], what + ': the plan\'s output (R)') <= B.RIGOROUS

    # ---- backward: dH graded in the columns, zero where the last ReLU is disputed
    dH = [(torch.randn(M, F, generator=g) * B.grade_cols(F)[None, :] * (~cases[id(plan.cb[i])].disputed)).to(DEV) for i, M in enumerate(Ms)]
    torch.autograd.backward(H, dH)
    torch.cuda.synchronize()
    assert calls['stage_bwd'] == 3, f'cwn_dense_stage_bwd_f32 took {calls["stage_bwd"]} of the 3 backward launches'
    assert calls['reduce'] == (1 if live_bwd else 3), f'LIVE_BN_BWD = {live_bwd}: {calls["reduce"]} reduce launches'
    _form(tag, 'cwn_dense_stage_bwd_f32' + (' with the slot sums of its producers' if live_bwd else ' behind cwn_norm_bwd_reduce_f32') + ' backward')
    assert len(handed) == 3 and [len(h[0]) for h in handed] == [nd, 2 * nd, 2 * nd]
    for k, got_dy in enumerate(handed[0][1]):
        assert torch.equal(got_dy, dH[k]), 'the combine stage was not handed dH'

    def hold_backward(st, c, dy, dz, x_act, dx_got, what):
        """x_act: the Tracked activation the stage's Linear read; dx_got: what the stage passed down."""
        ref = c.bwd_handed(B.FMA, dy)
        got = dict(dz=dz, s1=st.norm.bias.grad, s2=st.norm.weight.grad)
        for name in ('dz', 's1', 's2'):
            assert B.ratio(got[name], ref[name], f'{what} {name} (R)') <= B.RIGOROUS, (what, name)
        W = cpu(st.lin.weight)
        assert B.ratio(dx_got, B.linear(B.inp(dz), W.t(), None, B.SPLIT(F)), what + ' dx (R)') <= B.RIGOROUS, what
        M = dz.size(0)
        dW = B.linear(B.Tracked(x_act.v.t(), x_act.c.t()), cpu(dz).t(), None, B.SPLIT(M))           # (6 M: either form of cwn_gemm_tn_f32)
        assert B.ratio(st.lin.weight.grad.t(), dW, what + ' dW (R)') <= B.RIGOROUS, what
        assert B.ratio(st.lin.bias.grad, B.col_sum(B.inp(dz), B.FMA), what + ' db (R)') <= B.RIGOROUS, what

    def activation(st):
        """relu(z scale + shift) as a consumer's prologue forms it from the stage's stored affine rows (inputs)."""
        a, c = aff_of[id(st)], cases[id(st)]
        return B.act(B.add(B.mul(B.inp(c.z), B.inp(a[0])), B.inp(a[1])), 'relu')

    for i, M in enumerate(Ms):
        ups = [plan.chains[i][br] for br in range(2)]
        st = plan.cb[i]
        dy1 = [handed[1][1][2 * i + br] for br in range(2)]                  # what the last update stages were handed
        hold_backward(st, cases[id(st)], dH[i], handed[0][0][i], B.cat([activation(ch[1]) for ch in ups]), torch.cat(dy1, 1),
                      f'{tag} M={M} combine')
        for br in range(2):
            k = 2 * i + br
            hold_backward(ups[br][1], cases[id(ups[br][1])], dy1[br], handed[1][0][k], activation(ups[br][0]), handed[2][1][k],
                          f'{tag} M={M} branch {br} stage 1')
            hold_backward(ups[br][0], cases[id(ups[br][0])], handed[2][1][k], handed[2][0][k], B.inp(xs[k]), xs[k].grad,
                          f'{tag} M={M} branch {br} stage 0')
