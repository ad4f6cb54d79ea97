"""The dense-product kernels under GRADED operands, held entry by entry (tests/_bounds.py; tests/test_bounds_host.py proves
on the CPU that these checks can fail).

tests/_product.gate bounds max|got - ref| by 1e-5 * |ref|_inf: with one magnitude in every row, column and k-position (randn)
that is a fair bound, and with graded ones it sees the largest entries only.  Here rows are scaled by 2^((7r mod 25) - 12),
output columns (weight rows, bias) by 2^((11n mod 25) - 12), the contraction index by 2^((5k mod 17) - 8) on X and its inverse
on W, and every case asserts
  (R) |got - v| <= 2 * 2^-24 * c, c the first-order bound of the float64 reference with the accumulation steps of the kernel
      form that ran (K per output for an fma / fp32-MFMA chain, 6 K for the six-plane bf16 split);
  (E) the same ratio with one step per product, within MARGIN x the ratio of float32 torch on the CPU on the same operands;
  (equivariance) where the operation is positively homogeneous (ReLU or id, no statistics): the bits of the launch on the
      operands without the column and inner grades, times the column grades -- and times the row grades too where no bias
      breaks homogeneity in the rows.  Power-of-two scaling commutes with the rne split, bf16 products and fp32 accumulation in
      a fixed order, so a difference is a value-dependent path or a hidden absolute constant.
Which kernel form ran is asserted in every case (ops.gemm_uses_split, cwn_gemm_tn_would_split, the `*_applies` predicates, or
the C entry point called directly: a non-zero code raises), so nothing passes on a fall-back to torch.
Rows are tests/_windows.ROWS = (1, 33, 70); widths one MFMA-exact one and one ragged one of the kernel's own test module."""
import pytest
import torch

from cwn_amd import _ffi, ops
from tests import _bounds as B
from tests._windows import ROWS

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)


def _rand(g, *shape):
    return torch.randn(*shape, generator=g)


def _form(what, form):
    print(f'[cw] {what}: served by {form}')


def _product_case(g, M, K, N, bias=True):
    """(plain, graded) CPU operands (X, W, b) of one product.  `plain` keeps the row grades when there is a bias (a bias is not
    homogeneous in the rows) and carries none otherwise; returns with them the row / column grades that lead from the plain
    output to the graded one."""
    X, W = _rand(g, M, K), _rand(g, N, K) / K ** 0.5
    b = _rand(g, N) if bias else None
    graded = B.graded(X, W, b)
    plain = B.graded(X, W, b, rows=bias, cols=False, inner=False)
    return plain, graded, (None if bias else B.grade_rows(M)), B.grade_cols(N)


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


# ------------------------------------------------------------------------------------------------------------------------------
# 1. cwn_gemm_f32, exact and split form
# ------------------------------------------------------------------------------------------------------------------------------
GEMM_CASES = {
    # name: (N, K, K2, w_trans, bias, relu, add_out, packed, exact flag, split expected)
    'exact_64x64_bias_relu': (64, 64, 0, False, True, True, False, False, False, False),
    'exact_40x24': (40, 24, 0, False, False, False, False, False, False, False),
    'exact_40x24_bias_relu': (40, 24, 0, False, True, True, False, False, False, False),
    'exact_128x128_forced': (128, 128, 0, False, False, False, False, False, True, False),
    'w_trans_128x128': (128, 128, 0, True, False, False, False, False, False, False),
    'w_trans_40x24_bias': (40, 24, 0, True, True, False, False, False, False, False),
    'concat_64x24+12_bias_relu': (64, 24, 12, False, True, True, False, False, False, False),
    'concat_128x64+64': (128, 64, 64, False, False, False, False, False, False, False),
    'add_out_40x24': (40, 24, 0, False, False, False, True, False, False, False),
    'add_out_128x128': (128, 128, 0, False, False, False, True, False, False, False),
    'split_128x128': (128, 128, 0, False, False, False, False, False, False, True),
    'split_128x128_bias_relu': (128, 128, 0, False, True, True, False, False, False, True),
    'split_128x128_packed_bias': (128, 128, 0, False, True, False, False, True, False, True),
}


def _gemm_launch(case, X, W, b, Y0):
    N, K, K2, w_trans, bias, relu, add_out, packed, exact, split = GEMM_CASES[case]
    Xd, Wd, bd = _dev(X, W.t().contiguous() if w_trans else W, b)
    Wp = torch.nn.Parameter(Wd) if packed else Wd
    gm = ops.Gemm(X=Xd[:, :K].contiguous(), X2=Xd[:, K:].contiguous() if K2 else None, W=Wp, bias=bd, relu=relu, w_trans=w_trans,
                  exact=exact, add_out=add_out, out=Y0.to(DEV) if add_out else None,
                  w_packed=ops.pack_gemm_weight(Wp) if packed else None)
    assert not packed or gm.w_packed is not None
    assert ops.gemm_uses_split([gm], DEV) == split, f'{case}: not the kernel form the case is written for'
    with torch.no_grad():
        return ops.run_gemm([gm], DEV)[0]


@pytest.mark.parametrize('case', sorted(GEMM_CASES))
def test_gemm(case):
    """cwn_gemm_f32: the exact fp32-MFMA kernel (natural and transposed weight, the X | X2 concatenation, bias, the ReLU
    epilogue, ADD_OUT, and CWN_GEMM_EXACT at the split kernel's own shape) and the bf16-split kernel (fp32 and packed weight)."""
    N, K, K2, w_trans, bias, relu, add_out, packed, exact, split = GEMM_CASES[case]
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    steps = B.SPLIT if split else B.FMA
    for M in ROWS:
        what = f'gemm {case} M={M}'
        (Xp, Wp, bp), (X, W, b), gr, gc = _product_case(g, M, K + K2, N, bias)
        Y0p = _rand(g, M, N) if add_out else None
        Y0 = Y0p * B.grade_rows(M)[:, None] * gc[None, :] if add_out else None
        got = _gemm_launch(case, X, W, b, Y0)
        _form(what, 'the bf16-split kernel' if split else 'the exact fp32-MFMA kernel')

        def ref_of(s):
            t = B.linear(B.inp(X), W, b, s(K + K2))
            t = B.act(t, 'relu') if relu else t
            return B.add(B.inp(Y0), t) if add_out else t
        cpu32 = X @ W.t() + (b if bias else 0)
        cpu32 = torch.relu(cpu32) if relu else cpu32
        cpu32 = Y0 + cpu32 if add_out else cpu32
        B.check(got, ref_of, steps, cpu32, what)
        plain = _gemm_launch(case, Xp, Wp, bp, Y0p)
        B.equivariant(got, plain, gr, gc, what)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. cwn_gemm_tn_f32, both forms: the reduce dimension is M
# ------------------------------------------------------------------------------------------------------------------------------
TN_BAND = 128                      # kBandRows of csrc/cwn_gemm_tn.hip: the rows of one workgroup's partial sum (ordered form: always)
TN_ROWS = ROWS + (TN_BAND + 1,)    # ... and one row past it: a second band of one row


def _tn_launch(dZ, X, K, K2, ordered, want_split):
    M, N = dZ.shape
    dZd, Xd = _dev(dZ, X)
    X1 = Xd[:, :K].contiguous()
    X2 = Xd[:, K:].contiguous() if K2 else None
    dW, db = torch.zeros(N, K + K2, device=DEV), torch.zeros(N, device=DEV)
    d = _ffi.GemmTnDesc(dZ=dZd.data_ptr(), X=X1.data_ptr(), X2=_ffi.ptr(X2), in_scale=None, in_shift=None, in_scale2=None,
                        in_shift2=None, dW=dW.data_ptr(), db=db.data_ptr(), M=M, lddz=N, ldx=K, ldx2=K2, lddw=K + K2, N=N, K=K, K2=K2,
                        in_relu=0)
    assert _ffi.gemm_tn_would_split([d]) == want_split, 'not the kernel form the case is written for'
    prev = _ffi.DETERMINISTIC_TN
    _ffi.DETERMINISTIC_TN = ordered
    try:
        _ffi.gemm_tn([d], DEV)
    finally:
        _ffi.DETERMINISTIC_TN = prev
    torch.cuda.synchronize()
    return dW, db


@pytest.mark.parametrize('ordered', [False, True], ids=['atomic', 'ordered'])
@pytest.mark.parametrize('N,K,K2,split', [(128, 128, 0, True), (128, 64, 64, True), (64, 64, 0, False), (40, 24, 12, False)])
def test_gemm_tn(N, K, K2, split, ordered):
    """dW = dZ^T [X | X2] and db = the column sums of dZ.  The output rows are the columns of dZ (row grades), the output columns
    those of X (column grades), and the reduce index runs over the M rows (inner grades on dZ, their inverse on X).  The
    ordered form adds its band partials in band order: bit-identical under the grades; the atomic form promises no order
    between bands and keeps (R) and (E) only.  db is a sum over the graded index itself: (R) and (E)."""
    g = torch.Generator().manual_seed(N + 3 * K + 7 * K2)
    steps = B.SPLIT if split else B.FMA
    for M in TN_ROWS:
        what = f'gemm_tn {N}x{K}+{K2} {"ordered" if ordered else "atomic"} M={M}'
        dZ, X = _rand(g, M, N), _rand(g, M, K + K2) / M ** 0.5
        At, Bt, _ = B.graded(dZ.t().contiguous(), X.t().contiguous())          # [N, M] and [K + K2, M]
        dW, db = _tn_launch(At.t().contiguous(), Bt.t().contiguous(), K, K2, ordered, split)
        _form(what, 'the bf16-split kernel' if split else 'the fp32-MFMA kernel')
        B.check(dW, lambda s: B.linear(B.inp(At), Bt, None, s(M)), steps, At @ Bt.t(), what + ' dW')
        ones = torch.ones(1, M)
        B.check(db[:, None], lambda s: B.linear(B.inp(At), ones, None, s(M)), B.FMA, (At @ ones.t()), what + ' db')
        if ordered:
            dWp, _ = _tn_launch(dZ, X, K, K2, ordered, split)
            B.equivariant(dW, dWp, B.grade_rows(N), B.grade_cols(K + K2), what + ' dW')


# ------------------------------------------------------------------------------------------------------------------------------
# 3. cwn_linear_wide_f32 and the product output of cwn_linear_stats_f32
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('w_trans', [False, True], ids=['natural', 'transposed'])
@pytest.mark.parametrize('K,K2,N', [(160, 160, 160), (100, 157, 160), (129, 0, 5)])
def test_linear_wide(K, K2, N, w_trans):
    """cwn_linear_wide_f32 (K + K2 beyond cwn_gemm_f32's 256 and a ragged pair of widths), the C entry point itself."""
    assert ops.linear_wide_applies(K, K2, N)
    g = torch.Generator().manual_seed(1000 * K + 10 * K2 + N)

    def launch(X, W, b):
        Xd, Wd, bd = _dev(X, W.t().contiguous() if w_trans else W, b)
        Y = torch.full((X.size(0), N), float('nan'), device=DEV)
        d = ops._wide_desc(Xd[:, :K].contiguous(), Xd[:, K:].contiguous() if K2 else None, Wd, bd, Y, w_trans)
        _ffi.check(_ffi.lib().cwn_linear_wide_f32((_ffi.LinearWideDesc * 1)(d), 1, _ffi.stream_ptr(DEV)), 'cwn_linear_wide_f32')
        return Y

    for M in ROWS:
        for bias in (True, False):
            what = f'linear_wide {"W" if w_trans else "W^T"} K={K}+{K2} N={N} bias={bias} M={M}'
            (Xp, Wp, bp), (X, W, b), gr, gc = _product_case(g, M, K + K2, N, bias)
            got = launch(X, W, b)
            _form(what, 'cwn_linear_wide_f32 (called directly)')
            B.check(got, lambda s: B.linear(B.inp(X), W, b, s(K + K2)), B.FMA, X @ W.t() + (b if bias else 0), what)
            B.equivariant(got, launch(Xp, Wp, bp), gr, gc, what)


@pytest.mark.parametrize('K,K2,N', [(48, 0, 48), (13, 0, 24), (37, 0, 100), (128, 128, 128)])
def test_linear_stats_product(K, K2, N):
    """Y of cwn_linear_stats_f32 (the band statistics divide nothing here, but they are sums of squares of graded values: out of
    scope, and not asked for)."""
    g = torch.Generator().manual_seed(1000 * K + 10 * K2 + N)

    def launch(X, W, b):
        Xd, Wd, bd = _dev(X, W, b)
        Y = torch.full((X.size(0), N), float('nan'), device=DEV)
        gm = ops.Gemm(X=Xd[:, :K].contiguous(), X2=Xd[:, K:].contiguous() if K2 else None, W=Wd, bias=bd, exact=True, out=Y)
        _ffi.linear_stats([gm.desc(Y)], DEV)
        return Y

    for M in ROWS:
        for bias in (True, False):
            what = f'linear_stats K={K}+{K2} N={N} bias={bias} M={M}'
            (Xp, Wp, bp), (X, W, b), gr, gc = _product_case(g, M, K + K2, N, bias)
            got = launch(X, W, b)
            _form(what, 'cwn_linear_stats_f32 (called directly)')
            B.check(got, lambda s: B.linear(B.inp(X), W, b, s(K + K2)), B.FMA, X @ W.t() + (b if bias else 0), what)
            B.equivariant(got, launch(Xp, Wp, bp), gr, gc, what)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. cwn_dense_stage_f32 / cwn_dense_stage_ex_f32 / dx of cwn_dense_stage_bwd_f32
# ------------------------------------------------------------------------------------------------------------------------------
def _stage_launch(F, blocks, cases):
    """One launch over `cases` = [(X [M, blocks * F], W [F, blocks * F], b)], a descriptor each."""
    Ws = [torch.nn.Parameter(W.to(DEV)) for _, W, _ in cases]
    ops.pack_stage_weights_many(Ws)
    gemms = []
    for (X, _, b), W in zip(cases, Ws):
        Xb = [X[:, j * F:(j + 1) * F].contiguous().to(DEV) for j in range(blocks)]
        gemms.append(ops.Gemm(X=Xb[0], X2=Xb[1] if blocks > 1 else None, W=W, bias=None if b is None else b.to(DEV),
                              more=tuple((x, False, None) for x in Xb[2:])))
    with torch.no_grad():
        got = ops.run_stage(gemms, DEV)
    assert got is not None, 'the stage kernel refused a launch it is written for'
    return got


@pytest.mark.parametrize('F', [64, 128])
@pytest.mark.parametrize('blocks', [1, 2, 3, 4])
def test_dense_stage(blocks, F):
    """cwn_dense_stage_f32 (F -> F, 2F -> F) and cwn_dense_stage_ex_f32 (3F, 4F -> F): every row count a descriptor of one
    launch, with and without a bias."""
    g = torch.Generator().manual_seed(F + 5 * blocks)
    K = blocks * F
    for bias in (True, False):
        cs = [_product_case(g, M, K, F, bias) for M in ROWS]
        got = _stage_launch(F, blocks, [c[1] for c in cs])
        plain = _stage_launch(F, blocks, [c[0] for c in cs])
        for M, (_, (X, W, b), gr, gc), y, yp in zip(ROWS, cs, got, plain):
            what = f'dense stage{"_ex" if blocks > 2 else ""} F={F} blocks={blocks} bias={bias} M={M}'
            _form(what, 'the stage kernel (ops.run_stage took the launch)')
            B.check(y, lambda s: B.linear(B.inp(X), W, b, s(K)), B.SPLIT, X @ W.t() + (b if bias else 0), what)
            B.equivariant(y, yp, gr, gc, what)


@pytest.mark.parametrize('F', [64, 128])
@pytest.mark.parametrize('wide', [False, True], ids=['F', '2F'])
def test_dense_stage_backward_dx(wide, F):
    """dx = (dy * [z > 0]) W of cwn_dense_stage_bwd_f32 without a norm, for a Linear(F -> F) and the two halves of a
    Linear(2F -> F).  The mask comes from z, which is not graded; dz = the masked dy bit for bit."""
    g = torch.Generator().manual_seed(17 * F + wide)
    n_in = 2 * F if wide else F

    def launch(cases):
        Ws = [torch.nn.Parameter(Wt.t().contiguous().to(DEV)) for _, Wt, _ in cases]         # Linear layout [F, n_in]
        ops.pack_stage_weights_many(Ws)
        entries, keep = [], []
        for (dy, _, z), W in zip(cases, Ws):
            M = dy.size(0)
            dyd, zd = dy.to(DEV), z.to(DEV)
            dz, out = torch.full((M, F), float('nan'), device=DEV), torch.full((M, n_in), float('nan'), device=DEV)
            bnb = _ffi.GemmBnb(z=zd.data_ptr(), dz=dz.data_ptr(), ldz=F, lddz=F, relu=1)
            entries.append((dyd, bnb, W, out[:, :F], out[:, F:] if wide else None))
            keep.append((dyd, zd, dz, out))
        assert ops.run_stage_bwd(entries, DEV), 'the backward stage kernel refused a launch it is written for'
        torch.cuda.synchronize()
        return [(k[2], k[3]) for k in keep]

    zs = [_rand(g, M, F) for M in ROWS]
    cs = [_product_case(g, M, F, n_in, bias=False) for M in ROWS]             # x = dy [M, F], "W" = W^T [n_in, F]
    got = launch([(c[1][0], c[1][1], z) for c, z in zip(cs, zs)])
    plain = launch([(c[0][0], c[0][1], z) for c, z in zip(cs, zs)])
    for M, (_, (dy, Wt, _), gr, gc), z, (dz, dx), (_, dxp) in zip(ROWS, cs, zs, got, plain):
        what = f'dense stage backward F={F} n_in={n_in} M={M}'
        _form(what, 'the backward stage kernel (ops.run_stage_bwd took the launch)')
        masked = dy * (z > 0)
        assert torch.equal(dz.cpu(), masked), what + ': dz is not the masked dy'
        B.check(dx, lambda s: B.linear(B.inp(masked), Wt, None, s(F)), B.SPLIT, masked @ Wt.t(), what + ' dx')
        B.equivariant(dx, dxp, gr, gc, what + ' dx')


# ------------------------------------------------------------------------------------------------------------------------------
# 5. cwn_target_head_f32 and cwn_linear_many_f64
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,K', [(64, 10), (128, 64), (20, 3)])
def test_target_head(H, K):
    """out[c] = W x[rows[c]] + b: one marked row per complex out of 3 C + 2 rows of x."""
    from cwn_amd.csr import _err_flag, check_errors
    g = torch.Generator().manual_seed(H + K)
    for Cn in ROWS:
        n = 3 * Cn + 2
        rows = (torch.arange(Cn) * 3 + 1).to(torch.int32)
        for bias in (True, False):
            what = f'target_head H={H} K={K} bias={bias} complexes={Cn}'
            (Xp, Wp, bp), (X, W, b), gr, gc = _product_case(g, n, H, K, bias)

            def launch(X, W, b):
                Xd, Wd, bd = _dev(X, W, b)
                assert ops.target_head_applies(Xd, rows.to(DEV), Wd, bd), what
                out = _ffi.target_head(Xd, rows.to(DEV), Wd, bd, _err_flag(DEV))
                check_errors(DEV)
                return out
            got = launch(X, W, b)
            _form(what, 'cwn_target_head_f32 (called directly)')
            sel = rows.long()
            B.check(got, lambda s: B.linear(B.rows(B.inp(X), sel), W, b, s(H)), B.FMA, X[sel] @ W.t() + (b if bias else 0), what)
            B.equivariant(got, launch(Xp, Wp, bp), None if gr is None else gr[sel], gc, what)


@pytest.mark.parametrize('act', ['id', 'relu'])
@pytest.mark.parametrize('K,N', [(128, 128), (24, 40), (1, 5)])
def test_linear_many_f64(K, N, act):
    """cwn_linear_many_f64: the unit is 2^-53 and the gate its analogue of (R) only; every row count a product of one launch."""
    g = torch.Generator().manual_seed(K * N)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    cases = []
    for M in ROWS:
        X, W, b = rnd(M, K), rnd(N, K) / K ** 0.5, rnd(N)
        cases.append((B.graded(X, W, b, cols=False, inner=False), B.graded(X, W, b)))          # (row grades only, all grades)
    run = lambda which: ops.linear_many_f64([tuple(_dev(*c[which])) + (act,) for c in cases])
    got, plain = run(1), run(0)
    for M, (_, (X, W, b)), y, yp in zip(ROWS, cases, got, plain):
        what = f'linear_many_f64 K={K} N={N} act={act} M={M}'
        _form(what, 'cwn_linear_many_f64 (ops.linear_many_f64 has no other route)')
        assert y.dtype == torch.float64
        B.check(y, lambda s: B.act(B.linear(B.inp(X), W, b, s(K)), act), B.FMA, None, what, unit=B.UNIT64)
        B.equivariant(y, yp, None, B.grade_cols(N).double(), what)


# ------------------------------------------------------------------------------------------------------------------------------
# 6. the update / combine chains: cwn_update_mlp_f32, cwn_update_mlp3_f32, cwn_update_chain_f32 / _f64
# ------------------------------------------------------------------------------------------------------------------------------
class _Chain:
    """`branches` two-stage networks F_in -> H -> H and a combine branches * H -> H, each stage act(scale * (x W^T + b) + shift)
    (an eval-mode BatchNorm folded to an affine; the second stage of the first branch carries none), float32 on the CPU.

    grade(hidden): the rows of the inputs by grade_rows; the input columns by grade_inner and its inverse on the first
    stages' weight columns; with `hidden` (ReLU and id: positively homogeneous) every hidden layer's columns by grade_inner --
    weight rows, bias and shift of the stage that writes them, the inverse on the weight columns of the stage that reads them
    -- and the output columns by grade_cols.  An activation that is not homogeneous gets no grade behind it.
    `plain()` keeps the row grades only (the biases are not homogeneous in the rows)."""

    def __init__(self, g, M, F_in, H, branches, act, dtype=torch.float32):
        self.M, self.F_in, self.H, self.nb, self.act, self.dtype = M, F_in, H, branches, act, dtype
        shapes = [(H, F_in), (H, H)] * branches + [(H, branches * H)]
        self.W = [_rand(g, o, i).to(dtype) / i ** 0.5 for o, i in shapes]
        self.b = [_rand(g, o).to(dtype) * 0.5 for o, _ in shapes]
        self.fold = [(None, None) if k == 1 else ((torch.rand(o, generator=g) + 0.5).to(dtype), _rand(g, o).to(dtype) * 0.3)
                     for k, (o, _) in enumerate(shapes)]
        self.x = [_rand(g, M, F_in).to(dtype) * 2 for _ in range(branches)]

    def _with(self, x, W, b, fold):
        c = object.__new__(_Chain)
        c.__dict__.update(self.__dict__)
        c.x, c.W, c.b, c.fold = x, W, b, fold
        return c

    def plain(self):
        gr = B.grade_rows(self.M).to(self.dtype)[:, None]
        return self._with([x * gr for x in self.x], self.W, self.b, self.fold)

    def graded(self):
        hidden = self.act in ('relu', 'id')
        dt, H, nb = self.dtype, self.H, self.nb
        gr, gi = B.grade_rows(self.M).to(dt)[:, None], B.grade_inner(self.F_in).to(dt)
        one = torch.ones(H, dtype=dt)
        gh = B.grade_inner(H).to(dt) if hidden else one
        gc = B.grade_cols(H).to(dt) if hidden else one
        x = [t * gr * gi[None, :] for t in self.x]
        W, b, fold = list(self.W), list(self.b), list(self.fold)
        outs = [gh] * (2 * nb) + [gc]                                    # the grade of each stage's output columns
        ins = [gi, gh] * nb + [gh.repeat(nb)]                            # ... and of the columns it reads
        for k in range(2 * nb + 1):
            W[k] = self.W[k] * outs[k][:, None] / ins[k][None, :]
            b[k] = self.b[k] * outs[k]
            sc, sh = self.fold[k]
            fold[k] = (sc, None if sh is None else sh * outs[k])
        return self._with(x, W, b, fold), (gc if hidden else None)

    def _stage(self, k, t, steps):
        t = B.linear(t, self.W[k], self.b[k], steps(self.W[k].size(1)))
        sc, sh = self.fold[k]
        if sc is not None:
            t = B.scale(t, sc, sh)
        return B.act(t, self.act)

    def ref_of(self, steps):
        hs = [self._stage(2 * j + 1, self._stage(2 * j, B.inp(x), steps), steps) for j, x in enumerate(self.x)]
        return self._stage(2 * self.nb, B.cat(hs), steps)

    def cpu(self):
        """The restatement in the chain's own precision in torch on the CPU."""
        f = B.ACTS[self.act]

        def stage(k, x):
            y = x @ self.W[k].t() + self.b[k]
            sc, sh = self.fold[k]
            return f(y if sc is None else y * sc + sh)
        return stage(2 * self.nb, torch.cat([stage(2 * j + 1, stage(2 * j, x)) for j, x in enumerate(self.x)], 1))

    def linears(self):
        out = []
        for W, b in zip(self.W, self.b):
            lin = torch.nn.Linear(W.size(1), W.size(0))
            with torch.no_grad():
                lin.weight.copy_(W)
                lin.bias.copy_(b)
            out.append(lin.to(DEV))
        return out

    def dev_folds(self):
        return [(None if s is None else s.to(DEV), None if t is None else t.to(DEV)) for s, t in self.fold]


def _chain_checks(make, launch, steps, what, unit=B.UNIT32):
    """`make(M)` a _Chain; `launch(chains)` the kernel's outputs for a list of them (one dimension each)."""
    base = [make(M) for M in ROWS]
    graded = [c.graded() for c in base]
    got = launch([c for c, _ in graded])
    plain = launch([c.plain() for c in base])
    for M, (c, gc), y, yp in zip(ROWS, graded, got, plain):
        w = f'{what} M={M}'
        B.check(y, c.ref_of, steps, c.cpu() if unit == B.UNIT32 else None, w, unit=unit)
        if c.act in ('relu', 'id'):
            B.equivariant(y, yp, None, gc, w)


@pytest.mark.parametrize('F,w_in', [(64, 64), (128, 128), (64, 20), (128, 3)])
def test_update_mlp(F, w_in):
    """cwn_update_mlp_f32: five Linear layers per dimension, the three row counts the three dimensions of one launch; F-wide
    and narrow (in_width) inputs."""
    g = torch.Generator().manual_seed(3 * F + w_in)

    def launch(chains):
        dims = [ops.MlpDim(x_up=c.x[0].to(DEV), x_b=c.x[1].to(DEV), linears=c.linears(), folds=c.dev_folds()) for c in chains]
        assert ops.update_mlp_applies(dims), 'cwn_update_mlp_f32 does not take the case written for it'
        with torch.no_grad():
            return ops.update_mlp(dims)

    what = f'update_mlp F={F} in_width={w_in}'
    _form(what, 'cwn_update_mlp_f32 (ops.update_mlp has no other route)')
    _chain_checks(lambda M: _Chain(g, M, w_in, F, 2, 'relu'), launch, B.SPLIT, what)


@pytest.mark.parametrize('F', [64, 128])
def test_update_mlp3(F):
    """cwn_update_mlp3_f32: seven Linear layers per dimension."""
    g = torch.Generator().manual_seed(5 * F)

    def launch(chains):
        dims = [ops.Mlp3Dim(xs=[x.to(DEV) for x in c.x], linears=c.linears(), folds=c.dev_folds()) for c in chains]
        assert ops.update_mlp3_applies(dims), 'cwn_update_mlp3_f32 does not take the case written for it'
        with torch.no_grad():
            return ops.update_mlp3(dims)

    what = f'update_mlp3 F={F}'
    _form(what, 'cwn_update_mlp3_f32 (ops.update_mlp3 has no other route)')
    _chain_checks(lambda M: _Chain(g, M, F, F, 3, 'relu'), launch, B.SPLIT, what)


def _chain_dims(chains):
    return [ops.ChainDim(in_up=c.x[0].to(DEV), in_b=c.x[1].to(DEV), weights=_dev(*c.W), biases=_dev(*c.b), folds=c.dev_folds(),
                         act=c.act) for c in chains]


@pytest.mark.parametrize('act', ['relu', 'id', 'tanh', 'elu', 'sigmoid'])
@pytest.mark.parametrize('F,H', [(64, 64), (128, 128), (24, 40), (100, 128)])
def test_update_chain_f32(F, H, act):
    """cwn_update_chain_f32 (exact fp32 MFMA) at an MFMA-exact and a ragged pair of widths; tanh, ELU and sigmoid are not
    homogeneous: no grade behind the first activation and no equivariance, (R) and (E) all the same."""
    g = torch.Generator().manual_seed(F + 3 * H + len(act))

    def launch(chains):
        dims = _chain_dims(chains)
        assert ops.update_chain_f32_applies(dims), 'cwn_update_chain_f32 does not take the case written for it'
        with torch.no_grad():
            return ops.update_chain_f32(dims)

    what = f'update_chain_f32 F={F} H={H} act={act}'
    _form(what, 'cwn_update_chain_f32 (ops.update_chain_f32 has no other route)')
    _chain_checks(lambda M: _Chain(g, M, F, H, 2, act), launch, B.FMA, what)


@pytest.mark.parametrize('act', ['relu', 'elu'])
@pytest.mark.parametrize('F,H', [(64, 64), (24, 40)])
def test_update_chain_f64(F, H, act):
    """cwn_update_chain_f64 with the float64 unit: the analogue of (R)."""
    g = torch.Generator().manual_seed(F + 3 * H + len(act))

    def launch(chains):
        dims = _chain_dims(chains)
        assert ops.update_chain_f64_applies(dims), 'cwn_update_chain_f64 does not take the case written for it'
        with torch.no_grad():
            return ops.update_chain_f64(dims)

    what = f'update_chain_f64 F={F} H={H} act={act}'
    _form(what, 'cwn_update_chain_f64 (ops.update_chain_f64 has no other route)')
    _chain_checks(lambda M: _Chain(g, M, F, H, 2, act, dtype=torch.float64), launch, B.FMA, what, unit=B.UNIT64)


# ------------------------------------------------------------------------------------------------------------------------------
# 7. layers over a graph: cwn_gin_layer_f32, cwn_gine_layer_f32, cwn_oriented_layer_f32
# ------------------------------------------------------------------------------------------------------------------------------
def _coo(g, n, per_row=3):
    """A COO index [2, E] (source, destination) over n rows in shuffled entry order; every third row has no entry."""
    deg = torch.randint(1, 2 * per_row, (n,), generator=g)
    deg[torch.arange(n) % 3 == 1] = 0
    if n == 1:
        deg[0] = 2
    dst = torch.repeat_interleave(torch.arange(n), deg)
    src = torch.randint(0, n, (int(deg.sum()),), generator=g)
    p = torch.randperm(dst.numel(), generator=g)
    return torch.stack([src[p], dst[p]])


class _TwoStage:
    """The two (Linear, folded norm) groups of a GINConv / GINEConv network w -> H -> H with the grades of `_Chain`: the input
    columns, the hidden columns (ReLU and id only) and the output columns (ReLU and id only)."""

    def __init__(self, g, w, H, act):
        self.w, self.H, self.act = w, H, act
        self.stages = [(_rand(g, H, k) / k ** 0.5, 0.3 * _rand(g, H), 1.0 + 0.3 * torch.rand(H, generator=g), 0.3 * _rand(g, H))
                       for k in (w, H)]

    def graded(self):
        hom = self.act in ('relu', 'id')
        one = torch.ones(self.H)
        gi, gh, gc = B.grade_inner(self.w), (B.grade_inner(self.H) if hom else one), (B.grade_cols(self.H) if hom else one)
        out = []
        for (W, b, sc, sh), go, gin in zip(self.stages, (gh, gc), (gi, gh)):
            out.append((W * go[:, None] / gin[None, :], b * go, sc, sh * go))
        return out, gi, (gc if hom else None)

    def tracked(self, t, stages, steps):
        for W, b, sc, sh in stages:
            t = B.act(B.scale(B.linear(t, W, b, steps(W.size(1))), sc, sh), self.act)
        return t

    def cpu(self, s, stages):
        f = B.ACTS[self.act]
        for W, b, sc, sh in stages:
            s = f((s @ W.t() + b) * sc + sh)
        return s


def _dev_stages(stages):
    return [tuple(t.to(DEV) for t in s) for s in stages]


@pytest.mark.parametrize('act', ['relu', 'tanh'])
@pytest.mark.parametrize('w,H', [(64, 64), (100, 128), (3, 5)])
def test_gin_layer(w, H, act):
    """cwn_gin_layer_f32: s = A x + (1 + eps) x, two (Linear, affine, act) stages.  The rows of x carry the row grades, so a
    destination sums neighbours of up to 2^24 apart; the sum mixes rows, so the equivariance is held under the column and
    inner grades."""
    from cwn_amd import csr
    g = torch.Generator().manual_seed(w * 1000 + H + len(act))
    eps = 0.375                       # (a float32 number: the kernel reads eps in float32)
    net = _TwoStage(g, w, H, act)
    graded, gi, gc = net.graded()
    for n in ROWS:
        what = f'gin_layer w={w} H={H} act={act} n={n}'
        idx = _coo(g, n)
        adj = csr.Adjacency.from_index(idx.to(DEV), n, n)
        xp = _rand(g, n, w) * B.grade_rows(n)[:, None]
        x = xp * gi[None, :]

        def launch(x, stages):
            xd, sd = x.to(DEV), _dev_stages(stages)
            assert ops.gin_layer_applies(xd, sd), what
            with torch.no_grad():
                return ops.gin_layer(xd, adj, eps, sd, act)
        got = launch(x, graded)
        _form(what, 'cwn_gin_layer_f32 (ops.gin_layer has no other route)')

        def ref_of(s):
            t = B.inp(x)
            agg = B.add(B.segment_sum(B.rows(t, idx[0]), idx[1], n), B.scale(t, 1.0 + eps))
            return net.tracked(agg, graded, s)
        s32 = torch.zeros(n, w).index_add_(0, idx[1], x[idx[0]]) + (1.0 + eps) * x
        B.check(got, ref_of, B.FMA, net.cpu(s32, graded), what)
        if gc is not None:
            B.equivariant(got, launch(xp, net.stages), None, gc, what)


@pytest.mark.parametrize('act', ['relu', 'elu'])
@pytest.mark.parametrize('w,H', [(64, 64), (100, 128), (5, 64)])
def test_gine_layer(w, H, act):
    """cwn_gine_layer_f32 with one edge row per entry: s = sum relu(x_j + e_ji) + (1 + eps) x_i.  The edge rows are graded like
    rows of x (and in the columns with it: the message is homogeneous in the column grade)."""
    from cwn_amd import csr
    g = torch.Generator().manual_seed(w * 1000 + H + len(act))
    eps = 0.375                       # (a float32 number: the kernel reads eps in float32)
    net = _TwoStage(g, w, H, act)
    graded, gi, gc = net.graded()
    for n in ROWS:
        what = f'gine_layer w={w} H={H} act={act} n={n}'
        idx = _coo(g, n)
        E = idx.size(1)
        adj = csr.Adjacency.from_index(idx.to(DEV), n, n)
        xp, ep = _rand(g, n, w) * B.grade_rows(n)[:, None], _rand(g, E, w) * B.grade_rows(E)[:, None]
        x, e = xp * gi[None, :], ep * gi[None, :]

        def launch(x, e, stages):
            xd, ed, sd = x.to(DEV), e.to(DEV), _dev_stages(stages)
            assert ops.gine_layer_applies(xd, ed, sd), what
            with torch.no_grad():
                return ops.gine_layer(xd, adj, ed, eps, sd, act, edge_mode='perm')
        got = launch(x, e, graded)
        _form(what, 'cwn_gine_layer_f32 (ops.gine_layer has no other route)')

        def ref_of(s):
            t = B.inp(x)
            msg = B.act(B.add(B.rows(t, idx[0]), B.inp(e)), 'relu')
            agg = B.add(B.segment_sum(msg, idx[1], n), B.scale(t, 1.0 + eps))
            return net.tracked(agg, graded, s)
        s32 = torch.zeros(n, w).index_add_(0, idx[1], torch.relu(x[idx[0]] + e)) + (1.0 + eps) * x
        B.check(got, ref_of, B.FMA, net.cpu(s32, graded), what)
        if gc is not None:
            B.equivariant(got, launch(xp, ep, net.stages), None, gc, what)


@pytest.mark.parametrize('act', ['relu', 'id', 'sigmoid'])
@pytest.mark.parametrize('w,H', [(64, 64), (12, 20), (100, 128)])
def test_oriented_layer(w, H, act):
    """cwn_oriented_layer_f32: act(x Ws^T + (A_up o_up x) Wu^T + (A_dn o_dn x) Wd^T) with orientations +-1: one product over
    the three blocks [x | A_up o x | A_dn o x] in the tracked reference.  Sigmoid is the tightest (R) of the module (1.49 measured):
    rows graded to 2^-12 give z ~ 0, so c ~ |v| = 1/2 alone, and 1 / (1 + expf(-z)) is three rounded operations."""
    from cwn_amd import csr
    g = torch.Generator().manual_seed(w * 1000 + H + len(act))
    hom = act in ('relu', 'id')
    Ws = [_rand(g, H, w) / (3 * w) ** 0.5 for _ in range(3)]
    gi, gc = B.grade_inner(w), (B.grade_cols(H) if hom else torch.ones(H))
    Wg = [W * gc[:, None] / gi[None, :] for W in Ws]
    for n in ROWS:
        what = f'oriented_layer w={w} H={H} act={act} n={n}'
        iu, il = _coo(g, n), _coo(g, n, per_row=2)
        ou, ol = (torch.randint(0, 2, (i.size(1),), generator=g).float() * 2 - 1 for i in (iu, il))
        au, al = (csr.Adjacency.from_index(i.to(DEV), n, n) for i in (iu, il))
        xp = _rand(g, n, w) * B.grade_rows(n)[:, None]
        x = xp * gi[None, :]

        def launch(x, W):
            xd, wd = x.to(DEV), [t.to(DEV) for t in W]
            assert ops.oriented_layer_applies(xd, wd), what
            with torch.no_grad():
                return ops.oriented_layer(xd, au, ou.to(DEV), al, ol.to(DEV), wd[0], wd[1], wd[2], act)
        got = launch(x, Wg)
        _form(what, 'cwn_oriented_layer_f32 (ops.oriented_layer has no other route)')

        def ref_of(s):
            t = B.inp(x)
            blocks = [t] + [B.segment_sum(B.scale(B.rows(t, i[0]), o[:, None]), i[1], n) for i, o in ((iu, ou), (il, ol))]
            return B.act(B.linear(B.cat(blocks), torch.cat(Wg, 1), None, s(3 * w)), act)
        a32 = [torch.zeros(n, w).index_add_(0, i[1], o[:, None] * x[i[0]]) for i, o in ((iu, ou), (il, ol))]
        cpu32 = B.ACTS[act](x @ Wg[0].t() + a32[0] @ Wg[1].t() + a32[1] @ Wg[2].t())
        B.check(got, ref_of, B.FMA, cpu32, what)
        if hom:
            B.equivariant(got, launch(xp, Ws), None, gc, what)


# ------------------------------------------------------------------------------------------------------------------------------
# 8. readouts: cwn_embed_pool_f32 + cwn_agnostic_head_f32, cwn_head_f32, cwn_flow_head_f32
# ------------------------------------------------------------------------------------------------------------------------------
def _ptr(sizes):
    return torch.cat([torch.zeros(1, dtype=torch.long), torch.tensor(sizes).cumsum(0)])


def _complex_of(ptr):
    return torch.repeat_interleave(torch.arange(ptr.numel() - 1), ptr[1:] - ptr[:-1])


SIZES = ([9, 37, 0, 23, 1], [12, 40, 0, 30, 4], [1, 11, 0, 3, 0])       # cells per complex and dimension; complex 2 is empty


@pytest.mark.parametrize('mean', [False, True], ids=['sum', 'mean'])
@pytest.mark.parametrize('act', ['relu', 'tanh'])
@pytest.mark.parametrize('K,H,O', [(64, 64, 10), (7, 20, 3)])
def test_embed_pool_and_agnostic_head(K, H, O, act, mean):
    """pooled_d = pool_c(act(x_d W_d^T + b_d)) (cwn_embed_pool_f32), out = sum_d act(pooled_d W1^T + b1) W2^T + b2
    (cwn_agnostic_head_f32, fed with the first launch's output): both results through one tracked reference."""
    g = torch.Generator().manual_seed(K + 3 * H + O + len(act) + mean)
    hom = act in ('relu', 'id')
    one = torch.ones(H)
    gi, gh, gh2 = B.grade_inner(K), (B.grade_inner(H) if hom else one), (B.grade_cols(H) if hom else one)
    go = B.grade_cols(O)
    ptrs = [_ptr(s) for s in SIZES]
    Cn = len(SIZES[0])
    xp = [_rand(g, int(p[-1]), K) * B.grade_rows(int(p[-1]))[:, None] for p in ptrs]
    We, be = [_rand(g, H, K) / K ** 0.5 for _ in ptrs], [0.3 * _rand(g, H) for _ in ptrs]
    W1, b1, W2, b2 = _rand(g, H, H) / H ** 0.5, 0.3 * _rand(g, H), _rand(g, O, H) / H ** 0.5, 0.3 * _rand(g, O)
    plain = (xp, We, be, W1, b1, W2, b2)
    graded = ([x * gi[None, :] for x in xp], [W * gh[:, None] / gi[None, :] for W in We], [b * gh for b in be],
              W1 * gh2[:, None] / gh[None, :], b1 * gh2, W2 * go[:, None] / gh2[None, :], b2 * go)

    def launch(x, We, be, W1, b1, W2, b2):
        with torch.no_grad():
            pooled = ops.embed_pool(_dev(*x), _dev(*ptrs), Cn, _dev(*We), _dev(*be), act, mean=mean)
            return pooled, ops.agnostic_head(pooled, *_dev(W1, b1, W2, b2), act)

    x, We_, be_, W1_, b1_, W2_, b2_ = graded
    pooled, out = launch(*graded)
    what = f'K={K} H={H} O={O} act={act} {"mean" if mean else "sum"}'
    _form('embed_pool + agnostic_head ' + what, 'cwn_embed_pool_f32 and cwn_agnostic_head_f32 (the wrappers have no other route)')

    def tracked(s):
        ps = [B.segment_sum(B.act(B.linear(B.inp(x[d]), We_[d], be_[d], s(K)), act), _complex_of(ptrs[d]), Cn, mean=mean)
              for d in range(3)]
        hs = [B.act(B.linear(p, W1_, b1_, s(H)), act) for p in ps]
        return ps, B.linear(B.add(B.add(hs[0], hs[1]), hs[2]), W2_, b2_, s(H))
    f = B.ACTS[act]
    ps32 = []
    for d in range(3):
        p = torch.zeros(Cn, H).index_add_(0, _complex_of(ptrs[d]), f(x[d] @ We_[d].t() + be_[d]))
        ps32.append(p / torch.tensor(SIZES[d]).clamp(min=1)[:, None] if mean else p)
    out32 = sum(f(p @ W1_.t() + b1_) for p in ps32) @ W2_.t() + b2_
    for d in range(3):
        B.check(pooled[d], lambda s: tracked(s)[0][d], B.FMA, ps32[d], f'embed_pool {what} dim {d}')
    B.check(out, lambda s: tracked(s)[1], B.FMA, out32, f'agnostic_head {what}')
    if hom:
        pooled_p, out_p = launch(*plain)
        for d in range(3):
            B.equivariant(pooled[d], pooled_p[d], None, gh, f'embed_pool {what} dim {d}')
        B.equivariant(out, out_p, None, go, f'agnostic_head {what}')


@pytest.mark.parametrize('mean', [False, True], ids=['sum', 'mean'])
@pytest.mark.parametrize('K,H2,O', [(64, 128, 2), (20, 12, 3), (640, 128, 2), (2048, 8, 1)])
def test_head(K, H2, O, mean):
    """cwn_head_f32: pool per complex (sum / mean, one empty complex), relu(lin1_d) per dimension, their sum, lin2.  K = 640
    and 2048: a thread of the 512 holds more than one column of a chunked or a partials sum.  A sixth complex of 300 cells per
    dimension is summed chunk by chunk -- inside the head launch, or by the pooling launch ahead of it (HEAD_POOL_SPLIT '4') --
    while the small ones take the one-pass form: the same bits from both launches."""
    from tests._readout_bwd import HEAD_SIZES
    assert tuple(s[:-1] for s in HEAD_SIZES) == SIZES
    g = torch.Generator().manual_seed(K + H2 + O + mean)
    gi, gh, go = B.grade_inner(K), B.grade_inner(H2), B.grade_cols(O)
    ptrs = [_ptr(s) for s in HEAD_SIZES]
    Cn = len(HEAD_SIZES[0])
    xp = [_rand(g, int(p[-1]), K) * B.grade_rows(int(p[-1]))[:, None] for p in ptrs]
    W1, b1 = [_rand(g, H2, K) / K ** 0.5 for _ in ptrs], [0.3 * _rand(g, H2) for _ in ptrs]
    W2, b2 = _rand(g, O, H2) / H2 ** 0.5, 0.3 * _rand(g, O)
    x = [t * gi[None, :] for t in xp]
    W1g, b1g, W2g, b2g = [W * gh[:, None] / gi[None, :] for W in W1], [b * gh for b in b1], W2 * go[:, None] / gh[None, :], b2 * go

    def launch(x, W1, b1, W2, b2, split=None):
        prev = ops.HEAD_POOL_SPLIT
        ops.HEAD_POOL_SPLIT = prev if split is None else split
        try:
            with torch.no_grad():
                return ops.head(_dev(*x), _dev(*ptrs), Cn, _dev(*W1), _dev(*b1), W2.to(DEV), b2.to(DEV), mean_readout=mean, want_pooled=True)
        finally:
            ops.HEAD_POOL_SPLIT = prev
    out, pooled = launch(x, W1g, b1g, W2g, b2g)
    what = f'head K={K} H2={H2} O={O} {"mean" if mean else "sum"}'
    _form(what, 'cwn_head_f32 (ops.head has no other route)')
    out_s, pooled_s = launch(x, W1g, b1g, W2g, b2g, split='4')
    assert torch.equal(out_s, out), what + ': the pooling launch ahead of the head changes the prediction'
    for d in range(3):
        assert torch.equal(pooled_s[d], pooled[d]), f'{what}: the pooling launch ahead of the head changes pooled dim {d}'

    def tracked(s):
        ps = [B.segment_sum(B.inp(x[d]), _complex_of(ptrs[d]), Cn, mean=mean) for d in range(3)]
        hs = [B.act(B.linear(ps[d], W1g[d], b1g[d], s(K)), 'relu') for d in range(3)]
        return ps, B.linear(B.add(B.add(hs[0], hs[1]), hs[2]), W2g, b2g, s(H2))
    ps32 = []
    for d in range(3):
        p = torch.zeros(Cn, K).index_add_(0, _complex_of(ptrs[d]), x[d])
        ps32.append(p / torch.tensor(HEAD_SIZES[d]).clamp(min=1)[:, None] if mean else p)
    out32 = sum(torch.relu(ps32[d] @ W1g[d].t() + b1g[d]) for d in range(3)) @ W2g.t() + b2g
    for d in range(3):
        B.check(pooled[d], lambda s: tracked(s)[0][d], B.FMA, ps32[d], f'{what} pooled dim {d}')
        assert not bool(pooled[d][2].any()), 'the empty complex pools to zeros'
    B.check(out, lambda s: tracked(s)[1], B.FMA, out32, what)
    out_p, pooled_p = launch(xp, W1, b1, W2, b2)
    B.equivariant(out, out_p, None, go, what)
    for d in range(3):
        B.equivariant(pooled[d], pooled_p[d], None, gi, f'{what} pooled dim {d}')


@pytest.mark.parametrize('mean', [False, True], ids=['sum', 'mean'])
@pytest.mark.parametrize('take_abs', [True, False], ids=['abs', 'signed'])
@pytest.mark.parametrize('K,H,O', [(64, 64, 2), (20, 12, 3)])
def test_flow_head(K, H, O, take_abs, mean):
    """cwn_flow_head_f32: pooled = sum (mean) of |x| or x per cochain (one of them empty), lin2 relu(lin1 pooled + b1) + b2."""
    g = torch.Generator().manual_seed(K + H + O + take_abs + 2 * mean)
    gi, gh, go = B.grade_inner(K), B.grade_inner(H), B.grade_cols(O)
    sizes = SIZES[1]
    ptr, Cn = _ptr(sizes), len(sizes)
    xp = _rand(g, int(ptr[-1]), K) * B.grade_rows(int(ptr[-1]))[:, None]
    W1, b1, W2, b2 = _rand(g, H, K) / K ** 0.5, 0.3 * _rand(g, H), _rand(g, O, H) / H ** 0.5, 0.3 * _rand(g, O)
    x, W1g, b1g, W2g, b2g = xp * gi[None, :], W1 * gh[:, None] / gi[None, :], b1 * gh, W2 * go[:, None] / gh[None, :], b2 * go

    def launch(x, W1, b1, W2, b2):
        ops_ = _dev(x, ptr, W1, b1, W2, b2)
        assert ops.flow_head_applies(*ops_)
        with torch.no_grad():
            return ops.flow_head(*ops_, abs=take_abs, mean=mean)
    out = launch(x, W1g, b1g, W2g, b2g)
    what = f'flow_head K={K} H={H} O={O} {"abs" if take_abs else "signed"} {"mean" if mean else "sum"}'
    _form(what, 'cwn_flow_head_f32 (ops.flow_head has no other route)')
    fx = x.abs() if take_abs else x                                    # (|.| is exact)

    def ref_of(s):
        p = B.segment_sum(B.inp(fx), _complex_of(ptr), Cn, mean=mean)
        return B.linear(B.act(B.linear(p, W1g, b1g, s(K)), 'relu'), W2g, b2g, s(H))
    p32 = torch.zeros(Cn, K).index_add_(0, _complex_of(ptr), fx)
    p32 = p32 / torch.tensor(sizes).clamp(min=1)[:, None] if mean else p32
    B.check(out, ref_of, B.FMA, torch.relu(p32 @ W1g.t() + b1g) @ W2g.t() + b2g, what)
    B.equivariant(out, launch(xp, W1, b1, W2, b2), None, go, what)


# ------------------------------------------------------------------------------------------------------------------------------
# 9. cwn_layer_fused_f32: both forms and a BIG record
# ------------------------------------------------------------------------------------------------------------------------------
def _layer_tracked(conv, b, steps):
    """[(out_up, out_b)] per dimension as tests/test_gpu_blocked._oracle_scope states them, tracked:
    out_up = sum_{j -> i, shared s} relu(W [x_j | x'_s] + bias) + (1 + eps1) x_i,  out_b = sum of the boundary rows + (1 + eps2) x_i."""
    from tests.test_gpu_blocked import cpu
    xs = {d: B.inp(b.cochains[d].x) for d in range(3)}
    outs = []
    for d in range(3):
        c, lvl = b.cochains[d], conv.mp_levels[d]
        n, F = xs[d].v.shape
        zero = B.inp(torch.zeros(n, F))
        up = bnd = zero
        if (d + 1) in b.cochains and c.upper_index is not None:
            ui, sh = cpu(c.upper_index), cpu(c.shared_coboundaries)
            pair = B.cat([B.rows(xs[d], ui[0]), B.rows(xs[d + 1], sh)])
            msg = B.act(B.linear(pair, lvl.msg_up_nn[1].weight, lvl.msg_up_nn[1].bias, steps(2 * F)), 'relu')
            up = B.segment_sum(msg, ui[1], n)
        if d > 0 and c.boundary_index is not None:
            bi = cpu(c.boundary_index)
            bnd = B.segment_sum(B.rows(xs[d - 1], bi[0]), bi[1], n)
        outs.append((B.add(up, B.scale(xs[d], 1.0 + float(lvl.eps1))), B.add(bnd, B.scale(xs[d], 1.0 + float(lvl.eps2)))))
    return outs


def _big_batch(F, seed):
    """Five molecules of 10 - 20 atoms and one of 50 - 60, which one workgroup does not hold at width 128: a BIG record."""
    from cwn_amd.complex import ComplexBatch
    from cwn_amd.synthetic import molhiv_like_complexes
    cxs = molhiv_like_complexes(5, seed, 6, n_lo=10, n_hi=20)
    cxs = cxs[:2] + molhiv_like_complexes(1, seed + 1, 6, n_lo=50, n_hi=60) + cxs[2:]
    b = ComplexBatch.from_complex_list(cxs, max_dim=2).to(DEV)
    g = torch.Generator().manual_seed(seed + 17)
    for d in range(3):
        b.cochains[d].x = _rand(g, b.cochains[d].num_cells, F).to(DEV)
    return b


@pytest.mark.parametrize('F,variant,big', [(64, '0', False), (64, '1', False), (128, '0', False), (128, '1', False), (128, '0', True)],
                         ids=['64-16wave', '64-two_per_cu', '128-16wave', '128-two_per_cu', '128-big'])
def test_layer_fused(F, variant, big):
    """cwn_layer_fused_f32 on six small synthetic complexes, eps = 0.25: the 16-wave and the two-per-CU form, and a batch one
    complex of which is a BIG record.  The cell rows of every dimension carry the row grades; the features' columns one grade g, which the message
    network hands on (weight rows and bias by g, both column halves by 1 / g): messages and self terms then add up in one scale
    per column, and the outputs are those of the row-graded launch times g."""
    from tests.test_gpu_blocked import _batch, _conv, _oracle_scope
    from tests.test_gpu_split_terms import _run_variant
    b = _big_batch(F, seed=41) if big else _batch('zinc', 6, F, seed=41)
    conv = _conv(F, seed=42, eps=0.25)
    gcol = B.grade_inner(F)
    plain_x = [b.cochains[d].x.cpu() * B.grade_rows(b.cochains[d].num_cells)[:, None] for d in range(3)]
    plain_w = [(lvl.msg_up_nn[1].weight.detach().cpu().clone(), lvl.msg_up_nn[1].bias.detach().cpu().clone()) for lvl in conv.mp_levels]

    def run(graded):
        with torch.no_grad():
            for d, lvl in enumerate(conv.mp_levels):
                W, bias = plain_w[d]
                x = plain_x[d]
                if graded:
                    W, bias, x = W * gcol[:, None] / torch.cat([gcol, gcol])[None, :], bias * gcol, x * gcol[None, :]
                lvl.msg_up_nn[1].weight.copy_(W)
                lvl.msg_up_nn[1].bias.copy_(bias)
                b.cochains[d].x = x.to(DEV)
        outs, table = _run_variant(conv, b, variant, big=big)                # (asserts that the blocked layer served the launch)
        assert table.variant == int(variant) and (table.n_big > 0) == big, (table.variant, table.n_big)
        return outs

    plain = run(False)
    got = run(True)                                                          # (conv and b stay graded for the references)
    what = f'layer_fused F={F} variant {variant}{" BIG" if big else ""}'
    _form(what, f'cwn_layer_fused_f32, variant {variant}, {"BIG records" if big else "no BIG record"}')
    cpu32 = _oracle_scope(conv, b, dtype=torch.float32)
    for d in range(3):
        for k, name in enumerate(('out_up', 'out_b')):
            w = f'{what} {name}[{d}]'
            B.check(got[2 * d + k], lambda s: _layer_tracked(conv, b, s)[d][k], B.SPLIT, cpu32[d][k], w)
            B.equivariant(got[2 * d + k], plain[2 * d + k], None, gcol, w)
