"""A float64 reference that carries its own first-order error bound, and the componentwise gates built on it.

tests/_product.gate is one max-norm bound per tensor, 1e-5 * max(1, |ref|_inf): an entry far below |ref|_inf may be wholly
wrong inside it.  Here every reference value v travels with c, the amplification of ONE rounding into it (float64 CPU tensors
of one shape; an input has c = 0), and a result is held entry by entry to

    |got - v| <= ratio * unit * c            unit = 2^-24 (float32) or 2^-53 (float64)

  (R) rigorous:   ratio <= 2, c built with the number of accumulation steps the kernel form performs per output (`n_acc`: K for
                  an fma / fp32-MFMA chain, 6 K for the six-plane bf16 split); the 2 covers an adder that chops.  Never tuned.
  (E) empirical:  ratio <= MARGIN * max(1, ratio_cpu32), c built with n_acc = 1 and ratio_cpu32 the same ratio of the same
                  operation in float32 torch on the CPU, on the same operands: never measured against the kernel.

Operands are GRADED: powers of two on rows, output columns and the contraction index, so that the entries of one output
differ by up to 2^48 and a localised error cannot hide behind |ref|_inf.  Power-of-two scaling commutes with the rne split,
with bf16 products and with fp32 accumulation in a fixed order, so a positively homogeneous operation gives bit-identical
output (`equivariant`).  The same code runs over torch emulations on the CPU (tests/test_bounds_host.py: the checks can fail)
and over the kernels (tests/test_gpu_componentwise.py)."""
from dataclasses import dataclass

import torch

UNIT32 = 2.0 ** -24
UNIT64 = 2.0 ** -53
# (E).  Started at 4; on the device cwn_linear_wide_f32 (K = 100 + 157, one fma chain of 257 steps) came to 4.8 against a limit
# of 6.7 -- within 2x of it -- so the margin went to the next power of two.  DESIGN.md, "Componentwise gate", holds the ratios.
MARGIN = 8.0
RIGOROUS = 2.0        # (R)


@dataclass
class Tracked:
    v: torch.Tensor       # the reference value, float64 on the CPU
    c: torch.Tensor       # first-order error amplification, in units of one rounding


def _d(t) -> torch.Tensor:
    return t.detach().cpu().double()


def inp(t) -> Tracked:
    v = _d(t)
    return Tracked(v, torch.zeros_like(v))


def linear(x: Tracked, W, b, n_acc: float) -> Tracked:
    """x W^T + b with W [N, K]; `n_acc` accumulation steps per output."""
    W = _d(W)
    b = torch.zeros(W.size(0), dtype=torch.float64) if b is None else _d(b)
    v = x.v @ W.t() + b
    c = x.c @ W.abs().t() + n_acc * (x.v.abs() @ W.abs().t()) + b.abs() + v.abs()
    return Tracked(v, c)


ACTS = {'relu': torch.relu, 'elu': torch.nn.functional.elu, 'tanh': torch.tanh, 'sigmoid': torch.sigmoid, 'id': lambda t: t}


def act(x: Tracked, name: str) -> Tracked:
    """Every activation here is 1-Lipschitz: the incoming error passes at most unchanged, and the result is rounded once."""
    v = ACTS[name](x.v)
    return Tracked(v, x.c + v.abs())


def add(a: Tracked, b: Tracked) -> Tracked:
    v = a.v + b.v
    return Tracked(v, a.c + b.c + v.abs())


def scale(x: Tracked, s, shift=None) -> Tracked:
    """s * x (+ shift): (1 + eps) * x, or an eval-mode BatchNorm folded to an affine."""
    s = _d(s) if torch.is_tensor(s) else torch.tensor(float(s), dtype=torch.float64)
    v = x.v * s
    c = x.c * s.abs() + v.abs()
    if shift is not None:
        v = v + _d(shift)
        c = c + _d(shift).abs() + v.abs()
    return Tracked(v, c)


# elementwise forms (an optimizer's update): every result is rounded once, and the incoming amplifications pass through the
# first derivatives
def scalar(x, c: float = 0.0) -> Tracked:
    """A scalar that broadcasts: a hyperparameter as the kernel holds it (c = 0), or a value computed on the way (c > 0)."""
    return Tracked(torch.tensor(float(x), dtype=torch.float64), torch.tensor(float(c), dtype=torch.float64))


def sub(a: Tracked, b: Tracked) -> Tracked:
    v = a.v - b.v
    return Tracked(v, a.c + b.c + v.abs())


def mul(a: Tracked, b: Tracked) -> Tracked:
    v = a.v * b.v
    return Tracked(v, a.c * b.v.abs() + a.v.abs() * b.c + v.abs())


def div(a: Tracked, b: Tracked) -> Tracked:
    v = a.v / b.v
    return Tracked(v, a.c / b.v.abs() + v.abs() * b.c / b.v.abs() + v.abs())


def sqrt(a: Tracked) -> Tracked:
    """d sqrt(x) = dx / (2 sqrt(x)); a.v > 0."""
    v = a.v.sqrt()
    return Tracked(v, a.c / (2 * v) + v.abs())


def power(a: Tracked, t: float) -> Tracked:
    """a^t for an exact exponent t >= 1: d a^t = t a^(t-1) da."""
    v = a.v ** t
    return Tracked(v, a.c * t * a.v.abs() ** (t - 1) + v.abs())


def cat(xs) -> Tracked:
    return Tracked(torch.cat([x.v for x in xs], 1), torch.cat([x.c for x in xs], 1))


def rows(x: Tracked, index) -> Tracked:
    """A gather of rows: exact."""
    return Tracked(x.v[index], x.c[index])


def segment_sum(x: Tracked, index: torch.Tensor, n_out: int, mean: bool = False) -> Tracked:
    """out[index[i]] += x[i] (index_add / segment sum / segment mean): c sums the sources' c, plus the row length (the number
    of sources of the output row) times the sum of their |v|."""
    index = index.cpu().long()
    z = lambda: torch.zeros((n_out,) + tuple(x.v.shape[1:]), dtype=torch.float64)
    v, c, a = z().index_add_(0, index, x.v), z().index_add_(0, index, x.c), z().index_add_(0, index, x.v.abs())
    n = torch.bincount(index, minlength=n_out).double().view(-1, *([1] * (x.v.dim() - 1)))
    c = c + n * a
    if mean:
        v, c = v / n.clamp(min=1), c / n.clamp(min=1)
        c = c + v.abs()
    return Tracked(v, c)


def ratio(got, t: Tracked, what: str = '', unit: float = UNIT32, tol: float = 1e-5) -> float:
    """max |got - t.v| / (unit * t.c) over the entries with t.c > 0; where t.c == 0, `got` must equal t.v exactly.  One [cw]
    line per call: the ratio, where it is attained, and what tests/_product.gate would have said of the same pair."""
    g = _d(got)
    assert g.shape == t.v.shape, (what, tuple(g.shape), tuple(t.v.shape))
    assert bool(torch.isfinite(g).all()), f'{what}: a non-finite result'
    err = (g - t.v).abs()
    live = t.c > 0
    exact = bool((err[~live] == 0).all())
    if not bool(live.any()):
        print(f'[cw] {what}: no entry carries an error bound; exact = {exact}')
        assert exact, f'{what}: an entry without a rounding differs from the reference'
        return 0.0
    q = torch.where(live, err / (unit * t.c).clamp(min=1e-300), torch.zeros_like(err))
    at = int(q.argmax())
    r = float(q.view(-1)[at])
    where = tuple(int(i) for i in torch.unravel_index(torch.tensor(at), q.shape)) if q.dim() else ()
    top, worst = max(1.0, float(t.v.abs().max())), float(err.max())
    print(f'[cw] {what}: ratio = {r:.3g} at {where} (|v| = {float(t.v.abs().view(-1)[at]):.3g}, c = {float(t.c.view(-1)[at]):.3g}); '
          f'gate: max|delta| = {worst:.3e} against {tol * top:.3e} -> {"passes" if worst <= tol * top else "FAILS"}')
    assert exact, f'{what}: an entry without a rounding differs from the reference'
    return r


def measure(got, ref_of, n_acc_of, cpu32, what: str, unit: float = UNIT32, margin: float = MARGIN):
    """The figures of (R) and (E) for one result, nothing asserted but the shapes and the exact entries.  ref_of(steps) builds
    the Tracked reference, `steps(K)` giving the accumulation steps of a product with K terms: `n_acc_of` for (R), one for (E).
    `cpu32`: the float32 CPU restatement's result (None: (R) only, the float64 kernels).  Returns (ratio of (R), ratio of (E),
    limit of (E), ratio of the restatement)."""
    r = ratio(got, ref_of(n_acc_of), what + ' (R)', unit)
    if cpu32 is None:
        return r, None, None, None
    one = ref_of(lambda K: 1)
    rc = ratio(cpu32, one, what + ' float32 torch on the CPU', unit)
    e = ratio(got, one, what + ' (E)', unit)
    limit = margin * max(1.0, rc)
    print(f'[cw] {what}: (E) {e:.3g} against {margin:g} * max(1, {rc:.3g}) = {limit:.3g}')
    return r, e, limit, rc


def check(got, ref_of, n_acc_of, cpu32, what: str, unit: float = UNIT32, margin: float = MARGIN):
    """(R) and (E) asserted; returns measure()'s figures."""
    r, e, limit, rc = measure(got, ref_of, n_acc_of, cpu32, what, unit, margin)
    assert r <= RIGOROUS, f'{what}: (R) ratio {r:.3g} > {RIGOROUS:g}'
    assert e is None or e <= limit, f'{what}: (E) ratio {e:.3g} > {limit:.3g}'
    return r, e, limit, rc


FMA = lambda K: K               # an fma or fp32-MFMA chain
SPLIT = lambda K: 6 * K         # the six-plane bf16 split (csrc/cwn_split.h)


# ---------------------------------------------------------------------------------------------------------------------------
# graded operands
# ---------------------------------------------------------------------------------------------------------------------------
def _grade(n: int, step: int, period: int, low: int) -> torch.Tensor:
    return torch.ldexp(torch.ones(n), (torch.arange(n) * step) % period - low)


def grade_rows(M: int) -> torch.Tensor:
    return _grade(M, 7, 25, 12)


def grade_cols(N: int) -> torch.Tensor:
    return _grade(N, 11, 25, 12)


def grade_inner(K: int) -> torch.Tensor:
    return _grade(K, 5, 17, 8)


def graded(X, W, b=None, rows=True, cols=True, inner=True):
    """X [M, K], W [N, K], b [N] with the grades applied: rows of X; the contraction index of X and its inverse on W; rows of
    W and the bias.  All powers of two: every product is the ungraded one times 2^e, |e| <= 24 + 16."""
    M, K = X.shape
    N = W.size(0)
    gr = grade_rows(M) if rows else torch.ones(M)
    gc = grade_cols(N) if cols else torch.ones(N)
    gk = grade_inner(K) if inner else torch.ones(K)
    Xg = X * gr[:, None] * gk[None, :]
    Wg = W * gc[:, None] / gk[None, :]
    return Xg, Wg, (None if b is None else b * gc)


def equivariant(got_graded, got_plain, row_grade, col_grade, what: str) -> None:
    """Bit-identity of the output on graded operands with the output on the plain ones times the grades."""
    g = got_graded.detach().cpu()
    want = got_plain.detach().cpu()
    if row_grade is not None:
        want = want * row_grade.to(want.dtype)[:, None]
    if col_grade is not None:
        want = want * col_grade.to(want.dtype)[None, :]
    bad = int((g != want).sum())
    print(f'[cw] {what}: equivariance under power-of-two grades: {bad} of {g.numel()} elements differ')
    assert torch.equal(g, want), f'{what}: {bad} elements change under power-of-two grading'


def grade_ratio(N: int) -> torch.Tensor:
    """Per column |mean| / spread = 2^(5n mod 13), 1 ... 4096, negative in every third column."""
    n = torch.arange(N)
    return torch.ldexp(torch.ones(N), (5 * n) % 13) * torch.where(n % 3 == 2, -1.0, 1.0)


def graded_z(g, M: int, N: int, rows: bool = False) -> torch.Tensor:
    """A pre-activation [M, N] as a graded Linear leaves it: column n has spread grade_cols(N)[n] and mean grade_ratio(N)[n]
    spreads; with `rows` the deviations carry grade_rows(M) as well (the column's mean then stands far above most of them)."""
    d = torch.randn(M, N, generator=g)
    if rows:
        d = d * grade_rows(M)[:, None]
    return (d + grade_ratio(N)[None, :]) * grade_cols(N)[None, :]


# ---------------------------------------------------------------------------------------------------------------------------
# normalisation: BatchNorm1d(train) as csrc/cwn_norm.hip, cwn_bn_live.h and the stage kernels state it, LayerNorm as
# csrc/cwn_layernorm.hip does.  A c is, as everywhere above, a magnitude times the number of roundings that can reach it.
# ---------------------------------------------------------------------------------------------------------------------------
F64_IN_F32 = 2.0 ** -29          # one float64 rounding in units of a float32 one


def col_sum(x: Tracked, steps) -> Tracked:
    """The sum over the rows, bounded order-free as segment_sum is: the sources' c plus steps(rows) times the sum of their |v|
    (steps = FMA: rows; any order of any tree, LDS partials, slots and atomics included)."""
    return Tracked(x.v.sum(0), x.c.sum(0) + steps(x.v.size(0)) * x.v.abs().sum(0))


@dataclass
class BnStats:
    M: int
    mean: Tracked         # [N]: the float64 mean rounded to float32
    var: Tracked          # [N]: the biased variance (never stored; `fp64` is what reaches rstd and the running variance of it)
    rstd: Tracked         # [N]: 1 / sqrt(var + eps) rounded to float32
    fp64: torch.Tensor    # [N]: the float64 arithmetic's own error in var (sum y^2 / M - mean^2 cancels), in float32 units


def bn_stats(z, eps: float, steps) -> BnStats:
    """Column mean over the M rows, biased variance and rstd of a float32 matrix z (an input: what the launch itself stored).
    The kernels sum y and y^2 in float64 and finalize in float64, so each of the three is the exact value rounded ONCE -- plus
    what float64 loses in sum y^2 / M - mean^2: (depth + 2) float64 roundings of E y^2 + 2 |mean| E|y|, which at
    |mean| / spread = 4096 is 2^24 times the variance.  depth = the additions one term can pass through: at most steps(M), and
    in every form at most 64 inside its workgroup's row tile (32 or 64 rows) plus one per 32-row band of the matrix, whatever
    the order between the tiles (band partials summed by the finalize launch, or atomics into the slots)."""
    zv = _d(z)
    M = zv.size(0)
    mean = zv.mean(0)
    var = ((zv - mean) ** 2).mean(0)
    w = F64_IN_F32 * (min(steps(M), 64 + (M + 31) // 32) + 2)
    fp64 = w * ((zv * zv).mean(0) + 2 * mean.abs() * zv.abs().mean(0))
    e = float(torch.tensor(eps, dtype=torch.float32))                     # eps as the descriptor holds it
    rstd = 1.0 / torch.sqrt(var + e)
    return BnStats(M, Tracked(mean, mean.abs() + w * zv.abs().mean(0)), Tracked(var, var.abs() + fp64),
                   Tracked(rstd, rstd.abs() * (1 + 2 * F64_IN_F32) + fp64 * rstd ** 3 / 2), fp64)


def bn_affine(z, st: BnStats, gamma, beta):
    """(scale, shift, y) of the folded affine: scale = gamma rstd, shift = beta - mean scale, y = z scale + shift, every
    operation a float32 one (a contraction into an fma only removes a rounding)."""
    one = torch.ones_like(st.mean.v)
    scale = mul(inp(one if gamma is None else gamma), st.rstd)
    shift = sub(inp(0 * one if beta is None else beta), mul(st.mean, scale))
    return scale, shift, add(mul(inp(z), scale), shift)


def bn_running(prev, new: Tracked, momentum: float) -> Tracked:
    """(1 - momentum) prev + momentum new in float32; 1 - momentum is itself a rounded float32 difference."""
    m = float(torch.tensor(momentum, dtype=torch.float32))
    return add(mul(scalar(1.0 - m, abs(1.0 - m)), inp(prev)), mul(scalar(m), new))


def bn_unbiased(st: BnStats, roundings: int) -> Tracked:
    """var M / (M - 1) (M = 1: var) as the running variance takes it: ONE rounding where float64 forms it (cwn_bn_finalize_f32),
    three where (float) var meets a float32 quotient (cwn_bn_live.h)."""
    f = st.M / (st.M - 1.0) if st.M > 1 else 1.0
    v = st.var.v * f
    return Tracked(v, st.fp64 * f + roundings * v.abs())


def sign_disputed(y: Tracked, unit: float = UNIT32) -> torch.Tensor:
    """The entries where float32 and float64 may disagree about the sign of y: |v| <= 4 unit c.  ReLU is 1-Lipschitz, so the
    forward result stays gated there; a test zeroes the incoming GRADIENT there before the launch, so that neither side's
    column sums depend on the disputed mask."""
    return y.v.abs() <= 4 * unit * y.c


def bn_backward(z, dyh, st: BnStats, scale: Tracked, steps, form: str = 'apply'):
    """(dz, s1, s2) of BatchNorm1d(train) behind dyh = dy [y > 0] (an input: the mask is settled by the caller; or Tracked):
    xhat = (z - mean) rstd, s1 = sum dyh, s2 = sum dyh xhat (order-free), 1 / M a rounded float32 reciprocal, and
        'apply'  dz = scale (dyh - s1 / M - xhat s2 / M)                        cwn_norm_bwd_apply_f32, cwn_norm_bwd_f32, bnb
        'stage'  dz = scale dyh + a0 + a1 (z - mean), a0 = -scale (s1 / M), a1 = -scale (rstd (s2 / M))    cwn_dense_stage_bwd_f32"""
    dyh = dyh if isinstance(dyh, Tracked) else inp(dyh)          # (Tracked: a gradient whose mask is disputed in places)
    xc = sub(inp(z), st.mean)
    xhat = mul(xc, st.rstd)
    s1, s2 = col_sum(dyh, steps), col_sum(mul(dyh, xhat), steps)
    inv = scalar(1.0 / st.M, 1.0 / st.M)
    if form == 'apply':
        dz = mul(scale, sub(sub(dyh, mul(s1, inv)), mul(xhat, mul(s2, inv))))
    else:
        a0, a1 = mul(scale, mul(s1, inv)), mul(scale, mul(st.rstd, mul(s2, inv)))
        dz = sub(sub(mul(scale, dyh), a0), mul(a1, xc))
    return dz, s1, s2


def _ln_centered(x: torch.Tensor, off: torch.Tensor, steps):
    """x - mu along the rows as the LayerNorm kernels reach it: e = x - m with m a float32 mean that is off by at most `off`
    ([M, 1], a magnitude), then e - mean_N(e).  Whatever m is, e - mean(e) = x - mu exactly, so m's own error never enters:
    what does is one rounding of every e (|e| <= |x - mu| + off), the N-term sum of them and the rounding of the difference.
    Returns (x - mu tracked, the bound of |e|, the c of e, the c of mean_N(e))."""
    N = x.size(1)
    d = x - x.mean(1, keepdim=True)
    mag = d.abs() + off
    c_cc = mag.mean(1, keepdim=True) * (1 + steps(N)) + off
    return Tracked(d, mag + c_cc + d.abs()), mag, mag, c_cc


def ln_forward(z, gamma, beta, eps: float, steps, relu: bool):
    """cwn_layernorm_act_f32: two-pass row statistics in float32 with the second pass's correction of the mean.  Returns a
    dict of Tracked: y (before the activation), out, mean, rstd."""
    x = _d(z)
    N = x.size(1)
    mu = x.mean(1, keepdim=True)
    off = RIGOROUS * UNIT32 * (steps(N) + 1) * x.abs().mean(1, keepdim=True)        # the first pass: an N-term sum and a division
    xc, mag, c_e, c_cc = _ln_centered(x, off, steps)
    var = (xc.v ** 2).mean(1, keepdim=True)
    c_var = (2 * mag * c_e + mag * mag).mean(1, keepdim=True) + steps(N) * (mag * mag).mean(1, keepdim=True) + 2 * var \
        + 2 * off * c_cc + off * off
    e = float(torch.tensor(eps, dtype=torch.float32))
    rstd = 1.0 / torch.sqrt(var + e)
    t_rstd = Tracked(rstd, (c_var + var + e) * rstd ** 3 / 2 + 2 * rstd)             # var + eps, sqrtf, the division
    one = torch.ones(N, dtype=torch.float64)
    y = add(mul(mul(xc, t_rstd), inp(one if gamma is None else gamma)), inp(0 * one if beta is None else beta))
    return dict(y=y, out=act(y, 'relu') if relu else y, mean=Tracked(mu[:, 0], (c_cc + mu.abs())[:, 0]),
                rstd=Tracked(rstd[:, 0], t_rstd.c[:, 0]))


def ln_backward(z, dyh, gamma, fwd: dict, steps):
    """cwn_layernorm_bwd_f32 behind dyh = dy [out > 0] (an input): g = dyh gamma, d = z - mean (the STORED float32 mean, off by
    what `fwd['mean']` allows), c = mean_N(d), k1 = mean_N(g), k2 = rstd (sum g d - c sum g) / N, xhat = (d - c) rstd,
    dz = rstd (g - k1 - xhat k2); dbeta = sum_m dyh, dgamma = sum_m dyh xhat (order-free).  Returns (dz, dgamma, dbeta)."""
    x, dyh = _d(z), inp(dyh)
    M, N = x.shape
    off = (RIGOROUS * UNIT32 * fwd['mean'].c)[:, None]
    xc, mag, c_e, c_cc = _ln_centered(x, off, steps)
    rstd = Tracked(fwd['rstd'].v[:, None], fwd['rstd'].c[:, None])
    g = dyh if gamma is None else mul(dyh, inp(gamma))
    rs = lambda t: t.sum(1, keepdim=True)
    sg = Tracked(rs(g.v), rs(g.c) + steps(N) * rs(g.v.abs()))
    k1 = Tracked(sg.v / N, sg.c / N + sg.v.abs() / N)
    T = rs(g.v * xc.v)
    c_T = rs(g.c * mag + g.v.abs() * c_e + g.v.abs() * mag) + steps(N) * rs(g.v.abs() * mag) \
        + c_cc * sg.v.abs() + off * sg.c + off * sg.v.abs() + T.abs()
    k2v = rstd.v * T / N
    k2 = Tracked(k2v, (c_T * rstd.v + T.abs() * rstd.c) / N + 2 * k2v.abs())
    xhat = mul(xc, rstd)
    dz = mul(rstd, sub(sub(g, k1), mul(xhat, k2)))
    return dz, col_sum(mul(dyh, xhat), steps), col_sum(dyh, steps)


# ---------------------------------------------------------------------------------------------------------------------------
# torch emulations (the CPU twins of the kernels' arithmetic)
# ---------------------------------------------------------------------------------------------------------------------------
def planes(x: torch.Tensor):
    """(hi, mid, lo) of csrc/cwn_split.h: bf16 numbers held in float32, round to nearest even at each step."""
    x = x.detach().cpu().float()
    hi = x.bfloat16().float()
    mid = (x - hi).bfloat16().float()
    lo = (x - hi - mid).bfloat16().float()
    return hi, mid, lo


def split_product(X, W, terms: int = 6) -> torch.Tensor:
    """X W^T as the kept bf16 piece products accumulated in float32, smallest first (mfma_split6); terms = 3 keeps
    hi*hi + hi*mid + mid*hi only: a split that lost its second order."""
    (xh, xm, xl), (wh, wm, wl) = planes(X), planes(W)
    order = [(xh, wl), (xl, wh), (xm, wm), (xh, wm), (xm, wh), (xh, wh)]
    out = torch.zeros(X.size(0), W.size(0))
    for a, b in (order if terms == 6 else order[3:]):
        out = out + a @ b.t()
    return out


def _f32(x) -> torch.Tensor:
    return torch.tensor(x, dtype=torch.float32)


BN_ALTERED = ('sums_fp32', 'squares_fp32', 'capacity', 'biased_running', 'shift_mean')


def bn_forward_twin(z, gamma, beta, eps, running_mean, running_var, momentum, alter=None, cap=None, live=False):
    """cwn_bn_finalize_f32 + cwn_norm_act_f32 (no activation) in torch on the CPU: float64 column sums of y and of float64
    squares, float64 finalize, one rounding to the float32 rstd, the float32 folded affine.  `live`: the running variance as
    cwn_bn_live.h forms it (float32 var times a float32 quotient).  `alter` (BN_ALTERED), each a way to get it wrong:
      sums_fp32       both column sums accumulated in float32
      squares_fp32    y * y formed in float32 ahead of a float64 sum
      capacity        1 / M from `cap`, the rows the buffer holds, not the rows that exist
      biased_running  the running variance fed the biased variance
      shift_mean      shift = beta - mean' scale with mean' the column sum over `cap` while scale and rstd use M"""
    z = z.detach().cpu().float()
    M = z.size(0)
    zd = z.double()
    if alter == 'sums_fp32':
        s, sq = z.sum(0).double(), (z * z).sum(0).double()
    elif alter == 'squares_fp32':
        s, sq = zd.sum(0), (z * z).double().sum(0)
    else:
        s, sq = zd.sum(0), (zd * zd).sum(0)
    Md = float(cap if alter == 'capacity' else M)
    mean = s / Md
    var = (sq / Md - mean * mean).clamp(min=0.0)
    rstd = (1.0 / torch.sqrt(var + _f32(eps).double())).float()
    scale = gamma * rstd
    mean_shift = (s / float(cap)) if alter == 'shift_mean' else mean
    shift = beta - mean_shift.float() * scale
    out = z * scale + shift
    mom = _f32(momentum)
    grow = 1.0 if (M <= 1 or alter == 'biased_running') else None
    if live:
        unb = var.float() * (_f32(float(M)) / _f32(float(M - 1)) if grow is None else _f32(1.0))
    else:
        unb = (var * (M / (M - 1.0) if grow is None else 1.0)).float()
    rm = (1.0 - mom) * running_mean + mom * mean.float()
    rv = (1.0 - mom) * running_var + mom * unb
    return dict(out=out, scale=scale, shift=shift, mean=mean.float(), rstd=rstd, running_mean=rm, running_var=rv)


def bn_backward_twin(z, dyh, scale, mean, rstd, form='apply', alter=None):
    """The BatchNorm backward of bn_backward's two forms in float32 torch; sums in torch's float32 order.  `alter`:
      drop_xhat_term  the xhat s2 / M term left out of the column with the smallest grade
      dgamma_short    s2 without the last row"""
    z, dyh = z.detach().cpu().float(), dyh.detach().cpu().float()
    M, N = z.shape
    xc = z - mean
    xhat = xc * rstd
    s1, p = dyh.sum(0), dyh * xhat
    s2 = p[:-1].sum(0) if alter == 'dgamma_short' else p.sum(0)
    inv = _f32(1.0) / _f32(float(M))
    keep = torch.ones(N)
    if alter == 'drop_xhat_term':
        keep[int(grade_cols(N).argmin())] = 0.0
    if form == 'apply':
        dz = scale * (dyh - s1 * inv - xhat * (s2 * inv) * keep)
    else:
        a0, a1 = -scale * (s1 * inv), -scale * (rstd * (s2 * inv))
        dz = scale * dyh + a0 + a1 * keep * xc
    return dz, s1, s2


def ln_forward_twin(z, gamma, beta, eps, relu, alter=None):
    """cwn_layernorm_act_f32 in float32 torch.  alter = 'no_correction': the second pass does not take the mean of the
    deviations out again (plain two-pass statistics around a rounded mean)."""
    z = z.detach().cpu().float()
    fN = _f32(float(z.size(1)))
    mean = z.sum(1, keepdim=True) / fN
    d = z - mean
    c = d.sum(1, keepdim=True) / fN
    var = (d * d).sum(1, keepdim=True) / fN - c * c
    if alter == 'no_correction':
        c, var = torch.zeros_like(c), (d * d).sum(1, keepdim=True) / fN
    var = var.clamp(min=0.0)
    rstd = 1.0 / torch.sqrt(var + _f32(eps))
    y = (d - c) * rstd
    y = y if gamma is None else y * gamma
    y = y if beta is None else y + beta
    return dict(out=torch.relu(y) if relu else y, mean=(mean + c)[:, 0], rstd=rstd[:, 0])


def ln_backward_twin(z, dyh, gamma, mean, rstd):
    """cwn_layernorm_bwd_f32 in float32 torch behind dyh = dy [out > 0]: (dz, dgamma, dbeta)."""
    z, dyh = z.detach().cpu().float(), dyh.detach().cpu().float()
    fN = _f32(float(z.size(1)))
    d = z - mean[:, None]
    g = dyh if gamma is None else dyh * gamma
    rs = lambda t: t.sum(1, keepdim=True)
    c, k1 = rs(d) / fN, rs(g) / fN
    k2 = rstd[:, None] * (rs(g * d) - c * rs(g)) / fN
    xhat = (d - c) * rstd[:, None]
    return rstd[:, None] * (g - k1 - xhat * k2), (dyh * xhat).sum(0), dyh.sum(0)
