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
