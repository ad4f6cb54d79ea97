"""tests/_bounds.py on the CPU, over torch emulations: the componentwise gates pass what is right and CAN fail (the twin of
tests/test_windows_host.py).  Operands are graded on rows, output columns and the contraction index; the shapes M x K x N are
those at which the gap of tests/_product.gate was measured:

  * a float32 matmul and the six-term split of csrc/cwn_split.h pass (R) and (E);
  * the smallest-grade output row times 1 + 2^-10 fails both, and tests/_product.gate passes it;
  * the last output column computed from K - 1 terms fails;
  * a split that keeps hi*hi + hi*mid + mid*hi only fails (E);
  * a two-stage ReLU chain in float32 passes; with the stage-1 bias dropped on the last hidden column it fails;
  * the float32 restatement alone meets (R) with at least 4x to spare."""
import pytest
import torch

from tests import _bounds as B
from tests._product import gate

SHAPES = [(70, 128, 128), (33, 24, 40), (70, 256, 128), (515, 64, 64)]          # M, K, N
IDS = ['x'.join(map(str, s)) for s in SHAPES]


def _case(M, K, N, seed=0):
    g = torch.Generator().manual_seed(seed + M + 3 * K + 7 * N)
    X, W, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    X, W, b = B.graded(X, W, b)
    ref_of = lambda steps: B.linear(B.inp(X), W, b, steps(K))
    return X, W, b, ref_of


def _smallest_row(M):
    return int(B.grade_rows(M).argmin())


@pytest.mark.parametrize('M,K,N', SHAPES, ids=IDS)
def test_graded_operands_are_powers_of_two_in_range(M, K, N):
    for gr, lo, hi in ((B.grade_rows(M), -12, 12), (B.grade_cols(N), -12, 12), (B.grade_inner(K), -8, 8)):
        m, e = torch.frexp(gr)
        assert bool((m == 0.5).all()) and int(e.min()) - 1 >= lo and int(e.max()) - 1 <= hi
    X, W, b, ref_of = _case(M, K, N)
    v = ref_of(B.FMA).v
    assert float(v.abs().max()) < 2.0 ** 45 and float(v.abs()[v != 0].min()) > 2.0 ** -45
    if M >= 25 and N >= 25:
        assert float(B.grade_rows(M).max() / B.grade_rows(M).min()) == 2.0 ** 24


@pytest.mark.parametrize('M,K,N', SHAPES, ids=IDS)
def test_float32_matmul_passes_and_the_reference_has_room(M, K, N):
    X, W, b, ref_of = _case(M, K, N)
    cpu32 = X @ W.t() + b
    what = f'float32 matmul {M}x{K}x{N}'
    B.check(cpu32, ref_of, B.FMA, cpu32, what)
    # another accumulation order of the same product: the contraction index reversed, in four chunks
    parts = [X[:, k0:k0 + (K + 3) // 4].flip(1) @ W[:, k0:k0 + (K + 3) // 4].flip(1).t() for k0 in range(0, K, (K + 3) // 4)]
    other = parts[3] + parts[2] + parts[1] + parts[0] + b
    B.check(other, ref_of, B.FMA, cpu32, what + ', another order')
    # the restatement alone: (R) with at least 4x to spare
    r = B.ratio(cpu32, ref_of(B.FMA), what + ': the restatement under (R)')
    assert r <= B.RIGOROUS / 4, r


@pytest.mark.parametrize('M,K,N', SHAPES, ids=IDS)
def test_six_term_split_passes(M, K, N):
    X, W, b, ref_of = _case(M, K, N)
    got = B.split_product(X, W) + b
    B.check(got, ref_of, B.SPLIT, X @ W.t() + b, f'six-term split {M}x{K}x{N}')


@pytest.mark.parametrize('M,K,N', SHAPES, ids=IDS)
def test_three_term_split_fails_the_empirical_gate_and_passes_the_old_one(M, K, N):
    X, W, b, ref_of = _case(M, K, N)
    got = B.split_product(X, W, terms=3) + b
    what = f'three-term split {M}x{K}x{N}'
    gate(got, ref_of(B.FMA).v, what)
    r, e, limit, rc = B.measure(got, ref_of, B.SPLIT, X @ W.t() + b, what)
    assert e > limit, (e, limit)
    with pytest.raises(AssertionError, match=r'\(E\) ratio'):
        B.check(got, ref_of, B.SPLIT, X @ W.t() + b, what)


@pytest.mark.parametrize('M,K,N', SHAPES, ids=IDS)
def test_a_perturbed_small_row_fails_both_and_passes_the_old_gate(M, K, N):
    X, W, b, ref_of = _case(M, K, N)
    cpu32 = X @ W.t() + b
    got = cpu32.clone()
    row = _smallest_row(M)
    got[row] *= 1 + 2.0 ** -10
    what = f'row {row} times 1 + 2^-10, {M}x{K}x{N}'
    gate(got, ref_of(B.FMA).v, what)                      # the max-norm gate does not see it
    r, e, limit, rc = B.measure(got, ref_of, B.FMA, cpu32, what)
    assert r > B.RIGOROUS and e > limit, (r, e, limit)
    with pytest.raises(AssertionError, match=r'\(R\) ratio'):
        B.check(got, ref_of, B.FMA, cpu32, what)


@pytest.mark.parametrize('M,K,N', SHAPES, ids=IDS)
def test_a_last_column_short_of_one_term_fails(M, K, N):
    X, W, b, ref_of = _case(M, K, N)
    cpu32 = X @ W.t() + b
    got = cpu32.clone()
    got[:, -1] = X[:, :-1] @ W[-1, :-1] + b[-1]
    what = f'last column from K - 1 terms, {M}x{K}x{N}'
    r, e, limit, rc = B.measure(got, ref_of, B.FMA, cpu32, what)
    assert r > B.RIGOROUS and e > limit, (r, e, limit)


def _chain(M, K, N, drop_bias_on_last_hidden=False):
    """relu(relu(X W1^T + b1) W2^T + b2) with a K -> N -> N shape, float32; graded rows and output columns (ReLU is positively
    homogeneous: the hidden layer carries the row grades on)."""
    g = torch.Generator().manual_seed(5 + M + K + N)
    X, W1, b1 = B.graded(torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g),
                         cols=False)
    b1 = b1 * B.grade_rows(M).min()            # (a bias at the scale of the smallest rows: it matters there and nowhere else)
    H0, W2, b2 = B.graded(torch.zeros(M, N), torch.randn(N, N, generator=g) / N ** 0.5, torch.randn(N, generator=g), rows=False)
    b1_used = b1.clone()
    if drop_bias_on_last_hidden:
        b1_used[-1] = 0
    h = torch.relu(X @ W1.t() + b1_used)
    got = torch.relu(h @ W2.t() + b2)

    def ref_of(steps):
        t = B.act(B.linear(B.inp(X), W1, b1, steps(K)), 'relu')
        return B.act(B.linear(t, W2, b2, steps(N)), 'relu')
    return got, ref_of


@pytest.mark.parametrize('M,K,N', SHAPES, ids=IDS)
def test_two_stage_relu_chain(M, K, N):
    good, ref_of = _chain(M, K, N)
    what = f'two-stage ReLU chain {M}x{K}x{N}'
    B.check(good, ref_of, B.FMA, good, what)
    bad, _ = _chain(M, K, N, drop_bias_on_last_hidden=True)
    r, e, limit, rc = B.measure(bad, ref_of, B.FMA, good, what + ', stage-1 bias dropped on the last hidden column')
    assert r > B.RIGOROUS and e > limit, (r, e, limit)


def test_exact_entries_must_be_exact():
    """Where c == 0 (an input handed through) the result equals the reference, or ratio() refuses."""
    x = torch.randn(5, 3, generator=torch.Generator().manual_seed(1))
    t = B.rows(B.inp(x), torch.tensor([4, 0, 2]))
    assert B.ratio(x[[4, 0, 2]], t, 'a gather') == 0.0
    with pytest.raises(AssertionError, match='without a rounding'):
        B.ratio(x[[4, 0, 2]] * (1 + 2.0 ** -20), t, 'a gather, perturbed')


def test_segment_forms():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(40, 8, generator=g) * B.grade_rows(40)[:, None]
    index = torch.randint(0, 6, (40,), generator=g)
    index[index == 3] = 2                                      # (an empty segment)
    for mean in (False, True):
        t = B.segment_sum(B.inp(x), index, 6, mean=mean)
        got = torch.zeros(6, 8).index_add_(0, index, x)
        if mean:
            got = got / torch.bincount(index, minlength=6).clamp(min=1)[:, None]
        assert bool((t.c[3] == 0).all()) and bool((t.v[3] == 0).all())
        assert B.ratio(got, t, f'segment {"mean" if mean else "sum"}') <= B.RIGOROUS
        bad = got.clone()
        bad[0] -= x[index == 0][0] * 2.0 ** -8
        assert B.ratio(bad, t, 'segment sum, one source short by 2^-8') > B.RIGOROUS


def test_equivariance_of_the_emulations():
    """The exact-equivariance check on the split emulation: bit-identical under all three grades, and not when the product
    hides an absolute constant."""
    g = torch.Generator().manual_seed(3)
    M, K, N = 33, 64, 40
    X, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / 8
    Xg, Wg, _ = B.graded(X, W)
    plain, grd = B.split_product(X, W), B.split_product(Xg, Wg)
    B.equivariant(grd, plain, B.grade_rows(M), B.grade_cols(N), 'split emulation')
    with pytest.raises(AssertionError, match='change under'):
        B.equivariant(grd + 1e-9, plain + 1e-9, B.grade_rows(M), B.grade_cols(N), 'split emulation with an absolute constant')
