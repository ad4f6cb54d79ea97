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


# ---------------------------------------------------------------------------------------------------------------------------
# Adam, one launch (tests/_adam.py): the gates of tests/test_gpu_adam_componentwise.py over numpy float32
# ---------------------------------------------------------------------------------------------------------------------------
from tests import _adam as A          # noqa: E402


def test_elementwise_tracked_forms():
    """mul, div, sqrt, power and sub bound float32 results on graded operands, and see a relative error of 2^-20."""
    g = torch.Generator().manual_seed(4)
    a = (torch.rand(300, generator=g) + 0.5) * B._grade(300, 7, 41, 20)
    b = (torch.rand(300, generator=g) + 0.5) * B._grade(300, 11, 41, 20) * (torch.randint(0, 2, (300,), generator=g) * 2.0 - 1)
    forms = {'mul': (a * b, B.mul(B.inp(a), B.inp(b))), 'div': (a / b, B.div(B.inp(a), B.inp(b))),
             'sqrt': (a.sqrt(), B.sqrt(B.inp(a))), 'sub': (a - b, B.sub(B.inp(a), B.inp(b))),
             'sqrt of a product': ((a * a).sqrt(), B.sqrt(B.mul(B.inp(a), B.inp(a)))),
             'scaled': (a * 0.75, B.mul(B.scalar(0.75), B.inp(a))),
             'cube': (a * a * a, B.power(B.inp(a), 3.0))}
    for name, (got, t) in forms.items():
        assert got.dtype == torch.float32
        assert B.ratio(got, t, name) <= (B.RIGOROUS if name != 'cube' else 2 * B.RIGOROUS)      # (a a a: two roundings for power's one)
        assert B.ratio(got * (1 + 2.0 ** -20), t, name + ' times 1 + 2^-20') > B.RIGOROUS
    s = B.scalar(0.1)
    assert float(s.c) == 0.0 and s.v.dtype == torch.float64 and float(B.scalar(2.0, 3.0).c) == 3.0


@pytest.mark.parametrize('hyper', A.HYPERS, ids=A.HYPER_IDS)
def test_adam_operands_are_graded_and_normal(hyper):
    p, g, m, v = A.operands(4099, hyper)
    tiny = 2.0 ** -120
    assert float(g.abs().min()) < 2.0 ** -39 and 2.0 ** 9 <= float(g.abs().max()) < 2.0 ** 10
    assert float(p.abs().min()) < 2.0 ** -19 and 0.5 <= float(p.abs().max()) < 1.0
    for x in (p, g, m, v, (1 - A.f32(hyper[1])) * g.double() * g.double()):
        assert float(x.abs().min()) > tiny
    m1, v1, p1 = A.reference(p, g, m, v, 1, hyper)
    eps = A.f32(A.EPS)
    # sqrt(v') on both sides of eps: far below it without weight decay; with it wd |p| >= 2^-27 is a floor under |gr|
    assert float(v1.v.sqrt().min()) < eps * (2.0 ** -10 if hyper[2] == 0 else 1.0) and float(v1.v.sqrt().max()) > eps * 2.0 ** 20
    gr = g.double() + A.f32(hyper[2]) * p.double()
    opposite = (m.double() * gr) < 0
    assert 0.3 < float(opposite.double().mean()) < 0.7                    # b1 m and (1 - b1) gr of opposite sign
    assert float(((p1.v - p.double()).abs() > p.double().abs() * 2.0 ** -10).double().mean()) > 0.3        # the update is visible in p'


@pytest.mark.parametrize('t', A.STEPS)
@pytest.mark.parametrize('hyper', A.HYPERS, ids=A.HYPER_IDS)
def test_adam_float32_restatement_passes_both_gates(hyper, t):
    """The kernel's formula in numpy float32 meets (R) on the moments and (E) on the parameter at every size, with room: (R)
    with 2x to spare (measured 0.95 at the most), and its own p' ratio stays below 1, so the limit of (E) is MARGIN."""
    for n in A.SIZES:
        ops = A.operands(n, hyper)
        good = A.restatement(*ops, t, hyper)
        rm, rv, e, limit, rc = A.check(good, A.reference(*ops, t, hyper), good, f'Adam restatement {hyper} t={t} n={n}')
        assert rm <= B.RIGOROUS / 2 and rv <= B.RIGOROUS / 2 and rc <= 1.0 and limit == B.MARGIN, (rm, rv, rc)


def _altered_cases():
    """(alteration, hyper, t, n) at which the alteration changes the float32 result at all: decoupled decay needs wd > 0; in
    float32 sqrt(1 - b2^t) is 1 from t = 1e5 on (and 1 - 4e-5 at b2 = 0.99, t = 1000), where eps / bc2_sqrt is eps and the
    corrections at t and t - 1 coincide; a tail exists where n % 4 != 0; the eps variants need elements with sqrt(v') below eps,
    which a handful of elements need not hold."""
    out = []
    for hyper in A.HYPERS:
        for t in A.STEPS:
            short = t <= 10 or (t == 1000 and hyper[1] == 0.999)
            out.append(('eps_in_root', hyper, t, 4099))
            if short:
                out.append(('eps_over_bc2', hyper, t, 4099))
            if short and t >= 2:
                out.append(('bias_at_t_minus_1', hyper, t, 4099))
            if hyper[2] > 0:
                out.append(('decoupled_wd', hyper, t, 4099))
            out += [('tail_unwritten', hyper, t, n) for n in A.SIZES if n % 4]
    return out


def test_adam_altered_restatements_fail():
    """Every wrong Adam of ALTERED is refused by the gates that pass the restatement, wherever it differs from it in float32
    (_altered_cases) -- the p'-only ones by (E) alone, asserted at 10x the limit (measured: bias corrections at t - 1 = 999,
    beta2 = 0.999: ratio 412 against 8; everywhere else above 9e3).

    What the parameter gate these tests stand beside (tests/test_gpu_parity.py::test_flat_adam_matches_torch_adam: float32
    torch.optim.Adam, rtol 2e-5 + atol 2e-6, five steps on randn parameters, gradients randn * 10^(it - 2), betas (0.9, 0.99),
    wd 0.01) makes of the same alterations is measured by test_what_the_old_parameter_gate_makes_of_the_alterations below."""
    for alt, hyper, t, n in _altered_cases():
        ops = A.operands(n, hyper)
        good, bad = A.restatement(*ops, t, hyper), A.restatement(*ops, t, hyper, alter=alt)
        fig = A.judge(bad, A.reference(*ops, t, hyper), good, f'Adam {alt} {hyper} t={t} n={n}')
        assert not A.passes(fig), (alt, hyper, t, n, fig)
        rm, rv, e, limit, rc = fig
        if alt in ('eps_in_root', 'eps_over_bc2', 'bias_at_t_minus_1'):
            assert rm <= B.RIGOROUS and rv <= B.RIGOROUS and e > 10 * limit, (alt, hyper, t, n, fig)
        if alt in ('decoupled_wd', 'tail_unwritten'):
            assert rm > B.RIGOROUS and rv > B.RIGOROUS, (alt, hyper, t, n, fig)


def _old_gate(alter, first_step, n=35000):
    """tests/test_gpu_parity.py::test_flat_adam_matches_torch_adam with the restatement (altered from step `first_step` on) in
    the kernel's place: max over five steps of |p - p_torch| / (2e-6 + 2e-5 |p_torch|); <= 1 passes."""
    torch.manual_seed(0)
    p = torch.randn(n)
    q = torch.nn.Parameter(p.clone())
    ref = torch.optim.Adam([q], lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.01)
    m, v = torch.zeros(n), torch.zeros(n)
    g = torch.Generator().manual_seed(1)
    worst = 0.0
    for it in range(5):
        gr = torch.randn(n, generator=g) * 10.0 ** (it - 2)
        q.grad = gr.clone()
        ref.step()
        m, v, p = A.restatement(p, gr, m, v, it + 1, (0.9, 0.99, 0.01), lr=3e-3, alter=alter if it + 1 >= first_step else None)
        worst = max(worst, float(((p - q.data).abs() / (2e-6 + 2e-5 * q.data.abs())).max()))
    return worst


def test_what_the_old_parameter_gate_makes_of_the_alterations():
    """The old gate, emulated on the CPU over its own data (35 000 elements, as its shapes hold), in units of its tolerance:

        the restatement itself                               0.007    passes
        eps divided by bc2_sqrt along with sqrt(v)           0.08     PASSES when wrong from step 2 on (at step 1 alone it
                                                                      is refused whenever a |g| below ~1e-5 was drawn)
        eps inside the root                                  270      refused
        decoupled weight decay                               1.1e3    refused
        bias corrections at t - 1 from step 2 on             800      refused

    So on its data that gate does tell three of the four apart (its gradients randn * 1e-2 reach below sqrt(eps), and wd p is as
    large as they are); what it never sees is the moments, beta2 = 0.999, the tail path and t beyond 5.  The tail alteration
    cannot reach it: FlatGradBucket pads every parameter to a multiple of four."""
    assert _old_gate(None, 1) <= 0.1
    assert _old_gate('eps_over_bc2', 2) <= 0.5
    for alt in ('eps_in_root', 'decoupled_wd', 'bias_at_t_minus_1'):
        assert _old_gate(alt, 2) > 50, alt


# ---------------------------------------------------------------------------------------------------------------------------
# normalisation (tests/_norm_cases.py): the gates of tests/test_gpu_norm_componentwise.py over the float32 torch twins of
# csrc/cwn_norm.hip, cwn_bn_live.h, the stage backward and csrc/cwn_layernorm.hip
# ---------------------------------------------------------------------------------------------------------------------------
from tests import _norm_cases as NC          # noqa: E402

BN_SHAPES = [(M, N) for M in (33, 70, 300) for N in (64, 100)]
BN_IDS = [f'{M}x{N}' for M, N in BN_SHAPES]
FWD = ('out', 'mean', 'rstd', 'running_mean', 'running_var')


def _bn_twin(c, live=False, **kw):
    t = B.bn_forward_twin(c.z, c.gamma, c.beta, c.eps, c.rm0, c.rv0, NC.MOM, live=live, **kw)
    t['out'] = torch.relu(t['out']) if c.relu else t['out']
    return t


def _bn_cpu32(c):
    return c.cpu32()


def test_grade_ratio_and_graded_z():
    r = B.grade_ratio(40)
    m, e = torch.frexp(r.abs())
    assert bool((m == 0.5).all()) and int(e.min()) - 1 == 0 and int(e.max()) - 1 == 12
    assert bool((r[2::3] < 0).all()) and bool((r[0::3] > 0).all()) and bool((r[1::3] > 0).all())
    assert [int(x) for x in r[:4].abs()] == [1, 32, 1024, 4]
    z = B.graded_z(torch.Generator().manual_seed(0), 300, 40)
    ratio = (z.double().mean(0) / z.double().std(0)).abs() / r.abs()
    assert float(ratio.min()) > 0.8 and float(ratio.max()) < 1.25                  # the column means stand grade_ratio spreads off
    spread = z.double().std(0) / B.grade_cols(40)
    assert float(spread.min()) > 0.8 and float(spread.max()) < 1.25


def test_sign_disputed_marks_what_a_rounding_can_flip():
    y = B.Tracked(torch.tensor([1.0, 3e-7, -3e-7, 0.0, -1.0], dtype=torch.float64), torch.ones(5, dtype=torch.float64))
    assert B.sign_disputed(y).tolist() == [False, False, False, True, False]           # 4 * 2^-24 = 2.4e-7
    y.c *= 2
    assert B.sign_disputed(y).tolist() == [False, True, True, True, False]


@pytest.mark.parametrize('rows', [False, True], ids=['cols', 'rows'])
@pytest.mark.parametrize('M,N', BN_SHAPES, ids=BN_IDS)
def test_batchnorm_twins_pass_both_gates(M, N, rows):
    """The kernels' arithmetic in float32 torch -- finalize and live form of the forward, both forms of the backward -- is
    inside (R) and (E); tests/_product.gate calls the same correct `out` a failure (the [cw] lines), which is why no test used
    such inputs.  The disputed ReLU signs stay under their cap on the reference alone."""
    c = NC.BnCase(M, N, rows=rows)
    assert c.share() <= NC.DISPUTED_CAP
    cpu = _bn_cpu32(c)
    for live in (False, True):
        t = _bn_twin(c, live=live)
        what = f'batchnorm twin {"live" if live else "finalize"} {c.what}'
        NC.hold(t, lambda s: c.fwd(s, 3 if live else 1), cpu, FWD, what)
        NC.hold(t, c.fwd, None, ('scale', 'shift'), what)
    for form in ('apply', 'stage'):
        dz, s1, s2 = B.bn_backward_twin(c.z, c.dyh, t['scale'], t['mean'], t['rstd'], form)
        NC.hold(dict(dz=dz, s1=s1, s2=s2), lambda s: c.bwd(s, form), cpu, ('dz', 's1', 's2'), f'batchnorm twin backward {form} {c.what}')


def test_batchnorm_twin_at_one_row():
    """M = 1: variance 0, rstd = eps^-1/2, y = beta after a cancellation of ~1e3; torch refuses the batch, so (R) alone, and the
    backward without ReLU (a third of the signs are disputed)."""
    c = NC.BnCase(1, 64, relu=False)
    t = _bn_twin(c)
    NC.hold(t, c.fwd, None, FWD + ('scale', 'shift'), 'batchnorm twin M=1')
    dz, s1, s2 = B.bn_backward_twin(c.z, c.dyh, t['scale'], t['mean'], t['rstd'])
    NC.hold(dict(dz=dz, s1=s1, s2=s2), c.bwd, None, ('dz', 's1', 's2'), 'batchnorm twin backward M=1')
    share = float(B.sign_disputed(c.fwd(B.FMA)['y']).double().mean())
    print(f'[cw] M=1: {100 * share:.3g}% of the ReLU signs would be disputed')
    assert share > NC.DISPUTED_CAP


def _verdicts(got, ref_of, cpu, names, what):
    figs = NC.hold(got, ref_of, cpu, names, what, assert_=False)
    for name, fig in figs.items():
        print(f'[mutant] {what}: {name} caught by {NC.caught_by(fig)}')
    return figs


@pytest.mark.parametrize('alter', B.BN_ALTERED)
@pytest.mark.parametrize('M,N', BN_SHAPES, ids=BN_IDS)
def test_altered_batchnorm_forward_fails(M, N, alter):
    """Every wrong forward of BN_ALTERED is refused on the column-graded operands by the result it damages: float32 column
    sums and float32 squares by rstd, out and the running variance; a count taken from the capacity by everything; a biased
    running variance by the running variance alone; a shift from another mean by out alone.
    With the ROWS graded as well the spread of a column is that of its largest rows and |mean| / spread falls to ~1: there
    float32 squares pass both gates in places -- printed, a limit of the inputs, not asserted."""
    cap = (M + 63) // 64 * 64 if M % 64 else M + 64
    for rows in (False, True):
        c = NC.BnCase(M, N, rows=rows)
        figs = _verdicts(_bn_twin(c, alter=alter, cap=cap), c.fwd, _bn_cpu32(c), FWD, f'{alter} {c.what}')
        damaged = {'sums_fp32': ('rstd', 'out', 'running_var'), 'squares_fp32': ('rstd', 'out', 'running_var'), 'capacity': FWD,
                   'biased_running': ('running_var',), 'shift_mean': ('out',)}[alter]
        if not rows:
            for name in damaged:
                assert not NC.passes(figs[name]), (alter, name, figs[name])
        elif all(NC.passes(f) for f in figs.values()):
            print(f'[mutant] {alter} {c.what}: passes BOTH gates on every result -- beyond the method with these inputs')
        for name in set(FWD) - set(damaged):          # ... and nothing else is blamed
            if alter not in ('sums_fp32', 'squares_fp32'):
                assert NC.passes(figs[name]), (alter, name, figs[name])


@pytest.mark.parametrize('alter', ['drop_xhat_term', 'dgamma_short'])
@pytest.mark.parametrize('M,N', BN_SHAPES, ids=BN_IDS)
def test_altered_batchnorm_backward_fails(M, N, alter):
    """The xhat s2 / M term left out of the smallest-grade column, and s2 short of its last row: refused by dz (and s2).  Without
    ReLU: in the smallest-grade column eps outweighs the variance (2^-24 against 1e-5), y is beta there, and under ReLU a
    negative beta masks the whole column -- the alteration then changes nothing (printed for the ReLU cases)."""
    for relu in (False, True):
        c = NC.BnCase(M, N, relu=relu)
        t = _bn_twin(c)
        for form in ('apply', 'stage'):
            dz, s1, s2 = B.bn_backward_twin(c.z, c.dyh, t['scale'], t['mean'], t['rstd'], form, alter=alter)
            figs = _verdicts(dict(dz=dz, s1=s1, s2=s2), lambda s: c.bwd(s, form), _bn_cpu32(c), ('dz', 's1', 's2'), f'{alter} {form} {c.what}')
            if not relu:
                assert not NC.passes(figs['dz']), (alter, form, figs['dz'])
                assert NC.passes(figs['s1']) and NC.passes(figs['s2']) == (alter == 'drop_xhat_term')
            elif all(NC.passes(f) for f in figs.values()):
                col = int(B.grade_cols(N).argmin())
                assert alter == 'drop_xhat_term' and not bool(c.mask[:, col].any()), 'passes both gates with a live column'
                print(f'[mutant] {alter} {form} {c.what}: no effect, column {col} is masked entirely')


LN_SHAPES = [(M, N) for M in (33, 70) for N in (3, 100, 160, 260)]
LN_NAMES = ('out', 'mean', 'rstd', 'dz', 'dgamma', 'dbeta')


def _ln_twin(c, alter=None):
    t = B.ln_forward_twin(c.z, c.gamma, c.beta, NC.EPS, c.relu, alter=alter)
    dz, dg, db = B.ln_backward_twin(c.z, c.dy * (t['out'] > 0) if c.relu else c.dy, c.gamma, t['mean'], t['rstd'])
    t.update(dz=dz, dgamma=dg, dbeta=db)
    return t


@pytest.mark.parametrize('M,N', LN_SHAPES, ids=[f'{M}x{N}' for M, N in LN_SHAPES])
def test_layernorm_twin_passes_and_without_the_correction_fails(M, N):
    """cwn_layernorm's two-pass statistics with the second pass's correction of the mean are inside both gates on rows that
    stand up to 4096 spreads off zero; without the correction `out` leaves (R) at ratios 20 - 2000.  F.layer_norm in float32
    on the CPU is itself that far out on these rows (its ratio is the (E) limit's base), so (E) does not see it: (R) does."""
    c = NC.LnCase(M, N)
    assert c.share() <= NC.DISPUTED_CAP
    ref_of = lambda s: {**c.fwd(s), **c.bwd(s)}
    NC.hold(_ln_twin(c), ref_of, c.torch32(), LN_NAMES, f'layernorm twin {c.what}')
    figs = _verdicts(_ln_twin(c, alter='no_correction'), ref_of, c.torch32(), LN_NAMES, f'no_correction {c.what}')
    assert figs['out'][0] > B.RIGOROUS, figs['out']
