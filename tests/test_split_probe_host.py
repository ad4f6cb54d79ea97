"""The probes of tests/_split_probe.py can see what they are for -- checked on the CPU model of the split, no GPU.

For every operand class, at the shapes tests/test_gpu_split_terms.py multiplies: the six-term model equals the int64 product
exactly; removing any one term the class exercises, or moving any one non-zero plane of either operand by one position along
the contraction index, changes at least half of the non-zero outputs.  A GPU test that asserts torch.equal on these inputs
therefore fails for a kernel with one of those faults.  The shares are properties of the inputs: if one comes out low, the
inputs change, not the threshold."""
import pytest
import torch

from tests import _split_probe as P

MIN_SHARE = 0.5


def test_pools_hold_what_they_are_named_for():
    for name, (has_mid, has_lo) in (('one', (False, False)), ('two', (True, False)), ('three', (True, True))):
        vals = P.pool(name)
        _, mid, lo = P.split(vals.float())
        assert vals.numel() and bool((vals > 0).any()) and bool((vals < 0).any())
        assert bool((mid != 0).all()) == has_mid and bool((mid == 0).all()) == (not has_mid), name
        assert bool((lo != 0).all()) == has_lo and bool((lo == 0).all()) == (not has_lo), name
    # round to nearest makes pieces of either sign by itself
    _, mid, lo = P.split(P.pool('three').float())
    assert bool((mid > 0).any()) and bool((mid < 0).any()) and bool((lo > 0).any()) and bool((lo < 0).any())
    # no integer of 17 bits has a third piece (why `three` is 18 bits wide)
    assert not bool(P.split(torch.arange(1 << 16, 1 << 17).float())[2].any())


def _fault_matrix(cls, name, X, W, ref):
    """One printed line per fault; X / W are the operands as emulate takes them."""
    assert torch.equal(P.emulate(X, W), ref), f'{name} class {cls}: the six-term model is not the exact product'
    faults = [('drop', t) for t in P.CLASS_TERMS[cls]] + [('roll', r) for r in P.CLASS_PLANES[cls]]
    for kind, f in faults:
        got = P.emulate(X, W, drop=f) if kind == 'drop' else P.emulate(X, W, roll=f)
        share = P.changed_share(got, ref)
        label = f'drop {f}' if kind == 'drop' else f'roll {f[0]}{f[1]}'
        print(f'[fault matrix] {name:18s} class {cls}  {label:12s} changes {share:6.1%} of the non-zero outputs')
        assert share >= MIN_SHARE, (name, cls, label, share)
    # a term the class does not exercise is zero: dropping it changes nothing
    for t in P.TERMS:
        if t not in P.CLASS_TERMS[cls]:
            assert torch.equal(P.emulate(X, W, drop=t), ref), (name, cls, t)


@pytest.mark.parametrize('name', sorted(P.SHAPES))
@pytest.mark.parametrize('cls', ['A', 'B', 'C'])
def test_probe_sees_every_term_and_plane(cls, name):
    M, N, K, nnz = P.SHAPES[name]
    p = P.make_case(cls, M, N, K, nnz=nnz, seed=1, cap=P.LAYER_CAP_C if cls == 'C' and name.startswith('layer') else 0)
    assert torch.equal(p.ref, (p.Xi @ p.Wi.t()).double())
    _fault_matrix(cls, name, p.X, p.W, p.ref)


@pytest.mark.parametrize('name', sorted(P.TN_SHAPES))
@pytest.mark.parametrize('cls', ['A', 'B', 'C'])
def test_weight_gradient_probe_sees_every_term_and_plane(cls, name):
    M, N, K = P.TN_SHAPES[name]
    p = P.make_tn_case(cls, M, N, K, seed=3)
    # (the class's X pool is the dense operand here: emulate's X is X^T [K, M], its W is dZ^T [N, M], the result dW^T)
    _fault_matrix(cls, name, p.X.t().contiguous(), p.dZ.t().contiguous(), p.ref().t().contiguous())
    assert torch.equal(p.ref_db(), p.dZi.sum(0).double())


@pytest.mark.parametrize('cls', ['A', 'B', 'C'])
def test_scaled_probe_stays_exact_and_sensitive(cls):
    """A power of two on every row of X and of W: the model is still exact, the reference scales with it, the faults show."""
    M, N, K, nnz = P.SHAPES['gemm']
    p = P.make_case(cls, M, N, K, nnz=nnz, seed=1, scaled=True)
    assert int(p.ex.min()) >= -30 and int(p.ex.max()) <= 30 and p.ex.unique().numel() > 8
    assert torch.equal(p.ref, p.scaled_like_ref(p.Xi @ p.Wi.t()))
    for piece in P.split(p.X) + P.split(p.W):
        nz = piece[piece != 0].abs()
        assert not nz.numel() or float(nz.min()) >= 2.0 ** -126          # every piece a normal number
    _fault_matrix(cls, 'gemm (scaled)', p.X, p.W, p.ref)
    t = P.make_tn_case(cls, 1024, 128, 128, seed=3, scaled=True)
    _fault_matrix(cls, 'gemm_tn (scaled)', t.X.t().contiguous(), t.dZ.t().contiguous(), t.ref().t().contiguous())


def test_exactness_condition_rejects_inputs_beyond_it():
    g = torch.Generator().manual_seed(0)
    X = P.sparse_rows('three', 64, 128, 8, g)
    with pytest.raises(AssertionError, match='dropped term'):
        P.assert_exact(X, P.draw('three', (16, 128), g))              # lo * lo exists
    with pytest.raises(AssertionError, match='2\\^24'):
        P.assert_exact(X * 4, P.draw('one', (16, 128), g))            # 8 * 3 * 2^20 > 2^24
