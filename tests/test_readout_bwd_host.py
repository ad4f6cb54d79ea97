"""tests/_readout_bwd.py on the CPU: the assertions of tests/test_gpu_readout_bwd_componentwise.py accept a float32 twin of each
readout backward and CAN fail (the twin of tests/test_bounds_host.py for these launches).

  * the twins of cwn_head_bwd_f32, cwn_target_head_bwd_f32 and cwn_flow_head_bwd_f32 pass (R), (E) and the equivariance;
  * each seeded fault is rejected: head dx columns >= 512 left stale, the mask h >= 0, the final mean's divisor applied twice,
    a shared target row taken once, db summed over the capacity, sgn(+-0) = 1;
  * one dx entry of the smallest-grade rows off by 2^-18 relative is rejected, and tests/_product.gate accepts it: the gap;
  * a mean divisor left unclamped for a complex without cells changes NO output of a backward (such a complex has no row of dx,
    and dh_out is formed ahead of the division): the one seeded fault these launches cannot show, stated as such."""
import pytest
import torch

from tests import _bounds as B
from tests import _readout_bwd as R
from tests._product import gate

HEAD_SHAPES = [(20, 12, 3), (64, 128, 2), (512, 4, 1), (516, 8, 1), (640, 128, 2), (1024, 64, 1), (2048, 512, 2)]
REJECTED = r'\(R\) ratio|\(E\) ratio|differs from the reference|non-finite|is not zero'


# ---- cwn_head_bwd_f32 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mean', [False, True], ids=['sum', 'mean'])
@pytest.mark.parametrize('K,H2,O', HEAD_SHAPES)
def test_head_twin_passes(K, H2, O, mean):
    case = R.head_case(K, H2, O, mean, mean_final=mean)
    dxs, dhs = R.head_twin(case)
    R.check_head(case, dxs, dhs, f'head twin K={K} H2={H2} O={O}', plain=R.head_twin(case, case.plain))
    # the operands do what the module says: no entry of h within 2^-10 of zero but exact zeros of both signs; dx spans the grades
    for h in case.h:
        assert float(h.abs()[h != 0].min()) >= 2.0 ** -10 and int((h == 0).sum()) == 3
    v = R.head_ref(case, B.FMA)[0][0].v.abs()
    assert float(v.max()) / float(v[v > 0].min()) > 2.0 ** 24


@pytest.mark.parametrize('mean', [False, True], ids=['sum', 'mean'])
@pytest.mark.parametrize('K,H2,O', [(516, 8, 1), (640, 128, 2), (2048, 512, 2)])
def test_head_stale_columns_beyond_512_are_rejected(K, H2, O, mean):
    case = R.head_case(K, H2, O, mean)
    dxs, dhs = R.head_twin(case, alter='stale_512')
    with pytest.raises(AssertionError, match=REJECTED):
        R.check_head(case, dxs, dhs, f'head K={K}: columns >= 512 stale')
    # ... and up to 512 there is nothing to leave out
    narrow = R.head_case(512, 4, 1, mean)
    for a, b in zip(R.head_twin(narrow, alter='stale_512')[0], R.head_twin(narrow)[0]):
        assert torch.equal(a, b)


@pytest.mark.parametrize('K,H2,O', [(20, 12, 3), (64, 128, 2)])
def test_head_mask_ge_is_rejected(K, H2, O):
    case = R.head_case(K, H2, O, mean=True)
    dxs, dhs = R.head_twin(case, alter='mask_ge')
    with pytest.raises(AssertionError, match='differs from the reference'):      # dh_out at h = +-0: an entry without a rounding
        R.check_head(case, dxs, dhs, 'head: mask h >= 0')
    with pytest.raises(AssertionError, match=REJECTED):                          # ... and dx alone shows it too
        R.check_head(case, dxs, R.head_twin(case)[1], 'head: mask h >= 0, dx alone')


@pytest.mark.parametrize('n_dims', [2, 3])
def test_head_mean_final_twice_is_rejected(n_dims):
    case = R.head_case(64, 128, 2, mean=True, mean_final=True, sizes=R.HEAD_SIZES[:n_dims])
    dxs, dhs = R.head_twin(case, alter='mean_final_twice')
    with pytest.raises(AssertionError, match=REJECTED):
        R.check_head(case, dxs, dhs, f'head: / n_dims twice, {n_dims} dimensions')


def test_an_unclamped_mean_divisor_changes_no_output_of_a_backward():
    """dpooled / 0 of a complex without cells is broadcast to no row: dx and dh_out are the same bits.  (The FORWARD's clamp is
    held by test_head of tests/test_gpu_componentwise.py: the empty complex pools to zeros.)"""
    case = R.head_case(64, 128, 2, mean=True)
    assert int((R.counts_of(case.ptrs[0]) == 0).sum()) == 1
    for a, b in zip(sum(R.head_twin(case, alter='mean_unclamped'), []), sum(R.head_twin(case), [])):
        assert torch.equal(a, b)
    flow = R.flow_case(20, 12, 3, True, True)
    assert int((R.counts_of(flow.ptr) == 0).sum()) == 1
    for a, b in zip(R.flow_twin(flow, alter='mean_unclamped'), R.flow_twin(flow)):
        assert torch.equal(a, b)


def _small_entry(ref_one: B.Tracked, rows: torch.Tensor):
    """Among `rows` of a reference built with one step per product, the entry with the largest |v| / c."""
    q = torch.where(ref_one.c > 0, ref_one.v.abs() / ref_one.c.clamp(min=1e-300), torch.zeros_like(ref_one.c))[rows]
    at = int(q.argmax())
    return int(rows[at // q.size(1)]), at % q.size(1), float(q.view(-1)[at])


@pytest.mark.parametrize('mean', [False, True], ids=['sum', 'mean'])
def test_head_one_small_entry_off_by_2_to_the_minus_18_is_rejected_and_passes_the_max_norm_gate(mean):
    case = R.head_case(512, 4, 1, mean)
    dxs, dhs = R.head_twin(case)
    ref = R.head_ref(case, R.ONE)[0][0]
    small = int(case.row_grade.argmin())
    rows = torch.nonzero(R.owner_of(case.ptrs[0]) == small).view(-1)
    r, k, room = _small_entry(ref, rows)
    assert room > 1.0 / 8, room              # (E)'s limit is 8 x 2^-24 c at least: 2^-18 |v| has to stand above it
    dxs[0] = dxs[0].clone()
    dxs[0][r, k] *= 1.0 + 2.0 ** -18
    gate(dxs[0], ref.v, 'head dx with one small entry off by 2^-18: the max-norm gate')             # accepts
    assert float(ref.v[r, k].abs()) < 2.0 ** -8 * float(ref.v.abs().max())
    with pytest.raises(AssertionError, match=r'\(R\) ratio|\(E\) ratio'):
        R.check_head(case, dxs, dhs, 'head dx with one small entry off by 2^-18')


# ---- cwn_target_head_bwd_f32 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Cn', [1, 64, 65, 129])
@pytest.mark.parametrize('H,K', [(4, 1), (60, 5), (68, 17), (512, 64)])
def test_target_twin_passes(H, K, Cn):
    case = R.target_case(H, K, Cn)
    R.check_target(case, *R.target_twin(case), f'target twin H={H} K={K} C={Cn}', plain=R.target_twin(case, case.plain))
    shared = torch.bincount(case.rows.long()).max()
    assert int(shared) == (3 if Cn >= 4 else 1) and int(case.rows[-1]) == case.N - 1 and case.N % 64 != 0


def test_target_twin_passes_beyond_4096_complexes_and_counted():
    big = R.target_case(4, 2, 4100)
    R.check_target(big, *R.target_twin(big), 'target twin C=4100')
    case = R.target_case(68, 17, 130)
    for live in (70, 3):
        R.check_target(case, *R.target_twin(case, live=live), f'target twin capacity 130, live {live}', live=live)


@pytest.mark.parametrize('Cn', [64, 129])
def test_target_shared_row_taken_once_is_rejected(Cn):
    case = R.target_case(68, 17, Cn)
    with pytest.raises(AssertionError, match=REJECTED):
        R.check_target(case, *R.target_twin(case, alter='shared_once'), 'target: a shared row taken once')


@pytest.mark.parametrize('live', [70, 3])
def test_target_db_over_the_capacity_is_rejected(live):
    case = R.target_case(68, 17, 130)
    with pytest.raises(AssertionError, match=REJECTED):
        R.check_target(case, *R.target_twin(case, live=live, alter='db_capacity'), 'target: db over the capacity', live=live)


# ---- cwn_flow_head_bwd_f32 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mean', [False, True], ids=['sum', 'mean'])
@pytest.mark.parametrize('take_abs', [True, False], ids=['abs', 'signed'])
@pytest.mark.parametrize('K,H,O', [(1, 1, 1), (3, 5, 2), (20, 12, 3), (128, 128, 64)])
def test_flow_twin_passes(K, H, O, take_abs, mean):
    case = R.flow_case(K, H, O, take_abs, mean)
    R.check_flow(case, *R.flow_twin(case), f'flow twin K={K} H={H} O={O}', plain=R.flow_twin(case, case.plain))
    zeros = case.x == 0
    assert bool(zeros.any()) and bool(torch.signbit(case.x[zeros]).any()) and not bool(torch.signbit(case.x[zeros]).all())
    assert bool((case.x < 0).any()) and bool((case.x > 0).any())
    live = R.flow_trimmed(case, 4)
    R.check_flow(live, *R.flow_twin(live), f'flow twin K={K} H={H} O={O}, four cochains')


@pytest.mark.parametrize('K,H,O', [(3, 5, 2), (128, 128, 64)])
def test_flow_sgn_of_zero_is_rejected(K, H, O):
    case = R.flow_case(K, H, O, True, True)
    with pytest.raises(AssertionError, match='differs from the reference'):
        R.check_flow(case, *R.flow_twin(case, alter='sgn_zero_one'), 'flow: sgn(+-0) = 1')


def test_flow_mask_ge_is_rejected():
    case = R.flow_case(20, 12, 3, True, False)
    with pytest.raises(AssertionError, match=REJECTED):
        R.check_flow(case, *R.flow_twin(case, alter='mask_ge'), 'flow: mask h >= 0')


def test_flow_one_small_entry_off_by_2_to_the_minus_18_is_rejected_and_passes_the_max_norm_gate():
    case = R.flow_case(3, 5, 2, False, False)
    dx, dh = R.flow_twin(case)
    ref = R.flow_ref(case, R.ONE)[0]
    counts = R.counts_of(case.ptr)
    small = int(torch.where(counts > 0, case.row_grade, torch.full_like(case.row_grade, float('inf'))).argmin())
    rows = torch.nonzero(R.owner_of(case.ptr) == small).view(-1)
    r, k, room = _small_entry(ref, rows)
    assert room > 1.0 / 8, room
    dx = dx.clone()
    dx[r, k] *= 1.0 + 2.0 ** -18
    gate(dx, ref.v, 'flow dx with one small entry off by 2^-18: the max-norm gate')                 # accepts
    with pytest.raises(AssertionError, match=r'\(R\) ratio|\(E\) ratio'):
        R.check_flow(case, dx, dh, 'flow dx with one small entry off by 2^-18')
