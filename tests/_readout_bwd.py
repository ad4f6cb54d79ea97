"""The three readout-backward launches of a training step -- cwn_head_bwd_f32, cwn_target_head_bwd_f32, cwn_flow_head_bwd_f32 /
_bwd_dev_f32 -- as tests/_bounds.py holds a forward: graded operands, a float64 reference that carries its own error bound, a
float32 restatement in torch on the CPU (the TWIN of the kernel's arithmetic, which can also be told to get it wrong), and the
assertions themselves.  tests/test_gpu_readout_bwd_componentwise.py runs the assertions over the kernels,
tests/test_readout_bwd_host.py over the twins: they accept the right one and reject every seeded fault.

Grades (powers of two, tests/_bounds.py): a contracted index is graded on one operand and inversely on the other -- the outputs
o and the hidden units j of the pooled heads, the classes k and the complexes c of the target head; a free index is graded
directly -- the complexes / cochains (rows of the incoming gradient), the hidden units of dh_out, the output columns.
The ReLU mask comes from `h`, an OPERAND of these launches, so it is exact: every entry of h is either at least 2^-10 in
magnitude or an exact +0.0 / -0.0 (the documented `h > 0` decides those, and nothing else can tell `h > 0` from `h >= 0`)."""
from dataclasses import dataclass
from typing import List, Optional

import torch

from tests import _bounds as B

HEAD_THREADS = 512                                  # kHeadThreads of csrc/cwn_ends.hip
# cells per complex and dimension: SIZES of tests/test_gpu_componentwise.py (complex 2 is empty, some have one cell) and a sixth
# complex of 300 cells in every dimension (more than one 128-row chunk, more rows than any row group takes in one pass)
SIZES = ([9, 37, 0, 23, 1], [12, 40, 0, 30, 4], [1, 11, 0, 3, 0])
HEAD_SIZES = tuple(s + [300] for s in SIZES)
FLOW_ROWS = [0, 1, 127, 128, 129, 300]              # rows per cochain: the edges of the 128-row chunks and an idle slot
ONE = lambda K: 1                                   # (E): one step per product


def ptr_of(sizes) -> torch.Tensor:
    return torch.cat([torch.zeros(1, dtype=torch.long), torch.tensor(list(sizes), dtype=torch.long).cumsum(0)])


def owner_of(ptr: torch.Tensor) -> torch.Tensor:
    """Row -> its complex / cochain."""
    return torch.repeat_interleave(torch.arange(ptr.numel() - 1), ptr[1:] - ptr[:-1])


def counts_of(ptr: torch.Tensor) -> torch.Tensor:
    return ptr[1:] - ptr[:-1]


def mask_operand(g, rows: int, cols: int) -> torch.Tensor:
    """A pre-activation [rows, cols]: no entry within 2^-10 of zero but three exact zeros (+0.0 first and in the middle, -0.0
    last), whose gradient is zero by `h > 0`."""
    z = torch.randn(rows, cols, generator=g)
    h = torch.where(z < 0, z - 2.0 ** -10, z + 2.0 ** -10)
    flat = h.view(-1)
    flat[0], flat[flat.numel() // 2], flat[-1] = 0.0, 0.0, -0.0
    return h


def select(t: B.Tracked, keep: torch.Tensor) -> B.Tracked:
    """t where `keep`, else 0: a select rounds nothing."""
    m = keep.double()
    return B.Tracked(t.v * m, t.c * m)


def cached(fn):
    """ref_of(steps) for B.check that builds each of its two references (the kernel's steps, one step) once."""
    memo = {}

    def ref_of(steps):
        key = steps(2)
        if key not in memo:
            memo[key] = fn(steps)
        return memo[key]
    return ref_of


class Worst:
    """The largest (R) and (E) ratios of a launch over the checks of one test, printed as one [cw] line."""

    def __init__(self, launch: str):
        self.launch, self.r, self.e = launch, 0.0, 0.0

    def take(self, figures):
        r, e, _, _ = figures
        self.r, self.e = max(self.r, r), max(self.e, e or 0.0)

    def report(self, what: str):
        print(f'[cw] {self.launch} {what}: largest (R) = {self.r:.3g}, largest (E) = {self.e:.3g}')


# ---------------------------------------------------------------------------------------------------------------------------
# cwn_head_bwd_f32
# ---------------------------------------------------------------------------------------------------------------------------
@dataclass
class HeadCase:
    K: int
    H2: int
    O: int
    mean: bool
    mean_final: bool
    ptrs: List[torch.Tensor]            # int64 [C + 1] per dimension
    h: List[torch.Tensor]               # [C, H2] per dimension: the mask operand
    plain: tuple                        # (g [C, O], w2 [O, H2], [w1_d [H2, K]]) without grades
    graded: tuple
    row_grade: torch.Tensor             # [C]
    hid_grade: torch.Tensor             # [H2]
    col_grade: torch.Tensor             # [K]

    @property
    def C(self) -> int:
        return self.ptrs[0].numel() - 1

    @property
    def n_dims(self) -> int:
        return len(self.ptrs)


def head_case(K, H2, O, mean, mean_final=False, sizes=HEAD_SIZES, seed=0) -> HeadCase:
    g = torch.Generator().manual_seed(seed + K + 3 * H2 + 7 * O + 11 * mean + 13 * mean_final + 17 * len(sizes))
    ptrs = [ptr_of(s) for s in sizes]
    C = len(sizes[0])
    go = torch.randn(C, O, generator=g)
    w2 = torch.randn(O, H2, generator=g) / H2 ** 0.5
    w1 = [torch.randn(H2, K, generator=g) / K ** 0.5 for _ in sizes]
    h = [mask_operand(g, C, H2) for _ in sizes]
    gr, gi_o, gi_h, gc = B.grade_rows(C), B.grade_inner(O), B.grade_inner(H2), B.grade_cols(K)
    graded = (go * gr[:, None] * gi_o[None, :], w2 * gi_h[None, :] / gi_o[:, None], [w * gc[None, :] / gi_h[:, None] for w in w1])
    return HeadCase(K, H2, O, bool(mean), bool(mean_final), ptrs, h, (go, w2, w1), graded, gr, gi_h, gc)


def head_ref(case: HeadCase, steps):
    """([dx_d], [dh_d]) tracked.  Steps read from head_bwd_kernel: ds is one fma chain over the O outputs; dpooled is a chain over
    the j of one of S = 512 / (K / 4) slices (at most H2 steps) and the S slice partials added one after the other."""
    g, w2, w1 = case.graded
    S = HEAD_THREADS // (case.K // 4)
    ds = B.linear(B.inp(g), w2.t(), None, steps(case.O))
    if case.mean_final:
        ds = B.div(ds, B.scalar(case.n_dims))
    dxs, dhs = [], []
    for d in range(case.n_dims):
        dh = select(ds, case.h[d] > 0)
        dp = B.linear(dh, w1[d].t(), None, steps(case.H2 + S))
        if case.mean:
            dp = B.div(dp, B.inp(counts_of(case.ptrs[d]).clamp(min=1)[:, None]))
        dxs.append(B.rows(dp, owner_of(case.ptrs[d])))
        dhs.append(dh)
    return dxs, dhs


HEAD_ALTERED = ('stale_512', 'mask_ge', 'mean_unclamped', 'mean_final_twice')


def head_twin(case: HeadCase, operands=None, alter: Optional[str] = None):
    """([dx_d], [dh_d]) in float32 torch on the CPU.  `alter` (HEAD_ALTERED), each a way to get it wrong:
      stale_512         columns >= 512 of dpooled keep what the buffer held (here: the previous complex's)
      mask_ge           the mask h >= 0 instead of h > 0
      mean_unclamped    the mean readout's divisor not clamped to 1 for a complex without cells
      mean_final_twice  the final mean's divisor applied twice"""
    assert alter is None or alter in HEAD_ALTERED
    g, w2, w1 = operands if operands is not None else case.graded
    nd = torch.tensor(float(case.n_dims))
    ds = g @ w2
    if case.mean_final:
        ds = ds / nd
        if alter == 'mean_final_twice':
            ds = ds / nd
    dxs, dhs = [], []
    for d in range(case.n_dims):
        keep = case.h[d] >= 0 if alter == 'mask_ge' else case.h[d] > 0
        dh = torch.where(keep, ds, torch.zeros_like(ds))
        dp = dh @ w1[d]
        if case.mean:
            n = counts_of(case.ptrs[d]).float()[:, None]
            dp = dp / (n if alter == 'mean_unclamped' else n.clamp(min=1))
        if alter == 'stale_512':
            dp = torch.cat([dp[:, :512], dp.roll(1, 0)[:, 512:]], 1)
        dxs.append(dp[owner_of(case.ptrs[d])])
        dhs.append(dh)
    return dxs, dhs


def head_row_grade(case: HeadCase, d: int) -> torch.Tensor:
    return case.row_grade[owner_of(case.ptrs[d])]


def check_head(case: HeadCase, dxs, dhs, what: str, plain=None, worst: Optional[Worst] = None):
    """(R) and (E) of every dx (None: a dimension whose data gradient was not asked for) and every dh_out; with `plain` =
    (dxs, dhs) of the launch on the operands without grades, the equivariance as well."""
    ref = cached(lambda s: head_ref(case, s))
    cpu_dx, cpu_dh = head_twin(case)
    worst = worst or Worst('cwn_head_bwd_f32')
    for d in range(case.n_dims):
        worst.take(B.check(dhs[d], lambda s: ref(s)[1][d], B.FMA, cpu_dh[d], f'{what} dh_out[{d}]'))
        if dxs[d] is not None:
            worst.take(B.check(dxs[d], lambda s: ref(s)[0][d], B.FMA, cpu_dx[d], f'{what} dx[{d}]'))
        if plain is not None:
            B.equivariant(dhs[d], plain[1][d], case.row_grade, case.hid_grade, f'{what} dh_out[{d}]')
            if dxs[d] is not None:
                B.equivariant(dxs[d], plain[0][d], head_row_grade(case, d), case.col_grade, f'{what} dx[{d}]')
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# cwn_target_head_bwd_f32
# ---------------------------------------------------------------------------------------------------------------------------
TARGET_STAGE = 64                                   # kStage of csrc/cwn_target_head.hip: complexes per group of dW / db


@dataclass
class TargetCase:
    H: int
    K: int
    C: int
    N: int
    rows: torch.Tensor                  # int32 [C] ascending; three complexes share one row (C >= 4); the last sits in row N - 1
    plain: tuple                        # (dlogits [C, K], W [K, H], x [N, H]): the grades of the complexes only
    graded: tuple
    cls_grade: torch.Tensor             # [K]: on the columns of dlogits, inversely on the rows of W; the rows of dW, db
    dx_grade: torch.Tensor              # [H]: the columns of W, so of dx
    dw_grade: torch.Tensor              # [H]: the columns of x, so of dW


def target_case(H, K, C, seed=0) -> TargetCase:
    g = torch.Generator().manual_seed(seed + H + 3 * K + 7 * C)
    N = 3 * C + 2
    N += N % 64 == 0
    rows = torch.arange(C) * 3 + 1
    if C >= 4:
        j = (C - 3) // 2
        rows[j + 1] = rows[j + 2] = rows[j]
    rows[C - 1] = N - 1                              # in the last, partial chunk of 64 rows
    assert N % 64 != 0 and bool((rows[1:] >= rows[:-1]).all())
    dl, W, x = torch.randn(C, K, generator=g), torch.randn(K, H, generator=g) / K ** 0.5, torch.randn(N, H, generator=g)
    # the complexes are free in dx and contracted in dW / db: dlogits rows carry their grade, the target rows of x its inverse
    gr = B.grade_rows(C)
    first = torch.ones(N)
    first[rows.flip(0)] = gr.flip(0)                 # (a shared row: its first complex's)
    dl, x = dl * gr[:, None], x / first[:, None]
    gk, gh, gw = B.grade_inner(K), B.grade_cols(H), B.grade_cols(H).flip(0)
    graded = (dl * gk[None, :], W * gh[None, :] / gk[:, None], x * gw[None, :])
    return TargetCase(H, K, C, N, rows.to(torch.int32), (dl, W, x), graded, gk, gh, gw)


def target_ref(case: TargetCase, steps, live: Optional[int] = None):
    """(dx, dW, db) tracked over the first `live` complexes.  Steps read from target_head_bwd_kernel: a dx row is ONE chain
    over the K classes of every complex that shares it; an element of dW / db a chain over the complexes of a group of 64 and
    the groups' partials added one after the other (C + groups bounds both)."""
    C = case.C if live is None else live
    dl, W, x = case.graded
    dl, rows = dl[:C], case.rows[:C].long()
    run = torch.bincount(rows, minlength=case.N)[rows].double()[:, None]
    k_steps = steps(case.K)
    per = B.linear(B.inp(dl), W.t(), None, k_steps * run if k_steps != 1 else 1)
    dx = B.segment_sum(per, rows, case.N)
    n_acc = steps(C + (C + TARGET_STAGE - 1) // TARGET_STAGE)
    dW = B.linear(B.inp(dl.t()), x[rows].t(), None, n_acc)
    db = B.linear(B.inp(dl.t()), torch.ones(1, C), None, n_acc)
    return dx, dW, db


TARGET_ALTERED = ('shared_once', 'db_capacity')


def target_twin(case: TargetCase, operands=None, live: Optional[int] = None, alter: Optional[str] = None):
    """(dx, dW, db [K, 1]) in float32 torch on the CPU.  `alter` (TARGET_ALTERED):
      shared_once   a row that several complexes share takes the first of them, not their sum
      db_capacity   db summed over the capacity, not the live count"""
    assert alter is None or alter in TARGET_ALTERED
    C = case.C if live is None else live
    dl_all, W, x = operands if operands is not None else case.graded
    dl, rows = dl_all[:C], case.rows[:C].long()
    per = dl @ W
    if alter == 'shared_once':
        dx = torch.zeros(case.N, case.H)
        dx[rows.flip(0)] = per.flip(0)
    else:
        dx = torch.zeros(case.N, case.H).index_add_(0, rows, per)
    db = (dl_all if alter == 'db_capacity' else dl).sum(0)
    return dx, dl.t() @ x[rows], db[:, None]


def check_target(case: TargetCase, dx, dW, db, what: str, plain=None, live: Optional[int] = None, worst: Optional[Worst] = None):
    """(R) and (E) of dx, dW, db; rows of dx without a target exactly zero; with `plain` = (dx, dW, db) of the launch on
    case.plain, the equivariance under the class and column grades."""
    C = case.C if live is None else live
    ref = cached(lambda s: target_ref(case, s, live))
    cpu = target_twin(case, live=live)
    worst = worst or Worst('cwn_target_head_bwd_f32')
    no_target = torch.ones(case.N, dtype=torch.bool)
    no_target[case.rows[:C].long()] = False
    assert not bool(dx.detach().cpu()[no_target].any()), f'{what}: a row of dx without a target is not zero'
    db = db.detach().cpu().view(-1, 1)
    for k, (got, name) in enumerate(((dx, 'dx'), (dW, 'dW'), (db, 'db'))):
        worst.take(B.check(got, lambda s: ref(s)[k], B.FMA, cpu[k], f'{what} {name}'))
    if plain is not None:
        B.equivariant(dx, plain[0], None, case.dx_grade, f'{what} dx')
        B.equivariant(dW, plain[1], case.cls_grade, case.dw_grade, f'{what} dW')
        B.equivariant(db, plain[2].detach().cpu().view(-1, 1), case.cls_grade, None, f'{what} db')
    return worst


# ---------------------------------------------------------------------------------------------------------------------------
# cwn_flow_head_bwd_f32 / _bwd_dev_f32
# ---------------------------------------------------------------------------------------------------------------------------
@dataclass
class FlowCase:
    K: int
    H: int
    O: int
    take_abs: bool
    mean: bool
    ptr: torch.Tensor                   # int64 [C + 1]
    h: torch.Tensor                     # [C, H]: the mask operand
    x: torch.Tensor                     # [N, K]: only its signs enter (take_abs); rows of both signs and all grades, +0.0 and -0.0
    plain: tuple                        # (g [C, O], W1 [H, K], W2 [O, H])
    graded: tuple
    row_grade: torch.Tensor             # [C]
    hid_grade: torch.Tensor             # [H]
    col_grade: torch.Tensor             # [K]

    @property
    def C(self) -> int:
        return self.ptr.numel() - 1

    @property
    def N(self) -> int:
        return int(self.ptr[-1])


def flow_case(K, H, O, take_abs, mean, sizes=FLOW_ROWS, seed=0) -> FlowCase:
    g = torch.Generator().manual_seed(seed + K + 3 * H + 7 * O + 11 * take_abs + 13 * mean)
    ptr = ptr_of(sizes)
    C, N = len(sizes), int(ptr[-1])
    go, W1, W2 = torch.randn(C, O, generator=g), torch.randn(H, K, generator=g) / K ** 0.5, torch.randn(O, H, generator=g) / H ** 0.5
    h = mask_operand(g, C, H)
    x = torch.randn(N, K, generator=g).abs() * (B.grade_rows(N) * torch.where(torch.arange(N) % 3 == 1, -1.0, 1.0))[:, None]
    x[torch.rand(N, K, generator=g) < 0.25] *= -1.0
    flat = x.view(-1)
    flat[0::7], flat[3::11] = 0.0, -0.0              # exact zeros of both signs: their dx is exactly 0 under take_abs
    gr, gi_o, gi_h, gc = B.grade_rows(C), B.grade_inner(O), B.grade_inner(H), B.grade_cols(K)
    graded = (go * gr[:, None] * gi_o[None, :], W1 * gc[None, :] / gi_h[:, None], W2 * gi_h[None, :] / gi_o[:, None])
    return FlowCase(K, H, O, bool(take_abs), bool(mean), ptr, h, x, (go, W1, W2), graded, gr, gi_h, gc)


def flow_trimmed(case: FlowCase, live: int) -> FlowCase:
    """The first `live` cochains of `case` as a case of their own: what a counted launch computes."""
    cut = lambda ops_: (ops_[0][:live],) + tuple(ops_[1:])
    return FlowCase(case.K, case.H, case.O, case.take_abs, case.mean, case.ptr[:live + 1], case.h[:live], case.x[:int(case.ptr[live])],
                    cut(case.plain), cut(case.graded), case.row_grade[:live], case.hid_grade, case.col_grade)


def _sgn(case: FlowCase, zero_is_one: bool = False) -> torch.Tensor:
    if not case.take_abs:
        return torch.ones_like(case.x)
    return torch.where(case.x < 0, -1.0, 1.0) if zero_is_one else torch.sign(case.x)


def flow_ref(case: FlowCase, steps):
    """(dx, dh) tracked.  Steps read from flow_head_bwd_small_kernel: one fma chain over o for ds, one over j for dpooled."""
    g, W1, W2 = case.graded
    ds = B.linear(B.inp(g), W2.t(), None, steps(case.O))
    dh = select(ds, case.h > 0)
    dp = B.linear(dh, W1.t(), None, steps(case.H))
    if case.mean:
        dp = B.div(dp, B.inp(counts_of(case.ptr).clamp(min=1)[:, None]))
    dx = B.rows(dp, owner_of(case.ptr))
    sg = _sgn(case).double()
    return B.Tracked(dx.v * sg, dx.c * sg.abs()), dh


FLOW_ALTERED = ('sgn_zero_one', 'mask_ge', 'mean_unclamped')


def flow_twin(case: FlowCase, operands=None, alter: Optional[str] = None):
    """(dx, dh) in float32 torch on the CPU.  `alter` (FLOW_ALTERED): sgn_zero_one -- sgn(+-0) = 1 instead of 0; mask_ge and
    mean_unclamped as head_twin's."""
    assert alter is None or alter in FLOW_ALTERED
    g, W1, W2 = operands if operands is not None else case.graded
    ds = g @ W2
    dh = torch.where(case.h >= 0 if alter == 'mask_ge' else case.h > 0, ds, torch.zeros_like(ds))
    dp = dh @ W1
    if case.mean:
        n = counts_of(case.ptr).float()[:, None]
        dp = dp / (n if alter == 'mean_unclamped' else n.clamp(min=1))
    return dp[owner_of(case.ptr)] * _sgn(case, alter == 'sgn_zero_one'), dh


def check_flow(case: FlowCase, dx, dh, what: str, plain=None, worst: Optional[Worst] = None):
    """(R) and (E) of dx and dh_out (an entry of dx at x = +-0 under take_abs carries no bound: exactly 0); with `plain` =
    (dx, dh) of the launch on case.plain, the equivariance."""
    ref = cached(lambda s: flow_ref(case, s))
    cpu = flow_twin(case)
    worst = worst or Worst('cwn_flow_head_bwd_f32')
    worst.take(B.check(dh, lambda s: ref(s)[1], B.FMA, cpu[1], f'{what} dh_out'))
    worst.take(B.check(dx, lambda s: ref(s)[0], B.FMA, cpu[0], f'{what} dx'))
    if plain is not None:
        B.equivariant(dh, plain[1], case.row_grade, case.hid_grade, f'{what} dh_out')
        B.equivariant(dx, plain[0], case.row_grade[owner_of(case.ptr)], case.col_grade, f'{what} dx')
    return worst
