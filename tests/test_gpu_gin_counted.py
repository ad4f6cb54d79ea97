"""The counted GIN layers on the device: ops.gin_layer_counted / ops.gine_layer_counted (cwn_gin_layer_dev_f32 /
cwn_gine_layer_dev_f32: the kernels of the host-count entries with the live row count read on the device) against the
host-count ops on the operands TRIMMED to the live rows -- bit for bit: a live row's bits depend neither on the count, nor on
the capacity, nor on what lies behind the count.

Capacity 70 rows (three tiles of CWN_GIN_TM = 32); live counts 0, 1, 31, 32, 33, 64, 69, 70, a count of 75 (clamped to the
capacity: the full launch) and a count of -3 (nothing is written).  Widths (5, 12) -- the element-by-element loads and stores
-- (12, 128), (64, 64), (128, 128).  The graph over the live rows has a hub row of 11 entries (the folds go four entries at a
time plus a tail), a row without entries and rows of 1 .. 3 entries.

Everything behind the count is poisoned with values that stay INSIDE the buffers, so that a wrong kernel fails an assertion
and cannot fault: rows [live, cap) of x are NaN, the rows of e that only dead entries name are NaN, rowptr[r] for r > live is
the live entry count (what cwn_csr_build leaves there under its e_dev), col / eidx behind the live entries are 0, and out is
pre-filled with a sentinel bit pattern that must survive in every row from the count on and beside a column-slice out."""
import pytest
import torch

from cwn_amd import _ffi, csr, ops
from tests.test_gpu_gin import EPS, TM, XSCALE, _operands

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CAP = 70
E_PAD = 13                                  # capacity entries behind the live ones
# (the count the device holds, the rows the operands are live for, the rows the launch must serve)
COUNTS = [(0, 0, 0), (1, 1, 1), (31, 31, 31), (32, 32, 32), (33, 33, 33), (64, 64, 64), (69, 69, 69), (70, 70, 70), (75, 70, 70),
          (-3, 33, 0)]
WIDTHS = [(5, 12), (12, 128), (64, 64), (128, 128)]
SENTINEL = 0x5A5AC3C3
# (act, act_post, out is a column slice of a wider buffer, n_dev handed over as an address)
SETTINGS = [('relu', 'id', False, False), ('tanh', 'tanh', False, True), ('relu', 'id', True, False)]
HUB = 11

assert TM == 32 and CAP == 2 * TM + 6


def _live_index(L: int) -> torch.Tensor:
    """COO [2, E] over L live rows in shuffled entry order: row 0 a hub of HUB entries, row 1 without entries, row r >= 2 with
    1 + r % 3 entries; sources anywhere in [0, L)."""
    if L == 0:
        return torch.zeros(2, 0, dtype=torch.long)
    g = torch.Generator().manual_seed(900 + L)
    deg = torch.tensor([HUB] + [0] * (L > 1) + [1 + r % 3 for r in range(2, L)])
    dst = torch.repeat_interleave(torch.arange(L), deg)
    src = torch.randint(0, L, (int(deg.sum()),), generator=g)
    p = torch.randperm(dst.numel(), generator=g)
    return torch.stack([src[p], dst[p]])


class _CapacityPlan(csr.Adjacency):
    """A plan over CAP rows and E_live + E_PAD entries as a csr-mode slot of a static batch holds it after a fill with L live rows:
    the live rows' plan in front, rowptr[r] = E_live for every r > L, col / aux / perm behind the live entries 0."""

    def __init__(self, live, L: int, n_aux_cap: int):
        E = live.n_entries if live is not None else 0
        self.key = self.val = self.aux_index = None
        self.n_entries, self.n_dst, self.n_val, self.n_aux = E + E_PAD, CAP, CAP, n_aux_cap
        self.device = DEV
        self.rowptr = torch.full((CAP + 1,), E, dtype=torch.int32, device=DEV)
        self.col, self.aux, self.perm = (torch.zeros(E + E_PAD, dtype=torch.int32, device=DEV) for _ in range(3))
        if live is not None:
            self.rowptr[:L + 1] = live.rowptr
            self.col[:E], self.aux[:E], self.perm[:E] = live.col, live.aux, live.perm
        self.long_cap, self.long_rows, self.n_long = 1, None, None
        self.built, self.ready = True, None
        self._t_src = self._t_aux = None
        self._counts = None


_GRAPHS = {}


def _graph(L: int):
    """(live plan or None, capacity plan, live edge cells n_e, live entries E) of the L-live-row case, built once."""
    if L not in _GRAPHS:
        idx = _live_index(L)
        n_e = max(1, L // 2) if L else 0
        live = None
        if L:
            shared = torch.randint(0, n_e, (idx.size(1),), generator=torch.Generator().manual_seed(70 + L))
            live = csr.Adjacency.from_index(idx.to(DEV), L, L, shared.to(DEV), n_e)
            deg = torch.bincount(idx[1], minlength=L)
            assert int(deg[0]) >= 9 and (L < 2 or int(deg[1]) == 0) and (L < 5 or {1, 2, 3} <= set(deg[2:].tolist()))
        _GRAPHS[L] = (live, _CapacityPlan(live, L, CAP // 2 + 3), n_e, int(idx.size(1)))
    return _GRAPHS[L]


def _sentinel(rows: int, cols: int) -> torch.Tensor:
    buf = torch.empty(rows, cols, device=DEV)
    buf.view(torch.int32).fill_(SENTINEL)
    return buf


def _kept(t: torch.Tensor) -> bool:
    return bool((t.contiguous().view(torch.int32) == SENTINEL).all())


@pytest.mark.parametrize('kind', ['gin', 'gine-aux', 'gine-perm'])
@pytest.mark.parametrize('w,H', WIDTHS)
def test_counted_launch_equals_the_host_count_launch_on_the_trimmed_operands(w, H, kind):
    x, stages = _operands(w, H, CAP, 31 * w + H)
    sd = [tuple(t.to(DEV) for t in s) for s in stages]
    eps = torch.tensor([EPS], device=DEV)
    mode = kind[5:] or None
    g = torch.Generator().manual_seed(5 * w + H)
    for count, L, served in COUNTS:
        live, cap_plan, n_e, E = _graph(L)
        xd = torch.full((CAP, w), float('nan'), device=DEV)             # rows [L, CAP): NaN
        xd[:L] = x[:L].to(DEV)
        if mode is not None:
            rows_live, rows_cap = (n_e, cap_plan.n_aux) if mode == 'aux' else (E, cap_plan.n_entries)
            ed = torch.full((rows_cap, w), float('nan'), device=DEV)    # the rows only dead entries name: NaN
            ed[:rows_live] = (XSCALE * torch.randn(rows_live, w, generator=g)).to(DEV)
        n_dev = torch.tensor([count], dtype=torch.int64, device=DEV)
        for act, post, sliced, as_address in SETTINGS:
            if L == 0:
                ref = torch.empty(0, H, device=DEV)
            elif mode is None:
                ref = ops.gin_layer(xd[:L], live, eps, sd, act, post)
            else:
                ref = ops.gine_layer(xd[:L], live, ed[:rows_live], eps, sd, act, post, edge_mode=mode)
            assert L == 0 or bool(torch.isfinite(ref).all())
            buf = _sentinel(CAP, H + 8 if sliced else H)
            out = buf[:, 4:4 + H] if sliced else buf
            n_arg = n_dev.data_ptr() if as_address else n_dev
            if mode is None:
                got = ops.gin_layer_counted(xd, cap_plan, eps, sd, act, post, out=out, n_dev=n_arg)
            else:
                got = ops.gine_layer_counted(xd, cap_plan, ed, eps, sd, act, post, out=out, edge_mode=mode, n_dev=n_arg)
            what = f'{kind} w={w} H={H} count={count} live={L} act={act} post={post} sliced={sliced}'
            assert got.data_ptr() == out.data_ptr(), what
            assert torch.equal(out[:served], ref[:served]), what
            assert _kept(out[served:]), f'{what}: a row from the count on was written'
            if sliced:
                assert _kept(buf[:, :4]) and _kept(buf[:, 4 + H:]), f'{what}: an element beside the out slice was written'


def test_counted_ops_run_inside_dynamic_rows_and_the_host_count_ops_still_refuse():
    """ops.gin_layer_counted brings its own count: it runs under _ffi.dynamic_rows (a static batch), where ops.gin_layer
    declines as before."""
    x, stages = _operands(12, 128, CAP, 3)
    sd = [tuple(t.to(DEV) for t in s) for s in stages]
    live, cap_plan, _, _ = _graph(33)
    xd = x.to(DEV)
    n_dev = torch.tensor([33], dtype=torch.int64, device=DEV)
    ref = ops.gin_layer(xd[:33], live, None, sd, 'relu')
    out = _sentinel(CAP, 128)
    with _ffi.dynamic_rows({CAP: n_dev.data_ptr()}):
        ops.gin_layer_counted(xd, cap_plan, None, sd, 'relu', out=out, n_dev=n_dev)
        with pytest.raises(RuntimeError, match='does not run under _ffi.dynamic_rows'):
            ops.gin_layer(xd, cap_plan, None, sd, 'relu')
    assert torch.equal(out[:33], ref) and _kept(out[33:])
    with pytest.raises(TypeError, match='n_dev'):
        ops.gin_layer_counted(xd, cap_plan, None, sd, 'relu', n_dev=torch.tensor([33], dtype=torch.int64))     # a CPU count
    with pytest.raises(TypeError, match='float64'):
        ops.gin_layer_counted(xd.double(), cap_plan, None, sd, 'relu', n_dev=n_dev)
