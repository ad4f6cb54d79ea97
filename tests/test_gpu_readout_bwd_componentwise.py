"""The readout BACKWARD launches of a training step under graded operands, held entry by entry: cwn_head_bwd_f32,
cwn_target_head_bwd_f32, cwn_flow_head_bwd_f32 / _bwd_dev_f32 (tests/_readout_bwd.py builds the operands, the float64 tracked
references and the float32 restatements, and holds the assertions; tests/test_readout_bwd_host.py proves on the CPU that they
can fail).

Their own modules (test_gpu_ends.py, test_gpu_ring.py, test_gpu_flow_head.py) gate max|got - ref| by 1e-5 * |ref|_inf on randn
operands.  The outputs of these launches differ by orders of magnitude from entry to entry -- the dx rows of a mean readout are
divided by the cell count, dx of the target head is zero on most rows, dW follows the feature scale -- so every case here asserts
  (R) and (E) of tests/_bounds.check against the tracked reference and the float32 restatement, the step counts read from the
      kernels (tests/_readout_bwd.py states them);
  (equivariance) the launch is linear in the incoming gradient with the mask fixed by an operand: the bits of the launch on the
      operands without grades, times the row and column grades;
and the C entry points are called directly: a non-zero code raises, nothing passes on a fall-back.  Outputs are pre-filled with
NaN (tests/_bounds.ratio refuses a non-finite entry: every element has to be written) and carry guard rows that must keep their
value."""
import pytest
import torch

from cwn_amd import _ffi, ops
from tests import _readout_bwd as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
NAN = float('nan')
SENTINEL = -77.25


def _equal_bits(a, b, what):
    for k, (s, t) in enumerate(zip(a, b)):
        if s is None and t is None:
            continue
        assert torch.equal(s, t), f'{what}: output {k} differs in {int((s != t).sum())} of {s.numel()} elements'


# ------------------------------------------------------------------------------------------------------------------------------
# (a) cwn_head_bwd_f32
# ------------------------------------------------------------------------------------------------------------------------------
HEAD_SHAPES = [(20, 12, 3),        # KQ = 5 does not divide 512 (idle tail threads), H2 < slices (empty j ranges), the j tail loop
               (64, 128, 2),       # plain
               (512, 4, 1),        # the last K one pass of the 512 threads covers
               (516, 8, 1),        # the first beyond
               (640, 128, 2),      # five blocks of 128 through dx_more
               (1024, 64, 1),      # eight blocks
               (2048, 512, 2)]     # S = 1, NG = 1, both maxima
HEAD_PARTS = {640: 5, 1024: 8}


def _head_bwd(case, operands, row_split=1, n_parts=1, null_dx=(), hs=None):
    """One cwn_head_bwd_f32 launch -> ([dx_d [n_d, K] or None], [dh_out_d]).  Every block of dx is [n_d + 1, K / n_parts]: NaN
    in the rows of the complexes, a guard row behind n_cells that must keep SENTINEL."""
    g, w2, w1 = operands
    Cn, K, H2, Kp = case.C, case.K, case.H2, case.K // n_parts
    gd, w2d = g.detach().to(DEV).contiguous(), w2.detach().to(DEV).contiguous()
    dims, bufs, dhs, keep = [], [], [], []
    for d in range(case.n_dims):
        n = int(case.ptrs[d][-1])
        hd = (case.h[d] if hs is None else hs[d]).to(DEV).contiguous()
        w1d, pd = w1[d].detach().to(DEV).contiguous(), case.ptrs[d].to(DEV)
        buf = torch.full((n_parts, n + 1, Kp), NAN, device=DEV)
        buf[:, n] = SENTINEL
        dh = torch.full((Cn, H2), NAN, device=DEV)
        D = _ffi.HeadBwdDim(h=hd.data_ptr(), w1=w1d.data_ptr(), cell_ptr=pd.data_ptr(), dx=None if d in null_dx else buf.data_ptr(),
                            dh_out=dh.data_ptr(), n_cells=n, lddx=Kp, n_parts=n_parts)
        for q in range(1, n_parts):
            D.dx_more[q - 1] = buf[q].data_ptr()
        dims.append(D)
        bufs.append(buf)
        dhs.append(dh)
        keep += [hd, w1d, pd]
    arr = (_ffi.HeadBwdDim * case.n_dims)(*dims)
    _ffi.check(_ffi.lib().cwn_head_bwd_f32(arr, case.n_dims, Cn, K, H2, int(case.mean), int(case.mean_final), w2d.data_ptr(), case.O,
                                           gd.data_ptr(), None, 0, row_split, _ffi.stream_ptr(DEV)), 'cwn_head_bwd_f32')
    torch.cuda.synchronize()
    dxs = []
    for d, buf in enumerate(bufs):
        n = buf.size(1) - 1
        assert bool((buf[:, n] == SENTINEL).all()), f'dx[{d}]: the row behind n_cells was written'
        if d in null_dx:
            assert bool(buf[:, :n].isnan().all())
            dxs.append(None)
        else:
            dxs.append(torch.cat([buf[q, :n] for q in range(n_parts)], 1))
    return dxs, dhs


def _head_checks(case, what, **kw):
    got = _head_bwd(case, case.graded, **kw)
    _equal_bits(got[0] + got[1], sum(_head_bwd(case, case.graded, **kw), []), what + ', the same launch again')
    plain = _head_bwd(case, case.plain, **kw)
    R.check_head(case, got[0], got[1], what, plain=plain).report(what)
    return got


@pytest.mark.parametrize('mean', [False, True], ids=['sum', 'mean'])
@pytest.mark.parametrize('K,H2,O', HEAD_SHAPES)
def test_head_bwd(K, H2, O, mean):
    """dx of every dimension and dh_out over six complexes per dimension (one empty, some of one cell, one of 300 cells)."""
    case = R.head_case(K, H2, O, mean)
    _head_checks(case, f'head_bwd K={K} H2={H2} O={O} {"mean" if mean else "sum"}', n_parts=HEAD_PARTS.get(K, 1))


@pytest.mark.parametrize('n_dims', [2, 3])
@pytest.mark.parametrize('K,H2,O', [(20, 12, 3), (640, 128, 2)])
def test_head_bwd_mean_final(K, H2, O, n_dims):
    """ds / n_dims with two and with three dimensions (neither 1 / 3 nor the mean readout's counts are powers of two)."""
    case = R.head_case(K, H2, O, mean=True, mean_final=True, sizes=R.HEAD_SIZES[:n_dims])
    _head_checks(case, f'head_bwd K={K} H2={H2} O={O} mean, mean_final over {n_dims} dimensions', n_parts=HEAD_PARTS.get(K, 1))


@pytest.mark.parametrize('row_split', [1, 3, 64])
@pytest.mark.parametrize('K,H2,O', [(64, 128, 2), (640, 128, 2)])
def test_head_bwd_row_split(K, H2, O, row_split):
    """C x P workgroups: 3 does not divide 300; 64 exceeds the rows of the small complexes, whose chunks past r1 write nothing.
    The same bits as one workgroup per complex."""
    case = R.head_case(K, H2, O, mean=True)
    n_parts = HEAD_PARTS.get(K, 1)
    got = _head_checks(case, f'head_bwd K={K} H2={H2} O={O} mean, row_split {row_split}', n_parts=n_parts, row_split=row_split)
    one = _head_bwd(case, case.graded, n_parts=n_parts)
    _equal_bits(got[0] + got[1], one[0] + one[1], f'row_split {row_split} against 1')


@pytest.mark.parametrize('K,H2,O', [(64, 128, 2), (516, 8, 1)])
def test_head_bwd_skipped_dimensions(K, H2, O):
    """dx = NULL in dimension 1 (nothing of its buffer is touched) and n_cells = 0 in dimension 2: both skipped, their dh_out
    written all the same."""
    case = R.head_case(K, H2, O, mean=True, sizes=(R.HEAD_SIZES[0], R.HEAD_SIZES[1], [0] * len(R.HEAD_SIZES[0])))
    got = _head_checks(case, f'head_bwd K={K} H2={H2} O={O} mean, dx NULL / no cells', null_dx=(1,))
    assert got[0][1] is None and tuple(got[0][2].shape) == (0, K)


def test_head_bwd_autograd_route_at_K_640():
    """ops.head_train over five blocks of 128 per dimension: x.grad of every block is the direct cwn_head_bwd_f32 call fed the
    `hidden` of ops.head(..., want_hidden=True) on the same operands, with the same head_split, bit for bit."""
    K0, n_parts, H2, O = 128, 5, 128, 2
    case = R.head_case(K0 * n_parts, H2, O, mean=True)
    g, w2, w1 = case.plain
    gen = torch.Generator().manual_seed(640)
    ptrs = [p.to(DEV) for p in case.ptrs]
    blocks = [[torch.randn(int(p[-1]), K0, generator=gen).to(DEV).requires_grad_(True) for _ in range(n_parts)] for p in case.ptrs]
    w1s = [w.to(DEV).requires_grad_(True) for w in w1]
    w2d, b2 = w2.to(DEV).requires_grad_(True), torch.zeros(O, device=DEV, requires_grad=True)
    out, _ = ops.head_train([list(b) for b in blocks], ptrs, case.C, w1s, [None] * 3, w2d, b2, mean_readout=True, mean_final=False)
    out.backward(g.to(DEV))
    with torch.no_grad():
        _, _, hidden, _ = ops.head([[x.detach() for x in b] for b in blocks], ptrs, case.C, w1s, [None] * 3, w2d, b2, mean_readout=True,
                                   want_hidden=True)
    P = ops.head_split(sum(int(p[-1]) for p in case.ptrs), case.C)
    dxs, _ = _head_bwd(case, (g, w2d, w1s), row_split=P, n_parts=n_parts, hs=hidden)
    for d in range(3):
        grad = torch.cat([x.grad for x in blocks[d]], 1)
        bad = int((grad != dxs[d]).sum())
        print(f'[cw] head_train K=640 dim {d}: {bad} of {grad.numel()} elements of x.grad differ from the direct launch')
        assert torch.equal(grad, dxs[d]), f'dim {d}: {bad} elements differ'


# ------------------------------------------------------------------------------------------------------------------------------
# (c) cwn_target_head_bwd_f32
# ------------------------------------------------------------------------------------------------------------------------------
def _target_bwd(case, operands, n_complexes=None, live=None):
    """One launch over the first `n_complexes` complexes as the HOST count (default: all) -> (dx [N, H], dW, db); `live`: the
    device count m_dev in front of that capacity."""
    dl, W, x = operands
    Cn = case.C if n_complexes is None else n_complexes
    H, K, N = case.H, case.K, case.N
    dld, Wd, xd = dl[:Cn].to(DEV).contiguous(), W.to(DEV).contiguous(), x.to(DEV).contiguous()
    rows = case.rows[:Cn].to(DEV).contiguous()
    dx = torch.full((N + 1, H), NAN, device=DEV)
    dx[N] = SENTINEL
    dW, db = torch.full((K, H), NAN, device=DEV), torch.full((K,), NAN, device=DEV)
    nbytes = int(_ffi.lib().cwn_target_head_bwd_workspace_bytes(Cn, H, K))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV) if nbytes else None
    m_dev = None if live is None else torch.tensor([live], dtype=torch.int64, device=DEV)
    _ffi.check(_ffi.lib().cwn_target_head_bwd_f32(dld.data_ptr(), K, xd.data_ptr(), N, H, rows.data_ptr(), Cn, Wd.data_ptr(), dx.data_ptr(),
                                                  H, dW.data_ptr(), db.data_ptr(), H, K, _ffi.ptr(ws), nbytes, _ffi.ptr(m_dev),
                                                  _ffi.stream_ptr(DEV)), 'cwn_target_head_bwd_f32')
    torch.cuda.synchronize()
    assert bool((dx[N] == SENTINEL).all()), 'the row behind N was written'
    return dx[:N], dW, db


def _target_checks(case, what, worst):
    got = _target_bwd(case, case.graded)
    _equal_bits(got, _target_bwd(case, case.graded), what + ', the same launch again')
    R.check_target(case, *got, what, plain=_target_bwd(case, case.plain), worst=worst)


@pytest.mark.parametrize('K', [1, 5, 17, 64])
@pytest.mark.parametrize('H', [4, 60, 68, 260, 512])
def test_target_head_bwd(H, K):
    """H: a ragged single slab, a second slab of one quad, the q1 lanes, the maximum; K = 17 takes the kk + 16 j, j = 1 class;
    C: one group straight into dW, then two and three groups (the last ragged) through the workspace and the sum launch."""
    worst = R.Worst('cwn_target_head_bwd_f32')
    for Cn in (1, 64, 65, 129):
        _target_checks(R.target_case(H, K, Cn), f'target_head_bwd H={H} K={K} C={Cn}', worst)
    worst.report(f'H={H} K={K}')


def test_target_head_bwd_searches_beyond_4096_complexes():
    """C = 4100 > kScanMax: a chunk of dx rows finds its complexes by two binary searches."""
    worst = R.Worst('cwn_target_head_bwd_f32')
    _target_checks(R.target_case(4, 2, 4100), 'target_head_bwd H=4 K=2 C=4100', worst)
    worst.report('H=4 K=2 C=4100')


@pytest.mark.parametrize('live', [70, 3])
def test_target_head_bwd_counted(live):
    """m_dev in front of a capacity of 130: the bits of the host-count launch on the trimmed operands (rows of dlogits behind the
    count hold values that must enter nothing)."""
    case = R.target_case(68, 17, 130)
    what = f'target_head_bwd H=68 K=17 capacity 130, live {live}'
    got = _target_bwd(case, case.graded, live=live)
    _equal_bits(got, _target_bwd(case, case.graded, n_complexes=live), what + ' against the host count')
    R.check_target(case, *got, what, live=live).report(what)


# ------------------------------------------------------------------------------------------------------------------------------
# (d) cwn_flow_head_bwd_f32 / cwn_flow_head_bwd_dev_f32
# ------------------------------------------------------------------------------------------------------------------------------
def _flow_bwd(case, operands, window=False, cochains=None, live=None, n_dev=False):
    """One launch -> (dx [N, K], dh_out).  `window`: x and dx as windows of matrices one column wider (ldx % 4 != 0: the element
    form).  `cochains`: the host counts are those of the first `cochains` cochains (trimmed operands).  `live`: the counted
    entry, *c_dev = live in front of the capacity (`n_dev`: the live rows given as well, else read from ptr)."""
    g, W1, W2 = operands
    Cn = case.C if cochains is None else cochains
    K, H, O = case.K, case.H, case.O
    N = int(case.ptr[Cn])
    ld = K + 1 if window else K
    xb = torch.zeros(N + 1, ld)
    xb[:N, :K] = case.x[:N]
    xb, dxb = xb.to(DEV), torch.full((N + 1, ld), SENTINEL, device=DEV)
    gd, hd, pd = g[:Cn].to(DEV).contiguous(), case.h[:Cn].to(DEV).contiguous(), case.ptr[:Cn + 1].to(DEV)
    W1d, W2d = W1.to(DEV).contiguous(), W2.to(DEV).contiguous()
    dh = torch.full((Cn, H), NAN, device=DEV)
    floats = int(_ffi.lib().cwn_flow_head_workspace_floats(N, Cn, K))
    ws = torch.empty(max(floats, 4), dtype=torch.float32, device=DEV)
    head = (gd.data_ptr(), O, hd.data_ptr(), xb.data_ptr(), N, ld, pd.data_ptr(), Cn, W1d.data_ptr(), W2d.data_ptr(), dxb.data_ptr(), ld,
            dh.data_ptr(), K, H, O, int(case.take_abs), int(case.mean))
    tail = (ws.data_ptr(), ws.numel(), _ffi.stream_ptr(DEV))
    if live is None:
        _ffi.check(_ffi.lib().cwn_flow_head_bwd_f32(*head, *tail), 'cwn_flow_head_bwd_f32')
    else:
        c_dev = torch.tensor([live], dtype=torch.int64, device=DEV)
        nd = torch.tensor([int(case.ptr[live])], dtype=torch.int64, device=DEV) if n_dev else None
        _ffi.check(_ffi.lib().cwn_flow_head_bwd_dev_f32(*head, _ffi.ptr(nd), c_dev.data_ptr(), *tail), 'cwn_flow_head_bwd_dev_f32')
    torch.cuda.synchronize()
    n_live = N if live is None else int(case.ptr[live])
    assert bool((dxb[n_live:] == SENTINEL).all()), 'a row of dx behind the live rows was written'
    assert bool((dxb[:, K:] == SENTINEL).all()), 'a column outside the window was written'
    return dxb[:n_live, :K].contiguous(), dh


@pytest.mark.parametrize('mean', [False, True], ids=['sum', 'mean'])
@pytest.mark.parametrize('take_abs', [True, False], ids=['abs', 'signed'])
@pytest.mark.parametrize('K,H,O', [(1, 1, 1), (3, 5, 2), (20, 12, 3), (128, 128, 64)])
def test_flow_head_bwd(K, H, O, take_abs, mean):
    """K = 3: the element form alone; K = 20: cols = 5, thread 255 has no slot.  Cochains of 0, 1, 127, 128, 129 and 300 rows.
    Under take_abs x holds +0.0 and -0.0, whose dx is exactly 0 (the reference gives those entries no bound)."""
    case = R.flow_case(K, H, O, take_abs, mean)
    what = f'flow_head_bwd K={K} H={H} O={O} {"abs" if take_abs else "signed"} {"mean" if mean else "sum"}'
    got = _flow_bwd(case, case.graded)
    _equal_bits(got, _flow_bwd(case, case.graded), what + ', the same launch again')
    _equal_bits(got, _flow_bwd(case, case.graded, window=True), what + ', the element form on a window with ldx % 4 != 0')
    if take_abs:
        assert not bool(got[0].cpu()[case.x == 0].any()), what + ': dx is not 0 where x is +0.0 or -0.0'
    R.check_flow(case, *got, what, plain=_flow_bwd(case, case.plain)).report(what)


@pytest.mark.parametrize('n_dev', [False, True], ids=['rows_from_ptr', 'rows_given'])
@pytest.mark.parametrize('take_abs', [True, False], ids=['abs', 'signed'])
@pytest.mark.parametrize('K,H,O', [(20, 12, 3), (128, 128, 64)])
def test_flow_head_bwd_counted(K, H, O, take_abs, n_dev):
    """A capacity of 6 cochains with 4 live: the live rows of dx and dh_out have the bits of the host-count launch on the trimmed
    operands, dh_out of the absent cochains is zero, the rows of dx behind the live total keep their sentinel (_flow_bwd)."""
    case, live = R.flow_case(K, H, O, take_abs, mean=True), 4
    what = f'flow_head_bwd_dev K={K} H={H} O={O} {"abs" if take_abs else "signed"} capacity 6, live {live}'
    dx, dh = _flow_bwd(case, case.graded, live=live, n_dev=n_dev)
    host = _flow_bwd(case, case.graded, cochains=live)
    _equal_bits((dx, dh[:live]), host, what + ' against the host count')
    assert not bool(dh[live:].any()), what + ': dh_out of an absent cochain is not zero'
    R.check_flow(R.flow_trimmed(case, live), dx, dh[:live], what, worst=R.Worst('cwn_flow_head_bwd_dev_f32')).report(what)
