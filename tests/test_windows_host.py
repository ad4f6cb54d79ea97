"""The host half of the operand-window contract (include/cwn_hip.h, "OPERAND WINDOWS"; the device half: test_gpu_windows.py):
  * the refusals an entry point decides before any device call, through the C ABI with dummy pointer values of the right
    alignment class (never dereferenced: each entry's argument checks were read, the refusal precedes everything else);
  * cwn_gemm_would_split / cwn_gemm_tn_would_split per window class (pure functions of their arguments);
  * a self-test of tests/_windows.py: its checks FAIL on an emulated kernel that overruns its output window by one column or
    lets a neighbour column into a sum, and pass on the correct one -- the GPU assertions can fail without a kernel having to
    be broken to prove it."""
import ctypes as C

import pytest
import torch

from cwn_amd import _ffi
from tests._windows import CLASSES, NAN, SENT, VEC_OFF, Windows, bits

BAD_ARG, ALIGN = 1, 5
BASE = 1 << 20                 # a 16-byte aligned "address"; operand k of a descriptor lives at BASE * (k + 1)
FORBIDDEN = {'W2': ALIGN, 'W3': BAD_ARG}      # the "16-B aligned, strides multiples of 4" entries: a pointer / a stride


def _p(k, cls):
    """The dummy address of operand k as a window of class cls: its buffer's 16-byte aligned start + 4 * col0."""
    return BASE * (k + 1) + 4 * CLASSES[cls][0]


def _ld(w, cls):
    return w + CLASSES[cls][1]


@pytest.mark.parametrize('F', [64, 128])
@pytest.mark.parametrize('cls', ['W2', 'W3'])
def test_stage_entries_refuse_a_forbidden_window_before_any_device_call(cls, F):
    """cwn_dense_stage_f32 / _ex / _bwd, cwn_update_mlp_f32 (F-wide inputs) and cwn_update_mlp3_f32: "pointers 16-B aligned,
    strides multiples of 4" -- CWN_ERR_ALIGN for a pointer off 16 bytes (W2), CWN_ERR_BAD_ARG for a stride that is no multiple
    of 4 (W3); each with ONE operand in the class and all others contiguous, so that every operand's check is reached."""
    L = _ffi.lib()
    want = FORBIDDEN[cls]
    ok = lambda k: (BASE * (k + 1), F)
    bad = lambda k: (_p(k, cls), _ld(F, cls))

    def stage(which):
        p = {n: (bad(k) if n == which else ok(k)) for k, n in enumerate(('X', 'X2', 'Y', 'X3'))}
        d = _ffi.StageDesc(X=p['X'][0], X2=p['X2'][0], w_packed=BASE * 9, w2_packed=BASE * 10, Y=p['Y'][0], M=70, ldx=p['X'][1],
                           ldx2=p['X2'][1], ldy=p['Y'][1], in_relu=3)
        ex = (_ffi.StageExtra * 2)()
        ex[0].X, ex[0].w_packed, ex[0].ldx = p['X3'][0], BASE * 11, p['X3'][1]
        return (_ffi.StageDesc * 1)(d), ex

    for which in ('X', 'X2', 'Y'):
        arr, ex = stage(which)
        assert L.cwn_dense_stage_f32(arr, 1, F, None) == want, which
        assert L.cwn_dense_stage_ex_f32(arr, ex, 1, F, None) == want, which
    arr, ex = stage('X3')
    assert L.cwn_dense_stage_ex_f32(arr, ex, 1, F, None) == want

    for which in ('dy', 'z', 'dz', 'dx', 'dx2'):
        p = {n: (bad(k) if n == which else ok(k)) for k, n in enumerate(('dy', 'z', 'dz', 'dx', 'dx2'))}
        d = _ffi.StageBwdDesc(dy=p['dy'][0], z=p['z'][0], dz=p['dz'][0], wt_packed=BASE * 9, wt2_packed=BASE * 10, dx=p['dx'][0],
                              dx2=p['dx2'][0], M=70, lddy=p['dy'][1], ldz=p['z'][1], lddz=p['dz'][1], lddx=p['dx'][1], lddx2=p['dx2'][1],
                              relu=1)
        assert L.cwn_dense_stage_bwd_f32((_ffi.StageBwdDesc * 1)(d), 1, F, None) == want, which
    # (its constants: "every acc1 / acc2 / s1 / s2 / constant pointer 16-B aligned")
    for name in ('scale', 'shift', 'mean', 'rstd', 's1', 's2', 'acc1', 'acc2'):
        kw = {n: BASE * (20 + k) for k, n in enumerate(('scale', 'shift', 'mean', 'rstd', 's1', 's2', 'acc1', 'acc2'))}
        kw[name] += 4
        d = _ffi.StageBwdDesc(dy=BASE, z=2 * BASE, wt_packed=BASE * 9, dx=3 * BASE, M=70, lddy=F, ldz=F, lddx=F, relu=1, **kw)
        assert L.cwn_dense_stage_bwd_f32((_ffi.StageBwdDesc * 1)(d), 1, F, None) == ALIGN, name

    for which in ('x_up', 'x_b', 'y'):
        p = {n: (bad(k) if n == which else ok(k)) for k, n in enumerate(('x_up', 'x_b', 'y'))}
        arr = (_ffi.MlpDim * 1)()
        a = arr[0]
        a.x_up, a.x_b, a.y, a.M, a.ldx_up, a.ldx_b, a.ldy = p['x_up'][0], p['x_b'][0], p['y'][0], 70, p['x_up'][1], p['x_b'][1], p['y'][1]
        for k in range(6):
            a.w_packed[k] = BASE * (9 + k)
        assert L.cwn_update_mlp_f32(arr, 1, F, None) == want, which
        if which != 'y':       # in_width: "any value >= in_width and the two pointers need 4-byte alignment only" -- no refusal left
            a.in_width = 20    # but a NULL weight, which ends the call before the launch: the window itself was accepted
            a.w_packed[5] = None
            assert L.cwn_update_mlp_f32(arr, 1, F, None) == BAD_ARG, which
        else:                  # y keeps its rule with narrow inputs
            a.in_width = 20
            assert L.cwn_update_mlp_f32(arr, 1, F, None) == want, which

    for which in ('x0', 'x1', 'x2', 'y'):
        p = {n: (bad(k) if n == which else ok(k)) for k, n in enumerate(('x0', 'x1', 'x2', 'y'))}
        arr = (_ffi.Mlp3Dim * 1)()
        a = arr[0]
        for k in range(3):
            a.x[k], a.ldx[k] = p[f'x{k}']
        a.y, a.ldy, a.M = p['y'][0], p['y'][1], 70
        for k in range(9):
            a.w_packed[k] = BASE * (9 + k)
        assert L.cwn_update_mlp3_f32(arr, 1, F, None) == want, which


@pytest.mark.parametrize('cls', ['W2', 'W3'])
def test_norm_bwd_fused_and_the_gemm_backward_prologue_refuse_a_forbidden_window(cls):
    """cwn_norm_bwd_f32: "needs 16-byte aligned operands and strides (CWN_ERR_ALIGN otherwise)"; cwn_gemm_desc.bnb: z / dz "16-byte
    aligned", row strides multiples of 4 -- CWN_ERR_ALIGN, decided while the descriptors are read, before any device call."""
    L = _ffi.lib()
    N = 64
    for which in ('dy', 'z', 'out'):
        p = {n: ((_p(k, cls), _ld(N, cls)) if n == which else (BASE * (k + 1), N)) for k, n in enumerate(('dy', 'z', 'out'))}
        d = _ffi.NormDesc(dy=p['dy'][0], z=p['z'][0], out=p['out'][0], M=70, lddy=p['dy'][1], ldz=p['z'][1], ldout=p['out'][1], N=N, relu=1)
        assert L.cwn_norm_bwd_f32((_ffi.NormDesc * 1)(d), 1, 0, None) == ALIGN, which
    d = _ffi.NormDesc(dy=BASE, z=2 * BASE, out=3 * BASE, M=70, lddy=37, ldz=37, ldout=37, N=37, relu=1)
    assert L.cwn_norm_bwd_f32((_ffi.NormDesc * 1)(d), 1, 0, None) == ALIGN          # a width that is no multiple of 4
    for which in ('z', 'dz'):
        p = {n: ((_p(k, cls), _ld(N, cls)) if n == which else (BASE * (k + 1), N)) for k, n in enumerate(('z', 'dz'))}
        bnb = _ffi.GemmBnb(z=p['z'][0], dz=p['dz'][0], ldz=p['z'][1], lddz=p['dz'][1], relu=1)
        g = _ffi.GemmDesc(X=5 * BASE, W=6 * BASE, Y=7 * BASE, M=70, N=N, K=N, ldx=N, ldw=N, ldy=N, w_trans=1, bnb=C.pointer(bnb))
        assert L.cwn_gemm_f32((_ffi.GemmDesc * 1)(g), 1, None) == ALIGN, which


@pytest.mark.parametrize('cls', ['W2', 'W3'])
def test_heads_refuse_a_forbidden_window_before_any_device_call(cls):
    """cwn_head_f32 / cwn_head_bwd_f32: x / dx "row stride (multiple of 4)", 16-byte aligned -- CWN_ERR_BAD_ARG for the stride,
    CWN_ERR_ALIGN for the pointer; cwn_target_head_f32 / _bwd_f32: "CWN_ERR_ALIGN: x / W off 16 bytes, ldx % 4 != 0"."""
    L = _ffi.lib()
    K, H2, O, Cn, M = 16, 8, 3, 4, 70
    D = _ffi.HeadDim()
    D.x, D.cell_ptr, D.w1t, D.n_cells, D.ldx, D.n_parts = _p(0, cls), 2 * BASE, 3 * BASE, M, _ld(K, cls), 1
    assert L.cwn_head_f32((_ffi.HeadDim * 1)(D), 1, Cn, K, H2, 0, 0, 4 * BASE, None, O, 5 * BASE, None, None, 0, None, 0, 1, None) \
        == FORBIDDEN[cls]
    B = _ffi.HeadBwdDim()
    B.h, B.w1, B.cell_ptr, B.dx, B.n_cells, B.lddx, B.n_parts = BASE * 6, BASE * 7, 2 * BASE, _p(0, cls), M, _ld(K, cls), 1
    assert L.cwn_head_bwd_f32((_ffi.HeadBwdDim * 1)(B), 1, Cn, K, H2, 0, 0, 4 * BASE, O, 5 * BASE, None, 0, 1, None) == FORBIDDEN[cls]
    H, Kc = 64, 5
    assert L.cwn_target_head_f32(_p(0, cls), M, _ld(H, cls), 2 * BASE, Cn, 3 * BASE, None, 4 * BASE, Kc, H, Kc, None, None, None) == ALIGN
    assert L.cwn_target_head_bwd_f32(5 * BASE, Kc, 6 * BASE, M, H, 2 * BASE, Cn, 3 * BASE, _p(0, cls), _ld(H, cls), None, None, H, Kc,
                                     None, 0, None, None) == ALIGN
    assert L.cwn_target_head_bwd_f32(5 * BASE, Kc, _p(0, cls), M, _ld(H, cls), 2 * BASE, Cn, 3 * BASE, None, H, 7 * BASE, None, H, Kc,
                                     None, 0, None, None) == ALIGN


@pytest.mark.parametrize('cls', sorted(CLASSES))
def test_would_split_predicates_per_window_class(cls):
    """cwn_gemm_would_split: "16-B aligned operands" (and row strides that are multiples of 4: the split kernel moves 16 bytes a
    lane) -- 1 in W0 / W1, 0 in W2 - W4 whichever operand carries the window; 0 with CWN_GEMM_EXACT or CWN_GEMM_ADD_OUT in any
    class; the packed weight's ldw is ignored.  cwn_gemm_tn_would_split: "every operand is 16-byte aligned with strides and
    widths that are multiples of 4" -- the same per class for dZ, X and X2; dW / db are accumulated element by element: their
    window does not matter."""
    L = _ffi.lib()
    vec_ok = cls in ('W0', 'W1')
    F = 128

    def gemm(which, **kw):
        p = {n: ((_p(k, cls), _ld(F, cls)) if n in which else (BASE * (k + 1), F)) for k, n in enumerate(('X', 'W', 'Y'))}
        v = {n: BASE * (5 + k) + (4 * VEC_OFF[cls] if n in which else 0) for k, n in enumerate(('bias', 'out_scale', 'out_shift'))}
        d = _ffi.GemmDesc(X=p['X'][0], W=p['W'][0], Y=p['Y'][0], M=70, N=F, K=F, ldx=p['X'][1], ldw=p['W'][1], ldy=p['Y'][1], **v)
        for k, val in kw.items():
            setattr(d, k, val)
        return L.cwn_gemm_would_split((_ffi.GemmDesc * 1)(d), 1)

    for which in (('X',), ('W',), ('Y',), ('bias',), ('out_scale',), ('out_shift',), ('X', 'W', 'Y', 'bias', 'out_scale', 'out_shift')):
        assert gemm(which) == int(vec_ok), which
        assert gemm(which, flags=_ffi.GEMM_EXACT) == 0 and gemm(which, flags=_ffi.GEMM_ADD_OUT) == 0, which
    assert gemm(('X',), K=64, ldw=64) == 0 and gemm(('X',), N=64) == 0 and gemm(('X',), w_trans=1) == 0      # not its shape
    assert gemm((), flags=_ffi.GEMM_W_PACKED, ldw=131) == 1                                                    # ldw ignored

    def tn(which, N=128, K=128, K2=0):
        w = {'dZ': N, 'X': K, 'X2': K2, 'dW': K + K2}
        p = {n: ((_p(k, cls), _ld(w[n], cls)) if n in which else (BASE * (k + 1), w[n])) for k, n in enumerate(('dZ', 'X', 'X2', 'dW'))}
        d = _ffi.GemmTnDesc(dZ=p['dZ'][0], X=p['X'][0], X2=p['X2'][0] if K2 else None, dW=p['dW'][0],
                            db=BASE * 9 + (4 * VEC_OFF[cls] if 'db' in which else 0), M=70, lddz=p['dZ'][1], ldx=p['X'][1],
                            ldx2=p['X2'][1] if K2 else 0, lddw=p['dW'][1], N=N, K=K, K2=K2)
        return L.cwn_gemm_tn_would_split((_ffi.GemmTnDesc * 1)(d), 1)

    for which in (('dZ',), ('X',), ('dZ', 'X', 'dW', 'db')):
        assert tn(which) == int(vec_ok), which
    assert tn(('X2',), K=64, K2=64) == int(vec_ok)
    assert tn(('dW', 'db')) == 1                        # accumulated element by element
    assert tn(('X',), N=64, K=64) == 0 and tn((), N=128, K=126) == 0 and tn((), N=130, K=128) == 0     # narrow; widths % 4


# ---- the checkers can fail ---------------------------------------------------------------------------------------------------
def _emulate(how: str):
    """Y = X W^T over windowed CPU buffers, emulated in torch: 'right'; 'overrun' -- the store runs one column over the
    output window; 'neighbour' -- the load takes one column too many of X into the sum."""
    g = torch.Generator().manual_seed(1)
    M, N, K = 33, 8, 6
    X, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    ws = Windows(torch.device('cpu'))
    x, w, y = ws.inp('X', X, 'W1'), ws.inp('W', W, 'W1'), ws.out('Y', M, N, 'W1')
    xbuf, ybuf = ws.items[0][1], ws.items[2][1]
    c0 = CLASSES['W1'][0]
    if how == 'right':
        y.copy_(x @ w.t())
    elif how == 'overrun':
        ybuf[:, c0:c0 + N + 1] = torch.cat([x @ w.t(), torch.zeros(M, 1)], 1)
    elif how == 'neighbour':
        y.copy_(xbuf[:, c0:c0 + K + 1] @ torch.cat([w, torch.ones(N, 1)], 1).t())
    elif how == 'input':
        y.copy_(x @ w.t())
        xbuf[0, 0] = 0.0
    return ws, y, X.double() @ W.double().t()


def test_window_checkers_fail_on_a_wrong_kernel_and_pass_on_the_right_one():
    from tests._product import gate
    ws, y, ref = _emulate('right')
    ws.neighbours('right')
    ws.no_leak(y, 'right')
    gate(y, ref, 'right')
    with pytest.raises(AssertionError, match='was to write nothing'):
        ws.unchanged('right')                       # (a refused call must not even have written its window)

    ws, y, ref = _emulate('overrun')                # (c) fails; the window itself is right and clean
    with pytest.raises(AssertionError, match='beside the output window'):
        ws.neighbours('overrun')
    ws.no_leak(y, 'overrun')
    gate(y, ref, 'overrun')

    ws, y, ref = _emulate('neighbour')              # (d) fails (and with it parity); nothing beside the window was written
    ws.neighbours('neighbour')
    with pytest.raises(AssertionError, match='NaN inside the result window'):
        ws.no_leak(y, 'neighbour')
    with pytest.raises(AssertionError):
        gate(y, ref, 'neighbour')

    ws, y, ref = _emulate('input')                  # (c) fails for an input that was written
    with pytest.raises(AssertionError, match='an input buffer was written'):
        ws.neighbours('input')


def test_window_helper_lays_operands_out_as_the_classes_say():
    ws = Windows(torch.device('cpu'))
    data = torch.arange(12.0).view(3, 4)
    for cls, (c0, extra) in CLASSES.items():
        v = ws.inp('x', data, cls)
        buf = ws.items[-1][1]
        assert tuple(buf.shape) == (3, 4 + extra) and v.stride(0) == 4 + extra and v.storage_offset() == c0 and torch.equal(v, data)
        outside = torch.ones_like(buf, dtype=torch.bool)
        outside[:, c0:c0 + 4] = False
        assert bool(torch.isnan(buf[outside]).all())
        o = ws.out('y', 3, 4, cls)
        assert bool((ws.items[-1][1] == SENT).all()) and o.stride(0) == 4 + extra and o.storage_offset() == c0
    a, b = ws.halves('h', 3, 4, 'W1')
    assert a.storage_offset() == 4 and b.storage_offset() == 8 and a.stride(0) == b.stride(0) == 16
    b2, a2 = ws.halves('h', 3, 4, 'W1', reverse=True)
    assert a2.storage_offset() == 4 and b2.storage_offset() == 8
    v = ws.vec('v', torch.arange(4.0), 3)
    assert v.storage_offset() == 3 and bool(torch.isnan(ws.items[-1][1][:3]).all()) and bool(torch.isnan(ws.items[-1][1][7:]).all())
    assert torch.equal(bits(torch.tensor([NAN])), bits(torch.tensor([NAN])))
    assert not torch.equal(bits(torch.tensor([0.0])), bits(torch.tensor([-0.0])))
