"""The operand-window contract of include/cwn_hip.h ("OPERAND WINDOWS") on every f32 entry point that carries a row stride:

    "a kernel reads and writes the [rows, width] window of each operand only; what lies between `width` and the row stride is
     never written and never influences a result; each entry states its own alignment and stride rule and refuses everything
     else before launching."

Every test here lays the operands of ONE entry point out as windows of wider buffers (tests/_windows.py: NaN around an input
window, a sentinel around an output window, per-column vectors inside longer NaN-padded ones) in the window classes
    W0 (0, 0) contiguous;  W1 (4, 8) 16-byte pointer, stride % 4 == 0;  W2 (1, 8) 4-byte pointer;  W3 (0, 3) stride % 4 != 0;
    W4 (0, 1) one element between the rows (the tail of a width that is no multiple of 4)
as (first column, stride - width), at M = 1, 33 and 70 rows, and asserts per case
  (a) the window's result against a float64 reference evaluated on the CPU from the window's contents, inside
      tests/_product.gate: 1e-5 * max(1, |ref|_inf);
  (b) bit-identity with the same entry point on contiguous copies wherever the same kernel form serves both, or the header
      promises one order for both forms; which form ran is asserted (ops.gemm_uses_split, cwn_gemm_tn_would_split, the
      entry's own vector predicate restated) and printed;
  (c) every element of every output buffer outside its window, and every element of every input buffer, keeps its bits;
  (d) no NaN inside a result window;
  (e) the classes an entry's header forbids: the C entry point returns the documented code and writes nothing (the checks
      were read: every refusal below precedes the launch), and the ops-level wrapper -- where one exists -- serves the same
      window through a copy or another kernel, by (a).
Kernels whose own test files hold a window case are not repeated: cwn_layernorm_* (test_gpu_layernorm.py:
test_strided_operands), cwn_linear_stats_f32 (test_gpu_linear_stats.py: test_x_as_a_column_slice_with_an_odd_row_stride),
cwn_linear_wide_f32 (test_gpu_linear_wide.py: every parity case, `_view`), cwn_update_chain_f32 (test_gpu_chain_f32.py:
test_update_chain_allocates_its_outputs_and_takes_strided_operands), cwn_gin_layer_f32 (test_gpu_gin.py:
test_strided_operands_inside_one_buffer), cwn_gine_layer_f32 (test_gpu_gine.py: test_strided_operands_inside_wider_buffers),
cwn_flow_head_f32 (test_gpu_flow_head.py: test_forward_against_float64), the float64 paths (test_gpu_f64.py,
test_gpu_f64_dense.py), cwn_embed_pool / cwn_agnostic_head (test_gpu_agnostic.py: `_Dim`).  Where those cases padded an
input window with finite numbers (or zeros), the padding is NaN now, and test_gpu_linear_wide.py checks the padding of its
output view: (c) and (d) hold there too."""
import ctypes as C

import pytest
import torch

from cwn_amd import _ffi, ops
from tests._product import gate
from tests._windows import CLASSES, NAN, ROWS, SENT, VEC_OFF, Windows, aligned16, bits

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BAD_ARG, ALIGN = 1, 5
ALL = ('W0', 'W1', 'W2', 'W3', 'W4')
VECTOR_OK = ('W0', 'W1')               # the classes the "16-B aligned, strides multiples of 4" entries take
FORBIDDEN = {'W2': ALIGN, 'W3': BAD_ARG}      # ... and what they answer to the others: a pointer / a stride


def _rand(g, *shape):
    return torch.randn(*shape, generator=g)


def _stream():
    return _ffi.stream_ptr(DEV)


def _form(what, form):
    print(f'[window] {what}: {form}')


def _contig(cls_run, *args, **kw):
    """The same launch on contiguous copies (class W0)."""
    return cls_run('W0', *args, **kw)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. cwn_gemm_f32
# ------------------------------------------------------------------------------------------------------------------------------
GEMM_CASES = {
    # name: (N, K, K2, w_trans, add_out, packed, epilogue (out affine + relu), prologue, statistics, w_col0, split-eligible)
    'exact_40x24': (40, 24, 0, False, False, False, True, False, False, False, False),
    'exact_37x23': (37, 23, 0, False, False, False, True, False, False, False, False),
    'exact_130x23': (130, 23, 0, False, False, False, False, False, False, False, False),
    'exact_64x64': (64, 64, 0, False, False, False, False, False, False, False, False),
    'concat_x2': (64, 24, 12, False, False, False, True, True, False, False, False),
    'w_trans_40x24': (40, 24, 0, True, False, False, False, False, False, False, False),
    'w_trans_37x23': (37, 23, 0, True, False, False, False, False, False, False, False),
    'w_trans_128': (128, 128, 0, True, False, False, False, False, False, False, False),
    'add_out_40x24': (40, 24, 0, False, True, False, False, False, False, False, False),
    'add_out_37x23': (37, 23, 0, False, True, False, False, False, False, False, False),
    'stats_40x24': (40, 24, 0, False, False, False, False, True, True, False, False),
    'w_col0_64x64': (64, 64, 0, False, False, False, False, False, False, True, False),
    'split_128': (128, 128, 0, False, False, False, True, False, False, False, True),
    'split_128_w_col0': (128, 128, 0, False, False, False, False, False, False, True, True),
    'split_128_packed': (128, 128, 0, False, False, True, True, False, False, False, True),
}


def _gemm_run(cls, case, M, T):
    """One cwn_gemm_f32 launch of `case` through ops.run_gemm with every operand a window of class `cls`; T: the CPU operands."""
    N, K, K2, w_trans, add_out, packed, epi, pro, stats, w_col0, split = GEMM_CASES[case]
    ws = Windows(DEV)
    off = VEC_OFF[cls]
    X = ws.inp('X', T['X'][:M], cls)
    X2 = ws.inp('X2', T['X2'][:M], cls) if K2 else None
    if packed:
        W, pk = T['Wparam'], ops.pack_gemm_weight(T['Wparam'])
        assert pk is not None
    else:
        W, pk = ws.inp('W', T['W'], cls), None
    col0 = None
    if w_col0:                              # the whole wider weight, its window named by the column offset
        col0, W = CLASSES[cls][0], ws.items[-1][1]
    vec = lambda name: ws.vec(name, T[name], off)
    Y = ws.out('Y', M, N, cls, prefill=T['Y0'][:M] if add_out else None)
    cs = torch.full((2, ops.stat_rows(M), N), SENT, dtype=torch.float64, device=DEV) if stats else None
    gm = ops.Gemm(X=X, X2=X2, W=W, bias=vec('bias'), relu=epi, out_scale=vec('osc') if epi else None,
                  out_shift=vec('osh') if epi else None, in_scale=vec('isc') if pro else None, in_shift=vec('ish') if pro else None,
                  in_scale2=vec('isc2') if pro and K2 else None, in_shift2=vec('ish2') if pro and K2 else None,
                  in_relu=(3 if K2 else 1) if pro else 0, col_stats=cs, w_trans=w_trans, out=Y, w_col0=col0, w_packed=pk,
                  add_out=add_out)
    uses_split = ops.gemm_uses_split([gm], DEV)
    d = gm.desc(Y)
    fast = all(p % 16 == 0 for p in (d.X, d.X2 or 0, d.W, d.Y)) and d.ldx % 4 == 0 and d.ldw % 4 == 0 and d.ldy % 4 == 0 \
        and (K2 == 0 or d.ldx2 % 4 == 0) and K % 4 == 0 and K2 % 4 == 0
    ops.run_gemm([gm], DEV)
    return ws, Y, cs, uses_split, fast


@pytest.mark.parametrize('cls', ALL)
@pytest.mark.parametrize('case', sorted(GEMM_CASES))
def test_gemm_windows(case, cls):
    """cwn_gemm_f32 (csrc/cwn_gemm.hip, csrc/cwn_gemm_split.hip): X, X2, W and Y as windows, bias / the prologue and epilogue
    vectors inside longer ones; the exact kernel on its 64 x 64 and 32 x 128 tiles at N x K = 40 x 24, 37 x 23 (no width a
    multiple of 4), 130 x 23 (two column tiles), 64 x 64, with the K-concatenation and the prologue, w_trans, ADD_OUT onto a
    pre-filled window, the statistics epilogue, W named by `w_col0` inside the wider weight; the bf16-split kernel at
    128 x 128 with the fp32 and the packed weight.  The exact kernel's 16-byte form (every pointer 16-byte aligned, every stride
    and K a multiple of 4) and its element-wise twin are "bitwise an fmaf chain per output element": bit-identity is held
    between them; the split kernel takes W0 / W1 only (cwn_gemm_would_split) and hands W2 - W4 to the exact kernel, where the
    result is held to the gate."""
    N, K, K2, w_trans, add_out, packed, epi, pro, stats, w_col0, split = GEMM_CASES[case]
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    Kt = K + K2
    T = {'X': _rand(g, max(ROWS), K), 'X2': _rand(g, max(ROWS), max(K2, 1)), 'Y0': _rand(g, max(ROWS), N),
         'W': (_rand(g, Kt, N) if w_trans else _rand(g, N, Kt)) / Kt ** 0.5, 'bias': _rand(g, N),
         'osc': torch.rand(N, generator=g) + 0.5, 'osh': _rand(g, N), 'isc': torch.rand(K, generator=g) + 0.5, 'ish': _rand(g, K),
         'isc2': torch.rand(max(K2, 1), generator=g) + 0.5, 'ish2': _rand(g, max(K2, 1))}
    T['Wparam'] = torch.nn.Parameter(T['W'].to(DEV))
    for M in ROWS:
        what = f'gemm {case} {cls} M={M}'
        ws, Y, cs, uses_split, fast = _gemm_run(cls, case, M, T)
        assert uses_split == (split and cls in VECTOR_OK), what
        _form(what, 'bf16-split kernel' if uses_split else f'exact kernel, {"16-byte" if fast else "element-wise"} form')
        # (ONE row at column 0 has no stride to speak of: with the weight contiguous -- the packed case -- W3 / W4 are W0 there)
        mats_ok = cls in VECTOR_OK or (M == 1 and packed and CLASSES[cls][0] == 0)
        assert fast == (mats_ok and K % 4 == 0 and K2 % 4 == 0 and N % 4 == 0), what
        x = T['X'][:M].double()
        if pro:
            x = (x * T['isc'].double() + T['ish'].double()).relu()
        if K2:
            x2 = T['X2'][:M].double()
            x = torch.cat([x, (x2 * T['isc2'].double() + T['ish2'].double()).relu() if pro else x2], 1)
        z = x @ (T['W'].double() if w_trans else T['W'].double().t()) + T['bias'].double()
        ref = (z * T['osc'].double() + T['osh'].double()).relu() if epi else z
        ref = ref + T['Y0'][:M].double() if add_out else ref
        ws.no_leak(Y, what)
        gate(Y, ref, what)
        ws.neighbours(what)
        if stats:
            zp = torch.cat([z, z.new_zeros((-M) % 32, N)]).view(-1, 32, N)
            gate(cs[0], zp.sum(1), what + ' col_sum')
            gate(cs[1], (zp * zp).sum(1), what + ' col_sumsq')
        _, Yc, csc, split_c, _ = _contig(_gemm_run, case, M, T)
        if uses_split == split_c:
            assert torch.equal(Y, Yc), f'{what}: not the bits of the launch on contiguous copies'
            assert not stats or torch.equal(cs, csc), what


@pytest.mark.parametrize('F', [64, 128])
@pytest.mark.parametrize('cls', ['W0', 'W1', 'W2', 'W3'])
def test_gemm_batchnorm_backward_prologue_windows(cls, F):
    """cwn_gemm_desc.bnb (the BatchNorm + ReLU backward as the prologue of the input-gradient GEMM): dy, z, the weight and dx
    as windows, dz an output window of its own, the constants and sums inside longer vectors, acc1 / acc2 pre-filled.  "w_trans
    launches with 16-byte aligned operands": W0 / W1 run (bit-identical to each other: one kernel form); W2 / W3 are refused
    before the launch -- CWN_ERR_ALIGN, z / dz being checked first -- and nothing is written."""
    g = torch.Generator().manual_seed(31 * F)
    Mx = max(ROWS)
    T = {'dy': _rand(g, Mx, F), 'z': _rand(g, Mx, F) * 2 + 0.5, 'W': _rand(g, F, F) / F ** 0.5, 'acc': _rand(g, 2, F)}
    con = {'scale': torch.rand(F, generator=g) + 0.5, 'shift': _rand(g, F), 'mean': _rand(g, F), 'rstd': torch.rand(F, generator=g) + 0.5,
           's1': _rand(g, F), 's2': _rand(g, F)}

    def run(c, M):
        ws = Windows(DEV)
        off = VEC_OFF[c]
        dy, z, W = ws.inp('dy', T['dy'][:M], c), ws.inp('z', T['z'][:M], c), ws.inp('W', T['W'], c)
        dz, dx = ws.out('dz', M, F, c), ws.out('dx', M, F, c)
        v = {k: ws.vec(k, t, off) for k, t in con.items()}
        a1, a2 = ws.vec('acc1', T['acc'][0], off, out=True), ws.vec('acc2', T['acc'][1], off, out=True)
        bnb = _ffi.GemmBnb(z=z.data_ptr(), dz=dz.data_ptr(), scale=v['scale'].data_ptr(), shift=v['shift'].data_ptr(),
                           mean=v['mean'].data_ptr(), rstd=v['rstd'].data_ptr(), s1=v['s1'].data_ptr(), s2=v['s2'].data_ptr(),
                           acc1=a1.data_ptr(), acc2=a2.data_ptr(), ldz=z.stride(0), lddz=dz.stride(0), relu=1)
        gm = ops.Gemm(X=dy, W=W, w_trans=True, bnb=bnb, out=dx)
        return ws, gm, dz, dx, a1, a2

    for M in ROWS:
        what = f'gemm bnb F={F} {cls} M={M}'
        ws, gm, dz, dx, a1, a2 = run(cls, M)
        if cls in FORBIDDEN:
            rc = _ffi.lib().cwn_gemm_f32((_ffi.GemmDesc * 1)(gm.desc(dx)), 1, _stream())
            torch.cuda.synchronize()
            assert rc == ALIGN, (what, rc)
            ws.unchanged(what)
            _form(what, 'refused (CWN_ERR_ALIGN), nothing written')
            continue
        ops.run_gemm([gm], DEV)
        _form(what, 'exact kernel, 16-byte form, BatchNorm-backward prologue')
        dyd, zd = T['dy'][:M].double(), T['z'][:M].double()
        c = {k: t.double() for k, t in con.items()}
        dyh = dyd * (zd * c['scale'] + c['shift'] > 0)
        rdz = c['scale'] * (dyh - c['s1'] / M - (zd - c['mean']) * c['rstd'] * c['s2'] / M)
        for name, t, ref in (('dz', dz, rdz), ('dx', dx, rdz @ T['W'].double()), ('acc1', a1, T['acc'][0].double() + c['s1']),
                             ('acc2', a2, T['acc'][1].double() + c['s2'])):
            ws.no_leak(t, f'{what} {name}')
            gate(t, ref, f'{what} {name}')
        ws.neighbours(what)
        _, gmc, dzc, dxc, _, _ = run('W0', M)
        ops.run_gemm([gmc], DEV)
        assert torch.equal(dz, dzc) and torch.equal(dx, dxc), what


def test_run_gemm_refuses_an_out_that_is_not_row_major():
    """ops.run_gemm took `Gemm.out` as it was and Gemm.desc passed ldy = out.stride(0): an `out` whose columns are not unit-stride
    would have been written as if it were row-major.
    FOUND by this test: `buf[:, ::2]` (row stride 2N >= N, column stride 2) passed every check of the C ABI and received a
    row-major image -- the odd columns of `buf` overwritten, half of the window never written; `buf.t()` (row stride 1) was
    refused only by the C entry's ldy < N (one row, or N = 1, passed).  run_gemm now refuses such an `out` itself."""
    g = torch.Generator().manual_seed(5)
    M, N, K = 33, 40, 24
    X, W = _rand(g, M, K).to(DEV), _rand(g, N, K).to(DEV)
    for name in ('buf.t()', 'buf[:, ::2]'):
        buf = torch.full((N, M) if name == 'buf.t()' else (M, 2 * N), SENT, device=DEV)
        view = buf.t() if name == 'buf.t()' else buf[:, ::2]
        assert tuple(view.shape) == (M, N)
        with pytest.raises(ValueError, match='row-major'):
            ops.run_gemm([ops.Gemm(X=X, W=W, out=view)], DEV)
        torch.cuda.synchronize()
        assert bool((buf == SENT).all()), f'{name}: written although refused'
    # (what is row-major is still served: a column window, and one row of anything)
    wide = torch.full((M, N + 8), SENT, device=DEV)
    ops.run_gemm([ops.Gemm(X=X, W=W, out=wide[:, 4:4 + N])], DEV)
    gate(wide[:, 4:4 + N], X.cpu().double() @ W.cpu().double().t(), 'run_gemm out = a column window')
    assert bool((wide[:, :4] == SENT).all()) and bool((wide[:, 4 + N:] == SENT).all())


# ------------------------------------------------------------------------------------------------------------------------------
# 2. cwn_gemm_tn_f32
# ------------------------------------------------------------------------------------------------------------------------------
def _tn_run(cls, N, K, K2, M, T, deterministic):
    ws = Windows(DEV)
    off = VEC_OFF[cls]
    dZ, X = ws.inp('dZ', T['dZ'][:M], cls), ws.inp('X', T['X'][:M], cls)
    X2 = ws.inp('X2', T['X2'][:M], cls) if K2 else None
    sc, sh = ws.vec('in_scale', T['sc'], off), ws.vec('in_shift', T['sh'], off)
    dW = ws.out('dW', N, K + K2, cls, prefill=T['dW0'])
    db = ws.vec('db', T['db0'], off, out=True)
    d = _ffi.GemmTnDesc(dZ=dZ.data_ptr(), X=X.data_ptr(), X2=_ffi.ptr(X2), in_scale=sc.data_ptr(), in_shift=sh.data_ptr(),
                        in_scale2=None, in_shift2=None, dW=dW.data_ptr(), db=db.data_ptr(), M=M, lddz=dZ.stride(0), ldx=X.stride(0),
                        ldx2=X2.stride(0) if K2 else 0, lddw=dW.stride(0), N=N, K=K, K2=K2, in_relu=1)
    would = _ffi.gemm_tn_would_split([d])
    prev = _ffi.DETERMINISTIC_TN
    _ffi.DETERMINISTIC_TN = deterministic
    try:
        _ffi.gemm_tn([d], DEV)
    finally:
        _ffi.DETERMINISTIC_TN = prev
    return ws, dW, db, would


@pytest.mark.parametrize('deterministic', [False, True])
@pytest.mark.parametrize('cls', ALL)
@pytest.mark.parametrize('N,K,K2', [(128, 128, 0), (128, 64, 64), (64, 64, 64), (40, 24, 12), (37, 23, 0)])
def test_gemm_tn_windows(N, K, K2, cls, deterministic):
    """cwn_gemm_tn_f32 (csrc/cwn_gemm_tn.hip): dZ, X and X2 as windows, dW a pre-filled window with lddw > K + K2 (it is ADDED
    to: the window holds pre-fill + the product, its neighbours their sentinel), db and the prologue vectors inside longer
    ones.  The bf16-split form (N > 64, cwn_gemm_tn_would_split: W0 / W1 only) and the fp32 form with 16-byte and with element
    loads; 37 x 23 has no width that is a multiple of 4.  The deterministic (workspace) form is held to bit-identity with
    contiguous copies in W0 / W1, where the same kernel form serves both; the atomic form and the classes that change the form
    are held to the gate."""
    g = torch.Generator().manual_seed(N + 3 * K + 7 * K2)
    Mx = max(ROWS)
    T = {'dZ': _rand(g, Mx, N), 'X': _rand(g, Mx, K), 'X2': _rand(g, Mx, max(K2, 1)), 'sc': torch.rand(K, generator=g) + 0.5,
         'sh': _rand(g, K), 'dW0': _rand(g, N, K + K2), 'db0': _rand(g, N)}
    widths_ok = N % 4 == 0 and K % 4 == 0 and K2 % 4 == 0
    for M in ROWS:
        what = f'gemm_tn {N}x{K}+{K2} {cls} det={deterministic} M={M}'
        ws, dW, db, would = _tn_run(cls, N, K, K2, M, T, deterministic)
        assert would == (N > 64 and widths_ok and cls in VECTOR_OK), (what, would)
        vec = cls in VECTOR_OK and widths_ok
        _form(what, 'bf16-split kernel' if would else f'fp32 kernel, {"16-byte" if vec else "element"} loads')
        A = torch.relu(T['X'][:M].double() * T['sc'].double() + T['sh'].double())
        if K2:
            A = torch.cat([A, T['X2'][:M].double()], 1)
        ws.no_leak(dW, what + ' dW')
        ws.no_leak(db, what + ' db')
        gate(dW, T['dW0'].double() + T['dZ'][:M].double().t() @ A, what + ' dW')
        gate(db, T['db0'].double() + T['dZ'][:M].double().sum(0), what + ' db')
        ws.neighbours(what)
        if deterministic and cls in VECTOR_OK:
            _, dWc, dbc, would_c = _contig(_tn_run, N, K, K2, M, T, True)
            assert would_c == would, what
            assert torch.equal(dW, dWc) and torch.equal(db, dbc), f'{what}: not the bits of the launch on contiguous copies'


# ------------------------------------------------------------------------------------------------------------------------------
# 3. cwn_dense_stage_f32 / cwn_dense_stage_ex_f32 / cwn_dense_stage_bwd_f32
# ------------------------------------------------------------------------------------------------------------------------------
STAGE_CLASSES = ('W0', 'W1', 'S12', 'W2', 'W3')       # S12: (0, 12), a larger stride that is a multiple of 4
_STAGE = dict(CLASSES, S12=(0, 12))


def _cls(c):
    return _STAGE[c]


def _stage_weight(g, F, blocks):
    W = torch.nn.Parameter((_rand(g, F, blocks * F) / (blocks * F) ** 0.5).to(DEV))
    ops.pack_stage_weights_many([W])
    return W


def _stage_desc(ws, c, M, F, blocks, T, W, halves):
    """The cwn_stage_desc (and extras) of one product with `blocks` K-blocks over windows of class c.  halves: X and X2 are the
    two halves of ONE wider matrix (the torch.cat of combine_nn, never written)."""
    off = 4 if c == 'W1' else 0                          # (the constants: 16-byte aligned in every class)
    if halves and blocks >= 2:
        buf = torch.full((M, 2 * F + _cls(c)[1]), NAN)
        c0 = _cls(c)[0]
        buf[:, c0:c0 + F], buf[:, c0 + F:c0 + 2 * F] = T['X'][:M], T['X2'][:M]
        buf = buf.to(DEV)
        ws._keep('X|X2', buf, None)
        Xs = [buf[:, c0:c0 + F], buf[:, c0 + F:c0 + 2 * F]] + ([ws.inp('X3', T['X3'][:M], _cls(c))] if blocks == 3 else [])
    else:
        Xs = [ws.inp(n, T[n][:M], _cls(c)) for n in ('X', 'X2', 'X3')[:blocks]]
    Y = ws.out('Y', M, F, _cls(c))
    v = {k: ws.vec(k, T[k], off) for k in ('bias', 'sc', 'sh', 'sc2', 'sh2')}
    bands = ops.stat_rows(M)
    cs, cq = (torch.full((bands, F), SENT, dtype=torch.float64, device=DEV) for _ in range(2))
    two = blocks >= 2
    d = _ffi.StageDesc(X=Xs[0].data_ptr(), X2=Xs[1].data_ptr() if two else None, w_packed=ops.packed_stage_block(W, 0).data_ptr(),
                       w2_packed=ops.packed_stage_block(W, F).data_ptr() if two else None, bias=v['bias'].data_ptr(),
                       in_scale=v['sc'].data_ptr(), in_shift=v['sh'].data_ptr(), in_scale2=v['sc2'].data_ptr() if two else None,
                       in_shift2=v['sh2'].data_ptr() if two else None, Y=Y.data_ptr(), col_sum=cs.data_ptr(), col_sumsq=cq.data_ptr(),
                       M=M, ldx=Xs[0].stride(0), ldx2=Xs[1].stride(0) if two else 0, ldy=Y.stride(0), in_relu=3 if two else 1)
    ex = None
    if blocks == 3:
        ex = (_ffi.StageExtra * 2)()
        ex[0].X, ex[0].w_packed, ex[0].ldx, ex[0].relu = Xs[2].data_ptr(), ops.packed_stage_block(W, 2 * F).data_ptr(), Xs[2].stride(0), 1
    return d, ex, Xs, Y, cs, cq, v


def _stage_call(d, ex, F):
    arr = (_ffi.StageDesc * 1)(d)
    if ex is None:
        return _ffi.lib().cwn_dense_stage_f32(arr, 1, F, _stream())
    return _ffi.lib().cwn_dense_stage_ex_f32(arr, ex, 1, F, _stream())


@pytest.mark.parametrize('F', [64, 128])
@pytest.mark.parametrize('form', ['single', 'cat', 'cat_halves', 'ex'])
@pytest.mark.parametrize('cls', STAGE_CLASSES)
def test_dense_stage_windows(cls, form, F):
    """cwn_dense_stage_f32 / cwn_dense_stage_ex_f32 (csrc/cwn_stage.hip): "pointers 16-B aligned, strides multiples of 4" -- X,
    X2, the extra block and Y as windows in W0, W1 and a larger stride (0, 12); `cat_halves`: X and X2 the two halves of one
    wider matrix.  Y and the band statistics against float64, bit-identical to contiguous copies (one kernel form).  W2 (a
    pointer off 16 bytes: CWN_ERR_ALIGN) and W3 (a stride that is no multiple of 4: CWN_ERR_BAD_ARG) are refused before the
    launch with nothing written, and ops.run_stage declines them (None) so that its caller's cwn_gemm_f32 launch serves the
    same windows."""
    blocks = {'single': 1, 'cat': 2, 'cat_halves': 2, 'ex': 3}[form]
    g = torch.Generator().manual_seed(F + 5 * blocks)
    W = _stage_weight(g, F, blocks)
    Wc = W.detach().cpu().double()
    Mx = max(ROWS)
    T = {'X': _rand(g, Mx, F), 'X2': _rand(g, Mx, F), 'X3': _rand(g, Mx, F), 'bias': _rand(g, F),
         'sc': torch.rand(F, generator=g) + 0.5, 'sh': _rand(g, F), 'sc2': torch.rand(F, generator=g) + 0.5, 'sh2': _rand(g, F)}
    for M in ROWS:
        what = f'stage {form} F={F} {cls} M={M}'
        ws = Windows(DEV)
        d, ex, Xs, Y, cs, cq, v = _stage_desc(ws, cls, M, F, blocks, T, W, form == 'cat_halves')
        x = [(T['X'][:M].double() * T['sc'].double() + T['sh'].double()).relu()]
        if blocks >= 2:
            x.append((T['X2'][:M].double() * T['sc2'].double() + T['sh2'].double()).relu())
        if blocks == 3:
            x.append(T['X3'][:M].double().relu())
        ref = torch.cat(x, 1) @ Wc.t() + T['bias'].double()
        rc = _stage_call(d, ex, F)
        if cls in FORBIDDEN:
            torch.cuda.synchronize()
            assert rc == FORBIDDEN[cls], (what, rc)
            ws.unchanged(what)
            assert bool((cs == SENT).all()) and bool((cq == SENT).all()), what
            _form(what, f'refused (code {rc}), nothing written')
            if blocks <= 2:                  # (the wrapper: declines, and the same windows run on cwn_gemm_f32)
                gm = ops.Gemm(X=Xs[0], X2=Xs[1] if blocks == 2 else None, W=W.detach(), bias=v['bias'], in_scale=v['sc'],
                              in_shift=v['sh'], in_scale2=v['sc2'] if blocks == 2 else None,
                              in_shift2=v['sh2'] if blocks == 2 else None, in_relu=3 if blocks == 2 else 1)
                assert ops.run_stage([gm], DEV) is None, what
                out = ops.run_gemm([gm], DEV)[0]
                ws.no_leak(out, what + ' (cwn_gemm_f32)')
                gate(out, ref, what + ' (cwn_gemm_f32)')
                ws.unchanged(what)
            continue
        _ffi.check(rc, 'cwn_dense_stage_f32')
        _form(what, 'stage kernel (bf16 split, 16-byte accesses)')
        ws.no_leak(Y, what)
        gate(Y, ref, what + ' Y')
        zp = torch.cat([ref, ref.new_zeros((-M) % 32, F)]).view(-1, 32, F)
        gate(cs, zp.sum(1), what + ' col_sum')
        gate(cq, (zp * zp).sum(1), what + ' col_sumsq')
        ws.neighbours(what)
        wc = Windows(DEV)
        dc, exc, _, Yc, csc, cqc, _ = _stage_desc(wc, 'W0', M, F, blocks, T, W, False)
        _ffi.check(_stage_call(dc, exc, F), 'cwn_dense_stage_f32')
        assert torch.equal(Y, Yc) and torch.equal(cs, csc) and torch.equal(cq, cqc), f'{what}: not the bits of the contiguous launch'


@pytest.mark.parametrize('F', [64, 128])
@pytest.mark.parametrize('halves', ['separate', 'halves', 'halves_reversed'])
@pytest.mark.parametrize('cls', STAGE_CLASSES)
def test_dense_stage_backward_windows(cls, halves, F):
    """cwn_dense_stage_bwd_f32 (csrc/cwn_stage.hip): dy and z as windows, dz an output window, dx and dx2 as windows of their own
    or as the two halves of ONE wider matrix (the gradient of a torch.cat, written in place) in either order; the constants
    and sums 16-byte aligned inside longer vectors, acc1 / acc2 pre-filled.  dz = scale * (dyh - s1 / M - xhat * s2 / M) and
    dx = dz W against float64, bit-identical to contiguous copies.  W2 (CWN_ERR_ALIGN) and W3 (CWN_ERR_BAD_ARG) are refused
    before the launch with nothing written, and ops.run_stage_bwd declines them (False, nothing launched)."""
    g = torch.Generator().manual_seed(17 * F + len(halves))
    W = _stage_weight(g, F, 2)
    Wc = W.detach().cpu().double()
    Mx = max(ROWS)
    T = {'dy': _rand(g, Mx, F), 'z': _rand(g, Mx, F) * 2 + 0.5, 'acc': _rand(g, 2, F)}
    con = {'scale': torch.rand(F, generator=g) + 0.5, 'shift': _rand(g, F), 'mean': _rand(g, F), 'rstd': torch.rand(F, generator=g) + 0.5,
           's1': _rand(g, F), 's2': _rand(g, F)}

    def build(c, M, how):
        ws = Windows(DEV)
        off = 4 if c == 'W1' else 0
        dy, z = ws.inp('dy', T['dy'][:M], _cls(c)), ws.inp('z', T['z'][:M], _cls(c))
        dz = ws.out('dz', M, F, _cls(c))
        if how == 'separate':
            dx, dx2 = ws.out('dx', M, F, _cls(c)), ws.out('dx2', M, F, _cls(c))
        else:
            dx, dx2 = ws.halves('dx|dx2', M, F, _cls(c), reverse=how == 'halves_reversed')
        v = {k: ws.vec(k, t, off) for k, t in con.items()}
        a1, a2 = ws.vec('acc1', T['acc'][0], off, out=True), ws.vec('acc2', T['acc'][1], off, out=True)
        d = _ffi.StageBwdDesc(dy=dy.data_ptr(), z=z.data_ptr(), dz=dz.data_ptr(), scale=v['scale'].data_ptr(), shift=v['shift'].data_ptr(),
                              mean=v['mean'].data_ptr(), rstd=v['rstd'].data_ptr(), s1=v['s1'].data_ptr(), s2=v['s2'].data_ptr(),
                              acc1=a1.data_ptr(), acc2=a2.data_ptr(), wt_packed=ops.packed_stage_block(W, 0, transposed=True).data_ptr(),
                              wt2_packed=ops.packed_stage_block(W, F, transposed=True).data_ptr(), dx=dx.data_ptr(), dx2=dx2.data_ptr(),
                              M=M, lddy=dy.stride(0), ldz=z.stride(0), lddz=dz.stride(0), lddx=dx.stride(0), lddx2=dx2.stride(0), relu=1)
        bnb = _ffi.GemmBnb(z=z.data_ptr(), dz=dz.data_ptr(), scale=v['scale'].data_ptr(), shift=v['shift'].data_ptr(),
                           mean=v['mean'].data_ptr(), rstd=v['rstd'].data_ptr(), s1=v['s1'].data_ptr(), s2=v['s2'].data_ptr(),
                           acc1=a1.data_ptr(), acc2=a2.data_ptr(), ldz=z.stride(0), lddz=dz.stride(0), relu=1)
        return ws, d, (dy, bnb, W.detach(), dx, dx2), dz, dx, dx2, a1, a2

    for M in ROWS:
        what = f'stage bwd {halves} F={F} {cls} M={M}'
        ws, d, entry, dz, dx, dx2, a1, a2 = build(cls, M, halves)
        rc = _ffi.lib().cwn_dense_stage_bwd_f32((_ffi.StageBwdDesc * 1)(d), 1, F, _stream())
        if cls in FORBIDDEN:
            torch.cuda.synchronize()
            assert rc == FORBIDDEN[cls], (what, rc)
            ws.unchanged(what)
            assert ops.run_stage_bwd([entry], DEV) is False, what
            torch.cuda.synchronize()
            ws.unchanged(what)
            _form(what, f'refused (code {rc}), nothing written; ops.run_stage_bwd declines')
            continue
        _ffi.check(rc, 'cwn_dense_stage_bwd_f32')
        _form(what, 'stage backward kernel (bf16 split, 16-byte accesses)')
        c = {k: t.double() for k, t in con.items()}
        dyd, zd = T['dy'][:M].double(), T['z'][:M].double()
        dyh = dyd * (zd * c['scale'] + c['shift'] > 0)
        rdz = c['scale'] * (dyh - c['s1'] / M - (zd - c['mean']) * c['rstd'] * c['s2'] / M)
        rdx = rdz @ Wc
        for name, t, ref in (('dz', dz, rdz), ('dx', dx, rdx[:, :F]), ('dx2', dx2, rdx[:, F:]),
                             ('acc1', a1, T['acc'][0].double() + c['s1']), ('acc2', a2, T['acc'][1].double() + c['s2'])):
            ws.no_leak(t, f'{what} {name}')
            gate(t, ref, f'{what} {name}')
        ws.neighbours(what)
        _, dc, _, dzc, dxc, dx2c, _, _ = build('W0', M, 'separate')
        _ffi.check(_ffi.lib().cwn_dense_stage_bwd_f32((_ffi.StageBwdDesc * 1)(dc), 1, F, _stream()), 'cwn_dense_stage_bwd_f32')
        assert torch.equal(dz, dzc) and torch.equal(dx, dxc) and torch.equal(dx2, dx2c), f'{what}: not the bits of the contiguous launch'


# ------------------------------------------------------------------------------------------------------------------------------
# 4. cwn_update_mlp_f32 / cwn_update_mlp3_f32
# ------------------------------------------------------------------------------------------------------------------------------
def _mlp_net(g, F, w_in, branches):
    lins, folds = [], []
    shapes = [(F, w_in), (F, F)] * branches + [(F, branches * F)]
    for k, (o, i) in enumerate(shapes):
        lin = torch.nn.Linear(i, o)
        with torch.no_grad():
            lin.weight.copy_(_rand(g, o, i) / i ** 0.5)
            lin.bias.copy_(_rand(g, o) * 0.5)
        lins.append(lin.to(DEV))
        folds.append((None, None) if k == 1 else (torch.rand(o, generator=g) + 0.5, _rand(g, o) * 0.3))
    return lins, folds


def _mlp_ref(xs, lins, folds, M):
    def stage(k, x):
        y = x @ lins[k].weight.detach().cpu().double().t() + lins[k].bias.detach().cpu().double()
        if folds[k][0] is not None:
            y = y * folds[k][0].double() + folds[k][1].double()
        return y.relu()
    hs = [stage(2 * b + 1, stage(2 * b, x[:M].double())) for b, x in enumerate(xs)]
    return stage(len(lins) - 1, torch.cat(hs, 1))


def _mlp_epilogues(ws, a, lins, folds, off):
    for k, (lin, (sc, sh)) in enumerate(zip(lins, folds)):
        a.bias[k] = ws.vec(f'bias{k}', lin.bias.detach().cpu(), off).data_ptr()
        a.scale[k] = None if sc is None else ws.vec(f'scale{k}', sc, off).data_ptr()
        a.shift[k] = None if sh is None else ws.vec(f'shift{k}', sh, off).data_ptr()


def _mlp_dev_folds(folds):
    return [(None if s is None else s.to(DEV), None if t is None else t.to(DEV)) for s, t in folds]


@pytest.mark.parametrize('F', [64, 128])
@pytest.mark.parametrize('cls', ['W0', 'W1', 'W2', 'W3'])
def test_update_mlp_windows(cls, F):
    """cwn_update_mlp_f32 (csrc/cwn_mlp.hip) with F-wide inputs: "every pointer 16-B aligned, row strides multiples of 4" -- x_up,
    x_b and y as windows, every bias / scale / shift 16-byte aligned inside a longer vector; y against float64 through all
    five Linear layers and bit-identical to contiguous copies.  W2 (CWN_ERR_ALIGN) and W3 (CWN_ERR_BAD_ARG) are refused before
    the launch, nothing written.
    FOUND by this test: ops.update_mlp (and MlpLaunch.run, in both bindings) handed an F-wide window that is row-major but off
    16 bytes or with a stride that is no multiple of 4 straight to the entry point, whose refusal surfaced as a CwnError where
    every neighbouring wrapper copies; the wrappers now copy such an operand (a clone: ONE row off 16 bytes is "contiguous" to
    torch as it lies, `.contiguous()` hands it back)."""
    g = torch.Generator().manual_seed(3 * F)
    lins, folds = _mlp_net(g, F, F, 2)
    Mx = max(ROWS)
    T = {'xu': _rand(g, Mx, F) * 2, 'xb': _rand(g, Mx, F) * 2}
    packed = []
    for l in lins:
        packed += list(ops.pack_mlp_weight(l.weight))

    def build(c, M):
        ws = Windows(DEV)
        xu, xb, y = ws.inp('xu', T['xu'][:M], c), ws.inp('xb', T['xb'][:M], c), ws.out('y', M, F, c)
        arr = (_ffi.MlpDim * 1)()
        a = arr[0]
        a.x_up, a.x_b, a.y, a.M, a.ldx_up, a.ldx_b, a.ldy, a.in_width = xu.data_ptr(), xb.data_ptr(), y.data_ptr(), M, xu.stride(0), \
            xb.stride(0), y.stride(0), 0
        for k, pk in enumerate(packed):
            a.w_packed[k] = pk.data_ptr()
        _mlp_epilogues(ws, a, lins, folds, 4 if c == 'W1' else 0)
        return ws, arr, xu, xb, y

    for M in ROWS:
        what = f'update_mlp F={F} {cls} M={M}'
        ws, arr, xu, xb, y = build(cls, M)
        ref = _mlp_ref([T['xu'], T['xb']], lins, folds, M)
        rc = _ffi.lib().cwn_update_mlp_f32(arr, 1, F, _stream())
        if cls in FORBIDDEN:
            torch.cuda.synchronize()
            assert rc == FORBIDDEN[cls], (what, rc)
            ws.unchanged(what)
            dims = [ops.MlpDim(x_up=xu, x_b=xb, linears=lins, folds=_mlp_dev_folds(folds))]
            assert ops.update_mlp_applies(dims), what
            out = ops.update_mlp(dims)[0]
            ws.no_leak(out, what + ' (ops.update_mlp)')
            gate(out, ref, what + ' (ops.update_mlp)')
            out2 = ops.MlpLaunch(dims, []).run([xu], [xb])[0]
            assert torch.equal(out, out2), what + ' (ops.MlpLaunch)'
            ws.unchanged(what)
            _form(what, f'refused (code {rc}), nothing written; ops.update_mlp / MlpLaunch copy the operand')
            continue
        _ffi.check(rc, 'cwn_update_mlp_f32')
        _form(what, 'update / combine kernel, 16-byte row loads')
        ws.no_leak(y, what)
        gate(y, ref, what)
        ws.neighbours(what)
        _, arrc, _, _, yc = build('W0', M)
        _ffi.check(_ffi.lib().cwn_update_mlp_f32(arrc, 1, F, _stream()), 'cwn_update_mlp_f32')
        assert torch.equal(y, yc), f'{what}: not the bits of the contiguous launch'


@pytest.mark.parametrize('F', [64, 128])
@pytest.mark.parametrize('w_in', [1, 3, 20])
@pytest.mark.parametrize('cls', ALL)
def test_update_mlp_narrow_input_windows(cls, w_in, F):
    """cwn_mlp_dim.in_width = 1, 3, 20: "the row strides may be any value >= in_width and the two pointers need 4-byte alignment
    only" -- x_up / x_b in every class (the rows are staged element-wise and zero-padded: the NaN behind column in_width of a
    row must not reach the tile), y in the class where the entry takes it (W0 / W1; contiguous otherwise).  Bit-identical to
    contiguous copies: one kernel form."""
    g = torch.Generator().manual_seed(3 * F + w_in)
    lins, folds = _mlp_net(g, F, w_in, 2)
    Mx = max(ROWS)
    T = {'xu': _rand(g, Mx, w_in) * 2, 'xb': _rand(g, Mx, w_in) * 2}
    packed = []
    for k, l in enumerate(lins):
        packed += list(ops.pack_mlp_weight(ops._mlp_first_weight(l.weight, F) if k in (0, 2) else l.weight))

    def run(c, M):
        ws = Windows(DEV)
        cy = c if c in VECTOR_OK else 'W0'
        xu, xb, y = ws.inp('xu', T['xu'][:M], c), ws.inp('xb', T['xb'][:M], c), ws.out('y', M, F, cy)
        arr = (_ffi.MlpDim * 1)()
        a = arr[0]
        a.x_up, a.x_b, a.y, a.M, a.ldx_up, a.ldx_b, a.ldy, a.in_width = xu.data_ptr(), xb.data_ptr(), y.data_ptr(), M, xu.stride(0), \
            xb.stride(0), y.stride(0), w_in
        for k, pk in enumerate(packed):
            a.w_packed[k] = pk.data_ptr()
        _mlp_epilogues(ws, a, lins, folds, 4 if cy == 'W1' else 0)
        _ffi.check(_ffi.lib().cwn_update_mlp_f32(arr, 1, F, _stream()), 'cwn_update_mlp_f32')
        return ws, y

    for M in ROWS:
        what = f'update_mlp F={F} in_width={w_in} {cls} M={M}'
        ws, y = run(cls, M)
        _form(what, 'update / combine kernel, narrow inputs staged element-wise')
        ws.no_leak(y, what)
        gate(y, _mlp_ref([T['xu'], T['xb']], lins, folds, M), what)
        ws.neighbours(what)
        _, yc = run('W0', M)
        assert torch.equal(y, yc), f'{what}: not the bits of the contiguous launch'


@pytest.mark.parametrize('F', [64, 128])
@pytest.mark.parametrize('cls', ['W0', 'W1', 'W2', 'W3'])
def test_update_mlp3_windows(cls, F):
    """cwn_update_mlp3_f32 (csrc/cwn_mlp3.hip): "same limits, alignment and arithmetic as cwn_update_mlp_f32" -- the three inputs
    and y as windows; W2 / W3 refused before the launch, and served by ops.update_mlp3 through a copy (FOUND by this test: it
    passed such a window through to the refusal, as ops.update_mlp did)."""
    g = torch.Generator().manual_seed(5 * F)
    lins, folds = _mlp_net(g, F, F, 3)
    Mx = max(ROWS)
    T = {f'x{k}': _rand(g, Mx, F) * 2 for k in range(3)}
    wc = ops.pack_mlp_weight(lins[6].weight)
    packed = []
    for k in range(3):
        packed += [ops.pack_mlp_weight(lins[2 * k].weight)[0], ops.pack_mlp_weight(lins[2 * k + 1].weight)[0], wc[k]]

    def build(c, M):
        ws = Windows(DEV)
        xs = [ws.inp(f'x{k}', T[f'x{k}'][:M], c) for k in range(3)]
        y = ws.out('y', M, F, c)
        arr = (_ffi.Mlp3Dim * 1)()
        a = arr[0]
        for k in range(3):
            a.x[k], a.ldx[k] = xs[k].data_ptr(), xs[k].stride(0)
        a.y, a.M, a.ldy = y.data_ptr(), M, y.stride(0)
        for k, pk in enumerate(packed):
            a.w_packed[k] = pk.data_ptr()
        _mlp_epilogues(ws, a, lins, folds, 4 if c == 'W1' else 0)
        return ws, arr, xs, y

    for M in ROWS:
        what = f'update_mlp3 F={F} {cls} M={M}'
        ws, arr, xs, y = build(cls, M)
        ref = _mlp_ref([T['x0'], T['x1'], T['x2']], lins, folds, M)
        rc = _ffi.lib().cwn_update_mlp3_f32(arr, 1, F, _stream())
        if cls in FORBIDDEN:
            torch.cuda.synchronize()
            assert rc == FORBIDDEN[cls], (what, rc)
            ws.unchanged(what)
            dims = [ops.Mlp3Dim(xs=xs, linears=lins, folds=_mlp_dev_folds(folds))]
            assert ops.update_mlp3_applies(dims), what
            out = ops.update_mlp3(dims)[0]
            ws.no_leak(out, what + ' (ops.update_mlp3)')
            gate(out, ref, what + ' (ops.update_mlp3)')
            ws.unchanged(what)
            _form(what, f'refused (code {rc}), nothing written; ops.update_mlp3 copies the operand')
            continue
        _ffi.check(rc, 'cwn_update_mlp3_f32')
        _form(what, 'CIN++ update / combine kernel, 16-byte row loads')
        ws.no_leak(y, what)
        gate(y, ref, what)
        ws.neighbours(what)
        _, arrc, _, yc = build('W0', M)
        _ffi.check(_ffi.lib().cwn_update_mlp3_f32(arrc, 1, F, _stream()), 'cwn_update_mlp3_f32')
        assert torch.equal(y, yc), f'{what}: not the bits of the contiguous launch'


# ------------------------------------------------------------------------------------------------------------------------------
# 5. cwn_norm_act_f32 / cwn_norm_bwd_reduce_f32 / cwn_norm_bwd_apply_f32 / cwn_norm_bwd_f32
# ------------------------------------------------------------------------------------------------------------------------------
SEED, STEP, SITE, P = 1234567, 3, 5, 0.5


def _drop_state():
    return torch.tensor([SEED, STEP], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize('N', [64, 37, 130])
@pytest.mark.parametrize('cls', ALL)
def test_norm_pieces_windows(cls, N):
    """cwn_norm_act_f32, cwn_norm_bwd_reduce_f32 (with dropout on the incoming gradient and dy_out / lddy_out) and
    cwn_norm_bwd_apply_f32 (csrc/cwn_norm.hip): "16-byte accesses where pointer, stride and widths allow, element by element
    otherwise" -- z, dy, out and dy_out as windows, scale / shift / mean / rstd / s1 / s2 inside longer vectors (s1 / s2 and acc1
    / acc2 pre-filled: they are added to).  N = 64 takes the 16-byte form in W0 / W1 and the element-wise one in W2 - W4;
    N = 37 and 130 are element-wise everywhere.  dy_out (a product with 0 or 2) has the bits of the contiguous launch in every
    class, the activation wherever the same form serves both (the header promises no common order for the two forms: there
    the comparison is printed); the column sums s1 / s2 are atomic adds, dz depends on them: the gate."""
    from tests._philox_ref import multipliers
    g = torch.Generator().manual_seed(7 * N)
    Mx = max(ROWS)
    T = {'z': _rand(g, Mx, N) * 2 + 0.5, 'dy': _rand(g, Mx, N), 's0': _rand(g, 2, N), 'acc0': _rand(g, 2, N)}
    con = {'scale': torch.rand(N, generator=g) + 0.5, 'shift': _rand(g, N), 'mean': _rand(g, N), 'rstd': torch.rand(N, generator=g) + 0.5}
    state = _drop_state()

    def run(c, M):
        ws = Windows(DEV)
        off = VEC_OFF[c]
        z, dy = ws.inp('z', T['z'][:M], c), ws.inp('dy', T['dy'][:M], c)
        H, dyo, dz = ws.out('out', M, N, c), ws.out('dy_out', M, N, c), ws.out('dz', M, N, c)
        v = {k: ws.vec(k, t, off) for k, t in con.items()}
        s1, s2 = ws.vec('s1', T['s0'][0], off, out=True), ws.vec('s2', T['s0'][1], off, out=True)
        a1, a2 = ws.vec('acc1', T['acc0'][0], off, out=True), ws.vec('acc2', T['acc0'][1], off, out=True)

        def desc(**kw):
            d = _ffi.NormDesc(z=z.data_ptr(), scale=v['scale'].data_ptr(), shift=v['shift'].data_ptr(), mean=v['mean'].data_ptr(),
                              rstd=v['rstd'].data_ptr(), s1=s1.data_ptr(), s2=s2.data_ptr(), M=M, ldz=z.stride(0), N=N, relu=1)
            for k, val in kw.items():
                setattr(d, k, val)
            return d
        vec = all(aligned16(t) for t in (z, dy, H, dyo, dz, s1, v['scale'])) and N % 4 == 0 and z.stride(0) % 4 == 0
        _ffi.norm_act([desc(out=H.data_ptr(), ldout=H.stride(0))], DEV)
        _ffi.norm_bwd_reduce([desc(dy=dy.data_ptr(), lddy=dy.stride(0), dy_out=dyo.data_ptr(), lddy_out=dyo.stride(0),
                                   drop=_ffi.Dropout(state=state.data_ptr(), p=P, site=SITE))], DEV)
        _ffi.norm_bwd_apply([desc(dy=dyo.data_ptr(), lddy=dyo.stride(0), out=dz.data_ptr(), ldout=dz.stride(0), acc1=a1.data_ptr(),
                                  acc2=a2.data_ptr())], DEV)
        return ws, vec, H, dyo, dz, s1, s2, a1, a2

    for M in ROWS:
        what = f'norm N={N} {cls} M={M}'
        ws, vec, H, dyo, dz, s1, s2, a1, a2 = run(cls, M)
        assert vec == (N % 4 == 0 and cls in VECTOR_OK), what
        _form(what, '16-byte form' if vec else 'element-wise form')
        c = {k: t.double() for k, t in con.items()}
        zd = T['z'][:M].double()
        y = zd * c['scale'] + c['shift']
        mult = torch.as_tensor(multipliers((M, N), P, SEED, STEP, SITE)).reshape(M, N).double()
        gd = T['dy'][:M].double() * mult
        dyh = gd * (y > 0)
        xhat = (zd - c['mean']) * c['rstd']
        r1, r2 = T['s0'][0].double() + dyh.sum(0), T['s0'][1].double() + (dyh * xhat).sum(0)
        # (the apply's reference: the formula on the fp32 sums the reduce launch left)
        k1, k2 = s1.cpu().double() / M, s2.cpu().double() / M
        for name, t, ref in (('out', H, y.relu()), ('dy_out', dyo, gd), ('s1', s1, r1), ('s2', s2, r2),
                             ('dz', dz, c['scale'] * (dyh - k1 - xhat * k2)), ('acc1', a1, T['acc0'][0].double() + s1.cpu().double()),
                             ('acc2', a2, T['acc0'][1].double() + s2.cpu().double())):
            ws.no_leak(t, f'{what} {name}')
            gate(t, ref, f'{what} {name}')
        ws.neighbours(what)
        _, vec_c, Hc, dyoc, dzc, _, _, _, _ = run('W0', M)
        assert torch.equal(dyo, dyoc), f'{what}: dy_out is not the bits of the contiguous launch'      # (a product with 0 or 2)
        same = torch.equal(H, Hc)
        print(f'[window] {what}: out {"has" if same else "has NOT"} the bits of the contiguous launch ({"same" if vec == vec_c else "other"} form)')
        assert same or vec != vec_c, f'{what}: not the bits of the contiguous launch'


@pytest.mark.parametrize('cls', ['W0', 'W1', 'W2', 'W3'])
def test_norm_backward_fused_windows(cls):
    """cwn_norm_bwd_f32 (reduce + apply in one launch): "needs 16-byte aligned operands and strides (CWN_ERR_ALIGN otherwise)" --
    W0 / W1 run: dz and the WRITTEN s1 / s2 against float64, bit-identical to contiguous copies (no atomics); W2 / W3 are
    refused with CWN_ERR_ALIGN before the launch, nothing written."""
    N = 64
    g = torch.Generator().manual_seed(11)
    Mx = max(ROWS)
    T = {'z': _rand(g, Mx, N) * 2 + 0.5, 'dy': _rand(g, Mx, N)}
    con = {'scale': torch.rand(N, generator=g) + 0.5, 'shift': _rand(g, N), 'mean': _rand(g, N), 'rstd': torch.rand(N, generator=g) + 0.5}

    def build(c, M):
        ws = Windows(DEV)
        off = 4 if c == 'W1' else 0
        z, dy, dz = ws.inp('z', T['z'][:M], c), ws.inp('dy', T['dy'][:M], c), ws.out('dz', M, N, c)
        v = {k: ws.vec(k, t, off) for k, t in con.items()}
        s1, s2 = ws.vec('s1', torch.full((N,), SENT), off, out=True), ws.vec('s2', torch.full((N,), SENT), off, out=True)
        d = _ffi.NormDesc(dy=dy.data_ptr(), z=z.data_ptr(), scale=v['scale'].data_ptr(), shift=v['shift'].data_ptr(),
                          mean=v['mean'].data_ptr(), rstd=v['rstd'].data_ptr(), s1=s1.data_ptr(), s2=s2.data_ptr(), out=dz.data_ptr(), M=M,
                          lddy=dy.stride(0), ldz=z.stride(0), ldout=dz.stride(0), N=N, relu=1)
        return ws, d, dz, s1, s2

    for M in ROWS:
        what = f'norm_bwd (one launch) {cls} M={M}'
        ws, d, dz, s1, s2 = build(cls, M)
        rc = _ffi.lib().cwn_norm_bwd_f32((_ffi.NormDesc * 1)(d), 1, 0, _stream())
        if cls in FORBIDDEN:
            torch.cuda.synchronize()
            assert rc == ALIGN, (what, rc)
            ws.unchanged(what)
            _form(what, 'refused (CWN_ERR_ALIGN), nothing written')
            continue
        _ffi.check(rc, 'cwn_norm_bwd_f32')
        _form(what, 'fused reduce + apply kernel')
        c = {k: t.double() for k, t in con.items()}
        zd = T['z'][:M].double()
        dyh = T['dy'][:M].double() * (zd * c['scale'] + c['shift'] > 0)
        xhat = (zd - c['mean']) * c['rstd']
        r1, r2 = dyh.sum(0), (dyh * xhat).sum(0)
        for name, t, ref in (('s1', s1, r1), ('s2', s2, r2), ('dz', dz, c['scale'] * (dyh - r1 / M - xhat * r2 / M))):
            ws.no_leak(t, f'{what} {name}')
            gate(t, ref, f'{what} {name}')
        ws.neighbours(what)
        _, dc, dzc, s1c, s2c = build('W0', M)
        _ffi.check(_ffi.lib().cwn_norm_bwd_f32((_ffi.NormDesc * 1)(dc), 1, 0, _stream()), 'cwn_norm_bwd_f32')
        assert torch.equal(dz, dzc) and torch.equal(s1, s1c) and torch.equal(s2, s2c), f'{what}: not the bits of the contiguous launch'


# ------------------------------------------------------------------------------------------------------------------------------
# 6. cwn_dropout_f32
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [64, 37, 7])
@pytest.mark.parametrize('in_place', [False, True])
@pytest.mark.parametrize('cls', ALL)
def test_dropout_windows(cls, in_place, N):
    """cwn_dropout_f32 (csrc/cwn_norm.hip): "e = row * N + column of the [M, N] matrix the application covers (row stride
    irrelevant)" -- the multiplier of an element does not depend on the window it lies in: x times tests/_philox_ref's
    multipliers, bit-identical to the contiguous call in EVERY class (the 16-byte form at N = 64 in W0 / W1, the element-wise
    one elsewhere), x == out in place included."""
    from tests._philox_ref import multipliers
    g = torch.Generator().manual_seed(N)
    Mx = max(ROWS)
    X = _rand(g, Mx, N)
    state = _drop_state()
    rec = _ffi.Dropout(state=state.data_ptr(), p=P, site=SITE)

    def run(c, M):
        ws = Windows(DEV)
        if in_place:
            x = out = ws.out('x', M, N, c, prefill=X[:M])
        else:
            x, out = ws.inp('x', X[:M], c), ws.out('out', M, N, c)
        _ffi.check(_ffi.lib().cwn_dropout_f32(x.data_ptr(), out.data_ptr(), M, N, x.stride(0), out.stride(0), C.byref(rec), None,
                                              _stream()), 'cwn_dropout_f32')
        return ws, out, aligned16(x) and aligned16(out) and N % 4 == 0 and x.stride(0) % 4 == 0

    for M in ROWS:
        what = f'dropout N={N} {cls} in_place={in_place} M={M}'
        ws, out, vec = run(cls, M)
        assert vec == (N % 4 == 0 and cls in VECTOR_OK), what
        _form(what, '16-byte form' if vec else 'element-wise form')
        mult = torch.as_tensor(multipliers((M, N), P, SEED, STEP, SITE)).reshape(M, N)
        ws.no_leak(out, what)
        gate(out, X[:M].double() * mult.double(), what)
        assert torch.equal(out.cpu(), X[:M] * mult), what            # (a product with 0 or 2: exact in fp32)
        ws.neighbours(what)
        _, outc, _ = run('W0', M)
        assert torch.equal(out, outc), f'{what}: not the bits of the contiguous call'
    with pytest.raises(ValueError, match='row-major'):               # (the wrapper: an `out` whose columns are strided)
        ops.dropout_apply(X[:4].to(DEV), rec, out=torch.empty(4, 2 * N, device=DEV)[:, ::2])


# ------------------------------------------------------------------------------------------------------------------------------
# 7. cwn_gather_rows_f32
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [8, 6, 37])
@pytest.mark.parametrize('shift', [0, 4, 2, 1])
def test_gather_rows_windows(F, shift):
    """cwn_gather_rows_f32 (csrc/cwn_aggregate.hip) carries no stride: its window is where src and out BEGIN inside a longer
    allocation -- 16 / 8 / 4-byte aligned starts pick the 16 / 8 / 4-byte row copies.  The rows it gathers are exact copies; the
    elements before and behind out keep their sentinel, NaN before and behind src stays out."""
    g = torch.Generator().manual_seed(F + shift)
    n_src, n_idx = 57, max(ROWS)
    src, idx = _rand(g, n_src, F), torch.randint(0, n_src, (n_idx,), generator=g)
    idx[0], idx[1] = 0, n_src - 1                       # (the rows next to the padding)
    ws = Windows(DEV)
    s = ws.vec('src', src.reshape(-1), shift)
    o = ws.vec('out', torch.full((n_idx * F,), SENT), shift, out=True)
    idx_d = idx.to(DEV)
    _ffi.check(_ffi.lib().cwn_gather_rows_f32(s.data_ptr(), n_src, F, idx_d.data_ptr(), n_idx, o.data_ptr(), _stream()),
               'cwn_gather_rows_f32')
    what = f'gather_rows F={F} start +{shift} floats'
    vec = 4 if F % 4 == 0 and shift % 4 == 0 else (2 if F % 2 == 0 and shift % 2 == 0 else 1)
    _form(what, f'{4 * vec}-byte row copies')
    ws.no_leak(o, what)
    assert torch.equal(o.view(n_idx, F).cpu(), src[idx]), what
    ws.neighbours(what)


# ------------------------------------------------------------------------------------------------------------------------------
# 8. cwn_head_f32 / cwn_head_bwd_f32
# ------------------------------------------------------------------------------------------------------------------------------
def _cell_ptr(n_cells):
    """Four complexes over the cells, the second of them EMPTY."""
    return torch.tensor([0, n_cells // 3, n_cells // 3, (2 * n_cells) // 3, n_cells], dtype=torch.int64)


@pytest.mark.parametrize('parts', [1, 2])
@pytest.mark.parametrize('cls', ['W0', 'W1', 'S12', 'W2', 'W3'])
def test_head_windows(cls, parts):
    """cwn_head_f32 (csrc/cwn_ends.hip), the operand that carries a stride: x "[n_cells, K], row stride ldx (multiple of 4)",
    16-byte aligned -- as a window, and (n_parts = 2, jumping knowledge 'cat') as the two K / 2-column blocks x, x_more[0] of ONE
    wider matrix.  out and pooled_out against float64, bit-identical to contiguous copies.  W2 (CWN_ERR_ALIGN) and W3
    (CWN_ERR_BAD_ARG) are refused before the launch; ops.head serves the same window through a copy and the prepared
    ops.HeadLaunch declines it (None: its caller goes through ops.head).
    FOUND by this test: ONE row of a wider matrix is "contiguous" to torch wherever it starts and whatever its stride says, so
    ops.head's `.contiguous()` left a one-cell x at a 4-byte offset (or with an odd row stride) as it lay and the entry
    point's refusal surfaced as a CwnError; ops.HeadLaunch.run passed any misaligned window through to the same refusal.
    ops.head now copies such a block, HeadLaunch.run declines it."""
    K, H2, O = 16, 8, 3
    g = torch.Generator().manual_seed(K + parts)
    W1, b1, W2, b2 = _rand(g, H2, K) / K ** 0.5, _rand(g, H2), _rand(g, O, H2) / H2 ** 0.5, _rand(g, O)
    W1d, b1d, W2d, b2d = W1.to(DEV), b1.to(DEV), W2.to(DEV), b2.to(DEV)
    w1t = W1.t().contiguous().to(DEV)
    Mx = max(ROWS)
    X = _rand(g, Mx, K)

    def build(c, M):
        ws = Windows(DEV)
        x = ws.inp('x', X[:M], _cls(c))               # (the blocks of n_parts = 2: its two column halves, one row stride)
        ptr = _cell_ptr(M)
        Cn = ptr.numel() - 1
        ptr_d = ptr.to(DEV)
        out, pooled = ws.out('out', Cn, O, 'W0'), ws.out('pooled', Cn, K, 'W0')
        D = _ffi.HeadDim()
        D.x, D.cell_ptr, D.w1t, D.b1, D.pooled_out, D.n_cells, D.ldx, D.n_parts = x.data_ptr(), ptr_d.data_ptr(), w1t.data_ptr(), \
            b1d.data_ptr(), pooled.data_ptr(), M, x.stride(0), parts
        if parts == 2:
            D.x_more[0] = x[:, K // 2:].data_ptr()
        call = lambda: _ffi.lib().cwn_head_f32((_ffi.HeadDim * 1)(D), 1, Cn, K, H2, 0, 0, W2d.data_ptr(), b2d.data_ptr(), O,
                                               out.data_ptr(), None, None, 0, None, 0, 1, _stream())
        return ws, call, x, ptr, ptr_d, out, pooled, (D, ptr_d)

    for M in ROWS:
        what = f'head parts={parts} {cls} M={M}'
        ws, call, x, ptr, ptr_d, out, pooled, keep = build(cls, M)
        Cn = ptr.numel() - 1
        rp = torch.stack([X[ptr[c]:ptr[c + 1]].double().sum(0) for c in range(Cn)])
        ref = (rp @ W1.double().t() + b1.double()).relu() @ W2.double().t() + b2.double()
        rc = call()
        if cls in FORBIDDEN:
            torch.cuda.synchronize()
            assert rc == FORBIDDEN[cls], (what, rc)
            ws.unchanged(what)
            xs = [[x[:, :K // 2], x[:, K // 2:]]] if parts == 2 else [x]
            got = ops.head(xs, [ptr_d], Cn, [W1d], [b1d], W2d, b2d)
            ws.no_leak(got, what + ' (ops.head)')
            gate(got, ref, what + ' (ops.head)')
            assert ops.HeadLaunch(xs, [ptr_d], Cn, [W1d], [b1d], W2d, b2d, False, False).run(xs) is None, what
            ws.unchanged(what)
            _form(what, f'refused (code {rc}), nothing written; ops.head copies the operand, ops.HeadLaunch declines')
            continue
        _ffi.check(rc, 'cwn_head_f32')
        _form(what, 'head kernel, 16-byte row loads')
        ws.no_leak(out, what)
        gate(pooled, rp, what + ' pooled')
        gate(out, ref, what + ' out')
        ws.neighbours(what)
        _, callc, _, _, _, outc, pooledc, keepc = build('W0', M)
        _ffi.check(callc(), 'cwn_head_f32')
        assert torch.equal(out, outc) and torch.equal(pooled, pooledc), f'{what}: not the bits of the contiguous launch'


@pytest.mark.parametrize('parts', [1, 2])
@pytest.mark.parametrize('cls', ['W0', 'W1', 'S12', 'W2', 'W3'])
def test_head_backward_windows(cls, parts):
    """cwn_head_bwd_f32: dx "[n_cells, K], row stride lddx" (16-byte aligned, lddx % 4 == 0) as an output window, and with
    n_parts = 2 as the two blocks dx, dx_more[0] of one wider matrix: every row of a complex receives W1^T dh, the columns
    beside the window keep their sentinel.  W2 / W3: refused before the launch, nothing written."""
    K, H2, O = 16, 8, 3
    g = torch.Generator().manual_seed(3 * K + parts)
    W1, W2 = _rand(g, H2, K) / K ** 0.5, _rand(g, O, H2) / H2 ** 0.5
    W1d, W2d = W1.to(DEV), W2.to(DEV)

    def build(c, M):
        ws = Windows(DEV)
        ptr = _cell_ptr(M)
        Cn = ptr.numel() - 1
        gg =torch.Generator().manual_seed(M)
        h, go = _rand(gg, Cn, H2), _rand(gg, Cn, O)
        hd, god, ptr_d = h.to(DEV), go.to(DEV), ptr.to(DEV)
        dx = ws.out('dx', M, K, _cls(c))
        dh = ws.out('dh', Cn, H2, 'W0')
        D = _ffi.HeadBwdDim()
        D.h, D.w1, D.cell_ptr, D.dx, D.dh_out, D.n_cells, D.lddx, D.n_parts = hd.data_ptr(), W1d.data_ptr(), ptr_d.data_ptr(), \
            dx.data_ptr(), dh.data_ptr(), M, dx.stride(0), parts
        if parts == 2:
            D.dx_more[0] = dx[:, K // 2:].data_ptr()
        call = lambda: _ffi.lib().cwn_head_bwd_f32((_ffi.HeadBwdDim * 1)(D), 1, Cn, K, H2, 0, 0, W2d.data_ptr(), O, god.data_ptr(), None,
                                                   0, 1, _stream())
        return ws, call, ptr, h, go, dx, dh, (hd, god, ptr_d, D)

    for M in ROWS:
        what = f'head bwd parts={parts} {cls} M={M}'
        ws, call, ptr, h, go, dx, dh, keep = build(cls, M)
        rc = call()
        if cls in FORBIDDEN:
            torch.cuda.synchronize()
            assert rc == FORBIDDEN[cls], (what, rc)
            ws.unchanged(what)
            _form(what, f'refused (code {rc}), nothing written')
            continue
        _ffi.check(rc, 'cwn_head_bwd_f32')
        _form(what, 'head backward kernel, 16-byte row stores')
        rdh = (go.double() @ W2.double()) * (h.double() > 0)
        rdp = rdh @ W1.double()
        rdx = torch.zeros(M, K, dtype=torch.float64)
        for c in range(ptr.numel() - 1):
            rdx[ptr[c]:ptr[c + 1]] = rdp[c]
        ws.no_leak(dx, what)
        gate(dh, rdh, what + ' dh')
        gate(dx, rdx, what + ' dx')
        ws.neighbours(what)
        _, callc, _, _, _, dxc, dhc, keepc = build('W0', M)
        _ffi.check(callc(), 'cwn_head_bwd_f32')
        assert torch.equal(dx, dxc) and torch.equal(dh, dhc), f'{what}: not the bits of the contiguous launch'


# ------------------------------------------------------------------------------------------------------------------------------
# 9. cwn_target_head_f32 / cwn_target_head_bwd_f32
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,K', [(64, 5), (8, 3), (128, 32)])       # (W through L2; ... ; 16 KiB of W staged in LDS)
@pytest.mark.parametrize('cls', ALL)
def test_target_head_windows(cls, H, K):
    """cwn_target_head_f32 / cwn_target_head_bwd_f32 (csrc/cwn_target_head.hip): x and dx "16-byte aligned, ldx % 4 == 0", out
    [C, K] and dlogits [C, K] with ANY row stride (ldout, lddl) and 4-byte alignment.  In W0 / W1 all four are windows of the
    class; in W2 - W4 out and dlogits still are (the entry takes them) while x / dx in that class are refused with
    CWN_ERR_ALIGN before the launch -- then run with x / dx contiguous -- and ops.target_head serves the x window through its
    gather + linear form.  dx: EVERY row is written (zeros off the target rows), the columns beside the window keep their
    sentinel; dW / db are written, not accumulated."""
    g = torch.Generator().manual_seed(H + K)
    Wt, b = _rand(g, K, H) / H ** 0.5, _rand(g, K)
    Wd, bd = Wt.to(DEV), b.to(DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    for N in ROWS:
        what = f'target_head H={H} K={K} {cls} N={N}'
        Cn = min(N, 5)
        rows = torch.linspace(0, N - 1, Cn).long().to(torch.int32)
        rows_d = rows.to(DEV)
        X, dl = _rand(g, N, H), _rand(g, Cn, K)
        L = _ffi.lib()

        def fwd(cx, cy):
            ws = Windows(DEV)
            x, out = ws.inp('x', X, cx), ws.out('out', Cn, K, cy)
            rc = L.cwn_target_head_f32(x.data_ptr(), N, x.stride(0), rows_d.data_ptr(), Cn, Wd.data_ptr(), bd.data_ptr(), out.data_ptr(),
                                       out.stride(0), H, K, err.data_ptr(), None, _stream())
            return ws, rc, x, out

        def bwd(cx, cy):
            ws = Windows(DEV)
            x, d, dx = ws.inp('x', X, cx), ws.inp('dlogits', dl, cy), ws.out('dx', N, H, cx)
            dW, db = ws.out('dW', K, H, 'W0'), ws.vec('db', torch.full((K,), SENT), VEC_OFF[cy], out=True)
            rc = L.cwn_target_head_bwd_f32(d.data_ptr(), d.stride(0), x.data_ptr(), N, x.stride(0), rows_d.data_ptr(), Cn, Wd.data_ptr(),
                                           dx.data_ptr(), dx.stride(0), dW.data_ptr(), db.data_ptr(), H, K, None, 0, None, _stream())
            return ws, rc, dx, dW, db

        ref = X[rows.long()].double() @ Wt.double().t() + b.double()
        rdx = torch.zeros(N, H, dtype=torch.float64).index_add_(0, rows.long(), dl.double() @ Wt.double())
        cx = cls
        if cls not in VECTOR_OK:
            for name, (ws, rc, *_rest) in (('forward', fwd(cls, cls)), ('backward', bwd(cls, cls))):
                torch.cuda.synchronize()
                assert rc == ALIGN, (what, name, rc)
                ws.unchanged(f'{what} {name}')
            ws, _, x, _ = fwd(cls, cls)
            got = ops.target_head(x, rows_d, Wd, bd)
            ws.no_leak(got, what + ' (ops.target_head)')
            gate(got, ref, what + ' (ops.target_head)')
            ws.unchanged(what)
            _form(what, 'x / dx refused (CWN_ERR_ALIGN), nothing written; ops.target_head: gather + linear')
            cx = 'W0'
        ws, rc, x, out = fwd(cx, cls)
        _ffi.check(rc, 'cwn_target_head_f32')
        _form(what, f'target-head kernel, x {cx}, out / dlogits {cls}')
        ws.no_leak(out, what)
        gate(out, ref, what + ' out')
        ws.neighbours(what)
        ws2, rc, dx, dW, db = bwd(cx, cls)
        _ffi.check(rc, 'cwn_target_head_bwd_f32')
        for name, t, r in (('dx', dx, rdx), ('dW', dW, dl.double().t() @ X[rows.long()].double()), ('db', db, dl.double().sum(0))):
            ws2.no_leak(t, f'{what} {name}')
            gate(t, r, f'{what} {name}')
        ws2.neighbours(what + ' backward')
        _, rc, _, outc = fwd('W0', 'W0')
        _, rc2, dxc, dWc, dbc = bwd('W0', 'W0')
        assert rc == 0 and rc2 == 0
        assert torch.equal(out, outc) and torch.equal(dx, dxc) and torch.equal(dW, dWc) and torch.equal(db, dbc), \
            f'{what}: not the bits of the contiguous launch'
    assert int(err) == 0


# ------------------------------------------------------------------------------------------------------------------------------
# 10. cwn_oriented_dz_f32
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H', [64, 37])
@pytest.mark.parametrize('act', [_ffi.ACT_RELU, _ffi.ACT_ELU, _ffi.ACT_TANH, _ffi.ACT_SIGMOID])
@pytest.mark.parametrize('cls', ALL)
def test_oriented_dz_windows(cls, act, H):
    """cwn_oriented_dz_f32 (csrc/cwn_oriented.hip): dout, out and dz with their own row strides (lddout, ldout, lddz), 4-byte
    alignment: dz = dout * act'(out) element by element in every class, bit-identical to the contiguous call, in place (dz
    aliasing dout) as well."""
    g = torch.Generator().manual_seed(H + act)
    Mx = max(ROWS)
    z = _rand(g, Mx, H)
    O = {_ffi.ACT_RELU: z.relu(), _ffi.ACT_ELU: torch.nn.functional.elu(z), _ffi.ACT_TANH: z.tanh(), _ffi.ACT_SIGMOID: z.sigmoid()}[act]
    G = _rand(g, Mx, H)

    def run(c, M, alias):
        ws = Windows(DEV)
        out = ws.inp('out', O[:M], c)
        if alias:
            dout = dz = ws.out('dout', M, H, c, prefill=G[:M])
        else:
            dout, dz = ws.inp('dout', G[:M], c), ws.out('dz', M, H, c)
        _ffi.check(_ffi.lib().cwn_oriented_dz_f32(dout.data_ptr(), out.data_ptr(), dz.data_ptr(), M, H, dout.stride(0), out.stride(0),
                                                  dz.stride(0), act, None, _stream()), 'cwn_oriented_dz_f32')
        return ws, dz

    for M in ROWS:
        o = O[:M].double()
        d = {_ffi.ACT_RELU: (o > 0).double(), _ffi.ACT_ELU: torch.where(o > 0, torch.ones_like(o), o + 1), _ffi.ACT_TANH: 1 - o * o,
             _ffi.ACT_SIGMOID: o * (1 - o)}[act]
        base = None
        for alias in (False, True):
            what = f'oriented_dz H={H} act={act} {cls} alias={alias} M={M}'
            ws, dz = run(cls, M, alias)
            ws.no_leak(dz, what)
            gate(dz, G[:M].double() * d, what)
            ws.neighbours(what)
            _, dzc = run('W0', M, alias)
            assert torch.equal(dz, dzc), f'{what}: not the bits of the contiguous call'
            assert base is None or torch.equal(dz, base), what
            base = dz
    _form(f'oriented_dz H={H} act={act} {cls}', 'element-wise kernel')


# ------------------------------------------------------------------------------------------------------------------------------
# 11. the weight packers
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cls', ALL)
def test_weight_packers_take_a_window_of_a_wider_weight(cls):
    """cwn_gemm_pack_weights_f32, cwn_update_mlp_pack_weights_f32 / _many / _t_many / _both_many and cwn_layer_pack_weights_f32 /
    _many / _t_many / _both_many: "W [.., ..] (row stride ldw)", 4-byte aligned, "a column offset selects half of a combine
    weight" -- the packed bytes of a window of a wider NaN-padded weight equal the packed bytes of a contiguous copy, in every
    class, and the weight is left as it was."""
    L = _ffi.lib()
    g = torch.Generator().manual_seed(19)
    s = _stream()

    def many(fn, views, F, nbytes, both=False):
        n = len(views)
        outs = [torch.zeros(nbytes, dtype=torch.uint8, device=DEV) for _ in range(2 * n if both else n)]
        Wp = (C.c_void_p * n)(*[v.data_ptr() for v in views])
        ld = (C.c_int64 * n)(*[v.stride(0) for v in views])
        Op = (C.c_void_p * n)(*[o.data_ptr() for o in outs[:n]])
        if both:
            Tp = (C.c_void_p * n)(*[o.data_ptr() for o in outs[n:]])
            _ffi.check(fn(Wp, ld, F, Op, Tp, n, s), 'pack (both)')
        else:
            _ffi.check(fn(Wp, ld, F, Op, n, s), 'pack (many)')
        return outs

    def single(fn, view, nbytes, F=None):
        out = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
        args = (view.data_ptr(), view.stride(0)) + (() if F is None else (F,)) + (out.data_ptr(), s)
        _ffi.check(fn(*args), 'pack')
        return [out]

    def packs(c):
        ws = Windows(DEV)
        res = []
        W128 = ws.inp('W128', Ws['g'], c)
        res += single(L.cwn_gemm_pack_weights_f32, W128, int(L.cwn_gemm_packed_weight_bytes()))
        for F in (64, 128):
            Wc = ws.inp(f'Wc{F}', Ws[f'c{F}'], c)                       # [F, 2F]: its two column halves
            halves = [Wc[:, :F], Wc[:, F:]]
            nb = int(L.cwn_update_mlp_packed_weight_bytes(F))
            for h in halves:
                res += single(L.cwn_update_mlp_pack_weights_f32, h, nb, F)
            res += many(L.cwn_update_mlp_pack_weights_many_f32, halves, F, nb)
            res += many(L.cwn_update_mlp_pack_weights_t_many_f32, halves, F, nb)
            res += many(L.cwn_update_mlp_pack_weights_both_many_f32, halves, F, nb, both=True)
            nl = int(L.cwn_layer_packed_weight_bytes(F))
            res += single(L.cwn_layer_pack_weights_f32, Wc, nl, F)
            res += many(L.cwn_layer_pack_weights_many_f32, [Wc], F, nl)
            res += many(L.cwn_layer_pack_weights_t_many_f32, [Wc], F, nl)
            res += many(L.cwn_layer_pack_weights_both_many_f32, [Wc], F, nl, both=True)
        torch.cuda.synchronize()
        ws.unchanged(f'packers {c}')
        return res

    Ws = {'g': _rand(g, 128, 128), 'c64': _rand(g, 64, 128), 'c128': _rand(g, 128, 256)}
    got, want = packs(cls), packs('W0')
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), f'packers {cls}: pack {k} differs from the pack of the contiguous copy'
        assert bool(a.any()), k
    _form(f'packers {cls}', f'{len(got)} packs, byte-identical to the contiguous weight')


# ------------------------------------------------------------------------------------------------------------------------------
# 12. ONE-row windows through the ops wrappers: the two forms of the 16-byte rule
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['run_stage-W3', 'run_stage-W2', 'target_head_applies-W3', 'head-W3', 'head-W2', 'update_mlp-W3'])
def test_one_row_windows_through_the_wrappers(case):
    """M = 1, F = 64: the smallest shapes at which "16-byte readable" judged on the RECORDED row stride and judged on the stride
    a descriptor carries (one row: the width) differ -- W3 is [1, 67][:, :64], aligned with an odd recorded stride; W2 starts
    4 bytes off.  Each wrapper's decision is pinned as it stands:
      ops.run_stage             judges the recorded stride: declines both windows (None; it takes the contiguous row);
      ops.target_head_applies   judges the recorded stride: False on W3 (True on the contiguous row);
      ops.head                  judges the recorded stride: both blocks are copied -- the bits of the contiguous launch;
      ops.update_mlp            `_rowmajor16` judges the stride the descriptor carries: the W3 row is kept AS IT LIES (the W2
                                row is copied) -- the bits of the contiguous launch.
    Inputs keep their bits in every case."""
    op, cls = case.split('-')
    F = 64
    g = torch.Generator().manual_seed(len(case))
    X, X2 = _rand(g, 1, F), _rand(g, 1, F)
    ws = Windows(DEV)
    x = ws.inp('x', X, cls)
    assert x.size(0) == 1 and (x.stride(0) % 4 != 0 if cls == 'W3' else not aligned16(x)), case
    if op == 'run_stage':
        W, bias = _stage_weight(g, F, 1), _rand(g, F).to(DEV)
        taken = ops.run_stage([ops.Gemm(X=X.to(DEV), W=W.detach(), bias=bias)], DEV)
        assert taken is not None, f'{case}: the contiguous row was to run on the stage kernel'
        gm = ops.Gemm(X=x, W=W.detach(), bias=bias)
        assert ops.run_stage([gm], DEV) is None, case
        ref = X.double() @ W.detach().cpu().double().t() + bias.cpu().double()
        gate(taken[0], ref, case + ' (contiguous, stage kernel)')
        gate(ops.run_gemm([gm], DEV)[0], ref, case + ' (cwn_gemm_f32)')
        _form(case, 'ops.run_stage declines (None), cwn_gemm_f32 serves the window')
    elif op == 'target_head_applies':
        Wd, bd, rows = (_rand(g, 5, F) / F ** 0.5).to(DEV), _rand(g, 5).to(DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        assert ops.target_head_applies(X.to(DEV), rows, Wd, bd) is True, case
        assert ops.target_head_applies(x, rows, Wd, bd) is False, case
        _form(case, 'ops.target_head_applies: False')
    elif op == 'head':
        H2, O = 8, 3
        W1, b1, W2, b2 = _rand(g, H2, F) / F ** 0.5, _rand(g, H2), _rand(g, O, H2) / H2 ** 0.5, _rand(g, O)
        dev = [t.to(DEV) for t in (W1, b1, W2, b2)]
        ptr = _cell_ptr(1)
        ptr_d, Cn = ptr.to(DEV), ptr.numel() - 1
        run = lambda t: ops.head([t], [ptr_d], Cn, [dev[0]], [dev[1]], dev[2], dev[3])
        got, want = run(x), run(X.to(DEV))
        rp = torch.stack([X[ptr[c]:ptr[c + 1]].double().sum(0) for c in range(Cn)])
        ws.no_leak(got, case)
        gate(got, (rp @ W1.double().t() + b1.double()).relu() @ W2.double().t() + b2.double(), case)
        assert torch.equal(got, want), f'{case}: not the bits of the contiguous launch'
        _form(case, 'ops.head copies the block')
    else:
        lins, folds = _mlp_net(g, F, F, 2)
        xb = ws.inp('xb', X2, cls)
        assert ops._rowmajor16(x, 'x_up') is x and ops._rowmajor16(xb, 'x_b') is xb, f'{case}: the row was to be kept as it lies'
        run = lambda u, b: ops.update_mlp([ops.MlpDim(x_up=u, x_b=b, linears=lins, folds=_mlp_dev_folds(folds))])[0]
        got, want = run(x, xb), run(X.to(DEV), X2.to(DEV))
        ws.no_leak(got, case)
        gate(got, _mlp_ref([X, X2], lins, folds, 1), case)
        assert torch.equal(got, want), f'{case}: not the bits of the contiguous launch'
        _form(case, 'ops.update_mlp keeps the row as it lies')
    torch.cuda.synchronize()
    ws.neighbours(case)
