"""cwn_linear_wide_f32 on the GPU (csrc/cwn_linear_wide.hip) and ops.linear_wide on top of it:
  1. parity against float64 on the CPU inside the project gate, both weight layouts, with and without bias / X2, padded row
     strides and an odd base offset; below GEMM_MAX_K the bits of cwn_gemm_f32's exact kernel;
  2. the device-side row count over NaN-poisoned padding rows and a NaN-prefilled Y;
  3. a row's bits do not depend on the batch it sits in;
  4. the gradients of ops.linear_wide against float64 autograd, eager and under _ffi.dynamic_rows with poisoned rows behind
     the count;
  5. integer-valued operands: the exact answer."""
import pytest
import torch

from cwn_amd import _ffi, ops
from tests._product import gate

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
NAN = float('nan')
SHAPES = [(160, 160, 160), (1, 0, 1), (129, 0, 5), (100, 157, 160), (256, 256, 256)]
ROWS = (1, 31, 33, 70)


def _rand(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def _view(t: torch.Tensor, pad: int, off: int) -> torch.Tensor:
    """A GPU copy of `t` as a view with `pad` extra floats per row that starts `off` floats into its buffer (off = 1: a base
    address off 16 bytes, which the contract allows -- 4 bytes is all a float pointer needs)."""
    rows, cols = t.shape
    buf = torch.full((rows * (cols + pad) + off,), NAN, dtype=torch.float32, device=DEV)
    v = buf[off:].view(rows, cols + pad)[:, :cols]
    v.copy_(t)
    return v


def _padding_untouched(v: torch.Tensor, what: str) -> None:
    """Every element of the buffer behind a `_view` that lies outside the view still holds its NaN: the floats in front of it,
    the `pad` floats behind every row."""
    buf = v._base
    keep = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    rows, cols = v.shape
    idx = v.storage_offset() + torch.arange(rows, device=buf.device)[:, None] * v.stride(0) + torch.arange(cols, device=buf.device)
    keep[idx.reshape(-1)] = False
    assert bool(torch.isnan(buf.reshape(-1)[keep]).all()), f'{what}: an element beside the output window was written'


def _launch(X, X2, W, bias, Y, w_trans=False, m_dev=None):
    d = ops._wide_desc(X, X2, W, bias, Y, w_trans)
    if m_dev is not None:
        d.m_dev = m_dev.data_ptr()
    code = _ffi.lib().cwn_linear_wide_f32((_ffi.LinearWideDesc * 1)(d), 1, _ffi.stream_ptr(DEV))
    assert code == 0, code
    return Y


def _operands(g, M, K, K2, N, bias=True, pad=0, off=0, w_trans=False):
    X, X2 = _rand(g, M, K), (_rand(g, M, K2) if K2 else None)
    W = _rand(g, N, K + K2) / max(1.0, float(K + K2) ** 0.5)
    b = _rand(g, N) if bias else None
    ref = torch.cat([X] + ([X2] if K2 else []), 1).double() @ W.double().t() + (b.double() if bias else 0.0)
    Wk = W.t().contiguous() if w_trans else W
    dev = dict(X=_view(X, pad, off), X2=None if X2 is None else _view(X2, pad + 3 if pad else 0, off),
               W=_view(Wk, pad, off), bias=None if b is None else b.to(DEV))
    Y = _view(torch.full((M, N), NAN), pad, off)
    return dev, Y, ref


@pytest.mark.parametrize('w_trans', [False, True], ids=['natural', 'transposed'])
@pytest.mark.parametrize('K,K2,N', SHAPES)
def test_parity_against_float64_in_both_weight_layouts(K, K2, N, w_trans):
    g = torch.Generator().manual_seed(1000 * K + 10 * K2 + N)
    for M in ROWS:
        for bias, pad, off in ((True, 0, 0), (False, 0, 0), (True, 5, 1), (True, 4, 0)):
            o, Y, ref = _operands(g, M, K, K2, N, bias=bias, pad=pad, off=off, w_trans=w_trans)
            _launch(o['X'], o['X2'], o['W'], o['bias'], Y, w_trans)
            gate(Y, ref, f'linear_wide {"W" if w_trans else "W^T"} M={M} K={K}+{K2} N={N} bias={bias} pad={pad} off={off}')
            _padding_untouched(Y, f'linear_wide M={M} K={K}+{K2} N={N} pad={pad} off={off}')
            if K2:       # ... and without X2: the first K columns alone
                W1 = o['W'][:K] if w_trans else o['W'][:, :K]
                Y1 = torch.full((M, N), NAN, device=DEV)
                _launch(o['X'], None, W1, o['bias'], Y1, w_trans)
                Wd = (o['W'][:K].t() if w_trans else o['W'][:, :K]).cpu().double()
                gate(Y1, o['X'].cpu().double() @ Wd.t() + (o['bias'].cpu().double() if bias else 0.0),
                     f'linear_wide without X2, M={M} K={K} N={N}')


@pytest.mark.parametrize('K,K2,N', [(129, 0, 5), (100, 156, 160), (128, 128, 128)])
def test_bits_of_the_exact_gemm_kernel_where_both_apply(K, K2, N):
    """At K + K2 <= 256 the accumulation order is cwn_gemm_f32's exact kernel's: equal bit for bit."""
    g = torch.Generator().manual_seed(7)
    o, Y, _ = _operands(g, 70, K, K2, N)
    _launch(o['X'], o['X2'], o['W'], o['bias'], Y)
    want = ops.run_gemm([ops.Gemm(X=o['X'], X2=o['X2'], W=o['W'], bias=o['bias'], exact=True)], DEV)[0]
    assert torch.equal(Y, want)


CAP = 70


@pytest.mark.parametrize('w_trans', [False, True], ids=['natural', 'transposed'])
@pytest.mark.parametrize('K,K2,N', [(160, 160, 160), (100, 157, 160), (129, 0, 5)])
def test_device_side_row_count(K, K2, N, w_trans):
    g = torch.Generator().manual_seed(3)
    o, Y, _ = _operands(g, CAP, K, K2, N, w_trans=w_trans)
    full = _launch(o['X'], o['X2'], o['W'], o['bias'], Y, w_trans).clone()
    assert torch.isfinite(full).all()
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    for live in (0, 1, 31, 32, 33, CAP):
        X, X2 = o['X'].clone(), None if o['X2'] is None else o['X2'].clone()
        X[live:] = NAN                                        # the padding rows: poison
        if X2 is not None:
            X2[live:] = NAN
        Yc = torch.full((CAP, N), NAN, device=DEV)
        count.fill_(live)
        _launch(X, X2, o['W'], o['bias'], Yc, w_trans, m_dev=count)
        assert torch.equal(Yc[:live], full[:live]), live      # bit for bit the uncounted launch
        assert torch.isnan(Yc[live:]).all(), live             # the prefill: never written
    count.fill_(CAP + 1000)                                    # a count beyond the capacity is clamped to it
    Yc = torch.full((CAP, N), NAN, device=DEV)
    _launch(o['X'], o['X2'], o['W'], o['bias'], Yc, w_trans, m_dev=count)
    assert torch.equal(Yc, full)


@pytest.mark.parametrize('w_trans', [False, True], ids=['natural', 'transposed'])
def test_a_rows_bits_do_not_depend_on_its_batch(w_trans):
    K, K2, N = 100, 157, 160
    g = torch.Generator().manual_seed(5)
    o, _, _ = _operands(g, 70, K, K2, N, w_trans=w_trans)
    row, row2 = _rand(g, 1, K).to(DEV), _rand(g, 1, K2).to(DEV)

    def run(X, X2):
        return _launch(X.contiguous(), X2.contiguous(), o['W'], o['bias'], torch.empty(X.size(0), N, device=DEV), w_trans)

    alone = run(row, row2)
    a = run(torch.cat([o['X'][:36], row, o['X'][36:]]), torch.cat([o['X2'][:36], row2, o['X2'][36:]]))     # row 36 of 71
    b = run(torch.cat([row, o['X'][:2]]), torch.cat([row2, o['X2'][:2]]))                                    # row 0 of 3
    assert torch.equal(alone[0], a[36]) and torch.equal(alone[0], b[0])


def _grads_f64(X, X2, W, b, live, dY):
    xs = [t.detach().cpu().double()[:live].requires_grad_(True) for t in ([X] + ([X2] if X2 is not None else []))]
    Wd, bd = W.detach().cpu().double().requires_grad_(True), b.detach().cpu().double().requires_grad_(True)
    (torch.cat(xs, 1) @ Wd.t() + bd).backward(dY.cpu().double()[:live])
    return xs[0].grad, (xs[1].grad if X2 is not None else None), Wd.grad, bd.grad


@pytest.mark.parametrize('K,K2,N', [(160, 160, 160), (129, 0, 5), (100, 157, 160), (99, 57, 33)])
def test_gradients_against_float64_autograd_eager_and_under_a_row_count(K, K2, N):
    g = torch.Generator().manual_seed(11)
    M = 70
    mk = lambda *s: _rand(g, *s).to(DEV).requires_grad_(True)
    X, X2, W, b = mk(M, K), (mk(M, K2) if K2 else None), (_rand(g, N, K + K2) / (K + K2) ** 0.5).to(DEV).requires_grad_(True), mk(N)
    dY = _rand(g, M, N).to(DEV)
    Y = ops.linear_wide(X, X2, W, b)
    Y.backward(dY)
    want = _grads_f64(X, X2, W, b, M, dY)
    for name, got, ref in zip(('dX', 'dX2', 'dW', 'db'), (X.grad, None if X2 is None else X2.grad, W.grad, b.grad), want):
        if ref is not None:
            gate(got, ref, f'linear_wide eager {name}, K={K}+{K2} N={N}')
    # under a count: rows behind it are poison in every operand and in the incoming gradient
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    for live in (33, 1):
        count.fill_(live)
        Xp, X2p, dYp = X.detach().clone(), None if X2 is None else X2.detach().clone(), dY.clone()
        Xp[live:], dYp[live:] = NAN, NAN
        if X2p is not None:
            X2p[live:] = NAN
            X2p.requires_grad_(True)
        Xp.requires_grad_(True)
        W.grad = b.grad = None
        with _ffi.dynamic_rows({M: count.data_ptr()}):
            Yp = ops.linear_wide(Xp, X2p, W, b)
            Yp.backward(dYp)
        torch.cuda.synchronize()
        want = _grads_f64(X, X2, W, b, live, dY)
        assert torch.equal(Yp[:live], Y[:live])
        gate(Xp.grad[:live], want[0], f'linear_wide counted dX, live={live}')
        if X2 is not None:
            gate(X2p.grad[:live], want[1], f'linear_wide counted dX2, live={live}')
        gate(W.grad, want[2], f'linear_wide counted dW (poisoned rows behind the count), live={live}')
        gate(b.grad, want[3], f'linear_wide counted db, live={live}')


def test_weight_gradients_go_into_grad_inside_accumulate_into_grad():
    g = torch.Generator().manual_seed(13)
    M, K, K2, N = 40, 160, 160, 160
    X, X2, dY = _rand(g, M, K).to(DEV), _rand(g, M, K2).to(DEV), _rand(g, M, N).to(DEV)
    lin = torch.nn.Linear(K + K2, N).to(DEV)
    lin.weight.grad, lin.bias.grad = torch.ones_like(lin.weight), torch.ones_like(lin.bias)
    with ops.accumulate_into_grad():
        ops.linear_wide(X, X2, lin.weight, lin.bias).backward(dY)
    torch.cuda.synchronize()
    _, _, dW, db = _grads_f64(X, X2, lin.weight, lin.bias, M, dY)
    gate(lin.weight.grad, dW + 1.0, 'linear_wide: dW added into .grad')
    gate(lin.bias.grad, db + 1.0, 'linear_wide: db added into .grad')


@pytest.mark.parametrize('w_trans', [False, True], ids=['natural', 'transposed'])
@pytest.mark.parametrize('K,K2,N', [(160, 160, 160), (100, 157, 160), (256, 256, 256)])
def test_integer_operands_give_the_exact_answer(K, K2, N, w_trans):
    g = torch.Generator().manual_seed(17)
    ri = lambda *s: torch.randint(-4, 5, s, generator=g).float()
    M = 33
    X, X2, W, b = ri(M, K), ri(M, K2), ri(N, K + K2), ri(N)
    want = (torch.cat([X, X2], 1).double() @ W.double().t() + b.double()).float()       # |.| <= 512 * 16 + 4: exact in fp32
    Wk = W.t().contiguous() if w_trans else W
    Y = _launch(X.to(DEV), X2.to(DEV), Wk.to(DEV), b.to(DEV), torch.empty(M, N, device=DEV), w_trans)
    assert torch.equal(Y.cpu(), want)
