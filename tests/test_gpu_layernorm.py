"""cwn_layernorm_act_f32 / cwn_layernorm_bwd_f32 (csrc/cwn_layernorm.hip) and ops.layer_norm_act_many on the GPU.

The reference is torch.nn.functional.layer_norm + relu evaluated in float64 on the upcast fp32 inputs, with its float64
autograd gradients; the bound is tests/_product.gate (1e-5 * max(1, |ref|_inf)) for out, dz, dgamma and dbeta.  Inputs are
z ~ 3 N(0, 1) + 0.5 with random gamma / beta, so the ReLU mask is mixed."""
import pytest
import torch
import torch.nn.functional as F

from cwn_amd import _ffi, ops
from tests._product import gate

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
EPS = 1e-5
NS = (1, 3, 4, 64, 100, 128, 160, 256, 260, 1024)
MS = (1, 5, 64, 65, 257)


def _ld(t):
    return t.stride(0) if t.size(0) > 1 else t.size(1)


def _inputs(M, N, seed, affine=True, shift=0.5, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(M, N, generator=g) * scale + shift).to(DEV)
    dy = torch.randn(M, N, generator=g).to(DEV)
    gamma = (torch.randn(N, generator=g) * 0.5 + 1.0).to(DEV) if affine else None
    beta = torch.randn(N, generator=g).to(DEV) if affine else None
    return z, dy, gamma, beta


def _fwd_desc(z, gamma, beta, relu, out, mean=None, rstd=None):
    return _ffi.LnDesc(z=z.data_ptr(), gamma=_ffi.ptr(gamma), beta=_ffi.ptr(beta), out=out.data_ptr(), mean=_ffi.ptr(mean),
                       rstd=_ffi.ptr(rstd), M=z.size(0), ldz=_ld(z), ldout=_ld(out), N=z.size(1), relu=int(relu), eps=EPS)


def _bwd_desc(z, gamma, relu, out, mean, rstd, dy, dz, dgamma, dbeta, accumulate=0):
    return _ffi.LnDesc(z=z.data_ptr(), gamma=_ffi.ptr(gamma), out=out.data_ptr(), mean=mean.data_ptr(), rstd=rstd.data_ptr(),
                       dy=dy.data_ptr(), dz=dz.data_ptr(), dgamma=_ffi.ptr(dgamma), dbeta=_ffi.ptr(dbeta), M=z.size(0),
                       ldz=_ld(z), ldout=_ld(out), lddy=_ld(dy), lddz=_ld(dz), N=z.size(1), relu=int(relu), eps=EPS,
                       accumulate=accumulate)


def _run(z, dy, gamma, beta, relu):
    """Forward + backward of one matrix through the C ABI: (out, dz, dgamma, dbeta, mean, rstd)."""
    M, N = z.shape
    out, dz = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
    mean, rstd = torch.empty(max(M, 1), device=DEV), torch.empty(max(M, 1), device=DEV)
    dgamma, dbeta = torch.full((N,), 7.0, device=DEV), torch.full((N,), 7.0, device=DEV)     # (written, not added to)
    _ffi.layer_norm_act([_fwd_desc(z, gamma, beta, relu, out, mean, rstd)], DEV)
    _ffi.layer_norm_bwd([_bwd_desc(z, gamma, relu, out, mean, rstd, dy, dz, dgamma, dbeta)], DEV)
    return out, dz, dgamma, dbeta, mean, rstd


def _reference(z, dy, gamma, beta, relu):
    """float64: (out, dz, dgamma, dbeta); the sums w.r.t. an implicit gamma = 1 / beta = 0 without the affine."""
    N = z.size(1)
    z64 = z.double().requires_grad_(True)
    g64 = (gamma.double() if gamma is not None else torch.ones(N, dtype=torch.float64, device=z.device)).requires_grad_(True)
    b64 = (beta.double() if beta is not None else torch.zeros(N, dtype=torch.float64, device=z.device)).requires_grad_(True)
    y = F.layer_norm(z64, (N,), g64, b64, EPS)
    y = torch.relu(y) if relu else y
    y.backward(dy.double())
    return y.detach(), z64.grad, g64.grad, b64.grad


def _check(got, ref, what):
    for name, a, b in zip(('out', 'dz', 'dgamma', 'dbeta'), got, ref):
        assert torch.isfinite(a).all(), (what, name)
        gate(a, b, f'{what} {name}')


@pytest.mark.parametrize('N', NS)
def test_shapes_against_float64(N):
    """Scalar path (N % 4 != 0), one to four vectors per lane, a ragged last vector, one band and several bands."""
    for M in MS:
        for relu in (0, 1):
            z, dy, gamma, beta = _inputs(M, N, seed=1000 * N + 10 * M + relu)
            got = _run(z, dy, gamma, beta, relu)
            _check(got, _reference(z, dy, gamma, beta, relu), f'N={N} M={M} relu={relu}')
            # the statistics the backward reads
            mu = z.double().mean(1)
            gate(got[4][:M], mu, f'N={N} M={M} mean')
            gate(got[5][:M], 1.0 / torch.sqrt(z.double().var(1, unbiased=False) + EPS), f'N={N} M={M} rstd')


def test_without_affine_and_without_statistics():
    for N, M in ((160, 65), (3, 5)):
        for relu in (0, 1):
            z, dy, _, _ = _inputs(M, N, seed=7 + relu, affine=False)
            got = _run(z, dy, None, None, relu)
            _check(got, _reference(z, dy, None, None, relu), f'no affine N={N} relu={relu}')
            out = torch.empty(M, N, device=DEV)
            _ffi.layer_norm_act([_fwd_desc(z, None, None, relu, out)], DEV)                # inference: no mean / rstd
            assert torch.equal(out, got[0])
            # no column sums wanted: no workspace, the same dz
            dz = torch.empty(M, N, device=DEV)
            _ffi.layer_norm_bwd([_bwd_desc(z, None, relu, got[0], got[4], got[5], dy, dz, None, None)], DEV)
            assert torch.equal(dz, got[1])


def test_empty_matrix_is_no_launch(monkeypatch):
    calls = []
    real = _ffi.layer_norm_act
    monkeypatch.setattr(_ffi, 'layer_norm_act', lambda descs, dev: (calls.append(len(descs)), real(descs, dev)))
    norm = torch.nn.LayerNorm(8).to(DEV)
    z = torch.empty(0, 8, device=DEV, requires_grad=True)
    out, = ops.layer_norm_act_many([z], [norm])
    assert out.shape == (0, 8) and calls == []
    out.sum().backward()
    assert z.grad.shape == (0, 8) and torch.equal(norm.weight.grad, torch.zeros(8, device=DEV))
    with torch.no_grad():
        assert ops.layer_norm_act_many([z], [norm])[0].shape == (0, 8) and calls == []
    # ... next to matrices that have rows
    z2 = torch.randn(5, 8, device=DEV)
    with torch.no_grad():
        o0, o2 = ops.layer_norm_act_many([z.detach(), z2], [norm, norm])
    assert calls == [1] and o0.shape == (0, 8)
    gate(o2, torch.relu(F.layer_norm(z2.double(), (8,), norm.weight.double(), norm.bias.double(), EPS)), 'beside empty')


def test_constant_rows():
    """Variance 0: out = act(beta), finite everywhere; dz is the float64 reference's rstd * (g - mean_N(g)) -- exactly 0
    where g is constant along the row (no affine, dy constant per row)."""
    for N in (160, 100, 3):
        M = 5
        g = torch.Generator().manual_seed(N)
        vals = torch.tensor([0.0, 0.1, -3.7, 100.3, 1e4])
        z = vals[:, None].expand(M, N).contiguous().to(DEV)
        dy = torch.randn(M, N, generator=g).to(DEV)
        gamma, beta = (torch.randn(N, generator=g) + 1.0).to(DEV), torch.randn(N, generator=g).to(DEV)
        for relu in (0, 1):
            got = _run(z, dy, gamma, beta, relu)
            _check(got, _reference(z, dy, gamma, beta, relu), f'constant rows N={N} relu={relu}')
            gate(got[0], (torch.relu(beta) if relu else beta).expand(M, N), f'constant rows N={N} out = act(beta)')
        # (dy in few mantissa bits: g - mean_N(g) is exact, and rstd = 316 has nothing to magnify)
        dyc = torch.tensor([1.0, -2.0, 0.5, 3.0, 0.25])[:, None].expand(M, N).contiguous().to(DEV)
        got = _run(z, dyc, None, None, 0)
        assert torch.isfinite(got[1]).all()
        gate(got[1], torch.zeros(M, N), f'constant rows N={N} dz = 0')


@pytest.mark.parametrize('col0', (8, 1))
def test_strided_operands(col0):
    """z, out, dy and dz as column slices of wider matrices: [:, 8:8+N] keeps the 16-byte form, [:, 1:1+N] takes the
    element-wise one.  The bytes outside the slices stay as they were."""
    M, N, W = 65, 160, 176
    z, dy, gamma, beta = _inputs(M, N, seed=3)
    ref = _reference(z, dy, gamma, beta, 1)
    plain = _run(z, dy, gamma, beta, 1)
    # (NaN around the z and dy slices: a load that strays and is not discarded shows in a result; sentinels around out and dz)
    wide = [torch.full((M, W), float('nan') if k in (0, 2) else float(-7 - k), device=DEV) for k in range(4)]
    zs, outs, dys, dzs = [w[:, col0:col0 + N] for w in wide]
    zs.copy_(z)
    dys.copy_(dy)
    before = [w.clone() for w in wide]
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    dgamma, dbeta = torch.empty(N, device=DEV), torch.empty(N, device=DEV)
    _ffi.layer_norm_act([_fwd_desc(zs, gamma, beta, 1, outs, mean, rstd)], DEV)
    _ffi.layer_norm_bwd([_bwd_desc(zs, gamma, 1, outs, mean, rstd, dys, dzs, dgamma, dbeta)], DEV)
    _check((outs, dzs, dgamma, dbeta), ref, f'strided col0={col0}')
    if col0 % 4 == 0:           # the same form of the kernel as the contiguous call: the same bits
        assert torch.equal(outs, plain[0]) and torch.equal(dzs, plain[1]) and torch.equal(dgamma, plain[2])
    keep = torch.ones(M, W, dtype=torch.bool, device=DEV)
    keep[:, col0:col0 + N] = False
    i32 = lambda t: t.contiguous().view(torch.int32)
    for k, (w, b) in enumerate(zip(wide, before)):
        assert torch.equal(i32(w[keep]), i32(b[keep])), k
    assert torch.equal(i32(wide[0]), i32(before[0])) and torch.equal(i32(wide[2]), i32(before[2]))         # z and dy are read only
    assert not any(bool(torch.isnan(t).any()) for t in (outs, dzs, dgamma, dbeta, mean, rstd))
    # dz may alias dy
    dy2 = dy.clone()
    _ffi.layer_norm_bwd([_bwd_desc(z, gamma, 1, plain[0], plain[4], plain[5], dy2, dy2, None, None)], DEV)
    assert torch.equal(dy2, plain[1])


def test_grouped_launch_equals_single_launches():
    """18 descriptors of mixed (M, N, alignment) in one call -- two launches -- against the same matrices one by one."""
    shapes = [(65, 160), (5, 3), (257, 64), (1, 1024), (64, 100), (130, 260), (0, 64), (7, 4), (65, 128)] * 2
    mats = []
    for k, (M, N) in enumerate(shapes):
        z, dy, gamma, beta = _inputs(M, N, seed=50 + k, affine=k % 3 != 2)
        if k % 4 == 1 and N % 4 == 0:         # an unaligned view of an aligned shape
            wz, wdy = torch.zeros(M, N + 4, device=DEV), torch.zeros(M, N + 4, device=DEV)
            wz[:, 1:1 + N], wdy[:, 1:1 + N] = z, dy
            z, dy = wz[:, 1:1 + N], wdy[:, 1:1 + N]
        mats.append((z, dy, gamma, beta, k % 2))

    def buffers():
        return [dict(out=torch.zeros(M, N, device=DEV), dz=torch.zeros(M, N, device=DEV), mean=torch.zeros(max(M, 1), device=DEV),
                     rstd=torch.zeros(max(M, 1), device=DEV), dgamma=torch.zeros(N, device=DEV), dbeta=torch.zeros(N, device=DEV))
                for M, N in shapes]

    def descs(bufs, bwd):
        res = []
        for (z, dy, gamma, beta, relu), b in zip(mats, bufs):
            res.append(_bwd_desc(z, gamma, relu, b['out'], b['mean'], b['rstd'], dy, b['dz'], b['dgamma'], b['dbeta']) if bwd
                       else _fwd_desc(z, gamma, beta, relu, b['out'], b['mean'], b['rstd']))
        return res

    one, many = buffers(), buffers()
    for bwd in (False, True):
        fn = _ffi.layer_norm_bwd if bwd else _ffi.layer_norm_act
        fn(descs(many, bwd), DEV)
        for d in descs(one, bwd):
            fn([d], DEV)
    for k, (a, b) in enumerate(zip(one, many)):
        for name in a:
            assert torch.equal(a[name], b[name]), (k, shapes[k], name)
    z, dy, gamma, beta, relu = mats[0]
    _check((many[0]['out'], many[0]['dz'], many[0]['dgamma'], many[0]['dbeta']), _reference(z, dy, gamma, beta, relu), 'grouped 0')


def test_shifted_rows_against_torch_float32():
    """z ~ N(100, 1): the mean dominates the deviations.  torch's own float32 layer_norm on the same device is measured against
    the float64 reference; the kernel must stay within max(the gate's bound, 2 x torch's float32 error) -- two-pass statistics
    in fp32 round the way torch's do, twice is slack for a different summation order."""
    M, N = 65, 160
    z, dy, gamma, beta = _inputs(M, N, seed=11, shift=100.0, scale=1.0)
    ref = _reference(z, dy, gamma, beta, 1)
    z32 = z.clone().requires_grad_(True)
    g32, b32 = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y32 = torch.relu(F.layer_norm(z32, (N,), g32, b32, EPS))
    y32.backward(dy)
    got = _run(z, dy, gamma, beta, 1)
    for name, mine, theirs, r in zip(('out', 'dz', 'dgamma', 'dbeta'), got, (y32.detach(), z32.grad, g32.grad, b32.grad), ref):
        e_mine, e_torch = float((mine.double() - r).abs().max()), float((theirs.double() - r).abs().max())
        bound = max(1e-5 * max(1.0, float(r.abs().max())), 2.0 * e_torch)
        print(f'[gate] shifted rows {name}: max|delta| = {e_mine:.3e} (kernel)  {e_torch:.3e} (torch float32)  '
              f'|ref|_inf = {float(r.abs().max()):.3g}  bound = {bound:.3e}')
        assert e_mine <= bound, (name, e_mine, e_torch, bound)


def test_device_side_row_count():
    """A static batch: capacity 257, 130 rows exist.  The rows below the count and the column sums equal the 130-row call bit
    for bit, the rows beyond keep what they held, and a count of 0 writes zero sums and nothing else."""
    M, N, cnt = 257, 160, 130
    z, dy, gamma, beta = _inputs(M, N, seed=5)
    small = _run(z[:cnt].contiguous(), dy[:cnt].contiguous(), gamma, beta, 1)
    for count in (cnt, 0):
        n_dev = torch.tensor([count], dtype=torch.int64, device=DEV)
        out, dz = torch.full((M, N), -9.0, device=DEV), torch.full((M, N), -9.0, device=DEV)
        mean, rstd = torch.full((M,), -9.0, device=DEV), torch.full((M,), -9.0, device=DEV)
        dgamma, dbeta = torch.full((N,), -9.0, device=DEV), torch.full((N,), -9.0, device=DEV)
        with _ffi.dynamic_rows({M: n_dev.data_ptr()}):
            _ffi.layer_norm_act([_fwd_desc(z, gamma, beta, 1, out, mean, rstd)], DEV)
            _ffi.layer_norm_bwd([_bwd_desc(z, gamma, 1, out, mean, rstd, dy, dz, dgamma, dbeta)], DEV)
        if count:
            assert torch.equal(out[:cnt], small[0]) and torch.equal(dz[:cnt], small[1])
            assert torch.equal(mean[:cnt], small[4]) and torch.equal(rstd[:cnt], small[5])
            assert torch.equal(dgamma, small[2]) and torch.equal(dbeta, small[3])
        else:
            assert torch.equal(dgamma, torch.zeros(N, device=DEV)) and torch.equal(dbeta, torch.zeros(N, device=DEV))
        assert (out[count:] == -9.0).all() and (dz[count:] == -9.0).all()
        assert (mean[count:] == -9.0).all() and (rstd[count:] == -9.0).all()
        if count == 0:
            # accumulate: the targets stay as they are
            acc = torch.full((N,), 2.5, device=DEV)
            with _ffi.dynamic_rows({M: n_dev.data_ptr()}):
                _ffi.layer_norm_bwd([_bwd_desc(z, gamma, 1, out, mean, rstd, dy, dz, acc, acc.clone(), accumulate=1)], DEV)
            assert (acc == 2.5).all()


def test_backward_is_bit_reproducible():
    M, N = 257, 160
    z, dy, gamma, beta = _inputs(M, N, seed=9)
    a, b = _run(z, dy, gamma, beta, 1), _run(z, dy, gamma, beta, 1)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # accumulate = 1 onto equal starting buffers; and it ADDS the sums of the plain call
    g = torch.Generator().manual_seed(1)
    start = torch.randn(2, N, generator=g).to(DEV)
    res = []
    for _ in range(2):
        t = start.clone()
        dz = torch.empty(M, N, device=DEV)
        _ffi.layer_norm_bwd([_bwd_desc(z, gamma, 1, a[0], a[4], a[5], dy, dz, t[0], t[1], accumulate=1)], DEV)
        res.append((dz, t))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][0], a[1])
    assert torch.equal(res[0][1][0], start[0] + a[2]) and torch.equal(res[0][1][1], start[1] + a[3])


def _modules(shapes, affine=True):
    torch.manual_seed(0)
    norms = [torch.nn.LayerNorm(N, elementwise_affine=affine).to(DEV) for _, N in shapes]
    if affine:
        with torch.no_grad():
            for m in norms:
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_()
    return norms


@pytest.mark.parametrize('into_grad', (False, True))
def test_autograd_against_float64_modules(into_grad):
    shapes = [(65, 160), (5, 3), (130, 64)]
    norms = _modules(shapes)
    ins = [_inputs(M, N, seed=20 + k) for k, (M, N) in enumerate(shapes)]
    zs = [i[0].clone().requires_grad_(True) for i in ins]
    if into_grad:       # a caller that owns the gradient buffers (train.TrainStep): the sums are ADDED to them
        for m in norms:
            m.weight.grad, m.bias.grad = torch.full_like(m.weight, 0.25), torch.full_like(m.bias, -0.5)
    with ops.accumulate_into_grad(into_grad):
        outs = ops.layer_norm_act_many(zs, norms, relu=True)
        torch.autograd.backward(outs, [i[1] for i in ins])
    for k, (m, (z, dy, _, _)) in enumerate(zip(norms, ins)):
        ref = _reference(z, dy, m.weight.detach(), m.bias.detach(), 1)
        off = (0.25, -0.5) if into_grad else (0.0, 0.0)
        _check((outs[k], zs[k].grad, m.weight.grad - off[0], m.bias.grad - off[1]), ref, f'autograd {shapes[k]} into_grad={into_grad}')
    # inference: the same outputs, no graph
    with torch.no_grad():
        plain = ops.layer_norm_act_many([z.detach() for z in zs], norms, relu=True)
    assert all(torch.equal(a, b) and not a.requires_grad for a, b in zip(plain, outs))
    # relu=False, no affine, gradient w.r.t. z only
    na = _modules(shapes[:1], affine=False)
    z = ins[0][0].clone().requires_grad_(True)
    out, = ops.layer_norm_act_many([z], na, relu=False)
    out.backward(ins[0][1])
    ref = _reference(ins[0][0], ins[0][1], None, None, 0)
    gate(out, ref[0], 'autograd no affine out')
    gate(z.grad, ref[1], 'autograd no affine dz')


def test_fallbacks_and_refusals():
    N = 16
    norm64 = torch.nn.LayerNorm(N).to(DEV).double()
    z64 = torch.randn(9, N, dtype=torch.float64, device=DEV, requires_grad=True)
    out, = ops.layer_norm_act_many([z64], [norm64])
    assert out.dtype == torch.float64 and torch.equal(out, torch.relu(norm64(z64)))         # float64: torch, exactly
    out.sum().backward()
    assert z64.grad is not None and norm64.weight.grad is not None
    cpu = torch.nn.LayerNorm(N)
    zc = torch.randn(4, N)
    assert torch.equal(ops.layer_norm_act_many([zc], [cpu], relu=False)[0], cpu(zc))         # CPU tensors: torch
    wide = torch.nn.LayerNorm(1028).to(DEV)
    zw = torch.randn(3, 1028, device=DEV)
    assert torch.equal(ops.layer_norm_act_many([zw], [wide])[0], torch.relu(wide(zw)))       # beyond a wave's registers: torch
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(TypeError):
            ops.layer_norm_act_many([torch.randn(4, N, device=DEV, dtype=dt)], [torch.nn.LayerNorm(N).to(DEV).to(dt)])
    with pytest.raises(_ffi.CwnError):
        _ffi.layer_norm_act([_ffi.LnDesc(z=zw.data_ptr(), out=torch.empty_like(zw).data_ptr(), M=3, ldz=1028, ldout=1028, N=1028,
                                         eps=EPS)], DEV)
