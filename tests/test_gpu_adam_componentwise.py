"""Adam entry by entry: single launches of cwn_adam_f32 and cwn_adam_dev_f32 (adam_body, csrc/cwn_norm.hip) on graded operands
against the float64 reference of tests/_adam.py that carries its own error bound.

  (R) on m' and v' (multiplies, adds and fmas only): |got - v| <= RIGOROUS * 2^-24 * c, never tuned;
  (E) on p' (powf, a division and a root on the way): the ratio against MARGIN * max(1, ratio of the numpy float32 restatement);
  the words behind n keep their bits (a float4 store over a tail would not); a device `active` of 0 changes nothing and 1 is
  None bit for bit; the pad elements of FlatAdam's buffers stay zero under weight decay.

The step counter is written into the device int32, so t = 1e5 costs what t = 1 does.  tests/test_bounds_host.py runs the same
gates over numpy on the CPU, where they refuse five wrong Adams."""
import pytest
import torch

from tests import _adam as A

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
ENTRIES = ('cwn_adam_f32', 'cwn_adam_dev_f32')
SENT = 0x7FC12345                                                                # a NaN's bits: a rewritten word would not keep them
BEHIND = 8                                                                       # words behind n


def _padded(x, n):
    """x [n] on the device in a buffer of n + BEHIND words, the words behind holding SENT."""
    buf = torch.full((n + BEHIND,), SENT, dtype=torch.int32, device=DEV)
    buf[:n] = x.to(DEV).view(torch.int32)
    return buf


def _launch(entry, ops, t, hyper, active=None, lr=A.LR, eps=A.EPS):
    """One launch on fresh copies of ops = (p, g, m, v); returns the four int32 buffers (n + BEHIND words) after it."""
    from cwn_amd import _ffi
    n = ops[0].numel()
    p, g, m, v = (_padded(x, n) for x in ops)
    assert all(b.data_ptr() % 16 == 0 for b in (p, g, m, v))
    step = torch.tensor([t], dtype=torch.int32, device=DEV)
    act = None if active is None else torch.tensor([active], dtype=torch.int64, device=DEV)
    b1, b2, wd = hyper
    L = _ffi.lib()
    if entry == 'cwn_adam_f32':
        code = L.cwn_adam_f32(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, b1, b2, eps, wd, step.data_ptr(),
                              _ffi.ptr(act), _ffi.stream_ptr(DEV))
    else:
        rec = torch.tensor([lr, b1, b2, eps, wd, 0, 0, 0], dtype=torch.float32).to(DEV)
        code = L.cwn_adam_dev_f32(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, rec.data_ptr(), step.data_ptr(),
                                  _ffi.ptr(act), _ffi.stream_ptr(DEV))
    _ffi.check(code, entry)
    torch.cuda.synchronize()
    assert int(step.item()) == t, f'{entry}: the launch moved the step counter'
    return [b.cpu() for b in (p, g, m, v)]


def _floats(buf, n):
    return buf[:n].view(torch.float32)


def _behind_untouched(bufs, ops, n, what):
    for name, b, x in zip('pgmv', bufs, ops):
        assert bool((b[n:] == SENT).all()), f'{what}: a word of {name} behind n = {n} was written'
    assert torch.equal(bufs[1][:n], ops[1].view(torch.int32)), f'{what}: the gradient was written'


@pytest.mark.parametrize('t', A.STEPS)
@pytest.mark.parametrize('hyper', A.HYPERS, ids=A.HYPER_IDS)
def test_one_launch_entry_by_entry(hyper, t):
    worst, differ, total = [0.0, 0.0, 0.0, 0.0, 0.0], 0, 0
    for n in A.SIZES:
        ops = A.operands(n, hyper)
        ref, cpu32 = A.reference(*ops, t, hyper), A.restatement(*ops, t, hyper)
        outs = {}
        for entry in ENTRIES:
            what = f'{entry} {hyper} t={t} n={n}'
            bufs = _launch(entry, ops, t, hyper)
            _behind_untouched(bufs, ops, n, what)
            got = (_floats(bufs[2], n), _floats(bufs[3], n), _floats(bufs[0], n))
            fig = A.check(got, ref, cpu32, what)
            worst = [max(a, b) for a, b in zip(worst, fig)]
            differ, total = differ + sum(int((a != b).sum()) for a, b in zip(got, cpu32)), total + 3 * n
            outs[entry] = bufs
        for a, b in zip(outs[ENTRIES[0]], outs[ENTRIES[1]]):
            assert torch.equal(a, b), f'{hyper} t={t} n={n}: the two entry points differ in a bit'
    print(f"[cw] Adam {hyper} t={t}, all sizes, both entry points: m' (R) {worst[0]:.3g}, v' (R) {worst[1]:.3g}; "
          f"p' (E) {worst[2]:.3g} / {worst[4]:.3g} / {worst[3]:.3g}; {differ} of {total} results differ from the restatement in a bit")


@pytest.mark.parametrize('n', [3, 4, 1025])
@pytest.mark.parametrize('entry', ENTRIES)
def test_active_zero_changes_nothing_and_one_is_none(entry, n):
    hyper, t = A.HYPERS[1], 3
    ops = A.operands(n, hyper)
    off = _launch(entry, ops, t, hyper, active=0)
    for name, b, x in zip('pgmv', off, ops):
        assert torch.equal(b[:n], x.view(torch.int32)) and bool((b[n:] == SENT).all()), f'{entry} n={n}: active = 0 wrote {name}'
    on, none = _launch(entry, ops, t, hyper, active=1), _launch(entry, ops, t, hyper, active=None)
    for name, a, b in zip('pgmv', on, none):
        assert torch.equal(a, b), f'{entry} n={n}: active = 1 and no active differ in {name}'
    assert not torch.equal(on[0][:n], ops[0].view(torch.int32)), f'{entry} n={n}: active = 1 changed nothing'


def test_flat_adam_pads_stay_zero_under_weight_decay():
    """FlatGradBucket pads a (1,) and a (7, 3) parameter to 4 and 24 elements: the 3 + 3 pad elements of the parameter buffer and
    of both moments are exactly zero after three steps with wd > 0 (0 + wd 0 = 0, and 0 / (0 + eps) = 0), and the parameters move."""
    from cwn_amd.dist import FlatGradBucket
    from cwn_amd.train import FlatAdam
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(1, device=DEV)), torch.nn.Parameter(torch.randn(7, 3, device=DEV))]
    before = [p.detach().clone() for p in ps]
    bucket = FlatGradBucket(ps)
    opt = FlatAdam(bucket, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    assert bucket.offsets == [0, 4] and opt.flat_p.numel() == 28
    pad = torch.tensor([1, 2, 3, 25, 26, 27], device=DEV)
    g = torch.Generator().manual_seed(1)
    for it in range(3):
        for p in ps:
            p.grad.copy_(torch.randn(*p.shape, generator=g).to(DEV))
        opt.step()
    torch.cuda.synchronize()
    assert int(opt.t.item()) == 3
    for name, buf in (('flat_p', opt.flat_p), ('exp_avg', opt.exp_avg), ('exp_avg_sq', opt.exp_avg_sq)):
        assert bool((buf[pad].view(torch.int32) == 0).all()), f'{name}: a pad element is not +0 after three steps'
    assert bool((bucket.flat[pad] == 0).all())
    for p, b in zip(ps, before):
        assert bool((p.detach() != b).all())
