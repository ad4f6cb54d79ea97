"""FlatAdam as a torch optimizer, checked without a GPU (no kernel launch: the flat buffers, the param group, the learning-rate
schedulers of exp/run_exp.py:343-408 and checkpoints in torch.optim.Adam's format), and the ABI of cwn_adam_dev_f32."""
import ctypes
import os
import subprocess
import warnings

import pytest
import torch

from cwn_amd import _ffi
from cwn_amd.dist import FlatGradBucket
from cwn_amd.train import FlatAdam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(seed=0, frozen=False):
    torch.manual_seed(seed)
    m = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.ReLU(), torch.nn.Linear(7, 3), torch.nn.BatchNorm1d(3),
                            torch.nn.Linear(3, 2))
    if frozen:
        m[2].bias.requires_grad_(False)
    return m


def _staged_bucket(model):
    """A bucket laid out by stage (the later layers first), as TrainStep builds it under data parallelism: not the order of
    model.parameters()."""
    ps = [p for p in model.parameters() if p.requires_grad]
    stage_of = {id(p): (0 if k < 2 else 1 if k < 4 else 2) for k, p in enumerate(ps)}
    bucket = FlatGradBucket(model.parameters(), stage_of, 3)
    assert [p.shape for p in bucket.params] != [p.shape for p in ps]
    return bucket


def _torch_adam_after(model, steps=3, **kw):
    opt = torch.optim.Adam(model.parameters(), **kw)
    g = torch.Generator().manual_seed(7)
    for _ in range(steps):
        for p in model.parameters():
            if p.requires_grad:
                p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return opt


def test_flat_adam_is_a_torch_optimizer_with_one_adam_group():
    m = _model()
    opt = FlatAdam(FlatGradBucket(m.parameters()), lr=3e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.01)
    assert isinstance(opt, torch.optim.Optimizer)
    ref = torch.optim.Adam(_model().parameters(), lr=3e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.01)
    assert len(opt.param_groups) == 1
    assert set(opt.param_groups[0]) == set(ref.param_groups[0])
    for k, v in ref.param_groups[0].items():
        if k != 'params':
            assert opt.param_groups[0][k] == v, k
    assert [tuple(p.shape) for p in opt.param_groups[0]['params']] == [tuple(p.shape) for p in m.parameters()]
    # the attributes of the first form are the group's values
    opt.lr = 1e-4
    assert opt.param_groups[0]['lr'] == 1e-4 and opt.lr == 1e-4 and opt.betas == (0.8, 0.99)
    # what existing callers read
    assert opt.flat_p.numel() == opt.exp_avg.numel() == opt.exp_avg_sq.numel() == opt.bucket.flat.numel()
    assert opt.state_tensors() == [opt.exp_avg, opt.exp_avg_sq, opt.t] and opt.active is None and opt.counted is False


def test_unsupported_adam_forms_are_refused():
    with pytest.raises(NotImplementedError):
        FlatAdam(FlatGradBucket(_model().parameters()), amsgrad=True)
    with pytest.raises(NotImplementedError):
        FlatAdam(FlatGradBucket(_model().parameters()), maximize=True)
    opt = FlatAdam(FlatGradBucket(_model().parameters()))
    with pytest.raises(NotImplementedError):
        opt.add_param_group({'params': [torch.nn.Parameter(torch.zeros(2))]})
    opt.param_groups[0]['amsgrad'] = True
    with pytest.raises(NotImplementedError):
        opt.sync()


def test_schedulers_drive_the_group_and_the_device_record():
    m = _model()
    opt = FlatAdam(FlatGradBucket(m.parameters()), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
    assert opt.sync() and not opt.sync()               # written once, then only on a change
    assert opt.hyper.dtype == torch.float32 and opt.hyper.numel() == 8
    assert torch.equal(opt.hyper[:5], torch.tensor([1e-3, 0.9, 0.999, 1e-8, 0.0], dtype=torch.float32))
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    lrs = []
    with warnings.catch_warnings():
        warnings.simplefilter('error')                  # neither "lr_scheduler.step() before optimizer.step()" nor "overridden"
        for _ in range(3):
            opt._opt_called = True                      # (what a replayed training step records: TrainStep._before_replay)
            sched.step()
            lrs.append(opt.param_groups[0]['lr'])
            assert opt.sync()
            assert float(opt.hyper[0]) == torch.tensor(lrs[-1], dtype=torch.float32).item()
    assert lrs == [5e-4, 2.5e-4, 1.25e-4]
    # ReduceLROnPlateau on a plateau, and the reference's early stop (exp/run_exp.py: lr < --lr_scheduler_min)
    opt2 = FlatAdam(FlatGradBucket(_model(1).parameters()), lr=1e-4)
    plateau = torch.optim.lr_scheduler.ReduceLROnPlateau(opt2, mode='min', factor=0.5, patience=1)
    epochs = 0
    while opt2.param_groups[0]['lr'] >= 1e-5:
        plateau.step(1.0)
        epochs += 1
        assert epochs < 50
    assert opt2.param_groups[0]['lr'] == pytest.approx(6.25e-6) and epochs == 9
    # lr as a 0-d tensor
    opt2.param_groups[0]['lr'] = torch.tensor(2e-3)
    assert opt2.sync() and float(opt2.hyper[0]) == torch.tensor(2e-3).item()


@pytest.mark.parametrize('staged,frozen', [(False, False), (True, False), (True, True)])
def test_state_dict_has_torch_adams_layout(staged, frozen):
    m, mt = _model(2, frozen), _model(2, frozen)
    bucket = _staged_bucket(m) if staged else FlatGradBucket(m.parameters())
    opt = FlatAdam(bucket, lr=2e-3)
    empty = opt.state_dict()
    assert empty['state'] == {} and empty['param_groups'][0]['params'] == list(range(len(list(m.parameters()))))
    ref = _torch_adam_after(mt, 3, lr=2e-3)
    want = ref.state_dict()
    opt.load_state_dict(want)
    got = opt.state_dict()
    assert set(got) == set(want)
    assert got['param_groups'] == want['param_groups']
    assert sorted(got['state']) == sorted(want['state'])
    for i, st in want['state'].items():
        assert list(got['state'][i]) == list(st)
        for k, v in st.items():
            assert got['state'][i][k].shape == v.shape and got['state'][i][k].dtype == v.dtype, (i, k)
            assert torch.equal(got['state'][i][k], v), (i, k)


def test_a_torch_adam_state_dict_lands_in_the_flat_buffers_value_for_value():
    m, mt = _model(3), _model(3)
    bucket = _staged_bucket(m)
    opt = FlatAdam(bucket, lr=1e-3)
    ref = _torch_adam_after(mt, 3, lr=5e-4, betas=(0.85, 0.995), weight_decay=0.02)
    opt.load_state_dict(ref.state_dict())
    assert int(opt.t) == 3
    for p, q in zip(m.parameters(), mt.parameters()):
        off = opt._offset[id(p)]
        n = p.numel()
        st = ref.state[q]
        assert torch.equal(opt.exp_avg[off:off + n], st['exp_avg'].reshape(-1))
        assert torch.equal(opt.exp_avg_sq[off:off + n], st['exp_avg_sq'].reshape(-1))
    # the padding between parameters stays zero
    covered = torch.zeros(opt.exp_avg.numel(), dtype=torch.bool)
    for p, off in zip(bucket.params, bucket.offsets):
        covered[off:off + p.numel()] = True
    assert not opt.exp_avg[~covered].any() and not opt.exp_avg_sq[~covered].any()
    g = opt.param_groups[0]
    assert (g['lr'], g['betas'], g['weight_decay']) == (5e-4, (0.85, 0.995), 0.02)
    assert opt.sync() and float(opt.hyper[0]) == torch.tensor(5e-4).item()
    # ... and back: a torch Adam over the same parameters takes the flat optimizer's state
    back = torch.optim.Adam(_model(3).parameters())
    back.load_state_dict(opt.state_dict())
    for q, r in zip(mt.parameters(), back.param_groups[0]['params']):
        for k in ('exp_avg', 'exp_avg_sq'):
            assert torch.equal(back.state[r][k], ref.state[q][k])
        assert float(back.state[r]['step']) == 3.0
    # loading in place keeps the buffers the captured graphs read
    ptrs = [t.data_ptr() for t in opt.state_tensors()] + [opt.flat_p.data_ptr(), opt.hyper.data_ptr()]
    opt.load_state_dict(ref.state_dict())
    assert ptrs == [t.data_ptr() for t in opt.state_tensors()] + [opt.flat_p.data_ptr(), opt.hyper.data_ptr()]


def test_a_step_mismatch_and_a_foreign_layout_are_refused():
    m, mt = _model(4), _model(4)
    opt = FlatAdam(FlatGradBucket(m.parameters()))
    sd = _torch_adam_after(mt, 2).state_dict()
    sd['state'][1]['step'] = torch.tensor(5.0)
    with pytest.raises(ValueError, match='different steps'):
        opt.load_state_dict(sd)
    sd = _torch_adam_after(_model(4), 2).state_dict()
    sd['state'][0]['exp_avg'] = torch.zeros(3, 3)
    with pytest.raises(ValueError, match='exp_avg'):
        opt.load_state_dict(sd)
    sd = _torch_adam_after(_model(4), 2).state_dict()
    sd['param_groups'][0]['params'] = sd['param_groups'][0]['params'][:-1]
    with pytest.raises(ValueError, match='parameters'):
        opt.load_state_dict(sd)
    sd = _torch_adam_after(_model(4), 2, amsgrad=True).state_dict()
    with pytest.raises(NotImplementedError):
        opt.load_state_dict(sd)
    assert int(opt.t) == 0 and not opt.exp_avg.any()


def test_adam_hyper_record_abi():
    header = open(os.path.join(ROOT, 'include', 'cwn_hip.h')).read()
    assert 'cwn_adam_dev_f32' in _ffi.EXPORTS and 'cwn_adam_dev_f32(' in header
    assert hasattr(_ffi.lib(), 'cwn_adam_dev_f32') and _ffi.lib().cwn_abi_version() == 24
    assert ctypes.sizeof(_ffi.AdamHyper) == 32
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cwn_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(cwn_adam_hyper));']
    for fname, _ in _ffi.AdamHyper._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(cwn_adam_hyper, {fname}));')
    lines.append('return 0; }')
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, 'probe.c'), os.path.join(d, 'probe')
        open(src, 'w').write('\n'.join(lines))
        subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), src, '-o', exe], check=True)
        got = dict(l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got['size']) == 32
    for fname, _ in _ffi.AdamHyper._fields_:
        assert int(got[fname]) == getattr(_ffi.AdamHyper, fname).offset, fname
    # argument errors are caught on the host, before any launch
    lib = _ffi.lib()
    buf = (ctypes.c_float * 16)()
    a = ctypes.addressof(buf)
    assert lib.cwn_adam_dev_f32(a, a, a, a, -1, a, a, None, None) != 0
    assert lib.cwn_adam_dev_f32(a, a, a, a, 0, None, None, None, None) == 0          # nothing to do
    assert lib.cwn_adam_dev_f32(a, a, a, a, 4, None, a, None, None) != 0              # no record
    assert lib.cwn_adam_dev_f32(a, a, a, a, 4, a + 4, a, None, None) != 0             # misaligned record
