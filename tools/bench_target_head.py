"""Time the target-cell head (csrc/cwn_target_head.hip, ops.target_head) against the form it replaces -- gather_rows on the
same rows + linear: what a checkout without the kernel would run, and what CWN_FUSED_TARGET_HEAD=0 keeps -- and RingSparseCIN's
forward and training step with either head, at ring 10 and ring 30, batch 32 and batch 1024.

Scopes (each captured into a HIP graph, so that what is timed is the device's work and not the interpreter's):
  head fwd          ops.target_head without autograd on x [batch * ring, 64], 5 classes; 20 calls per graph
  head fwd+bwd      the same with autograd and backward of the logits (x, weight and bias need gradients); 20 calls per graph
  model fwd         StaticForward.replay over a packed ring dataset (mode 'csr', items=True): fill + 3-layer RingSparseCIN, hidden 64
  model step        StaticTrainStep.step over it: fill, forward, cross-entropy, backward, Adam
The form (ops.FUSED_TARGET_HEAD) is held around every timed replay and the tool asserts that no graph was re-captured while
it was timed: a StaticForward re-captures when another model is built or a training step runs elsewhere in the process.
A region is as many replays as fill >= 50 ms between two device events; the two forms alternate region by region; the figure is
the median of five regions per form, in microseconds per call, with the spread (min .. max).  `launches` counts the kernels of
one eager call (torch.profiler; '-' where the profiler is not available).

    python tools/bench_target_head.py [--out profiles/ring_transfer.md] [--regions 5] [--min-ms 50]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd import models, ops, synthetic                                # noqa: E402
from cwn_amd.packed import PackedComplexes                                # noqa: E402
from cwn_amd.static_batch import StaticBatch                              # noqa: E402
from cwn_amd.static_graph import StaticForward, StaticTrainStep           # noqa: E402

DEV = torch.device('cuda', 0)
CALLS = 20


def region_us(replay, calls, min_ms):
    """Microseconds per call over one region of >= min_ms."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 1
    while True:
        a.record()
        for _ in range(n):
            replay()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= min_ms:
            return ms * 1e3 / (n * calls)
        n = max(n + 1, int(n * min_ms / max(ms, 1e-3) * 1.2))


def ab(replays, calls, regions, min_ms):
    """replays: {form: replay}; alternating regions -> {form: (median, min, max)}."""
    got = {k: [] for k in replays}
    for k, r in replays.items():
        region_us(r, calls, min_ms / 5)                                    # warm-up
    for _ in range(regions):
        for k, r in replays.items():
            got[k].append(region_us(r, calls, min_ms))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in got.items()}


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA'))
        return str(n) if n else '-'
    except Exception:
        return '-'


def captured(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            fn()
    return g.replay


def with_form(fused, fn):
    def call(*a):
        prev = ops.FUSED_TARGET_HEAD
        ops.FUSED_TARGET_HEAD = fused
        try:
            return fn(*a)
        finally:
            ops.FUSED_TARGET_HEAD = prev
    return call


def head_scopes(ring, batch):
    torch.manual_seed(0)
    N, H, K = ring * batch, 64, 5
    x = torch.randn(N, H, device=DEV, requires_grad=True)
    lin = torch.nn.Linear(H, K).to(DEV)
    rows = (torch.arange(batch, device=DEV) * ring).to(torch.int32)
    gout = torch.randn(batch, K, device=DEV)

    def fwd():
        with torch.no_grad():
            ops.target_head(x, rows, lin.weight, lin.bias)

    def fwd_bwd():
        x.grad = lin.weight.grad = lin.bias.grad = None
        ops.target_head(x, rows, lin.weight, lin.bias).backward(gout)
    return {'head fwd': fwd, 'head fwd+bwd': fwd_bwd}


def model_scopes(ring, batch, fused):
    """-> {'model fwd': replay, 'model step': replay} with the head in the given form.  A StaticForward re-captures when the
    model-state epochs move (building another model, a training step elsewhere), so the form is HELD around every replay, and
    `check` asserts after the timing that the graph timed is the one captured under that form."""
    pool = synthetic.ring_transfer(ring, batch * 2 if batch * 2 % 5 == 0 else batch * 2 // 5 * 5 + 5, 5)
    packed = PackedComplexes(pool, DEV, max_dim=2, with_csr=True)
    idx = np.arange(batch)
    torch.manual_seed(1)
    out = {}
    m = models.RingSparseCIN(5, 5, 3, 64, use_coboundaries=True).to(DEV).eval()
    m2 = models.RingSparseCIN(5, 5, 3, 64, use_coboundaries=True).to(DEV).train()
    sf = StaticForward(m, StaticBatch(packed, batch, mode='csr', items=True))

    def fwd_replay():
        sf.sb.rewind(0)                      # (the cursor back to this batch: one fill launch, both forms)
        with torch.no_grad():
            sf.replay()
    out['model fwd'] = with_form(fused, fwd_replay)
    sb = StaticBatch(packed, batch, mode='csr', items=True)
    sb.set_batch(idx)
    st = StaticTrainStep(m2, sb, task_type='classification', lr=1e-3)
    with_form(fused, st.step_on)([idx])
    out['model step'] = with_form(fused, lambda: (sb.rewind(0), st.step()))
    with torch.no_grad():
        with_form(fused, sf.run)(idx)
    armed = {}

    def arm():                               # after EVERY model of the process is built: the re-capture the epochs ask for
        out['model fwd']()                   # happens here, under the form
        armed['graph'] = sf.graph

    def check():
        assert sf.graph is armed['graph'], 'the forward graph was re-captured during its timing'
        assert len(st._graphs) == 1, 'the training step was re-captured during the timing'
    out['arm'] = arm
    out['check'] = check
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--min-ms', type=float, default=50.0)
    ap.add_argument('--out', default=None)
    ap.add_argument('--shapes', default='10x32,10x1024,30x32,30x1024')
    args = ap.parse_args()
    lines = [f'median of {args.regions} regions of >= {args.min_ms:g} ms per form, forms alternating; us per call [min .. max]; '
             f'{torch.cuda.get_device_name(0)}', '',
             '| ring x batch | scope | fused head | gather_rows + linear | launches fused / former |', '|---|---|---|---|---|']
    verdict = []
    for shape in args.shapes.split(','):
        ring, batch = (int(v) for v in shape.split('x'))
        scopes = head_scopes(ring, batch)
        for name, fn in scopes.items():
            forms = {'fused': with_form(True, fn), 'former': with_form(False, fn)}
            n_l = {k: launches(f) for k, f in forms.items()}
            try:
                reps, calls = {k: captured(f) for k, f in forms.items()}, CALLS
            except Exception as e:                 # (a form that cannot be captured is timed as eager calls, both forms alike)
                print(f'{name}: not capturable ({type(e).__name__}: {str(e)[:100]}): eager calls, host time included', flush=True)
                torch.cuda.synchronize()
                reps, calls, name = forms, 1, name + ' (eager)'
            r = ab(reps, calls, args.regions, args.min_ms)
            lines.append(f'| {ring} x {batch} | {name} | {r["fused"][0]:.2f} [{r["fused"][1]:.2f} .. {r["fused"][2]:.2f}] | '
                         f'{r["former"][0]:.2f} [{r["former"][1]:.2f} .. {r["former"][2]:.2f}] | {n_l["fused"]} / {n_l["former"]} |')
            verdict.append((shape, name, r['fused'][0], r['former'][0]))
            print(lines[-1], flush=True)
        ms = {}
        for form, fused in (('fused', True), ('former', False)):
            try:
                ms[form] = model_scopes(ring, batch, fused)
            except Exception as e:                 # (reported, not hidden: a form that cannot be captured has no figure)
                lines.append(f'| {ring} x {batch} | model, {form} head | failed: {type(e).__name__}: {str(e)[:160]} | | |')
                print(lines[-1], flush=True)
                torch.cuda.synchronize()
        for v in ms.values():
            v['arm']()
        for name in ('model fwd', 'model step'):
            if name == 'model step':           # (a training step moves the state epoch: the forward graphs are checked before)
                for v in ms.values():
                    v['check']()
            r = ab({k: v[name] for k, v in ms.items()}, 1, args.regions, args.min_ms)
            cell = lambda k: f'{r[k][0]:.1f} [{r[k][1]:.1f} .. {r[k][2]:.1f}]' if k in r else '-'
            lines.append(f'| {ring} x {batch} | {name} | {cell("fused")} | {cell("former")} | |')
            if len(r) == 2:
                verdict.append((shape, name, r['fused'][0], r['former'][0]))
            print(lines[-1], flush=True)
    slower = [(s, n) for s, n, a, b in verdict if a > b]
    lines += ['', 'fused no slower than the former form in every scope: ' + ('yes' if not slower else f'NO: {slower}')]
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
