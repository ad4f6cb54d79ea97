"""Time MessagePassingAgnostic as two launches (csrc/cwn_agnostic.hip; models.FUSED_AGNOSTIC) against the form it replaces
-- per dimension a Linear, an activation and the pooling reduce, then a stack, lin1, the activation, a sum and lin2 as torch
modules and the segmented-reduce kernel -- in ONE process, the two forms alternating.

Input: a batch of 8 ring lifts (rings up to 6) of the SR(16,6,2,2) graphs -- the 4 x 4 rook's graph, the Shrikhande graph
and three vertex-relabelled copies of each -- the batch size and the family of exp/scripts/cwn-sr-base.sh.  Model: the
untrained control of that experiment: hidden 256, ELU, sum readout, 16 classes; float64 (the experiment's) and float32.

The forward is eager and under torch.no_grad() as the experiment runs it, so the figure is what a user waits for:
interpreter, launches and kernels.  A region is as many forwards as fill >= --min-ms between two device events; warm-up
regions of both forms come first; then the forms alternate region by region.  Reported: the median of --regions regions per
form in microseconds per forward, with the spread [min .. max], and the kernels of one forward (torch.profiler, in a call of
its own).  The verdict line applies the rule for the default: the route is on by default for a dtype only when it is faster
than the unfused form by more than the run-to-run spread (max - min) of either form.

    python tools/bench_agnostic.py [--out profiles/sr_baseline.md] [--regions 5] [--min-ms 50]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd import models                                                  # noqa: E402
from cwn_amd.complex import ComplexBatch                                    # noqa: E402
from cwn_amd.models import MessagePassingAgnostic                           # noqa: E402
from cwn_amd.synthetic import relabel, rook_4x4, shrikhande, sr_lift        # noqa: E402

DEV = torch.device('cuda', 0)
TOL = {torch.float32: 1e-5, torch.float64: 1e-11}


def sr_batch(dtype):
    rng = np.random.default_rng(43)
    graphs = []
    for g in (rook_4x4(), shrikhande()):
        graphs += [g] + [relabel(*g, rng.permutation(16)) for _ in range(3)]
    return ComplexBatch.from_complex_list([sr_lift(n, bonds, dtype=dtype, max_k=6) for n, bonds in graphs], max_dim=2).to(DEV)


def with_form(on, model, batch):
    def call():
        prev = models.FUSED_AGNOSTIC
        models.FUSED_AGNOSTIC = on
        try:
            with torch.no_grad():
                out = model(batch)
        finally:
            models.FUSED_AGNOSTIC = prev
        assert model.last_route == ('fused' if on else 'torch')
        return out
    return call


def region_us(fn, min_ms):
    """Microseconds per call over one region of >= min_ms between two device events."""
    n = 1
    while True:
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(n):
            fn()
        end.record()
        end.synchronize()
        ms = start.elapsed_time(end)
        if ms >= min_ms:
            return ms * 1e3 / n
        n = max(n + 1, int(n * min_ms / max(ms, 1e-3) * 1.2))


def ab(forms, regions, min_ms):
    got = {k: [] for k in forms}
    for k, f in forms.items():
        region_us(f, min_ms / 4)                                             # warm-up: code objects, rocBLAS's choices
    for _ in range(regions):
        for k, f in forms.items():
            got[k].append(region_us(f, min_ms))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--regions', type=int, default=5)
    ap.add_argument('--min-ms', type=float, default=50.0)
    ap.add_argument('--hidden', type=int, default=256)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is no other figure'
    cells = [sr_batch(torch.float64).cochains[d].num_cells for d in range(3)]
    lines = [f'{torch.cuda.get_device_name(0)}; batch of 8 SR(16,6,2,2) ring lifts: {cells} cells in dimensions 0, 1, 2; '
             f'MessagePassingAgnostic, hidden {args.hidden}, ELU, sum readout; eager, torch.no_grad(); median of {args.regions} regions of '
             f'>= {args.min_ms:g} ms between device events per form, forms alternating; us per forward [min .. max]', '',
             '| dtype | FUSED_AGNOSTIC on | FUSED_AGNOSTIC off | off / on | kernels per forward on / off |', '|---|---|---|---|---|']
    verdict = {}
    for dtype in (torch.float64, torch.float32):
        torch.manual_seed(0)
        model = MessagePassingAgnostic(1, 16, args.hidden, dropout_rate=0.0, max_dim=2, nonlinearity='elu',
                                       readout='sum').to(dtype).to(DEV).eval()
        batch = sr_batch(dtype)
        forms = {'on': with_form(True, model, batch), 'off': with_form(False, model, batch)}
        a, b = forms['on'](), forms['off']()
        dev = float((a.double() - b.double()).abs().max()) / max(1.0, float(b.abs().max()))
        assert dev <= TOL[dtype], (dtype, dev)                               # faster and different is not faster
        n_l = {k: launches(f) for k, f in forms.items()}
        r = ab(forms, args.regions, args.min_ms)
        cell = lambda k: f'{r[k][0]:.1f} [{r[k][1]:.1f} .. {r[k][2]:.1f}]'
        name = str(dtype).replace('torch.', '')
        lines.append(f'| {name} | {cell("on")} | {cell("off")} | {r["off"][0] / r["on"][0]:.2f} | {n_l["on"]} / {n_l["off"]} |')
        print(lines[-1] + f'   (on vs off: {dev:.1e} relative)', flush=True)
        verdict[name] = r
    lines.append('')
    for name, r in verdict.items():
        gain = r['off'][0] - r['on'][0]
        spread = max(r['on'][2] - r['on'][1], r['off'][2] - r['off'][1])
        lines.append(f'{name}: on is {gain:.1f} us per forward faster than off; the larger spread of the two forms is {spread:.1f} us: '
                     + ('faster by more than the spread' if gain > spread else 'NOT faster by more than the spread'))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
