"""Time the float64 dense path (csrc/cwn_dense_f64.hip; layers.FUSED_F64_DENSE) against the form it replaces -- the
torch.nn modules of a double model, a rocBLAS dgemm + bias add + activation launch per Linear -- in ONE process, the two
forms alternating.

Input: a batch of 8 ring lifts (rings up to 6) of the SR(16,6,2,2) graphs -- the 4 x 4 rook's graph, the Shrikhande graph
and three vertex-relabelled copies of each -- the batch size and the family of exp/scripts/cwn-sr.sh.  Model: the untrained
SparseCIN of that experiment (ELU, graph_norm 'id', sum readouts, coboundaries), hidden 16 (the experiment's) and 64.

Scopes, all eager and under torch.no_grad() as the experiment runs them (the float64 path has no captured form), so the
figure is what a user waits for: interpreter, launches and kernels.
  layer            one SparseCINConv (a middle layer: hidden -> hidden) on the batch
  forward, 3 / 5   the whole model, 3 and 5 layers
A region is as many calls as fill >= --min-ms of host clock, closed by a device synchronise; warm-up regions of both forms
come first; then the forms alternate region by region.  Reported: the median of --regions regions per form in microseconds
per call, with the spread [min .. max], and the kernels of one call (torch.profiler, in a call of its own).  The verdict
line applies the rule for the default: at hidden 16 the forward with the switch on must be faster than with it off by more
than the run-to-run spread (max - min) of either form.

    python tools/bench_f64_dense.py [--out profiles/f64_dense.md] [--regions 7] [--min-ms 200]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd import layers                                                  # noqa: E402
from cwn_amd.complex import ComplexBatch                                    # noqa: E402
from cwn_amd.models import SparseCIN                                        # noqa: E402
from cwn_amd.synthetic import relabel, rook_4x4, shrikhande, sr_lift        # noqa: E402

DEV = torch.device('cuda', 0)
F64 = torch.float64


def sr_batch():
    rng = np.random.default_rng(43)
    graphs = []
    for g in (rook_4x4(), shrikhande()):
        graphs += [g] + [relabel(*g, rng.permutation(16)) for _ in range(3)]
    return ComplexBatch.from_complex_list([sr_lift(n, bonds, dtype=F64, max_k=6) for n, bonds in graphs], max_dim=2).to(DEV)


def with_form(on, fn):
    def call():
        prev = layers.FUSED_F64_DENSE
        layers.FUSED_F64_DENSE = on
        try:
            with torch.no_grad():
                return fn()
        finally:
            layers.FUSED_F64_DENSE = prev
    return call


def region_us(fn, min_ms):
    """Microseconds per call over one region of >= min_ms of host clock that ends in a device synchronise."""
    n = 1
    while True:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
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


def scopes(hidden):
    """{scope: fn} on the SR batch; every fn leaves the batch as it found it."""
    out = {}
    batch = sr_batch()
    for num_layers in (3, 5):
        torch.manual_seed(0)
        model = SparseCIN(num_input_features=1, num_classes=16, num_layers=num_layers, hidden=hidden, dropout_rate=0.0,
                          max_dim=2, use_coboundaries=True, nonlinearity='elu', graph_norm='id', readout='sum',
                          final_readout='sum', readout_dims=(0, 1, 2)).double().to(DEV).eval()
        x0 = [batch.cochains[d].x for d in range(3)]

        def forward(model=model, x0=x0):
            batch.set_xs(x0)                                                # (the model's layers write their outputs into the batch)
            return model(batch)
        out[f'forward, {num_layers} layers'] = forward
        if num_layers == 3:
            conv = model.convs[1]
            g = torch.Generator().manual_seed(1)
            xs = [torch.randn(batch.cochains[d].num_cells, hidden, generator=g, dtype=F64).to(DEV) for d in range(3)]

            def layer(conv=conv, xs=xs):
                batch.set_xs(xs)
                return conv(*batch.get_all_cochain_params(max_dim=2, include_down_features=False))
            out = {'layer': layer, **out}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--regions', type=int, default=7)
    ap.add_argument('--min-ms', type=float, default=200.0)
    ap.add_argument('--hidden', default='16,64')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is no other figure'
    cells = [sr_batch().cochains[d].num_cells for d in range(3)]
    lines = [f'{torch.cuda.get_device_name(0)}; batch of 8 SR(16,6,2,2) ring lifts: {cells} cells in dimensions 0, 1, 2; float64; eager, '
             f'torch.no_grad(); median of {args.regions} regions of >= {args.min_ms:g} ms per form, forms alternating; '
             'us per call [min .. max]', '',
             '| hidden | scope | switch on | switch off | off / on | kernels per call on / off |', '|---|---|---|---|---|---|']
    verdict = {}
    for hidden in (int(h) for h in args.hidden.split(',')):
        for name, fn in scopes(hidden).items():
            forms = {'on': with_form(True, fn), 'off': with_form(False, fn)}
            a, b = forms['on'](), forms['off']()
            a, b = (a, b) if torch.is_tensor(a) else (torch.cat([t.flatten() for t in a]), torch.cat([t.flatten() for t in b]))
            dev = float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
            assert dev <= 1e-11, (hidden, name, dev)                        # faster and different is not faster
            n_l = {k: launches(f) for k, f in forms.items()}
            r = ab(forms, args.regions, args.min_ms)
            cell = lambda k: f'{r[k][0]:.1f} [{r[k][1]:.1f} .. {r[k][2]:.1f}]'
            lines.append(f'| {hidden} | {name} | {cell("on")} | {cell("off")} | {r["off"][0] / r["on"][0]:.2f} | {n_l["on"]} / {n_l["off"]} |')
            print(lines[-1] + f'   (on vs off: {dev:.1e} relative)', flush=True)
            verdict[(hidden, name)] = r
    lines.append('')
    for (hidden, name), r in verdict.items():
        if hidden == 16 and name.startswith('forward'):
            gain = r['off'][0] - r['on'][0]
            spread = max(r['on'][2] - r['on'][1], r['off'][2] - r['off'][1])
            lines.append(f'hidden 16, {name}: on is {gain:.1f} us per call faster than off; the larger spread of the two forms is {spread:.1f} us: '
                         + ('faster by more than the spread' if gain > spread else 'NOT faster by more than the spread'))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
