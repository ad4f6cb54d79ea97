"""One SparseCINConv layer built with graph_norm='ln': the grouped GEMM + LayerNorm launches (cwn_amd/dense_ln.py,
csrc/cwn_layernorm.hip) against the torch modules the layer ran before (dense_ln.FUSED_LN = False, CWN_FUSED_LN=0), in the
same process.

Shapes: a ZINC-like batch of 128 molecules at width 128, and the CSL batch of exp/scripts/cwn-csl.sh (12 circulant graphs of
41 vertices, rings up to 8) at width 160.  Modes: forward without autograd, and forward + backward.

Timing: graph-free back-to-back calls between two device events after a warm-up, as many calls per region as make it last
at least 50 ms, the two forms alternating, five regions each, the median per call with the spread.  Launches: the device
kernels of ONE call, counted by torch.profiler in a run of its own.

    python tools/bench_ln.py [--out profiles/ln_layer.md]        (needs an MI355X)
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd import dense_ln                                               # noqa: E402
from cwn_amd.complex import ComplexBatch                                   # noqa: E402
from cwn_amd.layers import SparseCINConv                                   # noqa: E402
from cwn_amd.synthetic import csl_graphs, zinc_like_batch                  # noqa: E402

DEV = torch.device('cuda', 0)
REGION_MS, REGIONS = 50.0, 5


def make_case(batch, F):
    torch.manual_seed(0)
    conv = SparseCINConv(F, F, F, None, None, None, None, max_dim=2, hidden=F, act_module=torch.nn.ReLU, layer_dim=F,
                         use_coboundaries=True, graph_norm=torch.nn.LayerNorm).to(DEV)
    g = torch.Generator().manual_seed(1)
    for d in range(3):
        batch.cochains[d].x = torch.randn(batch.cochains[d].num_cells, F, generator=g)
    batch = batch.to(DEV).prepare(backward=True)
    xs = [batch.cochains[d].x.requires_grad_(True) for d in range(3)]
    params = batch.get_all_cochain_params(max_dim=2, include_down_features=False)

    def forward():
        with torch.no_grad():
            return conv.eval()(*params)

    def train():
        conv.train()
        for t in list(conv.parameters()) + xs:
            t.grad = None
        outs = conv(*params)
        torch.autograd.backward(outs, [torch.ones_like(o) for o in outs])
        return outs

    return {'forward': forward, 'forward + backward': train}


def with_switch(on, fn):
    prev, dense_ln.FUSED_LN = dense_ln.FUSED_LN, on
    try:
        return fn()
    finally:
        dense_ln.FUSED_LN = prev


def region(fn, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if getattr(e, 'device_type', None) == torch.autograd.DeviceType.CUDA
               and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='write the table (markdown) here as well')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ln needs the GPU: nothing is measured without one')
    shapes = [('ZINC-like batch of 128, width 128', zinc_like_batch(128, seed=0), 128),
              ('CSL batch (12 x 41 vertices, rings <= 8), width 160',
               ComplexBatch.from_complex_list(csl_graphs(12, seed=0, max_ring=8), max_dim=2), 160)]
    rows = []
    for label, batch, F in shapes:
        cells = [batch.cochains[d].num_cells for d in range(3)]
        for mode, fn in make_case(batch, F).items():
            forms = {'grouped GEMM + LayerNorm launches': True, 'torch modules (CWN_FUSED_LN=0)': False}
            # the outputs of the two forms agree (fp32 rounding) before anything is timed
            a, b = with_switch(True, fn), with_switch(False, fn)
            diff = max(float((x - y).abs().max()) for x, y in zip(a, b))
            calls, times, launches = {}, {name: [] for name in forms}, {}
            for name, on in forms.items():
                for _ in range(10):
                    with_switch(on, fn)
                torch.cuda.synchronize()
                per = with_switch(on, lambda: region(fn, 20)) / 20
                calls[name] = max(20, int(REGION_MS / per) + 1)
            for _ in range(REGIONS):
                for name, on in forms.items():          # alternating: drift hits both forms alike
                    times[name].append(with_switch(on, lambda: region(fn, calls[name])) / calls[name] * 1e3)
            for name, on in forms.items():
                try:
                    launches[name] = with_switch(on, lambda: count_launches(fn))
                except Exception as e:                   # (the count is a by-product: the times stand without it)
                    launches[name] = f'not counted ({type(e).__name__})'
            for name in forms:
                ts = times[name]
                rows.append(dict(shape=label, cells=cells, mode=mode, form=name, us=round(statistics.median(ts), 2),
                                 us_min=round(min(ts), 2), us_max=round(max(ts), 2), calls_per_region=calls[name],
                                 launches=launches[name], max_abs_diff_between_forms=diff))
    lines = ['| shape | mode | form | us per call (median of 5) | min .. max | device launches per call |',
             '|---|---|---|---|---|---|']
    for r in rows:
        lines.append(f"| {r['shape']} (cells {r['cells']}) | {r['mode']} | {r['form']} | {r['us']:.1f} | {r['us_min']:.1f} .. "
                     f"{r['us_max']:.1f} | {r['launches']} |")
    table = '\n'.join(lines)
    print(table)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(table + '\n')
    print(json.dumps(dict(tool='bench_ln', region_ms=REGION_MS, regions=REGIONS, rows=rows)))


if __name__ == '__main__':
    main()
