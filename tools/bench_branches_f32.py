"""Time the float32 update branches (csrc/cwn_branches_f32.hip; layers.FUSED_BRANCHES_F32) against the routes they replace, in
ONE process, the two forms alternating -- the same build with the switch off is the route of the commit before:
  regime 'relu_width'   a grouped cwn_gemm_f32 launch per update stage, then torch.cat + combine_nn as torch modules (ReLU
                        networks that cwn_update_mlp3_f32 does not take)
  regime 'act'          the torch.nn modules of the update / combine networks (elu: a GEMM, a bias add, a BatchNorm and an
                        activation launch per Linear, and the cat)

Input: synthetic.zinc_like_batch(128).  Untrained, eval mode:
  EmbedCINpp, hidden 48, ReLU, 2 layers             (exp/scripts/cin++-zinc-small.sh: --emb_dim 48)
  EmbedCINpp, hidden 16, elu, 2 layers
  CINpp over one raw feature per cell, hidden 64, ReLU, 2 layers    (the first layer has F != H; the second is
                                                                     cwn_update_mlp3_f32's with the switch on or off)
  one CINppConv(coboundary_stream=True) layer at 64, ReLU, random features   (four branches)
Eager, under torch.no_grad().  A region is as many calls as fill >= --min-ms of host clock, closed by a device synchronise;
warm-up regions of both forms come first; then the forms alternate region by region.  Reported: the median of --regions
regions per form in microseconds per call with p10 .. p90 and [min .. max], and the kernels of one call (torch.profiler, in a
call of its own).  The verdict lines apply the rule for the default: a regime is on by default when every one of its scopes
is faster with the switch on than with it off by more than the larger run-to-run spread (max - min) of the two forms.

    python tools/bench_branches_f32.py [--out profiles/branches_f32.md] [--regions 15] [--min-ms 150]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd import layers                                                  # noqa: E402
from cwn_amd.layers import CINppConv                                        # noqa: E402
from cwn_amd.models import CINpp, EmbedCINpp                                # noqa: E402
from cwn_amd.synthetic import zinc_like_batch                               # noqa: E402

DEV = torch.device('cuda', 0)
LAYERS = 2


def with_form(on, fn):
    def call():
        prev = layers.FUSED_BRANCHES_F32
        layers.FUSED_BRANCHES_F32 = layers.BRANCHES_F32_REGIMES if on else frozenset()
        try:
            with torch.no_grad():
                return fn()
        finally:
            layers.FUSED_BRANCHES_F32 = prev
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
        region_us(f, min_ms / 4)                                             # warm-up: code objects, prepared launches
    for _ in range(regions):
        for k, f in forms.items():
            got[k].append(region_us(f, min_ms))
    return {k: dict(med=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)), lo=min(v), hi=max(v))
            for k, v in got.items()}


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


def scope(kind, hidden, nonlinearity):
    """(cells, name, fn) on the ZINC-like batch; fn leaves the batch as it found it."""
    batch = zinc_like_batch(128, seed=0).to(DEV)
    cells = [batch.cochains[d].num_cells for d in range(3)]
    torch.manual_seed(0)
    if kind == 'CINppConv 4 streams':
        act = {'relu': torch.nn.ReLU, 'elu': torch.nn.ELU}[nonlinearity]
        conv = CINppConv(hidden, hidden, hidden, None, None, None, None, None, None, max_dim=2, hidden=hidden, act_module=act,
                         layer_dim=hidden, use_coboundaries=True, coboundary_stream=True).to(DEV).eval()
        g = torch.Generator().manual_seed(1)
        xs = [torch.randn(n, hidden, generator=g).to(DEV) for n in cells]

        def layer():
            batch.set_xs(xs)
            return conv(*batch.get_all_cochain_params(max_dim=2, include_down_features=False))
        return cells, 'layer', layer
    if kind == 'EmbedCINpp':
        model = EmbedCINpp(28, 4, 1, LAYERS, hidden, dropout_rate=0.0, embed_edge=True, use_coboundaries=True, nonlinearity=nonlinearity)
        x0 = [batch.cochains[d].x for d in range(3)]
    else:
        model = CINpp(1, 1, LAYERS, hidden, dropout_rate=0.0, max_dim=2, use_coboundaries=True, nonlinearity=nonlinearity)
        x0 = [torch.ones(n, 1, device=DEV) for n in cells]
    model = model.to(DEV).eval()

    def forward():
        batch.set_xs(x0)                                                    # (the model's layers write their outputs into the batch)
        return model(batch)
    return cells, f'forward, {LAYERS} layers', forward


CONFIGS = [('EmbedCINpp', 48, 'relu', 'relu_width'), ('EmbedCINpp', 16, 'elu', 'act'), ('CINpp raw features', 64, 'relu', 'relu_width'),
           ('CINppConv 4 streams', 64, 'relu', 'relu_width')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--regions', type=int, default=15)
    ap.add_argument('--min-ms', type=float, default=150.0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is no other figure'
    lines, verdict, cells = [], {}, None
    for kind, hidden, act, regime in CONFIGS:
        cells, name, fn = scope(kind, hidden, act)
        forms = {'on': with_form(True, fn), 'off': with_form(False, fn)}
        a, b = forms['on'](), forms['off']()
        a, b = (a, b) if torch.is_tensor(a) else (torch.cat([t.flatten() for t in a]), torch.cat([t.flatten() for t in b]))
        dev = float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
        assert dev <= 1e-5, (kind, hidden, name, dev)                       # faster and different is not faster
        n_l = {k: launches(f) for k, f in forms.items()}
        r = ab(forms, args.regions, args.min_ms)
        cell = lambda k: f'{r[k]["med"]:.1f} ({r[k]["p10"]:.1f} .. {r[k]["p90"]:.1f}) [{r[k]["lo"]:.1f} .. {r[k]["hi"]:.1f}]'
        lines.append(f'| {kind} {hidden} {act} | {regime} | {name} | {cell("on")} | {cell("off")} | {r["off"]["med"] / r["on"]["med"]:.2f} | '
                     f'{n_l["on"]} / {n_l["off"]} |')
        print(lines[-1] + f'   (on vs off: {dev:.1e} relative)', flush=True)
        verdict[(kind, hidden, act, regime, name)] = r
    head = [f'{torch.cuda.get_device_name(0)}; synthetic.zinc_like_batch(128): {cells} cells in dimensions 0, 1, 2; float32; eager, '
            f'torch.no_grad(); median of {args.regions} regions of >= {args.min_ms:g} ms per form, forms alternating; us per call: '
            'median (p10 .. p90) [min .. max]', '',
            '| model | regime | scope | switch on | switch off | off / on | kernels per call on / off |', '|---|---|---|---|---|---|---|']
    lines = head + lines + ['']
    wins = {}
    for (kind, hidden, act, regime, name), r in verdict.items():
        gain = r['off']['med'] - r['on']['med']
        spread = max(r['on']['hi'] - r['on']['lo'], r['off']['hi'] - r['off']['lo'])
        wins.setdefault(regime, []).append(gain > spread)
        lines.append(f"'{regime}', {kind} {hidden} {act}, {name}: on is {gain:.1f} us per call faster than off; the larger spread of the "
                     f'two forms is {spread:.1f} us: ' + ('faster by more than the spread' if gain > spread else
                                                           'NOT faster by more than the spread'))
    lines.append('')
    for regime, ws in wins.items():
        lines.append(f"'{regime}': " + ('every scope is faster by more than the spread' if all(ws) else 'not every scope is faster by more than the spread'))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
