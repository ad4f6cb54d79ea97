"""Time the float32 update chain (csrc/cwn_chain_f32.hip; layers.FUSED_CHAIN_F32) against the routes it replaces, in ONE
process, the two forms alternating:
  regime 'relu_width'   a grouped cwn_gemm_f32 launch per update stage + the combine launch (ReLU at a width that
                        cwn_update_mlp_f32 does not take)
  regime 'act'          the torch.nn modules of the update / combine networks (elu: a GEMM, a bias add, a BatchNorm and an
                        activation launch per Linear)

Input: synthetic.zinc_like_batch(128).  Models, untrained, eval mode:
  EmbedSparseCIN, hidden 48 and 16, ReLU, 4 layers        (exp/scripts/cwn-zinc-small.sh: --emb_dim 48; the TU grid's 16)
  SparseCIN, hidden 64, elu, 4 layers, one constant input feature per cell
Scopes, eager and under torch.no_grad(): one SparseCINConv (a middle layer: hidden -> hidden, random features) and the whole
4-layer forward.  A region is as many calls as fill >= --min-ms of host clock, closed by a device synchronise; warm-up regions
of both forms come first; then the forms alternate region by region.  Reported: the median of --regions regions per form in
microseconds per call with the spread [min .. max], and the kernels of one call (torch.profiler, in a call of its own).
The verdict lines apply the rule for the default: a regime is on by default when its forward with the switch on is
faster than with it off by more than the larger run-to-run spread (max - min) of the two forms.

    python tools/bench_chain_f32.py [--out profiles/chain_f32.md] [--regions 7] [--min-ms 200]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd import layers                                                  # noqa: E402
from cwn_amd.models import EmbedSparseCIN, SparseCIN                        # noqa: E402
from cwn_amd.synthetic import zinc_like_batch                               # noqa: E402

DEV = torch.device('cuda', 0)
LAYERS = 4


def with_form(on, fn):
    def call():
        prev = layers.FUSED_CHAIN_F32
        layers.FUSED_CHAIN_F32 = layers.CHAIN_F32_REGIMES if on else frozenset()
        try:
            with torch.no_grad():
                return fn()
        finally:
            layers.FUSED_CHAIN_F32 = prev
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


def scopes(kind, hidden, nonlinearity):
    """{scope: fn} on the ZINC-like batch; every fn leaves the batch as it found it."""
    batch = zinc_like_batch(128, seed=0).to(DEV)
    cells = [batch.cochains[d].num_cells for d in range(3)]
    torch.manual_seed(0)
    if kind == 'EmbedSparseCIN':
        model = EmbedSparseCIN(28, 4, 1, LAYERS, hidden, dropout_rate=0.0, embed_edge=True, use_coboundaries=True,
                               nonlinearity=nonlinearity)
        x0 = [batch.cochains[d].x for d in range(3)]
    else:
        model = SparseCIN(1, 1, LAYERS, hidden, dropout_rate=0.0, max_dim=2, use_coboundaries=True, nonlinearity=nonlinearity)
        x0 = [torch.ones(n, 1, device=DEV) for n in cells]
    model = model.to(DEV).eval()
    g = torch.Generator().manual_seed(1)
    xs = [torch.randn(n, hidden, generator=g).to(DEV) for n in cells]
    conv = model.convs[1]

    def layer():
        batch.set_xs(xs)
        return conv(*batch.get_all_cochain_params(max_dim=2, include_down_features=False))

    def forward():
        batch.set_xs(x0)                                                    # (the model's layers write their outputs into the batch)
        return model(batch)
    return cells, {'layer': layer, f'forward, {LAYERS} layers': forward}


CONFIGS = [('EmbedSparseCIN', 48, 'relu', 'relu_width'), ('EmbedSparseCIN', 16, 'relu', 'relu_width'), ('SparseCIN', 64, 'elu', 'act')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--regions', type=int, default=7)
    ap.add_argument('--min-ms', type=float, default=200.0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is no other figure'
    lines, verdict, cells = [], {}, None
    for kind, hidden, act, regime in CONFIGS:
        cells, fns = scopes(kind, hidden, act)
        for name, fn in fns.items():
            forms = {'on': with_form(True, fn), 'off': with_form(False, fn)}
            a, b = forms['on'](), forms['off']()
            a, b = (a, b) if torch.is_tensor(a) else (torch.cat([t.flatten() for t in a]), torch.cat([t.flatten() for t in b]))
            dev = float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
            assert dev <= 1e-5, (kind, hidden, name, dev)                   # faster and different is not faster
            n_l = {k: launches(f) for k, f in forms.items()}
            r = ab(forms, args.regions, args.min_ms)
            cell = lambda k: f'{r[k][0]:.1f} [{r[k][1]:.1f} .. {r[k][2]:.1f}]'
            lines.append(f'| {kind} {hidden} {act} | {regime} | {name} | {cell("on")} | {cell("off")} | {r["off"][0] / r["on"][0]:.2f} | '
                         f'{n_l["on"]} / {n_l["off"]} |')
            print(lines[-1] + f'   (on vs off: {dev:.1e} relative)', flush=True)
            verdict[(kind, hidden, act, regime, name)] = r
    head = [f'{torch.cuda.get_device_name(0)}; synthetic.zinc_like_batch(128): {cells} cells in dimensions 0, 1, 2; float32; eager, '
            f'torch.no_grad(); median of {args.regions} regions of >= {args.min_ms:g} ms per form, forms alternating; us per call '
            '[min .. max]', '',
            '| model | regime | scope | switch on | switch off | off / on | kernels per call on / off |', '|---|---|---|---|---|---|---|']
    lines = head + lines + ['']
    for (kind, hidden, act, regime, name), r in verdict.items():
        if name.startswith('forward'):
            gain = r['off'][0] - r['on'][0]
            spread = max(r['on'][2] - r['on'][1], r['off'][2] - r['off'][1])
            lines.append(f"'{regime}', {kind} {hidden} {act}, {name}: on is {gain:.1f} us per call faster than off; the larger spread of the "
                         f'two forms is {spread:.1f} us: ' + ('faster by more than the spread' if gain > spread else
                                                               'NOT faster by more than the spread'))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
