"""Time the activated coboundary message (csrc/cwn_aggregate_act.hip; layers.FUSED_ACT_MESSAGE) against the form it replaces
-- the generic propagate of an act(Linear(cat(x_j, up_attr))) message: two row gathers, a cat, a per-entry product, the
activation, the segmented reduce -- in ONE process, the two forms alternating.

Shapes:
  float64   the batch of 8 ring lifts of the SR(16,6,2,2) graphs of tools/bench_f64_dense.py under the untrained ELU
            SparseCIN of exp/scripts/cwn-sr.sh, hidden 16 and 64; scopes: one middle layer, the 3- and the 5-layer forward
  float32   an ELU SparseCIN (3 layers, hidden 64) on 128 synthetic ZINC-like molecules; scopes: one middle layer, forward
All eager and under torch.no_grad().  A region is as many calls as fill >= --min-ms of host clock, closed by a device
synchronise; warm-up regions of both forms come first; then the forms alternate region by region.  Reported: the median of
--regions regions per form in microseconds per call, with the spread [min .. max], and the kernels of one call
(torch.profiler, in a pass of its own).  Before anything is timed both forms must agree within the project's gates (1e-11
relative in float64, 1e-5 in float32).  The verdict lines apply the rule for the default, per dtype: the forward with the
switch on must be faster than with it off by more than the larger run-to-run spread (max - min) of the two forms.

    python tools/bench_act_message.py [--out profiles/act_message.md] [--regions 7] [--min-ms 200]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_f64_dense import DEV, F64, ab, launches, sr_batch                # noqa: E402
from cwn_amd import layers                                                  # noqa: E402
from cwn_amd.models import SparseCIN                                        # noqa: E402
from cwn_amd.synthetic import zinc_like_batch                               # noqa: E402

GATE = {torch.float64: 1e-11, torch.float32: 1e-5}


def with_form(on, fn):
    def call():
        prev = layers.FUSED_ACT_MESSAGE
        layers.FUSED_ACT_MESSAGE = on
        try:
            with torch.no_grad():
                return fn()
        finally:
            layers.FUSED_ACT_MESSAGE = prev
    return call


def scopes(batch, x0, dtype, hidden, depths):
    """{scope: fn} of the ELU SparseCIN on `batch`, whose input features are `x0`; every fn sets the features it reads."""
    out = {}
    for num_layers in depths:
        torch.manual_seed(0)
        model = SparseCIN(num_input_features=1, num_classes=16, num_layers=num_layers, hidden=hidden, dropout_rate=0.0,
                          max_dim=2, use_coboundaries=True, nonlinearity='elu', graph_norm='id', readout='sum',
                          final_readout='sum', readout_dims=(0, 1, 2)).to(dtype).to(DEV).eval()

        def forward(model=model):
            batch.set_xs(x0)                                                # (the model's layers write their outputs into the batch)
            return model(batch)
        out[f'forward, {num_layers} layers'] = forward
        if num_layers == depths[0]:
            conv = model.convs[1]
            g = torch.Generator().manual_seed(1)
            xs = [(0.1 * torch.randn(batch.cochains[d].num_cells, hidden, generator=g, dtype=F64)).to(dtype).to(DEV) for d in range(3)]

            def layer(conv=conv, xs=xs):
                batch.set_xs(xs)
                return conv(*batch.get_all_cochain_params(max_dim=2, include_down_features=False))
            out = {'layer': layer, **out}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--regions', type=int, default=7)
    ap.add_argument('--min-ms', type=float, default=200.0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is no other figure'
    sr = sr_batch()
    zinc = zinc_like_batch(128, seed=0, device=DEV)
    shapes = [('float64', 'SR x 8', sr, torch.float64, 16, (3, 5)), ('float64', 'SR x 8', sr, torch.float64, 64, (3, 5)),
              ('float32', 'ZINC-like x 128', zinc, torch.float32, 64, (3,))]
    # (the scopes write the layers' outputs into the batch; SparseCIN takes features as given: rings without any get ones)
    x0 = {id(b): [b.cochains[d].x if b.cochains[d].x is not None else torch.ones(b.cochains[d].num_cells, 1, device=DEV)
                  for d in range(3)] for b in (sr, zinc)}
    cells = lambda b: [b.cochains[d].num_cells for d in range(3)]
    lines = [f'{torch.cuda.get_device_name(0)}; SR x 8: 8 SR(16,6,2,2) ring lifts, {cells(sr)} cells in dimensions 0, 1, 2; ZINC-like x 128: '
             f'{cells(zinc)} cells; ELU SparseCIN, graph_norm id; eager, torch.no_grad(); median of {args.regions} regions of >= '
             f'{args.min_ms:g} ms per form, forms alternating; us per call [min .. max]', '',
             '| dtype | batch | hidden | scope | switch on | switch off | off / on | kernels per call on / off |', '|---|---|---|---|---|---|---|---|']
    verdict = {}
    for dname, bname, batch, dtype, hidden, depths in shapes:
        for name, fn in scopes(batch, x0[id(batch)], dtype, hidden, depths).items():
            forms = {'on': with_form(True, fn), 'off': with_form(False, fn)}
            a, b = forms['on'](), forms['off']()
            a, b = (a, b) if torch.is_tensor(a) else (torch.cat([t.flatten() for t in a]), torch.cat([t.flatten() for t in b]))
            dev = float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
            assert dev <= GATE[dtype], (dname, hidden, name, dev)            # faster and different is not faster
            n_l = {k: launches(f) for k, f in forms.items()}
            r = ab(forms, args.regions, args.min_ms)
            cell = lambda k: f'{r[k][0]:.1f} [{r[k][1]:.1f} .. {r[k][2]:.1f}]'
            lines.append(f'| {dname} | {bname} | {hidden} | {name} | {cell("on")} | {cell("off")} | {r["off"][0] / r["on"][0]:.2f} | '
                         f'{n_l["on"]} / {n_l["off"]} |')
            print(lines[-1] + f'   (on vs off: {dev:.1e} relative)', flush=True)
            verdict[(dname, hidden, name)] = r
    lines.append('')
    for (dname, hidden, name), r in verdict.items():
        if name.startswith('forward') and (dname, hidden) in (('float64', 16), ('float32', 64)):
            gain = r['off'][0] - r['on'][0]
            spread = max(r['on'][2] - r['on'][1], r['off'][2] - r['off'][1])
            lines.append(f'{dname}, hidden {hidden}, {name}: on is {gain:.1f} us per call faster than off; the larger spread of the two forms is '
                         f'{spread:.1f} us: ' + ('faster by more than the spread' if gain > spread else 'NOT faster by more than the spread'))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
