"""Time forward + backward of a non-ReLU model with the activated message's backward on the device
(csrc/cwn_aggregate_act_bwd.hip; ops.ACT_MESSAGE_BACKWARD) against the form it replaces under a recording autograd -- the
generic propagate of an act(Linear(cat(x_j, up_attr))) message: two row gathers, a cat, a per-entry product, the
activation, the segmented reduce, and autograd's own backward over those per-entry tensors -- in ONE process, the two forms
alternating.

Shapes:
  float64   the batch of 8 ring lifts of the SR(16,6,2,2) graphs of tools/bench_f64_dense.py under the untrained ELU
            SparseCIN of exp/scripts/cwn-sr.sh (hidden 16, 3 layers)
  float32   an ELU SparseCIN (3 layers, hidden 64) on 128 synthetic ZINC-like molecules
One call is model(batch), an MSE loss against a fixed target and loss.backward(), eager, layers.FUSED_ACT_MESSAGE on for
both forms (it decides the inference route only).  A region is as many calls as fill >= --min-ms of host clock, closed by a
device synchronise; warm-up regions of both forms come first; then the forms alternate region by region.  Reported: the
median of --regions regions per form in microseconds per call with [p10 .. p90], and the kernels of one call (torch.profiler,
in a pass of its own).  Before anything is timed the two forms' losses and weight gradients must agree within the project's
gates (1e-11 relative in float64, 1e-5 in float32).  The verdict lines say whether the switch-on form is faster by more than
the larger spread (p90 - p10) of the two forms.  The default of the switch does not follow from the figure: it stays off.

    python tools/bench_act_message_train.py [--out profiles/act_message_train.md] [--regions 9] [--min-ms 200]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_f64_dense import DEV, launches, region_us, sr_batch              # noqa: E402
from cwn_amd import layers, ops                                             # noqa: E402
from cwn_amd.models import SparseCIN                                        # noqa: E402
from cwn_amd.synthetic import zinc_like_batch                               # noqa: E402

GATE = {torch.float64: 1e-11, torch.float32: 1e-5}


def with_form(on, fn):
    def call():
        prev = ops.ACT_MESSAGE_BACKWARD, layers.FUSED_ACT_MESSAGE
        ops.ACT_MESSAGE_BACKWARD, layers.FUSED_ACT_MESSAGE = on, True
        try:
            return fn()
        finally:
            ops.ACT_MESSAGE_BACKWARD, layers.FUSED_ACT_MESSAGE = prev
    return call


def step_of(batch, x0, dtype, hidden, num_layers):
    """(fn, model): fn runs forward, loss and backward of the ELU SparseCIN on `batch` and returns the loss."""
    torch.manual_seed(0)
    model = SparseCIN(num_input_features=1, num_classes=16, num_layers=num_layers, hidden=hidden, dropout_rate=0.0, max_dim=2,
                      use_coboundaries=True, nonlinearity='elu', graph_norm='id', readout='sum', final_readout='sum',
                      readout_dims=(0, 1, 2)).to(dtype).to(DEV).eval()
    target = None

    def step():
        nonlocal target
        batch.set_xs(x0)                                                    # (the model's layers write their outputs into the batch)
        model.zero_grad(set_to_none=True)
        out = model(batch)
        if target is None:
            target = torch.linspace(-1, 1, out.numel(), dtype=dtype, device=DEV).reshape(out.shape)
        loss = torch.nn.functional.mse_loss(out, target)
        loss.backward()
        return loss.detach()
    return step, model


def ab(forms, regions, min_ms):
    got = {k: [] for k in forms}
    for f in forms.values():
        region_us(f, min_ms / 4)                                            # warm-up: code objects, rocBLAS's choices
    for _ in range(regions):
        for k, f in forms.items():
            got[k].append(region_us(f, min_ms))
    return {k: (float(np.median(v)), float(np.percentile(v, 10)), float(np.percentile(v, 90))) for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--regions', type=int, default=9)
    ap.add_argument('--min-ms', type=float, default=200.0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is no other figure'
    sr = sr_batch()
    zinc = zinc_like_batch(128, seed=0, device=DEV)
    shapes = [('float64', 'SR x 8', sr, torch.float64, 16, 3), ('float32', 'ZINC-like x 128', zinc, torch.float32, 64, 3)]
    x0 = {id(b): [b.cochains[d].x if b.cochains[d].x is not None else torch.ones(b.cochains[d].num_cells, 1, device=DEV)
                  for d in range(3)] for b in (sr, zinc)}
    cells = lambda b: [b.cochains[d].num_cells for d in range(3)]
    lines = [f'{torch.cuda.get_device_name(0)}; SR x 8: 8 SR(16,6,2,2) ring lifts, {cells(sr)} cells in dimensions 0, 1, 2; ZINC-like x 128: '
             f'{cells(zinc)} cells; ELU SparseCIN, 3 layers, graph_norm id; forward + MSE loss + backward, eager; median of '
             f'{args.regions} regions of >= {args.min_ms:g} ms per form, forms alternating; us per call [p10 .. p90]', '',
             '| dtype | batch | hidden | switch on | switch off | off / on | kernels per call on / off |', '|---|---|---|---|---|---|---|']
    verdicts = []
    for dname, bname, batch, dtype, hidden, depth in shapes:
        step, model = step_of(batch, x0[id(batch)], dtype, hidden, depth)
        forms = {'on': with_form(True, step), 'off': with_form(False, step)}
        ref = {}
        for k, f in forms.items():
            loss = f()
            ref[k] = torch.cat([loss.reshape(1)] + [p.grad.flatten() for p in model.parameters() if p.grad is not None])
        dev = float((ref['on'] - ref['off']).abs().max()) / max(1.0, float(ref['off'].abs().max()))
        assert dev <= GATE[dtype], (dname, hidden, dev)                     # faster and different is not faster
        n_l = {k: launches(f) for k, f in forms.items()}
        r = ab(forms, args.regions, args.min_ms)
        cell = lambda k: f'{r[k][0]:.1f} [{r[k][1]:.1f} .. {r[k][2]:.1f}]'
        lines.append(f'| {dname} | {bname} | {hidden} | {cell("on")} | {cell("off")} | {r["off"][0] / r["on"][0]:.2f} | '
                     f'{n_l["on"]} / {n_l["off"]} |')
        print(lines[-1] + f'   (loss and gradients, on vs off: {dev:.1e} relative)', flush=True)
        gain = r['off'][0] - r['on'][0]
        spread = max(r['on'][2] - r['on'][1], r['off'][2] - r['off'][1])
        verdicts.append(f'{dname}, hidden {hidden}, forward + backward: on is {gain:.1f} us per call faster than off; the larger spread '
                        f'(p90 - p10) of the two forms is {spread:.1f} us: '
                        + ('faster by more than the spread' if gain > spread else 'NOT faster by more than the spread'))
    text = '\n'.join(lines + [''] + verdicts)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
