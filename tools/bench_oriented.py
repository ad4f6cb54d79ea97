"""Time the fused OrientedConv layer (csrc/cwn_oriented.hip) against the launches it replaces, on the flow workload of
examples/train_flow.py: edge_flows(64, side 32) as one CochainBatch (64 x ~2700 edges).

Scopes, each as the median of HIP-event intervals around ONE call (warm-up first, then --iters timed calls; the spread is
the 10th .. 90th percentile), with layers.FUSED_ORIENTED on and again off:
  layer fwd           one OrientedConv.forward, no autograd, at (w, H) = (1, 64) and (64, 64), tanh
  layer fwd+bwd       the same with autograd recording plus backward of out.sum() (weights and, at 64, x need gradients)
  model fwd           a 4-layer EdgeOrient (hidden 64, tanh) eval forward
  model step          an eager training step of it: forward, cross-entropy, backward, torch.optim.Adam.step

    python tools/bench_oriented.py [--iters 300] [--warmup 30] [--only off] [--out profiles/oriented_layer.md]

--only off: the unfused figures alone -- what a checkout without the fused layer runs (given this file and
cwn_amd/synthetic.py; the switch is then absent and ignored): the parent's figures of profiles/oriented_layer.md.  Results are printed as a markdown table and appended to --out when given.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd import layers, models                                      # noqa: E402
from cwn_amd.complex import CochainBatch                                 # noqa: E402
from cwn_amd.synthetic import edge_flows                                 # noqa: E402

DEV = torch.device('cuda', 0)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[len(ts) // 10], ts[len(ts) * 9 // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=300)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--complexes', type=int, default=64)
    ap.add_argument('--side', type=int, default=32)
    ap.add_argument('--only', choices=('both', 'off'), default='both')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    data = CochainBatch.from_cochain_list(edge_flows(args.complexes, args.side, seed=0))
    for k in ('x', 'upper_index', 'lower_index', 'upper_orient', 'lower_orient', 'batch', 'y'):
        setattr(data, k, getattr(data, k).to(DEV))
    x1 = data.x.clone()
    n = x1.size(0)
    torch.manual_seed(0)
    x64 = torch.randn(n, 64, device=DEV)
    act = torch.tanh
    lin = lambda w: torch.nn.Linear(w, 64, bias=False)
    convs = {w: layers.OrientedConv(1, w, w, lin(w), lin(w), lin(w), act).to(DEV) for w in (1, 64)}
    model = models.EdgeOrient(1, 2, 4, 64, nonlinearity='tanh').to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    y = data.y.view(-1)

    def layer_fwd(w):
        data.x = x1 if w == 1 else x64
        with torch.no_grad():
            convs[w](data)

    def layer_fwd_bwd(w):
        data.x = x1 if w == 1 else x64.requires_grad_(True)
        convs[w](data).sum().backward()

    def model_fwd():
        data.x = x1
        with torch.no_grad():
            model(data)

    def model_step():
        data.x = x1
        opt.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(model(data), y).backward()
        opt.step()

    scopes = [('layer fwd (1, 64)', lambda: layer_fwd(1)), ('layer fwd (64, 64)', lambda: layer_fwd(64)),
              ('layer fwd+bwd (1, 64)', lambda: layer_fwd_bwd(1)), ('layer fwd+bwd (64, 64)', lambda: layer_fwd_bwd(64)),
              ('model fwd, 4 layers', model_fwd), ('model step, 4 layers', model_step)]
    lines = [f'rows {n}, lower entries {data.lower_index.size(1)}, upper entries {data.upper_index.size(1)}; '
             f'{args.iters} timed calls after {args.warmup}; median [p10 .. p90] in us', '',
             '| scope | fused on | fused off |', '|---|---|---|']
    for name, fn in scopes:
        cells = []
        for fused in (True, False):
            if fused and (args.only == 'off' or not hasattr(layers, 'FUSED_ORIENTED')):
                cells.append('-')
                continue
            model.eval() if 'fwd' in name and 'bwd' not in name else model.train()
            layers.FUSED_ORIENTED = fused
            med, lo, hi = timed(fn, args.iters, args.warmup)
            cells.append(f'{med:.1f} [{lo:.1f} .. {hi:.1f}]')
        layers.FUSED_ORIENTED = True
        lines.append(f'| {name} | {cells[0]} | {cells[1]} |')
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
