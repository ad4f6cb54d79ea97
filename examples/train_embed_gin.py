"""The graph baseline of the reference's molecular experiments (exp/run_exp.py --model embed_gin over ZINC) on this library:
models.EmbedGIN -- the embedding front over atoms and bonds, GINEConv layers over the vertex graph whose edge features are
the bonds' rows, the readout over the vertices -- on synthetic ZINC-like molecules, Adam at 1e-3, L1 loss as the reference's
ZINC regression, mean absolute error on a held-out split.

The loop is plain autograd with torch.optim.Adam over collated ComplexBatch inputs: EmbedGIN's one-launch layer
(cwn_gine_layer_f32, layers.FUSED_GINE) takes host row counts, so the static batches of the other molecular examples do not
apply to its training (StaticTrainStep refuses the GIN family: its BatchNorm would take statistics over a slot's capacity rows).
Training runs every layer through the differentiable route (one aggregation launch with the message relu(A + B)
forward, its transposed launches backward, the torch modules of the network); the evaluation pass runs one launch per layer.
With --static-eval the validation pass is device-resident instead: the held-out molecules packed once, a
StaticBatch(mode='csr') + StaticForward replaying ONE captured graph per group of slots, evaluate.evaluate for the metric --
every layer the counted launch where layers.FUSED_GIN_STATIC (CWN_FUSED_GIN_STATIC=1) is on, the generic route otherwise.
The synthetic targets are random, so the curve shows the loop, not a chemistry result.

    python examples/train_embed_gin.py [--graphs N] [--epochs E] [--layers 4] [--hidden 128] [--static-eval]   (needs an MI355X)
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd import csr                                                  # noqa: E402
from cwn_amd.complex import ComplexBatch                                 # noqa: E402
from cwn_amd.models import EmbedGIN                                      # noqa: E402
from cwn_amd.synthetic import zinc_like_complexes                        # noqa: E402


def batches_of(pool, B, dev, gen=None):
    """Collated batches up to dimension 1.  A forward replaces a batch's features by their embeddings, so every pass collates
    anew, as the reference's loader does (the collate copies: the pool keeps its integer features)."""
    order = torch.randperm(len(pool), generator=gen).tolist() if gen is not None else list(range(len(pool)))
    return [ComplexBatch.from_complex_list([pool[i] for i in order[lo:lo + B]], max_dim=1).to(dev)
            for lo in range(0, len(order), B)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--graphs', type=int, default=1024)
    ap.add_argument('--epochs', type=int, default=10)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--layers', type=int, default=4)
    ap.add_argument('--hidden', type=int, default=128)
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--static-eval', action='store_true', help='validate through StaticForward + evaluate.evaluate')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    pool = zinc_like_complexes(args.graphs, seed=0, max_ring=6)
    n_train = args.graphs * 7 // 8
    train, val = pool[:n_train], pool[n_train:]
    torch.manual_seed(0)
    model = EmbedGIN(28, 4, 1, args.layers, args.hidden, dropout_rate=0.0, nonlinearity='relu', readout='sum', train_eps=False,
                     init_reduce='sum', embed_edge=True).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    gen = torch.Generator().manual_seed(0)
    static = None
    if args.static_eval:
        import numpy as np
        from cwn_amd.evaluate import Evaluator, evaluate
        from cwn_amd.packed import PackedComplexes
        from cwn_amd.static_batch import StaticBatch
        from cwn_amd.static_graph import StaticForward
        packed = PackedComplexes(val, dev, max_dim=1, with_csr=True)
        val_batches = [np.arange(lo, min(lo + args.batch, len(val))) for lo in range(0, len(val), args.batch)]
        forward = StaticForward(model, StaticBatch(packed, args.batch, slots=min(4, len(val_batches)), mode='csr'))
        static = (forward, val_batches, Evaluator('mae'))
    for epoch in range(args.epochs):
        model.train()
        t0 = time.perf_counter()
        losses = []
        for b in batches_of(train, args.batch, dev, gen):
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.l1_loss(model(b).view(-1), b.y.view(-1))
            loss.backward()
            opt.step()
            losses.append(loss.detach())
        losses = [float(l) for l in losses]
        dt = time.perf_counter() - t0
        if not all(math.isfinite(l) for l in losses):
            raise SystemExit(f'epoch {epoch}: a non-finite loss')
        model.eval()
        if static is not None:
            mae, _ = evaluate(static[0], static[1], static[2], 'regression')
        else:
            err, count = 0.0, 0
            with torch.no_grad():
                for b in batches_of(val, args.batch, dev):
                    err += float((model(b).view(-1) - b.y.view(-1)).abs().sum())
                    count += b.y.numel()
            mae = err / count
        routes = {c.last_route for c in model.convs}
        print(f'epoch {epoch}: train loss {sum(losses) / len(losses):.4f}, validation MAE {mae:.4f} '
              f'({len(losses)} steps in {dt * 1e3:.1f} ms; evaluation layers: {", ".join(sorted(routes))})')
    csr.check_errors(dev)


if __name__ == '__main__':
    main()
