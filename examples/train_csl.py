"""The reference's CSL experiment (exp/scripts/cwn-csl.sh) on this library: circulant skip-link graphs C_{41,R}, ten
isomorphism classes that 1-WL cannot tell apart, lifted with rings up to size 8; EmbedSparseCIN with LayerNorm
(--graph_norm ln), width 160, 3 layers, mean readout, edge features, coboundaries, batch 12, Adam at 5e-4 under a
ReduceLROnPlateau on the validation accuracy (patience 20, early stop below 1e-6), cross-entropy over the ten classes.

The update / combine networks of every layer run as grouped GEMM + LayerNorm launches (cwn_amd/dense_ln.py,
csrc/cwn_layernorm.hip), and every training step is a captured graph replayed per batch (cwn_amd.train.TrainStep).

    python examples/train_csl.py [--graphs 150] [--epochs 300] [--patience 20]       (needs an MI355X)
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
from cwn_amd.models import EmbedSparseCIN                                # noqa: E402
from cwn_amd.synthetic import CSL_SKIPS, csl_graphs                      # noqa: E402
from cwn_amd.train import TrainStep                                      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--graphs', type=int, default=150)            # the dataset: 15 relabelled copies of each class
    ap.add_argument('--epochs', type=int, default=300)
    ap.add_argument('--batch', type=int, default=12)
    ap.add_argument('--lr', type=float, default=5e-4)
    ap.add_argument('--patience', type=int, default=20)
    ap.add_argument('--lr-min', type=float, default=1e-6)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    pool = csl_graphs(args.graphs, seed=0, max_ring=8)
    n_train = max(args.batch, args.graphs * 4 // 5)                # (the reference: 5 folds)
    B = args.batch
    batches = [ComplexBatch.from_complex_list(pool[lo:lo + B], max_dim=2).to(dev) for lo in range(0, n_train, B)]
    val = [ComplexBatch.from_complex_list(pool[lo:lo + B], max_dim=2).to(dev) for lo in range(n_train, args.graphs, B)]
    # (the models write every layer's features into the batch they are given: the validation inputs are put back per pass)
    # (rings carry no features of their own: theirs come from the init reduction)
    val_x = [[None if b.cochains[d].x is None else b.cochains[d].x.clone() for d in range(3)] for b in val]
    torch.manual_seed(0)
    model = EmbedSparseCIN(1, 1, len(CSL_SKIPS), 3, 160, dropout_rate=0.0, max_dim=2, jump_mode=None, nonlinearity='relu',
                           readout='mean', final_readout='sum', apply_dropout_before='lin2', init_reduce='sum', embed_edge=True,
                           use_coboundaries=True, graph_norm='ln').to(dev)
    step = TrainStep(model, batches, task_type='classification', lr=args.lr, use_graph=True)
    # exp/run_exp.py: mode 'max' for a metric that is not minimised (accuracy), factor and patience from the parser
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(step.opt, mode='max', factor=0.5, patience=args.patience)
    for epoch in range(args.epochs):
        model.train()
        t0 = time.perf_counter()
        losses = [float(step.step(i)) for i in range(len(batches))]
        dt = time.perf_counter() - t0
        if not all(math.isfinite(l) for l in losses):
            raise SystemExit(f'epoch {epoch}: a non-finite loss: {losses}')
        model.eval()
        hit, n = 0, 0
        with torch.no_grad():
            for b, xs in zip(val, val_x):
                for d in range(3):
                    b.cochains[d].x = None if xs[d] is None else xs[d].clone()
                y = b.y.view(-1)
                hit += int((model(b).argmax(1) == y).sum())
                n += y.numel()
        acc = hit / max(n, 1)
        lr = step.opt.param_groups[0]['lr']
        print(f'epoch {epoch}: lr {lr:.3e}, train loss {sum(losses) / len(losses):.4f}, validation accuracy {acc:.3f} '
              f'({len(batches)} steps in {dt * 1e3:.1f} ms)')
        scheduler.step(acc)
        if step.opt.param_groups[0]['lr'] < args.lr_min:
            print(f'early stop after epoch {epoch}: lr {step.opt.param_groups[0]["lr"]:.3e} < {args.lr_min:g}')
            break
    csr.check_errors(dev)
    print(f'done: {int(step.opt.t)} optimizer steps')


if __name__ == '__main__':
    main()
