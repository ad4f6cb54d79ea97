"""The reference's CSL experiment (exp/scripts/cwn-csl.sh) on this library: circulant skip-link graphs C_{41,R}, ten
isomorphism classes that 1-WL cannot tell apart, lifted with rings up to size 8; EmbedSparseCIN with LayerNorm
(--graph_norm ln), width 160, 3 layers, mean readout, edge features, coboundaries, batch 12, Adam at 5e-4 under a
ReduceLROnPlateau on the validation accuracy (patience 20, early stop below 1e-6), cross-entropy over the ten classes.

The update / combine networks of every layer run as grouped GEMM + LayerNorm launches (cwn_amd/dense_ln.py,
csrc/cwn_layernorm.hip; the 320-wide combine product on csrc/cwn_linear_wide.hip), and every training step is a captured
graph replayed per batch (cwn_amd.train.TrainStep): fixed batches, one graph per batch.

--static trains the reference's way instead -- every epoch a fresh shuffle of the training fold (PackedLoader) -- over ONE
captured graph: a packed dataset in HBM, StaticBatch(mode='csr'), StaticTrainStep.run_epoch, validation through
StaticForward.  --folds K runs K of the five folds (the reference: all five, 20 seeds each).

    python examples/train_csl.py [--graphs 150] [--epochs 300] [--patience 20] [--static] [--folds 1]     (needs an MI355X)
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd import csr                                                  # noqa: E402
from cwn_amd.complex import ComplexBatch                                 # noqa: E402
from cwn_amd.models import EmbedSparseCIN                                # noqa: E402
from cwn_amd.synthetic import CSL_SKIPS, csl_graphs                      # noqa: E402
from cwn_amd.train import TrainStep                                      # noqa: E402


def _model(dev):
    torch.manual_seed(0)
    return EmbedSparseCIN(1, 1, len(CSL_SKIPS), 3, 160, dropout_rate=0.0, max_dim=2, jump_mode=None, nonlinearity='relu',
                          readout='mean', final_readout='sum', apply_dropout_before='lin2', init_reduce='sum', embed_edge=True,
                          use_coboundaries=True, graph_norm='ln').to(dev)


def _fold(args, fold: int):
    """(first, one past the last) graph of the fold's validation block: fold 0 holds out the last fifth, fold 1 the one before."""
    G, blk = args.graphs, 4 - fold
    lo = max(args.batch, G * 4 // 5) if blk == 4 else G * blk // 5
    return lo, G * (blk + 1) // 5


def static_fold(args, dev, packed, fold: int) -> int:
    """One fold on shuffled epochs: every step a replay of one captured graph on a batch it has never seen."""
    from cwn_amd.packed import PackedLoader
    from cwn_amd.static_batch import StaticBatch
    from cwn_amd.static_graph import StaticForward, StaticTrainStep
    lo, hi = _fold(args, fold)
    idx = np.arange(args.graphs)
    train_idx, val_idx = np.concatenate([idx[:lo], idx[hi:]]), idx[lo:hi]
    B = args.batch
    model = _model(dev)
    step = StaticTrainStep(model, StaticBatch(packed, B, slots=args.slots, mode='csr'), task_type='classification', lr=args.lr)
    ev = StaticForward(model, StaticBatch(packed, B, slots=1, mode='csr'))
    loader = PackedLoader(packed, batch_size=B, shuffle=True, indices=train_idx, seed=fold)
    val = [val_idx[k:k + B] for k in range(0, len(val_idx), B)]
    val_y = [packed.collate(v).y.view(-1) for v in val]
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(step.opt, mode='max', factor=0.5, patience=args.patience)
    for epoch in range(args.epochs):
        model.train()
        loader.set_epoch(epoch)
        batches = loader.batches()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses = [float(l) for l in step.run_epoch(batches)]
        dt = time.perf_counter() - t0
        if not all(math.isfinite(l) for l in losses):
            raise SystemExit(f'epoch {epoch}: a non-finite loss: {losses}')
        model.eval()
        hit, n = 0, 0
        with torch.no_grad():
            for pred, y in zip(ev.run_epoch(val), val_y):
                hit += int((pred.argmax(1) == y).sum())
                n += y.numel()
        acc = hit / max(n, 1)
        lr = step.opt.param_groups[0]['lr']
        print(f'epoch {epoch}: lr {lr:.3e}, train loss {sum(losses) / len(losses):.4f}, validation accuracy {acc:.3f} '
              f'({len(batches)} steps in {dt * 1e3:.1f} ms)' + (f' [fold {fold}]' if args.folds > 1 else ''))
        scheduler.step(acc)
        if step.opt.param_groups[0]['lr'] < args.lr_min:
            print(f'early stop after epoch {epoch}: lr {step.opt.param_groups[0]["lr"]:.3e} < {args.lr_min:g}')
            break
    return int(step.opt.t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--graphs', type=int, default=150)            # the dataset: 15 relabelled copies of each class
    ap.add_argument('--epochs', type=int, default=300)
    ap.add_argument('--batch', type=int, default=12)
    ap.add_argument('--lr', type=float, default=5e-4)
    ap.add_argument('--patience', type=int, default=20)
    ap.add_argument('--lr-min', type=float, default=1e-6)
    ap.add_argument('--static', action='store_true')              # shuffled epochs over one captured graph
    ap.add_argument('--slots', type=int, default=1)               # --static: steps behind one replay
    ap.add_argument('--folds', type=int, default=1)               # --static: folds to run, 1 .. 5
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    pool = csl_graphs(args.graphs, seed=0, max_ring=8)
    if args.static:
        from cwn_amd.packed import PackedComplexes
        if not 1 <= args.folds <= 5:
            raise SystemExit('--folds: 1 .. 5')
        packed = PackedComplexes(pool, dev, max_dim=2, with_csr=True)
        steps = sum(static_fold(args, dev, packed, fold) for fold in range(args.folds))
        csr.check_errors(dev)
        print(f'done: {steps} optimizer steps')
        return
    if args.folds != 1:
        raise SystemExit('--folds needs --static (fixed batches train the one fold)')
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
