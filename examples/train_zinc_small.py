"""exp/scripts/cwn-zinc-small.sh's loop -- the 100k-parameter budget: hidden 48, BatchNorm, Adam, ReduceLROnPlateau on the
validation MAE, early stop on the learning rate -- on captured training steps.  Hidden 48 is no width of the blocked layer
kernels or of the stage kernels, so the static batch is built with mode='csr' (the streaming aggregation over plans rebuilt on
the device per fill) and every update / combine stage runs on cwn_linear_stats_f32, whose BatchNorm statistics count the rows
the batch has:

    packed dataset --PackedLoader(shuffle=True)--> StaticBatch(mode='csr') --StaticTrainStep.run_epoch--> one replay per S steps
    validation: cwn_amd.evaluate.evaluate(StaticForward, batches, Evaluator('mae'), 'regression') -> scheduler.step(mae)

    python examples/train_zinc_small.py [--graphs N] [--epochs E] [--hidden H]     (needs an MI355X; synthetic molecules)
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd import csr                                                  # noqa: E402
from cwn_amd.evaluate import Evaluator, evaluate                         # noqa: E402
from cwn_amd.models import EmbedSparseCIN                                # noqa: E402
from cwn_amd.packed import PackedComplexes, PackedLoader                 # noqa: E402
from cwn_amd.static_batch import StaticBatch                             # noqa: E402
from cwn_amd.static_graph import StaticForward, StaticTrainStep          # noqa: E402
from cwn_amd.synthetic import zinc_like_complexes                        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--graphs', type=int, default=1024)
    ap.add_argument('--epochs', type=int, default=10)             # (cwn-zinc-small.sh: 1000; the early stop ends it first)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--hidden', type=int, default=48)             # --emb_dim 48
    ap.add_argument('--layers', type=int, default=2)              # --num_layers 2
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--patience', type=int, default=2)            # (--lr_scheduler_patience 20)
    ap.add_argument('--lr-min', type=float, default=1e-5)         # --lr_scheduler_min
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    pool = zinc_like_complexes(args.graphs, seed=0, max_ring=6)
    packed = PackedComplexes(pool, dev, max_dim=2, with_csr=True)
    n_train = args.graphs * 7 // 8
    train_idx, val_idx = np.arange(n_train), np.arange(n_train, args.graphs)
    torch.manual_seed(0)
    model = EmbedSparseCIN(28, 4, 1, args.layers, args.hidden, dropout_rate=0.0, max_dim=2, jump_mode=None, nonlinearity='relu',
                           readout='sum', train_eps=False, final_hidden_multiplier=2, final_readout='sum', init_reduce='sum',
                           embed_edge=True, use_coboundaries=True, graph_norm='bn').to(dev)
    print(f'{sum(p.numel() for p in model.parameters())} parameters at hidden {args.hidden}')
    B, S = args.batch, 4
    loader = PackedLoader(packed, batch_size=B, shuffle=True, indices=train_idx, seed=1)
    sb = StaticBatch(packed, B, slots=S, mode='csr')              # (mode 'blocked' serves widths 64 and 128 only, and says so)
    step = StaticTrainStep(model, sb, task_type='regression', lr=args.lr)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(step.opt, mode='min', factor=0.5, patience=args.patience)
    forward = StaticForward(model, StaticBatch(packed, B, mode='csr'))
    held_out = [val_idx[lo:lo + B] for lo in range(0, len(val_idx), B)]
    evaluator = Evaluator('mae')
    for epoch in range(args.epochs):
        model.train()
        loader.set_epoch(epoch)
        batches = loader.batches()
        assert sb.fits(batches).all(), 'a batch beyond the capacities of the static buffers'
        t0 = time.perf_counter()
        losses = step.run_epoch(batches)
        train_loss = float(torch.stack(losses).mean())
        dt = time.perf_counter() - t0
        mae, val_loss = evaluate(forward, held_out, evaluator, 'regression')          # (puts the model in eval mode)
        lr = step.opt.param_groups[0]['lr']
        print(f'epoch {epoch}: lr {lr:.3e}, train L1 {train_loss:.4f}, validation MAE {mae:.4f} (mean loss {val_loss:.4f}; '
              f'{len(batches)} steps in {dt * 1e3:.1f} ms)')
        scheduler.step(mae)
        if step.opt.param_groups[0]['lr'] < args.lr_min:
            print(f'early stop after epoch {epoch}: lr {step.opt.param_groups[0]["lr"]:.3e} < {args.lr_min:g}')
            break
    csr.check_errors(dev)
    print(f'done: {int(step.opt.t)} optimizer steps')


if __name__ == '__main__':
    main()
