"""The reference's experiment loop as exp/scripts/cwn-zinc.sh runs it (exp/run_exp.py:343-408): Adam, a ReduceLROnPlateau on
the validation loss, and an early stop once the learning rate falls below --lr_scheduler_min -- on captured training steps,
with checkpoints and a resume:

    for epoch: StaticTrainStep.run_epoch (one hipGraph replay per S steps; the scheduler's lr reaches the captured Adam
               launch through FlatAdam's device record, no re-capture)
               StaticForward over the validation split -> scheduler.step(val_loss)
               stop when optimizer.param_groups[0]['lr'] < lr_min
               every --ckpt-every epochs: torch.save({step: TrainStep.state_dict(), scheduler, epoch})

    python examples/train_zinc_schedule.py [--graphs N] [--epochs E] [--patience P] [--ckpt PATH] [--ckpt-every K] [--resume]
    (needs an MI355X; synthetic ZINC-like molecules)
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd import csr                                                  # noqa: E402
from cwn_amd.models import EmbedSparseCIN                                # noqa: E402
from cwn_amd.packed import PackedComplexes, PackedLoader                 # noqa: E402
from cwn_amd.static_batch import StaticBatch                             # noqa: E402
from cwn_amd.static_graph import StaticForward, StaticTrainStep          # noqa: E402
from cwn_amd.synthetic import zinc_like_complexes                        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--graphs', type=int, default=1024)
    ap.add_argument('--epochs', type=int, default=20)             # (cwn-zinc.sh: 1000; the early stop ends it first)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--patience', type=int, default=2)            # (cwn-zinc.sh: --lr_scheduler_patience 20)
    ap.add_argument('--lr-min', type=float, default=1e-5)         # --lr_scheduler_min (exp/parser.py:53)
    ap.add_argument('--ckpt', default='zinc_schedule.pt')
    ap.add_argument('--ckpt-every', type=int, default=2)
    ap.add_argument('--resume', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    pool = zinc_like_complexes(args.graphs, seed=0, max_ring=6)
    packed = PackedComplexes(pool, dev, max_dim=2, with_csr=True)
    n_train = args.graphs * 7 // 8
    train_idx, val_idx = np.arange(n_train), np.arange(n_train, args.graphs)
    torch.manual_seed(0)
    model = EmbedSparseCIN(28, 4, 1, 4, 128, dropout_rate=0.0, max_dim=2, jump_mode=None, nonlinearity='relu', readout='sum',
                           train_eps=False, final_hidden_multiplier=2, final_readout='sum', init_reduce='sum', embed_edge=True,
                           use_coboundaries=True, graph_norm='bn').to(dev)
    B, S = args.batch, 4
    loader = PackedLoader(packed, batch_size=B, shuffle=True, indices=train_idx, seed=1)
    sb = StaticBatch(packed, B, slots=S)
    step = StaticTrainStep(model, sb, task_type='regression', lr=args.lr)
    # exp/run_exp.py: optimizer = optim.Adam(model.parameters(), lr=args.lr); scheduler = ReduceLROnPlateau(optimizer, ...)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(step.opt, mode='min', factor=0.5, patience=args.patience)
    ev = StaticForward(model, StaticBatch(packed, B))
    start = 0
    if args.resume and os.path.exists(args.ckpt):
        ck = torch.load(args.ckpt, weights_only=False)
        step.load_state_dict(ck['step'])
        scheduler.load_state_dict(ck['scheduler'])
        start = ck['epoch'] + 1
        print(f'resumed from {args.ckpt} after epoch {ck["epoch"]} (lr {step.opt.param_groups[0]["lr"]:.3e})')
    for epoch in range(start, args.epochs):
        model.train()
        loader.set_epoch(epoch)
        batches = loader.batches()
        assert sb.fits(batches).all(), 'a molecule beyond a workgroup: route its batch through PackedComplexes.collate'
        t0 = time.perf_counter()
        losses = step.run_epoch(batches)
        train_loss = float(torch.stack(losses).mean())
        dt = time.perf_counter() - t0
        # validation: exp/train_utils.py's eval() pass, one captured forward per batch
        model.eval()
        err, n = 0.0, 0
        with torch.no_grad():
            for lo in range(0, len(val_idx), B):
                idx = val_idx[lo:lo + B]
                pred = ev.run(idx)[:len(idx)]
                err += float((pred - packed.collate(idx).y.view(pred.shape)).abs().sum())
                n += len(idx)
        val_loss = err / n
        lr = step.opt.param_groups[0]['lr']
        print(f'epoch {epoch}: lr {lr:.3e}, train L1 {train_loss:.4f}, validation L1 {val_loss:.4f} '
              f'({len(batches)} steps in {dt * 1e3:.1f} ms)')
        scheduler.step(val_loss)
        if (epoch + 1) % args.ckpt_every == 0:
            torch.save({'step': step.state_dict(), 'scheduler': scheduler.state_dict(), 'epoch': epoch}, args.ckpt)
            print(f'checkpoint after epoch {epoch}: {args.ckpt}')
        if step.opt.param_groups[0]['lr'] < args.lr_min:      # exp/run_exp.py: early stop on the learning rate
            print(f'early stop after epoch {epoch}: lr {step.opt.param_groups[0]["lr"]:.3e} < {args.lr_min:g}')
            break
    csr.check_errors(dev)
    print(f'done: {int(step.opt.t)} optimizer steps')


if __name__ == '__main__':
    main()
