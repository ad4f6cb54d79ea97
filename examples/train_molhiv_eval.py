"""The reference's epoch as exp/run_exp.py runs it for ogbg-molhiv (exp/scripts/cwn-molhiv.sh: --eval_metric ogbg-molhiv,
--task_type bin_classification, ReduceLROnPlateau on the validation metric), both halves on the device:

    train:     PackedLoader(shuffle=True) -> RoutedTrainStep.run_epoch       (captured steps, dropout inside the kernels)
    validate:  cwn_amd.evaluate.evaluate(RoutedForward, batches, Evaluator('ogbg-molhiv'), 'bin_classification')
               -> (ROC-AUC over the held-out split, mean over its batches of BCE-with-logits); the predictions and labels
               never leave the device, the host waits once per pass
    schedule:  ReduceLROnPlateau(mode='max').step(ROC-AUC)                   (the lr reaches the captured Adam launch through
                                                                              FlatAdam's device record)

    python examples/train_molhiv_eval.py [n_molecules] [epochs] [tail]     (needs an MI355X; synthetic molecules, a toy label
    with a fifth of the held-out molecules unlabeled, as ogbg-mol* sets have them)
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd import csr                                                   # noqa: E402
from cwn_amd.evaluate import Evaluator, evaluate                          # noqa: E402
from cwn_amd.models import OGBEmbedSparseCIN                              # noqa: E402
from cwn_amd.packed import PackedComplexes, PackedLoader                  # noqa: E402
from cwn_amd.static_graph import RoutedForward, RoutedTrainStep, StaticRouter   # noqa: E402
from cwn_amd.synthetic import molhiv_like_complexes                       # noqa: E402


def main():
    n_mol = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    tail = float(sys.argv[3]) if len(sys.argv) > 3 else 2e-3
    dev = torch.device('cuda', 0)
    pool = molhiv_like_complexes(n_mol, seed=0, max_ring=6, tail=tail)
    n_train = n_mol * 3 // 4
    for k, c in enumerate(pool):          # a toy label a model can learn: does the molecule have more than two rings?
        c.y = torch.tensor([[float(c.cochains[2].num_cells > 2 if c.dimension >= 2 else 0.0)]])
        if k >= n_train and k % 5 == 0:
            c.y = torch.tensor([[float('nan')]])          # unlabeled: in neither the metric nor the loss
    packed = PackedComplexes(pool, dev, max_dim=2, with_csr=True)
    torch.manual_seed(0)
    model = OGBEmbedSparseCIN(1, 2, 64, dropout_rate=0.5, indropout_rate=0.0, max_dim=2, readout='mean', final_readout='sum',
                              apply_dropout_before='lin2', init_reduce='sum', embed_edge=True, use_coboundaries=True,
                              graph_norm='bn').to(dev)
    B, S = 64, 4
    loader = PackedLoader(packed, batch_size=B, shuffle=True, indices=np.arange(n_train), seed=1)
    step = RoutedTrainStep(model, StaticRouter(packed, B, slots=S), task_type='bin_classification', lr=1e-3)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(step.opt, mode='max', factor=0.5, patience=1)
    model.eval()
    forward = RoutedForward(model, StaticRouter(packed, B, slots=S))
    evaluator = Evaluator('ogbg-molhiv')
    held_out = [np.arange(lo, min(lo + B, n_mol)) for lo in range(n_train, n_mol, B)]
    for epoch in range(epochs):
        model.train()
        loader.set_epoch(epoch)
        batches = loader.batches()
        losses = step.run_epoch(batches)
        train_loss = float(torch.stack(losses).mean())
        t0 = time.perf_counter()
        auc, val_loss = evaluate(forward, held_out, evaluator, 'bin_classification')          # (puts the model in eval mode)
        dt = time.perf_counter() - t0
        print(f'epoch {epoch}: lr {step.opt.param_groups[0]["lr"]:.3e}, train loss {train_loss:.4f}, held-out ROC-AUC {auc:.4f}, '
              f'mean loss {val_loss:.4f} ({sum(len(b) for b in held_out)} molecules evaluated in {dt * 1e3:.1f} ms)')
        scheduler.step(auc)
    csr.check_errors(dev)
    print(f'done: {int(step.opt.t)} optimizer steps')


if __name__ == '__main__':
    main()
