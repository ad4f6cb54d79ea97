"""The strongly-regular-graph isomorphism experiment of the reference (exp/scripts/cwn-sr.sh, exp/run_sr_exp.py,
exp/test_sr.py:81-128) on the two graphs of the family SR(16, 6, 2, 2), which need no data file: the 4 x 4 rook's graph and
the Shrikhande graph.  An UNTRAINED SparseCIN (hidden 16, ELU, no normalisation, sum readouts, coboundary features) embeds
the ring lift (rings up to 6) of each graph and of a vertex-relabelled copy, in float64 -- the experiment sets
torch.set_default_dtype(torch.float64) because sum aggregation reaches 1e8 without a norm layer, and two isomorphic complexes
must land within 0.01 of each other (torch.pdist) while non-isomorphic ones are told apart.

Every gather and segmented reduce of the float64 model is a launch of csrc/cwn_aggregate_f64.hip.  The dense parts are
launches of csrc/cwn_dense_f64.hip: per layer ONE launch for the update and combine networks of all three dimensions, and
two for the head (the lin1s with their activation, lin2); its arithmetic is row-independent, so a complex gets the same
bits whatever else shares its batch.  The ELU(Linear(cat)) message is two per-cell products and one launch of
csrc/cwn_aggregate_act.hip per layer (sum of ELU(Y1[src] + Y2[shared]) in CSR order); CWN_FUSED_ACT_MESSAGE=0 puts it back on
the generic propagate.  CWN_FUSED_F64_DENSE=0 puts every Linear back on torch.nn.Linear (rocBLAS dgemm).

--finetune N adds N Adam steps (torch.optim.Adam, plain autograd) on the 3-layer model with ops.ACT_MESSAGE_BACKWARD on: the
ELU message then runs forward on csrc/cwn_aggregate_act.hip and backward on csrc/cwn_aggregate_act_bwd.hip (one launch per
layer each way) instead of leaving the device path under a recording autograd.  The toy objective pulls the normalised
embeddings of the two graphs to two fixed targets; the loop, not the task, is what it shows.

    python examples/sr_isomorphism.py [seed] [--finetune N]        (needs an MI355X)
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd.complex import ComplexBatch                                   # noqa: E402
from cwn_amd.models import SparseCIN                                       # noqa: E402
from cwn_amd.synthetic import relabel, rook_4x4, shrikhande, sr_lift       # noqa: E402

EPS = 0.01                   # the reference's criterion (exp/test_sr.py:82)


def finetune(model, complexes, dev, steps: int):
    """`steps` Adam steps on `model` with the activated message's backward on the device; prints the loss of every step and
    how many descriptors went through the two activated launches."""
    from cwn_amd import _ffi, layers, ops
    counts = {'aggregate_act': 0, 'aggregate_act_bwd': 0}
    real = {k: getattr(_ffi, k) for k in counts}

    def counting(name):
        def call(descs, device, dtype=torch.float32):
            counts[name] += len(descs)
            return real[name](descs, device, dtype)
        return call
    prev = ops.ACT_MESSAGE_BACKWARD, layers.FUSED_ACT_MESSAGE
    ops.ACT_MESSAGE_BACKWARD, layers.FUSED_ACT_MESSAGE = True, True
    for k in counts:
        setattr(_ffi, k, counting(k))
    try:
        model.train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        target = torch.zeros(len(complexes), 16, device=dev)
        target[:2, 0], target[2:, 1] = 1.0, 1.0                            # rook and its copy; Shrikhande and its copy
        for step in range(steps):
            opt.zero_grad(set_to_none=True)
            emb = model(ComplexBatch.from_complex_list(complexes, max_dim=2).to(dev))
            emb = emb / emb.norm(dim=1, keepdim=True).clamp_min(1e-30)      # (sum aggregation: the raw embeddings reach 1e5)
            loss = torch.nn.functional.mse_loss(emb, target)
            loss.backward()
            opt.step()
            print(f'  finetune step {step}: loss {float(loss.detach()):.6e}')
        print(f'  descriptors through cwn_aggregate_act_f64: {counts["aggregate_act"]}, '
              f'through cwn_aggregate_act_bwd_f64: {counts["aggregate_act_bwd"]}')
    finally:
        for k in counts:
            setattr(_ffi, k, real[k])
        ops.ACT_MESSAGE_BACKWARD, layers.FUSED_ACT_MESSAGE = prev
        model.eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('seed', nargs='?', type=int, default=0)
    ap.add_argument('--finetune', type=int, default=0, metavar='N', help='N Adam steps with ops.ACT_MESSAGE_BACKWARD on')
    args = ap.parse_args()
    seed = args.seed
    dev = torch.device('cuda', 0)
    torch.set_default_dtype(torch.float64)
    rng = np.random.default_rng(43)
    graphs = {'rook 4x4': rook_4x4(), 'Shrikhande': shrikhande()}
    batch, names = [], []
    for name, g in graphs.items():
        batch += [sr_lift(*g, max_k=6), sr_lift(*relabel(*g, rng.permutation(16)), max_k=6)]
        names += [name, name + ' (relabelled)']
    for num_layers in (3, 5):
        torch.manual_seed(seed)
        model = SparseCIN(num_input_features=1, num_classes=16, num_layers=num_layers, hidden=16, dropout_rate=0.0, max_dim=2,
                          use_coboundaries=True, nonlinearity='elu', graph_norm='id', readout='sum', final_readout='sum',
                          readout_dims=(0, 1, 2)).to(dev).eval()
        with torch.no_grad():
            emb = model(ComplexBatch.from_complex_list(batch, max_dim=2).to(dev))
        apex = float(emb.abs().max())
        print(f'{num_layers} layers: embeddings {tuple(emb.shape)} {emb.dtype}, max |embedding| = {apex:.4g} '
              f'({"below" if apex < 5e8 else "NOT below"} 5e8)')
        for i in (0, 2):
            d = float(torch.pdist(emb[i:i + 2], p=2))
            print(f'  {names[i]:<12} vs its relabelled copy: {d:.3e}  ({"isomorphic: within" if d <= EPS else "ABOVE"} {EPS})')
        d = float(torch.pdist(emb[[0, 2]], p=2))
        print(f'  rook 4x4 vs Shrikhande:              {d:.3e}  ({"told apart" if d > EPS else "NOT told apart"})')
        if args.finetune > 0 and num_layers == 3:
            finetune(model, batch, dev, args.finetune)


if __name__ == '__main__':
    main()
