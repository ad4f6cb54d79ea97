"""The reference's edge-flow experiments (exp/scripts/mpsn-flow.sh, gnn-inv-flow.sh) on this library: synthetic flows on a
triangulated square with two holes -- which hole did the path go around? -- under random edge orientations; EdgeOrient
(orientation-equivariant layers, |.| behind them) or EdgeMPNN (the line-graph baseline), 4 layers, hidden 64, batch 64,
Adam at 1e-3 under StepLR(20, 0.5), cross-entropy, accuracy through evaluate.Evaluator('accuracy').

Every layer is ONE launch (ops.oriented_layer, csrc/cwn_oriented.hip) forward and at most two plus the weight-gradient GEMM
backward.  The default loop is plain autograd with torch.optim.Adam over CochainBatch inputs.

--packed keeps the cochains in HBM (packed.PackedCochains): every batch is one collate launch that also brings the layers'
CSR plans (no host collate, no per-batch sort), the head runs as ops.flow_head (models.FUSED_FLOW_HEAD is turned on), and the
test pass goes through evaluate.evaluate with the labels gathered by `labels(idx)`.

--static goes one step further: the whole optimisation step (moving to the next batch, collate, forward, cross-entropy,
backward, FlatAdam) is captured once in a hipGraph over a static_cochains.StaticCochainBatch and replayed for every batch of
every shuffled epoch (static_graph.StaticCochainTrainStep; an epoch's segment tables go up in one copy); StepLR drives the
step's param group, and the test pass runs through static_graph.StaticCochainForward and evaluate.evaluate.

    python examples/train_flow.py [--packed | --static] [--model edge_orient|edge_mpnn] [--nonlinearity id|tanh|relu] [--epochs 40]   (needs an MI355X)
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd import csr, evaluate, models                                # noqa: E402
from cwn_amd.complex import CochainBatch                                 # noqa: E402
from cwn_amd.evaluate import Evaluator                                   # noqa: E402
from cwn_amd.models import EdgeMPNN, EdgeOrient                          # noqa: E402
from cwn_amd.packed import CochainForward, PackedCochains                # noqa: E402
from cwn_amd.synthetic import edge_flows                                 # noqa: E402


def batches_of(cochains, B, dev, gen=None):
    order = torch.randperm(len(cochains), generator=gen).tolist() if gen is not None else list(range(len(cochains)))
    return [CochainBatch.from_cochain_list([cochains[i] for i in order[lo:lo + B]]).to(dev) for lo in range(0, len(order), B)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', choices=('edge_orient', 'edge_mpnn'), default='edge_orient')
    ap.add_argument('--nonlinearity', choices=('id', 'tanh', 'relu', 'elu', 'sigmoid'), default='id')
    ap.add_argument('--train', type=int, default=1000)
    ap.add_argument('--test', type=int, default=200)
    ap.add_argument('--side', type=int, default=32)              # ~1000 points, as the reference's num_points
    ap.add_argument('--epochs', type=int, default=40)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--layers', type=int, default=4)
    ap.add_argument('--hidden', type=int, default=64)
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--packed', action='store_true', help='device-resident dataset, one-launch collate with plans, fused head')
    ap.add_argument('--static', action='store_true', help='the packed dataset through a captured training step and a captured forward')
    ap.add_argument('--slots', type=int, default=8, help='--static: steps per replayed graph')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    train, test = edge_flows(args.train, args.side, seed=0), edge_flows(args.test, args.side, seed=1)
    torch.manual_seed(0)
    if args.model == 'edge_orient':
        model = EdgeOrient(1, 2, args.layers, args.hidden, nonlinearity=args.nonlinearity, readout='sum', fully_invar=False)
    else:
        model = EdgeMPNN(1, 2, args.layers, args.hidden, nonlinearity=args.nonlinearity, readout='sum', fully_invar=True)
    model = model.to(dev)
    if args.static:
        return train_static(args, model, Evaluator('accuracy'), train, test, dev)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=20, gamma=0.5)
    evaluator = Evaluator('accuracy')
    if args.packed:
        return train_packed(args, model, opt, sched, evaluator, train, test, dev)
    test_batches = batches_of(test, args.batch, dev)
    test_x = [b.x.clone() for b in test_batches]                 # (the models write every layer's features into their batch)
    gen = torch.Generator().manual_seed(0)
    for epoch in range(args.epochs):
        model.train()
        t0 = time.perf_counter()
        losses = []
        for b in batches_of(train, args.batch, dev, gen):        # a new shuffled split every epoch, as the reference's loader
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.cross_entropy(model(b), b.y.view(-1))
            loss.backward()
            opt.step()
            losses.append(loss.detach())
        losses = [float(l) for l in losses]
        dt = time.perf_counter() - t0
        if not all(math.isfinite(l) for l in losses):
            raise SystemExit(f'epoch {epoch}: a non-finite loss')
        sched.step()
        model.eval()
        preds, ys = [], []
        with torch.no_grad():
            for b, x in zip(test_batches, test_x):
                b.x = x.clone()
                preds.append(model(b))
                ys.append(b.y.view(-1))
        acc = evaluator.eval({'y_pred': torch.cat(preds), 'y_true': torch.cat(ys)})
        print(f'epoch {epoch}: lr {opt.param_groups[0]["lr"]:.3e}, train loss {sum(losses) / len(losses):.4f}, test accuracy {acc:.3f} '
              f'({len(losses)} steps in {dt * 1e3:.1f} ms)')
    csr.check_errors(dev)


def train_packed(args, model, opt, sched, evaluator, train, test, dev):
    """The same experiment over packed.PackedCochains: shuffled batches by one collate launch each, the fused head."""
    models.FUSED_FLOW_HEAD = True
    packed_train, packed_test = PackedCochains(train, dev), PackedCochains(test, dev)
    test_forward, test_idx = CochainForward(model, packed_test), packed_test.batch_indices(args.batch)
    for epoch in range(args.epochs):
        model.train()
        t0 = time.perf_counter()
        losses = []
        for b in packed_train.batches(args.batch, shuffle=True, seed=0):       # a new permutation every epoch
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.cross_entropy(model(b), b.y.view(-1))
            loss.backward()
            opt.step()
            losses.append(loss.detach())
        losses = [float(l) for l in losses]
        dt = time.perf_counter() - t0
        if not all(math.isfinite(l) for l in losses):
            raise SystemExit(f'epoch {epoch}: a non-finite loss')
        sched.step()
        acc, test_loss = evaluate.evaluate(test_forward, test_idx, evaluator, 'classification')
        print(f'epoch {epoch}: lr {opt.param_groups[0]["lr"]:.3e}, train loss {sum(losses) / len(losses):.4f}, test accuracy {acc:.3f}, '
              f'test loss {test_loss:.4f} ({len(losses)} steps in {dt * 1e3:.1f} ms, head route {model.last_head_route})')
    csr.check_errors(dev)


def train_static(args, model, evaluator, train, test, dev):
    """The same experiment with every step and every test forward replayed from a captured graph."""
    from cwn_amd.static_cochains import StaticCochainBatch
    from cwn_amd.static_graph import StaticCochainForward, StaticCochainTrainStep
    packed_train, packed_test = PackedCochains(train, dev), PackedCochains(test, dev)
    step = StaticCochainTrainStep(model, StaticCochainBatch(packed_train, args.batch, slots=args.slots), 'classification', lr=args.lr)
    sched = torch.optim.lr_scheduler.StepLR(step.opt, step_size=20, gamma=0.5)
    test_forward = StaticCochainForward(model, StaticCochainBatch(packed_test, args.batch, slots=args.slots))
    test_idx = packed_test.batch_indices(args.batch)
    for epoch in range(args.epochs):
        model.train()
        t0 = time.perf_counter()
        losses = step.run_epoch(packed_train.batch_indices(args.batch, shuffle=True, seed=0, epoch=epoch))
        losses = [float(l) for l in losses]
        dt = time.perf_counter() - t0
        if not all(math.isfinite(l) for l in losses):
            raise SystemExit(f'epoch {epoch}: a non-finite loss')
        sched.step()
        acc, test_loss = evaluate.evaluate(test_forward, test_idx, evaluator, 'classification')
        print(f'epoch {epoch}: lr {step.opt.param_groups[0]["lr"]:.3e}, train loss {sum(losses) / len(losses):.4f}, test accuracy {acc:.3f}, '
              f'test loss {test_loss:.4f} ({len(losses)} steps in {dt * 1e3:.1f} ms, head route {model.last_head_route})')
    csr.check_errors(dev)


if __name__ == '__main__':
    main()
