"""The reference's ring-transfer experiment (exp/run_ring_exp.py over exp/run_exp.py --dataset RING-TRANSFER --model
ring_sparse_cin) on this library: for every ring size 10, 12 .. 30 a fresh 3-layer RingSparseCIN has to carry the one-hot
label from vertex n // 2 of an n-ring to vertex 0 -- three cellular layers do it at every size, because the ring's two-cell
touches every edge.  5000 training and 500 test rings per size, cross-entropy, Adam without a schedule, accuracy.

Both halves on the device, nothing per batch on the host:

    train:     PackedComplexes -> PackedLoader(shuffle=True) -> StaticTrainStep.run_epoch   (captured steps; the prediction is
               ops.target_head on the target rows the collate launch writes into the static slot)
    evaluate:  cwn_amd.evaluate.evaluate(StaticForward, batches, Evaluator('accuracy'), 'classification')

The static batches are built with mode='csr', items=True: the first layer's 5-wide features take the streaming launches,
the 64-wide layers the complex-blocked ones -- what each takes on a collated batch.

    python examples/train_ring_transfer.py [--quick] [--sizes 10 20 30] [--epochs 30] [--seeds 1]     (needs an MI355X)

--model gin_ring runs the other curve of the reference's figure (--model gin_ring of exp/run_exp.py): RingGIN over the vertex
graph of the same rings, with nodes // 2 layers by default -- a GIN layer moves the label one hop, so it needs that many.  It
trains eagerly (PackedLoader batches, autograd over ops.aggregate and the torch modules, torch.optim.Adam) and is evaluated in
inference, where every layer is one cwn_gin_layer_f32 launch (layers.FUSED_GIN).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd import csr                                                   # noqa: E402
from cwn_amd.evaluate import Evaluator, evaluate                          # noqa: E402
from cwn_amd.models import RingGIN, RingSparseCIN                                # noqa: E402
from cwn_amd.packed import PackedComplexes, PackedLoader                  # noqa: E402
from cwn_amd.static_batch import StaticBatch                              # noqa: E402
from cwn_amd.static_graph import StaticForward, StaticTrainStep           # noqa: E402
from cwn_amd.synthetic import ring_transfer                               # noqa: E402

CLASSES = 5


def run(nodes, seed, args, dev):
    pool = ring_transfer(nodes, args.train, CLASSES) + ring_transfer(nodes, args.test, CLASSES)
    packed = PackedComplexes(pool, dev, max_dim=2, with_csr=True)
    torch.manual_seed(seed)
    model = RingSparseCIN(CLASSES, CLASSES, 3 if args.layers is None else args.layers, args.hidden, max_dim=2, nonlinearity='relu', use_coboundaries=True,
                          graph_norm='id').to(dev)
    B, S = args.batch, args.slots
    loader = PackedLoader(packed, batch_size=B, shuffle=True, indices=np.arange(args.train), seed=seed)
    step = StaticTrainStep(model, StaticBatch(packed, B, slots=S, mode='csr', items=True), task_type='classification', lr=args.lr)
    forward = StaticForward(model, StaticBatch(packed, B, slots=S, mode='csr', items=True))
    evaluator = Evaluator('accuracy')
    train_b = [np.arange(lo, min(lo + B, args.train)) for lo in range(0, args.train, B)]
    test_b = [np.arange(lo, min(lo + B, len(pool))) for lo in range(args.train, len(pool), B)]
    t0 = time.perf_counter()
    loss = float('nan')
    for epoch in range(args.epochs):
        model.train()
        loader.set_epoch(epoch)
        losses = step.run_epoch(loader.batches())
        loss = float(torch.stack(losses).mean())
        if args.verbose:
            acc, _ = evaluate(forward, test_b, evaluator, 'classification')
            print(f'  ring {nodes} seed {seed} epoch {epoch}: train loss {loss:.4f}, test accuracy {acc:.3f}')
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    train_acc, _ = evaluate(forward, train_b, evaluator, 'classification')           # (puts the model in eval mode)
    test_acc, test_loss = evaluate(forward, test_b, evaluator, 'classification')
    csr.check_errors(dev)
    return train_acc, test_acc, loss, test_loss, dt, int(step.opt.t)


def run_gin(nodes, seed, args, dev):
    """RingGIN, eagerly: one collate launch, forward, cross-entropy, backward and Adam step per batch."""
    pool = ring_transfer(nodes, args.train, CLASSES) + ring_transfer(nodes, args.test, CLASSES)
    packed = PackedComplexes(pool, dev, max_dim=2, with_csr=True)
    torch.manual_seed(seed)
    layers_ = args.layers if args.layers is not None else nodes // 2
    model = RingGIN(CLASSES, layers_, args.hidden, CLASSES, nonlinearity='relu', graph_norm='bn').to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=args.lr)
    B = args.batch
    loader = PackedLoader(packed, batch_size=B, shuffle=True, indices=np.arange(args.train), seed=seed)

    def accuracy(lo, hi):
        model.eval()
        hits, losses = 0, []
        with torch.no_grad():
            for a in range(lo, hi, B):
                batch = packed.collate(np.arange(a, min(a + B, hi)))
                out, y = model(batch), batch.y.view(-1)
                hits += int((out.argmax(dim=1) == y).sum())
                losses.append(float(torch.nn.functional.cross_entropy(out, y, reduction='sum')))
        return hits / (hi - lo), sum(losses) / (hi - lo)

    t0 = time.perf_counter()
    loss, steps = float('nan'), 0
    for epoch in range(args.epochs):
        model.train()
        loader.set_epoch(epoch)
        losses = []
        for idx in loader.batches():
            batch = packed.collate(idx)
            opt.zero_grad(set_to_none=True)
            l = torch.nn.functional.cross_entropy(model(batch), batch.y.view(-1))
            l.backward()
            opt.step()
            losses.append(l.detach())
            steps += 1
        loss = float(torch.stack(losses).mean())
        if args.verbose:
            print(f'  ring {nodes} seed {seed} epoch {epoch}: train loss {loss:.4f}, test accuracy {accuracy(args.train, len(pool))[0]:.3f}')
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    train_acc, _ = accuracy(0, args.train)
    test_acc, test_loss = accuracy(args.train, len(pool))
    csr.check_errors(dev)
    return train_acc, test_acc, loss, test_loss, dt, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', choices=('ring_sparse_cin', 'gin_ring'), default='ring_sparse_cin')
    ap.add_argument('--quick', action='store_true', help='one ring size, a few epochs on a small dataset')
    ap.add_argument('--sizes', type=int, nargs='*', default=list(range(10, 32, 2)))
    ap.add_argument('--train', type=int, default=5000)
    ap.add_argument('--test', type=int, default=500)
    ap.add_argument('--epochs', type=int, default=30)
    ap.add_argument('--seeds', type=int, default=1)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--slots', type=int, default=4)
    ap.add_argument('--layers', type=int, default=None, help='default: 3 for ring_sparse_cin, nodes // 2 for gin_ring')
    ap.add_argument('--hidden', type=int, default=64)
    ap.add_argument('--lr', type=float, default=1e-3)
    ap.add_argument('--verbose', action='store_true')
    args = ap.parse_args()
    if args.quick:
        args.sizes, args.train, args.test, args.epochs, args.seeds = [10], 500, 100, 3, 1
    dev = torch.device('cuda', 0)
    print('| ring size | seed | train accuracy | test accuracy | last train loss | test loss | steps | training time |')
    print('|---|---|---|---|---|---|---|---|')
    for nodes in args.sizes:
        for seed in range(args.seeds):
            tr, te, loss, test_loss, dt, steps = (run if args.model == 'ring_sparse_cin' else run_gin)(nodes, seed, args, dev)
            print(f'| {nodes} | {seed} | {tr:.3f} | {te:.3f} | {loss:.4f} | {test_loss:.4f} | {steps} | {dt:.2f} s |', flush=True)


if __name__ == '__main__':
    main()
