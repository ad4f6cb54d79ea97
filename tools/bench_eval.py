"""Times the evaluation pass over one validation split on one MI355X (profiles/eval_pass.md):

    evaluate   cwn_amd.evaluate.evaluate(StaticForward, batches, Evaluator('mae'), 'regression'): the predictions stay on the
               device, the labels are one gather, the per-batch criterion one launch, the metric two, one wait at the end
    loop       the validation loop of examples/train_zinc_schedule.py:76-84, reproduced here: per batch one ev.run(idx), one
               packed.collate(idx) for its .y and one float(...) that waits for the device

    python tools/bench_eval.py [--graphs 1000] [--batch 128] [--passes 30] [--warmup 5] [--json PATH]
    python tools/bench_eval.py --rank 4113 32901 [--pos 0.035]     the rank kernel alone (one column each; run it under
                                                                   rocprofv3 --kernel-trace --stats for the kernel times)

The two forms alternate inside one process, pass by pass, so that drift of the machine hits both; reported are the median
and the 10th / 90th percentile of the passes (host clock around work that ends in the device wait of the read-out)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd.evaluate import Evaluator, evaluate, rank_counts            # noqa: E402
from cwn_amd.models import EmbedSparseCIN                                # noqa: E402
from cwn_amd.packed import PackedComplexes                               # noqa: E402
from cwn_amd.static_batch import StaticBatch                             # noqa: E402
from cwn_amd.static_graph import StaticForward                           # noqa: E402
from cwn_amd.synthetic import zinc_like_complexes                        # noqa: E402


def stats(ms):
    ms = np.asarray(ms)
    return {'median_ms': float(np.median(ms)), 'p10_ms': float(np.percentile(ms, 10)), 'p90_ms': float(np.percentile(ms, 90)),
            'min_ms': float(ms.min()), 'max_ms': float(ms.max()), 'passes': int(ms.size)}


def rank_only(sizes, pos):
    dev = torch.device('cuda', 0)
    for n in sizes:
        g = torch.Generator().manual_seed(n)
        s = torch.randn(n, 1, generator=g).to(dev)
        y = (torch.rand(n, 1, generator=g) < pos).float().to(dev)
        for _ in range(3):
            rank_counts(s, y)
        torch.cuda.synchronize()
        t = []
        for _ in range(20):
            t0 = time.perf_counter()
            counts, ap_sum, flag = rank_counts(s, y)
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        c = counts.cpu()[0].tolist()
        print(f'rank n {n}: {c[0]} positives, {c[1]} negatives, AUC {(c[2] + 0.5 * c[3]) / (c[0] * c[1]):.4f}; three launches + wait '
              f'{np.median(t):.3f} ms (median of 20, host clock)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--graphs', type=int, default=1000)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--passes', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--json', default=None)
    ap.add_argument('--rank', type=int, nargs='*', default=None)
    ap.add_argument('--pos', type=float, default=0.035)          # ogbg-molhiv's share of positives
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'
    if args.rank is not None:
        return rank_only(args.rank or [4113, 32901], args.pos)
    dev = torch.device('cuda', 0)
    pool = zinc_like_complexes(args.graphs, seed=0, max_ring=6)
    packed = PackedComplexes(pool, dev, max_dim=2, with_csr=True)
    torch.manual_seed(0)
    model = EmbedSparseCIN(28, 4, 1, 4, 128, dropout_rate=0.0, max_dim=2, jump_mode=None, nonlinearity='relu', readout='sum',
                           train_eps=False, final_hidden_multiplier=2, final_readout='sum', init_reduce='sum', embed_edge=True,
                           use_coboundaries=True, graph_norm='bn').to(dev).eval()
    B = args.batch
    val_idx = np.arange(args.graphs)
    batches = [val_idx[lo:lo + B] for lo in range(0, len(val_idx), B)]
    ev_loop = StaticForward(model, StaticBatch(packed, B))                 # as the example builds it: one slot
    ev_new = StaticForward(model, StaticBatch(packed, B, slots=4))
    evaluator = Evaluator('mae')

    def loop():
        err, n = 0.0, 0
        with torch.no_grad():
            for lo in range(0, len(val_idx), B):
                idx = val_idx[lo:lo + B]
                pred = ev_loop.run(idx)[:len(idx)]
                err += float((pred - packed.collate(idx).y.view(pred.shape)).abs().sum())
                n += len(idx)
        return err / n

    def new():
        return evaluate(ev_new, batches, evaluator, 'regression')[0]

    a, b = loop(), new()
    assert abs(a - b) <= 1e-5 * max(1.0, abs(a)), (a, b)
    for _ in range(args.warmup):
        loop()
        new()
    torch.cuda.synchronize()
    t_loop, t_new = [], []
    for _ in range(args.passes):
        for fn, acc in ((loop, t_loop), (new, t_new)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()                                                        # (ends in a read-out: the device has finished)
            acc.append((time.perf_counter() - t0) * 1e3)
    res = {'graphs': args.graphs, 'batch': B, 'batches': len(batches), 'device': torch.cuda.get_device_name(0),
           'validation_mae_loop': a, 'validation_mae_evaluate': b, 'loop': stats(t_loop), 'evaluate': stats(t_new)}
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
