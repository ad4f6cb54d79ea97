"""Time of the float64 aggregation launch (csrc/cwn_aggregate_f64.hip) against two baselines, per shape:

  f64        ops.run_aggregate on float64 operands (cwn_aggregate_f64)
  f32        the same launch on float32 operands (cwn_aggregate_f32: the kernel every other model of the project runs)
  torch f64  what a user has without the float64 kernels: index_select + index_add_ in float64 through torch

Shapes: (a) the SR batch -- 8 ring-lifted rook-sized complexes, F = 16, every adjacency of a SparseCIN layer in ONE launch;
(b) the upper adjacency of the edges of a ZINC-like batch of 128, F = 128; (c) the upper adjacency of the vertices of
REDDIT-like clique complexes (hub rows), F = 64.

Each variant is captured into a graph of LAUNCHES back-to-back launches (so the figure is device time, not Python's enqueue
rate) and replayed between two device events; variants alternate, REPEATS times, and the median per-launch time is reported
with the spread.  Algorithmic bytes = gathered rows + written rows + indices.

    python tools/bench_agg_f64.py [--launches 200] [--repeats 7]        (needs an MI355X)
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd import ops                                                    # noqa: E402
from cwn_amd.complex import ComplexBatch                                   # noqa: E402
from cwn_amd.csr import Adjacency                                          # noqa: E402
from cwn_amd.synthetic import reddit_like_complexes, rook_4x4, shrikhande, sr_lift, zinc_like_batch   # noqa: E402

DEV = torch.device('cuda', 0)


def streams_of(batch, dims_up, dims_b):
    """[(index [2, E], n_dst, n_src)] of the upper / boundary adjacencies of the given dimensions."""
    out = []
    for d in dims_up:
        c = batch.cochains[d]
        out.append((c.upper_index, c.num_cells, c.num_cells))
    for d in dims_b:
        c = batch.cochains[d]
        out.append((c.boundary_index, c.num_cells, batch.cochains[d - 1].num_cells))
    return out


def shapes():
    sr = ComplexBatch.from_complex_list([sr_lift(*(rook_4x4() if k % 2 == 0 else shrikhande()), dtype=torch.float32)
                                         for k in range(8)], max_dim=2).to(DEV)
    zinc = zinc_like_batch(128, seed=0, device=DEV)
    red = ComplexBatch.from_complex_list(reddit_like_complexes(32, seed=1), max_dim=2).to(DEV)
    return [('SR batch (8 complexes), F = 16, 4 adjacencies', streams_of(sr, (0, 1), (1, 2)), 16),
            ('ZINC-128 edge-upper, F = 128', streams_of(zinc, (1,), ()), 128),
            ('REDDIT-like vertex-upper (hubs), F = 64', streams_of(red, (0,), ()), 64)]


def make_variants(adjs, F):
    g = torch.Generator().manual_seed(0)
    plans = [(Adjacency.from_index(idx, n_dst, n_src), idx, n_dst, n_src) for idx, n_dst, n_src in adjs]
    variants = {}
    for name, dtype in (('f64', torch.float64), ('f32', torch.float32)):
        specs = [ops.AggSpec(adj=adj, n_dst=n_dst, F=F, A=torch.randn(n_src, F, generator=g).to(dtype).to(DEV), ia=adj.col,
                             out=torch.empty(n_dst, F, dtype=dtype, device=DEV)) for adj, idx, n_dst, n_src in plans]
        variants[name] = (lambda specs=specs: ops.run_aggregate(specs, DEV))
    xs = [torch.randn(n_src, F, generator=g).double().to(DEV) for _, _, _, n_src in plans]

    def torch_f64():
        return [torch.zeros(n_dst, F, dtype=torch.float64, device=DEV).index_add_(0, idx[1], x.index_select(0, idx[0]))
                for (_, idx, n_dst, _), x in zip(plans, xs)]
    variants['torch f64'] = torch_f64
    nbytes = {name: sum(idx.size(1) * (F * e + 4) + n_dst * (F * e + 4) for _, idx, n_dst, _ in plans)
              for name, e in (('f64', 8), ('f32', 4), ('torch f64', 8))}
    return variants, nbytes, sum(idx.size(1) for _, idx, _, _ in plans)


def capture(fn, launches):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(launches):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    return graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_agg_f64 needs the GPU: nothing is measured without one')
    rows = []
    for label, adjs, F in shapes():
        variants, nbytes, entries = make_variants(adjs, F)
        graphs = {name: capture(fn, args.launches) for name, fn in variants.items()}
        times = {name: [] for name in graphs}
        for _ in range(args.repeats):
            for name, graph in graphs.items():          # alternating: drift hits every variant alike
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                graph.replay()
                t1.record()
                t1.synchronize()
                times[name].append(t0.elapsed_time(t1) * 1e3 / args.launches)
        print(f'{label}: {entries} entries')
        for name, ts in times.items():
            med = statistics.median(ts)
            print(f'  {name:<10} {med:9.2f} us per launch  (min {min(ts):.2f}, max {max(ts):.2f})   '
                  f'{nbytes[name] / med / 1e3:8.1f} GB/s algorithmic')
            rows.append(dict(shape=label, variant=name, us=round(med, 3), us_min=round(min(ts), 3), us_max=round(max(ts), 3),
                             gbps=round(nbytes[name] / med / 1e3, 1)))
    print(json.dumps(dict(tool='bench_agg_f64', launches=args.launches, repeats=args.repeats, rows=rows)))


if __name__ == '__main__':
    main()
