"""The captured training step of the reference's CSL configuration (exp/scripts/cwn-csl.sh: EmbedSparseCIN, LayerNorm, width
160, 3 layers, mean readout, batch 12) on batches it has never seen, against the only route such a batch had before
StaticTrainStep served graph_norm='ln': PackedComplexes.collate(idx) + TrainStep(use_graph=False) per batch.  Both forms in
ONE process, alternating, on the same shuffled epochs:

    static     StaticBatch(mode='csr', slots S) + StaticTrainStep.run_epoch: one graph replay per S optimisation steps
    per batch  for idx in epoch: collate(idx), plans, forward, loss, backward, Adam as ordinary launches

Milliseconds per optimisation step (host clock around whole epochs closed by a device synchronise: interpreter, launches and
kernels), median with the 10th .. 90th percentile over the regions.  Kernels per step: device kernel events of one step of
each form run as ordinary launches under torch.profiler (the captured graph replays the launches of the eager static step).

Next to it, reported and not gated: the eager combine product of a 160-wide layer, ops.linear_wide against
torch.cat + torch.nn.functional.linear (rocBLAS), forward, and forward + backward, at the rows of a batch of 12 CSL graphs.

    python tools/bench_static_ln.py --out profiles/static_ln.md
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd import csr, ops                                                  # noqa: E402
from cwn_amd.models import EmbedSparseCIN                                     # noqa: E402
from cwn_amd.packed import PackedComplexes                                    # noqa: E402
from cwn_amd.static_batch import StaticBatch                                  # noqa: E402
from cwn_amd.static_graph import StaticTrainStep                              # noqa: E402
from cwn_amd.synthetic import CSL_SKIPS, csl_graphs                           # noqa: E402
from cwn_amd.train import TrainStep                                           # noqa: E402

DEV = torch.device('cuda', 0)
B, WIDTH, LAYERS = 12, 160, 3


def model_of(seed=0):
    torch.manual_seed(seed)
    return EmbedSparseCIN(1, 1, len(CSL_SKIPS), LAYERS, WIDTH, dropout_rate=0.0, max_dim=2, jump_mode=None, nonlinearity='relu',
                          readout='mean', final_readout='sum', apply_dropout_before='lin2', init_reduce='sum', embed_edge=True,
                          use_coboundaries=True, graph_norm='ln').to(DEV)


def epochs_of(n, n_epochs, seed=1):
    """Shuffled epochs of whole batches."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_epochs):
        perm = rng.permutation(n)
        out.append([perm[lo:lo + B] for lo in range(0, n - B + 1, B)])
    return out


class PerBatch:
    """The route without a static batch: every batch of the epoch is collated, planned and stepped on eagerly."""

    def __init__(self, model, packed, first):
        self.p = packed
        self.ts = TrainStep(model, [packed.collate(first)], task_type='classification', lr=5e-4, use_graph=False)

    def run_epoch(self, batches):
        ts = self.ts
        for idx in batches:
            b = self.p.collate(idx)
            ts.batches[0] = b
            ts.inputs[0] = [None if c.x is None else c.x.clone() for c in ts._cochains(b)]
            ts.step(0)


def region_ms(run, epochs, k, least=0.25):
    """Milliseconds per step over one region: epochs k, k + 1, ... until >= `least` s of host clock, closed by a synchronise."""
    torch.cuda.synchronize()
    t0, steps = time.perf_counter(), 0
    while True:
        ep = epochs[k % len(epochs)]
        run(ep)
        steps += len(ep)
        k += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= least:
            return dt * 1e3 / steps, k


def stat(v):
    return f'{np.median(v):.3f} [{np.percentile(v, 10):.3f} .. {np.percentile(v, 90):.3f}]'


def kernels_of(fn):
    """Device kernel events of one call of `fn` (ordinary launches), or None where the profiler is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA') and 'memcpy' not in e.name.lower()
                and 'memset' not in e.name.lower())
        return n or None
    except Exception as e:                       # (the figure is a side note of the table: say why it is missing)
        print(f'kernel count unavailable: {type(e).__name__}: {e}', file=sys.stderr)
        return None


def combine_product(rows, regions=9, iters=200):
    """us per call of the eager combine product Linear(320 -> 160) at `rows` rows: ops.linear_wide against cat + linear."""
    g = torch.Generator().manual_seed(0)
    X, X2 = torch.randn(rows, WIDTH, generator=g).to(DEV), torch.randn(rows, WIDTH, generator=g).to(DEV)
    lin = torch.nn.Linear(2 * WIDTH, WIDTH).to(DEV)
    dY = torch.randn(rows, WIDTH, generator=g).to(DEV)

    def wide(train):
        if not train:
            with torch.no_grad():
                return ops.linear_wide(X, X2, lin.weight, lin.bias)
        lin.zero_grad(set_to_none=True)
        ops.linear_wide(X, X2, lin.weight, lin.bias).backward(dY)

    def blas(train):
        if not train:
            with torch.no_grad():
                return torch.nn.functional.linear(torch.cat([X, X2], dim=-1), lin.weight, lin.bias)
        lin.zero_grad(set_to_none=True)
        torch.nn.functional.linear(torch.cat([X, X2], dim=-1), lin.weight, lin.bias).backward(dY)

    res = {}
    for train in (False, True):
        forms = {'linear_wide': wide, 'cat + linear': blas}
        got = {k: [] for k in forms}
        for fn in forms.values():
            for _ in range(20):
                fn(train)
        for _ in range(regions):
            for name, fn in forms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(iters):
                    fn(train)
                torch.cuda.synchronize()
                got[name].append((time.perf_counter() - t0) * 1e6 / iters)
        res[train] = got
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--graphs', type=int, default=150)
    ap.add_argument('--slots', type=int, nargs='*', default=[1, 4])
    ap.add_argument('--regions', type=int, default=9)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    pool = csl_graphs(args.graphs, seed=0, max_ring=8)
    packed = PackedComplexes(pool, DEV, max_dim=2, with_csr=True)
    epochs = epochs_of(len(pool), 6)
    n_steps = len(epochs[0])
    M = int(packed.collate(epochs[0][0]).cochains[1].x.size(0))              # the edges of one batch
    lines = [f'{torch.cuda.get_device_name(0)}; synthetic.csl_graphs({args.graphs}, max_ring=8), batch {B}, {n_steps} steps per shuffled '
             f'epoch, EmbedSparseCIN {LAYERS} layers, width {WIDTH}, LayerNorm, mean readout, cross-entropy, float32; median [10th .. 90th '
             f'percentile] of {args.regions} regions of >= 0.25 s per form, forms alternating in one process; ms per optimisation step', '',
             '| form | step (ms) | per batch / this | kernels per step |', '|---|---|---|---|']
    m_ref = model_of()
    pb = PerBatch(m_ref, packed, epochs[0][0])
    forms = {'per batch (collate + TrainStep(use_graph=False))': pb.run_epoch}
    statics = {}
    for S in args.slots:
        sb = StaticBatch(packed, B, slots=S, mode='csr')
        assert sb.fits(epochs[0]).all()
        sb.set_epoch(epochs[0])
        st = StaticTrainStep(model_of(), sb, task_type='classification', lr=5e-4)
        statics[S] = st
        forms[f"static (mode='csr', slots={S})"] = (lambda ep, st=st: st.run_epoch(ep, keep_losses=False))
    got, k = {name: [] for name in forms}, {name: 0 for name in forms}
    for name, run in forms.items():
        run(epochs[0])                                                       # warm-up: captures, code objects, prepared launches
        run(epochs[1])
    for _ in range(args.regions):
        for name, run in forms.items():
            ms, k[name] = region_ms(run, epochs, k[name])
            got[name].append(ms)
    for st in statics.values():
        assert all(bool(torch.isfinite(l)) for l in st.run_epoch(epochs[3]))
    csr.check_errors(DEV)
    # kernels per step: one step of each form as ordinary launches
    sb1 = StaticBatch(packed, B, slots=1, mode='csr')
    sb1.set_batch(epochs[0][0])
    eager_static = StaticTrainStep(model_of(), sb1, task_type='classification', lr=5e-4, use_graph=False)
    eager_static.step_on([epochs[0][0]]), eager_static.step_on([epochs[0][1]])
    n_static = kernels_of(lambda: eager_static.step_on([epochs[0][2]]))
    n_batch = kernels_of(lambda: pb.run_epoch([epochs[0][2]]))
    base = float(np.median(got['per batch (collate + TrainStep(use_graph=False))']))
    for name in forms:
        n = n_batch if name.startswith('per batch') else n_static
        lines.append(f'| {name} | {stat(got[name])} | {base / float(np.median(got[name])):.2f} | {n if n is not None else "n/a"} |')
        print(lines[-1], flush=True)
    cp = combine_product(M, regions=args.regions)
    lines += ['', f'Eager combine product of one dimension, Linear(320 -> 160) at {M} rows (the edges of a batch of {B} CSL graphs), us per '
              f'call on the host clock, median [10th .. 90th percentile] of {args.regions} regions of 200 calls, forms alternating; reported, not gated', '',
              '| pass | ops.linear_wide | torch.cat + linear (rocBLAS) |', '|---|---|---|']
    for train, label in ((False, 'forward'), (True, 'forward + backward')):
        lines.append(f"| {label} | {stat(cp[train]['linear_wide'])} | {stat(cp[train]['cat + linear'])} |")
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
