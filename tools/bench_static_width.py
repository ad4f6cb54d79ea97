"""The captured training step over shuffled batches at hidden widths the stage kernels do not hold (48, 16), against the
only route such a model had for batches it has never seen: PackedComplexes.collate(idx) + TrainStep(use_graph=False) per
batch.  Both forms in ONE process, alternating, on the same shuffled epochs:

    EmbedSparseCIN(28, 4, 1, 4 layers, hidden H, BatchNorm), synthetic.zinc_like_complexes, batch 128

    static     StaticBatch(mode='csr', slots S) + StaticTrainStep.run_epoch: one graph replay per S optimisation steps
    per batch  for idx in epoch: collate(idx), plans, forward, loss, backward, Adam as ordinary launches

and, as a check that nothing moved where the stage kernels already served the step, the static step at hidden 128 in mode
'blocked' (compare two builds of the library).

Milliseconds per optimisation step (host clock around whole epochs closed by a device synchronise: interpreter, launches and
kernels), median with the 10th .. 90th percentile over the regions.

    python tools/bench_static_width.py --out profiles/static_any_width.md

Kernels per step are counted in runs of their own under rocprofv3 --kernel-trace (tools/bench_static_width_kernels.sh): the
tracer behind torch.profiler drops events of graph replays.  `--count FORM --hidden H --epochs N` runs N epochs of one form
and nothing else; the script takes the difference of two run lengths, so warm-up and capture cancel.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd import csr                                                       # noqa: E402
from cwn_amd.models import EmbedSparseCIN                                     # noqa: E402
from cwn_amd.packed import PackedComplexes                                    # noqa: E402
from cwn_amd.static_batch import StaticBatch                                  # noqa: E402
from cwn_amd.static_graph import StaticTrainStep                              # noqa: E402
from cwn_amd.synthetic import zinc_like_complexes                             # noqa: E402
from cwn_amd.train import TrainStep                                           # noqa: E402

DEV = torch.device('cuda', 0)
LAYERS, B = 4, 128


def model_of(hidden, seed=0):
    torch.manual_seed(seed)
    return EmbedSparseCIN(28, 4, 1, LAYERS, hidden, dropout_rate=0.0, max_dim=2, embed_edge=True, use_coboundaries=True,
                          graph_norm='bn').to(DEV)


def epochs_of(n, n_epochs, seed=1):
    """Shuffled epochs of whole batches (the reference's loader drops nothing; the pool is a multiple of the batch here)."""
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
        self.ts = TrainStep(model, [packed.collate(first)], lr=1e-3, use_graph=False)

    def run_epoch(self, batches):
        ts = self.ts
        for idx in batches:
            b = self.p.collate(idx)
            ts.batches[0] = b
            ts.inputs[0] = [None if c.x is None else c.x.clone() for c in ts._cochains(b)]
            ts.step(0)


def region_ms(run, epochs, k):
    """Milliseconds per step over one region: epochs k, k + 1, ... until >= 0.25 s of host clock, closed by a synchronise."""
    torch.cuda.synchronize()
    t0, steps = time.perf_counter(), 0
    while True:
        ep = epochs[k % len(epochs)]
        run(ep)
        steps += len(ep)
        k += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= 0.25:
            return dt * 1e3 / steps, k


def stat(v):
    return f'{np.median(v):.3f} [{np.percentile(v, 10):.3f} .. {np.percentile(v, 90):.3f}]'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hidden', type=int, nargs='*', default=[48, 16])
    ap.add_argument('--complexes', type=int, default=2048)
    ap.add_argument('--slots', type=int, default=8)
    ap.add_argument('--regions', type=int, default=9)
    ap.add_argument('--out', default=None)
    ap.add_argument('--count', choices=['static', 'per_batch'], default=None, help='run --epochs epochs of this form at --hidden[0] only')
    ap.add_argument('--epochs', type=int, default=4)
    args = ap.parse_args()
    pool = zinc_like_complexes(args.complexes, seed=0)
    packed = PackedComplexes(pool, DEV, max_dim=2, with_csr=True)
    epochs = epochs_of(len(pool), 6)
    n_steps = len(epochs[0])
    if args.count:
        hidden = args.hidden[0]
        m = model_of(hidden)
        if args.count == 'static':
            sb = StaticBatch(packed, B, slots=args.slots, mode='blocked' if hidden in (64, 128) else 'csr')
            sb.set_epoch(epochs[0])
            run = StaticTrainStep(m, sb, lr=1e-3).run_epoch
        else:
            run = PerBatch(m, packed, epochs[0][0]).run_epoch
        for e in range(args.epochs):
            run(epochs[e % len(epochs)])
        torch.cuda.synchronize()
        print(f'counted: {args.count} hidden {hidden}: {args.epochs * n_steps} steps')
        return
    lines = [f'{torch.cuda.get_device_name(0)}; synthetic.zinc_like_complexes({args.complexes}), batch {B}, {n_steps} steps per shuffled '
             f'epoch, EmbedSparseCIN {LAYERS} layers, BatchNorm, float32; static: StaticBatch(mode=..., slots={args.slots}); median '
             f'[10th .. 90th percentile] of {args.regions} regions of >= 0.25 s per form, forms alternating; ms per optimisation step', '',
             '| hidden | static mode | static step | per-batch step | per batch / static |',
             '|---|---|---|---|---|']
    for hidden in args.hidden:
        m1, m2 = model_of(hidden), model_of(hidden)
        sb = StaticBatch(packed, B, slots=args.slots, mode='csr')
        assert sb.fits(epochs[0]).all()
        sb.set_epoch(epochs[0])
        st = StaticTrainStep(m1, sb, lr=1e-3)
        pb = PerBatch(m2, packed, epochs[0][0])
        forms = {'static': lambda ep: st.run_epoch(ep, keep_losses=False), 'per batch': pb.run_epoch}
        got, k = {name: [] for name in forms}, {name: 0 for name in forms}
        for name, run in forms.items():
            run(epochs[0])                                                   # warm-up: captures, code objects, prepared launches
            run(epochs[1])
        for _ in range(args.regions):
            for name, run in forms.items():
                ms, k[name] = region_ms(run, epochs, k[name])
                got[name].append(ms)
        losses = st.run_epoch(epochs[3])
        assert all(bool(torch.isfinite(l)) for l in losses)
        csr.check_errors(DEV)
        ratio = float(np.median(got['per batch']) / np.median(got['static']))
        lines.append(f"| {hidden} | csr | {stat(got['static'])} | {stat(got['per batch'])} | {ratio:.2f} |")
        print(lines[-1], flush=True)
    # hidden 128, the flagship form: nothing of this route is taken there
    m = model_of(128)
    sb = StaticBatch(packed, B, slots=args.slots)
    sb.set_epoch(epochs[0])
    st = StaticTrainStep(m, sb, lr=1e-3)
    run = lambda ep: st.run_epoch(ep, keep_losses=False)
    run(epochs[0]), run(epochs[1])
    v, k = [], 0
    for _ in range(args.regions):
        ms, k = region_ms(run, epochs, k)
        v.append(ms)
    csr.check_errors(DEV)
    lines.append(f'| 128 | blocked | {stat(v)} | - | - |')
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
