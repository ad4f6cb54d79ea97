"""Time the graph baselines over batches never seen before, three forms in ONE process, alternating round by round so that
all see the same clocks and the same neighbours on the machine (tools/bench_gine.py's method):

  (a) counted   StaticBatch(mode='csr') + StaticForward with layers.FUSED_GIN_STATIC on: one captured graph, every GINConv /
                GINEConv ONE counted launch (cwn_gin_layer_dev_f32 / cwn_gine_layer_dev_f32)
  (b) generic   the same with layers.FUSED_GIN_STATIC off: one captured graph, every layer an aggregation launch and the torch
                modules of its network
  (c) collated  PackedComplexes.collate(idx) + model(batch) as ordinary launches per batch (the one-launch layers with host
                row counts: layers.FUSED_GIN / FUSED_GINE)

Scopes, inference (eval, no autograd):
  EmbedGIN hidden 128, 4 layers   128 ZINC-like molecules per batch (synthetic.zinc_like_complexes), 8 batches per epoch
  RingGIN 16 layers, hidden 64    32 rings of 32 vertices per batch (synthetic.ring_transfer), 10 batches per epoch

A round is --epochs epochs, each over a fresh permutation of the dataset, between two HIP events -- set_epoch and the replays
for (a) and (b), collate and forward per batch for (c) -- divided by its number of batches.  Per scope and form: kernels per batch
(torch.profiler's device-side kernel records of the same launches issued eagerly, the fill's included for (a) and (b)), the
median of --rounds rounds and the run-to-run spread, the 10th .. 90th percentile of the rounds.  The verdict for
layers.FUSED_GIN_STATIC_DEFAULT is (a) against (b): on only if (a) is faster by more than the larger spread of the two.

    python tools/bench_gin_static.py [--rounds 15] [--epochs 10] [--warmup 3] [--slots 4] [--out profiles/gin_static.md]

Results are printed as a markdown table and appended to --out when given."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_gin import stats                                               # noqa: E402
from cwn_amd import layers, models                                        # noqa: E402
from cwn_amd.packed import PackedComplexes                                # noqa: E402
from cwn_amd.static_batch import StaticBatch                              # noqa: E402
from cwn_amd.static_graph import StaticForward                            # noqa: E402
from cwn_amd.synthetic import ring_transfer, zinc_like_complexes          # noqa: E402

DEV = torch.device('cuda', 0)


def kernels(fn) -> int:
    from torch.profiler import profile, ProfilerActivity
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower()
               and 'memset' not in e.name.lower())


def round_time(fn, epochs) -> float:
    """us per batch of one round: `epochs` epochs, back to back between two events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for batches in epochs:
        fn(batches)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / sum(len(batches) for batches in epochs)


def scope(name, model, complexes, B, max_dim, slots, args):
    packed = PackedComplexes(complexes, DEV, max_dim=max_dim, with_csr=True)
    n_batches = len(complexes) // B
    rng = np.random.default_rng(1)

    def epoch():
        perm = rng.permutation(len(complexes))
        return [perm[k * B:(k + 1) * B] for k in range(n_batches)]

    forms, static = {}, {}
    for form, on in (('counted', True), ('generic', False)):
        layers.FUSED_GIN_STATIC = on
        sb = StaticBatch(packed, B, slots=slots, mode='csr')
        sf = StaticForward(model, sb)
        first = epoch()
        assert sb.fits(first).all()
        sf.run_epoch(first)                       # (captures the graph under this setting of the switch)
        route = 'fused_counted' if on else 'generic'
        assert all(m.last_route == route for m in model.modules() if isinstance(m, (layers.GINConv, layers.GINEConv))), form
        static[form] = (sb, sf)
        forms[form] = lambda batches, sf=sf: sf.run_epoch(batches)

    def collated(batches):
        with torch.no_grad():
            for idx in batches:
                model(packed.collate(idx))
    forms['collated'] = collated

    counts = {}
    for form, (sb, sf) in static.items():
        layers.FUSED_GIN_STATIC = form == 'counted'
        sb.set_epoch(epoch())
        sf.eager()
        sb.set_epoch(epoch())
        counts[form] = kernels(sf.eager) / slots
    one = epoch()[:1]
    collated(one)
    counts['collated'] = float(kernels(lambda: collated(one)))
    times = {form: [] for form in forms}
    for form, fn in forms.items():
        for _ in range(args.warmup):
            fn(epoch())
    for _ in range(args.rounds):
        for form, fn in forms.items():
            times[form].append(round_time(fn, [epoch() for _ in range(args.epochs)]))
    (ma, la, ha), (mb, lb, hb), (mc, lc, hc) = (stats(times[f]) for f in ('counted', 'generic', 'collated'))
    spread = max(ha - la, hb - lb)
    line = (f'| {name} | {counts["counted"]:.1f} | {counts["generic"]:.1f} | {counts["collated"]:.0f} | {ma:.1f} [{la:.1f} .. {ha:.1f}] | '
            f'{mb:.1f} [{lb:.1f} .. {hb:.1f}] | {mc:.1f} [{lc:.1f} .. {hc:.1f}] | '
            f'{"yes" if mb - ma > spread else "no"} ({mb - ma:+.1f} against {spread:.1f}) |')
    return line, mb - ma > spread


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--epochs', type=int, default=10)
    ap.add_argument('--slots', type=int, default=4)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    was = layers.FUSED_GIN, layers.FUSED_GINE, layers.FUSED_GIN_STATIC
    layers.FUSED_GIN = layers.FUSED_GINE = True
    lines = [f'{args.rounds} rounds per form, alternating, after {args.warmup} warm-up epochs each; a round is {args.epochs} epochs, each over a fresh '
             f'permutation; {args.slots} slots per replay; median of the rounds [p10 .. p90] in us per batch', '',
             '| scope | kernels (a) | kernels (b) | kernels (c) | (a) counted | (b) generic | (c) collated | (a) faster than (b) by more '
             'than the larger spread |', '|---|---|---|---|---|---|---|---|']
    verdicts = []
    try:
        model = models.EmbedGIN(28, 4, 1, num_layers=4, hidden=128, embed_edge=True).to(DEV).eval()
        line, won = scope('EmbedGIN hidden 128, 4 layers, 128 molecules', model, zinc_like_complexes(8 * 128, seed=0), 128, 1,
                          args.slots, args)
        lines.append(line)
        verdicts.append(won)
        rings = ring_transfer(32, 320)
        model = models.RingGIN(5, 16, 64, 5).to(DEV).eval()
        line, won = scope('RingGIN 16 layers, hidden 64, 32 rings of 32', model, rings, 32, 2, args.slots, args)
        lines.append(line)
        verdicts.append(won)
    finally:
        layers.FUSED_GIN, layers.FUSED_GINE, layers.FUSED_GIN_STATIC = was
    lines += ['', f'Verdict: layers.FUSED_GIN_STATIC_DEFAULT = {all(verdicts)} by the rule (on only where (a) is faster than (b) by more '
              'than the larger p10 .. p90 spread of the two, in every scope).']
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
