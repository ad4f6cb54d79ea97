"""Time the GINE layer as ONE launch (csrc/cwn_gine.hip; layers.FUSED_GINE) against the route it replaces -- one aggregation
launch (the message relu(A + B)) and the torch modules of the layer's network -- in ONE process, alternating between the two
routes round by round so that both see the same clocks and the same neighbours on the machine (tools/bench_gin.py's method).

Scopes, inference (eval, no autograd), on a ZINC-like batch of 128 molecules of synthetic.zinc_like_complexes:
  layer (w, w)                   one GINEConv.forward over the vertex graph at (w, H) = (64, 64) and (128, 128), relu, eval-mode
                                 BatchNorm, the edge features one row per bond read through the shared-coboundary index
  EmbedGIN hidden 128, 4 layers  the whole model: the embedding front, four layers, the readout, the head

Per scope and route: kernels per forward (torch.profiler's device-side kernel records of one forward), the median of
--rounds round medians -- a round is --iters forwards between two HIP events, divided by --iters -- and the run-to-run
spread, the 10th .. 90th percentile of the round medians.

    python tools/bench_gine.py [--rounds 15] [--iters 50] [--warmup 20] [--out profiles/gine_layer.md]

Results are printed as a markdown table and appended to --out when given."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_gin import kernels_per_forward, round_time, stats            # noqa: E402
from cwn_amd import layers, models                                       # noqa: E402
from cwn_amd.cell_mp import IndexedRows                                   # noqa: E402
from cwn_amd.complex import ComplexBatch                                  # noqa: E402
from cwn_amd.synthetic import zinc_like_complexes                         # noqa: E402

DEV = torch.device('cuda', 0)
MOLECULES = 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    batch = ComplexBatch.from_complex_list(zinc_like_complexes(MOLECULES, seed=0), max_dim=1).to(DEV)
    v = batch.cochains[0]
    n0, n1, E = v.x.size(0), batch.cochains[1].x.size(0), v.upper_index.size(1)
    scopes = []
    for w in (64, 128):
        x, e = torch.randn(n0, w, device=DEV), torch.randn(n1, w, device=DEV)
        conv = layers.GINEConv(models._gin_network(w, w, torch.nn.BatchNorm1d, torch.nn.ReLU)).to(DEV).eval()
        attr = IndexedRows(e, v.shared_coboundaries)

        def layer(conv=conv, x=x, attr=attr):
            with torch.no_grad():
                conv(x, v.upper_index, attr)
        scopes.append((f'layer ({w}, {w})', layer))
    model = models.EmbedGIN(28, 4, 1, num_layers=4, hidden=128, embed_edge=True).to(DEV).eval()
    vx, ex = v.x.clone(), batch.cochains[1].x.clone()

    def forward():
        batch.set_xs([vx, ex])                   # (the forward replaces the features by their embeddings)
        with torch.no_grad():
            model(batch)
    scopes.append(('EmbedGIN hidden 128, 4 layers', forward))

    lines = [f'{MOLECULES} molecules per batch ({n0} vertices, {n1} bonds, {E} entries); {args.rounds} rounds of {args.iters} '
             f'forwards per route, alternating, after {args.warmup} warm-up forwards each; median of the round medians '
             '[p10 .. p90] in us per forward', '',
             '| scope | kernels fused | kernels generic | fused | generic | faster by more than the larger spread |',
             '|---|---|---|---|---|---|']
    was = layers.FUSED_GINE
    try:
        for name, fn in scopes:
            counts, times = {}, {True: [], False: []}
            for fused in (True, False):
                layers.FUSED_GINE = fused
                for _ in range(args.warmup):
                    fn()
                counts[fused] = kernels_per_forward(fn)
            for _ in range(args.rounds):
                for fused in (True, False):
                    layers.FUSED_GINE = fused
                    times[fused].append(round_time(fn, args.iters))
            (mf, lf, hf), (mt, lt, ht) = stats(times[True]), stats(times[False])
            spread = max(hf - lf, ht - lt)
            lines.append(f'| {name} | {counts[True]} | {counts[False]} | {mf:.1f} [{lf:.1f} .. {hf:.1f}] | {mt:.1f} [{lt:.1f} .. {ht:.1f}] | '
                         f'{"yes" if mt - mf > spread else "no"} ({mt - mf:+.1f} against {spread:.1f}) |')
    finally:
        layers.FUSED_GINE = was
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
