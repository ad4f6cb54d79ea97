"""Time the GIN layer as ONE launch (csrc/cwn_gin.hip; layers.FUSED_GIN) against the route it replaces -- one aggregation
launch and the torch modules of the layer's network -- in ONE process, alternating between the two routes round by round so
that both see the same clocks and the same neighbours on the machine.

Scopes, inference (eval, no autograd), on batches of 32 rings of synthetic.ring_transfer:
  layer (64, 64)               one GINConv.forward at (w, H) = (64, 64), relu, eval-mode BatchNorm, 32 ten-rings (320 rows)
  RingGIN L layers, n-rings    the whole model (hidden 64, relu, BatchNorm) at L = 5 and 16 on rings of 10 and 32 vertices

Per scope and route: kernels per forward (torch.profiler's device-side kernel records of one forward), the median of
--rounds round medians -- a round is --iters forwards between two HIP events, divided by --iters -- and the run-to-run
spread, the 10th .. 90th percentile of the round medians.

    python tools/bench_gin.py [--rounds 15] [--iters 50] [--warmup 20] [--out profiles/gin_layer.md]

Results are printed as a markdown table and appended to --out when given."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd import layers, models                                       # noqa: E402
from cwn_amd.complex import ComplexBatch                                  # noqa: E402
from cwn_amd.synthetic import ring_transfer                               # noqa: E402

DEV = torch.device('cuda', 0)
RINGS = 32


def round_time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def kernels_per_forward(fn) -> int:
    from torch.profiler import profile, ProfilerActivity
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower()
               and 'memset' not in e.name.lower())


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[len(ts) // 10], ts[len(ts) * 9 // 10]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    batches = {n: ComplexBatch.from_complex_list(ring_transfer(n, RINGS * 5)[::5], max_dim=2).to(DEV) for n in (10, 32)}
    assert batches[10].nodes.x.size(0) == RINGS * 10
    x64 = torch.randn(RINGS * 10, 64, device=DEV)
    net = models._gin_network(64, 64, torch.nn.BatchNorm1d, torch.nn.ReLU)
    conv = layers.GINConv(net).to(DEV).eval()
    index = batches[10].nodes.upper_index

    def layer():
        with torch.no_grad():
            conv(x64, index)

    scopes = [('layer (64, 64), 32 ten-rings', layer)]
    for L in (5, 16):
        for n in (10, 32):
            model = models.RingGIN(5, L, 64, 5).to(DEV).eval()

            def forward(model=model, data=batches[n]):
                with torch.no_grad():
                    model(data)
            scopes.append((f'RingGIN {L} layers, 32 {n}-rings', forward))

    lines = [f'{RINGS} rings per batch; {args.rounds} rounds of {args.iters} forwards per route, alternating, after {args.warmup} '
             'warm-up forwards each; median of the round medians [p10 .. p90] in us per forward', '',
             '| scope | kernels fused | kernels torch | fused | torch modules | faster by more than the larger spread |', '|---|---|---|---|---|---|']
    was = layers.FUSED_GIN
    try:
        for name, fn in scopes:
            counts, times = {}, {True: [], False: []}
            for fused in (True, False):
                layers.FUSED_GIN = fused
                for _ in range(args.warmup):
                    fn()
                counts[fused] = kernels_per_forward(fn)
            for _ in range(args.rounds):
                for fused in (True, False):
                    layers.FUSED_GIN = fused
                    times[fused].append(round_time(fn, args.iters))
            (mf, lf, hf), (mt, lt, ht) = stats(times[True]), stats(times[False])
            spread = max(hf - lf, ht - lt)
            lines.append(f'| {name} | {counts[True]} | {counts[False]} | {mf:.1f} [{lf:.1f} .. {hf:.1f}] | {mt:.1f} [{lt:.1f} .. {ht:.1f}] | '
                         f'{"yes" if mt - mf > spread else "no"} ({mt - mf:+.1f} against {spread:.1f}) |')
    finally:
        layers.FUSED_GIN = was
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
