"""Time the device-resident data path of the edge-flow experiments (packed.PackedCochains, ops.flow_head) against the route it
replaces, in ONE process, alternating between the two forms round by round so that both see the same clocks and the same
neighbours on the machine.  Setting: synthetic.edge_flows at the reference's size (side 32: ~3 000 edges and tens of
thousands of adjacency entries per cochain), batch 64, EdgeOrient hidden 64 x 4 layers.

  batch construction   one never-seen batch on the device, ready for a training step: CochainBatch.from_cochain_list + .to(device)
                       + the four CSR builds (upper, lower, their transposes) against PackedCochains.collate.  Host clock
                       around work that ends in a synchronise; every batch is a fresh random draw of 64 cochains.
  head                 |x| -> readout -> lin1 -> ReLU -> lin2 on a [N, 64] matrix of one batch, forward (no autograd) and
                       forward + backward: the generic route (torch.abs, global_pool, the Linear modules; its CSR over the
                       batch vector is cached, i.e. NOT counted) against ops.flow_head.  HIP events; kernels per call from
                       torch.profiler.
  optimisation step    examples/train_flow.py's loop without and with --packed: wall time per step over epochs of shuffled
                       batches (collate, forward, loss, backward, Adam), the epochs of the two forms alternating.

  optimisation step,   the --packed loop (one collate, ~120 launches issued from Python, torch.optim.Adam per step) against the
  static               captured step of --static (static_graph.StaticCochainTrainStep over a static_cochains.StaticCochainBatch:
                       advance, collate, forward, cross-entropy, backward and FlatAdam replayed from one hipGraph, an epoch's
                       tables uploaded once), the epochs of the two forms alternating, every epoch a new permutation: never-seen
                       batches.  Kernels per step from torch.profiler over one epoch of each form.

Per scope and form: the median of the round values and the run-to-run spread, their 10th .. 90th percentile.

    python tools/bench_flow.py [--train 512] [--rounds 21] [--out profiles/flow_packed.md]
    python tools/bench_flow.py --static-only [--slots 8] [--out profiles/flow_static.md]      the last scope alone

Results are printed as a markdown table and appended to --out when given."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd import csr, models                                          # noqa: E402
from cwn_amd.complex import CochainBatch                                  # noqa: E402
from cwn_amd.packed import PackedCochains                                 # noqa: E402
from cwn_amd.synthetic import edge_flows                                  # noqa: E402

DEV = torch.device('cuda', 0)


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[len(ts) // 10], ts[len(ts) * 9 // 10]


def cell(ts, unit='', digits=1):
    m, lo, hi = stats(ts)
    return f'{m:.{digits}f} [{lo:.{digits}f} .. {hi:.{digits}f}]{unit}', m, hi - lo


def verdict(old, new, digits=1):
    (_, mo, so), (_, mn, sn) = cell(old), cell(new)
    spread = max(so, sn)
    return f'{"yes" if mo - mn > spread else "no"} ({mo - mn:+.{digits}f} against {spread:.{digits}f}; x{mo / mn:.2f})'


def kernels_per_call(fn) -> int:
    from torch.profiler import profile, ProfilerActivity
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'memcpy' not in e.name.lower()
               and 'memset' not in e.name.lower())


def event_time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def host_batch(cochains, idx, parts=None):
    """The parent route to a batch a training step can run on: host collate, upload, the plans and their transposes.
    `parts`: a list that receives (host collate, upload, plan builds) in ms -- two more synchronisations."""
    t0 = time.perf_counter()
    b = CochainBatch.from_cochain_list([cochains[i] for i in idx])
    t1 = time.perf_counter()
    b = b.to(DEV)
    if parts is not None:
        torch.cuda.synchronize()
    t2 = time.perf_counter()
    n = b.num_cells
    adjs = [csr.cached_adjacency(b.upper_index, n, n, build=False), csr.cached_adjacency(b.lower_index, n, n, build=False)]
    for a in adjs:
        a.transposes()
    csr.build_many(adjs + [a._t_src for a in adjs])
    if parts is not None:
        torch.cuda.synchronize()
        parts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (time.perf_counter() - t2) * 1e3))
    return b


def static_scope(args, pc, lines):
    """'optimisation step, static': the --packed loop against the captured step, alternating epoch by epoch."""
    from cwn_amd.static_cochains import StaticCochainBatch
    from cwn_amd.static_graph import StaticCochainTrainStep
    B = args.batch
    was = models.FUSED_FLOW_HEAD
    models.FUSED_FLOW_HEAD = True
    try:
        torch.manual_seed(0)
        m_packed = models.EdgeOrient(1, 2, args.layers, args.hidden, nonlinearity='id').to(DEV).train()
        opt = torch.optim.Adam(m_packed.parameters(), lr=1e-3)
        torch.manual_seed(0)
        m_static = models.EdgeOrient(1, 2, args.layers, args.hidden, nonlinearity='id').to(DEV)
        sb = StaticCochainBatch(pc, B, slots=args.slots)
        step = StaticCochainTrainStep(m_static, sb, 'classification', lr=1e-3)
        epoch = [0]

        def run(form):
            batches = pc.batch_indices(B, shuffle=True, seed=0, epoch=epoch[0])       # a permutation neither form has seen
            epoch[0] += 1
            if form == 'static':
                step.run_epoch(batches, keep_losses=False)
                return len(batches)
            for idx in batches:
                b = pc.collate(idx)
                opt.zero_grad(set_to_none=True)
                loss = torch.nn.functional.cross_entropy(m_packed(b), b.y.view(-1))
                loss.backward()
                opt.step()
            return len(batches)
        times, counts = {'packed': [], 'static': []}, {}
        for r in range(args.rounds + 2):
            for form in ('packed', 'static'):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                steps = run(form)
                torch.cuda.synchronize()
                if r >= 2:                                   # (two warm-up epochs per form: the captures)
                    times[form].append((time.perf_counter() - t0) * 1e3 / steps)
        counts['packed'] = kernels_per_call(lambda: run('packed')) / steps
        # (the profiler does not list the kernels of a graph replay: the SAME launches issued one by one -- what the capture recorded)
        counts['static'] = kernels_per_call(lambda: step._eager(0))
        assert m_packed.last_head_route == 'fused' and m_static.last_head_route == 'counted'
        lines.append(f'| optimisation step, static, ms (epochs of {steps} never-seen shuffled batches, {args.slots} steps per replay; '
                     f'{counts["packed"]:.0f} against {counts["static"]:.0f} kernels per step) | {cell(times["packed"], digits=2)[0]} (--packed) | '
                     f'{cell(times["static"], digits=2)[0]} (--static) | {verdict(times["packed"], times["static"], 2)} |')
    finally:
        models.FUSED_FLOW_HEAD = was


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--train', type=int, default=512)
    ap.add_argument('--side', type=int, default=32)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--hidden', type=int, default=64)
    ap.add_argument('--layers', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=21)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--slots', type=int, default=8, help='steps per replay of the static form')
    ap.add_argument('--static-only', action='store_true', help="the scope 'optimisation step, static' alone")
    args = ap.parse_args()
    B = args.batch
    cochains = edge_flows(args.train, args.side, seed=0)
    t0 = time.perf_counter()
    pc = PackedCochains(cochains, DEV)
    torch.cuda.synchronize()
    t_pack = time.perf_counter() - t0
    rng = np.random.default_rng(0)
    entries = int(cochains[0].upper_index.size(1) + cochains[0].lower_index.size(1))
    lines = [f'edge_flows({args.train}, side={args.side}): {cochains[0].num_cells} edges and {entries} adjacency entries per cochain; batch {B}; '
             f'EdgeOrient hidden {args.hidden} x {args.layers} layers; {args.rounds} rounds per form ({3 * args.rounds} for the batch construction), alternating; '
             f'median [p10 .. p90]; '
             f'packing the dataset once (upload + the CSRs of every cochain): {t_pack * 1e3:.0f} ms', '',
             '| scope | parent route | packed / fused | faster by more than the larger spread |', '|---|---|---|---|']

    if args.static_only:
        static_scope(args, pc, lines)
        return finish(lines, args)

    # ---- batch construction ----------------------------------------------------------------------------------------------------
    times = {'host': [], 'packed': []}
    for r in range(3 * args.rounds + 2):                     # (milliseconds each: three times the rounds of the other scopes)
        for form in ('host', 'packed'):
            idx = rng.choice(args.train, size=B, replace=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            b = host_batch(cochains, idx) if form == 'host' else pc.collate(idx)
            torch.cuda.synchronize()
            if r >= 2:                                       # (two warm-up rounds)
                times[form].append((time.perf_counter() - t0) * 1e3)
            del b
    lines.append(f'| one batch on the device with its plans, ms | {cell(times["host"])[0]} | {cell(times["packed"])[0]} | '
                 f'{verdict(times["host"], times["packed"])} |')
    parts = []
    for _ in range(args.rounds):
        host_batch(cochains, rng.choice(args.train, size=B, replace=False), parts)
    split = ', '.join(f'{name} {cell([p[k] for p in parts])[0]}' for k, name in enumerate(('host collate', 'upload', 'four CSR builds')))
    lines.append(f'| ... the parent route by part, ms (a run of its own, synchronised between the parts) | {split} | | |')

    # ---- the head -----------------------------------------------------------------------------------------------------------------
    torch.manual_seed(0)
    model = models.EdgeOrient(1, 2, args.layers, args.hidden, nonlinearity='id').to(DEV).train()
    batch = pc.collate(np.arange(B))
    x = torch.randn(batch.num_cells, args.hidden, device=DEV)
    was = models.FUSED_FLOW_HEAD

    def head(grad):
        def fn():
            if not grad:
                with torch.no_grad():
                    models._edge_readout(model, batch, x, False)
                return
            xg = x.detach().requires_grad_(True)
            model.zero_grad(set_to_none=True)
            models._edge_readout(model, batch, xg, False).square().sum().backward()
        return fn
    try:
        for grad, name in ((False, 'head forward'), (True, 'head forward + backward')):
            fn = head(grad)
            counts, times = {}, {False: [], True: []}
            for fused in (False, True):
                models.FUSED_FLOW_HEAD = fused
                for _ in range(10):
                    fn()
                assert model.last_head_route == ('fused' if fused else 'generic')
                counts[fused] = kernels_per_call(fn)
            for _ in range(args.rounds):
                for fused in (False, True):
                    models.FUSED_FLOW_HEAD = fused
                    times[fused].append(event_time(fn, args.iters))
            lines.append(f'| {name} on [{x.size(0)}, {args.hidden}], us ({counts[False]} against {counts[True]} kernels) | '
                         f'{cell(times[False])[0]} | {cell(times[True])[0]} | {verdict(times[False], times[True])} |')

        # ---- one optimisation step ----------------------------------------------------------------------------------------------------
        forms = {}
        for packed_form in (False, True):
            torch.manual_seed(0)
            m = models.EdgeOrient(1, 2, args.layers, args.hidden, nonlinearity='id').to(DEV).train()
            forms[packed_form] = (m, torch.optim.Adam(m.parameters(), lr=1e-3))
        gen = torch.Generator().manual_seed(0)
        times = {False: [], True: []}
        for r in range(args.rounds + 1):
            for packed_form in (False, True):
                m, opt = forms[packed_form]
                models.FUSED_FLOW_HEAD = packed_form
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                steps = 0
                if packed_form:
                    it = pc.batches(B, shuffle=True, seed=0)
                else:
                    order = torch.randperm(args.train, generator=gen).tolist()
                    it = (CochainBatch.from_cochain_list([cochains[i] for i in order[lo:lo + B]]).to(DEV) for lo in range(0, args.train, B))
                for b in it:
                    opt.zero_grad(set_to_none=True)
                    loss = torch.nn.functional.cross_entropy(m(b), b.y.view(-1))
                    loss.backward()
                    opt.step()
                    steps += 1
                torch.cuda.synchronize()
                if r >= 1:                                   # (one warm-up epoch per form)
                    times[packed_form].append((time.perf_counter() - t0) * 1e3 / steps)
                assert m.last_head_route == ('fused' if packed_form else 'generic')
        lines.append(f'| optimisation step, ms (epochs of {steps} shuffled batches) | {cell(times[False])[0]} | {cell(times[True])[0]} | '
                     f'{verdict(times[False], times[True])} |')
    finally:
        models.FUSED_FLOW_HEAD = was
    static_scope(args, pc, lines)
    finish(lines, args)


def finish(lines, args):
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
