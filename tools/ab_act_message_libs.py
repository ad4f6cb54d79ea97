"""The activated message's kernels (cwn_aggregate_act_*, cwn_aggregate_act_bwd_*) of TWO builds of the library in ONE process:
the same descriptors go to the loaded library (`new`) and to the one given on the command line (`parent`), 20 launches between
two device events, the libraries alternating region by region.  Shape: 200 000 rows of 0..12 entries (50 of them 300, through
the long-row pass), F = 16 and 64, id / elu / tanh, float32 and float64 -- launches of 50 us to 1 ms, bound by the device.
Reported: us per launch, median [min .. max] of 9 regions, and whether new - parent is within the larger of the two spreads.

    python tools/ab_act_message_libs.py /path/to/the/other/libcwn_hip.so
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd import _ffi, ops
from cwn_amd.csr import Adjacency

DEV = 'cuda:0'
STRUCT = {'aggregate_act': _ffi.AggActDesc, 'aggregate_act_bwd': _ffi.AggActBwdDesc}


def entry(lib, stem, dtype):
    fn = getattr(lib, f'cwn_{stem}_{"f32" if dtype == torch.float32 else "f64"}')
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(STRUCT[stem]), C.c_int, C.c_void_p]
    return fn


def time_ab(libs, stem, dtype, descs):
    arr = (STRUCT[stem] * len(descs))(*descs)
    s = _ffi.stream_ptr(torch.device(DEV))
    fns = {k: entry(lib, stem, dtype) for k, lib in libs.items()}
    got = {k: [] for k in fns}
    for k, fn in fns.items():
        for _ in range(5):
            assert fn(arr, len(descs), s) == 0
    torch.cuda.synchronize()
    for _ in range(9):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20):
                fn(arr, len(descs), s)
            b.record()
            torch.cuda.synchronize()
            got[k].append(a.elapsed_time(b) * 1e3 / 20)
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in got.items()}


def main():
    assert len(sys.argv) == 2 and torch.cuda.is_available(), __doc__
    libs = {'parent': C.CDLL(os.path.abspath(sys.argv[1])), 'new': _ffi.lib()}
    rng = np.random.default_rng(0)
    n_dst, n_src, n_cob = 200_000, 150_000, 120_000
    deg = rng.integers(0, 13, n_dst)
    deg[:50] = 300                                   # long rows through LDS
    dst = np.repeat(np.arange(n_dst), deg)
    E = dst.size
    src, cob = rng.integers(0, n_src, E), rng.integers(0, n_cob, E)
    p = rng.permutation(E)
    dst, src, cob = (torch.as_tensor(t[p]).long() for t in (dst, src, cob))
    adj = Adjacency.from_index(torch.stack([src, dst]).to(DEV), n_dst, n_src, aux_index=cob.to(DEV), n_aux=n_cob)
    print(f'{torch.cuda.get_device_name(0)}; {n_dst} rows, {E} entries (50 rows of 300), sources {n_src}, shared cells {n_cob}; us per launch, '
          'median [min .. max] of 9 regions of 20 launches, libraries alternating in one process')
    print('| kernel | dtype | F | act | parent | new | new - parent | larger spread | within |')
    print('|---|---|---|---|---|---|---|---|---|')
    ok = True
    for dtype in (torch.float32, torch.float64):
        for F in (16, 64):
            g = torch.Generator().manual_seed(1)
            mk = lambda n: (0.5 * torch.randn(n, F, generator=g, dtype=torch.float64)).to(dtype).to(DEV)
            A, B, self_x, gr = mk(n_src), mk(n_cob), mk(n_dst), mk(n_dst)
            eps = torch.tensor([0.25], dtype=dtype, device=DEV)
            for act in ('id', 'elu', 'tanh'):
                code = ops.ACT_CODES[act]
                f = ops.AggActSpec(adj=adj, n_dst=n_dst, F=F, act=code, A=A, ia=adj.col, B=B, ib=adj.aux, self_x=self_x, eps=eps)
                ops.run_aggregate_act([f], DEV)
                ts, ta = adj.t_src, adj.t_aux
                bw = [ops.AggActBwdSpec(adj=ts, F=F, act=code, g=gr, ig=ts.col, P=A, Q=B, iq=ts.aux),
                      ops.AggActBwdSpec(adj=ta, F=F, act=code, g=gr, ig=ta.col, P=B, Q=A, iq=ta.aux)]
                ops.run_aggregate_act_bwd(bw, DEV)
                torch.cuda.synchronize()
                for stem, descs in (('aggregate_act', [f.desc()]), ('aggregate_act_bwd', [s.desc() for s in bw])):
                    r = time_ab(libs, stem, dtype, descs)
                    d = r['new'][0] - r['parent'][0]
                    spread = max(r['new'][2] - r['new'][1], r['parent'][2] - r['parent'][1])
                    ok = ok and d <= spread
                    cell = lambda k: f'{r[k][0]:.1f} [{r[k][1]:.1f} .. {r[k][2]:.1f}]'
                    print(f'| {stem} | {str(dtype)[6:]} | {F} | {act} | {cell("parent")} | {cell("new")} | {d:+.1f} | {spread:.1f} | '
                          f'{"yes" if d <= spread else "NO"} |', flush=True)
    print('every case within the margin' if ok else 'NOT every case within the margin')


if __name__ == '__main__':
    main()
