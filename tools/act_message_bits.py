"""The bits of the activated coboundary message, forward (cwn_aggregate_act_*) and backward (cwn_aggregate_act_bwd_*), as
one SHA-256 per case: five activations x {float32, float64} x F in {3, 64, 200}, on the adjacency of
tests/test_gpu_act_message_bwd.py (rows of 0, 1, 16, 17, 64, 65 and 300 entries in every keying) with operands from an
integer formula.  Two builds of the library that print the same lines compute the same bits: with -ffp-contract=off and the
order of the sums fixed by the source, another instruction schedule must not change one.

    python tools/act_message_bits.py > new.txt;  CWN_HIP_LIB=/path/to/other/libcwn_hip.so python tools/act_message_bits.py > old.txt
"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cwn_amd import _ffi, ops                                               # noqa: E402
from cwn_amd.csr import Adjacency                                           # noqa: E402

DEV = 'cuda:0'
N_DST, N_SRC, N_COB = 40, 24, 20
SPECIAL = (0, 1, 16, 17, 64, 65, 300)
N_ENTRIES = sum(SPECIAL) + 66


def lengths(n):
    rest, k = N_ENTRIES - sum(SPECIAL), n - len(SPECIAL)
    return list(SPECIAL) + [rest // k + (1 if i < rest % k else 0) for i in range(k)]


def operand(rows, F, k, dtype):
    """[rows, F] of ((7 i + 3 j + k) mod 11 - 5) / 4: quarters in [-1.25, 1.25], exact in both types."""
    i, j = torch.arange(rows).unsqueeze(1), torch.arange(F).unsqueeze(0)
    return (((7 * i + 3 * j + k) % 11 - 5).to(torch.float64) / 4).to(dtype).to(DEV)


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def main():
    assert torch.cuda.is_available(), 'the kernels run on the GPU; there is no other figure'
    rng = np.random.default_rng(7)
    dst, src, cob = (torch.as_tensor(rng.permutation(np.repeat(np.arange(n), lengths(n)))).long() for n in (N_DST, N_SRC, N_COB))
    adj = Adjacency.from_index(torch.stack([src, dst]).to(DEV), N_DST, N_SRC, aux_index=cob.to(DEV), n_aux=N_COB)
    print(f'# {_ffi.LIB_PATH}', file=sys.stderr)
    for act, code in sorted(ops.ACT_CODES.items(), key=lambda kv: kv[1]):
        for dtype in (torch.float32, torch.float64):
            for F in (3, 64, 200):
                A, B, self_x, g = (operand(n, F, k, dtype) for k, n in enumerate((N_SRC, N_COB, N_DST, N_DST)))
                eps = torch.tensor([0.25], dtype=dtype, device=DEV)
                fwd = ops.run_aggregate_act([ops.AggActSpec(adj=adj, n_dst=N_DST, F=F, act=code, A=A, ia=adj.col, B=B, ib=adj.aux,
                                                            self_x=self_x, eps=eps)], DEV)
                ts, ta = adj.t_src, adj.t_aux
                bwd = ops.run_aggregate_act_bwd([ops.AggActBwdSpec(adj=ts, F=F, act=code, g=g, ig=ts.col, P=A, Q=B, iq=ts.aux),
                                                 ops.AggActBwdSpec(adj=ta, F=F, act=code, g=g, ig=ta.col, P=B, Q=A, iq=ta.aux)], DEV)
                torch.cuda.synchronize()
                assert all(bool(torch.isfinite(t).all()) for t in fwd + bwd)
                name = str(dtype).replace('torch.', '')
                print(f'{act:8s} {name} F={F:<3d} forward  {digest(fwd)}')
                print(f'{act:8s} {name} F={F:<3d} backward {digest(bwd)}', flush=True)


if __name__ == '__main__':
    main()
