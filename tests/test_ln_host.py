"""Host-side facts of the LayerNorm path (no GPU): the three entry points are exported, declared and bound, the
descriptor's ctypes layout is the header's, the argument checks refuse before any launch, and dense_ln.supported accepts
exactly the Linear -> LayerNorm -> ReLU networks of a graph_norm='ln' layer."""
import ctypes
import os
import subprocess
import tempfile

import torch
from torch.nn import BatchNorm1d as BN, ELU, LayerNorm as LN, Linear, ReLU, Sequential

from cwn_amd import _ffi, dense_ln
from cwn_amd.layers import CINppConv, SparseCINConv, _mlp_stages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('cwn_layernorm_act_f32', 'cwn_layernorm_bwd_workspace_bytes', 'cwn_layernorm_bwd_f32')


def test_exports_header_library():
    header = open(os.path.join(ROOT, 'include', 'cwn_hip.h')).read()
    lib = _ffi.lib()
    for name in NAMES:
        assert name in _ffi.EXPORTS and name + '(' in header and hasattr(lib, name), name
    assert lib.cwn_layernorm_act_f32.restype is ctypes.c_int and lib.cwn_layernorm_bwd_f32.restype is ctypes.c_int
    assert lib.cwn_layernorm_bwd_workspace_bytes.restype is ctypes.c_size_t
    assert lib.cwn_abi_version() == 24 == _ffi.ABI_VERSION and '#define CWN_ABI_VERSION 24' in header


def test_ln_desc_layout_matches_the_header():
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cwn_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(cwn_ln_desc));']
    for fname, _ in _ffi.LnDesc._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(cwn_ln_desc, {fname}));')
    lines.append('return 0; }')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, 'probe.c'), os.path.join(d, 'probe')
        open(src, 'w').write('\n'.join(lines))
        subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), src, '-o', exe], check=True)
        got = dict(l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got['size']) == ctypes.sizeof(_ffi.LnDesc)
    for fname in ('out', 'N', 'm_dev'):
        assert int(got[fname]) == getattr(_ffi.LnDesc, fname).offset, fname
    for fname, _ in _ffi.LnDesc._fields_:
        assert int(got[fname]) == getattr(_ffi.LnDesc, fname).offset, fname


def test_argument_errors_come_before_any_launch():
    lib = _ffi.lib()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    a += (-a) % 16

    def desc(**kw):
        base = dict(z=a, out=a + 64, mean=a, rstd=a, dy=a, dz=a + 64, M=1, ldz=4, ldout=4, lddy=4, lddz=4, N=4, relu=1, eps=1e-5)
        base.update(kw)
        return _ffi.LnDesc(**base)

    def act(ds):
        return lib.cwn_layernorm_act_f32((_ffi.LnDesc * len(ds))(*ds), len(ds), None)

    def bwd(ds, ws=None, nbytes=0):
        return lib.cwn_layernorm_bwd_f32((_ffi.LnDesc * len(ds))(*ds), len(ds), ws, nbytes, None)

    assert act([desc(N=0)]) == 1 and act([desc(N=1025, ldz=1025, ldout=1025)]) == 1          # CWN_ERR_BAD_ARG
    assert act([desc(M=0)] * 17) == 1 and act([desc(M=-1)]) == 1
    assert act([desc(ldz=3)]) == 1 and act([desc(out=a)]) == 1 and act([desc(z=None)]) == 1
    assert act([desc(z=a + 2)]) == 5                                                         # CWN_ERR_ALIGN
    assert act([desc(M=0)]) == 0 and act([desc(M=0, z=None, out=None)] * 16) == 0            # nothing to do
    assert bwd([desc(N=0)]) == 1 and bwd([desc(dy=None)]) == 1 and bwd([desc(mean=None)]) == 1 and bwd([desc(dz=a)]) == 1
    # the partial column sums: one [2, N] per 64-row band of the descriptors that ask for dgamma / dbeta
    ds = [desc(M=257, N=160, ldz=160, ldout=160, lddy=160, lddz=160, dgamma=a, dbeta=a), desc(M=65, dbeta=a), desc(M=1000)]
    arr = (_ffi.LnDesc * 3)(*ds)
    assert lib.cwn_layernorm_bwd_workspace_bytes(arr, 3) == 4 * (5 * 2 * 160 + 2 * 2 * 4)
    assert lib.cwn_layernorm_bwd_workspace_bytes(arr, 17) == 0
    assert bwd(ds[:1], a, 4 * (5 * 2 * 160) - 4) == 1 and bwd(ds[:1], None, 0) == 1          # undersized workspace


def _conv(cls=SparseCINConv, norm=LN, act=ReLU, hidden=32, **kw):
    args = (hidden, hidden, hidden) + (None,) * (4 if cls is SparseCINConv else 6)
    return cls(*args, max_dim=2, hidden=hidden, act_module=act, layer_dim=hidden, graph_norm=norm, use_coboundaries=True, **kw)


def _branches(conv):
    lvl = conv.mp_levels[0]
    nets = [lvl.update_up_nn, lvl.update_boundaries_nn]
    if isinstance(conv, CINppConv):
        nets.append(lvl.update_down_nn)
        if lvl.update_coboundaries_nn is not None:
            nets.append(lvl.update_coboundaries_nn)
    return nets


def _chains(conv):
    nb = len(_branches(conv))
    return conv._ln_chains([[None] * nb] * 3, [None] * (3 * nb), 0)


def test_supported_accepts_layer_norm_networks_only():
    ln = _chains(_conv())
    assert ln is not None and dense_ln.supported(*ln)
    assert len(ln[0]) == 3 and all(len(b) == 2 for b in ln[0]) and len(ln[1]) == 3
    assert dense_ln.supported(*_chains(_conv(norm=lambda n: LN(n, elementwise_affine=False))))
    assert dense_ln.supported(*_chains(_conv(CINppConv)))                               # three branches
    assert dense_ln.supported(*_chains(_conv(CINppConv, coboundary_stream=True)))       # four
    assert dense_ln.supported(*_chains(_conv(hidden=160)))                              # (combine K = 320: torch.cat + linear)
    assert not dense_ln.supported(*_chains(_conv(norm=BN)))
    assert not dense_ln.supported(*_chains(_conv(norm=torch.nn.Identity)))
    elu = _chains(_conv(act=ELU))
    assert elu[0][0][0] is None and not dense_ln.supported(*elu)                        # (_mlp_stages knows ReLU groups only)
    assert not dense_ln.supported(*_chains(_conv(norm=lambda n: LN(n // 2))))           # a LayerNorm of another width
    # ... in one stage of one branch only; and chains of unequal depth
    conv = _conv()
    conv.mp_levels[1].update_up_nn[4] = LN(16)
    assert not dense_ln.supported(*_chains(conv))
    conv = _conv()
    conv.mp_levels[2].update_boundaries_nn = Sequential(Linear(32, 32), LN(32), ReLU())
    assert not dense_ln.supported(*_chains(conv))
    assert not dense_ln.supported([], [])
    # a first stage wider than the grouped GEMM's K
    wide = Sequential(Linear(512, 32), LN(32), ReLU())
    assert not dense_ln.supported([[_mlp_stages(wide)]], [_mlp_stages(Sequential(Linear(32, 32), LN(32), ReLU()))])


def test_csl_graphs_are_the_circulant_classes():
    from cwn_amd.synthetic import CSL_SKIPS, csl_graph, csl_graphs
    assert CSL_SKIPS == (2, 3, 4, 5, 6, 9, 11, 12, 13, 16)
    pool = csl_graphs(20, seed=1)
    for k, cx in enumerate(pool):
        assert cx.cochains[0].num_cells == 41 and cx.cochains[1].num_cells == 82 and int(cx.y) == k % 10
        deg = torch.bincount(cx.cochains[1].boundary_index[0], minlength=41)
        assert bool((deg == 4).all())
        # a relabelled copy has the rings of its class
        assert cx.cochains[2].num_cells == pool[k % 10].cochains[2].num_cells
    assert len({tuple(csl_graph(r)[1]) for r in CSL_SKIPS}) == 10


def test_switch_reads_the_environment():
    env = dict(os.environ, CWN_FUSED_LN='0')
    out = subprocess.run([os.sys.executable, '-c', 'from cwn_amd import dense_ln; print(dense_ln.FUSED_LN)'], env=env, cwd=ROOT,
                         check=True, capture_output=True, text=True).stdout
    assert out.strip() == 'False' and dense_ln.FUSED_LN is (os.environ.get('CWN_FUSED_LN') != '0')
