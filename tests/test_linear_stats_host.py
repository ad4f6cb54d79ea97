"""cwn_linear_stats_f32 without a GPU (csrc/cwn_linear_stats.hip behind ops.run_linear_stats and dense_train's forward): the
symbol is declared, exported and bound under ABI 24, the launcher refuses every malformed descriptor before anything is
launched and takes empty launches without a device, the router declines every launch that is not its own, and the static
drivers refuse at construction what no static batch of that mode serves."""
import os
import re

import pytest
import torch

from cwn_amd import _ffi, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, ALIGN = 0, 1, 5
P = 0x100000


def test_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'cwn_hip.h')).read()
    lib = _ffi.lib()
    assert re.search(r'\bint cwn_linear_stats_f32\s*\(const cwn_gemm_desc\* descs_host, int n, cwn_stream_t stream\)', header)
    assert 'cwn_linear_stats_f32' in _ffi.EXPORTS and hasattr(lib, 'cwn_linear_stats_f32')
    assert lib.cwn_linear_stats_f32.argtypes[0]._type_ is _ffi.GemmDesc           # cwn_gemm_desc, unchanged
    assert lib.cwn_abi_version() == _ffi.ABI_VERSION == 24
    assert int(re.search(r'#define CWN_ABI_VERSION (\d+)', header).group(1)) == 24
    section = header[header.index('A Linear stage with band statistics under a row count'):header.index('int cwn_linear_stats_f32')]
    for said in ('m_dev', 'never', 'NaN', 'CWN_STAT_ROWS(live)', 'cwn_bn_finalize_f32', 'bit for bit', 'CWN_ERR_BAD_ARG',
                 'without a device'):
        assert said in section, said
    assert 'cwn_linear_stats.hip' in open(os.path.join(ROOT, 'cwn_amd', 'csrc', 'Makefile')).read()
    assert _ffi.lib().cwn_error_string(BAD_ARG) and _ffi.lib().cwn_error_string(ALIGN)


def _desc(**kw):
    """A descriptor that passes every check (made-up, aligned addresses far apart: a call that passed the checks with rows
    would launch, so every case below breaks exactly one thing or has no rows)."""
    d = _ffi.GemmDesc(X=P, X2=2 * P, W=3 * P, bias=4 * P, in_scale=5 * P, in_shift=6 * P, in_scale2=7 * P, in_shift2=8 * P,
                      col_sum=9 * P, col_sumsq=10 * P, Y=11 * P, M=70, ldx=13, ldx2=6, ldw=19, ldy=37, N=37, K=13, K2=5,
                      in_relu=3, flags=_ffi.GEMM_EXACT, m_dev=12 * P)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _call(*ds, n=None):
    arr = (_ffi.GemmDesc * max(len(ds), 1))(*ds)
    return _ffi.lib().cwn_linear_stats_f32(arr if ds else None, len(ds) if n is None else n, None)


BAD = {
    'w_trans': dict(w_trans=1),
    'bnb': dict(bnb=_ffi.C.pointer(_ffi.GemmBnb())),
    'out_scale': dict(out_scale=20 * P, out_shift=21 * P),
    'out_shift alone': dict(out_shift=21 * P),
    'relu': dict(relu=1),
    'flag W_PACKED': dict(flags=_ffi.GEMM_EXACT | _ffi.GEMM_W_PACKED),
    'flag ADD_OUT': dict(flags=_ffi.GEMM_ADD_OUT),
    'a debug flag': dict(flags=1 << 8),
    'col_sum alone': dict(col_sumsq=None),
    'col_sumsq alone': dict(col_sum=None),
    'N = 0': dict(N=0),
    'N = 129': dict(N=129, ldy=129),
    'K = 0': dict(K=0),
    'K2 < 0': dict(K2=-1),
    'K + K2 = 257': dict(K=252, ldx=252, ldw=257),
    'X2 without K2': dict(K2=0),
    'K2 without X2': dict(X2=None),
    'M < 0': dict(M=-1),
    'ldx < K': dict(ldx=12),
    'ldx2 < K2': dict(ldx2=4),
    'ldw < K + K2': dict(ldw=17),
    'ldy < N': dict(ldy=36),
    'in_scale alone': dict(in_shift=None),
    'in_shift2 alone': dict(in_scale2=None),
    'X NULL with rows': dict(X=None),
    'W NULL with rows': dict(W=None),
    'Y NULL with rows': dict(Y=None),
}


@pytest.mark.parametrize('case', sorted(BAD))
def test_malformed_descriptors_are_refused_before_any_launch(case):
    assert _call(_desc()) is not None
    assert _call(_desc(**BAD[case])) == BAD_ARG, case
    assert _call(_desc(M=0), _desc(**BAD[case])) == BAD_ARG, case           # ... wherever it stands in the launch


def test_descriptor_counts_and_empty_launches():
    lib = _ffi.lib()
    assert _call(n=-1) == BAD_ARG
    assert _call(n=_ffi.MAX_DESCS + 1) == BAD_ARG
    assert lib.cwn_linear_stats_f32(None, 1, None) == BAD_ARG
    assert lib.cwn_linear_stats_f32(None, 0, None) == OK                   # nothing to do, no device touched
    assert _call(_desc(M=0)) == OK
    assert _call(*[_desc(M=0, K2=0, X2=None, in_scale2=None, in_shift2=None, col_sum=None, col_sumsq=None, bias=None)
                   for _ in range(_ffi.MAX_DESCS)]) == OK
    assert _call(_desc(M=0, X=None, W=None, Y=None)) == OK                 # (operands are required with rows only)
    assert _call(_desc(M=0, X=P + 2)) == ALIGN and _call(_desc(M=0, col_sum=9 * P + 4)) == ALIGN


def _gemm(M=40, K=12, N=20, stats=True, **kw):
    X, W = torch.zeros(M, K), torch.zeros(N, K)
    cs = torch.zeros(2, ops.stat_rows(M), N, dtype=torch.float64) if stats else None
    return ops.Gemm(X=X, W=W, col_stats=cs, **kw)


def test_router_declines_without_a_device_side_count():
    """Outside a static slot nothing has a device-side count: the eager step keeps cwn_gemm_f32 at every width."""
    assert not _ffi.DYN_ROWS
    assert ops.run_linear_stats([_gemm()], torch.device('cpu')) is None
    assert ops.run_linear_stats([], torch.device('cpu')) is None
    with _ffi.dynamic_rows({41: P}):                                       # a count, but not of these rows
        assert ops.run_linear_stats([_gemm()], torch.device('cpu')) is None
    with _ffi.dynamic_rows({40: P}):                                       # counted rows without statistics: cwn_gemm_f32 has the count
        assert ops.run_linear_stats([_gemm(stats=False)], torch.device('cpu')) is None


@pytest.mark.parametrize('what', ['w_trans', 'bnb', 'relu', 'out_scale', 'add_out', 'stat_slots', 'in_bn', 'more', 'wide', 'deep',
                                  'too many', 'stats shape'])
def test_router_declines_what_the_entry_point_refuses(what):
    """... and inside one, a launch that needs what cwn_linear_stats_f32 refuses goes on to cwn_gemm_f32 (which then names the
    conflict itself)."""
    kw = {'w_trans': dict(w_trans=True), 'bnb': dict(bnb=_ffi.GemmBnb()), 'relu': dict(relu=True),
          'out_scale': dict(out_scale=torch.ones(20), out_shift=torch.zeros(20)), 'add_out': dict(add_out=True),
          'stat_slots': dict(stat_slots=torch.zeros(_ffi.BN_SLOTS, 2, 20, dtype=torch.float64)), 'in_bn': dict(in_bn=object()),
          'more': dict(more=((torch.zeros(40, 12), True, None),))}.get(what, {})
    with _ffi.dynamic_rows({40: P}):
        gms = [_gemm(**kw)]
        if what == 'wide':
            gms = [_gemm(N=129)]
        elif what == 'deep':
            gms = [_gemm(K=257)]
        elif what == 'too many':
            gms = [_gemm() for _ in range(_ffi.MAX_DESCS + 1)]
        elif what == 'stats shape':
            gms[0].col_stats = torch.zeros(2, 3, 20, dtype=torch.float64)
        assert ops.run_linear_stats(gms, torch.device('cpu')) is None
        # (one good product next to it does not change the answer: the launch is taken whole or not at all)
        assert ops.run_linear_stats([_gemm()] + gms, torch.device('cpu')) is None


def test_stage_bwd_takes_reads_width_and_shape():
    """The lazy BatchNorm-backward form is kept under a count only where the backward stage launch takes the product."""
    assert not ops.stage_bwd_takes(torch.zeros(48, 48), 48)
    assert not ops.stage_bwd_takes(torch.zeros(64, 7), 64)                 # a first layer over raw features
    assert not ops.stage_bwd_takes(torch.zeros(64, 64), 64)                # (no packed block: nothing was packed on the CPU)
    assert not ops.stage_bwd_takes(torch.zeros(64, 128), 64, blocks=3)


class _Static:
    def __init__(self, mode):
        self.mode = mode


def test_static_drivers_name_the_mode_or_the_layer_at_other_widths():
    from cwn_amd.models import EmbedCINpp, EmbedSparseCIN, SparseCIN
    from cwn_amd.static_graph import refuse_unsupported_layers
    kw = dict(dropout_rate=0.0, max_dim=2, embed_edge=True, use_coboundaries=True)
    m48, m128 = EmbedSparseCIN(28, 4, 1, 2, 48, **kw), EmbedSparseCIN(28, 4, 1, 2, 128, **kw)
    for who, training in (('StaticForward', False), ('StaticTrainStep', True)):
        refuse_unsupported_layers(m128, who, _Static('blocked'), training=training)
        refuse_unsupported_layers(m48, who, _Static('csr'), training=training)
        with pytest.raises(NotImplementedError, match=r"\[48\].*mode='csr'"):
            refuse_unsupported_layers(m48, who, _Static('blocked'), training=training)
    raw = SparseCIN(7, 3, 2, 64, max_dim=2, dropout_rate=0.0, graph_norm='bn')
    refuse_unsupported_layers(raw, 'StaticTrainStep', _Static('csr'), training=True)
    with pytest.raises(NotImplementedError, match="mode='csr'"):
        refuse_unsupported_layers(raw, 'StaticTrainStep', _Static('blocked'), training=True)
    # CIN++: the combine network of a width the stage kernels do not hold runs as torch modules -- BatchNorm(train) over the
    # capacity rows of a slot
    pp48, pp64 = EmbedCINpp(28, 4, 1, 2, 48, **kw), EmbedCINpp(28, 4, 1, 2, 64, **kw)
    refuse_unsupported_layers(pp64, 'StaticTrainStep', _Static('csr'), training=True)
    refuse_unsupported_layers(pp48, 'StaticForward', _Static('csr'), training=False)
    with pytest.raises(NotImplementedError, match=r'CINppConv\(width 48\).*capacity rows'):
        refuse_unsupported_layers(pp48, 'StaticTrainStep', _Static('csr'), training=True)
