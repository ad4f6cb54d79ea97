"""Host-side checks of the counted GIN layers (cwn_gin_layer_dev_f32 / cwn_gine_layer_dev_f32, ops.gin_layer_counted /
gine_layer_counted, the 'fused_counted' route of layers.GINConv / GINEConv) -- no GPU needed: the C ABI (both symbols declared,
exported, bound, the ABI number unmoved), every argument check (those of the host-count entries, then the count's own: they
all precede the first HIP call, so made-up aligned addresses never reach a device), the ops' refusals, and the dispatch
predicates of the layers under _ffi.dynamic_rows."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from cwn_amd import _ffi, layers, ops
from tests import test_gin_host as gin_host
from tests import test_gine_host as gine_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, TOO_LARGE, ALIGN = 0, 1, 2, 5
P = gin_host.P
N_DEV = 50 * P                      # a made-up, 8-byte aligned address for the count


def _gin(d, n_dev=N_DEV):
    return _ffi.lib().cwn_gin_layer_dev_f32(C.byref(d), n_dev, None)


def _gine(d, n_dev=N_DEV):
    return _ffi.lib().cwn_gine_layer_dev_f32(C.byref(d), n_dev, None)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_both_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, 'include', 'cwn_hip.h')).read()
    lib = _ffi.lib()
    for name in ('cwn_gin_layer_dev_f32', 'cwn_gine_layer_dev_f32'):
        assert re.search(r'\bint %s\s*\(const cwn_gine?_desc\* \w+, const int64_t\* n_dev, cwn_stream_t stream\)' % name, header)
        assert name in _ffi.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).restype is C.c_int and len(getattr(lib, name).argtypes) == 3
    assert callable(_ffi.gin_layer_counted) and callable(_ffi.gine_layer_counted)
    assert lib.cwn_abi_version() == _ffi.ABI_VERSION == 24
    assert int(re.search(r'#define CWN_ABI_VERSION (\d+)', header).group(1)) == 24
    section = header[header.index('The counted GIN layers'):header.index('int cwn_gin_layer_dev_f32')]
    assert 'CAPACITY' in section and 'rows_clamped' in section and 'never written' in section
    # the count reader is written once, in the shared header, and both kernels take the count beside their arguments
    csrc = os.path.join(ROOT, 'cwn_amd', 'csrc')
    tile = open(os.path.join(csrc, 'cwn_gin_tile.h')).read()
    assert 'int64_t live_rows(' in tile and 'cwn::rows_clamped(' in tile and 'int gin_count_check(' in tile
    for f in ('cwn_gin.hip', 'cwn_gine.hip'):
        src = open(os.path.join(csrc, f)).read()
        assert 'live_rows(P, n_dev)' in src and 'rows_clamped' not in src and 'int64_t live_rows(' not in src, f


# ---- the argument checks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sorted(gin_host.BAD))
def test_gin_check_cases_are_refused_before_any_hip_call(case):
    assert _gin(gin_host._desc(**gin_host.BAD[case])) == BAD_ARG, case
    assert _gine(gine_host._desc(**gin_host.BAD[case])) == BAD_ARG, case


@pytest.mark.parametrize('case', sorted(gine_host.BAD_EDGE))
def test_gine_edge_cases_are_refused_before_any_hip_call(case):
    assert _gine(gine_host._desc(**gine_host.BAD_EDGE[case])) == BAD_ARG, case


def test_null_descriptor_misaligned_pointers_and_too_many_tiles():
    assert _ffi.lib().cwn_gin_layer_dev_f32(None, N_DEV, None) == BAD_ARG
    assert _ffi.lib().cwn_gine_layer_dev_f32(None, N_DEV, None) == BAD_ARG
    for field in ('x', 'rowptr', 'col', 'eps_dev', 'W1', 'b1', 'scale1', 'shift1', 'W2', 'b2', 'scale2', 'shift2', 'out'):
        assert _gin(gin_host._desc(**{field: 40 * P + 2})) == ALIGN, field
        assert _gine(gine_host._desc(**{field: 40 * P + 2})) == ALIGN, field
    for field in ('e', 'eidx'):
        assert _gine(gine_host._desc(**{field: 40 * P + 2})) == ALIGN, field
    big = dict(n=_ffi.GIN_TM * (2 ** 31 - 1), x=0x10, out=0x7f0000000000)
    assert _gin(gin_host._desc(**big)) == TOO_LARGE and _gine(gine_host._desc(**big)) == TOO_LARGE


def test_the_count_is_required_and_8_byte_aligned():
    for call, desc in ((_gin, gin_host._desc), (_gine, gine_host._desc)):
        assert call(desc(), None) == BAD_ARG                    # n > 0 and no count
        assert call(desc(), N_DEV + 4) == ALIGN                 # 4-byte aligned is not enough for an int64
        assert call(desc(), N_DEV + 2) == ALIGN
        # the descriptor's own checks come first, with their codes
        assert call(desc(w=0), N_DEV + 4) == BAD_ARG
        assert call(desc(x=40 * P + 2), None) == ALIGN
        assert call(desc(**{'n': _ffi.GIN_TM * (2 ** 31 - 1), 'x': 0x10, 'out': 0x7f0000000000}), None) == TOO_LARGE
    assert _gine(gine_host._desc(e=None), None) == BAD_ARG


def test_empty_launches_are_ok_without_a_device():
    """n == 0 returns before the first HIP call, with or without a count."""
    for call, desc in ((_gin, gin_host._desc), (_gine, gine_host._desc)):
        assert call(desc(n=0)) == OK
        assert call(desc(n=0), None) == OK
        assert call(desc(n=0, x=None, out=None, W1=None, W2=None), None) == OK
        assert call(desc(n=0), N_DEV + 4) == ALIGN
    assert _gine(gine_host._desc(n=0, rowptr=None, col=None, e=None, eidx=None, lde=0, n_e=0)) == OK


# ---- the ops --------------------------------------------------------------------------------------------------------------------
def test_ops_signatures_and_refusals():
    assert list(inspect.signature(ops.gin_layer_counted).parameters) == ['x', 'adj', 'eps', 'stages', 'act', 'act_post', 'out',
                                                                         'n_dev']
    assert list(inspect.signature(ops.gine_layer_counted).parameters) == ['x', 'adj', 'edge', 'eps', 'stages', 'act', 'act_post',
                                                                          'out', 'edge_mode', 'n_dev']
    x, e = torch.randn(4, 3), torch.randn(2, 3)
    st = [(torch.randn(5, 3), None, None, None), (torch.randn(5, 5), None, None, None)]
    n_dev = torch.tensor([4])
    with pytest.raises(TypeError, match='gin_layer_counted: x must be a float32 tensor on the GPU'):
        ops.gin_layer_counted(x, None, None, st, 'relu', n_dev=n_dev)
    with pytest.raises(TypeError, match='gin_layer_counted: x must be float32 .got torch.float64.'):
        ops.gin_layer_counted(x.double(), None, None, st, 'relu', n_dev=n_dev)
    with pytest.raises(TypeError, match='gine_layer_counted: x must be float32 .got torch.float64.'):
        ops.gine_layer_counted(x.double(), None, None, None, st, 'relu', n_dev=n_dev)
    with pytest.raises(TypeError, match='gine_layer_counted: edge must be float32 .got torch.float16.'):
        ops.gine_layer_counted(x, None, e.half(), None, st, 'relu', n_dev=n_dev)
    with pytest.raises(TypeError, match='n_dev'):
        ops.gine_layer_counted(x, None, None, None, st, 'relu', n_dev=None)
    with pytest.raises(ValueError, match='edge_mode'):
        ops.gine_layer_counted(x, None, None, None, st, 'relu', edge_mode='col', n_dev=n_dev)
    with pytest.raises(TypeError):
        ops.gin_layer_counted(x, None, None, st, 'relu')                    # n_dev is required
    # the count: one int64 on x's device, or an address
    dev = torch.device('cpu')
    assert ops._count_address('op', n_dev, dev) == n_dev.data_ptr() and ops._count_address('op', 4096, dev) == 4096
    for bad in (torch.tensor([4], dtype=torch.int32), torch.tensor([4, 5]), torch.tensor([4.0]), None, 0, True, 4.0):
        with pytest.raises(TypeError, match='op: n_dev'):
            ops._count_address('op', bad, dev)


def test_host_count_ops_still_refuse_a_static_batch():
    """ops.gin_layer / gine_layer decline under _ffi.dynamic_rows, as before (the check sits behind the operand checks, which
    CPU tensors do not pass: read from the source, and pinned on the device by tests/test_gpu_gine.py)."""
    src = inspect.getsource(ops._gin_descriptor)
    assert 'if _ffi.DYN_ROWS and not counted:' in src and 'does not run under _ffi.dynamic_rows' in src


# ---- the dispatch predicates ------------------------------------------------------------------------------------------------------
def _net(w, H):
    return torch.nn.Sequential(torch.nn.Linear(w, H), torch.nn.Identity(), torch.nn.ReLU(),
                               torch.nn.Linear(H, H), torch.nn.Identity(), torch.nn.ReLU())


def _switch(on):
    class _S:
        def __enter__(self):
            self.old, layers.FUSED_GIN_STATIC = layers.FUSED_GIN_STATIC, on

        def __exit__(self, *exc):
            layers.FUSED_GIN_STATIC = self.old
    return _S()


def test_the_switch_exists_and_follows_its_default():
    assert layers.FUSED_GIN_STATIC_DEFAULT in (True, False) and isinstance(layers.FUSED_GIN_STATIC, bool)
    if os.environ.get('CWN_FUSED_GIN_STATIC') not in ('0', '1'):
        assert layers.FUSED_GIN_STATIC is layers.FUSED_GIN_STATIC_DEFAULT


@pytest.mark.parametrize('kind', ['gin', 'gine'])
def test_layers_answer_generic_under_dynamic_rows_without_the_switch_or_a_count(kind):
    torch.manual_seed(0)
    conv = (layers.GINConv if kind == 'gin' else layers.GINEConv)(_net(3, 4)).eval()
    x = torch.randn(6, 3)
    idx = torch.tensor([[0, 1, 2, 5], [1, 0, 1, 1]])
    args = (x, idx) if kind == 'gin' else (x, idx, torch.randn(4, 3))
    with torch.no_grad():
        ref = conv(*args)
    count = torch.tensor([6])
    # (switch, the capacity the count is registered for): off with a count for x's rows; on with a count for another capacity;
    # on with a count for x's rows but operands the launch does not take (CPU tensors)
    for on, cap in ((False, 6), (True, 7), (True, 6)):
        conv.last_route = None
        with _switch(on), _ffi.dynamic_rows({cap: count.data_ptr()}), torch.no_grad():
            assert conv.counted_stages(x) is None and conv.fused_stages(x) is None
            y = conv(*args)
        assert conv.last_route == 'generic', (on, cap)
        assert torch.equal(y, ref)
    # outside dynamic_rows the counted route is never asked for
    with _switch(True), torch.no_grad():
        assert conv.counted_stages(x) is None
