"""Cellular message-passing layers on the MI355X engine.

Host-side mirror of the reference's mp/layers.py: same class names, constructor arguments,
`forward` signatures and parameter names (state_dicts are interchangeable -- the golden tests load
the reference's state_dict), so mp/models.py / mp/molec_models.py-style model code runs on it
unchanged.  What changes is HOW a layer runs:

  * SparseCINConv.forward (mp/layers.py:333-342) issues ONE aggregation launch for all cochain
    dimensions and both adjacencies (upper + boundary), with the GIN self terms
    `+(1+eps)*x` (:191-192) and the zero rows of absent adjacencies folded into it;
  * the coboundary message  ReLU(Linear_{2F->F}(cat(x_j, up_attr)))  (:290-293) is evaluated as
    ReLU(Y1[j] + Y2[c]) with Y1 = X_d W[:, :F]^T + b and Y2 = X_{d+1} W[:, F:]^T: the per-message
    `[E, 2F]` matrix and GEMM disappear (GEMM rows drop from E to N_d + N_{d+1}); the result
    differs from the reference only by fp32 summation order (< 1e-5, tested);
  * `up_attr` arrives lazily (IndexedRows), so the K3 gather of data/complex.py:579-580 is never
    materialised;
  * anything not recognised (custom message nets, other activations) takes the generic
    gather-kernel -> hook -> segmented-reduce-kernel path of CochainMessagePassing and is still
    correct.
"""
import os
import weakref
from abc import ABC, abstractmethod
from typing import Any, Callable, List, Optional

import torch
from torch import Tensor
from torch.nn import BatchNorm1d as BN, Linear, ReLU, Sequential

from . import ops
from .blockplan import I_CN, I_TASK0, T_N
from .cell_mp import CochainMessagePassing, CochainMessagePassingParams, IndexedRows, _zero_dtype, dense
from .csr import Adjacency, cached_adjacency


def reset(nn):
    """torch_geometric.nn.inits.reset semantics (used at mp/layers.py:88-92, 201-208)."""
    def _reset(item):
        if hasattr(item, 'reset_parameters'):
            item.reset_parameters()
    if nn is not None:
        if hasattr(nn, 'children') and len(list(nn.children())) > 0:
            for item in nn.children():
                _reset(item)
        else:
            _reset(nn)


class Catter(torch.nn.Module):
    """mp/layers.py:263-268."""

    def forward(self, x):
        return torch.cat(x, dim=-1)


class FirstOf(torch.nn.Module):
    """The `lambda xs: xs[0]` of mp/layers.py:295 as a named module, so the engine can recognise
    the identity message and fuse it."""

    def forward(self, xs):
        return xs[0]


class Passthrough(torch.nn.Module):
    """The `lambda x: x` of mp/layers.py:299."""

    def forward(self, x):
        return x


def _attr_operand(attr):
    """(B matrix, ib_mode) for an attribute that is lazy (gather through the shared-cell index) or
    dense (one row per entry)."""
    if isinstance(attr, IndexedRows):
        return attr.src, 'aux'
    return attr, 'perm'


def _is_cat_linear_relu(nn) -> bool:
    return (isinstance(nn, Sequential) and len(nn) == 3 and isinstance(nn[0], Catter)
            and isinstance(nn[1], Linear) and isinstance(nn[2], ReLU))


def identity(x):
    """The 'id' nonlinearity (mp/nn.py:16-17) as ONE function object, so that a layer can recognise it."""
    return x


# The five nonlinearities of mp/nn.py:7-28 by their ops.ACT_CODES name, as (module class, function): what
# models.get_nonlinearity hands out, and how a layer recognises what it was given.
ACTIVATIONS = {'relu': (ReLU, torch.nn.functional.relu), 'elu': (torch.nn.ELU, torch.nn.functional.elu),
               'id': (torch.nn.Identity, identity), 'sigmoid': (torch.nn.Sigmoid, torch.sigmoid), 'tanh': (torch.nn.Tanh, torch.tanh)}


def _act_name(module) -> Optional[str]:
    """The ACTIVATIONS name of an activation module; None for any other module and for an ELU whose alpha is not 1 (the
    kernels compute expm1 alone)."""
    name = next((n for n, (cls, _) in ACTIVATIONS.items() if type(module) is cls), None)
    return None if name == 'elu' and module.alpha != 1.0 else name


def _act_name_of_function(fn) -> Optional[str]:
    return next((n for n, (_, f) in ACTIVATIONS.items() if f is fn), None)


def _cat_linear_act(nn) -> Optional[str]:
    """The activation's name when `nn` is Sequential(Catter, Linear, ELU | Tanh | Sigmoid | Identity), else None (ReLU
    too: that form is `_is_cat_linear_relu`'s, with routes of its own)."""
    if not (isinstance(nn, Sequential) and len(nn) == 3 and isinstance(nn[0], Catter) and isinstance(nn[1], Linear)):
        return None
    name = _act_name(nn[2])
    return None if name == 'relu' else name


# A coboundary message act(Linear(cat(x_j, up_attr))) with an activation other than ReLU as two per-cell products and one
# cwn_aggregate_act_f32 / _f64 launch (csrc/cwn_aggregate_act.hip; inference only unless ops.ACT_MESSAGE_BACKWARD is on, which
# puts the recording autograd on the same launch and its backward on cwn_aggregate_act_bwd_f32 / _f64) instead of the generic propagate (two row
# gathers, cat, a per-entry product, the activation, the segmented reduce).  True / False: for every dtype / for none
# (CWN_FUSED_ACT_MESSAGE=1 / =0); a set of dtypes: for those -- the default, FUSED_ACT_MESSAGE_DEFAULT, holds the dtypes at
# which the route has measured faster than the generic propagate by more than the run-to-run spread of both forms
# (tools/bench_act_message.py, profiles/act_message.md: float64 1.32 against 1.92 ms for the SR forward; the float32 forward
# has no figure yet, so float32 stays off unless asked for).
FUSED_ACT_MESSAGE_DEFAULT = frozenset({torch.float64})
FUSED_ACT_MESSAGE = {'0': False, '1': True}.get(os.environ.get('CWN_FUSED_ACT_MESSAGE'), FUSED_ACT_MESSAGE_DEFAULT)


def _act_message_on(dtype) -> bool:
    on = FUSED_ACT_MESSAGE
    return dtype in on if isinstance(on, (set, frozenset)) else bool(on)
FUSED_DENSE_TRAINING = True   # set False to run the update / combine networks as torch modules
FUSED_CINPP_COMBINE = os.environ.get('CWN_FUSED_CINPP_COMBINE') != '0'    # False: CINppConv's combine network as torch modules behind the fused branches
FUSED_CIN_TRAINING = os.environ.get('CWN_FUSED_CIN_TRAINING') != '0'      # False: CINCochainConv's training forward on the generic path
FUSED_UPDATE_MLP = os.environ.get('CWN_FUSED_UPDATE_MLP') != '0'   # False: the update / combine networks as three grouped GEMM launches
BLOCKED_TRAIN_FORWARD = os.environ.get('CWN_BLOCKED_TRAIN_FORWARD') != '0'    # the training forward through the blocked kernel too
BLOCKED_LAYER = os.environ.get('CWN_BLOCKED_LAYER') != '0'   # False: propagate scope as grouped GEMM + CSR aggregation
# False: the dense parts of a float64 model (SparseCINConv's update / combine networks, the message products, the head's
# lin1s / lin2) as torch modules -- a rocBLAS dgemm, a bias add and an activation launch per Linear -- instead of the
# csrc/cwn_dense_f64.hip launches
FUSED_F64_DENSE = os.environ.get('CWN_FUSED_F64_DENSE') != '0'
# The update / combine networks of a float32 SparseCINConv layer in inference as ONE cwn_update_chain_f32 launch
# (csrc/cwn_chain_f32.hip: any width up to 128, any of the five activations) where cwn_update_mlp_f32 -- 64 / 128 with ReLU --
# does not serve them.  A set of regimes:
#   'relu_width'  ReLU networks at a width other than 64 / 128, instead of a grouped GEMM launch per stage + the combine;
#   'act'         networks with elu / tanh / sigmoid / id at any width up to 128, instead of the torch modules.
# CWN_FUSED_CHAIN_F32=1 / =0: both / neither; unset: FUSED_CHAIN_F32_DEFAULT, which holds the regimes in which the route has
# measured faster than the one it replaces by more than the run-to-run spread of both (tools/bench_chain_f32.py,
# profiles/chain_f32.md) with the whole suite passing.  True / False are read as both / neither.
CHAIN_F32_REGIMES = frozenset({'relu_width', 'act'})
FUSED_CHAIN_F32_DEFAULT = frozenset({'relu_width', 'act'})


def _chain_f32_switch(value: Optional[str]):
    """The regimes CWN_FUSED_CHAIN_F32 = `value` turns on."""
    return {'0': frozenset(), '1': CHAIN_F32_REGIMES}.get(value, FUSED_CHAIN_F32_DEFAULT)


FUSED_CHAIN_F32 = _chain_f32_switch(os.environ.get('CWN_FUSED_CHAIN_F32'))


def _chain_f32_on(regime: str) -> bool:
    on = FUSED_CHAIN_F32
    return regime in on if isinstance(on, (set, frozenset)) else bool(on)
# The update / combine networks of a float32 CINppConv layer in inference -- three or four branches and the nb*H-wide
# combine -- as ONE cwn_update_branches_f32 launch (csrc/cwn_branches_f32.hip: any width up to 128, any of the five
# activations) where cwn_update_mlp3_f32 does not serve them.  A switch of its own, a set of regimes as FUSED_CHAIN_F32 is:
#   'relu_width'  ReLU networks that cwn_update_mlp3_f32 does not take -- a width other than 64 / 128, a first layer with
#                 F != H, four branches at any width -- instead of a grouped GEMM launch per stage + torch.cat + combine_nn;
#   'act'         networks with elu / tanh / sigmoid / id at any width up to 128, instead of the torch modules.
# CWN_FUSED_BRANCHES_F32=1 / =0: both / neither; unset: FUSED_BRANCHES_F32_DEFAULT, which holds the regimes in which the route
# has measured faster than the one it replaces by more than the run-to-run spread of both (tools/bench_branches_f32.py,
# profiles/branches_f32.md) with the whole suite passing.  True / False are read as both / neither.
BRANCHES_F32_REGIMES = frozenset({'relu_width', 'act'})
FUSED_BRANCHES_F32_DEFAULT = frozenset({'relu_width', 'act'})


def _branches_f32_switch(value: Optional[str]):
    """The regimes CWN_FUSED_BRANCHES_F32 = `value` turns on."""
    return {'0': frozenset(), '1': BRANCHES_F32_REGIMES}.get(value, FUSED_BRANCHES_F32_DEFAULT)


FUSED_BRANCHES_F32 = _branches_f32_switch(os.environ.get('CWN_FUSED_BRANCHES_F32'))


def _branches_f32_on(regime: str) -> bool:
    on = FUSED_BRANCHES_F32
    return regime in on if isinstance(on, (set, frozenset)) else bool(on)
CSR_REUSE = True              # blocked layer kernel: sort a batch's adjacencies once, later layers load the result
# One workgroup per item and one item per CU at a time: the blocked kernel wins while the items fit the chip
# a few times over (measured on ZINC-like batches, tools/range_of_use.sh, M cells/s blocked vs CSR path: 256
# complexes 646 vs 428, 512: 761 vs 588, 1024: 788 vs 759, 2048: 836 vs 900, 8192: 863 vs 981); beyond
# ~2600 items (two per complex) the two-kernel path's streaming wins.
BLOCKED_MAX_ITEMS = int(os.environ.get('CWN_BLOCKED_MAX_ITEMS', '2600'))
# Which form of the blocked kernel a launch takes (include/cwn_hip.h, cwn_layer_plan.variant): 'auto' = the 16-wave
# one-per-CU form while the items fit the chip once (TWO_PER_CU_MIN_ITEMS), the 8-wave two-per-CU form beyond that
# when every complex fits its smaller caps; '0' / '1' force one (A/B measurements, tests).
LAYER_VARIANT = os.environ.get('CWN_LAYER_VARIANT', 'auto')
# A complex beyond a workgroup's LDS (a molecule of more than ~44 atoms at width 128, ~115 at 64) is streamed by its own
# workgroup inside the blocked launch (BIG records) instead of sending the whole batch to the two-kernel path -- while
# such complexes are the exception (at most BIG_MAX_SHARE of the items: a batch of hub complexes IS the streaming case).
BIG_ITEMS = {'0': False, 'always': 'always'}.get(os.environ.get('CWN_BIG_ITEMS', '1'), True)   # 'always': skip the cost model below (tests, A/B)
BIG_MAX_SHARE = 0.25
TWO_PER_CU_MIN_ITEMS = int(os.environ.get('CWN_TWO_PER_CU_MIN_ITEMS', '256'))
def _streaming_pays(table, F: int) -> bool:
    """BIG records against sending the whole batch to the two-kernel path.  The launch lasts as long as its longest
    workgroup: a streamed complex takes ~0.07 us per staged row at width 128 (~0.035 at 64; a 200-atom molecule = 415
    rows ~ 30 us), the rest of the batch ~8.7 us per round of 256 items, and the two-kernel path ~1.9 x the blocked time
    of the same batch without its giants.  Calibrated on tools/big_items_bench.py (share of the all-small rate, streamed
    / two-kernel path): molhiv-512 with 5 % giants of 60 - 200 atoms 0.87 / 0.43, ZINC-512 0.77 / 0.67, ZINC-128 0.38 /
    0.54 -- the one case that keeps the two-kernel path: a launch of 9 us cannot hide a 30-us workgroup."""
    recs = table.big_records
    rows = max(int(r[I_TASK0 + T_N]) + int(r[I_CN]) for r in recs)
    t_big = (0.07 if F == 128 else 0.035) * rows
    rounds = max(1, -(-(table.n_items - table.n_big) // TWO_PER_CU_MIN_ITEMS))
    return t_big < 1.9 * 8.7 * rounds


def _mixed_wins(tm, table0, lower: int, F: int = 128) -> bool:
    """Two launches (two-per-CU form for the complexes that fit + 16-wave form for the rest) against one launch of the
    16-wave form for all: rounds as in _two_per_cu_wins, plus one launch boundary.  Measured on batches with the size
    spread of the real ZINC subset (9 - 38 atoms, tools/ab_mixed.sh; M cells/s mixed / 16-wave form with big items /
    two-kernel path): batch 512: 798 / 849 / 577 (the one-round second launch costs more than it saves), batch 2048:
    1054 / 954 / 851; batch 128 has one round either way: 558 / 558 / 325."""
    slots = TWO_PER_CU_MIN_ITEMS
    rounds = lambda n, per: -(-n // per) if n <= 2 * per else n / per      # (a partial LAST round of many costs its share)
    t1, t0 = tm.parts
    if t0.n_big and BIG_ITEMS != 'always' and not (BIG_ITEMS and _streaming_pays(t0, F)):
        return False
    mixed = 1.3 * rounds(t1.n_items, 2 * slots) + rounds(t0.n_items, slots) + 0.2
    alone = rounds(table0.n_items if table0 is not None else lower, slots) if table0 is not None else 2.0 * rounds(lower, slots)
    return mixed < alone


def _two_per_cu_wins(n0: int, n1: int) -> bool:
    """A launch of n0 items in the 16-wave form (256 at a time) against n1 items in the two-per-CU form (512 at a
    time, each ~1.3 x as long: 8 waves, a neighbour on the CU): whole rounds while a launch is a few rounds (the last
    round costs as much as a full one), the ratio beyond.  Calibrated on tools/ab_variant.sh (M cells/s, 16-wave /
    two-per-CU): ZINC 160 complexes 555 / 639, 192: 649 / 744, 256: 756 / 905, 384: 844 / 1009; molhiv 256: 1351 /
    1575, 512: 2143 / 1974 (445 items in two rounds against 677 in two longer ones: the one case the 16-wave form
    keeps), 1024: 2354 / 2550, 2048: 2603 / 2905."""
    slots = TWO_PER_CU_MIN_ITEMS                       # = CUs
    r0 = -(-n0 // slots) if n0 <= 4 * slots else n0 / slots
    r1 = -(-n1 // (2 * slots)) if n1 <= 8 * slots else n1 / (2 * slots)
    return 1.3 * r1 < r0


class ByModule:
    """A mapping keyed by a module's IDENTITY that forgets a module when it dies -- weakref.WeakKeyDictionary's job at a plain
    dict's price: `get` there builds a weak reference per call (~0.7 us; five look-ups per layer of an eager forward).  An
    entry holds a weak reference with a callback of its own, so a recycled id() never answers for another module."""

    def __init__(self):
        self._d = {}

    def get(self, module, default=None):
        hit = self._d.get(id(module))
        return hit[1] if hit is not None and hit[0]() is module else default

    def __contains__(self, module) -> bool:
        hit = self._d.get(id(module))
        return hit is not None and hit[0]() is module

    def __getitem__(self, module):
        hit = self._d.get(id(module))
        if hit is None or hit[0]() is not module:
            raise KeyError(module)
        return hit[1]

    def __setitem__(self, module, value) -> None:
        key = id(module)
        self._d[key] = (weakref.ref(module, lambda _r, k=key, d=self._d: d.pop(k, None) if (d.get(k) or (None,))[0] is _r else None), value)

    def __delitem__(self, module) -> None:
        if module not in self:
            raise KeyError(module)
        del self._d[id(module)]

    def pop(self, module, *default):
        if module in self:
            return self._d.pop(id(module))[1]
        if default:
            return default[0]
        raise KeyError(module)

    def setdefault(self, module, default):
        if module not in self:
            self[module] = default
        return self._d[id(module)][1]

    def __len__(self) -> int:
        return len(self._d)

    def clear(self) -> None:
        self._d.clear()

    def values(self):
        return [v for _r, v in self._d.values()]


# prepared launches per (layer module, batch): kept OUTSIDE the modules (ctypes records do not deepcopy / pickle)
_BLOCKED_CACHE = ByModule()
_MLP_CACHE = ByModule()            # layer module -> (ops.MlpLaunch, (start, dims, outputs), BatchNorm modules)
_CHAIN_CACHE = ByModule()          # layer module -> {regime: (ops.ChainLaunch or None: declined, (start, dims), BatchNorm modules, STRUCT_EPOCH)}
_BRANCHES_CACHE = ByModule()       # CINppConv module -> {regime: (ops.BranchesLaunch or None: declined, (start, dims), BatchNorm modules, STRUCT_EPOCH)}
FUSED_OGB_FRONT = os.environ.get('CWN_FUSED_OGB_FRONT', '1') != '0'      # (A/B: '0' = the separate launches of the OGB encoders' front)
_FRONT_CACHE = ByModule()          # embedding front module -> {id(boundary_index_1): (ops.FrontLaunch, (rings?, reduce))}


def _ffi_dyn() -> bool:
    from . import _ffi
    return bool(_ffi.DYN_ROWS)


def _fold_norm(norm, width: int):
    """Eval-mode normalisation as a per-column affine (scale, shift) for the GEMM epilogue:
    BatchNorm1d with running statistics -> (w / sqrt(rv + eps), b - rm * scale); Identity ->
    (None, None).  Cached on the module and refreshed when any of its tensors changes.
    Returns None when the module cannot be folded (LayerNorm, BatchNorm without running stats)."""
    if isinstance(norm, torch.nn.Identity):
        return (None, None)
    if (not isinstance(norm, BN) or norm.training or norm.running_mean is None
            or norm.num_features != width):
        return None     # batch statistics (training) are not a fixed affine
    # (num_batches_tracked: torch's native batch_norm writes the running statistics of a TRAINING-mode forward without moving
    # their version counters; the module's own `num_batches_tracked.add_(1)` does move one -- found by tools/fuzz_round5.py in
    # round 5: an eval forward after a training-mode forward through the torch modules folded the OLD statistics)
    tensors = [t for t in (norm.weight, norm.bias, norm.running_mean, norm.running_var, norm.num_batches_tracked) if t is not None]
    key = (ops.STATE_EPOCH,) + tuple((t.data_ptr(), ops._ffi.tver(t)) for t in tensors)
    hit = getattr(norm, '_cwn_fold', None)
    if hit is not None and hit[0] == key:
        return hit[1]
    with torch.no_grad():
        scale = torch.rsqrt(norm.running_var + norm.eps)
        if norm.weight is not None:
            scale = scale * norm.weight
        shift = -norm.running_mean * scale
        if norm.bias is not None:
            shift = shift + norm.bias
        fold = (scale.contiguous(), shift.contiguous())
    norm._cwn_fold = (key, fold)
    return fold


def _f64_stages(nn, groups: int):
    """([(Linear, norm), ...], activation name) of a stock Sequential of `groups` (Linear, norm, act) groups whose
    activation modules are all the same one of the five of models.get_nonlinearity, or None."""
    if not isinstance(nn, Sequential) or len(nn) != 3 * groups:
        return None
    stages, acts = [], set()
    for i in range(0, len(nn), 3):
        lin, norm, act = nn[i], nn[i + 1], nn[i + 2]
        name = _act_name(act)
        if type(lin) is not Linear or name is None:
            return None
        stages.append((lin, norm))
        acts.add(name)
    return (stages, acts.pop()) if len(acts) == 1 else None


def _mlp_stages(nn):
    """[(Linear, norm), ...] of a Sequential of (Linear, norm, ReLU) groups, or None."""
    if not isinstance(nn, Sequential) or len(nn) % 3 != 0 or len(nn) == 0:
        return None
    stages = []
    for i in range(0, len(nn), 3):
        lin, norm, act = nn[i], nn[i + 1], nn[i + 2]
        if not (isinstance(lin, Linear) and isinstance(act, ReLU)):
            return None
        stages.append((lin, norm))
    return stages


def _combine_folds(combine):
    """[dim] -> `_fold_norm` of a combine network that is one stage, or None when some dimension's is another form."""
    if any(cb is None or len(cb) != 1 for cb in combine):
        return None
    folds = [_fold_norm(cb[0][1], cb[0][0].out_features) for cb in combine]
    return None if any(f is None for f in folds) else folds


# ------------------------------------------------------------------------------------------------
# test / toy layers
# ------------------------------------------------------------------------------------------------
class DummyCochainMessagePassing(CochainMessagePassing):
    """Parameter-free layer used by the reference's tests (mp/layers.py:14-40): messages are
    x_j + attr.  Fused here as CWN_MSG_A_PLUS_B."""

    def __init__(self, up_msg_size, down_msg_size, boundary_msg_size=None, use_boundary_msg=False,
                 use_down_msg=True):
        super().__init__(up_msg_size, down_msg_size, boundary_msg_size=boundary_msg_size,
                         use_boundary_msg=use_boundary_msg, use_down_msg=use_down_msg)

    def message_up(self, up_x_j: Tensor, up_attr: Tensor) -> Tensor:
        return up_x_j + up_attr

    def message_down(self, down_x_j: Tensor, down_attr: Tensor) -> Tensor:
        return down_x_j + down_attr

    def message_and_aggregate_up(self, up_adj_t: Adjacency, x, up_attr) -> Tensor:
        B, mode = _attr_operand(up_attr)
        return ops.aggregate(up_adj_t, up_adj_t.n_dst, x, msg_op=ops.MSG_A_PLUS_B, B=B, ib_mode=mode,
                             reduce=self.aggr_up)

    def message_and_aggregate_down(self, down_adj_t: Adjacency, x, down_attr) -> Tensor:
        B, mode = _attr_operand(down_attr)
        return ops.aggregate(down_adj_t, down_adj_t.n_dst, x, msg_op=ops.MSG_A_PLUS_B, B=B,
                             ib_mode=mode, reduce=self.aggr_down)

    def forward(self, cochain: CochainMessagePassingParams):
        up_out, down_out, boundary_out = self.propagate(
            cochain.up_index, cochain.down_index, cochain.boundary_index, x=cochain.x,
            up_attr=cochain.kwargs['up_attr'], down_attr=cochain.kwargs['down_attr'],
            boundary_attr=cochain.kwargs['boundary_attr'])
        return cochain.x + up_out + down_out + boundary_out


class DummyCellularMessagePassing(torch.nn.Module):
    """mp/layers.py:43-59."""

    def __init__(self, input_dim=1, max_dim: int = 2, use_boundary_msg=False, use_down_msg=True):
        super().__init__()
        self.max_dim = max_dim
        self.mp_levels = torch.nn.ModuleList(
            DummyCochainMessagePassing(input_dim, input_dim, boundary_msg_size=input_dim,
                                       use_boundary_msg=use_boundary_msg, use_down_msg=use_down_msg)
            for _ in range(max_dim + 1))

    def forward(self, *cochain_params: CochainMessagePassingParams):
        assert len(cochain_params) <= self.max_dim + 1
        return [self.mp_levels[d].forward(cochain_params[d]) for d in range(len(cochain_params))]


# ------------------------------------------------------------------------------------------------
# CIN (upper + lower adjacencies, per-message networks)
# ------------------------------------------------------------------------------------------------
class CINCochainConv(CochainMessagePassing):
    """mp/layers.py:62-103.  The message networks are arbitrary callables on cat(x_j, attr): in
    general they run on the generic path (gather kernel -> network -> segmented-reduce kernel);
    the Linear -> ReLU -> BatchNorm form the reference's models build (mp/models.py:40-47) has a
    fused inference path (_fused_inference)."""

    def __init__(self, up_msg_size: int, down_msg_size: int, msg_up_nn: Callable,
                 msg_down_nn: Callable, update_nn: Callable, eps: float = 0., train_eps: bool = False):
        super().__init__(up_msg_size, down_msg_size, use_boundary_msg=False)
        self.msg_up_nn = msg_up_nn
        self.msg_down_nn = msg_down_nn
        self.update_nn = update_nn
        self.initial_eps = eps
        if train_eps:
            self.eps = torch.nn.Parameter(torch.Tensor([eps]))
        else:
            self.register_buffer('eps', torch.Tensor([eps]))
        self.reset_parameters()

    def forward(self, cochain: CochainMessagePassingParams):
        fused = self._fused_inference(cochain)
        if fused is None:
            fused = self._fused_training(cochain)
        if fused is not None:
            return self.update_nn(fused)
        out_up, out_down, _ = self.propagate(cochain.up_index, cochain.down_index, None, x=cochain.x,
                                             up_attr=cochain.kwargs['up_attr'],
                                             down_attr=cochain.kwargs['down_attr'])
        out_up = out_up + (1 + self.eps) * cochain.x
        out_down = out_down + (1 + self.eps) * cochain.x
        return self.update_nn(out_up + out_down)

    # ---- fused inference -------------------------------------------------------------------------
    @staticmethod
    def _message_form(nn):
        """(Linear, (scale, shift) | None) when `nn` is Linear -> ReLU [-> BatchNorm1d(eval) | Identity]
        (the conv_up / conv_down of mp/models.py:40-47), else None."""
        if not isinstance(nn, Sequential) or len(nn) not in (2, 3):
            return None
        if not (isinstance(nn[0], Linear) and isinstance(nn[1], ReLU)):
            return None
        if len(nn) == 2:
            return nn[0], (None, None)
        fold = _fold_norm(nn[2], nn[0].out_features)
        return None if fold is None else (nn[0], fold)

    def _fused_plan(self, cochain: CochainMessagePassingParams):
        """The dense products and aggregation streams of _fused_inference, unlaunched (CINConv
        groups the plans of all dimensions into one GEMM launch + one aggregation launch), or None
        when the fused path does not apply."""
        x = cochain.x
        if torch.is_grad_enabled() or x is None or not x.is_cuda or x.dtype != torch.float32:
            return None                  # (the products are fp32 MFMA GEMMs: float64 takes propagate() and the torch modules)
        if (self.aggr_up or 'add') != 'add' or (self.aggr_down or 'add') != 'add':
            return None
        n, F = x.size(0), x.size(1)
        jobs = []
        for index, name, attr, nn in ((cochain.up_index, 'up', cochain.kwargs.get('up_attr'), self.msg_up_nn),
                                      (cochain.down_index, 'down', cochain.kwargs.get('down_attr'), self.msg_down_nn)):
            if index is None or (name == 'down' and not self.use_down_msg):
                continue
            form = self._message_form(nn)
            if form is None or attr is None:
                return None
            lin = form[0]
            attr_src, mode = _attr_operand(attr)
            if lin.in_features != F + attr_src.size(1) or lin.out_features != F \
                    or max(F, attr_src.size(1)) > ops.GEMM_MAX_K:
                return None
            jobs.append((index, name, attr_src, mode, form))
        kw = dict(x=x, up_attr=cochain.kwargs.get('up_attr'), down_attr=cochain.kwargs.get('down_attr'))
        gemms, adjs = [], []
        for index, name, attr_src, mode, (lin, _) in jobs:
            gemms += [ops.Gemm(X=x, W=lin.weight, w_col0=0, bias=lin.bias),
                      ops.Gemm(X=attr_src, W=lin.weight, w_col0=F)]
            size = self.__check_input_separately__(index, None)
            adjs.append(self._adjacency(index, name, size, kw))
        return dict(x=x, jobs=jobs, gemms=gemms, adjs=adjs)

    def _fused_streams(self, plan, ys: List[Tensor]) -> List[ops.Stream]:
        x = plan['x']
        return [ops.Stream(adj=adj, n_dst=x.size(0), width=x.size(1), A=ys[2 * k], B=ys[2 * k + 1],
                           msg_op=ops.MSG_RELU_A_PLUS_B, ib_mode=job[3])
                for k, (job, adj) in enumerate(zip(plan['jobs'], plan['adjs']))]

    def _fused_finish(self, plan, outs: List[Tensor]) -> Tensor:
        """out_up + out_down (with both self terms) from the aggregated ReLU sums."""
        total = (2 * (1 + self.eps)) * plan['x']
        for out, adj, job in zip(outs, plan['adjs'], plan['jobs']):
            scale, shift = job[4][1]
            if scale is None:
                total = total + out
            else:
                deg = (adj.rowptr[1:] - adj.rowptr[:-1]).to(out.dtype).unsqueeze(1)
                total = total + out * scale + deg * shift
        return total

    def _fused_inference(self, cochain: CochainMessagePassingParams) -> Optional[Tensor]:
        """out_up + out_down of forward() without materialising a message, when nothing needs a
        gradient and both message networks are Linear -> ReLU -> BatchNorm(eval).  The per-ENTRY
        network splits exactly:  BN(relu(W [x_j | a_e] + b)) = s * relu(Y1[j] + Y2[c]) + t  with
        Y1 = X W[:, :F]^T + b, Y2 = X_attr W[:, F:]^T computed once per CELL, so
            sum_e msg_e = s * (sum_e relu(Y1[j_e] + Y2[c_e])) + deg_i * t
        -- one grouped GEMM launch and one aggregation launch for both adjacencies.  Returns None
        when it does not apply (training, other network shapes, CPU tensors)."""
        plan = self._fused_plan(cochain)
        if plan is None:
            return None
        ys = ops.run_gemm(plan['gemms'], plan['x'].device) if plan['gemms'] else []
        streams = self._fused_streams(plan, ys)
        outs = ops.aggregate_many(streams) if streams else []
        return self._fused_finish(plan, outs)

    # ---- fused training (round 4) ----------------------------------------------------------------
    @staticmethod
    def _message_form_train(nn):
        """(Linear, norm | None) when `nn` is Linear -> ReLU [-> BatchNorm1d | Identity] in a state the fused training path
        reproduces, else None."""
        if not isinstance(nn, Sequential) or len(nn) not in (2, 3):
            return None
        if not (isinstance(nn[0], Linear) and isinstance(nn[1], ReLU)):
            return None
        norm = nn[2] if len(nn) == 3 else None
        if norm is None or isinstance(norm, torch.nn.Identity):
            return nn[0], None
        if not isinstance(norm, BN) or norm.num_features != nn[0].out_features:
            return None
        if norm.training and norm.track_running_stats and norm.momentum is None:
            return None                  # (cumulative moving average: not restated)
        if not norm.training and norm.running_mean is None:
            return None
        return nn[0], norm

    def _fused_training(self, cochain: CochainMessagePassingParams) -> Optional[Tensor]:
        """out_up + out_down of forward() WITH autograd and without a message ever materialised, for the
        message networks the reference's models build (mp/models.py:40-47: Linear -> ReLU -> BatchNorm).  The split of
        _fused_inference holds in training too -- relu(W [x_j | a_e] + b) = relu(Y1[j] + Y2[c]), Y1 / Y2 once per CELL on
        the MFMA kernel (ops.gemm_many: differentiable) -- and BatchNorm in TRAINING mode normalises over the ENTRIES of
        the adjacency, whose batch statistics are column sums of two aggregations:
            S_i = sum_{e -> i} r_e (CWN_MSG_RELU_A_PLUS_B),   Q_i = sum_{e -> i} r_e^2 (CWN_MSG_RELU_A_PLUS_B_SQ)
            mean = sum_i S_i / E,  var = sum_i Q_i / E - mean^2 (float64),   sum_e BN(r_e) = scale S_i + deg_i shift
        with the running statistics updated as torch does (momentum, unbiased variance).  Gradients: autograd over these
        few [n, F] tensor ops + the aggregations' own transposed launches (the squared form's is CWN_MSG_A_TIMES_2RELU).
        Per adjacency: 1 grouped GEMM + 1 aggregation launch (both sums) forward, against gather -> per-entry Linear ->
        ReLU -> BatchNorm -> scatter over E x 2F / E x F matrices.  None when it does not apply."""
        x = cochain.x
        if (not FUSED_CIN_TRAINING or not torch.is_grad_enabled() or x is None or not x.is_cuda or x.dtype != torch.float32
                or x.dim() != 2):
            return None
        if (self.aggr_up or 'add') != 'add' or (self.aggr_down or 'add') != 'add':
            return None
        n, F = x.size(0), x.size(1)
        jobs = []
        for index, name, attr, nn in ((cochain.up_index, 'up', cochain.kwargs.get('up_attr'), self.msg_up_nn),
                                      (cochain.down_index, 'down', cochain.kwargs.get('down_attr'), self.msg_down_nn)):
            if index is None or (name == 'down' and not self.use_down_msg):
                continue
            form = self._message_form_train(nn)
            if form is None or attr is None:
                return None
            lin, norm = form
            attr_src, mode = _attr_operand(attr)
            if lin.in_features != F + attr_src.size(1) or lin.out_features != F or max(F, attr_src.size(1)) > ops.GEMM_MAX_K:
                return None
            E = int(index.size(1))
            if isinstance(norm, BN) and norm.training and E < 2:
                return None              # (torch refuses BatchNorm over fewer than two values per channel: let it)
            jobs.append((index, name, attr_src, mode, lin, norm, E))
        kw = dict(x=x, up_attr=cochain.kwargs.get('up_attr'), down_attr=cochain.kwargs.get('down_attr'))
        total = (2 * (1 + self.eps)) * x
        if not jobs:
            return total
        gemms = []
        for index, name, attr_src, mode, lin, norm, E in jobs:
            gemms += [ops.Gemm(X=x, W=lin.weight, w_col0=0, bias=lin.bias), ops.Gemm(X=attr_src, W=lin.weight, w_col0=F)]
        ys = ops.gemm_many(gemms)
        streams, adjs = [], []
        for k, (index, name, attr_src, mode, lin, norm, E) in enumerate(jobs):
            size = self.__check_input_separately__(index, None)
            adj = self._adjacency(index, name, size, kw)
            adjs.append(adj)
            streams.append(ops.Stream(adj=adj, n_dst=n, width=F, A=ys[2 * k], B=ys[2 * k + 1], msg_op=ops.MSG_RELU_A_PLUS_B,
                                      ib_mode=mode))
            if isinstance(norm, BN) and norm.training:
                streams.append(ops.Stream(adj=adj, n_dst=n, width=F, A=ys[2 * k], B=ys[2 * k + 1],
                                          msg_op=ops.MSG_RELU_A_PLUS_B_SQ, ib_mode=mode))
        outs = ops.aggregate_many(streams)
        o = 0
        for (index, name, attr_src, mode, lin, norm, E), adj in zip(jobs, adjs):
            S = outs[o]
            o += 1
            if norm is None:
                total = total + S
                continue
            deg = (adj.rowptr[1:] - adj.rowptr[:-1]).to(S.dtype).unsqueeze(1)
            w = norm.weight.double() if norm.weight is not None else None
            if norm.training:
                Q = outs[o]
                o += 1
                mean = S.sum(0, dtype=torch.float64) / E
                var = (Q.sum(0, dtype=torch.float64) / E - mean * mean).clamp_min(0.0)      # biased, as BatchNorm normalises
                if norm.track_running_stats and norm.running_mean is not None:
                    with torch.no_grad():
                        m = float(norm.momentum)
                        norm.running_mean.mul_(1 - m).add_(mean.to(norm.running_mean.dtype), alpha=m)
                        norm.running_var.mul_(1 - m).add_((var * (E / (E - 1))).to(norm.running_var.dtype), alpha=m)
                        norm.num_batches_tracked += 1
            else:
                mean, var = norm.running_mean.double(), norm.running_var.double()
            scale = torch.rsqrt(var + norm.eps)
            if w is not None:
                scale = scale * w
            shift = -mean * scale
            if norm.bias is not None:
                shift = shift + norm.bias.double()
            total = total + S * scale.float() + deg * shift.float()
        return total

    def reset_parameters(self):
        reset(self.msg_up_nn)
        reset(self.msg_down_nn)
        reset(self.update_nn)
        self.eps.data.fill_(self.initial_eps)

    def message_up(self, up_x_j: Tensor, up_attr: Tensor) -> Tensor:
        if up_attr is not None:
            return self.msg_up_nn(torch.cat([up_x_j, up_attr], dim=-1))
        return self.msg_up_nn(up_x_j)

    def message_down(self, down_x_j: Tensor, down_attr: Tensor) -> Tensor:
        return self.msg_down_nn(torch.cat([down_x_j, down_attr], dim=-1))


class CINConv(torch.nn.Module):
    """mp/layers.py:106-124."""

    def __init__(self, up_msg_size: int, down_msg_size: int, msg_up_nn: Callable,
                 msg_down_nn: Callable, update_nn: Callable, eps: float = 0.,
                 train_eps: bool = False, max_dim: int = 2):
        super().__init__()
        self.max_dim = max_dim
        self.mp_levels = torch.nn.ModuleList(
            CINCochainConv(up_msg_size, down_msg_size, msg_up_nn, msg_down_nn, update_nn, eps, train_eps)
            for _ in range(max_dim + 1))

    def forward(self, *cochain_params: CochainMessagePassingParams):
        assert len(cochain_params) <= self.max_dim + 1
        n = len(cochain_params)
        # inference: the fused plans of ALL dimensions in one GEMM launch (per <= 8) + one aggregation
        plans = [self.mp_levels[d]._fused_plan(cochain_params[d]) for d in range(n)]
        if all(p is not None for p in plans):
            gemms = [gm for p in plans for gm in p['gemms']]
            ys = ops.run_gemm(gemms, cochain_params[0].x.device) if gemms else []
            streams, k = [], 0
            for d, p in enumerate(plans):
                m = len(p['gemms'])
                streams.append(self.mp_levels[d]._fused_streams(p, ys[k:k + m]))
                k += m
            flat = [st for sts in streams for st in sts]
            outs = ops.aggregate_many(flat) if flat else []
            res, k = [], 0
            for d, (p, sts) in enumerate(zip(plans, streams)):
                lvl = self.mp_levels[d]
                res.append(lvl.update_nn(lvl._fused_finish(p, outs[k:k + len(sts)])))
                k += len(sts)
            return res
        return [self.mp_levels[d].forward(cochain_params[d]) for d in range(n)]


class EdgeCINConv(torch.nn.Module):
    """mp/layers.py:127-151: CIN up to 1-cells."""

    def __init__(self, up_msg_size: int, down_msg_size: int, v_msg_up_nn: Callable,
                 e_msg_down_nn: Callable, e_msg_up_nn: Callable, v_update_nn: Callable,
                 e_update_nn: Callable, eps: float = 0., train_eps=False):
        super().__init__()
        self.max_dim = 1
        self.mp_levels = torch.nn.ModuleList([
            CINCochainConv(up_msg_size, down_msg_size, v_msg_up_nn, lambda *args: None, v_update_nn,
                           eps, train_eps),
            CINCochainConv(up_msg_size, down_msg_size, e_msg_up_nn, e_msg_down_nn, e_update_nn, eps,
                           train_eps)])

    def forward(self, *cochain_params: CochainMessagePassingParams):
        assert len(cochain_params) <= self.max_dim + 1
        return [self.mp_levels[d].forward(cochain_params[d]) for d in range(len(cochain_params))]


# ------------------------------------------------------------------------------------------------
# SparseCIN (upper + boundary adjacencies): the flagship layer of the hot path
# ------------------------------------------------------------------------------------------------
class SparseCINCochainConv(CochainMessagePassing):
    """mp/layers.py:154-214."""

    def __init__(self, dim: int, up_msg_size: int, down_msg_size: int,
                 boundary_msg_size: Optional[int], msg_up_nn: Callable, msg_boundaries_nn: Callable,
                 update_up_nn: Callable, update_boundaries_nn: Callable, combine_nn: Callable,
                 eps: float = 0., train_eps: bool = False):
        super().__init__(up_msg_size, down_msg_size, boundary_msg_size=boundary_msg_size,
                         use_down_msg=False)
        self.dim = dim
        self.msg_up_nn = msg_up_nn
        self.msg_boundaries_nn = msg_boundaries_nn
        self.update_up_nn = update_up_nn
        self.update_boundaries_nn = update_boundaries_nn
        self.combine_nn = combine_nn
        self.initial_eps = eps
        if train_eps:
            self.eps1 = torch.nn.Parameter(torch.Tensor([eps]))
            self.eps2 = torch.nn.Parameter(torch.Tensor([eps]))
        else:
            self.register_buffer('eps1', torch.Tensor([eps]))
            self.register_buffer('eps2', torch.Tensor([eps]))
        self.reset_parameters()

    def reset_parameters(self):
        reset(self.msg_up_nn)
        reset(self.msg_boundaries_nn)
        reset(self.update_up_nn)
        reset(self.update_boundaries_nn)
        reset(self.combine_nn)
        self.eps1.data.fill_(self.initial_eps)
        self.eps2.data.fill_(self.initial_eps)

    # ---- hooks (generic path, and what the reference's tests call) -----------------------------
    def message_up(self, up_x_j: Tensor, up_attr: Tensor) -> Tensor:
        return self.msg_up_nn((up_x_j, up_attr))

    def message_boundary(self, boundary_x_j: Tensor) -> Tensor:
        return self.msg_boundaries_nn(boundary_x_j)

    # ---- fused forms -----------------------------------------------------------------------------
    def _up_kind(self) -> str:
        if isinstance(self.msg_up_nn, FirstOf):
            return 'first'
        if _is_cat_linear_relu(self.msg_up_nn):
            return 'cat_linear_relu'
        # the same split behind another activation: a launch without a device-side row count, whose backward
        # (cwn_aggregate_act_bwd_f32 / _f64) is behind a switch of its own, so a static batch -- and, unless
        # ops.ACT_MESSAGE_BACKWARD is on, a recording autograd -- see the 'custom' network they saw before
        if (FUSED_ACT_MESSAGE and (ops.ACT_MESSAGE_BACKWARD or not torch.is_grad_enabled()) and not _ffi_dyn()
                and _cat_linear_act(self.msg_up_nn) is not None and _act_message_on(self.msg_up_nn[1].weight.dtype)):
            return 'cat_linear_act'
        return 'custom'

    def gemm_specs(self, cochain: CochainMessagePassingParams) -> List[ops.Gemm]:
        """The dense products the fused coboundary message needs: Y1 = X_d W[:, :F]^T + b and
        Y2 = X_{d+1} W[:, F:]^T ([] when the message network is another form or there is no upper
        adjacency).  SparseCINConv groups the specs of all dimensions into one MFMA launch."""
        x, up_attr = cochain.x, cochain.kwargs.get('up_attr')
        if (cochain.up_index is None or up_attr is None or self._up_kind() not in ('cat_linear_relu', 'cat_linear_act')
                or (self.aggr_up or 'add') != 'add' or x.dtype != torch.float32):
            return []                    # (float64: _torch_products, behind the same fused stream)
        lin = self.msg_up_nn[1]
        F = x.size(1)
        attr_src, _ = _attr_operand(up_attr)
        if lin.in_features != F + attr_src.size(1) or max(F, attr_src.size(1)) > ops.GEMM_MAX_K:
            return []
        # (column ranges of the one weight: autograd sees the Parameter itself, not two slices)
        return [ops.Gemm(X=x, W=lin.weight, w_col0=0, bias=lin.bias),
                ops.Gemm(X=attr_src, W=lin.weight, w_col0=F)]

    def _up_stream(self, adj: Adjacency, x: Tensor, up_attr, self_x=None, eps=None,
                   ys: Optional[List[Tensor]] = None) -> Optional[ops.Stream]:
        """The upper-adjacency aggregation as one fused stream, or None when the message network
        is not a recognised form.  `ys` = precomputed [Y1, Y2] of gemm_specs()."""
        kind = self._up_kind()
        if kind == 'first':
            return ops.Stream(adj=adj, n_dst=adj.n_dst, width=int(x.size(1)), A=x, self_x=self_x,
                              eps=eps, reduce=self.aggr_up or 'add')
        if kind in ('cat_linear_relu', 'cat_linear_act') and up_attr is not None and (self.aggr_up or 'add') == 'add':
            relu = kind == 'cat_linear_relu'
            if ys is None:
                specs = SparseCINCochainConv.gemm_specs(self, CochainMessagePassingParams(x, adj, up_attr=up_attr))
                ys = ops.gemm_many(specs) if specs else _torch_products(self.msg_up_nn[1], x, up_attr, part_of_message=not relu)
                if ys is None:
                    return None
            _, mode = _attr_operand(up_attr)
            if relu:
                return ops.Stream(adj=adj, n_dst=adj.n_dst, width=int(ys[0].size(1)), A=ys[0], B=ys[1],
                                  msg_op=ops.MSG_RELU_A_PLUS_B, ib_mode=mode, self_x=self_x, eps=eps)
            # act(Y1[src] + Y2[shared]) summed: the stream of cwn_aggregate_act_f32 / _f64
            return ops.Stream(adj=adj, n_dst=adj.n_dst, width=int(ys[0].size(1)), A=ys[0], B=ys[1], msg_op=ops.MSG_A_PLUS_B,
                              act=_cat_linear_act(self.msg_up_nn), ib_mode=mode, self_x=self_x, eps=eps)
        return None

    def _boundary_fusable(self) -> bool:
        return isinstance(self.msg_boundaries_nn, Passthrough)

    def _boundary_eps(self):
        return self.eps2          # mp/layers.py:192 (CIN++ numbers its three eps differently, :252-254)

    def message_and_aggregate_up(self, up_adj_t: Adjacency, x, up_attr) -> Tensor:
        st = self._up_stream(up_adj_t, x, up_attr)
        if st is not None:
            return ops.aggregate_many([st])[0]
        # unrecognised message network: gather -> network -> segmented reduce
        x_j = ops.gather_rows(x, up_adj_t.val, lambda a=up_adj_t: a.t_src)
        msg = self.message_up(x_j, dense(up_attr))
        return ops.aggregate(up_adj_t, up_adj_t.n_dst, msg, ia_mode='perm', reduce=self.aggr_up or 'add')

    def message_and_aggregate_boundary(self, boundary_adj_t: Adjacency, boundary_attr) -> Tensor:
        if self._boundary_fusable():
            return ops.aggregate(boundary_adj_t, boundary_adj_t.n_dst, boundary_attr,
                                 reduce=self.aggr_boundary or 'add')
        x_j = ops.gather_rows(boundary_attr, boundary_adj_t.val, lambda a=boundary_adj_t: a.t_src)
        return ops.aggregate(boundary_adj_t, boundary_adj_t.n_dst, self.message_boundary(x_j),
                             ia_mode='perm', reduce=self.aggr_boundary or 'add')

    # ---- forward, split so that SparseCINConv can batch all dimensions into one launch ------------
    def streams(self, cochain: CochainMessagePassingParams,
                ys: Optional[List[Tensor]] = None) -> Optional[List[ops.Stream]]:
        """[upper stream, boundary stream] with the self terms folded in, or None when a message
        network is not fusable (the caller then uses `forward_unfused`)."""
        x = cochain.x
        n, dev = x.size(0), x.device
        up_attr, b_attr = cochain.kwargs.get('up_attr'), cochain.kwargs.get('boundary_attr')
        kw = dict(x=x, up_attr=up_attr, boundary_attr=b_attr)
        if cochain.up_index is not None:
            size = self.__check_input_separately__(cochain.up_index, None)
            up = self._up_stream(self._adjacency(cochain.up_index, 'up', size, kw), x, up_attr,
                                 self_x=x, eps=self.eps1, ys=ys)
            if up is None:
                return None
        else:
            up = ops.Stream(adj=None, n_dst=n, width=int(x.size(1)), self_x=x, eps=self.eps1)
        if self.use_boundary_msg and b_attr is not None:
            if not self._boundary_fusable() or cochain.boundary_index is None:
                return None
            size = self.__check_input_separately__(cochain.boundary_index, None)
            adj = self._adjacency(cochain.boundary_index, 'boundary', size, kw)
            bnd = ops.Stream(adj=adj, n_dst=n, width=int(b_attr.size(1)), A=b_attr, self_x=x,
                             eps=self._boundary_eps(), reduce=self.aggr_boundary or 'add')
        else:
            bnd = ops.Stream(adj=None, n_dst=n, width=int(x.size(1)), self_x=x, eps=self._boundary_eps())
        if up.width != x.size(1) or bnd.width != x.size(1):
            return None   # self term needs message width == feature width
        return [up, bnd]

    def finish(self, out_up: Tensor, out_boundaries: Tensor) -> Tensor:
        """mp/layers.py:193-199."""
        out_up = self.update_up_nn(out_up)
        out_boundaries = self.update_boundaries_nn(out_boundaries)
        return self.combine_nn(torch.cat([out_up, out_boundaries], dim=-1))

    def aggregate_unfused(self, cochain: CochainMessagePassingParams):
        """The two aggregated inputs of the update networks, self terms added, through propagate() (mp/layers.py:184-192)."""
        out_up, _, out_boundaries = self.propagate(cochain.up_index, cochain.down_index,
                                                   cochain.boundary_index, x=cochain.x,
                                                   up_attr=cochain.kwargs['up_attr'],
                                                   boundary_attr=cochain.kwargs['boundary_attr'])
        out_up = out_up + (1 + self.eps1) * cochain.x
        out_boundaries = out_boundaries + (1 + self.eps2) * cochain.x
        return out_up, out_boundaries

    def forward_unfused(self, cochain: CochainMessagePassingParams) -> Tensor:
        """The reference's own sequence (mp/layers.py:184-199) through propagate()."""
        return self.finish(*self.aggregate_unfused(cochain))

    def forward(self, cochain: CochainMessagePassingParams):
        sts = self.streams(cochain)
        if sts is None:
            return self.forward_unfused(cochain)
        out_up, out_boundaries = ops.aggregate_many(sts)
        return self.finish(out_up, out_boundaries)


def _torch_products(lin, x: Tensor, attr, part_of_message: bool = False) -> Optional[List[Tensor]]:
    """Y1 = X W[:, :F]^T + b and Y2 = X_attr W[:, F:]^T of an act(Linear(cat(x_j, attr))) message for features the fp32 MFMA
    GEMMs do not take (float64): the same split on torch.nn.functional.linear (rocBLAS), so that the message still runs as
    a fused stream -- in float64 -- and no per-entry matrix is materialised.  None when the split does not apply (float32
    features reach here only after gemm_specs has refused their shape).  `part_of_message`: the products of the activated
    message ('cat_linear_act') go to the launcher behind ops.linear_many_f64, not through the public function."""
    F = int(x.size(1))
    src, _ = _attr_operand(attr)
    if x.dtype != torch.float64 or lin.in_features != F + src.size(1):
        return None
    W = lin.weight
    if (FUSED_F64_DENSE and not torch.is_grad_enabled() and x.is_cuda and src.dtype == torch.float64 and W.dtype == torch.float64
            and max(F, int(src.size(1)), lin.out_features) <= ops._ffi.LINEAR_F64_MAX_WIDTH and x.dim() == src.dim() == 2):
        # inference: both products in one launch (csrc/cwn_dense_f64.hip), the weight read as its two column slices
        launch = ops._linear_many_f64 if part_of_message else ops.linear_many_f64
        return launch([(x.contiguous(), W[:, :F], lin.bias, None), (src.contiguous(), W[:, F:], None, None)])
    return [torch.nn.functional.linear(x, W[:, :F], lin.bias), torch.nn.functional.linear(src, W[:, F:])]


def _update_mlp(layer_dim, hidden, graph_norm, act_module):
    return Sequential(Linear(layer_dim, hidden), graph_norm(hidden), act_module(),
                      Linear(hidden, hidden), graph_norm(hidden), act_module())


class SparseCINConv(torch.nn.Module):
    """mp/layers.py:271-342.  Cellular GIN over upper neighbours and boundaries."""

    def __init__(self, up_msg_size: int, down_msg_size: int, boundary_msg_size: Optional[int],
                 passed_msg_up_nn: Optional[Callable], passed_msg_boundaries_nn: Optional[Callable],
                 passed_update_up_nn: Optional[Callable],
                 passed_update_boundaries_nn: Optional[Callable], eps: float = 0.,
                 train_eps: bool = False, max_dim: int = 2, graph_norm=BN, use_coboundaries=False,
                 **kwargs):
        super().__init__()
        self.max_dim = max_dim
        self.mp_levels = torch.nn.ModuleList()
        for dim in range(max_dim + 1):
            msg_up_nn = passed_msg_up_nn
            if msg_up_nn is None:
                if use_coboundaries:
                    msg_up_nn = Sequential(Catter(),
                                           Linear(kwargs['layer_dim'] * 2, kwargs['layer_dim']),
                                           kwargs['act_module']())
                else:
                    msg_up_nn = FirstOf()
            msg_boundaries_nn = passed_msg_boundaries_nn
            if msg_boundaries_nn is None:
                msg_boundaries_nn = Passthrough()
            update_up_nn = passed_update_up_nn
            if update_up_nn is None:
                update_up_nn = _update_mlp(kwargs['layer_dim'], kwargs['hidden'], graph_norm,
                                           kwargs['act_module'])
            update_boundaries_nn = passed_update_boundaries_nn
            if update_boundaries_nn is None:
                update_boundaries_nn = _update_mlp(kwargs['layer_dim'], kwargs['hidden'], graph_norm,
                                                   kwargs['act_module'])
            combine_nn = Sequential(Linear(kwargs['hidden'] * 2, kwargs['hidden']),
                                    graph_norm(kwargs['hidden']), kwargs['act_module']())
            self.mp_levels.append(SparseCINCochainConv(
                dim, up_msg_size, down_msg_size, boundary_msg_size=boundary_msg_size,
                msg_up_nn=msg_up_nn, msg_boundaries_nn=msg_boundaries_nn, update_up_nn=update_up_nn,
                update_boundaries_nn=update_boundaries_nn, combine_nn=combine_nn, eps=eps,
                train_eps=train_eps))

    def propagate_all(self, *cochain_params: CochainMessagePassingParams, start_to_process=0):
        """Everything `propagate` does for all dimensions of this layer (the 3 propagate calls of
        mp/layers.py:337-341, plus the self terms) in TWO launches: one grouped MFMA GEMM for the
        coboundary-message products, one fused aggregation.  Returns (plans, outs): plans[dim] is
        None for dimensions that are not fusable / not processed, outs holds (up, boundary) pairs
        of the fusable ones in order."""
        n = len(cochain_params)
        fused = self._propagate_blocked(cochain_params, start_to_process)
        if fused is not None:
            return ['blocked'] * n, fused
        # An activated message under a recording autograd (ops.ACT_MESSAGE_BACKWARD): its products are made by the level's
        # own `_up_stream` (ops.gemm_many / _torch_products, differentiable) and its stream goes through ops.aggregate_many --
        # not through the one node around the products and the aggregation, which has no backward for it, and so through
        # neither the blocked training forward nor the deferred weight gradients, which belong to that node.
        act_train = ops.ACT_MESSAGE_BACKWARD and torch.is_grad_enabled() and any(
            self.mp_levels[dim]._up_kind() == 'cat_linear_act' for dim in range(start_to_process, n))
        specs, owner = [], []
        for dim in range(start_to_process, n):
            sp = [] if act_train else self.mp_levels[dim].gemm_specs(cochain_params[dim])
            specs += sp
            owner += [dim] * len(sp)
        plans = [None] * n
        pre = self._propagate_blocked_train(cochain_params, start_to_process, specs, owner) if specs else None

        def make_streams(ys):
            # the forward has run as the blocked launch: the streams only DESCRIBE the step for the autograd node, and its
            # backward is the owner-form launch over its own item table -- the CSR plans of the adjacencies are built when
            # somebody reads them (csr.deferred_builds; ops.gemm_aggregate builds them at once when the backward will)
            from .csr import deferred_builds
            import contextlib
            with (deferred_builds() if pre is not None else contextlib.nullcontext()):
                for dim in range(start_to_process, n):
                    mine = [y for y, o in zip(ys, owner) if o == dim]
                    plans[dim] = self.mp_levels[dim].streams(cochain_params[dim], mine or None)
            return [st for p in plans if p is not None for st in p]

        if specs:       # (training: ONE autograd node around the products and the aggregation, ops._GemmAggregate)
            _, outs = ops.gemm_aggregate(specs, make_streams, precomputed=pre)
        else:
            fused = make_streams([])
            outs = ops.aggregate_many(fused) if fused else []
        return plans, outs

    def _propagate_blocked(self, cochain_params, start_to_process) -> Optional[List[Tensor]]:
        """The whole propagate scope of this layer in ONE launch (csrc/cwn_layer.hip): Y1 / Y2 on
        the matrix cores into LDS, the batch's COO entries sorted per complex in LDS, both
        aggregations and the self terms out of LDS; no CSR plan, nothing but the two output
        streams written.  Applies to the form the reference's molecular models build (coboundary
        message ReLU(Linear(cat(x_j, up_attr))), identity boundary message, 'add' everywhere,
        mp/layers.py:286-299) on a batch that carries its per-complex tables, without autograd;
        None otherwise (the caller then runs the grouped GEMM + CSR aggregation;
        `self.blocked_reason` says why)."""
        from . import _ffi
        n = len(cochain_params)
        plan = getattr(cochain_params[0], 'block_plan', None)
        ent = None
        if plan is not None and BLOCKED_LAYER and not ops.GEMM_EXACT and start_to_process == 0:
            # fast path: everything about (this layer, this batch) that does not change between calls was
            # checked and laid out once (`_blocked_args`); per call only identities and the features are looked at
            ckey = id(plan)
            ent = _BLOCKED_CACHE.get(self, {}).get(ckey)
            if ent is not None and not self._blocked_still_valid(ent, cochain_params):
                ent = None
        if ent is None:
            args = self._blocked_args(cochain_params, start_to_process)
            if isinstance(args, str):
                self.blocked_reason = args
                return None
            dims, plan, table, key = args
            ckey = id(plan)
            lins = [self.mp_levels[d].msg_up_nn[1] for d, D in enumerate(dims) if D.msg_w_packed is not None]
            ent = dict(plan=plan, table=table, key=key, F=int(dims[0].x.size(1)), epochs=(ops.STATE_EPOCH, ops.STRUCT_EPOCH),
                       idx=[(c.up_index, c.boundary_index, getattr(c.kwargs.get('up_attr'), 'index', None))
                            for c in cochain_params],
                       # the packed weights follow the message weights' versions; bias / eps are read in place (their addresses)
                       marks=ops._marks([t for lin in lins for t in (lin.weight, lin.bias)]
                                        + self._blocked_eps(n)),   # (no ModuleList slice: a new container moves STRUCT_EPOCH)
                       launch=ops.LayerLaunch(dims, table))
            cache = _BLOCKED_CACHE.setdefault(self, {})
            if len(cache) > 64:
                cache.clear()
            cache[ckey] = ent
        self.__dict__['blocked_reason'] = None        # (plain attributes: Module.__setattr__ costs ~1 us each, per layer per call)
        table, key = ent['table'], ent['key']
        # the layers of one forward share their index tensors (mp/molec_models.py:110-116): the first
        # launch on them stores every item's sorted adjacency, the following ones load it back
        mode = _ffi.LAYER_CSR_LOAD if (CSR_REUSE and table.csr_key == key) else (_ffi.LAYER_CSR_STORE if CSR_REUSE else 0)
        try:
            outs = ent['launch'].run([c.x for c in cochain_params], mode)
        except (ValueError, TypeError):
            # features of another shape / type than the prepared launch takes (its own check, in C++ when the compiled
            # binding runs it): the long way decides what serves them
            _BLOCKED_CACHE.get(self, {}).pop(id(ent['plan']), None)
            args = self._blocked_args(cochain_params, start_to_process)
            if isinstance(args, str):
                self.blocked_reason = args
                return None
            raise
        if mode == _ffi.LAYER_CSR_STORE:
            table.csr_key = key
        plan = ent['plan']
        if not plan.validated and not torch.cuda.is_current_stream_capturing():
            from . import csr
            csr.check_errors(cochain_params[0].x.device)     # once per batch: the table belongs to these index tensors
            plan.validated = True
        return outs

    def _propagate_blocked_train(self, cochain_params, start_to_process, specs, owner):
        """The TRAINING forward of the propagate step through the blocked layer kernel (CWN_LAYER_STORE_Y): one launch
        (+ one small launch per message weight to pack it) instead of the grouped GEMM + the aggregation, with Y1 / Y2
        written out for the backward pass, which stays on the CSR path (ops._GemmAggregate).  Returns (ys, outs) in the
        order of `specs` / of the streams, or None when the blocked form does not apply to (this layer, this batch)."""
        if not (BLOCKED_TRAIN_FORWARD and torch.is_grad_enabled() and ops.FUSED_PROPAGATE_NODE):
            return None
        n = len(cochain_params)
        if len(specs) != 2 * sum(1 for d in range(n) if owner.count(d) == 2) or any(owner.count(d) not in (0, 2) for d in range(n)):
            return None
        args = self._blocked_args(cochain_params, start_to_process, training=True)
        if isinstance(args, str):
            self.blocked_reason = args
            return None
        dims, plan, table, key = args
        if getattr(table, 'variant', 0) == 'mixed' or getattr(table, 'n_big', 0):
            return None                  # (two launches into the same outputs / streamed complexes: inference only)
        dev, F = dims[0].x.device, int(dims[0].x.size(1))
        ys_of = [[None, None] for _ in range(n)]
        ys, ydims = [], []
        for d in range(n):
            if owner.count(d) == 2:
                if d + 1 >= n:
                    return None
                y1 = torch.empty(dims[d].x.size(0), F, dtype=torch.float32, device=dev)
                y2 = torch.empty(dims[d + 1].x.size(0), F, dtype=torch.float32, device=dev)
                ys_of[d][0], ys_of[d + 1][1] = y1, y2
                ys += [y1, y2]
                ydims += [(d, 'y1'), (d + 1, 'y2')]
        from . import _ffi
        launch = ops.LayerLaunch(dims, table)
        # (the layers of one forward share their index tensors: the first launch stores every item's sorted adjacency,
        # the following ones load it back -- as in the inference path)
        mode = _ffi.LAYER_CSR_LOAD if (CSR_REUSE and table.csr_key == key) else (_ffi.LAYER_CSR_STORE if CSR_REUSE else 0)
        outs = launch.run([c.x.detach() for c in cochain_params], mode, ys=[tuple(p) for p in ys_of])
        if mode == _ffi.LAYER_CSR_STORE:
            table.csr_key = key
        if not plan.validated and not torch.cuda.is_current_stream_capturing():
            from . import csr
            csr.check_errors(dev)
            plan.validated = True
        self.blocked_reason = None
        bwd_table = None
        if ops.BLOCKED_BACKWARD == 2:               # the owner form of the backward launch cuts a table of its own
            bwd_table = plan.bwd_items(F, [D.up_index is not None and D.up_index.size(1) > 0 for D in dims],
                                       [D.b_index is not None for D in dims])
        return ys, outs, (dims, table, ydims, bwd_table)    # (the last: what the blocked BACKWARD launch needs, ops._GemmAggregate)

    def _blocked_still_valid(self, ent, cochain_params) -> bool:
        """The per-call part of `_blocked_args`: autograd state, feature tensors, lazy attributes, and the
        packed weights (re-packed when an optimizer step has bumped the weight's version)."""
        if torch.is_grad_enabled() and (any(p.requires_grad for p in self.parameters())
                                        or any(c.x.requires_grad for c in cochain_params)):
            return False
        n = len(cochain_params)
        if n != len(ent['idx']) or cochain_params[0].block_plan is not ent['plan']:
            return False
        if ent['epochs'] != (ops.STATE_EPOCH, ops.STRUCT_EPOCH):
            return False              # a training kernel wrote the parameters (ops.state_changed) / a module tree changed
        for d, c in enumerate(cochain_params):
            up, bi, sh = ent['idx'][d]
            kw = c.kwargs
            attr = kw.get('up_attr')
            if c.up_index is not up or c.boundary_index is not bi or getattr(attr, 'index', None) is not sh:
                return False          # other index tensors than the prepared launch points at
            if up is not None and (not isinstance(attr, IndexedRows) or d + 1 >= n or attr.src is not cochain_params[d + 1].x):
                return False
            b_attr = kw.get('boundary_attr')
            if b_attr is not None and (d == 0 or b_attr is not cochain_params[d - 1].x):
                return False
        # (the features' shape / type / device: the launch's own check -- LayerLaunch.run raises, _propagate_blocked falls back)
        return ops._marks_current(ent['marks'])   # weights changed: rebuild (re-pack) through _blocked_args

    def _blocked_args(self, cochain_params, start_to_process, training=False):
        if not BLOCKED_LAYER:
            return 'layers.BLOCKED_LAYER is off'
        if ops.GEMM_EXACT:
            return 'exact fp32 GEMMs requested (the blocked kernel has only the split form)'
        if start_to_process != 0:
            return 'start_to_process != 0'
        n = len(cochain_params)
        plan = getattr(cochain_params[0], 'block_plan', None)
        if plan is None:
            return 'the batch carries no per-complex tables (ptr / __slices__)'
        if n > 3 or n != plan.n_dims:
            return 'dimension count'
        if not training and torch.is_grad_enabled() and (any(p.requires_grad for p in self.parameters())
                                                         or any(c.x.requires_grad for c in cochain_params)):
            return 'autograd is recording (inference path only)'
        F = int(cochain_params[0].x.size(1))
        if F not in (64, 128):
            return f'feature width {F} (64 or 128)'
        dims, has_up = [], []
        for d, c in enumerate(cochain_params):
            lvl = self.mp_levels[d]
            x = c.x
            if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2 or x.size(1) != F:
                return f'dim {d}: features must be fp32 [n, {F}] on the GPU'
            if (lvl.aggr_up or 'add') != 'add' or (lvl.aggr_boundary or 'add') != 'add':
                return f'dim {d}: reduce is not add'
            if not lvl._boundary_fusable() or lvl.up_msg_size != F:
                return f'dim {d}: boundary message network / message width'
            D = ops.LayerDim(x=x, eps1=lvl.eps1, eps2=lvl._boundary_eps())
            why = self._blocked_dim_extra(D, lvl, c, d)       # (CIN++: the third output; a stream the launch does not have)
            if why is not None:
                return why
            up = c.up_index is not None and c.up_index.size(1) > 0
            if c.up_index is not None:
                attr = c.kwargs.get('up_attr')
                lin = lvl.msg_up_nn[1] if lvl._up_kind() == 'cat_linear_relu' else None
                if lin is None or lin.in_features != 2 * F or lin.out_features != F:
                    return f'dim {d}: message network is not ReLU(Linear(cat))'
                if not isinstance(attr, IndexedRows) or d + 1 >= n or attr.src is not cochain_params[d + 1].x:
                    return f'dim {d}: up_attr is not the lazy gather of the next dimension\'s features'
                D.up_index, D.up_shared = c.up_index, attr.index
                D.msg_w_packed, D.msg_bias = ops.pack_layer_weight(lin.weight, fresh=training), lin.bias
            b_index, b_attr = c.boundary_index, c.kwargs.get('boundary_attr')
            if lvl.use_boundary_msg and b_attr is not None:
                if b_index is None or d == 0 or b_attr is not cochain_params[d - 1].x:
                    return f'dim {d}: boundary_attr is not the previous dimension\'s features'
                D.b_index = b_index
            dims.append(D)
            has_up.append(bool(up))
        has_b = [D.b_index is not None for D in dims]
        # Tables are keyed on the streams THIS layer runs (a layer without the boundary stream must not get
        # records that carry boundary entries) and on the form of the kernel.  Beyond one item per CU the two-per-CU
        # form is taken when every complex fits its smaller caps: it beats the 16-wave form AND the streaming CSR path
        # at every size measured (tools/ab_variant.sh, M cells/s, two-per-CU / 16-wave / CSR: 512 complexes 1090 / 874 /
        # 582, 2048: 1273 / 994 / 837, 8192: 1207 / 960 / 905; at 128 complexes = 256 items 633 / 711 / 322).
        lower = plan.at_least(F, has_up, has_b)
        table = None
        if LAYER_VARIANT == '1':
            table = plan.items(F, has_up, has_b, variant=1)
        elif LAYER_VARIANT == 'auto' and lower > 4 * TWO_PER_CU_MIN_ITEMS:
            table = plan.items(F, has_up, has_b, variant=1)          # many rounds either way: two per CU (if every complex fits)
        if table is None and LAYER_VARIANT != '1' and lower > BLOCKED_MAX_ITEMS:
            # too many items for the 16-wave form alone: the two-per-CU form for whatever fits it + the rest (mixed), or
            # the streaming path
            tm = plan.items_mixed(F, has_up, has_b) if LAYER_VARIANT in ('auto', 'mixed') else None
            if tm is None or tm.parts[1].n_items > BLOCKED_MAX_ITEMS or (tm.parts[1].n_big and BIG_ITEMS != 'always' and not (
                    BIG_ITEMS and _streaming_pays(tm.parts[1], F))):
                return f'more than {BLOCKED_MAX_ITEMS} items: beyond the range where one workgroup per item beats the streaming CSR path'
            table = tm
        if table is None and LAYER_VARIANT != '1':
            table = plan.items(F, has_up, has_b)
            if table is not None and LAYER_VARIANT == 'auto' and table.n_items > TWO_PER_CU_MIN_ITEMS:
                t1 = plan.items(F, has_up, has_b, variant=1)
                if t1 is not None and _two_per_cu_wins(table.n_items, t1.n_items):
                    table = t1
        if LAYER_VARIANT in ('auto', 'mixed') and lower > TWO_PER_CU_MIN_ITEMS and (table is None or table.variant == 0) \
                and lower <= BLOCKED_MAX_ITEMS:
            # more items than CUs, but some complex is too large for the two-per-CU form (its 80 KiB hold ~30 atoms at
            # width 128): that form for the complexes that fit, the 16-wave form (BIG records where needed) for the
            # rest -- two launches into the same outputs (blockplan.MixedTable)
            tm = plan.items_mixed(F, has_up, has_b)
            if tm is not None and (LAYER_VARIANT == 'mixed' or _mixed_wins(tm, table, lower, F)):
                table = tm
        if table is None and LAYER_VARIANT != '1' and BIG_ITEMS and lower <= BLOCKED_MAX_ITEMS:
            # some complex does not fit a workgroup's LDS: ITS workgroup streams it (BIG records, include/cwn_hip.h), the
            # rest of the batch stays blocked -- unless most of the batch is like that (REDDIT-like hub complexes)
            t = plan.items(F, has_up, has_b, variant=0, allow_big=True)
            if t is not None and (BIG_ITEMS == 'always' or (t.n_big <= max(2, BIG_MAX_SHARE * t.n_items) and _streaming_pays(t, F))):
                table = t
        if table is None:
            return 'a complex does not fit one workgroup (row / entry caps)'
        if table.variant == 0 and table.n_items > BLOCKED_MAX_ITEMS:     # (a MixedTable's variant is 'mixed')
            return f'{table.n_items} items: beyond the range where one workgroup per item beats the streaming CSR path'
        key = tuple((id(t), ops._ffi.tver(t)) for D in dims for t in (D.up_index, D.up_shared, D.b_index) if t is not None)
        return dims, plan, table, key

    def _blocked_dim_extra(self, D, lvl, cochain, d: int) -> Optional[str]:
        """Hook of `_blocked_args`: what a subclass adds to the launch's descriptor of dimension d, or why it cannot."""
        return None

    def _blocked_eps(self, n: int) -> List[Tensor]:
        """The eps tensors a prepared launch reads in place (its marks follow their versions)."""
        return [t for d in range(n) for t in (self.mp_levels[d].eps1, self.mp_levels[d].eps2)]

    @staticmethod
    def _n_streams(plan) -> int:
        """How many matrices of `outs` belong to a dimension with this entry of `plans`."""
        return 2

    def _update_nets(self, lvl, nb: int):
        """The update networks of a level in the order of `outs`."""
        return [lvl.update_up_nn, lvl.update_boundaries_nn]

    def _update_chains(self, plans, outs, start: int):
        """(active dimensions, branches per dimension, [dim][branch] -> update network, [dim] -> combine network) of the
        dimensions from `start` on, each network as `_mlp_stages` reads it ([(Linear, norm), ...], or None for another
        form), the branches in the order of `outs`.  None when a dimension has no fused streams or `outs` is not the same
        number of matrices for every dimension."""
        active = list(range(start, len(plans)))
        if not active or any(plans[d] is None for d in active):
            return None
        nb = self._n_streams(plans[active[0]])
        if any(self._n_streams(plans[d]) != nb for d in active) or len(outs) != nb * len(active):
            return None
        levels = [self.mp_levels[d] for d in active]
        return (active, nb, [[_mlp_stages(net) for net in self._update_nets(lvl, nb)] for lvl in levels],
                [_mlp_stages(lvl.combine_nn) for lvl in levels])

    def _dense_eval(self, plans, outs, start: int = 0) -> Optional[List[Tensor]]:
        """Inference: the update / combine networks of ALL dimensions (mp/layers.py:193-199, :255-260) with eval-mode
        BatchNorm and the ReLU folded into the epilogue -- in ONE launch where `_one_launch` has a kernel for them, else
        as one grouped MFMA launch per update stage over every branch and dimension, then the combine: two branches as a
        grouped launch with torch.cat folded into the K-concatenation, three or four as torch.cat + combine_nn.  ReLU networks
        at a width that kernel does not take go to `_dense_chain_f32` first (regime 'relu_width' of FUSED_CHAIN_F32); the three
        or four ReLU branches of a CIN++ layer that `_one_launch` did not take go to `_dense_branches_f32` (regime
        'relu_width' of FUSED_BRANCHES_F32) in front of the grouped launches.  No
        autograd, running statistics; returns None when it does not apply and the caller runs the torch modules instead."""
        from . import _ffi
        if torch.is_grad_enabled() or any(o.dtype != torch.float32 for o in outs):
            return None                  # (float64: _dense_f64 / the torch modules)
        ent = _MLP_CACHE.get(self)
        if ent is not None:
            # the prepared launch of this layer's networks (ops.MlpLaunch): per call only the rows are looked at
            launch, shape, norms = ent
            if (shape == (start, len(plans), len(outs)) and FUSED_UPDATE_MLP and not ops.GEMM_EXACT
                    and not any(m.training for m in norms) and None not in plans[start:] and launch.current()):
                res = launch.run(outs[0::2], outs[1::2])
                if res is not None:
                    return res
            else:
                del _MLP_CACHE[self]
        if FUSED_UPDATE_MLP and not ops.GEMM_EXACT:      # ReLU at a width the one-launch kernel below does not take
            res = self._dense_chain_f32(plans, outs, start, regime='relu_width')
            if res is None and self in _BRANCHES_CACHE:
                # a CIN++ layer that has been through the dispatch below: its prepared launch (ops.BranchesLaunch) without
                # reading the networks again -- what it holds are shapes `_one_launch` never takes
                res = self._dense_branches_f32(plans, outs, start, regime='relu_width')
            if res is not None:
                return res
        got = self._update_chains(plans, outs, start)
        if got is None:
            return None
        active, nb, chains, combine = got
        flat = [st for sts in chains for st in sts]                      # [dim][branch] flattened, as `outs`
        if any(st is None for st in flat) or len({len(st) for st in flat}) != 1:
            return None
        # (two branches: the combine is a launch of this path, so its network has to be one foldable stage within the
        #  GEMM's K; three or four: it is needed in that form by the one-launch kernel only)
        if nb == 2 and any(cb is None or len(cb) != 1 for cb in combine):
            return None
        if any(lin.in_features > ops.GEMM_MAX_K for st in flat + (combine if nb == 2 else []) for lin, _ in st):
            return None
        folds = [[_fold_norm(norm, lin.out_features) for lin, norm in st] for st in flat]
        if any(f is None for fs in folds for f in fs):
            return None
        depth = len(flat[0])
        fused = FUSED_UPDATE_MLP and not ops.GEMM_EXACT and depth == 2 and nb < 4
        cfolds = _combine_folds(combine) if nb == 2 or fused else None
        if nb == 2 and cfolds is None:
            return None
        if fused and cfolds is not None:
            # every Linear layer of every dimension in ONE launch: the activations between them stay in LDS.  Per
            # dimension: its matrices of `outs`, the stages (branch by branch, then the combine) and their folds
            dims = [(list(outs[nb * k: nb * (k + 1)]), [s for st in flat[nb * k: nb * (k + 1)] for s in st] + combine[k],
                     [f for fs in folds[nb * k: nb * (k + 1)] for f in fs] + [cfolds[k]]) for k in range(len(active))]
            res = self._one_launch(dims, (start, len(plans), len(outs)))
            if res is not None:
                return res
        if nb > 2 and FUSED_UPDATE_MLP and not ops.GEMM_EXACT:     # three or four ReLU branches the one-launch kernel above did not take
            res = self._dense_branches_f32(plans, outs, start, regime='relu_width')
            if res is not None:
                return res
        hs, dev = list(outs), outs[0].device
        for s in range(depth):
            gemms = [ops.Gemm(X=h, W=st[s][0].weight, bias=st[s][0].bias, relu=True, out_scale=fs[s][0], out_shift=fs[s][1],
                              w_packed=ops.pack_gemm_weight(st[s][0].weight)) for h, st, fs in zip(hs, flat, folds)]
            hs = []
            for lo in range(0, len(gemms), _ffi.MAX_DESCS):
                hs += ops.run_gemm(gemms[lo: lo + _ffi.MAX_DESCS], dev)
        if nb == 2:
            return ops.run_gemm([ops.Gemm(X=hs[2 * k], X2=hs[2 * k + 1], W=cb[0][0].weight, bias=cb[0][0].bias, relu=True,
                                          out_scale=cf[0], out_shift=cf[1])
                                 for k, (cb, cf) in enumerate(zip(combine, cfolds))], dev)
        return [self.mp_levels[d].combine_nn(torch.cat(hs[nb * k: nb * (k + 1)], dim=-1)) for k, d in enumerate(active)]

    def _one_launch(self, dims, shape) -> Optional[List[Tensor]]:
        """Hook of `_dense_eval`: two-stage update networks + the combine of every dimension in one launch (here
        csrc/cwn_mlp.hip: five Linear layers per dimension, prepared once per layer in _MLP_CACHE), or None."""
        mdims = [ops.MlpDim(x_up=xs[0], x_b=xs[1], linears=[lin for lin, _ in stages], folds=fs) for xs, stages, fs in dims]
        if not ops.update_mlp_applies(mdims):
            return None
        sources, norms = [], []
        for _, stages, _ in dims:
            for lin, norm in stages:
                sources += [lin.weight, lin.bias]
                if isinstance(norm, BN):
                    norms.append(norm)
                    sources += [norm.weight, norm.bias, norm.running_mean, norm.running_var, norm.num_batches_tracked]
        launch = ops.MlpLaunch(mdims, sources)
        _MLP_CACHE[self] = (launch, shape, norms)
        res = launch.run([D.x_up for D in mdims], [D.x_b for D in mdims])
        return res if res is not None else ops.update_mlp(mdims)

    def _chain_net(self, lvl, dtype, wmax: int):
        """(weights, biases, folds, activation) of one dimension's three networks in the order of ops.ChainDim, or None when
        they are not the stock Linear-norm-act structure with one of the five activations and Identity / eval-mode
        BatchNorm norms, hold another dtype, or are wider than `wmax`."""
        if type(lvl) is not SparseCINCochainConv:
            return None
        got = [_f64_stages(lvl.update_up_nn, 2), _f64_stages(lvl.update_boundaries_nn, 2), _f64_stages(lvl.combine_nn, 1)]
        if any(g is None for g in got) or len({g[1] for g in got}) != 1:
            return None
        stages = got[0][0] + got[1][0] + got[2][0]
        if any(lin.weight.dtype != dtype or lin.out_features > wmax for lin, _ in stages) or stages[0][0].in_features > wmax:
            return None                  # (hidden 256 of cwn-sr-base.sh: dgemm is the right tool)
        folds = [_fold_norm(norm, lin.out_features) for lin, norm in stages]
        if any(f is None for f in folds):
            return None                  # LayerNorm, a training-mode BatchNorm
        return [lin.weight for lin, _ in stages], [lin.bias for lin, _ in stages], folds, got[0][1]

    def _f64_chain(self, lvl):
        """`_chain_net` for the float64 launch (widths up to 64)."""
        return self._chain_net(lvl, torch.float64, ops._ffi.CHAIN_F64_MAX_WIDTH)

    def _dense_chain_f32(self, plans, outs, start: int = 0, cochain_params=None, regime: str = 'act') -> Optional[List[Tensor]]:
        """The update / combine networks of ALL dimensions of a float32 layer in ONE launch (ops.update_chain_f32,
        csrc/cwn_chain_f32.hip) in one of the regimes of FUSED_CHAIN_F32: 'relu_width' -- ReLU networks at a width that
        cwn_update_mlp_f32 does not take (asked by `_dense_eval` in front of its own launches) -- or 'act' -- networks
        with elu / tanh / sigmoid / id at any width up to 128 (asked by `forward` behind `_dense_eval`, which reads ReLU
        networks only).  In the 'act' regime a dimension whose message has no fused stream (plans[d] is None) runs its
        generic propagate first and joins the same launch, as in `_dense_f64`.  Inference only.  The launch is prepared
        once per layer (ops.ChainLaunch in _CHAIN_CACHE): per call only the rows are looked at.
        None when it does not apply -- the regime is off, a recording autograd, CIN++ (three or four branches:
        `CINppConv._dense_branches_f32`, a switch of its own), float64 or CPU features, LayerNorm or
        a training-mode BatchNorm, a passed-in network, a width above 128, more than 4 dimensions, ReLU at 64 / 128 --
        and the caller goes on as before."""
        if not _chain_f32_on(regime) or torch.is_grad_enabled() or type(self) is not SparseCINConv:
            return None
        active = list(range(start, len(plans)))
        unfused = [d for d in active if plans[d] is None]
        if not active or len(outs) != 2 * (len(active) - len(unfused)) or len(active) > ops._ffi.CHAIN_F32_MAX_DIMS:
            return None
        if unfused and (regime != 'act' or cochain_params is None or _ffi_dyn()):
            return None                  # (a static batch: the generic propagate is not part of its captured graph)
        feats = list(outs) + [cochain_params[d].x for d in unfused]
        if any(not isinstance(t, Tensor) or t.dtype != torch.float32 or not t.is_cuda for t in feats):
            return None
        key = (start, len(plans))
        ents = _CHAIN_CACHE.get(self)
        if ents is None:
            _CHAIN_CACHE[self] = ents = {}
        ent = ents.get(regime)
        if ent is not None and (ent[1] != key or ent[3] != ops.STRUCT_EPOCH or (ent[0] is not None and not ent[0].current())):
            ent = None
        if ent is None:
            got = self._chain_f32_launch(active, regime)
            if got is None and any(isinstance(m, BN) and m.training for d in active for m in self.mp_levels[d].modules()):
                return None              # (not remembered: eval() is no change of the module tree)
            ent = ents[regime] = (None, key, [], ops.STRUCT_EPOCH) if got is None else (got[0], key, got[1], ops.STRUCT_EPOCH)
        if ent[0] is None:
            return None                  # (these networks have been read and are not this regime's)
        launch, _, norms, _ = ent
        if any(m.training for m in norms):
            return None                  # batch statistics are no fixed affine
        ins, k = [], 0
        for d in active:
            if plans[d] is None:
                ins.append(self.mp_levels[d].aggregate_unfused(cochain_params[d]))
            else:
                ins.append((outs[k], outs[k + 1]))
                k += 2
        res = launch.run(ins)
        if res is None and unfused:      # (an input of another width than its network: let torch say so)
            return [self.mp_levels[d].finish(u, b) for d, (u, b) in zip(active, ins)]
        return res

    def _chain_f32_launch(self, active, regime: str):
        """(ops.ChainLaunch, BatchNorm modules) of the networks of the dimensions `active` when they are `regime`'s, or None:
        'relu_width' -- all ReLU and not the 64 / 128 shapes of cwn_update_mlp_f32; 'act' -- none of them ReLU."""
        nets = [self._chain_net(self.mp_levels[d], torch.float32, ops._ffi.CHAIN_F32_MAX_WIDTH) for d in active]
        if any(net is None for net in nets):
            return None
        relu = [net[3] == 'relu' for net in nets]
        if any(relu) != (regime == 'relu_width') or len(set(relu)) != 1:
            return None
        if regime == 'relu_width' and all(net[0][0].size(0) in (64, 128) and net[0][0].size(1) <= net[0][0].size(0) for net in nets):
            return None                  # ReLU at 64 / 128 is cwn_update_mlp_f32's, whatever makes that launch decline
        empty = lambda w: w.new_empty(0, w.size(1))
        dims = [ops.ChainDim(in_up=empty(net[0][0]), in_b=empty(net[0][0]), weights=net[0], biases=net[1], folds=net[2], act=net[3])
                for net in nets]
        if not ops.update_chain_f32_applies(dims):
            return None
        sources, norms = [], []
        for d in active:
            lvl = self.mp_levels[d]
            for m in list(lvl.update_up_nn) + list(lvl.update_boundaries_nn) + list(lvl.combine_nn):
                if isinstance(m, Linear):
                    sources += [m.weight, m.bias]
                elif isinstance(m, BN):
                    norms.append(m)
                    sources += [m.weight, m.bias, m.running_mean, m.running_var, m.num_batches_tracked]
        return ops.ChainLaunch(dims, sources), norms

    def _dense_branches_f32(self, plans, outs, start: int = 0, cochain_params=None, regime: str = 'act') -> Optional[List[Tensor]]:
        """Hook of `_dense_eval` and `forward`: the three or four branches of a CIN++ layer in one launch (CINppConv), or None."""
        return None

    def _dense_f64(self, plans, outs, start: int = 0, cochain_params=None) -> Optional[List[Tensor]]:
        """The update / combine networks of ALL dimensions of a float64 layer in ONE launch (ops.update_chain_f64,
        csrc/cwn_dense_f64.hip): five Linear layers per dimension, eval-mode BatchNorm folded, any of the five
        activations, widths up to 64.  A dimension whose message network has no fused stream (plans[d] is None: the
        act(Linear(cat)) message of an ELU model) runs its generic propagate first and joins the same launch.
        Inference only (the condition of `_dense_eval`).  None when it does not apply -- training or a recording
        autograd, LayerNorm, a passed-in network, widths above 64 (there dgemm is the right tool), CIN++, float32 or CPU
        features, FUSED_F64_DENSE off -- and the caller runs the torch modules."""
        if not FUSED_F64_DENSE or torch.is_grad_enabled() or type(self) is not SparseCINConv:
            return None
        active = list(range(start, len(plans)))
        unfused = [d for d in active if plans[d] is None]
        if not active or len(outs) != 2 * (len(active) - len(unfused)) or len(active) > ops._ffi.CHAIN_F64_MAX_DIMS:
            return None
        if unfused and cochain_params is None:
            return None
        feats = list(outs) + [cochain_params[d].x for d in unfused]
        if any(not isinstance(t, Tensor) or t.dtype != torch.float64 or not t.is_cuda for t in feats):
            return None
        nets = [self._f64_chain(self.mp_levels[d]) for d in active]
        if any(net is None for net in nets):
            return None
        ins, k = [], 0
        for d in active:
            if plans[d] is None:
                ins.append(self.mp_levels[d].aggregate_unfused(cochain_params[d]))
            else:
                ins.append((outs[k], outs[k + 1]))
                k += 2
        dims = [ops.ChainDim(in_up=u.contiguous(), in_b=b.contiguous(), weights=net[0], biases=net[1], folds=net[2], act=net[3])
                for (u, b), net in zip(ins, nets)]
        if not ops.update_chain_f64_applies(dims):       # (an input of another width than its network: let torch say so)
            return [self.mp_levels[d].finish(u, b) for d, (u, b) in zip(active, ins)]
        return ops.update_chain_f64(dims)

    def _dense_train(self, plans, outs, start: int = 0) -> Optional[List[Tensor]]:
        """The same networks with autograd and training-mode BatchNorm (batch statistics, running
        statistics updated) as grouped launches forward and backward: cwn_amd/dense_train.py.
        Returns None when it does not apply (LayerNorm, custom networks, fewer than two cells in
        a dimension) and the caller runs the torch modules instead."""
        from . import dense_train as DT
        got = self._train_chains(plans, outs, start)
        if got is None or any(cb is None or len(cb) != 1 for cb in got[3]):
            return None
        cbs = [DT.Stage(*cb[0]) for cb in got[3]]
        if not DT.supported(cbs):
            return None
        p = self._out_drop
        self._out_dropped = p > 0.0              # (the combine stage's activation launch applies it: dense_train._Plan.out_drop)
        return DT.dense_train(DT._Plan(got[2], cbs, p), outs)

    def _train_chains(self, plans, outs, start: int):
        """What `_update_chains` returns, with the update networks as dense_train.Stage lists, when the training launches
        serve them: autograd recording, float32, at least two rows everywhere, equally deep Linear -> BatchNorm(train) /
        Identity -> ReLU networks.  None otherwise."""
        from . import dense_train as DT
        if (not torch.is_grad_enabled() or not FUSED_DENSE_TRAINING or any(o.dtype != torch.float32 for o in outs)
                or any(o.size(0) < 2 for o in outs)):
            return None      # (one row: BatchNorm1d(train) needs more; let torch raise as the reference does)
        got = self._update_chains(plans, outs, start)
        if got is None:
            return None
        active, nb, raw, combine = got
        if any(st is None for sts in raw for st in sts) or len({len(st) for sts in raw for st in sts}) != 1:
            return None
        chains = [[[DT.Stage(lin, norm) for lin, norm in st] for st in sts] for sts in raw]
        if not all(DT.supported(c) for cs in chains for c in cs):       # (refuses a BatchNorm in eval mode too)
            return None
        return active, nb, chains, combine

    def _ln_chains(self, plans, outs, start: int):
        """([dim][branch] -> stages, [dim] -> combine stages) of the active dimensions as `_mlp_stages` reads them, or None."""
        got = self._update_chains(plans, outs, start)
        return None if got is None else got[2:]

    def _dense_ln(self, plans, outs, start: int = 0) -> Optional[List[Tensor]]:
        """The same networks built with graph_norm='ln', in inference and in training: one grouped GEMM and one LayerNorm +
        ReLU launch per stage over all dimensions and branches (cwn_amd/dense_ln.py).  None when it does not apply (another
        normalisation, custom networks, float64 or CPU features) and the caller runs the torch modules instead."""
        from . import dense_ln as DL
        if not DL.FUSED_LN or not outs or any(o.dtype != torch.float32 or not o.is_cuda for o in outs):
            return None
        got = self._ln_chains(plans, outs, start)
        if got is None or not DL.supported(*got):
            return None
        return DL.run(got[0], got[1], outs)

    # the caller's dropout of this layer's OUTPUT (OGBEmbedSparseCIN: after every conv, mp/molec_models.py:298-300), handed in
    # so that the fused training path applies it inside its last launch: forward(..., out_dropout=p).  _dense_train sets
    # _out_dropped when it has; every other path gets ops.dropout (one launch per dimension, no mask tensor).
    _out_drop = 0.0
    _out_dropped = False

    def _finish_dropout(self, out: List[Tensor], start: int) -> List[Tensor]:
        p, done = self._out_drop, self._out_dropped
        self.__dict__['_out_drop'], self.__dict__['_out_dropped'] = 0.0, False
        if p <= 0.0 or done:
            return out
        return [x if dim < start or x is None else ops.dropout(x, p, True) for dim, x in enumerate(out)]

    def forward(self, *cochain_params: CochainMessagePassingParams, start_to_process=0, out_dropout: float = 0.0):
        """mp/layers.py:333-342 (CINppConv: :418-427)."""
        assert len(cochain_params) <= self.max_dim + 1
        n = len(cochain_params)
        self.__dict__['_out_drop'], self.__dict__['_out_dropped'] = (float(out_dropout) if self.training else 0.0), False
        plans, outs = self.propagate_all(*cochain_params, start_to_process=start_to_process)
        dense = self._dense_eval(plans, outs, start_to_process)
        if dense is None:
            dense = self._dense_chain_f32(plans, outs, start_to_process, cochain_params)
        if dense is None:
            dense = self._dense_branches_f32(plans, outs, start_to_process, cochain_params)
        if dense is None:
            dense = self._dense_f64(plans, outs, start_to_process, cochain_params)
        if dense is None:
            dense = self._dense_train(plans, outs, start_to_process)
        if dense is None:
            dense = self._dense_ln(plans, outs, start_to_process)
        if dense is not None:
            it = iter(dense)
            return self._finish_dropout([cochain_params[dim].x if dim < start_to_process else next(it) for dim in range(n)],
                                        start_to_process)
        # update / combine networks per dimension
        out, k = [], 0
        for dim in range(n):
            if dim < start_to_process:
                out.append(cochain_params[dim].x)
            elif plans[dim] is None:
                out.append(self.mp_levels[dim].forward_unfused(cochain_params[dim]))
            else:
                m = self._n_streams(plans[dim])
                out.append(self.mp_levels[dim].finish(*outs[k:k + m]))
                k += m
        return self._finish_dropout(out, start_to_process)


# ------------------------------------------------------------------------------------------------
# CIN++ (upper + lower + boundary)
# ------------------------------------------------------------------------------------------------
class CINppCochainConv(SparseCINCochainConv):
    """mp/layers.py:216-260.  Quirk kept by default: forward does not pass `down_attr` (:244-247), and
    the molecular CIN++ models ask for include_down_features=False, so the lower stream is zeros
    there.  Two explicit switches do it properly (no reference oracle
    for either: parity unpinned, property-tested):
      feed_down_attr=True       `down_attr` reaches message_down -- the lower-adjacency stream CIN++
                                describes, msg_down_nn((x_j, shared-boundary features));
      coboundary_stream=True    a FOURTH stream: the sum over the cofaces of a cell (the co-boundary
                                aggregation mp/cell_mp.py:44 leaves as a TODO), with its own eps and
                                update network, concatenated before combine_nn (which then takes
                                4 * hidden inputs).  Needs params from Complex.get_cochain_params
                                (they carry `coboundary_index` / `coboundary_attr`)."""

    def __init__(self, dim: int, up_msg_size: int, down_msg_size: int, boundary_msg_size: int,
                 msg_up_nn: Callable[..., Any], msg_boundaries_nn: Callable[..., Any],
                 msg_down_nn: Callable[..., Any], update_up_nn: Callable[..., Any],
                 update_boundaries_nn: Callable[..., Any], update_down_nn: Callable[..., Any],
                 combine_nn: Callable[..., Any], eps: float = 0, train_eps: bool = False,
                 feed_down_attr: bool = False, update_coboundaries_nn: Optional[Callable[..., Any]] = None):
        super().__init__(dim, up_msg_size, down_msg_size, boundary_msg_size, msg_up_nn,
                         msg_boundaries_nn, update_up_nn, update_boundaries_nn, combine_nn, eps,
                         train_eps)
        # the reference inherits use_down_msg=False from SparseCINCochainConv (mp/layers.py:167-168): the
        # lower stream is OFF unless the caller asks for the proper form
        self.use_down_msg = bool(feed_down_attr)
        self.msg_down_nn = msg_down_nn
        self.update_down_nn = update_down_nn
        self.feed_down_attr = feed_down_attr
        self.update_coboundaries_nn = update_coboundaries_nn       # not None = the fourth stream is on
        if train_eps:
            self.eps3 = torch.nn.Parameter(torch.Tensor([eps]))
        else:
            self.register_buffer('eps3', torch.Tensor([eps]))
        reset(self.msg_down_nn)
        reset(self.update_down_nn)
        self.eps3.data.fill_(self.initial_eps)
        if update_coboundaries_nn is not None:
            if train_eps:
                self.eps4 = torch.nn.Parameter(torch.Tensor([eps]))
            else:
                self.register_buffer('eps4', torch.Tensor([eps]))
            reset(self.update_coboundaries_nn)

    def message_down(self, down_x_j: Tensor, down_attr: Tensor) -> Tensor:
        return self.msg_down_nn((down_x_j, down_attr))

    # ---- fused forms (round 4): every stream of the level in the layer's ONE aggregation launch --
    def _boundary_eps(self):
        return self.eps3          # mp/layers.py:254

    def _down_kind(self) -> str:
        if isinstance(self.msg_down_nn, FirstOf):
            return 'first'
        return 'cat_linear_relu' if _is_cat_linear_relu(self.msg_down_nn) else 'custom'

    def _down_active(self, cochain) -> bool:
        return bool(self.use_down_msg) and cochain.down_index is not None

    def _down_specs(self, cochain) -> List[ops.Gemm]:
        """The lower-adjacency message ReLU(Linear(cat(x_j, down_attr))) as Y1[j] + Y2[shared boundary] (the form of the
        coboundary message, SparseCINCochainConv.gemm_specs); [] when the lower stream is off (the reference's quirk, the
        default) or its network is another form."""
        x, attr = cochain.x, cochain.kwargs.get('down_attr')
        if (not self._down_active(cochain) or attr is None or self._down_kind() != 'cat_linear_relu'
                or (self.aggr_down or 'add') != 'add' or x.dtype != torch.float32):
            return []
        lin, F = self.msg_down_nn[1], x.size(1)
        src, _ = _attr_operand(attr)
        if lin.in_features != F + src.size(1) or max(F, src.size(1)) > ops.GEMM_MAX_K:
            return []
        return [ops.Gemm(X=x, W=lin.weight, w_col0=0, bias=lin.bias), ops.Gemm(X=src, W=lin.weight, w_col0=F)]

    def gemm_specs(self, cochain):
        return SparseCINCochainConv.gemm_specs(self, cochain) + self._down_specs(cochain)

    def streams(self, cochain, ys=None):
        """[upper, lower, boundary (, co-boundary)] with the self terms folded in -- (1 + eps1 / eps2 / eps3 / eps4) x,
        mp/layers.py:252-254 -- or None when a message network is not a recognised form (the caller then runs
        `forward_unfused`).  The lower stream of the default layer is its self term alone (the quirk: zeros + (1+eps2) x)."""
        n_up = len(SparseCINCochainConv.gemm_specs(self, cochain)) if ys else 0
        base = SparseCINCochainConv.streams(self, cochain, (list(ys[:n_up]) or None) if ys else None)
        if base is None:
            return None
        up, bnd = base
        x = cochain.x
        n, F = x.size(0), int(x.size(1))
        if self._down_active(cochain):
            attr = cochain.kwargs.get('down_attr') if self.feed_down_attr else None
            size = self.__check_input_separately__(cochain.down_index, None)
            adj = self._adjacency(cochain.down_index, 'down', size, dict(x=x, down_attr=attr))
            kind = self._down_kind()
            if kind == 'first':
                down = ops.Stream(adj=adj, n_dst=adj.n_dst, width=F, A=x, self_x=x, eps=self.eps2,
                                  reduce=self.aggr_down or 'add')
            elif kind == 'cat_linear_relu' and attr is not None and (self.aggr_down or 'add') == 'add':
                yd = list(ys[n_up:]) if ys else []
                if not yd:
                    specs = self._down_specs(cochain)
                    yd = ops.gemm_many(specs) if specs else _torch_products(self.msg_down_nn[1], x, attr)
                    if yd is None:
                        return None
                _, mode = _attr_operand(attr)
                down = ops.Stream(adj=adj, n_dst=adj.n_dst, width=int(yd[0].size(1)), A=yd[0], B=yd[1],
                                  msg_op=ops.MSG_RELU_A_PLUS_B, ib_mode=mode, self_x=x, eps=self.eps2)
            else:
                return None
        else:
            down = ops.Stream(adj=None, n_dst=n, width=F, self_x=x, eps=self.eps2)
        out = [up, down, bnd]
        if self.update_coboundaries_nn is not None:
            cob_index, cob_attr = getattr(cochain, 'coboundary_index', None), getattr(cochain, 'coboundary_attr', None)
            if cob_index is not None and cob_attr is not None:
                if cob_attr.dim() != 2 or cob_index.dim() != 2 or cob_index.size(0) != 2:
                    return None          # (propagate_coboundary raises the errors)
                t = cached_adjacency(cob_index, int(cob_attr.size(0)), int(n)).t_src     # keyed on this dimension's cell
                out.append(ops.Stream(adj=t, n_dst=n, width=int(cob_attr.size(1)), A=cob_attr, self_x=x, eps=self.eps4))
            else:
                out.append(ops.Stream(adj=None, n_dst=n, width=F, self_x=x, eps=self.eps4))
        if any(st.width != F for st in out):
            return None
        return out

    def finish(self, out_up: Tensor, out_down: Tensor, out_boundaries: Tensor, out_cob: Optional[Tensor] = None) -> Tensor:
        """mp/layers.py:255-260 (+ the fourth stream)."""
        parts = [self.update_up_nn(out_up), self.update_down_nn(out_down), self.update_boundaries_nn(out_boundaries)]
        if self.update_coboundaries_nn is not None:
            parts.append(self.update_coboundaries_nn(out_cob))
        return self.combine_nn(torch.cat(parts, dim=-1))

    def forward(self, cochain: CochainMessagePassingParams):
        sts = self.streams(cochain)
        if sts is None:
            return self.forward_unfused(cochain)
        return self.finish(*ops.aggregate_many(sts))

    def aggregate_unfused(self, cochain: CochainMessagePassingParams):
        """The three or four aggregated inputs of the update networks, self terms added, through propagate() and the hooks
        (mp/layers.py:243-254), in the order of `finish`; zeros for an absent co-boundary index."""
        kw = dict(x=cochain.x, up_attr=cochain.kwargs['up_attr'], boundary_attr=cochain.kwargs['boundary_attr'])
        down_index = cochain.down_index
        if self.feed_down_attr:
            kw['down_attr'] = cochain.kwargs.get('down_attr')
        out_up, out_down, out_boundaries = self.propagate(cochain.up_index, down_index, cochain.boundary_index, **kw)
        out_up = out_up + (1 + self.eps1) * cochain.x
        out_down = out_down + (1 + self.eps2) * cochain.x
        out_boundaries = out_boundaries + (1 + self.eps3) * cochain.x
        if self.update_coboundaries_nn is None:
            return out_up, out_down, out_boundaries
        cob_index = getattr(cochain, 'coboundary_index', None)
        cob_attr = getattr(cochain, 'coboundary_attr', None)
        if cob_index is not None and cob_attr is not None:
            out_cob = self.propagate_coboundary(cob_index, cob_attr, cochain.x.size(0))
        else:
            out_cob = ops.zeros_rows(cochain.x.size(0), cochain.x.size(1), cochain.x.device, _zero_dtype(cochain.x))
        return out_up, out_down, out_boundaries, out_cob + (1 + self.eps4) * cochain.x

    def forward_unfused(self, cochain: CochainMessagePassingParams):
        """The reference's own sequence (mp/layers.py:243-260) through propagate() and the hooks."""
        return self.finish(*self.aggregate_unfused(cochain))


class CINppConv(SparseCINConv):
    """mp/layers.py:344-427; `feed_down_attr` / `coboundary_stream`: see CINppCochainConv."""

    def __init__(self, up_msg_size: int, down_msg_size: int, boundary_msg_size: Optional[int],
                 passed_msg_up_nn: Optional[Callable], passed_msg_down_nn: Optional[Callable],
                 passed_msg_boundaries_nn: Optional[Callable],
                 passed_update_up_nn: Optional[Callable], passed_update_down_nn: Optional[Callable],
                 passed_update_boundaries_nn: Optional[Callable], eps: float = 0.,
                 train_eps: bool = False, max_dim: int = 2, graph_norm=BN, use_coboundaries=False,
                 feed_down_attr: bool = False, coboundary_stream: bool = False, **kwargs):
        super().__init__(up_msg_size, down_msg_size, boundary_msg_size, passed_msg_up_nn,
                         passed_msg_boundaries_nn, passed_update_up_nn, passed_update_boundaries_nn,
                         eps, train_eps, max_dim, graph_norm, use_coboundaries, **kwargs)
        self.mp_levels = torch.nn.ModuleList()
        ld, hid, act = kwargs['layer_dim'], kwargs['hidden'], kwargs['act_module']
        n_streams = 4 if coboundary_stream else 3
        for dim in range(max_dim + 1):
            def msg_net(passed):
                if passed is not None:
                    return passed
                return Sequential(Catter(), Linear(ld * 2, ld), act()) if use_coboundaries else FirstOf()
            self.mp_levels.append(CINppCochainConv(
                dim, up_msg_size, down_msg_size, boundary_msg_size=boundary_msg_size,
                msg_up_nn=msg_net(passed_msg_up_nn), msg_down_nn=msg_net(passed_msg_down_nn),
                msg_boundaries_nn=passed_msg_boundaries_nn or Passthrough(),
                update_up_nn=passed_update_up_nn or _update_mlp(ld, hid, graph_norm, act),
                update_down_nn=passed_update_down_nn or _update_mlp(ld, hid, graph_norm, act),
                update_boundaries_nn=passed_update_boundaries_nn or _update_mlp(ld, hid, graph_norm, act),
                combine_nn=Sequential(Linear(hid * n_streams, hid), graph_norm(hid), act()),
                eps=eps, train_eps=train_eps, feed_down_attr=feed_down_attr,
                update_coboundaries_nn=_update_mlp(ld, hid, graph_norm, act) if coboundary_stream else None))

    # Round 6: the layer as the reference's molecular models run it -- lower stream OFF (the quirk: include_down_features=False,
    # mp/molec_models.py:111 -> down_index None -> out_down = zeros + (1 + eps2) x, mp/layers.py:253) -- takes the blocked launch
    # of SparseCINConv: upper + boundary streams as there (boundary self term with eps3, :254), and the launch writes the
    # third output (1 + eps2) x from the registers that hold the row (cwn_layer_dim.out_down, ABI 22).  Outputs per dimension
    # in the order of torch.cat in :260: [out_up, out_down, out_b].  With `feed_down_attr` (a real lower adjacency) or the
    # co-boundary stream the layer keeps the grouped message GEMM + ONE aggregation launch for its three (four) streams.
    def _blocked_dim_extra(self, D, lvl, cochain, d: int) -> Optional[str]:
        if lvl._down_active(cochain):
            return f'dim {d}: CIN++ with a lower-adjacency stream (the blocked launch has upper + boundary + the self-only third)'
        if lvl.update_coboundaries_nn is not None:
            return f'dim {d}: CIN++ with the co-boundary stream (four streams)'
        D.eps3, D.want_down = lvl.eps2, True
        return None

    def _blocked_eps(self, n: int) -> List[Tensor]:
        return [t for d in range(n) for t in (self.mp_levels[d].eps1, self.mp_levels[d].eps2, self.mp_levels[d].eps3)]

    def _blocked_still_valid(self, ent, cochain_params) -> bool:
        if any(self.mp_levels[d]._down_active(c) for d, c in enumerate(cochain_params)):
            return False         # a lower adjacency has appeared: `_blocked_args` says why the launch does not serve it
        return super()._blocked_still_valid(ent, cochain_params)

    # (training: SparseCINConv._propagate_blocked_train serves this layer too -- the launch stores Y1 / Y2 and writes the third
    #  output; the blocked backward launch takes the gradients of out_up / out_b and ops._blocked_backward_impl adds
    #  (1 + eps2) g_down onto dx)

    @staticmethod
    def _n_streams(plan) -> int:
        return 3 if isinstance(plan, str) else len(plan)       # ('blocked': the launch's three outputs)

    def _update_nets(self, lvl, nb: int):
        nets = [lvl.update_up_nn, lvl.update_down_nn, lvl.update_boundaries_nn]
        return nets + [lvl.update_coboundaries_nn] if nb == 4 else nets

    def _one_launch(self, dims, shape) -> Optional[List[Tensor]]:
        """Three update networks + the 3F-wide combine of every dimension in ONE launch (csrc/cwn_mlp3.hip, round 6): the
        activations between the seven Linear layers stay in LDS, the combine is accumulated branch by branch."""
        mdims = [ops.Mlp3Dim(xs=xs, linears=[lin for lin, _ in stages], folds=fs) for xs, stages, fs in dims]
        return ops.update_mlp3(mdims) if ops.update_mlp3_applies(mdims) else None

    @staticmethod
    def _branch_net(lvl, wmax: int):
        """(weights, biases, folds, activation) of one dimension's three or four update networks and its combine in the order
        of ops.BranchDim, or None when they are not the stock Linear-norm-act structure with one of the five activations and
        Identity / eval-mode BatchNorm norms, are not float32, or are wider than `wmax`."""
        if type(lvl) is not CINppCochainConv:
            return None
        nets = [lvl.update_up_nn, lvl.update_down_nn, lvl.update_boundaries_nn]
        if lvl.update_coboundaries_nn is not None:
            nets.append(lvl.update_coboundaries_nn)
        got = [_f64_stages(net, 2) for net in nets] + [_f64_stages(lvl.combine_nn, 1)]
        if any(g is None for g in got) or len({g[1] for g in got}) != 1:
            return None
        stages = [st for g in got for st in g[0]]
        if (any(lin.weight.dtype != torch.float32 or lin.out_features > wmax for lin, _ in stages)
                or any(g[0][0][0].in_features > wmax for g in got[:-1])):
            return None
        folds = [_fold_norm(norm, lin.out_features) for lin, norm in stages]
        if any(f is None for f in folds):
            return None                  # LayerNorm, a training-mode BatchNorm
        return [lin.weight for lin, _ in stages], [lin.bias for lin, _ in stages], folds, got[0][1]

    def _dense_branches_f32(self, plans, outs, start: int = 0, cochain_params=None, regime: str = 'act') -> Optional[List[Tensor]]:
        """The three or four update networks and the combine of ALL dimensions of a float32 CIN++ layer in ONE launch
        (ops.update_branches_f32, csrc/cwn_branches_f32.hip) in one of the regimes of FUSED_BRANCHES_F32: 'relu_width' -- ReLU
        networks that cwn_update_mlp3_f32 does not take (asked by `_dense_eval` behind `_one_launch` and in front of its
        grouped launches) -- or 'act' -- networks with elu / tanh / sigmoid / id at any width up to 128 (asked by `forward`
        behind `_dense_eval`, which reads ReLU networks only).  The parallel of `SparseCINConv._dense_chain_f32`: in the 'act'
        regime a dimension whose message has no fused stream (plans[d] is None) runs its generic propagate first and joins
        the same launch; the three outputs of the blocked propagate are taken as they come, [up, down, boundaries].  Inference
        only.  The launch is prepared once per layer (ops.BranchesLaunch in _BRANCHES_CACHE): per call only the rows are
        looked at.
        None when it does not apply -- the regime is off, a recording autograd, float64 or CPU features, LayerNorm or a
        training-mode BatchNorm, a passed-in network of another form, a width above 128, more than 4 dimensions, an unfused
        dimension under a static batch, ReLU in the shapes of cwn_update_mlp3_f32 -- and the caller goes on as before.
        Out of scope: float64 (the torch modules), training, the compiled binding; the message products of
        `feed_down_attr` are upstream of this launch and unchanged."""
        if not _branches_f32_on(regime) or torch.is_grad_enabled() or type(self) is not CINppConv:
            return None
        active = list(range(start, len(plans)))
        unfused = [d for d in active if plans[d] is None]
        if not active or len(active) > ops._ffi.BRANCHES_F32_MAX_DIMS:
            return None
        if len(outs) != sum(self._n_streams(plans[d]) for d in active if plans[d] is not None):
            return None
        if unfused and (regime != 'act' or cochain_params is None or _ffi_dyn()):
            return None                  # (a static batch: the generic propagate is not part of its captured graph)
        feats = list(outs) + [cochain_params[d].x for d in unfused]
        if any(not isinstance(t, Tensor) or t.dtype != torch.float32 or not t.is_cuda for t in feats):
            return None
        key = (start, len(plans))
        ents = _BRANCHES_CACHE.get(self)
        if ents is None:
            _BRANCHES_CACHE[self] = ents = {}
        ent = ents.get(regime)
        if ent is not None and (ent[1] != key or ent[3] != ops.STRUCT_EPOCH or (ent[0] is not None and not ent[0].current())):
            ent = None
        if ent is None:
            got = self._branches_f32_launch(active, regime)
            if got is None and any(isinstance(m, BN) and m.training for d in active for m in self.mp_levels[d].modules()):
                return None              # (not remembered: eval() is no change of the module tree)
            ent = ents[regime] = (None, key, [], ops.STRUCT_EPOCH) if got is None else (got[0], key, got[1], ops.STRUCT_EPOCH)
        if ent[0] is None:
            return None                  # (these networks have been read and are not this regime's)
        launch, _, norms, _ = ent
        if any(m.training for m in norms):
            return None                  # batch statistics are no fixed affine
        ins, k = [], 0
        for d in active:
            if plans[d] is None:
                ins.append(self.mp_levels[d].aggregate_unfused(cochain_params[d]))
            else:
                m = self._n_streams(plans[d])
                ins.append(tuple(outs[k:k + m]))
                k += m
        res = launch.run(ins)
        if res is None and unfused:      # (an input of another width than its network: let torch say so)
            return [self.mp_levels[d].finish(*xs) for d, xs in zip(active, ins)]
        return res

    def _branches_f32_launch(self, active, regime: str):
        """(ops.BranchesLaunch, BatchNorm modules) of the networks of the dimensions `active` when they are `regime`'s, or
        None: 'relu_width' -- all ReLU and not the shapes of cwn_update_mlp3_f32 (three branches, (F, F) first layers, one
        width of 64 or 128 for every dimension); 'act' -- none of them ReLU."""
        nets = [self._branch_net(self.mp_levels[d], ops._ffi.BRANCHES_F32_MAX_WIDTH) for d in active]
        if any(net is None for net in nets):
            return None
        relu = [net[3] == 'relu' for net in nets]
        if any(relu) != (regime == 'relu_width') or len(set(relu)) != 1:
            return None
        shapes = {tuple(net[0][0].shape) + (len(net[0]),) for net in nets}
        if regime == 'relu_width' and shapes in ({(64, 64, 7)}, {(128, 128, 7)}):
            return None                  # cwn_update_mlp3_f32's, whatever makes that launch decline
        dims = []
        for net in nets:
            nb = (len(net[0]) - 1) // 2
            x = net[0][0].new_empty(0, net[0][0].size(1))
            dims.append(ops.BranchDim(ins=[x] * nb, weights=net[0], biases=net[1], folds=net[2], act=net[3]))
        if not ops.update_branches_f32_applies(dims):
            return None
        sources, norms = [], []
        for d in active:
            lvl = self.mp_levels[d]
            nns = [lvl.update_up_nn, lvl.update_down_nn, lvl.update_boundaries_nn, lvl.update_coboundaries_nn or [], lvl.combine_nn]
            for m in [m for nn in nns for m in nn]:
                if isinstance(m, Linear):
                    sources += [m.weight, m.bias]
                elif isinstance(m, BN):
                    norms.append(m)
                    sources += [m.weight, m.bias, m.running_mean, m.running_var, m.num_batches_tracked]
        return ops.BranchesLaunch(dims, sources), norms

    def _dense_train(self, plans, outs, start: int = 0) -> Optional[List[Tensor]]:
        """Training mode: the update networks of EVERY stream and dimension (three or four chains of Linear ->
        BatchNorm(train) -> ReLU stages per dimension) through dense_train's stage launches, forward and backward -- at most
        _ffi.MAX_DESCS chains per autograd node -- with the combine stage in the same node, or without combine stages and then
        torch.cat + combine_nn as torch modules (mp/layers.py:255-260).  None when it does not apply (LayerNorm, custom
        networks, fewer than two cells)."""
        from . import _ffi, dense_train as DT
        got = self._train_chains(plans, outs, start)
        if got is None:
            return None
        active, nb, chains, combine = got
        per = max(1, _ffi.MAX_DESCS // nb)                    # dimensions per autograd node
        # the combine stage in the same node (its third / fourth branch as extra K-blocks of cwn_dense_stage_ex_f32) ...
        cbs = [DT.Stage(*cb[0]) if cb is not None and len(cb) == 1 else None for cb in combine]
        full = (FUSED_CINPP_COMBINE and ops.STAGE_KERNEL and all(c is not None and DT.supported([c], max_k=4 * 128) and c.is_bn and c.norm.training
                                                                for c in cbs))
        if ops.STAGE_KERNEL:
            # This layer packs its own blocks on every training forward (one launch: update and combine networks), next to
            # whatever a model packed (fresh=False).  ALWAYS: a block is keyed on its weight's storage address, and a look-up
            # that trusted an earlier entry could be handed the block of a dead layer whose parameters lived at the same
            # address (seen in the tests: two layers built one after the other).
            ws = [st.lin.weight for cs in chains for c in cs for st in c if st.lin.weight.is_cuda]
            if full:
                ws += [c.lin.weight for c in cbs if c.lin.weight.is_cuda]
            if ws:
                ops.pack_stage_weights_many(ws, fresh=False)
        if full:
            res: List[Tensor] = []
            try:
                for lo in range(0, len(active), per):
                    grp = chains[lo: lo + per]
                    res += DT.dense_train(DT._Plan(grp, cbs[lo: lo + per], self._out_drop), outs[nb * lo: nb * (lo + len(grp))])
                self._out_dropped = self._out_drop > 0.0
                return res
            except DT.CombineNeedsStageKernel:
                if res:         # (a later group refused after an earlier one has run: running it again would count its batch twice)
                    raise
                # (raised before any launch of the first group: the whole layer takes the other form)
        # ... or on torch, behind the branches
        hs: List[Tensor] = []
        for lo in range(0, len(active), per):
            grp = chains[lo: lo + per]
            hs += DT.dense_train(DT._Plan(grp, None), outs[nb * lo: nb * (lo + len(grp))])
        return [self.mp_levels[d].combine_nn(torch.cat(hs[nb * k: nb * (k + 1)], dim=-1)) for k, d in enumerate(active)]


# ------------------------------------------------------------------------------------------------
# OrientedConv, InitReduceConv, embedding front-ends
# ------------------------------------------------------------------------------------------------
FUSED_ORIENTED = os.environ.get('CWN_FUSED_ORIENTED') != '0'    # False: OrientedConv as one aggregation launch + torch Linear / add / activation


class ZeroUpdate(torch.nn.Module):
    """An update map that discards its input: the recognisable, parameter-free form of the reference's
    `update_up = lambda x: 0` (EdgeMPNN, mp/models.py:569-570)."""

    def forward(self, x):
        return 0


class OrientedConv(CochainMessagePassing):
    """mp/layers.py:430-470: messages x_j * orientation (a +-1 scalar per adjacency entry).  With bias-free Linear update
    maps (EdgeOrient, EdgeMPNN) the whole layer is one launch, ops.oriented_layer; otherwise the two aggregations are one
    CWN_MSG_A_TIMES_B launch with a width-1 per-entry attribute and the maps run as the modules they are."""

    def __init__(self, dim: int, up_msg_size: int, down_msg_size: int,
                 update_up_nn: Optional[Callable], update_down_nn: Optional[Callable],
                 update_nn: Optional[Callable], act_fn, orient=True):
        super().__init__(up_msg_size, down_msg_size, use_boundary_msg=False)
        self.dim = dim
        self.update_up_nn = update_up_nn
        self.update_down_nn = update_down_nn
        self.update_nn = update_nn
        self.act_fn = act_fn
        self.orient = orient

    def _stream(self, adj: Adjacency, x: Tensor, attr: Tensor, aggr) -> ops.Stream:
        if not self.orient:
            return ops.Stream(adj=adj, n_dst=adj.n_dst, width=int(x.size(1)), A=x, reduce=aggr or 'add')
        return ops.Stream(adj=adj, n_dst=adj.n_dst, width=int(x.size(1)), A=x, B=dense(attr).to(x.dtype),
                          msg_op=ops.MSG_A_TIMES_B, ib_mode='perm', reduce=aggr or 'add')

    def propagate_both(self, cochain) -> Optional[List[Tensor]]:
        """(out_up, out_down) of mp/layers.py:441-446 in ONE aggregation launch (one autograd node in training) instead of
        one per adjacency; None when a subclass has replaced the hooks (forward then runs propagate())."""
        x = cochain.x
        if not isinstance(x, Tensor) or not x.is_cuda or not self._own_hooks():
            return None
        up_attr, down_attr = cochain.upper_orient.view(-1, 1), cochain.lower_orient.view(-1, 1)
        up_adj, down_adj = self._plans(cochain, up_attr, down_attr)
        sts = [self._stream(up_adj, x, up_attr, self.aggr_up), self._stream(down_adj, x, down_attr, self.aggr_down)]
        return ops.aggregate_many(sts)

    def _own_hooks(self) -> bool:
        """Are the message / aggregate / update hooks the class's own (a subclass may have replaced any of them)?"""
        return not (type(self).message_up is not OrientedConv.message_up
                    or type(self).message_down is not OrientedConv.message_down
                    or type(self).message_and_aggregate_up is not OrientedConv.message_and_aggregate_up
                    or type(self).message_and_aggregate_down is not OrientedConv.message_and_aggregate_down
                    or self._overrides['aggregate_up'] or self._overrides['aggregate_down'] or self._overrides['update'])

    def _plans(self, cochain, up_attr, down_attr):
        """The cached plans of the upper and the lower adjacency (the checks of propagate(), mp/cell_mp.py:146-193)."""
        kw = dict(x=cochain.x, up_attr=up_attr, down_attr=down_attr)
        up_size = self.__check_input_separately__(cochain.upper_index, None)
        down_size = self.__check_input_separately__(cochain.lower_index, None)
        self.__check_input_together__(cochain.upper_index, cochain.lower_index, up_size, down_size)
        return (self._adjacency(cochain.upper_index, 'up', up_size, kw),
                self._adjacency(cochain.lower_index, 'down', down_size, kw))

    def fused_operands(self, x):
        """(w_self, w_up, w_down, activation name) when the whole layer is ONE cwn_oriented_layer_f32 launch, else None: x
        float32 on the GPU, the class's own hooks, 'add' reduces, every update map a bias-free torch.nn.Linear of matching
        widths (<= 128) or a ZeroUpdate, the activation one of the five of models.get_nonlinearity.  A Linear with a
        bias, a user callable, float64, CPU tensors, another reduce: the path below, unchanged."""
        if (not FUSED_ORIENTED or not isinstance(x, Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2
                or not self._own_hooks() or (self.aggr_up or 'add') != 'add' or (self.aggr_down or 'add') != 'add'):
            return None
        act = _act_name_of_function(self.act_fn)
        if act is None:
            return None
        ws = []
        for nn in (self.update_nn, self.update_up_nn, self.update_down_nn):
            if type(nn) is ZeroUpdate:
                ws.append(None)
            elif type(nn) is torch.nn.Linear and nn.bias is None:
                ws.append(nn.weight)
            else:
                return None
        if not ops.oriented_layer_applies(x, ws):
            return None
        return ws[0], ws[1], ws[2], act

    def forward(self, cochain):
        assert len(cochain.upper_orient) == cochain.upper_index.size(1)
        assert len(cochain.lower_orient) == cochain.lower_index.size(1)
        fused = self.fused_operands(cochain.x)
        if fused is not None:
            w_self, w_up, w_down, act = fused
            up_adj, down_adj = self._plans(cochain, cochain.upper_orient.view(-1, 1), cochain.lower_orient.view(-1, 1))
            return ops.oriented_layer(cochain.x, up_adj, cochain.upper_orient if self.orient else None,
                                      down_adj, cochain.lower_orient if self.orient else None, w_self, w_up, w_down, act)
        both = self.propagate_both(cochain)
        if both is not None:
            out_up, out_down = both
        else:
            out_up, out_down, _ = self.propagate(
                cochain.upper_index, cochain.lower_index, None, x=cochain.x,
                up_attr=cochain.upper_orient.view(-1, 1), down_attr=cochain.lower_orient.view(-1, 1))
        out_up = self.update_up_nn(out_up)
        out_down = self.update_down_nn(out_down)
        x = self.update_nn(cochain.x)
        return self.act_fn(x + out_up + out_down)

    def reset_parameters(self):
        reset(self.update_up_nn)
        reset(self.update_down_nn)
        reset(self.update_nn)

    def message_up(self, up_x_j: Tensor, up_attr: Tensor) -> Tensor:
        return up_x_j * up_attr if self.orient else up_x_j

    def message_down(self, down_x_j: Tensor, down_attr: Tensor) -> Tensor:
        return down_x_j * down_attr if self.orient else down_x_j

    def _fused(self, adj: Adjacency, x, attr, aggr) -> Tensor:
        if not self.orient:
            return ops.aggregate(adj, adj.n_dst, x, reduce=aggr or 'add')
        attr = dense(attr).to(x.dtype)
        return ops.aggregate(adj, adj.n_dst, x, msg_op=ops.MSG_A_TIMES_B, B=attr, ib_mode='perm',
                             reduce=aggr or 'add')

    def message_and_aggregate_up(self, up_adj_t: Adjacency, x, up_attr) -> Tensor:
        return self._fused(up_adj_t, x, up_attr, self.aggr_up)

    def message_and_aggregate_down(self, down_adj_t: Adjacency, x, down_attr) -> Tensor:
        return self._fused(down_adj_t, x, down_attr, self.aggr_down)


# A GINConv in inference as ONE cwn_gin_layer_f32 launch (csrc/cwn_gin.hip; float32, widths up to 128, a stock two-stage
# network with foldable norms) instead of one aggregation launch and the torch modules of its network (two GEMMs with
# their bias adds, two BatchNorms, two activations).  CWN_FUSED_GIN=1 / =0 turns the route on / off; without it
# FUSED_GIN_DEFAULT decides, which follows the project's rule: on only where the route has measured faster than the
# torch-module route of the same commit by more than the larger run-to-run spread of the two (tools/bench_gin.py,
# profiles/gin_layer.md, 32 rings per batch, both routes alternating in one process: one layer at (64, 64) 44.6 against
# 121.7 us, spread 10.3 us, 1 kernel against 9; RingGIN with 16 layers on 32-rings 727.1 against 1812.7 us, spread 11.4 us,
# 18 kernels against 147; 5 layers on 10-rings 279.2 against 660.7 us, spread 16.7 us).
FUSED_GIN_DEFAULT = True
FUSED_GIN = {'0': False, '1': True}.get(os.environ.get('CWN_FUSED_GIN'), FUSED_GIN_DEFAULT)


# Under a static batch (_ffi.DYN_ROWS: x has the slot's capacity as its row count) the same layers as ONE counted launch,
# cwn_gin_layer_dev_f32 / cwn_gine_layer_dev_f32: the kernels of the host-count entries with the slot's live row count read on
# the device.  CWN_FUSED_GIN_STATIC=1 / =0 turns the route on / off (FUSED_GIN / FUSED_GINE must be on as well); without it
# FUSED_GIN_STATIC_DEFAULT decides, by the project's rule: on only where StaticForward with the counted launches has
# measured faster than StaticForward with the generic route of the same commit by more than the larger p10 .. p90 spread of
# the two (tools/bench_gin_static.py, profiles/gin_static.md: rounds of ten epochs over fresh permutations, the forms
# alternating in one process; EmbedGIN with hidden 128 and 4 layers on 128 ZINC-like molecules 187.3 against 238.9 us per
# batch, spread 2.5 us, 7.2 kernels against 39.2; RingGIN with 16 layers on 32 rings of 32 305.4 against 766.6 us, spread
# 8.9 us, 20.2 kernels against 149.2).
FUSED_GIN_STATIC_DEFAULT = True
FUSED_GIN_STATIC = {'0': False, '1': True}.get(os.environ.get('CWN_FUSED_GIN_STATIC'), FUSED_GIN_STATIC_DEFAULT)


def _gin_fused_stages(nn, eps, x, static: bool = False):
    """([(W, b, scale, shift)] * 2, activation name) of a GINConv's / GINEConv's network when its layer can be ONE launch
    (the route's own switch aside), else None: autograd off, x float32 on the GPU, no static batch (`static`: the caller
    brings a device count, a static batch is what it serves), `nn` a stock Sequential of two (Linear, norm, activation)
    groups whose norms fold, widths within 128."""
    if (torch.is_grad_enabled() or not isinstance(x, Tensor) or not x.is_cuda or x.dtype != torch.float32
            or (_ffi_dyn() and not static)):
        return None
    got = _f64_stages(nn, 2)
    if got is None or not (eps.is_cuda and eps.dtype == torch.float32):
        return None
    stages = []
    for lin, norm in got[0]:
        fold = _fold_norm(norm, lin.out_features)
        if fold is None:
            return None
        stages.append((lin.weight, lin.bias, fold[0], fold[1]))
    return (stages, got[1]) if ops.gin_layer_applies(x, stages) else None


class GINConv(torch.nn.Module):
    """torch_geometric.nn.GINConv (the layer of mp/graph_models.py and of RingGIN, mp/ring_exp_models.py:76-130) with its
    constructor and state: out_i = nn((1 + eps) * x_i + sum_{j -> i} x_j), `edge_index[0]` the source and `[1]` the target;
    `eps` a [1] tensor -- a Parameter with train_eps, a registered buffer otherwise, in the state_dict either way.

    forward has two routes; `last_route` names the one the last call took:
      'fused'    autograd off, float32 on the GPU, `nn` a stock Sequential of two (Linear, norm, activation) groups whose
                 norms fold (eval-mode BatchNorm1d or Identity), widths within 128, FUSED_GIN on, no static batch:
                 csr.cached_adjacency + ONE ops.gin_layer launch.
      'fused_counted'  the same layer under a static batch (a slot of static_batch.StaticBatch, mode 'csr'), FUSED_GIN_STATIC
                 on as well and a device count behind x's row count: the slot's plan + ONE ops.gin_layer_counted launch.
      'generic'  everything else (training, float64, LayerNorm, a custom nn, CPU tensors): on the GPU ops.aggregate with the
                 self term folded in (differentiable, float32 and float64), then `self.nn`; on the CPU index_add_, then
                 `self.nn`.
    `out` (a [n, H] view, e.g. a column slice of a JumpingKnowledge('cat') buffer) is written by the fused route alone: the
    caller sees from the result's data_ptr whether it was.  `act_post` names an activation applied to the result
    (RingGIN's `act(conv1(x))`)."""

    def __init__(self, nn: Callable, eps: float = 0., train_eps: bool = False):
        super().__init__()
        self.nn = nn
        self.initial_eps = eps
        if train_eps:
            self.eps = torch.nn.Parameter(torch.Tensor([eps]))
        else:
            self.register_buffer('eps', torch.Tensor([eps]))
        self.last_route = None
        self.reset_parameters()

    def reset_parameters(self):
        reset(self.nn)
        self.eps.data.fill_(self.initial_eps)

    def fused_stages(self, x):
        """([(W, b, scale, shift)] * 2, activation name) when the whole layer is ONE cwn_gin_layer_f32 launch, else None."""
        return _gin_fused_stages(self.nn, self.eps, x) if FUSED_GIN else None

    def counted_stages(self, x):
        """(stages, activation name, address of the device count) when, under a static batch, the whole layer is ONE
        cwn_gin_layer_dev_f32 launch, else None: FUSED_GIN_STATIC and FUSED_GIN on, a network that folds, and a count behind
        x's row count (_ffi.dyn).  Without a count the answer is None -- the generic route, never a launch over the capacity."""
        if not (FUSED_GIN_STATIC and FUSED_GIN and _ffi_dyn() and isinstance(x, Tensor)):
            return None
        n_dev = ops._ffi.dyn(x.size(0))
        got = _gin_fused_stages(self.nn, self.eps, x, static=True) if n_dev is not None else None
        return None if got is None else (got[0], got[1], n_dev)

    def forward(self, x: Tensor, edge_index: Optional[Tensor], out: Optional[Tensor] = None, act_post: str = 'id') -> Tensor:
        n = x.size(0)
        counted = self.counted_stages(x)
        if counted is not None:
            self.last_route = 'fused_counted'
            adj = None
            if edge_index is not None and edge_index.numel():
                adj = cached_adjacency(edge_index, n, n)
            return ops.gin_layer_counted(x, adj, self.eps, counted[0], counted[1], act_post=act_post, out=out, n_dev=counted[2])
        fused = self.fused_stages(x)
        if fused is not None:
            self.last_route = 'fused'
            adj = None
            if edge_index is not None and edge_index.numel():
                adj = cached_adjacency(edge_index, n, n)
            return ops.gin_layer(x, adj, self.eps, fused[0], fused[1], act_post=act_post, out=out)
        self.last_route = 'generic'
        if x.is_cuda:
            adj = None
            if edge_index is not None and edge_index.numel():
                adj = cached_adjacency(edge_index, n, n)
            s = ops.aggregate(adj, n, A=x, self_x=x, eps=self.eps)
        else:
            s = (1 + self.eps.to(x.dtype)) * x
            if edge_index is not None and edge_index.numel():
                s = torch.zeros_like(x).index_add_(0, edge_index[1], x[edge_index[0]]) + s
        y = self.nn(s)
        return y if act_post == 'id' else ACTIVATIONS[act_post][1](y)

    def __repr__(self):
        return f'{self.__class__.__name__}(nn={self.nn})'


# A GINEConv in inference as ONE cwn_gine_layer_f32 launch (csrc/cwn_gine.hip: the GIN kernel with relu(x_j + e_ji) as its
# message) instead of one aggregation launch (CWN_MSG_RELU_A_PLUS_B) and the torch modules of its network.
# CWN_FUSED_GINE=1 / =0 turns the route on / off; without it FUSED_GINE_DEFAULT decides, by the project's rule: on only
# where the route has measured faster than the generic route of the same commit by more than the larger run-to-run spread
# of the two, both routes alternating in one process (tools/bench_gine.py, profiles/gine_layer.md, 128 ZINC-like molecules
# per batch, rounds of 400 forwards: one layer at (64, 64) 59.5 against 112.4 us, spread 5.8 us, and at (128, 128) 59.3 against
# 111.3 us, spread 0.9 us, 1 kernel against 9; EmbedGIN with hidden 128 and 4 layers 326.9 against 547.5 us, spread 20.0 us, 7
# kernels against 39; rounds of 50 forwards on another machine: 62.0 against 129.0, 62.4 against 128.8, 339.0 against 589.3 us).
FUSED_GINE_DEFAULT = True
FUSED_GINE = {'0': False, '1': True}.get(os.environ.get('CWN_FUSED_GINE'), FUSED_GINE_DEFAULT)


def _edge_rows(edge_attr) -> Tensor:
    """One row per entry from an edge attribute that is lazy (IndexedRows) or dense, on either device."""
    if isinstance(edge_attr, IndexedRows):
        return edge_attr.tensor() if edge_attr.src.is_cuda else edge_attr.src[edge_attr.index]
    return edge_attr


class GINEConv(torch.nn.Module):
    """torch_geometric.nn.GINEConv as version 1.6.3 defines it (the layer of EmbedGIN, mp/molec_models.py:506-606) with its
    constructor and state: out_i = nn((1 + eps) * x_i + sum_{j -> i} relu(x_j + e_ji)), `edge_index[0]` the source and `[1]`
    the target; `eps` a [1] tensor -- a Parameter with train_eps, a registered buffer otherwise, in the state_dict either way.
    `edge_attr` is one row per entry of edge_index, or a cell_mp.IndexedRows (the `up_attr` a Complex hands out): then the
    rows of the edge cochain are read through the adjacency's shared-cell index and [E, w] is never materialised.
    edge_index None or empty: a graph without edges, edge_attr is not looked at.

    forward has two routes; `last_route` names the one the last call took:
      'fused'    autograd off, float32 on the GPU, `nn` a stock Sequential of two (Linear, norm, activation) groups whose
                 norms fold (eval-mode BatchNorm1d or Identity), widths within 128, the edge features float32, on the GPU
                 and as wide as x, FUSED_GINE on, no static batch: csr.cached_adjacency + ONE ops.gine_layer launch.
      'fused_counted'  the same layer under a static batch, FUSED_GIN_STATIC on as well and a device count behind x's row
                 count: the slot's plan (with its shared-coboundary index) + ONE ops.gine_layer_counted launch.
      'generic'  everything else: on the GPU ops.aggregate with the message relu(A + B) and the self term folded in
                 (differentiable with respect to x, the edge features and eps, float32 and float64), then `self.nn`; on
                 the CPU, and where the aggregation does not take the operands (edge features of another width, which
                 broadcast as in torch_geometric), the formula in plain torch, then `self.nn`.
    `out` and `act_post` as in GINConv."""

    def __init__(self, nn: Callable, eps: float = 0., train_eps: bool = False):
        super().__init__()
        self.nn = nn
        self.initial_eps = eps
        if train_eps:
            self.eps = torch.nn.Parameter(torch.Tensor([eps]))
        else:
            self.register_buffer('eps', torch.Tensor([eps]))
        self.last_route = None
        self.reset_parameters()

    def reset_parameters(self):
        reset(self.nn)
        self.eps.data.fill_(self.initial_eps)

    def fused_stages(self, x, edge=None):
        """([(W, b, scale, shift)] * 2, activation name) when the whole layer is ONE cwn_gine_layer_f32 launch, else None.
        `edge`: the matrix the launch would read (an IndexedRows' src, or the dense rows); None: no edges."""
        got = _gin_fused_stages(self.nn, self.eps, x) if FUSED_GINE else None
        return got if got is not None and ops.gine_layer_applies(x, edge, got[0]) else None

    def counted_stages(self, x, edge=None):
        """(stages, activation name, address of the device count) when, under a static batch, the whole layer is ONE
        cwn_gine_layer_dev_f32 launch, else None: FUSED_GIN_STATIC and FUSED_GINE on, a network that folds, edge features the
        launch takes, and a count behind x's row count (_ffi.dyn).  Without a count: None -- the generic route."""
        if not (FUSED_GIN_STATIC and FUSED_GINE and _ffi_dyn() and isinstance(x, Tensor)):
            return None
        n_dev = ops._ffi.dyn(x.size(0))
        got = _gin_fused_stages(self.nn, self.eps, x, static=True) if n_dev is not None else None
        if got is None or not ops.gine_layer_applies(x, edge, got[0]):
            return None
        return got[0], got[1], n_dev

    def forward(self, x: Tensor, edge_index: Optional[Tensor], edge_attr=None, out: Optional[Tensor] = None,
                act_post: str = 'id') -> Tensor:
        n = x.size(0)
        has_edges = edge_index is not None and edge_index.numel() > 0
        edge, mode = _attr_operand(edge_attr) if has_edges else (None, 'aux')
        if has_edges and edge is None:
            raise ValueError('GINEConv: edge_index has entries and edge_attr is None')
        aux = (edge_attr.index, edge.size(0)) if mode == 'aux' and has_edges else (None, 0)
        counted = self.counted_stages(x, edge)
        if counted is not None:
            self.last_route = 'fused_counted'
            adj = cached_adjacency(edge_index, n, n, *aux) if has_edges else None
            return ops.gine_layer_counted(x, adj, edge, self.eps, counted[0], counted[1], act_post=act_post, out=out,
                                          edge_mode=mode, n_dev=counted[2])
        fused = self.fused_stages(x, edge)
        if fused is not None:
            self.last_route = 'fused'
            adj = cached_adjacency(edge_index, n, n, *aux) if has_edges else None
            return ops.gine_layer(x, adj, edge, self.eps, fused[0], fused[1], act_post=act_post, out=out, edge_mode=mode)
        self.last_route = 'generic'
        takes = (x.is_cuda and x.dtype in (torch.float32, torch.float64)
                 and (not has_edges or (isinstance(edge, Tensor) and edge.dim() == 2 and edge.dtype == x.dtype
                                        and edge.device == x.device and edge.size(1) == x.size(1))))
        if takes and has_edges:
            s = ops.aggregate(cached_adjacency(edge_index, n, n, *aux), n, A=x, B=edge, msg_op=ops.MSG_RELU_A_PLUS_B,
                              ib_mode=mode, self_x=x, eps=self.eps)
        elif takes:
            s = ops.aggregate(None, n, A=x, self_x=x, eps=self.eps)
        else:
            s = (1 + self.eps.to(x.dtype)) * x
            if has_edges:
                msg = torch.relu(x[edge_index[0]] + _edge_rows(edge_attr))
                s = torch.zeros_like(x).index_add_(0, edge_index[1], msg) + s
        y = self.nn(s)
        return y if act_post == 'id' else ACTIVATIONS[act_post][1](y)

    def __repr__(self):
        return f'{self.__class__.__name__}(nn={self.nn})'


class InitReduceConv(torch.nn.Module):
    """mp/layers.py:473-487: initial features of d-cells = reduce of their boundary cells'.

    The reference sizes the output by `boundary_index[1].max() + 1` (a device sync on the GPU);
    pass `num_cells` to avoid it -- EmbedVEWithReduce does."""

    def __init__(self, reduce='add'):
        super().__init__()
        self.reduce = reduce

    def forward(self, boundary_x, boundary_index, num_cells: Optional[int] = None):
        from .csr import cached_adjacency
        if num_cells is None:
            num_cells = int(boundary_index[1, :].max()) + 1
        red = 'add' if self.reduce in ('add', 'sum') else self.reduce
        adj = cached_adjacency(boundary_index, num_cells, boundary_x.size(0))
        if red == 'min':
            return -ops.aggregate(adj, num_cells, -boundary_x, reduce='max')
        return ops.aggregate(adj, num_cells, boundary_x, reduce=red)


def _embed(layer, idx: Tensor) -> Tensor:
    """A torch.nn.Embedding, or a module holding a list of them whose outputs are summed over the
    index columns (the OGB Atom/BondEncoder form), as one fused gather-sum (ops.embedding_sum);
    anything else is called as it is."""
    def plain(e):
        return (isinstance(e, torch.nn.Embedding) and e.padding_idx is None and e.max_norm is None
                and not e.sparse and not e.scale_grad_by_freq)
    if idx.is_cuda and idx.numel() > 0:
        if plain(layer) and idx.dim() == 1:
            return ops.embedding_sum([layer.weight], idx)
        tables = None
        for name in ('atom_embedding_list', 'bond_embedding_list'):
            if hasattr(layer, name):
                tables = list(getattr(layer, name))
        if tables is not None and idx.dim() == 2 and idx.size(1) == len(tables) and all(plain(e) for e in tables):
            return ops.embedding_sum([e.weight for e in tables], idx)
    return layer(idx)


class AbstractEmbedVEWithReduce(torch.nn.Module, ABC):
    """mp/layers.py:490-547."""

    def __init__(self, v_embed_layer: Callable, e_embed_layer: Optional[Callable],
                 init_reduce: InitReduceConv):
        super().__init__()
        self.v_embed_layer = v_embed_layer
        self.e_embed_layer = e_embed_layer
        self.init_reduce = init_reduce

    @abstractmethod
    def _prepare_v_inputs(self, v_params):
        pass

    @abstractmethod
    def _prepare_e_inputs(self, e_params):
        pass

    def _check_v_inputs(self, v_params):      # the shape asserts of _prepare_*_inputs without the dtype conversion
        assert v_params.x is not None and v_params.x.dim() == 2

    def _check_e_inputs(self, e_params):
        assert self.e_embed_layer is not None and e_params.x.dim() == 2

    def forward(self, *cochain_params: CochainMessagePassingParams):
        assert 1 <= len(cochain_params) <= 3
        v_params = cochain_params[0]
        e_params = cochain_params[1] if len(cochain_params) >= 2 else None
        c_params = cochain_params[2] if len(cochain_params) == 3 else None
        fused = self._forward_fused(v_params, e_params, c_params)
        if fused is not None:
            return fused
        vx = _embed(self.v_embed_layer, self._prepare_v_inputs(v_params))
        out = [vx]
        if e_params is None:
            assert c_params is None
            return out
        n_e = getattr(e_params, 'num_cells', None) or (e_params.x.size(0) if e_params.x is not None else None)
        reduced_ex = self.init_reduce(vx, e_params.boundary_index, n_e)
        ex = reduced_ex
        if e_params.x is not None:
            ex = _embed(self.e_embed_layer, self._prepare_e_inputs(e_params))
            assert ex.size(1) == vx.size(1)
        out.append(ex)
        if c_params is not None:
            n_c = getattr(c_params, 'num_cells', None) or (c_params.x.size(0) if c_params.x is not None else None)
            # halved as in the reference (:538-540)
            out.append(self.init_reduce(reduced_ex, c_params.boundary_index, n_c) / 2.)
        return out

    def _forward_fused(self, v_params, e_params, c_params) -> Optional[List[Tensor]]:
        """The whole front in ONE launch (ops.embed_front, csrc/cwn_ends.hip): both embeddings, the reduction of
        the vertex embeddings onto the edges and of that onto the rings, halved -- the 8 launches below it were 29 us
        of a 167 us forward at the ZINC batch of 128.  Plain embedding tables and 'sum' reduction; with autograd
        (training) the same launch behind ops._EmbedFrontTrain.  None otherwise (the caller runs the separate launches)."""
        if not ops.FUSED_ENDS or e_params is None or v_params.x is None or not v_params.x.is_cuda:
            return None
        infer = not torch.is_grad_enabled()
        bi1, bi2 = e_params.boundary_index, (c_params.boundary_index if c_params is not None else None)
        ent = _FRONT_CACHE.get(self, {}).get(id(bi1)) if infer else None
        if (ent is not None and ent[1] == (c_params is not None, self.init_reduce.reduce) and ent[0].current(bi1, bi2)
                and (ent[0].te is not None) == (e_params.x is not None)):
            xs = ent[0].run(v_params.x, e_params.x)
            if xs is not None:
                return xs if c_params is not None else xs[:2]
        if self.init_reduce.reduce not in ('add', 'sum'):
            return None
        vt = _embedding_tables(self.v_embed_layer)
        et = _embedding_tables(self.e_embed_layer) if e_params.x is not None else None
        if vt is None or (e_params.x is not None and et is None):
            return None
        train = torch.is_grad_enabled() and any(w.requires_grad for w in vt + (et or []))
        if (len(vt) > 1 or (et is not None and len(et) > 1)) and not FUSED_OGB_FRONT:
            # OGB-style encoders (a table per integer feature column: 9 + 3 at molhiv).  ONE launch is slower there (44 - 60
            # us at the molhiv batch of 512: every ring row walks twelve vertices of nine columns), so cwn_embed_front_f32
            # makes it two -- the embeddings of both cell types, then the reductions from the x0 rows (round 6: 15 us against
            # the 40 us of the seven separate launches; in training the same forward behind ops._EmbedFrontTrain, whose
            # backward is the launches the separate path's autograd ran).
            return None
        if train and not ops.FUSED_FRONT_TRAINING:
            return None
        H = int(vt[0].size(1))
        if H % 4 != 0 or any(w.size(1) != H or not w.is_cuda or w.dtype != torch.float32 for w in vt + (et or [])):
            return None
        self._check_v_inputs(v_params)
        if e_params.x is not None:
            self._check_e_inputs(e_params)
        from .csr import cached_adjacency
        n0 = int(v_params.x.size(0))
        n1 = getattr(e_params, 'num_cells', None) or (e_params.x.size(0) if e_params.x is not None else None)
        if n1 is None or n0 == 0:
            return None
        n1 = int(n1)
        adj1 = cached_adjacency(e_params.boundary_index, n1, n0) if e_params.boundary_index is not None and n1 > 0 else None
        n2, adj2 = 0, None
        if c_params is not None:
            n2 = getattr(c_params, 'num_cells', None) or (c_params.x.size(0) if c_params.x is not None else None)
            if n2 is None:
                return None
            n2 = int(n2)
            if c_params.boundary_index is not None and n2 > 0 and n1 > 0:
                adj2 = cached_adjacency(c_params.boundary_index, n2, n1)
        if e_params.x is None and adj1 is None:
            return None                   # edges without features and without boundaries: let the plain path raise
        if train:
            if H * sum(int(w.size(0)) for w in vt) * 4 > 60 * 1024 or (et and H * sum(int(w.size(0)) for w in et) * 4 > 60 * 1024):
                return None               # tables beyond the LDS-table backward kernel: the generic path
            xs = ops.embed_front_train(vt, v_params.x, et, e_params.x if et is not None else None, n1, adj1, n2, adj2, halve=True)
        else:
            ex = e_params.x if et is not None else None
            if infer and not _ffi_dyn() and all(f is None or (f.dim() == 2 and f.is_contiguous() and f.dtype in (torch.float32, torch.long))
                                                for f in (v_params.x, ex)):
                # the prepared form of this launch for the next call on this batch (ops.FrontLaunch)
                launch = ops.FrontLaunch(vt, et, n0, n1, adj1, n2, adj2, True, bi1, bi2, v_params.x, ex)
                cache = _FRONT_CACHE.setdefault(self, {})            # (per batch, like _BLOCKED_CACHE: loops over a few batches)
                if len(cache) >= 16:
                    cache.clear()
                cache[id(bi1)] = (launch, (c_params is not None, self.init_reduce.reduce))
                xs = launch.run(v_params.x, ex)
                if xs is not None:
                    return xs if c_params is not None else xs[:2]
            xs = ops.embed_front(vt, v_params.x, et, ex, n1, adj1, n2, adj2, halve=True)
        return xs if c_params is not None else xs[:2]

    def reset_parameters(self):
        reset(self.v_embed_layer)
        reset(self.e_embed_layer)


def _embedding_tables(layer) -> Optional[List[Tensor]]:
    """The weight(s) of a plain torch.nn.Embedding or of an OGB-style encoder (a list of them, summed over the
    feature columns); None for anything else."""
    def plain(e):
        return (isinstance(e, torch.nn.Embedding) and e.padding_idx is None and e.max_norm is None
                and not e.sparse and not e.scale_grad_by_freq)
    if layer is None:
        return None
    if plain(layer):
        return [layer.weight]
    for name in ('atom_embedding_list', 'bond_embedding_list'):
        if hasattr(layer, name):
            tables = list(getattr(layer, name))
            return [e.weight for e in tables] if tables and all(plain(e) for e in tables) else None
    return None


class EmbedVEWithReduce(AbstractEmbedVEWithReduce):
    """mp/layers.py:550-570."""

    def _check_v_inputs(self, v_params):
        assert v_params.x is not None
        assert v_params.x.dim() == 2
        assert v_params.x.size(1) == 1

    def _check_e_inputs(self, e_params):
        assert self.e_embed_layer is not None
        assert e_params.x.dim() == 2
        assert e_params.x.size(1) == 1

    def _prepare_v_inputs(self, v_params):
        self._check_v_inputs(v_params)
        return v_params.x.squeeze(1).to(dtype=torch.long)

    def _prepare_e_inputs(self, e_params):
        self._check_e_inputs(e_params)
        return e_params.x.squeeze(1).to(dtype=torch.long)


class OGBEmbedVEWithReduce(AbstractEmbedVEWithReduce):
    """mp/layers.py:573-593 (the OGB Atom/Bond encoders themselves are third-party; any module
    mapping integer feature columns to embeddings fits)."""

    def _check_v_inputs(self, v_params):
        assert v_params.x is not None
        assert v_params.x.dim() == 2

    def _check_e_inputs(self, e_params):
        assert self.e_embed_layer is not None
        assert e_params.x.dim() == 2

    def _prepare_v_inputs(self, v_params):
        self._check_v_inputs(v_params)
        return v_params.x.to(dtype=torch.long)

    def _prepare_e_inputs(self, e_params):
        self._check_e_inputs(e_params)
        return e_params.x.to(dtype=torch.long)
