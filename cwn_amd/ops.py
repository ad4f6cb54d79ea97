"""Differentiable ops over the C ABI (include/cwn_hip.h).  Forward AND backward run the HIP
kernels of csrc/cwn_aggregate.hip: the gradient of a gather is a segmented reduce over the
transposed CSR and vice versa, so both directions are the same kernel on different plans.

`aggregate_many` runs any number of aggregation STREAMS (one stream = one adjacency of one cochain
dimension) in ONE kernel launch forward and ONE launch backward; `aggregate` is its single-stream
form.  There is no CPU path here by design; `oracle/` is the CPU checker.
"""
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import ctypes as C
import os
import weakref

import torch
from torch import Tensor

from . import _ffi
from ._window import aligned16, is_rowmajor, is_vec16, ld, rowmajor, rowmajor16
from .csr import Adjacency, wait_ready

MSG_A, MSG_A_PLUS_B, MSG_A_TIMES_B, MSG_RELU_A_PLUS_B, MSG_A_MASK_RELU, MSG_RELU_A_PLUS_B_SQ, MSG_A_TIMES_2RELU = range(7)


def _f32c(t: Optional[Tensor], name: str) -> Optional[Tensor]:
    """An operand of a kernel that exists in fp32 only (the fused layer / MLP / head / stage launches, the GEMMs, the
    embedding kernels).  The aggregate and the gather also run in float64: `_fc`."""
    if t is None:
        return None
    _ffi.require_gpu(t, name)
    if t.dtype != torch.float32:
        raise TypeError(f'{name} must be float32 (got {t.dtype}): this kernel computes in fp32 only '
                        '(float64 runs through aggregate_many / gather_rows and the torch modules)')
    return t.contiguous()


def _fc(t: Optional[Tensor], name: str) -> Optional[Tensor]:
    """An operand of the aggregate / gather kernels: on the GPU, float32 or float64, contiguous."""
    if t is None:
        return None
    _ffi.require_gpu(t, name)
    if t.dtype not in _ffi.FLOAT_DTYPES:
        raise TypeError(f'{name} must be float32 or float64 (got {t.dtype}); the engine computes in fp32 or fp64')
    return t.contiguous()


def _common_dtype(named) -> torch.dtype:
    """The one dtype of the tensor operands of a stream (`named`: (name, tensor or None) pairs); float32 without any."""
    first = None
    for name, t in named:
        dt = getattr(t, 'dtype', None)
        if dt is None:
            continue
        if first is None:
            first = (name, dt)
        elif dt != first[1]:
            raise TypeError(f'the operands of one stream share one dtype: {first[0]} is {first[1]}, {name} is {dt}')
    return torch.float32 if first is None else first[1]


def require_float32_model(model, what: str) -> None:
    """The captured / prepared machinery (StaticForward, TrainStep and what they are built of: FlatAdam, the blocked and
    fused launches, the C-ABI GEMMs) is float32 by construction.  A float64 model runs eagerly: model(batch), autograd and
    torch.optim, over cwn_aggregate_f64 / cwn_gather_rows_f64 and the torch modules."""
    for name, t in list(model.named_parameters()) + list(model.named_buffers()):
        if t.is_floating_point() and t.dtype != torch.float32:
            raise TypeError(f'{what} runs float32 models only: {name} is {t.dtype}.  A float64 model runs eagerly -- '
                            'model(batch), autograd and a torch.optim optimizer')


AGG_SMALL_OPERANDS = 1      # = CWN_AGG_SMALL_OPERANDS (include/cwn_hip.h)
# tests (and CWN_AGG_WIDE=1, for A/B timing) turn this off to run the 64-bit-address kernels on small inputs
ALLOW_SMALL_OPERANDS = os.environ.get('CWN_AGG_WIDE') != '1'


@dataclass
class AggSpec:
    """One descriptor of cwn_aggregate_f32 / cwn_aggregate_f64.  `ia`/`ib` are int32 tensors in CSR order.  `dtype`
    (float32 / float64) is that of every tensor operand; left None it is taken from A, else (adj=None) from self_x."""
    adj: Optional[Adjacency]
    n_dst: int
    F: int
    A: Optional[Tensor] = None
    ia: Optional[Tensor] = None
    B: Optional[Tensor] = None
    ib: Optional[Tensor] = None
    msg_op: int = MSG_A
    reduce: int = 0
    self_x: Optional[Tensor] = None
    eps: Optional[Tensor] = None
    self_pre: Optional[Tensor] = None
    out: Optional[Tensor] = None
    self_x2: Optional[Tensor] = None     # second self term: out += (1 + eps2) * self_x2
    eps2: Optional[Tensor] = None
    dtype: Optional[torch.dtype] = None

    def resolve_dtype(self) -> torch.dtype:
        if self.dtype is None:
            self.dtype = _common_dtype([('A', self.A), ('B', self.B), ('self_x', self.self_x), ('self_x2', self.self_x2),
                                        ('self_pre', self.self_pre), ('out', self.out)])
        return self.dtype

    def desc(self) -> _ffi.AggDesc:
        # an index with E = 0 is legal (mp/test_cell_mp.py:137-176) and behaves like an absent one
        absent = self.adj is None or self.adj.n_entries == 0
        bw = self.F if (self.B is None or self.B.size(1) == self.F) else int(self.B.size(1))
        # gathered operands within 4 GiB of their base pointers: 32-bit row offsets in the kernel
        esize = 8 if self.resolve_dtype() == torch.float64 else 4
        small = ALLOW_SMALL_OPERANDS and all(t is None or t.numel() * esize < (1 << 32) for t in (self.A, self.B))
        return _ffi.AggDesc(
            flags=AGG_SMALL_OPERANDS if small else 0,
            rowptr=None if absent else self.adj.rowptr.data_ptr(),
            ia=_ffi.ptr(self.ia), ib=_ffi.ptr(self.ib), A=_ffi.ptr(self.A), B=_ffi.ptr(self.B),
            self_x=_ffi.ptr(self.self_x), eps=_ffi.ptr(self.eps), self_pre=_ffi.ptr(self.self_pre),
            out=self.out.data_ptr(),
            long_rows=None if absent else _ffi.ptr(self.adj.long_rows),
            n_long=None if absent else _ffi.ptr(self.adj.n_long),
            long_cap=0 if absent else self.adj.long_cap,
            n_dst=self.n_dst, F=self.F, b_width=bw,
            msg_op=self.msg_op, reduce=self.reduce,
            self_x2=_ffi.ptr(self.self_x2), eps2=_ffi.ptr(self.eps2))


def run_aggregate(specs: Sequence[AggSpec], device) -> List[Tensor]:
    """Raw launch (no autograd): allocates missing outputs, ONE kernel per <= 8 descriptors of one dtype (the float32 and
    the float64 descriptors of a call are launched separately)."""
    for s in specs:
        if s.out is None:
            s.out = torch.empty(s.n_dst, s.F, dtype=s.resolve_dtype(), device=device)
    live = [s for s in specs if s.n_dst > 0]
    if live:
        late = [s.adj for s in live if s.adj is not None and not s.adj.built]     # handed out under csr.deferred_builds
        if late:
            from .csr import build_many
            build_many(late)
        wait_ready([s.adj for s in live])      # plans built on the side stream (csr.build_many)
        by_dtype = {}
        for s in live:
            by_dtype.setdefault(s.resolve_dtype(), []).append(s.desc())
        for dt, descs in by_dtype.items():
            _ffi.aggregate(descs, device, dt)
    return [s.out for s in specs]


@dataclass
class AggActSpec:
    """One descriptor of cwn_aggregate_act_f32 / cwn_aggregate_act_f64: out = sum_p act(A[ia[p]] + B[ib[p]]) + (1 + eps)
    self_x.  `ia` / `ib` are int32 tensors in CSR order, B has the width of A, `act` is a CWN_ACT_* code."""
    adj: Optional[Adjacency]
    n_dst: int
    F: int
    act: int
    A: Optional[Tensor] = None
    ia: Optional[Tensor] = None
    B: Optional[Tensor] = None
    ib: Optional[Tensor] = None
    self_x: Optional[Tensor] = None
    eps: Optional[Tensor] = None
    out: Optional[Tensor] = None
    dtype: Optional[torch.dtype] = None

    def resolve_dtype(self) -> torch.dtype:
        if self.dtype is None:
            self.dtype = _common_dtype([('A', self.A), ('B', self.B), ('self_x', self.self_x), ('out', self.out)])
        return self.dtype

    def desc(self) -> _ffi.AggActDesc:
        absent = self.adj is None or self.adj.n_entries == 0
        esize = 8 if self.resolve_dtype() == torch.float64 else 4
        small = ALLOW_SMALL_OPERANDS and all(t is None or t.numel() * esize < (1 << 32) for t in (self.A, self.B))
        return _ffi.AggActDesc(
            flags=AGG_SMALL_OPERANDS if small else 0,
            rowptr=None if absent else self.adj.rowptr.data_ptr(),
            ia=_ffi.ptr(self.ia), ib=_ffi.ptr(self.ib), A=_ffi.ptr(self.A), B=_ffi.ptr(self.B),
            self_x=_ffi.ptr(self.self_x), eps=_ffi.ptr(self.eps), out=self.out.data_ptr(),
            long_rows=None if absent else _ffi.ptr(self.adj.long_rows),
            n_long=None if absent else _ffi.ptr(self.adj.n_long),
            long_cap=0 if absent else self.adj.long_cap,
            n_dst=self.n_dst, F=self.F, act=self.act)


def _run_act_specs(specs: Sequence, device, launch) -> List[Tensor]:
    """What run_aggregate_act and run_aggregate_act_bwd do once their operands are checked: allocate missing outputs, build
    the plans handed out late, wait for those built on the side stream, and `launch` the descriptors dtype by dtype."""
    for s in specs:
        if s.out is None:
            s.out = torch.empty(s.n_dst, s.F, dtype=s.resolve_dtype(), device=device)
    live = [s for s in specs if s.n_dst > 0]
    if live:
        late = [s.adj for s in live if s.adj is not None and not s.adj.built]
        if late:
            from .csr import build_many
            build_many(late)
        wait_ready([s.adj for s in live])
        by_dtype = {}
        for s in live:
            by_dtype.setdefault(s.resolve_dtype(), []).append(s.desc())
        for dt, descs in by_dtype.items():
            launch(descs, device, dt)
    return [s.out for s in specs]


def run_aggregate_act(specs: Sequence[AggActSpec], device) -> List[Tensor]:
    """Raw launch of the activated message (no autograd): allocates missing outputs, ONE kernel per <= 8 descriptors of one
    dtype.  Row counts are host counts: the launch has no device-side row count, so it refuses to run under
    `_ffi.dynamic_rows` (no static batch reaches it)."""
    if _ffi.DYN_ROWS:
        raise _ffi.CwnError('cwn_aggregate_act_* has no device-side row count: it does not serve static batches')
    for s in specs:
        if s.dtype is not None and s.dtype not in _ffi.FLOAT_DTYPES:
            raise TypeError(f'aggregate_act computes in float32 or float64, not {s.dtype}')
    return _run_act_specs(specs, device, _ffi.aggregate_act)


# The backward of a stream with an activation (Stream.act) as descriptors of cwn_aggregate_act_bwd_f32 / _f64 over the
# transposed plans (csrc/cwn_aggregate_act_bwd.hip): with it on, aggregate_many is differentiable for such streams and
# layers.SparseCINCochainConv._up_kind() answers 'cat_linear_act' under a recording autograd too.  Off (the default, whatever
# tools/bench_act_message_train.py measures: profiles/act_message_train.md) such a stream is inference only, as before.
ACT_MESSAGE_BACKWARD = os.environ.get('CWN_ACT_MESSAGE_BACKWARD') == '1'


@dataclass
class AggActBwdSpec:
    """One descriptor of cwn_aggregate_act_bwd_f32 / _f64: out[r] = sum_p g[ig[p]] * act'(P[r] + Q[iq[p]]) over the
    transposed plan `adj` (rows = the rows of P).  `ig` / `iq` are int32 tensors in that plan's CSR order."""
    adj: Adjacency
    F: int
    act: int
    g: Tensor
    ig: Tensor
    P: Tensor
    Q: Tensor
    iq: Tensor
    out: Optional[Tensor] = None

    @property
    def n_dst(self) -> int:
        return self.adj.n_dst

    def resolve_dtype(self) -> torch.dtype:
        return self.g.dtype

    def desc(self) -> _ffi.AggActBwdDesc:
        absent = self.adj.n_entries == 0
        esize = 8 if self.g.dtype == torch.float64 else 4
        small = ALLOW_SMALL_OPERANDS and all(t.numel() * esize < (1 << 32) for t in (self.g, self.Q))
        return _ffi.AggActBwdDesc(
            flags=AGG_SMALL_OPERANDS if small else 0,
            rowptr=None if absent else self.adj.rowptr.data_ptr(),
            ig=_ffi.ptr(self.ig), iq=_ffi.ptr(self.iq), g=_ffi.ptr(self.g), P=_ffi.ptr(self.P), Q=_ffi.ptr(self.Q),
            out=self.out.data_ptr(),
            long_rows=None if absent else _ffi.ptr(self.adj.long_rows),
            n_long=None if absent else _ffi.ptr(self.adj.n_long),
            long_cap=0 if absent else self.adj.long_cap,
            n_dst=self.adj.n_dst, F=self.F, act=self.act)


def run_aggregate_act_bwd(specs: Sequence[AggActBwdSpec], device) -> List[Tensor]:
    """Raw launch of the activated message's backward: allocates missing outputs, ONE kernel per <= 8 descriptors of one
    dtype.  Host row counts, as `run_aggregate_act`: it refuses to run under `_ffi.dynamic_rows`."""
    if _ffi.DYN_ROWS:
        raise _ffi.CwnError('cwn_aggregate_act_bwd_* has no device-side row count: it does not serve static batches')
    for s in specs:
        for name, t in (('g', s.g), ('P', s.P), ('Q', s.Q)):
            if t.dtype != s.g.dtype or t.dtype not in _ffi.FLOAT_DTYPES or not t.is_contiguous() or t.size(1) != s.F:
                raise TypeError(f'aggregate_act_bwd: {name} must be a contiguous float32 / float64 [*, {s.F}] matrix of the '
                                f"stream's dtype (got {t.dtype}, {tuple(t.shape)})")
        if s.P.size(0) != s.adj.n_dst:
            raise ValueError(f'aggregate_act_bwd: P has {s.P.size(0)} rows, the transposed plan {s.adj.n_dst}')
    return _run_act_specs(specs, device, _ffi.aggregate_act_bwd)


def _act_backward_entries(act: int, z: Tensor, g: Tensor) -> Tensor:
    """g * act'(z) entry by entry with tensor ops, by the formulas of cwn_act.h (activate_bwd): the per-ENTRY operand of
    an activated stream ('perm' mode), which has no reduction."""
    if act == _ffi.ACT_RELU:
        return torch.where(z <= 0, torch.zeros_like(g), g)
    if act == _ffi.ACT_ELU:
        return torch.where(z > 0, g, g * torch.exp(z))
    if act == _ffi.ACT_TANH:
        y = torch.tanh(z)
        return g * (1 - y * y)
    if act == _ffi.ACT_SIGMOID:
        y = torch.sigmoid(z)
        return g * (y * (1 - y))
    return g


@dataclass
class Stream:
    """One aggregation stream:  out = reduce_p msg(A[ia[p]], B[ib[p]])  (+ (1 + eps) * self_x).

    adj      destination-sorted CSR, or None for an ABSENT adjacency (out = zeros + self term,
             CochainMessagePassing.update's zero fill, mp/cell_mp.py:517-522)
    ia_mode  'col'  A is a cell-feature matrix gathered through the adjacency's source index
             'perm' A holds one row per entry (output of a Python message hook; K2 alone)
    ib_mode  'aux'  B is a cell-feature matrix gathered through the adjacency's shared-cell index
             'perm' B holds one row per entry (e.g. `up_attr` as data/complex.py:579-580
                    materialises it)
    act      None, or an activation ('id' | 'relu' | 'elu' | 'tanh' | 'sigmoid', or its CWN_ACT_* code: ACT_CODES) applied
             to the message A + B: out = sum_p act(A[ia[p]] + B[ib[p]]) (+ self term).  Only with msg_op == MSG_A_PLUS_B,
             reduce == 'add' and a B as wide as A; the stream then runs on cwn_aggregate_act_f32 / _f64
             (run_aggregate_act); inference only unless ACT_MESSAGE_BACKWARD is on (run_aggregate_act_bwd).
    """
    adj: Optional[Adjacency]
    n_dst: int
    width: int
    A: Optional[Tensor] = None
    B: Optional[Tensor] = None
    msg_op: int = MSG_A
    reduce: str = 'add'
    ia_mode: str = 'col'
    ib_mode: str = 'aux'
    self_x: Optional[Tensor] = None
    eps: Optional[Tensor] = None
    dtype: Optional[torch.dtype] = None      # set by validate(): the one dtype of A, B and self_x
    act: Optional[object] = None

    def validate(self):
        if self.act is not None:
            _act_code(self.act)
            if self.msg_op != MSG_A_PLUS_B or self.reduce not in ('add', 'sum'):
                raise ValueError("a stream with an activation is act(A + B) summed: msg_op must be MSG_A_PLUS_B and reduce 'add' "
                                 f'(got msg_op {self.msg_op}, reduce {self.reduce!r})')
            if self.adj is not None and (self.A is None or self.B is None or self.A.dim() != 2 or self.B.dim() != 2
                                         or self.B.size(1) != self.A.size(1)):
                raise ValueError('a stream with an activation takes a B as wide as A (no scalar attribute): '
                                 f'A {None if self.A is None else tuple(self.A.shape)}, B {None if self.B is None else tuple(self.B.shape)}')
        self.A, self.B = _fc(self.A, 'A'), _fc(self.B, 'B')
        self.self_x, self.eps = _fc(self.self_x, 'self_x'), _fc(self.eps, 'eps')
        # one dtype per stream; eps, a device scalar (usually a parameter), follows it
        named = [('A', self.A), ('B', self.B), ('self_x', self.self_x)]
        if self.dtype is None or any(t is not None for _, t in named):      # (no tensor at all: zero rows of the given dtype)
            self.dtype = _common_dtype(named)
        if self.eps is not None and self.eps.dtype != self.dtype:
            self.eps = self.eps.to(self.dtype)
        adj = self.adj
        if adj is None:
            self.A = self.B = None
            return
        if self.ia_mode == 'col' and self.A.size(0) != adj.n_val:
            raise ValueError(f'Encountered tensor with size {self.A.size(0)} in dimension -2, '
                             f'but expected size {adj.n_val}.')
        if self.ia_mode == 'perm' and self.A.size(0) != adj.n_entries:
            raise ValueError(f'expected one message row per entry ({adj.n_entries}), '
                             f'got {self.A.size(0)}')
        if self.A.size(1) != self.width:
            raise ValueError(f'message width {self.A.size(1)} != declared width {self.width}')
        if self.msg_op != MSG_A:
            if self.ib_mode == 'aux' and adj.aux is None:
                raise ValueError('adjacency was built without a shared-cell index')
            want = adj.n_aux if self.ib_mode == 'aux' else adj.n_entries
            if self.B.size(0) != want:
                raise ValueError(f'attribute has {self.B.size(0)} rows, expected {want}')
            if self.B.size(1) not in (self.width, 1):
                raise ValueError(f'attribute width {self.B.size(1)} must be {self.width} or 1')
        else:
            self.B = None
        if self.self_x is not None and tuple(self.self_x.shape) != (self.n_dst, self.width):
            raise ValueError('self term must be [n_dst, width]')


def _ident(t: Tensor):
    """Identity of a tensor as a view of device memory (saved tensors come back re-wrapped)."""
    return (t.data_ptr(), tuple(t.shape), tuple(t.stride()))


def _aggregate_backward(streams, tensors, needs, gs, max_outs, device) -> List[Optional[Tensor]]:
    """Gradients of aggregate_many's tensor inputs (four per stream: A, B, self_x, eps; `needs` likewise).
    One launch.  A cell-feature matrix x usually enters several slots of the same call (the
    self term of the upper stream, the self term of the boundary stream, the gathered operand
    of the next dimension's boundary stream: mp/layers.py:185-192), and its gradient is the sum
    of a transposed aggregation and the scaled self terms.  Those are folded into ONE
    descriptor (gathered part + up to two self terms) whose result is returned in one slot,
    None in the others -- instead of one `g * (1 + eps)` kernel per self term plus autograd's
    add kernels (48 of the ~100 framework launches of a ZINC training step)."""
    grads: List[Optional[Tensor]] = [None] * len(tensors)
    specs, slots = [], []
    act_specs, act_slots = [], []    # streams with an activation: descriptors of the one cwn_aggregate_act_bwd_* launch
    ident = lambda t: (t.data_ptr(), tuple(t.shape), tuple(t.stride()))   # saved tensors are re-wrapped
    selfs = {}       # ident(x) -> [(slot, g, eps)] self-term contributions waiting for a host spec
    gathered = {}    # ident(x) -> index into specs of a gathered contribution to the same tensor
    for k, st in enumerate(streams):
        g = gs[k]
        if g is None:
            continue
        A, B, self_x, eps = tensors[4 * k: 4 * k + 4]
        need_A, need_B, need_self, need_eps = needs[4 * k: 4 * k + 4]
        g = g.contiguous()
        if self_x is not None:
            if need_self:
                selfs.setdefault(ident(self_x), []).append((4 * k + 2, g, eps))
            if need_eps and eps is not None:
                grads[4 * k + 3] = (g * self_x).sum().reshape(eps.shape)
        adj, op = st.adj, st.msg_op
        if adj is None or not (need_A or need_B):
            continue
        if not adj.built:                       # (handed out under csr.deferred_builds, wanted after all)
            from .csr import ensure_built
            ensure_built(adj)
        if getattr(st, 'act', None) is not None:
            # out = sum act(A[ia] + B[ib]): g * act'(A + B) summed over the transposed plans, the pre-activation recomputed
            # from the saved A and B -- nothing of size [E, F] is written unless an operand holds one row per ENTRY
            code = _act_code(st.act)
            F = g.size(1)
            if (need_A and st.ia_mode == 'perm') or (need_B and st.ib_mode == 'perm'):
                a_e = A if st.ia_mode == 'perm' else _ffi.gather_rows(A, adj.val)
                b_e = B if st.ib_mode == 'perm' else _ffi.gather_rows(B, adj.aux_index)
                g_e = _act_backward_entries(code, a_e + b_e, _ffi.gather_rows(g, adj.key))
                if need_A and st.ia_mode == 'perm':
                    grads[4 * k] = g_e
                if need_B and st.ib_mode == 'perm':
                    grads[4 * k + 1] = g_e
            if need_A and st.ia_mode == 'col':
                t = adj.t_src          # rows of A collect from the destinations they fed
                act_specs.append(AggActBwdSpec(adj=t, F=F, act=code, g=g, ig=t.col, P=A, Q=B,
                                               iq=t.aux if st.ib_mode == 'aux' else t.perm))
                act_slots.append(4 * k)
            if need_B and st.ib_mode == 'aux':
                t = adj.t_aux          # keyed on the shared cell: col = destination, aux = source
                act_specs.append(AggActBwdSpec(adj=t, F=F, act=code, g=g, ig=t.col, P=B, Q=A,
                                               iq=t.aux if st.ia_mode == 'col' else t.perm))
                act_slots.append(4 * k + 1)
            continue
        if st.reduce == 'max':
            out_k = max_outs[sum(1 for s_ in streams[:k] if s_.reduce == 'max')]
            if op != MSG_A:
                raise NotImplementedError("gradient of reduce='max' with a two-operand fused message: "
                                          'route the message through the generic (hook) path')
            if self_x is not None:
                # the saved output carries the self term: the bare row maxima again (found by gradcheck: the arg-max test
                # below compared A with max + (1 + eps) x and selected nothing)
                out_k, = run_aggregate([AggSpec(adj=adj, n_dst=st.n_dst, F=st.width, A=A, reduce=_ffi.REDUCE['max'],
                                                ia=adj.col if st.ia_mode == 'col' else adj.perm)], device)
            if need_A:
                grads[4 * k] = _AggregateMany._max_backward(st, A, out_k, g)
            continue
        if st.reduce == 'mean':
            g = g / adj.counts
        F = g.size(1)
        if need_A:
            if st.ia_mode == 'perm':   # A holds one row per ENTRY: dA[e] = g[dst[e]] (x the message's own derivative)
                gA = _ffi.gather_rows(g, adj.key)
                if op not in (MSG_A, MSG_A_PLUS_B):
                    b_e = B if st.ib_mode == 'perm' else _ffi.gather_rows(B, adj.aux_index)
                    if op == MSG_A_TIMES_B:
                        gA = gA * b_e
                    elif op == MSG_RELU_A_PLUS_B:
                        gA = gA * ((A + b_e) > 0)
                    else:
                        gA = gA * (2 * torch.relu(A + b_e))
                grads[4 * k] = gA
            else:
                t = adj.t_src          # rows of A collect from the destinations they fed
                s = AggSpec(adj=t, n_dst=t.n_dst, F=F, A=g, ia=t.col)
                if op == MSG_A_TIMES_B:
                    s.msg_op, s.B = MSG_A_TIMES_B, B
                    s.ib = t.aux if st.ib_mode == 'aux' else t.perm
                elif op in (MSG_RELU_A_PLUS_B, MSG_RELU_A_PLUS_B_SQ):
                    # B per shared cell (lazy up_attr) or per ENTRY (a materialised up_attr): the
                    # transposed plan's perm is the entry id of each of its positions
                    # (the squared form: d relu(a + b)^2 / da = 2 relu(a + b))
                    s.msg_op, s.B, s.self_pre = (MSG_A_MASK_RELU if op == MSG_RELU_A_PLUS_B else MSG_A_TIMES_2RELU), B, A
                    s.ib = t.aux if st.ib_mode == 'aux' else t.perm
                gathered.setdefault(ident(A), len(specs))
                specs.append(s)
                slots.append(4 * k)
        if need_B:
            if op == MSG_A_TIMES_B:
                raise NotImplementedError(
                    'no gradient for the multiplicative attribute; route it through the '
                    'generic (hook) path if it is trainable')
            if st.ib_mode == 'perm':
                gB = _ffi.gather_rows(g, adj.key)          # dB[e] = g[dst[e]] ...
                a_e = (lambda: A if st.ia_mode == 'perm' else _ffi.gather_rows(A, adj.val))
                if op == MSG_RELU_A_PLUS_B:                # ... where the entry's pre-activation is positive
                    gB = gB * ((a_e() + B) > 0)
                elif op == MSG_RELU_A_PLUS_B_SQ:
                    gB = gB * (2 * torch.relu(a_e() + B))
                grads[4 * k + 1] = gB
            else:
                t = adj.t_aux          # keyed on the aux cell: col = destination, aux = source
                s = AggSpec(adj=t, n_dst=t.n_dst, F=F, A=g, ia=t.col)
                if op in (MSG_RELU_A_PLUS_B, MSG_RELU_A_PLUS_B_SQ):
                    # (A per source cell, or per ENTRY: the transposed plan's perm is the entry id of each of its positions)
                    s.msg_op, s.B, s.self_pre = (MSG_A_MASK_RELU if op == MSG_RELU_A_PLUS_B else MSG_A_TIMES_2RELU), A, B
                    s.ib = t.aux if st.ia_mode == 'col' else t.perm
                gathered.setdefault(ident(B), len(specs))
                specs.append(s)
                slots.append(4 * k + 1)
    # fold the self terms: two per descriptor, onto a gathered contribution to the same tensor
    # when there is one, else onto a descriptor without adjacency (zeros + self terms)
    for key, terms in selfs.items():
        host = gathered.get(key)
        while terms:
            take, terms = terms[:2], terms[2:]
            if host is None:
                _, g0, _ = take[0]
                s = AggSpec(adj=None, n_dst=g0.size(0), F=g0.size(1))
                specs.append(s)
                slots.append(take[0][0])
            else:
                s, host = specs[host], None
            s.self_x, s.eps = take[0][1], take[0][2]
            if len(take) == 2:
                s.self_x2, s.eps2 = take[1][1], take[1][2]
    if specs:
        for slot, o in zip(slots, run_aggregate(specs, device)):
            grads[slot] = o
    if act_specs:
        for slot, o in zip(act_slots, run_aggregate_act_bwd(act_specs, device)):
            grads[slot] = o
    return grads


class _AggregateMany(torch.autograd.Function):
    """N streams, one launch forward, one launch backward.  Tensor inputs are flattened four per
    stream: (A, B, self_x, eps)."""

    @staticmethod
    def specs_of(streams, tensors) -> List[AggSpec]:
        specs = []
        for k, st in enumerate(streams):
            A, B, self_x, eps = tensors[4 * k: 4 * k + 4]
            if getattr(st, 'act', None) is not None:
                s = AggActSpec(adj=st.adj, n_dst=st.n_dst, F=st.width, act=_act_code(st.act), self_x=self_x, eps=eps,
                               dtype=getattr(st, 'dtype', None))
                if st.adj is not None:
                    s.A, s.B = A, B
                    s.ia = st.adj.col if st.ia_mode == 'col' else st.adj.perm
                    s.ib = st.adj.aux if st.ib_mode == 'aux' else st.adj.perm
                specs.append(s)
                continue
            s = AggSpec(adj=st.adj, n_dst=st.n_dst, F=st.width, msg_op=st.msg_op,
                        reduce=_ffi.REDUCE[st.reduce], self_x=self_x, eps=eps, dtype=getattr(st, 'dtype', None))
            if st.adj is not None:
                s.A = A
                s.ia = st.adj.col if st.ia_mode == 'col' else st.adj.perm
                if st.msg_op != MSG_A:
                    s.B = B
                    s.ib = st.adj.aux if st.ib_mode == 'aux' else st.adj.perm
            specs.append(s)
        return specs

    @staticmethod
    def forward(ctx, streams: Tuple[Stream, ...], device, *tensors):
        outs = _run_streams(_AggregateMany.specs_of(streams, tensors), device)     # (activated streams: a launch of their own)
        ctx.streams, ctx.device = streams, device
        ctx.n_in = len(tensors)
        keep = [o for o, st in zip(outs, streams) if st.reduce == 'max']     # arg-max recovery in backward
        ctx.save_for_backward(*tensors, *keep)
        return tuple(outs)

    @staticmethod
    def _max_backward(st: Stream, A: Tensor, out: Tensor, g: Tensor) -> Tensor:
        """Gradient of out[i] = max_p A[ia[p]] w.r.t. A: g[i, f] goes to ONE entry of the row, the first
        (in entry order) that attains the maximum -- torch-scatter's arg-max rule, the library behind
        mp/cell_mp.py:104-105, 439; torch's own amax spreads it over ties, identical without ties.
        Tensor ops for the selection, the library's own transposed aggregation for the sum: the mode is exercised by no
        reference test (parity unpinned), not a hot path."""
        adj = st.adj
        E = adj.n_entries
        src = (adj.col if st.ia_mode == 'col' else adj.perm).long()
        counts = (adj.rowptr[1:] - adj.rowptr[:-1]).long()
        rowid = torch.repeat_interleave(torch.arange(adj.n_dst, device=g.device), counts, output_size=E)
        eq = A[src] == out[rowid]
        c = eq.to(torch.int32).cumsum(0)
        start = adj.rowptr[:-1].long()[rowid]
        base = torch.where((start > 0).unsqueeze(1), c[(start - 1).clamp(min=0)], torch.zeros_like(c))
        first = eq & ((c - base) == 1)
        # the selected gradients go back to their SOURCE rows through the transposed plan (a segmented sum keyed on the
        # source cell, in entry order: deterministic) -- round 2 used index_add_, i.e. fp32 atomics in arrival order
        vals = g[rowid] * first                                   # [E, F] by CSR position
        by_entry = torch.empty_like(vals)
        by_entry[adj.perm.long()] = vals                          # ... by original entry number (a permutation)
        t = adj.t_src
        if st.ia_mode != 'col':                                   # per-entry operand: its "source rows" are the entries
            return by_entry
        return aggregate(t, t.n_dst, by_entry, ia_mode='perm')

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gs):
        saved = ctx.saved_tensors
        tensors, max_outs = saved[:ctx.n_in], list(saved[ctx.n_in:])
        grads = _aggregate_backward(ctx.streams, tensors, ctx.needs_input_grad[2:], gs, max_outs, ctx.device)
        return (None, None) + tuple(grads)


_ACT_NO_GRAD = ('a stream with an activation (Stream.act) runs on cwn_aggregate_act_f32 / _f64, which has no backward: '
                'inference only')


def _run_streams(specs: Sequence, device) -> List[Tensor]:
    """The specs of `_AggregateMany.specs_of` launched, outputs in spec order: those of streams with an activation through
    `run_aggregate_act`, the rest through `run_aggregate` (one call each, and only when it has something to run)."""
    acts = [s for s in specs if isinstance(s, AggActSpec)]
    if not acts:
        return run_aggregate(specs, device)
    plain = [s for s in specs if not isinstance(s, AggActSpec)]
    run_aggregate_act(acts, device)
    if plain:
        run_aggregate(plain, device)
    return [s.out for s in specs]


def aggregate_many(streams: Sequence[Stream]) -> List[Tensor]:
    """All streams in ONE kernel launch (per <= 8), differentiable w.r.t. A, B, self_x and eps.  Streams with an
    activation (Stream.act) take a launch of their own forward (run_aggregate_act) and, with ACT_MESSAGE_BACKWARD on, one
    backward (run_aggregate_act_bwd); with it off they are inference only.  The outputs come back in stream order either way."""
    device = None
    flat: List[Optional[Tensor]] = []
    for st in streams:
        st.validate()
        for t in (st.A, st.B, st.self_x, st.eps):
            if t is not None and device is None:
                device = t.device
        flat += [st.A, st.B, st.self_x, st.eps]
    if device is None:
        raise ValueError('aggregate_many needs at least one tensor to know the device')
    # plans not built yet (callers may hand over unbuilt adjacencies) and, when a gradient will be
    # needed, the transposed plans of the backward pass: ONE batched build call for all of them,
    # now, so the backward pass launches no index kernels
    from .csr import build_many
    todo = [st.adj for st in streams if st.adj is not None and not st.adj.built]
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in flat):
        for st in streams:
            if st.adj is not None and st.ia_mode == 'col':
                st.adj.transposes()
                todo += [a for a in (st.adj._t_src, st.adj._t_aux) if a is not None and not a.built]
    if todo:
        build_many(todo)
    if not (torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in flat)):
        # inference: no autograd node to build (Function.apply alone is ~15 us of host time)
        return _run_streams(_AggregateMany.specs_of(streams, flat), device)
    if not ACT_MESSAGE_BACKWARD and any(st.act is not None for st in streams):
        raise NotImplementedError(_ACT_NO_GRAD)
    return list(_AggregateMany.apply(tuple(streams), device, *flat))


def aggregate(adj: Optional[Adjacency], n_dst: int, A: Optional[Tensor], *, msg_op: int = MSG_A,
              reduce: str = 'add', ia_mode: str = 'col', B: Optional[Tensor] = None,
              ib_mode: str = 'aux', self_x: Optional[Tensor] = None,
              eps: Optional[Tensor] = None, width: Optional[int] = None) -> Tensor:
    """Single-stream form of aggregate_many (see Stream for the argument meaning)."""
    ref = A if A is not None else self_x
    if width is None:
        width = int(ref.size(1))
    return aggregate_many([Stream(adj=adj, n_dst=int(n_dst), width=int(width), A=A, B=B,
                                  msg_op=msg_op, reduce=reduce, ia_mode=ia_mode, ib_mode=ib_mode,
                                  self_x=self_x, eps=eps)])[0]


def zeros_rows(n: int, width: int, device, dtype: torch.dtype = torch.float32) -> Tensor:
    """K9: the zero fill for an absent adjacency when nothing else is launched."""
    return torch.zeros(n, width, dtype=dtype, device=device)


class _GatherRows(torch.autograd.Function):
    """K1 (mp/cell_mp.py:198): out[e] = src[idx[e]].  Backward: segmented sum over the CSR keyed on
    idx (`adj_for_idx().perm` lists, per source row, the entries that read it)."""

    @staticmethod
    def forward(ctx, src, idx, adj_for_idx):
        ctx.adj_for_idx = adj_for_idx
        return _ffi.gather_rows(src, idx)

    @staticmethod
    def backward(ctx, g):
        t = ctx.adj_for_idx()
        g = g.contiguous()
        out, = run_aggregate([AggSpec(adj=t, n_dst=t.n_dst, F=g.size(1), A=g, ia=t.perm)], g.device)
        return out, None, None


def gather_rows(src: Tensor, idx: Tensor, adj_for_idx=None) -> Tensor:
    """Differentiable row gather.  `adj_for_idx` is a zero-argument callable returning an Adjacency
    keyed on `idx` (only called in backward); when omitted one is built on demand."""
    src = _fc(src, 'src')
    _ffi.require_gpu(idx, 'idx')
    if idx.dtype != torch.long:
        raise TypeError('index must be int64')
    idx = idx.contiguous()
    if adj_for_idx is None:
        n_src = src.size(0)

        def adj_for_idx():
            return Adjacency.from_index(torch.stack([idx, idx]), n_src, n_src)
    return _GatherRows.apply(src, idx, adj_for_idx)


_arange_cache = {}


def embedding_sum(weights: Sequence[Tensor], idx: Tensor) -> Tensor:
    """out[i] = sum_c weights[c][idx[i, c]] -- torch.nn.Embedding (one column: v_embed_init /
    e_embed_init of mp/molec_models.py:44-52) and the OGB Atom/BondEncoder form (a sum of one
    embedding per integer feature column) as ONE gather-sum launch over the concatenated tables
    (cwn_embedding_fwd_f32), and a backward that accumulates the whole table per workgroup in LDS
    (cwn_embedding_bwd_f32) instead of torch's sort-based embedding_backward (154 us per table at
    ZINC size, 20 % of the training step).  Summation order per cell is c = 0, 1, ...:
    bit-identical to the Python `sum(...)` of the encoders.  An index outside its table raises
    IndexError (at the next validated plan build / csr.check_errors under stream capture)."""
    _ffi.require_gpu(idx, 'idx')
    if idx.dtype != torch.long:
        raise TypeError('index must be int64')
    if idx.dim() == 1:
        idx = idx.unsqueeze(1)
    N, Cn = idx.shape
    if len(weights) != Cn:
        raise ValueError(f'{Cn} index columns for {len(weights)} embedding tables')
    H = int(weights[0].size(1))
    V = sum(int(w.size(0)) for w in weights)
    if H % 4 != 0 or V * H * 4 > 60 * 1024 or weights[0].dtype != torch.float32:
        # a table too wide / too large for the dedicated kernels (or not float32): generic aggregation over a plan
        W = weights[0] if Cn == 1 else torch.cat(list(weights), 0)
        offs = torch.tensor([sum(int(w.size(0)) for w in weights[:c]) for c in range(Cn)],
                            dtype=torch.long, device=idx.device)
        src = (idx + offs).reshape(-1)
        dst = torch.arange(N, device=idx.device).repeat_interleave(Cn)
        adj = Adjacency.from_index(torch.stack([src, dst]), N, V, build=False)
        return aggregate(adj, N, W)
    return _EmbeddingSum.apply(idx.contiguous(), *weights)


def _adjacent_rows(tensors: Sequence[Tensor]) -> Optional[Tensor]:
    """The row-wise concatenation of `tensors` WITHOUT a copy when they already lie back to back in one storage -- the
    per-column tables of an OGB-style encoder re-homed into FlatAdam's parameter buffer (cwn_amd/train.py: consecutive
    parameters, every one a multiple of 16 bytes), and their gradients in the flat bucket: one [sum V, H] view over all of
    them.  None when they do not (the caller concatenates).  A training step changes every table, so the copy was a launch per
    encoder and step (molhiv-512: 2 x torch.cat forward, 2 x zero-fill + 2 x _foreach_add_ backward: round 6)."""
    t0 = tensors[0]
    if t0.dim() != 2 or t0.dtype != torch.float32 or not t0.is_contiguous():
        return None
    H, end, rows = int(t0.size(1)), t0.data_ptr(), 0
    for t in tensors:
        if (t.dim() != 2 or t.dtype != torch.float32 or not t.is_contiguous() or int(t.size(1)) != H or t.data_ptr() != end
                or t.device != t0.device or t.untyped_storage().data_ptr() != t0.untyped_storage().data_ptr()):
            return None
        end += t.numel() * 4
        rows += int(t.size(0))
    if end > t0.untyped_storage().data_ptr() + t0.untyped_storage().nbytes():
        return None
    return t0.as_strided((rows, H), (H, 1))


class _EmbeddingSum(torch.autograd.Function):
    """Forward: cwn_embedding_fwd_f32.  Backward: cwn_embedding_bwd_f32 into one zeroed buffer,
    handed back as per-table views (or added into the parameters' .grad directly when they are
    allocated)."""

    @staticmethod
    def _columns(weights, dev):
        """(col_off, col_size) device arrays of the table layout, cached; (None, None) for one."""
        if len(weights) == 1:
            return None, None
        dims = tuple(int(w.size(0)) for w in weights)
        key = ('cols', dims, dev)
        hit = _arange_cache.get(key)
        if hit is None:
            if len(_arange_cache) > 64:
                _arange_cache.clear()
            hit = (torch.tensor([sum(dims[:c]) for c in range(len(dims))], dtype=torch.long, device=dev),
                   torch.tensor(dims, dtype=torch.long, device=dev))
            _arange_cache[key] = hit
        return hit

    @staticmethod
    def forward(ctx, idx, *weights):
        from .csr import _err_flag, VALIDATE_INDICES, check_errors
        dev = idx.device
        W = weights[0] if len(weights) == 1 else _adjacent_rows([w.detach() for w in weights])
        if W is None:
            W = torch.cat([w.detach() for w in weights], 0)
        W = _f32c(W.detach(), 'embedding table')
        off, size = _EmbeddingSum._columns(weights, dev)
        N, Cn = idx.shape
        out = torch.empty(N, W.size(1), dtype=torch.float32, device=dev)
        _ffi.check(_ffi.lib().cwn_embedding_fwd_f32(
            W.data_ptr(), idx.data_ptr(), _ffi.ptr(off), _ffi.ptr(size), out.data_ptr(), N, Cn, W.size(1),
            W.size(0), _err_flag(dev).data_ptr(), _ffi.stream_ptr(dev)), 'cwn_embedding_fwd_f32')
        if VALIDATE_INDICES and not torch.cuda.is_current_stream_capturing():
            check_errors(dev)          # one sync, as a validated plan build does; IndexError on a bad index
        ctx.save_for_backward(idx)
        ctx.meta = (int(W.size(0)), int(W.size(1)), [int(w.size(0)) for w in weights])
        ctx.tables = weights
        return out

    @staticmethod
    def backward(ctx, g):
        idx, = ctx.saved_tensors
        return (None,) + tuple(_embedding_table_grads(ctx.tables, idx, g))


DETERMINISTIC = False


def deterministic(on: bool = True) -> None:
    """Bit-reproducible TRAINING arithmetic (DDP debugging: two runs, graph vs eager, rank vs rank give torch.equal gradients):
    every sum whose order the fast path leaves to the arrival order of atomics takes its ordered form --
      weight gradients: per-band partial tiles + a reduce in band order (cwn_gemm_tn_f32 with a workspace: _ffi.DETERMINISTIC_TN;
        bands of 128 rows whatever the capacity: a static batch's step has the bits of the step on the collated batch);
      BatchNorm(train) statistics: per-band partials summed in band order by cwn_bn_finalize_f32 (dense_train.LIVE_BN = False);
      BatchNorm backward sums: the one-launch column-owning form cwn_norm_bwd_f32 (dense_train.FUSED_NORM_BACKWARD; matrices
        of at most 4096 rows -- larger ones keep the atomic reduce) and no slot sums (LIVE_BN_BWD = False);
      embedding-table gradients: a destination-sorted plan keyed on the table row + one segmented reduce in cell order (the
        fused front backward and the band kernels add with atomics).
    Costs ~10 % of a ZINC-128 step.  Everything else on the path is ordered by construction (stable CSR order, owner-form
    backward, fixed trees).  Also settable with CWN_DETERMINISTIC=1."""
    global DETERMINISTIC, FUSED_FRONT_BACKWARD
    from . import dense_train
    if on:
        deterministic._saved = (_ffi.DETERMINISTIC_TN, dense_train.LIVE_BN, dense_train.LIVE_BN_BWD, dense_train.FUSED_NORM_BACKWARD,
                                FUSED_FRONT_BACKWARD)
        _ffi.DETERMINISTIC_TN, dense_train.LIVE_BN, dense_train.LIVE_BN_BWD, dense_train.FUSED_NORM_BACKWARD = True, False, False, True
        FUSED_FRONT_BACKWARD = False
    elif getattr(deterministic, '_saved', None) is not None:
        (_ffi.DETERMINISTIC_TN, dense_train.LIVE_BN, dense_train.LIVE_BN_BWD, dense_train.FUSED_NORM_BACKWARD,
         FUSED_FRONT_BACKWARD) = deterministic._saved
        deterministic._saved = None
    DETERMINISTIC = bool(on)


def _embedding_table_grads(tables, idx: Tensor, g: Tensor) -> List[Optional[Tensor]]:
    """d(table) of out[i] = sum_c table_c[idx[i, c]] given g = d out: cwn_embedding_bwd_f32 into one zeroed buffer, handed
    back as per-table views -- or added into the parameters' .grad directly where those are allocated (then None)."""
    H = int(tables[0].size(1))
    sizes = [int(w.size(0)) for w in tables]
    V = sum(sizes)
    g = g.contiguous()
    if idx.dim() == 1:
        idx = idx.unsqueeze(1)
    # the integer features as the containers deliver them: int64, or float32 (truncated by the kernel as `.to(torch.long)`
    # does) -- no converted copy, which a step captured over static buffers could not keep current
    if idx.dtype not in (torch.long, torch.float32):
        idx = idx.to(torch.long)
    idx = idx.contiguous()
    f32, n_dev = (1 if idx.dtype == torch.float32 else 0), _ffi.dyn(idx.size(0))
    if DETERMINISTIC and n_dev is None:
        # ordered form (ops.deterministic): dW[v] = the sum of g over the cells that looked row v up IN CELL ORDER -- a
        # destination-sorted plan keyed on the table row (stable: entry order = cell order) and one segmented reduce; no atomics
        li = idx.to(torch.long)
        Cn = int(li.size(1))
        offs = _EmbeddingSum._columns(tables, g.device)[0]          # (cached device array: nothing is uploaded inside a capture)
        rows = (li + offs if offs is not None else li).reshape(-1).contiguous()
        cells = torch.arange(li.size(0), device=g.device).repeat_interleave(Cn) if Cn > 1 else torch.arange(li.size(0), device=g.device)
        from .csr import build_many
        adj = Adjacency(rows, cells, V, int(li.size(0)))
        build_many([adj], validate=False)
        dW = run_aggregate([AggSpec(adj=adj, n_dst=V, F=H, A=g, ia=adj.col)], g.device)[0]
        if len(tables) == 1:
            t = _grad_target(tables[0])
            if t is not None and t.dtype == torch.float32 and tuple(t.shape) == (V, H):
                t.add_(dW)
                return [None]
        views, o = [], 0
        for n in sizes:
            views.append(dW[o:o + n])
            o += n
        return views
    off, size = _EmbeddingSum._columns(tables, g.device)
    if len(tables) == 1:
        # one table whose .grad is allocated: the kernel ADDS its band partials (fp32 atomics) -- straight into the gradient
        # buffer, no zeroed scratch and no add behind it (two launches per table of a ZINC training step)
        t = _grad_target(tables[0])
        if t is not None and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (V, H):
            _ffi.check(_ffi.lib().cwn_embedding_bwd_f32(
                g.data_ptr(), idx.data_ptr(), _ffi.ptr(off), _ffi.ptr(size), t.data_ptr(), idx.size(0),
                idx.size(1), H, V, f32, n_dev, _ffi.stream_ptr(g.device)), 'cwn_embedding_bwd_f32')
            return [None]
    else:
        # several tables whose .grad tensors lie back to back (views of the flat gradient bucket): the kernel adds into all of
        # them as ONE [V, H] matrix -- no zeroed scratch, no per-table views, no _foreach_add_ behind it
        targets = [_grad_target(w) for w in tables]
        flat_t = _adjacent_rows(targets) if all(t is not None for t in targets) else None
        if flat_t is not None and tuple(flat_t.shape) == (V, H):
            _ffi.check(_ffi.lib().cwn_embedding_bwd_f32(
                g.data_ptr(), idx.data_ptr(), _ffi.ptr(off), _ffi.ptr(size), flat_t.data_ptr(), idx.size(0),
                idx.size(1), H, V, f32, n_dev, _ffi.stream_ptr(g.device)), 'cwn_embedding_bwd_f32')
            return [None] * len(tables)
    dW = torch.zeros(V, H, dtype=torch.float32, device=g.device)
    _ffi.check(_ffi.lib().cwn_embedding_bwd_f32(
        g.data_ptr(), idx.data_ptr(), _ffi.ptr(off), _ffi.ptr(size), dW.data_ptr(), idx.size(0),
        idx.size(1), H, V, f32, n_dev, _ffi.stream_ptr(g.device)), 'cwn_embedding_bwd_f32')
    views, o = [], 0
    for n in sizes:
        views.append(dW[o:o + n])
        o += n
    grads, acc_dst, acc_src = [], [], []
    for w, v in zip(tables, views):
        t = _grad_target(w)
        if t is None:
            grads.append(v)
        else:
            acc_dst.append(t)
            acc_src.append(v)
            grads.append(None)
    if acc_dst:
        torch._foreach_add_(acc_dst, acc_src)
    return grads


# ------------------------------------------------------------------------------------------------
# the two ends of a model forward, one launch each (csrc/cwn_ends.hip; inference)
# ------------------------------------------------------------------------------------------------
FUSED_ENDS = True            # False: the front / head run as the separate launches they replace (A/B, tests)
FUSED_FRONT_TRAINING = os.environ.get('CWN_FUSED_FRONT_TRAINING') != '0'  # the front with autograd as one forward launch
FUSED_HEAD_TRAINING = os.environ.get('CWN_FUSED_HEAD_TRAINING') != '0'    # the head with autograd as two launches (+ weight-gradient GEMMs)

_table_cache = {}            # concatenated embedding tables, keyed on the weights' identities and versions


def _embed_table(weights: Sequence[Tensor], feats: Tensor, keep: list) -> _ffi.EmbedTable:
    """cwn_embed_table of one table set + the integer features as the container delivers them (float32 or int64,
    [n] or [n, cols])."""
    dev = feats.device
    if len(weights) == 1:
        W = _f32c(weights[0].detach(), 'embedding table')
    else:
        key = tuple((id(w), _ffi.tver(w)) for w in weights) + (STATE_EPOCH,)
        hit = _table_cache.get(key)
        if hit is None:
            if len(_table_cache) > 32:
                _table_cache.clear()
            flat_w = _adjacent_rows([w.detach() for w in weights])
            hit = ((flat_w if flat_w is not None else torch.cat([w.detach() for w in weights], 0).contiguous()),
                   [weakref.ref(w) for w in weights])
            _table_cache[key] = hit
        W = hit[0]
    off, size = _EmbeddingSum._columns(weights, dev)
    if feats.dim() == 1:
        feats = feats.unsqueeze(1)
    if feats.dtype not in (torch.float32, torch.long):
        feats = feats.to(torch.long)
    feats = feats.contiguous()
    if feats.size(1) != len(weights):
        raise ValueError(f'{feats.size(1)} index columns for {len(weights)} embedding tables')
    keep += [W, off, size, feats]
    return _ffi.EmbedTable(W=W.data_ptr(), src=feats.data_ptr(), col_off=_ffi.ptr(off), col_size=_ffi.ptr(size),
                           V=int(W.size(0)), cols=int(feats.size(1)), src_is_f32=1 if feats.dtype == torch.float32 else 0)


def embed_front(v_weights: Sequence[Tensor], v_feats: Tensor, e_weights: Optional[Sequence[Tensor]],
                e_feats: Optional[Tensor], n1: int, adj1, n2: int, adj2, halve: bool = True) -> List[Tensor]:
    """[x0, x1, x2] of EmbedVEWithReduce.forward (mp/layers.py:509-547) in ONE launch (cwn_embed_front_f32):
    embedded vertices, embedded edges (or, without an edge table, the sum of their embedded boundary vertices), rings
    = half the sum over their boundary edges of THOSE sums.  adj1 / adj2: the destination-sorted plans of
    boundary_index_1 / _2 (csr.cached_adjacency), None = no reduction.  No autograd (the caller checks)."""
    from .csr import _err_flag, VALIDATE_INDICES, check_errors
    _ffi.require_gpu(v_feats, 'vertex features')
    dev = v_feats.device
    H = int(v_weights[0].size(1))
    keep: list = []
    tv = _embed_table(v_weights, v_feats, keep)
    # (a batch without a single edge -- isolated vertices only -- has no edge features to hand over: an empty tensor's null
    #  address is what cwn_embed_front_f32 refuses as a table without features; with n1 = 0 there is nothing to embed)
    te = _embed_table(e_weights, e_feats, keep) if e_weights is not None and int(n1) > 0 else None
    n0 = int(v_feats.size(0))
    # one allocation for the three outputs (rows of H floats: every block 16-B aligned)
    buf = torch.empty(n0 + n1 + n2, H, dtype=torch.float32, device=dev)
    x0, x1, x2 = buf[:n0], buf[n0:n0 + n1], buf[n0 + n1:]
    for adj in (adj1, adj2):
        if adj is not None and adj.ready is not None:
            torch.cuda.current_stream(dev).wait_event(adj.ready)
    _ffi.check(_ffi.lib().cwn_embed_front_f32(
        tv, n0, x0.data_ptr(), te, n1, x1.data_ptr(),
        _ffi.ptr(adj1.rowptr) if adj1 is not None else None, _ffi.ptr(adj1.col) if adj1 is not None else None,
        adj1.n_entries if adj1 is not None else 0, n2, x2.data_ptr(),
        _ffi.ptr(adj2.rowptr) if adj2 is not None else None, _ffi.ptr(adj2.col) if adj2 is not None else None,
        adj2.n_entries if adj2 is not None else 0, H, 1 if halve else 0, _err_flag(dev).data_ptr(), _front_counts(n0, n1, n2),
        _ffi.stream_ptr(dev)), 'cwn_embed_front_f32')
    if VALIDATE_INDICES and not torch.cuda.is_current_stream_capturing():
        check_errors(dev)
    return [x0, x1, x2]


def _marks(tensors):
    """What `current()` of a prepared launch compares: (tensors, [(address, version)]) -- in C++ when the compiled binding is
    there (csrc/cwn_torch_ext.cpp: TensorMarks)."""
    from . import _cext
    ts = [t for t in tensors if t is not None]
    X = _cext.ext()
    if X is not None:
        return X.TensorMarks(ts)
    return (ts, [(t.data_ptr(), _ffi.tver(t)) for t in ts])


def _marks_current(m) -> bool:
    if not isinstance(m, tuple):
        return m.current()
    for t, (p, v) in zip(*m):
        if _ffi.tver(t) != v or t.data_ptr() != p:
            return False
    return True


class FrontLaunch:
    """A prepared cwn_embed_front_f32 call (inference) for one (front module, batch): tables, plans and sizes resolved once;
    `run` takes the two feature tensors.  The range check of a feature tensor (one read of the device's error word) is made
    once per tensor VERSION: a batch that is run again is not checked again."""

    def __init__(self, v_weights, e_weights, n0, n1, adj1, n2, adj2, halve, bi1, bi2, v_feats, e_feats):
        from .csr import _err_flag
        for f in (v_feats, e_feats):
            if f is not None and (f.dim() != 2 or f.dtype not in (torch.float32, torch.long) or not f.is_contiguous()):
                raise ValueError('FrontLaunch: 2-D contiguous float32 / int64 feature tensors (the caller converts others per call)')
        self.dev = dev = v_feats.device
        self.n = (int(n0), int(n1), int(n2))
        self.H = H = int(v_weights[0].size(1))
        self.keep: list = []
        self.tv = _embed_table(v_weights, v_feats, self.keep)
        self.te = _embed_table(e_weights, e_feats, self.keep) if e_weights is not None and int(n1) > 0 else None    # (embed_front)
        self.dtypes = (v_feats.dtype, None if e_feats is None else e_feats.dtype)
        self.adjs, self.bi = (adj1, adj2), (bi1, bi2)
        self.marks = _marks(list(v_weights) + list(e_weights or []) + [bi1, bi2])       # (the plans belong to the indices' values)
        self.epochs = (STATE_EPOCH, STRUCT_EPOCH)
        self.err = _err_flag(dev)
        p = _ffi.ptr
        self.tail = (p(adj1.rowptr) if adj1 is not None else None, p(adj1.col) if adj1 is not None else None,
                     adj1.n_entries if adj1 is not None else 0)
        self.tail2 = (p(adj2.rowptr) if adj2 is not None else None, p(adj2.col) if adj2 is not None else None,
                      adj2.n_entries if adj2 is not None else 0, H, 1 if halve else 0, self.err.data_ptr())
        self.fn = _ffi.lib().cwn_embed_front_f32
        self._seen = None

    def current(self, bi1, bi2) -> bool:
        return (bi1 is self.bi[0] and bi2 is self.bi[1] and self.epochs == (STATE_EPOCH, STRUCT_EPOCH) and not _ffi.DYN_ROWS
                and _marks_current(self.marks))

    def run(self, v_feats: Tensor, e_feats: Optional[Tensor]) -> Optional[List[Tensor]]:
        n0, n1, n2 = self.n
        for f, n, dt, tab in ((v_feats, n0, self.dtypes[0], self.tv), (e_feats, n1, self.dtypes[1], self.te)):
            if tab is None:
                if f is not None and (n > 0 or f.size(0) > 0):
                    return None
                continue
            if (f is None or f.dtype != dt or f.dim() != 2 or f.size(0) != n or f.size(1) != tab.cols or not f.is_contiguous()
                    or f.device != self.dev):
                return None
        from . import csr
        buf = torch.empty(n0 + n1 + n2, self.H, dtype=torch.float32, device=self.dev)
        x0, x1, x2 = buf[:n0], buf[n0:n0 + n1], buf[n0 + n1:]
        for adj in self.adjs:
            if adj is not None and adj.ready is not None:
                torch.cuda.current_stream(self.dev).wait_event(adj.ready)
        self.tv.src = v_feats.data_ptr()
        if self.te is not None:
            self.te.src = e_feats.data_ptr()
        rc = self.fn(self.tv, n0, x0.data_ptr(), self.te, n1, x1.data_ptr(), *self.tail, n2, x2.data_ptr(), *self.tail2, None,
                     _ffi.stream_ptr(self.dev))
        if rc != 0:
            _ffi.check(rc, 'cwn_embed_front_f32')
        if csr.VALIDATE_INDICES and not torch.cuda.is_current_stream_capturing():
            seen = (id(v_feats), _ffi.tver(v_feats), id(e_feats), None if e_feats is None else _ffi.tver(e_feats), csr.ERROR_EPOCH)
            if self._seen is None or self._seen[0] != seen or self._seen[1]() is not v_feats or \
                    (e_feats is not None and self._seen[2]() is not e_feats):
                self._seen = (seen, weakref.ref(v_feats), None if e_feats is None else weakref.ref(e_feats))
                csr.check_errors(self.dev)
        return [x0, x1, x2]


def _front_counts(n0: int, n1: int, n2: int) -> Optional[int]:
    """Device address of the int64 triple (actual n0, n1, n2) when the three row counts are the capacities of a static batch
    (_ffi.dynamic_rows: static_graph.StaticBatch keeps the three counts consecutive in memory), else None."""
    p0, p1, p2 = _ffi.dyn(n0), _ffi.dyn(n1), (_ffi.dyn(n2) if n2 else None)
    if p0 is None:
        return None
    if p1 != p0 + 8 or (n2 and p2 != p0 + 16):
        raise _ffi.CwnError('embed_front: the device-side row counts of the three dimensions are not consecutive')
    return p0


def _long_index(feats: Tensor) -> Tensor:
    """The integer features of a batch as int64 [n, cols] (what cwn_embedding_bwd_f32 indexes with), converted once per
    feature tensor (they do not change between the steps that reuse a batch)."""
    hit = getattr(feats, '_cwn_long', None)
    if hit is None or hit[0] != _ffi.tver(feats):
        f = feats if feats.dim() == 2 else feats.unsqueeze(1)
        hit = (_ffi.tver(feats), f.to(torch.long).contiguous())
        try:
            feats._cwn_long = hit
        except AttributeError:
            pass
    return hit[1]


class _EmbedFrontTrain(torch.autograd.Function):
    """EmbedVEWithReduce.forward with autograd: forward = the one launch of embed_front; backward = the transposed
    reductions (rings -> edges -> vertices, the vertices' own gradient folded in as the self term) and one
    cwn_embedding_bwd_f32 per table set.  Replaces 8 forward launches (two index conversions, two gather-sums, two
    reductions, the halving) of the unfused path.  tensors = v tables..., e tables..."""

    @staticmethod
    def forward(ctx, meta, v_feats, e_feats, *tables):
        nv, n1, adj1, n2, adj2, halve = meta
        vt, et = list(tables[:nv]), list(tables[nv:])
        xs = embed_front(vt, v_feats, et or None, e_feats if et else None, n1, adj1, n2, adj2, halve=halve)
        ctx.meta, ctx.tables = meta, (vt, et)
        ctx.idx = (v_feats, e_feats if et else None)          # (as delivered: float32 or int64; _embedding_table_grads)
        return tuple(xs)

    @staticmethod
    def backward(ctx, g0, g1, g2):
        nv, n1, adj1, n2, adj2, halve = ctx.meta
        vt, et = ctx.tables
        iv, ie = ctx.idx
        dev = iv.device
        H = int(vt[0].size(1))
        fused = _front_backward_fused(ctx, g0, g1, g2)
        if fused is not None:
            return (None, None, None) + tuple(fused)
        # d red1[e] = (1/2) sum_{rings containing e} g2[ring]  (+ g1[e] when the edges have no table of their own: x1 = red1)
        t1 = None
        if g2 is not None and adj2 is not None and n2 > 0:
            t = adj2.t_src
            t1 = aggregate(t, t.n_dst, (g2 * 0.5 if halve else g2).contiguous(), self_x=None if (et or g1 is None) else g1.contiguous())
        elif not et and g1 is not None:
            t1 = g1.contiguous()
        dv = None if g0 is None else g0.contiguous()
        if t1 is not None and adj1 is not None:
            t = adj1.t_src
            dv = aggregate(t, t.n_dst, t1, self_x=dv)
        grads = [None] * (len(vt) + len(et))
        if dv is not None and any(ctx.needs_input_grad[3:3 + len(vt)]):
            grads[:len(vt)] = _embedding_table_grads(vt, iv, dv)
        if et and g1 is not None and any(ctx.needs_input_grad[3 + len(vt):]):
            grads[len(vt):] = _embedding_table_grads(et, ie, g1)
        return (None, None, None) + tuple(grads)


FUSED_FRONT_BACKWARD = os.environ.get('CWN_FUSED_FRONT_BACKWARD', '1') != '0'


def _front_backward_fused(ctx, g0, g1, g2) -> Optional[List[Optional[Tensor]]]:
    """cwn_embed_front_bwd_f32: the whole backward of the front in one launch (one vertex table, at most one edge table, one
    integer feature each, width 64 / 128 / 256: the ZINC models) -- or None (the caller runs the launches it replaces: the
    halving, two transposed aggregations, two table gradients)."""
    nv, n1, adj1, n2, adj2, halve = ctx.meta
    vt, et = ctx.tables
    iv, ie = ctx.idx
    if not FUSED_FRONT_BACKWARD or nv != 1 or len(et) > 1:
        return None
    H, Vv = int(vt[0].size(1)), int(vt[0].size(0))
    Ve = int(et[0].size(0)) if et else 0
    if H not in (64, 128, 256) or Vv > 64 or Ve > 64 or (et and int(et[0].size(1)) != H):
        return None
    feats = [iv] + ([ie] if et else [])
    for f in feats:
        if f is None or f.dtype not in (torch.long, torch.float32) or (f.dim() == 2 and f.size(1) != 1) or f.dim() > 2:
            return None
    if (et and g1 is None) or not any(ctx.needs_input_grad[3:]):
        return None
    dev = iv.device
    n0 = int(iv.size(0))
    gs = [None if g is None else _f32c(g, 'grad') for g in (g0, g1, g2)]
    if any(g is not None and not aligned16(g) for g in gs):
        return None
    t1 = adj1.t_src if (adj1 is not None and n1 > 0) else None      # per vertex its edges
    t2 = adj2.t_src if (adj2 is not None and n2 > 0 and gs[2] is not None) else None      # per edge its rings
    outs, targets = [], []
    for w in [vt[0]] + list(et):
        t = _grad_target(w)
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.shape != w.shape):
            t = None
        targets.append(t if t is not None else torch.zeros_like(w, dtype=torch.float32))
        outs.append(None if t is not None else targets[-1])
    fv = iv.contiguous()
    fe = ie.contiguous() if et else None
    a = _ffi.FrontBwd(g0=_ffi.ptr(gs[0]), g1=_ffi.ptr(gs[1]), g2=_ffi.ptr(gs[2]),
                      rowptr1=None if t1 is None else t1.rowptr.data_ptr(), col1=None if t1 is None else t1.col.data_ptr(),
                      rowptr2=None if t2 is None else t2.rowptr.data_ptr(), col2=None if t2 is None else t2.col.data_ptr(),
                      v_src=fv.data_ptr(), e_src=_ffi.ptr(fe), dWv=targets[0].data_ptr(),
                      dWe=targets[1].data_ptr() if et else None, n0=n0, n1=int(n1) if (et or t1 is not None) else 0,
                      n0_dev=_ffi.dyn(n0), n1_dev=_ffi.dyn(int(n1)) if n1 else None, H=H, Vv=Vv, Ve=Ve,
                      src_f32=(1 if fv.dtype == torch.float32 else 0) | (2 if (fe is not None and fe.dtype == torch.float32) else 0),
                      halve=int(bool(halve)))
    _ffi.check(_ffi.lib().cwn_embed_front_bwd_f32(C.byref(a), _ffi.stream_ptr(dev)), 'cwn_embed_front_bwd_f32')
    return outs


def embed_front_train(v_weights, v_feats, e_weights, e_feats, n1, adj1, n2, adj2, halve=True) -> List[Tensor]:
    """embed_front with autograd w.r.t. the tables (see _EmbedFrontTrain); the transposed plans of the two boundary
    adjacencies are built here, in one batched call, so that the backward pass launches no index kernels."""
    from .csr import build_many
    todo = []
    for adj in (adj1, adj2):
        if adj is not None:
            adj.transposes()
            todo += [a for a in (adj, adj._t_src) if a is not None and not a.built]
    if todo:
        build_many(todo)
    meta = (len(v_weights), int(n1), adj1, int(n2), adj2, bool(halve))
    return list(_EmbedFrontTrain.apply(meta, v_feats, e_feats, *v_weights, *(e_weights or [])))


_w1t_cache = {}


def _transposed(weight: Tensor) -> Tensor:
    """lin1's weight [H2, K] as [K, H2] (what cwn_head_f32 reads coalesced), once per weight version."""
    key = id(weight)
    hit = _w1t_cache.get(key)
    if hit is not None and hit[0]() is weight and hit[1] == (_ffi.tver(weight), STATE_EPOCH):
        return hit[2]
    if len(_w1t_cache) > 64:
        _w1t_cache.clear()
    t = _f32c(weight.detach(), 'lin1 weight').t().contiguous()
    _w1t_cache[key] = (weakref.ref(weight), (_ffi.tver(weight), STATE_EPOCH), t)
    return t


def _transpose_many(weights: Sequence[Tensor]) -> None:
    """The transposes of all of a head's lin1 weights that `_transposed` would miss, in ONE launch (a training step changes
    every weight: three copy launches per step otherwise)."""
    stale = [w for w in weights if not ((h := _w1t_cache.get(id(w))) is not None and h[0]() is w and h[1] == (_ffi.tver(w), STATE_EPOCH))]
    if len(stale) < 2 or len({(tuple(w.shape), w.dtype, w.device) for w in stale}) != 1 or stale[0].dtype != torch.float32:
        return
    if len(_w1t_cache) > 64:
        _w1t_cache.clear()
    K = int(stale[0].size(1))
    both = torch.cat([w.detach().t() for w in stale], dim=0)          # [n K, H2], one kernel
    for k, w in enumerate(stale):
        _w1t_cache[id(w)] = (weakref.ref(w), (_ffi.tver(w), STATE_EPOCH), both[k * K: (k + 1) * K])


HEAD_POOL_SPLIT = os.environ.get('CWN_HEAD_POOL_SPLIT', 'auto')       # 'auto' | 1 (never) | P


def head_split(rows_total: int, n_complexes: int) -> int:
    """Row chunks per complex for the head's pooling / its backward's broadcast: 1 for molecules; for complexes of thousands
    of cells (REDDIT-like) enough workgroups to fill the chip (at most 32, ~128 rows per chunk at least)."""
    if HEAD_POOL_SPLIT != 'auto':
        return max(1, min(64, int(HEAD_POOL_SPLIT)))
    if n_complexes <= 0:
        return 1
    per = rows_total / n_complexes
    if per < 512 or n_complexes >= 512:
        return 1
    # (one 128-row chunk per workgroup and dimension where the chip has room: REDDIT-32 forward 0.340 -> 0.332 ms against two)
    # (the pooling launch only asks whether this is > 1: it runs one workgroup per 128-row chunk of the whole batch)
    return int(max(1, min(32, min(per // 128, -(-1024 // n_complexes)))))


def _head_parts(x):
    """x of one dimension: a tensor, None, or the list of a jumping-knowledge concatenation's blocks -> (blocks, width)."""
    if x is None:
        return None, 0
    blocks = list(x) if isinstance(x, (list, tuple)) else [x]
    blocks = [_f32c(b, 'x') for b in blocks]
    blocks = [rowmajor16(b) for b in blocks]       # (cwn_head_f32 reads a row 16 bytes at a time; the RECORDED stride is judged)
    if len(blocks) > 1:
        w = int(blocks[0].size(1))
        if any(b.size(1) != w or b.size(0) != blocks[0].size(0) or b.stride(0) != blocks[0].stride(0) for b in blocks) \
                or len(blocks) > _ffi.HEAD_MAX_PARTS or w % 4 != 0:
            blocks = [torch.cat(blocks, dim=-1)]
    return blocks, sum(int(b.size(1)) for b in blocks)


def head(xs: Sequence, cell_ptrs: Sequence[Tensor], n_complexes: int, lin1_weights: Sequence[Tensor],
         lin1_biases: Sequence[Optional[Tensor]], lin2_weight: Tensor, lin2_bias: Optional[Tensor],
         mean_readout: bool = False, mean_final: bool = False, want_pooled: bool = False, want_hidden: bool = False,
         drop: Optional['_ffi.Dropout'] = None, drop_pos: int = 0):
    """pool_complex + lin1s (+ReLU) + final readout + lin2 in ONE launch (cwn_head_f32), one workgroup per complex.
    xs[d]: [N_d, K], None (dimension absent from the batch: pooled zeros, mp/nn.py:55-56), or a LIST of matrices [N_d, K / n]
    -- the layer outputs of a jumping-knowledge model (jump_mode 'cat'), read block by block: the concatenation is never
    written; cell_ptrs[d]: device int64 [C + 1], the collate's `ptr`.  Complexes of thousands of cells: their rows are summed
    by `head_split` workgroups each in a launch ahead (cwn_head_f32: pool_partials).  Returns out [C, O] (and the pooled
    [C, K] per dimension)."""
    parts = [_head_parts(x) for x in xs]
    x0 = next(b[0] for b, _ in parts if b is not None)
    _ffi.require_gpu(x0, 'x')
    dev = x0.device
    K, H2, O = int(lin1_weights[0].size(1)), int(lin1_weights[0].size(0)), int(lin2_weight.size(0))
    _transpose_many(lin1_weights)
    keep, dims, pooled, hidden = [], [], [], []
    rows_total = 0
    for d, (blocks, width) in enumerate(parts):
        D = _ffi.HeadDim()
        if blocks is not None:
            if width != K:
                raise ValueError(f'dim {d}: {width} features for a lin1 of {K} inputs')
            x = blocks[0]
            D.x, D.cell_ptr, D.n_cells, D.ldx = x.data_ptr(), cell_ptrs[d].data_ptr(), int(x.size(0)), int(x.stride(0))
            D.n_parts = len(blocks)
            for q, b in enumerate(blocks[1:]):
                D.x_more[q] = b.data_ptr()
            rows_total += int(x.size(0))
        w1t = _transposed(lin1_weights[d])
        b1 = None if lin1_biases[d] is None else _f32c(lin1_biases[d].detach(), 'lin1 bias')
        D.w1t, D.b1 = w1t.data_ptr(), _ffi.ptr(b1)
        if want_pooled or want_hidden:
            po = torch.empty(n_complexes, K, dtype=torch.float32, device=dev)
            pooled.append(po)
            D.pooled_out = po.data_ptr()
        if want_hidden:
            ho = torch.empty(n_complexes, H2, dtype=torch.float32, device=dev)
            hidden.append(ho)
            D.h_out = ho.data_ptr()
        keep += [blocks, w1t, b1]
        dims.append(D)
    w2 = _f32c(lin2_weight.detach(), 'lin2 weight')
    b2 = None if lin2_bias is None else _f32c(lin2_bias.detach(), 'lin2 bias')
    out = torch.empty(n_complexes, O, dtype=torch.float32, device=dev)
    s_out = torch.empty(n_complexes, H2, dtype=torch.float32, device=dev) if want_hidden else None
    P = head_split(rows_total, n_complexes)
    arr = (_ffi.HeadDim * len(dims))(*dims)
    n_part = int(_ffi.lib().cwn_head_pool_floats(arr, len(dims), n_complexes, K)) if P > 1 else 0
    partials = torch.empty(n_part, dtype=torch.float32, device=dev) if P > 1 else None
    _ffi.check(_ffi.lib().cwn_head_f32(arr, len(dims), n_complexes, K, H2, 1 if mean_readout else 0,
                                       1 if mean_final else 0, w2.data_ptr(), _ffi.ptr(b2), O, out.data_ptr(),
                                       _ffi.ptr(s_out), drop, int(drop_pos) if drop is not None else 0, _ffi.ptr(partials), n_part, P,
                                       _ffi.stream_ptr(dev)), 'cwn_head_f32')
    if want_hidden:
        return out, pooled, hidden, s_out
    return (out, pooled) if want_pooled else out


class HeadLaunch:
    """A prepared cwn_head_f32 call (inference: no dropout, no side outputs) for one (model, batch): transposed weights, the
    batch's `ptr` tables, the pooling split resolved once; `run` takes the feature matrices (or jumping-knowledge blocks)."""

    def __init__(self, hx, cell_ptrs, n_complexes, lin1_weights, lin1_biases, lin2_weight, lin2_bias, mean_readout, mean_final):
        parts = [_head_parts(x) for x in hx]
        x0 = next(b[0] for b, _ in parts if b is not None)
        self.dev = dev = x0.device
        self.C = int(n_complexes)
        self.K, self.H2, self.O = int(lin1_weights[0].size(1)), int(lin1_weights[0].size(0)), int(lin2_weight.size(0))
        _transpose_many(lin1_weights)
        self.keep, self.shapes = [], []
        self.arr = (_ffi.HeadDim * len(parts))()
        rows_total = 0
        for d, (blocks, width) in enumerate(parts):
            D = self.arr[d]
            if blocks is not None:
                if width != self.K:
                    raise ValueError(f'dim {d}: {width} features for a lin1 of {self.K} inputs')
                x = blocks[0]
                D.cell_ptr, D.n_cells, D.n_parts = cell_ptrs[d].data_ptr(), int(x.size(0)), len(blocks)
                rows_total += int(x.size(0))
                self.shapes.append((len(blocks), int(x.size(0)), int(x.size(1))))
            else:
                self.shapes.append(None)
            w1t = _transposed(lin1_weights[d])
            b1 = None if lin1_biases[d] is None else _f32c(lin1_biases[d].detach(), 'lin1 bias')
            D.w1t, D.b1 = w1t.data_ptr(), _ffi.ptr(b1)
            self.keep += [w1t, b1, cell_ptrs[d]]
        self.w2 = _f32c(lin2_weight.detach(), 'lin2 weight')
        self.b2 = None if lin2_bias is None else _f32c(lin2_bias.detach(), 'lin2 bias')
        self.P = head_split(rows_total, self.C)
        self.n_part = int(_ffi.lib().cwn_head_pool_floats(self.arr, len(parts), self.C, self.K)) if self.P > 1 else 0
        self.flags = (1 if mean_readout else 0, 1 if mean_final else 0)
        self.marks = _marks(list(lin1_weights) + list(lin1_biases) + [lin2_weight, lin2_bias])
        self.epochs = (STATE_EPOCH, STRUCT_EPOCH)
        self.fn = _ffi.lib().cwn_head_f32

    def current(self) -> bool:
        return self.epochs == (STATE_EPOCH, STRUCT_EPOCH) and not _ffi.DYN_ROWS and _marks_current(self.marks)

    def run(self, hx) -> Optional[Tensor]:
        if len(hx) != len(self.shapes):
            return None
        for d, (x, shape) in enumerate(zip(hx, self.shapes)):
            if (x is None) != (shape is None):
                return None
            if x is None:
                continue
            blocks = x if isinstance(x, (list, tuple)) else (x,)
            n_b, rows, w = shape
            if len(blocks) != n_b:
                return None
            ldx = blocks[0].stride(0)
            for b in blocks:
                if (b.dtype != torch.float32 or b.dim() != 2 or b.size(0) != rows or b.size(1) != w or b.device != self.dev
                        or b.stride(0) != ldx or not is_rowmajor(b) or not is_vec16(b)):   # (cwn_head_f32: 16-byte rows -- the long way copies)
                    return None
            D = self.arr[d]
            D.x, D.ldx = blocks[0].data_ptr(), ldx
            for q in range(1, n_b):
                D.x_more[q - 1] = blocks[q].data_ptr()
        out = torch.empty(self.C, self.O, dtype=torch.float32, device=self.dev)
        partials = torch.empty(self.n_part, dtype=torch.float32, device=self.dev) if self.P > 1 else None
        rc = self.fn(self.arr, len(self.shapes), self.C, self.K, self.H2, self.flags[0], self.flags[1], self.w2.data_ptr(),
                     _ffi.ptr(self.b2), self.O, out.data_ptr(), None, None, 0, _ffi.ptr(partials), self.n_part, self.P,
                     _ffi.stream_ptr(self.dev))
        if rc != 0:
            _ffi.check(rc, 'cwn_head_f32')
        return out


class _HeadTrain(torch.autograd.Function):
    """The same head with autograd (the training step, exp/train_utils.py:57-75): forward = cwn_head_f32 leaving the
    pooled vectors, the pre-activations and the hidden vector; backward = ONE launch per complex (cwn_head_bwd_f32:
    dL/dx of every dimension) + the weight gradients as [C, .]^T [C, .] products through cwn_gemm_tn_f32 (deferred and
    merged with the step's other weight gradients inside accumulate_into_grad).  Replaces 5 forward and 16 backward
    launches of the unfused path (readout, two grouped GEMMs, ReLU masks, adds).  A dimension's x may be the blocks of a
    jumping-knowledge concatenation (meta: blocks per dimension): every block is an input of its own and gets its own
    gradient -- no torch.cat forward, no strided slice copies and adds backward."""

    @staticmethod
    def forward(ctx, meta, *tensors):
        n_dims, cell_ptrs, C, mean_readout, mean_final = meta[:5]
        drop_p, drop_pos = meta[5:7] if len(meta) > 5 else (0.0, 0)
        counts = list(meta[7]) if len(meta) > 7 else [1] * n_dims
        n_x = sum(counts)
        flat = tensors[:n_x]
        xs, o = [], 0
        for cnt in counts:
            blk = list(flat[o:o + cnt])
            o += cnt
            xs.append(None if blk[0] is None else (blk[0] if cnt == 1 else blk))
        w1s = tensors[n_x:n_x + n_dims]
        b1s = tensors[n_x + n_dims:n_x + 2 * n_dims]
        w2, b2 = tensors[n_x + 2 * n_dims], tensors[n_x + 2 * n_dims + 1]
        # the head's dropout (`apply_dropout_before`): multipliers derived in the kernel, re-derived by the backward
        first = next(t for t in flat if t is not None)
        ctx.drop = dropout_record(first.device, drop_p, tag=('head', int(drop_pos))) if drop_p > 0 and drop_pos else None
        ctx.drop_pos = int(drop_pos)
        out, pooled, hidden, s_out = head(xs, cell_ptrs, C, w1s, b1s, w2, b2, mean_readout, mean_final, want_hidden=True,
                                          drop=ctx.drop, drop_pos=ctx.drop_pos)
        ctx.meta, ctx.counts = meta, counts
        ctx.shapes = [None if x is None else (int(x.size(0)), int(x.size(1))) for x in flat]
        ctx.params = (w1s, b1s, w2, b2)
        ctx.save_for_backward(*pooled, *hidden, s_out)
        ctx.mark_non_differentiable(*pooled)
        ctx.set_materialize_grads(False)            # (else autograd fills a [C, K] zero gradient per pooled output)
        return (out,) + tuple(pooled)

    @staticmethod
    def backward(ctx, g_out, *_):
        n_dims, cell_ptrs, C, mean_readout, mean_final = ctx.meta[:5]
        counts = ctx.counts
        n_x = sum(counts)
        saved = ctx.saved_tensors
        pooled, hidden, s_out = saved[:n_dims], saved[n_dims:2 * n_dims], saved[2 * n_dims]
        w1s, b1s, w2, b2 = ctx.params
        if g_out is None:
            return (None,) * (1 + n_x + 2 * n_dims + 2)
        dev = g_out.device
        g_out = _f32c(g_out, 'grad')
        K, H2, O = int(w1s[0].size(1)), int(w1s[0].size(0)), int(w2.size(0))
        dims, dxs, dhs, keep = [], [None] * n_x, [], []
        o, rows_total = 0, 0
        for d in range(n_dims):
            cnt = counts[d]
            D = _ffi.HeadBwdDim(h=hidden[d].data_ptr())
            dh = torch.empty(C, H2, dtype=torch.float32, device=dev)
            dhs.append(dh)
            D.dh_out = dh.data_ptr()
            if ctx.shapes[o] is not None and any(ctx.needs_input_grad[1 + o + q] for q in range(cnt)):
                w1 = _f32c(w1s[d].detach(), 'lin1 weight')
                rows, Kp = ctx.shapes[o]
                # (all blocks of a dimension in one buffer: one allocation, equal row strides)
                buf = torch.empty(cnt, rows, Kp, dtype=torch.float32, device=dev)
                D.w1, D.cell_ptr, D.dx, D.n_cells, D.lddx = w1.data_ptr(), cell_ptrs[d].data_ptr(), buf[0].data_ptr(), rows, Kp
                D.n_parts = cnt
                for q in range(1, cnt):
                    D.dx_more[q - 1] = buf[q].data_ptr()
                for q in range(cnt):
                    if ctx.needs_input_grad[1 + o + q]:
                        dxs[o + q] = buf[q]
                keep.append(w1)
                rows_total += rows
            o += cnt
            dims.append(D)
        w2c = _f32c(w2.detach(), 'lin2 weight')
        arr = (_ffi.HeadBwdDim * n_dims)(*dims)
        _ffi.check(_ffi.lib().cwn_head_bwd_f32(arr, n_dims, C, K, H2, 1 if mean_readout else 0, 1 if mean_final else 0,
                                               w2c.data_ptr(), O, g_out.data_ptr(), ctx.drop, ctx.drop_pos if ctx.drop is not None else 0,
                                               head_split(rows_total, C), _ffi.stream_ptr(dev)), 'cwn_head_bwd_f32')
        # weight gradients: sums over the complexes = dZ^T X on [C, .] matrices; in-place targets when the caller owns them
        jobs = [(dhs[d], pooled[d], w1s[d], b1s[d]) for d in range(n_dims)] + [(g_out, s_out, w2, b2)]
        grads_w, grads_b, descs, scratch = [], [], [], []
        in_place = True
        for k, (dZ, X, W, b) in enumerate(jobs):
            nW = ctx.needs_input_grad[1 + n_x + k] if k < n_dims else ctx.needs_input_grad[1 + n_x + 2 * n_dims]
            nb = b is not None and (ctx.needs_input_grad[1 + n_x + n_dims + k] if k < n_dims else ctx.needs_input_grad[2 + n_x + 2 * n_dims])
            tw = _grad_target(W) if nW else None
            tb = _grad_target(b) if nb else None
            dW = tw if tw is not None else torch.zeros(W.shape, dtype=torch.float32, device=dev)
            db = (tb if tb is not None else torch.zeros(W.size(0), dtype=torch.float32, device=dev)) if nb else None
            in_place = in_place and (tw is not None or not nW) and (tb is not None or not nb)
            grads_w.append(None if (tw is not None or not nW) else dW)
            grads_b.append(None if (tb is not None or not nb) else db)
            scratch += [dW, db]
            descs.append(_ffi.GemmTnDesc(dZ=dZ.data_ptr(), X=X.data_ptr(), X2=None, in_scale=None, in_shift=None,
                                         in_scale2=None, in_shift2=None, dW=dW.data_ptr(), db=_ffi.ptr(db), M=C,
                                         lddz=dZ.size(1), ldx=X.size(1), ldx2=0, lddw=dW.stride(0), N=W.size(0), K=X.size(1),
                                         K2=0, in_relu=0))
        _ffi.gemm_tn(descs, dev, keep=[dhs, list(pooled), s_out, g_out, scratch], deferrable=ACCUMULATE_INTO_GRAD and in_place)
        return (None,) + tuple(dxs) + tuple(grads_w[:n_dims]) + tuple(grads_b[:n_dims]) + (grads_w[n_dims], grads_b[n_dims])


def head_train(xs, cell_ptrs, n_complexes, lin1_weights, lin1_biases, lin2_weight, lin2_bias, mean_readout=False,
               mean_final=False, drop_p: float = 0.0, drop_pos: int = 0):
    """(out, pooled list) with autograd: see _HeadTrain.  drop_p / drop_pos (_ffi.HEAD_DROP_*): the head's dropout, in-kernel.
    xs[d] may be a list of blocks (jumping knowledge, jump_mode 'cat')."""
    n = len(xs)
    flat, counts = [], []
    for x in xs:
        blk = list(x) if isinstance(x, (list, tuple)) else [x]
        if len(blk) > 1:
            w = int(blk[0].size(1))
            if (len(blk) > _ffi.HEAD_MAX_PARTS or w % 4 != 0 or
                    any(b.size(1) != w or b.size(0) != blk[0].size(0) or b.dtype != torch.float32 for b in blk)):
                blk = [torch.cat(blk, dim=-1)]
        flat += blk
        counts.append(len(blk))
    meta = (n, list(cell_ptrs), int(n_complexes), bool(mean_readout), bool(mean_final), float(drop_p), int(drop_pos), tuple(counts))
    res = _HeadTrain.apply(meta, *flat, *lin1_weights, *lin1_biases, lin2_weight, lin2_bias)
    return res[0], list(res[1:])


# ------------------------------------------------------------------------------------------------
# dropout without a mask tensor (csrc/cwn_dropout.h; include/cwn_hip.h: cwn_dropout)
# ------------------------------------------------------------------------------------------------
# F.dropout of the callers (mp/molec_models.py:104-106, 298-300, 338-346): the keep decision of an element is a pure function of
# (seed, step, site, element), so the launch that produces a value applies it in its epilogue and the launch that consumes the
# gradient re-derives it -- cwn_norm_act_f32 / cwn_norm_bwd_reduce_f32 for a conv layer's output, cwn_head_f32 / _bwd for the
# head's positions, cwn_dropout_f32 (a launch of its own, the same multipliers) everywhere else.  {seed, step} live in device
# memory: a TrainStep's opening launch (cwn_step_begin) advances `step`, so a replayed graph never repeats a mask; `site` is a
# host counter, new for every application (baked into a captured launch) and restarted by every step bracket (ops.step_arena):
# an eager step and the replay of its capture draw the same masks.
_drop_states: Dict[torch.device, Tensor] = {}
_drop_site = 0
DROPOUT_TRACE: Optional[list] = None          # tests: a list that receives (site, p, tag) of every application


def dropout_state(device) -> Tensor:
    """device int64 [2] {seed, step}; the seed is torch's (torch.initial_seed()) when the state is first needed."""
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    t = _drop_states.get(device)
    if t is None:
        seed = int(torch.initial_seed())
        try:                                   # data parallel: every rank its own stream (ranks usually share torch's seed)
            import torch.distributed as _dist
            if _dist.is_available() and _dist.is_initialized():
                seed += 0x9E3779B97F4A7C15 * int(_dist.get_rank())
        except Exception:
            pass
        t = _drop_states[device] = torch.tensor([seed & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64, device=device)
    return t


def dropout_seed(seed: int, device=None) -> None:
    """Re-seed (and rewind) the dropout stream of `device` (default: every device that has one, and the current one)."""
    global _drop_site
    _drop_site = 0
    devs = [torch.device(device)] if device is not None else (list(_drop_states) or [torch.device('cuda', torch.cuda.current_device())])
    for d in devs:
        dropout_state(d).copy_(torch.tensor([int(seed) & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64))


def dropout_record(device, p: float, site: Optional[int] = None, tag=None) -> '_ffi.Dropout':
    """The cwn_dropout record of a NEW application (or of `site`: the backward's)."""
    global _drop_site
    if site is None:
        _drop_site = (_drop_site + 1) & 0xFFFFFFFF
        site = _drop_site
        if DROPOUT_TRACE is not None:
            DROPOUT_TRACE.append((site, float(p), tag))
    return _ffi.Dropout(state=dropout_state(device).data_ptr(), p=float(p), site=int(site))


def dropout_apply(x: Tensor, rec: '_ffi.Dropout', out: Optional[Tensor] = None) -> Tensor:
    """out = x * multipliers(rec) over the last dimension's rows (cwn_dropout_f32)."""
    x2 = x if x.dim() == 2 else x.reshape(-1, x.size(-1) if x.dim() else 1)
    x2 = _rowmajor(x2, 'x')
    M, N = int(x2.size(0)), int(x2.size(1))
    if out is None:
        out = torch.empty(x2.shape, dtype=torch.float32, device=x2.device)
    elif out.dim() == 2:
        _out_window(out, M, N, 'out')
    if M and N:
        _ffi.check(_ffi.lib().cwn_dropout_f32(x2.data_ptr(), out.data_ptr(), M, N, ld(x2), ld(out), rec, _ffi.dyn(M),
                                              _ffi.stream_ptr(x2.device)), 'cwn_dropout_f32')
    return out.view(x.shape) if out.shape != x.shape else out


class _Dropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p):
        rec = dropout_record(x.device, p, tag=('tensor', tuple(x.shape)))
        ctx.p, ctx.site = float(p), int(rec.site)
        return dropout_apply(x, rec)

    @staticmethod
    def backward(ctx, g):
        return dropout_apply(g, dropout_record(g.device, ctx.p, ctx.site)), None


def dropout(x: Tensor, p: float, training: bool = True) -> Tensor:
    """F.dropout(x, p, training) on the device path: one launch forward, one backward, no mask tensor (the framework's form
    is a fused dropout launch + a mask tensor + a masked multiply in the backward).  CPU tensors / other dtypes: F.dropout."""
    if not training or p <= 0.0:
        return x
    if not x.is_cuda or x.dtype != torch.float32 or p >= 1.0 or x.numel() == 0:
        return torch.nn.functional.dropout(x, p=p, training=True)
    return _Dropout.apply(x, float(p))


def dropout_multipliers(shape, p: float, site: int, device, step: Optional[int] = None) -> Tensor:
    """The multipliers (0 or 1 / (1 - p)) application `site` uses over a matrix of `shape` at `step` (default: the current
    one) -- what a checker applies in its own arithmetic."""
    st = dropout_state(device)
    if step is not None:
        st = torch.stack([st[0], torch.tensor(int(step), dtype=torch.int64, device=st.device)])
    rec = _ffi.Dropout(state=st.data_ptr(), p=float(p), site=int(site))
    ones = torch.ones(shape, dtype=torch.float32, device=st.device)
    out = dropout_apply(ones, rec)
    torch.cuda.synchronize(st.device)           # (`st` may be a temporary)
    return out


# ------------------------------------------------------------------------------------------------
# dense parts: grouped fp32-MFMA GEMM (csrc/cwn_gemm.hip)
# ------------------------------------------------------------------------------------------------
def _rowmajor(t: Tensor, name: str) -> Tensor:
    """2-D fp32 GPU tensor whose rows are contiguous (column slices of a Linear weight qualify)."""
    _ffi.require_gpu(t, name)
    if t.dtype != torch.float32 or t.dim() != 2:
        raise TypeError(f'{name} must be a 2-D float32 tensor (got {t.dtype}, {t.dim()}-D): the GEMM kernels are fp32 MFMA '
                        'only; float64 products run on torch.nn.Linear')
    return rowmajor(t)


def _rowmajor16(t: Tensor, name: str) -> Tensor:
    """`_rowmajor` for the F-wide inputs of cwn_update_mlp_f32 / _mlp3_f32, read 16 bytes at a time: copied where the entry refuses it."""
    t = _rowmajor(t, name)
    return rowmajor16(t, ld(t))


def _out_window(out: Tensor, rows: int, cols: int, name: str) -> Tensor:
    """A preallocated output handed to a launch by address and row stride: it has to BE row-major (a column window of a wider
    matrix is) -- a transposed or column-strided view would receive a row-major image beside its own elements.  An output
    cannot be copied the way `_rowmajor` copies an input: it is refused."""
    if out.dim() != 2 or tuple(out.shape) != (rows, cols) or out.dtype != torch.float32:
        raise ValueError(f'{name} must be a float32 [{rows}, {cols}] matrix (got {out.dtype} {tuple(out.shape)})')
    if not is_rowmajor(out):
        raise ValueError(f'{name} must be row-major (unit column stride, row stride >= {cols}); got strides {tuple(out.stride())}: '
                         'a window of a wider matrix is fine, a transposed or column-strided view is not')
    return out


@dataclass
class Gemm:
    """Y = epilogue([X | X2] @ W^T + bias): see cwn_gemm_desc in include/cwn_hip.h."""
    X: Tensor
    W: Tensor                      # [N, K (+K2)], torch Linear layout (a column slice is fine)
    bias: Optional[Tensor] = None
    X2: Optional[Tensor] = None
    relu: bool = False
    out_scale: Optional[Tensor] = None   # BatchNorm (eval) folded to a per-column affine; no grad
    out_shift: Optional[Tensor] = None
    in_scale: Optional[Tensor] = None    # producer's BatchNorm apply (+ReLU) on the fly; no grad
    in_shift: Optional[Tensor] = None
    in_relu: int = 0                     # bit 0: ReLU on X after the affine, bit 1: on X2
    col_stats: Optional[Tensor] = None   # [2, stat_rows(M), N] fp64 out: per-32-row-band sum / sum of squares
    debug: int = 0                       # timing experiments only (tools/ubench_gemm.py)
    exact: bool = False                  # keep the launch on the exact fp32-MFMA kernel (CWN_GEMM_EXACT)
    in_scale2: Optional[Tensor] = None   # the same prologue for X2
    in_shift2: Optional[Tensor] = None
    w_trans: bool = False                # W is [K (+K2), N]: Y = [X | X2] @ W  (dX = dY @ W of a Linear)
    out: Optional[Tensor] = None         # preallocated Y (may be a column slice of a wider matrix)
    w_col0: Optional[int] = None         # use columns [w_col0, w_col0 + K + K2) of W (not with w_trans):
                                         # lets autograd see the whole Parameter instead of a slice
    w_packed: Optional[Tensor] = None    # pack_gemm_weight(W): used when the launch runs on the bf16-split path
                                         # (inference: one split per weight version, not per workgroup)
    add_out: bool = False                # `out` += the product instead of `out` = the product (no other writer of `out`)
    bnb: Optional[object] = None         # _ffi.GemmBnb: X is dy of a BatchNorm / ReLU stage, the GEMM multiplies its dz (w_trans only)
    # cwn_dense_stage_f32 only (include/cwn_hip.h: cwn_bn_live): the statistics of Y go to `stat_slots` ([BN_SLOTS, 2, F] fp64,
    # zero on entry); the prologue of X / X2 is the BatchNorm record `in_bn` / `in_bn2` (_ffi.BnLive), derived in the kernel
    stat_slots: Optional[Tensor] = None
    in_bn: Optional[object] = None
    in_bn2: Optional[object] = None
    # cwn_dense_stage_ex_f32 only: a third / fourth K-block (CIN++'s 3F / 4F-wide combine) -- (X, relu, _ffi.BnLive or None)
    # each; W is then [F, 3F] / [F, 4F]
    more: Sequence = ()

    def desc(self, Y: Tensor, packed: bool = False) -> _ffi.GemmDesc:
        if self.more:
            raise RuntimeError('a product of more than two K-blocks is served by cwn_dense_stage_ex_f32 only')
        X, W, X2 = self.X, self.W, self.X2
        packed = packed and self.w_packed is not None
        K = X.size(1)
        K2 = X2.size(1) if X2 is not None else 0
        if self.w_col0 is not None:
            if self.w_trans or W.size(1) < self.w_col0 + K + K2:
                raise ValueError('w_col0 selects columns of an untransposed weight')
        elif W.size(0 if self.w_trans else 1) != K + K2:
            raise ValueError(f'weight has {W.size(0 if self.w_trans else 1)} input columns, '
                             f'operands have {K + K2}')
        if X2 is not None and X2.size(0) != X.size(0):
            raise ValueError('X and X2 must have the same number of rows')
        cs = self.col_stats
        m_dev = _ffi.dyn(X.size(0))
        if m_dev is not None and (cs is not None or self.bnb is not None):
            # (cwn_gemm_f32 refuses m_dev with col_sum / col_sumsq / bnb; WITHOUT it the statistics epilogue sums, and the
            #  BatchNorm-backward prologue divides by, the capacity rows of a static batch -- stale rows of an earlier batch in
            #  every BatchNorm of every step.  cwn_dense_stage_f32 / cwn_dense_stage_bwd_f32 carry the count.)
            raise RuntimeError('cwn_gemm_f32 takes no device-side row count together with BatchNorm statistics or the '
                               'BatchNorm-backward prologue: inside a static batch these launches run on the stage kernels '
                               '(cwn_dense_stage_f32 / cwn_dense_stage_bwd_f32: hidden width 64 or 128, and not with '
                               'CWN_STAGE_KERNEL=0 / ops.STAGE_KERNEL = False)')
        return _ffi.GemmDesc(
            X=X.data_ptr(), X2=_ffi.ptr(X2), W=self.w_packed.data_ptr() if packed else W.data_ptr() + 4 * (self.w_col0 or 0),
            bias=_ffi.ptr(self.bias),
            in_scale=_ffi.ptr(self.in_scale), in_shift=_ffi.ptr(self.in_shift),
            in_scale2=_ffi.ptr(self.in_scale2), in_shift2=_ffi.ptr(self.in_shift2),
            out_scale=_ffi.ptr(self.out_scale), out_shift=_ffi.ptr(self.out_shift),
            col_sum=None if cs is None else cs[0].data_ptr(),
            col_sumsq=None if cs is None else cs[1].data_ptr(),
            Y=Y.data_ptr(), M=X.size(0), ldx=ld(X, max(K, 1)), ldx2=ld(X2, max(K2, 1)) if X2 is not None else 0, ldw=ld(W), ldy=ld(Y),
            N=W.size(1 if self.w_trans else 0), K=K, K2=K2, relu=int(self.relu), in_relu=int(self.in_relu),
            w_trans=int(self.w_trans), bnb=None if self.bnb is None else C.pointer(self.bnb),
            # (a static batch: the rows that exist -- the launch walks the row tiles below the device-side count only)
            m_dev=m_dev,
            flags=(_ffi.GEMM_EXACT if (self.exact or GEMM_EXACT) else 0) | (_ffi.GEMM_W_PACKED if packed else 0)
            | (_ffi.GEMM_ADD_OUT if self.add_out else 0) | (int(self.debug) << 8))


def stat_rows(M: int) -> int:
    """CWN_STAT_ROWS: 32-row bands the statistics epilogue of cwn_gemm_f32 writes partials for."""
    return (int(M) + 31) // 32


GEMM_MAX_K = 256   # K + K2 the MFMA kernel supports (whole-K weight tile resident in LDS)

# Precision policy of the dense launches, applied PER CALL through cwn_gemm_desc.flags (the library
# keeps no state): False (default) = eligible launches run on the bf16 matrix pipe through the exact
# three-way split (fp32 accuracy, csrc/cwn_split.h); True (or CWN_GEMM_SPLIT=0 in the environment) =
# every launch on the exact fp32-MFMA kernel, and the complex-blocked layer kernel (which has only
# the split form) is not used.
GEMM_EXACT = os.environ.get('CWN_GEMM_SPLIT') == '0'


def set_gemm_exact(exact: bool) -> bool:
    """Set the module's dense precision policy; returns the previous value."""
    global GEMM_EXACT
    prev, GEMM_EXACT = GEMM_EXACT, bool(exact)
    return prev


def run_gemm(gemms: Sequence[Gemm], device) -> List[Tensor]:
    """Raw grouped launch (no autograd)."""
    outs, descs = [], []
    for gm in gemms:
        if gm.stat_slots is not None or gm.in_bn is not None or gm.in_bn2 is not None:
            raise RuntimeError('a live BatchNorm record (cwn_bn_live) is served by cwn_dense_stage_f32 only')
        gm.X, gm.W = _rowmajor(gm.X, 'X'), _rowmajor(gm.W, 'W')
        if gm.X2 is not None:
            gm.X2 = _rowmajor(gm.X2, 'X2')
        Y = gm.out
        if Y is None:
            Y = torch.empty(gm.X.size(0), gm.W.size(1 if gm.w_trans else 0), dtype=torch.float32,
                            device=device)
        else:
            _ffi.require_gpu(Y, 'out')
            _out_window(Y, int(gm.X.size(0)), int(gm.W.size(1 if gm.w_trans else 0)), 'out')
        outs.append(Y)
        if Y.numel():
            descs.append(gm.desc(Y))
    if descs:
        # packed weights exist in the split kernel's form only: use them when this launch runs there
        if any(gm.w_packed is not None for gm in gemms) and len(descs) <= _ffi.MAX_DESCS and _ffi.gemm_would_split(descs):
            descs = [gm.desc(Y, packed=True) for gm, Y in zip(gemms, outs) if Y.numel()]
        _ffi.gemm(descs, device)
    return outs


def gemm_uses_split(gemms: Sequence[Gemm], device) -> bool:
    """True when run_gemm(gemms) is served by the bf16-split kernel (cwn_gemm_split.hip)."""
    descs = []
    for gm in gemms:
        Y = gm.out if gm.out is not None else torch.empty(gm.X.size(0), gm.W.size(1 if gm.w_trans else 0),
                                                          dtype=torch.float32, device=device)
        if Y.numel():
            descs.append(gm.desc(Y))
    return bool(descs) and len(descs) <= _ffi.MAX_DESCS and _ffi.gemm_would_split(descs)


# Off by default: adding dW straight into an existing `.grad` and returning None to autograd skips
# parameter grad hooks (DDP's reducer), breaks torch.autograd.grad() and gradient checkpointing.
# cwn_amd.train.TrainStep -- which owns the flat gradient bucket and the all-reduce -- turns it on
# around its own backward with `accumulate_into_grad()`.
ACCUMULATE_INTO_GRAD = False
DEFER_WEIGHT_GRADS = os.environ.get('CWN_DEFER_WEIGHT_GRADS') != '0'     # A/B: '0' launches every weight gradient where it arises


class accumulate_into_grad:
    """Context manager: inside, the weight-gradient kernels add into existing `.grad` buffers directly."""

    def __init__(self, on: bool = True):
        self.on = on

    def __enter__(self):
        global ACCUMULATE_INTO_GRAD
        self.prev, ACCUMULATE_INTO_GRAD = ACCUMULATE_INTO_GRAD, self.on
        # ... and, since nothing reads those buffers before the caller's optimizer step, the weight-gradient launches
        # are collected and run together when the block ends (_ffi.gemm_tn / flush_tn)
        self.defer = self.on and DEFER_WEIGHT_GRADS and _ffi._tn_queue is None
        if self.defer:
            _ffi.defer_tn(True)
        return self

    def __exit__(self, *exc):
        global ACCUMULATE_INTO_GRAD
        ACCUMULATE_INTO_GRAD = self.prev
        if self.defer:
            if exc[0] is None:
                _ffi.flush_tn()
            else:
                _ffi._tn_queue.clear()
            _ffi.defer_tn(False)
        return False


def _grad_target(p: Optional[Tensor]) -> Optional[Tensor]:
    """The tensor a gradient kernel may accumulate into directly: the parameter's existing `.grad`
    (leaf tensors only; fp32, row-major, same shape), or None.  With a target the backward
    returns None to autograd for that input: `p.grad += dW` has already happened, without the
    per-parameter add kernel autograd would launch (265 of them per step for the ZINC model).
    Only inside `accumulate_into_grad()` (a plain .backward() into buffers the caller owns)."""
    if not ACCUMULATE_INTO_GRAD or p is None or not p.is_leaf or not p.requires_grad:
        return None
    g = p.grad
    if (g is None or g.dtype != torch.float32 or g.shape != p.shape or g.device != p.device
            or (g.dim() == 2 and (g.stride(1) != 1 or g.stride(0) < g.size(1)))       # (stricter than is_rowmajor: ONE row is judged too)
            or (g.dim() == 1 and g.stride(0) != 1)):
        return None
    return g


def _gemm_backward(gemms, tensors, outs, needs, gs, acc=None) -> List[Optional[Tensor]]:
    """Gradients of gemm_many's tensor inputs (four per GEMM: X, X2, W, bias; `needs` likewise).
    Grouped launches again: every dX (and dX2) of the group is one transposed-weight
    cwn_gemm_f32, every dW / db one cwn_gemm_tn_f32 (accumulating into one zeroed buffer).
    `acc` (identity of an input tensor -> buffer): the FIRST product into that input is added onto the buffer in the GEMM's
    epilogue (CWN_GEMM_ADD_OUT) instead of written to a new matrix, and its slot gets None -- the caller hands the buffer on."""
    n = len(gemms)
    grads: List[Optional[Tensor]] = [None] * (4 * n)
    live = []
    nn_specs, nn_slot, tn_jobs, total = [], [], [], 0
    for k, gm in enumerate(gemms):
        g = gs[k]
        if g is None:
            continue
        X, X2, W, bias = tensors[4 * k: 4 * k + 4]
        nX, nX2, nW, nb = needs[4 * k: 4 * k + 4]
        if gm.relu:
            g = g * (outs[k] > 0)
        if gm.out_scale is not None:
            g = g * gm.out_scale
        g = _rowmajor(g, 'grad')
        live.append(g)
        K = X.size(1)
        c0 = gm.w_col0 or 0
        if nX:
            into = None if acc is None else acc.pop(_ident(X), None)        # (one product per buffer: the kernel's contract)
            nn_specs.append(Gemm(X=g, W=W[:, c0:c0 + K], w_trans=True, out=into, add_out=into is not None))
            nn_slot.append(None if into is not None else 4 * k)
        if nX2 and X2 is not None:
            into = None if acc is None else acc.pop(_ident(X2), None)
            nn_specs.append(Gemm(X=g, W=W[:, c0 + K:c0 + K + X2.size(1)], w_trans=True, out=into, add_out=into is not None))
            nn_slot.append(None if into is not None else 4 * k + 1)
        want_b = nb and bias is not None
        if nW or want_b:
            tn_jobs.append((k, g, X, X2, W, bias, nW, want_b, c0))
    dev = live[0].device if live else None
    if nn_specs:
        for slot, y in zip(nn_slot, run_gemm(nn_specs, dev)):
            if slot is not None:
                grads[slot] = y
    if tn_jobs:
        # gradient targets: the parameter's own .grad when it is allocated (a FlatGradBucket /
        # zero_grad(set_to_none=False)) and ACCUMULATE_INTO_GRAD is on -- the kernel adds into it
        # and autograd gets None -- else one zeroed scratch buffer handed back to autograd
        targets, scratch = [], 0
        for k, g, X, X2, W, bias, nW, want_b, c0 in tn_jobs:
            tw = _grad_target(W) if nW else None
            tb = _grad_target(bias) if want_b else None
            targets.append((tw, tb))
            scratch += (W.numel() if nW and tw is None else 0) + (W.size(0) if want_b and tb is None else 0)
        flat = torch.zeros(scratch, dtype=torch.float32, device=dev) if scratch else None
        off, descs = 0, []
        for (k, g, X, X2, W, bias, nW, want_b, c0), (tw, tb) in zip(tn_jobs, targets):
            Xc = _rowmajor(X, 'X')
            X2c = None if X2 is None else _rowmajor(X2, 'X2')
            live += [Xc, X2c]
            dW = db = None
            if nW:
                if tw is None:
                    dW = flat[off: off + W.numel()].view(W.size(0), W.size(1))
                    off += W.numel()
                    grads[4 * k + 2] = dW
                else:
                    dW = tw
            if want_b:
                if tb is None:
                    db = flat[off: off + W.size(0)]
                    off += W.size(0)
                    grads[4 * k + 3] = db
                else:
                    db = tb
            if g.size(0):
                if dW is None:      # only the bias gradient is wanted: a throw-away dW
                    dW = torch.zeros(W.size(0), W.size(1), dtype=torch.float32, device=dev)
                descs.append(_ffi.GemmTnDesc(
                    dZ=g.data_ptr(), X=Xc.data_ptr(), X2=_ffi.ptr(X2c), in_scale=None, in_shift=None,
                    in_scale2=None, in_shift2=None, dW=dW.data_ptr() + 4 * c0, db=_ffi.ptr(db), M=g.size(0),
                    lddz=ld(g), ldx=ld(Xc), ldx2=0 if X2c is None else ld(X2c), lddw=dW.stride(0),
                    N=W.size(0), K=Xc.size(1), K2=0 if X2c is None else X2c.size(1), in_relu=0))
        if descs:
            # in-place targets only (no scratch handed back to autograd): the launch may wait for the end of the backward
            _ffi.gemm_tn(descs, dev, keep=live + [flat], deferrable=ACCUMULATE_INTO_GRAD and flat is None)
    return grads


class _GemmMany(torch.autograd.Function):
    """Grouped GEMM forward on the MFMA kernel; tensor inputs flattened (X, X2, W, bias) per GEMM.
    Backward: dX = g W, dW = g^T [X|X2], db = sum g on the same kernels (see backward)."""

    @staticmethod
    def forward(ctx, gemms: Tuple[Gemm, ...], device, *tensors):
        outs = run_gemm(gemms, device)
        ctx.gemms = gemms
        ctx.save_for_backward(*tensors, *outs)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        n = len(ctx.gemms)
        saved = ctx.saved_tensors
        grads = _gemm_backward(ctx.gemms, saved[:4 * n], saved[4 * n:], ctx.needs_input_grad[2:], gs)
        return (None, None) + tuple(grads)


def gemm_many(gemms: Sequence[Gemm]) -> List[Tensor]:
    """All GEMMs in ONE launch (per <= 8); differentiable w.r.t. X, X2, W, bias."""
    flat: List[Optional[Tensor]] = []
    device = gemms[0].X.device
    for gm in gemms:
        if gm.in_scale is not None and torch.is_grad_enabled() and gm.X.requires_grad:
            raise NotImplementedError('the input-affine prologue has no backward; apply it outside')
        flat += [gm.X, gm.X2, gm.W, gm.bias]
    if not (torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in flat)):
        return run_gemm(gemms, device)
    return list(_GemmMany.apply(tuple(gemms), device, *flat))


# ------------------------------------------------------------------------------------------------
# a Linear product beyond GEMM_MAX_K, K streamed, under a device-side row count (csrc/cwn_linear_wide.hip)
# ------------------------------------------------------------------------------------------------
_WIDE_ROWS = dict(dtypes=(torch.float32,), what='linear_wide: ',
                  hint='cwn_linear_wide_f32 computes in fp32 only (float64 products run on torch.nn.functional.linear)')


def linear_wide_applies(K: int, K2: int, N: int) -> bool:
    """The shapes cwn_linear_wide_f32 takes: 1 <= N <= 256, K >= 1, K2 >= 0, K + K2 <= 512."""
    return 1 <= N <= _ffi.LINEAR_WIDE_MAX_N and K >= 1 and K2 >= 0 and K + K2 <= _ffi.LINEAR_WIDE_MAX_K


def _wide_desc(X: Tensor, X2: Optional[Tensor], W: Tensor, bias: Optional[Tensor], Y: Tensor, w_trans: bool) -> '_ffi.LinearWideDesc':
    return _ffi.LinearWideDesc(X=X.data_ptr(), X2=_ffi.ptr(X2), W=W.data_ptr(), bias=_ffi.ptr(bias), Y=Y.data_ptr(),
                               M=X.size(0), ldx=ld(X), ldx2=0 if X2 is None else ld(X2), ldw=ld(W), ldy=ld(Y),
                               N=Y.size(1), K=X.size(1), K2=0 if X2 is None else X2.size(1), w_trans=int(w_trans))


def _wide_operands(X, X2, weight, bias):
    for t, name in ((X, 'X'), (X2, 'X2'), (weight, 'weight'), (bias, 'bias')):      # every dtype before the first device
        if t is not None:
            _operand_dtype(t, name, _WIDE_ROWS['dtypes'], _WIDE_ROWS['what'], _WIDE_ROWS['hint'])
    X = _rows_operand(X, 'X', 2, **_WIDE_ROWS)
    X2 = _rows_operand(X2, 'X2', 2, **_WIDE_ROWS)
    weight = _rows_operand(weight, 'weight', 2, **_WIDE_ROWS)
    bias = _rows_operand(bias, 'bias', 1, **_WIDE_ROWS)
    if X is None or weight is None:
        raise TypeError('linear_wide: X and weight are required')
    K, K2, N = X.size(1), 0 if X2 is None else X2.size(1), weight.size(0)
    if weight.size(1) != K + K2:
        raise ValueError(f'linear_wide: weight has {weight.size(1)} input columns, the operands have {K + K2}')
    if X2 is not None and (X2.size(0) != X.size(0) or K2 == 0):
        raise ValueError('linear_wide: X and X2 must have the same number of rows, and X2 at least one column')
    if bias is not None and bias.numel() != N:
        raise ValueError(f'linear_wide: bias has {bias.numel()} entries, weight {N} rows')
    if not linear_wide_applies(K, K2, N):
        raise ValueError(f'linear_wide: cwn_linear_wide_f32 takes 1 <= N <= {_ffi.LINEAR_WIDE_MAX_N}, K >= 1 and K + K2 <= '
                         f'{_ffi.LINEAR_WIDE_MAX_K} (got N = {N}, K = {K}, K2 = {K2})')
    return X, X2, weight, bias


class _LinearWide(torch.autograd.Function):
    """Forward: one cwn_linear_wide_f32 launch.  Backward: dX / dX2 = g W[:, :K] / g W[:, K:] as one launch of the transposed
    form (the layer's own weight, no copy), dW / db one cwn_gemm_tn_f32 launch; all under the row count of _ffi.dyn."""

    @staticmethod
    def forward(ctx, X, X2, weight, bias):
        Y = torch.empty(X.size(0), weight.size(0), dtype=torch.float32, device=X.device)
        if Y.numel():
            _ffi.linear_wide([_wide_desc(X, X2, weight, bias, Y, False)], X.device)
        ctx.has_bias = bias is not None
        ctx.params = (weight, bias)                 # (the Parameters: their .grad is the target inside accumulate_into_grad())
        ctx.save_for_backward(X, X2, weight)
        return Y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        X, X2, W = ctx.saved_tensors
        weight_p, bias_p = ctx.params
        nX, nX2, nW, nb = ctx.needs_input_grad
        dev, K, N = X.device, X.size(1), W.size(0)
        K2 = 0 if X2 is None else X2.size(1)
        g = _rowmajor(g, 'grad')
        dX = dX2 = dW = db = None
        descs = []
        CN = _ffi.LINEAR_WIDE_MAX_N                 # (the transposed form's N is an input width: column blocks of at most 256)
        if nX:
            dX = torch.empty(X.size(0), K, dtype=torch.float32, device=dev)
            descs += [_wide_desc(g, None, W[:, c:min(c + CN, K)], None, dX[:, c:min(c + CN, K)], True) for c in range(0, K, CN)]
        if nX2 and X2 is not None:
            dX2 = torch.empty(X.size(0), K2, dtype=torch.float32, device=dev)
            descs += [_wide_desc(g, None, W[:, K + c:K + min(c + CN, K2)], None, dX2[:, c:min(c + CN, K2)], True)
                      for c in range(0, K2, CN)]
        if descs and g.size(0):
            _ffi.linear_wide(descs, dev)
        want_b = nb and ctx.has_bias
        if nW or want_b:
            tw = _grad_target(weight_p) if nW else None
            tb = _grad_target(bias_p) if want_b else None
            in_place = (tw is not None or not nW) and (tb is not None or not want_b)
            # (a throw-away dW when only the bias gradient is wanted: cwn_gemm_tn_f32 always accumulates one)
            tgt_w = tw if tw is not None else torch.zeros(N, K + K2, dtype=torch.float32, device=dev)
            tgt_b = None
            if want_b:
                tgt_b = tb if tb is not None else torch.zeros(N, dtype=torch.float32, device=dev)
            if nW and tw is None:
                dW = tgt_w
            if want_b and tb is None:
                db = tgt_b
            if g.size(0):
                tn = dict(dZ=g.data_ptr(), in_scale=None, in_shift=None, in_scale2=None, in_shift2=None, M=g.size(0), lddz=ld(g),
                          lddw=tgt_w.stride(0), N=N, in_relu=0)
                if X2 is None or K % 4 == 0:
                    tns = [_ffi.GemmTnDesc(X=X.data_ptr(), X2=_ffi.ptr(X2), dW=tgt_w.data_ptr(), db=_ffi.ptr(tgt_b), ldx=ld(X),
                                           ldx2=0 if X2 is None else ld(X2), K=K, K2=K2, **tn)]
                else:
                    # (cwn_gemm_tn_f32 wants K % 4 == 0 next to X2: two descriptors into the column halves of dW)
                    tns = [_ffi.GemmTnDesc(X=X.data_ptr(), X2=None, dW=tgt_w.data_ptr(), db=_ffi.ptr(tgt_b), ldx=ld(X), ldx2=0,
                                           K=K, K2=0, **tn),
                           _ffi.GemmTnDesc(X=X2.data_ptr(), X2=None, dW=tgt_w.data_ptr() + 4 * K, db=None, ldx=ld(X2), ldx2=0,
                                           K=K2, K2=0, **tn)]
                # in-place targets only (nothing handed back to autograd): the launch may wait for the end of the backward
                _ffi.gemm_tn(tns, dev, keep=[g, X, X2, tgt_w, tgt_b], deferrable=ACCUMULATE_INTO_GRAD and in_place)
        return dX, dX2, dW, db


def linear_wide(X: Tensor, X2: Optional[Tensor], weight: Tensor, bias: Optional[Tensor] = None) -> Tensor:
    """[X | X2] @ weight.T + bias in float32 from ONE cwn_linear_wide_f32 launch: weight [N, K + K2] with N <= 256 and
    K + K2 <= 512 -- beyond GEMM_MAX_K (the combine network of a 160-wide layer: Linear(320 -> 160)).  X2 and bias may be
    None; rows may be strided views.  Differentiable w.r.t. all four; inside a static batch (_ffi.dynamic_rows) the forward
    and every part of the backward take the rows that exist from the device-side count, so rows behind the count are neither
    written nor summed into dW / db.  Inside accumulate_into_grad() dW / db are added into the parameters' .grad."""
    X, X2, weight, bias = _wide_operands(X, X2, weight, bias)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (X, X2, weight, bias)):
        return _LinearWide.apply(X, X2, weight, bias)
    Y = torch.empty(X.size(0), weight.size(0), dtype=torch.float32, device=X.device)
    if Y.numel():
        _ffi.linear_wide([_wide_desc(X, X2, weight.detach(), None if bias is None else bias.detach(), Y, False)], X.device)
    return Y


# ------------------------------------------------------------------------------------------------
# LayerNorm (+ ReLU) over the rows of several matrices: graph_norm='ln' (csrc/cwn_layernorm.hip)
# ------------------------------------------------------------------------------------------------
def _ln_descs(zs, gammas, betas, outs, epss, relu: bool, stats=None) -> List['_ffi.LnDesc']:
    descs, off = [], 0
    for k, (z, out) in enumerate(zip(zs, outs)):
        M, N = z.shape
        if M:
            d = _ffi.LnDesc(z=z.data_ptr(), gamma=_ffi.ptr(gammas[k]), beta=_ffi.ptr(betas[k]), out=out.data_ptr(),
                            M=M, ldz=ld(z), ldout=ld(out), N=N, relu=int(relu), eps=float(epss[k]))
            if stats is not None:
                d.mean, d.rstd = stats[0, off:].data_ptr(), stats[1, off:].data_ptr()
            descs.append(d)
        off += M
    return descs


class _LayerNormActMany(torch.autograd.Function):
    """tensors = (z, gamma, beta) per matrix (gamma / beta None without the affine).  The forward is one
    cwn_layernorm_act_f32 launch and keeps z, out and the rows' mean / rstd; the backward is one cwn_layernorm_bwd_f32
    call (dz, and the column sums dgamma / dbeta without atomics)."""

    @staticmethod
    def forward(ctx, relu: bool, epss: Tuple[float, ...], *tensors):
        n = len(tensors) // 3
        zs = [_rowmajor(tensors[3 * k], 'z') for k in range(n)]
        gammas = [None if tensors[3 * k + 1] is None else tensors[3 * k + 1].contiguous() for k in range(n)]
        betas = [None if tensors[3 * k + 2] is None else tensors[3 * k + 2].contiguous() for k in range(n)]
        dev = zs[0].device
        outs = [torch.empty(z.size(0), z.size(1), dtype=torch.float32, device=dev) for z in zs]
        stats = torch.empty(2, max(sum(z.size(0) for z in zs), 1), dtype=torch.float32, device=dev)
        descs = _ln_descs(zs, gammas, betas, outs, epss, relu, stats)
        if descs:
            _ffi.layer_norm_act(descs, dev)
        ctx.relu, ctx.epss, ctx.n = relu, epss, n
        ctx.params = [(tensors[3 * k + 1], tensors[3 * k + 2]) for k in range(n)]     # (the Parameters: their .grad is the target)
        ctx.save_for_backward(stats, *zs, *outs, *[g for g in gammas if g is not None])
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gs):
        n, relu = ctx.n, ctx.relu
        saved = ctx.saved_tensors
        stats, zs, outs = saved[0], saved[1:1 + n], saved[1 + n:1 + 2 * n]
        gsaved = iter(saved[1 + 2 * n:])
        needs = ctx.needs_input_grad[2:]
        grads: List[Optional[Tensor]] = [None] * (3 * n)
        dev = stats.device
        descs, live, off = [], [], 0
        for k in range(n):
            z, out = zs[k], outs[k]
            M, N = z.shape
            gamma_p, beta_p = ctx.params[k]
            gamma = next(gsaved) if gamma_p is not None else None
            g = gs[k]
            row0, off = off, off + M
            if g is None:
                continue
            want_g = gamma_p is not None and needs[3 * k + 1]
            want_b = beta_p is not None and needs[3 * k + 2]
            # the column sums go straight into the parameters' .grad where both wanted ones have one (accumulate_into_grad())
            tg = _grad_target(gamma_p) if want_g else None
            tb = _grad_target(beta_p) if want_b else None
            acc = (want_g or want_b) and (tg is not None or not want_g) and (tb is not None or not want_b)
            dgamma = dbeta = None
            if want_g:
                dgamma = tg if acc else torch.zeros(N, dtype=torch.float32, device=dev)
                grads[3 * k + 1] = None if acc else dgamma
            if want_b:
                dbeta = tb if acc else torch.zeros(N, dtype=torch.float32, device=dev)
                grads[3 * k + 2] = None if acc else dbeta
            dy = _rowmajor(g, 'grad')
            dz = torch.empty(M, N, dtype=torch.float32, device=dev)
            if needs[3 * k]:
                grads[3 * k] = dz
            live += [dy, dz, dgamma, dbeta]
            if M:
                descs.append(_ffi.LnDesc(
                    z=z.data_ptr(), gamma=_ffi.ptr(gamma), out=out.data_ptr(), mean=stats[0, row0:].data_ptr(),
                    rstd=stats[1, row0:].data_ptr(), dy=dy.data_ptr(), dz=dz.data_ptr(), dgamma=_ffi.ptr(dgamma),
                    dbeta=_ffi.ptr(dbeta), M=M, ldz=ld(z), ldout=ld(out), lddy=ld(dy), lddz=ld(dz), N=N,
                    relu=int(relu), eps=float(ctx.epss[k]), accumulate=int(bool(acc))))
        if descs:
            _ffi.layer_norm_bwd(descs, dev)
        return (None, None) + tuple(grads)


def _ln_on_kernel(z: Tensor, norm) -> bool:
    """Does cwn_layernorm_* take this matrix?  float32 rows of at most _ffi.LN_MAX_N columns on the GPU, normalised over the
    last dimension; float64, CPU tensors and wider rows run torch.nn.functional.layer_norm."""
    for t in (z, norm.weight, norm.bias):
        if t is not None and t.dtype in (torch.float16, torch.bfloat16):
            raise TypeError(f'layer_norm_act_many computes in float32 (or float64 through torch): got {t.dtype}')
    return (z.is_cuda and z.dtype == torch.float32 and z.dim() == 2 and tuple(norm.normalized_shape) == (z.size(1),)
            and 1 <= z.size(1) <= _ffi.LN_MAX_N
            and all(p is None or (p.is_cuda and p.dtype == torch.float32) for p in (norm.weight, norm.bias)))


def layer_norm_act_many(zs: Sequence[Tensor], norms: Sequence[torch.nn.LayerNorm], relu: bool = True) -> List[Tensor]:
    """act(norm_k(z_k)) for every matrix of a stage in ONE launch (per <= 16), act = ReLU or nothing; differentiable
    w.r.t. z, weight and bias.  Inside accumulate_into_grad() the weight / bias gradients are added into their .grad."""
    if len(zs) != len(norms):
        raise ValueError('one LayerNorm per matrix')
    res: List[Optional[Tensor]] = [None] * len(zs)
    take = []
    for k, (z, norm) in enumerate(zip(zs, norms)):
        if _ln_on_kernel(z, norm):
            take.append(k)
        else:
            y = torch.nn.functional.layer_norm(z, norm.normalized_shape, norm.weight, norm.bias, norm.eps)
            res[k] = torch.relu(y) if relu else y
    if not take:
        return res
    flat: List[Optional[Tensor]] = []
    for k in take:
        flat += [zs[k], norms[k].weight, norms[k].bias]
    epss = tuple(float(norms[k].eps) for k in take)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in flat):
        outs = _LayerNormActMany.apply(bool(relu), epss, *flat)
    else:
        zc = [_rowmajor(zs[k], 'z') for k in take]
        gammas = [None if norms[k].weight is None else norms[k].weight.detach().contiguous() for k in take]
        betas = [None if norms[k].bias is None else norms[k].bias.detach().contiguous() for k in take]
        outs = [torch.empty(z.size(0), z.size(1), dtype=torch.float32, device=z.device) for z in zc]
        descs = _ln_descs(zc, gammas, betas, outs, epss, bool(relu))
        if descs:
            _ffi.layer_norm_act(descs, zc[0].device)
    for k, o in zip(take, outs):
        res[k] = o
    return res


# ------------------------------------------------------------------------------------------------
# OrientedConv as one launch (csrc/cwn_oriented.hip)
# ------------------------------------------------------------------------------------------------
def _oriented_launch(x: Tensor, up, dn, w_self, w_up, w_dn, act: int, H: int, agg_out: Optional[Tensor] = None,
                     trans: bool = False) -> Tensor:
    """One cwn_oriented_layer_f32 call.  `up` / `dn`: (built plan, orient [E] float32 or None), or None for an absent
    stream (its weight is then not passed either)."""
    n, w = x.shape
    out = torch.empty(n, H, dtype=torch.float32, device=x.device)
    if n == 0:
        return out
    d = _ffi.OrientedDesc(x=x.data_ptr(), w_self=_ffi.ptr(w_self), out=out.data_ptr(), agg_out=_ffi.ptr(agg_out), n=n,
                          ldx=x.stride(0), ldout=H, w=w, H=H, act=int(act), w_trans=int(bool(trans)))
    if up is not None:
        d.up_rowptr, d.up_col, d.up_perm = up[0].rowptr.data_ptr(), up[0].col.data_ptr(), up[0].perm.data_ptr()
        d.up_orient, d.w_up = _ffi.ptr(up[1]), w_up.data_ptr()
    if dn is not None:
        d.dn_rowptr, d.dn_col, d.dn_perm = dn[0].rowptr.data_ptr(), dn[0].col.data_ptr(), dn[0].perm.data_ptr()
        d.dn_orient, d.w_dn = _ffi.ptr(dn[1]), w_dn.data_ptr()
    _ffi.oriented_layer(d, x.device)
    return out


class _OrientedLayer(torch.autograd.Function):
    """out = act(x W^T + (A_up o x) W_up^T + (A_dn o x) W_dn^T): one launch forward; backward dZ = g * act'(out) (one launch,
    none for 'id'), dx through the same kernel over the transposed plans (one launch, skipped when x needs no gradient) and
    the weight gradients as ONE cwn_gemm_tn_f32 call over dZ against x and the two halves of the stored aggregates."""

    @staticmethod
    def forward(ctx, x, w_self, w_up, w_dn, up, dn, act, H):
        need = ctx.needs_input_grad
        n, w = x.shape
        agg = None
        if (need[2] and up is not None) or (need[3] and dn is not None):
            agg = torch.empty(n, 2 * w, dtype=torch.float32, device=x.device)
        out = _oriented_launch(x, up, dn, w_self, w_up if up is not None else None, w_dn if dn is not None else None, act, H,
                               agg_out=agg)
        ctx.up, ctx.dn, ctx.act = up, dn, act
        ctx.params = (w_self, w_up, w_dn)             # (the parameters themselves: `_grad_target` asks for their .grad)
        ctx.save_for_backward(x, out, agg, w_self, w_up, w_dn)
        return out

    @staticmethod
    def backward(ctx, g):
        x, out, agg, w_self, w_up, w_dn = ctx.saved_tensors
        need = ctx.needs_input_grad
        up, dn, act = ctx.up, ctx.dn, ctx.act
        n, w = x.shape
        H = out.size(1)
        dev = x.device
        g = g.contiguous()
        dz = g if act == _ffi.ACT_ID or n == 0 else _ffi.oriented_dz(g, out, act)
        dx = None
        if need[0]:
            t_up = None if up is None else (up[0].t_src, up[1])       # (perm of a transposed plan: the ORIGINAL entry)
            t_dn = None if dn is None else (dn[0].t_src, dn[1])
            wait_ready([t[0] for t in (t_up, t_dn) if t is not None])
            dx = _oriented_launch(dz, t_up, t_dn, w_self, w_up if up is not None else None, w_dn if dn is not None else None,
                                  _ffi.ACT_ID, w, trans=True)
        grads, descs, in_place, targets = [None, None, None], [], True, []
        for k, (W, X, ldx) in enumerate(((w_self, x, x.stride(0)), (w_up, agg, 2 * w),
                                         (w_dn, None if agg is None else agg[:, w:], 2 * w))):
            if W is None or not need[1 + k]:
                continue
            # inside accumulate_into_grad() (train.TrainStep) the product is added onto the parameter's .grad by the launch
            # itself: no zero fill, no add kernel of autograd's, and the launch may wait for the end of the backward
            dW = _grad_target(ctx.params[k])
            if dW is None:
                dW = grads[k] = torch.zeros(H, w, dtype=torch.float32, device=dev)
                in_place = False
            targets.append(dW)
            if n == 0 or (k == 1 and up is None) or (k == 2 and dn is None):
                continue                                              # (an absent stream: its aggregate is zero)
            descs.append(_ffi.GemmTnDesc(dZ=dz.data_ptr(), X=X.data_ptr(), X2=None, in_scale=None, in_shift=None, in_scale2=None,
                                         in_shift2=None, dW=dW.data_ptr(), db=None, M=n, lddz=H, ldx=ldx, ldx2=0, lddw=dW.stride(0),
                                         N=H, K=w, K2=0, in_relu=0))
        if descs:
            _ffi.gemm_tn(descs, dev, keep=[dz, x, agg, targets], deferrable=ACCUMULATE_INTO_GRAD and in_place)
        return (dx, grads[0], grads[1], grads[2], None, None, None, None)


def oriented_layer_applies(x: Tensor, weights: Sequence[Optional[Tensor]]) -> bool:
    """Does cwn_oriented_layer_f32 take these operands?  float32 on the GPU, rows of 1 .. 128 columns in and out."""
    ws = [t for t in weights if t is not None]
    if not ws or not (isinstance(x, Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2):
        return False
    H, w = ws[0].shape
    return (1 <= w <= _ffi.ORIENTED_MAX_WIDTH and 1 <= H <= _ffi.ORIENTED_MAX_WIDTH and x.size(1) == w
            and all(t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (H, w) for t in ws))


def oriented_layer(x: Tensor, up_adj: Optional[Adjacency], up_orient: Optional[Tensor], dn_adj: Optional[Adjacency],
                   dn_orient: Optional[Tensor], w_self: Optional[Tensor], w_up: Optional[Tensor], w_dn: Optional[Tensor],
                   act='id') -> Tensor:
    """A whole OrientedConv layer (mp/layers.py:441-454 with bias-free Linear maps) in ONE launch:

        out = act(x w_self^T + (A_up o_up x) w_up^T + (A_dn o_dn x) w_dn^T)

    `up_adj` / `dn_adj` are destination-sorted plans over the rows of x (None or without entries: the stream is absent),
    `up_orient` / `dn_orient` one multiplier per original entry (None: 1, OrientedConv(orient=False)), the weights
    `[H, w]` as torch.nn.Linear holds them (None: the map is absent -- EdgeMPNN's upper map).  `act`: 'id', 'relu', 'elu',
    'tanh', 'sigmoid'.  Differentiable w.r.t. x and the weights (the orientations get no gradient, as in the reference's
    data); float32, widths up to 128 (`oriented_layer_applies`) -- anything else is an error, not a fallback."""
    act = _act_code(act)
    x = _f32c(x, 'x')
    w_self, w_up, w_dn = _f32c(w_self, 'w_self'), _f32c(w_up, 'w_up'), _f32c(w_dn, 'w_dn')
    if not oriented_layer_applies(x, (w_self, w_up, w_dn)):
        raise ValueError('oriented_layer takes float32 x [n, w] and weights [H, w] of one shape with 1 <= w, H <= '
                         f'{_ffi.ORIENTED_MAX_WIDTH}, at least one of them given')
    H = next(int(t.size(0)) for t in (w_self, w_up, w_dn) if t is not None)
    n = x.size(0)
    streams = []
    for adj, orient, W in ((up_adj, up_orient, w_up), (dn_adj, dn_orient, w_dn)):
        if adj is None or adj.n_entries == 0 or W is None:
            streams.append(None)
            continue
        if adj.n_dst != n or adj.n_val != n:
            raise ValueError(f'adjacency over {adj.n_val} -> {adj.n_dst} rows, x has {n}')
        if orient is not None:
            orient = _f32c(orient.detach().reshape(-1), 'orient')
            if orient.numel() != adj.n_entries:
                raise ValueError(f'one orientation per entry ({adj.n_entries}), got {orient.numel()}')
        streams.append((adj, orient))
    up, dn = streams
    grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, w_self, w_up, w_dn))
    from .csr import build_many
    todo = [s[0] for s in streams if s is not None and not s[0].built]
    if grad and x.requires_grad:
        for s in streams:
            if s is not None:
                s[0].transposes()
                todo += [a for a in (s[0]._t_src,) if a is not None and not a.built]
    if todo:
        build_many(todo)
    wait_ready([s[0] for s in streams if s is not None])
    if not grad:
        return _oriented_launch(x, up, dn, w_self, w_up if up is not None else None, w_dn if dn is not None else None, act, H)
    return _OrientedLayer.apply(x, w_self, w_up, w_dn, up, dn, act, H)


# ------------------------------------------------------------------------------------------------
# The target-cell head (csrc/cwn_target_head.hip): lin1(x[mask]) of RingSparseCIN, one launch each way
# ------------------------------------------------------------------------------------------------
FUSED_TARGET_HEAD = os.environ.get('CWN_FUSED_TARGET_HEAD') != '0'     # A/B: '0' keeps gather_rows + linear


class _TargetHead(torch.autograd.Function):
    """out[c] = W x[rows[c]] + b: cwn_target_head_f32 forward, cwn_target_head_bwd_f32 backward (dx with every row written,
    dW and db summed in complex order: the same bits on every run, with or without `deterministic()`)."""

    @staticmethod
    def forward(ctx, x, rows, weight, bias, err):
        ctx.save_for_backward(x, rows, weight)
        ctx.has_bias = bias is not None
        return _ffi.target_head(x, rows, weight, bias, err)

    @staticmethod
    def backward(ctx, g):
        x, rows, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        g = _f32c(g, 'grad')
        dx, dW, db = _ffi.target_head_bwd(g, x, rows, weight, need[0], need[2], ctx.has_bias and need[3])
        return dx, None, dW, db, None


def target_head_applies(x: Tensor, target_rows: Tensor, weight: Tensor, bias: Optional[Tensor]) -> bool:
    """Do cwn_target_head_f32 / _bwd_f32 take these operands?  float32 on the GPU, x [N, H] with 16-byte rows, weight
    [K, H], H % 4 == 0, H <= 512, K <= 64, int32 rows."""
    ts = (x, weight) + ((bias,) if bias is not None else ())
    if not all(isinstance(t, Tensor) and t.is_cuda and t.dtype == torch.float32 for t in ts):
        return False
    if not (isinstance(target_rows, Tensor) and target_rows.is_cuda and target_rows.dtype == torch.int32 and target_rows.dim() == 1):
        return False
    if x.dim() != 2 or weight.dim() != 2 or x.size(1) != weight.size(1) or (bias is not None and tuple(bias.shape) != (weight.size(0),)):
        return False
    return (_ffi.target_head_served(int(weight.size(1)), int(weight.size(0))) and x.stride(1) == 1 and is_vec16(x))


def target_head(x: Tensor, target_rows: Tensor, weight: Tensor, bias: Optional[Tensor] = None) -> Tensor:
    """A prediction read off one marked cell per complex -- `lin1(x[mask])` of mp/ring_exp_models.py:61-64 with the marked
    rows given as numbers (ComplexBatch.target_rows: int32, one per complex, ascending), so that nothing synchronises:

        out[c, :] = weight . x[target_rows[c], :] + bias            [len(target_rows), K]

    One launch forward, one backward (csrc/cwn_target_head.hip), differentiable w.r.t. x, weight and bias; under
    `_ffi.dynamic_rows` (a static batch) the rows past the live number of complexes are left unwritten.  The launch takes
    float32 operands with H % 4 == 0, H <= 512, K <= 64 (`target_head_applies`); float64, other widths or class counts and
    CWN_FUSED_TARGET_HEAD=0 (`ops.FUSED_TARGET_HEAD = False`) take the former form -- gather_rows on the same rows, then
    linear -- which is capturable too.  A row outside x raises IndexError (at the model's one check, or at the next
    csr.check_errors under capture)."""
    _ffi.require_gpu(x, 'x')
    _ffi.require_gpu(target_rows, 'target_rows')
    if target_rows.dtype not in (torch.int32, torch.long) or target_rows.dim() != 1:
        raise TypeError('target_rows: a vector of int32 (or int64) row numbers')
    if FUSED_TARGET_HEAD and target_rows.dtype == torch.int32:
        xc = x if x.dim() != 2 or x.stride(1) == 1 else x.contiguous()
        wc = weight.contiguous()
        if target_head_applies(xc, target_rows, wc, bias):
            from .csr import _err_flag, VALIDATE_INDICES, check_errors
            rows = target_rows.contiguous()
            bc = None if bias is None else bias.contiguous()
            err = _err_flag(x.device)
            if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (xc, wc, bc)):
                out = _TargetHead.apply(xc, rows, wc, bc, err)
            else:
                out = _ffi.target_head(xc, rows, wc, bc, err)
            if VALIDATE_INDICES and not torch.cuda.is_current_stream_capturing():
                check_errors(x.device)
            return out
    idx = target_rows.to(torch.long)           # (a launch of its own, inside a capture too: a static slot's rows change under it)
    return torch.nn.functional.linear(gather_rows(x, idx), weight, bias)


# ------------------------------------------------------------------------------------------------
# The edge-flow readout head (csrc/cwn_flow_head.hip): |x| -> readout per cochain -> lin1 -> ReLU -> lin2 of EdgeOrient /
# EdgeMPNN, two launches forward, two backward (+ the weight gradients through cwn_gemm_tn_f32)
# ------------------------------------------------------------------------------------------------
# an operand of cwn_flow_head_f32 / _bwd_f32
_FLOW_ROWS = dict(dtypes=(torch.float32,), what='flow_head: ', hint='cwn_flow_head_f32 computes in fp32 only (float64 runs through '
                  'ops.aggregate and the torch modules: the generic route of models.EdgeOrient / EdgeMPNN)')


def _flow_shapes_ok(x: Tensor, ptr_dev: Tensor, w1: Tensor, b1, w2: Tensor, b2) -> bool:
    if x.dim() != 2 or w1.dim() != 2 or w2.dim() != 2 or ptr_dev.dim() != 1 or ptr_dev.numel() < 1:
        return False
    (H, K), O = w1.shape, int(w2.size(0))
    return (1 <= K <= _ffi.FLOW_HEAD_MAX_WIDTH and 1 <= H <= _ffi.FLOW_HEAD_MAX_WIDTH and 1 <= O <= _ffi.FLOW_HEAD_MAX_OUT
            and x.size(1) == K and w2.size(1) == H and (b1 is None or tuple(b1.shape) == (H,))
            and (b2 is None or tuple(b2.shape) == (O,)))


def flow_head_applies(x, ptr_dev, lin1_w, lin1_b, lin2_w, lin2_b) -> bool:
    """Do cwn_flow_head_f32 / _bwd_f32 take these operands?  float32 on the GPU, x [N, K] with contiguous rows (a row stride
    is allowed), lin1_w [H, K] and lin2_w [O, H] contiguous, the biases [H] / [O] or None, 1 <= K, H <= 128, 1 <= O <= 64,
    ptr_dev a contiguous int64 vector on the GPU, and no `_ffi.dynamic_rows` in force (the launches take host row counts)."""
    ts = [x, lin1_w, lin2_w] + [b for b in (lin1_b, lin2_b) if b is not None]
    if _ffi.DYN_ROWS or not all(isinstance(t, Tensor) and t.is_cuda and t.dtype == torch.float32 for t in ts):
        return False
    if not (isinstance(ptr_dev, Tensor) and ptr_dev.is_cuda and ptr_dev.dtype == torch.long and ptr_dev.is_contiguous()):
        return False
    if not (_rows_contiguous(x, 2) and lin1_w.is_contiguous() and lin2_w.is_contiguous()
            and all(b is None or b.is_contiguous() for b in (lin1_b, lin2_b))):
        return False
    return _flow_shapes_ok(x, ptr_dev, lin1_w, lin1_b, lin2_w, lin2_b)


class _FlowHead(torch.autograd.Function):
    """cwn_flow_head_f32 forward (keeping the pooled rows and lin1's pre-activation), cwn_flow_head_bwd_f32 backward: dx
    with every row written, dh; the weight gradients are sums over the cochains, one cwn_gemm_tn_f32 call each way of
    loading (dW1 = dh^T pooled with db1, dW2 = g^T relu(h) with db2)."""

    @staticmethod
    def forward(ctx, x, ptr_dev, w1, b1, w2, b2, take_abs, mean):
        out, pooled, h = _ffi.flow_head(x, ptr_dev, w1, b1, w2, b2, take_abs, mean, keep=True)
        ctx.save_for_backward(x, ptr_dev, w1, w2, pooled, h)
        ctx.flags = (take_abs, mean, b1 is not None, b2 is not None)
        return out

    @staticmethod
    def backward(ctx, g):
        x, ptr_dev, w1, w2, pooled, h = ctx.saved_tensors
        take_abs, mean, has_b1, has_b2 = ctx.flags
        need = ctx.needs_input_grad
        g = _f32c(g, 'grad')
        dev = x.device
        Cn, (H, K), O = int(g.size(0)), w1.shape, int(w2.size(0))
        dx, dh = _ffi.flow_head_bwd(g, h, x, ptr_dev, w1, w2, take_abs, mean, need[0])
        grads = {}
        descs = []
        for name, wanted, b_wanted, dZ, X, N_, K_, relu in (('1', need[2], has_b1 and need[3], dh, pooled, H, K, 0),
                                                           ('2', need[4], has_b2 and need[5], g, h, O, H, 1)):
            if not (wanted or b_wanted):
                continue
            dW = torch.zeros(N_, K_, dtype=torch.float32, device=dev)
            db = torch.zeros(N_, dtype=torch.float32, device=dev) if b_wanted else None
            grads['w' + name], grads['b' + name] = (dW if wanted else None), db
            if Cn:
                descs.append(_ffi.GemmTnDesc(dZ=dZ.data_ptr(), X=X.data_ptr(), X2=None, in_scale=None, in_shift=None, in_scale2=None,
                                             in_shift2=None, dW=dW.data_ptr(), db=_ffi.ptr(db), M=Cn, lddz=N_, ldx=K_, ldx2=0,
                                             lddw=K_, N=N_, K=K_, K2=0, in_relu=relu))
        if descs:
            _ffi._flush_descs(descs, dev)
        return (dx, None, grads.get('w1'), grads.get('b1'), grads.get('w2'), grads.get('b2'), None, None)


def flow_head(x: Tensor, ptr_dev: Tensor, lin1_w: Tensor, lin1_b: Optional[Tensor], lin2_w: Tensor, lin2_b: Optional[Tensor], *,
              abs: bool = True, mean: bool = False, n_cochains: Optional[int] = None) -> Tensor:
    """The head of EdgeOrient / EdgeMPNN (mp/models.py:531-545) on the device, float32:

        pooled[c, :] = sum over the rows ptr[c] .. ptr[c + 1] - 1 of f(x[r, :])      f = |.| (`abs`) or identity;
                                                                                     / max(rows, 1) with `mean`
        out[c, :]    = lin2_w relu(lin1_w pooled[c, :] + lin1_b) + lin2_b            [C, O]

    `ptr_dev`: the collate's `ptr` as an int64 vector of C + 1 entries ON THE DEVICE (packed.PackedCochains.collate's
    `ptr_dev`): ascending from 0 to the rows of x -- nothing is read back to check it; the kernels clamp what lies outside.
    `n_cochains`, when given, is checked against its length.  Two launches forward, two backward, no atomics: a cochain's
    prediction has the same bits alone, anywhere in any batch and on every run.  Differentiable w.r.t. x and the four
    parameters (d|x|/dx = sgn(x), 0 at 0, as torch).  float32 on the GPU with 1 <= K, H <= 128, 1 <= O <= 64
    (`flow_head_applies`): another dtype or device is a TypeError that names it, another shape a ValueError -- never a
    fallback."""
    x = _rows_operand(x, 'x', 2, **_FLOW_ROWS)
    w1, w2 = _rows_operand(lin1_w, 'lin1_w', 2, **_FLOW_ROWS), _rows_operand(lin2_w, 'lin2_w', 2, **_FLOW_ROWS)
    b1, b2 = _rows_operand(lin1_b, 'lin1_b', 1, **_FLOW_ROWS), _rows_operand(lin2_b, 'lin2_b', 1, **_FLOW_ROWS)
    if x is None or w1 is None or w2 is None:
        raise TypeError('flow_head: x, lin1_w and lin2_w are required')
    for name, W in (('lin1_w', w1), ('lin2_w', w2)):
        if not W.is_contiguous():             # (a row-strided view: the launches take the weights as torch.nn.Linear holds them)
            raise TypeError(f'flow_head: {name} must be a contiguous 2-D float32 tensor (shape {tuple(W.shape)}, strides '
                            f'{tuple(W.stride())})')
    if not isinstance(ptr_dev, Tensor) or ptr_dev.dtype != torch.long or not ptr_dev.is_cuda:
        got = f'{ptr_dev.dtype} on {ptr_dev.device}' if isinstance(ptr_dev, Tensor) else type(ptr_dev).__name__
        raise TypeError(f'flow_head: ptr_dev must be an int64 tensor on the GPU (got {got})')
    if ptr_dev.dim() != 1 or ptr_dev.numel() < 1 or (n_cochains is not None and ptr_dev.numel() != int(n_cochains) + 1):
        want = 'C + 1 >= 1' if n_cochains is None else f'{int(n_cochains) + 1}'
        raise ValueError(f'flow_head: ptr_dev holds C + 1 row offsets ({want} entries), got shape {tuple(ptr_dev.shape)}')
    if _ffi.DYN_ROWS:
        raise RuntimeError('flow_head takes host row counts: it does not run under _ffi.dynamic_rows (a static batch)')
    ptr_dev = ptr_dev.contiguous()
    if not _flow_shapes_ok(x, ptr_dev, w1, b1, w2, b2):
        raise ValueError(f'flow_head takes x [N, K], lin1_w [H, K], lin2_w [O, H] with 1 <= K, H <= {_ffi.FLOW_HEAD_MAX_WIDTH}, '
                         f'1 <= O <= {_ffi.FLOW_HEAD_MAX_OUT} and biases [H] / [O]: x {tuple(x.shape)}, lin1_w {tuple(w1.shape)}, '
                         f'lin2_w {tuple(w2.shape)}, lin1_b {None if b1 is None else tuple(b1.shape)}, '
                         f'lin2_b {None if b2 is None else tuple(b2.shape)}')
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, w1, b1, w2, b2)):
        return _FlowHead.apply(x, ptr_dev, w1, b1, w2, b2, bool(abs), bool(mean))
    return _ffi.flow_head(x, ptr_dev, w1, b1, w2, b2, bool(abs), bool(mean), keep=False)[0]


class _FlowHeadCounted(torch.autograd.Function):
    """_FlowHead under a capacity: cwn_flow_head_dev_f32 / cwn_flow_head_bwd_dev_f32 with the live counts on the device; dW / db
    through cwn_gemm_tn_f32 over the capacity rows with m_dev = the live cochains.  Rows of dx beyond the live rows are unwritten."""

    @staticmethod
    def forward(ctx, x, ptr_dev, n_dev, c_dev, w1, b1, w2, b2, take_abs, mean):
        out, pooled, h = _ffi.flow_head_counted(x, ptr_dev, n_dev, c_dev, w1, b1, w2, b2, take_abs, mean, keep=True)
        ctx.save_for_backward(x, ptr_dev, c_dev, w1, w2, pooled, h)
        ctx.n_dev = n_dev
        ctx.params = {'w1': w1, 'b1': b1, 'w2': w2, 'b2': b2}
        ctx.flags = (take_abs, mean, b1 is not None, b2 is not None)
        return out

    @staticmethod
    def backward(ctx, g):
        x, ptr_dev, c_dev, w1, w2, pooled, h = ctx.saved_tensors
        take_abs, mean, has_b1, has_b2 = ctx.flags
        need = ctx.needs_input_grad
        g = _f32c(g, 'grad')
        dev = x.device
        Cn, (H, K), O = int(g.size(0)), w1.shape, int(w2.size(0))
        dx = torch.empty_like(x, memory_format=torch.contiguous_format) if need[0] else None
        dh = _ffi.flow_head_counted_bwd(g, h, x, ptr_dev, ctx.n_dev, c_dev, w1, w2, take_abs, mean, dx)
        grads, descs, in_place, targets = {}, [], True, []
        for name, wanted, b_wanted, dZ, X, N_, K_, relu in (('1', need[4], has_b1 and need[5], dh, pooled, H, K, 0),
                                                           ('2', need[6], has_b2 and need[7], g, h, O, H, 1)):
            if not (wanted or b_wanted):
                continue
            # (inside accumulate_into_grad() the launch adds onto the parameters' .grad itself, as _OrientedLayer's does)
            dW = _grad_target(ctx.params['w' + name]) if wanted else None
            db = _grad_target(ctx.params['b' + name]) if b_wanted else None
            if dW is None:
                dW = torch.zeros(N_, K_, dtype=torch.float32, device=dev)      # (a throw-away one when only db is wanted)
                grads['w' + name] = dW if wanted else None
                in_place = in_place and not wanted
            if b_wanted and db is None:
                db = grads['b' + name] = torch.zeros(N_, dtype=torch.float32, device=dev)
                in_place = False
            targets += [dW, db]
            descs.append(_ffi.GemmTnDesc(dZ=dZ.data_ptr(), X=X.data_ptr(), X2=None, in_scale=None, in_shift=None, in_scale2=None,
                                         in_shift2=None, dW=dW.data_ptr(), db=_ffi.ptr(db), M=Cn, lddz=N_, ldx=K_, ldx2=0,
                                         lddw=dW.stride(0), N=N_, K=K_, K2=0, in_relu=relu))
        if descs:
            # M = the capacity of THIS head's cochains, its count c_dev: mapped here for a launch that runs now; a deferred one
            # (in-place targets only) runs at the end of the backward under the static batch's own mapping of that capacity
            if ACCUMULATE_INTO_GRAD and in_place and _ffi._tn_queue is not None:
                _ffi.gemm_tn(descs, dev, keep=[dh, pooled, g, h, targets], deferrable=True)
            else:
                with _ffi.dynamic_rows({Cn: c_dev.data_ptr()}):
                    _ffi._flush_descs(descs, dev)
        return (dx, None, None, None, grads.get('w1'), grads.get('b1'), grads.get('w2'), grads.get('b2'), None, None)


def flow_head_counted(x: Tensor, ptr_dev: Tensor, c_dev: Tensor, lin1_w: Tensor, lin1_b: Optional[Tensor], lin2_w: Tensor,
                      lin2_b: Optional[Tensor], *, n_dev: Optional[Tensor] = None, abs: bool = True, mean: bool = False) -> Tensor:
    """`flow_head` for a capacity-sized batch (static_cochains.StaticCochainBatch inside a captured graph): x [N, K] and
    ptr_dev [C + 1] have the CAPACITY's sizes, `c_dev` is a device int64 word with the cochains of the batch, `n_dev` one with
    its rows (None: ptr_dev[*c_dev]).  The same arithmetic and the same bits as `flow_head` over the live rows and cochains;
    out [C, O] with zeros for absent cochains; the backward leaves the rows of dx beyond the live rows unwritten and sums the
    weight gradients over the live cochains.  Same operands and limits as `flow_head`; no fallback."""
    x = _rows_operand(x, 'x', 2, **_FLOW_ROWS)
    w1, w2 = _rows_operand(lin1_w, 'lin1_w', 2, **_FLOW_ROWS), _rows_operand(lin2_w, 'lin2_w', 2, **_FLOW_ROWS)
    b1, b2 = _rows_operand(lin1_b, 'lin1_b', 1, **_FLOW_ROWS), _rows_operand(lin2_b, 'lin2_b', 1, **_FLOW_ROWS)
    if x is None or w1 is None or w2 is None:
        raise TypeError('flow_head_counted: x, lin1_w and lin2_w are required')
    for name, t, n in (('ptr_dev', ptr_dev, None), ('c_dev', c_dev, 1), ('n_dev', n_dev, 1)):
        if t is None and name == 'n_dev':
            continue
        if not isinstance(t, Tensor) or t.dtype != torch.long or not t.is_cuda or not t.is_contiguous() or t.dim() != 1 \
                or (n is not None and t.numel() != n) or t.numel() < 1:
            raise TypeError(f'flow_head_counted: {name} must be a contiguous int64 vector on the GPU'
                            + (' of one element' if n else ' of C + 1 >= 1 entries'))
    if not (w1.is_contiguous() and w2.is_contiguous()) or not _flow_shapes_ok(x, ptr_dev, w1, b1, w2, b2):
        raise ValueError(f'flow_head_counted takes x [N, K], contiguous lin1_w [H, K], lin2_w [O, H] with 1 <= K, H <= '
                         f'{_ffi.FLOW_HEAD_MAX_WIDTH}, 1 <= O <= {_ffi.FLOW_HEAD_MAX_OUT} and biases [H] / [O]: x {tuple(x.shape)}, '
                         f'lin1_w {tuple(w1.shape)}, lin2_w {tuple(w2.shape)}')
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, w1, b1, w2, b2)):
        return _FlowHeadCounted.apply(x, ptr_dev, n_dev, c_dev, w1, b1, w2, b2, bool(abs), bool(mean))
    return _ffi.flow_head_counted(x, ptr_dev, n_dev, c_dev, w1, b1, w2, b2, bool(abs), bool(mean), keep=False)[0]


# ------------------------------------------------------------------------------------------------
# The float64 dense path (csrc/cwn_dense_f64.hip): the Linear layers of a double model, inference only
# ------------------------------------------------------------------------------------------------
ACT_CODES = ACTS = {'id': _ffi.ACT_ID, 'relu': _ffi.ACT_RELU, 'elu': _ffi.ACT_ELU, 'tanh': _ffi.ACT_TANH, 'sigmoid': _ffi.ACT_SIGMOID}


def _act_code(act) -> int:
    if act is None:
        return _ffi.ACT_ID
    code = ACT_CODES.get(act, act) if isinstance(act, str) else act
    if not isinstance(code, int) or not _ffi.ACT_ID <= code <= _ffi.ACT_SIGMOID:
        raise ValueError(f'unknown activation {act!r}: one of {sorted(ACT_CODES)} or a CWN_ACT_* code')
    return code


def _rows_contiguous(t: Tensor, dim: int) -> bool:
    """`dim`-D with unit stride along the last axis; a 2-D tensor may be a row-strided view whose rows do not overlap."""
    return t.dim() == dim and (t.numel() == 0 or (t.stride(-1) == 1 and (dim != 2 or is_rowmajor(t))))


def _operand_dtype(t, name: str, dtypes, what: str, hint: str) -> None:
    if not isinstance(t, Tensor) or t.dtype not in dtypes:
        kinds = ' or '.join(str(d)[len('torch.'):] for d in dtypes)
        raise TypeError(f'{what}{name} must be {kinds} (got {getattr(t, "dtype", type(t).__name__)}): {hint}')


def _rows_operand(t, name: str, dim: int, dtypes, what: str = '', hint: str = '', rows_got: bool = False) -> Optional[Tensor]:
    """An operand of the inference kernels that take views: None, or a tensor of one of `dtypes`, on the GPU, rows
    contiguous (a row stride is allowed).  Anything else is a TypeError `what` + `name` + ..., the dtype's with `hint`; an
    op of one dtype names it bare, one of several as the tensor prints it."""
    if t is None:
        return None
    _operand_dtype(t, name, dtypes, what, hint)
    one = len(dtypes) == 1
    kind = str(dtypes[0])[len('torch.'):] if one else t.dtype
    if not t.is_cuda:
        where = f'got {t.dtype} on {t.device}' if one else f'it is on {t.device}'
        raise TypeError(f'{what}{name} must be a {kind} tensor on the GPU ({where})')
    if not _rows_contiguous(t, dim):
        got = f'got {t.dtype}, ' if rows_got else ''
        raise TypeError(f'{what}{name} must be a {dim}-D {kind} tensor with contiguous rows ({got}shape {tuple(t.shape)}, '
                        f'strides {tuple(t.stride())})')
    return t


# an operand of the float64 dense kernels
_F64_ROWS = dict(dtypes=(torch.float64,), rows_got=True,
                 hint='this kernel computes in fp64 only (float32 runs through the MFMA launches: gemm_many, update_mlp)')


def linear_many_f64(items) -> List[Tensor]:
    """[act(x @ weight.T + bias) for (x, weight, bias, act) in items] in float64 from ONE launch (16 products at most per
    launch; a longer list takes more).  x [M, K] and weight [N, K] may be row-strided views -- the two column slices
    W[:, :F], W[:, F:] of a message weight are -- with 1 <= K, N <= 128 and any M >= 0; bias [N] or None; act one of
    'id', 'relu', 'elu', 'tanh', 'sigmoid' (or its CWN_ACT_* code, None = 'id').  Inference only: nothing is recorded
    for autograd.  Each output element is one fma chain over k in ascending order, so a row's result depends on that
    row and the weights alone (include/cwn_hip.h).  Anything but float64 GPU tensors is a TypeError."""
    return _linear_many_f64(items)


def _linear_many_f64(items) -> List[Tensor]:
    """The launcher behind `linear_many_f64`, which callers inside the package use for products that are part of another
    op -- the Y1 / Y2 of an activated coboundary message (layers._torch_products) -- so that the public function's calls
    stay the ones a model's Linear layers make."""
    descs, outs, dev = [], [], None
    for i, (x, w, b, act) in enumerate(items):
        x, w, b = (_rows_operand(t, f'{name}[{i}]', dim, **_F64_ROWS)
                   for t, name, dim in ((x, 'x', 2), (w, 'weight', 2), (b, 'bias', 1)))
        M, K = int(x.size(0)), int(x.size(1))
        N = int(w.size(0))
        if int(w.size(1)) != K or (b is not None and b.numel() != N):
            raise ValueError(f'product {i}: x {tuple(x.shape)}, weight {tuple(w.shape)}, bias {None if b is None else tuple(b.shape)}')
        if not (1 <= K <= _ffi.LINEAR_F64_MAX_WIDTH and 1 <= N <= _ffi.LINEAR_F64_MAX_WIDTH):
            raise ValueError(f'product {i}: widths K = {K}, N = {N} outside [1, {_ffi.LINEAR_F64_MAX_WIDTH}]')
        dev = x.device
        y = torch.empty(M, N, dtype=torch.float64, device=dev)
        outs.append(y)
        descs.append(_ffi.LinearDescF64(X=x.data_ptr(), W=w.data_ptr(), bias=_ffi.ptr(b), Y=y.data_ptr(), M=M, ldx=ld(x),
                                        ldw=ld(w), ldy=N, K=K, N=N, act=_act_code(act)))
    for lo in range(0, len(descs), _ffi.LINEAR_F64_MAX_DESCS):
        part = descs[lo:lo + _ffi.LINEAR_F64_MAX_DESCS]
        _ffi.check(_ffi.lib().cwn_linear_many_f64((_ffi.LinearDescF64 * len(part))(*part), len(part), _ffi.stream_ptr(dev)),
                   'cwn_linear_many_f64')
    return outs


@dataclass
class ChainDim:
    """One dimension of `update_chain_f64`: the two aggregated inputs [n, F] (self terms added), the weights and biases of
    update_up_nn[0], update_up_nn[3], update_boundaries_nn[0], update_boundaries_nn[3], combine_nn[0] in that order, per
    stage a (scale, shift) pair of [H] tensors or (None, None) (layers._fold_norm), and the activation of all five stages.
    `out`: an output buffer [>= n, H] of the caller's (only its first n rows are written), or None."""
    in_up: Tensor
    in_b: Tensor
    weights: Sequence[Tensor]
    biases: Sequence[Optional[Tensor]]
    folds: Sequence[Tuple[Optional[Tensor], Optional[Tensor]]]
    act: object = 'relu'
    out: Optional[Tensor] = None


def _chain_shapes(d: ChainDim, paired: bool = True) -> Optional[Tuple[int, int, int]]:
    """(n, F, H) when the shapes of `d` are those of a SparseCINConv dimension, else None.  `paired`: a stage's scale and
    shift come together or not at all (the float64 launch; the float32 one takes either alone)."""
    ts = [d.in_up, d.in_b] + list(d.weights)
    if len(d.weights) != 5 or len(d.biases) != 5 or len(d.folds) != 5 or not all(isinstance(t, Tensor) and t.dim() == 2 for t in ts):
        return None
    n, F = int(d.in_up.size(0)), int(d.in_up.size(1))
    H = int(d.weights[0].size(0))
    want = [(H, F), (H, H), (H, F), (H, H), (H, 2 * H)]
    if tuple(d.in_b.shape) != (n, F) or [tuple(w.shape) for w in d.weights] != want:
        return None
    vecs = list(d.biases) + [t for f in d.folds for t in f]
    if any(len(f) != 2 for f in d.folds) or any(t is not None and tuple(t.shape) != (H,) for t in vecs):
        return None
    if paired and any((s is None) != (t is None) for s, t in d.folds):
        return None
    if d.out is not None and (d.out.dim() != 2 or d.out.size(0) < n or d.out.size(1) != H):
        return None
    return n, F, H


def update_chain_f64_applies(dims: Sequence[ChainDim]) -> bool:
    """Does cwn_update_chain_f64 take these dimensions?  1 to 4 of them, every tensor float64 on the GPU with contiguous
    rows (the weights contiguous), 1 <= F, H <= 64, the five-stage shapes of a SparseCINConv dimension, a known activation."""
    if not 1 <= len(dims) <= _ffi.CHAIN_F64_MAX_DIMS:
        return False
    for d in dims:
        shp = _chain_shapes(d)
        if shp is None or not (1 <= shp[1] <= _ffi.CHAIN_F64_MAX_WIDTH and 1 <= shp[2] <= _ffi.CHAIN_F64_MAX_WIDTH):
            return False
        ts = [d.in_up, d.in_b, d.out] + list(d.weights) + list(d.biases) + [t for f in d.folds for t in f]
        if not all(t is None or (t.dtype == torch.float64 and t.is_cuda and _rows_contiguous(t, t.dim())) for t in ts):
            return False
        if not all(w.is_contiguous() for w in d.weights):
            return False
        if isinstance(d.act, str) and d.act not in ACT_CODES:
            return False
    return True


def update_chain_f64(dims: Sequence[ChainDim]) -> List[Tensor]:
    """act(aff(combine_nn[0](cat(update_up_nn(in_up), update_boundaries_nn(in_b))))) of every dimension of a SparseCINConv
    layer (mp/layers.py:193-199) in ONE float64 launch -- five Linear layers per dimension with everything between the
    two inputs and the output in LDS and registers (csrc/cwn_dense_f64.hip).  Returns the outputs [n, H] per dimension.
    Inference only; the arithmetic is row-independent (see `linear_many_f64`).  Anything but float64 GPU tensors is a
    TypeError, shapes the launch does not take (`update_chain_f64_applies`) a ValueError."""
    descs, outs, dev = [], [], None
    for i, d in enumerate(dims):
        named = [('in_up', d.in_up, 2), ('in_b', d.in_b, 2)] + [(f'weights[{s}]', w, 2) for s, w in enumerate(d.weights)] + \
                [(f'biases[{s}]', b, 1) for s, b in enumerate(d.biases)] + \
                [(f'folds[{s}]', t, 1) for s, f in enumerate(d.folds) for t in f] + [('out', d.out, 2)]
        for name, t, dim in named:
            _rows_operand(t, f'dims[{i}].{name}', dim, **_F64_ROWS)
    if not update_chain_f64_applies(dims):
        raise ValueError('update_chain_f64: 1 to 4 dimensions of the five-stage shapes [H, F], [H, H], [H, F], [H, H], [H, 2H] '
                         f'with 1 <= F, H <= {_ffi.CHAIN_F64_MAX_WIDTH}, contiguous weights, a known activation')
    for d in dims:
        n, F, H = _chain_shapes(d)
        dev = d.in_up.device
        out = torch.empty(n, H, dtype=torch.float64, device=dev) if d.out is None else d.out[:n]
        outs.append(out)
        D = _ffi.ChainDescF64(in_up=d.in_up.data_ptr(), in_b=d.in_b.data_ptr(), out=out.data_ptr(), n=n, ld_up=ld(d.in_up),
                              ld_b=ld(d.in_b), ld_out=H if d.out is None else ld(d.out, H), F=F, H=H, act=_act_code(d.act))
        for s in range(5):
            D.W[s], D.bias[s] = d.weights[s].data_ptr(), _ffi.ptr(d.biases[s])
            D.scale[s], D.shift[s] = _ffi.ptr(d.folds[s][0]), _ffi.ptr(d.folds[s][1])
        descs.append(D)
    _ffi.check(_ffi.lib().cwn_update_chain_f64((_ffi.ChainDescF64 * len(descs))(*descs), len(descs), _ffi.stream_ptr(dev)),
               'cwn_update_chain_f64')
    return outs


# ------------------------------------------------------------------------------------------------
# The float32 update chain (csrc/cwn_chain_f32.hip): the same networks in float32 at any width up to 128, inference only
# ------------------------------------------------------------------------------------------------
# an operand of the float32 chain kernel
_F32_ROWS = dict(dtypes=(torch.float32,), rows_got=True,
                 hint='this kernel computes in fp32 only (float64 runs through update_chain_f64)')


def _chain_f32_tensors(d: ChainDim) -> list:
    return [d.in_up, d.in_b, d.out] + list(d.weights) + list(d.biases) + [t for f in d.folds for t in f]


def update_chain_f32_applies(dims: Sequence[ChainDim]) -> bool:
    """Does cwn_update_chain_f32 take these dimensions?  1 to 4 of them, every tensor float32 on the GPU with contiguous
    rows (the weights contiguous), 1 <= F, H <= 128, the five-stage shapes of a SparseCINConv dimension, a known activation."""
    if not 1 <= len(dims) <= _ffi.CHAIN_F32_MAX_DIMS:
        return False
    wmax = _ffi.CHAIN_F32_MAX_WIDTH
    for d in dims:
        shp = _chain_shapes(d, paired=False)
        if shp is None or not (1 <= shp[1] <= wmax and 1 <= shp[2] <= wmax):
            return False
        if not all(t is None or (t.dtype == torch.float32 and t.is_cuda and _rows_contiguous(t, t.dim())) for t in _chain_f32_tensors(d)):
            return False
        if not all(w.is_contiguous() for w in d.weights):
            return False
        if isinstance(d.act, str) and d.act not in ACT_CODES:
            return False
    return True


def update_chain_f32(dims: Sequence[ChainDim]) -> List[Tensor]:
    """`update_chain_f64` in float32: act(aff(combine_nn[0](cat(update_up_nn(in_up), update_boundaries_nn(in_b))))) of every
    dimension of a SparseCINConv layer in ONE launch at any widths 1 <= F, H <= 128 and with any of the five activations
    (csrc/cwn_chain_f32.hip: exact-fp32 MFMA, everything between the two inputs and the output in LDS).  Takes the same
    `ChainDim`s -- here a stage's scale and shift may be absent independently -- and returns the outputs [n, H] per
    dimension (`out`, when given, has its first n rows written).  Inference only: nothing is recorded for autograd.  A row's
    result depends on that row and the weights alone.  Inside `_ffi.dynamic_rows` a row count that is a capacity is read
    from the device (include/cwn_hip.h, "Conventions").  ctypes only: the compiled binding does not carry this launch.
    Anything but float32 GPU tensors is a TypeError, shapes the launch does not take (`update_chain_f32_applies`) a
    ValueError."""
    descs, outs, dev = [], [], None
    for i, d in enumerate(dims):
        named = [('in_up', d.in_up, 2), ('in_b', d.in_b, 2)] + [(f'weights[{s}]', w, 2) for s, w in enumerate(d.weights)] + \
                [(f'biases[{s}]', b, 1) for s, b in enumerate(d.biases)] + \
                [(f'folds[{s}]', t, 1) for s, f in enumerate(d.folds) for t in f] + [('out', d.out, 2)]
        for name, t, dim in named:
            _rows_operand(t, f'dims[{i}].{name}', dim, **_F32_ROWS)
    if not update_chain_f32_applies(dims):
        raise ValueError('update_chain_f32: 1 to 4 dimensions of the five-stage shapes [H, F], [H, H], [H, F], [H, H], [H, 2H] '
                         f'with 1 <= F, H <= {_ffi.CHAIN_F32_MAX_WIDTH}, contiguous weights, a known activation')
    for d in dims:
        n, F, H = _chain_shapes(d, paired=False)
        dev = d.in_up.device
        out = torch.empty(n, H, dtype=torch.float32, device=dev) if d.out is None else d.out[:n]
        outs.append(out)
        D = _ffi.ChainDescF32(in_up=d.in_up.data_ptr(), in_b=d.in_b.data_ptr(), out=out.data_ptr(), n=n, ld_up=ld(d.in_up),
                              ld_b=ld(d.in_b), ld_out=H if d.out is None else ld(d.out, H), F=F, H=H, act=_act_code(d.act))
        for s in range(5):
            D.W[s], D.bias[s] = d.weights[s].data_ptr(), _ffi.ptr(d.biases[s])
            D.scale[s], D.shift[s] = _ffi.ptr(d.folds[s][0]), _ffi.ptr(d.folds[s][1])
        descs.append(D)
    _ffi._set_dyn(descs, 'n')
    _ffi.check(_ffi.lib().cwn_update_chain_f32((_ffi.ChainDescF32 * len(descs))(*descs), len(descs), _ffi.stream_ptr(dev)),
               'cwn_update_chain_f32')
    return outs


class ChainLaunch:
    """A prepared cwn_update_chain_f32 call for one layer, as MlpLaunch is for cwn_update_mlp_f32 (an eager forward is bound
    by its host time, and re-reading fifteen Linear layers and their norms per call costs more than the launch): the weights,
    biases, folds and activation of `dims` -- which `update_chain_f32` has taken -- filled in once; `run` fills in the rows
    of this call and launches.  `sources`: every tensor the record was derived from (Linear weights and biases, the
    BatchNorm tensors behind the folds); `current()` is false as soon as one of them was written in place or moved, the
    module tree changed (STRUCT_EPOCH), or a raw-pointer writer ran (STATE_EPOCH)."""

    def __init__(self, dims: Sequence[ChainDim], sources: Sequence[Tensor]):
        self.n = len(dims)
        self.dev = dims[0].in_up.device
        self.arr = (_ffi.ChainDescF32 * self.n)()
        self.widths = []
        self.keep = [(d.weights, d.biases, d.folds) for d in dims]
        for D, d in zip(self.arr, dims):
            _, F, H = _chain_shapes(d, paired=False)
            self.widths.append((F, H))
            D.F, D.H, D.ld_out, D.act = F, H, H, _act_code(d.act)
            for s in range(5):
                D.W[s], D.bias[s] = d.weights[s].data_ptr(), _ffi.ptr(d.biases[s])
                D.scale[s], D.shift[s] = _ffi.ptr(d.folds[s][0]), _ffi.ptr(d.folds[s][1])
        self.marks = _marks(sources)
        self.epochs = (STATE_EPOCH, STRUCT_EPOCH)
        self.fn = _ffi.lib().cwn_update_chain_f32

    def current(self) -> bool:
        return self.epochs == (STATE_EPOCH, STRUCT_EPOCH) and _marks_current(self.marks)

    def run(self, ins: Sequence[Tuple[Tensor, Tensor]]) -> Optional[List[Tensor]]:
        """None: these inputs are not what the launch takes (another width / dtype / device, rows that are not contiguous)
        -- the caller then goes the long way, which says what is wrong."""
        if len(ins) != self.n:
            return None
        outs = []
        for D, (u, b), (F, H) in zip(self.arr, ins, self.widths):
            for x in (u, b):
                if (x.dim() != 2 or x.size(1) != F or x.dtype != torch.float32 or x.device != self.dev or not is_rowmajor(x)):
                    return None
            n = u.size(0)
            if b.size(0) != n:
                return None
            out = torch.empty(n, H, dtype=torch.float32, device=self.dev)
            outs.append(out)
            D.in_up, D.in_b, D.out, D.n = u.data_ptr(), b.data_ptr(), out.data_ptr(), n
            D.ld_up, D.ld_b = ld(u), ld(b)
            D.m_dev = _ffi.dyn(n)
        rc = self.fn(self.arr, self.n, _ffi.stream_ptr(self.dev))
        if rc != 0:
            _ffi.check(rc, 'cwn_update_chain_f32')
        return outs


# ------------------------------------------------------------------------------------------------
# The float32 update branches (csrc/cwn_branches_f32.hip): the three or four update networks and the combine of a CIN++
# layer in float32 at any width up to 128, inference only
# ------------------------------------------------------------------------------------------------
# an operand of the float32 branches kernel
_F32_BRANCH_ROWS = dict(dtypes=(torch.float32,), rows_got=True,
                        hint='this kernel computes in fp32 only (a float64 CIN++ layer keeps the torch modules)')


@dataclass
class BranchDim:
    """One dimension of `update_branches_f32`: the nb = 3 or 4 aggregated inputs [n, F] (self terms added) in the order of
    torch.cat in mp/layers.py:255-260 -- up, down, boundaries, then the co-boundary branch; the weights and biases of the
    2 nb + 1 Linear layers -- branch by branch its two, then combine_nn[0] [H, nb H]; per stage a (scale, shift) pair of [H]
    tensors, either of them None (layers._fold_norm); the activation of all stages.  `out`: an output buffer [>= n, H] of
    the caller's (only its first n rows are written), or None."""
    ins: Sequence[Tensor]
    weights: Sequence[Tensor]
    biases: Sequence[Optional[Tensor]]
    folds: Sequence[Tuple[Optional[Tensor], Optional[Tensor]]]
    act: object = 'relu'
    out: Optional[Tensor] = None


def _branch_shapes(d: BranchDim) -> Optional[Tuple[int, int, int, int]]:
    """(n, F, H, nb) when the shapes of `d` are those of a CINppConv dimension, else None."""
    nb = len(d.ins)
    if not _ffi.BRANCHES_F32_MIN_BRANCHES <= nb <= _ffi.BRANCHES_F32_MAX_BRANCHES:
        return None
    stages = 2 * nb + 1
    ts = list(d.ins) + list(d.weights)
    if (len(d.weights) != stages or len(d.biases) != stages or len(d.folds) != stages
            or not all(isinstance(t, Tensor) and t.dim() == 2 for t in ts)):
        return None
    n, F = int(d.ins[0].size(0)), int(d.ins[0].size(1))
    H = int(d.weights[0].size(0))
    want = [(H, F), (H, H)] * nb + [(H, nb * H)]
    if any(tuple(x.shape) != (n, F) for x in d.ins) or [tuple(w.shape) for w in d.weights] != want:
        return None
    if any(len(f) != 2 for f in d.folds):
        return None
    vecs = list(d.biases) + [t for f in d.folds for t in f]
    if any(t is not None and tuple(t.shape) != (H,) for t in vecs):
        return None
    if d.out is not None and (d.out.dim() != 2 or d.out.size(0) < n or d.out.size(1) != H):
        return None
    return n, F, H, nb


def _branch_tensors(d: BranchDim) -> list:
    return list(d.ins) + [d.out] + list(d.weights) + list(d.biases) + [t for f in d.folds for t in f]


def update_branches_f32_applies(dims: Sequence[BranchDim]) -> bool:
    """Does cwn_update_branches_f32 take these dimensions?  1 to 4 of them, each with 3 or 4 branches, every tensor float32 on
    the GPU with contiguous rows (the weights contiguous), 1 <= F, H <= 128, the shapes of a CINppConv dimension, a known
    activation."""
    if not 1 <= len(dims) <= _ffi.BRANCHES_F32_MAX_DIMS:
        return False
    wmax = _ffi.BRANCHES_F32_MAX_WIDTH
    for d in dims:
        shp = _branch_shapes(d)
        if shp is None or not (1 <= shp[1] <= wmax and 1 <= shp[2] <= wmax):
            return False
        if not all(t is None or (t.dtype == torch.float32 and t.is_cuda and _rows_contiguous(t, t.dim())) for t in _branch_tensors(d)):
            return False
        if not all(w.is_contiguous() for w in d.weights):
            return False
        if isinstance(d.act, str) and d.act not in ACT_CODES:
            return False
    return True


_BRANCH_SHAPES = ('1 to 4 dimensions of 3 or 4 branches with the shapes [H, F], [H, H] per branch and [H, nb H] of the combine, '
                  f'1 <= F, H <= {_ffi.BRANCHES_F32_MAX_WIDTH}, contiguous weights, a known activation')


def _branch_stages(D, d: BranchDim) -> None:
    for s in range(len(d.weights)):
        D.W[s], D.bias[s] = d.weights[s].data_ptr(), _ffi.ptr(d.biases[s])
        D.scale[s], D.shift[s] = _ffi.ptr(d.folds[s][0]), _ffi.ptr(d.folds[s][1])


def update_branches_f32(dims: Sequence[BranchDim]) -> List[Tensor]:
    """act(aff(combine_nn[0](cat(update_up_nn(in_up), update_down_nn(in_down), update_boundaries_nn(in_b)
    [, update_coboundaries_nn(in_cob)])))) of every dimension of a CINppConv layer (mp/layers.py:255-260) in ONE float32
    launch at any widths 1 <= F, H <= 128 and with any of the five activations (csrc/cwn_branches_f32.hip: exact-fp32
    MFMA, the branches one after the other through LDS, the combine one accumulator over them).  Returns the outputs
    [n, H] per dimension (`out`, when given, has its first n rows written).  Inference only: nothing is recorded for
    autograd.  A row's result depends on that row and the weights alone.  Inside `_ffi.dynamic_rows` a row count that is a
    capacity is read from the device (include/cwn_hip.h, "Conventions").  ctypes only: the compiled binding does not carry
    this launch.  Anything but float32 GPU tensors is a TypeError, shapes the launch does not take
    (`update_branches_f32_applies`) a ValueError."""
    descs, outs, dev = [], [], None
    for i, d in enumerate(dims):
        named = [(f'ins[{k}]', x, 2) for k, x in enumerate(d.ins)] + [(f'weights[{s}]', w, 2) for s, w in enumerate(d.weights)] + \
                [(f'biases[{s}]', b, 1) for s, b in enumerate(d.biases)] + \
                [(f'folds[{s}]', t, 1) for s, f in enumerate(d.folds) for t in f] + [('out', d.out, 2)]
        for name, t, dim in named:
            _rows_operand(t, f'dims[{i}].{name}', dim, **_F32_BRANCH_ROWS)
    if not update_branches_f32_applies(dims):
        raise ValueError('update_branches_f32: ' + _BRANCH_SHAPES)
    for d in dims:
        n, F, H, nb = _branch_shapes(d)
        dev = d.ins[0].device
        out = torch.empty(n, H, dtype=torch.float32, device=dev) if d.out is None else d.out[:n]
        outs.append(out)
        D = _ffi.BranchesDescF32(out=out.data_ptr(), n=n, ld_out=H if d.out is None else ld(d.out, H), F=F, H=H,
                                 act=_act_code(d.act), nb=nb)
        for k, x in enumerate(d.ins):
            D.ins[k], D.ld_in[k] = x.data_ptr(), ld(x)
        _branch_stages(D, d)
        descs.append(D)
    _ffi._set_dyn(descs, 'n')
    _ffi.check(_ffi.lib().cwn_update_branches_f32((_ffi.BranchesDescF32 * len(descs))(*descs), len(descs), _ffi.stream_ptr(dev)),
               'cwn_update_branches_f32')
    return outs


class BranchesLaunch:
    """A prepared cwn_update_branches_f32 call for one layer, as ChainLaunch is for cwn_update_chain_f32: the weights, biases,
    folds and activation of `dims` -- which `update_branches_f32` has taken -- filled in once; `run` fills in the rows of
    this call and launches.  `sources`: every tensor the record was derived from (Linear weights and biases, the BatchNorm
    tensors behind the folds); `current()` is false as soon as one of them was written in place or moved, the module tree
    changed (STRUCT_EPOCH), or a raw-pointer writer ran (STATE_EPOCH)."""

    def __init__(self, dims: Sequence[BranchDim], sources: Sequence[Tensor]):
        self.n = len(dims)
        self.dev = dims[0].ins[0].device
        self.arr = (_ffi.BranchesDescF32 * self.n)()
        self.shapes = []
        self.keep = [(d.weights, d.biases, d.folds) for d in dims]
        for D, d in zip(self.arr, dims):
            _, F, H, nb = _branch_shapes(d)
            self.shapes.append((F, H, nb))
            D.F, D.H, D.ld_out, D.act, D.nb = F, H, H, _act_code(d.act), nb
            _branch_stages(D, d)
        self.marks = _marks(sources)
        self.epochs = (STATE_EPOCH, STRUCT_EPOCH)
        self.fn = _ffi.lib().cwn_update_branches_f32

    def current(self) -> bool:
        return self.epochs == (STATE_EPOCH, STRUCT_EPOCH) and _marks_current(self.marks)

    def run(self, ins: Sequence[Sequence[Tensor]]) -> Optional[List[Tensor]]:
        """None: these inputs are not what the launch takes (another branch count / width / dtype / device, rows that are not
        contiguous) -- the caller then goes the long way, which says what is wrong."""
        if len(ins) != self.n:
            return None
        outs = []
        for D, xs, (F, H, nb) in zip(self.arr, ins, self.shapes):
            if len(xs) != nb:
                return None
            n = xs[0].size(0) if xs[0].dim() == 2 else -1
            for k, x in enumerate(xs):
                if (x.dim() != 2 or x.size(0) != n or x.size(1) != F or x.dtype != torch.float32 or x.device != self.dev
                        or not is_rowmajor(x)):
                    return None
                D.ins[k], D.ld_in[k] = x.data_ptr(), ld(x)
            out = torch.empty(n, H, dtype=torch.float32, device=self.dev)
            outs.append(out)
            D.out, D.n = out.data_ptr(), n
            D.m_dev = _ffi.dyn(n)
        rc = self.fn(self.arr, self.n, _ffi.stream_ptr(self.dev))
        if rc != 0:
            _ffi.check(rc, 'cwn_update_branches_f32')
        return outs


# ------------------------------------------------------------------------------------------------
# The message-passing-agnostic baseline (csrc/cwn_agnostic.hip): embed + activate + pool, and the head, inference only
# ------------------------------------------------------------------------------------------------
def _agnostic_dtype(named, what: str) -> torch.dtype:
    """The one dtype of the operands of an `embed_pool` / `agnostic_head` call: float32 or float64, on the GPU, rows
    contiguous (a row stride is allowed).  Anything else is a TypeError that names the dtype."""
    named = [(name, t, dim) for name, t, dim in named if t is not None]
    dtype = None
    for name, t, dim in named:               # every dtype ahead of any device or shape
        _operand_dtype(t, name, _ffi.FLOAT_DTYPES, f'{what}: ', 'the kernels of csrc/cwn_agnostic.hip compute in fp32 or fp64 only')
        if dtype is None:
            dtype = t.dtype
        if t.dtype != dtype:
            raise TypeError(f'{what}: {name} is {t.dtype}, the operands before it {dtype}: all operands of a call share one dtype')
    for name, t, dim in named:
        _rows_operand(t, name, dim, _ffi.FLOAT_DTYPES, f'{what}: ')
    if dtype is None:
        raise ValueError(f'{what}: no operand')
    return dtype


def embed_pool(xs, cell_ptrs, n_complexes: int, weights, biases, act, mean: bool = False) -> List[Tensor]:
    """[pool_c(act(x @ weight.T + bias)) for x, weight, bias in zip(xs, weights, biases)] -> a list of [n_complexes, H]:
    the per-complex sum (mean: the mean, an empty complex gives zeros) of the activated embedding of every dimension from
    ONE launch (8 dimensions at most per launch; a longer list takes more) that writes nothing but the results.
    x [N, K] and weight [H, K] may be row-strided views, 1 <= K <= 128, 1 <= H <= 1024, bias [H] or None; cell_ptrs[i]:
    the collate's `ptr` of that dimension as a device int64 [n_complexes + 1] (`BlockPlan.cell_ptr_device`); act one of
    'id', 'relu', 'elu', 'tanh', 'sigmoid' (or its CWN_ACT_* code, None = 'id').  Inference only: nothing is recorded for
    autograd.  The bits of a complex's row depend on its own rows in order and the weights alone (include/cwn_hip.h).
    All operands are float32 or all float64, on the GPU: anything else is a TypeError that names the dtype."""
    if not (len(xs) == len(cell_ptrs) == len(weights) == len(biases)) or not xs:
        raise ValueError(f'embed_pool: {len(xs)} inputs, {len(cell_ptrs)} cell_ptrs, {len(weights)} weights, {len(biases)} biases')
    named = [(f'{n}[{i}]', t, dim) for i in range(len(xs))
             for n, t, dim in (('xs', xs[i], 2), ('weights', weights[i], 2), ('biases', biases[i], 1))]
    dtype = _agnostic_dtype(named, 'embed_pool')
    C_, code = int(n_complexes), _act_code(act)
    descs, outs, dev = [], [], xs[0].device
    for i, (x, ptr, w, b) in enumerate(zip(xs, cell_ptrs, weights, biases)):
        N, K, H = int(x.size(0)), int(x.size(1)), int(w.size(0))
        if int(w.size(1)) != K or (b is not None and b.numel() != H):
            raise ValueError(f'embed_pool {i}: x {tuple(x.shape)}, weight {tuple(w.shape)}, bias {None if b is None else tuple(b.shape)}')
        if not (1 <= K <= _ffi.EMBED_POOL_MAX_K and 1 <= H <= _ffi.AGNOSTIC_MAX_WIDTH):
            raise ValueError(f'embed_pool {i}: K = {K} outside [1, {_ffi.EMBED_POOL_MAX_K}] or H = {H} outside [1, {_ffi.AGNOSTIC_MAX_WIDTH}]')
        if not isinstance(ptr, Tensor) or ptr.dtype != torch.int64 or ptr.device != dev or ptr.numel() != C_ + 1 \
                or not ptr.is_contiguous():
            raise ValueError(f'embed_pool {i}: cell_ptr must be a contiguous int64 [{C_ + 1}] on {dev}')
        out = torch.empty(C_, H, dtype=dtype, device=dev)
        outs.append(out)
        descs.append(_ffi.EmbedPoolDesc(x=x.data_ptr() if N else None, cell_ptr=ptr.data_ptr(), W=w.data_ptr(), bias=_ffi.ptr(b),
                                        out=out.data_ptr(), N=N, C=C_, ldx=ld(x), ldw=ld(w), ldo=H, K=K, H=H, act=code,
                                        mean=int(bool(mean))))
    fn, name = _ffi.typed_entry('embed_pool', dtype)
    for lo in range(0, len(descs), _ffi.MAX_DESCS):
        part = descs[lo:lo + _ffi.MAX_DESCS]
        _ffi.check(fn((_ffi.EmbedPoolDesc * len(part))(*part), len(part), _ffi.stream_ptr(dev)), name)
    return outs


def agnostic_head(pooled, lin1_w: Tensor, lin1_b: Optional[Tensor], lin2_w: Tensor, lin2_b: Optional[Tensor], act,
                  n_complexes: Optional[int] = None) -> Tensor:
    """sum_d act(pooled[d] @ lin1_w.T + lin1_b) @ lin2_w.T + lin2_b -> [C, O] from ONE launch: the part of
    MessagePassingAgnostic behind the readout.  pooled: 1 to 8 matrices [C, H]; None stands for a matrix of zeros (an
    absent dimension, which still contributes act(lin1_b)) -- with nothing but None, `n_complexes` says C.  lin1_w [H, H],
    lin2_w [O, H], 1 <= H, O <= 1024, the biases or None.  Inference only; a row depends on that complex's rows alone.
    All operands are float32 or all float64, on the GPU: anything else is a TypeError that names the dtype."""
    pooled = list(pooled)
    if not 1 <= len(pooled) <= _ffi.MAX_DESCS:
        raise ValueError(f'agnostic_head: {len(pooled)} pooled matrices (1 to {_ffi.MAX_DESCS})')
    named = [(f'pooled[{d}]', p, 2) for d, p in enumerate(pooled)] + [('lin1_w', lin1_w, 2), ('lin1_b', lin1_b, 1),
                                                                        ('lin2_w', lin2_w, 2), ('lin2_b', lin2_b, 1)]
    if lin1_w is None or lin2_w is None:
        raise ValueError('agnostic_head: lin1_w and lin2_w are required')
    dtype = _agnostic_dtype(named, 'agnostic_head')
    have = [p for p in pooled if p is not None]
    C_ = int(have[0].size(0)) if have else n_complexes
    if C_ is None:
        raise ValueError('agnostic_head: every pooled matrix is None and n_complexes is not given')
    H, O = int(lin1_w.size(0)), int(lin2_w.size(0))
    if tuple(lin1_w.shape) != (H, H) or int(lin2_w.size(1)) != H or any(tuple(p.shape) != (C_, H) for p in have) \
            or (lin1_b is not None and lin1_b.numel() != H) or (lin2_b is not None and lin2_b.numel() != O):
        raise ValueError(f'agnostic_head: pooled {[None if p is None else tuple(p.shape) for p in pooled]}, lin1_w '
                         f'{tuple(lin1_w.shape)}, lin2_w {tuple(lin2_w.shape)}')
    if not (1 <= H <= _ffi.AGNOSTIC_MAX_WIDTH and 1 <= O <= _ffi.AGNOSTIC_MAX_WIDTH):
        raise ValueError(f'agnostic_head: widths H = {H}, O = {O} outside [1, {_ffi.AGNOSTIC_MAX_WIDTH}]')
    dev = lin1_w.device
    out = torch.empty(C_, O, dtype=dtype, device=dev)
    D = _ffi.AgnosticHeadDesc(W1=lin1_w.data_ptr(), b1=_ffi.ptr(lin1_b), W2=lin2_w.data_ptr(), b2=_ffi.ptr(lin2_b),
                              out=out.data_ptr(), C=C_, ldw1=ld(lin1_w), ldw2=ld(lin2_w), ldo=O, D=len(pooled), H=H, O=O,
                              act=_act_code(act))
    for d, p in enumerate(pooled):
        D.P[d], D.ldp[d] = (p.data_ptr() if p is not None and C_ else None), (ld(p) if p is not None else H)
    fn, name = _ffi.typed_entry('agnostic_head', dtype)
    _ffi.check(fn(C.byref(D), _ffi.stream_ptr(dev)), name)
    return out


# ------------------------------------------------------------------------------------------------
# GINConv as one launch (csrc/cwn_gin.hip): the layer of the graph baselines, float32, inference only
# ------------------------------------------------------------------------------------------------
# an operand of cwn_gin_layer_f32
_GIN_ROWS = dict(dtypes=(torch.float32,), what='gin_layer: ', hint='cwn_gin_layer_f32 computes in fp32 only (float64 and training '
                 'run through ops.aggregate and the torch modules: layers.GINConv)')


def gin_layer_applies(x: Tensor, stages) -> bool:
    """Does cwn_gin_layer_f32 take these operands?  `stages`: two (weight, bias, scale, shift) tuples, the two (Linear,
    folded norm) groups of a GINConv's network.  float32 on the GPU, x [n, w] with contiguous rows, weights [H, w] and
    [H, H] contiguous, 1 <= w, H <= 128, the vectors [H] or None."""
    if not (isinstance(x, Tensor) and x.is_cuda and x.dtype == torch.float32 and _rows_contiguous(x, 2)):
        return False
    if len(stages) != 2 or any(len(s) != 4 for s in stages):
        return False
    (W1, _, _, _), (W2, _, _, _) = stages
    if not all(isinstance(W, Tensor) and W.dim() == 2 and W.is_contiguous() for W in (W1, W2)):
        return False
    H, w = int(W1.size(0)), int(W1.size(1))
    if tuple(W2.shape) != (H, H) or x.size(1) != w or not (1 <= w <= _ffi.GIN_MAX_WIDTH and 1 <= H <= _ffi.GIN_MAX_WIDTH):
        return False
    for W, b, sc, sh in stages:
        if not (W.is_cuda and W.dtype == torch.float32):
            return False
        for v in (b, sc, sh):
            if v is not None and not (isinstance(v, Tensor) and v.is_cuda and v.dtype == torch.float32
                                      and tuple(v.shape) == (H,) and v.is_contiguous()):
                return False
    return True


def gin_layer(x: Tensor, adj: Optional[Adjacency], eps, stages, act, act_post='id', out: Optional[Tensor] = None) -> Tensor:
    """A whole GINConv (torch_geometric's definition, `edge_index[0]` the source) in inference as ONE launch:

        s   = A x + (1 + eps) * x          (A: `adj`, a destination-sorted plan over the rows of x; None: no edges)
        h   = act((s W1^T + b1) * scale1 + shift1)
        out = act_post(act((h W2^T + b2) * scale2 + shift2))

    `stages`: [(W1, b1, scale1, shift1), (W2, b2, scale2, shift2)] -- weights as torch.nn.Linear holds them, an eval-mode
    norm folded to a per-column affine (layers._fold_norm), any of bias / scale / shift None.  `eps`: a float32 tensor of
    one element on the device (GINConv's buffer or Parameter: it is read by the kernel, never on the host), None or a
    Python number.  `act` / `act_post`: 'id', 'relu', 'elu', 'tanh', 'sigmoid' or a CWN_ACT_* code.  `out`: a [n, H]
    float32 view to write into -- a column slice of a JumpingKnowledge('cat') buffer, which x may be another slice of as long
    as the two do not overlap; nothing outside it is written.  Inference only: under a recording autograd (an operand that
    requires a gradient while gradients are enabled) this raises instead of detaching.  float32 on the GPU and widths up to
    128 (`gin_layer_applies`); another dtype or device is a TypeError that names it, never a fallback."""
    x, out, d = _gin_descriptor('gin_layer', 'cwn_gin_layer_f32', _GIN_ROWS, 'layers.GINConv', x, eps, stages, act, act_post, out)
    if d is None:
        return out
    _gin_plan(d, 'gin_layer', adj, int(x.size(0)))
    _ffi.gin_layer(d, x.device)
    return out


# an operand of the counted entries
_GIN_COUNTED_ROWS = dict(_GIN_ROWS, what='gin_layer_counted: ', hint='cwn_gin_layer_dev_f32 computes in fp32 only')


def _count_address(op: str, n_dev, device) -> int:
    """`n_dev` of a counted launch as an address: a device int64 tensor of one element on `device`, or the address itself."""
    if isinstance(n_dev, Tensor):
        if n_dev.dtype != torch.int64 or n_dev.numel() != 1 or n_dev.device != device:
            raise TypeError(f'{op}: n_dev is a {str(n_dev.dtype).replace("torch.", "")} tensor of {n_dev.numel()} element(s) on '
                            f'{n_dev.device}: it must be one int64 on {device}')
        return n_dev.data_ptr()
    if isinstance(n_dev, int) and not isinstance(n_dev, bool) and n_dev > 0:
        return n_dev
    raise TypeError(f'{op}: n_dev is {type(n_dev).__name__}: a device int64 tensor of one element, or its address')


def gin_layer_counted(x: Tensor, adj: Optional[Adjacency], eps, stages, act, act_post='id', out: Optional[Tensor] = None, *,
                      n_dev) -> Tensor:
    """`gin_layer` over a CAPACITY-sized x with the rows that exist counted on the device (cwn_gin_layer_dev_f32): the launch a
    static batch takes.  x.size(0) is the capacity; `n_dev`, a device int64 tensor of one element or its address, holds the
    live count, which the kernel clamps to [0, capacity].  Rows of `out` from the count on are left as they are; rows of x
    from the count on, the plan's rowptr behind rowptr[count] and the entries behind it are never read.  A live row has the
    bits `gin_layer` gives it on the operands trimmed to the count.  `adj` is a plan over the capacity whose first
    rowptr[count] entries are the plan of the live rows (a csr-mode slot's plan, rebuilt per fill).  The operand checks,
    inference only, float32 on the GPU, widths 1 .. 128 and the TypeError for anything else are those of `gin_layer`; this op
    runs inside and outside `_ffi.dynamic_rows`."""
    x, out, d = _gin_descriptor('gin_layer_counted', 'cwn_gin_layer_dev_f32', _GIN_COUNTED_ROWS, 'layers.GINConv', x, eps, stages,
                                act, act_post, out, counted=True)
    addr = _count_address('gin_layer_counted', n_dev, x.device)
    if d is None:
        return out
    _gin_plan(d, 'gin_layer_counted', adj, int(x.size(0)))
    _ffi.gin_layer_counted(d, addr, x.device)
    return out


def _gin_descriptor(op: str, entry: str, rows: dict, layer: str, x, eps, stages, act, act_post, out, counted: bool = False):
    """The operand checks that gin_layer and gine_layer share, and the cwn_gin_desc without its plan: (x, out, descriptor);
    the descriptor is None when there is nothing to launch (no rows).  `counted`: the caller is a counted op, which brings its
    own device count and therefore runs under `_ffi.dynamic_rows` too."""
    x = _rows_operand(x, 'x', 2, **rows)
    if len(stages) != 2 or any(len(s) != 4 for s in stages):
        raise ValueError(f'{op}: stages is [(W1, b1, scale1, shift1), (W2, b2, scale2, shift2)]')
    named = []
    for k, (W, b, sc, sh) in enumerate(stages, 1):
        named.append(tuple(_rows_operand(t, f'{name}{k}', dim, **rows)
                           for t, name, dim in ((W, 'W', 2), (b, 'b', 1), (sc, 'scale', 1), (sh, 'shift', 1))))
    if isinstance(eps, Tensor):
        eps = _rows_operand(eps.reshape(-1), 'eps', 1, **rows)
        if eps.numel() != 1:
            raise ValueError(f'{op}: eps holds {eps.numel()} elements, not one')
    elif eps is not None:
        eps = None if float(eps) == 0.0 else torch.full((1,), float(eps), dtype=torch.float32, device=x.device)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in [x, eps] + [t for s in named for t in s]):
        raise RuntimeError(f'{op} is inference only ({entry} has no backward) and an operand requires a gradient '
                           f'while autograd is recording: run it under torch.no_grad(), or use {layer}, whose '
                           'generic route is differentiable')
    if _ffi.DYN_ROWS and not counted:
        raise RuntimeError(f'{op} takes host row counts: it does not run under _ffi.dynamic_rows (a static batch)')
    named = [tuple(None if t is None else t.contiguous() for t in s) for s in named]
    if not gin_layer_applies(x, named):
        raise ValueError(f'{op} takes x [n, w], W1 [H, w], W2 [H, H] with 1 <= w, H <= {_ffi.GIN_MAX_WIDTH} and vectors '
                         f'[H]: x {tuple(x.shape)}, W1 {tuple(named[0][0].shape)}, W2 {tuple(named[1][0].shape)}')
    n, w = int(x.size(0)), int(x.size(1))
    H = int(named[0][0].size(0))
    if out is None:
        out = torch.empty(n, H, dtype=torch.float32, device=x.device)
    else:
        out = _rows_operand(out, 'out', 2, **rows)
        if tuple(out.shape) != (n, H) or out.device != x.device:
            raise ValueError(f'{op}: out is {tuple(out.shape)} on {out.device}, the result {(n, H)} on {x.device}')
    if n == 0:
        return x, out, None
    d = _ffi.GinDesc(x=x.data_ptr(), eps_dev=_ffi.ptr(eps), out=out.data_ptr(), n=n, ldx=ld(x), ldout=ld(out), w=w, H=H,
                     act=_act_code(act), act_post=_act_code(act_post))
    (d.W1, d.b1, d.scale1, d.shift1), (d.W2, d.b2, d.scale2, d.shift2) = [[_ffi.ptr(t) for t in s] for s in named]
    d._keep = (eps, named)             # (what the descriptor points at, alive until the launch is issued)
    return x, out, d


def _gin_plan(d, op: str, adj: Optional[Adjacency], n: int) -> bool:
    """rowptr / col of a built plan over the n rows of x into the descriptor; False where there are no entries."""
    if adj is None or not adj.n_entries:
        return False
    if adj.n_dst != n or adj.n_val != n:
        raise ValueError(f'{op}: adjacency over {adj.n_val} -> {adj.n_dst} rows, x has {n}')
    if not adj.built:
        from .csr import build_many
        build_many([adj])
    wait_ready([adj])
    d.rowptr, d.col = adj.rowptr.data_ptr(), adj.col.data_ptr()
    return True


# an operand of cwn_gine_layer_f32
_GINE_ROWS = dict(dtypes=(torch.float32,), what='gine_layer: ', hint='cwn_gine_layer_f32 computes in fp32 only (float64 and '
                  'training run through ops.aggregate and the torch modules: layers.GINEConv)')


def gine_layer_applies(x: Tensor, edge, stages) -> bool:
    """Does cwn_gine_layer_f32 take these operands?  What `gin_layer_applies` asks of x and the stages, and of `edge` (None: a
    graph without edges): float32 on the GPU, [rows, w] with contiguous rows, as wide as x."""
    if not gin_layer_applies(x, stages):
        return False
    return edge is None or (isinstance(edge, Tensor) and edge.is_cuda and edge.dtype == torch.float32 and edge.device == x.device
                            and _rows_contiguous(edge, 2) and edge.size(1) == x.size(1))


def gine_layer(x: Tensor, adj: Optional[Adjacency], edge: Optional[Tensor], eps, stages, act, act_post='id',
               out: Optional[Tensor] = None, edge_mode: str = 'aux') -> Tensor:
    """A whole GINEConv (torch_geometric 1.6.3's definition, `edge_index[0]` the source) in inference as ONE launch:

        s   = sum_{j -> i} relu(x_j + e_ji) + (1 + eps) * x_i      (`adj`: a destination-sorted plan over the rows of x;
        h   = act((s W1^T + b1) * scale1 + shift1)                   None or without entries: no edges, `edge` is not read)
        out = act_post(act((h W2^T + b2) * scale2 + shift2))

    `edge` holds the edge features, as wide as x, in one of two forms.  edge_mode='aux': one row per edge CELL, read through
    the plan's shared-cell index (`adj.aux`; the src of a cell_mp.IndexedRows -- the [E, w] matrix is never materialised), so
    the plan must have been built with that index and edge.size(0) == adj.n_aux.  edge_mode='perm': one row per entry of the
    index the plan was built from, as a torch_geometric caller hands edge_attr: edge.size(0) == adj.n_entries.  Everything
    else -- `eps`, `stages`, `act`, `act_post`, `out`, inference only, float32 on the GPU, widths up to 128, TypeError and
    never a fallback for another dtype or device -- is as in `gin_layer`."""
    return _gine('gine_layer', 'cwn_gine_layer_f32', _GINE_ROWS, x, adj, edge, eps, stages, act, act_post, out, edge_mode, None)


def gine_layer_counted(x: Tensor, adj: Optional[Adjacency], edge: Optional[Tensor], eps, stages, act, act_post='id',
                       out: Optional[Tensor] = None, edge_mode: str = 'aux', *, n_dev) -> Tensor:
    """`gine_layer` over a CAPACITY-sized x with the rows that exist counted on the device (cwn_gine_layer_dev_f32), as
    `gin_layer_counted` is of `gin_layer`: x.size(0) is the capacity, `n_dev` a device int64 tensor of one element or its
    address.  `edge` is capacity-sized too (edge.size(0) == adj.n_aux, or adj.n_entries with edge_mode='perm'); the rows of it
    that only entries behind rowptr[count] name are never read."""
    if n_dev is None:
        raise TypeError('gine_layer_counted: n_dev is NoneType: a device int64 tensor of one element, or its address')
    return _gine('gine_layer_counted', 'cwn_gine_layer_dev_f32', _GINE_COUNTED_ROWS, x, adj, edge, eps, stages, act, act_post, out,
                 edge_mode, n_dev)


_GINE_COUNTED_ROWS = dict(_GINE_ROWS, what='gine_layer_counted: ', hint='cwn_gine_layer_dev_f32 computes in fp32 only')


def _gine(op: str, entry: str, rows: dict, x, adj, edge, eps, stages, act, act_post, out, edge_mode, n_dev):
    """gine_layer (n_dev None) and gine_layer_counted: one body."""
    if edge_mode not in ('aux', 'perm'):
        raise ValueError(f"{op}: edge_mode {edge_mode!r}: 'aux' or 'perm'")
    edge = _rows_operand(edge, 'edge', 2, **rows)
    x, out, d = _gin_descriptor(op, entry, rows, 'layers.GINEConv', x, eps, stages, act, act_post, out,
                                counted=n_dev is not None)
    has_edges = adj is not None and adj.n_entries > 0
    if has_edges:
        if edge is None:
            raise ValueError(f'{op}: the adjacency has entries and edge is None')
        if torch.is_grad_enabled() and edge.requires_grad:
            raise RuntimeError(f'{op} is inference only ({entry} has no backward) and edge requires a gradient '
                               'while autograd is recording: run it under torch.no_grad(), or use layers.GINEConv, whose '
                               'generic route is differentiable')
        if edge.size(1) != x.size(1) or edge.device != x.device:
            raise ValueError(f'{op}: edge is {tuple(edge.shape)} on {edge.device}: its width must be that of x '
                             f'{tuple(x.shape)} on {x.device} (another width runs through layers.GINEConv\'s generic route)')
        if edge_mode == 'aux':
            if adj.aux is None:
                raise ValueError(f"{op}: edge_mode='aux' needs an adjacency built with a shared-cell index (aux_index)")
            if edge.size(0) != adj.n_aux:
                raise ValueError(f"{op}: edge_mode='aux': edge has {edge.size(0)} rows, the plan's shared cells are {adj.n_aux}")
        elif edge.size(0) != adj.n_entries:
            raise ValueError(f"{op}: edge_mode='perm': edge has {edge.size(0)} rows, the plan has {adj.n_entries} entries")
    addr = None if n_dev is None else _count_address(op, n_dev, x.device)
    if d is None:
        return out
    D = _ffi.GineDesc(g=d)
    if _gin_plan(D.g, op, adj, int(x.size(0))):
        D.e, D.lde, D.n_e = edge.data_ptr(), ld(edge), int(edge.size(0))
        D.eidx = (adj.aux if edge_mode == 'aux' else adj.perm).data_ptr()
    if addr is None:
        _ffi.gine_layer(D, x.device)
    else:
        _ffi.gine_layer_counted(D, addr, x.device)
    return out


# ------------------------------------------------------------------------------------------------
# gemm_many + aggregate_many of one propagate step as ONE autograd node
# ------------------------------------------------------------------------------------------------
FUSED_PROPAGATE_NODE = os.environ.get('CWN_FUSED_PROPAGATE_NODE') != '0'     # A/B: '0' keeps the two nodes


class _GemmAggregate(torch.autograd.Function):
    """The message products and the aggregation of a SparseCINConv layer (SparseCINConv.propagate_all, training) behind one
    node.  As two nodes (_GemmMany, _AggregateMany) every cell-feature matrix received its gradient in pieces -- from the
    aggregation (self terms, boundary gather) and from each product it entered -- and the autograd engine added the
    pieces with one framework kernel per piece: 16 add kernels per ZINC training step.  Here the aggregation's backward
    writes its piece first and a transposed-weight GEMM adds its piece onto it (CWN_GEMM_ADD_OUT, one product per
    matrix; x_1, which enters two products, still gets one framework add): 4 add kernels per step instead of 16.
    tensors = 4 per GEMM (X, X2, W, bias) then 4 per stream (A, B, self_x, eps); `links[(k, slot)]` = the GEMM whose
    output is stream k's A (slot 0) or B (slot 1) -- those tensor slots hold None.  `ys` may be a _Precomputed: the
    products AND the outputs already exist (the training forward through the blocked layer kernel)."""

    @staticmethod
    def forward(ctx, gemms, streams, links, ys, device, *tensors):
        links = dict(links)           # ((stream, slot), gemm) pairs: a tuple, not a dict (the profiler's argument recorder)
        ng = len(gemms)
        st_tensors = list(tensors[4 * ng:])
        for (k, slot), gi in links.items():
            st_tensors[4 * k + slot] = ys[gi]
        pre = getattr(ys, 'outs', None)          # the blocked layer kernel has already produced the outputs (and ys)
        outs = list(pre) if pre is not None else run_aggregate(_AggregateMany.specs_of(streams, st_tensors), device)
        ctx.gemms, ctx.streams, ctx.links, ctx.device, ctx.ng = gemms, streams, links, device, ng
        ctx.blocked = getattr(ys, 'blocked', None)       # (dims, table, where each stored product lives): the forward ran blocked
        keep = [o for o, st in zip(outs, streams) if st.reduce == 'max']
        ctx.n_in = len(tensors)
        ctx.save_for_backward(*tensors, *ys, *keep)
        return tuple(outs)

    _blocked_backward = staticmethod(lambda *a: _blocked_backward_impl(*a))

    @staticmethod
    def backward(ctx, *gs):
        ng, links = ctx.ng, ctx.links
        saved = ctx.saved_tensors
        tensors = saved[:ctx.n_in]
        ys = saved[ctx.n_in: ctx.n_in + ng]
        max_outs = list(saved[ctx.n_in + ng:])
        g_tensors, s_tensors = tensors[:4 * ng], list(tensors[4 * ng:])
        needs = list(ctx.needs_input_grad[5:])
        g_needs, s_needs = needs[:4 * ng], needs[4 * ng:]
        g_of = [None] * ng          # gradient of every GEMM output, from the streams it feeds
        for (k, slot), gi in links.items():
            s_tensors[4 * k + slot] = ys[gi]
            s_needs[4 * k + slot] = any(g_needs[4 * gi: 4 * gi + 4])
        blocked = _GemmAggregate._blocked_backward(ctx, gs, ys, g_tensors, g_needs, s_tensors, s_needs)
        if blocked is not None:
            return (None, None, None, None, None) + blocked
        s_grads = _aggregate_backward(ctx.streams, s_tensors, s_needs, gs, max_outs, ctx.device)
        for (k, slot), gi in links.items():
            g = s_grads[4 * k + slot]
            s_grads[4 * k + slot] = None
            if g is not None:
                g_of[gi] = g if g_of[gi] is None else g_of[gi] + g
        # the matrices that already hold a gradient piece take the GEMMs' pieces on top of it
        acc = {}
        for q, t in enumerate(s_tensors):
            if s_grads[q] is not None and t is not None and q % 4 in (0, 2) and (q // 4, q % 4) not in links:
                if s_grads[q].dim() == 2 and s_grads[q].is_contiguous():
                    acc.setdefault(_ident(t), s_grads[q])
        # (two products may enter the same matrix -- x_1 is the first operand of its own dimension's message and the second of
        # the dimension below: the first takes the buffer, the second returns its own matrix and the engine adds it)
        g_grads = _gemm_backward(ctx.gemms, g_tensors, ys, g_needs, g_of, acc=acc)
        return (None, None, None, None, None) + tuple(g_grads) + tuple(s_grads)


def _blocked_backward_impl(ctx, gs, ys, g_tensors, g_needs, s_tensors, s_needs):
    """The backward of a propagate step whose forward ran as the blocked launch, as ONE launch over the same item table
    (layer_backward) + the weight-gradient GEMMs; None = does not apply (the streaming backward runs)."""
    info = ctx.blocked
    if info is None or not BLOCKED_BACKWARD:
        return None
    dims, table, ydims = info[:3]
    bwd_table = info[3] if len(info) > 3 else None
    if BLOCKED_BACKWARD == 2 and bwd_table is None:
        return None                        # some complex is beyond the owner form's workgroup: the streaming backward
    n, ng = len(dims), ctx.ng
    # outputs per dimension: (up, b), or (up, down, b) of a CIN++ layer (LayerDim.want_down: out_down = (1 + eps3) x)
    k_out = 3 if getattr(dims[0], 'want_down', False) else 2
    if len(ctx.streams) != k_out * n or len(gs) != k_out * n:
        return None
    if any(s_needs[4 * k + 3] and s_tensors[4 * k + 3] is not None for k in range(k_out * n)):
        return None                        # trainable eps: its gradient is a reduction the launch does not take
    # transposed packed weight of every dimension with an upper adjacency (packed with the forward's weights)
    wt_of = [None] * n
    for gi, (d, which) in enumerate(ydims):
        if which == 'y1':
            W = ctx.gemms[gi].W
            wt_of[d] = packed_layer_weight_t(W)
            if wt_of[d] is None:
                return None
    ys_of = [[None, None] for _ in range(n)]
    for gi, (d, which) in enumerate(ydims):
        ys_of[d][0 if which == 'y1' else 1] = ys[gi]
    res = layer_backward(dims, table, [tuple(p) for p in ys_of], [(gs[k_out * d], gs[k_out * d + k_out - 1]) for d in range(n)], wt_of,
                         bwd_table=bwd_table if BLOCKED_BACKWARD == 2 else None,
                         fuse_bn=k_out == 2)       # (a CIN++ layer adds its third output's piece onto dx AFTER the launch)
    if res is None:
        return None
    dxs, gys = res
    if k_out == 3:
        # the third output's piece: d out_down / d x = (1 + eps3) -- one fused multiply-add per dimension onto the launch's dx
        # (the scale stays a device scalar: no host read inside a captured step)
        # -- all dimensions in ONE launch (cwn_axpy_eps_f32, ABI 24; the framework's `1 + eps` and addcmul_ per dimension were 24
        # launches of a ZINC CIN++ step)
        todo, keep = [], []
        for d in range(n):
            g_down = gs[3 * d + 1]
            if g_down is None or dxs[d] is None or dxs[d].numel() == 0:
                continue
            e3 = dims[d].eps3
            e3 = None if e3 is None else _f32c(e3.detach(), 'eps3')
            g_down = _f32c(g_down, 'gradient of out_down')
            if not dxs[d].is_contiguous() or dxs[d].numel() % 4 or not aligned16(dxs[d]) or not aligned16(g_down):
                dxs[d].add_(g_down) if e3 is None else dxs[d].addcmul_(g_down, (1.0 + e3).view(1, 1))
                continue
            keep += [g_down, e3, dxs[d]]
            todo.append(_ffi.AxpyDesc(y=dxs[d].data_ptr(), x=g_down.data_ptr(), eps=_ffi.ptr(e3), n=dxs[d].numel()))
        for lo in range(0, len(todo), _ffi.AXPY_MAX_DESCS):
            chunk = todo[lo: lo + _ffi.AXPY_MAX_DESCS]
            _ffi.check(_ffi.lib().cwn_axpy_eps_f32((_ffi.AxpyDesc * len(chunk))(*chunk), len(chunk), _ffi.stream_ptr(keep[-1].device)),
                       'cwn_axpy_eps_f32')
    g_of = [gys[d][0 if which == 'y1' else 1] for (d, which) in ydims]
    # weight (and bias) gradients of the message Linear: gY^T x through the merged weight-gradient launches; dX is done
    needs_w = list(g_needs)
    for k in range(ng):
        needs_w[4 * k] = needs_w[4 * k + 1] = False
    g_grads = _gemm_backward(ctx.gemms, g_tensors, ys, needs_w, g_of)
    s_grads: List[Optional[Tensor]] = [None] * len(s_tensors)
    for d in range(n):
        want = _ident(dims[d].x)
        slots = [q for q, t in enumerate(s_tensors) if t is not None and q % 4 in (0, 2) and s_needs[q] and _ident(t) == want]
        if slots:
            s_grads[slots[0]] = dxs[d]
    return tuple(g_grads) + tuple(s_grads)


class _Precomputed(tuple):
    """The GEMM outputs of a propagate step together with the step's OUTPUTS, both already produced (by the blocked layer
    kernel with CWN_LAYER_STORE_Y): what _GemmAggregate's forward then has left to do is remember them."""
    outs = None
    blocked = None


def gemm_aggregate(gemms: Sequence[Gemm], make_streams, precomputed=None) -> Tuple[List[Stream], List[Tensor]]:
    """ys = gemm_many(gemms); streams = make_streams(ys); outs = aggregate_many(streams) -- with ONE autograd node around
    both when a gradient is wanted (see _GemmAggregate).  Returns (streams, outs).  `precomputed` = (ys, outs): forward
    results that already exist (the training forward through the blocked layer kernel); the node then only records."""
    flat_g: List[Optional[Tensor]] = []
    for gm in gemms:
        flat_g += [gm.X, gm.X2, gm.W, gm.bias]
    device = gemms[0].X.device
    grad = torch.is_grad_enabled()
    if precomputed is None and (not (grad and FUSED_PROPAGATE_NODE) or any(
            gm.in_scale is not None or gm.relu or gm.out_scale is not None for gm in gemms)):
        ys = gemm_many(gemms)
        streams = make_streams(ys)
        return streams, (aggregate_many(streams) if streams else [])
    if precomputed is not None:
        ys = _Precomputed(precomputed[0])
        ys.outs = tuple(precomputed[1])
        ys.blocked = precomputed[2] if len(precomputed) > 2 else None
        for gm in gemms:
            gm.X, gm.W = _rowmajor(gm.X, 'X'), _rowmajor(gm.W, 'W')
    else:
        ys = run_gemm(gemms, device)
    streams = make_streams(ys)
    if not streams:
        return streams, []
    links, flat_s = {}, []
    for k, st in enumerate(streams):
        st.validate()
        row = [st.A, st.B, st.self_x, st.eps]
        for slot in (0, 1):
            for gi, y in enumerate(ys):
                if row[slot] is y:
                    links[(k, slot)] = gi
                    row[slot] = None
        flat_s += row
    if not any(t is not None and t.requires_grad for t in flat_g + flat_s):
        if precomputed is not None:
            return streams, list(precomputed[1])
        for (k, slot), gi in links.items():
            flat_s[4 * k + slot] = ys[gi]
        return streams, _run_streams(_AggregateMany.specs_of(streams, flat_s), device)
    if any(st.act is not None for st in streams):
        raise NotImplementedError(_ACT_NO_GRAD)
    # the adjacency plans and their transposes in one batched build -- unless neither pass will read them: the forward is
    # precomputed (the blocked launch) and the backward is the owner-form launch over its own item table (a backward that
    # falls back to the streaming path after all builds them when it asks for them: csr.Adjacency.t_src / t_aux)
    blocked = getattr(ys, 'blocked', None)
    plans_unused = (precomputed is not None and BLOCKED_BACKWARD == 2 and blocked is not None and len(blocked) > 3
                    and blocked[3] is not None)
    if not plans_unused:
        from .csr import build_many
        todo = [st.adj for st in streams if st.adj is not None and not st.adj.built]
        for st in streams:
            if st.adj is not None and st.ia_mode == 'col':
                st.adj.transposes()
                todo += [a for a in (st.adj._t_src, st.adj._t_aux) if a is not None and not a.built]
        if todo:
            build_many(todo)
    outs = _GemmAggregate.apply(tuple(gemms), tuple(streams), tuple(links.items()), ys if isinstance(ys, _Precomputed) else tuple(ys), device,
                                *flat_g, *flat_s)
    return streams, list(outs)


# ------------------------------------------------------------------------------------------------
# One SparseCIN propagate step of a layer in one launch (csrc/cwn_layer.hip)
# ------------------------------------------------------------------------------------------------
@dataclass
class LayerDim:
    """One cochain dimension of cwn_layer_fused_f32 (cwn_layer_dim in include/cwn_hip.h)."""
    x: Tensor
    up_index: Optional[Tensor] = None       # [2, E] int64
    up_shared: Optional[Tensor] = None      # [E] int64 (shared_coboundaries)
    b_index: Optional[Tensor] = None        # [2, B] int64
    msg_w_packed: Optional[Tensor] = None   # pack_layer_weight(Linear(2F -> F).weight)
    msg_bias: Optional[Tensor] = None
    eps1: Optional[Tensor] = None
    eps2: Optional[Tensor] = None
    # a CIN++ layer (mp/layers.py:243-260, lower stream off): the launch also writes out_down = (1 + eps3) x and returns
    # [out_up, out_down, out_b] per dimension -- the order of torch.cat in :260
    eps3: Optional[Tensor] = None
    want_down: bool = False


# Prepared forms of model state -- packed weights, BatchNorm folded into an affine, prepared launches -- are
# cached on (storage, tensor version).  The library's own training kernels write parameters and running
# statistics through raw pointers (cwn_adam_f32, the BatchNorm-statistics epilogue), also from replayed hipGraphs,
# where no Python runs at all: tensor versions do not see those writes.  Every such writer calls
# state_changed(); the epoch is part of every cache key.  (A caller who replays its own graph of training kernels
# calls it too.)
STATE_EPOCH = 0
# ... and the subset of those writes that touch PARAMETERS (the optimizer: cwn_adam_f32, a replayed training step) -- the
# BatchNorm-statistics epilogue moves STATE_EPOCH inside every training forward, between the packing of a step's weight
# blocks and their use, without touching a weight; the packed blocks of the stage kernels are validated against this one.
WEIGHT_EPOCH = 0


def state_changed() -> None:
    global STATE_EPOCH
    STATE_EPOCH += 1


# Prepared launches (LayerLaunch, MlpLaunch: records derived once from a layer's parameters) are checked per call against the
# tensors they were derived from -- address and version counter, which every in-place write bumps -- and against this counter,
# which moves whenever ANY module, parameter or buffer is (re)registered anywhere in the process (torch's global registration
# hooks): a replaced submodule or parameter object is invisible to the version counters of the old ones.
STRUCT_EPOCH = 0


def _struct_changed(*_args) -> None:
    global STRUCT_EPOCH
    STRUCT_EPOCH += 1


def _install_struct_hooks() -> None:
    from torch.nn.modules import module as _m
    for reg in (_m.register_module_module_registration_hook, _m.register_module_parameter_registration_hook,
                _m.register_module_buffer_registration_hook):
        reg(_struct_changed)


_install_struct_hooks()


def weights_changed() -> None:
    """A raw-pointer writer has changed parameters (FlatAdam.step, every replay of a captured training step)."""
    global WEIGHT_EPOCH
    WEIGHT_EPOCH += 1
    state_changed()


_packed_weights = {}


_pack_token = 0          # bumped by every pack_layer_weights_many call: entries it wrote are "fresh" until the next one
_packed_weights_t = {}   # id(weight) -> (token, weakref, buffer): the TRANSPOSED packs of the latest batch (backward launch)


def pack_layer_weight(weight: Tensor, fresh: bool = False) -> Tensor:
    """The message Linear's weight [F, 2F] in the form cwn_layer_fused_f32 reads (bf16 hi / mid / lo
    planes in MFMA-fragment order, include/cwn_hip.h: cwn_layer_pack_weights_f32): one small launch
    per weight VERSION, cached on (storage, version) -- an optimizer step bumps the version and the
    next forward re-packs.  Weight preparation (like folding BatchNorm into an affine), not per step.
    `fresh` (the training forward, whose weights change between any two calls -- also inside a replayed graph, where
    no version counter moves): only an entry written by the LATEST pack_layer_weights_many call counts as a hit."""
    import weakref
    w = weight.detach()
    key = id(weight)
    ver = (w.data_ptr(), _ffi.tver(weight), STATE_EPOCH, tuple(w.shape), w.device)
    hit = _packed_weights.get(key)
    if hit is not None and hit[1]() is weight:
        if not fresh and hit[0] == ver:
            return hit[2]
        # (the latest batch's entries: the state epoch moves INSIDE a training forward -- every layer's BatchNorm statistics
        # bump it -- without touching the message weights, which only the optimizer writes)
        if fresh and hit[3] == _pack_token and hit[0][:2] == ver[:2] and hit[0][3:] == ver[3:]:
            return hit[2]
    w = _f32c(w, 'weight')
    F = int(w.size(0))
    if w.dim() != 2 or w.size(1) != 2 * F:
        raise ValueError('expected the [F, 2F] weight of Linear(2F -> F)')
    L = _ffi.lib()
    out = torch.empty(int(L.cwn_layer_packed_weight_bytes(F)), dtype=torch.uint8, device=w.device)
    _ffi.check(L.cwn_layer_pack_weights_f32(w.data_ptr(), w.stride(0), F, out.data_ptr(), _ffi.stream_ptr(w.device)),
               'cwn_layer_pack_weights_f32')
    _packed_weights[key] = (ver, weakref.ref(weight, lambda _r, k=key: _packed_weights.pop(k, None)), out, -1)
    return out


def packed_layer_weight_t(weight: Tensor) -> Optional[Tensor]:
    """The transposed pack of `weight` written by the LATEST pack_layer_weights_many(..., transposed=True), or None."""
    hit = _packed_weights_t.get(id(weight))
    if hit is not None and hit[0] == _pack_token and hit[1]() is weight:
        return hit[2]
    return None


def pack_layer_weights_many(weights: Sequence[Tensor], transposed: bool = False) -> None:
    """Pack the message weights of ALL layers of a model in one launch per width (cwn_layer_pack_weights_many_f32) and
    leave them in pack_layer_weight's cache as fresh entries: a training forward calls this once, its layers then find
    their weight packed (8 launches per ZINC step otherwise).  `transposed`: also the form the backward launch multiplies
    with (cwn_layer_pack_weights_t_many_f32; packed_layer_weight_t hands it out)."""
    import weakref
    global _pack_token
    _pack_token += 1
    L = _ffi.lib()
    by_F = {}
    for weight in weights:
        w = weight.detach()
        if w.dim() != 2 or w.size(1) != 2 * w.size(0) or w.size(0) not in (64, 128) or not w.is_cuda or w.dtype != torch.float32 \
                or w.stride(1) != 1:
            continue
        by_F.setdefault(int(w.size(0)), []).append((weight, w))
    for F, ws in by_F.items():
        n = len(ws)
        nbytes = int(L.cwn_layer_packed_weight_bytes(F))
        outs = [torch.empty(nbytes, dtype=torch.uint8, device=w.device) for _, w in ws]
        Wp = (C.c_void_p * n)(*[w.data_ptr() for _, w in ws])
        lds = (C.c_int64 * n)(*[w.stride(0) for _, w in ws])
        Op = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
        outs_t = [torch.empty(nbytes, dtype=torch.uint8, device=w.device) for _, w in ws] if transposed else None
        if transposed:
            Ot = (C.c_void_p * n)(*[o.data_ptr() for o in outs_t])
            _ffi.check(L.cwn_layer_pack_weights_both_many_f32(Wp, lds, F, Op, Ot, n, _ffi.stream_ptr(ws[0][1].device)),
                       'cwn_layer_pack_weights_both_many_f32')
        else:
            _ffi.check(L.cwn_layer_pack_weights_many_f32(Wp, lds, F, Op, n, _ffi.stream_ptr(ws[0][1].device)),
                       'cwn_layer_pack_weights_many_f32')
        for (weight, w), out in zip(ws, outs):
            key = id(weight)
            ver = (w.data_ptr(), _ffi.tver(weight), STATE_EPOCH, tuple(w.shape), w.device)
            _packed_weights[key] = (ver, weakref.ref(weight, lambda _r, k=key: _packed_weights.pop(k, None)), out, _pack_token)
        if transposed:
            for (weight, w), out in zip(ws, outs_t):
                key = id(weight)
                _packed_weights_t[key] = (_pack_token, weakref.ref(weight, lambda _r, k=key: _packed_weights_t.pop(k, None)), out)


_packed_gemm_weights = {}


def pack_gemm_weight(weight: Tensor) -> Optional[Tensor]:
    """A Linear(128 -> 128) weight in the form the bf16-split GEMM reads its stationary operand
    (include/cwn_hip.h: cwn_gemm_pack_weights_f32), cached per weight version like pack_layer_weight;
    None for any other shape (the launch then takes the fp32 weight)."""
    import weakref
    w = weight.detach()
    if w.dim() != 2 or tuple(w.shape) != (128, 128) or not w.is_cuda or w.dtype != torch.float32:
        return None
    key = id(weight)
    ver = (w.data_ptr(), _ffi.tver(weight), STATE_EPOCH, w.device)
    hit = _packed_gemm_weights.get(key)
    if hit is not None and hit[0] == ver and hit[1]() is weight:
        return hit[2]
    w = _rowmajor(w, 'W')
    L = _ffi.lib()
    out = torch.empty(int(L.cwn_gemm_packed_weight_bytes()), dtype=torch.uint8, device=w.device)
    _ffi.check(L.cwn_gemm_pack_weights_f32(w.data_ptr(), w.stride(0), out.data_ptr(), _ffi.stream_ptr(w.device)),
               'cwn_gemm_pack_weights_f32')
    _packed_gemm_weights[key] = (ver, weakref.ref(weight, lambda _r, k=key: _packed_gemm_weights.pop(k, None)), out)
    return out


@dataclass
class MlpDim:
    """One cochain dimension of cwn_update_mlp_f32 (cwn_mlp_dim in include/cwn_hip.h): the two outputs of
    the propagate step, the five Linear layers (order 1u, 2u, 1b, 2b, combine) and their folded norms."""
    x_up: Tensor
    x_b: Tensor
    linears: Sequence[torch.nn.Linear]                         # five modules
    folds: Sequence[tuple]                                     # five (scale, shift) pairs, (None, None) = identity


def update_mlp_applies(dims: Sequence[MlpDim]) -> bool:
    """The fused update / combine launch serves networks whose Linear layers are all 64 or all 128 wide."""
    cap = int(_ffi.lib().cwn_update_mlp_max_rows())
    if any(len(D.linears) != 5 for D in dims):
        return False
    F = mlp_width(dims)
    if F not in (64, 128):
        return False
    for D in dims:
        w_in = int(D.x_up.size(1))           # (narrower than F: the first layer of a model over raw features, cwn_mlp_dim.in_width)
        if D.x_up.size(0) > cap or w_in > F or w_in < 1 or D.x_b.size(1) != w_in:
            return False
        shapes = [tuple(l.weight.shape) for l in D.linears]
        if shapes != [(F, w_in), (F, F), (F, w_in), (F, F), (F, 2 * F)]:
            return False
    return True


def mlp_width(dims: Sequence[MlpDim]) -> int:
    """F of cwn_update_mlp_f32: the width of the second Linear of the upper branch (the inputs may be narrower)."""
    return int(dims[0].linears[1].weight.size(0))


_padded_weights = {}


def _mlp_first_weight(weight: Tensor, F: int) -> Tensor:
    """A first-stage weight [F, w_in] as the [F, F] matrix the launch multiplies: itself, or -- w_in < F -- zero-padded
    (cached per weight version; the input tile's other columns are zeros too)."""
    if weight.size(1) == F:
        return weight
    key = id(weight)
    ver = (weight.data_ptr(), _ffi.tver(weight), STATE_EPOCH, tuple(weight.shape))
    hit = _padded_weights.get(key)
    if hit is not None and hit[0] == ver and hit[1]() is weight:
        return hit[2]
    pad = torch.zeros(F, F, dtype=torch.float32, device=weight.device)
    pad[:, :weight.size(1)] = weight.detach()
    _padded_weights[key] = (ver, weakref.ref(weight, lambda _r, k=key: _padded_weights.pop(k, None)), pad)
    return pad


def _mlp_epilogues(a, D) -> list:
    """The bias / scale / shift pointers of a cwn_mlp_dim / cwn_mlp3_dim record `a`, one per Linear of D; returns the
    tensors behind them (to be kept alive with the record)."""
    keep = []
    for s_, (lin, (sc, sh)) in enumerate(zip(D.linears, D.folds)):
        b = None if lin.bias is None else _f32c(lin.bias, 'bias')
        a.bias[s_], a.scale[s_], a.shift[s_] = _ffi.ptr(b), _ffi.ptr(sc), _ffi.ptr(sh)
        keep += [b, sc, sh]
    return keep


def _mlp_dim_static(a, D: MlpDim, F: int) -> list:
    """The half of a cwn_mlp_dim record that does not depend on the rows of a call: in_width, ldy, the packed weights (the
    first stages' padded to [F, F]) and the epilogues; returns the tensors behind the pointers."""
    w_in = int(D.x_up.size(1))
    a.in_width, a.ldy = (w_in if w_in < F else 0), F
    keep, k = [], 0
    for j, l in enumerate(D.linears):
        w = _mlp_first_weight(l.weight, F) if j in (0, 2) else l.weight
        keep.append(w)
        for pk in pack_mlp_weight(w):               # (the combine weight: its two F-column blocks)
            a.w_packed[k] = pk.data_ptr()
            keep.append(pk)
            k += 1
    return keep + _mlp_epilogues(a, D)


def update_mlp(dims: Sequence[MlpDim]) -> List[Tensor]:
    """mp/layers.py:193-199 for every dimension in ONE launch (csrc/cwn_mlp.hip); inference only."""
    dev = dims[0].x_up.device
    F = mlp_width(dims)
    arr = (_ffi.MlpDim * len(dims))()
    outs, keep = [], []
    for i, D in enumerate(dims):
        rm = _rowmajor if int(D.x_up.size(1)) < F else _rowmajor16     # (narrow inputs are staged element-wise: any window)
        xu, xb = rm(D.x_up, 'x_up'), rm(D.x_b, 'x_b')
        y = torch.empty(xu.size(0), F, dtype=torch.float32, device=dev)
        outs.append(y)
        a = arr[i]
        a.x_up, a.x_b, a.y, a.M = xu.data_ptr(), xb.data_ptr(), y.data_ptr(), xu.size(0)
        a.ldx_up, a.ldx_b, a.m_dev = ld(xu), ld(xb), _ffi.dyn(xu.size(0))
        keep += _mlp_dim_static(a, D, F) + [xu, xb]
    _ffi.check(_ffi.lib().cwn_update_mlp_f32(arr, len(dims), F, _ffi.stream_ptr(dev)), 'cwn_update_mlp_f32')
    return outs


@dataclass
class Mlp3Dim:
    """One cochain dimension of cwn_update_mlp3_f32 (cwn_mlp3_dim in include/cwn_hip.h): the three outputs of a CIN++ layer's
    propagate step (up, down, boundaries), the seven Linear layers in the order (1u, 2u, 1d, 2d, 1b, 2b, combine) and their
    folded norms."""
    xs: Sequence[Tensor]                                       # three [M, F]
    linears: Sequence[torch.nn.Linear]                         # seven modules
    folds: Sequence[tuple]                                     # seven (scale, shift) pairs, (None, None) = identity


def update_mlp3_applies(dims: Sequence[Mlp3Dim]) -> bool:
    cap = int(_ffi.lib().cwn_update_mlp_max_rows())
    if not dims or any(len(D.linears) != 7 or len(D.xs) != 3 or len(D.folds) != 7 for D in dims):
        return False
    F = int(dims[0].linears[1].weight.size(0))
    if F not in (64, 128):
        return False
    for D in dims:
        if any(x.dim() != 2 or x.size(1) != F or x.size(0) != D.xs[0].size(0) or x.size(0) > cap or x.dtype != torch.float32
               or not x.is_cuda for x in D.xs):
            return False
        if [tuple(l.weight.shape) for l in D.linears] != [(F, F)] * 6 + [(F, 3 * F)]:
            return False
    return True


def update_mlp3(dims: Sequence[Mlp3Dim]) -> List[Tensor]:
    """mp/layers.py:255-260 for every dimension in ONE launch (csrc/cwn_mlp3.hip); inference only.  The packed weights are
    cached per weight version (pack_mlp_weight); the descriptor itself is a few microseconds of host time."""
    dev = dims[0].xs[0].device
    F = int(dims[0].linears[1].weight.size(0))
    n = len(dims)
    arr = (_ffi.Mlp3Dim * n)()
    rows = [int(D.xs[0].size(0)) for D in dims]
    buf = torch.empty(sum(rows), F, dtype=torch.float32, device=dev)
    outs = list(buf.split(rows))
    keep, off = [], 0
    for i, D in enumerate(dims):
        a = arr[i]
        for k in range(3):
            x = _rowmajor16(D.xs[k], 'x')
            keep.append(x)
            a.x[k], a.ldx[k] = x.data_ptr(), ld(x, F)
        a.y, a.M, a.ldy = buf.data_ptr() + off * 4 * F, rows[i], F
        a.m_dev = _ffi.dyn(rows[i])
        off += rows[i]
        wc = pack_mlp_weight(D.linears[6].weight)               # the three F-column blocks of the combine weight
        for k in range(3):
            a.w_packed[3 * k] = pack_mlp_weight(D.linears[2 * k].weight)[0].data_ptr()
            a.w_packed[3 * k + 1] = pack_mlp_weight(D.linears[2 * k + 1].weight)[0].data_ptr()
            a.w_packed[3 * k + 2] = wc[k].data_ptr()
        keep += _mlp_epilogues(a, D)
    _ffi.check(_ffi.lib().cwn_update_mlp3_f32(arr, n, F, _ffi.stream_ptr(dev)), 'cwn_update_mlp3_f32')
    return outs


class MlpLaunch:
    """A prepared cwn_update_mlp_f32 call for one layer (round 5: the eager forward spent 3/4 of its host time re-deriving
    this record on every call): packed weights, biases and folded norms of every dimension filled in once; `run` fills in
    the rows of this call and launches.  `sources`: every tensor the record was derived from (Linear weights and biases, the
    BatchNorm tensors behind the folds) -- `current()` is false as soon as one of them was written in place, moved, or the
    module tree changed (STRUCT_EPOCH), or a raw-pointer writer ran (STATE_EPOCH)."""

    def __init__(self, dims: Sequence[MlpDim], sources: Sequence[Tensor]):
        self.n = len(dims)
        self.F = F = mlp_width(dims)
        self.dev = dims[0].x_up.device
        self.arr = (_ffi.MlpDim * self.n)()
        self.keep = []
        self.w_in = [int(D.x_up.size(1)) for D in dims]            # input columns per dimension (< F: cwn_mlp_dim.in_width)
        for i, D in enumerate(dims):
            self.keep += _mlp_dim_static(self.arr[i], D, F)
        self.sources = [t for t in sources if t is not None]
        self.marks = [(t.data_ptr(), _ffi.tver(t)) for t in self.sources]
        self.epochs = (STATE_EPOCH, STRUCT_EPOCH)
        self.cap = int(_ffi.lib().cwn_update_mlp_max_rows())
        self.fn = _ffi.lib().cwn_update_mlp_f32
        from . import _cext
        X = _cext.ext()
        self._c = None if X is None else X.MlpCall(C.addressof(self.arr), C.sizeof(self.arr), self.n, F, self.cap,
                                                   _cext.fn_address(self.fn), self.dev.index, self.sources, *self.epochs)

    def current(self) -> bool:
        if self._c is not None:
            return self._c.current(STATE_EPOCH, STRUCT_EPOCH)
        if self.epochs != (STATE_EPOCH, STRUCT_EPOCH):
            return False
        for t, (p, v) in zip(self.sources, self.marks):
            if _ffi.tver(t) != v or t.data_ptr() != p:
                return False
        return True

    def run(self, xs_up: Sequence[Tensor], xs_b: Sequence[Tensor]) -> Optional[List[Tensor]]:
        """None: these inputs are not what the launch takes (more rows than a launch serves, another width / dtype /
        device) -- the caller then goes the long way, which raises where something is wrong."""
        F, n = self.F, self.n
        if self._c is not None and not _ffi.DYN_ROWS:
            return self._c.run(list(xs_up), list(xs_b))
        if len(xs_up) != n or len(xs_b) != n:
            return None
        rows = []
        for xu, xb, w in zip(xs_up, xs_b, self.w_in):
            M = xu.size(0)
            if (M > self.cap or xb.size(0) != M or xu.dim() != 2 or xb.dim() != 2 or xu.size(1) != w or xb.size(1) != w
                    or xu.dtype != torch.float32 or xb.dtype != torch.float32 or xu.device != self.dev or xb.device != self.dev):
                return None
            rows.append(M)
        buf = torch.empty(sum(rows), F, dtype=torch.float32, device=self.dev)
        outs = buf.split(rows)
        base, off, hold = buf.data_ptr(), 0, []
        for i in range(n):
            xu, xb, M = xs_up[i], xs_b[i], rows[i]          # (dtype, device and shape were checked above)
            xu, xb = (rowmajor(xu), rowmajor(xb)) if self.w_in[i] < F else (rowmajor16(xu, ld(xu)), rowmajor16(xb, ld(xb)))
            hold += [xu, xb]                       # (a contiguous copy lives until the launch is enqueued)
            a = self.arr[i]
            a.x_up, a.x_b, a.y, a.M = xu.data_ptr(), xb.data_ptr(), base + off * 4 * F, M
            a.ldx_up, a.ldx_b = (xu.stride(0), xb.stride(0)) if M > 1 else (self.w_in[i],) * 2      # (inline on the eager path: _window.ld)
            a.m_dev = _ffi.dyn(M)
            off += M
        rc = self.fn(self.arr, n, F, _ffi.stream_ptr(self.dev))
        if rc != 0:
            _ffi.check(rc, 'cwn_update_mlp_f32')
        return list(outs)


_packed_mlp_weights = {}


def pack_mlp_weight(weight: Tensor):
    """An [F, F] weight -- or the F-column blocks of an [F, 2F] / [F, 3F] combine weight -- in the form cwn_update_mlp_f32 /
    cwn_update_mlp3_f32 stream (cwn_update_mlp_pack_weights_f32); a tuple of one to three buffers, cached per weight version."""
    import weakref
    w = weight.detach()
    key = id(weight)
    ver = (w.data_ptr(), _ffi.tver(weight), STATE_EPOCH, tuple(w.shape), w.device)
    hit = _packed_mlp_weights.get(key)
    if hit is not None and hit[0] == ver and hit[1]() is weight:
        return hit[2]
    w = _rowmajor(w, 'W')
    F = int(w.size(0))
    L = _ffi.lib()
    n = int(L.cwn_update_mlp_packed_weight_bytes(F))
    if n == 0 or w.size(1) not in (F, 2 * F, 3 * F):
        raise ValueError('expected an [F, F], [F, 2F] or [F, 3F] weight with F in (64, 128)')
    parts = []
    for c0 in range(0, w.size(1), F):
        out = torch.empty(n, dtype=torch.uint8, device=w.device)
        _ffi.check(L.cwn_update_mlp_pack_weights_f32(w.data_ptr() + 4 * c0, w.stride(0), F, out.data_ptr(),
                                                     _ffi.stream_ptr(w.device)), 'cwn_update_mlp_pack_weights_f32')
        parts.append(out)
    parts = tuple(parts)
    _packed_mlp_weights[key] = (ver, weakref.ref(weight, lambda _r, k=key: _packed_mlp_weights.pop(k, None)), parts)
    return parts


# ---- one stage of the update / combine networks in training mode on the inference kernels' arithmetic (cwn_dense_stage_f32) ----
# The training forward of a layer's dense networks is three grouped launches (stage 1, stage 2, combine), each followed by
# cwn_bn_finalize_f32: batch statistics are a reduction over all rows between any two stages.  STAGE_KERNEL routes them
# to csrc/cwn_stage.hip -- pre-packed bf16-split weights streamed into registers, the tile split once into LDS planes --
# when every product of the launch is F -> F or 2F -> F with F in (64, 128) and its weight block was packed by the
# latest pack_stage_weights_many call (the training forward packs all of a model's blocks in one launch, after the
# optimizer has written them); anything else stays on cwn_gemm_f32.
STAGE_KERNEL = os.environ.get('CWN_STAGE_KERNEL') != '0'
_stage_token = 0
_packed_stage = {}       # (storage address, shape, row stride, col0) -> (token, block, transposed block)


def _stage_key(w: Tensor, col0: int):
    # (by storage, not by object: the backward sees its saved weights re-wrapped)
    return (w.data_ptr(), tuple(w.shape), int(w.stride(0)), int(col0))


def pack_stage_weights_many(weights: Sequence[Tensor], transposed: bool = True, fresh: bool = True) -> None:
    """Pack the [F, F] weights (and the two column halves of the [F, 2F] ones) of all given Linear layers in one launch per
    width (+ one for the transposed blocks the backward stage multiplies with); `packed_stage_block` hands the blocks out
    until the next call.  `fresh=False` (a single layer packing its own blocks next to a model's): the blocks of earlier
    calls stay valid -- each is still guarded by its weight's version and the parameter epoch."""
    global _stage_token
    if fresh:
        _stage_token += 1
        _packed_stage.clear()               # (entries of earlier calls are stale by definition)
    else:
        # (a model made of layers that pack their own blocks never comes through `fresh`: entries -- and the
        #  device buffers they hold -- of layers that have died would pile up)
        for k in [k for k, v in _packed_stage.items() if v[5]() is None]:
            del _packed_stage[k]
    L = _ffi.lib()
    by_F = {}
    for weight in weights:
        w = weight.detach()
        F = int(w.size(0)) if w.dim() == 2 else 0
        if F not in (64, 128) or w.size(1) not in (F, 2 * F, 3 * F, 4 * F) or not w.is_cuda or w.dtype != torch.float32 \
                or w.stride(1) != 1 or not is_vec16(w):
            continue
        for c0 in range(0, int(w.size(1)), F):
            by_F.setdefault(F, []).append((weight, w, c0))
    for F, blocks in by_F.items():
        nbytes = int(L.cwn_update_mlp_packed_weight_bytes(F))
        per = _ffi.STAGE_PACK_MAX // 2 if transposed else _ffi.STAGE_PACK_MAX     # (both forms share a launch's table)
        for lo in range(0, len(blocks), per):
            part = blocks[lo: lo + per]
            n = len(part)
            dev = part[0][1].device
            buf = torch.empty(n * nbytes, dtype=torch.uint8, device=dev)
            outs = [buf[k * nbytes: (k + 1) * nbytes] for k in range(n)]
            Wp = (C.c_void_p * n)(*[w.data_ptr() + 4 * c0 for _, w, c0 in part])
            lds = (C.c_int64 * n)(*[w.stride(0) for _, w, _ in part])
            Op = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
            outs_t = [None] * n
            if transposed:                      # ... and the blocks of the transposed weight (cwn_dense_stage_bwd_f32: dX = dz W)
                buf_t = torch.empty(n * nbytes, dtype=torch.uint8, device=dev)
                outs_t = [buf_t[k * nbytes: (k + 1) * nbytes] for k in range(n)]
                Tp = (C.c_void_p * n)(*[o.data_ptr() for o in outs_t])
                _ffi.check(L.cwn_update_mlp_pack_weights_both_many_f32(Wp, lds, F, Op, Tp, n, _ffi.stream_ptr(dev)),
                           'cwn_update_mlp_pack_weights_both_many_f32')
            else:
                _ffi.check(L.cwn_update_mlp_pack_weights_many_f32(Wp, lds, F, Op, n, _ffi.stream_ptr(dev)),
                           'cwn_update_mlp_pack_weights_many_f32')
            for (weight, w, c0), o, ot in zip(part, outs, outs_t):
                # (a weak reference to the tensor that was packed: an entry whose weight has died -- a layer that is gone, its
                #  storage address handed to a NEW parameter of the same shape -- is not served, ADVICE r3 / round 4's CIN++ tests)
                _packed_stage[_stage_key(w, c0)] = (_stage_token, o, ot, _ffi.tver(weight), WEIGHT_EPOCH, weakref.ref(weight))


# ---- the step arena: the zeroed scratch of a training step ------------------------------------------------------------
# What a step needs ZERO on entry -- the slot sums of every live BatchNorm (cwn_bn_live), the s1 / s2 sums of their backward --
# used to be cleared by launches of their own (cwn_bn_finalize_f32 cleared the backward sums; a live BatchNorm has no such
# launch).  A driver of whole steps (train.TrainStep) brackets each with step_arena(device): ONE fill over the bytes the
# previous steps used, then zeros_scratch() hands out regions of it in call order; outside such a bracket zeros_scratch() is a
# torch.zeros.  A region lives until the NEXT step begins: fine for everything a step's own forward + backward touch, not for a
# graph kept beyond its step (retain_graph into the next step).
_ARENA_MIN = 1 << 22


class _Arena:
    def __init__(self, device):
        self.buf = torch.zeros(_ARENA_MIN, dtype=torch.uint8, device=device)
        self.used = 0             # bytes handed out in the current step
        self.high = 0             # bytes ever handed out: everything behind is still zero
        self.want = 0             # bytes the last step asked for beyond the buffer
        self.active = False
        self.retired = []


_arenas: Dict[torch.device, '_Arena'] = {}


class step_arena:
    """with ops.step_arena(device): ...one training step...
    `flat` (a float32 gradient buffer to zero), `counter` / `active` (an int32 step counter to advance unless *active <= 0):
    done by the SAME launch as the arena's fill (cwn_step_begin)."""

    def __init__(self, device, flat: Optional[Tensor] = None, counter: Optional[Tensor] = None, active: Optional[Tensor] = None):
        self.device = torch.device(device)
        self.flat, self.counter, self.active = flat, counter, active

    def __enter__(self):
        a = _arenas.get(self.device)
        capturing = torch.cuda.is_current_stream_capturing()
        if a is None or (a.want and not capturing):
            size = _ARENA_MIN if a is None else max(2 * a.buf.numel(), 2 * (a.buf.numel() + a.want))
            a = _arenas[self.device] = _Arena(self.device) if a is None else a
            if a.buf.numel() < size:
                a.retired.append(a.buf)          # (captured steps keep replaying into the buffer they were captured with)
                a.buf = torch.zeros(size, dtype=torch.uint8, device=self.device)
                a.high = 0
            a.want = 0
        flat = self.flat
        if flat is not None and (flat.dtype != torch.float32 or not flat.is_contiguous() or not aligned16(flat) or (4 * flat.numel()) % 16):
            flat.zero_()
            flat = None
        global _drop_site
        _drop_site = 0                           # (sites number the applications of ONE step: the step counter tells steps apart --
                                                 #  an eager step and its captured replay then draw the same masks)
        ds = _drop_states.get(self.device)       # (exists once a dropout has been applied on this device: fresh masks per step)
        if a.high or flat is not None or self.counter is not None or ds is not None:
            _ffi.check(_ffi.lib().cwn_step_begin(_ffi.ptr(flat), 0 if flat is None else 4 * flat.numel(), a.buf.data_ptr(),
                                                 (a.high + 15) // 16 * 16, _ffi.ptr(self.counter), _ffi.ptr(self.active),
                                                 _ffi.ptr(ds), _ffi.stream_ptr(self.device)), 'cwn_step_begin')
        a.used, a.active = 0, True
        bn_registry_clear()                      # (entries name tensors of the previous step)
        return self

    def __exit__(self, *exc):
        a = _arenas[self.device]
        a.active = False
        return False


def zeros_scratch(nbytes: int, device) -> Tensor:
    """`nbytes` of zeroed device memory (uint8, 256-B aligned) -- a region of the step arena inside step_arena(), else fresh."""
    a = _arenas.get(torch.device(device))
    n = (int(nbytes) + 255) // 256 * 256
    if a is not None and a.active:
        if a.used + n <= a.buf.numel():
            out = a.buf[a.used: a.used + n]
            a.used += n
            a.high = max(a.high, a.used)
            return out
        a.want += n               # (the next bracket outside a capture grows the buffer)
    return torch.zeros(n, dtype=torch.uint8, device=device)


def packed_stage_block(weight: Tensor, col0: int, transposed: bool = False) -> Optional[Tensor]:
    """The packed block weight[:, col0 : col0 + F] (or the block of the transposed weight) written by the LATEST
    pack_stage_weights_many call, or None."""
    hit = _packed_stage.get(_stage_key(weight, col0)) if weight.dim() == 2 else None
    # (an entry is keyed on the weight's STORAGE -- the backward sees its saved weights re-wrapped -- so it must
    # also prove that nothing has written that storage since: the tensor version (torch optimizers, in-place ops) and the
    # parameter epoch (FlatAdam / a replayed step write through raw pointers).  A miss sends the caller to cwn_gemm_f32.)
    if hit is not None and hit[0] == _stage_token and hit[3] == _ffi.tver(weight) and hit[4] == WEIGHT_EPOCH:
        # ... and that the tensor that was packed is alive AND still owns that storage (a Parameter re-pointed by
        # `.data =` / load_state_dict(assign=True) stays alive while its old storage is recycled for another weight of the
        # same shape and version)
        owner = hit[5]()
        if owner is not None and owner.data_ptr() == weight.data_ptr():
            return hit[2] if transposed else hit[1]
    return None


def run_stage_bwd(entries, device, live=None) -> bool:
    """cwn_dense_stage_bwd_f32 over `entries` = [(dy, bnb, W, dx, dx2)]: dy the gradient of a stage's output, bnb the
    _ffi.GemmBnb extension dense_train prepared for the transposed-weight GEMM (z, dz, the norm's constants and sums), W the
    Linear's weight Parameter, dx (and dx2 for an [F, 2F] weight) the outputs.  False: does not apply, nothing launched.
    `live` (or None): per entry (s_slots, out_bn, out_bn2) -- the slot-sum forms of the BatchNorm backward's reduce
    (include/cwn_hip.h: cwn_bn_bwd_live): a [BN_SLOTS, 2, F] fp32 tensor this stage takes its s1 / s2 from, and the
    _ffi.BnBwdLive records of the stages that receive dx / dx2 as their dy; each may be None."""
    if not STAGE_KERNEL or not entries or len(entries) > _ffi.MAX_DESCS:
        return False
    F = int(entries[0][0].size(1))
    if F not in (64, 128):
        return False
    arr = (_ffi.StageBwdDesc * len(entries))()
    keep = []
    ok_t = lambda t, w: t.dtype == torch.float32 and t.is_cuda and t.dim() == 2 and t.size(1) == w and t.stride(1) == 1 and is_vec16(t)
    for k, ent in enumerate(entries):
        dy, b, W, dx, dx2 = ent[:5]
        c0 = int(ent[5]) if len(ent) > 5 else 0          # (a wider weight: the blocks W[:, c0 : c0 + F (+ F)])
        if b is None or W.dim() != 2 or W.size(0) != F or (W.size(1) != (2 * F if dx2 is not None else F) if len(ent) <= 5
                                                           else W.size(1) < c0 + (2 * F if dx2 is not None else F)):
            return False
        M = int(dy.size(0))
        if M == 0 or not ok_t(dy, F) or not ok_t(dx, F) or (dx2 is not None and not ok_t(dx2, F)) or dx.size(0) != M:
            return False
        w1 = packed_stage_block(W, c0, transposed=True)
        w2 = packed_stage_block(W, c0 + F, transposed=True) if dx2 is not None else None
        if w1 is None or (dx2 is not None and w2 is None):
            return False
        ptrs = [b.scale, b.shift, b.mean, b.rstd, b.s1, b.s2, b.acc1, b.acc2, b.z, b.dz]
        if any(p is not None and p % 16 for p in ptrs) or b.ldz % 4 or (b.dz is not None and b.lddz % 4):
            return False
        arr[k] = _ffi.StageBwdDesc(dy=dy.data_ptr(), z=b.z, dz=b.dz, scale=b.scale, shift=b.shift, mean=b.mean, rstd=b.rstd,
                                   s1=b.s1, s2=b.s2, acc1=b.acc1, acc2=b.acc2, wt_packed=w1.data_ptr(), wt2_packed=_ffi.ptr(w2),
                                   dx=dx.data_ptr(), dx2=_ffi.ptr(dx2), M=M, lddy=ld(dy), ldz=int(b.ldz), lddz=int(b.lddz),
                                   lddx=ld(dx), lddx2=0 if dx2 is None else ld(dx2), relu=int(b.relu), m_dev=_ffi.dyn(M))
        if live is not None:
            sl, o1, o2 = live[k]
            if sl is not None:
                if sl.dtype != torch.float32 or tuple(sl.shape) != (_ffi.BN_SLOTS, 2, F) or not sl.is_contiguous() or b.scale is None:
                    return False
                arr[k].s_slots = sl.data_ptr()
            if o1 is not None:
                arr[k].out_bn = o1
            if o2 is not None:
                if dx2 is None:
                    return False
                arr[k].out_bn2 = o2
        keep += [w1, w2]
    _ffi.check(_ffi.lib().cwn_dense_stage_bwd_f32(arr, len(entries), F, _ffi.stream_ptr(device)), 'cwn_dense_stage_bwd_f32')
    return True


def run_stage(gemms: Sequence['Gemm'], device) -> Optional[List[Tensor]]:
    """The grouped launch `gemms` on cwn_dense_stage_f32, or None when it does not apply (the caller runs cwn_gemm_f32)."""
    if not STAGE_KERNEL or not gemms or len(gemms) > _ffi.MAX_DESCS:
        return None
    F = int(gemms[0].X.size(1))
    if F not in (64, 128):
        return None
    arr = (_ffi.StageDesc * len(gemms))()
    extras = None
    keep, outs = [], []
    for k, g in enumerate(gemms):
        X, X2, W = g.X, g.X2, g.W
        if (g.relu or g.out_scale is not None or g.w_trans or g.bnb is not None or g.add_out or g.out is not None or g.exact
                or g.w_col0 is not None or g.debug):
            return None
        more = list(g.more)
        if more and (X2 is None or len(more) > 2):
            return None
        if W.dim() != 2 or W.size(0) != F or W.size(1) != ((2 + len(more)) * F if X2 is not None else F):
            return None
        for t in [X, X2] + [m[0] for m in more]:
            if t is not None and (t.dtype != torch.float32 or not t.is_cuda or t.dim() != 2 or t.size(1) != F or t.stride(1) != 1
                                  or not is_vec16(t) or t.size(0) != X.size(0)):
                return None
        w1 = packed_stage_block(W, 0)
        w2 = packed_stage_block(W, F) if X2 is not None else None
        wm = [packed_stage_block(W, (2 + j) * F) for j in range(len(more))]
        if w1 is None or (X2 is not None and w2 is None) or any(w is None for w in wm):
            return None
        cons = [g.bias, g.in_scale, g.in_shift, g.in_scale2, g.in_shift2]
        cons = [None if t is None else _f32c(t, 'constant') for t in cons]
        if any(t is not None and (t.numel() != F or not aligned16(t)) for t in cons):
            return None
        cs = g.col_stats
        M = int(X.size(0))
        if cs is not None and (cs.dtype != torch.float64 or tuple(cs.shape) != (2, stat_rows(M), F) or not cs.is_contiguous()):
            return None
        ss = g.stat_slots
        if ss is not None and (cs is not None or ss.dtype != torch.float64 or tuple(ss.shape) != (_ffi.BN_SLOTS, 2, F)
                               or not ss.is_contiguous()):
            return None
        Y = torch.empty(M, F, dtype=torch.float32, device=X.device)
        arr[k] = _ffi.StageDesc(X=X.data_ptr(), X2=_ffi.ptr(X2), w_packed=w1.data_ptr(), w2_packed=_ffi.ptr(w2),
                                bias=_ffi.ptr(cons[0]), in_scale=_ffi.ptr(cons[1]), in_shift=_ffi.ptr(cons[2]),
                                in_scale2=_ffi.ptr(cons[3]), in_shift2=_ffi.ptr(cons[4]), Y=Y.data_ptr(),
                                col_sum=None if cs is None else cs[0].data_ptr(), col_sumsq=None if cs is None else cs[1].data_ptr(),
                                M=M, ldx=ld(X), ldx2=0 if X2 is None else ld(X2), ldy=F, in_relu=int(g.in_relu), m_dev=_ffi.dyn(M),
                                stat_slots=_ffi.ptr(ss))
        if g.in_bn is not None:
            arr[k].in_bn = g.in_bn
        if g.in_bn2 is not None:
            arr[k].in_bn2 = g.in_bn2
        for j, (xm, relu_m, bn_m) in enumerate(more):
            if extras is None:
                extras = (_ffi.StageExtra * (2 * len(gemms)))()
            e = extras[2 * k + j]
            e.X, e.w_packed, e.ldx, e.relu = xm.data_ptr(), wm[j].data_ptr(), ld(xm), int(bool(relu_m))
            if bn_m is not None:
                e.bn = bn_m
        keep += cons + [w1, w2] + wm
        outs.append(Y)
    if extras is not None:
        _ffi.check(_ffi.lib().cwn_dense_stage_ex_f32(arr, extras, len(gemms), F, _ffi.stream_ptr(device)), 'cwn_dense_stage_ex_f32')
    else:
        _ffi.check(_ffi.lib().cwn_dense_stage_f32(arr, len(gemms), F, _ffi.stream_ptr(device)), 'cwn_dense_stage_f32')
    return outs


LINEAR_STATS_MAX_N, LINEAR_STATS_MAX_K = 128, 256      # cwn_linear_stats_f32: N, K + K2


def run_linear_stats(gemms: Sequence['Gemm'], device) -> Optional[List[Tensor]]:
    """The grouped launch `gemms` on cwn_linear_stats_f32 (a Linear stage whose band statistics count the rows that EXIST, at
    any width up to 128), or None when it does not apply and the caller runs cwn_gemm_f32: it takes a launch in which at
    least one product carries a device-side row count together with `col_stats` -- what cwn_gemm_f32 refuses -- and nothing
    needs what this entry point refuses (w_trans, bnb, an output affine or ReLU, add_out, a live BatchNorm record, a third
    K-block, widths beyond its limits).  Outside a static slot no row has a device-side count: None, always."""
    if not gemms or not _ffi.DYN_ROWS or len(gemms) > _ffi.MAX_DESCS:
        return None
    if not any(g.col_stats is not None and _ffi.dyn(g.X.size(0)) is not None for g in gemms):
        return None
    for g in gemms:
        if (g.relu or g.out_scale is not None or g.out_shift is not None or g.w_trans or g.bnb is not None or g.add_out
                or g.stat_slots is not None or g.in_bn is not None or g.in_bn2 is not None or g.more or g.debug
                or g.w_packed is not None):
            return None
        K = int(g.X.size(1)) + (int(g.X2.size(1)) if g.X2 is not None else 0)
        if g.W.dim() != 2 or not (1 <= g.W.size(0) <= LINEAR_STATS_MAX_N) or not (1 <= int(g.X.size(1)) and K <= LINEAR_STATS_MAX_K):
            return None
        cs = g.col_stats
        if cs is not None and (cs.dtype != torch.float64 or tuple(cs.shape) != (2, stat_rows(g.X.size(0)), g.W.size(0))
                               or not cs.is_contiguous()):
            return None
    outs, descs, keep = [], [], []
    for g in gemms:
        g.X, g.W = _rowmajor(g.X, 'X'), _rowmajor(g.W, 'W')
        if g.X2 is not None:
            g.X2 = _rowmajor(g.X2, 'X2')
        cons = {k: (None if getattr(g, k) is None else _f32c(getattr(g, k), k)) for k in ('bias', 'in_scale', 'in_shift', 'in_scale2', 'in_shift2')}
        keep.append(cons)
        X, X2, W = g.X, g.X2, g.W
        M, N, K1 = int(X.size(0)), int(W.size(0)), int(X.size(1))
        K2 = int(X2.size(1)) if X2 is not None else 0
        if g.w_col0 is not None:
            if W.size(1) < g.w_col0 + K1 + K2:
                raise ValueError('w_col0 selects columns of an untransposed weight')
        elif W.size(1) != K1 + K2:
            raise ValueError(f'weight has {W.size(1)} input columns, operands have {K1 + K2}')
        if X2 is not None and X2.size(0) != M:
            raise ValueError('X and X2 must have the same number of rows')
        Y = g.out if g.out is not None else torch.empty(M, N, dtype=torch.float32, device=device)
        outs.append(Y)
        if not Y.numel():
            continue
        cs = g.col_stats
        descs.append(_ffi.GemmDesc(
            X=X.data_ptr(), X2=_ffi.ptr(X2), W=W.data_ptr() + 4 * (g.w_col0 or 0), bias=_ffi.ptr(cons['bias']),
            in_scale=_ffi.ptr(cons['in_scale']), in_shift=_ffi.ptr(cons['in_shift']),
            in_scale2=_ffi.ptr(cons['in_scale2']), in_shift2=_ffi.ptr(cons['in_shift2']),
            col_sum=None if cs is None else cs[0].data_ptr(), col_sumsq=None if cs is None else cs[1].data_ptr(),
            Y=Y.data_ptr(), M=M, ldx=ld(X), ldx2=ld(X2, max(K2, 1)) if X2 is not None else 0, ldw=ld(W), ldy=ld(Y, N),
            N=N, K=K1, K2=K2, relu=0, in_relu=int(g.in_relu) & (3 if X2 is not None else 1), w_trans=0, bnb=None,
            m_dev=_ffi.dyn(M), flags=_ffi.GEMM_EXACT))
    if descs:
        _ffi.linear_stats(descs, device)
    return outs


def stage_bwd_takes(W: Tensor, F: int, blocks: int = 1) -> bool:
    """Would run_stage_bwd take the input-gradient product of a stage of width F whose weight is `blocks` [F, F] blocks side
    by side?  (The lazy BatchNorm-backward form -- cwn_gemm_bnb -- has the device-side row count on that launch only.)"""
    return bool(STAGE_KERNEL and F in (64, 128) and W.dim() == 2 and tuple(W.shape) == (F, blocks * F)
                and all(packed_stage_block(W, c * F, transposed=True) is not None for c in range(blocks)))


def layer_fused(dims: Sequence[LayerDim], table, csr_mode: int = 0) -> List[Tensor]:
    """[out_up_0, out_b_0, out_up_1, out_b_1, ...] ([out_up_d, out_down_d, out_b_d] for a dimension with `want_down`); no
    autograd (inference path).  `table` is one of the
    batch's item tables (cwn_amd/blockplan.py: ItemTable); csr_mode 0 sorts the COO entries in the
    kernel, _ffi.LAYER_CSR_STORE also stores every item's CSR in the table's cache, _ffi.LAYER_CSR_LOAD
    reads it back instead (same index tensors as the storing call).  Index errors go to the sticky
    error word of cwn_amd/csr.py (`csr.check_errors`)."""
    from .csr import _err_flag
    dev = dims[0].x.device
    F = int(dims[0].x.size(1))
    outs, arr = [], (_ffi.LayerDim * len(dims))()
    keep = []
    for d, D in enumerate(dims):
        x = _f32c(D.x, 'x')
        if x.size(1) != F:
            raise ValueError('every dimension must have the same feature width')
        up, sh, bi = D.up_index, D.up_shared, D.b_index
        for t, name in ((up, 'up_index'), (sh, 'up_shared'), (bi, 'b_index')):
            if t is not None and (t.dtype != torch.long or not t.is_cuda or not t.is_contiguous()):
                raise TypeError(f'{name} must be a contiguous int64 GPU tensor')
        w, b = D.msg_w_packed, _f32c(D.msg_bias, 'msg_bias')
        e1, e2 = _f32c(D.eps1, 'eps1'), _f32c(D.eps2, 'eps2')
        out_up = torch.empty_like(x)
        out_b = torch.empty_like(x)
        out_d = torch.empty_like(x) if D.want_down else None
        e3 = _f32c(D.eps3, 'eps3') if D.want_down else None
        outs += [out_up, out_b] if out_d is None else [out_up, out_d, out_b]
        keep += [x, w, b, e1, e2, e3]
        e_up = 0 if up is None else int(up.size(1))
        arr[d] = _ffi.LayerDim(x=x.data_ptr(), up_index=_ffi.ptr(up) if e_up else None,
                               up_shared=_ffi.ptr(sh) if e_up else None,
                               b_index=_ffi.ptr(bi) if bi is not None and bi.size(1) else None,
                               msg_w_packed=_ffi.ptr(w), msg_bias=_ffi.ptr(b), eps1=_ffi.ptr(e1), eps2=_ffi.ptr(e2),
                               out_up=out_up.data_ptr(), out_b=out_b.data_ptr(), n_cells=x.size(0),
                               e_up=e_up, n_b=0 if bi is None else int(bi.size(1)),
                               out_down=_ffi.ptr(out_d), eps3=_ffi.ptr(e3))
    plan = table.c_plan(with_cache=csr_mode != 0)
    _ffi.check(_ffi.lib().cwn_layer_fused_f32(arr, len(dims), F, plan, int(csr_mode), _err_flag(dev).data_ptr(),
                                               _ffi.stream_ptr(dev)), 'cwn_layer_fused_f32')
    return outs


# ---- the reduce half of a conv layer's OUTPUT BatchNorm, taken over by the blocked backward of the NEXT layer (round 6) ----------
# The combine network of a SparseCINConv ends in Linear -> BatchNorm -> ReLU (mp/layers.py:322-325) and its output H is the next
# conv layer's input x.  Autograd hands the next layer's dx to this layer's backward as dy, and the BatchNorm backward begins with
# two column sums over dy (d beta, d gamma) -- a launch of its own, cwn_norm_bwd_reduce_f32, 5.9 us x 4 per ZINC step, because
# the producer of dy was a launch "on the other side of autograd".  It need not be: dense_train's forward REGISTERS H here
# (pre-normalisation z, the stage's constants, a zeroed slot buffer, a token); the blocked backward of the layer that reads H as
# its x looks its inputs up, lets cwn_layer_bwd_own_f32 add the sums of the dx rows every workgroup owns into the slots
# (cwn_layer_bwd_dim.out_bn) and MARKS the dx tensor it returns with the token; dense_train's backward, handed exactly that
# tensor as dy (same address: autograd adds nothing when H has one consumer), takes the slot sums and launches no reduce.
# Anything else -- another consumer, a copy, a stale entry -- misses and runs the reduce as before.
BN_BWD_FUSE = os.environ.get('CWN_BN_BWD_FUSE', '1') != '0'
BN_BWD_FUSED = [0]                         # reduce launches taken over so far (tests: the path that ran)
_bn_out: Dict[tuple, tuple] = {}           # (device, H.data_ptr()) -> (token, z, aff, slots, shape of H)
_bn_sums: Dict[tuple, object] = {}         # (device, dx.data_ptr()) -> token


def bn_registry_clear() -> None:
    _bn_out.clear()
    _bn_sums.clear()


def bn_out_register(h: Tensor, z: Tensor, aff: Tensor, slots: Tensor) -> object:
    # (steps outside a step_arena bracket: nothing clears the registry, and an entry keeps its z / constants / slots alive -- a
    #  few forwards' worth at most: an entry older than that names tensors whose backward has long run or never will)
    if len(_bn_out) >= 32 or len(_bn_sums) >= 32:
        bn_registry_clear()
    token = object()
    _bn_out[(h.device.index, h.data_ptr())] = (token, z, aff, slots, tuple(h.shape))
    return token


def bn_out_lookup(x: Tensor) -> Optional[tuple]:
    e = _bn_out.get((x.device.index, x.data_ptr())) if (BN_BWD_FUSE and x is not None) else None
    return e if (e is not None and e[4] == tuple(x.shape) and x.is_contiguous()) else None


def bn_sums_ready(dy: Tensor, token) -> bool:
    return token is not None and _bn_sums.get((dy.device.index, dy.data_ptr())) is token


# The backward of the propagate step as ONE launch.  Two forms:
#   2 (default) the OWNER form (cwn_layer_bwd_own_f32, csrc/cwn_layer_bwd_own.hip) over a table of its own
#     (blockplan.BlockPlan.bwd_items): an item owns the rows of one dimension for a range of complexes and gathers
#     everything they receive -- one writer per dx row, plain stores, no fill, deterministic.  18.6 us per launch at the
#     ZINC batch of 128 against ~30 for what it replaces (transposed aggregation + transposed-weight GEMM + an add); the
#     training step 0.993 -> 0.948 ms.  A batch with a complex beyond a workgroup keeps the streaming backward.
#   1 the first, ATOMIC form (cwn_layer_bwd_f32) over the forward's item table: a dx row receives pieces from up to three
#     workgroups through fp32 atomics onto a zeroed matrix -- 25 us + the fill, no gain over the streaming path; kept for
#     the comparison (tools/ubench_layer_bwd.py).
#   0 the streaming backward (transposed CSR aggregation + GEMM).
BLOCKED_BACKWARD = int(os.environ.get('CWN_BLOCKED_BACKWARD', '2') or 0)
BLOCKED_BACKWARD_LAUNCHES = [0, 0]         # launches of the atomic / owner form so far (tests: the path that ran)


def layer_backward(dims: Sequence[LayerDim], table, ys_of, gs_of, wt_of, bwd_table=None, fuse_bn: bool = False) -> Optional[Tuple[List[Tensor], List]]:
    """cwn_layer_bwd_f32: the backward of one propagate step over the item table of its forward launch.  dims: the
    LayerDim list of the forward; ys_of[d] = (Y1_d or None, Y2 stored at dimension d or None); gs_of[d] = (dL/d out_up_d,
    dL/d out_b_d), None = zero; wt_of[d] = transposed packed weight or None.  Returns ([dx_d], [(gY1_d, gY2 at d)]) or
    None when the launch does not apply (a table in another form, an item beyond the backward's LDS)."""
    own = bwd_table is not None            # the owner form (cwn_layer_bwd_own_f32): its own table, dx stored once
    if not own and (getattr(table, 'variant', 0) != 0 or getattr(table, 'n_big', 0)):
        return None
    n, F = len(dims), int(dims[0].x.size(1))
    L = _ffi.lib()
    if not own and int(L.cwn_layer_bwd_lds_bytes(F, int(table.max_rows))) == 0:
        return None
    dev = dims[0].x.device
    rows = [int(D.x.size(0)) for D in dims]
    # atomic form: every piece is ADDED (one fill for the layer); owner form: every row is written once
    # (the owner form writes the rows its table owns -- a table that ends before a matrix does leaves the rest
    # unwritten: zero-filled then, unless the rows are a static batch's capacity padding, which nothing ever reads)
    covered = own and all(int(bwd_table.cells_end[d]) == rows[d] for d in range(n))
    dx_buf = (torch.empty if covered else torch.zeros)(sum(rows), F, dtype=torch.float32, device=dev)
    dxs = list(dx_buf.split(rows))
    arr = (_ffi.LayerBwdDim * n)()
    gys, keep = [], []
    for d, D in enumerate(dims):
        e_up = 0 if D.up_index is None else int(D.up_index.size(1))
        n_b = 0 if D.b_index is None else int(D.b_index.size(1))
        y1, y2 = ys_of[d]
        gy1 = torch.empty(rows[d], F, dtype=torch.float32, device=dev) if y1 is not None else None
        gy2 = torch.empty(rows[d], F, dtype=torch.float32, device=dev) if y2 is not None else None
        gys.append((gy1, gy2))
        gu, gb = gs_of[d]
        gu = None if gu is None else _f32c(gu, 'grad')
        gb = None if gb is None else _f32c(gb, 'grad')
        e1, e2 = _f32c(D.eps1, 'eps1'), _f32c(D.eps2, 'eps2')
        keep += [gu, gb, e1, e2]
        if e_up and wt_of[d] is None:
            return None
        arr[d] = _ffi.LayerBwdDim(g_up=_ffi.ptr(gu), g_b=_ffi.ptr(gb), y1=_ffi.ptr(y1), y2=_ffi.ptr(y2),
                                  up_index=_ffi.ptr(D.up_index) if e_up else None, up_shared=_ffi.ptr(D.up_shared) if e_up else None,
                                  b_index=_ffi.ptr(D.b_index) if n_b else None, wt_packed=_ffi.ptr(wt_of[d]) if e_up else None,
                                  eps1=_ffi.ptr(e1), eps2=_ffi.ptr(e2), dx=dxs[d].data_ptr(), gy1=_ffi.ptr(gy1), gy2=_ffi.ptr(gy2),
                                  n_cells=rows[d], e_up=e_up, n_b=n_b)
    from .csr import _err_flag
    if own:
        # x_d registered as the output of a BatchNorm stage (bn_out_register): this launch takes the reduce of its backward
        marks = []
        if fuse_bn and F in (64, 128):
            for d, D in enumerate(dims):
                e = bn_out_lookup(D.x)
                if e is None or rows[d] == 0:
                    continue
                token, z, aff, slots, _ = e
                if (z.shape != D.x.shape or z.stride(1) != 1 or not is_vec16(z) or not aligned16(aff)
                        or aff.numel() != 4 * F or slots.numel() != _ffi.BN_SLOTS * 2 * F):
                    continue
                arr[d].out_bn = _ffi.BnBwdLive(z=z.data_ptr(), aff=aff.data_ptr(), slots=slots.data_ptr(), ldz=z.stride(0))
                marks.append((d, token))
        _ffi.check(L.cwn_layer_bwd_own_f32(arr, n, F, bwd_table.c_plan(), _err_flag(dev).data_ptr(), _ffi.stream_ptr(dev)),
                   'cwn_layer_bwd_own_f32')
        BLOCKED_BACKWARD_LAUNCHES[1] += 1
        for d, token in marks:
            _bn_sums[(dxs[d].device.index, dxs[d].data_ptr())] = token
            # one shot: the slots now hold this backward's sums -- a SECOND backward over the same forward (retain_graph) finds no
            # entry, adds nothing onto them, marks nothing, and the stage's own reduce launch runs
            _bn_out.pop((dims[d].x.device.index, dims[d].x.data_ptr()), None)
        return dxs, gys
    plan = table.c_plan(with_cache=False)
    _ffi.check(L.cwn_layer_bwd_f32(arr, n, F, plan, _err_flag(dev).data_ptr(), _ffi.stream_ptr(dev)), 'cwn_layer_bwd_f32')
    BLOCKED_BACKWARD_LAUNCHES[0] += 1
    return dxs, gys


class LayerLaunch:
    """A prepared cwn_layer_fused_f32 call for one (layer, batch): the descriptor array with everything
    that does not change between calls filled in once (indices, packed weights, eps, sizes) and the
    cwn_layer_plan of the batch's item table.  `run(xs, csr_mode)` fills in the feature and output
    pointers and launches: ~10 us of host time instead of ~60."""

    def __init__(self, dims: Sequence[LayerDim], table):
        self.table = table
        # one launch per item table: a MixedTable (blockplan.py) is two -- the two-per-CU form for the complexes that
        # fit it, the 16-wave form for the rest -- over complementary complexes, into the same outputs
        self.parts = list(getattr(table, 'parts', [table]))
        self.n = len(dims)
        self.F = int(dims[0].x.size(1))
        self.arr = (_ffi.LayerDim * self.n)()
        self.keep = []
        self.rows = []
        for d, D in enumerate(dims):
            up, sh, bi = D.up_index, D.up_shared, D.b_index
            for t, name in ((up, 'up_index'), (sh, 'up_shared'), (bi, 'b_index')):
                if t is not None and (t.dtype != torch.long or not t.is_cuda or not t.is_contiguous()):
                    raise TypeError(f'{name} must be a contiguous int64 GPU tensor')
            w, b = D.msg_w_packed, _f32c(D.msg_bias, 'msg_bias')
            e1, e2 = _f32c(D.eps1, 'eps1'), _f32c(D.eps2, 'eps2')
            e3 = _f32c(D.eps3, 'eps3') if D.want_down else None
            self.keep += [up, sh, bi, w, b, e1, e2, e3]
            e_up = 0 if up is None else int(up.size(1))
            self.arr[d] = _ffi.LayerDim(eps3=_ffi.ptr(e3), up_index=_ffi.ptr(up) if e_up else None, up_shared=_ffi.ptr(sh) if e_up else None,
                                        b_index=_ffi.ptr(bi) if bi is not None and bi.size(1) else None,
                                        msg_w_packed=_ffi.ptr(w), msg_bias=_ffi.ptr(b), eps1=_ffi.ptr(e1),
                                        eps2=_ffi.ptr(e2), n_cells=int(D.x.size(0)), e_up=e_up,
                                        n_b=0 if bi is None else int(bi.size(1)))
            self.rows.append(int(D.x.size(0)))
        for part in self.parts:
            if getattr(part, 'n_big', 0):
                self._attach_big(dims, part)
        self._big_y = [(self.arr[d].big_y1, self.arr[d].big_y2) for d in range(self.n)]     # the BIG records' scratch
        self.total_rows = sum(self.rows)
        # outputs per dimension: (out_up, out_b), or (out_up, out_down, out_b) when the layer wants the third (all or none)
        downs = [bool(D.want_down) for D in dims]
        if any(downs) and not all(downs):
            raise ValueError('want_down: every dimension of a layer or none')
        self.n_out = 3 if downs[0] else 2
        self._sizes = [r for r in self.rows for _ in range(self.n_out)]   # rows of the outputs, in output order
        self._off = [sum(self._sizes[:i]) for i in range(len(self._sizes))]
        self.dev = dims[0].x.device
        self._plans = {}
        from .csr import _err_flag
        self.err = _err_flag(self.dev)
        self._err_ptr = self.err.data_ptr()
        self.fn = _ffi.lib().cwn_layer_fused_f32
        # the per-call part in C++ when the compiled binding is there (csrc/cwn_torch_ext.cpp keeps a copy of the array)
        from . import _cext
        X = _cext.ext()
        self._c = None if X is None else X.LayerCall(C.addressof(self.arr), C.sizeof(self.arr), self.n, self.F,
                                                     self.rows, self._err_ptr, _cext.fn_address(self.fn), self.dev.index,
                                                     self.n_out)

    def _attach_big(self, dims: Sequence[LayerDim], table) -> None:
        """BIG records (include/cwn_hip.h): complexes no workgroup's LDS holds are streamed by their workgroup, which
        needs (a) the destination-sorted CSR of THEIR entries of every adjacency, in global cell numbers -- built here
        once per batch from slices of the batch's own index tensors (the table records where each complex's entries
        lie), cached on the table for all layers -- and (b) scratch matrices for Y1 / Y2."""
        from .blockplan import I_FLAGS, I_G, I_NT, I_TASK0, I_UE0, I_UNE, T_BE0, T_BNE, T_DIM, T_INTS
        from .csr import Adjacency, build_many
        key = tuple((id(t), _ffi.tver(t)) for D in dims for t in (D.up_index, D.up_shared, D.b_index) if t is not None)
        ctx = table.big_ctx
        if ctx is None or ctx['key'] != key or ctx['F'] != self.F:
            recs = table.big_records
            dev, n, F = dims[0].x.device, len(dims), self.F
            ctx = {'key': key, 'F': F, 'dims': [dict() for _ in range(n)], 'keep': []}
            todo = []
            dummy_i = torch.zeros(4, dtype=torch.int32, device=dev)
            for d, D in enumerate(dims):
                N = int(D.x.size(0))
                c = ctx['dims'][d]
                if D.up_index is not None and D.up_index.size(1) > 0:
                    sl = [(int(r[I_UE0]), int(r[I_UNE])) for r in recs if (r[I_FLAGS] & 1) and int(r[I_G]) == d and r[I_UNE] > 0]
                    if sl:
                        idx = torch.cat([D.up_index[:, a:a + m] for a, m in sl], 1).contiguous()
                        sh = torch.cat([D.up_shared[a:a + m] for a, m in sl]).contiguous()
                        adj = Adjacency.from_index(idx, N, N, sh, int(dims[d + 1].x.size(0)), build=False)
                        todo.append(adj)
                        c['up'] = adj
                        ctx['keep'] += [idx, sh]
                    # scratch: Y1 of this dimension, Y2 of the next one (only complexes with BIG records write / read them)
                    c['y1'] = torch.empty(N if sl else 4, F, dtype=torch.float32, device=dev)
                    ctx['dims'][d + 1]['y2'] = torch.empty(int(dims[d + 1].x.size(0)) if sl else 4, F, dtype=torch.float32, device=dev)
                if D.b_index is not None and D.b_index.size(1) > 0 and d > 0:
                    sl = []
                    for r in recs:
                        for t in range(int(r[I_NT])):
                            o = I_TASK0 + T_INTS * t
                            if int(r[o + T_DIM]) == d and r[o + T_BNE] > 0:
                                sl.append((int(r[o + T_BE0]), int(r[o + T_BNE])))
                    if sl:
                        idx = torch.cat([D.b_index[:, a:a + m] for a, m in sl], 1).contiguous()
                        adj = Adjacency.from_index(idx, N, int(dims[d - 1].x.size(0)), build=False)
                        todo.append(adj)
                        c['b'] = adj
                        ctx['keep'].append(idx)
            build_many(todo)
            ctx['dummy'] = dummy_i
            table.big_ctx = ctx
        self.keep.append(ctx)
        dummy = ctx['dummy']
        for d, D in enumerate(dims):
            c, a = ctx['dims'][d], self.arr[d]
            if a.e_up > 0:
                up = c.get('up')
                rowptr = up.rowptr if up is not None else self._zero_rowptr(ctx, int(D.x.size(0)), dummy.device)
                a.big_up_rowptr = rowptr.data_ptr()
                a.big_up_col = (up.col if up is not None else dummy).data_ptr()
                a.big_up_aux = (up.aux if up is not None else dummy).data_ptr()
                a.big_y1 = c['y1'].data_ptr()
            if 'y2' in c:
                a.big_y2 = c['y2'].data_ptr()
            if a.n_b > 0:
                b = c.get('b')
                rowptr = b.rowptr if b is not None else self._zero_rowptr(ctx, int(D.x.size(0)), dummy.device)
                a.big_b_rowptr = rowptr.data_ptr()
                a.big_b_col = (b.col if b is not None else dummy).data_ptr()

    @staticmethod
    def _zero_rowptr(ctx, n, dev):
        z = ctx.setdefault('zeros', {})
        if n not in z:
            z[n] = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        return z[n]

    def run(self, xs: Sequence[Tensor], csr_mode: int = 0, ys: Optional[Sequence] = None) -> List[Tensor]:
        """`ys` (training forward): per dimension (Y1 matrix or None, Y2 matrix or None), [n_cells, F] fp32 -- every item
        also writes its rows of the message products there (CWN_LAYER_STORE_Y)."""
        F = self.F
        if self._c is not None:
            c = self._c
            cached = (int(csr_mode) & (_ffi.LAYER_CSR_STORE | _ffi.LAYER_CSR_LOAD)) != 0
            if not c.has_plans(cached):
                plans = self._plans[cached] = [t.c_plan(with_cache=cached) for t in self.parts]
                c.set_plans(cached, [C.addressof(p) for p in plans], C.sizeof(plans[0]))
            return c.run(xs, int(csr_mode), ys)
        for d in range(self.n):
            y1, y2 = ys[d] if ys is not None else (None, None)
            a = self.arr[d]
            a.big_y1 = y1.data_ptr() if y1 is not None else self._big_y[d][0]
            a.big_y2 = y2.data_ptr() if y2 is not None else self._big_y[d][1]
        if ys is not None:
            csr_mode = int(csr_mode) | _ffi.LAYER_STORE_Y
        k = self.n_out
        buf = torch.empty(k * self.total_rows, F, dtype=torch.float32, device=self.dev)   # all six (nine) outputs
        outs = buf.split(self._sizes)                       # one call: [out_up_0, out_b_0, out_up_1, ...]
        base, row_b = buf.data_ptr(), 4 * F
        for d in range(self.n):
            x = xs[d]
            if not x.is_contiguous():
                x = x.contiguous()
            if x.dim() != 2 or x.size(0) != self.rows[d] or x.size(1) != F:
                raise ValueError('feature rows / width do not match the batch this launch was prepared for')
            if x.dtype != torch.float32 or x.device != self.dev:
                raise TypeError('features must be float32 tensors on the GPU this launch was prepared for')
            a = self.arr[d]
            a.x = x.data_ptr()
            a.out_up = base + self._off[k * d] * row_b
            a.out_b = base + self._off[k * d + k - 1] * row_b
            if k == 3:
                a.out_down = base + self._off[k * d + 1] * row_b
        cached = (int(csr_mode) & (_ffi.LAYER_CSR_STORE | _ffi.LAYER_CSR_LOAD)) != 0
        plans = self._plans.get(cached)
        if plans is None:
            plans = self._plans[cached] = [t.c_plan(with_cache=cached) for t in self.parts]
        stream = _ffi.stream_ptr(self.dev)
        for plan in plans:
            rc = self.fn(self.arr, self.n, F, plan, int(csr_mode), self._err_ptr, stream)
            if rc != 0:
                _ffi.check(rc, 'cwn_layer_fused_f32')
        return list(outs)


if os.environ.get('CWN_DETERMINISTIC') == '1':
    deterministic(True)
