"""A batch of cochains of FIXED CAPACITY that a captured hipGraph refills on the device: the edge-flow experiments' shuffled
epoch (`for batch in loader`, every step a batch never seen before) on the graph path -- the cochain counterpart of
static_batch.StaticBatch(mode='csr'), over a packed.PackedCochains(with_csr=True).

What a batch changes lives in device memory:

  * x, y, the batch vector, both index tensors with their orientations and the four CSR plans (upper, lower, their
    source-keyed transposes) are capacity-sized buffers, filled by ONE cwn_collate launch from the packed dataset;
  * the segment tables of that launch, the head's `ptr` and the live counts (rows, upper / lower entries, cochains) are ONE
    fixed block of int64 words; the tables of a whole epoch are cut on the host (packed.cochain_epoch_tables: numpy), uploaded
    with one copy (`set_epoch`), and a one-workgroup launch (cwn_table_advance) moves the block to the next batch and
    advances a device cursor -- a replayed step needs nothing from the host;
  * the layers read the live row count through m_dev (`dynamic()`), the head through `head_counts` (ops.flow_head_counted).

Padding rows of every float buffer may hold anything (the tests poison them with NaN): no launch of the served path reads them.
One set of buffers serves every step of a captured sequence -- the steps run one after the other on one stream; `slots` is the
number of steps a captured sequence holds (static_graph.StaticCochainForward / StaticCochainTrainStep).
"""
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _ffi, csr
from .complex import CochainBatch
from .packed import EPOCH_COUNTS, PackedCochains, cochain_epoch_layout, cochain_epoch_tables

_INDEX = ('upper_index', 'lower_index')
_CAP_KEYS = ('rows',) + _INDEX
MAX_SLOTS = 64


def capacities(meta: dict, batch_size: int, caps: Optional[dict] = None) -> dict:
    """{'rows', 'upper_index', 'lower_index'} -> capacity: what the `batch_size` largest cochains of the dataset need together (no
    batch can exceed it), `caps` overriding; at least 1; then moved up until the three are pairwise distinct and distinct from
    batch_size -- a row count identifies what it counts (_ffi.dynamic_rows).  numpy only."""
    B = int(batch_size)
    if B < 1:
        raise ValueError('batch_size >= 1')
    sizes = {'rows': meta['n_cells']}
    for key in _INDEX:
        sizes[key] = meta['length'][meta['keys'].index(key)] if key in meta['keys'] else np.zeros(1, dtype=np.int64)
    unknown = set(caps or {}) - set(_CAP_KEYS)
    if unknown:
        raise ValueError(f'caps: unknown entries {sorted(unknown)} (rows, upper_index, lower_index)')
    out, used = {}, {B}
    for name in _CAP_KEYS:
        col = np.sort(np.asarray(sizes[name], dtype=np.int64))
        cap = int((caps or {}).get(name, int(col[-min(B, col.size):].sum())))
        if cap < int(col[-1]):
            raise ValueError(f'caps[{name!r}] = {cap} is below the largest cochain of the dataset ({int(col[-1])}): no batch with '
                             'that cochain would fit')
        cap = max(cap, 1)
        while cap in used:
            cap += 1
        used.add(cap)
        out[name] = cap
    return out


def check_capacity(meta: dict, batches: Sequence[Sequence[int]], batch_size: int, caps: dict) -> None:
    """ValueError naming the first batch beyond `batch_size` cochains or beyond a capacity, and what overflowed."""
    cols = {'rows': meta['n_cells']}
    for key in _INDEX:
        if key in meta['keys']:
            cols[key] = meta['length'][meta['keys'].index(key)]
    what = {'rows': 'rows', 'upper_index': "entries of 'upper_index'", 'lower_index': "entries of 'lower_index'"}
    for j, idx in enumerate(batches):
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        if idx.size == 0 or idx.size > batch_size:
            raise ValueError(f'batch {j}: 1 .. {batch_size} cochains (got {idx.size})')
        if idx.min() < 0 or idx.max() >= meta['n_cells'].size:
            raise IndexError(f'batch {j}: cochain numbers outside 0 .. {meta["n_cells"].size - 1}')
        for name, col in cols.items():
            tot = int(col[idx].sum())
            if tot > caps[name]:
                raise ValueError(f'batch {j}: {tot} {what[name]} exceed the capacity {caps[name]} of this StaticCochainBatch; build '
                                 'it with larger `caps`, or run this batch through PackedCochains.collate')


class StaticCochains(CochainBatch):
    """The CochainBatch over the buffers of a StaticCochainBatch: its plans are written by the collate launch."""

    def prepare(self, *args, **kwargs):
        return self

    def forget_plans(self):
        return self


class StaticCochainBatch:
    """Capacity-sized device buffers for batches of `batch_size` cochains of `packed`, the fixed table block, the epoch's tables
    and the launches that move to the next batch (`advance`).  caps: {'rows' | 'upper_index' | 'lower_index': capacity}."""

    def __init__(self, packed: PackedCochains, batch_size: int, caps: Optional[dict] = None, slots: int = 1):
        if not isinstance(packed, PackedCochains):
            raise TypeError('StaticCochainBatch takes a packed.PackedCochains')
        if not packed.with_csr:
            raise ValueError('StaticCochainBatch needs a PackedCochains built with with_csr=True (the plans of a batch are the '
                             'concatenation of the per-cochain CSRs it keeps)')
        if packed.device.type != 'cuda':
            raise _ffi.CwnError('StaticCochainBatch needs the packed cochains on the GPU')
        self.S = int(slots)
        if self.S < 1 or self.S > MAX_SLOTS:
            raise ValueError(f'1 .. {MAX_SLOTS} slots')
        self.packed, self.B, self.device = packed, int(batch_size), packed.device
        meta, dev, B = packed.meta, packed.device, self.B
        self.caps = capacities(meta, B, caps)
        self.lay = cochain_epoch_layout(meta, B)
        T = self.T = self.lay['len']
        self.table = torch.zeros(T, dtype=torch.int64, device=dev)
        # the epoch's tables: room for an epoch over the whole dataset and a replay's worth of empty batches behind it -- a
        # captured step holds this buffer's address and length (reserve_epoch asks for more BEFORE the first capture)
        self.n_batches = -(-packed.num // B) + self.S
        self.epoch = torch.zeros(self.n_batches, T, dtype=torch.int64, device=dev)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=dev)
        self.advances = 0
        c = self.lay['counts']
        self.counts = {name: self.table[c + i:c + i + 1] for i, name in enumerate(EPOCH_COUNTS)}
        self.active = self.counts['cochains']                       # (FlatAdam.active: a step on an empty batch changes nothing)
        self._build_buffers()

    # ---- buffers, plans, descriptors ------------------------------------------------------------------------------
    def count_ptr(self, name: str) -> int:
        return self.table.data_ptr() + 8 * (self.lay['counts'] + EPOCH_COUNTS.index(name))

    def _build_buffers(self) -> None:
        pc, dev, B, lay = self.packed, self.device, self.B, self.lay
        n = self.caps['rows']
        at = lambda name: self.table.data_ptr() + 8 * lay[name]
        b = self.batch = StaticCochains(pc.dim)
        self.bufs, descs = {}, []
        y_len = 0
        for key in pc.meta['keys']:
            pk = pc._packs[key]
            if key == 'x':
                cap, val = n * pk.width, torch.zeros(n, pk.width, dtype=pk.data.dtype, device=dev)
            elif key == 'y':
                y_len = int(np.asarray(pk.length).max(initial=0))
                cap = B * max(y_len, 1)
                val = torch.zeros((cap // max(pk.width, 1),) + pc._y_tail, dtype=pk.data.dtype, device=dev)
            elif pk.rows == 2:
                cap, val = self.caps[key], torch.zeros(2, self.caps[key], dtype=pk.data.dtype, device=dev)
            else:
                cap = self.caps[key.replace('orient', 'index')]
                val = torch.zeros(cap, dtype=pk.data.dtype, device=dev)
            self.bufs[key] = val
            if key == 'x':
                b._x = val
            else:
                setattr(b, key, val)
            descs.append(_ffi.CollateDesc(src=pk.data.data_ptr(), dst=val.data_ptr(), dst_start=at('dst_' + key), src_start=at('src_' + key),
                                          add=at('cell_off') if pk.rows == 2 else None,
                                          src_row_stride=pk.data.size(-1) if pk.rows == 2 else 0,
                                          dst_row_stride=cap if pk.rows == 2 else 0, n_rows=pk.rows, op=pk.op))
        self.input = self.bufs.get('x')
        b.batch = self.bufs['batch'] = torch.zeros(n, dtype=torch.int64, device=dev)
        descs.append(_ffi.CollateDesc(src=None, dst=b.batch.data_ptr(), dst_start=at('seg'), src_start=None, add=None, src_row_stride=0,
                                      dst_row_stride=0, n_rows=1, op=_ffi.COLLATE_SEGID64))
        # the plans: capacity-sized csr.Adjacency objects whose arrays the collate launch writes (no cwn_csr_build), entered
        # where OrientedConv looks plans up, tagged with the device words of their live counts (never looked up by value)
        self.plans: List[csr.Adjacency] = []
        self._long: List[csr.Adjacency] = []
        for key, local in pc._csr.items():
            index = self.bufs.get(key)
            if index is None:
                continue
            adj = csr.Adjacency(index[1], index[0], n, n)
            adj.transposes()
            for a, (rp, col, perm) in zip((adj, adj._t_src), local):
                a.rowptr.zero_()
                a.col.zero_()
                a.perm.zero_()
                a.e_dev_ptr, a.rows_dev_ptr = self.count_ptr(key), self.count_ptr('rows')
                if pc.has_long_rows and a.long_rows is not None:
                    a.n_long.zero_()
                    self._long.append(a)            # (filled by every advance: cwn_csr_long_rows under the live row count)
                else:
                    a.long_rows = a.n_long = None   # nothing fills them: no list, and the aggregation walks every row itself
                one = lambda src, dst, dst_start, src_start, add: _ffi.CollateDesc(
                    src=src.data_ptr(), dst=dst, dst_start=at(dst_start), src_start=at(src_start), add=None if add is None else at(add),
                    src_row_stride=0, dst_row_stride=0, n_rows=1, op=_ffi.COLLATE_COPY32 if add is None else _ffi.COLLATE_ADD32)
                descs.append(one(pc._zero, a.rowptr.data_ptr(), 'one_dst', 'zero_src', None))
                descs.append(one(rp, a.rowptr.data_ptr() + 4, 'seg', 'row0', 'dst_' + key))
                descs.append(one(col, a.col.data_ptr(), 'dst_' + key, 'src_' + key, 'cell_off'))
                descs.append(one(perm, a.perm.data_ptr(), 'dst_' + key, 'src_' + key, 'dst_' + key))
                a.built = True
                self.plans.append(a)
            csr.register_adjacency(index, adj)
        if len(descs) > _ffi.MAX_COLLATE_DESCS:
            raise _ffi.CwnError(f'{len(descs)} collate descriptors, one launch takes {_ffi.MAX_COLLATE_DESCS}')
        self._descs = (_ffi.CollateDesc * len(descs))(*descs)
        self._long_descs = None
        if self._long:
            self._long_descs = (_ffi.LongRowsDesc * len(self._long))(*[
                _ffi.LongRowsDesc(rowptr=a.rowptr.data_ptr(), n_rows=a.n_dst, m_dev=a.rows_dev_ptr, long_rows=a.long_rows.data_ptr(),
                                  n_long=a.n_long.data_ptr(), long_cap=a.long_cap) for a in self._long])
        o = lay['seg']
        b.ptr = None
        b.ptr_dev = self.table[o:o + B + 1]
        b.head_counts = (self.counts['rows'], self.counts['cochains'])
        b.__num_cochains__ = B
        b.__num_cells__ = n
        b.__num_cells_up__ = 0
        if pc.dim > 0:
            b.__num_cells_down__ = 0
        b.__slices__ = {}
        self.y_per_cochain = y_len

    # ---- what the step drivers ask ------------------------------------------------------------------------------------
    def restore(self) -> None:
        """The raw input features back into the container (the models overwrite `x` layer by layer)."""
        self.batch._x = self.input

    def dynamic(self) -> _ffi.dynamic_rows:
        """Context manager: inside, a launch over the capacity rows reads the live row count, one over the capacity's cochains
        (the loss, the head's weight gradients) the live cochains."""
        return _ffi.dynamic_rows({self.caps['rows']: self.count_ptr('rows'), self.B: self.count_ptr('cochains')})

    def sizes(self) -> dict:
        """The live counts of the batch the buffers hold (host sync: tests, diagnostics)."""
        c = self.lay['counts']
        return dict(zip(EPOCH_COUNTS, self.table[c:c + 4].tolist()))

    def poison(self, value: float = float('nan')) -> None:
        """Every float buffer filled with `value` (tests: no launch may read a padding row)."""
        for t in self.bufs.values():
            if t.is_floating_point():
                t.fill_(value)

    # ---- epochs -------------------------------------------------------------------------------------------------------
    def reserve_epoch(self, n_batches: int) -> None:
        """Room for epochs of up to n_batches batches -- before the first advance: a captured step holds the buffer's address."""
        n = int(n_batches) + self.S
        if n <= self.n_batches:
            return
        if self.advances > 0:
            raise RuntimeError(f'reserve_epoch({n_batches}) after the first advance: a captured step reads the buffer of '
                               f'{self.n_batches - self.S} batches it was captured with -- ask before building the step')
        self.n_batches = n
        self.epoch = torch.zeros(n, self.T, dtype=torch.int64, device=self.device)

    def epoch_tables(self, batches: Sequence[Sequence[int]]) -> np.ndarray:
        """The host half of `set_epoch`: the capacity check, then one array with every batch's tables."""
        check_capacity(self.packed.meta, batches, self.B, self.caps)
        return cochain_epoch_tables(self.packed.meta, batches, self.B)

    def set_epoch(self, batches: Sequence[Sequence[int]]) -> int:
        """Upload the tables of an epoch's batches (ONE host -> device copy, S empty batches behind them) and rewind the cursor:
        advance number j after this call moves to batch j.  Returns the number of batches."""
        self.reserve_epoch(len(batches))
        host = np.zeros((len(batches) + self.S, self.T), dtype=np.int64)
        host[:len(batches)] = self.epoch_tables(batches)
        self.epoch[:host.shape[0]].copy_(torch.from_numpy(host))
        self.cursor.zero_()
        return len(batches)

    def set_batches(self, batches: Sequence[Sequence[int]]) -> None:
        if not (1 <= len(batches) <= self.S):
            raise ValueError(f'1 .. {self.S} batches')
        self.set_epoch(batches)

    def set_batch(self, idx: Sequence[int]) -> None:
        self.set_batches([idx])

    def rewind(self, j: int = 0) -> None:
        self.cursor.fill_(int(j))

    def advance(self) -> None:
        """Move to the next batch of the epoch: the table block (cwn_table_advance: tables, live counts, cursor), the arrays and
        plans (cwn_collate) and, where the dataset has hub rows, their lists.  Graph-capturable, no host sync."""
        L, s = _ffi.lib(), _ffi.stream_ptr(self.device)
        _ffi.check(L.cwn_table_advance(self.epoch.data_ptr(), self.n_batches, self.T, self.cursor.data_ptr(), self.table.data_ptr(), s),
                   'cwn_table_advance')
        _ffi.check(L.cwn_collate(self._descs, len(self._descs), self.B, s), 'cwn_collate')
        if self._long_descs is not None:
            _ffi.check(L.cwn_csr_long_rows(self._long_descs, len(self._long_descs), s), 'cwn_csr_long_rows')
        self.advances += 1
