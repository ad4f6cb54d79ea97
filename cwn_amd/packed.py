"""Device-side batching: a dataset of complexes packed in HBM, batches built by ONE kernel.

The reference collates on the CPU: `ComplexBatch.from_complex_list` (data/complex.py:690-728) ->
`CochainBatch.from_cochain_list` (:323-458), a Python loop of per-complex tensor adds and one
`torch.cat` per key, followed by `batch.to(device)`.  Once propagate runs in tens of microseconds
that loop IS the step.  Here every complex's tensors are uploaded ONCE, concatenated per key
(288 GB of HBM holds any of the reference's datasets), and `collate(indices)`:
  * computes the per-array segment tables (lengths, source offsets, running cell offsets of
    data/complex.py:148-169) on the host from numpy metadata -- no device sync,
  * uploads them with ONE small H2D copy,
  * fills every array of the ComplexBatch with ONE launch of cwn_collate.
The integer layout is bit-exact against the reference's (tests/golden/batching.npz).
"""
from typing import Dict, List, Sequence

import numpy as np
import torch

from . import _ffi
from .complex import CochainBatch, Complex, ComplexBatch

_INDEX_KEYS = ('upper_index', 'lower_index', 'shared_boundaries', 'shared_coboundaries', 'boundary_index')
_ALL_KEYS = ('x', 'y') + _INDEX_KEYS
# The destination-sorted CSR of a complex's boundary adjacency and of its transpose, kept per complex in LOCAL numbers
# (`with_csr=True`).  A batch is block-diagonal and per-complex contiguous (data/complex.py:148-169), so the batch's CSR is
# the concatenation of its complexes' CSRs: the `col` arrays collate like an index row (+ the cell offset of the source
# dimension), the row pointers -- stored WITHOUT their leading zero, one number per cell -- collate to rowptr[1:] + the
# running entry count.  What cwn_csr_build does per batch (two launches per step for the front's plans and their transposes)
# is then part of the one collate launch.
_CSR_KEYS = ('b_rowptr', 'b_col', 'bt_rowptr', 'bt_col')
# The node-level target of the ring experiment (data/datasets/ringtransfer.py:69-72: `mask`, one marked vertex per complex):
# kept as the LOCAL number of the marked cell, one int32 per complex.  It collates like a CSR column -- + the complex's
# first row of that dimension, the existing add-an-offset op -- into the global row numbers ops.target_head reads
# (ComplexBatch.target_rows): no host work per batch, and a slot of a StaticBatch holds them like any other key.
_TARGET_KEY = 'target'


class _Packed:
    """One key of one dimension, all complexes concatenated along the last axis."""
    __slots__ = ('data', 'start', 'length', 'has', 'rows', 'width', 'op')

    def __init__(self, data, start, length, has, rows, width, op):
        self.data, self.start, self.length, self.has = data, start, length, has
        self.rows, self.width, self.op = rows, width, op


class PackedComplexes:
    """`complexes` (cwn_amd Complex objects with CPU tensors) packed on `device`."""

    def __init__(self, complexes: Sequence[Complex], device, max_dim: int = 2, with_csr: bool = False):
        self.device = torch.device(device)
        self.max_dim = max_dim
        self.with_csr = bool(with_csr)
        self.num = len(complexes)
        self.dims = np.array([min(c.dimension, max_dim) for c in complexes], dtype=np.int64)
        C = self.num
        D = max_dim + 1
        self.n_cells = np.zeros((D, C), dtype=np.int64)
        self.has_cells = np.zeros((D, C), dtype=bool)
        self.n_up = np.zeros((D, C), dtype=np.int64)
        self.n_down = np.zeros((D, C), dtype=np.int64)
        for ci, cx in enumerate(complexes):
            for d in range(D):
                if d in cx.cochains and d <= cx.dimension:
                    c = cx.cochains[d]
                    n = c.num_cells
                    self.has_cells[d, ci] = n is not None
                    self.n_cells[d, ci] = n or 0
                    self.n_up[d, ci] = c.num_cells_up or 0
                    self.n_down[d, ci] = (c.num_cells_down or 0) if d > 0 else 0
                elif d - 1 in cx.cochains:
                    # a complex without this dimension still shifts later boundary indices by its
                    # number of (d-1)-cells (data/complex.py:709-716)
                    self.n_down[d, ci] = cx.cochains[d - 1].num_cells or 0
        self.keys: List[Dict[str, _Packed]] = []
        for d in range(D):
            per_key = {}
            for key in _ALL_KEYS:
                items = [(cx.cochains[d][key] if (d in cx.cochains and d <= cx.dimension) else None)
                         for cx in complexes]
                if all(t is None for t in items):
                    continue
                per_key[key] = self._pack(items, key)
            self.keys.append(per_key)
        for d in range(D):
            masks = [getattr(cx.cochains[d], 'mask', None) if (d in cx.cochains and d <= cx.dimension) else None for cx in complexes]
            if all(m is None for m in masks):
                continue
            local = np.zeros(C, dtype=np.int64)
            for ci, m in enumerate(masks):
                hit = None if m is None else torch.nonzero(m.reshape(-1)).reshape(-1)
                if hit is None or hit.numel() != 1:
                    raise ValueError(f'complex {ci}: the mask of dimension {d} must mark exactly one cell (it marks '
                                     f'{0 if hit is None else hit.numel()}): a packed dataset carries ONE target row per complex')
                if int(m.numel()) != int(self.n_cells[d, ci]):
                    raise IndexError(f'complex {ci}: a mask of {int(m.numel())} entries over {int(self.n_cells[d, ci])} cells of dimension {d}')
                local[ci] = int(hit[0])
            self._add_target(d, local)
        ys = [cx.y for cx in complexes]
        self.y = self._pack(ys, 'y') if all(t is not None for t in ys) else None
        self._finalise()

    @classmethod
    def from_arrays(cls, device, max_dim: int, dims, n_cells, has_cells, n_up, n_down, keys, y=None,
                    with_csr: bool = False) -> 'PackedComplexes':
        """A packed dataset from arrays that are ALREADY concatenated per key (cwn_amd.lifting.pack_graph_dataset_*:
        a dataset lifted by cwn_lift_many goes from graphs to HBM without per-complex Python objects).
        keys[d][name] = (data, lengths, has): `data` as the constructor would concatenate it (x: [rows, width] or flat;
        a two-row index: [2, total]; else 1-D), `lengths` per complex in the constructor's units (x: rows * width; an
        index: columns), `has` per complex."""
        self = cls.__new__(cls)
        self.device = torch.device(device)
        self.max_dim = max_dim
        self.with_csr = bool(with_csr)
        self.dims = np.minimum(np.asarray(dims, dtype=np.int64), max_dim)
        self.num = int(self.dims.size)
        D = max_dim + 1
        self.n_cells = np.asarray(n_cells, dtype=np.int64)[:D]
        self.has_cells = np.asarray(has_cells, dtype=bool)[:D]
        self.n_up = np.asarray(n_up, dtype=np.int64)[:D]
        self.n_down = np.asarray(n_down, dtype=np.int64)[:D]
        self.keys = []
        for d in range(D):
            per_key = {}
            for key in _ALL_KEYS:            # the constructor's key order
                if key in keys[d] and np.asarray(keys[d][key][2], dtype=bool).any():
                    per_key[key] = self._packed(*keys[d][key], key)
            self.keys.append(per_key)
        for d in range(D):
            if _TARGET_KEY in keys[d]:     # the marked cell of every complex, LOCAL numbers: an array of one integer per complex
                self._add_target(d, np.asarray(torch.as_tensor(keys[d][_TARGET_KEY]).cpu().numpy(), dtype=np.int64).reshape(-1))
        self.y = self._packed(*y, 'y') if y is not None else None
        self._finalise()
        return self

    def _add_target(self, d: int, local: np.ndarray) -> None:
        """The packed key (d, 'target'): `local[c]` = the marked cell of complex c among its cells of dimension d."""
        n = np.asarray(self.n_cells[d], dtype=np.int64)
        if local.shape != (self.num,):
            raise ValueError(f'one target per complex ({self.num}), got {local.shape}')
        if self.num and (local.min() < 0 or (local >= n).any()):
            bad = int(np.nonzero((local < 0) | (local >= n))[0][0])
            raise IndexError(f'target of dimension {d}: complex {bad} marks cell {int(local[bad])} of its {int(n[bad])}: a local '
                             'index outside its complex')
        ones = np.ones(self.num, dtype=np.int64)
        self.keys[d][_TARGET_KEY] = _Packed(torch.from_numpy(local.astype(np.int32)).to(self.device), np.arange(self.num, dtype=np.int64),
                                            ones, ones > 0, 1, 1, _ffi.COLLATE_ADD32)

    def _packed(self, data: torch.Tensor, lengths, has, key) -> _Packed:
        lengths = np.asarray(lengths, dtype=np.int64)
        width = 1
        if key == 'x':
            width = int(data.size(1)) if data.dim() == 2 else 1
            data = data.reshape(-1)
        start = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
        return _Packed(data.contiguous().to(self.device), start, lengths, np.asarray(has, dtype=bool),
                       2 if key in ('upper_index', 'lower_index', 'boundary_index') else 1, width, self._op(data, key))

    @staticmethod
    def _op(data: torch.Tensor, key: str) -> int:
        if data.dtype == torch.float32 or data.dtype == torch.int32:
            return _ffi.COLLATE_COPY32
        if data.dtype == torch.int64:
            return _ffi.COLLATE_ADD64 if key in _INDEX_KEYS else _ffi.COLLATE_COPY64
        raise TypeError(f'{key}: unsupported dtype {data.dtype} (float32 / int32 / int64 only)')

    def _pack(self, items, key) -> _Packed:
        ref = next(t for t in items if t is not None)
        two_rows = key in ('upper_index', 'lower_index', 'boundary_index')
        width = 1
        if key == 'x':
            width = int(ref.size(1)) if ref.dim() == 2 else 1
        lengths = np.array([0 if t is None else (int(t.size(-1)) if key != 'x' else int(t.size(0)) * width)
                            for t in items], dtype=np.int64)
        has = np.array([t is not None for t in items], dtype=bool)
        start = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
        present = [t for t in items if t is not None]
        if key == 'x':
            data = torch.cat([t.reshape(-1) for t in present])
        else:
            data = torch.cat([t.unsqueeze(0) if t.dim() == 0 else t for t in present], dim=-1)
        return _Packed(data.contiguous().to(self.device), start, lengths, has, 2 if two_rows else 1, width,
                       self._op(data, key))

    # --------------------------------------------------------------------------------------------
    def _add_csr_keys(self) -> None:
        """Per complex, in local numbers: the destination-sorted CSR of boundary_index_d (rows = cells of d, col = boundary
        cell) and of its transpose (rows = cells of d - 1, col = cell), stable in entry order -- what cwn_csr_build
        produces for the batched index, cut at the complexes (module comment at _CSR_KEYS)."""
        D = self.max_dim + 1
        for d in range(1, D):
            pk = self.keys[d].get('boundary_index')
            if pk is None:
                continue
            idx = pk.data.detach().cpu().numpy()                       # [2, E]: row 0 boundary cell, row 1 cell (local)
            E = int(idx.shape[1])
            lengths = np.asarray(pk.length, dtype=np.int64)
            C = self.num
            cid = np.repeat(np.arange(C, dtype=np.int64), lengths)
            ent0 = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
            for name, rows_of, key_row, val_row in (('b', self.n_cells[d], 1, 0), ('bt', self.n_down[d], 0, 1)):
                rows_of = np.asarray(rows_of, dtype=np.int64)
                row0 = np.concatenate([[0], np.cumsum(rows_of)[:-1]]).astype(np.int64)
                key, val = idx[key_row].astype(np.int64), idx[val_row].astype(np.int64)
                if E and (key.min() < 0 or (key >= rows_of[cid]).any()):
                    raise IndexError(f'boundary_index of dimension {d}: a local index outside its complex')
                g = row0[cid] + key                                    # row number in packed order: sorted by complex already
                order = np.argsort(g, kind='stable')
                col = val[order].astype(np.int32)
                counts = np.bincount(g, minlength=int(rows_of.sum())).astype(np.int64)
                incl = np.cumsum(counts) - np.repeat(ent0, rows_of)    # local inclusive row pointers: rowptr[1:] of each complex
                dev = self.device
                self.keys[d][name + '_rowptr'] = _Packed(torch.from_numpy(incl.astype(np.int32)).to(dev), row0, rows_of,
                                                         rows_of > 0, 1, 1, _ffi.COLLATE_ADD32)
                self.keys[d][name + '_col'] = _Packed(torch.from_numpy(col).to(dev), ent0, lengths, lengths > 0, 1, 1,
                                                      _ffi.COLLATE_ADD32)

    def _finalise(self) -> None:
        """Per-complex metadata of every key stacked into matrices: a batch's tables are then a dozen numpy calls
        in all (the first form made ~100 small ones, 150 us of host time per batch of 128 -- four propagate
        steps)."""
        D = self.max_dim + 1
        if self.with_csr:
            self._add_csr_keys()
        self._klist = [(d, key, pk) for d in range(D) for key, pk in self.keys[d].items()]
        if self.y is not None:
            self._klist.append((-1, 'y', self.y))
        # one row per complex: [cells, down, up] of every dimension, then length / start / has of every key -- a
        # batch needs ONE gather of its rows
        cols = [np.stack([self.n_cells, self.n_down, self.n_up], axis=1).reshape(3 * D, self.num)]
        for f in ('length', 'start', 'has'):
            cols += [np.asarray(getattr(pk, f), dtype=np.int64)[None] for _, _, pk in self._klist]
        self._meta = np.ascontiguousarray(np.concatenate(cols, axis=0).T)                  # [num, 3D + 3K]
        self._meta_dev = None          # the same matrix in HBM (cwn_collate_tables: the tables of a batch built on the device)

    def meta_device(self) -> torch.Tensor:
        if self._meta_dev is None:
            self._meta_dev = torch.from_numpy(self._meta).to(self.device)
        return self._meta_dev

    def key_index(self, d: int, key: str) -> int:
        """Position of (dimension, key) in the table layout (the `k` of cwn_collate_tables), -1 when the dataset has no such array."""
        for k, (dd, kk, _) in enumerate(self._klist):
            if dd == d and kk == key:
                return k
        return -1

    # add-table of a key inside a dimension's block of five offset rows (here, here, down, here, up), in rows
    _ADD_ROW = {'upper_index': 0, 'lower_index': 0, 'shared_boundaries': 2, 'shared_coboundaries': 4, 'boundary_index': 2,
                _TARGET_KEY: 0}

    def _prepare(self, idx):
        """Host half of collate: output tensors (uninitialised), ONE int64 array holding every segment table, and
        the launch plan -- entries (packed or None, out, offset of dst_start [B + 1], offset of src_start [B] or None,
        offset of the add rows or None, total elements per row)."""
        idx = np.asarray(idx, dtype=np.int64)
        B = int(idx.size)
        if B == 0:
            raise ValueError('collate of an empty index list')
        dimension = int(self.dims[idx].max())
        dev = self.device
        D, K = self.max_dim + 1, len(self._klist)
        m = self._meta[idx]                                               # [B, 3D + 3K]
        cs = np.cumsum(m[:, :3 * D + K], axis=0)
        # running cell offsets of data/complex.py:148-169, all dimensions at once: [D, (here, down, up), B]
        cnt = np.ascontiguousarray(m[:, :3 * D].T).reshape(D, 3, B)
        end = np.ascontiguousarray(cs[:, :3 * D].T).reshape(D, 3, B)
        off = end - cnt
        tot = end[:, :, -1].tolist()
        dst = np.zeros((K, B + 1), dtype=np.int64)
        dst[:, 1:] = cs[:, 3 * D:].T
        totals = dst[:, -1].tolist()
        present = m[:, 3 * D + 2 * K:].any(axis=0).tolist()
        seg = np.concatenate([off[:, 0, :], end[:, 0, -1:]], axis=1)                   # [D, B + 1]: batch-vector segments
        o_src = K * (B + 1)
        o_off = o_src + K * B
        o_seg = o_off + D * 5 * B
        tables = np.concatenate([dst.reshape(-1), m[:, 3 * D + K:3 * D + 2 * K].T.reshape(-1),
                                 off[:, (0, 0, 1, 0, 2), :].reshape(-1), seg.reshape(-1)])
        plan = []
        cochains = [CochainBatch(d) for d in range(dimension + 1)]
        for cb in cochains:
            cb.__slices__ = {}
        y = None
        for k, (d, key, pk) in enumerate(self._klist):
            if d > dimension:
                continue
            total = totals[k]
            if d < 0:                       # the complexes' labels
                y = torch.empty(total, dtype=pk.data.dtype, device=dev)
                plan.append((pk, y, k * (B + 1), o_src + k * B, None, total))
                continue
            if not present[k] or key in _CSR_KEYS:
                continue                    # (the per-complex CSRs serve the static path: cwn_amd/static_graph.py)
            if key == 'x':
                out = torch.empty(total // pk.width, pk.width, dtype=pk.data.dtype, device=dev)
            elif pk.rows == 2:
                out = torch.empty(2, total, dtype=pk.data.dtype, device=dev)
            else:
                out = torch.empty(total, dtype=pk.data.dtype, device=dev)
            row = self._ADD_ROW.get(key)
            plan.append((pk, out, k * (B + 1), o_src + k * B, None if row is None else o_off + (d * 5 + row) * B, total))
            cb = cochains[d]
            if key == 'x':
                cb._x = out
            elif key == _TARGET_KEY:
                cb.target = out
            else:
                cb.__slices__[key] = dst[k].tolist()
                setattr(cb, key, out)
        for d, cb in enumerate(cochains):
            n_sel = cnt[d, 0]
            # the per-complex tables the reference's collate keeps (data/complex.py:344-441): the blocked layer
            # kernel's item table is cut from them (cwn_amd/blockplan.py)
            cb.__num_cells_list__ = n_sel.tolist()
            has = self.has_cells[d, idx]
            if has.any():
                # batch vector: complexes that have cells of this dimension, numbered by position
                out = torch.empty(tot[d][0], dtype=torch.int64, device=dev)
                plan.append((None, out, o_seg + d * (B + 1), None, None, tot[d][0]))
                cb.batch = out
                cb.ptr = [0] + np.cumsum(n_sel[has]).tolist()
            cb.__num_cells__ = tot[d][0]
            cb.__num_cells_up__ = tot[d][2]
            if d > 0:
                cb.__num_cells_down__ = tot[d][1]
            cb.__num_cochains__ = B
        return cochains, y, tables, plan

    def collate(self, idx: Sequence[int]) -> ComplexBatch:
        """The ComplexBatch of complexes `idx` (in that order), on the device."""
        cochains, y, tables, plan = self._prepare(idx)
        B = cochains[0].__num_cochains__
        dev = self.device
        # one H2D copy for every table, one launch for every array
        tab = torch.from_numpy(tables).to(dev, non_blocking=True)
        base = tab.data_ptr()
        descs = []
        for pk, out, o_dst, o_src, o_add, total in plan:
            if total == 0:
                continue
            if pk is None:
                descs.append(_ffi.CollateDesc(src=None, dst=out.data_ptr(), dst_start=base + 8 * o_dst,
                                              src_start=None, add=None, src_row_stride=0, dst_row_stride=0,
                                              n_rows=1, op=_ffi.COLLATE_SEGID64))
                continue
            descs.append(_ffi.CollateDesc(
                src=pk.data.data_ptr(), dst=out.data_ptr(), dst_start=base + 8 * o_dst,
                src_start=base + 8 * o_src, add=None if o_add is None else base + 8 * o_add,
                src_row_stride=pk.data.size(-1) if pk.rows == 2 else 0,
                dst_row_stride=total if pk.rows == 2 else 0, n_rows=pk.rows, op=pk.op))
        L = _ffi.lib()
        s = _ffi.stream_ptr(dev)
        for i in range(0, len(descs), _ffi.MAX_COLLATE_DESCS):
            chunk = descs[i:i + _ffi.MAX_COLLATE_DESCS]
            arr = (_ffi.CollateDesc * len(chunk))(*chunk)
            _ffi.check(L.cwn_collate(arr, len(chunk), B, s), 'cwn_collate')
        tab.record_stream(torch.cuda.current_stream(dev))
        for cb in cochains:
            # the reference's key, for code that takes `x[mask]` literally (RingSparseCIN reads `target`): three small launches
            # per batch (zeros, the int64 rows, index_fill_), no host work
            if cb.target is not None:
                cb.mask = torch.zeros(cb.__num_cells__, dtype=torch.bool, device=dev).index_fill_(0, cb.target.to(torch.long), True)
        batch = ComplexBatch(*cochains, y=y, num_complexes=B, dimension=len(cochains) - 1)
        batch._collate_tables = tab     # keep the tables alive until the launch has consumed them
        return batch

    def labels(self, idx: Sequence[int]) -> torch.Tensor:
        """The labels of the complexes `idx`, in that order: equal to `collate(idx).y`, as one gather from the packed `y`
        (the source positions come from the host's metadata: one small upload, no collate launch, no synchronisation)."""
        if self.y is None:
            raise ValueError('the packed complexes carry no labels')
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= self.num):
            raise IndexError(f'complex numbers outside 0 .. {self.num - 1}')
        pk = self.y
        ln, st = np.asarray(pk.length, dtype=np.int64)[idx], np.asarray(pk.start, dtype=np.int64)[idx]
        if ln.size and (ln == 1).all():
            src = st
        else:
            src = np.repeat(st, ln) + (np.arange(int(ln.sum()), dtype=np.int64) - np.repeat(np.cumsum(ln) - ln, ln))
        src_dev = torch.from_numpy(np.ascontiguousarray(src)).to(self.device, non_blocking=True)
        return pk.data.reshape(-1).index_select(0, src_dev)


class PackedLoader:
    """The reference's DataLoader (data/data_loading.py:84-111: `for batch in loader` of exp/train_utils.py:35)
    over an HBM-resident packed dataset: every batch is one `collate(indices)` launch on the device, no worker
    processes, no host collate.  `indices` selects a split (train / valid / test ids, data/datasets/dataset.py
    get_idx_split); `shuffle` draws a new permutation per epoch from `seed + epoch` (every rank draws the same one);
    with world > 1 rank r takes permutation entries r, r + world, ... of each GLOBAL batch -- the complexes of a
    batch shard across the ranks (cwn_amd/dist.py), and every rank sees the same number of batches (the tail that
    does not fill one complex per rank is dropped, as is an incomplete last batch with drop_last)."""

    def __init__(self, packed: PackedComplexes, batch_size: int = 1, shuffle: bool = False,
                 indices: Sequence[int] = None, drop_last: bool = False, seed: int = 0, rank: int = 0, world: int = 1):
        if batch_size < 1 or world < 1 or not (0 <= rank < world):
            raise ValueError('batch_size >= 1, world >= 1, 0 <= rank < world')
        self.packed, self.batch_size, self.shuffle, self.drop_last = packed, int(batch_size), shuffle, drop_last
        self.indices = np.arange(packed.num, dtype=np.int64) if indices is None else np.asarray(indices, dtype=np.int64)
        if self.indices.size and (self.indices.min() < 0 or self.indices.max() >= packed.num):
            raise IndexError('split index outside the dataset')
        self.seed, self.rank, self.world = int(seed), int(rank), int(world)
        self.epoch = 0

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def batches(self) -> List[np.ndarray]:
        """This rank's index lists for the current epoch."""
        order = self.indices
        if self.shuffle:
            order = order[np.random.default_rng(self.seed + self.epoch).permutation(order.size)]
        out = []
        for lo in range(0, order.size, self.batch_size):
            glob = order[lo:lo + self.batch_size]
            if glob.size < self.batch_size and self.drop_last:
                break
            if glob.size < self.world:          # not one complex per rank: a rank would sit out a collective
                break
            out.append(glob[self.rank::self.world])
        return out

    def __len__(self) -> int:
        n, b = self.indices.size, self.batch_size
        full, tail = divmod(n, b)
        return full + (1 if tail and not self.drop_last and tail >= self.world else 0) if b >= self.world else 0

    def __iter__(self):
        for idx in self.batches():
            yield self.packed.collate(idx)
        self.epoch += 1


# ------------------------------------------------------------------------------------------------------------------------------
# Cochains (the edge-flow experiments: a dataset of `Cochain`s of ONE dimension, batched by CochainBatch.from_cochain_list)
# ------------------------------------------------------------------------------------------------------------------------------
_COCHAIN_KEYS = ('x', 'y', 'upper_index', 'lower_index', 'upper_orient', 'lower_orient')
# Their offsets need the cell counts of OTHER dimensions (complex.py from_cochain_list: below / above), which a list of
# cochains of one dimension does not carry; `mask` needs the target machinery of PackedComplexes.  Out of scope here.
_COCHAIN_REFUSED = ('shared_boundaries', 'shared_coboundaries', 'boundary_index', 'mask')
_ORIENT_OF = {'upper_orient': 'upper_index', 'lower_orient': 'lower_index'}
_SLICE_KEYS = ('upper_index', 'lower_index', 'shared_boundaries', 'shared_coboundaries', 'boundary_index')   # complex.INDEX_KEYS


def cochain_meta(cochains) -> dict:
    """The numpy metadata of a list of cochains, after every check PackedCochains makes (no tensor leaves the host):
    `dim`; per cochain `n_cells` (0 without cells), `has_cells`, `n_up`, `n_down`; `keys` (those of _COCHAIN_KEYS some cochain
    carries) and per key `length` / `start` / `has` [len(keys), C] -- lengths and starts in elements of the packed array
    (x: rows * width, y: rows * its width, an index: columns, an orient: entries) -- and `width` of x and y."""
    if len(cochains) == 0:
        raise ValueError('PackedCochains needs at least one cochain')
    dim = cochains[0].dim
    C = len(cochains)
    width = {}
    for ci, c in enumerate(cochains):
        if c.dim != dim:
            raise ValueError(f'cochain {ci} has dim {c.dim}, cochain 0 has dim {dim}: a packed dataset holds cochains of one dimension')
        for key in _COCHAIN_REFUSED:
            if getattr(c, key, None) is not None:
                raise ValueError(f'cochain {ci} carries {key}: PackedCochains does not batch it (its offsets need the cells of '
                                 'another dimension, or the target rows of PackedComplexes); pack the complexes instead')
        x = c.x
        if x is not None:
            if x.dtype != torch.float32:
                raise TypeError(f'cochain {ci}: x is {x.dtype}, PackedCochains packs float32 features (the float64 path batches '
                                'on the host: CochainBatch.from_cochain_list)')
            if x.dim() != 2 or width.setdefault('x', int(x.size(1))) != int(x.size(1)):
                raise ValueError(f'cochain {ci}: x is {tuple(x.shape)}, a packed dataset holds [n, {width.get("x", "w")}] features')
        y = c.y
        if y is not None:
            if y.dtype not in (torch.float32, torch.int32, torch.int64):
                raise TypeError(f'cochain {ci}: y is {y.dtype} (float32 / int32 / int64 only)')
            tail = tuple(y.shape[1:])
            if width.setdefault('y_tail', tail) != tail or width.setdefault('y_dtype', y.dtype) != y.dtype:
                raise ValueError(f'cochain {ci}: y is {y.dtype} {tuple(y.shape)}, the others are {width["y_dtype"]} [.., '
                                 f'{width["y_tail"]}]')
        for key in ('upper_index', 'lower_index'):
            t = c[key]
            if t is not None and (t.dtype != torch.long or t.dim() != 2 or t.size(0) != 2):
                raise ValueError(f'cochain {ci}: {key} must be an int64 [2, e] tensor (got {t.dtype} {tuple(t.shape)})')
        for key, of in _ORIENT_OF.items():
            t, index = c[key], c[of]
            if t is None:
                continue
            if t.dtype != torch.float32 or t.dim() != 1:
                raise ValueError(f'cochain {ci}: {key} must be a float32 [e] vector (got {t.dtype} {tuple(t.shape)})')
            cols = 0 if index is None else int(index.size(1))
            if int(t.numel()) != cols:
                raise ValueError(f'cochain {ci}: {key} has {int(t.numel())} entries, {of} has {cols} columns: one orientation per '
                                 'adjacency entry')
    width['y'] = int(np.prod(width.pop('y_tail', ()), dtype=np.int64))
    width.pop('y_dtype', None)
    n_here = [c.num_cells for c in cochains]
    meta = dict(dim=dim, width=width,
                n_cells=np.array([n or 0 for n in n_here], dtype=np.int64), has_cells=np.array([n is not None for n in n_here], dtype=bool),
                # (the increments from_cochain_list takes without the shared keys: the counts a cochain was GIVEN)
                n_up=np.array([c.__num_cells_up__ or 0 for c in cochains], dtype=np.int64),
                n_down=np.array([(c.__num_cells_down__ or 0) if dim > 0 else 0 for c in cochains], dtype=np.int64))
    keys = tuple(k for k in _COCHAIN_KEYS if any(c[k] is not None for c in cochains))
    length = np.zeros((len(keys), C), dtype=np.int64)
    for ki, key in enumerate(keys):
        for ci, c in enumerate(cochains):
            t = c[key]
            if t is None:
                continue
            if key == 'x':
                length[ki, ci] = int(t.size(0)) * width['x']
            elif key == 'y':
                length[ki, ci] = (1 if t.dim() == 0 else int(t.size(0))) * width['y']
            else:
                length[ki, ci] = int(t.size(-1))
    meta.update(keys=keys, length=length, start=np.cumsum(length, axis=1) - length,
                has=np.array([[c[k] is not None for c in cochains] for k in keys], dtype=bool).reshape(len(keys), C))
    return meta


def cochain_tables(meta: dict, idx) -> dict:
    """The segment tables of the batch of cochains `idx` (in that order) -- numpy in, numpy out, nothing touches a device:
      cells [B], cell_off [B] (the running cell offset the index values shift by), seg [B + 1] (cell_off and the total: the
      segments of the batch vector; a cochain without cells is an empty one), ptr ([0] + the running cell count over the
      cochains that HAVE cells, or None when none has), num_cells / num_cells_up / num_cells_down, num_cells_list (None for
      a cochain without cells), dst[key] [B + 1] / src[key] [B] / present[key] for every packed key (element offsets in the
      batched and in the packed array) and slices[key] for the five index keys of the reference's `__slices__`."""
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    B = int(idx.size)
    if B == 0:
        raise ValueError('collate of an empty index list')
    C = int(meta['n_cells'].size)
    if idx.min() < 0 or idx.max() >= C:
        raise IndexError(f'cochain numbers outside 0 .. {C - 1}')
    cells, has_cells = meta['n_cells'][idx], meta['has_cells'][idx]
    seg = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(cells, out=seg[1:])
    out = dict(B=B, cells=cells, cell_off=seg[:-1], seg=seg, num_cells=int(seg[-1]), num_cells_up=int(meta['n_up'][idx].sum()),
               num_cells_down=int(meta['n_down'][idx].sum()) if meta['dim'] > 0 else None,
               num_cells_list=[int(n) if h else None for n, h in zip(cells.tolist(), has_cells.tolist())],
               ptr=np.concatenate([[0], np.cumsum(cells[has_cells])]).astype(np.int64) if has_cells.any() else None,
               dst={}, src={}, present={}, slices={k: [0] * (B + 1) for k in _SLICE_KEYS})
    for ki, key in enumerate(meta['keys']):
        dst = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(meta['length'][ki, idx], out=dst[1:])
        out['dst'][key], out['src'][key] = dst, meta['start'][ki, idx]
        out['present'][key] = bool(meta['has'][ki, idx].any())
        if key in out['slices']:
            out['slices'][key] = dst.tolist()
    return out


EPOCH_COUNTS = ('rows', 'upper_index', 'lower_index', 'cochains')     # the live counts at the end of an epoch-table row


def cochain_epoch_layout(meta: dict, B: int) -> dict:
    """Where every table of a batch of at most B cochains sits in one row of the epoch tables (`cochain_epoch_tables`): name ->
    offset in int64 elements, and 'len' (a multiple of 2: rows stay 16-byte aligned).  Per packed key `dst_<key>` [B + 1] and
    `src_<key>` [B]; `cell_off` [2 B] (both rows of an index); `seg` [B + 1] (the batch vector's segments = the head's `ptr`);
    `row0` [B] (first cell of every cochain in packed order), `one_dst` [B + 1] and `zero_src` [B] (a plan's leading zero);
    `counts` [8]: EPOCH_COUNTS, then zeros."""
    off, run = {}, 0
    for name, n in ([(p + key, B + (p == 'dst_')) for key in meta['keys'] for p in ('dst_', 'src_')]
                    + [('cell_off', 2 * B), ('seg', B + 1), ('row0', B), ('one_dst', B + 1), ('zero_src', B), ('counts', 8)]):
        off[name] = run
        run += n
    off['len'] = run + (run & 1)
    return off


def cochain_epoch_tables(meta: dict, batches, B: int) -> np.ndarray:
    """int64 [len(batches), layout['len']]: row j holds `cochain_tables(meta, batches[j])` in the layout above, written for a
    batch of CAPACITY B -- the places of the cochains a shorter batch does not have are empty segments behind the last one
    (dst / seg / cell_off repeat the total, src / row0 are 0), so that a collate over B segments copies nothing for them.
    numpy in, numpy out: one array per epoch, one H2D copy."""
    lay = cochain_epoch_layout(meta, B)
    row0 = np.cumsum(meta['n_cells']) - meta['n_cells']
    out = np.zeros((len(batches), lay['len']), dtype=np.int64)
    for j, idx in enumerate(batches):
        t = cochain_tables(meta, idx)
        b, r = t['B'], out[j]
        if b > B:
            raise ValueError(f'batch {j}: {b} cochains exceed the capacity {B}')
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        for key in meta['keys']:
            o = lay['dst_' + key]
            r[o:o + b + 1], r[o + b + 1:o + B + 1] = t['dst'][key], t['dst'][key][-1]
            r[lay['src_' + key]:lay['src_' + key] + b] = t['src'][key]
        for o in (lay['cell_off'], lay['cell_off'] + B):
            r[o:o + b], r[o + b:o + B] = t['cell_off'], t['num_cells']
        o = lay['seg']
        r[o:o + b + 1], r[o + b + 1:o + B + 1] = t['seg'], t['num_cells']
        r[lay['row0']:lay['row0'] + b] = row0[idx]
        r[lay['one_dst'] + 1:lay['one_dst'] + B + 1] = 1
        c = lay['counts']
        r[c:c + 4] = [t['num_cells']] + [int(t['dst'][k][-1]) if k in t['dst'] else 0 for k in ('upper_index', 'lower_index')] + [b]
    return out


class PackedCochains:
    """A dataset of `Cochain`s (CPU tensors, one `dim`) packed on `device`; `collate(idx)` is the CochainBatch
    `CochainBatch.from_cochain_list([cochains[i] for i in idx]).to(device)` would be, field for field, from ONE small H2D
    copy of the segment tables (`cochain_tables`) and ONE cwn_collate launch.  The batch also carries `ptr_dev`: int64
    [B + 1] on the device, the first row of every cochain by its place in the batch and the row total -- `ptr` itself when
    every cochain has cells -- which ops.flow_head reads.

    `with_csr`: the destination-sorted CSR of every cochain's upper and lower adjacency and of their source-keyed
    transposes is built ONCE here (cwn_csr_build over the block-diagonal index of the whole dataset, cut at the cochains,
    local numbers).  A batch is block-diagonal and per-cochain contiguous, so its plans are the concatenations: `col` and
    `perm` collate as ADD32 with the cell and the entry offset, `rowptr` without its leading zero plus the running entry
    count (the scheme of PackedComplexes' boundary CSRs), all in the same launch.  The batch's index tensors are then
    registered with their built `csr.Adjacency` (and `_t_src`) where OrientedConv looks plans up: no cwn_csr_build per
    batch, forward or backward.  Long-row lists: none when no row of the dataset exceeds csr.LONG_ROW, else filled by
    cwn_csr_long_rows over the collated row pointers (one more launch)."""

    def __init__(self, cochains, device, with_csr: bool = True):
        self.meta = cochain_meta(cochains)
        self.device = torch.device(device)
        self.with_csr = bool(with_csr)
        self.num = len(cochains)
        self.dim = self.meta['dim']
        self.epoch = 0
        m = self.meta
        self._packs = {}
        for ki, key in enumerate(m['keys']):
            present = [c[key] for c in cochains if c[key] is not None]
            if key in ('x', 'y'):
                data = torch.cat([t.reshape(-1) for t in present])
            else:
                data = torch.cat(present, dim=-1)
            rows = 2 if key in ('upper_index', 'lower_index') else 1
            op = _ffi.COLLATE_ADD64 if rows == 2 else (_ffi.COLLATE_COPY64 if data.dtype == torch.int64 else _ffi.COLLATE_COPY32)
            self._packs[key] = _Packed(data.contiguous().to(self.device), m['start'][ki], m['length'][ki], m['has'][ki], rows,
                                       m['width'].get(key, 1), op)
        self._y_tail = tuple(next(c.y for c in cochains if c.y is not None).shape[1:]) if 'y' in self._packs else ()
        self._row0 = np.cumsum(m['n_cells']) - m['n_cells']           # first cell of every cochain in packed order
        self._csr = {}               # 'upper_index' / 'lower_index' -> ((rowptr, col, perm), the same of the transpose), local
        self.has_long_rows = False
        if self.with_csr:
            self._build_csr()

    def _build_csr(self) -> None:
        from .csr import LONG_ROW, Adjacency
        dev, C = self.device, self.num
        n = torch.from_numpy(self.meta['n_cells']).to(dev)
        row0 = torch.from_numpy(self._row0).to(dev)
        total = int(self.meta['n_cells'].sum())
        self._zero = torch.zeros(1, dtype=torch.int32, device=dev)     # a plan's rowptr[0]
        for key in ('upper_index', 'lower_index'):
            pk = self._packs.get(key)
            if pk is None:
                continue
            E = int(pk.data.size(1))
            if E >= 2 ** 31 - 1 or total >= 2 ** 31 - 1:
                raise ValueError(f'{key}: {E} entries over {total} cells do not fit the int32 plans; pack the dataset in parts')
            cid = torch.repeat_interleave(torch.arange(C, device=dev), torch.from_numpy(np.asarray(pk.length)).to(dev), output_size=E)
            ent0 = torch.from_numpy(np.asarray(pk.start)).to(dev)
            if E and bool(((pk.data < 0) | (pk.data >= n[cid])).any()):
                raise IndexError(f'{key}: a local index outside its cochain')
            adj = Adjacency.from_index((pk.data + row0[cid]).contiguous(), total, total)
            local = []
            for a in (adj, adj.t_src):
                rp = a.rowptr.long()
                self.has_long_rows = self.has_long_rows or bool(((rp[1:] - rp[:-1]) > LONG_ROW).any())
                local.append(((rp[1:] - torch.repeat_interleave(ent0, n, output_size=total)).to(torch.int32),
                              (a.col.long() - row0[cid]).to(torch.int32), (a.perm.long() - ent0[cid]).to(torch.int32)))
            self._csr[key] = tuple(local)

    # --------------------------------------------------------------------------------------------
    def collate(self, idx: Sequence[int]) -> CochainBatch:
        """The CochainBatch of the cochains `idx` (in that order), on the device."""
        from . import csr
        t = cochain_tables(self.meta, idx)
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        B, dev, n = t['B'], self.device, t['num_cells']
        keys = self.meta['keys']
        # ONE int64 array: per key dst [B + 1] and src [B]; the cell offsets twice (both rows of an index); the batch
        # vector's segments; every cochain's first cell in packed order; the tables of the plans' leading zero
        parts, off, run = [], {}, 0

        def put(name, a):
            nonlocal run
            off[name] = run
            parts.append(np.asarray(a, dtype=np.int64).reshape(-1))
            run += parts[-1].size
        for key in keys:
            put('dst_' + key, t['dst'][key])
            put('src_' + key, t['src'][key])
        put('cell_off', np.concatenate([t['cell_off'], t['cell_off']]))
        put('seg', t['seg'])
        if self._csr:
            put('row0', self._row0[idx])
            put('one_dst', np.concatenate([[0], np.ones(B, dtype=np.int64)]))
            put('zero_src', np.zeros(B, dtype=np.int64))
        tab = torch.from_numpy(np.concatenate(parts)).to(dev, non_blocking=True)
        base = tab.data_ptr()
        at = lambda name: base + 8 * off[name]
        out = CochainBatch(self.dim)
        descs = []
        for key in keys:
            pk, total = self._packs[key], int(t['dst'][key][-1])
            if not t['present'][key]:
                continue                      # (no cochain of the batch has it: the attribute stays None, as on the host)
            if key == 'x':
                val = torch.empty(total // pk.width, pk.width, dtype=pk.data.dtype, device=dev)
            elif key == 'y':
                val = torch.empty((total // max(pk.width, 1),) + self._y_tail, dtype=pk.data.dtype, device=dev)
            elif pk.rows == 2:
                val = torch.empty(2, total, dtype=pk.data.dtype, device=dev)
            else:
                val = torch.empty(total, dtype=pk.data.dtype, device=dev)
            if key == 'x':
                out._x = val
            else:
                setattr(out, key, val)
            if total:
                descs.append(_ffi.CollateDesc(src=pk.data.data_ptr(), dst=val.data_ptr(), dst_start=at('dst_' + key), src_start=at('src_' + key),
                                              add=at('cell_off') if pk.rows == 2 else None,
                                              src_row_stride=pk.data.size(-1) if pk.rows == 2 else 0,
                                              dst_row_stride=total if pk.rows == 2 else 0, n_rows=pk.rows, op=pk.op))
        if t['ptr'] is not None:
            out.batch = torch.empty(n, dtype=torch.int64, device=dev)
            out.ptr = t['ptr'].tolist()
            if n:
                descs.append(_ffi.CollateDesc(src=None, dst=out.batch.data_ptr(), dst_start=at('seg'), src_start=None, add=None,
                                              src_row_stride=0, dst_row_stride=0, n_rows=1, op=_ffi.COLLATE_SEGID64))
        plans = []
        for key, local in self._csr.items():
            index = getattr(out, key, None)
            if index is None:
                continue
            adj = csr.Adjacency(index[1], index[0], n, n)
            adj.transposes()
            E = adj.n_entries
            for a, (rp, col, perm) in zip((adj, adj._t_src), local):
                if not self.has_long_rows:
                    a.long_rows = a.n_long = None              # (known at construction: nothing to list, nothing to zero)
                one = lambda src, dst, dst_start, src_start, add: _ffi.CollateDesc(
                    src=src.data_ptr(), dst=dst, dst_start=at(dst_start), src_start=at(src_start), add=None if add is None else at(add),
                    src_row_stride=0, dst_row_stride=0, n_rows=1, op=_ffi.COLLATE_COPY32 if add is None else _ffi.COLLATE_ADD32)
                descs.append(one(self._zero, a.rowptr.data_ptr(), 'one_dst', 'zero_src', None))
                if n:                         # rowptr[1:]: a cochain's inclusive local pointers + the entries in front of it
                    descs.append(one(rp, a.rowptr.data_ptr() + 4, 'seg', 'row0', 'dst_' + key))
                if E:
                    descs.append(one(col, a.col.data_ptr(), 'dst_' + key, 'src_' + key, 'cell_off'))
                    descs.append(one(perm, a.perm.data_ptr(), 'dst_' + key, 'src_' + key, 'dst_' + key))
                a.built = True
                plans.append(a)
            csr.register_adjacency(index, adj)             # (held by the plan cache for as long as the index tensor lives)
        L = _ffi.lib()
        s = _ffi.stream_ptr(dev)
        for i in range(0, len(descs), _ffi.MAX_COLLATE_DESCS):        # (23 descriptors at most: one launch)
            chunk = descs[i:i + _ffi.MAX_COLLATE_DESCS]
            _ffi.check(L.cwn_collate((_ffi.CollateDesc * len(chunk))(*chunk), len(chunk), B, s), 'cwn_collate')
        if self.has_long_rows:
            todo = [a for a in plans if a.long_rows is not None]
            if todo:
                arr = (_ffi.LongRowsDesc * len(todo))(*[
                    _ffi.LongRowsDesc(rowptr=a.rowptr.data_ptr(), n_rows=a.n_dst, m_dev=None, long_rows=a.long_rows.data_ptr(),
                                      n_long=a.n_long.data_ptr(), long_cap=a.long_cap) for a in todo])
                _ffi.check(L.cwn_csr_long_rows(arr, len(todo), s), 'cwn_csr_long_rows')
        tab.record_stream(torch.cuda.current_stream(dev))
        out.ptr_dev = tab[off['seg']:off['seg'] + B + 1]
        out._collate_tables = tab           # keep the tables alive until the launch has consumed them
        out.__num_cochains__ = B
        out.__num_cells__ = n
        out.__num_cells_up__ = t['num_cells_up']
        if self.dim > 0:
            out.__num_cells_down__ = t['num_cells_down']
        out.__num_cells_list__ = t['num_cells_list']
        out.__slices__ = t['slices']
        return out

    def labels(self, idx: Sequence[int]) -> torch.Tensor:
        """The labels of the cochains `idx`, in that order: equal to `collate(idx).y`, as one gather from the packed `y`
        (source positions from the host's metadata: one small upload, no collate launch, no synchronisation)."""
        pk = self._packs.get('y')
        if pk is None:
            raise ValueError('the packed cochains carry no labels')
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= self.num):
            raise IndexError(f'cochain numbers outside 0 .. {self.num - 1}')
        ln, st = np.asarray(pk.length, dtype=np.int64)[idx], np.asarray(pk.start, dtype=np.int64)[idx]
        src = np.repeat(st, ln) + (np.arange(int(ln.sum()), dtype=np.int64) - np.repeat(np.cumsum(ln) - ln, ln))
        src_dev = torch.from_numpy(np.ascontiguousarray(src)).to(self.device, non_blocking=True)
        return pk.data.index_select(0, src_dev).reshape((-1,) + self._y_tail)

    # --------------------------------------------------------------------------------------------
    def batch_indices(self, batch_size: int, shuffle: bool = False, seed: int = 0, drop_last: bool = False,
                      epoch: int = 0) -> List[np.ndarray]:
        """The index lists of one epoch: the cochains in order, or (`shuffle`) in the permutation drawn from `seed + epoch`."""
        if batch_size < 1:
            raise ValueError('batch_size >= 1')
        order = np.arange(self.num, dtype=np.int64)
        if shuffle:
            order = np.random.default_rng(int(seed) + int(epoch)).permutation(self.num).astype(np.int64)
        out = [order[lo:lo + batch_size] for lo in range(0, self.num, batch_size)]
        return out[:-1] if drop_last and out and out[-1].size < batch_size else out

    def batches(self, batch_size: int, shuffle: bool = False, seed: int = 0, drop_last: bool = False):
        """One epoch of collated batches (the reference's `for batch in loader`): every batch one `collate` on the device, a
        freshly drawn permutation per epoch -- `self.epoch` counts the epochs begun and moves with every call."""
        epoch, self.epoch = self.epoch, self.epoch + 1
        for idx in self.batch_indices(batch_size, shuffle, seed, drop_last, epoch):
            yield self.collate(idx)


class CochainForward:
    """A model over a packed cochain dataset in the form evaluate.evaluate / evaluate.infer take as `forward`: `batches` are
    the index arrays of the pass (PackedCochains.batch_indices), every batch is one `collate` and one eager forward, and the
    labels come from `labels(idx)` -- one gather, no collate."""

    def __init__(self, model, packed_cochains: PackedCochains):
        self.model, self.packed = model, packed_cochains
        self.sb = self                       # (evaluate reads the dataset as forward.sb.packed)

    def run_epoch(self, batches) -> List[torch.Tensor]:
        return [self.model(self.packed.collate(idx)) for idx in batches]
