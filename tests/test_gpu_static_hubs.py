"""Hub rows through the COLLATED plans of a csr-mode static batch, by value.

A csr-mode StaticBatch takes every boundary adjacency and its TRANSPOSE from the collate launch, not from cwn_csr_build.  The
transposed plan has hub rows (a vertex of degree 200 is the boundary of 200 edges), and cwn_aggregate_f32 / _f64, handed
long-row lists, leaves every row above CWN_LONG_ROW to them: a list that the fill which wrote the row pointers has not written
drops those rows.  tests/test_gpu_static_csr.py checks the lists; here a VALUE computed through every collated plan is compared
with a float64 index_add_ on the CPU over the entries of the collated batch of the same complexes -- integer features, so
every sum is exact in any order and the comparison is torch.equal, outputs pre-filled with NaN so that a row nobody wrote is
seen with certainty -- and the readers of those plans are run at model level: an inference forward with a co-boundary stream,
a routed forward, an autograd backward outside StaticTrainStep.  Last, capacities that coincide with a model width: the
device-side row count is found by VALUE (_ffi.dynamic_rows), and B = hidden is the most common real configuration."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
W_IN = 64                  # width of the pool's own features (the models below take them as they are)
LONG = 64                  # = CWN_LONG_ROW


# ---- the pool: hand-built complexes, a few hundred cells each at most ------------------------------------------------------
def _star(k):
    """Hub 0 with k leaves and ONE triangle (0, 1, 2): the hub's row of the transposed edge -> vertex plan has k entries."""
    return k + 1, [(0, i) for i in range(1, k + 1)] + [(1, 2)]


def _book(k):
    """k triangles on the spine (0, 1): the spine's row of the transposed triangle -> edge plan has k entries, the rows of
    the vertices 0 and 1 of the edge -> vertex plan k + 1."""
    return k + 2, [(0, 1)] + [(a, i) for i in range(2, k + 2) for a in (0, 1)]


def _bipartite(a, b):
    """K(a, b): every vertex row of the transposed plan is as long as the other side; no triangle."""
    return a + b, [(i, a + j) for i in range(a) for j in range(b)]


def _path(n):
    return n, [(i, i + 1) for i in range(n - 1)]


def _triangle_tail(n):
    return n, [(0, 1), (0, 2), (1, 2)] + [(i, i + 1) for i in range(2, n - 1)]


NAMES = ['s63', 's64', 's65', 's66', 's129', 's200', 'k65', 'book64', 'book65', 'path5', 'path7', 'path10', 'tri3', 'tri6', 'path6', 'path8']
_SHAPES = {'k65': lambda: _bipartite(65, 65), 'book64': lambda: _book(64), 'book65': lambda: _book(65), 'tri3': lambda: _triangle_tail(3),
           'tri6': lambda: _triangle_tail(6)}
_pool_cache = {}


def _pool():
    """(complexes, PackedComplexes): features are integers in [-4, 4] (the higher cells' their vertices' sums)."""
    if 'p' not in _pool_cache:
        from cwn_amd.packed import PackedComplexes
        from cwn_amd.synthetic import clique_lift
        g = torch.Generator().manual_seed(5)
        pool = []
        for k, name in enumerate(NAMES):
            if name in _SHAPES:
                n, edges = _SHAPES[name]()
            else:
                n, edges = (_star if name[0] == 's' else _path)(int(name.lstrip('spath')))
            vx = torch.randint(-4, 5, (n, W_IN), generator=g).float()
            pool.append(clique_lift(n, edges, vx, max_dim=2, init_method='sum', y=torch.tensor([k % 2])))
        _pool_cache['p'] = (pool, PackedComplexes(pool, DEV, max_dim=2, with_csr=True))
    return _pool_cache['p']


def _ids(*names):
    return np.array([NAMES.index(n) for n in names], dtype=np.int64)


def _collated(idx):
    """The host copy of the boundary indices and the cell counts of PackedComplexes.collate(idx): computed once per index
    list, shared by the tests, never written."""
    key = ('c',) + tuple(int(i) for i in idx)
    if key not in _pool_cache:
        ref = _pool()[1].collate(idx)
        _pool_cache[key] = ([ref.cochains[d].num_cells for d in range(3)],
                            [None] + [ref.cochains[d].boundary_index.cpu() for d in (1, 2)])
    return _pool_cache[key]


# the two fills of part 1.  A: a hub complex in the LAST position of slot 0, a short batch without one in slot 1, slot 2
# empty.  B: the reverse in slots 0 / 1 (the lists must describe this fill, not the one before), K(65, 65) -- every vertex row
# long -- in slot 1, slot 2 full.  Every hub degree -- both sides of CWN_LONG_ROW, beyond two chunks per lane group -- is in one of them: 63 (B1), 64 (A0, B2), 65 (A0), 66 (B2),
# 129 (B2), 200 (B1).
FILL_A = [('s64', 'book64', 'book65', 's65'), ('tri3', 'tri6')]
FILL_B = [('tri6', 'path10', 'tri3'), ('s63', 'k65', 'book65', 's200'), ('s66', 's129', 's64', 'book64')]


def _reference(bi, key_row, n_rows, A, B, reduce):
    """out[i] = reduce over the entries e with bi[key_row, e] == i of A[j] (* B[j]), j = bi[1 - key_row, e]: float64, CPU."""
    dst, src = bi[key_row], bi[1 - key_row]
    m = A[src] if B is None else A[src] * B[src]
    cnt = torch.bincount(dst, minlength=n_rows)
    if reduce == 'max':
        out = torch.full((n_rows, m.size(1)), float('-inf'), dtype=torch.float64).scatter_reduce_(0, dst[:, None].expand_as(m), m, 'amax')
        return torch.where((cnt > 0)[:, None], out, torch.zeros_like(out))
    out = torch.zeros(n_rows, m.size(1), dtype=torch.float64).index_add_(0, dst, m)
    return out / cnt.clamp(min=1)[:, None].double() if reduce == 'mean' else out


def _check_fill(sb, fill, F, dtype, what):
    """Every collated plan of every slot, five (message, reduce) forms each, against the float64 reference; the rows the test
    is about asserted from the host copy of the row pointers; the long-row lists against those row pointers."""
    from cwn_amd import _ffi, csr, ops
    from cwn_amd.static_batch import _CollatedAdjacency
    g = torch.Generator().manual_seed(11)
    forms = [(ops.MSG_A, 'add'), (ops.MSG_A, 'mean'), (ops.MSG_A, 'max'), (ops.MSG_A_TIMES_B, 'add'), (ops.MSG_A_TIMES_B, 'max')]
    seen = {1: set(), 2: set()}                 # row lengths of the TRANSPOSED plans over the live rows, per dimension

    def plans():
        """(slot number, slot, names, dimension, plan, key row, live rows, host entries or None) of every collated plan"""
        for j, slot in enumerate(sb.slots):
            names = fill[j] if j < len(fill) else ()
            sizes = slot.sizes()
            if not names:
                assert sizes == [0, 0, 0, 0], (what, j, sizes)
                bis = None
            else:
                n_cells, bis = _collated(_ids(*names))
                assert sizes == n_cells + [len(names)], (what, j, sizes, n_cells)
            for d in (1, 2):
                bi_dev = slot.batch.cochains[d].boundary_index
                adj = csr.cached_adjacency(bi_dev, sb.cap_cells[d], sb.cap_cells[d - 1], build=False)
                assert isinstance(adj, _CollatedAdjacency) and isinstance(adj._t_src, _CollatedAdjacency), (what, j, d)
                for plan, key_row, row_dim in ((adj, 1, d), (adj._t_src, 0, d - 1)):
                    yield j, slot, names, d, plan, key_row, sizes[row_dim], None if bis is None else bis[d]

    # first: the rows this test is about are in the plans the kernel will read -- at the threshold and beyond it, in both
    # transposed plans -- from the host copy of the row pointers over the live rows
    for j, slot, names, d, plan, key_row, rows, bi in plans():
        if not names:
            continue
        lens = torch.bincount(bi[key_row], minlength=rows)
        rp = plan.rowptr.cpu().long()[:rows + 1]
        assert torch.equal(rp[1:] - rp[:-1], lens), (what, j, d, key_row)
        if key_row == 0:
            seen[d].update(lens.tolist())
    for d in (1, 2):
        assert LONG in seen[d] and max(seen[d]) > LONG, (what, d, sorted(seen[d])[-4:])
    # then the values, and the lists the plans carry
    for j, slot, names, d, plan, key_row, rows, bi in plans():
        A = torch.randint(-4, 5, (plan.n_val, F), generator=g).to(dtype)
        B = torch.randint(-4, 5, (plan.n_val, F), generator=g).to(dtype)
        Ad, Bd = A.to(DEV), B.to(DEV)
        specs = [ops.AggSpec(adj=plan, n_dst=plan.n_dst, F=F, A=Ad, ia=plan.col, msg_op=op, reduce=_ffi.REDUCE[red],
                             B=None if op == ops.MSG_A else Bd, ib=None if op == ops.MSG_A else plan.col,
                             out=torch.full((plan.n_dst, F), float('nan'), dtype=dtype, device=DEV)) for op, red in forms]
        with slot.dynamic():
            outs = ops.run_aggregate(specs, DEV)
        if not names:
            continue                    # (an empty slot: no live row, nothing is written by contract)
        lens = torch.bincount(bi[key_row], minlength=rows)
        for (op, red), out in zip(forms, outs):
            want = _reference(bi, key_row, rows, A.double(), None if op == ops.MSG_A else B.double(), red).to(dtype)
            live = out[:rows].cpu()
            bad = torch.nonzero((live != want).any(1)).view(-1)
            assert torch.equal(live, want), (what, j, d, 'transposed' if key_row == 0 else 'plan', op, red,
                                             f'{bad.numel()} rows differ, the first {bad[:4].tolist()} of lengths {lens[bad[:4]].tolist()}, '
                                             f'NaN in {int(torch.isnan(live).any(1).sum())} rows')
        if key_row == 0:
            n_long = int((lens > LONG).sum())
            if plan.long_rows is not None:      # the lists on the plan are those of THIS fill
                nl = plan.n_long.cpu().tolist()
                got = sorted(plan.long_rows[0, :nl[0]].cpu().tolist())
                assert sum(nl[1:]) == 0 and got == torch.nonzero(lens > LONG).view(-1).tolist(), (what, j, d, nl, n_long)
                assert n_long <= plan.long_cap
            if 'k65' in names and d == 1:
                print(f'[hubs] {what}: slot {j}: {n_long} long rows of {rows}, long_cap {plan.long_cap}')
                assert n_long >= 130 and 4 * n_long >= 3 * plan.long_cap         # every vertex row of K(65, 65): near the capacity
    return seen


def _static(B=4, S=3):
    from cwn_amd.static_batch import StaticBatch
    pool, p = _pool()
    sb = StaticBatch(p, B, slots=S, mode='csr')
    fills = [[_ids(*names) for names in fill] for fill in (FILL_A, FILL_B)]
    assert all(bool(sb.fits(f).all()) for f in fills)
    return sb, fills


# ---- 1. aggregation through every collated plan, exactly -------------------------------------------------------------------
@pytest.mark.parametrize('F', [3, 64])
@pytest.mark.parametrize('build_backward', [False, True])
def test_aggregate_through_every_collated_plan_is_exact(build_backward, F):
    """Boundary plan and transposed plan of both dimensions of every slot after a fill, with and without the flag a training
    step sets; then ANOTHER fill that swaps the hub complexes between the slots.  F = 3: the lanes of a row split its entries
    (rows above 16 entries at F <= 14); F = 64: one lane per column."""
    from cwn_amd import csr
    sb, fills = _static()
    sb.build_backward = build_backward
    all_seen = set()
    for fill, ids, tag in ((FILL_A, fills[0], 'A'), (FILL_B, fills[1], 'B')):
        sb.set_batches(ids)
        sb.fill()
        seen = _check_fill(sb, fill, F, torch.float32, f'build_backward={build_backward} F={F} fill {tag}')
        all_seen |= seen[1]
    torch.cuda.synchronize()
    csr.check_errors(DEV)
    assert {63, 64, 65, 66, 129, 200} <= all_seen


def test_aggregate_through_every_collated_plan_is_exact_in_float64():
    """cwn_aggregate_f64 shares the body: the same check once, without the training step's flag."""
    from cwn_amd import csr
    sb, fills = _static()
    for fill, ids, tag in ((FILL_A, fills[0], 'A'), (FILL_B, fills[1], 'B')):
        sb.set_batches(ids)
        sb.fill()
        _check_fill(sb, fill, 8, torch.float64, f'float64 fill {tag}')
    torch.cuda.synchronize()
    csr.check_errors(DEV)


# ---- 2. the readers, at model level ----------------------------------------------------------------------------------------
def _hub_rows_present(sb, j, what):
    """From the host copy of slot j's transposed edge -> vertex plan: a row above CWN_LONG_ROW is among its live rows."""
    from cwn_amd import csr
    bi = sb.slots[j].batch.cochains[1].boundary_index
    t = csr.cached_adjacency(bi, sb.cap_cells[1], sb.cap_cells[0], build=False)._t_src
    n = sb.slots[j].sizes()[0]
    rp = t.rowptr.cpu().long()[:n + 1]
    lens = rp[1:] - rp[:-1]
    assert n > 0 and int(lens.max()) > LONG, (what, j, n)
    return lens


def _scaled(model):
    with torch.no_grad():
        for q in model.parameters():
            q.mul_(0.3)              # (degrees in the hundreds: keep the activations small, as the reddit-like tests do)
    return model


def _cinpp_with_coboundary_stream(layers=2, hidden=64):
    """Two CINppConv layers built as tests/test_gpu_parity.py::test_cinpp_with_a_real_lower_stream_and_coboundary_stream builds
    its layer (use_coboundaries, feed_down_attr, coboundary_stream: four streams, the fourth through the transposed boundary
    plan) inside the SparseCIN stack, whose sum readout + head is the one a static batch serves (the stack asks its layers
    for include_down_features=False and the pool has no lower adjacency: the lower stream is its self term)."""
    from cwn_amd import layers as Lm
    from cwn_amd.models import SparseCIN

    class HubCINpp(SparseCIN):
        def _make_conv(self, layer_dim, hidden, act_module, train_eps, use_coboundaries):
            return Lm.CINppConv(layer_dim, layer_dim, layer_dim, None, None, None, None, None, None, max_dim=self.max_dim,
                                hidden=hidden, act_module=act_module, layer_dim=layer_dim, use_coboundaries=True,
                                feed_down_attr=True, coboundary_stream=True, graph_norm=self.graph_norm)

    torch.manual_seed(1)
    m = HubCINpp(W_IN, 2, layers, hidden, dropout_rate=0.0, max_dim=2, jump_mode='cat', readout='sum', use_coboundaries=True,
                 graph_norm='bn').to(DEV)
    assert all(lvl.update_coboundaries_nn is not None for conv in m.convs for lvl in conv.mp_levels)
    return _scaled(m).eval()


EPOCH = [('s64', 'book64', 'book65', 's65'), ('s63', 'k65', 'book65', 's200'), ('s66', 's129', 'tri6'), ('path5', 's200', 'path7', 's64')]


def test_static_forward_with_a_coboundary_stream_over_hub_complexes_is_bit_identical_to_per_batch_launches():
    """The inference reader: the co-boundary stream of CIN++ aggregates the cofaces' features through the transposed boundary
    plan, which on a csr-mode static batch is the collated one.  StaticForward over hub complexes, two replays of two slots,
    a short batch among them, against model(collate) of the same complexes: torch.equal, the standard of
    test_static_forward_on_reddit_like_batches_is_bit_identical_to_per_batch_launches."""
    from cwn_amd import csr
    from cwn_amd.static_batch import StaticBatch
    from cwn_amd.static_graph import StaticForward
    pool, p = _pool()
    model = _cinpp_with_coboundary_stream()
    S = 2
    sb = StaticBatch(p, 4, slots=S, mode='csr')
    epoch = [_ids(*names) for names in EPOCH]
    assert sb.fits(epoch).all()
    sf = StaticForward(model, sb)
    sb.set_epoch(epoch)
    with torch.no_grad():
        for r in range(2):
            outs = [o.clone() for o in sf.replay()]
            for j in range(S):
                idx = epoch[r * S + j]
                _hub_rows_present(sb, j, ('forward', r))
                want = model(p.collate(idx))
                got = outs[j][:len(idx)]
                print(f'[hubs] forward replay {r} slot {j}: max|delta| = {float((got - want).abs().max()):.3e}, |want|_inf = {float(want.abs().max()):.3e}')
                assert torch.isfinite(want).all()
                assert torch.equal(got, want), (r, j, float((got - want).abs().max()))
    torch.cuda.synchronize()
    csr.check_errors(DEV)


def test_routed_forward_regroups_a_hub_complex_beyond_a_workgroup():
    """RoutedForward(regroup=True) pools the complexes beyond a workgroup -- here K(65, 65) and the large stars -- into a
    csr-mode static batch of its own.  (The router's blocked half refuses a four-stream CIN++ layer, so the model is the
    SparseCIN stack with the co-boundary message: the pooled batch runs its streaming path over hub rows.)  The predictions
    against the whole-batch routing and model(collate): the gate of test_routed_forward_regroups_the_complexes_beyond_a_workgroup."""
    from cwn_amd import csr
    from cwn_amd.models import SparseCIN
    from cwn_amd.static_graph import RoutedForward, StaticRouter
    pool, p = _pool()
    torch.manual_seed(2)
    model = _scaled(SparseCIN(W_IN, 2, 2, 64, dropout_rate=0.0, max_dim=2, jump_mode='cat', readout='sum', use_coboundaries=True,
                              graph_norm='bn').to(DEV)).eval()
    epoch = [_ids(*names) for names in EPOCH]
    whole = RoutedForward(model, StaticRouter(p, 4, slots=2), regroup=False)
    re = RoutedForward(model, StaticRouter(p, 4, slots=2), regroup=True, pool_batch=2)
    assert re.fbig is not None and not re.mask[NAMES.index('k65')], re.mask
    pooled = sorted({NAMES[i] for idx in epoch for i in idx[~re.mask[idx]]})
    print(f'[hubs] routed: pooled {pooled}')
    with torch.no_grad():
        a = whole.run_epoch(epoch)
        b = re.run_epoch(epoch)
        for k, idx in enumerate(epoch):
            want = model(p.collate(idx))
            assert a[k].shape == b[k].shape == want.shape
            scale = max(1.0, float(want.abs().max()))
            for got, name in ((a[k], 'whole'), (b[k], 'regrouped')):
                err = float((got - want).abs().max())
                print(f'[hubs] routed {name} batch {k}: max|delta| = {err:.3e} against {1e-5 * scale:.3e}')
                assert err <= 1e-5 * scale, (k, name, err)
    # the pooled static batch held a hub row when it ran last
    _hub_rows_present(re.big, 0, 'routed')
    torch.cuda.synchronize()
    csr.check_errors(DEV)


def _oracle_cx(b):
    cpu = lambda t: None if t is None else t.detach().cpu()
    cx = {'dimension': b.dimension, 'y': None, 'num_complexes': b.num_complexes, 'cochains': [
        {k: cpu(b.cochains[d][k]) for k in ('x', 'upper_index', 'lower_index', 'shared_boundaries', 'shared_coboundaries',
                                            'boundary_index', 'y', 'batch')} for d in range(b.dimension + 1)]}
    for c in cx['cochains']:
        c['x'] = c['x'].double()
    return cx


def test_autograd_backward_over_a_static_slot_outside_a_training_step():
    """The eager reader: model(slot.batch) under slot.dynamic() with autograd recording, loss.backward() -- no StaticTrainStep,
    nothing sets build_backward.  The backward of the boundary stream runs through the collated transposed plan (hub rows),
    the backward of the upper stream through transposes that are built on demand over the slot's capacity-sized entries.  The
    parameter gradients of the static slot AND of the per-batch path, each against torch autograd over the oracle in float64
    on the CPU, by the suite's gate (tests/_product.gate, the bound tests/_bounds.ratio reports beside its own: the
    componentwise bounds of tests/_bounds.py need a tracked reference per operation, which exists for the dense kernels
    only).  Two fills, the second with another batch: the transposes describe the entries the slot holds now."""
    from cwn_amd import csr
    from cwn_amd.models import SparseCIN
    from cwn_amd.static_batch import StaticBatch
    from oracle import cwn_oracle as O
    from tests._product import gate, to_double
    pool, p = _pool()
    L = 2
    torch.manual_seed(3)
    model = _scaled(SparseCIN(W_IN, 2, L, 64, dropout_rate=0.0, max_dim=2, jump_mode='cat', readout='sum', use_coboundaries=False,
                              graph_norm='id').to(DEV)).train()
    state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    sb = StaticBatch(p, 4, slots=2, mode='csr')
    assert not sb.build_backward

    def grads_of(run):
        model.zero_grad(set_to_none=True)
        run()
        return {n: (None if q.grad is None else q.grad.detach().clone()) for n, q in model.named_parameters()}

    for step, names in enumerate([('tri6', 's65', 'book65', 's200'), ('s129', 'path7', 's66')]):
        idx = _ids(*names)
        assert sb.fits([idx]).all()
        sb.set_batches([idx])
        sb.fill()
        slot = sb.slots[0]
        _hub_rows_present(sb, 0, ('backward', step))

        def on_slot():
            # (forward AND backward inside dynamic(): the backward launches read the device-side row counts too; the
            #  predictions of the complexes that exist are the first len(idx) rows)
            slot.restore()
            try:
                with slot.dynamic():
                    model(slot.batch)[:len(idx)].sum().backward()
            finally:
                slot.restore()
        got = grads_of(on_slot)
        ref_batch = p.collate(idx)
        per_batch = grads_of(lambda: model(ref_batch).sum().backward())
        leaves = {k: v.double().requires_grad_(True) for k, v in state.items() if v.is_floating_point()}
        ostate = dict(to_double(state))
        ostate.update(leaves)
        out, _ = O.sparse_cin_model_forward(ostate, _oracle_cx(p.collate(idx)), L, use_coboundaries=False, training=True, norm='id',
                                            embed=None, jump_mode='cat')
        out.sum().backward()
        n_par = 0
        for name, _ in model.named_parameters():
            r = leaves[name].grad
            if r is None:
                assert got[name] is None or not got[name].any(), name
                continue
            n_par += 1
            for g, path in ((per_batch[name], 'per-batch'), (got[name], 'static slot')):
                assert g is not None, (name, path)
                gate(g, r, f'fill {step}: d loss / d {name}, {path} vs float64 oracle autograd')
        assert n_par >= 8
    torch.cuda.synchronize()
    csr.check_errors(DEV)


# ---- 3. capacities that coincide with model widths -------------------------------------------------------------------------
def _zinc_pool(n=100):
    if 'z' not in _pool_cache:
        from cwn_amd.packed import PackedComplexes
        from cwn_amd.synthetic import zinc_like_complexes
        pool = zinc_like_complexes(n, seed=8, max_ring=6, n_lo=6, n_hi=10)
        _pool_cache['z'] = (pool, PackedComplexes(pool, DEV, max_dim=2, with_csr=True))
    return _pool_cache['z']


def _zinc_model(hidden, seed=6):
    from cwn_amd.models import EmbedSparseCIN
    torch.manual_seed(seed)
    return EmbedSparseCIN(28, 4, 1, 2, hidden, dropout_rate=0.0, max_dim=2, jump_mode=None, nonlinearity='relu', readout='sum',
                          train_eps=False, final_hidden_multiplier=2, final_readout='sum', init_reduce='sum', embed_edge=True,
                          use_coboundaries=True, graph_norm='bn').to(DEV)


def _forward_and_first_step(make_static, batches, hidden, mode, monkeypatch):
    """StaticForward bit-identical to the per-batch launches; the first StaticTrainStep loss within 1e-5 of TrainStep on the
    collated batch from the same state (the bound of test_static_train_step_on_reddit_like_batches_with_cross_entropy), the
    second within its 2e-2."""
    from cwn_amd import csr, layers
    from cwn_amd.static_graph import StaticForward, StaticTrainStep
    from cwn_amd.train import TrainStep
    pool, p = _zinc_pool()
    model = _zinc_model(hidden).eval()
    sb = make_static()
    assert sb.fits(batches).all()
    sf = StaticForward(model, sb)
    with torch.no_grad():
        outs = [o.clone() for o in sf.run_many(batches)]
        if mode == 'csr':
            # (a csr-mode slot streams -- grouped GEMM + aggregation --; the per-batch launches of the same path)
            monkeypatch.setattr(layers, 'BLOCKED_LAYER', False)
        for j, idx in enumerate(batches):
            want = model(p.collate(idx))
            print(f'[widths] {mode} slot {j}: {len(idx)} complexes, max|delta| = {float((outs[j] - want).abs().max()):.3e}')
            assert torch.equal(outs[j], want), (j, float((outs[j] - want).abs().max()))
        monkeypatch.undo()
    m1, m2 = _zinc_model(hidden, 7), _zinc_model(hidden, 7)
    m2.load_state_dict(m1.state_dict())
    sb2 = make_static()
    st = StaticTrainStep(m1, sb2, lr=1e-3)
    ref = TrainStep(m2, [p.collate(idx) for idx in batches], lr=1e-3, use_graph=False)
    sb2.set_epoch(batches)
    got = [float(l) for l in st.step()][:len(batches)]
    want = [float(ref.step(j)) for j in range(len(batches))]
    torch.cuda.synchronize()
    csr.check_errors(DEV)
    print(f'[widths] {mode} losses', got, 'vs', want)
    for k, (a, b) in enumerate(zip(got, want)):
        tol = 1e-5 if k == 0 else 2e-2
        assert abs(a - b) <= tol * max(1.0, abs(b)), (k, got, want)


@pytest.mark.parametrize('mode', ['blocked', 'csr'])
def test_batch_size_equal_to_the_hidden_width_with_a_short_batch(mode, monkeypatch):
    """B = hidden = 64: the capacity of the per-complex rows is the width of every weight matrix; the last batch is short,
    so a launch that picked the complexes' live count up for an operand of 64 rows of its own would leave rows unwritten."""
    from cwn_amd.static_batch import StaticBatch
    pool, p = _zinc_pool()
    B = hidden = 64
    perm = np.random.default_rng(2).permutation(len(pool))
    batches = [perm[:B], perm[B:]]
    assert len(batches[1]) == 36

    def make():
        sb = StaticBatch(p, B, slots=2, mode=mode)
        assert sb.B == hidden and hidden not in sb.cap_cells
        return sb
    _forward_and_first_step(make, batches, hidden, mode, monkeypatch)


@pytest.mark.parametrize('mode', ['blocked', 'csr'])
def test_a_cell_capacity_equal_to_the_hidden_width(mode, monkeypatch):
    """caps={'cells': [64, ...]}: the capacity of the vertices IS the hidden width, and survives the de-duplication."""
    from cwn_amd.static_batch import StaticBatch
    pool, p = _zinc_pool()
    B, hidden = 6, 64
    small = np.argsort([c.cochains[0].num_cells for c in pool], kind='stable')      # (the smallest molecules: 64 vertices hold six)
    batches = [small[:B], small[B:B + 4]]

    def make():
        sb = StaticBatch(p, B, slots=2, mode=mode, caps={'cells': [64, 96, 40]})
        assert sb.cap_cells[0] == hidden, sb.cap_cells
        return sb
    _forward_and_first_step(make, batches, hidden, mode, monkeypatch)
