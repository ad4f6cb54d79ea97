"""The launches that open and close a training step's table work, exactly (second half of csrc/cwn_norm.hip):

  1. cwn_embedding_bwd_f32 called directly, form by form -- the ballot kernel of one small table, the column-walk kernel of
     several tables / one table of many rows, the table-in-LDS kernel in its vector (H % 4 == 0) and scalar sub-branches;
  2. the same through ops.embedding_sum and autograd, with the three destinations of ops._embedding_table_grads (a fresh
     buffer, an allocated .grad, the back-to-back .grad views of a FlatGradBucket), also under ops.deterministic(True);
  3. cwn_embed_front_bwd_f32 through ops.embed_front_train at H = 64 / 128 / 256 (kPer = 8 / 16 / 32) on the structures of
     tests/_structures.py, against the launches it replaces, bit for bit;
  4. cwn_step_begin on two regions carved from one allocation with sentinel words around them.

Gradients are integers in [-8, 8]: every sum (and every half of one) is exact in float32 in ANY order, so the comparison is
torch.equal against an index_add_ in float64.  dW starts from a non-zero integer: the kernels add, and rows nobody looks up keep
it.  Each case prints the form it ran (`[route]`); which form a direct call takes is decided by its arguments alone (_form
restates the dispatch of cwn_embedding_bwd_f32)."""
import pytest
import torch

from tests import _structures as S

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
FILL = 3.0                                   # what dW holds before a launch
NS = (1, 63, 64, 65, 128, 129)               # cells: bands of 64
BAD_INDEX = 10 ** 6


def _form(H, sizes, one_table_without_offsets=True):
    """The kernel cwn_embedding_bwd_f32 launches for these arguments."""
    V = sum(sizes)
    if len(sizes) == 1 and one_table_without_offsets and V <= 64 and H in (64, 128, 256):
        return 'ballot'
    if H in (64, 128, 256):
        return 'column-walk'
    assert V * H * 4 <= 60 * 1024
    return 'table-in-LDS, vector' if H % 4 == 0 else 'table-in-LDS, scalar'


def _ints(gen, *shape):
    return torch.randint(-8, 9, shape, generator=gen).float()


def _indices(gen, N, sizes, bad=True):
    """[N, cols] int64, column c in [0, sizes[c]); with `bad`, cell 1 of every column holds -1 and the cell before the last its
    table's size (N >= 4): cells the forward flags and the backward skips."""
    idx = torch.stack([torch.randint(0, s, (N,), generator=gen) for s in sizes], 1)
    if bad and N >= 4:
        idx[1] = -1
        idx[N - 2] = torch.tensor(sizes)
    return idx


def _reference(g, idx, sizes, live=None):
    """FILL + sum over the cells (the first `live`) and columns with an index inside its table, float64."""
    H, n = g.size(1), idx.size(0) if live is None else live
    ref = torch.full((sum(sizes), H), FILL, dtype=torch.float64)
    off = 0
    for c, s in enumerate(sizes):
        col = idx[:n, c]
        ok = (col >= 0) & (col < s)
        ref.index_add_(0, col[ok] + off, g[:n][ok].double())
        off += s
    return ref


def _bwd(g, idx, sizes, f32, count=None):
    """One direct launch into a dW pre-filled with FILL; `count`: a device int64 holding the live rows (the capacity is
    idx.size(0))."""
    from cwn_amd import _ffi
    N, cols = idx.shape
    H, V = int(g.size(1)), sum(sizes)
    src = (idx.float() if f32 else idx).contiguous().to(DEV)
    gd = g.contiguous().to(DEV)
    off = None if cols == 1 else torch.tensor([sum(sizes[:c]) for c in range(cols)], dtype=torch.int64, device=DEV)
    size = None if cols == 1 else torch.tensor(sizes, dtype=torch.int64, device=DEV)
    dW = torch.full((V, H), FILL, dtype=torch.float32, device=DEV)
    if count is None:
        n_dev = None
    else:
        with _ffi.dynamic_rows({N: count.data_ptr()}):
            n_dev = _ffi.dyn(N)
        assert n_dev == count.data_ptr()
    _ffi.check(_ffi.lib().cwn_embedding_bwd_f32(gd.data_ptr(), src.data_ptr(), _ffi.ptr(off), _ffi.ptr(size), dW.data_ptr(), N, cols,
                                                H, V, int(f32), n_dev, _ffi.stream_ptr(DEV)), 'cwn_embedding_bwd_f32')
    torch.cuda.synchronize()
    return dW.cpu()


def _exact(got, ref, what):
    ref32 = ref.float()
    assert torch.equal(ref32.double(), ref), what + ': the reference is not exact in float32'
    bad = int((got != ref32).sum())
    assert torch.equal(got, ref32), f'{what}: {bad} of {got.numel()} entries differ, first at {tuple((got != ref32).nonzero()[0].tolist())}'


def _direct(g, idx, sizes, f32, form, what):
    assert _form(g.size(1), sizes) == form, (what, _form(g.size(1), sizes))
    _exact(_bwd(g, idx, sizes, f32), _reference(g, idx, sizes), what)


def _no_error_raised():
    from cwn_amd.csr import check_errors
    check_errors(DEV)                  # the backward skips a cell outside its table silently: the forward is what flags it


# ------------------------------------------------------------------------------------------------------------------------------
# 1. cwn_embedding_bwd_f32, form by form
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('f32', [False, True], ids=['int64', 'float32'])
@pytest.mark.parametrize('H', [64, 128, 256])
def test_ballot_kernel_one_small_table(H, f32):
    gen = torch.Generator().manual_seed(H + int(f32))
    for V in (1, 2, 64):
        for N in NS:
            g, idx = _ints(gen, N, H), _indices(gen, N, (V,))
            _direct(g, idx, (V,), f32, 'ballot', f'ballot H={H} V={V} N={N} f32={f32}')
    # every cell on one row (the last: a full 64-bit ballot per band)
    g, idx = _ints(gen, 129, H), torch.full((129, 1), 27)
    _direct(g, idx, (28,), f32, 'ballot', f'ballot H={H}: every cell on row 27')
    # every row hit by exactly one cell of each 16-cell slice
    idx = torch.cat([torch.randperm(16, generator=gen) for _ in range(8)]).view(-1, 1)
    _direct(_ints(gen, 128, H), idx, (16,), f32, 'ballot', f'ballot H={H}: one cell per row and 16-cell slice')
    print(f'[route] cwn_embedding_bwd_f32 direct, H={H}, {"float32" if f32 else "int64"} indices: ballot kernel, 20 launches exact')
    _no_error_raised()


def _column_case(gen, N, cols):
    """sizes and indices of `cols` tables: column 0 a table of one row (a single distinct value), column 1 a table of 70 rows
    whose 64 cells of a band all differ, the rest small tables of random sizes."""
    sizes = [1, 70] + [int(torch.randint(2, 13, (1,), generator=gen)) for _ in range(cols - 2)]
    idx = _indices(gen, N, sizes, bad=False)
    perm = torch.randperm(70, generator=gen)[:64]
    idx[:, 1] = perm[torch.arange(N) % 64]
    if N >= 4:
        idx[1] = -1
        idx[N - 2] = torch.tensor(sizes)
    return tuple(sizes), idx


@pytest.mark.parametrize('f32', [False, True], ids=['int64', 'float32'])
@pytest.mark.parametrize('H', [64, 128, 256])
def test_column_walk_kernel(H, f32):
    gen = torch.Generator().manual_seed(7 * H + int(f32))
    n = 0
    for N in NS:
        for V in (65, 200):                                     # one table beyond the ballot kernel's 64 rows
            g, idx = _ints(gen, N, H), _indices(gen, N, (V,))
            _direct(g, idx, (V,), f32, 'column-walk', f'column-walk H={H} one table V={V} N={N} f32={f32}')
            n += 1
        for cols in (2, 8, 9, 17):                              # kColChunk = 8: below it, at it, one more, two chunks and one
            sizes, idx = _column_case(gen, N, cols)
            _direct(_ints(gen, N, H), idx, sizes, f32, 'column-walk', f'column-walk H={H} cols={cols} N={N} f32={f32}')
            n += 1
    print(f'[route] cwn_embedding_bwd_f32 direct, H={H}, {"float32" if f32 else "int64"} indices: column-walk kernel, {n} launches exact')
    _no_error_raised()


@pytest.mark.parametrize('f32', [False, True], ids=['int64', 'float32'])
@pytest.mark.parametrize('H', [4, 12, 96, 260, 1, 3, 30])
def test_table_in_lds_kernel(H, f32):
    """Vector sub-branch: H / 4 lanes per cell -- 1, 3, 24 and 65, of which 3 and 65 do not divide 256 (threads beyond
    per * lanes idle); scalar sub-branch (H % 4 != 0): min(H, 256) lanes per cell."""
    form = 'table-in-LDS, vector' if H % 4 == 0 else 'table-in-LDS, scalar'
    gen = torch.Generator().manual_seed(11 * H + int(f32))
    for sizes in ((28,), (9, 5, 4)):
        for N in NS:
            g, idx = _ints(gen, N, H), _indices(gen, N, sizes)
            _direct(g, idx, sizes, f32, form, f'{form} H={H} tables={sizes} N={N} f32={f32}')
    print(f'[route] cwn_embedding_bwd_f32 direct, H={H}, {"float32" if f32 else "int64"} indices: {form}, 12 launches exact')
    _no_error_raised()


@pytest.mark.parametrize('H,sizes,form', [(64, (28,), 'ballot'), (256, (64,), 'ballot'), (128, (9, 5, 4), 'column-walk'),
                                          (64, (200,), 'column-walk'), (96, (9, 5, 4), 'table-in-LDS, vector'),
                                          (12, (28,), 'table-in-LDS, vector'), (30, (9, 5, 4), 'table-in-LDS, scalar')])
def test_device_side_row_count_below_the_capacity(H, sizes, form):
    """Capacity 129, live rows 0 / 1 / 64 / 70 / 129 in a device int64: the rows behind the count hold NaN gradients and an
    index far outside every table; dW is exact on the live rows."""
    gen = torch.Generator().manual_seed(13 * H + len(sizes))
    CAP = 129
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    g0, idx0 = _ints(gen, CAP, H), _indices(gen, CAP, sizes, bad=False)
    assert _form(H, sizes) == form
    for f32 in (False, True):
        for live in (0, 1, 64, 70, 129):
            g, idx = g0.clone(), idx0.clone()
            g[live:], idx[live:] = float('nan'), BAD_INDEX
            count.fill_(live)
            _exact(_bwd(g, idx, sizes, f32, count=count), _reference(g0, idx0, sizes, live=live),
                   f'{form} H={H} tables={sizes} live={live} of {CAP} f32={f32}')
    print(f'[route] cwn_embedding_bwd_f32 direct with a device-side row count, H={H} tables={sizes}: {form}')
    _no_error_raised()


# ------------------------------------------------------------------------------------------------------------------------------
# 2. through ops.embedding_sum and autograd
# ------------------------------------------------------------------------------------------------------------------------------
class _Spy:
    """Records the (dW address, cols, H, V, has col_off) of every cwn_embedding_bwd_f32 call made through cwn_amd._ffi.lib()."""

    def __enter__(self):
        from cwn_amd import _ffi
        self.lib, self.orig, self.calls = _ffi.lib(), _ffi.lib().cwn_embedding_bwd_f32, []

        def spy(g, src, off, size, dW, n, cols, H, V, f32, n_dev, stream):
            self.calls.append(dict(dW=dW, cols=cols, H=H, V=V, off=off is not None, n=n))
            return self.orig(g, src, off, size, dW, n, cols, H, V, f32, n_dev, stream)
        self.lib.cwn_embedding_bwd_f32 = spy
        return self

    def __exit__(self, *exc):
        self.lib.cwn_embedding_bwd_f32 = self.orig
        return False


OPS_CASES = [(64, (28,), 'ballot'), (128, (9, 5, 4), 'column-walk'), (64, (200,), 'column-walk'),
             (96, (9, 5, 4), 'table-in-LDS, vector'), (12, (28,), 'table-in-LDS, vector')]


def _tables(gen, H, sizes):
    return [torch.nn.Parameter(_ints(gen, s, H).to(DEV)) for s in sizes]


@pytest.mark.parametrize('dest', ['fresh buffer', 'allocated .grad', 'flat bucket'])
@pytest.mark.parametrize('H,sizes,form', OPS_CASES)
def test_embedding_sum_backward_exact_by_destination(H, sizes, form, dest):
    """(The scalar sub-branch of the table-in-LDS kernel is not reachable here: ops.embedding_sum sends H % 4 != 0 to the generic
    aggregation.)  One launch of the expected form, into the expected destination."""
    from cwn_amd import ops
    from cwn_amd.dist import FlatGradBucket
    gen = torch.Generator().manual_seed(17 * H + len(sizes))
    N = 129
    ws = _tables(gen, H, sizes)
    idx = _indices(gen, N, sizes, bad=False)
    G = _ints(gen, N, H)
    fill = 0.0 if dest == 'fresh buffer' else FILL
    bucket = None
    if dest == 'allocated .grad':
        for w in ws:
            w.grad = torch.full_like(w, FILL)
    elif dest == 'flat bucket':
        bucket = FlatGradBucket(ws)
        bucket.flat.fill_(FILL)
    with _Spy() as spy:
        out = ops.embedding_sum(ws, idx.to(DEV))
        if dest == 'fresh buffer':
            (out * G.to(DEV)).sum().backward()
        else:
            with ops.accumulate_into_grad():
                (out * G.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert len(spy.calls) == 1, spy.calls
    call = spy.calls[0]
    assert (call['cols'], call['H'], call['V'], call['n']) == (len(sizes), H, sum(sizes), N)
    assert _form(H, sizes, one_table_without_offsets=not call['off']) == form
    direct = dest != 'fresh buffer' and (len(sizes) == 1 or dest == 'flat bucket')
    if direct:
        assert call['dW'] == ws[0].grad.data_ptr(), f'{dest}: the kernel did not add into the gradient itself'
    elif dest != 'fresh buffer':
        assert all(call['dW'] != w.grad.data_ptr() for w in ws)
    ref = _reference(G, idx, sizes) - FILL + fill
    got = torch.cat([w.grad.detach().cpu() for w in ws], 0)
    _exact(got, ref, f'ops.embedding_sum H={H} tables={sizes} -> {dest}')
    if bucket is not None:
        used = torch.zeros(bucket.flat.numel(), dtype=torch.bool)
        for w, o in zip(bucket.params, bucket.offsets):
            used[o:o + w.numel()] = True
        assert bool((bucket.flat.cpu()[~used] == FILL).all()), 'a pad element of the flat bucket was written'
    print(f'[route] ops.embedding_sum backward, H={H} tables={sizes}: {form} -> {dest}'
          f'{" (the kernel adds into it)" if direct else " (a zeroed buffer, then added)"}')


@pytest.mark.parametrize('H,sizes,form', OPS_CASES)
def test_embedding_sum_backward_exact_when_deterministic(H, sizes, form):
    """ops.deterministic(True): the ordered form (a destination-sorted plan and one segmented reduce) launches no
    cwn_embedding_bwd_f32 and is exact as well, into a fresh buffer and into an allocated .grad."""
    from cwn_amd import ops
    gen = torch.Generator().manual_seed(19 * H + len(sizes))
    N = 129
    idx = _indices(gen, N, sizes, bad=False)
    G = _ints(gen, N, H)
    ops.deterministic(True)
    try:
        for dest in ('fresh buffer', 'allocated .grad'):
            ws = _tables(gen, H, sizes)
            if dest == 'allocated .grad':
                for w in ws:
                    w.grad = torch.full_like(w, FILL)
            with _Spy() as spy:
                out = ops.embedding_sum(ws, idx.to(DEV))
                with ops.accumulate_into_grad(dest == 'allocated .grad'):
                    (out * G.to(DEV)).sum().backward()
            torch.cuda.synchronize()
            assert not spy.calls, 'the ordered form went through the atomic kernels'
            ref = _reference(G, idx, sizes) - (FILL if dest == 'fresh buffer' else 0.0)
            _exact(torch.cat([w.grad.detach().cpu() for w in ws], 0), ref, f'deterministic ops.embedding_sum H={H} tables={sizes} -> {dest}')
    finally:
        ops.deterministic(False)
    assert ops.DETERMINISTIC is False
    print(f'[route] ops.embedding_sum backward under ops.deterministic, H={H} tables={sizes}: plan + segmented reduce (not {form})')


# ------------------------------------------------------------------------------------------------------------------------------
# 3. cwn_embed_front_bwd_f32 through ops.embed_front_train
# ------------------------------------------------------------------------------------------------------------------------------
def _rings(*ks):
    return [c for k in ks for c in S.ring(k)]


# name -> (complexes, max_dim, n0, n1): bands of 32 cells, so 31 / 32 / 33 / 64 / 65 sit on either side of a band's edge
FRONT_CASES = {
    'K6': (lambda: S.clique(6), 2, 6, 15),                                   # a vertex in five edges, an edge in four triangles
    'K6+path27': (lambda: S.clique(6) + S.path(27), 2, 33, 41),
    'star31': (lambda: S.star(31), 1, 32, 31),                               # the hub in k edges, no rings
    'star32': (lambda: S.star(32), 1, 33, 32),
    'star64': (lambda: S.star(64), 1, 65, 64),
    'ring18+13': (lambda: _rings(18, 13), 2, 31, 31),                        # long rings
    'ring18x3+10': (lambda: _rings(18, 18, 18, 10), 2, 64, 64),
    'ring18x3+11': (lambda: _rings(18, 18, 18, 11), 2, 65, 65),
    'path33': (lambda: S.path(33), 2, 33, 32),
    'path34': (lambda: S.path(34), 2, 34, 33),
    'path65': (lambda: S.path(65), 2, 65, 64),
    'vertices+bond': (lambda: [c for _ in range(30) for c in S.vertex()] + S.bond(), 2, 32, 1),
    'bond+vertices': (lambda: S.bond() + [c for _ in range(62) for c in S.vertex()], 2, 64, 1),
    'vertex': (S.vertex, 2, 1, 0),
    'mixed': (S.mixed, 2, 7, 6),
    'bag40': (lambda: S.bag(40, 1), 2, None, None),
}
TABLES = [(1, 1), (28, 4), (64, 64)]             # rows of the vertex and of the edge table
LANDINGS = {1, 31, 32, 33, 64, 65}


def test_front_cases_land_on_the_band_edges():
    assert LANDINGS <= {v[2] for v in FRONT_CASES.values()} and LANDINGS <= {v[3] for v in FRONT_CASES.values()}


def _front_batch(name):
    make, max_dim, n0, n1 = FRONT_CASES[name]
    b = S.collate(make(), max_dim)
    c1, c2 = b.cochains.get(1), b.cochains.get(2)
    shape = dict(n0=int(b.cochains[0].num_cells), n1=int(c1.num_cells) if c1 is not None else 0,
                 n2=int(c2.num_cells) if c2 is not None else 0)
    bi1 = c1.boundary_index if c1 is not None and shape['n1'] > 0 else None
    bi2 = c2.boundary_index if c2 is not None and shape['n2'] > 0 else None
    if n0 is not None:
        assert (shape['n0'], shape['n1']) == (n0, n1), (name, shape)
    return shape, bi1, bi2


def _front_reference(g0, g1, g2, bi1, bi2, idv, ide, Vv, Ve, halve, fill):
    """dv = g0 + sum over the edges of v of ([no edge table] g1[e] + s * sum over the rings of e of g2[ring]); dWv[id[v]] += dv;
    dWe[id[e]] += g1[e]: float64."""
    H = g0.size(1)
    s = 0.5 if halve else 1.0
    per_edge = torch.zeros(g1.size(0), H, dtype=torch.float64)
    if bi2 is not None:
        per_edge.index_add_(0, bi2[0], g2.double()[bi2[1]] * s)
    if ide is None:
        per_edge += g1.double()
    dv = g0.double().clone()
    if bi1 is not None:
        dv.index_add_(0, bi1[0], per_edge[bi1[1]])
    dWv = torch.full((Vv, H), fill, dtype=torch.float64).index_add_(0, idv, dv)
    dWe = None if ide is None else torch.full((Ve, H), fill, dtype=torch.float64).index_add_(0, ide, g1.double())
    return dWv, dWe


@pytest.mark.parametrize('name', list(FRONT_CASES))
@pytest.mark.parametrize('H', [64, 128, 256])
def test_front_backward_exact_on_structures(H, name):
    """Every combination of halve, edge table and (with one) the index types of vertices and edges; the table sizes and the
    destination (a fresh buffer / an allocated .grad pre-filled with FILL) rotate over the combinations.  The one-launch
    backward must have run, and the launches it replaces (FUSED_FRONT_BACKWARD = False) give the same bits."""
    from cwn_amd import ops
    from cwn_amd.csr import cached_adjacency
    shape, bi1, bi2 = _front_batch(name)
    n0, n1, n2 = shape['n0'], shape['n1'], shape['n2']
    gen = torch.Generator().manual_seed(23 * H + len(name))
    g0, g1, g2 = _ints(gen, n0, H), _ints(gen, n1, H), _ints(gen, n2, H)
    gs = [g.to(DEV) for g in (g0, g1, g2)]
    adj1 = cached_adjacency(bi1.to(DEV), n1, n0) if bi1 is not None else None
    adj2 = cached_adjacency(bi2.to(DEV), n2, n1) if bi2 is not None else None
    calls = []
    orig = ops._front_backward_fused
    ops._front_backward_fused = lambda *a: (lambda r: (calls.append(r is not None), r)[1])(orig(*a))
    combos = [(halve, edge, vf, ef) for halve in (True, False) for edge in (True, False) for vf in (False, True)
              for ef in ((False, True) if edge else (False,))]
    ran = 0
    try:
        for k, (halve, edge, vf, ef) in enumerate(combos):
            if not edge and adj1 is None:
                continue                                 # edges without a table and without boundaries: nothing defines x1
            Vv, Ve = TABLES[(k + H // 64) % 3]
            into_grad = k % 2 == 1
            fill = FILL if into_grad else 0.0
            idv, ide = torch.randint(0, Vv, (n0,), generator=gen), (torch.randint(0, Ve, (n1,), generator=gen) if edge else None)
            fv = (idv.float() if vf else idv).view(-1, 1).to(DEV)
            fe = None if ide is None else (ide.float() if ef else ide).view(-1, 1).to(DEV)
            want = _front_reference(g0, g1, g2, bi1, bi2, idv, ide, Vv, Ve, halve, fill)
            got = {}
            for fused in (True, False):
                ops.FUSED_FRONT_BACKWARD = fused
                wv = torch.nn.Parameter(_ints(torch.Generator().manual_seed(k), Vv, H).to(DEV))
                we = torch.nn.Parameter(_ints(torch.Generator().manual_seed(k + 1), Ve, H).to(DEV)) if edge else None
                if into_grad:
                    for w in (wv, we):
                        if w is not None:
                            w.grad = torch.full_like(w, FILL)
                del calls[:]
                xs = ops.embed_front_train([wv], fv, [we] if edge else None, fe, n1, adj1, n2, adj2, halve=halve)
                with ops.accumulate_into_grad(into_grad):
                    sum((x * g).sum() for x, g in zip(xs, gs)).backward()
                torch.cuda.synchronize()
                assert calls == [fused], f'one-launch backward taken: {calls}, expected {[fused]}'
                got[fused] = (wv.grad.detach().cpu(), None if we is None else we.grad.detach().cpu())
            what = f'front backward {name} H={H} halve={halve} edge table={edge} Vv={Vv} Ve={Ve} f32 indices=({vf}, {ef}) into .grad={into_grad}'
            _exact(got[True][0], want[0], what + ': d vertex table')
            assert torch.equal(got[True][0], got[False][0]), what + ': the unfused path differs in the vertex table'
            if edge:
                _exact(got[True][1], want[1], what + ': d edge table')
                assert torch.equal(got[True][1], got[False][1]), what + ': the unfused path differs in the edge table'
            ran += 1
    finally:
        ops.FUSED_FRONT_BACKWARD, ops._front_backward_fused = True, orig
    assert ran >= 8
    print(f'[route] cwn_embed_front_bwd_f32 (kPer = {32 * H // 256}) through ops.embed_front_train, {name}: n0={n0} n1={n1} n2={n2}, '
          f'{ran} combinations exact, one launch each; the unfused launches give the same bits')


def test_front_forward_on_a_batch_without_edges():
    """The 'vertex' case above found it: with an edge table and n1 = 0 the edge features are an empty tensor, whose null address
    cwn_embed_front_f32 refused as a bad argument (ops.embed_front and ops.FrontLaunch handed the table over all the same).
    Both now leave the edge table out when there is no edge: x0 is the looked-up rows, x1 and x2 are empty."""
    from cwn_amd import ops
    gen = torch.Generator().manual_seed(3)
    H = 64
    wv, we = _ints(gen, 28, H).to(DEV), _ints(gen, 4, H).to(DEV)
    for n0 in (1, 33):
        idv = torch.randint(0, 28, (n0, 1), generator=gen)
        fv, fe = idv.to(DEV), torch.zeros(0, 1, dtype=torch.long, device=DEV)
        with torch.no_grad():
            xs = ops.embed_front([wv], fv, [we], fe, 0, None, 0, None)
            launch = ops.FrontLaunch([wv], [we], n0, 0, None, 0, None, True, None, None, fv, fe)
            ys = launch.run(fv, fe)
        assert ys is not None
        for got in (xs, ys):
            assert torch.equal(got[0].cpu(), wv.cpu()[idv.view(-1)]) and got[1].shape == (0, H) and got[2].shape == (0, H)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. cwn_step_begin
# ------------------------------------------------------------------------------------------------------------------------------
NAN_BITS, GUARD = 0x7FC00001, 0x5A5A5A5A


@pytest.mark.parametrize('a_bytes,b_bytes', [(16, 0), (0, 16), (16, 16), (4096 * 256 * 16 + 16, 48), (0, 0)],
                         ids=['a16', 'b16', 'a16-b16', 'second-grid-pass', 'step-only'])
def test_step_begin_zeroes_its_two_regions_and_counts(a_bytes, b_bytes):
    """[guard | a | guard | b | guard] in one allocation, 16 bytes a guard, the regions pre-filled with a NaN's bits: afterwards
    both regions are zero, the guards untouched and the step counter up by one -- without `active` and with active = 1; with
    active = 0 the counter stays and the regions are zeroed all the same.  4096 * 256 * 16 + 16 bytes is one 16-byte store more
    than the grid of 4096 workgroups covers in a pass."""
    from cwn_amd import _ffi
    wa, wb = a_bytes // 4, b_bytes // 4
    a0, b0 = 4, 4 + wa + 4
    buf = torch.empty(4 + wa + 4 + wb + 4, dtype=torch.int32, device=DEV)
    guards = torch.zeros(buf.numel(), dtype=torch.bool, device=DEV)
    for lo in (0, a0 + wa, b0 + wb):
        guards[lo:lo + 4] = True
    assert buf.data_ptr() % 16 == 0
    for active, moved in ((None, 1), (1, 1), (0, 0)):
        buf.fill_(NAN_BITS)
        buf[guards] = GUARD
        step = torch.tensor([7, GUARD], dtype=torch.int32, device=DEV)
        act = None if active is None else torch.tensor([active], dtype=torch.int64, device=DEV)
        code = _ffi.lib().cwn_step_begin(buf.data_ptr() + 4 * a0, a_bytes, buf.data_ptr() + 4 * b0, b_bytes, step.data_ptr(), _ffi.ptr(act),
                                         None, _ffi.stream_ptr(DEV))
        _ffi.check(code, 'cwn_step_begin')
        torch.cuda.synchronize()
        what = f'cwn_step_begin a={a_bytes} b={b_bytes} active={active}'
        assert step.tolist() == [7 + moved, GUARD], f'{what}: the step counter reads {step.tolist()}'
        assert bool((buf[guards] == GUARD).all()), f'{what}: a guard word was written'
        assert bool((buf[~guards] == 0).all()), f'{what}: {int((buf[~guards] != 0).sum())} words of the regions are not zero'
