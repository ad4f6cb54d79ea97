"""The owner form of the blocked backward launch (csrc/cwn_layer_bwd_own.hip, `cwn_layer_bwd_own_f32`) on structures the
molecular generators never produce (tests/_structures.py; the same cases tests/test_bwd_items.py executes on the CPU):

  * TOP-row slicing: one TOP row with 306 matches over many entry chunks (a ring of 18), a row count that is a power of two
    (strip(16): 16, star(32): 32 = one slice at width 128), at the cap (star(64) at width 64) and 20 / 35 of K6 / K7;
  * walk_matches over more than one chunk of lanes (the hub of a star: 32, 33, 64 matches), odd counts, exactly one match;
  * own rows one past a round of lane groups (33 at width 128, 65 / 67 at width 64);
  * PA|TOP records of a one-dimensional batch, TOP records without TOP rows (a lone bond), records without entries (an
    isolated vertex), items over several complexes some of them empty in a dimension (a bag of 600).

The reference is a float64 restatement of the backward formulas in the kernel's header whose mask is the kernel's contract:
(Y1[src] + Y2[cof]) > 0 evaluated in fp32 on the STORED fp32 products.  On integer values (and eps that are multiples of
1/4, distinct per level and per stream: a swapped or misplaced eps shows) every sum is exact, masks tie at 0, and the
launch must reproduce the reference bit for bit."""
import functools

import numpy as np
import pytest
import torch

from tests import _structures as S
from tests.test_gpu_blocked import DEV, _gate, _oracle_scope, _run, cpu

pytestmark = pytest.mark.gpu

EPS1 = (0.5, 0.25, 1.0)
EPS2 = (-0.25, 0.75, -0.5)


@functools.lru_cache(maxsize=None)
def _complexes(name):
    """The complexes of a case (lifted once per session; collating does not change them).  `strip5` besides CASES."""
    return tuple(S.strip(5)) if name == 'strip5' else tuple(S.CASES[name][0]())


def _max_dim(name):
    return 2 if name == 'strip5' else S.CASES[name][1]


def _conv(F, max_dim, seed, integer):
    from cwn_amd.layers import SparseCINConv
    torch.manual_seed(seed)
    conv = SparseCINConv(F, F, F, None, None, None, None, max_dim=max_dim, hidden=F, eps=0.0, train_eps=False,
                         act_module=torch.nn.ReLU, layer_dim=F, use_coboundaries=True).to(DEV)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for d, lvl in enumerate(conv.mp_levels):
            lvl.eps1.fill_(EPS1[d])
            lvl.eps2.fill_(EPS2[d])
            if integer:
                lin = lvl.msg_up_nn[1]
                lin.weight.copy_(torch.randint(-1, 2, lin.weight.shape, generator=g).float())
                lin.bias.copy_(torch.randint(-2, 3, lin.bias.shape, generator=g).float())
    return conv


def _device_batch(name, F, integer, seed, dup=False):
    b = S.collate(list(_complexes(name)), _max_dim(name))
    if dup:
        S.duplicate_entries(b, np.random.default_rng(seed))
    b = b.to(DEV)
    g = torch.Generator().manual_seed(seed + 17)
    for d in sorted(b.cochains):
        n = b.cochains[d].num_cells
        x = torch.randint(-3, 4, (n, F), generator=g).float() if integer else torch.randn(n, F, generator=g)
        b.cochains[d].x = x.to(DEV)
    return b


class _Problem:
    """A batch on the device with everything one backward launch reads: the LayerDim list, the stored products Y1 / Y2
    (fp32, computed with torch on the host: exact on integers), the output gradients and the transposed packed weights."""

    def __init__(self, name, F, integer, seed=0, dup=False, null=()):
        from cwn_amd import ops
        self.name, self.F = name, F
        md = _max_dim(name)
        self.b = b = _device_batch(name, F, integer, seed, dup)
        self.conv = conv = _conv(F, md, seed + 3, integer).train()
        self.nd = nd = len(b.cochains)
        params = b.get_all_cochain_params(max_dim=md, include_down_features=False)
        args = conv._blocked_args(params, 0, training=True)
        self.table = None
        if isinstance(args, str):              # no forward table for this batch: the descriptors by hand (the owner form reads
            self.why_by_hand = args            # the indices, eps and sizes; the forward's item table it does not read)
            self.dims = []
            for d in range(nd):
                c, lvl = b.cochains[d], conv.mp_levels[d]
                up = d + 1 < nd and c.upper_index is not None and c.upper_index.size(1) > 0
                self.dims.append(ops.LayerDim(x=c.x, eps1=lvl.eps1, eps2=lvl.eps2,
                                              up_index=c.upper_index if up else None, up_shared=c.shared_coboundaries if up else None,
                                              b_index=c.boundary_index if d > 0 else None))
            self.plan = b.block_plan()
        else:
            self.dims, self.plan, self.table, _ = args
        dims = self.dims
        self.has_up = [D.up_index is not None and D.up_index.size(1) > 0 for D in dims]
        self.bwd_table = self.plan.bwd_items(F, self.has_up, [D.b_index is not None for D in dims])
        self.rows = [int(D.x.size(0)) for D in dims]
        # host copies: indices, weights, the stored products
        self.up = [cpu(D.up_index) if self.has_up[d] else None for d, D in enumerate(dims)]
        self.sh = [cpu(D.up_shared) if self.has_up[d] else None for d, D in enumerate(dims)]
        self.bi = [cpu(D.b_index) if (D.b_index is not None and D.b_index.size(1)) else None for D in dims]
        self.W = [cpu(conv.mp_levels[d].msg_up_nn[1].weight) if self.has_up[d] else None for d in range(nd)]
        self.Y1, self.Y2 = [None] * nd, [None] * nd
        for d in range(nd):
            if self.has_up[d]:
                bias = cpu(conv.mp_levels[d].msg_up_nn[1].bias)
                self.Y1[d] = cpu(dims[d].x) @ self.W[d][:, :F].t() + bias
                self.Y2[d + 1] = cpu(dims[d + 1].x) @ self.W[d][:, F:].t()
        self.ys_of = [(None if self.Y1[d] is None else self.Y1[d].to(DEV), None if self.Y2[d] is None else self.Y2[d].to(DEV))
                      for d in range(nd)]
        g = torch.Generator().manual_seed(seed + 5)
        self.gs = []                            # [gU_0, gB_0, gU_1, ...] on the host; None = an output nobody differentiates
        for d in range(nd):
            for k in range(2):
                t = (torch.randint(-2, 3, (self.rows[d], F), generator=g).float() if integer
                     else torch.randn(self.rows[d], F, generator=g))
                self.gs.append(None if (2 * d + k) in null else t)
        ws = [conv.mp_levels[d].msg_up_nn[1].weight for d in range(nd) if self.has_up[d]]
        ops.pack_layer_weights_many(ws, transposed=True)
        self.wt_of = [ops.packed_layer_weight_t(conv.mp_levels[d].msg_up_nn[1].weight) if self.has_up[d] else None for d in range(nd)]
        assert all((w is not None) == h for w, h in zip(self.wt_of, self.has_up))

    def sums(self):
        """Y1[src] + Y2[cof] of every live entry, in fp32: what the kernel masks on."""
        return torch.cat([(self.Y1[d][self.up[d][0]] + self.Y2[d + 1][self.sh[d]]).flatten() for d in range(self.nd) if self.has_up[d]])

    def reference(self):
        """dx, gY1, gY2 per dimension in float64: the formulas of the kernel's header, mask from the stored fp32 products."""
        F, nd = self.F, self.nd
        zero = lambda d: torch.zeros(self.rows[d], F, dtype=torch.float64)
        gU = [zero(d) if self.gs[2 * d] is None else self.gs[2 * d].double() for d in range(nd)]
        gB = [zero(d) if self.gs[2 * d + 1] is None else self.gs[2 * d + 1].double() for d in range(nd)]
        dx = [(1 + EPS1[d]) * gU[d] + (1 + EPS2[d]) * gB[d] for d in range(nd)]
        gY1, gY2 = [None] * nd, [None] * nd
        for d in range(nd):
            if self.has_up[d]:
                src, dst, cof = self.up[d][0], self.up[d][1], self.sh[d]
                s = self.Y1[d][src] + self.Y2[d + 1][cof]
                assert s.dtype == torch.float32
                m = gU[d][dst] * (s > 0)
                gY1[d] = zero(d).index_add_(0, src, m)
                gY2[d + 1] = zero(d + 1).index_add_(0, cof, m)
                W = self.W[d].double()
                dx[d] += gY1[d] @ W[:, :F]
                dx[d + 1] += gY2[d + 1] @ W[:, F:]
            if self.bi[d] is not None:
                dx[d - 1].index_add_(0, self.bi[d][0], gB[d][self.bi[d][1]])
        return dx, gY1, gY2

    def launch(self, own=True):
        """One launch of the owner form (or of the atomic form over the forward's table; None where that does not apply).
        Whatever the allocator hands out for the outputs holds NaN: a row the launch does not write shows."""
        from cwn_amd import csr, ops
        if not own and self.table is None:
            return None
        gs = [None if g is None else g.to(DEV) for g in self.gs]
        junk = torch.full((sum(self.rows) * 3, self.F), float('nan'), device=DEV)
        del junk
        got = ops.layer_backward(self.dims, self.table, self.ys_of, [(gs[2 * d], gs[2 * d + 1]) for d in range(self.nd)], self.wt_of,
                                 bwd_table=self.bwd_table if own else None)
        if got is None:
            assert not own
            return None
        csr.check_errors(DEV)
        return got

    def outputs(self, got, ref):
        """[(name, launch's tensor, reference)] over dx of every dimension and the product gradients that exist."""
        dxs, gys = got
        dx_ref, gy1_ref, gy2_ref = ref
        out = []
        for d in range(self.nd):
            out.append((f'dx[{d}]', dxs[d], dx_ref[d]))
            assert (gys[d][0] is not None) == (gy1_ref[d] is not None) and (gys[d][1] is not None) == (gy2_ref[d] is not None)
            if gy1_ref[d] is not None:
                out.append((f'gY1[{d}]', gys[d][0], gy1_ref[d]))
            if gy2_ref[d] is not None:
                out.append((f'gY2[{d}]', gys[d][1], gy2_ref[d]))
        return out


def _assert_exact(P, forms=('own', 'atomic')):
    assert P.bwd_table is not None, 'tests/_structures.py: this case has an owner table at this width'
    s = P.sums()
    assert (s == 0).any() and (s < 0).any() and (s > 0).any(), 'the masks of this problem do not tie'
    ref = P.reference()
    ran = []
    for form in forms:
        got = P.launch(own=form == 'own')
        if got is None:
            continue
        ran.append(form)
        for what, t, r in P.outputs(got, ref):
            r32 = r.float()
            assert torch.equal(r32.double(), r), 'the reference itself is not exact in fp32'
            t = cpu(t)
            if not torch.equal(t, r32):
                bad = (t != r32) | torch.isnan(t)
                rows = bad.any(1).nonzero().flatten().tolist()
                raise AssertionError(f'{P.name}, F = {P.F}, {form} form, {what}: {int(bad.sum())} elements differ in rows {rows[:12]}'
                                     f'{" ..." if len(rows) > 12 else ""}; first: got {t[bad][0].item()}, want {r32[bad][0].item()}')
    assert 'own' in ran
    return ran


def _params(F_cases):
    return [pytest.param(F, c, id=f'{c}-F{F}') for F in (128, 64) for c in F_cases(F)]


@pytest.mark.parametrize('F,case', _params(S.cases_with_table))
def test_owner_backward_exact_on_integers(F, case):
    """(a) integer values, distinct dyadic eps per level and stream: bit-identical to the reference, in both forms."""
    _assert_exact(_Problem(case, F, integer=True, seed=1))


@pytest.mark.parametrize('F,case', _params(lambda F: ['K6', 'strip16', 'bag600']))
def test_owner_backward_exact_with_duplicated_entries(F, case):
    """(b) entries repeated inside their complex's slice are summed with multiplicity."""
    P = _Problem(case, F, integer=True, seed=8, dup=True)          # (a seed that repeats entries of BOTH adjacencies of a lone complex)
    plain = S.collate(list(_complexes(case)), 2)
    for d in range(2):
        assert P.up[d].size(1) > plain.cochains[d].upper_index.size(1), f'no entry of dimension {d} was duplicated'
    _assert_exact(P)


@pytest.mark.parametrize('F,case', _params(lambda F: ['ring18', 'K6', 'star32', 'bag600']))
def test_owner_backward_real_values(F, case):
    """(c) randn values at the project's gate, 1e-5 max(1, |ref|_inf), against the reference with the kernel's own masks."""
    P = _Problem(case, F, integer=False, seed=3)
    assert P.bwd_table is not None
    ref = P.reference()
    seen = []
    for form in ('own', 'atomic'):
        got = P.launch(own=form == 'own')
        if got is None:
            continue
        for what, t, r in P.outputs(got, ref):
            err = (cpu(t).double() - r).abs().max().item() if r.numel() else 0.0
            bound = 1e-5 * max(1.0, r.abs().max().item() if r.numel() else 1.0)          # (the bound of _gate)
            seen.append((err / bound, f'{form} form, {what}: max|delta| = {err:.3e}, gate {bound:.3e}', err, bound))
    assert any(s[1].startswith('own') for s in seen)
    for form in ('own', 'atomic'):
        of_form = [s for s in seen if s[1].startswith(form)]
        if of_form:
            worst = max(of_form)
            print(f'[gate] blocked backward on {case}, F = {F}: worst of {len(of_form)} tensors: {worst[1]} ({worst[0]:.3f} of the gate)')
    for _, what, err, bound in seen:
        assert err <= bound, (case, F, what)


_G = ('gU0', 'gB0', 'gU1', 'gB1', 'gU2', 'gB2')
_NULLS = ([pytest.param(F, (k,), id=f'F{F}-without-{_G[k]}') for F in (128, 64) for k in range(6)]
          + [pytest.param(F, tuple(q for q in range(6) if q != k), id=f'F{F}-only-{_G[k]}') for F in (128, 64) for k in range(6)])


@pytest.mark.parametrize('F,null', _NULLS)
def test_owner_backward_null_gradients(F, null):
    """(d) strip(5): each of the six output gradients NULL alone, then each the only one that is not."""
    _assert_exact(_Problem('strip5', F, integer=True, seed=4, null=null))


@pytest.mark.parametrize('F,case', _params(lambda F: ['bag600', 'K6']))
def test_owner_backward_two_launches_are_bit_identical(F, case):
    """(e) "Deterministic; the caller does not zero anything": two launches over the same inputs, every output equal."""
    P = _Problem(case, F, integer=False, seed=5)
    assert P.bwd_table is not None
    ref = P.reference()                      # (only to name the outputs)
    first = [(what, cpu(t)) for what, t, _ in P.outputs(P.launch(), ref)]
    second = [(what, cpu(t)) for what, t, _ in P.outputs(P.launch(), ref)]
    for (what, a), (_, c) in zip(first, second):
        assert not torch.isnan(a).any(), what
        assert torch.equal(a, c), (case, F, what)


@pytest.mark.parametrize('case,table', [('strip17', False), ('star33', False), ('K7', False), ('strip16', True)])
def test_training_step_without_an_owner_table_takes_the_streaming_backward(case, table):
    """(f) width 128, a complex beyond the owner form's workgroup: the training forward still runs as the blocked launch, the
    backward falls back to the streaming one (no owner launch is counted) and the gradients of x are right.  strip(16), which
    has a table, is the control: there the counter moves."""
    from cwn_amd import ops
    F = 128
    assert S.CASES[case][2] == table
    md = _max_dim(case)
    b = _device_batch(case, F, integer=True, seed=6)
    conv = _conv(F, md, seed=7, integer=True).train()
    nd = len(b.cochains)
    g = torch.Generator().manual_seed(8)
    gs = [torch.randint(-2, 3, (b.cochains[d].num_cells, F), generator=g).float() for d in range(nd) for _ in range(2)]
    ops.pack_layer_weights_many([conv.mp_levels[d].msg_up_nn[1].weight for d in range(nd - 1)], transposed=True)
    xin = [b.cochains[d].x.detach().clone().requires_grad_() for d in range(nd)]
    b.set_xs(xin)
    before = list(ops.BLOCKED_BACKWARD_LAUNCHES)
    plans, outs = conv.propagate_all(*b.get_all_cochain_params(max_dim=md, include_down_features=False))
    assert len(outs) == 2 * nd and conv.blocked_reason is None
    sum((o * w.to(DEV)).sum() for o, w in zip(outs, gs)).backward()
    assert ops.BLOCKED_BACKWARD_LAUNCHES[0] == before[0]
    assert ops.BLOCKED_BACKWARD_LAUNCHES[1] == before[1] + (1 if table else 0)
    # float64 autograd of the plain restatement
    xs = [cpu(x).double().requires_grad_() for x in xin]
    loss = 0.0
    for d in range(nd):
        c, lvl = b.cochains[d], conv.mp_levels[d]
        out_up = (1 + EPS1[d]) * xs[d]
        if d + 1 < nd and c.upper_index is not None and c.upper_index.size(1):
            W, bias = cpu(lvl.msg_up_nn[1].weight).double(), cpu(lvl.msg_up_nn[1].bias).double()
            ui, sh = cpu(c.upper_index), cpu(c.shared_coboundaries)
            msg = torch.relu((xs[d] @ W[:, :F].t() + bias)[ui[0]] + (xs[d + 1] @ W[:, F:].t())[sh])
            out_up = out_up + torch.zeros_like(xs[d]).index_add(0, ui[1], msg)
        out_b = (1 + EPS2[d]) * xs[d]
        if d > 0 and c.boundary_index is not None and c.boundary_index.size(1):
            bi = cpu(c.boundary_index)
            out_b = out_b + torch.zeros_like(xs[d]).index_add(0, bi[1], xs[d - 1][bi[0]])
        loss = loss + (out_up * gs[2 * d].double()).sum() + (out_b * gs[2 * d + 1].double()).sum()
    loss.backward()
    for d in range(nd):
        _gate(xin[d].grad, xs[d].grad, f'{case}, F = {F}: dL/dx[{d}] through the {"owner" if table else "streaming"} backward')


@pytest.mark.parametrize('F,case', _params(lambda F: [c for c in S.cases_with_table(F) if S.CASES[c][1] == 2 and not c.startswith('path')]))
def test_blocked_forward_exact_with_distinct_eps(F, case):
    """The forward suite gives every level the same eps1 == eps2 too: the blocked forward on the same structures, integer
    values and the distinct eps, bit-identical to the oracle in fp32."""
    b = _device_batch(case, F, integer=True, seed=9)
    conv = _conv(F, 2, seed=10, integer=True).eval()
    ref = _oracle_scope(conv, b, dtype=torch.float32)
    outs = _run(conv, b, blocked=True)                       # (asserts that the blocked launch is what ran)
    for d in range(3):
        assert torch.equal(cpu(outs[2 * d]), ref[d][0]), (case, F, d, 'up')
        assert torch.equal(cpu(outs[2 * d + 1]), ref[d][1]), (case, F, d, 'boundary')
