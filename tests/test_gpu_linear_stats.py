"""cwn_linear_stats_f32 (csrc/cwn_linear_stats.hip) on the GPU -- the forward of a Linear stage that leaves BatchNorm band
statistics over the rows that exist, at any width up to 128 -- and the captured training step it completes:
  1. the launch against cwn_gemm_f32 on the same descriptor (bit for bit, no count) and against float64;
  2. the device-side row-count contract of tests/test_gpu_row_counts.py, cwn_bn_finalize_f32 under the same count included;
  3. StaticTrainStep over StaticBatch(mode='csr') at hidden 48 and 16 against the per-batch step;
  4. SparseCIN over raw 7-wide features at hidden 64 (first layer on the new launch, second on the stage kernels);
  5. two slots and an epoch of three batches at hidden 48;
  6. a spy on the entry point: no call at hidden 128 nor in an eager step."""
import functools

import numpy as np
import pytest
import torch

from cwn_amd import _ffi, ops
from tests._product import gate

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
CAP = 200                      # tests/test_gpu_row_counts.py: its capacity, its live counts, its sentinel
SENT = -9.0
LIVES = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 95, 96, 97, 127, 128, 129, 199, 200)
NAN = float('nan')
EPS, MOM = 1e-5, 0.1


def _rand(g, *shape):
    return torch.randn(*shape, generator=g)


def _linear_stats(gm: ops.Gemm, Y: torch.Tensor):
    """The new entry point on the descriptor ops.Gemm.desc builds for cwn_gemm_f32 (no device-side count here)."""
    d = gm.desc(Y)
    assert d.m_dev is None
    _ffi.linear_stats([d], DEV)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. against cwn_gemm_f32 and float64
# ------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(48, 0, 48), (16, 0, 16), (5, 0, 64), (13, 0, 24), (37, 0, 100), (48, 48, 48), (128, 128, 128)]
ROWS = (1, 31, 32, 33, 130)


def _case(g, M, K, K2, N, bias, pro, x_slice=False):
    """Operands on the device, the float64 reference of Y and of both band arrays."""
    if x_slice:                     # X a column slice of a wider matrix: row stride K + 2, start 4 bytes into a row
        Xw = _rand(g, M, K + 2)
        Xw[:, 0] = Xw[:, K + 1] = float('nan')      # (NaN beside the window: a load that strays and is not discarded shows in Y)
        X = Xw.to(DEV)[:, 1:K + 1]
    else:
        X = _rand(g, M, K).to(DEV)
    X2 = _rand(g, M, K2).to(DEV) if K2 else None
    W = (_rand(g, N, K + K2) / (K + K2) ** 0.5).to(DEV)
    b = _rand(g, N).to(DEV) if bias else None
    sc = sh = sc2 = sh2 = None
    if pro == 3:
        sc, sh = (torch.rand(K, generator=g) + 0.5).to(DEV), _rand(g, K).to(DEV)
        if K2:
            sc2, sh2 = (torch.rand(K2, generator=g) + 0.5).to(DEV), _rand(g, K2).to(DEV)
    x = X.double().cpu()
    if sc is not None:
        x = x * sc.double().cpu() + sh.double().cpu()
    if pro & 1:
        x = x.relu()
    if K2:
        x2 = X2.double().cpu()
        if sc2 is not None:
            x2 = x2 * sc2.double().cpu() + sh2.double().cpu()
        if pro & 2:
            x2 = x2.relu()
        x = torch.cat([x, x2], 1)
    y = x @ W.double().cpu().t()
    if b is not None:
        y = y + b.double().cpu()
    bands = ops.stat_rows(M)
    pad = torch.zeros(bands * 32 - M, N, dtype=torch.float64)
    yb = torch.cat([y, pad]).view(bands, 32, N)
    kw = dict(X=X, X2=X2, W=W, bias=b, in_scale=sc, in_shift=sh, in_scale2=sc2, in_shift2=sh2, in_relu=pro & (3 if K2 else 1), exact=True)
    return kw, y, yb.sum(1), (yb * yb).sum(1)


def _both(kw, M, N, stats=True):
    """(Y, band statistics) of cwn_gemm_f32 and of cwn_linear_stats_f32 on the same descriptor, outputs pre-filled with a sentinel."""
    res = []
    for mine in (False, True):
        Y = torch.full((M, N), SENT, dtype=torch.float32, device=DEV)
        cs = torch.full((2, ops.stat_rows(M), N), SENT, dtype=torch.float64, device=DEV) if stats else None
        gm = ops.Gemm(col_stats=cs, out=Y, **kw)
        if mine:
            _linear_stats(gm, Y)
        else:
            assert not ops.gemm_uses_split([gm], DEV)          # (statistics: always the exact kernel)
            ops.run_gemm([gm], DEV)
        res.append((Y, cs))
    return res


@pytest.mark.parametrize('K,K2,N', SHAPES)
def test_launch_equals_gemm_f32_bit_for_bit_and_float64_inside_the_gate(K, K2, N):
    g = torch.Generator().manual_seed(1000 * K + 10 * K2 + N)
    for M in ROWS:
        for bias in (True, False):
            for pro in (0, 1, 3):
                kw, y, s1, s2 = _case(g, M, K, K2, N, bias, pro)
                (Yg, cg), (Ym, cm) = _both(kw, M, N)
                what = f'linear_stats K={K} K2={K2} N={N} M={M} bias={bias} in_relu={pro}'
                assert torch.equal(Ym, Yg), what
                assert torch.equal(cm, cg), what
                gate(Ym, y, what + ' Y')
                gate(cm[0], s1, what + ' band sums')
                gate(cm[1], s2, what + ' band sums of squares')
    kw, y, _, _ = _case(g, 33, K, K2, N, True, 3)              # an identity norm: no statistics asked for
    (Yg, _), (Ym, _) = _both(kw, 33, N, stats=False)
    assert torch.equal(Ym, Yg)
    gate(Ym, y, f'linear_stats K={K} K2={K2} N={N} without statistics')


@pytest.mark.parametrize('K,N,M', [(13, 24, 33), (48, 48, 130)])
def test_x_as_a_column_slice_with_an_odd_row_stride(K, N, M):
    """X[:, 1 : K + 1] of an [M, K + 2] matrix: a row stride that is no multiple of 4 and a start that is not 16-byte aligned
    -- the element-by-element path at a width the 16-byte path would otherwise take.  The two columns beside the window hold
    NaN: nothing of them reaches Y or a band sum."""
    g = torch.Generator().manual_seed(K * N)
    kw, y, s1, s2 = _case(g, M, K, 0, N, True, 3, x_slice=True)
    assert kw['X'].stride(0) % 4 != 0 and kw['X'].data_ptr() % 16 != 0
    (Yg, cg), (Ym, cm) = _both(kw, M, N)
    assert torch.equal(Ym, Yg) and torch.equal(cm, cg)
    gate(Ym, y, 'slice Y')
    gate(cm[0], s1, 'slice band sums')
    gate(cm[1], s2, 'slice band sums of squares')


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the row-count contract
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,N', [(48, 48), (5, 64)])
def test_device_side_row_count(K, N):
    """Capacity 200, padding rows of X NaN, Y and both band arrays pre-filled with a sentinel, the count in a device int64:
    rows of Y at or beyond the count and bands at or beyond CWN_STAT_ROWS(count) keep the sentinel bit for bit, everything
    below equals the M = count call bit for bit, a count of 0 writes nothing; cwn_bn_finalize_f32 under the same count gives
    the mean, rstd and running statistics of BatchNorm1d(train) over the live rows of the kernel's own y (float64)."""
    g = torch.Generator().manual_seed(K + N)
    X = _rand(g, CAP, K)
    W = (_rand(g, N, K) / K ** 0.5).to(DEV)
    bias = _rand(g, N).to(DEV)
    sc, sh = (torch.rand(K, generator=g) + 0.5).to(DEV), _rand(g, K).to(DEV)
    gamma, beta = (torch.rand(N, generator=g) + 0.5).to(DEV), _rand(g, N).to(DEV)
    rm0, rv0 = _rand(g, N), torch.rand(N, generator=g) + 0.5
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    bands = ops.stat_rows(CAP)
    for live in LIVES:
        Xd = X.clone()
        Xd[live:] = NAN
        Xd = Xd.to(DEV)
        Y = torch.full((CAP, N), SENT, dtype=torch.float32, device=DEV)
        cs = torch.full((2, bands, N), SENT, dtype=torch.float64, device=DEV)
        aff = torch.full((4, N), SENT, dtype=torch.float32, device=DEV)
        rm, rv = rm0.to(DEV), rv0.to(DEV)
        nbt = torch.full((1,), 5, dtype=torch.int64, device=DEV)
        bwd = torch.full((2, N), SENT, dtype=torch.float32, device=DEV)
        count.fill_(live)
        what = f'linear_stats count K={K} N={N} live={live}'
        with _ffi.dynamic_rows({CAP: count.data_ptr()}):
            gm = ops.Gemm(X=Xd, W=W, bias=bias, in_scale=sc, in_shift=sh, in_relu=1, col_stats=cs, out=Y)
            with pytest.raises(RuntimeError, match='takes no device-side row count'):
                gm.desc(Y)                                     # (cwn_gemm_f32 still refuses this launch)
            res = ops.run_linear_stats([gm], DEV)
            assert res is not None and res[0] is Y, what
            _ffi.bn_finalize([_ffi.BnDesc(col_sum=cs[0].data_ptr(), col_sumsq=cs[1].data_ptr(), gamma=gamma.data_ptr(),
                                          beta=beta.data_ptr(), running_mean=rm.data_ptr(), running_var=rv.data_ptr(),
                                          scale=aff[0].data_ptr(), shift=aff[1].data_ptr(), mean=aff[2].data_ptr(),
                                          rstd=aff[3].data_ptr(), M=CAP, N=N, eps=EPS, momentum=MOM,
                                          num_batches_tracked=nbt.data_ptr(), bwd_sums=bwd.data_ptr())], DEV)
        nb = ops.stat_rows(live)
        assert bool((Y[live:] == SENT).all()), what + ': a row at or beyond the count was written'
        assert bool((cs[:, nb:] == SENT).all()), what + ': a band at or beyond the count was written'
        assert not torch.isnan(Y[:live]).any() and not torch.isnan(cs[:, :nb]).any(), what
        if live == 0:
            assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0) and int(nbt) == 5, what
            continue
        # the M = live call on a copy of the live rows: no count, nothing behind them
        Y1 = torch.full((live, N), SENT, dtype=torch.float32, device=DEV)
        c1 = torch.full((2, nb, N), SENT, dtype=torch.float64, device=DEV)
        _linear_stats(ops.Gemm(X=Xd[:live].clone(), W=W, bias=bias, in_scale=sc, in_shift=sh, in_relu=1, col_stats=c1, out=Y1, exact=True), Y1)
        assert torch.equal(Y[:live], Y1), what + ': a live row depends on the count or on the padding'
        assert torch.equal(cs[:, :nb], c1), what + ': a band depends on the count or on the padding'
        x = (X[:live].double() * sc.double().cpu() + sh.double().cpu()).relu()
        gate(Y[:live], x @ W.double().cpu().t() + bias.double().cpu(), what + ' Y')
        z = Y[:live].double().cpu()
        mean, var = z.mean(0), z.var(0, unbiased=False)
        gate(aff[2], mean, what + ' mean')
        gate(aff[3], 1.0 / torch.sqrt(var + EPS), what + ' rstd')
        gate(rm, (1 - MOM) * rm0.double() + MOM * mean, what + ' running_mean')
        gate(rv, (1 - MOM) * rv0.double() + MOM * (z.var(0, unbiased=True) if live > 1 else var), what + ' running_var')
        assert int(nbt) == 6, what


# ------------------------------------------------------------------------------------------------------------------------------
# 3. - 6. the captured step
# ------------------------------------------------------------------------------------------------------------------------------
B = 20


@functools.lru_cache(maxsize=None)
def _zinc():
    from cwn_amd.packed import PackedComplexes
    from cwn_amd.synthetic import zinc_like_complexes
    pool = zinc_like_complexes(40, seed=3, max_ring=6, n_lo=9, n_hi=28)
    return pool, PackedComplexes(pool, DEV, max_dim=2, with_csr=True)


@functools.lru_cache(maxsize=None)
def _raw(width=7):
    """Ring-lifted molecules with `width` raw float features on every cell (what SparseCIN takes as given)."""
    from cwn_amd.packed import PackedComplexes
    from cwn_amd.synthetic import random_molecule, ring_lift
    rng, g = np.random.default_rng(5), torch.Generator().manual_seed(5)
    pool = []
    for _ in range(40):
        n, bonds = random_molecule(rng, 9, 28)
        cx = ring_lift(n, bonds, _rand(g, n, width), _rand(g, len(bonds), width), max_k=6, y=_rand(g, 1))
        if cx.dimension >= 2:
            cx.cochains[2].x = _rand(g, cx.cochains[2].num_cells, width)
        pool.append(cx)
    return pool, PackedComplexes(pool, DEV, max_dim=2, with_csr=True)


def _rings(cx) -> int:
    return cx.cochains[2].num_cells if cx.dimension >= 2 else 0


def _three_batches(pool, seed=13):
    """20, 7 and one lone complex with at least two rings, in that order: from the second step on the padding rows of every
    buffer hold rows of an earlier, larger batch."""
    perm = np.random.default_rng(seed).permutation(len(pool))
    batches = [perm[:B], perm[B:B + 7]]
    used = set(int(i) for b in batches for i in b)
    lone = next(i for i in range(len(pool)) if i not in used and _rings(pool[i]) >= 2)
    return batches + [np.array([lone])]


def _embed_model(hidden, layers=2, seed=4):
    from cwn_amd.models import EmbedSparseCIN
    torch.manual_seed(seed)
    return EmbedSparseCIN(28, 4, 1, layers, hidden, dropout_rate=0.0, max_dim=2, embed_edge=True, use_coboundaries=True,
                          graph_norm='bn').to(DEV)


def _raw_model(seed=4):
    from cwn_amd.models import SparseCIN
    torch.manual_seed(seed)
    return SparseCIN(7, 1, 2, 64, dropout_rate=0.0, max_dim=2, graph_norm='bn').to(DEV)


class _Spy:
    """Counts the calls of entry points of the library (the ctypes functions the wrappers look up on every call)."""

    def __init__(self, monkeypatch, *names):
        self.n = {k: 0 for k in names}
        L = _ffi.lib()
        for k in names:
            monkeypatch.setattr(L, k, self._wrap(k, getattr(L, k)), raising=True)

    def _wrap(self, k, fn):
        def call(*a):
            self.n[k] += 1
            return fn(*a)
        return call


def _steps_against_per_batch_steps(make, pool, p, batches, slots=1):
    """tests/test_gpu_static.py::_static_steps_against_per_batch_steps over StaticBatch(mode='csr'): StaticTrainStep.step_on
    against TrainStep(use_graph=False) on the collated batches, from ONE state per step; every figure is printed before it is
    asserted."""
    from cwn_amd import csr
    from cwn_amd.static_batch import StaticBatch
    from cwn_amd.static_graph import StaticTrainStep
    from cwn_amd.train import TrainStep
    m1, m2 = make(), make()
    m2.load_state_dict(m1.state_dict())
    sb = StaticBatch(p, B, slots=slots, mode='csr')
    sb.set_batch(batches[0])
    st = StaticTrainStep(m1, sb, lr=1e-3)
    ref = TrainStep(m2, [p.collate(idx) for idx in batches], lr=1e-3, use_graph=False)
    for j, idx in enumerate(batches):
        l1 = st.step_on([idx])[0].clone()
        l2 = ref.step(j)
        torch.cuda.synchronize()
        g1, g2 = st.bucket.flat, ref.bucket.flat
        rel = float((g1 - g2).norm() / g2.norm())
        print(f'[static any width] step {j} ({len(idx)} complexes): loss {float(l1):.6f} vs {float(l2):.6f}, relative L2 distance '
              f'of the gradient {rel:.2e}')
        bad, worst = [], 0.0
        for (n_, a), (_, b) in zip(m1.named_buffers(), m2.named_buffers()):
            if a.dtype.is_floating_point:            # BatchNorm running statistics: the batch's own rows only
                worst = max(worst, float((a - b).abs().max()))
                if not torch.allclose(a, b, rtol=5e-3, atol=2e-3):
                    bad.append((n_, float((a - b).abs().max())))
            elif not torch.equal(a, b):
                bad.append((n_, 'counter'))
        print(f'[static any width] step {j}: largest distance of a BatchNorm running statistic {worst:.3e}; outside rtol 5e-3 / '
              f'atol 2e-3: {bad[:4]}')
        assert abs(float(l1) - float(l2)) <= 1e-5 * max(1.0, abs(float(l2))), (j, float(l1), float(l2))
        assert rel < 2e-5, (j, rel)
        assert not bad, (j, bad)
        ref.opt.flat_p.copy_(st.opt.flat_p)
        ref.opt.exp_avg.copy_(st.opt.exp_avg)
        ref.opt.exp_avg_sq.copy_(st.opt.exp_avg_sq)
        for (_, a), (_, b) in zip(m1.named_buffers(), m2.named_buffers()):
            b.copy_(a)
    csr.check_errors(DEV)
    assert len(st._graphs) == 1
    return st


@pytest.mark.parametrize('hidden', [48, 16])
def test_static_train_step_at_other_widths_matches_the_per_batch_step(hidden, monkeypatch):
    """EmbedSparseCIN with BatchNorm at hidden 48 / 16: one captured graph replayed on batches of 20, 7 and 1 complexes inside
    the bounds of test_static_train_step_matches_the_per_batch_step (loss 1e-5 relative, flat gradient 2e-5 relative L2,
    running statistics rtol 5e-3 / atol 2e-3, batch counters equal).  Every update and combine stage goes through
    cwn_linear_stats_f32; without it the capture fails in ops.Gemm.desc ('takes no device-side row count ...')."""
    spy = _Spy(monkeypatch, 'cwn_linear_stats_f32', 'cwn_dense_stage_f32')
    pool, p = _zinc()
    _steps_against_per_batch_steps(lambda: _embed_model(hidden), pool, p, _three_batches(pool))
    print('[static any width] launches recorded:', spy.n)
    assert spy.n['cwn_linear_stats_f32'] > 0 and spy.n['cwn_dense_stage_f32'] == 0


def test_static_train_step_of_sparse_cin_over_raw_features(monkeypatch):
    """SparseCIN(7 -> 64, two layers, BatchNorm): the first layer's 7 -> 64 stage goes through cwn_linear_stats_f32 and its
    backward through reduce + apply + a plain transposed-weight GEMM (the lazy form has no count on cwn_gemm_f32); the 64 -> 64
    stages stay on the stage kernels, forward and backward."""
    spy = _Spy(monkeypatch, 'cwn_linear_stats_f32', 'cwn_dense_stage_f32', 'cwn_dense_stage_bwd_f32', 'cwn_norm_bwd_apply_f32')
    pool, p = _raw()
    _steps_against_per_batch_steps(_raw_model, pool, p, _three_batches(pool, seed=17))
    print('[static any width] launches recorded:', spy.n)
    assert all(v > 0 for v in spy.n.values()), spy.n


def test_two_slots_and_an_epoch_of_three_batches_at_hidden_48():
    """set_epoch + step() with two slots over three batches (the second replay runs one empty slot): the losses against the
    per-batch step, in the form of test_static_train_step_on_reddit_like_batches_with_cross_entropy."""
    from cwn_amd import csr
    from cwn_amd.static_batch import StaticBatch
    from cwn_amd.static_graph import StaticTrainStep
    from cwn_amd.train import TrainStep
    pool, p = _zinc()
    m1, m2 = _embed_model(48, seed=3), _embed_model(48, seed=3)
    m2.load_state_dict(m1.state_dict())
    perm = np.random.default_rng(11).permutation(len(pool))
    epoch = [perm[:B], perm[B:B + 13], perm[B + 13:]]
    sb = StaticBatch(p, B, slots=2, mode='csr')
    st = StaticTrainStep(m1, sb, lr=1e-3)
    ref = TrainStep(m2, [p.collate(idx) for idx in epoch], lr=1e-3, use_graph=False)
    sb.set_epoch(epoch)
    got = []
    for r in range(2):
        got += [float(l) for l in st.step()]
    want = [float(ref.step(j)) for j in range(3)]
    torch.cuda.synchronize()
    csr.check_errors(DEV)
    print('[static any width] two slots, losses', got, 'vs', want)
    for k, (a, b) in enumerate(zip(got, want)):
        tol = 1e-5 if k == 0 else 2e-2            # (later steps: one Adam sign flip of a noise-level gradient apart at most)
        assert abs(a - b) <= tol * max(1.0, abs(b)), (k, got, want)
    assert int(st.opt.t) == 3 == int(ref.opt.t)


def test_entry_point_is_not_called_where_nothing_moved(monkeypatch):
    """A static step at hidden 128 (blocked mode: the stage kernels, as before) and an eager TrainStep at hidden 48 (no
    device-side count: cwn_gemm_f32, as before) never reach cwn_linear_stats_f32."""
    from cwn_amd.static_batch import StaticBatch
    from cwn_amd.static_graph import StaticTrainStep
    from cwn_amd.train import TrainStep
    spy = _Spy(monkeypatch, 'cwn_linear_stats_f32', 'cwn_gemm_f32', 'cwn_dense_stage_f32')
    pool, p = _zinc()
    batches = _three_batches(pool)
    sb = StaticBatch(p, B)
    sb.set_batch(batches[0])
    st = StaticTrainStep(_embed_model(128), sb, lr=1e-3)
    for idx in batches:
        assert torch.isfinite(st.step_on([idx])[0])
    assert spy.n['cwn_linear_stats_f32'] == 0 and spy.n['cwn_dense_stage_f32'] > 0, spy.n
    spy.n['cwn_gemm_f32'] = 0
    ref = TrainStep(_embed_model(48), [p.collate(idx) for idx in batches], lr=1e-3, use_graph=False)
    for j in range(len(batches)):
        assert torch.isfinite(ref.step(j))
    torch.cuda.synchronize()
    assert spy.n['cwn_linear_stats_f32'] == 0 and spy.n['cwn_gemm_f32'] > 0, spy.n
