"""The evaluation pass on the device (cwn_amd/evaluate.py, csrc/cwn_metrics.hip) against the numpy restatements of
tests/_metrics_ref.py (pinned to sklearn by tests/test_eval_host.py) and against torch's criteria in float64.

Shapes sit around what the kernels tile by: 256 rows for the rank kernel (CWN_METRIC_TILE: 255 / 256 / 257, and 1000 = four
tiles with a ragged last one), 2048 rows per workgroup of the strided reductions (2049: two partials), 64 rows and 32
columns for the pair distances (65, 130; d = 33)."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _metrics_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2.0 ** -40


def _gate(got, ref):
    """The project's gate: 1e-5 * max(1, |ref|_inf)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max()), (got, ref)


# ---- rank counts -----------------------------------------------------------------------------------------------------------------
def _scores(kind, n, cols, rng):
    s = rng.standard_normal((n, cols)).astype(np.float32)
    if kind == 'rounded':
        s = (np.round(s * 2) / 2).astype(np.float32)
    elif kind == 'equal':
        s[:] = 0.25
    elif kind == 'zeros':
        s = np.where(rng.random((n, cols)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        assert n < 8 or (np.signbit(s).any() and not np.signbit(s).all())
    return s


def _labels(n, cols, rng):
    y = (rng.random((n, cols)) < 0.3).astype(np.float32)
    y[rng.random((n, cols)) < 0.15] = np.nan
    if cols >= 3:
        y[:, 1] = 1.0            # all positive
        y[:, 2] = np.nan         # all unlabeled
    return y


@pytest.mark.parametrize('cols', [1, 3])
@pytest.mark.parametrize('n', [1, 2, 255, 256, 257, 1000])
def test_rank_counts(n, cols):
    from cwn_amd.evaluate import rank_counts
    rng = np.random.default_rng(1000 * cols + n)
    y = _labels(n, cols, rng)
    for kind in ('random', 'rounded', 'equal', 'zeros'):
        s = _scores(kind, n, cols, rng)
        want_c, want_ap = R.rank_table(s, y)
        sd, yd = torch.from_numpy(s).to(DEV), torch.from_numpy(y).to(DEV)
        counts, ap_sum, flag = rank_counts(sd, yd)
        counts2, ap_sum2, flag2 = rank_counts(sd, yd)
        assert int(flag.cpu()) == 0 and int(flag2.cpu()) == 0
        assert torch.equal(counts.cpu(), torch.from_numpy(want_c)), (kind, counts.cpu(), want_c)
        assert torch.equal(counts, counts2) and torch.equal(ap_sum.view(torch.int64), ap_sum2.view(torch.int64))   # same bits
        got_ap = ap_sum.cpu().numpy()
        for t, (n_pos, n_neg, lt, eq) in enumerate(want_c.tolist()):
            if n_pos:
                d_ap = abs(got_ap[t] / n_pos - R.ap_from(n_pos, want_ap[t]))
                print(f'n {n} cols {cols} {kind} column {t}: |ap - ref| {d_ap:.3e}')
                assert d_ap <= TOL
            else:
                assert got_ap[t] == 0.0
            if n_pos and n_neg:
                c = counts[t].cpu().tolist()
                d_auc = abs(R.auc_from(*c) - R.auc_from(n_pos, n_neg, lt, eq))
                assert d_auc <= TOL


def test_rank_nonfinite_predictions_and_bad_labels():
    from cwn_amd.evaluate import Evaluator
    rng = np.random.default_rng(3)
    s = rng.standard_normal((300, 2)).astype(np.float32)
    y = (rng.random((300, 2)) < 0.4).astype(np.float32)
    y[7, 1] = np.nan
    y[290, 0] = np.nan
    ev = Evaluator('ogbg-molhiv')
    ok = ev.eval({'y_pred': torch.from_numpy(s).to(DEV), 'y_true': torch.from_numpy(y).to(DEV)})
    s_un = s.copy()
    s_un[7, 1], s_un[290, 0] = np.inf, np.nan                     # at unlabeled entries: ignored with them
    assert ev.eval({'y_pred': torch.from_numpy(s_un).to(DEV), 'y_true': torch.from_numpy(y).to(DEV)}) == ok
    for bad in (np.inf, -np.inf, np.nan):
        s_lab = s.copy()
        s_lab[280, 1] = bad                                       # a labeled entry of the second tile
        with pytest.raises(ValueError):
            ev.eval({'y_pred': torch.from_numpy(s_lab).to(DEV), 'y_true': torch.from_numpy(y).to(DEV)})
    y_bad = y.copy()
    y_bad[5, 0] = 2.0
    with pytest.raises(ValueError):
        ev.eval({'y_pred': torch.from_numpy(s).to(DEV), 'y_true': torch.from_numpy(y_bad).to(DEV)})
    with pytest.raises(ValueError):                                # 'ap' is sklearn's call: it takes no NaN labels
        Evaluator('ap').eval({'y_pred': s, 'y_true': y})


def test_evaluator_ap_and_ogb_rule():
    from cwn_amd.evaluate import Evaluator
    rng = np.random.default_rng(4)
    n, cols = 300, 10
    s = (np.round(rng.standard_normal((n, cols)) * 2) / 2).astype(np.float32)
    y = (rng.random((n, cols)) < 0.2).astype(np.float32)
    # 'ap': the macro mean over the columns; numpy in, device in: the same float
    want = R.average_precision(s, y)
    got_np = Evaluator('ap').eval({'y_pred': s, 'y_true': y})
    got_dev = Evaluator('ap').eval({'y_pred': torch.from_numpy(s).to(DEV), 'y_true': torch.from_numpy(y).to(DEV)})
    assert isinstance(got_np, float) and got_np == got_dev and abs(got_np - want) <= TOL
    # the OGB rule: columns over their labeled entries, single-class and unlabeled columns skipped
    y[rng.random((n, cols)) < 0.2] = np.nan
    y[:, 1] = 1.0
    y[:, 2] = 0.0
    y[:, 3] = np.nan
    for name, key in (('ogbg-molhiv', 'rocauc'), ('ogbg-moltox21', 'rocauc'), ('ogbg-molpcba', 'ap'), ('ogbg-molmuv', 'ap')):
        got = Evaluator(name).eval({'y_pred': torch.from_numpy(s).to(DEV), 'y_true': torch.from_numpy(y).to(DEV)})
        assert abs(got - R.ogb_metric(s, y, key)) <= TOL, name
        assert 0.0 <= got <= 1.0
    for name in ('ogbg-molhiv', 'ogbg-molpcba'):
        with pytest.raises(RuntimeError):                          # no column with both classes
            Evaluator(name).eval({'y_pred': s[:, 1:4], 'y_true': y[:, 1:4]})
    # one column as a 1-D array
    lab = ~np.isnan(y[:, 0])
    got = Evaluator('ogbg-molhiv').eval({'y_pred': s[:, 0], 'y_true': y[:, 0]})
    assert abs(got - R.roc_auc(s[lab, 0], y[lab, 0])) <= TOL


# ---- MAE, accuracy ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [1, 11])
@pytest.mark.parametrize('n', [1, 255, 2049, 5000])
def test_mae(n, T):
    from cwn_amd.evaluate import Evaluator, abs_err
    rng = np.random.default_rng(10 * n + T)
    p = rng.standard_normal((n, T)).astype(np.float32)
    y = rng.standard_normal((n, T)).astype(np.float32)
    pd_, yd = torch.from_numpy(p).to(DEV), torch.from_numpy(y).to(DEV)
    got = Evaluator('mae').eval({'y_pred': pd_, 'y_true': yd})
    want = R.mae(p, y)
    print(f'mae n {n} T {T}: relative difference {abs(got - want) / want:.3e}')
    assert abs(got - want) <= n * 2.0 ** -52 * want
    assert got == Evaluator('mae').eval({'y_pred': pd_, 'y_true': yd})          # same bits
    # the kernel's own outputs, with unlabeled entries: per-column float64 sums and labeled counts
    y[rng.random((n, T)) < 0.2] = np.nan
    s, c = abs_err(pd_, torch.from_numpy(y).to(DEV))
    want_s, want_c = R.mae_sums(p, y)
    assert torch.equal(c.cpu(), torch.from_numpy(want_c))
    assert np.all(np.abs(s.cpu().numpy() - want_s) <= n * 2.0 ** -52 * np.maximum(want_s, 1e-300))
    if np.isnan(y).any():
        with pytest.raises(ValueError):
            Evaluator('mae').eval({'y_pred': pd_, 'y_true': torch.from_numpy(y).to(DEV)})


@pytest.mark.parametrize('C', [2, 10])
@pytest.mark.parametrize('n', [1, 257, 2049])
def test_accuracy_first_maximum(n, C):
    from cwn_amd.evaluate import Evaluator
    rng = np.random.default_rng(100 * n + C)
    p = rng.integers(0, 3, (n, C)).astype(np.float32)             # small integers: most rows hold tied maxima
    assert n < 8 or ((p == p.max(1, keepdims=True)).sum(1) > 1).any()
    if n > 8:
        p[5, C - 1] = np.nan                                      # numpy's argmax takes the first NaN
    y = rng.integers(0, C, n)
    y[::3] = np.argmax(p, axis=1)[::3]
    want = R.argmax_hits(p, y) / n
    ev = Evaluator('accuracy')
    assert ev.eval({'y_pred': torch.from_numpy(p).to(DEV), 'y_true': torch.from_numpy(y).to(DEV)}) == want
    assert ev.eval({'y_pred': p, 'y_true': y.reshape(-1, 1)}) == want


# ---- isomorphism -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [1, 16, 33])
@pytest.mark.parametrize('n', [2, 3, 65, 130])
def test_pdist_count(n, d):
    from cwn_amd.evaluate import Evaluator, pdist_below
    rng = np.random.default_rng(7 * n + d)
    centres = rng.standard_normal((5, d)) * 3.0
    x = centres[rng.integers(0, 5, n)] + 1e-4 * rng.standard_normal((n, d))
    eps = 0.01
    want, gap = R.pdist_below(x, eps)
    assert gap > 1e-9                                             # no pair sits on the threshold
    xt = torch.from_numpy(x)
    assert want == int((torch.pdist(xt) < eps).sum())
    got = pdist_below(xt.to(DEV), eps)
    assert int(got.cpu()) == want
    pairs = n * (n - 1) // 2
    assert Evaluator('isomorphism').eval({'y_pred': xt.to(DEV)}) == want / pairs
    assert Evaluator('isomorphism').eval({'y_pred': x}) == want / pairs
    assert Evaluator('isomorphism', p=1).eval({'y_pred': x}) == int((torch.pdist(xt, p=1) < eps).sum()) / pairs
    with pytest.raises(TypeError):
        Evaluator('isomorphism').eval({'y_pred': xt.float().to(DEV)})


# ---- the per-batch criterion -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cols', [1, 10])
@pytest.mark.parametrize('task', ['regression', 'mse_regression', 'bin_classification', 'classification'])
def test_loss_segments(task, cols):
    from cwn_amd.evaluate import loss_segments
    from cwn_amd.train import _LOSSES
    rng = np.random.default_rng(cols + len(task))
    sizes = [1, 7, 128, 7]                                        # the last batch carries no label at all
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(ptr[-1])
    pred = torch.from_numpy((2.0 * rng.standard_normal((n, cols))).astype(np.float32))
    crit = _LOSSES[task]
    if task == 'classification':
        y = torch.from_numpy(rng.integers(0, cols, n))
        y[3] = -100                                               # torch's ignore_index
        y[ptr[3]:] = -100
        ref = [crit(pred[a:b].double(), y[a:b]) for a, b in zip(ptr[:-1], ptr[1:])]
    else:
        y = torch.from_numpy(rng.standard_normal((n, cols)).astype(np.float32))
        if task == 'bin_classification':
            y = (y > 0).float()
        y[rng.random((n, cols)) < 0.1] = float('nan')
        y[0] = 0.5 if task != 'bin_classification' else 1.0       # (the one-row batch keeps its labels)
        y[ptr[3]:] = float('nan')
        ref = []
        for a, b in zip(ptr[:-1], ptr[1:]):
            m = ~torch.isnan(y[a:b])
            ref.append(crit(pred[a:b][m].double(), y[a:b][m].double()))
    ref = torch.stack(ref).numpy()
    got = loss_segments(task, pred.to(DEV), y.to(DEV), torch.from_numpy(ptr).to(DEV)).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (4,)
    assert np.isnan(ref[3]) and np.isnan(got[3])
    print(f'{task} cols {cols}: |got - ref| {np.abs(got[:3] - ref[:3]).max():.3e}')
    _gate(got[:3], ref[:3])


# ---- labels, infer, evaluate -------------------------------------------------------------------------------------------------------
def _pool(n=40, seed=11, labels='regression'):
    from cwn_amd.packed import PackedComplexes
    from cwn_amd.synthetic import zinc_like_complexes
    pool = zinc_like_complexes(n, seed=seed, max_ring=6, n_lo=9, n_hi=24)
    rng = np.random.default_rng(seed)
    for k, c in enumerate(pool):
        if labels == 'multi':
            c.y = torch.from_numpy(rng.standard_normal((1, 3)).astype(np.float32))
        elif labels == 'class':
            c.y = torch.tensor([int(rng.integers(0, 4))], dtype=torch.int64)
        elif labels == 'binary':
            c.y = torch.tensor([[float('nan') if k % 5 == 0 else float(rng.integers(0, 2))]])
    return pool, PackedComplexes(pool, DEV, max_dim=2, with_csr=True)


@pytest.mark.parametrize('labels', ['regression', 'multi', 'class'])
def test_labels_equal_the_collated_batch(labels):
    pool, p = _pool(12, labels=labels)
    idx = np.random.default_rng(0).permutation(12)[:9]
    got, want = p.labels(idx), p.collate(idx).y
    assert got.dtype == want.dtype and got.dtype == (torch.int64 if labels == 'class' else torch.float32)
    assert torch.equal(got, want) and got.numel() == (27 if labels == 'multi' else 9)
    with pytest.raises(IndexError):
        p.labels([12])


def _model(seed=0):
    from cwn_amd.models import EmbedSparseCIN
    torch.manual_seed(seed)
    return EmbedSparseCIN(28, 4, 1, 2, 64, dropout_rate=0.0, max_dim=2, jump_mode=None, nonlinearity='relu', readout='sum',
                          train_eps=False, final_hidden_multiplier=2, final_readout='sum', init_reduce='sum', embed_edge=True,
                          use_coboundaries=True, graph_norm='bn').to(DEV).eval()


def _forwards(model, p, B):
    from cwn_amd.static_batch import StaticBatch
    from cwn_amd.static_graph import RoutedForward, StaticForward, StaticRouter
    return {'static': StaticForward(model, StaticBatch(p, B, slots=2)), 'routed': RoutedForward(model, StaticRouter(p, B, slots=2))}


def test_infer_and_evaluate_end_to_end():
    from cwn_amd.evaluate import Evaluator, evaluate, infer
    B = 16
    batches = [np.arange(lo, min(lo + B, 40)) for lo in range(0, 40, B)]          # 16, 16, 8
    pool, p = _pool(40)
    model = _model()
    fw = _forwards(model, p, B)
    fresh = lambda: [p.collate(idx) for idx in batches]          # (a model embeds a batch's features in place: one use each)
    collated = fresh()
    l1 = torch.nn.L1Loss()
    for name in ('static', 'routed', 'eager'):
        if name == 'eager':
            with torch.no_grad():
                outs = [model(b) for b in fresh()]
            pred = infer((model, fresh()))
            metric, mean_loss = evaluate((model, fresh()), None, Evaluator('mae'), 'regression')
        else:
            with torch.no_grad():
                outs = [o.clone() for o in fw[name].run_epoch(batches)]
            pred = infer(fw[name], batches)
            metric, mean_loss = evaluate(fw[name], batches, Evaluator('mae'), 'regression')
        assert pred.is_cuda and torch.equal(pred, torch.cat(outs, 0)), name            # bit-identical
        y = p.labels(np.concatenate(batches)).view(pred.shape)
        want_metric = float((pred.double() - y.double()).abs().mean())
        want_loss = float(np.mean([float(l1(o.double(), b.y.view(o.shape).double())) for o, b in zip(outs, collated)]))
        print(f'{name}: mae {metric:.6f} (torch {want_metric:.6f}), mean loss {mean_loss:.6f} (torch {want_loss:.6f})')
        assert isinstance(metric, float) and isinstance(mean_loss, float)
        _gate([metric], [want_metric])
        _gate([mean_loss], [want_loss])
    # isomorphism has no criterion: the loss is NaN
    x = torch.randn(6, 4, dtype=torch.float64, device=DEV)

    class Fixed(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1, device=DEV))

        def forward(self, b):
            return b

    m, loss = evaluate((Fixed(), [x[:3], x[3:]]), None, Evaluator('isomorphism'), 'isomorphism')
    assert m == 0.0 and math.isnan(loss)


def test_evaluate_bin_classification_with_unlabeled_molecules():
    from cwn_amd.evaluate import Evaluator, evaluate
    B = 16
    batches = [np.arange(lo, min(lo + B, 40)) for lo in range(0, 40, B)]
    pool, p = _pool(40, labels='binary')
    model = _model(1)
    bce = torch.nn.BCEWithLogitsLoss()
    for name, fwd in _forwards(model, p, B).items():
        metric, mean_loss = evaluate(fwd, batches, Evaluator('ogbg-molhiv'), 'bin_classification')
        with torch.no_grad():
            outs = [o.clone() for o in fwd.run_epoch(batches)]
        pred = torch.cat(outs, 0).cpu().numpy()
        y = torch.cat([c.y for c in pool], 0).numpy()
        assert np.isnan(y).sum() == 8
        assert abs(metric - R.ogb_metric(pred, y, 'rocauc')) <= TOL and 0.0 <= metric <= 1.0, name
        want = []
        for o, idx in zip(outs, batches):
            t = torch.from_numpy(y[idx]).to(DEV)
            m = ~torch.isnan(t)
            want.append(float(bce(o[m].double(), t[m].double())))
        _gate([mean_loss], [float(np.mean(want))])


def test_example_trains_and_reports_roc_auc():
    pr = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'train_molhiv_eval.py'), '256', '2'], capture_output=True,
                        text=True, timeout=600)
    assert pr.returncode == 0, pr.stdout[-2000:] + pr.stderr[-2000:]
    aucs = [float(v) for v in re.findall(r'ROC-AUC ([0-9.]+)', pr.stdout)]
    assert len(aucs) == 2 and all(0.0 <= a <= 1.0 for a in aucs), pr.stdout
    assert len(re.findall(r'mean loss ([0-9.]+)', pr.stdout)) == 2
