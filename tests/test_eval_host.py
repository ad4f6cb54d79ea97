"""Host-side checks of the evaluation pass (cwn_amd/evaluate.py, csrc/cwn_metrics.hip): the C ABI is declared, exported and
validates its arguments before it touches a device; the Evaluator takes the reference's metric names; and the numpy
restatements the GPU suite compares against (tests/_metrics_ref.py) equal sklearn, the library the reference calls."""
import os
import re

import numpy as np
import pytest

from cwn_amd import _ffi
from cwn_amd.evaluate import Evaluator
from tests import _metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('cwn_metric_rank_workspace_bytes', 'cwn_metric_rank_f32', 'cwn_metric_abs_err_workspace_bytes', 'cwn_metric_abs_err_f32',
       'cwn_metric_argmax_hits_workspace_bytes', 'cwn_metric_argmax_hits_f32', 'cwn_metric_pdist_below_workspace_bytes',
       'cwn_metric_pdist_below_f64', 'cwn_loss_segments_f32')
TOL = 2.0 ** -40


def test_entry_points_declared_exported_and_abi_unchanged():
    header = open(os.path.join(ROOT, 'include', 'cwn_hip.h')).read()
    declared = set(re.findall(r'\b(cwn_[a-z0-9_]+)\s*\(', header))
    lib = _ffi.lib()
    for name in NEW:
        assert name in declared and name in _ffi.EXPORTS and hasattr(lib, name), name
    assert lib.cwn_abi_version() == _ffi.ABI_VERSION == 24
    assert int(re.search(r'#define CWN_ABI_VERSION (\d+)', header).group(1)) == 24
    assert int(re.search(r'#define CWN_METRIC_TILE (\d+)', header).group(1)) == 256
    assert int(re.search(r'#define CWN_METRIC_PDIST_TILE (\d+)', header).group(1)) == 64


def test_entry_points_validate_before_any_launch():
    lib = _ffi.lib()
    BAD, TOO_LARGE = 1, 2
    assert lib.cwn_metric_rank_f32(None, None, 8, 1, None, 0, None, None, None, None) == BAD
    assert lib.cwn_metric_rank_f32(None, None, 0, 1, None, 0, None, None, None, None) == BAD
    assert lib.cwn_metric_abs_err_f32(None, None, 8, 1, None, 0, None, None, None) == BAD
    assert lib.cwn_metric_argmax_hits_f32(None, None, 8, 2, None, 0, None, None) == BAD
    assert lib.cwn_metric_pdist_below_f64(None, 8, 4, 0.01, None, 0, None, None) == BAD
    assert lib.cwn_loss_segments_f32(0, None, None, None, 1, 8, 1, None, None) == BAD
    assert lib.cwn_loss_segments_f32(9, None, None, None, 1, 8, 1, None, None) == BAD
    # workspace sizes: a tile of 256 rows holds 256 scores and three 8-byte partials, a column four 8-byte words
    assert lib.cwn_metric_rank_workspace_bytes(1, 1) == 32 + 24 + 1024
    assert lib.cwn_metric_rank_workspace_bytes(257, 3) == 3 * (32 + 2 * 24 + 2 * 1024)
    assert lib.cwn_metric_rank_workspace_bytes(0, 1) == 0 and lib.cwn_metric_rank_workspace_bytes(2 ** 31, 1) == 0
    assert lib.cwn_metric_abs_err_workspace_bytes(1000, 11) == 11 * 16
    assert lib.cwn_metric_argmax_hits_workspace_bytes(5000) == 3 * 8
    assert lib.cwn_metric_pdist_below_workspace_bytes(130) == 9 * 8


def test_evaluator_metric_names():
    for m in ('isomorphism', 'accuracy', 'ap', 'mae', 'ogbg-molhiv', 'ogbg-molpcba', 'ogbg-molmuv', 'ogbg-moltox21',
              'ogbg-moltoxcast', 'ogbg-molbace', 'ogbg-molbbbp', 'ogbg-molclintox', 'ogbg-molsider'):
        Evaluator(m)
    ev = Evaluator('isomorphism', eps=0.5, p=1)
    assert ev.eps == 0.5 and ev.p_norm == 1
    ev = Evaluator('isomorphism')
    assert ev.eps == 0.01 and ev.p_norm == 2
    assert Evaluator('ogbg-molhiv')._key == 'rocauc' and Evaluator('ogbg-molpcba')._key == 'ap'
    assert Evaluator('ogbg-molmuv')._key == 'ap'
    for m in ('rmse', 'f1', 'ogbg-molesol', 'ogbg-ppa', ''):
        with pytest.raises(NotImplementedError, match='is not yet supported'):
            Evaluator(m)


def _cases():
    rng = np.random.default_rng(0)
    for trial in range(60):
        n = int(rng.integers(2, 400))
        y = (rng.random(n) < rng.choice([0.03, 0.3, 0.5, 0.9])).astype(np.float64)
        if y.sum() == 0 or y.sum() == n:
            y[0], y[1] = 1.0, 0.0
        s = rng.standard_normal(n).astype(np.float32)
        if trial % 3 == 1:
            s = (np.round(s * 2) / 2).astype(np.float32)        # heavy ties
        if trial % 3 == 2:
            s[:] = 0.25                                         # all tied
        yield s, y


def test_reference_equals_sklearn():
    met = pytest.importorskip('sklearn.metrics')
    for s, y in _cases():
        assert abs(R.roc_auc(s, y) - met.roc_auc_score(y, s)) <= TOL
        assert abs(R.average_precision(s, y) - met.average_precision_score(y, s)) <= TOL
    rng = np.random.default_rng(1)
    for rounded in (False, True):
        Y = (rng.random((200, 10)) < 0.2).astype(np.float64)
        S = rng.standard_normal((200, 10)).astype(np.float32)
        if rounded:
            S = (np.round(S * 2) / 2).astype(np.float32)
        assert abs(R.average_precision(S, Y) - met.average_precision_score(Y, S)) <= TOL
    for T in (1, 11):
        P = rng.standard_normal((300, T)).astype(np.float32)
        Y = rng.standard_normal((300, T)).astype(np.float32)
        # sklearn gets the same fp32 values as float64 arrays: on fp32 arrays it subtracts and averages in fp32 (its result is
        # then an fp32 number, ~6e-9 from the float64 mean of the same differences), and the kernel promotes first
        assert abs(R.mae(P, Y) - met.mean_absolute_error(Y.astype(np.float64), P.astype(np.float64))) <= TOL
        assert abs(R.mae(P, Y) - met.mean_absolute_error(Y, P)) <= 300 * 2.0 ** -24       # ... and its fp32 form: fp32 rounding
    P = rng.integers(0, 3, (100, 10)).astype(np.float32)         # tied maxima in most rows
    y = rng.integers(0, 10, 100)
    assert R.argmax_hits(P, y) / 100 == met.accuracy_score(y, np.argmax(P, axis=1))


def test_reference_ogb_rule():
    rng = np.random.default_rng(2)
    S = rng.standard_normal((50, 4)).astype(np.float32)
    Y = (rng.random((50, 4)) < 0.4).astype(np.float64)
    Y[::7, 0] = np.nan
    Y[:, 1] = 1.0                                               # single class: skipped
    Y[:, 2] = np.nan                                            # unlabeled: skipped
    lab = ~np.isnan(Y[:, 0])
    want = 0.5 * (R.roc_auc(S[lab, 0], Y[lab, 0]) + R.roc_auc(S[:, 3], Y[:, 3]))
    assert abs(R.ogb_metric(S, Y, 'rocauc') - want) <= TOL
    with pytest.raises(RuntimeError):
        R.ogb_metric(S[:, 1:3], Y[:, 1:3], 'rocauc')
