"""The evaluation half of an epoch on the device: `Evaluator`, `evaluate()` and `infer()` of exp/train_utils.py:77-211.

The reference moves every batch's predictions to the host, concatenates them in numpy and calls sklearn (and the OGB
evaluator); its per-batch `loss.item()` synchronises once per batch.  Here the predictions of the epoch stay on the device
(`run_epoch` of a StaticForward / RoutedForward already returns device tensors), the labels are ONE gather from the packed
dataset (`PackedComplexes.labels`), the per-batch criterion is ONE launch (cwn_loss_segments_f32), the metric a few more
(csrc/cwn_metrics.hip), and the host waits once, for the numbers.

Metrics, as functions of the integer counts the kernels return (include/cwn_hip.h has the definitions):
    ROC-AUC  = (sum lt + 0.5 sum eq) / (n_pos n_neg)        sklearn.metrics.roc_auc_score, ties included
    AP       = ap_sum / n_pos                                sklearn.metrics.average_precision_score, ties included
    MAE      = mean over columns of sum |pred - y| / n       sklearn.metrics.mean_absolute_error
    accuracy = hits / n with numpy's first-maximum argmax    sklearn.metrics.accuracy_score(y, argmax(pred, 1))
The 'ogbg-mol*' metrics restate the published OGB evaluator (each column over its labeled entries, averaged over the columns
that hold a positive and a negative); that package is third party and not available to this repository's tests, so the rule
is NOT pinned against it.  Predictions are compared as the fp32 values the models produce; other dtypes
are cast to fp32 first ('isomorphism' takes float64, as the reference asserts).
"""
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _ffi

_LOSS_KIND = {'regression': 0, 'mse_regression': 1, 'bin_classification': 2, 'classification': 3}      # = CWN_LOSS_*
FLAG_NONFINITE, FLAG_LABEL = 1, 2                       # = CWN_METRIC_FLAG_*
# OGB's master table: average precision for the sets with very few positives, ROC-AUC for the other classification sets
_OGB_AP = ('ogbg-molpcba', 'ogbg-molmuv')
_OGB_ROCAUC = ('ogbg-molhiv', 'ogbg-moltox21', 'ogbg-molbace', 'ogbg-molbbbp', 'ogbg-molclintox', 'ogbg-molsider',
               'ogbg-moltoxcast')


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=device)


def _device_of(*xs, default=None) -> torch.device:
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    return torch.device(default if default is not None else 'cuda')


def _to_dev(x, device, dtype=None) -> torch.Tensor:
    t = torch.as_tensor(x)
    t = t.to(device=device, dtype=dtype if dtype is not None else t.dtype)
    return t.contiguous()


# ---- the launches (device tensors in, device tensors out, nothing waits) ---------------------------------------------------------
def rank_counts(pred: torch.Tensor, y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """cwn_metric_rank_f32 over pred / y [n, cols] (fp32; y: 1, 0 or NaN) -> counts int64 [cols, 4] = (n_pos, n_neg, sum lt,
    sum eq), ap_sum float64 [cols], flag int32 [1]."""
    n, cols = pred.shape
    dev = pred.device
    L = _ffi.lib()
    nbytes = L.cwn_metric_rank_workspace_bytes(n, cols)
    ws = _ws(nbytes, dev)
    counts = torch.empty(cols, 4, dtype=torch.int64, device=dev)
    ap_sum = torch.empty(cols, dtype=torch.float64, device=dev)
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    _ffi.check(L.cwn_metric_rank_f32(pred.data_ptr(), y.data_ptr(), n, cols, ws.data_ptr(), ws.numel(), counts.data_ptr(),
                                     ap_sum.data_ptr(), flag.data_ptr(), _ffi.stream_ptr(dev)), 'cwn_metric_rank_f32')
    return counts, ap_sum, flag


def abs_err(pred: torch.Tensor, y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """cwn_metric_abs_err_f32 over [n, cols] fp32 -> (sum float64 [cols], labeled count int64 [cols])."""
    n, cols = pred.shape
    dev = pred.device
    L = _ffi.lib()
    ws = _ws(L.cwn_metric_abs_err_workspace_bytes(n, cols), dev)
    s = torch.empty(cols, dtype=torch.float64, device=dev)
    c = torch.empty(cols, dtype=torch.int64, device=dev)
    _ffi.check(L.cwn_metric_abs_err_f32(pred.data_ptr(), y.data_ptr(), n, cols, ws.data_ptr(), ws.numel(), s.data_ptr(),
                                        c.data_ptr(), _ffi.stream_ptr(dev)), 'cwn_metric_abs_err_f32')
    return s, c


def argmax_hits(pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """cwn_metric_argmax_hits_f32: pred [n, C] fp32, y [n] int64 -> int64 [1]."""
    n, C = pred.shape
    dev = pred.device
    L = _ffi.lib()
    ws = _ws(L.cwn_metric_argmax_hits_workspace_bytes(n), dev)
    hits = torch.empty(1, dtype=torch.int64, device=dev)
    _ffi.check(L.cwn_metric_argmax_hits_f32(pred.data_ptr(), y.data_ptr(), n, C, ws.data_ptr(), ws.numel(), hits.data_ptr(),
                                            _ffi.stream_ptr(dev)), 'cwn_metric_argmax_hits_f32')
    return hits


def pdist_below(x: torch.Tensor, eps: float) -> torch.Tensor:
    """cwn_metric_pdist_below_f64: x [n, d] float64 -> int64 [1], the pairs i < j closer than eps (Euclidean)."""
    n, d = x.shape
    dev = x.device
    L = _ffi.lib()
    ws = _ws(L.cwn_metric_pdist_below_workspace_bytes(n), dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    _ffi.check(L.cwn_metric_pdist_below_f64(x.data_ptr(), n, d, float(eps), ws.data_ptr(), ws.numel(), count.data_ptr(),
                                            _ffi.stream_ptr(dev)), 'cwn_metric_pdist_below_f64')
    return count


def loss_segments(task_type: str, pred: torch.Tensor, y: torch.Tensor, ptr: torch.Tensor) -> torch.Tensor:
    """cwn_loss_segments_f32: the task's criterion over rows ptr[b] .. ptr[b + 1] of pred [n, cols] for every b -> fp32
    [len(ptr) - 1].  y: fp32 of pred's shape (NaN = no label), or one int64 class per row for 'classification'."""
    kind = _LOSS_KIND[task_type]
    if pred.dtype != torch.float32 or pred.dim() != 2 or not pred.is_contiguous():
        raise TypeError('loss_segments: pred must be a contiguous fp32 [n, cols] tensor')
    n, cols = pred.shape
    if task_type == 'classification':
        if y.dtype != torch.int64 or y.numel() != n:
            raise TypeError('loss_segments: one int64 class per row')
    elif y.dtype != torch.float32 or y.numel() != pred.numel():
        raise TypeError('loss_segments: fp32 targets of the predictions\' shape')
    if ptr.dtype != torch.int64 or ptr.numel() < 2:
        raise TypeError('loss_segments: ptr is an int64 [n_batches + 1] device tensor')
    out = torch.empty(ptr.numel() - 1, dtype=torch.float32, device=pred.device)
    _ffi.check(_ffi.lib().cwn_loss_segments_f32(kind, pred.data_ptr(), y.contiguous().data_ptr(), ptr.data_ptr(), ptr.numel() - 1,
                                                n, cols, out.data_ptr(), _ffi.stream_ptr(pred.device)), 'cwn_loss_segments_f32')
    return out


# ---- the Evaluator ---------------------------------------------------------------------------------------------------------------
class Evaluator(object):
    """exp/train_utils.py:147-211: `Evaluator(metric, **kwargs).eval({'y_pred': ..., 'y_true': ...}) -> float`.
    metric: 'isomorphism' (eps=0.01, p=2), 'accuracy', 'ap', 'mae' or an 'ogbg-mol*' classification set.  y_pred / y_true may
    be device tensors (nothing is copied), CPU tensors or numpy arrays (uploaded; `device=` says where, default the
    current GPU).  One synchronisation per call: the read-out of the result."""

    def __init__(self, metric, **kwargs):
        self.metric = metric
        self.device = kwargs.get('device', None)
        if metric == 'isomorphism':
            self.eps = kwargs.get('eps', 0.01)
            self.p_norm = kwargs.get('p', 2)
            self._launch, self._finish = self._isomorphism, self._isomorphism_value
        elif metric == 'accuracy':
            self._launch, self._finish = self._accuracy, self._accuracy_value
        elif metric == 'ap':
            self._launch, self._finish = self._rank, self._ap_value
        elif metric == 'mae':
            self._launch, self._finish = self._mae, self._mae_value
        elif isinstance(metric, str) and metric in _OGB_AP + _OGB_ROCAUC:
            self._key = 'ap' if metric in _OGB_AP else 'rocauc'
            self._launch, self._finish = self._rank, self._ogb_value
        else:
            raise NotImplementedError('Metric {} is not yet supported.'.format(metric))

    def eval(self, input_dict) -> float:
        return self._finish(*[t.cpu() for t in self._launch(input_dict)])

    # every _launch returns device tensors; the matching _finish takes their host copies
    def launch(self, input_dict) -> List[torch.Tensor]:
        """The metric's launches only (no wait): `finish(*[t.cpu() for t in launch(d)])` is `eval(d)`."""
        return self._launch(input_dict)

    def finish(self, *host) -> float:
        return self._finish(*host)

    def _pair(self, input_dict):
        y_true, y_pred = input_dict['y_true'], input_dict['y_pred']
        assert y_true is not None
        assert y_pred is not None
        dev = _device_of(y_pred, y_true, default=self.device)
        pred = _to_dev(y_pred, dev, torch.float32)
        if pred.dim() == 1:
            pred = pred.view(-1, 1)
        return dev, pred.reshape(pred.size(0), -1), y_true

    def _rank(self, input_dict):
        dev, pred, y_true = self._pair(input_dict)
        y = _to_dev(y_true, dev, torch.float32).reshape(pred.size(0), -1)
        if y.shape != pred.shape:
            raise ValueError(f'y_true {tuple(y.shape)} and y_pred {tuple(pred.shape)} differ in shape')
        return list(rank_counts(pred, y)) + [torch.tensor([pred.size(0)])]

    @staticmethod
    def _check_flag(flag):
        f = int(flag[0])
        if f & FLAG_NONFINITE:
            raise ValueError('y_pred contains NaN or infinity at a labeled entry')
        if f & FLAG_LABEL:
            raise ValueError('y_true holds a label that is neither 0, 1 nor NaN')

    def _ap_value(self, counts, ap_sum, flag, n):
        # sklearn's average_precision_score(y_true, y_pred): the macro mean over the columns; it takes no NaN labels
        self._check_flag(flag)
        n_pos, n_neg = counts[:, 0], counts[:, 1]
        if bool(((n_pos + n_neg) != int(n[0])).any()):
            raise ValueError('y_true contains NaN: the \'ap\' metric does not mask unlabeled entries')
        ap = torch.where(n_pos > 0, ap_sum / n_pos.clamp(min=1).double(), torch.zeros_like(ap_sum))   # (no positive: sklearn gives 0)
        return float(ap.mean())

    def _ogb_value(self, counts, ap_sum, flag, n):
        self._check_flag(flag)
        n_pos, n_neg, lt, eq = (counts[:, k] for k in range(4))
        valid = (n_pos > 0) & (n_neg > 0)
        if not bool(valid.any()):
            raise RuntimeError('No positively labeled data available. Cannot compute ' +
                               ('Average Precision.' if self._key == 'ap' else 'ROC-AUC.'))
        if self._key == 'ap':
            per = ap_sum[valid] / n_pos[valid].double()
        else:
            per = (lt[valid].double() + 0.5 * eq[valid].double()) / (n_pos[valid].double() * n_neg[valid].double())
        return float(per.sum() / int(valid.sum()))

    def _mae(self, input_dict):
        dev, pred, y_true = self._pair(input_dict)
        y = _to_dev(y_true, dev, torch.float32).reshape(pred.size(0), -1)
        if y.shape != pred.shape:
            raise ValueError(f'y_true {tuple(y.shape)} and y_pred {tuple(pred.shape)} differ in shape')
        return list(abs_err(pred, y)) + [torch.tensor([pred.size(0)])]

    def _mae_value(self, s, c, n):
        if bool((c != int(n[0])).any()):
            raise ValueError('y_true contains NaN')
        return float((s / c.double()).mean())

    def _accuracy(self, input_dict):
        dev, pred, y_true = self._pair(input_dict)
        y = _to_dev(y_true, dev, torch.int64).reshape(-1)
        if y.numel() != pred.size(0):
            raise ValueError('accuracy: one class per row of y_pred')
        return [argmax_hits(pred, y), torch.tensor([pred.size(0)])]

    def _accuracy_value(self, hits, n):
        return int(hits[0]) / int(n[0])

    def _isomorphism(self, input_dict):
        # NB: the failure share, the smaller the better (exp/train_utils.py:170-179)
        preds = input_dict['y_pred']
        assert preds is not None
        dtype = preds.dtype
        if not (dtype == torch.float64 if isinstance(preds, torch.Tensor) else np.dtype(dtype) == np.float64):
            raise TypeError(f'isomorphism: float64 predictions, not {dtype}')
        x = _to_dev(preds, _device_of(preds, default=self.device))
        x = x.reshape(x.size(0), -1)
        n = x.size(0)
        if n < 2:
            raise ValueError('isomorphism: at least two embeddings')
        if self.p_norm == 2:
            wrong = pdist_below(x, self.eps)
        else:
            wrong = (torch.pdist(x, p=self.p_norm) < self.eps).sum().view(1)
        return [wrong, torch.tensor([n * (n - 1) // 2])]

    def _isomorphism_value(self, wrong, pairs):
        return int(wrong[0]) / int(pairs[0])


# ---- eval() and infer() ----------------------------------------------------------------------------------------------------------
def _model_of(forward):
    if isinstance(forward, tuple):
        return forward[0]
    return forward.model if hasattr(forward, 'model') else forward.fa.model


def _packed_of(forward):
    sb = forward.sb if hasattr(forward, 'sb') else forward.router.blocked
    return sb.packed


def _predict(forward, batches, want_labels: bool):
    """(predictions [N, out] on the device, labels or None, rows per batch)."""
    model = _model_of(forward)
    model.eval()
    if isinstance(forward, tuple):                            # the eager path: (model, [ComplexBatch, ...])
        data = forward[1] if batches is None else batches
        with torch.no_grad():
            outs = [model(b) for b in data]
        y = torch.cat([b.y.reshape(-1) for b in data]) if want_labels else None
    else:
        batches = [np.asarray(b, dtype=np.int64) for b in batches]
        # uploads first: a copy issued between the replays would wait for them
        y = _packed_of(forward).labels(np.concatenate(batches)) if want_labels else None
        with torch.no_grad():
            outs = forward.run_epoch(batches)
    sizes = [int(o.size(0)) for o in outs]
    return torch.cat(outs, dim=0), y, sizes


def infer(forward, batches=None) -> torch.Tensor:
    """exp/train_utils.py:77-89: the predictions of every batch, concatenated -- on the device.  `forward`: a StaticForward or
    RoutedForward with `batches` = the index arrays of the epoch, or a `(model, [ComplexBatch, ...])` pair (the eager path: the
    embedding models write a batch's embedded features back into it, as the reference's do, so a batch serves one pass)."""
    return _predict(forward, batches, False)[0]


def evaluate(forward, batches, evaluator: Evaluator, task_type: str) -> Tuple[float, float]:
    """exp/train_utils.py:92-144: (evaluator's metric over the epoch's predictions, mean over the batches of the task's
    criterion).  mean_loss is NaN for a task without a criterion ('isomorphism')."""
    want = task_type in _LOSS_KIND
    if want:
        # the segment table goes up before the forwards run
        if isinstance(forward, tuple):
            rows = [int(b.num_complexes) for b in (forward[1] if batches is None else batches)]
        else:
            rows = [len(b) for b in batches]
        dev = next(_model_of(forward).parameters()).device
        ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)).to(dev, non_blocking=True)
    pred, y, sizes = _predict(forward, batches, task_type != 'isomorphism')
    losses: Optional[torch.Tensor] = None
    if want:
        assert sizes == rows, 'a forward returned other row counts than its batches hold'
        if task_type == 'classification':
            targets = y.reshape(-1)
            y_true = y
        else:
            targets = y.to(torch.float32).reshape(pred.shape)
            y_true = y.reshape(pred.shape)
        p2 = pred.reshape(pred.size(0), -1).contiguous()
        losses = loss_segments(task_type, p2, targets, ptr)
    else:
        y_true = y
    res = evaluator.launch({'y_pred': pred, 'y_true': y_true})
    metric = evaluator.finish(*[t.cpu() for t in res])           # the one wait of the pass
    mean_loss = float(np.mean(losses.cpu().numpy().astype(np.float64))) if losses is not None else float('nan')
    return metric, mean_loss
