"""numpy restatements of the evaluation metrics (cwn_amd/evaluate.py, csrc/cwn_metrics.hip), shared by the host and the GPU
suite: the O(n^2) integer rank counts and the two formulas on top of them, MAE, first-maximum accuracy, the pair-distance
count and the OGB column rule.  tests/test_eval_host.py pins them to sklearn where that is installed."""
import numpy as np


def rank_counts(s, y):
    """One column: scores s (compared as fp32), labels y (1, 0, NaN = unlabeled) -> (n_pos, n_neg, sum lt, sum eq, ap_sum) with
    lt_i / eq_i the negatives below / tied with positive i, ge_i the positives at or above it, and
    ap_sum = sum_i ge_i / (ge_i + n_neg - lt_i) in float64, summed in row order."""
    s = np.asarray(s, dtype=np.float32).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    sp, sn = s[y == 1], s[y == 0]
    n_pos, n_neg = int(sp.size), int(sn.size)
    lt = (sn[None, :] < sp[:, None]).sum(1).astype(np.int64)
    eq = (sn[None, :] == sp[:, None]).sum(1).astype(np.int64)
    ge = (sp[None, :] >= sp[:, None]).sum(1).astype(np.int64)
    terms = ge.astype(np.float64) / (ge + (n_neg - lt)).astype(np.float64) if n_pos else np.zeros(0)
    return n_pos, n_neg, int(lt.sum()), int(eq.sum()), float(np.sum(terms))


def rank_table(S, Y):
    """Every column of S / Y [n, cols] -> (counts int64 [cols, 4], ap_sum float64 [cols])."""
    S, Y = np.asarray(S), np.asarray(Y)
    rows = [rank_counts(S[:, t], Y[:, t]) for t in range(S.shape[1])]
    return np.array([r[:4] for r in rows], dtype=np.int64).reshape(-1, 4), np.array([r[4] for r in rows], dtype=np.float64)


def auc_from(n_pos, n_neg, lt, eq):
    return (lt + 0.5 * eq) / (n_pos * n_neg)


def ap_from(n_pos, ap_sum):
    return ap_sum / n_pos


def roc_auc(s, y):
    n_pos, n_neg, lt, eq, _ = rank_counts(s, y)
    return auc_from(n_pos, n_neg, lt, eq)


def average_precision(s, y):
    """1-D: the column's AP; [n, cols]: the macro mean (sklearn's default for multilabel input)."""
    s, y = np.asarray(s), np.asarray(y)
    if s.ndim == 1:
        n_pos, _, _, _, ap_sum = rank_counts(s, y)
        return ap_from(n_pos, ap_sum)
    return float(np.mean([average_precision(s[:, t], y[:, t]) for t in range(s.shape[1])]))


def mae_sums(P, Y):
    """[n, cols] -> (sum |p - y| in float64 over the labeled rows, their number) per column."""
    P, Y = np.asarray(P, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    lab = ~np.isnan(Y)
    return np.where(lab, np.abs(P - np.where(lab, Y, 0.0)), 0.0).sum(0), lab.sum(0).astype(np.int64)


def mae(P, Y):
    P, Y = np.asarray(P), np.asarray(Y)
    s, c = mae_sums(P.reshape(P.shape[0], -1), Y.reshape(Y.shape[0], -1))
    return float(np.mean(s / c))


def argmax_hits(P, y):
    """Rows whose first maximal column is their class (numpy's argmax)."""
    return int((np.argmax(np.asarray(P), axis=1) == np.asarray(y).reshape(-1)).sum())


def pdist_below(X, eps):
    """Pairs i < j with Euclidean distance below eps, and the smallest relative gap of any pair's distance to eps."""
    X = np.asarray(X, dtype=np.float64)
    i, j = np.triu_indices(X.shape[0], k=1)
    dist = np.sqrt(((X[i] - X[j]) ** 2).sum(1))
    return int((dist < eps).sum()), float(np.min(np.abs(dist - eps)) / eps)


def ogb_metric(S, Y, key):
    """The OGB evaluator's rule for the classification sets: key 'rocauc' or 'ap' per column over its labeled entries,
    averaged over the columns that hold a positive and a negative; RuntimeError without such a column."""
    counts, ap_sum = rank_table(S, Y)
    per = []
    for (n_pos, n_neg, lt, eq), a in zip(counts.tolist(), ap_sum.tolist()):
        if n_pos > 0 and n_neg > 0:
            per.append(auc_from(n_pos, n_neg, lt, eq) if key == 'rocauc' else ap_from(n_pos, a))
    if not per:
        raise RuntimeError('no column with a positive and a negative')
    return sum(per) / len(per)
