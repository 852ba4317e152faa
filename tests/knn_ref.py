"""float64 numpy restatement of the nearest-neighbour feature (include/kws.h: kws_rows_normalize, kws_knn, kws_knn_vote;
kws_amd.neighbors): brute-force scores, the total order (score, then the lower reference index) by np.lexsort, the vote,
label_issues and duplicates on top of them.  No torch."""
import numpy as np

DOT, L2 = 0, 1


def normalize(x):
    """-> (unit rows, norms); a zero row stays zero"""
    x = np.asarray(x, np.float64)
    n = np.sqrt((x * x).sum(1))
    return np.where(n[:, None] > 0, x / np.where(n > 0, n, 1.0)[:, None], 0.0), n


def scores(queries, refs, metric):
    q, r = np.asarray(queries, np.float64), np.asarray(refs, np.float64)
    d = q @ r.T
    if metric == DOT:
        return d
    return np.maximum(0.0, (q * q).sum(1)[:, None] + (r * r).sum(1)[None, :] - 2.0 * d)


def knn(queries, refs, k, metric=DOT, exclude=None):
    """-> (idx (Q, k) int32, score (Q, k) float64): per query the k best by (score, lower index); the tail of a short row is -1 with
    -inf (DOT) / +inf (L2).  exclude: None or (Q) reference rows to skip (-1: none)."""
    s = scores(queries, refs, metric)
    Q, N = s.shape
    worst = -np.inf if metric == DOT else np.inf
    idx = np.full((Q, k), -1, np.int32)
    out = np.full((Q, k), worst, np.float64)
    for i in range(Q):
        key = -s[i] if metric == DOT else s[i]                      # ascending key = best first
        order = np.lexsort((np.arange(N), key))                     # last key is the primary one: key, then the index
        if exclude is not None and exclude[i] >= 0:
            order = order[order != exclude[i]]
        order = order[:k]
        idx[i, :order.size] = order
        out[i, :order.size] = s[i, order]
    return idx, out


def vote(idx, score, labels, C, weighted=False, own_labels=None):
    """-> (pred, support[, own]): entries -1 cast no vote, a tie goes to the lower class, no vote at all gives (-1, 0); weighted votes
    count max(score, 0)"""
    idx, labels = np.asarray(idx), np.asarray(labels)
    Q, k = idx.shape
    pred, support, own = np.full((Q,), -1, np.int32), np.zeros((Q,)), np.zeros((Q,))
    for i in range(Q):
        tally = np.zeros((C,))
        for a in range(k):
            if idx[i, a] >= 0:
                tally[labels[idx[i, a]]] += max(float(score[i, a]), 0.0) if weighted else 1.0
        total = tally.sum()
        if total > 0:
            pred[i] = int(np.argmax(tally))                         # the first of equal maxima: the lower class
            support[i] = tally[pred[i]] / total
            if own_labels is not None:
                own[i] = tally[own_labels[i]] / total
    return (pred, support) if own_labels is None else (pred, support, own)


def label_issues(emb, y, C, k=10):
    """-> (rows, label, suggested, own_share, support), sorted by ascending own_share, descending support, row"""
    unit, _ = normalize(emb)
    y = np.asarray(y)
    idx, score = knn(unit, unit, k, DOT, exclude=np.arange(unit.shape[0]))
    pred, support, own = vote(idx, score, y, C, own_labels=y)
    rows = np.nonzero((pred >= 0) & (pred != y))[0]
    rows = rows[np.lexsort((rows, -support[rows], own[rows]))]
    return rows, y[rows], pred[rows], own[rows], support[rows]


def duplicates(emb, other=None, threshold=0.9995, k=4):
    """-> (row_a, row_b, cosine) sorted by (row_a, row_b); inside one set each pair once with row_a < row_b"""
    ua, _ = normalize(emb)
    if other is None:
        idx, score = knn(ua, ua, k, DOT, exclude=np.arange(ua.shape[0]))
    else:
        idx, score = knn(ua, normalize(other)[0], k, DOT)
    pairs = {}
    for a in range(idx.shape[0]):
        for p in range(k):
            b = int(idx[a, p])
            if b >= 0 and score[a, p] >= threshold:
                pairs[(min(a, b), max(a, b)) if other is None else (a, b)] = float(score[a, p])
    keys = sorted(pairs)
    return (np.array([p[0] for p in keys], np.int64), np.array([p[1] for p in keys], np.int64), np.array([pairs[p] for p in keys]))
