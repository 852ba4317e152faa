"""Nearest neighbours over embeddings: dataset hygiene before anything is trained (include/kws.h: kws_rows_normalize, kws_knn,
kws_knn_vote).

    emb = kws_amd.transfer.embed(model, x)          # (N, E) on the GPU: the way in; KWSModel itself has nothing new
    issues = label_issues(emb, y, num_classes)      # rows whose neighbours carry another label, the most suspicious first
    a, b, cos = duplicates(emb)                     # pairs of (near-)identical clips inside one set
    a, b, cos = duplicates(train_emb, val_emb)      # ... and between two sets: leakage across a split
    pred, support = knn_predict(train_emb, train_y, query_emb, k=5, num_classes=C)      # the few-shot baseline that needs no training

All tensors are torch device tensors and the arithmetic is the kernels': exact float32 scores, neighbours in the total order (score,
then the lower reference row), the same bits for every `slices`.  Everything is validated on the host before any device work
(ValueError)."""
import numpy as np

from . import lib as _l

METRICS = ("cosine", "dot", "l2")


class LabelIssues(object):
    """rows: the suspicious rows, the most suspicious first; label: what they carry; suggested: the neighbours' majority; own_share: the
    share of the neighbours that carry the row's own label; support: the share that carry `suggested`.  numpy arrays of equal length."""

    def __init__(self, rows, label, suggested, own_share, support):
        self.rows, self.label, self.suggested, self.own_share, self.support = rows, label, suggested, own_share, support

    def __len__(self):
        return int(self.rows.shape[0])


# ---- host-side validation ------------------------------------------------------------------------------------------------------
def _check_emb(emb, name="emb", need_device=True, min_rows=1):
    import torch
    if not isinstance(emb, torch.Tensor) or emb.dim() != 2 or emb.dtype != torch.float32 or not emb.is_contiguous() or emb.shape[0] < min_rows:
        raise ValueError("%s must be a contiguous float32 tensor of shape (N, E), N >= %d" % (name, min_rows))
    N, E = int(emb.shape[0]), int(emb.shape[1])
    if E < 4 or E > 128 or E % 4:
        raise ValueError("E = %d: the embedding width must be a multiple of 4 in 4..128" % E)
    if N > 2 ** 31 - 1:
        raise ValueError("%s has %d rows, at most 2^31 - 1" % (name, N))
    if need_device and not emb.is_cuda:
        raise ValueError("%s must live on the GPU (kws_amd.transfer.embed returns it there)" % name)
    return N, E


def _check_k(k):
    k = int(k)
    if k < 1 or k > _l.KNN_MAX_K:
        raise ValueError("k = %d: 1..%d neighbours" % (k, _l.KNN_MAX_K))
    return k


def _check_classes(C):
    C = int(C)
    if C < 2 or C > 1024:
        raise ValueError("num_classes = %d: the vote takes 2..1024 classes" % C)
    return C


def _labels(y, N, C, name="labels"):
    import torch
    y = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
    y = y.reshape(-1)
    if y.shape[0] != N:
        raise ValueError("%d %s for %d embeddings" % (y.shape[0], name, N))
    if y.dtype.kind not in "iu":
        raise ValueError("%s must be integers" % name)
    if y.size and (y.min() < 0 or y.max() >= C):
        raise ValueError("%s outside [0, %d)" % (name, C))
    return y.astype(np.int32)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ---- the kernels -------------------------------------------------------------------------------------------------------------------
def normalize(emb):
    """-> (unit, norms): unit[i] = emb[i] / ||emb[i]|| (a zero row stays zero), norms (N) float32.  emb is not written."""
    import torch
    N, E = _check_emb(emb, min_rows=0)
    unit, norms = torch.empty_like(emb), torch.empty((N,), dtype=torch.float32, device=emb.device)
    if N == 0:
        return unit, norms
    with torch.cuda.device(emb.device):
        _l.check(_l.get_lib().kws_rows_normalize(emb.data_ptr(), N, E, unit.data_ptr(), norms.data_ptr(), _stream()))
    return unit, norms


def knn(queries, refs, k, metric="cosine", exclude_self=False, slices=0):
    """For every row of queries (Q, E) its k best rows of refs (N, E) -> (idx (Q, k) int32, score (Q, k) float32), sorted best first, ties
    to the lower row.  metric: 'cosine' (both sides go through normalize, then the dot product; best = largest), 'dot' (best = largest)
    or 'l2' (the squared distance max(0, q.q + r.r - 2 q.r); best = smallest; it loses near-identical rows to cancellation, so look for
    duplicates with cosine).  Where fewer than k candidates exist the tail is idx = -1 with score -inf (+inf for l2).
    exclude_self: query i skips reference row i -- the search of a set in itself.  It requires `queries is refs` or two tensors of equal
    shape (row i of one is then taken to BE row i of the other; nothing compares their contents).
    slices: 0 lets the library cut the reference rows over enough blocks to fill the chip; any value gives the same bits."""
    import torch
    if metric not in METRICS:
        raise ValueError("metric must be one of %s, not %r" % (", ".join(METRICS), metric))
    k = _check_k(k)
    slices = int(slices)
    if slices < 0 or slices > 1024:
        raise ValueError("slices = %d: 0 (the library chooses) or 1..1024" % slices)
    Q, E = _check_emb(queries, "queries", need_device=False, min_rows=0)
    N, E2 = _check_emb(refs, "refs", need_device=False)
    if E != E2:
        raise ValueError("queries are %d wide, refs %d" % (E, E2))
    if exclude_self and queries is not refs and tuple(queries.shape) != tuple(refs.shape):
        raise ValueError("exclude_self needs `queries is refs` or equal shapes, got %s and %s" % (tuple(queries.shape), tuple(refs.shape)))
    _check_emb(queries, "queries", min_rows=0)
    _check_emb(refs, "refs")
    if queries.device != refs.device:
        raise ValueError("queries and refs live on different devices")
    dev = refs.device
    if Q == 0:
        return torch.empty((0, k), dtype=torch.int32, device=dev), torch.empty((0, k), dtype=torch.float32, device=dev)
    if metric == "cosine":
        same = queries is refs
        refs = normalize(refs)[0]
        queries = refs if same else normalize(queries)[0]
    L = _l.get_lib()
    idx = torch.empty((Q, k), dtype=torch.int32, device=dev)
    score = torch.empty((Q, k), dtype=torch.float32, device=dev)
    need = int(L.kws_knn_workspace_bytes(Q, N, E, k, slices))
    if need < 0:
        _l.check(need)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev) if need else None
    excl = torch.arange(Q, dtype=torch.int32, device=dev) if exclude_self else None
    with torch.cuda.device(dev):
        _l.check(L.kws_knn(queries.data_ptr(), Q, refs.data_ptr(), N, E, _l.KNN_METRICS["l2" if metric == "l2" else "dot"], k,
                           excl.data_ptr() if excl is not None else None, slices, idx.data_ptr(), score.data_ptr(),
                           ws.data_ptr() if ws is not None else None, need, _stream()))
    return idx, score


def vote(idx, score, labels, num_classes, weighted=False, own_labels=None, metric="cosine"):
    """The neighbours' votes (kws_knn_vote).  idx / score (Q, k) as knn returns them, labels (N) of the reference rows (host or device
    integers in [0, num_classes)).  -> (pred (Q) int32, support (Q) float32[, own (Q) float32 when own_labels (Q) is given]).  An entry
    idx = -1 casts no vote, a tie goes to the lower class, a query without a vote gets pred -1 and support 0.  weighted: a vote counts
    its score (negative scores count 0), which has a meaning for similarities only: with metric 'l2' it is refused."""
    import torch
    if metric not in METRICS:
        raise ValueError("metric must be one of %s, not %r" % (", ".join(METRICS), metric))
    if weighted and metric == "l2":
        raise ValueError("weighted votes count similarities: not with metric 'l2'")
    C = _check_classes(num_classes)
    for name, t, dt in (("idx", idx, torch.int32), ("score", score, torch.float32)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != dt or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor of shape (Q, k)" % (name, dt))
    if tuple(idx.shape) != tuple(score.shape):
        raise ValueError("idx is %s, score %s" % (tuple(idx.shape), tuple(score.shape)))
    Q, k = int(idx.shape[0]), _check_k(idx.shape[1])
    n_lab = int(labels.numel()) if isinstance(labels, torch.Tensor) else int(np.asarray(labels).size)
    if n_lab < 1:
        raise ValueError("no labels")
    lab = _labels(labels, n_lab, C)
    own = _labels(own_labels, Q, C, "own labels") if own_labels is not None else None
    if not idx.is_cuda or not score.is_cuda:
        raise ValueError("idx and score must live on the GPU (knn returns them there)")
    dev = idx.device
    lab_d = torch.from_numpy(lab).to(dev)
    own_d = torch.from_numpy(own).to(dev) if own is not None else None
    pred = torch.empty((Q,), dtype=torch.int32, device=dev)
    support = torch.empty((Q,), dtype=torch.float32, device=dev)
    own_share = torch.empty((Q,), dtype=torch.float32, device=dev) if own is not None else None
    if Q == 0:
        return (pred, support) if own is None else (pred, support, own_share)
    with torch.cuda.device(dev):
        _l.check(_l.get_lib().kws_knn_vote(idx.data_ptr(), score.data_ptr(), Q, k, lab_d.data_ptr(), n_lab, C, 1 if weighted else 0,
                                           own_d.data_ptr() if own_d is not None else None, pred.data_ptr(), support.data_ptr(),
                                           own_share.data_ptr() if own_share is not None else None, _stream()))
    return (pred, support) if own is None else (pred, support, own_share)


# ---- what people ask of their data -------------------------------------------------------------------------------------------------
def knn_predict(train_emb, train_y, query_emb, k, num_classes, weighted=False):
    """k-NN on frozen embeddings with cosine similarity: -> (pred (Q) int32, support (Q) float32) on the GPU.  weighted: the neighbours
    vote with their cosine instead of 1 each."""
    C = _check_classes(num_classes)
    k = _check_k(k)
    N, E = _check_emb(train_emb, "train_emb", need_device=False)
    _labels(train_y, N, C)
    _check_emb(query_emb, "query_emb", need_device=False, min_rows=0)
    idx, score = knn(query_emb, train_emb, k, "cosine")
    return vote(idx, score, train_y, C, weighted=weighted)


def label_issues(emb, y, num_classes, k=10):
    """The rows of emb (N, E) / y (N) whose own label is not the majority of their k nearest OTHER rows (cosine) -> LabelIssues, sorted by
    ascending own_share, then descending support, then the row number."""
    C = _check_classes(num_classes)
    k = _check_k(k)
    N, E = _check_emb(emb, need_device=False)
    yh = _labels(y, N, C)
    idx, score = knn(emb, emb, k, "cosine", exclude_self=True)
    pred, support, own = vote(idx, score, yh, C, own_labels=yh)
    pred, support, own = pred.cpu().numpy(), support.cpu().numpy(), own.cpu().numpy()
    rows = np.nonzero((pred >= 0) & (pred != yh))[0]
    order = np.lexsort((rows, -support[rows].astype(np.float64), own[rows].astype(np.float64)))
    rows = rows[order]
    return LabelIssues(rows.astype(np.int64), yh[rows], pred[rows], own[rows], support[rows])


def duplicates(emb, other=None, threshold=0.9995, k=4):
    """Pairs of rows whose cosine is at or above `threshold` -> (row_a, row_b, cosine), numpy arrays sorted by (row_a, row_b).  Inside one
    set (other None) every pair is reported once, with row_a < row_b; with `other`, row_a indexes emb and row_b indexes other -- the
    leakage check between a training and a validation set.  Every row reports at most its k nearest, so a clip with more than k copies
    needs a larger k to list them all."""
    k = _check_k(k)
    threshold = float(threshold)
    if not -1.0 <= threshold <= 1.0:
        raise ValueError("threshold = %g is no cosine" % threshold)
    _check_emb(emb, need_device=False)
    if other is not None:
        _check_emb(other, "other", need_device=False)
        idx, score = knn(emb, other, k, "cosine")
    else:
        idx, score = knn(emb, emb, k, "cosine", exclude_self=True)
    idx, score = idx.cpu().numpy(), score.cpu().numpy()
    a, pos = np.nonzero((idx >= 0) & (score >= np.float32(threshold)))
    b, c = idx[a, pos].astype(np.int64), score[a, pos]
    a = a.astype(np.int64)
    if other is None:
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        pairs, first = np.unique(np.stack([lo, hi], 1), axis=0, return_index=True) if a.size else (np.zeros((0, 2), np.int64), np.zeros((0,), np.int64))
        return pairs[:, 0], pairs[:, 1], c[first]
    order = np.lexsort((b, a))
    return a[order], b[order], c[order]
