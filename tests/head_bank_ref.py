"""float64 numpy restatement of kws_heads_apply (include/kws.h, the head-bank block): every row through the Dense(E -> C_h, softmax)
head it names.  No torch, no library.  A head is (kernel (E, C), bias (C)); a bank is a list of heads, None for an empty slot."""
import numpy as np

U = 2.0 ** -24                      # unit roundoff of float32


def gamma(n):
    """Higham's gamma_n for float32: the relative error bound of n chained roundings"""
    return n * U / (1.0 - n * U)


def logits(x, head):
    k, b = head
    return np.asarray(x, np.float64) @ np.asarray(k, np.float64) + np.asarray(b, np.float64)


def logit_bound(x, head):
    """|float32 chain - exact| <= gamma_E (|b_c| + sum_e |x_e W_ec|): the chain acc = b; acc = fma(x_e, W_ec, acc) rounds E times, and
    every rounding error is relative to a partial sum that is at most the sum of the magnitudes"""
    k, b = head
    E = np.asarray(k).shape[0]
    return gamma(E) * (np.abs(np.asarray(x, np.float64)) @ np.abs(np.asarray(k, np.float64)) + np.abs(np.asarray(b, np.float64)))


def softmax(l):
    l = np.asarray(l, np.float64)
    e = np.exp(l - l.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def argmax_low(l):
    """arg-max, an exact tie to the lower class (numpy's argmax returns the first maximum)"""
    return np.argmax(np.asarray(l), axis=-1)


def apply(emb, bank, head_ids, Cmax, rows=None):
    """-> (logits (R, Cmax), bound (R, Cmax), probs (R, Cmax), pred (R)) in float64 / int64.  A row whose head id is outside the bank,
    whose slot is empty or whose row number is outside emb is zeros with pred -1; the columns past a head's classes are zeros."""
    emb = np.asarray(emb, np.float64)
    head_ids = np.asarray(head_ids).reshape(-1)
    R = head_ids.size
    rows = np.arange(R) if rows is None else np.asarray(rows).reshape(-1)
    lg, bd, pr = (np.zeros((R, Cmax)) for _ in range(3))
    pred = np.full(R, -1, np.int64)
    for r in range(R):
        h, s = int(head_ids[r]), int(rows[r])
        if not (0 <= h < len(bank)) or bank[h] is None or not (0 <= s < emb.shape[0]):
            continue
        C = np.asarray(bank[h][1]).shape[0]
        l = logits(emb[s], bank[h])
        lg[r, :C], bd[r, :C], pr[r, :C], pred[r] = l, logit_bound(emb[s], bank[h]), softmax(l), argmax_low(l)
    return lg, bd, pr, pred


def score(emb, y, bank, rows_per_head):
    """-> (hits, n, mean loss) per head on its own rows: hits by arg-max (tie: lower class), loss the mean of -log softmax_y"""
    out = []
    y = np.asarray(y)
    for h, rows in enumerate(rows_per_head):
        rows = np.asarray(rows)
        l = logits(np.asarray(emb, np.float64)[rows], bank[h])
        p = softmax(l)
        out.append((int((argmax_low(l) == y[rows]).sum()), rows.size, float(-np.log(p[np.arange(rows.size), y[rows]]).mean())))
    return out
