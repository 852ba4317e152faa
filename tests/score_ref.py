"""numpy reference of kws_score_hist (include/kws.h) and of the curve arithmetic of kws_amd.metrics: the fp32 binning rule, the three
count arrays by np.add.at and plain loops, and a brute-force pairwise AUC over binned scores.  Shared by test_score_host.py and
test_score_gpu.py; everything here is integers, so the comparisons with the device are exact."""
import numpy as np


def score_bin(p, bins):
    """bin of fp32 scores: !(p > 0) -> 0 (zero, negatives, NaN); p >= 1 -> bins - 1; else min(bins - 1, (int)(p * (float)bins)) in fp32"""
    p = np.asarray(p, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = p * np.float32(bins)                                   # fp32 product, as on the device
        inner = np.minimum(np.nan_to_num(prod, nan=0.0, posinf=0.0, neginf=0.0), np.float32(bins)).astype(np.int64)
        b = np.where(p >= np.float32(1), bins - 1, np.minimum(bins - 1, inner))
        b = np.where(p > np.float32(0), b, 0)
    return b.astype(np.int64)


def true_rank(probs, labels):
    """rank of the true class of every row (labels valid): #{c: p_c > p_y} + #{c < y: p_c == p_y}; a row with a NaN -> C - 1"""
    probs = np.asarray(probs, np.float32)
    B, C = probs.shape
    py = probs[np.arange(B), labels][:, None]
    idx = np.arange(C)[None, :]
    with np.errstate(invalid="ignore"):
        ahead = (probs > py) | ((probs == py) & (idx < np.asarray(labels)[:, None]))
    rank = ahead.sum(1)
    rank[np.isnan(probs).any(1)] = C - 1
    return rank.astype(np.int64)


def score_counts(probs, labels, bins, out=None):
    """-> (hist (C, 2, bins), rank_counts (C,), calib (2, bins)) int64 of a batch; `out` = a tuple of arrays to accumulate into"""
    probs = np.asarray(probs, np.float32)
    labels = np.asarray(labels, np.int64).reshape(-1)
    B, C = probs.shape
    hist, rank_counts, calib = out if out is not None else (np.zeros((C, 2, bins), np.int64), np.zeros((C,), np.int64),
                                                            np.zeros((2, bins), np.int64))
    keep = (labels >= 0) & (labels < C)
    p, y = probs[keep], labels[keep]
    if len(y) == 0:
        return hist, rank_counts, calib
    b = score_bin(p, bins)                                            # (n, C)
    cls = np.broadcast_to(np.arange(C)[None, :], b.shape)
    is_target = (cls == y[:, None]).astype(np.int64)
    np.add.at(hist, (cls.ravel(), is_target.ravel(), b.ravel()), 1)
    rank = true_rank(p, y)
    np.add.at(rank_counts, rank, 1)
    top_bin = b.max(1)                                                # the bin of the largest score: binning is monotone, NaN -> bin 0
    np.add.at(calib[0], top_bin, 1)
    np.add.at(calib[1], top_bin[rank == 0], 1)
    return hist, rank_counts, calib


def score_counts_loops(probs, labels, bins):
    """the same three arrays by plain Python loops (small inputs): an independent statement of the definitions"""
    probs = np.asarray(probs, np.float32)
    B, C = probs.shape
    hist, rank_counts, calib = np.zeros((C, 2, bins), np.int64), np.zeros((C,), np.int64), np.zeros((2, bins), np.int64)
    for i in range(B):
        y = int(labels[i])
        if y < 0 or y >= C:
            continue
        bs = [int(score_bin(probs[i, c], bins)) for c in range(C)]
        for c in range(C):
            hist[c, 1 if c == y else 0, bs[c]] += 1
        if np.isnan(probs[i]).any():
            r = C - 1
        else:
            r = sum(1 for c in range(C) if probs[i, c] > probs[i, y] or (probs[i, c] == probs[i, y] and c < y))
        rank_counts[r] += 1
        calib[0, max(bs)] += 1
        if r == 0:
            calib[1, max(bs)] += 1
    return hist, rank_counts, calib


def pairwise_auc(target_hist, non_target_hist):
    """Mann-Whitney AUC of two bin-count vectors by brute force over all pairs of bins, in exact rational arithmetic -> float"""
    from fractions import Fraction
    t, n = [int(v) for v in target_hist], [int(v) for v in non_target_hist]
    T, N = sum(t), sum(n)
    if T == 0 or N == 0:
        return float("nan")
    wins = Fraction(0)
    for i, ti in enumerate(t):
        if ti == 0:
            continue
        for j, nj in enumerate(n):
            if nj == 0:
                continue
            if i > j:
                wins += ti * nj
            elif i == j:
                wins += Fraction(ti * nj, 2)
    return float(wins / (T * N))
