"""numpy restatement of the KL (entropy) calibration of include/kws.h: the binning of the histogram pass and the KL search of
kws_quant_kl_ranges, written from the contract (double throughout, the groups split with integer arithmetic)."""
import numpy as np

BINS = 2048
GROUPS = 128


def bin_factor(amax):
    """k_t = (float)(2048.0 / (double)amax_t), 0 for amax_t == 0"""
    a = float(np.float32(amax))
    return np.float32(2048.0 / a) if a > 0 else np.float32(0.0)


def histogram(values, amax):
    """counts of the nonzero |values| binned by amax as the histogram pass bins them (one fp32 multiply, truncation)"""
    k = bin_factor(amax)
    h = np.zeros(BINS, np.int64)
    if k == 0:
        return h
    v = np.abs(np.asarray(values, np.float32).reshape(-1))
    v = v[v != 0]
    b = np.minimum((v * k).astype(np.int64), BINS - 1)          # float32 * float32 -> float32, then truncation
    np.add.at(h, b, 1)
    return h


def kl_divergences(hist):
    """KL_i for i = 128 .. 2048 (index i - 128), +inf where the contract says so"""
    h = np.asarray(hist, np.float64).reshape(BINS)
    out = np.full(BINS - GROUPS + 1, np.inf)
    for i in range(GROUPS, BINS + 1):
        P = h[:i].copy()
        P[i - 1] += h[i:].sum()
        starts = np.arange(GROUPS) * i // GROUPS                     # group g = [g i // 128, (g + 1) i // 128), never empty for i >= 128
        lengths = np.diff(np.append(starts, i))
        S = np.add.reduceat(h[:i], starts)
        n = np.add.reduceat((h[:i] != 0).astype(np.float64), starts)
        mean = np.divide(S, n, out=np.zeros(GROUPS), where=n > 0)
        Q = np.where(h[:i] != 0, np.repeat(mean, lengths), 0.0)
        sq = Q.sum()
        if sq == 0:
            continue
        p, q = P / P.sum(), Q / sq
        m = p > 0
        if (q[m] == 0).any():
            continue
        out[i - GROUPS] = float(np.sum(p[m] * np.log(p[m] / q[m])))
    return out


def kl_search(hist, amax):
    """-> (i*, A): the smallest i of least KL_i and A = i* amax / 2048 (double, rounded once to float); (0, 0) for no counts"""
    h = np.asarray(hist, np.float64).reshape(BINS)
    if h.sum() == 0:
        return 0, np.float32(0.0)
    kl = kl_divergences(h)
    i = int(np.argmin(kl)) + GROUPS                                 # argmin returns the first of equal minima
    return i, np.float32(i * float(np.float32(amax)) / BINS)
