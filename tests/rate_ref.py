"""float64 numpy restatement of the sample-rate conversion (include/kws.h: kws_rate_*) for tests/test_rate_host.py,
tests/test_rate_gpu.py and tests/test_stream_rates_gpu.py: the bank, the emission counts M and total, and every output sample.  Next to
every output sample it returns A[n] = sum |w| |v| and the tap count T[n] (the taps that fall inside the stream; the others multiply a
zero and add no error), which the float32 error bound of the GPU tests is made of."""
import math

import numpy as np

KAISER_BEST_BETA = 8.555504641634386
DEFAULTS = dict(zero_crossings=16, beta=KAISER_BEST_BETA, rolloff=0.85)


def _i0(x):
    """I0 by its power series, float64 (every term positive)"""
    x = np.asarray(x, np.float64)
    quarter = 0.25 * x * x
    term, total = np.ones_like(x), np.ones_like(x)
    for k in range(1, 500):
        term = term * quarter / (k * k)
        total = total + term
        if np.all(term < 1e-17 * total):
            break
    return total


def kernel(x, Z, beta, rolloff):
    """h(x) = rolloff sinc(rolloff x) kaiser_beta(x / Z) for 0 <= x < Z, 0 from Z on (float64)"""
    x = np.asarray(x, np.float64)
    u = x / Z
    h = rolloff * np.sinc(rolloff * x) * _i0(beta * np.sqrt(np.maximum(1.0 - u * u, 0.0))) / _i0(beta)
    return np.where(x < Z, h, 0.0)


class Bank(object):
    """p, q, K, s and W64 (q, 2K) float64 from the formula; W32 its float32 rounding"""

    def __init__(self, f_in, f_out, zero_crossings=16, beta=KAISER_BEST_BETA, rolloff=0.85):
        g = math.gcd(int(f_in), int(f_out))
        self.p, self.q, self.Z = int(f_in) // g, int(f_out) // g, int(zero_crossings)
        p, q, Z = self.p, self.q, self.Z
        self.K = 0 if p == q else (Z if p < q else (Z * p + q - 1) // q)
        self.s = min(1.0, q / p)
        K = self.K
        m = np.arange(q, dtype=np.int64)[:, None]
        k = np.arange(K, dtype=np.int64)[None, :]
        den = max(p, q)                                        # s d / q = d / max(p, q) for the integer distance d
        self.dist = np.concatenate([m + k * q, q - m + k * q], axis=1)                      # (q, 2K) integers, in units of 1 / q
        self.W64 = np.where(self.dist >= Z * den, 0.0, self.s * kernel(self.dist / float(den), Z, beta, rolloff))
        self.W32 = self.W64.astype(np.float32)
        self.dead = self.dist >= Z * den                       # s * distance >= Z


def emitted(N, p, q, K):
    """M(N)"""
    N = int(N)
    return 0 if N <= K else -((-(N - K) * q) // p)


def total(N, p, q):
    return -((-int(N) * q) // p)


def emitted_brute(N, p, q, K):
    """outputs n whose rightmost tap n0 + K is among the first N samples, counted one by one (n0 does not decrease with n)"""
    n = 0
    while (n * p) // q + K <= N - 1:
        n += 1
    return n


def max_chunk(chunk_size, p, q):
    return int(chunk_size) * p // q


def convert(x, bank, W=None, n_lo=0, n_hi=None, n_avail=None):
    """Outputs n_lo <= n < n_hi of the stream x (1-D int16) whose first n_avail samples exist (the rest are taken as 0):
    -> (y, A, T), float64 / float64 / int64.  n_hi defaults to total(n_avail); W (q, 2K) float32 defaults to the bank's own rounding."""
    x = np.asarray(x)
    assert x.dtype == np.int16 and x.ndim == 1
    p, q, K = bank.p, bank.q, bank.K
    N = len(x) if n_avail is None else int(n_avail)
    if n_hi is None:
        n_hi = total(N, p, q)
    v = x[:N].astype(np.float64) / 32768.0
    n = np.arange(n_lo, n_hi, dtype=np.int64)
    if K == 0:
        y = np.where(n < N, v[np.minimum(n, max(N - 1, 0))] if N else 0.0, 0.0) if len(n) else np.zeros(0)
        return y, np.abs(y), np.zeros(len(n), np.int64)
    Wd = (bank.W32 if W is None else np.asarray(W, np.float32)).astype(np.float64)
    assert Wd.shape == (q, 2 * K)
    n0, m = (n * p) // q, (n * p) % q
    acc, A, T = np.zeros(len(n)), np.zeros(len(n)), np.zeros(len(n), np.int64)
    for wing in range(2):
        for k in range(K):
            j = n0 - k if wing == 0 else n0 + 1 + k
            live = (j >= 0) & (j < N)
            w = Wd[m, wing * K + k]
            xv = np.where(live, v[np.clip(j, 0, max(N - 1, 0))] if N else 0.0, 0.0)
            acc += w * xv
            A += np.abs(w) * np.abs(xv)
            T += live
    return acc, A, T


def to_int16(y):
    """clamp(rint(y * 32768)), half to even, of float32 samples"""
    y = np.asarray(y, np.float32)
    return np.clip(np.rint(y * np.float32(32768.0)), -32768, 32767).astype(np.int16)


def stream_int16(x, bank, cuts):
    """The reference's own streaming form: the int16 outputs each push emits when the stream x is cut at `cuts` (chunk lengths).  Every
    push sees only the samples delivered so far; its outputs are n in [M(N), M(N + len))."""
    out, N = [], 0
    for c in cuts:
        lo, hi = emitted(N, bank.p, bank.q, bank.K), emitted(N + c, bank.p, bank.q, bank.K)
        y, _, _ = convert(x, bank, n_lo=lo, n_hi=hi, n_avail=N + c)
        out.append(to_int16(y))
        N += c
    return out
