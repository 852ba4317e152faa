"""float64 numpy restatement of the speed and loudness perturbation (include/kws.h: kws_resampler_*, kws_speed_apply) for
tests/test_speed_host.py and tests/test_speed_gpu.py: the Kaiser-windowed sinc table, the band-limited interpolation, the level and
the draws.  Next to every output sample it returns A[n] = s sum |w| |v| and the tap count T[n], which the float32 error bound of the
GPU tests is made of."""
import math

import numpy as np

from aug_ref import np_hash, np_unit

MIX = 0xA0761D6478BD642F
EPS32 = float(np.finfo(np.float32).eps)
DEFAULTS = dict(zero_crossings=16, phases=512, beta=8.555504641634386, rolloff=0.85)


def _fmaf(a, b, c):
    """float32 fmaf(a, b, c): the product of two float32 is exact in float64"""
    return (a.astype(np.float64) * np.float64(b) + np.float64(c)).astype(np.float32)


def np_draws(seed, step, pos, speed_rate=0.0, speed=(1.0, 1.0), loud_rate=0.0, loudness=(0.0, 0.0)):
    """-> (resampled bool, r float32, levelled bool, target float32) per clip at the global positions pos, seed = WaveAugment's"""
    seed_s = seed ^ MIX
    pos = np.asarray(pos, np.uint64)
    u = [np_unit(np_hash(seed_s, step, np.uint64(4) * pos + np.uint64(f))) for f in range(4)]
    lo, hi = np.float32(speed[0]), np.float32(speed[1])
    dlo, dhi = np.float32(loudness[0]), np.float32(loudness[1])
    return (u[0] < np.float32(speed_rate), _fmaf(u[1], hi - lo, lo), u[2] < np.float32(loud_rate), _fmaf(u[3], dhi - dlo, dlo))


def table(zero_crossings=16, phases=512, beta=8.555504641634386, rolloff=0.85):
    """h[i] = rolloff sinc(rolloff i / P) kaiser_beta(i / (P Z)), i = 0 .. Z P: float64, rounded to float32 as the device stores it"""
    Z, P = int(zero_crossings), int(phases)
    i = np.arange(Z * P + 1, dtype=np.float64)
    u = i / (P * Z)
    h = rolloff * np.sinc(rolloff * i / P) * np.i0(beta * np.sqrt(np.maximum(1.0 - u * u, 0.0))) / np.i0(beta)
    return h.astype(np.float32)


def out_length(Ls, r, max_samples):
    """L' of a resampled clip (r a float32 ratio)"""
    if Ls == 0:
        return 0
    return min(int(math.ceil(float(Ls) / float(np.float32(r)))), int(max_samples))


def resample(v, r, max_samples, h, zero_crossings, phases):
    """-> (y, A, T) float64 / float64 / int of length L': the clip v (1-D, its whole valid length) played r times faster"""
    v = np.asarray(v, np.float64)
    Ls, Z, P = len(v), int(zero_crossings), int(phases)
    r = float(np.float32(r))
    Lp = out_length(Ls, r, max_samples)
    hd = np.asarray(h, np.float32).astype(np.float64)
    assert hd.shape == (Z * P + 1,)
    s = 1.0 / r if r > 1.0 else 1.0
    lim = float(Z * P)
    n = np.arange(Lp, dtype=np.float64)
    t = n * r
    n0 = np.floor(t)
    phi = t - n0
    n0 = n0.astype(np.int64)
    assert Lp == 0 or n0.max() < Ls
    acc, A, T = np.zeros(Lp), np.zeros(Lp), np.zeros(Lp, np.int64)
    for x0, j0, dj in ((phi, n0, -1), (1.0 - phi, n0 + 1, 1)):                  # left wing, then right wing
        live = np.ones(Lp, bool)
        k = 0
        while True:
            j = j0 + dj * k
            pos = ((x0 + float(k)) * s) * float(P)
            live &= (j >= 0) & (j < Ls) & (pos < lim)
            if not live.any():
                break
            pl = pos[live]
            i = np.floor(pl).astype(np.int64)
            w = hd[i] + (pl - i) * (hd[i + 1] - hd[i])
            x = v[j[live]]
            acc[live] += w * x
            A[live] += np.abs(w) * np.abs(x)
            T[live] += 1
            k += 1
    return s * acc, s * A, T


def gain(y, target_db):
    """float32 g of a levelled clip y (the values the level is taken of), target in dBFS"""
    y = np.asarray(y, np.float64)
    m = float(np.mean(y * y)) if len(y) else 0.0
    return np.sqrt(np.float32(10.0 ** (float(np.float32(target_db)) / 10.0) / (m + EPS32)))


def level_db(y):
    y = np.asarray(y, np.float64)
    return 10.0 * math.log10(float(np.mean(y * y)))


def perturb(v, r, target_db, max_samples, h=None, zero_crossings=16, phases=512):
    """one clip: -> dict(y float64 (L'), A, T, g float32) with r = 0 for "not resampled" and target_db = NaN for "not levelled";
    y is the resampled clip BEFORE the gain (the device's output is float32(g) y)"""
    v = np.asarray(v, np.float64)
    if float(r) == 0.0:
        y = v[:max_samples].copy()
        A, T = np.abs(y), np.ones(len(y), np.int64)
    else:
        y, A, T = resample(v, r, max_samples, h, zero_crossings, phases)
    g = np.float32(1.0) if np.isnan(target_db) else gain(y, target_db)
    return dict(y=y, A=A, T=T, g=g)
