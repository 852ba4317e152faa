"""float64 numpy restatements for the filter augmentation tests (tests/test_filter_host.py, tests/test_filter_gpu.py and the edge suite of
tests/wave_edge_cases.py): the draws of
kws_filter_apply and scipy.signal.filtfilt's defaults on second-order sections, batched over clips."""
import numpy as np

from aug_ref import np_pick

MIX = 0xD1B54A32D192ED03


def np_draws(seed, step, pos, rate, K):
    """filter index per clip, -1 when not drawn (before the Lv <= padlen rule)"""
    return np_pick(seed ^ MIX, step, pos, rate, K)


def _norm(sos):
    sos = np.asarray(sos, np.float64)
    return sos / sos[:, 3:4]


def sosfilt_zi(sos):
    """scipy.signal.sosfilt_zi: per section the steady state under a unit step, scaled by the DC gain of the sections before it"""
    sos = _norm(sos)
    zi = np.zeros((len(sos), 2))
    scale = 1.0
    for s, (b0, b1, b2, _, a1, a2) in enumerate(sos):
        g = (b0 + b1 + b2) / (1.0 + a1 + a2)
        zi[s] = scale * np.array([g - b0, b2 - a2 * g])
        scale *= g
    return zi


def sosfilt_batch(c, x, z):
    """transposed direct form II cascade over the rows of x (B, T); c (B, S, 6) normalised sections; z (B, S, 2) initial states"""
    z = np.array(z, np.float64)
    y = np.empty_like(x)
    b0, b1, b2, a1, a2 = (c[:, :, i] for i in (0, 1, 2, 4, 5))
    S = c.shape[1]
    for t in range(x.shape[1]):
        xt = x[:, t]
        for s in range(S):
            yt = b0[:, s] * xt + z[:, s, 0]
            z[:, s, 0] = b1[:, s] * xt - a1[:, s] * yt + z[:, s, 1]
            z[:, s, 1] = b2[:, s] * xt - a2[:, s] * yt
            xt = yt
        y[:, t] = xt
    return y


def odd_ext(v, padlen):
    v = np.asarray(v, np.float64)
    return np.r_[2 * v[0] - v[padlen:0:-1], v, 2 * v[-1] - v[-2:-(padlen + 2):-1]]


def filtfilt_batch(sos_list, clips, padlens):
    """filtfilt (padtype 'odd', scipy's zi) of every clip with its own sections and padlen, float64: a list of arrays of len(clip)"""
    B = len(clips)
    if B == 0:
        return []
    S = max(len(s) for s in sos_list)
    c = np.tile(np.array([1.0, 0, 0, 1.0, 0, 0]), (B, S, 1))
    zi = np.zeros((B, S, 2))
    for b, s in enumerate(sos_list):
        c[b, :len(s)] = _norm(s)
        zi[b, :len(s)] = sosfilt_zi(s)
    exts = [odd_ext(v, p) for v, p in zip(clips, padlens)]
    T = max(len(e) for e in exts)
    x = np.zeros((B, T))
    for b, e in enumerate(exts):
        x[b, :len(e)] = e
    yf = sosfilt_batch(c, x, zi * x[:, :1, None])
    u = np.zeros((B, T))
    for b, e in enumerate(exts):
        u[b, :len(e)] = yf[b, :len(e)][::-1]
    yb = sosfilt_batch(c, u, zi * u[:, :1, None])
    out = []
    for b, (e, p) in enumerate(zip(exts, padlens)):
        out.append(yb[b, :len(e)][::-1][p:len(e) - p])
    return out


def filtfilt(sos, v, padlen):
    return filtfilt_batch([sos], [v], [padlen])[0]


def keep_energy(v, y):
    """kws_filter_apply's rescale of a filtered clip y to the energy of its input v, float64"""
    v = np.asarray(v, np.float64)
    return y * np.sqrt(np.sum(v * v) / (np.sum(y * y) + len(v) * np.finfo(np.float32).eps))
