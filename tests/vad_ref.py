"""float64 numpy restatement of the voice-activity arithmetic (include/kws.h, "Voice-activity detection"), written from its
description: the yardstick of tests/test_vad_host.py, tests/test_vad_gpu.py and tests/test_vad_geometry_*.py.  One np.fft.rfft per
window.  (`ratios_f32` is no yardstick: it shows what float32 products cost, beside the device's error.)"""
import numpy as np


def geometry(rate, window_t=0.02, hop_t=0.01, band=(300, 3000), smooth_t=0.5):
    """-> (N, H, first band bin, last band bin, median length)"""
    N, H = int(rate * window_t), int(rate * hop_t)
    f = np.arange(1, N // 2 + 1) * (1.0 / (N * (1.0 / rate)))
    k = np.nonzero((band[0] < f) & (f < band[1]))[0] + 1
    m = int(smooth_t / window_t)
    if m % 2 == 0:
        m -= 1
    return N, H, int(k[0]), int(k[-1]), m


def n_windows(L, N, H):
    """windows w with w H < L - N"""
    return 0 if L <= N else -(-(L - N) // H)


def ratios(x, rate, **kw):
    """band / full per window in float64; 0 where full == 0 (the reference's nan compares False)"""
    N, H, lo, hi, _ = geometry(rate, **kw)
    x = np.asarray(x, dtype=np.float64)
    nw = n_windows(x.size, N, H)
    out = np.zeros(nw)
    for w in range(nw):
        E = np.abs(np.fft.rfft(x[w * H:w * H + N])) ** 2
        full = 2.0 * E[1:N // 2 + 1].sum()
        if full > 0.0:
            out[w] = 2.0 * E[lo:hi + 1].sum() / full
    return out


def ratios_f32(x_int16, rate, **kw):
    """the ratios as a float32 machine can form them, for comparison with the device's error (not a yardstick): a dense float32
    product of the windows (samples x / 32768, exact in float32) with the cos / sin of the band bins, squares summed in float32; the
    total from the Parseval form N sum x^2 - (sum x)^2 + (sum (-1)^n x_n)^2 in float64; the division in float64, rounded once"""
    N, H, lo, hi, _ = geometry(rate, **kw)
    x = np.asarray(x_int16, dtype=np.float64) / 32768.0
    nw = n_windows(x.size, N, H)
    if nw == 0:
        return np.zeros(0, np.float32)
    win = x[np.arange(nw)[:, None] * H + np.arange(N)[None, :]]                            # (nw, N), exact
    ang = 2.0 * np.pi * ((np.arange(N)[:, None] * np.arange(lo, hi + 1)[None, :]) % N) / N
    w32 = win.astype(np.float32)
    re, im = w32 @ np.cos(ang).astype(np.float32), w32 @ np.sin(ang).astype(np.float32)
    band = (re * re + im * im).sum(axis=1, dtype=np.float32).astype(np.float64)
    alt = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
    full = N * (win * win).sum(axis=1) - win.sum(axis=1) ** 2 + (win * alt).sum(axis=1) ** 2
    out = np.zeros(nw)
    ok = full > 0.0
    out[ok] = 2.0 * band[ok] / full[ok]
    return out.astype(np.float32)


def smooth(raw, m=25):
    """median of m 0/1 flags with the first and the last value replicated (m - 1) / 2 times: at least (m + 1) / 2 ones"""
    raw = np.asarray(raw, dtype=np.int64)
    if raw.size == 0:
        return raw.astype(np.uint8)
    h = (m - 1) // 2
    p = np.concatenate([np.full(h, raw[0]), raw, np.full(h, raw[-1])])
    c = np.concatenate([[0], np.cumsum(p)])
    return ((c[m:] - c[:-m]) > h).astype(np.uint8)


def intervals(sm, H):
    """[(begin sample, end sample)]: begin at the first 1-window, end at the next 0-window; an open interval is dropped"""
    out, begin = [], None
    for w, s in enumerate(sm):
        if s and begin is None:
            begin = w * H
        elif not s and begin is not None:
            out.append((begin, w * H))
            begin = None
    return out


def span(iv):
    return (min(b for b, _ in iv), max(e for _, e in iv)) if iv else (0, 0)


def energy_per_second(x_int16, rate):
    x = np.asarray(x_int16, dtype=np.float64) / 32768.0
    return float(np.sum(x * x) / (x.size / rate)) if x.size else 0.0


def detect(x, rate, threshold=0.6, flip=(), **kw):
    """-> dict(ratio, raw, smoothed, intervals, span); `flip`: windows whose raw flag is inverted (near-ties)"""
    N, H, lo, hi, m = geometry(rate, **kw)
    r = ratios(x, rate, **kw)
    raw = (r > threshold).astype(np.uint8)
    for w in flip:
        raw[w] ^= 1
    sm = smooth(raw, m)
    iv = intervals(sm, H)
    return {"ratio": r, "raw": raw, "smoothed": sm, "intervals": iv, "span": span(iv)}


def gather(x, L, begin, end, clip, pad_before=0, pad_after=0, align="left"):
    """clip of float32 samples x / 32768 cut from [max(0, begin - pad_before), min(L, end + pad_after))"""
    lo, hi = max(0, begin - pad_before), min(L, end + pad_after)
    cut = (np.asarray(x[lo:max(lo, hi)], dtype=np.float32) * np.float32(1.0 / 32768.0))[:clip]
    out = np.zeros(clip, np.float32)
    off = clip - cut.size if align == "left" else (clip - cut.size) // 2
    out[off:off + cut.size] = cut
    return out
