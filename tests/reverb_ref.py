"""float64 numpy restatements for the reverb edge tests (tests/test_wave_edges_host.py, tests/test_wave_edges_gpu.py), around
np_reverb of tests/test_reverb_gpu.py: the bank's own clipping of the taps, and the same convolution by np.fft.rfft for the pairs that
np.convolve's direct sum is too slow for (tests/test_wave_edges_host.py holds it to np.convolve)."""
import numpy as np

from test_reverb_gpu import np_reverb

DIRECT_LIMIT = 4000 * 4000     # Lv * Lh up to which the direct sum is used


def keep_energy_scale(v, y):
    """kws_reverb_apply's rescale factor of a wet clip y of the input v, in float64 throughout (np_reverb's comes out rounded to
    float32: numpy adds its Python float to Lv times a float32 eps in float32)"""
    v = np.asarray(v, np.float64)
    Lv = len(v)
    return float(np.sqrt(np.sum(v ** 2) / (np.sum(y[:Lv] ** 2) + Lv * float(np.finfo(np.float32).eps))))


def np_reverb_fft(v, h, ms, rescale):
    """np_reverb with the convolution done by a float64 real FFT: (y[:L'], scale)"""
    Lv = len(v)
    if Lv == 0:
        return np.zeros(0), 1.0
    v = np.asarray(v, np.float64)
    h = np.asarray(h, np.float64)[:ms]
    L = min(Lv + len(h) - 1, ms)
    n = 1
    while n < Lv + len(h) - 1:
        n *= 2
    y = np.fft.irfft(np.fft.rfft(v, n) * np.fft.rfft(h, n), n)[:L]
    s = keep_energy_scale(v, y) if rescale else 1.0
    return y * s, s


def bank_taps(h, bank_ms):
    """what a RirBank of max_samples = bank_ms keeps of a peak-first RIR"""
    return np.asarray(h)[:bank_ms]


def reverb_pair(v, h, bank_ms, ms):
    """one wet clip through a bank of max_samples = bank_ms in a call of max_samples = ms: (y[:L'] without the rescale, the scale
    that the rescale would apply)"""
    h = bank_taps(h, bank_ms)
    f = np_reverb if len(v) * min(len(h), ms) <= DIRECT_LIMIT else np_reverb_fft
    y = f(v, h, ms, False)[0]
    return y, keep_energy_scale(v, y) if len(v) else 1.0
