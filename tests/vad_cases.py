"""The recordings of tests/test_vad_gpu.py (and of the CPU check of their near-threshold windows in tests/test_vad_host.py):
R = 8 int16 recordings at 16 kHz in one packed buffer whose unused tail is a loud 1 kHz tone, so that a read past a recording's
length shows in its results."""
import numpy as np

RATE, N, H = 16000, 320, 160
STRIDE = 51200                                     # 3.2 s
LENGTHS = [0, N, N + 1, N + H + 1, N + 4 * H + 1, 49733, 36871, 27219]


def _tones(n, freqs, amp, phase=0.0):
    t = np.arange(n) / RATE
    return amp * sum(np.sin(2 * np.pi * f * t + phase + i) for i, f in enumerate(freqs)) / len(freqs)


def _i16(x):
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def recordings():
    """-> list of 8 int16 arrays"""
    rng = np.random.default_rng(77)
    out = [np.zeros(0, np.int16),
           _i16(rng.normal(0, 500, LENGTHS[1])),                                         # no window
           _i16(_tones(LENGTHS[2], (800, 2100), 9000)),                                  # one window
           np.zeros(LENGTHS[3], np.int16),                                               # all zero, two windows
           _i16(_tones(LENGTHS[4], (600, 1500), 12000) + rng.normal(0, 50, LENGTHS[4]))]  # 5 windows < the 12 replicated
    # three in-band two-tone bursts at different levels in Gaussian noise, an out-of-band burst, an exactly zero stretch
    L = LENGTHS[5]
    x = rng.normal(0, 120, L)
    for a, b, amp, fr in ((4000, 10500, 3000, (500, 1700)), (16100, 22333, 900, (950, 2600)), (30007, 37000, 15000, (400, 2900))):
        x[a:b] += _tones(b - a, fr, amp)
    x[40000:45000] += _tones(5000, (5000, 6000), 8000)
    x[24000:27000] = 0.0
    out.append(_i16(x))
    # +1000 DC offset; the last burst runs to the last sample: its interval stays open and is dropped
    L = LENGTHS[6]
    x = rng.normal(0, 200, L) + 1000.0
    x[5000:12000] += _tones(7000, (700, 1300), 5000)
    x[L - 9000:] += _tones(9000, (1000, 2000), 7000)
    out.append(_i16(x))
    # full scale: a clipped in-band two-tone burst and loud noise around it
    L = LENGTHS[7]
    x = rng.normal(0, 9000, L)
    x[6000:16000] += _tones(10000, (640, 1810), 80000)
    out.append(_i16(x))
    assert [a.size for a in out] == LENGTHS
    return out


def packed():
    """-> ((8, STRIDE) int16 with the tone past every length, lengths)"""
    buf = np.tile(_i16(_tones(STRIDE, (1000,), 20000)), (len(LENGTHS), 1))
    for r, a in enumerate(recordings()):
        buf[r, :a.size] = a
    return buf, list(LENGTHS)
