"""The geometries and recordings of tests/test_vad_geometry_gpu.py, and of the CPU proof of their properties in
tests/test_vad_geometry_host.py.  Host only, numpy only.

A geometry is a set of kws_amd.vad.Vad keyword arguments.  Each has ONE packed (R, stride) int16 buffer (`packed`) whose rows hold,
past their length, a loud in-band tone, so that a read past lengths[r] shows in the results.  The rows are built in the style of
tests/vad_cases.py: in-band two-tone bursts over an out-of-band hum and Gaussian noise, an out-of-band burst, an exactly zero
stretch, one row with a +1000 DC offset.  Frequencies are given in bins of the geometry's own window, so every geometry gets the
same picture.  (At N = 32 and N = 64 white noise alone has a band ratio above 0.6 - the band is most of the spectrum - so the
background everywhere is the hum, 1500, with noise of sigma 150 under it.)

A length is L = N + (n_win - 1) H + q with q in 1..H, which has n_win windows; q = H, 1, H - 1 gives the boundary remainders
(L - N) % H = 0, 1, H - 1, and `_Q` spreads them over the rows.

Seeds and amplitudes were chosen on tests/vad_ref.py alone: no float64 ratio of any row lies within 1e-4 of the threshold
(test_vad_geometry_host.py asserts it), and no seed was chosen by looking at device output.
"""
import functools

import numpy as np

import vad_ref

# id -> (Vad keyword arguments, expected (N, H, bin_lo, bin_hi, median))
GEOMETRIES = {
    "tiny": (dict(sample_rate=1600), (32, 16, 7, 16, 25)),
    "tiny_low": (dict(sample_rate=1600, band=(90, 310)), (32, 16, 2, 6, 25)),
    "r3200": (dict(sample_rate=3200), (64, 32, 7, 32, 25)),
    "r8000": (dict(sample_rate=8000), (160, 80, 7, 59, 25)),
    "r11025": (dict(sample_rate=11025), (220, 110, 6, 59, 25)),
    "r44100": (dict(sample_rate=44100), (882, 441, 7, 59, 25)),
    "r48000": (dict(sample_rate=48000), (960, 480, 7, 59, 25)),
    "even_lo": (dict(sample_rate=16000, band=(360, 3000)), (320, 160, 8, 59, 25)),
    "one_bin": (dict(sample_rate=16000, band=(975, 1025)), (320, 160, 20, 20, 25)),
    "full_band": (dict(sample_rate=16000, band=(300, 3150)), (320, 160, 7, 62, 25)),
    "n1024": (dict(sample_rate=16000, window_t=0.064, hop_t=0.032, band=(300, 1000)), (1024, 512, 20, 63, 7)),
    "median1": (dict(sample_rate=16000, smooth_t=0.02), (320, 160, 7, 59, 1)),
    "median255": (dict(sample_rate=16000, smooth_t=5.12), (320, 160, 7, 59, 255)),
    "thr0": (dict(sample_rate=16000, energy_threshold=0.0), (320, 160, 7, 59, 25)),
    # the two `tiny` variants of the chunk cases: event numbering across chunks, and the widest halo over the chunk edge
    "tiny_m1": (dict(sample_rate=1600, smooth_t=0.02), (32, 16, 7, 16, 1)),
    "tiny_m255": (dict(sample_rate=1600, smooth_t=5.12), (32, 16, 7, 16, 255)),
}
TABLE = ("tiny", "tiny_low", "r3200", "r8000", "r11025", "r44100", "r48000", "even_lo", "one_bin", "full_band", "n1024", "median1",
         "median255", "thr0")                                         # the issue's table; each gets the base rows
CHUNKED = ("tiny", "r3200")                                           # ... and these the chunk rows as well
ALL = TABLE + ("tiny_m1", "tiny_m255")

# (Vad keyword arguments, error code, a word of the message): kws_vad_create must refuse these
REFUSALS = [
    (dict(sample_rate=16000, band=(300, 3200)), -2, "57 bins"),
    (dict(sample_rate=16000, smooth_t=5.16), -2, "median of 257"),
    (dict(sample_rate=16000, window_t=0.02, hop_t=0.005), -2, "window == 2 * hop"),
    (dict(sample_rate=16000, band=(10, 20)), -2, "no frequency bin"),
    (dict(sample_rate=16000, energy_threshold=1.0), -1, "energy_threshold"),
]

# Largest |ratio - float64 ratio| measured on an MI355X on the geometry's rows, int16 and float32 input together
# (tests/test_vad_geometry_gpu.py prints it); the bound is 4x that, the margin tests/test_vad_gpu.py gives.  CEILING: no bound may
# pass the width at which the host test proves the rows clear of the threshold.
MEASURED_RATIO_ERR = {
    "tiny":       3.601e-07,        # bound 1.440e-06; float32 restatement on the CPU 4.5e-07
    "tiny_low":   3.063e-07,        # bound 1.225e-06; float32 restatement on the CPU 2.5e-07
    "r3200":      4.017e-07,        # bound 1.607e-06; float32 restatement on the CPU 3.8e-07
    "r8000":      3.224e-07,        # bound 1.290e-06; float32 restatement on the CPU 7.0e-07
    "r11025":     3.620e-07,        # bound 1.448e-06; float32 restatement on the CPU 8.7e-07
    "r44100":     7.936e-07,        # bound 3.174e-06; float32 restatement on the CPU 8.3e-07
    "r48000":     7.502e-07,        # bound 3.001e-06; float32 restatement on the CPU 6.4e-07
    "even_lo":    5.099e-07,        # bound 2.040e-06; float32 restatement on the CPU 9.7e-07
    "one_bin":    5.453e-07,        # bound 2.181e-06; float32 restatement on the CPU 3.0e-07
    "full_band":  5.054e-07,        # bound 2.022e-06; float32 restatement on the CPU 8.5e-07
    "n1024":      1.044e-06,        # bound 4.176e-06; float32 restatement on the CPU 8.4e-07
    "median1":    4.534e-07,        # bound 1.814e-06; float32 restatement on the CPU 9.0e-07
    "median255":  4.277e-07,        # bound 1.711e-06; float32 restatement on the CPU 1.0e-06
    "thr0":       4.261e-07,        # bound 1.704e-06; float32 restatement on the CPU 7.9e-07
    "tiny_m1":    3.822e-07,        # bound 1.529e-06; float32 restatement on the CPU 3.8e-07
    "tiny_m255":  3.458e-07,        # bound 1.383e-06; float32 restatement on the CPU 4.1e-07
}
CEILING = 1e-4
NEAR_WIDTH = 1e-4
RATIO_BOUND = {g: 4 * e for g, e in MEASURED_RATIO_ERR.items()}

HUM, SIGMA, LOUD = 1500.0, 150.0, 4500.0
END = 10 ** 6                                                         # "to the last sample" as a burst's end window
_Q = ("H", 1, "H-1")
_SEED = {}                                                            # geometry -> seed where 1000 + its index leaves a near-tie: none does


def vad_kwargs(gid):
    return dict(GEOMETRIES[gid][0])


def ref_kwargs(gid):
    """-> (rate, threshold, keyword arguments of vad_ref.geometry / ratios / detect)"""
    kw = vad_kwargs(gid)
    rate, thr = kw.pop("sample_rate"), kw.pop("energy_threshold", 0.6)
    return rate, thr, kw


def length(n_win, N, H, q):
    """a length with n_win windows; n_win == 0: N itself (q is not used)"""
    q = H if q == "H" else H - 1 if q == "H-1" else q
    assert 1 <= q <= H
    return N if n_win == 0 else N + (n_win - 1) * H + q


def _i16(x):
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


class _Maker(object):
    """rows of one geometry; positions are in windows (a burst over windows [a, b) covers samples [a H, b H))"""

    def __init__(self, gid):
        rate, _, kw = ref_kwargs(gid)
        self.N, self.H, self.lo, self.hi, self.m = vad_ref.geometry(rate, **kw)
        nb = self.hi - self.lo
        # in-band tones between the bins; a band of one bin has room for one tone only (two would beat with a period of windows)
        self.tones = (self.lo + 0.07,) if nb == 0 else (self.lo + 0.25 * nb + 0.13, self.lo + 0.7 * nb - 0.17)
        self.out = 2.2 if self.lo >= 5 else self.hi + 4.3              # the hum and the out-of-band burst: bins outside the band
        self.out2 = self.hi + 6.4 if self.hi + 8 < self.N // 2 else 3.6
        self.rng = np.random.default_rng(_SEED.get(gid, 1000 + ALL.index(gid)))
        self.rows, self.i = [], 0

    def sines(self, n0, n, bins, amp):
        t = np.arange(n0, n0 + n) * (2.0 * np.pi / self.N)
        return amp * sum(np.sin(b * t + i) for i, b in enumerate(bins))

    def row(self, n_win, bursts=(), oob=(), zero=(), dc=0.0, L=None, hum=HUM):
        """bursts: (a, b[, amplitude per tone]); oob: out-of-band bursts (a, b); zero: stretches set to exactly 0"""
        H = self.H
        if L is None:
            L = length(n_win, self.N, H, _Q[self.i % 3])
        self.i += 1
        x = self.rng.normal(0.0, SIGMA, L) + self.sines(0, L, (self.out,), hum) + dc
        for bu in bursts:
            a, b = bu[0] * H, min(bu[1] * H, L)
            x[a:b] += self.sines(a, b - a, self.tones, bu[2] if len(bu) > 2 else LOUD)
        for a, b in oob:
            x[a * H:b * H] += self.sines(a * H, (b - a) * H, (self.out2,), 8000.0)
        for a, b in zero:
            x[a * H:b * H] = 0.0
        self.rows.append(_i16(x))

    def base(self):
        self.row(0, L=0)
        self.row(0)                                                    # L == N: no window
        self.row(1, bursts=[(0, END, 9000.0)])
        self.row(2, zero=[(0, END)])                                   # all zero: ratio 0, no interval
        self.row(5, bursts=[(0, END, 12000.0)])                        # shorter than any median but 1
        self.row(62, bursts=[(10, 40)])
        self.row(63, bursts=[(20, 62)])
        self.row(64, bursts=[(30, 63)])                                # ends where the second job begins
        self.row(126, bursts=[(10, 50), (100, END)])                   # open at the last window
        self.row(127, bursts=[(30, 70), (100, 126)], dc=1000.0)        # +1000 DC offset
        # three bursts at different levels, an out-of-band burst, an exactly zero stretch
        self.row(300, bursts=[(25, 66), (100, 140, 2500.0), (188, 232, 12000.0)], oob=[(250, 281)], zero=[(150, 169)])

    def chunks(self):
        self.row(1023, bursts=[(100, 200), (1000, END)])               # open at the last window of chunk 0
        self.row(1024, bursts=[(50, 300), (900, 1010)])
        self.row(1025, bursts=[(200, 400), (1000, END)])               # open; begins in chunk 0, last window in chunk 1
        self.row(2048, bursts=[(100, 300), (1025, 1500), (1900, 2040)])           # a begin at window 1024
        self.row(2049, bursts=[(1024, 1400), (1990, 2048)])            # a begin at 1023; an end at 2048, the first window of chunk 2
        self.row(2100, bursts=[(700, 1024), (1500, 2060), (2081, END)])            # an end at 1024; open across 2048; open at the end
        self.row(2101, bursts=[(100, 400), (1000, 1025), (1100, 2065), (2085, END)])   # an end at 1025; all of chunk 1 inside one
        self.row(2102, bursts=[(100, 400), (1000, 1060), (1500, 2060), (2081, END)])   # intervals in all three chunks
        # bursts shorter than the median whose raw flags start ON windows 1024 and 2048: voted out only by the flags before the edge
        self.row(2103, bursts=[(300, 500), (1025, 1031), (2049, 2055)])


@functools.lru_cache(maxsize=None)
def recordings(gid):
    """-> tuple of int16 arrays"""
    m = _Maker(gid)
    if gid == "tiny_m1":
        # alternating 4-window bursts over three chunks: every one is an interval of its own under a median of 1
        m.row(2400, bursts=[(a, a + 4) for a in range(3, 2390, 8)])
    elif gid == "tiny_m255":
        # the end of the long burst sits just past window 1024: its median reads raw flags from both sides of the chunk edge, and
        # the short burst after it is voted out
        m.row(1100, bursts=[(300, 1030), (1060, 1080)])
        m.row(1101, bursts=[(100, 500), (880, END)])
        m.row(1102, bursts=[(200, 600), (1025, 1060)])                 # 36 raw flags from window 1024 on: voted out by the 127 before it
    else:
        m.base()
        if gid in CHUNKED:
            m.chunks()
    return tuple(m.rows)


@functools.lru_cache(maxsize=None)
def packed(gid):
    """-> ((R, stride) int16 with a loud in-band tone past every length, lengths).  Do not write to the buffer."""
    rows = recordings(gid)
    m = _Maker(gid)
    stride = max(a.size for a in rows)
    buf = np.tile(_i16(m.sines(0, stride, m.tones[:1], 20000.0)), (len(rows), 1))
    for r, a in enumerate(rows):
        buf[r, :a.size] = a
    buf.setflags(write=False)
    return buf, [a.size for a in rows]


@functools.lru_cache(maxsize=None)
def reference(gid):
    """-> (list of vad_ref.detect dicts, list of energy_per_second), computed once per process"""
    rate, thr, kw = ref_kwargs(gid)
    rows = recordings(gid)
    return ([vad_ref.detect(a, rate, threshold=thr, **kw) for a in rows], [vad_ref.energy_per_second(a, rate) for a in rows])


def near(ratio, thr, width):
    """windows that may resolve either way: within `width` of the threshold.  A window of exact zeros has ratio exactly 0 in the
    reference and on the device (integer / double sums), so it is no near-tie at threshold 0."""
    return (np.abs(ratio - thr) <= width) & (ratio != 0.0)


@functools.lru_cache(maxsize=None)
def f32_error(gid):
    """largest |vad_ref.ratios_f32 - float64 ratio| over the geometry's rows: what float32 products cost on the CPU"""
    rate, _, kw = ref_kwargs(gid)
    ref, _ = reference(gid)
    return max([float(np.abs(vad_ref.ratios_f32(a, rate, **kw).astype(np.float64) - d["ratio"]).max())
                for a, d in zip(recordings(gid), ref) if d["ratio"].size] + [0.0])
