"""Background-noise, room-reverberation, filter, speed, loudness, tempo and pitch augmentation of raw audio on the GPU (include/kws.h:
kws_noise_bank_*, kws_augment_*, kws_rir_bank_*, kws_reverb_apply, kws_filter_bank_*, kws_filter_apply, kws_resampler_*, kws_speed_apply,
kws_pitch_*), and SpecAugment of the features behind them (kws_feature_mask: FeatureMask, at the end of this file).

The reference makes training data robust offline: tools/audio_process/add_noise.py mixes a randomly chosen background recording into a
`noised_rate` fraction of the clips at an SNR drawn from a list and writes one fixed *_noised.wav copy per clip.  Here the same mix is
drawn afresh for every clip of every train step, inside the featurizer's sample loads:

    noise = NoiseBank("dataset/_background_noise_")          # or a list of 1-D float32 / int16 arrays
    aug = WaveAugment(noise, snr=(5, 10, 20), noised_rate=0.8, time_shift_ms=100, seed=1)
    model.fit(x_audio, y, augment=aug, sample_lengths=lengths)

The reference's other augmentation tool, tools/audio_process/audio_reverberation.py (or gpuRIR_reverberation.py), convolves every clip
with the impulse response of a random room and writes one *_reverb.wav copy.  Here a bank of room impulse responses (RIRs) is built once
-- from wav files, or simulated by simulate_rirs() with the reference's room draws -- and every clip of every step is convolved with a
RIR drawn afresh, before the noise is mixed in:

    aug = WaveAugment(noise, rirs=simulate_rirs(64, seed=0), reverb_rate=1.0, seed=1)     # noise may be None

The third tool, tools/audio_process/wav_filter.py, filters a clip with a Butterworth design (scipy.signal.butter) at zero phase
(scipy.signal.filtfilt).  Here a bank of designs (butter_sos, in float64 numpy) is built once, and a `filter_rate` share of the clips of
every step is filtered with one drawn afresh, after the reverberation and before the noise:

    aug = WaveAugment(noise, filters=random_filters(64, seed=0), filter_rate=0.5, seed=1)   # noise may be None

The fourth tool, tools/audio_process/audio_convert.py, resamples a file and sets it to a target loudness (pydub's apply_gain(target -
dBFS)).  Here a `speed_rate` share of the clips of every step is played at a ratio drawn from `speed` (tempo and pitch move together,
band-limited interpolation with the Kaiser-windowed sinc table of a Resampler), and a `loudness_rate` share is set to a level drawn from
`loudness` (dBFS), before every other stage:

    aug = WaveAugment(noise, speed=(0.9, 1.1), loudness=(-30, -15), seed=1)                 # noise may be None

resample(wav, orig_sr, target_sr) is the tool's file-conversion use of the same kernel at one fixed ratio.

The reference has no tool that changes a clip's tempo without its pitch or its pitch without its tempo.  Here a `tempo_rate` share of
the clips of every step is stretched in time at a tempo drawn from `tempo` and a `pitch_rate` share is shifted by a number of semitones
drawn from `pitch`, by a phase vocoder (and, for the pitch, the Resampler's interpolation behind it), before every other stage:

    aug = WaveAugment(noise, tempo=(0.85, 1.2), pitch=(-2, 2), seed=1)                      # noise may be None

time_stretch(wav, rate), pitch_shift(wav, n_steps) and stft(wav, n_fft) are the one-shot uses of the same kernels.

Argument checks run on the host; the device copy of a bank is made on first use."""
import ctypes
import math
import os

import numpy as np

from . import lib as _l

# one kws_aug_clip record
CLIP_DTYPE = np.dtype([("apply", "<i4"), ("segment", "<i4"), ("offset", "<i4"), ("shift", "<i4"), ("length", "<i4"),
                       ("snr_db", "<f4"), ("gain", "<f4"), ("voice_length", "<i4")])


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise _l.KwsError(-3, "no HIP device visible to torch: the augmentation has no CPU fallback")
    return torch


def _wav_code(t):
    import torch
    if t.dtype == torch.float32:
        return _l.WAV_F32
    if t.dtype == torch.int16:
        return _l.WAV_I16
    raise TypeError("waveforms must be float32 or int16, got %s" % t.dtype)


def _clip_batch(wav, valid_len, index, shape="(rows, stride)"):
    """-> (rows, stride, B, index pointer, valid_len pointer; 0 for None) of the B clips wav[index] (default: every row): the tensor
    checks of every stage and of the featurizer"""
    import torch
    if not wav.is_cuda or wav.dim() != 2 or not wav.is_contiguous():
        raise ValueError("wav must be a contiguous CUDA tensor of shape %s" % shape)
    rows, stride = wav.shape
    B, ix, vl = rows, 0, 0
    if index is not None:
        if index.dtype != torch.int32 or not index.is_cuda or index.dim() != 1 or not index.is_contiguous():
            raise ValueError("index must be a contiguous CUDA int32 vector")
        B, ix = index.numel(), index.data_ptr()
    if valid_len is not None:
        if valid_len.dtype != torch.int32 or not valid_len.is_cuda or valid_len.numel() != rows:
            raise ValueError("valid_len must be a CUDA int32 tensor with one element per row of wav")
        vl = valid_len.data_ptr()
    return rows, stride, B, ix, vl


def _explicit(values, dtype, B, what, noun="entries", flat=True):
    """the host's per-clip values of a stage (instead of its draws) as a contiguous (B,) array; None stays None"""
    if values is None:
        return None
    ex = np.asarray(values)
    ex = np.ascontiguousarray(ex.reshape(-1) if flat else ex, dtype)
    if ex.shape != (B,):
        raise ValueError("explicit %s has %s %s for %d clips" % (what, ex.shape, noun, B))
    return ex


def _outputs(wav, B, ms, out, lengths, *used):
    """-> [out, lengths, *used]: the caller's buffers, or fresh ones for None: out (B, ms) float32, lengths (B,) int32 and per
    (tensor, dtype) of `used` a (B,) vector, where False means "skip it" and comes back as None"""
    import torch
    if out is None:
        out = torch.empty((B, ms), dtype=torch.float32, device=wav.device)
    elif out.dim() != 2 or out.shape[0] < B or out.shape[1] < ms or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError("out must be a contiguous float32 CUDA tensor of at least (%d, %d)" % (B, ms))
    if lengths is None:
        lengths = torch.empty((B,), dtype=torch.int32, device=wav.device)
    return [out, lengths] + [torch.empty((B,), dtype=dt, device=wav.device) if u is None else None if u is False else u for u, dt in used]


def _ptr(t):
    return None if t is None else t.data_ptr()


def _host_ptr(a):
    return None if a is None else a.ctypes.data


def _rate(name, value):
    r = float(value)
    if not 0.0 <= r <= 1.0:
        raise ValueError("%s must be in [0, 1], got %r" % (name, value))
    return r


class _Handle(object):
    """Owner of one native handle: made on first use by _create(L, pointer to the handle) -> status, destroyed by the library
    function named _destroy."""
    _h = None
    _destroy = None

    def handle(self):
        if self._h is None:
            _torch()
            L = _l.get_lib()
            h = ctypes.c_void_p()
            _l.check(self._create(L, ctypes.byref(h)))
            self._h, self._L = h, L
        return self._h

    def close(self):
        if self._h is not None and self._h.value:
            getattr(self._L, self._destroy)(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NoiseBank(_Handle):
    """Background recordings (add_noise.py's noise_files): a folder of *.wav (read with common.data_utils.load_wav) or a list of 1-D
    float32 / int16 arrays (int16 is scaled by 1/32768, as the featurizer does)."""

    def __init__(self, noise):
        if isinstance(noise, (str, os.PathLike)):
            from classifier.data import load_noise_bank
            noise = load_noise_bank(noise)
        if isinstance(noise, np.ndarray) and noise.ndim == 1:
            noise = [noise]
        segs = [np.asarray(a) for a in noise]
        if not segs:
            raise ValueError("a noise bank needs at least one recording")
        for i, a in enumerate(segs):
            if a.ndim != 1 or a.size == 0:
                raise ValueError("noise recording %d must be a non-empty 1-D array, got shape %s" % (i, a.shape))
            if a.dtype not in (np.float32, np.float64, np.int16):
                raise TypeError("noise recording %d: float32 or int16 samples expected, got %s" % (i, a.dtype))
            if a.size >= 2 ** 31:
                raise ValueError("noise recording %d is too long" % i)
        if all(a.dtype == np.int16 for a in segs):
            self.samples, self.dtype = np.ascontiguousarray(np.concatenate(segs)), _l.WAV_I16
        else:
            f = [a.astype(np.float32) / 32768.0 if a.dtype == np.int16 else a.astype(np.float32) for a in segs]
            self.samples, self.dtype = np.ascontiguousarray(np.concatenate(f).astype(np.float32)), _l.WAV_F32
        self.seg_len = np.array([a.size for a in segs], np.int32)

    def __len__(self):
        return len(self.seg_len)

    def as_float32(self):
        """the bank as the device holds it (float32)"""
        return self.samples.astype(np.float32) / 32768.0 if self.dtype == _l.WAV_I16 else self.samples

    _destroy = "kws_noise_bank_destroy"

    def _create(self, L, out):
        return L.kws_noise_bank_create(self.samples.ctypes.data, self.dtype, self.seg_len.ctypes.data, len(self.seg_len), out)


def parse_snr(snr):
    """add_noise.py --snr: a comma list ('5,10,20') or numbers"""
    if isinstance(snr, str):
        snr = [s for s in snr.split(",") if s.strip()]
    if isinstance(snr, (int, float)):
        snr = [snr]
    return [float(s) for s in snr]


# the reverb draws use seed ^ REVERB_SEED_MIX, so that they are independent of the noise draws of the same seed (include/kws.h)
REVERB_SEED_MIX = 0x9E3779B97F4A7C15
SPEED_OF_SOUND = 343.0            # m/s
SINC_HALF_WIDTH = 16              # samples: the Hann-windowed sinc of a fractional delay spans [-16, 16] around it, shifted to be causal


class RirBank(_Handle):
    """Room impulse responses: a folder (searched recursively) or file of *.wav read with common.data_utils.load_wav (resampled to
    pr.sample_rate), or a list of 1-D float arrays.  Every RIR is trimmed to start at its peak argmax|h| (the propagation and
    fractional-delay lead-in goes, so labels keep their timing) and divided by it (the direct path is +1); taps at index >= max_samples
    (default pr.max_samples) can never reach an output sample and are clipped away."""

    def __init__(self, rirs, max_samples=None):
        from classifier.params import pr
        if isinstance(rirs, (str, os.PathLike)):
            from classifier.data import load_noise_bank
            rirs = load_noise_bank(rirs, what='RIR')
        if isinstance(rirs, np.ndarray) and rirs.ndim == 1:
            rirs = [rirs]
        ms = int(pr.max_samples if max_samples is None else max_samples)
        if not 1 <= ms <= _l.REVERB_MAX_SAMPLES:
            raise ValueError("max_samples must be in [1, %d], got %d" % (_l.REVERB_MAX_SAMPLES, ms))
        taps = []
        for i, h in enumerate(list(rirs)):
            h = np.asarray(h)
            if h.ndim != 1 or h.size == 0:
                raise ValueError("RIR %d must be a non-empty 1-D array, got shape %s" % (i, h.shape))
            if h.dtype not in (np.float32, np.float64):
                raise TypeError("RIR %d: float32 or float64 taps expected, got %s" % (i, h.dtype))
            if not np.all(np.isfinite(h)):
                raise ValueError("RIR %d has non-finite taps" % i)
            h = h.astype(np.float64)
            peak = int(np.argmax(np.abs(h)))
            if h[peak] == 0:
                raise ValueError("RIR %d is all zeros" % i)
            taps.append((h[peak:peak + ms] / h[peak]).astype(np.float32))
        if not taps:
            raise ValueError("a RIR bank needs at least one RIR")
        self.taps, self.max_samples = taps, ms
        self.rir_len = np.array([t.size for t in taps], np.int32)

    def __len__(self):
        return len(self.taps)

    _destroy = "kws_rir_bank_destroy"

    def _create(self, L, out):
        flat = np.ascontiguousarray(np.concatenate(self.taps), np.float32)
        return L.kws_rir_bank_create(flat.ctypes.data, self.rir_len.ctypes.data, len(self.taps), self.max_samples, out)


def _windowed_sinc_add(h, delay, amp):
    """h[n] += amp * sinc(n - c) * hann(n - c) for |n - c| < SINC_HALF_WIDTH, c = delay + SINC_HALF_WIDTH (vectorised over images)"""
    c = np.asarray(delay, np.float64) + SINC_HALF_WIDTH
    base = np.floor(c).astype(np.int64)
    offs = np.arange(-SINC_HALF_WIDTH + 1, SINC_HALF_WIDTH + 1)
    n = base[:, None] + offs[None, :]
    x = n - c[:, None]
    w = np.where(np.abs(x) < SINC_HALF_WIDTH, 0.5 * (1.0 + np.cos(np.pi * x / SINC_HALF_WIDTH)), 0.0)
    np.add.at(h, n.ravel(), (np.asarray(amp, np.float64)[:, None] * np.sinc(x) * w).ravel())


def shoebox_rir(room, source, mic, rt60, sample_rate=None, rng=None):
    """The impulse response (float64, not aligned) from `source` to one omni microphone `mic` in a shoebox `room` (metres) with
    reverberation time rt60 (s), from the textbook models:
      - Sabine: every wall reflects with beta = sqrt(1 - alpha), alpha = min(0.161 V / (S rt60), 1 - 1e-6);
      - image sources (Allen & Berkley) up to the time the Sabine decay reaches 15 dB: beta^reflections / (4 pi d) at delay
        d / c * fs (c = 343 m/s), through a Hann-windowed sinc fractional delay of half-width SINC_HALF_WIDTH (shifted to be causal);
      - from there to the 60 dB point a Gaussian tail with amplitude envelope exp(-6.9078 t / rt60), its level matched to the image
        sources' energy over the 5 ms before the hand-over."""
    from classifier.params import pr
    fs = float(sample_rate or pr.sample_rate)
    rng = np.random.default_rng() if rng is None else rng
    room, src, mic = (np.asarray(a, np.float64) for a in (room, source, mic))
    rt60 = float(rt60)
    V = float(np.prod(room))
    S = 2.0 * (room[0] * room[1] + room[0] * room[2] + room[1] * room[2])
    alpha = min(0.161 * V / (S * rt60), 1.0 - 1e-6)
    beta = math.sqrt(1.0 - alpha)
    t_diff, t_max = rt60 * 15.0 / 60.0, rt60            # Sabine decay: 15 dB and 60 dB
    n_diff = int(round(t_diff * fs)) + SINC_HALF_WIDTH
    n_len = int(round(t_max * fs)) + 2 * SINC_HALF_WIDTH + 1
    h = np.zeros(n_len + SINC_HALF_WIDTH + 1)
    d_max = t_diff * SPEED_OF_SOUND
    nmax = np.ceil(d_max / (2.0 * room)).astype(int) + 1
    grids = np.meshgrid(*[np.arange(-m, m + 1) for m in nmax], indexing="ij")
    cells = np.stack([g.ravel() for g in grids], 1)               # (n_cells, 3) image cell indices
    for parity in np.ndindex(2, 2, 2):
        u = np.array(parity)
        pos = (1 - 2 * u)[None, :] * src[None, :] + 2.0 * cells * room[None, :]
        refl = np.abs(2 * cells - u[None, :]).sum(1)
        d = np.sqrt(((pos - mic[None, :]) ** 2).sum(1))
        keep = d <= d_max
        d, refl = np.maximum(d[keep], 1e-3), refl[keep]
        _windowed_sinc_add(h, d / SPEED_OF_SOUND * fs, beta ** refl / (4.0 * np.pi * d))
    h = h[:n_len]
    if n_len > n_diff:
        w = max(int(0.005 * fs), 1)
        e_ism = float(np.mean(h[max(n_diff - w, 0):n_diff] ** 2))
        t = (np.arange(n_diff, n_len) - SINC_HALF_WIDTH) / fs
        env = np.exp(-6.9078 * t / rt60)
        g = math.sqrt(e_ism) / env[0]
        h[n_diff:] = g * env * rng.standard_normal(n_len - n_diff)
    return h


def simulate_rirs(count, seed=None, rt60=(0.3, 0.7), sample_rate=None, with_geometry=False):
    """`count` RIRs (float32, not aligned: RirBank aligns them) of random shoebox rooms, drawn as tools/audio_process/gpuRIR_reverberation.py
    of the reference draws them: rt60 uniform in the range, room uniform in [4, 3, 2.6]..[6, 4.8, 2.8] m, source uniform in
    [0.5, 0.5, 1.6]..[Lx - 0.5, Ly - 0.5, 1.9], one omni microphone (the centre of the reference's array) uniform in
    [0.5, 0.5]..[Lx - 0.5, Ly - 0.5] at 0.1 m.  Deterministic for a given seed.  with_geometry: also return a list of dicts
    (room, source, mic, rt60)."""
    count = int(count)
    if count < 1:
        raise ValueError("count must be >= 1, got %d" % count)
    lo, hi = (float(r) for r in rt60)
    if not 0.0 < lo <= hi:
        raise ValueError("rt60 range must satisfy 0 < low <= high, got %r" % (rt60,))
    rng = np.random.default_rng(seed)
    out, geo = [], []
    for _ in range(count):
        t60 = rng.uniform(lo, hi)
        room = rng.uniform([4.0, 3.0, 2.6], [6.0, 4.8, 2.8])
        src = rng.uniform([0.5, 0.5, 1.6], [room[0] - 0.5, room[1] - 0.5, 1.9])
        mic = np.r_[rng.uniform([0.5, 0.5], [room[0] - 0.5, room[1] - 0.5]), 0.1]
        out.append(shoebox_rir(room, src, mic, t60, sample_rate, rng).astype(np.float32))
        geo.append({"room": room, "source": src, "mic": mic, "rt60": t60})
    return (out, geo) if with_geometry else out


# the filter draws use seed ^ FILTER_SEED_MIX, independent of the noise and reverb draws of the same seed (include/kws.h)
FILTER_SEED_MIX = 0xD1B54A32D192ED03
FILTER_TYPES = ("lowpass", "highpass", "bandpass", "bandstop")


def _zpk_poly(r):
    return np.real(np.poly(r)) if len(r) else np.ones(1)


def _zpk2sos(z, p, k):
    """second-order sections (b0, b1, b2, 1, a1, a2) of a real zpk system with as many zeros as poles: conjugate pole pairs (and real
    poles two by two) make the sections, each pole pair takes its nearest zeros, the poles closest to the unit circle come last and the
    gain goes to the first section (the layout of scipy's zpk2sos)"""
    tol = 1e-10

    def split(r):
        r = np.asarray(r, complex)
        return list(r[r.imag > tol]), sorted(np.real(r[np.abs(r.imag) <= tol]))

    pc, preal = split(p)
    zc, zreal = split(z)
    groups = [[q, np.conj(q)] for q in pc]
    preal = sorted(preal, key=abs)
    while len(preal) >= 2:
        groups.append([preal.pop(), preal.pop()])
    if preal:
        groups.append([preal.pop()])
    groups.sort(key=lambda g: max(abs(q) for q in g))             # closest to the unit circle last
    zeros = [None] * len(groups)
    for i in reversed(range(len(groups))):                         # pair the poles nearest the circle first
        g = groups[i]
        ref = g[0]
        if len(g) == 2 and zc:
            j = int(np.argmin([abs(q - ref) for q in zc]))
            q = zc.pop(j)
            zeros[i] = [q, np.conj(q)]
        else:
            want = len(g)
            if len(zreal) < want:
                raise ValueError("zpk system with unpaired complex zeros")
            sel = []
            for _ in range(want):
                j = int(np.argmin([abs(q - ref) for q in zreal]))
                sel.append(zreal.pop(j))
            zeros[i] = sel
    sos = np.zeros((len(groups), 6))
    for i, (g, zz) in enumerate(zip(groups, zeros)):
        b, a = _zpk_poly(zz), _zpk_poly(g)
        sos[i, :3] = np.r_[b, np.zeros(3 - len(b))]
        sos[i, 3:] = np.r_[a, np.zeros(3 - len(a))]
    sos[0, :3] *= k
    return sos


def butter_sos(order, wn, btype="lowpass"):
    """A digital Butterworth filter as second-order sections, float64 (scipy.signal.butter(order, wn, btype, output='sos')): wn in (0, 1)
    as a fraction of the Nyquist frequency, a pair (low, high) for 'bandpass' / 'bandstop'.  The analog prototype's poles, pre-warping,
    the lowpass / highpass / bandpass / bandstop transform and the bilinear transform are the textbook zpk steps."""
    if btype not in FILTER_TYPES:
        raise ValueError("filter type must be one of %s, got %r" % (", ".join(FILTER_TYPES), btype))
    N = int(order)
    if N != order or N < 1:
        raise ValueError("filter order must be a positive integer, got %r" % (order,))
    band = btype in ("bandpass", "bandstop")
    wn = np.atleast_1d(np.asarray(wn, np.float64))
    if wn.shape != ((2,) if band else (1,)):
        raise ValueError("%s needs %s critical frequency, got %r" % (btype, "a (low, high)" if band else "one", wn.tolist()))
    if not np.all((wn > 0) & (wn < 1)):
        raise ValueError("critical frequencies must be in (0, 1) of Nyquist, got %r" % wn.tolist())
    if band and not wn[0] < wn[1]:
        raise ValueError("band edges need low < high, got %r" % wn.tolist())
    p = -np.exp(1j * np.pi * np.arange(-N + 1, N, 2) / (2 * N))     # analog prototype, cutoff 1 rad/s
    z = np.zeros(0, complex)
    k = 1.0
    fs = 2.0
    warped = 2 * fs * np.tan(np.pi * wn / fs)
    deg = len(p) - len(z)
    if btype == "lowpass":
        wo = warped[0]
        z, p, k = z * wo, p * wo, k * wo ** deg
    elif btype == "highpass":
        wo = warped[0]
        k = k * np.real(np.prod(-z) / np.prod(-p))
        z, p = np.r_[wo / z, np.zeros(deg)], wo / p
    else:
        wo, bw = np.sqrt(warped[0] * warped[1]), warped[1] - warped[0]
        if btype == "bandpass":
            zl, pl = z * bw / 2, p * bw / 2
            z = np.r_[zl + np.sqrt(zl ** 2 - wo ** 2), zl - np.sqrt(zl ** 2 - wo ** 2), np.zeros(deg)]
            p = np.r_[pl + np.sqrt(pl ** 2 - wo ** 2), pl - np.sqrt(pl ** 2 - wo ** 2)]
            k = k * bw ** deg
        else:
            k = k * np.real(np.prod(-z) / np.prod(-p))
            zh, ph = (bw / 2) / z, (bw / 2) / p
            z = np.r_[zh + np.sqrt(zh ** 2 - wo ** 2), zh - np.sqrt(zh ** 2 - wo ** 2), np.full(deg, 1j * wo), np.full(deg, -1j * wo)]
            p = np.r_[ph + np.sqrt(ph ** 2 - wo ** 2), ph - np.sqrt(ph ** 2 - wo ** 2)]
    fs2 = 2.0 * fs                                                    # bilinear transform
    deg = len(p) - len(z)
    k = k * np.real(np.prod(fs2 - z) / np.prod(fs2 - p))
    z = np.r_[(fs2 + z) / (fs2 - z), -np.ones(deg)]
    p = (fs2 + p) / (fs2 - p)
    return _zpk2sos(z, p, k)


def filter_padlen(order, btype):
    """filtfilt's default padlen 3 max(len(a), len(b)) = 3 (n + 1), n the transfer function's order (2 order for a band filter)"""
    n = int(order) * (2 if btype in ("bandpass", "bandstop") else 1)
    return 3 * (n + 1)


class FilterBank(_Handle):
    """Butterworth designs (tools/audio_process/wav_filter.py): specs (btype, order, freq) for 'lowpass' / 'highpass' or (btype, order,
    (low, high)) for 'bandpass' / 'bandstop', frequencies in Hz below the Nyquist frequency of sample_rate (default pr.sample_rate).
    Every design is butter_sos(order, 2 f / sample_rate, btype); at most FILTER_MAX_SECTIONS sections (order 8 for lowpass / highpass,
    4 for bandpass / bandstop)."""

    def __init__(self, specs, sample_rate=None):
        from classifier.params import pr
        sr = float(sample_rate or pr.sample_rate)
        if isinstance(specs, tuple) and specs and isinstance(specs[0], str):
            specs = [specs]
        specs = list(specs)
        if not specs:
            raise ValueError("a filter bank needs at least one filter")
        sos, pad, norm = [], [], []
        for i, spec in enumerate(specs):
            if len(spec) != 3:
                raise ValueError("filter %d: a spec is (btype, order, freq), got %r" % (i, spec))
            btype, order, freq = spec
            if btype not in FILTER_TYPES:
                raise ValueError("filter %d: type must be one of %s, got %r" % (i, ", ".join(FILTER_TYPES), btype))
            if isinstance(order, bool) or int(order) != order or order < 1:
                raise ValueError("filter %d: order must be a positive integer, got %r" % (i, order))
            band = btype in ("bandpass", "bandstop")
            sections = int(order) if band else (int(order) + 1) // 2
            if sections > _l.FILTER_MAX_SECTIONS:
                raise ValueError("filter %d: %s of order %d needs %d sections, more than %d (order <= %d)"
                                 % (i, btype, order, sections, _l.FILTER_MAX_SECTIONS, _l.FILTER_MAX_SECTIONS if band else 2 * _l.FILTER_MAX_SECTIONS))
            f = np.atleast_1d(np.asarray(freq, np.float64))
            if f.shape != ((2,) if band else (1,)):
                raise ValueError("filter %d: %s needs %s, got %r" % (i, btype, "(low, high) in Hz" if band else "one frequency in Hz", freq))
            if not np.all(np.isfinite(f)) or not np.all((f > 0) & (f < sr / 2)):
                raise ValueError("filter %d: frequencies must be in (0, %g) Hz (Nyquist), got %r" % (i, sr / 2, f.tolist()))
            if band and not f[0] < f[1]:
                raise ValueError("filter %d: band edges need low < high, got %r" % (i, f.tolist()))
            sos.append(butter_sos(int(order), 2.0 * f / sr if band else 2.0 * f[0] / sr, btype))
            pad.append(filter_padlen(order, btype))
            norm.append((btype, int(order), tuple(float(x) for x in f) if band else float(f[0])))
        self.specs, self.sos, self.sample_rate = norm, sos, sr
        self.padlen = np.array(pad, np.int32)
        self.n_sections = max(s.shape[0] for s in sos)
        table = np.tile(np.array([1.0, 0, 0, 1.0, 0, 0]), (len(sos), self.n_sections, 1))
        for i, s in enumerate(sos):
            table[i, :s.shape[0]] = s
        self.table = np.ascontiguousarray(table, np.float64)          # (K, n_sections, 6), identity sections pad the lower orders

    def __len__(self):
        return len(self.sos)

    _destroy = "kws_filter_bank_destroy"

    def _create(self, L, out):
        return L.kws_filter_bank_create(self.table.ctypes.data, self.n_sections, self.padlen.ctypes.data, len(self.sos), out)


def _log_uniform(rng, lo, hi):
    return float(np.exp(rng.uniform(np.log(lo), np.log(hi))))


def random_filters(count, types=("lowpass", "highpass", "bandpass"), order=4, seed=None, lowpass=(2000.0, 7000.0), highpass=(50.0, 500.0),
                   notch=(300.0, 4000.0)):
    """`count` random Butterworth specs for FilterBank, deterministic for a given seed: the type uniform over `types`, then
    log-uniform draws: a lowpass cutoff in `lowpass` Hz, a highpass cutoff in `highpass` Hz, a bandpass as one of each (low from
    `highpass`, high from `lowpass`), a bandstop as a third-octave notch [fc 2^(-1/6), fc 2^(1/6)] centred in `notch` Hz."""
    count = int(count)
    if count < 1:
        raise ValueError("count must be >= 1, got %d" % count)
    if isinstance(types, str):
        types = [t for t in types.split(",") if t.strip()]
    types = [t.strip() for t in types]
    if not types or any(t not in FILTER_TYPES for t in types):
        raise ValueError("filter types must be among %s, got %r" % (", ".join(FILTER_TYPES), types))
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        t = types[int(rng.integers(len(types)))]
        if t == "lowpass":
            out.append((t, order, _log_uniform(rng, *lowpass)))
        elif t == "highpass":
            out.append((t, order, _log_uniform(rng, *highpass)))
        elif t == "bandpass":
            lo = _log_uniform(rng, *highpass)
            out.append((t, order, (lo, _log_uniform(rng, *lowpass))))
        else:
            fc = _log_uniform(rng, *notch)
            out.append((t, order, (fc * 2.0 ** (-1.0 / 6.0), fc * 2.0 ** (1.0 / 6.0))))
    return out


# the speed / loudness draws use seed ^ SPEED_SEED_MIX, independent of the noise, reverb and filter draws of the same seed (include/kws.h)
SPEED_SEED_MIX = 0xA0761D6478BD642F
KAISER_BEST_BETA = 8.555504641634386      # the window of the widely used "kaiser_best" resampling table (stop band about -100 dB)


class Resampler(_Handle):
    """The interpolation table of the speed change (kws_resampler): the right half of a Kaiser-windowed sinc with `zero_crossings`
    lobes on each side, `phases` entries per zero crossing, window parameter `beta` and cutoff `rolloff` (a fraction of the lower
    Nyquist frequency).  A host object, made at once: the device copy is made by the first clip resampled with it."""
    _destroy = "kws_resampler_destroy"

    def __init__(self, zero_crossings=16, phases=512, beta=KAISER_BEST_BETA, rolloff=0.85):
        self.zero_crossings, self.phases, self.beta, self.rolloff = int(zero_crossings), int(phases), float(beta), float(rolloff)
        if self.zero_crossings != zero_crossings or self.phases != phases:
            raise ValueError("zero_crossings and phases must be integers, got %r and %r" % (zero_crossings, phases))
        L = _l.get_lib()
        h = ctypes.c_void_p()
        rc = L.kws_resampler_create(self.zero_crossings, self.phases, self.beta, self.rolloff, ctypes.byref(h))
        if rc != 0:
            raise ValueError(L.kws_last_error().decode("utf-8", "replace"))
        self._h, self._L = h, L

    def __len__(self):
        return self.zero_crossings * self.phases + 1

    def table(self):
        """h[0 .. zero_crossings * phases] as the device holds it (float32)"""
        out = np.zeros(len(self), np.float32)
        _l.check(self._L.kws_resampler_table(self.handle(), out.ctypes.data, out.size))
        return out

    def handle(self):
        if self._h is None:
            raise ValueError("this Resampler is closed")
        return self._h


def _range(name, value, lo, hi, unit=""):
    try:
        a, b = (float(x) for x in value)
    except (TypeError, ValueError):
        raise ValueError("%s must be a (low, high) pair, got %r" % (name, value))
    if not lo <= a <= b <= hi:
        raise ValueError("%s range must satisfy %g <= low <= high <= %g%s, got %r" % (name, lo, hi, unit, value))
    return a, b


# the tempo / pitch draws use seed ^ PITCH_SEED_MIX, independent of every other stage's draws of the same seed (include/kws.h)
PITCH_SEED_MIX = 0x8EBC6AF09C88C6E3
PITCH_TILE_CLIPS = 256            # clips the vocoder's workspace holds at a time by default


def pitch_workspace_bytes(n_fft, max_samples, tile_clips):
    """bytes of a vocoder workspace for tile_clips clips at a time (host only, no GPU)"""
    n = ctypes.c_size_t(0)
    _l.check(_l.get_lib().kws_pitch_workspace_bytes(int(n_fft), int(max_samples), int(tile_clips), ctypes.byref(n)))
    return n.value


class WaveAugment(object):
    """Per-clip background noise (add_noise.py:19-35) at an SNR drawn from `snr` for a `noised_rate` fraction of the clips, and an
    optional time shift of up to +-time_shift_ms (off by default; the reference has none).  With `rirs` (a RirBank, or anything RirBank
    accepts) a `reverb_rate` fraction of the clips is first convolved with a RIR drawn from the bank (audio_reverberation.py), with the
    clip's energy kept when `rescale` is on; `noise` may then be None.  With `filters` (a FilterBank, or specs FilterBank accepts) a
    `filter_rate` fraction of the clips is then filtered at zero phase with a design drawn from the bank (wav_filter.py), energy kept
    likewise.  With `speed` = (low, high) a `speed_rate` fraction of the clips is first of all played at a ratio drawn uniformly from
    it (0.5..2; `resampler`: the interpolation table, default Resampler()), and with `loudness` = (low_db, high_db) a `loudness_rate`
    fraction is set to a level drawn uniformly from it (dBFS, -80..0), as audio_convert.py does offline.  With `tempo` = (low, high) a
    `tempo_rate` fraction of the clips is, before all of that, stretched in time at a tempo drawn uniformly from it (0.5..2, pitch
    unchanged), and with `pitch` = (low, high) a `pitch_rate` fraction is shifted by a number of semitones drawn uniformly from it
    (-12..12, duration unchanged), by a phase vocoder of `pitch_n_fft` points (256, 512 or 1024; the pitch also uses `resampler`).
    Draws are counter-based, keyed by (seed, step) and indexed by the clip's position in the global batch."""

    def __init__(self, noise, snr=(50,), noised_rate=1.0, time_shift_ms=0, seed=None, sample_rate=None, rirs=None, reverb_rate=1.0,
                 rescale=True, filters=None, filter_rate=1.0, speed=None, speed_rate=1.0, loudness=None, loudness_rate=1.0, resampler=None,
                 tempo=None, tempo_rate=1.0, pitch=None, pitch_rate=1.0, pitch_n_fft=512):
        from classifier.params import pr
        if noise is None and rirs is None and filters is None and speed is None and loudness is None and tempo is None and pitch is None:
            raise ValueError("WaveAugment needs a noise bank, a RIR bank or both")
        srate, lrate = _rate("speed_rate", speed_rate), _rate("loudness_rate", loudness_rate)
        self.speed = None if speed is None else _range("speed", speed, 0.5, 2.0)
        self.loudness = None if loudness is None else _range("loudness", loudness, -80.0, 0.0, " dBFS")
        trate, prate = _rate("tempo_rate", tempo_rate), _rate("pitch_rate", pitch_rate)
        self.tempo = None if tempo is None else _range("tempo", tempo, 0.5, 2.0)
        self.pitch = None if pitch is None else _range("pitch", pitch, -12.0, 12.0, " semitones")
        if isinstance(pitch_n_fft, bool) or pitch_n_fft not in _l.PITCH_N_FFT:
            raise ValueError("pitch_n_fft must be one of %s, got %r" % (", ".join(str(n) for n in _l.PITCH_N_FFT), pitch_n_fft))
        self.tempo_rate, self.pitch_rate, self.pitch_n_fft = trate, prate, int(pitch_n_fft)
        if resampler is not None and not isinstance(resampler, Resampler):
            raise ValueError("resampler must be a kws_amd.augment.Resampler, got %r" % (resampler,))
        self.resampler = resampler if resampler is not None or (self.speed is None and self.pitch is None) else Resampler()
        self.speed_rate, self.loudness_rate = srate, lrate
        frate, rrate, rate = _rate("filter_rate", filter_rate), _rate("reverb_rate", reverb_rate), _rate("noised_rate", noised_rate)
        snr = parse_snr(snr)
        if not 1 <= len(snr) <= _l.AUG_MAX_SNR:
            raise ValueError("the SNR list needs 1..%d values, got %d" % (_l.AUG_MAX_SNR, len(snr)))
        for i, s in enumerate(snr):                         # kws_augment_plan's range: beyond it the float32 gain can overflow
            if not -_l.AUG_MAX_SNR_DB <= s <= _l.AUG_MAX_SNR_DB:
                raise ValueError("SNR %d (%r dB) is outside [-%g, %g]" % (i, s, _l.AUG_MAX_SNR_DB, _l.AUG_MAX_SNR_DB))
        if not float(time_shift_ms) >= 0:
            raise ValueError("time_shift_ms must be >= 0, got %r" % time_shift_ms)
        self.noise = None if noise is None else noise if isinstance(noise, NoiseBank) else NoiseBank(noise)
        self.rirs = None if rirs is None else rirs if isinstance(rirs, RirBank) else RirBank(rirs)
        self.filters = None if filters is None else filters if isinstance(filters, FilterBank) else FilterBank(filters, sample_rate)
        self.reverb_rate, self.rescale, self.filter_rate = rrate, bool(rescale), frate
        self.snr, self.noised_rate, self.time_shift_ms = snr, rate, float(time_shift_ms)
        sr = int(sample_rate or pr.sample_rate)
        self.max_shift = int(round(self.time_shift_ms * sr / 1000.0))
        self.seed = int(np.random.randint(0, 2 ** 62) if seed is None else seed) & (2 ** 64 - 1)

    @property
    def perturbs(self):
        """whether the speed / loudness stage is configured"""
        return self.speed is not None or self.loudness is not None

    @property
    def speed_seed(self):
        return self.seed ^ SPEED_SEED_MIX

    def speed_params(self, max_samples):
        p = _l.KwsSpeedParams()
        if self.speed is not None:
            p.speed_rate, p.speed_lo, p.speed_hi = self.speed_rate, self.speed[0], self.speed[1]
        if self.loudness is not None:
            p.loud_rate, p.loud_lo_db, p.loud_hi_db = self.loudness_rate, self.loudness[0], self.loudness[1]
        p.max_samples, p.reserved, p.seed = int(max_samples), 0, self.speed_seed
        return p

    def perturb(self, wav, valid_len=None, index=None, step=0, position_base=0, explicit_speed=None, explicit_db=None, max_samples=None,
                out=None, lengths=None, speed_used=None, gain_used=None):
        """-> (out (B, max_samples) float32, lengths (B,) int32, speed_used (B,) float32, gain_used (B,) float32): the B clips
        wav[index] (default: every row), each played at the ratio drawn for (seed, step) at global position position_base + b
        (speed_used = the ratio, 0 for a clip left at its speed: that one is the float32 conversion, bit for bit) and set to the level
        drawn for it (gain_used = the gain, 1 for a clip left at its level), head-aligned, zeros after.  A clip's whole valid length is
        the source, not only its first max_samples.  explicit_speed: B ratios (0, or 0.5..2) instead of the draws; explicit_db: B
        targets in dBFS (NaN: not levelled) instead of the draws.  out / lengths / speed_used / gain_used: optional preallocated CUDA
        buffers (out may be wider than max_samples; speed_used=False / gain_used=False skip them)."""
        from classifier.params import pr
        torch = _torch()
        _, stride, B, ix, vl = _clip_batch(wav, valid_len, index)
        ms = int(pr.max_samples if max_samples is None else max_samples)
        exs = _explicit(explicit_speed, np.float32, B, "speed")
        if exs is not None and self.resampler is None and exs.any():
            raise ValueError("this WaveAugment has no resampler: give speed=... or resampler=... to change a clip's speed")
        exd = _explicit(explicit_db, np.float32, B, "loudness")
        if exs is not None and speed_used is False:
            speed_used = None                               # the explicit ratios are staged there
        if exd is not None and gain_used is False:
            gain_used = None                                # the explicit targets are staged there
        out, lengths, speed_used, gain_used = _outputs(wav, B, ms, out, lengths, (speed_used, torch.float32), (gain_used, torch.float32))
        _l.check(_l.get_lib().kws_speed_apply(None if self.resampler is None else self.resampler.handle(), ctypes.byref(self.speed_params(ms)),
                                              wav.data_ptr(), _wav_code(wav), ix, B, stride, vl, int(position_base), int(step),
                                              _host_ptr(exs), _host_ptr(exd), out.data_ptr(), out.shape[1], lengths.data_ptr(),
                                              _ptr(speed_used), _ptr(gain_used), torch.cuda.current_stream().cuda_stream))
        if exs is not None or exd is not None:
            torch.cuda.current_stream().synchronize()       # the host values are copied from pageable memory
        return out, lengths, speed_used, gain_used

    @property
    def vocodes(self):
        """whether the tempo / pitch stage is configured"""
        return self.tempo is not None or self.pitch is not None

    @property
    def pitch_seed(self):
        return self.seed ^ PITCH_SEED_MIX

    def pitch_params(self, max_samples):
        p = _l.KwsPitchParams()
        if self.tempo is not None:
            p.tempo_rate, p.tempo_lo, p.tempo_hi = self.tempo_rate, self.tempo[0], self.tempo[1]
        if self.pitch is not None:
            p.pitch_rate, p.pitch_lo, p.pitch_hi = self.pitch_rate, self.pitch[0], self.pitch[1]
        p.n_fft, p.max_samples, p.reserved, p.seed = self.pitch_n_fft, int(max_samples), 0, self.pitch_seed
        return p

    def pitch_perturb(self, wav, valid_len=None, index=None, step=0, position_base=0, explicit_tempo=None, explicit_semitones=None,
                      max_samples=None, out=None, lengths=None, tempo_used=None, pitch_used=None, workspace=None, tile_clips=None):
        """-> (out (B, max_samples) float32, lengths (B,) int32, tempo_used (B,) float32, pitch_used (B,) float32): the B clips
        wav[index] (default: every row), each stretched at the tempo drawn for (seed, step) at global position position_base + b
        (tempo_used = the tempo, 0 for a clip left at its tempo) and shifted by the semitones drawn for it (pitch_used = the shift,
        NaN for a clip left at its pitch; a clip left at both is the float32 conversion, bit for bit), head-aligned, zeros after.  A
        clip's whole valid length is the source, not only its first max_samples.  explicit_tempo: B tempos (0, or 0.5..2) instead of
        the draws; explicit_semitones: B shifts in -12..12 (NaN: not pitched) instead of the draws.  out / lengths / tempo_used /
        pitch_used: optional preallocated CUDA buffers (out may be wider than max_samples; tempo_used=False / pitch_used=False skip
        them).  workspace: an optional CUDA uint8 tensor of at least pitch_workspace_bytes(pitch_n_fft, max_samples, 1) bytes (the
        batch is walked in tiles of as many clips as it holds); default: a fresh one for min(B, tile_clips or PITCH_TILE_CLIPS)
        clips.  The result does not depend on the tile."""
        from classifier.params import pr
        torch = _torch()
        _, stride, B, ix, vl = _clip_batch(wav, valid_len, index)
        ms = int(pr.max_samples if max_samples is None else max_samples)
        ext = _explicit(explicit_tempo, np.float32, B, "tempo")
        exp = _explicit(explicit_semitones, np.float32, B, "pitch")
        if exp is not None and self.resampler is None and not np.isnan(exp).all():
            raise ValueError("this WaveAugment has no resampler: give pitch=... or resampler=... to shift a clip's pitch")
        if ext is not None and tempo_used is False:
            tempo_used = None                               # the explicit tempos are staged there
        if exp is not None and pitch_used is False:
            pitch_used = None                               # the explicit shifts are staged there
        out, lengths, tempo_used, pitch_used = _outputs(wav, B, ms, out, lengths, (tempo_used, torch.float32), (pitch_used, torch.float32))
        if workspace is None and B > 0:
            tile = max(1, min(B, int(tile_clips or PITCH_TILE_CLIPS)))
            workspace = torch.empty((pitch_workspace_bytes(self.pitch_n_fft, ms, tile),), dtype=torch.uint8, device=wav.device)
        elif workspace is not None and (workspace.dtype != torch.uint8 or not workspace.is_cuda or not workspace.is_contiguous()):
            raise ValueError("workspace must be a contiguous CUDA uint8 tensor")
        _l.check(_l.get_lib().kws_pitch_apply(None if self.resampler is None else self.resampler.handle(), ctypes.byref(self.pitch_params(ms)),
                                              wav.data_ptr(), _wav_code(wav), ix, B, stride, vl, int(position_base), int(step),
                                              _host_ptr(ext), _host_ptr(exp), out.data_ptr(), out.shape[1], lengths.data_ptr(),
                                              _ptr(tempo_used), _ptr(pitch_used), _ptr(workspace),
                                              0 if workspace is None else workspace.numel(), torch.cuda.current_stream().cuda_stream))
        if ext is not None or exp is not None:
            torch.cuda.current_stream().synchronize()       # the host values are copied from pageable memory
        return out, lengths, tempo_used, pitch_used

    @property
    def reverb_seed(self):
        return self.seed ^ REVERB_SEED_MIX

    def reverb_params(self, max_samples):
        p = _l.KwsReverbParams()
        p.reverb_rate, p.rescale, p.max_samples, p.reserved, p.seed = self.reverb_rate, int(self.rescale), int(max_samples), 0, self.reverb_seed
        return p

    def reverberate(self, wav, valid_len=None, index=None, step=0, position_base=0, explicit=None, max_samples=None, out=None, lengths=None,
                    rir_used=None):
        """-> (out (B, max_samples) float32, lengths (B,) int32, rir_used (B,) int32): the B clips wav[index] (default: every row),
        each convolved with the RIR drawn for (seed, step) at global position position_base + b (rir_used = its index) or left dry
        (rir_used = -1), head-aligned, zeros after.  explicit: B ints in [-1, len(rirs)) instead of the draws.  out / lengths / rir_used:
        optional preallocated CUDA buffers (out may be wider than max_samples; rir_used=False skips it)."""
        from classifier.params import pr
        torch = _torch()
        if self.rirs is None:
            raise ValueError("this WaveAugment has no RIR bank")
        _, stride, B, ix, vl = _clip_batch(wav, valid_len, index)
        ms = int(pr.max_samples if max_samples is None else max_samples)
        ex = _explicit(explicit, np.int32, B, "RIR choice")
        out, lengths, rir_used = _outputs(wav, B, ms, out, lengths, (rir_used, torch.int32))
        _l.check(_l.get_lib().kws_reverb_apply(self.rirs.handle(), ctypes.byref(self.reverb_params(ms)), wav.data_ptr(), _wav_code(wav), ix, B,
                                               stride, vl, int(position_base), int(step), _host_ptr(ex), out.data_ptr(), out.shape[1],
                                               lengths.data_ptr(), _ptr(rir_used), torch.cuda.current_stream().cuda_stream))
        if ex is not None:
            torch.cuda.current_stream().synchronize()       # the host choices are copied from pageable memory
        return out, lengths, rir_used

    @property
    def filter_seed(self):
        return self.seed ^ FILTER_SEED_MIX

    def filter_params(self, max_samples):
        p = _l.KwsFilterParams()
        p.filter_rate, p.rescale, p.max_samples, p.reserved, p.seed = self.filter_rate, int(self.rescale), int(max_samples), 0, self.filter_seed
        return p

    def filter(self, wav, valid_len=None, index=None, step=0, position_base=0, explicit=None, max_samples=None, out=None, lengths=None,
               filter_used=None):
        """-> (out (B, max_samples) float32, lengths (B,) int32, filter_used (B,) int32): the B clips wav[index] (default: every row),
        each filtered at zero phase with the design drawn for (seed, step) at global position position_base + b (filter_used = its
        index) or left dry (filter_used = -1; also every clip of Lv <= padlen), head-aligned, zeros after.  explicit: B ints in
        [-1, len(filters)) instead of the draws.  out / lengths / filter_used: optional preallocated CUDA buffers (out may be wider than
        max_samples, and may be wav itself for a float32 wav without index; lengths may be valid_len then; filter_used=False skips it)."""
        from classifier.params import pr
        torch = _torch()
        if self.filters is None:
            raise ValueError("this WaveAugment has no filter bank")
        _, stride, B, ix, vl = _clip_batch(wav, valid_len, index)
        ms = int(pr.max_samples if max_samples is None else max_samples)
        ex = _explicit(explicit, np.int32, B, "filter choice")
        if ex is not None and filter_used is False:
            filter_used = None                              # the explicit choices are staged there
        out, lengths, filter_used = _outputs(wav, B, ms, out, lengths, (filter_used, torch.int32))
        _l.check(_l.get_lib().kws_filter_apply(self.filters.handle(), ctypes.byref(self.filter_params(ms)), wav.data_ptr(), _wav_code(wav), ix,
                                               B, stride, vl, int(position_base), int(step), _host_ptr(ex), out.data_ptr(), out.shape[1],
                                               lengths.data_ptr(), _ptr(filter_used), torch.cuda.current_stream().cuda_stream))
        if ex is not None:
            torch.cuda.current_stream().synchronize()       # the host choices are copied from pageable memory
        return out, lengths, filter_used

    def params(self, max_samples):
        p = _l.KwsAugmentParams()
        p.noised_rate = self.noised_rate
        p.n_snr = len(self.snr)
        for i, s in enumerate(self.snr):
            p.snr_db[i] = s
        p.max_shift, p.max_samples, p.seed = self.max_shift, int(max_samples), self.seed
        return p

    def plan(self, wav, valid_len=None, index=None, step=0, position_base=0, explicit=None, max_samples=None, out=None):
        """-> (B, 8) int32 CUDA tensor of kws_aug_clip records (records() reads them) for the B clips wav[index] (default: every row).
        explicit: a CLIP_DTYPE array (apply / segment / offset / shift / snr_db taken from it) instead of the draws."""
        from classifier.params import pr
        torch = _torch()
        if self.noise is None:
            raise ValueError("this WaveAugment has no noise bank")
        _, stride, B, ix, vl = _clip_batch(wav, valid_len, index)
        ex = _explicit(explicit, CLIP_DTYPE, B, "plan", "records", flat=False)
        if out is None:
            out = torch.empty((B, 8), dtype=torch.int32, device=wav.device)
        p = self.params(pr.max_samples if max_samples is None else max_samples)
        _l.check(_l.get_lib().kws_augment_plan(self.noise.handle(), ctypes.byref(p), wav.data_ptr(), _wav_code(wav), ix, B, stride, vl,
                                               int(position_base), int(step), out.data_ptr(), _host_ptr(ex),
                                               torch.cuda.current_stream().cuda_stream))
        if ex is not None:
            torch.cuda.current_stream().synchronize()       # the host records are copied from pageable memory
        return out

    def apply(self, wav, plan, index=None, max_samples=None):
        """-> (rows (B, max_samples) float32, lengths (B,) int32): the clips m' the featurizer sees, head-aligned"""
        from classifier.params import pr
        torch = _torch()
        ms = int(pr.max_samples if max_samples is None else max_samples)
        B = plan.shape[0]
        out = torch.empty((B, ms), dtype=torch.float32, device=wav.device)
        lens = torch.empty((B,), dtype=torch.int32, device=wav.device)
        ix = 0
        if index is not None:
            if index.dtype != torch.int32 or not index.is_cuda or index.numel() != B:
                raise ValueError("index must be a CUDA int32 vector with one element per planned clip")
            ix = index.data_ptr()
        _l.check(_l.get_lib().kws_augment_apply(self.noise.handle(), plan.data_ptr(), wav.data_ptr(), _wav_code(wav), ix, B, wav.shape[1], ms,
                                                out.data_ptr(), ms, lens.data_ptr(), torch.cuda.current_stream().cuda_stream))
        return out, lens


def resample(wav, orig_sr, target_sr, resampler=None):
    """-> (B, ceil(n / r)) float32 CUDA tensor: the rows of wav (a contiguous CUDA tensor (B, n), float32 or int16 scaled by 1/32768)
    converted from orig_sr to target_sr, r = orig_sr / target_sr in [0.5, 2]: the file-conversion use of audio_convert.py
    (audio_resample), with the band-limited interpolation of WaveAugment's speed change at one fixed ratio.  Equal rates give the
    float32 conversion.  common.data_utils.load_wav keeps its own (scipy) resampling."""
    torch = _torch()
    if not wav.is_cuda or wav.dim() != 2 or not wav.is_contiguous():
        raise ValueError("wav must be a contiguous CUDA tensor of shape (rows, samples)")
    if not (orig_sr > 0 and target_sr > 0):
        raise ValueError("sample rates must be positive, got %r and %r" % (orig_sr, target_sr))
    r = np.float32(float(orig_sr) / float(target_sr))
    if not 0.5 <= r <= 2.0:
        raise ValueError("orig_sr / target_sr must be in [0.5, 2], got %g" % r)
    if resampler is not None and not isinstance(resampler, Resampler):
        raise ValueError("resampler must be a kws_amd.augment.Resampler, got %r" % (resampler,))
    rs = resampler if resampler is not None else Resampler()
    B, n = wav.shape
    if n < 1:
        raise ValueError("wav has no samples")
    same = float(orig_sr) == float(target_sr)
    n_out = n if same else int(math.ceil(float(n) / float(r)))
    out = torch.empty((B, n_out), dtype=torch.float32, device=wav.device)
    lengths = torch.empty((B,), dtype=torch.int32, device=wav.device)
    used = torch.empty((B,), dtype=torch.float32, device=wav.device)
    p = _l.KwsSpeedParams()
    p.max_samples = n_out
    ex = np.full((B,), 0.0 if same else r, np.float32)
    _l.check(_l.get_lib().kws_speed_apply(rs.handle(), ctypes.byref(p), wav.data_ptr(), _wav_code(wav), 0, B, n, 0, 0, 0, ex.ctypes.data, None,
                                          out.data_ptr(), out.shape[1], lengths.data_ptr(), used.data_ptr(), None,
                                          torch.cuda.current_stream().cuda_stream))
    torch.cuda.current_stream().synchronize()               # ex is copied from pageable memory
    return out


def _one_shot(wav, what):
    if not wav.is_cuda or wav.dim() != 2 or not wav.is_contiguous():
        raise ValueError("wav must be a contiguous CUDA tensor of shape (rows, samples)")
    if wav.shape[1] < 1:
        raise ValueError("wav has no samples")
    if wav.shape[1] > _l.PITCH_MAX_SAMPLES:
        raise ValueError("%s takes rows of at most %d samples, got %d" % (what, _l.PITCH_MAX_SAMPLES, wav.shape[1]))


def time_stretch(wav, rate, n_fft=512):
    """-> (B, floor(n / rate + 0.5)) float32 CUDA tensor: the rows of wav (a contiguous CUDA tensor (B, n), float32 or int16 scaled by
    1/32768) played `rate` times faster (0.5..2) at their pitch: WaveAugment's phase vocoder at one fixed tempo."""
    _torch()
    _one_shot(wav, "time_stretch")
    rate = np.float32(rate)
    if not 0.5 <= rate <= 2.0:
        raise ValueError("rate must be in [0.5, 2], got %g" % rate)
    B, n = wav.shape
    n_out = max(int(math.floor(float(n) / float(rate) + 0.5)), 1)
    aug = WaveAugment(None, tempo=(1.0, 1.0), tempo_rate=0.0, pitch_n_fft=n_fft, seed=0)
    return aug.pitch_perturb(wav, explicit_tempo=np.full((B,), rate, np.float32), max_samples=n_out, tempo_used=None, pitch_used=False)[0]


def pitch_shift(wav, n_steps, n_fft=512, resampler=None):
    """-> (B, n) float32 CUDA tensor: the rows of wav (a contiguous CUDA tensor (B, n), float32 or int16 scaled by 1/32768) shifted by
    n_steps semitones (-12..12) at their duration (the last sample or two of a row may be zero: the length is rounded twice):
    WaveAugment's phase vocoder and resampling at one fixed shift."""
    _torch()
    _one_shot(wav, "pitch_shift")
    n_steps = np.float32(n_steps)
    if not -12.0 <= n_steps <= 12.0:
        raise ValueError("n_steps must be in [-12, 12] semitones, got %g" % n_steps)
    B, n = wav.shape
    aug = WaveAugment(None, pitch=(0.0, 0.0), pitch_rate=0.0, pitch_n_fft=n_fft, resampler=resampler, seed=0)
    return aug.pitch_perturb(wav, explicit_semitones=np.full((B,), n_steps, np.float32), max_samples=n, tempo_used=False, pitch_used=None)[0]


def stft(wav, n_fft=512, valid_len=None, index=None):
    """-> (B, 1 + n // (n_fft / 4), n_fft / 2 + 1) complex64 CUDA tensor: the vocoder's analysis of the clips wav[index] (a contiguous
    CUDA tensor (rows, n), float32 or int16 scaled by 1/32768; valid_len: their lengths): frames of n_fft samples at hop n_fft / 4 under a
    periodic Hann window, the first one centred on sample 0 (n_fft / 2 zeros in front); frames past a clip's last are zeros."""
    torch = _torch()
    if isinstance(n_fft, bool) or n_fft not in _l.PITCH_N_FFT:
        raise ValueError("n_fft must be one of %s, got %r" % (", ".join(str(n) for n in _l.PITCH_N_FFT), n_fft))
    _, stride, B, ix, vl = _clip_batch(wav, valid_len, index)
    frames = 1 + stride // (n_fft // 4)
    out = torch.empty((B, frames, n_fft // 2 + 1, 2), dtype=torch.float32, device=wav.device)
    _l.check(_l.get_lib().kws_pitch_stft(wav.data_ptr(), _wav_code(wav), ix, B, stride, vl, int(n_fft), out.data_ptr(), frames,
                                         torch.cuda.current_stream().cuda_stream))
    return torch.view_as_complex(out)


def records(plan):
    """(B, 8) int32 plan tensor -> numpy CLIP_DTYPE records"""
    return np.ascontiguousarray(plan.cpu().numpy()).view(CLIP_DTYPE).reshape(-1)


# the feature-mask draws use seed ^ FMASK_SEED_MIX, independent of every wave stage's draws of the same seed (include/kws.h)
FMASK_SEED_MIX = 0xE7037ED1A0B428DB
# one kws_fmask_clip record
FMASK_DTYPE = np.dtype([("apply", "<i4"), ("warp_center", "<i4"), ("warp_shift", "<i4"), ("n_time", "<i4"), ("n_freq", "<i4"),
                        ("t0", "<i4", (_l.FMASK_MAX,)), ("tw", "<i4", (_l.FMASK_MAX,)), ("f0", "<i4", (_l.FMASK_MAX,)),
                        ("fw", "<i4", (_l.FMASK_MAX,))])


def _count(name, value, hi=None):
    n = int(value)
    if n != value or n < 0 or (hi is not None and n > hi):
        raise ValueError("%s must be an integer in [0, %s], got %r" % (name, "inf" if hi is None else hi, value))
    return n


class FeatureMask(object):
    """SpecAugment of the features (include/kws.h: kws_feature_mask): a `rate` share of the clips of every step gets `time_masks` blocks
    of up to `time_width` frames and `freq_masks` blocks of up to `freq_width` coefficients overwritten with the fill value ('mean': the
    clip's own mean of that coefficient; 'zero'), after an optional time warp that moves one frame by up to `warp` frames and
    interpolates the rest.  It works on features, so it applies to cached-feature training as well as behind the featurizer; draws are
    counter-based, keyed by (seed, step) and indexed by the clip's position in the global batch.

        model.fit(x, y, feature_mask=FeatureMask(time_masks=2, time_width=4, freq_masks=2, freq_width=3))"""

    def __init__(self, time_masks=2, time_width=4, freq_masks=2, freq_width=3, warp=0, rate=1.0, fill='mean', seed=0):
        self.time_masks, self.freq_masks = _count("time_masks", time_masks, _l.FMASK_MAX), _count("freq_masks", freq_masks, _l.FMASK_MAX)
        self.time_width, self.freq_width, self.warp = _count("time_width", time_width), _count("freq_width", freq_width), _count("warp", warp)
        self.rate = _rate("rate", rate)
        if fill not in _l.FMASK_FILL:
            raise ValueError("fill must be one of %s, got %r" % (", ".join(sorted(_l.FMASK_FILL)), fill))
        self.fill = fill
        self.seed = int(np.random.randint(0, 2 ** 62) if seed is None else seed) & (2 ** 64 - 1)

    @property
    def mask_seed(self):
        return self.seed ^ FMASK_SEED_MIX

    def params(self):
        p = _l.KwsFeatureMaskParams()
        p.rate, p.n_time, p.max_time_width, p.n_freq, p.max_freq_width = self.rate, self.time_masks, self.time_width, self.freq_masks, self.freq_width
        p.max_warp, p.fill, p.reserved, p.seed = self.warp, _l.FMASK_FILL[self.fill], 0, self.mask_seed
        return p

    def draw(self, T, F, position, step):
        """-> one FMASK_DTYPE record: the plan of the clip at global batch position `position` in step `step` (host only, no GPU)"""
        rec = _l.KwsFmaskClip()
        _l.check(_l.get_lib().kws_feature_mask_draw(ctypes.byref(self.params()), int(T), int(F), int(position), int(step), ctypes.byref(rec)))
        return np.frombuffer(bytes(rec), FMASK_DTYPE)[0]

    def __call__(self, feat, step, position_base=0, out=None, plan=None, return_plan=False):
        """-> out (or (out, plan tensor) with return_plan): the clips feat (B, T, F) float32 CUDA, each transformed by the plan drawn for
        (seed, step) at global position position_base + b, on the current stream.  out: None (a new tensor), feat itself (in place) or a
        contiguous float32 CUDA tensor of feat's shape.  plan: B FMASK_DTYPE records from the caller instead of the draws.  The plan
        tensor is (B, 21) int32 (mask_records() reads it)."""
        torch = _torch()
        if not feat.is_cuda or feat.dim() != 3 or not feat.is_contiguous() or feat.dtype != torch.float32:
            raise ValueError("feat must be a contiguous float32 CUDA tensor of shape (clips, n_features, feature_size)")
        B, T, F = feat.shape
        if out is None:
            out = torch.empty_like(feat)
        elif out.shape != feat.shape or not out.is_cuda or not out.is_contiguous() or out.dtype != torch.float32:
            raise ValueError("out must be a contiguous float32 CUDA tensor of shape %s" % (tuple(feat.shape),))
        ex = _explicit(plan, FMASK_DTYPE, B, "plan", "records", flat=False)
        plan_t = None
        if ex is not None or return_plan:
            plan_t = torch.empty((B, FMASK_DTYPE.itemsize // 4), dtype=torch.int32, device=feat.device)
        _l.check(_l.get_lib().kws_feature_mask(ctypes.byref(self.params()), feat.data_ptr(), out.data_ptr(), B, T, F, int(position_base),
                                               int(step), _host_ptr(ex), _ptr(plan_t), torch.cuda.current_stream().cuda_stream))
        if ex is not None:
            torch.cuda.current_stream().synchronize()       # the host records are copied from pageable memory
        return (out, plan_t) if return_plan else out


def mask_records(plan):
    """(B, 21) int32 plan tensor of FeatureMask.__call__ -> numpy FMASK_DTYPE records"""
    return np.ascontiguousarray(plan.cpu().numpy()).view(FMASK_DTYPE).reshape(-1)


def white_noise(length_ms=1000, sample_rate=16000, amplitude=0.7, seed=None):
    """A white-noise segment as tools/audio_process/white_noise.py makes it: int16 samples of a normal distribution truncated to
    [-1, 1] standard deviations, scale min(2^16, 2^int(16 amplitude))."""
    if not length_ms > 0:
        raise ValueError("length_ms must be > 0")
    n = int(sample_rate * (length_ms / 1000.0))
    scale = min(2 ** 16, 2 ** int(16 * amplitude))
    rng = np.random.default_rng(seed)
    z = np.empty(0)
    while z.size < n:                                   # truncnorm(-1, 1) by rejection
        d = rng.standard_normal(2 * n + 16)
        z = np.concatenate([z, d[np.abs(d) <= 1.0]])
    return (z[:n] * scale).astype(np.int16)
