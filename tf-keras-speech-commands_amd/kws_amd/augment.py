"""Background-noise augmentation of raw audio on the GPU (include/kws.h: kws_noise_bank_*, kws_augment_*).

The reference makes training data robust offline: tools/audio_process/add_noise.py mixes a randomly chosen background recording into a
`noised_rate` fraction of the clips at an SNR drawn from a list and writes one fixed *_noised.wav copy per clip.  Here the same mix is
drawn afresh for every clip of every train step, inside the featurizer's sample loads:

    noise = NoiseBank("dataset/_background_noise_")          # or a list of 1-D float32 / int16 arrays
    aug = WaveAugment(noise, snr=(5, 10, 20), noised_rate=0.8, time_shift_ms=100, seed=1)
    model.fit(x_audio, y, augment=aug, sample_lengths=lengths)

Argument checks run on the host; the device copy of the bank is made on first use."""
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


class NoiseBank(object):
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
        self._h = None

    def __len__(self):
        return len(self.seg_len)

    def as_float32(self):
        """the bank as the device holds it (float32)"""
        return self.samples.astype(np.float32) / 32768.0 if self.dtype == _l.WAV_I16 else self.samples

    def handle(self):
        if self._h is None:
            _torch()
            L = _l.get_lib()
            h = ctypes.c_void_p()
            _l.check(L.kws_noise_bank_create(self.samples.ctypes.data, self.dtype, self.seg_len.ctypes.data, len(self.seg_len), ctypes.byref(h)))
            self._h, self._L = h, L
        return self._h

    def close(self):
        if self._h is not None and self._h.value:
            self._L.kws_noise_bank_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def parse_snr(snr):
    """add_noise.py --snr: a comma list ('5,10,20') or numbers"""
    if isinstance(snr, str):
        snr = [s for s in snr.split(",") if s.strip()]
    if isinstance(snr, (int, float)):
        snr = [snr]
    return [float(s) for s in snr]


class WaveAugment(object):
    """Per-clip background noise (add_noise.py:19-35) at an SNR drawn from `snr` for a `noised_rate` fraction of the clips, and an
    optional time shift of up to +-time_shift_ms (off by default; the reference has none).  Draws are counter-based, keyed by
    (seed, step) and indexed by the clip's position in the global batch."""

    def __init__(self, noise, snr=(50,), noised_rate=1.0, time_shift_ms=0, seed=None, sample_rate=None):
        from classifier.params import pr
        rate = float(noised_rate)
        if not 0.0 <= rate <= 1.0:
            raise ValueError("noised_rate must be in [0, 1], got %r" % noised_rate)
        snr = parse_snr(snr)
        if not 1 <= len(snr) <= _l.AUG_MAX_SNR:
            raise ValueError("the SNR list needs 1..%d values, got %d" % (_l.AUG_MAX_SNR, len(snr)))
        if not all(math.isfinite(s) for s in snr):
            raise ValueError("SNR values must be finite: %r" % (snr,))
        if not float(time_shift_ms) >= 0:
            raise ValueError("time_shift_ms must be >= 0, got %r" % time_shift_ms)
        self.noise = noise if isinstance(noise, NoiseBank) else NoiseBank(noise)
        self.snr, self.noised_rate, self.time_shift_ms = snr, rate, float(time_shift_ms)
        sr = int(sample_rate or pr.sample_rate)
        self.max_shift = int(round(self.time_shift_ms * sr / 1000.0))
        self.seed = int(np.random.randint(0, 2 ** 62) if seed is None else seed) & (2 ** 64 - 1)

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
        if not wav.is_cuda or wav.dim() != 2 or not wav.is_contiguous():
            raise ValueError("wav must be a contiguous CUDA tensor of shape (rows, stride)")
        rows, stride = wav.shape
        B, ix = rows, 0
        if index is not None:
            if index.dtype != torch.int32 or not index.is_cuda or index.dim() != 1 or not index.is_contiguous():
                raise ValueError("index must be a contiguous CUDA int32 vector")
            B, ix = index.numel(), index.data_ptr()
        vl = 0
        if valid_len is not None:
            if valid_len.dtype != torch.int32 or not valid_len.is_cuda or valid_len.numel() != rows:
                raise ValueError("valid_len must be a CUDA int32 tensor with one element per row of wav")
            vl = valid_len.data_ptr()
        ex = None
        if explicit is not None:
            ex = np.ascontiguousarray(np.asarray(explicit, CLIP_DTYPE))
            if ex.shape != (B,):
                raise ValueError("explicit plan has %s records for %d clips" % (ex.shape, B))
        if out is None:
            out = torch.empty((B, 8), dtype=torch.int32, device=wav.device)
        p = self.params(pr.max_samples if max_samples is None else max_samples)
        _l.check(_l.get_lib().kws_augment_plan(self.noise.handle(), ctypes.byref(p), wav.data_ptr(), _wav_code(wav), ix, B, stride, vl,
                                               int(position_base), int(step), out.data_ptr(), None if ex is None else ex.ctypes.data,
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


def records(plan):
    """(B, 8) int32 plan tensor -> numpy CLIP_DTYPE records"""
    return np.ascontiguousarray(plan.cpu().numpy()).view(CLIP_DTYPE).reshape(-1)


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
