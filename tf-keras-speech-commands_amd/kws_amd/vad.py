"""Voice-activity detection of whole recordings on the device (include/kws.h: kws_vad_*, csrc/kws_vad.hip).

`Vad` is the `simple` detector of the reference's tools/audio_process/speech_duration_check.py (class
VoiceActivityDetector, lines 21-176) for many recordings of ragged length at once: band-energy ratio per 20 ms window,
0.5 s median, speech intervals; plus the energy per second of tools/audio_process/silent_check.py:14-24 and a gather of
fixed-length clips for the featurizer and --raw_audio training.  `speech_duration` and `silent_check` mirror the two
reference functions for one file.  All arithmetic runs in the HIP library; there is no host fallback.
"""
import ctypes
import wave

import numpy as np

from . import lib as _l
from .stream import _pack_recordings, _stream, _torch


def read_wav(path):
    """-> (int16 mono samples, sample rate).  16-bit PCM; two channels are averaged as the reference's _convert_to_mono
    does (speech_duration_check.py:40-44)."""
    with wave.open(path, "rb") as wf:
        if wf.getsampwidth() != 2:
            raise ValueError("%s: only 16-bit PCM is supported" % path)
        ch, rate = wf.getnchannels(), wf.getframerate()
        data = np.frombuffer(wf.readframes(wf.getnframes()), dtype="<i2")
    if ch == 2:
        data = np.mean(data.reshape(-1, 2), axis=1, dtype=data.dtype)
    elif ch != 1:
        raise ValueError("%s: %d channels are not supported" % (path, ch))
    return np.ascontiguousarray(data, dtype=np.int16), rate


class VadResult(object):
    """ratio: (R, max_windows) float32 CUDA tensor, band / full per window (0 past n_windows[r]); smoothed: (R, max_windows)
    uint8 CUDA tensor; n_windows: list of R ints; segment_samples: (R, max_segments, 2) int32 CUDA tensor of {begin, end}
    sample indices; n_segments: (R,) int32 CUDA tensor, the true counts; span: (R, 2) int32 CUDA tensor;
    energy_per_second: (R,) float64 CUDA tensor.  `segments`, `span_seconds` and `is_silent` copy to the host."""

    def __init__(self, sample_rate, lengths, n_windows, ratio, smoothed, segment_samples, n_segments, span, energy_per_second):
        self.sample_rate, self.lengths, self.n_windows = sample_rate, lengths, n_windows
        self.ratio, self.smoothed, self.segment_samples = ratio, smoothed, segment_samples
        self.n_segments, self.span, self.energy_per_second = n_segments, span, energy_per_second

    @property
    def segments(self):
        """a list per recording of (begin_s, end_s), the reference's speech_begin / speech_end"""
        counts = self.n_segments.cpu().tolist()
        seg = self.segment_samples.cpu().numpy()
        cap = seg.shape[1]
        if any(c > cap for c in counts):
            raise ValueError("a recording has %d intervals, more than max_segments=%d" % (max(counts), cap))
        rate = self.sample_rate
        return [[(int(b) / rate, int(e) / rate) for b, e in seg[r, :c]] for r, c in enumerate(counts)]

    @property
    def span_seconds(self):
        """(R, 2) float64 array: (first begin, last end) in seconds, (0, 0) without an interval"""
        return self.span.cpu().numpy().astype(np.float64) / self.sample_rate

    def is_silent(self, threshold=0.2):
        """(R,) bool array, silent_check.py:21"""
        return self.energy_per_second.cpu().numpy() < threshold


class Vad(object):
    """VoiceActivityDetector of the reference with its defaults (speech_duration_check.py:25-32)."""

    def __init__(self, sample_rate=16000, window_t=0.02, hop_t=0.01, band=(300, 3000), energy_threshold=0.6, smooth_t=0.5):
        self._L = _l.get_lib()
        self.sample_rate = int(sample_rate)
        self._h = ctypes.c_void_p()
        _l.check(self._L.kws_vad_create(self.sample_rate, float(window_t), float(hop_t), float(band[0]), float(band[1]),
                                        float(energy_threshold), float(smooth_t), ctypes.byref(self._h)))
        v = [ctypes.c_int32(0) for _ in range(5)]
        _l.check(self._L.kws_vad_info(self._h, *[ctypes.byref(x) for x in v]))
        self.window_samples, self.hop_samples, self.bin_lo, self.bin_hi, self.median = [x.value for x in v]
        self.energy_threshold = float(energy_threshold)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.kws_vad_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def n_windows(self, n_samples):
        n = self._L.kws_vad_windows(self._h, int(n_samples))
        if n < 0:
            _l.check(int(n))
        return int(n)

    def _pack(self, torch, recordings, lengths):
        """-> ((R, stride) int16 or float32 CUDA tensor, host lengths)"""
        is_f32 = (isinstance(recordings, torch.Tensor) and recordings.dtype == torch.float32) or \
                 (isinstance(recordings, np.ndarray) and recordings.ndim == 2 and recordings.dtype == np.float32)
        if not is_f32:
            return _pack_recordings(torch, recordings, lengths, torch.device("cuda", torch.cuda.current_device()))
        t = recordings if isinstance(recordings, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(recordings))
        if t.dim() != 2:
            raise ValueError("float32 recordings must have shape (R, n)")
        if lengths is None:
            lens = [int(t.shape[1])] * int(t.shape[0])
        else:
            lens = [int(v) for v in (lengths.cpu().tolist() if isinstance(lengths, torch.Tensor) else np.asarray(lengths).tolist())]
        if len(lens) != t.shape[0] or any(v < 0 or v > t.shape[1] for v in lens):
            raise ValueError("lengths must give one sample count in 0..%d per recording" % t.shape[1])
        return t.cuda().contiguous(), lens

    def detect(self, recordings, lengths=None, max_segments=None, timings=None):
        """recordings: what kws_amd.stream.scan takes (a list of 1-D int16 arrays, or a padded (R, n) int16 array / CUDA
        tensor with `lengths`), or a padded (R, n) float32 array / tensor.  max_segments: capacity of the interval list per
        recording (default: what the longest recording can hold).  Two launches on the current stream; the host does not
        wait for the device.  `timings`: optional dict that receives a (start, end) CUDA event pair under "detect"."""
        torch = _torch()
        wav, lens = self._pack(torch, recordings, lengths)
        R, stride = int(wav.shape[0]), int(wav.shape[1])
        n_win = [self.n_windows(n) for n in lens]
        max_windows = self.n_windows(stride)
        if max_segments is None:
            max_segments = max(1, max_windows // 2 + 1)
        max_segments = int(max_segments)
        dev = wav.device
        ratio = torch.empty((R, max_windows), dtype=torch.float32, device=dev)
        smoothed = torch.empty((R, max_windows), dtype=torch.uint8, device=dev)
        segs = torch.empty((R, max_segments, 2), dtype=torch.int32, device=dev)
        n_seg = torch.zeros(R, dtype=torch.int32, device=dev)
        span = torch.zeros((R, 2), dtype=torch.int32, device=dev)
        eps = torch.zeros(R, dtype=torch.float64, device=dev)
        res = VadResult(self.sample_rate, lens, n_win, ratio, smoothed, segs, n_seg, span, eps)
        res.wav, res.d_lengths = wav, None
        if R == 0:
            return res
        d_len = torch.tensor(lens, dtype=torch.int32).to(dev, non_blocking=True)
        res.d_lengths = d_len
        ws_bytes = self._L.kws_vad_workspace_bytes(self._h, R, max_windows)
        if ws_bytes < 0:
            _l.check(int(ws_bytes))
        ws = torch.empty(int(ws_bytes) // 8, dtype=torch.int64, device=dev)
        code = _l.WAV_I16 if wav.dtype == torch.int16 else _l.WAV_F32
        ev = None
        if timings is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        _l.check(self._L.kws_vad_detect(self._h, wav.data_ptr(), code, R, stride, d_len.data_ptr(), max_windows, max_segments,
                                        ws.data_ptr(), int(ws_bytes), ratio.data_ptr(), smoothed.data_ptr(), segs.data_ptr(),
                                        n_seg.data_ptr(), span.data_ptr(), eps.data_ptr(), _stream()))
        if ev is not None:
            ev[1].record()
            timings["detect"] = ev
        return res

    def clips(self, recordings, result, clip_samples, pad_before=0, pad_after=0, align="left", triples=None):
        """One clip of `clip_samples` float32 samples (the featurizer's scaling) per detected interval, in recording order:
        cut from [max(0, begin - pad_before), min(L, end + pad_after)); align 'left' puts the zeros in front of a shorter
        cut (the data pipeline's audio_to_feature), 'center' on both sides; a longer cut keeps its head.  `triples`: an
        explicit (n, 3) int32 list of (recording, begin, end) instead of the result's intervals.  `recordings` may be None:
        the packed buffer of `result` is used.  -> ((n, clip_samples) float32 CUDA tensor, (n, 3) int32 CUDA tensor)"""
        torch = _torch()
        if align not in _l.VAD_ALIGN:
            raise ValueError("align must be 'left' or 'center'")
        if recordings is None:
            wav, lens, d_len = result.wav, result.lengths, result.d_lengths
        else:
            wav, lens = self._pack(torch, recordings, None if isinstance(recordings, (list, tuple)) else result.lengths)
            d_len = None
        dev = wav.device
        if d_len is None:
            d_len = torch.tensor(lens, dtype=torch.int32).to(dev)
        if triples is None:
            cap = result.segment_samples.shape[1]
            counts = torch.clamp(result.n_segments, max=cap).to(torch.int64)
            if bool((result.n_segments > cap).any()):
                raise ValueError("a recording has more intervals than max_segments=%d" % cap)
            keep = torch.arange(cap, device=dev)[None, :] < counts[:, None]                   # (R, cap)
            rec = torch.arange(wav.shape[0], device=dev, dtype=torch.int32)[:, None].expand(-1, cap)
            tri = torch.cat([rec[keep][:, None], result.segment_samples[keep]], dim=1).contiguous()
        else:
            tri = torch.as_tensor(np.ascontiguousarray(np.asarray(triples, dtype=np.int32).reshape(-1, 3))).to(dev)
        n = int(tri.shape[0])
        out = torch.empty((n, int(clip_samples)), dtype=torch.float32, device=dev)
        code = _l.WAV_I16 if wav.dtype == torch.int16 else _l.WAV_F32
        _l.check(self._L.kws_vad_gather_clips(wav.data_ptr(), code, int(wav.shape[0]), int(wav.shape[1]), d_len.data_ptr(), tri.data_ptr(),
                                              n, int(clip_samples), int(pad_before), int(pad_after), _l.VAD_ALIGN[align],
                                              out.data_ptr(), _stream()))
        return out, tri


def _load(wav_or_path):
    if isinstance(wav_or_path, (str, bytes)) or hasattr(wav_or_path, "__fspath__"):
        return read_wav(wav_or_path)
    data, rate = wav_or_path
    return np.ascontiguousarray(data, dtype=np.int16), int(rate)


def speech_duration(wav_or_path, vad=None):
    """speech_duration_check(wav_file, 'simple') of the reference (speech_duration_check.py:301-330) for a wav file or an
    (int16 samples, rate) pair -> (speech_begin, speech_end) in seconds, (0.0, 0.0) without an interval."""
    data, rate = _load(wav_or_path)
    vad = vad if vad is not None else Vad(rate)
    if vad.sample_rate != rate:
        raise ValueError("the detector is set up for %d Hz, the recording has %d Hz" % (vad.sample_rate, rate))
    b, e = vad.detect([data]).span_seconds[0]
    return float(b), float(e)


def silent_check(wav_or_path, threshold=0.2, vad=None):
    """silent_check(wav_file, threshold) of the reference (silent_check.py:14-24) -> bool"""
    data, rate = _load(wav_or_path)
    vad = vad if vad is not None else Vad(rate)
    return bool(vad.detect([data]).is_silent(threshold)[0])
