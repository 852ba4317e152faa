"""Sample-rate conversion in front of the detector (include/kws.h: kws_rate_*, csrc/kws_rate.hip).

`RateBank` is the polyphase bank of one (f_in, f_out) pair, a host object; `convert` turns ragged recordings of mixed rates into
recordings at one rate in one launch; `rate_table` and `launch` are the table and the call underneath, which `StreamServer` uses
with a history row per slot so that a stream may be cut into pushes anywhere and still give the same samples bit for bit.  The
definition (kernel, bank, order of the sums, emission rule) is the rate-conversion block of include/kws.h.  All arithmetic runs in
the HIP library; there is no host fallback.
"""
import ctypes

import numpy as np

from . import lib as _l
from .augment import KAISER_BEST_BETA


class RateBank(object):
    """The bank of f_in -> f_out: `p`, `q` (the rates over their gcd), `taps` (K, per wing; 0 when the rates are equal).
    ValueError for rates or parameters the library refuses (its message says which limit)."""

    def __init__(self, f_in, f_out, zero_crossings=16, beta=KAISER_BEST_BETA, rolloff=0.85):
        self.f_in, self.f_out, self.zero_crossings = int(f_in), int(f_out), int(zero_crossings)
        if self.f_in != f_in or self.f_out != f_out or self.zero_crossings != zero_crossings:
            raise ValueError("rates and zero_crossings must be integers, got %r, %r and %r" % (f_in, f_out, zero_crossings))
        self.beta, self.rolloff = float(beta), float(rolloff)
        L = _l.get_lib()
        h = ctypes.c_void_p()
        rc = L.kws_rate_bank_create(self.f_in, self.f_out, self.zero_crossings, self.beta, self.rolloff, ctypes.byref(h))
        if rc != 0:
            err = ValueError(L.kws_last_error().decode("utf-8", "replace"))
            err.code = rc
            raise err
        self._h, self._L = h, L
        p, q, k = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        _l.check(L.kws_rate_bank_info(h, ctypes.byref(p), ctypes.byref(q), ctypes.byref(k)))
        self.p, self.q, self.taps = p.value, q.value, k.value
        self.history = max(2 * self.taps - 1, 0)              # input samples a stream keeps between pushes

    def handle(self):
        if self._h is None:
            raise ValueError("this RateBank is closed")
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.kws_rate_bank_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def weights(self):
        """W as (q, 2K) float32, the values the device holds"""
        out = np.zeros((self.q, 2 * self.taps), np.float32)
        _l.check(self._L.kws_rate_bank_weights(self.handle(), out.ctypes.data, out.size))
        return out

    def counts(self, n_samples):
        """-> (emitted, total) of kws_rate_counts"""
        e, t = ctypes.c_int64(0), ctypes.c_int64(0)
        _l.check(self._L.kws_rate_counts(self.handle(), int(n_samples), ctypes.byref(e), ctypes.byref(t)))
        return e.value, t.value

    def emitted(self, n_samples):
        """M(N): outputs a stream has emitted after N input samples (an int, or an int64 array for an array)"""
        if isinstance(n_samples, np.ndarray):
            n = n_samples.astype(np.int64)
            return np.where(n <= self.taps, 0, -((-(n - self.taps) * self.q) // self.p))
        n = int(n_samples)
        return 0 if n <= self.taps else -((-(n - self.taps) * self.q) // self.p)

    def total(self, n_samples):
        """ceil(N q / p): outputs of a finished stream of N samples"""
        if isinstance(n_samples, np.ndarray):
            return -((-n_samples.astype(np.int64) * self.q) // self.p)
        return -((-int(n_samples) * self.q) // self.p)

    def max_chunk(self, chunk_size):
        """the longest push, in input samples, that emits at most chunk_size outputs: floor(chunk_size p / q)"""
        return int(chunk_size) * self.p // self.q


_banks = {}


def bank_for(f_in, f_out, zero_crossings=16, beta=KAISER_BEST_BETA, rolloff=0.85):
    """The shared `RateBank` of these arguments (made once per process, so its device copy is too)"""
    key = (int(f_in), int(f_out), int(zero_crossings), float(beta), float(rolloff))
    if key not in _banks:
        _banks[key] = RateBank(*key)
    return _banks[key]


def rate_table(bank, in_row, in_len, n_before, out_row, first, count, hist_in=-1, hist_out=-1, flags=0):
    """The (A, RATE_FIELDS) int32 table of kws_rate_convert from one value or one array of A values per field.  numpy only."""
    cols = [np.atleast_1d(np.asarray(v, dtype=np.int64)) for v in
            (bank, in_row, in_len, n_before, out_row, first, count, hist_in, hist_out, flags)]
    A = max(c.size for c in cols)
    b, row, ln, n, orow, fst, cnt, hin, hout, flg = [np.broadcast_to(c, (A,)) for c in cols]
    t = np.zeros((_l.RATE_FIELDS, A), np.int32)               # field-major while it is filled: contiguous writes

    def words(v):
        return (v & 0xFFFFFFFF).astype(np.uint32).view(np.int32), (v >> 32).astype(np.int32)

    t[_l.RATE_BANK], t[_l.RATE_IN_ROW], t[_l.RATE_IN_LEN], t[_l.RATE_OUT_ROW] = b, row, ln, orow
    t[_l.RATE_N_LO], t[_l.RATE_N_HI] = words(n)
    t[_l.RATE_FIRST_LO], t[_l.RATE_FIRST_HI] = words(fst)
    t[_l.RATE_COUNT], t[_l.RATE_HIST_IN], t[_l.RATE_HIST_OUT], t[_l.RATE_FLAGS] = cnt, hin, hout, flg
    return np.ascontiguousarray(t.T)


def launch(banks, wav, table, n_entries, out_i16=None, out_f32=None, out_width=None, hist=None, stream=None):
    """kws_rate_convert: `banks` a list of RateBank, `wav` an (rows, stride) int16 CUDA tensor, `table` an (>= n_entries,
    RATE_FIELDS) int32 CUDA tensor, out_i16 / out_f32 (rows, stride) CUDA tensors (one may be None), `hist` an (rows, stride)
    int16 CUDA tensor or None.  Stream-ordered; nothing is read back."""
    import torch
    out = out_i16 if out_i16 is not None else out_f32
    if out is None:
        raise ValueError("launch needs out_i16 or out_f32")
    for t, dt, name in ((wav, torch.int16, "wav"), (table, torch.int32, "table"), (out_i16, torch.int16, "out_i16"),
                        (out_f32, torch.float32, "out_f32"), (hist, torch.int16, "hist")):
        if t is not None and not (t.is_cuda and t.dtype == dt and t.dim() == 2 and t.is_contiguous()):
            raise ValueError("%s must be a contiguous 2-D CUDA tensor of %s" % (name, dt))
    if out_i16 is not None and out_f32 is not None and out_i16.shape != out_f32.shape:
        raise ValueError("out_i16 and out_f32 must have one shape")
    if table.shape[1] != _l.RATE_FIELDS or table.shape[0] < n_entries:
        raise ValueError("the table must hold %d entries of %d fields" % (n_entries, _l.RATE_FIELDS))
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    handles = (ctypes.c_void_p * len(banks))(*[b.handle() for b in banks])
    _l.check(_l.get_lib().kws_rate_convert(handles, len(banks), wav.data_ptr(), int(wav.shape[1]), int(wav.shape[0]), table.data_ptr(),
                                           int(n_entries), hist.data_ptr() if hist is not None else None,
                                           int(hist.shape[1]) if hist is not None else 0, int(hist.shape[0]) if hist is not None else 0,
                                           out_i16.data_ptr() if out_i16 is not None else None,
                                           out_f32.data_ptr() if out_f32 is not None else None, int(out.shape[1]), int(out.shape[0]),
                                           int(out.shape[1]) if out_width is None else int(out_width), stream))


def _rate_list(rates, R):
    if isinstance(rates, (int, np.integer)):
        return [int(rates)] * R
    rates = [int(v) for v in rates]
    if len(rates) != R:
        raise ValueError("%d sample rates for %d recordings" % (len(rates), R))
    return rates


def convert(recordings, rates, target_rate, lengths=None, dtype=np.int16, zero_crossings=16, beta=KAISER_BEST_BETA, rolloff=0.85,
            device=None):
    """Recordings at their own sample rates -> recordings at `target_rate`, in one launch.

    recordings: a list of 1-D int16 arrays, or a padded (R, n) int16 array / CUDA tensor with `lengths`; rates: one rate in Hz, or
    one per recording.  Returns (out, lengths): out the packed (R, stride) CUDA tensor, int16 (dtype=np.int16, what the detector
    reads) or float32 (dtype=np.float32, the samples before rounding), zero past each recording's own length
    ceil(n f_out / f_in); lengths the host list of those.  A recording already at target_rate is copied bit for bit."""
    import torch
    from .stream import _pack_recordings
    kind = np.dtype(dtype) if not isinstance(dtype, torch.dtype) else np.dtype(str(dtype).split(".")[-1])
    if kind not in (np.dtype(np.int16), np.dtype(np.float32)):
        raise ValueError("dtype must be int16 or float32, got %r" % (dtype,))
    if not torch.cuda.is_available():
        raise RuntimeError("kws_amd.rate needs a HIP device (torch.cuda.is_available() is False); there is no CPU fallback")
    dev = torch.device("cuda") if device is None else device
    n_rec = len(recordings) if not hasattr(recordings, "shape") else int(recordings.shape[0])
    rates = _rate_list(rates, n_rec)
    keys = sorted(set(rates))
    if len(keys) > _l.RATE_MAX_BANKS:
        raise ValueError("one call converts at most %d distinct sample rates, got %d" % (_l.RATE_MAX_BANKS, len(keys)))
    banks = [bank_for(r, target_rate, zero_crossings, beta, rolloff) for r in keys]
    wav, lens = _pack_recordings(torch, recordings, lengths, dev)
    which = np.array([keys.index(r) for r in rates], np.int64)
    n_in = np.array(lens, np.int64)
    total = np.array([banks[b].total(n) for b, n in zip(which, lens)], np.int64)
    stride = max(2, (int(total.max()) + 1) & ~1) if n_rec else 2
    out = torch.empty((n_rec, stride), dtype=torch.int16 if kind == np.dtype(np.int16) else torch.float32, device=dev)
    if n_rec:
        rows = np.arange(n_rec)
        table = rate_table(which, rows, n_in, 0, rows, 0, total, flags=_l.RATE_FINAL)
        d_table = torch.from_numpy(table).to(dev, non_blocking=True)
        i16 = kind == np.dtype(np.int16)
        launch(banks, wav, d_table, n_rec, out_i16=out if i16 else None, out_f32=None if i16 else out)
    return out, [int(v) for v in total]
