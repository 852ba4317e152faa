"""Streaming post-processing on the device (include/kws.h, csrc/kws_stream.hip).

Mirrors the two helper classes of the reference's listen.py with the same constructor arguments, attributes and
methods -- `ThresholdDecoder` (listen.py:452-522) and `TriggerDetector` (listen.py:525-559) -- and adds `StreamBatch`,
which runs the whole per-chunk loop of listen.py:350-375 (`update_vectors`, predict, argmax / max, decode, detector
update) for S audio streams at once, and `scan`, the same loop over whole recordings that already lie in memory,
parallel over time, and `sweep`, which walks the detector over a scan's decoded scores at a whole grid of operating points
and counts hits, false alarms and misses against labelled events, and `collect` / `peaks`, which turn a scan's activations and
near misses into `Detections`: the clips (`Detections.clips`, `.save`) the next training run needs as `background` examples.
`StreamServer` is `StreamBatch` for streams that do not advance together: slots that open and close, a push that names the slots
with audio, chunks of differing lengths, an operating point per slot (`RaggedPlan` is its host-only bookkeeping).
All arithmetic runs in the HIP library; there is no host fallback.
"""
import ctypes

import numpy as np

from . import lib as _l
from .featurizer import Featurizer


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("kws_amd.stream needs a HIP device (torch.cuda.is_available() is False); there is no CPU fallback")
    return torch


def _stream():
    return _torch().cuda.current_stream().cuda_stream


class ThresholdDecoder(object):
    """listen.py:452-522.  `cd`, `min_out`, `max_out`, `out_range`, `center` as in the reference."""

    def __init__(self, mu_stds, center=0.5, resolution=200, min_z=-4, max_z=4):
        _torch()
        self._L = _l.get_lib()
        pairs = np.ascontiguousarray(np.asarray(mu_stds, dtype=np.float64).reshape(-1, 2))
        self._h = ctypes.c_void_p()
        _l.check(self._L.kws_decoder_create(pairs.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), pairs.shape[0], float(center),
                                            int(resolution), float(min_z), float(max_z), ctypes.byref(self._h)))
        mn, rg, n = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0)
        _l.check(self._L.kws_decoder_info(self._h, ctypes.byref(mn), ctypes.byref(rg), ctypes.byref(n)))
        self.min_out, self.out_range, self.max_out = mn.value, rg.value, mn.value + rg.value
        self.center = float(center)
        self.cd = np.empty(n.value, dtype=np.float64)
        _l.check(self._L.kws_decoder_table(self._h, self.cd.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), self.cd.size))

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.kws_decoder_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decode_device(self, raw):
        """raw: CUDA tensor, float32 (live-loop semantics) or float64 (Python-float semantics) -> float64 CUDA tensor."""
        torch = _torch()
        if not raw.is_cuda or raw.dtype not in (torch.float32, torch.float64):
            raise ValueError("raw must be a CUDA float32 or float64 tensor")
        raw = raw.contiguous()
        out = torch.empty(raw.shape, dtype=torch.float64, device=raw.device)
        code = _l.RAW_F32 if raw.dtype == torch.float32 else _l.RAW_F64
        _l.check(self._L.kws_decoder_decode(self._h, raw.data_ptr(), code, out.data_ptr(), raw.numel(), _stream()))
        return out

    def decode(self, raw_output):
        """Scalar or array in, same kind out.  float32 inputs follow the live loop (listen.py:361-367), where numpy
        evaluates 1/x - 1 in float32; Python floats / float64 follow the scalar path."""
        torch = _torch()
        if isinstance(raw_output, torch.Tensor):
            return self.decode_device(raw_output)
        a = np.asarray(raw_output)
        dt = np.float32 if a.dtype == np.float32 else np.float64
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=dt).reshape(-1)).cuda()
        res = self.decode_device(t).cpu().numpy().reshape(a.shape)
        return float(res) if a.ndim == 0 else res

    def encode(self, threshold):
        out = ctypes.c_double(0.0)
        _l.check(self._L.kws_decoder_encode(self._h, float(threshold), ctypes.byref(out)))
        return out.value


class TriggerDetector(object):
    """listen.py:525-559 for one stream (state lives on the device; `StreamBatch` is the many-stream form)."""

    def __init__(self, chunk_size, class_names, sensitivity=0.5, trigger_level=3):
        torch = _torch()
        self._L = _l.get_lib()
        self.chunk_size = int(chunk_size)
        self.class_names = class_names
        self.sensitivity = sensitivity
        self.trigger_level = trigger_level
        self._background = [i for i, n in enumerate(class_names) if n == 'background']
        self._state = torch.tensor([[0, -1]], dtype=torch.int32, device="cuda")
        self._fired = torch.zeros(1, dtype=torch.int32, device="cuda")

    @property
    def activation(self):
        return int(self._state[0, 0].item())

    @property
    def record_index(self):
        v = int(self._state[0, 1].item())
        return None if v < 0 else v

    def update(self, index, score):
        """Returns whether the new prediction caused an activation"""
        torch = _torch()
        index = int(np.asarray(index).reshape(-1)[0])
        score = float(np.asarray(score).reshape(-1)[0])
        # several names may be 'background' only in a malformed list; the kernel takes one index, -1 = none
        bg = index if index in self._background else (self._background[0] if self._background else -1)
        idx = torch.tensor([index], dtype=torch.int32, device="cuda")
        sc = torch.tensor([score], dtype=torch.float64, device="cuda")
        _l.check(self._L.kws_trigger_update(idx.data_ptr(), sc.data_ptr(), 1, bg, float(self.sensitivity), int(self.trigger_level),
                                            self.chunk_size, self._state.data_ptr(), self._fired.data_ptr(), _stream()))
        return bool(self._fired.item())


# listen.py:111-112 re-applies add_deltas to the whole matrix on every chunk, which doubles its width and makes the next
# np.concatenate raise; streaming with deltas never worked in the reference
_NO_DELTAS = "streaming with use_delta=True is not usable in the reference (listen.py:111-112) and is not offered"
_NOT_INT16 = "chunks must be int16 PCM (the 1/32768 scaling of buffer_to_audio happens on the device), got %s"


def _pcm(chunk):
    """One chunk of audio as PyAudio / wave.readframes deliver it (bytes, bytearray, memoryview), or an array -> int16 ndarray"""
    if isinstance(chunk, (bytes, bytearray, memoryview)):
        return np.frombuffer(chunk, dtype='<i2')                                          # buffer_to_audio's view, data_utils.py:19-21
    a = np.asarray(chunk)
    if a.dtype != np.int16:
        raise ValueError(_NOT_INT16 % a.dtype)
    return a


def _defaults(pr, featurizer, decoder):
    """-> (featurizer, decoder), the one given or the one `pr` describes"""
    return (featurizer if featurizer is not None else Featurizer(pr),
            decoder if decoder is not None else ThresholdDecoder(pr.threshold_config, pr.threshold_center))


def _num_classes(device_model, quantized, heads=None):
    if heads is not None:
        return heads.max_classes
    return quantized.num_classes if quantized is not None else device_model.spec.num_classes


def _forward(device_model, quantized, feat, heads=None, key=None):
    """(N, F, D) features -> (N, C) float32 probabilities, from `quantized`'s int8 forward when there is one, else the model's.
    With `heads` (a kws_amd.transfer.HeadBank): the backbone once over all rows (kws_model_embed), then kws_heads_apply gives every
    row the head its key names -- key = (int32 tensor, stride, head_of_key or None) -- and C is the bank's max_classes, the columns
    past a head's own classes zero."""
    if heads is not None:
        k, stride, head_of_key = key
        emb = device_model.embed(feat)
        return heads.launch(emb, emb.shape[0], k, key_stride=stride, head_of_key=head_of_key, want=("probs",))[0]
    if quantized is not None:
        return quantized.forward(feat)[0]
    return device_model.forward(feat, want_probs=True, want_argmax=False)[0]


def _check_heads(device_model, quantized, heads):
    """the refusals of a head bank, on the host: not with an int8 forward, and only on the backbone whose embeddings it reads"""
    if heads is None:
        return
    if quantized is not None:
        raise ValueError("heads and quantized do not go together: the int8 forwards end in their own head")
    if heads.embed_size != device_model.embed_size:
        raise ValueError("the bank's heads read %d-wide embeddings, %s produces %d-wide ones"
                         % (heads.embed_size, device_model.spec.model_type, device_model.embed_size))


def _head_ids(heads, ids, n, what):
    """`n` head ids of a bank (None: all 0) as an int32 host array, or ValueError"""
    if heads is None:
        if ids is not None:
            raise ValueError("%s needs heads=HeadBank" % what)
        return None
    a = np.zeros(n, np.int64) if ids is None else np.asarray(ids).reshape(-1)
    if a.dtype.kind not in "iu" or a.size != n:
        raise ValueError("%s must give one integer head id for each of the %d" % (what, n))
    if a.size and (a.min() < 0 or a.max() >= heads.capacity):
        raise ValueError("%s: head ids must lie in 0..%d" % (what, heads.capacity - 1))
    return a.astype(np.int32)


class _Streams(object):
    """What `StreamBatch` and `StreamServer` share: the refusal of deltas, the model, featurizer and decoder, the geometry, and per
    stream the feature window (mfccs), the detector state and the last (index, score, fired)."""

    def __init__(self, pr, device_model, quantized, heads=None):
        if pr.use_delta:
            raise ValueError(_NO_DELTAS)
        _check_heads(device_model, quantized, heads)
        _torch()
        self._L = _l.get_lib()
        self.pr, self.model, self.quantized, self.heads = pr, device_model, quantized, heads

    def head_class_names(self, head):
        """the class names of an activation in a stream that listens with `head` of the bank (class_names without a bank)"""
        return self.class_names if self.heads is None else self.heads.class_names[int(head)]

    def _allocate(self, n_streams, chunk_size, class_names, decoder, featurizer, background_index):
        torch = _torch()
        pr = self.pr
        self.S, self.chunk_size = n_streams, chunk_size
        self.background_index = int(background_index)
        if class_names is not None:
            assert class_names[0] == 'background', '1st class should be background.'      # listen.py:66
        self.class_names = class_names
        self.featurizer, self.decoder = _defaults(pr, featurizer, decoder)
        self.window_samples, self.hop_samples = pr.window_samples, pr.hop_samples
        self.F, self.D = pr.n_features, pr.n_mfcc
        self.cap = self.window_samples + self.chunk_size                                  # a carry and one chunk
        S, dev = self.S, self.model.device
        self.mfccs = torch.zeros((S, self.F, self.D), dtype=torch.float32, device=dev)
        self.state = torch.zeros((S, 2), dtype=torch.int32, device=dev)
        self.state[:, 1] = -1
        self.index = torch.zeros(S, dtype=torch.int32, device=dev)
        self.score = torch.zeros(S, dtype=torch.float64, device=dev)
        self.fired = torch.zeros(S, dtype=torch.int32, device=dev)
        self.probs = None


class StreamBatch(_Streams):
    """S lock-stepped audio streams through update_vectors -> model -> decode -> trigger (listen.py:96-114, 350-375).

    push(chunks) takes one chunk of int16 PCM per stream -- (S, n) int16 array / CUDA tensor, or a list of S `bytes`
    objects as PyAudio / wave.readframes deliver them -- and returns (index, score, fired) as CUDA tensors of length S.
    With `quantized` (a kws_amd.quant.QuantizedCNN / QuantizedCNNLite) the probabilities come from its int8 forward instead of
    device_model's.  With `heads` (a kws_amd.transfer.HeadBank) stream s listens with head stream_heads[s] of the bank (default 0)
    on device_model's backbone; probs is then (S, heads.max_classes).
    """

    def __init__(self, pr, device_model, n_streams, chunk_size=1024, class_names=None, sensitivity=0.5, trigger_level=3,
                 decoder=None, featurizer=None, background_index=0, quantized=None, heads=None, stream_heads=None):
        torch = _torch()                                                                  # a missing device is named first, as `scan` does
        _Streams.__init__(self, pr, device_model, quantized, heads)
        self.sensitivity, self.trigger_level = float(sensitivity), int(trigger_level)
        ids = _head_ids(heads, stream_heads, int(n_streams), "stream_heads")
        self.stream_head = None if ids is None else torch.from_numpy(ids).to(device_model.device)
        self._allocate(int(n_streams), int(chunk_size), class_names, decoder, featurizer, background_index)
        self.win = torch.zeros((self.S, self.cap), dtype=torch.int16, device=device_model.device)     # carried + new samples
        self.n_win = 0

    def _chunk_tensor(self, chunks):
        torch = _torch()
        if isinstance(chunks, torch.Tensor):
            t = chunks
        else:
            if isinstance(chunks, (list, tuple)) and chunks and isinstance(chunks[0], (bytes, bytearray, memoryview)):
                a = np.stack([_pcm(c) for c in chunks])
            else:
                a = _pcm(chunks)
            t = torch.from_numpy(np.ascontiguousarray(a))
        if t.dim() != 2 or t.shape[0] != self.S or t.dtype != torch.int16:
            raise ValueError("expected %d int16 chunks of equal length" % self.S)
        if t.shape[1] > self.chunk_size:
            raise ValueError("chunk of %d samples exceeds chunk_size=%d" % (t.shape[1], self.chunk_size))
        return t.to(self.win.device, non_blocking=True)

    def update_vectors(self, chunks):
        """listen.py:96-114 for all streams; returns the (S, n_features, n_mfcc) feature tensor (device, updated in place)."""
        t = self._chunk_tensor(chunks)
        n = t.shape[1]
        self.win[:, self.n_win:self.n_win + n] = t
        self.n_win += n
        if self.n_win >= self.window_samples:
            rows = self.featurizer.raw(self.win, n_samples=self.n_win)                    # (S, n_new, D)
            n_new = rows.shape[1]
            _l.check(self._L.kws_stream_push_rows(self.mfccs.data_ptr(), rows.data_ptr(), self.S, self.F, self.D, n_new, _stream()))
            used = n_new * self.hop_samples
            keep = max(self.n_win - used, 0)              # hop > window: the rows may consume more than is held; the carry empties (listen.py:105)
            if keep > 0:
                self.win[:, :keep] = self.win[:, used:self.n_win].clone()
            self.n_win = keep
        return self.mfccs

    def push(self, chunks):
        """One step of the loop listen.py:350-375 for every stream."""
        self.probs = _forward(self.model, self.quantized, self.update_vectors(chunks), self.heads, (self.stream_head, 1, None))
        _l.check(self._L.kws_stream_postprocess(self.decoder.handle, self.probs.data_ptr(), self.S, self.probs.shape[1],
                                                self.background_index, self.sensitivity, self.trigger_level, self.chunk_size,
                                                self.state.data_ptr(), self.index.data_ptr(), self.score.data_ptr(),
                                                self.fired.data_ptr(), _stream()))
        return self.index, self.score, self.fired


class RaggedStep(object):
    """One push as `RaggedPlan.push` worked it out, entry a for slots[a]: table, the (A, RAGGED_FIELDS) int32 array the kernels
    read (include/kws.h); n_new, rows the push gives the slot; carry, its carry length after the push; first, the position in
    the slot's stream (samples since it was opened) of the first sample of the first new row -- row j covers
    [first + j * hop, first + j * hop + window); max_frames = max(n_new), 0 for an empty push.
    A push that names a slot with a sample rate of its own also has rate, the (pushed entries, RATE_FIELDS) int32 table of
    kws_rate_convert (None otherwise); emitted, per pushed entry the samples it gives the detector; and entries, the positions in the
    push of the entries that emit at least one: the ragged table, n_new, carry and first describe those alone, in converted samples."""

    def __init__(self, table, n_new, carry, first, hop_samples, rate=None, emitted=None, entries=None):
        self.table, self.n_new, self.carry, self.first, self.hop_samples = table, n_new, carry, first, hop_samples
        self.rate, self.emitted, self.entries = rate, emitted, entries
        self.A = int(table.shape[0])
        self.max_frames = int(n_new.max()) if self.A else 0

    def frame_starts(self, a):
        return [int(self.first[a]) + j * self.hop_samples for j in range(int(self.n_new[a]))]


class RaggedPlan(object):
    """The host's half of `StreamServer`: which slots are open, each slot's carry length (a mirror of what the device holds,
    kept with the arithmetic of listen.py:96-105, so nothing is ever read back), its operating point, the restart a freshly
    opened slot still owes, and the checks of a push's arguments.  numpy only, no device.

    With `sample_rate` (the detector's) a slot may be opened at a rate of its own: the plan then keeps its `RateBank` (`bank[slot]`, None
    for a slot at the detector's rate; `banks` lists the distinct ones, `banks[0]` the pass-through), the samples it has received
    (`received[slot]`, the N of include/kws.h's rate-conversion block; `sent[slot]` = M(N), what it has emitted), its longest push (`max_chunk[slot]`) and which of its two
    history rows is current (`parity[slot]`); chunk lengths of such a slot are in ITS samples, carry and position in converted ones."""

    def __init__(self, n_slots, chunk_size, window_samples, hop_samples, sensitivity=0.5, trigger_level=3, sample_rate=None):
        self.sample_rate = None if sample_rate is None else int(sample_rate)
        self.banks, self.bank, self.bank_index = [], [None] * int(n_slots), np.zeros(int(n_slots), np.int64)
        self.received = np.zeros(int(n_slots), np.int64)
        self.sent = np.zeros(int(n_slots), np.int64)           # M(received): samples the slot's converter has emitted
        self._pqk = np.tile(np.array([[1], [1], [0]], np.int64), (1, int(n_slots)))    # the bank's p, q, K per slot; 1, 1, 0 passes through
        self.parity = np.zeros(int(n_slots), np.int64)
        self.rate_reset = np.zeros(int(n_slots), bool)
        self.max_chunk = np.full(int(n_slots), int(chunk_size), np.int64)
        self.S, self.chunk_size = int(n_slots), int(chunk_size)
        self.window_samples, self.hop_samples = int(window_samples), int(hop_samples)
        if self.S < 0 or self.chunk_size < 1 or self.window_samples < 1 or self.hop_samples < 1:
            raise ValueError("RaggedPlan needs n_slots >= 0 and positive chunk_size / window / hop")
        self.cap = self.window_samples + self.chunk_size
        self.default_sensitivity, self.default_trigger_level = float(sensitivity), int(trigger_level)
        self.carry = np.zeros(self.S, np.int64)
        self.position = np.zeros(self.S, np.int64)             # samples of the slot's stream in front of its carry
        self.is_open = np.zeros(self.S, bool)
        self.reset = np.zeros(self.S, bool)
        self.sensitivity = np.full(self.S, self.default_sensitivity, np.float64)
        self.trigger_level = np.full(self.S, self.default_trigger_level, np.int32)

    def _bank(self, sample_rate):
        """-> (bank, its index in `banks`) of a slot at sample_rate, (None, 0) at the detector's own rate"""
        if sample_rate is None or (self.sample_rate is not None and int(sample_rate) == self.sample_rate):
            return None, 0
        if self.sample_rate is None:
            raise ValueError("a slot with a sample_rate of its own needs a plan made with the detector's sample_rate")
        from .rate import bank_for
        bank = bank_for(sample_rate, self.sample_rate)                         # ValueError for a pair the library refuses
        if not self.banks:
            self.banks.append(bank_for(self.sample_rate, self.sample_rate))
        if bank not in self.banks:
            if len(self.banks) == _l.RATE_MAX_BANKS:
                raise ValueError("a server converts from at most %d distinct sample rates" % (_l.RATE_MAX_BANKS - 1))
            self.banks.append(bank)
        return bank, self.banks.index(bank)

    def open(self, sensitivity=None, trigger_level=None, sample_rate=None):
        """-> the lowest free slot, marked for a restart that rides in its next push.  sample_rate: the rate its audio arrives at,
        None for the detector's."""
        bank, which = self._bank(sample_rate)
        free = np.flatnonzero(~self.is_open)
        if free.size == 0:
            raise RuntimeError("the server is full: all %d slots are open" % self.S)
        slot = int(free[0])
        self.bank[slot], self.bank_index[slot], self.received[slot], self.rate_reset[slot] = bank, which, 0, bank is not None
        self.sent[slot], self._pqk[:, slot] = 0, (1, 1, 0) if bank is None else (bank.p, bank.q, bank.taps)
        self.max_chunk[slot] = self.chunk_size if bank is None else bank.max_chunk(self.chunk_size)
        self.is_open[slot], self.reset[slot] = True, True
        self.carry[slot] = self.position[slot] = 0
        self.sensitivity[slot] = self.default_sensitivity if sensitivity is None else float(sensitivity)
        self.trigger_level[slot] = self.default_trigger_level if trigger_level is None else int(trigger_level)
        return slot

    def _open_slot(self, slot):
        if isinstance(slot, (bool, np.bool_)) or not isinstance(slot, (int, np.integer)):
            raise ValueError("a slot is an integer, got %r" % (slot,))
        if not 0 <= slot < self.S:
            raise ValueError("slot %d is out of range 0..%d" % (slot, self.S - 1))
        if not self.is_open[slot]:
            raise ValueError("slot %d is closed" % slot)
        return int(slot)

    def close(self, slot):
        self.is_open[self._open_slot(slot)] = False

    def check(self, slots, lengths):
        """-> (slots, lengths) as int64 arrays, or ValueError naming the fault; changes nothing"""
        s = np.asarray(slots).reshape(-1) if len(slots) else np.zeros(0, np.int64)
        n = np.asarray(lengths).reshape(-1) if len(lengths) else np.zeros(0, np.int64)
        if s.dtype.kind not in "iu" or n.dtype.kind not in "iu":
            raise ValueError("slots and lengths must be integers")
        s, n = s.astype(np.int64), n.astype(np.int64)
        if s.size != n.size:
            raise ValueError("%d slots for %d chunks" % (s.size, n.size))
        bad = np.flatnonzero((s < 0) | (s >= self.S))
        if bad.size:
            raise ValueError("slot %d is out of range 0..%d" % (s[bad[0]], self.S - 1))
        bad = np.flatnonzero(~self.is_open[s])
        if bad.size:
            raise ValueError("slot %d is closed" % s[bad[0]])
        if s.size > 1:
            o = np.sort(s)
            dup = np.flatnonzero(o[1:] == o[:-1])
            if dup.size:
                raise ValueError("slot %d is named twice in one push (duplicate slot)" % o[dup[0]])
        bad = np.flatnonzero(n < 1)
        if bad.size:
            raise ValueError("the chunk for slot %d is empty" % s[bad[0]])
        bad = np.flatnonzero(n > (self.max_chunk[s] if self.banks else self.chunk_size))    # no gather while every slot is native
        if bad.size:
            b = bad[0]
            if self.bank[s[b]] is None:
                raise ValueError("chunk of %d samples for slot %d exceeds chunk_size=%d" % (n[b], s[b], self.chunk_size))
            raise ValueError("chunk of %d samples for slot %d exceeds its max_chunk=%d: at %d Hz a longer one could give the detector more "
                             "than chunk_size=%d samples" % (n[b], s[b], self.max_chunk[s[b]], self.bank[s[b]].f_in, self.chunk_size))
        return s, n

    def chunks(self, slots, chunks, lengths=None):
        """A push's audio in the forms `StreamServer.push` takes -> (rows, lengths): rows is a list of 1-D int16 arrays, an
        (A, n) int16 array or an (A, n) int16 tensor; lengths the int64 sample counts, not yet checked against chunk_size."""
        A = len(slots)
        if hasattr(chunks, "is_cuda") or (isinstance(chunks, np.ndarray) and chunks.ndim == 2):
            if str(chunks.dtype).split(".")[-1] != "int16":                    # numpy's or torch's, without importing torch
                raise ValueError(_NOT_INT16 % chunks.dtype)
            if len(chunks.shape) != 2 or chunks.shape[0] != A:
                raise ValueError("expected an (A, n) array of A = %d chunks, got shape %s" % (A, tuple(chunks.shape)))
            n = int(chunks.shape[1])
            if lengths is None:
                lens = np.full(A, n, np.int64)
            else:
                if hasattr(lengths, "is_cuda") and lengths.is_cuda:
                    raise ValueError("lengths must be host values: the carry bookkeeping reads nothing back from the device")
                lens = np.asarray(lengths).reshape(-1)
                if lens.dtype.kind not in "iu" or lens.size != A:
                    raise ValueError("lengths must give one integer sample count per chunk")
                lens = lens.astype(np.int64)
                if lens.size and lens.max() > n:
                    raise ValueError("a length of %d exceeds the %d samples per row of chunks" % (lens.max(), n))
            return chunks, lens
        if lengths is not None:
            raise ValueError("lengths goes with a padded (A, n) array; a list of chunks carries its own")
        if len(chunks) != A:
            raise ValueError("%d slots for %d chunks" % (A, len(chunks)))
        rows = []
        for c in chunks:
            c = _pcm(c)
            if c.ndim != 1:
                raise ValueError("a chunk is a 1-D array of samples")
            rows.append(c)
        return rows, np.array([c.size for c in rows], np.int64)

    def push(self, slots, lengths):
        """Checks the push, advances the mirror and -> its `RaggedStep`."""
        s, n = self.check(slots, lengths)
        which = self.bank_index[s] if self.banks else None
        if which is None or not which.any():
            return self._advance(s, n)
        # some slot arrives at a rate of its own: every entry goes through kws_rate_convert (banks[0] passes the others through), which
        # packs the rows of those that emit a sample; only they reach the detector
        from .rate import rate_table
        conv = which > 0
        fresh = conv & self.rate_reset[s]
        going = conv & ~fresh
        before, first_out = np.where(going, self.received[s], 0), np.where(going, self.sent[s], 0)
        p, q, k = self._pqk[0][s], self._pqk[1][s], self._pqk[2][s]
        after = before + n
        sent = np.where(after <= k, 0, -((-(after - k) * q) // p))               # M(N + len); the pass-through's is len
        emitted = sent - first_out
        kept = np.flatnonzero(emitted > 0)
        out_row = np.full(s.size, -1, np.int64)
        out_row[kept] = np.arange(kept.size)
        row = 2 * s + self.parity[s]
        rate = rate_table(which, np.arange(s.size), n, before, out_row, first_out, emitted, np.where(conv, row, -1),
                          np.where(conv, row ^ 1, -1), np.where(fresh, _l.RATE_RESTART, 0))
        c = s[conv]
        self.received[c], self.sent[c], self.rate_reset[c] = after[conv], sent[conv], False
        self.parity[c] ^= 1
        step = self._advance(s[kept], emitted[kept])
        step.rate, step.emitted, step.entries = rate, emitted, kept
        return step

    def _advance(self, s, n):
        """The carry arithmetic of listen.py:96-105 for chunks of n samples at the detector's rate in the slots s"""
        W, H = self.window_samples, self.hop_samples
        reset = self.reset[s]
        carry = np.where(reset, 0, self.carry[s])
        first = np.where(reset, 0, self.position[s])
        L = carry + n
        n_new = np.where(L < W, 0, (L - W) // H + 1)                           # listen.py:103-105
        used = n_new * H
        keep = np.maximum(L - used, 0)                                         # hop > window: the carry empties
        table = np.zeros((s.size, _l.RAGGED_FIELDS), np.int32)
        table[:, _l.RAGGED_SLOT], table[:, _l.RAGGED_CARRY], table[:, _l.RAGGED_LEN] = s, carry, n
        table[:, _l.RAGGED_NEW], table[:, _l.RAGGED_RESET] = n_new, reset
        self.carry[s], self.position[s], self.reset[s] = keep, first + np.minimum(used, L), False
        return RaggedStep(table, n_new, keep, first, H)


class StreamServer(_Streams):
    """S independent audio streams ("slots") that need NOT advance together, through update_vectors -> model -> decode -> trigger
    (listen.py:96-114, 350-375): a push names the slots that have a chunk, each chunk of its own length 1..chunk_size, and
    only those slots move; every slot has its own sensitivity and trigger level, and slots open and close while others run.
    The contract is the ragged-streaming block of include/kws.h.  `StreamBatch` is the lockstep form.

    open(sensitivity=None, trigger_level=None) -> slot (the lowest free one; its carry, window and detector restart with its
    next push); close(slot); push(slots, chunks, lengths=None) -> (index, score, fired), CUDA tensors of length A = len(slots)
    in the order given (views of buffers the next push overwrites).  Per slot: mfccs (S, F, D), state (S, 2), index, score,
    fired (S), sensitivity, trigger_level (S), win (S, >= cap) with each slot's carry in front; probs: the last compact (A, C).
    A push enqueues one table copy, the chunk copy, kws_stream_ragged_append, kws_featurize_long (unless no slot completes a
    row), kws_stream_ragged_push_rows, the forward pass and kws_stream_ragged_postprocess on the current stream; it reads
    nothing back and does not wait for the device.

    open(..., sample_rate=f) takes the slot's audio at f Hz instead of pr.sample_rate (kws_amd.rate.RateBank says which pairs are
    supported); its chunks may then hold up to plan.max_chunk[slot] = floor(chunk_size f / pr.sample_rate) samples.  A push that names
    such a slot enqueues kws_rate_convert in front of the append -- one more launch, and the push's audio goes to a buffer of its own
    first -- which converts with the state the slot keeps between pushes (the converter block of include/kws.h: the same samples
    however the stream is cut) and hands the rest of the push the converted chunks.  An entry whose chunk yields no converted sample
    (the first K input samples of a stream, a tiny chunk at 48 kHz) gets no prediction: its place in the returned tensors holds the
    slot's previous index and score with fired = 0, and probs has a row only for the entries that took part.  A push that names
    only slots at pr.sample_rate runs the sequence above unchanged.

    heads=bank (a kws_amd.transfer.HeadBank) gives every slot a keyword set of its own on the one backbone: open(..., head=h) names
    the bank's head the slot listens with (slot_head (S) int32 on the device, a stream-ordered fill like sensitivity), and the
    forward pass of a push becomes kws_model_embed over the A windows followed by kws_heads_apply, which finds each row's head through
    the push's own table (key = the table's slot column, head_of_key = slot_head): one more launch, still nothing read back.  probs is
    then (A, bank.max_classes), the columns past a head's own classes zero; bank.set replaces a head between two pushes."""

    def __init__(self, pr, device_model, n_slots, chunk_size=1024, class_names=None, sensitivity=0.5, trigger_level=3,
                 decoder=None, featurizer=None, background_index=0, quantized=None, heads=None):
        _Streams.__init__(self, pr, device_model, quantized, heads)
        torch = _torch()
        self.plan = RaggedPlan(n_slots, chunk_size, pr.window_samples, pr.hop_samples, sensitivity, trigger_level,
                               sample_rate=pr.sample_rate)
        self._hist = self._raw = self._rate_table = None                                  # made when a slot opens at a rate of its own
        self._allocate(self.plan.S, self.plan.chunk_size, class_names, decoder, featurizer, background_index)
        S, dev = self.S, device_model.device
        self._stride = (self.cap + 7) & ~7                                                # rows start on 16 bytes
        self._max_frames = self.chunk_size // self.hop_samples + 1                        # rows a full buffer of cap samples gives
        self.win = torch.zeros((S, self._stride), dtype=torch.int16, device=dev)
        self.sensitivity = torch.full((S,), float(sensitivity), dtype=torch.float64, device=dev)
        self.trigger_level = torch.full((S,), int(trigger_level), dtype=torch.int32, device=dev)
        # per-push work buffers, sized for a push that names every slot
        self._table = torch.zeros((S, _l.RAGGED_FIELDS), dtype=torch.int32, device=dev)
        self._chunks = torch.zeros((S, self._stride), dtype=torch.int16, device=dev)
        self._act = torch.zeros((S, self._stride), dtype=torch.int16, device=dev)
        self._act_len = torch.zeros(S, dtype=torch.int32, device=dev)
        self._rows = torch.zeros(S * self._max_frames * self.D, dtype=torch.float32, device=dev)
        self._feat = torch.zeros((S, self.F, self.D), dtype=torch.float32, device=dev)
        self._index = torch.zeros(S, dtype=torch.int32, device=dev)
        self._score = torch.zeros(S, dtype=torch.float64, device=dev)
        self._fired = torch.zeros(S, dtype=torch.int32, device=dev)
        self.slot_head = torch.zeros(S, dtype=torch.int32, device=dev)                    # the bank's head each slot listens with
        self.launches, self.featurizer_launches = 0, 0                                    # stages enqueued so far (a forward counts as one)

    def open(self, sensitivity=None, trigger_level=None, sample_rate=None, head=0):
        head = int(_head_ids(self.heads, [head], 1, "head")[0]) if self.heads is not None or head != 0 else 0
        slot = self.plan.open(sensitivity, trigger_level, sample_rate)
        if self.heads is not None:
            self.slot_head[slot] = head                                                   # a stream-ordered fill, as the two below
        if self.plan.bank[slot] is not None and self._hist is None:
            torch, dev = _torch(), self.win.device
            # two history rows per slot (one read, one written, by turns); 2K - 1 <= 8 Z - 1 samples for every supported pair at Z = 16
            self._hist = torch.zeros((2 * self.S, 128), dtype=torch.int16, device=dev)
            self._rate_table = torch.zeros((self.S, _l.RATE_FIELDS), dtype=torch.int32, device=dev)
            self._gather = torch.zeros((2, self.S), dtype=torch.int64, device=dev)
        self.sensitivity[slot] = float(self.plan.sensitivity[slot])                       # stream-ordered fills, nothing waits
        self.trigger_level[slot] = int(self.plan.trigger_level[slot])
        return slot

    def close(self, slot):
        self.plan.close(slot)

    def _stage_chunks(self, torch, rows, lens, raw=False):
        """-> (device pointer, row stride in samples) of the push's audio; raw: (the (A, stride) device tensor) of audio that is still
        to be converted, in a buffer of its own that grows with the longest push"""
        A = len(lens)
        if hasattr(rows, "is_cuda"):
            if rows.is_cuda:
                t = rows.contiguous()                                                     # read in place, stream-ordered
                return t if raw else (t.data_ptr(), int(t.shape[1]))
            rows = rows.numpy()
        width = (int(lens.max()) + 7) & ~7
        if raw and (self._raw is None or self._raw.numel() < A * width):
            self._raw = torch.empty(A * width, dtype=torch.int16, device=self.win.device)
        pinned = torch.empty((A, width), dtype=torch.int16, pin_memory=True)
        host = pinned.numpy()
        if isinstance(rows, np.ndarray):
            n = min(width, rows.shape[1])
            host[:, :n] = rows[:, :n]
        else:
            for a, c in enumerate(rows):
                host[a, :c.size] = c
        d = (self._raw if raw else self._chunks.view(-1))[:A * width].view(A, width)
        d.copy_(pinned, non_blocking=True)
        return d if raw else (d.data_ptr(), width)

    def push(self, slots, chunks, lengths=None):
        """One chunk for each of the A distinct open `slots` (any order).  chunks: a list of A `bytes` objects or 1-D int16
        arrays of their own lengths, or an (A, n) int16 array / CUDA tensor with optional host `lengths`.  ValueError for a
        duplicate, closed or out-of-range slot, an empty chunk, one longer than chunk_size, or audio that is not int16."""
        slots = list(slots) if not isinstance(slots, np.ndarray) else slots
        rows, lens = self.plan.chunks(slots, chunks, lengths)
        self.plan.check(slots, lens)                                                      # before torch is touched
        torch = _torch()
        A = len(lens)
        if A == 0:
            self.probs = torch.empty((0, _num_classes(self.model, self.quantized, self.heads)), dtype=torch.float32, device=self.win.device)
            return self._index[:0], self._score[:0], self._fired[:0]
        step = self.plan.push(slots, lens)
        if step.rate is not None:
            return self._push_converted(torch, step, slots, rows, lens)
        self._detect(torch, step, lambda: self._stage_chunks(torch, rows, lens))
        return self._index[:A], self._score[:A], self._fired[:A]

    def _push_converted(self, torch, step, slots, rows, lens):
        """A push that names a slot at a rate of its own: kws_rate_convert turns every entry's audio into the detector's (the slots
        already at its rate pass through bit for bit) and packs the rows of those that emit a sample into the buffer
        kws_stream_ragged_append reads; the rest of the push runs on them alone."""
        from .rate import launch
        A, kept = len(lens), step.entries
        pinned = torch.empty((A, _l.RATE_FIELDS), dtype=torch.int32, pin_memory=True)
        pinned.numpy()[:] = step.rate
        self._rate_table[:A].copy_(pinned, non_blocking=True)
        raw = self._stage_chunks(torch, rows, lens, raw=True)
        launch(self.plan.banks, raw, self._rate_table, A, out_i16=self._chunks, out_width=int(step.emitted.max()), hist=self._hist)
        self.launches += 1
        if kept.size:
            self._detect(torch, step, lambda: (self._chunks.data_ptr(), self._stride))
        else:
            self.probs = torch.empty((0, _num_classes(self.model, self.quantized, self.heads)), dtype=torch.float32, device=self.win.device)
        if kept.size == A:
            return self._index[:A], self._score[:A], self._fired[:A]
        # an entry that emitted nothing was not predicted on: its place holds the slot's previous index and score, fired = 0
        pinned = torch.empty((2, A), dtype=torch.int64, pin_memory=True)
        pinned.numpy()[0], pinned.numpy()[1] = np.asarray(slots, np.int64), step.emitted > 0
        g = self._gather.view(-1)[:2 * A].view(2, A)
        g.copy_(pinned, non_blocking=True)
        return (self.index.index_select(0, g[0]), self.score.index_select(0, g[0]),
                (self.fired.index_select(0, g[0]) * g[1]).to(torch.int32))

    def _detect(self, torch, step, stage):
        """The push from its ragged table on, for the step's A entries; stage() -> (device pointer, row stride) of their audio"""
        A = step.A
        pinned = torch.empty((A, _l.RAGGED_FIELDS), dtype=torch.int32, pin_memory=True)
        pinned.numpy()[:] = step.table
        table = self._table[:A]
        table.copy_(pinned, non_blocking=True)
        src, src_stride = stage()
        L, st, mf = self._L, _stream(), step.max_frames
        _l.check(L.kws_stream_ragged_append(self.win.data_ptr(), self._stride, self.S, self.cap, src, src_stride, table.data_ptr(), A,
                                            self.chunk_size, self.window_samples, self.hop_samples, self._act.data_ptr(), self._stride,
                                            self._act_len.data_ptr(), st))
        if mf > 0:
            if mf > self._max_frames:
                raise RuntimeError("a push of %d rows per slot exceeds the %d the buffers hold" % (mf, self._max_frames))
            _l.check(L.kws_featurize_long(self.featurizer._h, self._act.data_ptr(), _l.WAV_I16, A, self._stride, self._act_len.data_ptr(), mf,
                                          self._rows.data_ptr(), st))
        feat = self._feat[:A]
        _l.check(L.kws_stream_ragged_push_rows(self.mfccs.data_ptr(), self.S, self.F, self.D, self._rows.data_ptr(), mf, table.data_ptr(), A,
                                               feat.data_ptr(), st))
        # with a bank, a row's head is slot_head[its slot], found through the push's own table
        key = None if self.heads is None else (table.view(-1)[_l.RAGGED_SLOT:], _l.RAGGED_FIELDS, self.slot_head)
        self.probs = _forward(self.model, self.quantized, feat, self.heads, key)
        _l.check(L.kws_stream_ragged_postprocess(self.decoder.handle, self.probs.data_ptr(), A, self.probs.shape[1], table.data_ptr(), self.S,
                                                 self.background_index, self.sensitivity.data_ptr(), self.trigger_level.data_ptr(),
                                                 self.chunk_size, self.state.data_ptr(), self.index.data_ptr(), self.score.data_ptr(),
                                                 self.fired.data_ptr(), self._index.data_ptr(), self._score.data_ptr(),
                                                 self._fired.data_ptr(), st))
        self.launches += 4 + (mf > 0) + (self.heads is not None)
        self.featurizer_launches += mf > 0


def scan_plan(n_samples, chunk_size, window_samples, hop_samples, n_features):
    """What the chunk loop (`StreamBatch.push` once per chunk, listen.py:96-114) does to a recording of `n_samples` samples,
    in closed form.  Returns (T, n, r, first):
      T        number of chunks, ceil(N / chunk_size) (the last one may be short, as wave.readframes delivers it);
      n[k-1]   samples that have arrived after chunk k = 1..T: min(k * chunk_size, N);
      r[k-1]   feature rows that exist after chunk k: with hop <= window the carry buffer always starts on a frame boundary, so
               0 if n < window else (n - window) // hop + 1, row j being vectorize_raw of samples [j*hop, j*hop + window);
      first[k-1]  index of the first row of the matrix the model sees at chunk k, r - n_features: the matrix is rows
               [first, r), all-zero rows standing for the negative indices (listen.py:92).
    Precondition: hop_samples <= window_samples.  With a larger hop a push can consume more samples than the carry buffer holds; the
    loop then empties the buffer (listen.py:105) and its next frame starts with the next chunk, wherever that falls, so its rows
    depend on the chunk size and no closed form over the recording gives them: ValueError.
    Pure Python, no device: the kernels behind `scan` compute the same numbers (csrc/kws_stream.hip)."""
    N, c, W, H, F = int(n_samples), int(chunk_size), int(window_samples), int(hop_samples), int(n_features)
    if N < 0 or c < 1 or W < 1 or H < 1 or F < 1:
        raise ValueError("scan_plan needs n_samples >= 0 and positive chunk_size / window / hop / n_features")
    _check_hop(W, H)
    T = -(-N // c)
    n = [min(k * c, N) for k in range(1, T + 1)]
    r = [0 if v < W else (v - W) // H + 1 for v in n]
    return T, n, r, [v - F for v in r]


def _check_hop(window_samples, hop_samples):
    if hop_samples > window_samples:
        raise ValueError("hop_samples=%d > window_samples=%d: the chunk loop's frames then start wherever a chunk does, not on multiples "
                         "of the hop, and the scan's closed form does not hold; run the chunk loop (StreamBatch.push)"
                         % (hop_samples, window_samples))


class ScanResult(object):
    """index / score / fired: (R, T_max) CUDA tensors, element (r, k) for chunk k of recording r (index -1, score 0,
    fired 0 past the recording's own n_chunks[r]); n_chunks: list of R ints; state: (R, 2) int32 CUDA tensor, the
    detector state {activation, record_index} after each recording's last chunk; probs: (R, T_max, C) or None.  With
    scan(..., keep_audio=True) also wav, the packed (R, stride) int16 CUDA tensor the scan read, and lengths, the host list of
    sample counts (both None otherwise): `Detections.clips` / `.save` then need no recordings."""

    def __init__(self, index, score, fired, n_chunks, state, probs=None, wav=None, lengths=None):
        self.index, self.score, self.fired, self.n_chunks, self.state, self.probs = index, score, fired, n_chunks, state, probs
        self.wav, self.lengths = wav, lengths

    def __iter__(self):
        return iter((self.index, self.score, self.fired, self.n_chunks, self.state))

    def sweep(self, sensitivities, trigger_levels, chunk_size, **kwargs):
        """`sweep` of this scan: the detector at every (sensitivity, trigger_level) of the grid, from the scores decoded once."""
        return sweep(self, sensitivities, trigger_levels, chunk_size, **kwargs)


def _pack_recordings(torch, recordings, lengths, device):
    """-> ((R, stride) int16 CUDA tensor, host list of lengths)"""
    if isinstance(recordings, torch.Tensor) or (isinstance(recordings, np.ndarray) and recordings.ndim == 2):
        t = recordings if isinstance(recordings, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(recordings))
        if t.dim() != 2 or t.dtype != torch.int16:
            raise ValueError("recordings must be int16 PCM of shape (R, n) (the 1/32768 scaling happens on the device)")
        if lengths is None:
            lens = [int(t.shape[1])] * int(t.shape[0])
        else:
            lens = [int(v) for v in (lengths.cpu().tolist() if isinstance(lengths, torch.Tensor) else np.asarray(lengths).tolist())]
        if len(lens) != t.shape[0] or any(v < 0 or v > t.shape[1] for v in lens):
            raise ValueError("lengths must give one sample count in 0..%d per recording" % t.shape[1])
        return t.to(device, non_blocking=True).contiguous(), lens
    if lengths is not None:
        raise ValueError("lengths goes with a padded (R, n) array; a list of recordings carries its own")
    arrs = [np.asarray(a) for a in recordings]
    if any(a.ndim != 1 or a.dtype != np.int16 for a in arrs):
        raise ValueError("recordings must be 1-D int16 PCM arrays (the 1/32768 scaling happens on the device)")
    lens = [int(a.size) for a in arrs]
    stride = max(2, (max(lens + [0]) + 1) & ~1)                # even rows: aligned two-sample loads for every recording
    host = np.zeros((len(arrs), stride), np.int16)
    for i, a in enumerate(arrs):
        host[i, :a.size] = a
    return torch.from_numpy(host).to(device, non_blocking=True), lens


def scan(pr, device_model, recordings, lengths=None, chunk_size=1024, class_names=None, sensitivity=0.5, trigger_level=3,
         decoder=None, featurizer=None, background_index=0, quantized=None, tile=4096, return_probs=False, timings=None,
         keep_audio=False, sample_rates=None, heads=None, recording_heads=None):
    """The chunk loop of `StreamBatch` over R whole recordings at once: for every chunk of every recording the (index,
    score, fired) that `push` would have returned for it, and the final detector state, as a `ScanResult`.

    recordings: a list of 1-D int16 arrays, or a padded (R, n) int16 array / CUDA tensor with `lengths`.  The rows of every
    recording come from one kws_featurize_long launch; then, `tile` windows at a time (all recordings advance together,
    tile // R chunks each), kws_stream_gather_windows -> the model's (or `quantized`'s) forward ->
    kws_stream_scan_postprocess, which carries the detector state from tile to tile.  Everything is enqueued on the
    current stream; the host does not wait for the device.  `timings`: an optional dict that receives lists of
    (start, end) CUDA event pairs per stage ("rows", "gather", "forward", "scan") for tools/scanbench.py.  keep_audio: the
    result keeps the packed int16 tensor and the lengths built here (`ScanResult.wav`, `.lengths`).  sample_rates: the rate of the
    recordings in Hz, one for all or one each; those not at pr.sample_rate are first converted to it by one kws_amd.rate.convert
    call, and chunks, lengths, events and times are then in converted samples (None: all are at pr.sample_rate).  heads (a
    kws_amd.transfer.HeadBank) with recording_heads, one head id per recording (default 0): every window of recording r goes through
    device_model's backbone and then through that head (kws_heads_apply); probs are (R, T_max, heads.max_classes)."""
    torch = _torch()
    if pr.use_delta:
        raise ValueError(_NO_DELTAS)
    _check_heads(device_model, quantized, heads)
    if class_names is not None:
        assert class_names[0] == 'background', '1st class should be background.'          # listen.py:66
    _check_hop(pr.window_samples, pr.hop_samples)
    L = _l.get_lib()
    chunk_size, tile = int(chunk_size), int(tile)
    if chunk_size < 1 or tile < 1:
        raise ValueError("chunk_size and tile must be positive")
    dev = device_model.device
    featurizer, decoder = _defaults(pr, featurizer, decoder)
    W, H, F, D = pr.window_samples, pr.hop_samples, pr.n_features, pr.n_mfcc
    if sample_rates is not None and np.any(np.asarray(sample_rates) != pr.sample_rate):
        from .rate import convert
        recordings, lengths = convert(recordings, sample_rates, pr.sample_rate, lengths=lengths, device=dev)
    wav, lens = _pack_recordings(torch, recordings, lengths, dev)
    R = len(lens)
    n_chunks = [-(-n // chunk_size) for n in lens]
    T_max = max(n_chunks + [0])
    C = _num_classes(device_model, quantized, heads)
    rec_heads = _head_ids(heads, recording_heads, R, "recording_heads")
    index = torch.empty((R, T_max), dtype=torch.int32, device=dev)
    score = torch.empty((R, T_max), dtype=torch.float64, device=dev)
    fired = torch.empty((R, T_max), dtype=torch.int32, device=dev)
    probs_all = torch.empty((R, T_max, C), dtype=torch.float32, device=dev) if return_probs else None
    state = torch.zeros((R, 2), dtype=torch.int32, device=dev)
    state[:, 1] = -1
    kept = (wav, lens) if keep_audio else (None, None)
    if R == 0 or T_max == 0:
        return ScanResult(index, score, fired, n_chunks, state, probs_all, *kept)
    st = _stream()

    def timed(name, fn):
        if timings is None:
            return fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        timings.setdefault(name, []).append((a, b))
        return out

    d_len = torch.tensor(lens, dtype=torch.int32).to(dev, non_blocking=True)
    d_chunks = torch.tensor(n_chunks, dtype=torch.int32).to(dev, non_blocking=True)
    max_frames = max(0 if n < W else (n - W) // H + 1 for n in lens)
    rows = torch.empty((R, max(max_frames, 1), D), dtype=torch.float32, device=dev)
    timed("rows", lambda: _l.check(L.kws_featurize_long(featurizer._h, wav.data_ptr(), _l.WAV_I16, R, wav.shape[1], d_len.data_ptr(),
                                                          max_frames, rows.data_ptr(), st)))
    per = max(1, tile // R)                                   # chunks of every recording per tile
    d_heads = None if heads is None else torch.from_numpy(rec_heads).to(dev, non_blocking=True)
    feat = torch.empty((R * min(per, T_max), F, D), dtype=torch.float32, device=dev)
    for k0 in range(0, T_max, per):
        n = min(per, T_max - k0)
        fv = feat[:R * n]
        timed("gather", lambda: _l.check(L.kws_stream_gather_windows(rows.data_ptr(), R, max_frames, d_len.data_ptr(), chunk_size, W, H, F, D,
                                                                       k0, n, fv.data_ptr(), st)))
        # window (r, k) of the tile is row r * n + k: its head is its recording's
        key = None if heads is None else (torch.repeat_interleave(d_heads, n, output_size=R * n), 1, None)
        probs = timed("forward", lambda: _forward(device_model, quantized, fv, heads, key))
        off = k0 * 4
        timed("scan", lambda: _l.check(L.kws_stream_scan_postprocess(decoder.handle, probs.data_ptr(), R, n, C, d_chunks.data_ptr(), k0,
                                                                       int(background_index), float(sensitivity), int(trigger_level), chunk_size,
                                                                       state.data_ptr(), index.data_ptr() + off, score.data_ptr() + 2 * off,
                                                                       fired.data_ptr() + off, T_max, st)))
        if return_probs:
            probs_all[:, k0:k0 + n] = probs.view(R, n, C)
    return ScanResult(index, score, fired, n_chunks, state, probs_all, *kept)


def events_to_chunks(events, n_samples, chunk_size, tolerance_samples, background_index=0, num_classes=None):
    """Labelled events in samples -> the chunk ranges in which a detection counts for them.  Pure Python, no device.

    events: per recording a list of (class_index, start_sample, end_sample) with 0 <= start < end; n_samples: per recording
    its sample count N.  An event becomes (class_index, lo, hi) with lo = start // chunk_size and
    hi = min(T - 1, (end - 1 + tolerance_samples) // chunk_size), T = ceil(N / chunk_size): the detector may fire from the
    chunk in which the keyword starts until `tolerance_samples` after its last sample, for as long as the keyword is still
    inside the model's buffer.  Returns per recording the list sorted by lo.  Raises ValueError, naming the recording, for
    an event that starts at or after the recording's end, a class that is the background or outside 0 .. num_classes - 1,
    and events whose chunk ranges overlap (lo[e + 1] <= hi[e]): kws_stream_sweep gives every fire to one event at most."""
    c, tol = int(chunk_size), int(tolerance_samples)
    if c < 1 or tol < 0:
        raise ValueError("events_to_chunks needs a positive chunk_size and tolerance_samples >= 0")
    if len(events) != len(n_samples):
        raise ValueError("%d event lists for %d recordings" % (len(events), len(n_samples)))
    out = []
    for r, (evs, N) in enumerate(zip(events, n_samples)):
        N = int(N)
        T = -(-N // c)
        rows = []
        for cls, start, end in evs:
            cls, start, end = int(cls), int(start), int(end)
            if not 0 <= start < end:
                raise ValueError("recording %d: event (%d, %d, %d) needs 0 <= start < end" % (r, cls, start, end))
            if start >= N:
                raise ValueError("recording %d: event (%d, %d, %d) starts at or after the recording's end (%d samples)" % (r, cls, start, end, N))
            if cls == background_index or cls < 0 or (num_classes is not None and cls >= int(num_classes)):
                raise ValueError("recording %d: event (%d, %d, %d) has the background's class or one outside the model's" % (r, cls, start, end))
            rows.append((cls, start // c, min(T - 1, (end - 1 + tol) // c)))
        rows.sort(key=lambda v: v[1])
        for a, b in zip(rows, rows[1:]):
            if b[1] <= a[2]:
                raise ValueError("recording %d: the chunk ranges %d..%d and %d..%d of two events overlap" % (r, a[1], a[2], b[1], b[2]))
        out.append(rows)
    return out


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


class SweepResult(object):
    """What `sweep` counted.  fires / hits / false_alarms / duplicates / latency_chunks: (R, S, L) int32 tensors, element
    (r, s, l) for recording r at sensitivities[s] and trigger_levels[l]; latency_chunks is the sum over the hits of
    (chunk of the fire - first chunk of the event).  n_events: list of R ints; seconds: per-recording durations or None."""

    def __init__(self, fires, hits, false_alarms, duplicates, latency_chunks, n_events, sensitivities, trigger_levels, seconds=None):
        self.fires, self.hits, self.false_alarms, self.duplicates, self.latency_chunks = fires, hits, false_alarms, duplicates, latency_chunks
        self.n_events = [int(v) for v in n_events]
        self.sensitivities = [float(v) for v in sensitivities]
        self.trigger_levels = [int(v) for v in trigger_levels]
        self.seconds = seconds

    def det(self, seconds=None):
        """(miss_rate, fa_per_hour): host (S, L) float64 arrays over all recordings, miss_rate = 1 - sum(hits) / sum(n_events)
        and fa_per_hour = sum(false_alarms) * 3600 / sum(seconds); NaN where the denominator is 0."""
        seconds = self.seconds if seconds is None else seconds
        if seconds is None:
            raise ValueError("det needs the recordings' durations in seconds")
        S, L = len(self.sensitivities), len(self.trigger_levels)
        hits = _host(self.hits).astype(np.int64).reshape(-1, S, L).sum(axis=0)
        fas = _host(self.false_alarms).astype(np.int64).reshape(-1, S, L).sum(axis=0)
        n_ev, total_s = sum(self.n_events), float(np.sum(np.asarray(seconds, dtype=np.float64)))
        nan = np.full((S, L), np.nan)
        miss = 1.0 - hits / float(n_ev) if n_ev > 0 else nan
        fa = fas * 3600.0 / total_s if total_s > 0 else nan.copy()
        return miss, fa

    def best(self, seconds=None, max_fa_per_hour=0.0):
        """The operating point to ship: among the points with fa_per_hour <= max_fa_per_hour the one with the lowest miss
        rate; ties go to the lower fa_per_hour, then the higher sensitivity, then the lower trigger level.  Returns a dict
        (s, l, sensitivity, trigger_level, miss_rate, fa_per_hour) or None when no point qualifies.  Without events every
        miss rate is NaN and the tie-breaks alone decide."""
        miss, fa = self.det(seconds)
        pick = None
        for s, sens in enumerate(self.sensitivities):
            for l, level in enumerate(self.trigger_levels):
                if not fa[s, l] <= max_fa_per_hour:                  # NaN does not qualify
                    continue
                m = float(miss[s, l])
                key = (float("inf") if m != m else m, float(fa[s, l]), -sens, level)
                if pick is None or key < pick[0]:
                    pick = (key, {"s": s, "l": l, "sensitivity": sens, "trigger_level": level, "miss_rate": m, "fa_per_hour": float(fa[s, l])})
        return None if pick is None else pick[1]


def sweep(result, sensitivities, trigger_levels, chunk_size, events=None, lengths=None, tolerance_samples=None, background_index=0,
          pr=None):
    """The trigger detector over scanned recordings at every point of the grid sensitivities x trigger_levels (sensitivity
    the major axis) in one kws_stream_sweep launch: the scan's argmax and decoded scores do not depend on the operating
    point, so they are computed once and only TriggerDetector.update is walked again, 64 points per wave.

    result: a `ScanResult`, or (index, score, n_chunks) with (R, stride) int32 / float64 CUDA tensors as `scan` writes
    them.  events: per recording a list of (class_index, start_sample, end_sample), converted by `events_to_chunks` with
    `lengths` (sample counts; default n_chunks * chunk_size) and `tolerance_samples` (default pr.max_samples: the keyword
    stays inside the model's buffer for that long after it ends); None counts fires only.  The decoder is the scan's.
    Returns a `SweepResult`; nothing is synchronised."""
    torch = _torch()
    chunk_size = int(chunk_size)
    scanned = _Scanned(result, chunk_size, events, lengths, tolerance_samples, background_index, pr)
    sens = [float(v) for v in sensitivities]
    levels = [int(v) for v in trigger_levels]
    S, L = len(sens), len(levels)
    R, P, dev = scanned.R, S * L, scanned.index.device
    counts = torch.zeros((R, P, 5), dtype=torch.int32, device=dev)
    if R > 0 and P > 0:
        d_sens = torch.tensor(np.repeat(sens, L), dtype=torch.float64).to(dev)
        d_level = torch.tensor(np.tile(levels, S), dtype=torch.int32).to(dev)
        ev = scanned.ev
        _l.check(_l.get_lib().kws_stream_sweep(scanned.index.data_ptr(), scanned.score.data_ptr(), R, scanned.stride,
                                               scanned.d_chunks.data_ptr(), int(background_index), chunk_size, d_sens.data_ptr(),
                                               d_level.data_ptr(), P, ev[0], ev[1], ev[2], ev[3], counts.data_ptr(), _stream()))
    f = counts.permute(2, 0, 1).contiguous().view(5, R, S, L)
    n_events = [0] * R if scanned.rows is None else [len(v) for v in scanned.rows]
    return SweepResult(f[0], f[1], f[2], f[3], f[4], n_events, sens, levels)


class _Scanned(object):
    """The opening steps of `sweep`, `collect` and `peaks`: a scan's arrays and the labelled events, checked and on the device.
    Every check runs on host data alone, the CUDA check last; only then is anything enqueued.

    index, score: the scan's (R, stride) tensors, contiguous; n_chunks: host list, d_chunks: its int32 device copy; rows: per
    recording the events as [(class, lo, hi), ...] in chunk units, None without labels; ev: the device pointers ev_off, ev_class,
    ev_lo, ev_hi (a CSR over the recordings; this object keeps their tensors alive), four NULLs without labels; audio: the (packed
    int16 tensor, lengths) a scan made with keep_audio kept, else None."""

    def __init__(self, result, chunk_size, events, lengths, tolerance_samples, background_index, pr):
        import torch
        self.audio = None
        if isinstance(result, ScanResult):
            index, score, n_chunks = result.index, result.score, result.n_chunks
            if result.wav is not None:
                self.audio = (result.wav, result.lengths)
        else:
            index, score, n_chunks = result
        if chunk_size < 1:
            raise ValueError("chunk_size must be positive")
        unfit = "index / score must be (R, stride) int32 / float64 CUDA tensors of one shape"
        if not (isinstance(index, torch.Tensor) and isinstance(score, torch.Tensor) and index.dtype == torch.int32
                and score.dtype == torch.float64 and index.dim() == 2 and index.shape == score.shape):
            raise ValueError(unfit)
        self.n_chunks = [int(v) for v in n_chunks]
        self.R, self.stride = int(index.shape[0]), int(index.shape[1])
        if len(self.n_chunks) != self.R or any(v < 0 or v > self.stride for v in self.n_chunks):
            raise ValueError("n_chunks must give one chunk count in 0..%d per recording" % self.stride)
        self.rows = None
        if events is not None:
            self.rows = _event_rows(events, self.n_chunks, chunk_size, lengths, tolerance_samples, background_index, pr)
        if not (index.is_cuda and score.is_cuda):                  # the last of the checks: every other one has passed on host data
            raise ValueError(unfit)
        dev = index.device
        self.index, self.score = index.contiguous(), score.contiguous()
        self.d_chunks = torch.tensor(self.n_chunks, dtype=torch.int32).to(dev)
        self._keep = [] if self.rows is None else _event_tensors(torch, self.rows, dev)
        self.ev = [t.data_ptr() for t in self._keep] or [0, 0, 0, 0]


def _event_rows(events, n_chunks, chunk_size, lengths, tolerance_samples, background_index, pr):
    """`sweep`'s handling of labelled events -> per recording [(class, lo, hi), ...] in chunk units.  Pure Python."""
    if tolerance_samples is None:
        if pr is None:
            from classifier.params import pr
        tolerance_samples = pr.max_samples
    lens = [n * chunk_size for n in n_chunks] if lengths is None else [int(v) for v in _host(lengths).tolist()]
    if [-(-n // chunk_size) for n in lens] != n_chunks:
        raise ValueError("lengths do not give the scan's chunk counts at chunk_size=%d" % chunk_size)
    return events_to_chunks(events, lens, chunk_size, tolerance_samples, background_index)


def _event_tensors(torch, rows, dev):
    """-> [ev_off, ev_class, ev_lo, ev_hi] device tensors (CSR over the recordings)"""
    off = np.concatenate(([0], np.cumsum([len(v) for v in rows]))).astype(np.int32)
    flat = np.array([e for v in rows for e in v] or [(0, 0, 0)], dtype=np.int32).reshape(-1, 3)
    return [torch.from_numpy(off).to(dev)] + [torch.from_numpy(np.ascontiguousarray(flat[:, i])).to(dev) for i in range(3)]


class Detections(object):
    """Chunks of scanned recordings worth keeping: the activations `collect` found, or the near misses of `peaks`.

    n: host list, per recording the number found (for `collect` also when a given max_det stored fewer: n_stored).
    recording / chunk / cls / kind / event (int32) and score (float64): CUDA tensors with one entry per stored detection,
    flattened recording by recording -- in chunk order for `collect`, in pick order (best first) for `peaks`.  kind is one of
    kws_amd.lib.DET_UNLABELLED / DET_HIT / DET_DUPLICATE / DET_FALSE_ALARM; event is the position of the matched event within
    its recording's (sorted) events, or -1."""

    def __init__(self, n, recording, chunk, cls, kind, event, score, chunk_size, n_stored=None, audio=None):
        self.n = [int(v) for v in n]
        self.n_stored = self.n if n_stored is None else [int(v) for v in n_stored]
        self.recording, self.chunk, self.cls, self.kind, self.event, self.score = recording, chunk, cls, kind, event, score
        self.chunk_size = int(chunk_size)
        self._audio = audio                                        # (packed int16 tensor, lengths) of a scan made with keep_audio

    def __len__(self):
        return int(self.chunk.shape[0])

    def select(self, kind=None):
        """The detections of one kind, or of any of several (an int or an iterable of ints; None keeps all), in the same
        order.  Reads the mask back to count per recording (one synchronisation)."""
        torch = _torch()
        if kind is None:
            return self
        kinds = [int(kind)] if isinstance(kind, (int, np.integer)) else [int(v) for v in kind]
        mask = torch.zeros_like(self.kind, dtype=torch.bool)
        for v in kinds:
            mask |= self.kind == v
        n = torch.bincount(self.recording[mask].to(torch.int64), minlength=len(self.n)).cpu().tolist() if len(self.n) else []
        return Detections(n, self.recording[mask], self.chunk[mask], self.cls[mask], self.kind[mask], self.event[mask], self.score[mask],
                          self.chunk_size, audio=self._audio)

    def times(self, chunk_size=None, sample_rate=None):
        """float64 CUDA tensor: seconds from the start of the recording to the first sample of each detection's chunk"""
        if sample_rate is None:
            from classifier.params import pr
            sample_rate = pr.sample_rate
        torch = _torch()
        c = self.chunk_size if chunk_size is None else int(chunk_size)
        first = (self.chunk.to(torch.int64) * c).to(torch.float64)
        # a tensor divisor: dividing by a Python scalar multiplies by its reciprocal on the device, one ulp off k * c / rate
        return first / torch.full_like(first, float(sample_rate))

    def clips(self, recordings=None, lengths=None, pr=None):
        """(len(self), pr.buffer_samples) float32 CUDA tensor: clip i is the listener's audio_buffer right after its chunk k
        (listen.py:90,100) -- samples [n_k - B, n_k) of its recording with n_k = min((k + 1) * chunk_size, N), scaled by
        1/32768, zeros in front where n_k < B.  It feeds `Featurizer` and raw-audio training as it is.  recordings: what `scan`
        takes (with `lengths` for a padded array); None uses the audio a scan(..., keep_audio=True) kept.  The triples are
        built with torch on the device and cut by kws_vad_gather_clips; nothing is synchronised."""
        torch = _torch()
        if pr is None:
            from classifier.params import pr
        B = int(pr.buffer_samples)
        if recordings is None:
            if self._audio is None:
                raise ValueError("clips needs the recordings, or detections of a scan made with keep_audio=True")
            wav, lens = self._audio
        else:
            wav, lens = _pack_recordings(torch, recordings, lengths, self.chunk.device)
        if len(lens) != len(self.n):
            raise ValueError("%d recordings for detections of %d" % (len(lens), len(self.n)))
        dev = wav.device
        n = len(self)
        out = torch.empty((n, B), dtype=torch.float32, device=dev)
        if n == 0:
            return out
        d_len = torch.tensor(lens, dtype=torch.int32).to(dev)
        rec = self.recording.to(torch.int64)
        end = torch.minimum((self.chunk.to(torch.int64) + 1) * self.chunk_size, d_len.to(torch.int64)[rec])
        tri = torch.stack([rec, torch.clamp(end - B, min=0), end], dim=1).to(torch.int32).contiguous()
        _l.check(_l.get_lib().kws_vad_gather_clips(wav.data_ptr(), _l.WAV_I16, int(wav.shape[0]), int(wav.shape[1]), d_len.data_ptr(),
                                                  tri.data_ptr(), n, B, 0, 0, _l.VAD_ALIGN["left"], out.data_ptr(), _stream()))
        return out

    def save(self, recordings, save_dir, class_names, names=None, session_id=None, pr=None, lengths=None, record_start=0):
        """Writes every detection's clip as <save_dir>/<class_names[cls]>/<session_id>_<record_num>.wav, the layout of the
        reference's Listener.on_activation (listen.py:299-308; record_num counts from record_start, session_id defaults to nine
        random digits as in listen.py:94), or, with `names` (one stem per recording), <stem>_<chunk>.wav.  16-bit mono at
        pr.sample_rate with the samples of the reference's save_audio, (audio * 32767).astype(int16) of the float64 buffer:
        truncated toward zero, not a copy of the PCM.  -> the list of paths, in detection order."""
        import os
        import wave
        from random import randint
        torch = _torch()
        if pr is None:
            from classifier.params import pr
        if pr.sample_depth != 2:
            raise ValueError("only 16-bit sample depth is supported")               # data_utils.py:44
        if names is not None and len(names) != len(self.n):
            raise ValueError("%d names for %d recordings" % (len(names), len(self.n)))
        if session_id is None:
            session_id = '%09d' % randint(0, 999999999)
        clips = self.clips(recordings, lengths=lengths, pr=pr)
        pcm = (clips.to(torch.float64) * 32767).to(torch.int16).cpu().numpy()    # float -> int conversion truncates toward zero
        rec, chunk, cls = self.recording.cpu().tolist(), self.chunk.cpu().tolist(), self.cls.cpu().tolist()
        paths = []
        for i in range(len(rec)):
            folder = os.path.join(save_dir, class_names[cls[i]])
            os.makedirs(folder, exist_ok=True)
            stem = '%s_%d' % (session_id, record_start + i) if names is None else '%s_%d' % (names[rec[i]], chunk[i])
            paths.append(os.path.join(folder, stem + '.wav'))
            wf = wave.open(paths[-1], 'wb')
            wf.setnchannels(1)
            wf.setsampwidth(pr.sample_depth)
            wf.setframerate(pr.sample_rate)
            wf.writeframes(pcm[i].astype('<i2').tobytes())
            wf.close()
        return paths


def _flatten(torch, counts, fields, score):
    """(R, cap, F) records and (R, cap) scores with counts (R) valid ones per recording -> (records, recording, score) of the
    valid ones, recording by recording"""
    R, cap = int(fields.shape[0]), int(fields.shape[1])
    dev = fields.device
    keep = torch.arange(cap, device=dev)[None, :] < counts[:, None]                       # (R, cap)
    rec = torch.arange(R, device=dev, dtype=torch.int32)[:, None].expand(-1, cap)[keep]
    return fields[keep], rec, score[keep]


def collect(result, chunk_size, sensitivity=0.5, trigger_level=3, events=None, lengths=None, tolerance_samples=None, background_index=0,
            max_det=None, pr=None):
    """The activations of scanned recordings at one operating point (kws_stream_collect): what Listener.on_activation
    (listen.py:291-308) would have been called for, file by file, with each activation classified against labelled events --
    hit, duplicate or false alarm, by `sweep`'s rule -- so the false alarms can become `background` clips.

    result / events / lengths / tolerance_samples / background_index / pr: as `sweep` takes them, with the same checks.  The
    walk is recomputed from the scan's index / score, so any point of a sweep can be collected without scanning again.
    max_det: slots per recording; the default is the largest count, found by a counting launch (max_det = 0) whose result
    is read back -- the one host synchronisation here.  Returns `Detections` in (recording, chunk) order."""
    chunk_size = int(chunk_size)
    if max_det is not None and int(max_det) < 0:
        raise ValueError("max_det must be >= 0")
    scanned = _Scanned(result, chunk_size, events, lengths, tolerance_samples, background_index, pr)
    torch = _torch()
    L = _l.get_lib()
    R, dev, ev = scanned.R, scanned.index.device, scanned.ev
    n_det = torch.zeros(R, dtype=torch.int32, device=dev)

    def launch(cap, det, det_score):
        _l.check(L.kws_stream_collect(scanned.index.data_ptr(), scanned.score.data_ptr(), R, scanned.stride, scanned.d_chunks.data_ptr(),
                                      int(background_index), chunk_size, float(sensitivity), int(trigger_level), ev[0], ev[1], ev[2], ev[3],
                                      cap, n_det.data_ptr(), det, det_score, _stream()))

    n = None
    if max_det is None:
        launch(0, 0, 0)
        n = n_det.cpu().tolist()
        cap = max(n + [0])
    else:
        cap = int(max_det)
    det = torch.empty((R, cap, 4), dtype=torch.int32, device=dev)
    det_score = torch.empty((R, cap), dtype=torch.float64, device=dev)
    if n is None or cap > 0:
        launch(cap, det.data_ptr(), det_score.data_ptr())
    if n is None:
        n = n_det.cpu().tolist()
    f, rec, sc = _flatten(torch, torch.clamp(n_det, max=cap), det, det_score)
    return Detections(n, rec, f[:, 0].contiguous(), f[:, 1].contiguous(), f[:, 2].contiguous(), f[:, 3].contiguous(), sc, chunk_size,
                      n_stored=[min(v, cap) for v in n], audio=scanned.audio)


def _check_peaks(k, min_gap):
    if not 1 <= int(k) <= 64:
        raise ValueError("k=%d peaks per recording is outside 1..64" % int(k))
    if min_gap is not None and int(min_gap) < 1:
        raise ValueError("min_gap=%d must be at least 1" % int(min_gap))


def peaks(result, chunk_size, k=8, min_score=0.0, min_gap=None, events=None, lengths=None, tolerance_samples=None, background_index=0,
          pr=None):
    """The near misses of scanned recordings (kws_stream_peaks): per recording the up to k highest-scoring non-background
    chunks with score > min_score, at least min_gap chunks apart (default ceil(pr.buffer_samples / chunk_size): their
    clips do not overlap), chosen greedily, best first, ties to the earlier chunk.  With `events` (as `sweep` takes them) the
    chunks inside any event's window are left out, whatever the class: labelled keywords are no negatives.  Returns
    `Detections` in (recording, pick) order with kind DET_UNLABELLED and event -1; n is read back (one synchronisation)."""
    chunk_size = int(chunk_size)
    _check_peaks(k, min_gap)
    scanned = _Scanned(result, chunk_size, events, lengths, tolerance_samples, background_index, pr)
    if min_gap is None:
        if pr is None:
            from classifier.params import pr
        min_gap = max(1, -(-int(pr.buffer_samples) // chunk_size))
    torch = _torch()
    k, min_gap = int(k), int(min_gap)
    R, dev, ev = scanned.R, scanned.index.device, scanned.ev
    n_peaks = torch.zeros(R, dtype=torch.int32, device=dev)
    found = torch.empty((R, k, 2), dtype=torch.int32, device=dev)
    found_score = torch.empty((R, k), dtype=torch.float64, device=dev)
    _l.check(_l.get_lib().kws_stream_peaks(scanned.index.data_ptr(), scanned.score.data_ptr(), R, scanned.stride, scanned.d_chunks.data_ptr(),
                                           int(background_index), float(min_score), min_gap, ev[0], ev[2], ev[3], k, n_peaks.data_ptr(),
                                           found.data_ptr(), found_score.data_ptr(), _stream()))
    n = n_peaks.cpu().tolist()
    f, rec, sc = _flatten(torch, n_peaks, found, found_score)
    chunk = f[:, 0].contiguous()
    return Detections(n, rec, chunk, f[:, 1].contiguous(), torch.zeros_like(chunk), torch.full_like(chunk, -1), sc, chunk_size, audio=scanned.audio)
