"""Labelled streaming test recordings from one-second clips, on the device (include/kws.h: kws_synth_plan, kws_synth_render;
csrc/kws_synth.hip).

`synthesize` lays clips of a Speech-Commands-style test set at random gaps over a continuous bed of background noise and writes down
where each one went: what TensorFlow's generate_streaming_test_wav does on the host, for R recordings at once and without a host loop
over the events.  The result, a `SynthSet`, carries the audio (a device tensor), the events in the form `kws_amd.stream.sweep` takes,
and the raw plan; `SynthSet.scan` / `.sweep` forward to kws_amd.stream, `.save` writes wavs and a labels file that
`listen.py --sweep --labels_path` reads.  All draws, gains and samples come from the HIP library; there is no host fallback.
"""
import ctypes
import os

import numpy as np

from . import lib as _l
from .augment import NoiseBank, _wav_code, parse_snr

REC_DTYPE = np.dtype([("segment", "<i4"), ("offset", "<i4"), ("bed_gain", "<f4"), ("n_events", "<i4")])
EVENT_DTYPE = np.dtype([("row", "<i4"), ("start", "<i4"), ("length", "<i4"), ("snr_db", "<f4"), ("gain", "<f4"), ("reserved", "<i4", (3,))])
MAX_EVENTS = 4096                                          # include/kws.h KWS_SYNTH_MAX_EVENTS
INT_MAX = 2 ** 31 - 1
OUT_DTYPES = ("int16", "float32")


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise _l.KwsError(-3, "no HIP device visible to torch: the synthesis has no CPU fallback")
    return torch


def _pair(name, value):
    try:
        lo, hi = (float(v) for v in value)
    except (TypeError, ValueError):
        raise ValueError("%s must be a (lo, hi) pair, got %r" % (name, value))
    if not lo <= hi:
        raise ValueError("%s needs lo <= hi, got %r" % (name, value))
    return lo, hi


def synth_params(gap=(16000, 48000), lead_in=16000, clip_cap=16000, snr=None, bed_gain=(0.05, 0.2), max_gain=8.0, fade=80, seed=0):
    """The checked kws_synth_params of a synthesis, everything in samples.  Pure Python: raises ValueError for what kws_synth_plan
    refuses."""
    lo, hi = _pair("gap", gap)
    lo, hi = int(lo), int(hi)
    if lo < 0 or hi > INT_MAX:
        raise ValueError("gap must lie in 0..2^31 - 1 samples, got %r" % (gap,))
    if int(lead_in) < 0:
        raise ValueError("lead_in must be >= 0, got %r" % (lead_in,))
    if int(clip_cap) < 1:
        raise ValueError("clip_cap must be >= 1, got %r" % (clip_cap,))
    snr = [] if snr is None else parse_snr(snr)
    if len(snr) > _l.AUG_MAX_SNR or not all(np.isfinite(snr)):
        raise ValueError("snr takes at most %d finite values" % _l.AUG_MAX_SNR)
    b_lo, b_hi = _pair("bed_gain", bed_gain)
    if not float(max_gain) > 0:
        raise ValueError("max_gain must be positive, got %r" % (max_gain,))
    if int(fade) < 0:
        raise ValueError("fade must be >= 0, got %r" % (fade,))
    p = _l.KwsSynthParams()
    p.gap_lo, p.gap_hi, p.lead_in, p.clip_cap, p.n_snr = lo, hi, int(lead_in), int(clip_cap), len(snr)
    for i, s in enumerate(snr):
        p.snr_db[i] = s
    p.bed_gain_lo, p.bed_gain_hi, p.max_gain, p.fade, p.seed = b_lo, b_hi, float(max_gain), int(fade), int(seed) & (2 ** 64 - 1)
    return p


def check_plan(plan, lengths, rows, clip_lengths=None):
    """A caller's events, per recording a list of (row, start) or (row, start, gain): sorted by start, inside the recording, no two
    overlapping, every row in the clip store.  clip_lengths: host lengths of the rows (None: not known here, the length check is
    left to the caller).  Pure Python; -> per recording [(row, start, gain), ...]."""
    if len(plan) != len(lengths):
        raise ValueError("%d event lists for %d recordings" % (len(plan), len(lengths)))
    out = []
    for r, (evs, N) in enumerate(zip(plan, lengths)):
        cur, prev_end = [], 0
        for e in evs:
            row, start = int(e[0]), int(e[1])
            gain = float(e[2]) if len(e) > 2 else 1.0
            if not 0 <= row < rows:
                raise ValueError("recording %d: row %d is outside the %d clips" % (r, row, rows))
            if start < prev_end:
                raise ValueError("recording %d: the event at %d starts before sample %d (unsorted or overlapping events)" % (r, start, prev_end))
            L = 0 if clip_lengths is None else int(clip_lengths[row])
            if start + L > int(N):
                raise ValueError("recording %d: the event at %d (%d samples) passes the recording's end (%d samples)" % (r, start, L, int(N)))
            prev_end = start + L
            cur.append((row, start, gain))
        out.append(cur)
    return out


def write_labels(path, events, names, class_names, sample_rate):
    """The labels file `listen.parse_labels` reads: `wav_name class_name start_seconds end_seconds` per event; nine decimals, so
    that the sample numbers come back exactly."""
    with open(path, "w") as f:
        f.write("# wav_name class_name start_seconds end_seconds\n")
        for name, evs in zip(names, events):
            for cls, start, end in evs:
                f.write("%s %s %.9f %.9f\n" % (name, class_names[int(cls)], start / float(sample_rate), end / float(sample_rate)))


def min_event_gap(events):
    """the smallest distance in samples from an event's end to the next one's start over all recordings, or None"""
    gaps = [b[1] - a[2] for evs in events for a, b in zip(evs, evs[1:])]
    return min(gaps) if gaps else None


class SynthSet(object):
    """What `synthesize` made.  wav: (R, stride) CUDA tensor, int16 or float32, zeros past a recording's length; lengths: host list of
    R sample counts; events: per recording [(class_index, start_sample, end_sample), ...] of the labelled clips, in order -- what
    `kws_amd.stream.events_to_chunks` / `sweep` take; rec / plan: the raw device records (`records()` reads them back)."""

    def __init__(self, wav, lengths, events, rec, plan, sample_rate):
        self.wav, self.lengths, self.events, self.rec, self.plan = wav, [int(v) for v in lengths], events, rec, plan
        self.sample_rate = int(sample_rate)

    @property
    def seconds(self):
        return [n / float(self.sample_rate) for n in self.lengths]

    def records(self):
        """-> (rec, events): numpy record arrays of REC_DTYPE (R,) and EVENT_DTYPE (R, max_events); one synchronisation"""
        rec = np.frombuffer(self.rec.cpu().numpy().tobytes(), dtype=REC_DTYPE).copy()
        ev = np.frombuffer(self.plan.cpu().numpy().tobytes(), dtype=EVENT_DTYPE).reshape(len(rec), -1).copy()
        return rec, ev

    def tolerance_samples(self, chunk_size, pr=None):
        """How long after a keyword's end a detection may still count for it without reaching into the next event's chunks: the
        model's buffer (pr.max_samples, `sweep`'s default), cut to the smallest gap between two events less one chunk."""
        if pr is None:
            from classifier.params import pr
        gap = min_event_gap(self.events)
        return int(pr.max_samples) if gap is None else max(0, min(int(pr.max_samples), gap - int(chunk_size)))

    def pcm(self):
        """the recordings as the int16 CUDA tensor `scan` reads (a float32 set is converted as the int16 render does)"""
        torch = _torch()
        if self.wav.dtype == torch.int16:
            return self.wav
        return torch.clamp(torch.round(self.wav * 32768.0), -32768, 32767).to(torch.int16)

    def scan(self, pr, device_model, **kwargs):
        """`kws_amd.stream.scan` of the recordings (the keywords are scan's)"""
        from .stream import scan
        return scan(pr, device_model, self.pcm(), lengths=self.lengths, **kwargs)

    def sweep(self, pr, device_model, sensitivities, trigger_levels, chunk_size=1024, tolerance_samples=None, background_index=0, **scan_kwargs):
        """One scan, then `kws_amd.stream.sweep` against this set's events.  -> SweepResult with `seconds` set; `self.last_scan`
        keeps the scan.  tolerance_samples defaults to `self.tolerance_samples(chunk_size)`."""
        from .stream import sweep
        if tolerance_samples is None:
            tolerance_samples = self.tolerance_samples(chunk_size, pr)
        self.last_scan = self.scan(pr, device_model, chunk_size=chunk_size, background_index=background_index, **scan_kwargs)
        out = sweep(self.last_scan, sensitivities, trigger_levels, chunk_size, events=self.events, lengths=self.lengths,
                    tolerance_samples=tolerance_samples, background_index=background_index, pr=pr)
        out.seconds = self.seconds
        return out

    def save(self, save_dir, class_names, prefix="synth"):
        """Writes <save_dir>/<prefix>_<r>.wav (16-bit mono) and <save_dir>/labels.txt (see `write_labels`).  -> (paths, labels path)"""
        import wave
        os.makedirs(save_dir, exist_ok=True)
        pcm = self.pcm().cpu().numpy()
        names = ["%s_%d.wav" % (prefix, r) for r in range(len(self.lengths))]
        paths = [os.path.join(save_dir, n) for n in names]
        for r, p in enumerate(paths):
            wf = wave.open(p, "wb")
            wf.setnchannels(1)
            wf.setsampwidth(2)
            wf.setframerate(self.sample_rate)
            wf.writeframes(pcm[r, :self.lengths[r]].astype("<i2").tobytes())
            wf.close()
        labels = os.path.join(save_dir, "labels.txt")
        write_labels(labels, self.events, names, class_names, self.sample_rate)
        return paths, labels


def _lengths(seconds, recordings, sample_rate):
    """seconds: one duration for `recordings` recordings, or a list with one per recording"""
    if isinstance(seconds, (list, tuple, np.ndarray)):
        lens = [int(round(float(s) * sample_rate)) for s in seconds]
    else:
        if int(recordings) < 0:
            raise ValueError("recordings must be >= 0, got %r" % (recordings,))
        lens = [int(round(float(seconds) * sample_rate))] * int(recordings)
    if any(n < 0 or n > INT_MAX for n in lens):
        raise ValueError("a recording needs 0..2^31 - 1 samples")
    return lens


def synthesize(clips, labels, valid_len=None, noise=None, recordings=8, seconds=600, gap_s=(1.0, 3.0), lead_in_s=1.0, snr=None,
               bed_gain=(0.05, 0.2), max_gain=8.0, fade_ms=5, seed=0, pick=None, out_dtype='int16', position_base=0, plan=None,
               background_index=0, max_events=None, sample_rate=None, clip_cap=None):
    """R = `recordings` test recordings of `seconds` each (a list gives ragged lengths, one per recording) from `clips`.

    clips: (rows, stride) float32 or int16 clip store (numpy or CUDA tensor), head-aligned as classifier.data.load_audio_samples
    returns it; labels: the class index of every row; valid_len: the rows' sample counts (None: stride).  noise: a
    kws_amd.augment.NoiseBank, or what it takes (a folder, a list of arrays); None gives a silent bed.  gap_s: bounds of the pause
    in front of every clip; snr: dB values a clip's level against the bed under it is drawn from (None: the clips as they are);
    bed_gain: bounds of the bed's gain, one draw per recording; max_gain caps a clip's gain; fade_ms: linear fade at both ends of
    a clip.  pick: row numbers to draw from (None: all).  position_base: global number of the first recording, so shards of one set
    draw what the whole set draws.  plan: per recording a list of (row, start_sample[, gain]) rendered instead of drawn events (the
    bed stays the drawn one); checked on the host (sorted, no overlap, inside the recording).  Clips of class `background_index` are rendered as distractors
    and listed in no event; neither are clips of no samples.  One synchronisation (the plan is read back for the events)."""
    if out_dtype not in OUT_DTYPES:
        raise ValueError("out_dtype must be one of %s, got %r" % (", ".join(OUT_DTYPES), out_dtype))
    if int(position_base) < 0:
        raise ValueError("position_base must be >= 0")
    if sample_rate is None or clip_cap is None:
        from classifier.params import pr
        sample_rate = pr.sample_rate if sample_rate is None else sample_rate
        clip_cap = pr.max_samples if clip_cap is None else clip_cap
    rate = int(sample_rate)
    lens = _lengths(seconds, recordings if plan is None else len(plan), rate)
    gap = tuple(int(round(v * rate)) for v in _pair("gap_s", gap_s))
    params = synth_params(gap, int(round(float(lead_in_s) * rate)), clip_cap, snr, bed_gain, max_gain, int(round(float(fade_ms) * rate / 1000.0)),
                          seed)
    R, max_len = len(lens), max(lens + [0])
    if max_events is None:
        max_events = min(MAX_EVENTS, max_len // max(1, params.gap_lo) + 1) if plan is None else max([len(v) for v in plan] + [1])
    if not 1 <= int(max_events) <= MAX_EVENTS:
        raise ValueError("max_events=%d is outside 1..%d" % (int(max_events), MAX_EVENTS))
    max_events = int(max_events)
    labels = np.asarray(labels).astype(np.int64).reshape(-1)
    if labels.shape[0] != len(clips):
        raise ValueError("%d labels for %d clips" % (labels.shape[0], len(clips)))
    rows = int(labels.shape[0])
    if rows < 1:
        raise ValueError("the clip store is empty")
    host_len = None
    if plan is not None:
        stride = int(clips.shape[1])
        host_len = np.full(rows, stride, np.int64) if valid_len is None else np.asarray(valid_len.cpu() if hasattr(valid_len, "cpu") else valid_len,
                                                                                         np.int64).reshape(-1)
        host_len = np.minimum(np.clip(host_len, 0, stride), int(clip_cap))
        plan = check_plan(plan, lens, rows, host_len)
    if pick is not None:
        pick_host = np.asarray(pick.cpu() if hasattr(pick, "cpu") else pick).astype(np.int64).reshape(-1)
        if pick_host.size < 1 or pick_host.min() < 0 or pick_host.max() >= rows:
            raise ValueError("pick must name at least one row in 0..%d" % (rows - 1))

    torch = _torch()
    L = _l.get_lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    if not isinstance(clips, torch.Tensor):
        clips = np.asarray(clips)
        clips = torch.from_numpy(np.ascontiguousarray(clips) if clips.flags.writeable else clips.copy())    # torch takes no read-only array
    wav = clips
    wav = wav.to(dev).contiguous()
    if wav.dim() != 2:
        raise ValueError("clips must have shape (rows, stride)")
    code = _wav_code(wav)
    stride = int(wav.shape[1])
    d_valid = None
    if valid_len is not None:
        d_valid = (valid_len if isinstance(valid_len, torch.Tensor) else torch.from_numpy(np.array(valid_len, np.int32))).to(dev).to(torch.int32).contiguous()
        if d_valid.numel() != rows:
            raise ValueError("valid_len must have one element per clip")
    d_pick = None if pick is None else torch.from_numpy(pick_host.astype(np.int32)).to(dev)
    bank = noise if noise is None or isinstance(noise, NoiseBank) else NoiseBank(noise)
    h_bank = None if bank is None else bank.handle()
    d_len = torch.tensor(lens, dtype=torch.int32).to(dev)
    rec = torch.zeros((R, REC_DTYPE.itemsize // 4), dtype=torch.int32, device=dev)
    events = torch.zeros((R, max_events, EVENT_DTYPE.itemsize // 4), dtype=torch.int32, device=dev)

    def launch_plan():
        _l.check(L.kws_synth_plan(h_bank, ctypes.byref(params), wav.data_ptr(), code, rows, stride, None if d_valid is None else d_valid.data_ptr(),
                                  None if d_pick is None else d_pick.data_ptr(), rows if d_pick is None else int(d_pick.numel()),
                                  d_len.data_ptr(), R, max_events, int(position_base), rec.data_ptr(), events.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream))

    def launch_render(out):
        _l.check(L.kws_synth_render(h_bank, wav.data_ptr(), code, rows, stride, rec.data_ptr(), events.data_ptr(), max_events, d_len.data_ptr(), R,
                                    max_len, params.fade, out.data_ptr(), _l.WAV_I16 if out.dtype == torch.int16 else _l.WAV_F32,
                                    int(out.shape[1]), torch.cuda.current_stream().cuda_stream))

    launch_plan()
    if plan is not None and R:
        # the bed stays the drawn one; the caller's events replace the drawn ones
        h_ev = np.zeros((R, max_events), EVENT_DTYPE)
        h_ev["row"] = -1
        for r, evs in enumerate(plan):
            for j, (row, start, gain) in enumerate(evs):
                h_ev[r, j] = (row, start, int(host_len[row]), 0.0, gain if host_len[row] > 0 else 0.0, (0, 0, 0))
        events.copy_(torch.from_numpy(h_ev.view(np.int32).reshape(R, max_events, -1)))
        rec[:, 3] = torch.tensor([len(v) for v in plan], dtype=torch.int32).to(dev)
    out_t = torch.int16 if out_dtype == 'int16' else torch.float32
    out_stride = (max_len + 7) & ~7                                      # whole 128-bit vectors of either dtype
    out = torch.empty((R, out_stride), dtype=out_t, device=dev)
    launch_render(out)
    result = SynthSet(out, lens, None, rec, events, rate)
    result.replan, result.rerender = launch_plan, lambda: launch_render(out)     # the same launches again (tools/synthbench.py times them)
    h_rec, h_ev = result.records()
    listed = []
    for r in range(R):
        evs = h_ev[r, :int(h_rec["n_events"][r])]
        listed.append([(int(labels[e["row"]]), int(e["start"]), int(e["start"]) + int(e["length"])) for e in evs
                       if e["length"] > 0 and labels[e["row"]] != background_index])
    result.events = listed
    result.bank = bank                                                   # keeps the bank's device memory alive with the set
    return result
