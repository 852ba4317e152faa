#!/usr/bin/env python3
# -*- coding: utf-8 -*-
"""Streaming keyword detection on the MI355X path: the `Listener` of the reference's listen.py with the same
constructor keywords and methods (`update_vectors`, `predict`, `run_wav`, `on_prediction`, `on_activation`), built on
kws_amd.stream.StreamBatch -- feature update, forward pass, score decoding and trigger logic all run on the device.
`Listener.scan_wav` (CLI: --scan) is the offline form for recorded audio: whole files, or a directory of them, go through
kws_amd.stream.scan at once and give per chunk what `run_wav` gives.  `Listener.sweep_wav` (CLI: --sweep) scans labelled
recordings once and evaluates the detector at a whole grid of (sensitivity, trigger_level): miss rate against false alarms per hour.
`--save_dir` saves the audio buffer of every activation as the reference does (listen.py:299-308): chunk by chunk in `run_wav`, and
for whole files at once in --scan / --sweep through `Listener.collect_wav` (kws_amd.stream.collect / peaks), which with labels
tells false alarms from hits and can add the near misses that never fired (--mine_peaks).  `Listener.sweep_synth` (CLI: --sweep
--synth_from DATASET_DIR) needs no labelled recordings: it synthesizes them on the device from a dataset's one-second clips and a
folder of background noise (kws_amd.synth) and sweeps those.  `--head_bank BANK.npz` (with --scan / --sweep) gives every recording a
keyword set of its own on the one backbone: a kws_amd.transfer.HeadBank, and `--head_map FILE` naming each recording's head.

Differences from listen.py: checkpoints are the `.npz` files classifier.model writes (no h5/pb/tflite/onnx/mnn
back ends); there is no PyAudio in this image, so `run_microphone` raises and `run_wav` does not play the audio while it
analyses it; `Listener.batch(n)` gives the many-stream form for serving.
"""
import argparse
import json
import os
import wave
from random import randint
from shutil import get_terminal_size

import numpy as np

from classifier.model import get_model
from classifier.params import inject_params, pr
from common.utils import get_classes
from kws_amd import lib as _lib
from kws_amd.stream import StreamBatch, ThresholdDecoder, TriggerDetector, scan  # noqa: F401  (re-exported like listen.py:452,525)
from kws_amd.stream import collect, peaks, sweep
from kws_amd.synth import synthesize

SAVE_KINDS = {                                         # --save_kind -> the kinds of kws_amd.stream.Detections it keeps
    "false_alarms": (_lib.DET_FALSE_ALARM,),
    "hits": (_lib.DET_HIT,),
    "duplicates": (_lib.DET_DUPLICATE,),
    "all": None,
}

default_config = {                                     # listen.py:31-40
    "model_path": '',
    "quantized_path": None,
    "model_type": 'simple_cnn',
    "rnn_layers": 1,
    "classes_path": os.path.join('configs', 'direction_classes.txt'),
    "params_path": None,
    "chunk_size": 1024,
    "sensitivity": 0.5,
    "trigger_level": 3,
    "save_dir": None,
    "input_wav": None,
    "scan": False,
    "scan_tile": 4096,
    "resample": False,
    "head_bank": None,
    "head_map": None,
}


def parse_sensitivities(text):
    """--sensitivities: 'a,b,c' (a list) or 'lo:hi:n' (n evenly spaced values from lo to hi, both ends included)"""
    text = text.strip()
    if ':' in text:
        parts = text.split(':')
        if len(parts) != 3:
            raise ValueError("expected lo:hi:n, got %r" % text)
        lo, hi, n = float(parts[0]), float(parts[1]), int(parts[2])
        if n < 1 or (n == 1 and lo != hi):
            raise ValueError("lo:hi:n needs n >= 2 (or lo == hi), got %r" % text)
        return [lo] if n == 1 else [lo + (hi - lo) * i / (n - 1) for i in range(n - 1)] + [hi]
    vals = [float(v) for v in text.split(',') if v.strip()]
    if not vals:
        raise ValueError("no sensitivity in %r" % text)
    return vals


def parse_trigger_levels(text):
    """--trigger_levels: '1,2,3'"""
    vals = [int(v) for v in text.split(',') if v.strip()]
    if not vals or min(vals) < 0:
        raise ValueError("expected non-negative trigger levels, got %r" % text)
    return vals


def parse_head_map(path, bank):
    """The file of --head_map: text, one recording per line, `wav_name head_name`; '#' starts a comment.  head_name is a name the bank
    holds (HeadBank.names) or a head id.  -> {wav_name: head id}; a wav it does not mention listens with head 0."""
    out = {}
    with open(path) as f:
        for no, line in enumerate(f, 1):
            fields = line.split('#', 1)[0].split()
            if not fields:
                continue
            if len(fields) != 2:
                raise ValueError("%s:%d: expected `wav_name head_name`" % (path, no))
            name, head = fields
            if head in bank.names:
                h = bank.names.index(head)
            elif head.isdigit() and int(head) < bank.capacity:
                h = int(head)
            else:
                raise ValueError("%s:%d: the bank has no head %r" % (path, no, head))
            if bank.classes[h] == 0:
                raise ValueError("%s:%d: head %r is empty" % (path, no, head))
            out[os.path.basename(name)] = h
    return out


def parse_labels(path, class_names, sample_rate):
    """The labels file of --sweep: text, one event per line, `wav_name class_name start_seconds end_seconds`; '#' starts a
    comment.  -> {wav_name: [(class_index, start_sample, end_sample), ...]}; a wav it does not mention has no events.
    class_names: the list, or a function of the wav's name that gives its list (a head per recording)."""
    out = {}
    names_of = class_names if callable(class_names) else (lambda wav_name: class_names)
    with open(path) as f:
        for no, line in enumerate(f, 1):
            fields = line.split('#', 1)[0].split()
            if not fields:
                continue
            if len(fields) != 4:
                raise ValueError("%s:%d: expected `wav_name class_name start_seconds end_seconds`" % (path, no))
            name, cls, start, end = fields
            class_names = names_of(os.path.basename(name))
            if cls not in class_names:
                raise ValueError("%s:%d: unknown class name %r" % (path, no, cls))
            a, b = int(round(float(start) * sample_rate)), int(round(float(end) * sample_rate))
            if not 0 <= a < b:
                raise ValueError("%s:%d: an event needs 0 <= start < end" % (path, no))
            out.setdefault(os.path.basename(name), []).append((class_names.index(cls), a, b))
    return out


def parse_gap(text):
    """--synth_gap_s: 'LO,HI' in seconds"""
    vals = [float(v) for v in text.split(',') if v.strip()]
    if len(vals) != 2 or not 0 <= vals[0] <= vals[1]:
        raise ValueError("expected LO,HI with 0 <= LO <= HI, got %r" % text)
    return vals[0], vals[1]


class Listener(object):
    _defaults = default_config

    @classmethod
    def get_defaults(cls, n):
        if n in cls._defaults:
            return cls._defaults[n]
        return "Unrecognized attribute name '" + n + "'"

    def __init__(self, **kwargs):
        self.__dict__.update(self._defaults)
        self.__dict__.update(kwargs)
        self.pr = inject_params(self.params_path) if self.params_path else pr
        self.class_names = get_classes(self.classes_path)
        assert self.class_names[0] == 'background', '1st class should be background.'
        self.quantized = None
        if getattr(self, "quantized_path", None):
            # an int8 model saved by eval.py --save_quantized: it computes the probabilities; the float model only carries the device
            from kws_amd.quant import load as load_quantized
            self.quantized = load_quantized(self.quantized_path)
            if self.quantized.num_classes != len(self.class_names):
                raise ValueError("%s has %d classes, %s lists %d" % (self.quantized_path, self.quantized.num_classes, self.classes_path,
                                                                    len(self.class_names)))
            self.model_type = self.quantized.spec.model_type
        self.model = kwargs.get("model") or get_model(self.model_type, len(self.class_names), weights_path=self.model_path or None,
                                                      num_layers=self.rnn_layers)
        self.threshold_decoder = ThresholdDecoder(self.pr.threshold_config, self.pr.threshold_center)
        # --head_bank: a keyword set per recording for scan_wav / sweep_wav / collect_wav; run_wav keeps the model's own head
        self.heads, self.head_of = None, {}
        if getattr(self, "head_bank", None):
            from kws_amd.transfer import HeadBank
            if self.quantized is not None:
                raise ValueError("--head_bank does not go with --quantized_path: the int8 forwards end in their own head")
            self.heads = HeadBank.load(self.head_bank)
            if getattr(self, "head_map", None):
                self.head_of = parse_head_map(self.head_map, self.heads)
        self._sb = self.batch(1)
        self.detector = self._sb                       # detector state lives in the stream batch (device)
        self.activations = []
        # listen.py:90,94: the last buffer_samples samples (kept as the PCM that arrived; `audio_buffer` scales them) and the
        # names of the clips --save_dir writes
        self._pcm_ring = np.zeros(self.pr.buffer_samples, dtype=np.int16)
        self.session_id, self.record_num = '%09d' % randint(0, 999999999), 0
        self.saved_paths = []

    def names_for(self, wav_path):
        """the class names of a recording: its head's in the bank (where the bank keeps names), else the listener's"""
        if self.heads is None:
            return self.class_names
        return self.heads.class_names[self.head_of.get(os.path.basename(wav_path), 0)] or self.class_names

    def batch(self, n_streams):
        """A StreamBatch of n lock-stepped streams sharing this listener's model, decoder and settings."""
        return StreamBatch(self.pr, self.model._device(), n_streams, chunk_size=self.chunk_size, class_names=self.class_names,
                           sensitivity=self.sensitivity, trigger_level=self.trigger_level, decoder=self.threshold_decoder,
                           quantized=self.quantized)

    @property
    def audio_buffer(self):
        """listen.py:90,100: the last buffer_samples samples as buffer_to_audio scales them (float64, zeros before the first)"""
        return self._pcm_ring.astype(np.float64) / 32768.0

    def _push_audio(self, chunk):
        new = np.frombuffer(chunk, dtype='<i2')[-self._pcm_ring.size:]
        self._pcm_ring = np.concatenate((self._pcm_ring[new.size:], new))

    def update_vectors(self, chunk):
        """listen.py:96-114: bytes of int16 PCM in, the (n_features, n_mfcc, 1) feature matrix out."""
        self._push_audio(chunk)
        feats = self._sb.update_vectors([chunk])
        return np.expand_dims(feats[0].cpu().numpy(), axis=-1)

    def predict(self, data):
        if self.quantized is not None:
            probs, _ = self.quantized.forward(np.asarray(data, dtype=np.float32))
            return probs.cpu().numpy()
        return self.model.predict(np.asarray(data, dtype=np.float32))

    def step(self, chunk):
        """One iteration of the loop listen.py:350-375: (index, score, activated)."""
        self._push_audio(chunk)
        index, score, fired = self._sb.push([chunk])
        return int(index[0]), float(score[0]), bool(fired[0])

    def on_prediction(self, index, score):
        width = min(get_terminal_size()[0], 80)
        class_name = self.class_names[index]
        if class_name == 'background':                 # show the inverted score and no label, listen.py:281-283
            score = 1.0 - score
            class_name = ''
        units = int(round(score * width))
        bar = 'X' * units + '-' * (width - units)
        cutoff = round(self.sensitivity * width)
        print(bar[:cutoff] + bar[cutoff:].replace('X', 'x') + class_name)

    def on_activation(self, index, play_activate=False, save=True):
        """listen.py:291-308.  save=False: the caller saves the clips itself (scan_wav: whole files at once, collect_wav)."""
        print('command {} detected!'.format(self.class_names[index]))
        self.activations.append(index)
        if self.save_dir and save:
            save_class_dir = os.path.join(self.save_dir, self.class_names[index])
            os.makedirs(save_class_dir, exist_ok=True)
            wav_path = os.path.join(save_class_dir, self.session_id + '_' + str(self.record_num) + '.wav')
            assert self.pr.sample_depth == 2, 'only support 16-bit sample depth.'
            wf = wave.open(wav_path, 'wb')
            wf.setnchannels(1)
            wf.setsampwidth(self.pr.sample_depth)
            wf.setframerate(self.pr.sample_rate)
            wf.writeframes((self.audio_buffer * 32767).astype('<i2').tobytes())      # save_audio, data_utils.py:46
            wf.close()
            print('Saved to ' + wav_path + '.')
            self.saved_paths.append(wav_path)
            self.record_num += 1

    def run_microphone(self):
        raise RuntimeError("PyAudio is not available in this image; feed chunks with Listener.step() or use run_wav()")

    def _run_converted(self, rate, quiet):
        """run_wav of a file at another rate (resample=True): the file is converted at once (kws_amd.rate.convert), then walked
        chunk by chunk like any other; chunks and the saved buffer are in converted samples."""
        from kws_amd.rate import convert
        out, lens = convert([self._read_wav(self.input_wav, with_rate=True)[0]], rate, self.pr.sample_rate)
        pcm = out[0, :lens[0]].cpu().numpy()
        results = []
        for k in range(0, pcm.size, self.chunk_size):
            index, score, fired = self.step(pcm[k:k + self.chunk_size].tobytes())
            if not quiet:
                self.on_prediction(index, score)
            if fired:
                self.on_activation(index, play_activate=False)
            results.append((index, score, fired))
        return results

    def run_wav(self, quiet=False):
        wf = wave.open(self.input_wav, 'rb')
        assert wf.getnchannels() == 1, 'input wav channels mismatch'
        if self.resample and wf.getframerate() != self.pr.sample_rate:
            rate = wf.getframerate()
            wf.close()
            return self._run_converted(rate, quiet)
        assert wf.getframerate() == self.pr.sample_rate, 'input wav sample rate mismatch'
        assert wf.getsampwidth() == self.pr.sample_depth, 'input wav sample depth mismatch'
        assert wf.getnframes() > 0, 'no valid data in input wav'
        results = []
        chunk = wf.readframes(self.chunk_size)
        while len(chunk) > 0:
            index, score, fired = self.step(chunk)
            if not quiet:
                self.on_prediction(index, score)
            if fired:
                self.on_activation(index, play_activate=False)
            results.append((index, score, fired))
            chunk = wf.readframes(self.chunk_size)
        wf.close()
        return results

    def _read_wav(self, path, with_rate=False):
        """-> the file's int16 samples; with_rate: (samples, its sample rate), which resample=True lets differ from pr.sample_rate"""
        wf = wave.open(path, 'rb')
        assert wf.getnchannels() == 1, 'input wav channels mismatch'
        rate = wf.getframerate()
        assert (with_rate and self.resample) or rate == self.pr.sample_rate, 'input wav sample rate mismatch'
        assert wf.getsampwidth() == self.pr.sample_depth, 'input wav sample depth mismatch'
        pcm = np.frombuffer(wf.readframes(wf.getnframes()), dtype='<i2')
        wf.close()
        return (pcm, rate) if with_rate else pcm

    def _scan_files(self, files, keep_audio=False):
        """-> (ScanResult of the files, their sample counts): read, packed and scanned at once.  With resample=True files at other
        rates are converted on the device first; the counts, like everything the scan returns, are then in converted samples."""
        read = [self._read_wav(p, with_rate=True) for p in files]
        pcm, rates = [a for a, _ in read], [r for _, r in read]
        rec_heads = None if self.heads is None else [self.head_of.get(os.path.basename(p), 0) for p in files]
        res = scan(self.pr, self.model._device(), pcm, chunk_size=self.chunk_size, class_names=self.class_names,
                   sensitivity=self.sensitivity, trigger_level=self.trigger_level, decoder=self.threshold_decoder,
                   quantized=self.quantized, tile=self.scan_tile, keep_audio=keep_audio, sample_rates=rates, heads=self.heads,
                   recording_heads=rec_heads)
        if all(r == self.pr.sample_rate for r in rates):
            return res, [int(a.size) for a in pcm]
        from kws_amd.rate import bank_for
        return res, [bank_for(r, self.pr.sample_rate).total(a.size) for a, r in zip(pcm, rates)]

    def scan_wav(self, paths=None, quiet=True):
        """run_wav for whole files at once (kws_amd.stream.scan): `paths` is one wav or a list of them (default: input_wav).
        Returns per file the list run_wav returns, [(index, score, fired), ...] per chunk, every file starting from a fresh
        detector; on_activation is called for every fired chunk in order (and on_prediction for every chunk unless quiet).
        `self.scan_times[i]` lists the times, in seconds from the start of file i, of its activations.  `self.last_scan` keeps
        (ScanResult, sample counts); with save_dir set the scan keeps its audio, for `collect_wav(..., scan=self.last_scan)`."""
        if paths is None:
            paths = self.input_wav
        single = isinstance(paths, (str, bytes, os.PathLike))
        files = [paths] if single else list(paths)
        res, lens = self.last_scan = self._scan_files(files, keep_audio=bool(self.save_dir))
        index, score, fired = res.index.cpu().numpy(), res.score.cpu().numpy(), res.fired.cpu().numpy()
        out, self.scan_times = [], []
        own_names = self.class_names
        for r, n in enumerate(res.n_chunks):
            self.class_names = self.names_for(files[r])            # what on_prediction / on_activation print: the recording's head's
            rows = [(int(index[r, k]), float(score[r, k]), bool(fired[r, k])) for k in range(n)]
            times = []
            for k, (i, sc, f) in enumerate(rows):
                if not quiet:
                    self.on_prediction(i, sc)
                if f:
                    times.append(k * self.chunk_size / float(self.pr.sample_rate))
                    self.on_activation(i, play_activate=False, save=False)
            out.append(rows)
            self.scan_times.append(times)
        self.class_names = own_names
        return out[0] if single else out

    def sweep_wav(self, paths, labels, sensitivities, trigger_levels, tolerance_s=None):
        """One scan of the files, then the detector at every (sensitivity, trigger_level) of the grid (kws_amd.stream.sweep).
        `labels`: a labels file (see parse_labels), a dict {wav_name: [(class_index, start_sample, end_sample), ...]} keyed by
        file name without its directory, or None (fires are counted, nothing else); a wav without an entry is a negative
        recording.  tolerance_s: how long after a keyword's end a detection still counts for it (default: the model's buffer).
        Returns the SweepResult, its `seconds` set to the files' durations; `self.sweep_scan` keeps the scan."""
        files = [paths] if isinstance(paths, (str, bytes, os.PathLike)) else list(paths)
        if isinstance(labels, (str, bytes, os.PathLike)):
            labels = parse_labels(labels, self.names_for, self.pr.sample_rate)
        res, lens = self._scan_files(files, keep_audio=bool(self.save_dir))
        events = None if labels is None else [labels.get(os.path.basename(p), []) for p in files]
        tol = None if tolerance_s is None else int(round(tolerance_s * self.pr.sample_rate))
        out = sweep(res, sensitivities, trigger_levels, self.chunk_size, events=events, lengths=lens, tolerance_samples=tol, pr=self.pr)
        out.seconds = [n / float(self.pr.sample_rate) for n in lens]
        self.sweep_scan, self.sweep_lengths = res, lens
        return out

    def sweep_synth(self, dataset_dir, sensitivities, trigger_levels, noise_path=None, recordings=8, seconds=600, gap_s=(1.0, 3.0), snr=None,
                    seed=0, save_dir=None, tolerance_s=None):
        """sweep_wav without recordings: the clips under dataset_dir (one folder per class, or a dataset folder with `sounds` in it;
        classifier.data.load_audio_samples) are laid over the noise under noise_path (classifier.data.load_noise_bank; None: silence)
        by kws_amd.synth.synthesize, scanned once and swept.  save_dir: also write the recordings and their labels.txt there, for
        sweep_wav / --labels_path later.  tolerance_s defaults to SynthSet.tolerance_samples (kept in `self.synth_tolerance_s`).  Returns the
        SweepResult; `self.synth_set` keeps the SynthSet, `self.sweep_scan` the scan."""
        from classifier.data import load_audio_samples, load_noise_bank
        sounds = os.path.join(dataset_dir, 'sounds')
        x, lengths, words = load_audio_samples(sounds if os.path.isdir(sounds) else dataset_dir, self.class_names)
        if len(x) == 0:
            raise ValueError('no clips of the listed classes under ' + str(dataset_dir))
        labels = [self.class_names.index(w.lower()) for w in words]
        noise = load_noise_bank(noise_path) if noise_path else None
        self.synth_set = synthesize(x, labels, valid_len=lengths, noise=noise, recordings=recordings, seconds=seconds, gap_s=gap_s, snr=snr,
                                    seed=seed, sample_rate=self.pr.sample_rate, clip_cap=self.pr.max_samples)
        if save_dir:
            self.synth_set.save(save_dir, self.class_names)
        tol = self.synth_set.tolerance_samples(self.chunk_size, self.pr) if tolerance_s is None else int(round(tolerance_s * self.pr.sample_rate))
        self.synth_tolerance_s = tol / float(self.pr.sample_rate)
        out = self.synth_set.sweep(self.pr, self.model._device(), sensitivities, trigger_levels, chunk_size=self.chunk_size,
                                   tolerance_samples=tol, class_names=self.class_names, decoder=self.threshold_decoder,
                                   quantized=self.quantized, tile=self.scan_tile, keep_audio=bool(self.save_dir))
        self.sweep_scan, self.sweep_lengths = self.synth_set.last_scan, self.synth_set.lengths
        return out

    def collect_wav(self, paths, labels=None, sensitivity=None, trigger_level=None, tolerance_s=None, save_dir=None, save_kind=None,
                    mine_peaks=0, min_peak_score=0.0, scan=None):
        """The activations of whole files as training clips (kws_amd.stream.collect -> Detections.save): what run_wav with
        save_dir writes file by file, for all files in one pass.  `labels` as sweep_wav takes them: every activation is then a
        hit, a duplicate or a false alarm, and save_kind ('false_alarms', the default, 'hits', 'duplicates' or 'all') says
        which are saved; without labels every activation is.  sensitivity / trigger_level default to the listener's (a sweep's
        chosen point goes here); save_dir defaults to the listener's, and nothing is written without one.  mine_peaks = K > 0
        also takes the K best well-separated non-background chunks per file above min_peak_score (kws_amd.stream.peaks; with
        labels outside every event's window) and saves them under <save_dir>/near_miss/<class>/.  scan: a (ScanResult made with
        keep_audio=True, sample counts) pair of the same files, e.g. (self.sweep_scan, self.sweep_lengths), instead of scanning.
        Returns the Detections (all kinds); `self.collected_paths` lists the files written, `self.near_misses` the peaks."""
        files = [paths] if isinstance(paths, (str, bytes, os.PathLike)) else list(paths)
        if isinstance(labels, (str, bytes, os.PathLike)):
            labels = parse_labels(labels, self.class_names, self.pr.sample_rate)
        save_dir = self.save_dir if save_dir is None else save_dir
        save_kind = save_kind or getattr(self, 'save_kind', None) or 'false_alarms'
        if save_kind not in SAVE_KINDS:
            raise ValueError("save_kind must be one of %s, got %r" % (', '.join(sorted(SAVE_KINDS)), save_kind))
        res, lens = scan if scan is not None else self._scan_files(files, keep_audio=True)
        if res.wav is None:
            raise ValueError("collect_wav needs a scan made with keep_audio=True")
        events = None if labels is None else [labels.get(os.path.basename(p), []) for p in files]
        tol = None if tolerance_s is None else int(round(tolerance_s * self.pr.sample_rate))
        common = dict(events=events, lengths=lens, tolerance_samples=tol, pr=self.pr)
        det = collect(res, self.chunk_size, sensitivity=self.sensitivity if sensitivity is None else sensitivity,
                      trigger_level=self.trigger_level if trigger_level is None else trigger_level, **common)
        self.near_misses = peaks(res, self.chunk_size, k=int(mine_peaks), min_score=float(min_peak_score), **common) if mine_peaks else None
        self.collected_paths = []
        if save_dir:
            keep = det if events is None else det.select(kind=SAVE_KINDS[save_kind])
            self.collected_paths = keep.save(None, save_dir, self.class_names, session_id=self.session_id, pr=self.pr,
                                             record_start=self.record_num)
            self.record_num += len(keep)
            if self.near_misses is not None:
                stems = [os.path.splitext(os.path.basename(p))[0] for p in files]
                self.collected_paths += self.near_misses.save(None, os.path.join(save_dir, 'near_miss'), self.class_names, names=stems,
                                                              pr=self.pr)
        return det

    def _collect_options(self):
        return dict(tolerance_s=getattr(self, 'tolerance_s', None), mine_peaks=getattr(self, 'mine_peaks', 0) or 0,
                    min_peak_score=getattr(self, 'min_peak_score', 0.0) or 0.0)

    def run_sweep(self):
        """--sweep: the (S, L) table of miss rate and false alarms per hour, and the chosen point under --max_fa_per_hour"""
        sens = parse_sensitivities(getattr(self, 'sensitivities', None) or str(self.sensitivity))
        levels = parse_trigger_levels(getattr(self, 'trigger_levels', None) or str(self.trigger_level))
        synth_from = getattr(self, 'synth_from', None)
        if synth_from:
            res = self.sweep_synth(synth_from, sens, levels, noise_path=getattr(self, 'noise_path', None),
                                   recordings=getattr(self, 'synth_recordings', 8), seconds=getattr(self, 'synth_seconds', 600),
                                   gap_s=parse_gap(getattr(self, 'synth_gap_s', None) or '1.0,3.0'), snr=getattr(self, 'synth_snr', None),
                                   seed=getattr(self, 'synth_seed', 0), save_dir=getattr(self, 'synth_save_dir', None),
                                   tolerance_s=getattr(self, 'tolerance_s', None))
            # the names SynthSet.save gives the recordings; their events and the sweep's tolerance go to collect_wav below
            files = ['synth_%d.wav' % r for r in range(len(res.seconds))]
            labels = dict(zip(files, self.synth_set.events))
            options = dict(self._collect_options(), tolerance_s=self.synth_tolerance_s)
        else:
            paths = self.input_wav
            if os.path.isdir(paths):
                paths = sorted(os.path.join(paths, n) for n in os.listdir(paths) if n.lower().endswith('.wav'))
            files = [paths] if isinstance(paths, str) else paths
            labels, options = getattr(self, 'labels_path', None), self._collect_options()
            res = self.sweep_wav(files, labels, sens, levels, tolerance_s=getattr(self, 'tolerance_s', None))
        miss, fa = res.det()
        print('%d files, %.1f s, %d events; miss rate / false alarms per hour' % (len(files), sum(res.seconds), sum(res.n_events)))
        print('%11s' % 'sensitivity' + ''.join('%18s' % ('level %d' % l) for l in levels))
        for s, v in enumerate(sens):
            print('%11.4f' % v + ''.join('%9.4f /%7.2f' % (miss[s, l], fa[s, l]) for l in range(len(levels))))
        budget = getattr(self, 'max_fa_per_hour', None)
        best = None if budget is None else res.best(max_fa_per_hour=budget)
        if budget is not None:
            if best is None:
                print('no operating point stays within %g false alarms per hour' % budget)
            else:
                print('chosen: sensitivity %.4f, trigger_level %d (miss rate %.4f, %.2f false alarms per hour)'
                      % (best['sensitivity'], best['trigger_level'], best['miss_rate'], best['fa_per_hour']))
        if getattr(self, 'sweep_out', None):
            nan = lambda a: [[None if v != v else float(v) for v in row] for row in a]          # noqa: E731  (JSON has no NaN)
            with open(self.sweep_out, 'w') as f:
                json.dump({"files": files, "seconds": res.seconds, "n_events": res.n_events, "sensitivities": sens, "trigger_levels": levels,
                           "miss_rate": nan(miss), "fa_per_hour": nan(fa), "max_fa_per_hour": budget, "chosen": best}, f, indent=1)
                f.write("\n")
        if self.save_dir and (budget is None or best is not None):
            # the clips of the chosen point (without a budget: the listener's own), from the scan the sweep made
            point = {} if best is None else dict(sensitivity=best['sensitivity'], trigger_level=best['trigger_level'])
            self.collect_wav(files, labels, scan=(self.sweep_scan, self.sweep_lengths), **point, **options)
            print('saved %d clips under %s' % (len(self.collected_paths), self.save_dir))
        return res

    def run(self):
        if (self.input_wav or getattr(self, 'synth_from', None)) and getattr(self, 'sweep', False):
            return self.run_sweep()
        if self.input_wav and self.scan:
            paths = self.input_wav
            if os.path.isdir(paths):
                paths = sorted(os.path.join(paths, n) for n in os.listdir(paths) if n.lower().endswith('.wav'))
            files = [paths] if isinstance(paths, str) else paths
            results = self.scan_wav(files, quiet=True)
            for path, rows, times in zip(files, results, self.scan_times):
                hits = [i for i, _, f in rows if f]
                print('%s: %d chunks, %d activations' % (path, len(rows), len(hits)))
                for t, i in zip(times, hits):
                    print('  %9.3f s  %s' % (t, self.names_for(path)[i]))
            if self.save_dir:
                self.collect_wav(files, getattr(self, 'labels_path', None), scan=self.last_scan, **self._collect_options())
                print('saved %d clips under %s' % (len(self.collected_paths), self.save_dir))
            return results
        if self.input_wav:
            return self.run_wav()
        return self.run_microphone()


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='keyword detection on a wav file (MI355X path)')
    parser.add_argument('--model_path', type=str, default=None, help='.npz weights written by classifier.model')
    parser.add_argument('--quantized_path', type=str, default=None,
                        help='stream with an int8 model written by eval.py --save_quantized (instead of, or beside, --model_path)')
    parser.add_argument('--model_type', type=str, default=default_config['model_type'])
    parser.add_argument('--rnn_layers', type=int, default=default_config['rnn_layers'], help="recurrent layers of simple_gru / simple_lstm, 1..4 (the reference's num_layers); the CNN types take 1 only, default=%(default)s")
    parser.add_argument('--classes_path', type=str, default=default_config['classes_path'])
    parser.add_argument('--params_path', type=str, default=None)
    parser.add_argument('--chunk_size', type=int, default=1024)
    parser.add_argument('--sensitivity', type=float, default=0.5)
    parser.add_argument('--trigger_level', type=int, default=3)
    parser.add_argument('--input_wav', type=str, default=None,
                        help='a wav file; with --scan also a directory of *.wav (required unless --synth_from is given)')
    parser.add_argument('--scan', action='store_true',
                        help='offline scan: the whole recording(s) at once instead of chunk by chunk; prints every activation with its time')
    parser.add_argument('--scan_tile', type=int, default=default_config['scan_tile'], help='windows per forward launch of --scan')
    parser.add_argument('--resample', action='store_true',
                        help='accept mono 16-bit wavs at other sample rates (a quarter to four times the model\'s): they are converted on the '
                             'device first, and chunks, times and labels then count converted samples')
    parser.add_argument('--head_bank', type=str, default=None,
                        help='--scan / --sweep: a kws_amd.transfer.HeadBank (.npz, HeadBank.save); every recording is scored by the '
                             'backbone of --model_path and its own head of the bank')
    parser.add_argument('--head_map', type=str, default=None,
                        help='--head_bank: text file, one line per recording: wav_name head_name (a name of the bank or a head id; '
                             'recordings it does not mention use head 0)')
    parser.add_argument('--sweep', action='store_true',
                        help='scan the recording(s) once and evaluate the detector at every (sensitivity, trigger level) of a grid')
    parser.add_argument('--labels_path', type=str, default=None,
                        help='--sweep (and --scan with --save_dir): text file, one event per line: wav_name class_name start_seconds end_seconds (# comments)')
    parser.add_argument('--sensitivities', type=str, default=None, help='--sweep: a,b,c or lo:hi:n (default: --sensitivity alone)')
    parser.add_argument('--trigger_levels', type=str, default=None, help='--sweep: 1,2,3,... (default: --trigger_level alone)')
    parser.add_argument('--tolerance_s', type=float, default=None,
                        help='--sweep: seconds after an event\'s end in which a detection still counts for it (default: the buffer length)')
    parser.add_argument('--max_fa_per_hour', type=float, default=None,
                        help='--sweep: report the point with the lowest miss rate within this many false alarms per hour')
    parser.add_argument('--sweep_out', type=str, default=None, help='--sweep: write the table and the chosen point to this JSON file')
    parser.add_argument('--save_dir', type=str, default=None,
                        help='folder to save false positives: the audio buffer of every activation, as <class>/<session>_<n>.wav; '
                             'with --scan / --sweep all files are collected in one pass (with --sweep at the chosen point)')
    parser.add_argument('--save_kind', type=str, default='false_alarms', choices=sorted(SAVE_KINDS),
                        help='--scan / --sweep with --labels_path: which activations --save_dir keeps (without labels: all)')
    parser.add_argument('--mine_peaks', type=int, default=0,
                        help='--scan / --sweep with --save_dir: also save the K best well-separated non-background chunks of every file '
                             '(1..64), fired or not, under <save_dir>/near_miss/<class>/; with labels outside the event windows')
    parser.add_argument('--min_peak_score', type=float, default=0.0, help='--mine_peaks: only chunks scoring above this')
    parser.add_argument('--synth_from', type=str, default=None,
                        help='--sweep without recordings: synthesize labelled ones on the device from this dataset folder (one folder of '
                             'one-second clips per class, as train.py reads it) and sweep those')
    parser.add_argument('--noise_path', type=str, default=None, help='--synth_from: folder (or file) of background wavs; default: a silent bed')
    parser.add_argument('--synth_recordings', type=int, default=8, help='--synth_from: number of recordings')
    parser.add_argument('--synth_seconds', type=float, default=600.0, help='--synth_from: length of every recording')
    parser.add_argument('--synth_gap_s', type=str, default='1.0,3.0', help='--synth_from: LO,HI seconds of pause in front of every clip')
    parser.add_argument('--synth_snr', type=str, default=None,
                        help='--synth_from: dB values, a,b,c: every clip is scaled to one of them against the noise under it (default: clips as they are)')
    parser.add_argument('--synth_seed', type=int, default=0)
    parser.add_argument('--synth_save_dir', type=str, default=None, help='--synth_from: also write the recordings and labels.txt here')
    args = parser.parse_args(argv)
    if not args.model_path and not args.quantized_path:
        parser.error('one of --model_path and --quantized_path is required')
    if args.rnn_layers != 1 and args.model_type not in ('simple_gru', 'simple_lstm'):
        parser.error('--rnn_layers %d does not apply to %s: only simple_gru / simple_lstm stack layers' % (args.rnn_layers, args.model_type))
    if not args.input_wav and not args.synth_from:
        parser.error('one of --input_wav and --synth_from is required')
    if args.synth_from and not args.sweep:
        parser.error('--synth_from goes with --sweep')
    if args.head_bank and not (args.scan or args.sweep):
        parser.error('--head_bank goes with --scan or --sweep')
    if args.head_bank and (args.quantized_path or args.synth_from):
        parser.error('--head_bank goes with neither --quantized_path nor --synth_from')
    if args.head_map and not args.head_bank:
        parser.error('--head_map goes with --head_bank')
    if args.synth_from:
        try:
            parse_gap(args.synth_gap_s)
        except ValueError as e:
            parser.error('--synth_gap_s: %s' % e)
    return args


def main():
    Listener(**vars(parse_args())).run()


if __name__ == '__main__':
    main()
