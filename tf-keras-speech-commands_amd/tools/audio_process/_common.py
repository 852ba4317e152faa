"""Shared by the audio_process tools: load a wav file or a directory of them, grouped by sample rate, so that every group
is packed once and goes through one Vad.detect call."""
import glob
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from kws_amd.vad import Vad, read_wav  # noqa: E402


def wav_files(path):
    return [path] if os.path.isfile(path) else sorted(glob.glob(os.path.join(path, "*.wav")))


def detect_all(paths):
    """-> [(rate, [path], [int16 samples], VadResult, Vad)], one entry per sample rate met"""
    by_rate = {}
    for p in paths:
        data, rate = read_wav(p)
        by_rate.setdefault(rate, ([], []))
        by_rate[rate][0].append(p)
        by_rate[rate][1].append(data)
    out = []
    for rate, (names, datas) in sorted(by_rate.items()):
        vad = Vad(rate)
        out.append((rate, names, datas, vad.detect(datas), vad))
    return out
