"""CPU tests of the voice-activity detector's host side: the float64 restatement (tests/vad_ref.py) against the reference's own
results (tests/golden/vad_golden.npz), window counts, band bins, refused sample rates, the C-ABI surface and the tools' parsers."""
import importlib
import os
import re
import sys

import numpy as np
import pytest

import vad_cases
import vad_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tf-keras-speech-commands_amd", "tools", "audio_process")


@pytest.fixture(scope="module")
def vad_golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "vad_golden.npz"))


def _tool(name):
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)
    return importlib.import_module(name)


def test_restatement_reproduces_the_reference(vad_golden):
    g = vad_golden
    assert int(g["n"]) >= 4
    for i in range(int(g["n"])):
        rate, x = int(g["rate_%d" % i]), g["x_%d" % i]
        N, H, _, _, _ = vad_ref.geometry(rate)
        d = vad_ref.detect(x, rate)
        win = g["windows_%d" % i]
        assert win.shape[0] == vad_ref.n_windows(x.size, N, H)
        assert np.array_equal(win[:, 0], np.arange(win.shape[0]) * float(H))
        assert np.array_equal(win[:, 1].astype(np.uint8), d["smoothed"])
        assert [tuple(v) for v in g["intervals_%d" % i].tolist()] == d["intervals"]
        assert [(b / rate, e / rate) for b, e in d["intervals"]] == [tuple(v) for v in g["seconds_%d" % i].tolist()]
        want = float(g["energy_%d" % i])
        assert abs(vad_ref.energy_per_second(x, rate) - want) <= 1e-12 * want


@pytest.mark.parametrize("rate", [8000, 16000, 32000, 48000])
def test_window_counts_and_band(rate):
    from kws_amd.vad import Vad
    v = Vad(rate)
    N, H = int(rate * 0.02), int(rate * 0.01)
    assert (v.window_samples, v.hop_samples, v.median) == (N, H, 25)
    assert (v.bin_lo, v.bin_hi) == (7, 59)
    assert vad_ref.geometry(rate) == (N, H, 7, 59, 25)
    for L, want in ((0, 0), (N, 0), (N + 1, 1), (N + H, 1), (N + H + 1, 2)):
        assert v.n_windows(L) == want == vad_ref.n_windows(L, N, H)


def test_44100_is_supported_and_22050_refused():
    import kws_amd
    from kws_amd.vad import Vad
    v = Vad(44100)
    assert (v.window_samples, v.hop_samples, v.bin_lo, v.bin_hi) == (882, 441, 7, 59)
    with pytest.raises(kws_amd.KwsError) as e:
        Vad(22050)
    assert e.value.code == -2 and "window == 2 * hop" in str(e.value) and "22050" in str(e.value)
    with pytest.raises(kws_amd.KwsError) as e:
        Vad(96000)                                   # N = 1920 > 1024
    assert e.value.code == -2


def test_symbols_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "kws.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    from kws_amd import get_lib
    L = get_lib()
    for n in ("kws_vad_create", "kws_vad_destroy", "kws_vad_info", "kws_vad_windows", "kws_vad_workspace_bytes", "kws_vad_detect",
              "kws_vad_gather_clips"):
        assert re.search(r"\b%s\s*\(" % n, text), n + " is not declared in include/kws.h"
        assert hasattr(L, n), "libkws_hip.so does not export " + n


def test_argument_errors_are_reported():
    import ctypes
    from kws_amd import lib as l
    L = l.get_lib()
    h = ctypes.c_void_p()
    assert L.kws_vad_create(16000, 0.02, 0.01, 3000.0, 300.0, 0.6, 0.5, ctypes.byref(h)) == -1
    assert b"band" in L.kws_last_error()
    assert L.kws_vad_gather_clips(None, l.WAV_I16, 1, 16, None, None, 1, 0, 0, 0, 0, None, None) == -1
    assert b"clip_samples" in L.kws_last_error()
    assert L.kws_vad_gather_clips(None, l.WAV_I16, 1, 16, None, None, 1, 8, 0, 0, 7, None, None) == -1
    assert b"alignment" in L.kws_last_error()


def test_tools_parse_their_arguments():
    sd, sc, sp = _tool("speech_duration_check"), _tool("silent_check"), _tool("vad_split")
    a = sd.build_parser().parse_args(["--wav_path", "x", "--vad_type", "simple", "--json", "o.json"])
    assert (a.wav_path, a.vad_type, a.json) == ("x", "simple", "o.json")
    a = sc.build_parser().parse_args(["--wav_path", "x", "--target_path", "t"])
    assert a.threshold == 0.2 and a.target_path == "t"
    a = sp.build_parser().parse_args(["--wav_path", "x", "--output_path", "o", "--clip_length", "1.5", "--pad_before", "0.1",
                                      "--pad_after", "0.2"])
    assert (a.clip_length, a.pad_before, a.pad_after, a.align) == (1.5, 0.1, 0.2, "left")
    with pytest.raises(ValueError, match="Unsupported VAD type"):
        sd.speech_durations("x", "webrtc")
    with pytest.raises(ValueError, match="Unsupported VAD type"):
        sd.main(["--wav_path", "x", "--vad_type", "webrtc"])


def test_gpu_test_inputs_stay_within_the_near_threshold_cap():
    """tests/test_vad_gpu.py may set aside at most 0.5 % of its windows as near-ties: at 1e-4, far above its bound, none is"""
    total = near = 0
    for x in vad_cases.recordings():
        r = vad_ref.ratios(x, vad_cases.RATE)
        total += r.size
        near += int((np.abs(r - 0.6) <= 1e-4).sum())
    assert total == 715 and near <= 0.005 * total
