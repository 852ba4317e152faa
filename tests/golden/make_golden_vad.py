"""Regenerates tests/golden/vad_golden.npz from the reference's VoiceActivityDetector (tools/audio_process/speech_duration_check.py).

    python tests/golden/make_golden_vad.py /path/to/reference

The reference module imports packages this project does not need (webrtcvad, matplotlib), so only the class's own AST node is
compiled, with numpy in its namespace, and `rate` / `data` are filled on an instance made with object.__new__.  The fixture holds
arrays only: int16 inputs (synthetic signals and two of the reference's example/*.wav as PCM), the detected_windows the class
returns, its interval lists in samples, and the energy per second of tools/audio_process/silent_check.py:17-18 evaluated in
float64 (its loader is not available here; the formula is sum((x / 32768)^2) / (len / rate)).
"""
import ast
import os
import sys
import wave

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def load_class(ref):
    path = os.path.join(ref, "tools", "audio_process", "speech_duration_check.py")
    tree = ast.parse(open(path).read())
    node = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "VoiceActivityDetector"][0]
    ns = {"np": np}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return ns["VoiceActivityDetector"]


def tone(rate, n, freqs, amp):
    t = np.arange(n) / rate
    return amp * sum(np.sin(2 * np.pi * f * t + i) for i, f in enumerate(freqs)) / len(freqs)


def signals(ref):
    rng = np.random.default_rng(2024)
    out = []
    for rate, secs in ((16000, 2.5), (8000, 3.0), (16000, 1.0)):
        n = int(rate * secs) + 37
        x = rng.normal(0, 300, n)
        for k in range(int(secs * 2)):
            if k % 2 == 1:
                a, b = int(k * 0.5 * rate), int((k * 0.5 + 0.35) * rate)
                x[a:b] += tone(rate, b - a, (700 + 150 * k, 1900), 6000)
        if secs == 1.0:
            x[-4000:] += tone(rate, 4000, (1000,), 8000)          # runs to the last sample: the open interval is dropped
        out.append((rate, np.clip(np.round(x), -32768, 32767).astype(np.int16)))
    for name in ("down_1.wav", "left_2.wav"):
        with wave.open(os.path.join(ref, "example", name), "rb") as wf:
            assert wf.getnchannels() == 1 and wf.getsampwidth() == 2
            out.append((wf.getframerate(), np.frombuffer(wf.readframes(wf.getnframes()), dtype="<i2").copy()))
    return out


def main():
    ref = sys.argv[1]
    cls = load_class(ref)
    arrays = {}
    sigs = signals(ref)
    for i, (rate, x) in enumerate(sigs):
        v = object.__new__(cls)
        v.rate, v.data, v.channels = rate, x, 1
        v.sample_window, v.sample_overlap, v.speech_window = 0.02, 0.01, 0.5
        v.speech_energy_threshold, v.speech_start_band, v.speech_end_band = 0.6, 300, 3000
        win = v.detect_speech()
        labels = v.convert_windows_to_readable_labels(win)
        iv = np.array([[round(l["speech_begin"] * rate), round(l["speech_end"] * rate)] for l in labels], dtype=np.int64).reshape(-1, 2)
        xf = x.astype(np.float64) / 32768.0
        arrays["rate_%d" % i] = np.int64(rate)
        arrays["x_%d" % i] = x
        arrays["windows_%d" % i] = win.astype(np.float64)
        arrays["intervals_%d" % i] = iv
        arrays["seconds_%d" % i] = np.array([[l["speech_begin"], l["speech_end"]] for l in labels], dtype=np.float64).reshape(-1, 2)
        arrays["energy_%d" % i] = np.float64(np.sum(xf * xf) / (len(xf) / rate))
    arrays["n"] = np.int64(len(sigs))
    np.savez_compressed(os.path.join(HERE, "vad_golden.npz"), **arrays)


if __name__ == "__main__":
    main()
