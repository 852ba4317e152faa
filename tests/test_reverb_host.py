"""CPU tests of the room-reverberation surface: RirBank input handling, the room model of simulate_rirs / shoebox_rir, WaveAugment and
train.py arguments, and the new C-ABI declarations."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf-keras-speech-commands_amd")


def test_rir_bank_argument_errors_need_no_device():
    from kws_amd.augment import RirBank
    with pytest.raises(ValueError):
        RirBank([])
    with pytest.raises(ValueError):
        RirBank([np.zeros(0, np.float32)])
    with pytest.raises(ValueError):
        RirBank([np.zeros((2, 3), np.float32)])
    with pytest.raises(ValueError):
        RirBank([np.array([0.5, np.nan], np.float32)])
    with pytest.raises(ValueError):
        RirBank([np.array([0.5, np.inf])])
    with pytest.raises(ValueError):
        RirBank([np.zeros(4, np.float32)])
    with pytest.raises(TypeError):
        RirBank([np.ones(4, np.int16)])
    with pytest.raises(ValueError):
        RirBank([np.ones(4, np.float32)], max_samples=16385)
    with pytest.raises(ValueError):
        RirBank([np.ones(4, np.float32)], max_samples=0)


def test_rir_bank_peak_alignment_normalisation_and_clipping():
    from kws_amd.augment import RirBank
    h = np.array([0.0, 0.01, -0.02, -0.5, 0.25, 0.125, 0.0625], np.float64)
    bank = RirBank([h, np.array([2.0], np.float32)], max_samples=3)
    np.testing.assert_allclose(bank.taps[0], [1.0, -0.5, -0.25], rtol=0, atol=0)      # starts at argmax|h|, divided by h[peak] = -0.5
    np.testing.assert_array_equal(bank.taps[1], [1.0])
    assert list(bank.rir_len) == [3, 1] and bank.max_samples == 3
    assert all(t.dtype == np.float32 for t in bank.taps)
    long = np.r_[np.zeros(5), 1.0, np.full(20000, 0.001)]
    b2 = RirBank(long)
    assert len(b2) == 1 and b2.rir_len[0] == 16000 and b2.taps[0][0] == 1.0


def test_rir_bank_folder_loading_through_load_wav(tmp_path):
    import wave
    from common.data_utils import save_audio
    from kws_amd.augment import RirBank
    (tmp_path / "rirs" / "sub").mkdir(parents=True)
    save_audio(str(tmp_path / "rirs" / "a.wav"), np.r_[np.zeros(10), 0.5, 0.25, np.zeros(100)])
    # a RIR at 8 kHz: load_wav resamples it to 16 kHz (twice the length)
    x = (np.r_[np.zeros(7), 0.6, 0.3, np.zeros(41)] * 32767).astype("<i2")
    w = wave.open(str(tmp_path / "rirs" / "sub" / "b.wav"), "wb")
    w.setnchannels(1)
    w.setsampwidth(2)
    w.setframerate(8000)
    w.writeframes(x.tobytes())
    w.close()
    bank = RirBank(str(tmp_path / "rirs"))
    assert len(bank) == 2
    assert bank.rir_len[0] == 112 - 10 and abs(float(bank.taps[0][1]) - 0.5) < 1e-3
    assert all(float(t[0]) == 1.0 for t in bank.taps)
    assert bank.rir_len[1] > 60                                     # 100 samples after resampling, trimmed at its peak
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError):
        RirBank(str(tmp_path / "empty"))


def test_simulate_rirs_deterministic_and_seeded():
    from kws_amd.augment import simulate_rirs
    a = simulate_rirs(3, seed=11)
    b = simulate_rirs(3, seed=11)
    c = simulate_rirs(3, seed=12)
    assert len(a) == 3 and all(x.dtype == np.float32 and x.ndim == 1 for x in a)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert any(x.shape != y.shape or not np.array_equal(x, y) for x, y in zip(a, c))
    with pytest.raises(ValueError):
        simulate_rirs(0)
    with pytest.raises(ValueError):
        simulate_rirs(1, rt60=(0.5, 0.3))


def _schroeder_rt60(h, fs):
    e = np.cumsum((np.asarray(h, np.float64) ** 2)[::-1])[::-1]
    db = 10.0 * np.log10(e / e[0])
    i0, i1 = int(np.argmax(db <= -5.0)), int(np.argmax(db <= -35.0))
    slope = np.polyfit(np.arange(i0, i1) / fs, db[i0:i1], 1)[0]
    return -60.0 / slope


def test_simulated_rooms_direct_path_draws_and_decay():
    from kws_amd.augment import SINC_HALF_WIDTH, SPEED_OF_SOUND, simulate_rirs
    fs = 16000
    rirs, geo = simulate_rirs(12, seed=5, rt60=(0.3, 0.7), sample_rate=fs, with_geometry=True)
    for h, g in zip(rirs, geo):
        room, src, mic = g["room"], g["source"], g["mic"]
        assert 0.3 <= g["rt60"] <= 0.7
        assert np.all(room >= [4, 3, 2.6]) and np.all(room <= [6, 4.8, 2.8])
        assert np.all(src >= [0.5, 0.5, 1.6]) and np.all(src <= [room[0] - 0.5, room[1] - 0.5, 1.9])
        assert mic[2] == 0.1 and np.all(mic[:2] >= 0.5) and np.all(mic[:2] <= room[:2] - 0.5)
        pos = np.linalg.norm(src - mic) / SPEED_OF_SOUND * fs + SINC_HALF_WIDTH
        p = int(np.floor(pos))
        # nothing arrives before the direct path, which is the largest tap up to its own arrival
        assert np.all(h[:max(p - SINC_HALF_WIDTH, 0)] == 0)
        assert abs(int(np.argmax(np.abs(h[:p + 2]))) - pos) <= 1.0
        assert np.abs(h).max() >= np.abs(h[:p + 2]).max()
        rt = _schroeder_rt60(h, fs)
        assert abs(rt / g["rt60"] - 1.0) < 0.2, (rt, g["rt60"])


def test_shoebox_rir_explicit_geometry_direct_path_is_largest_and_exact():
    from kws_amd.augment import SINC_HALF_WIDTH, SPEED_OF_SOUND, shoebox_rir
    fs = 16000
    d = 16 * SPEED_OF_SOUND / fs                 # a whole number of samples: the windowed sinc is a unit impulse
    h = shoebox_rir([6.0, 4.8, 2.8], [3.0, 2.4, 1.4], [3.0 + d, 2.4, 1.4], 0.5, fs, np.random.default_rng(0))
    assert int(np.argmax(np.abs(h))) == 16 + SINC_HALF_WIDTH
    assert abs(h[16 + SINC_HALF_WIDTH] * 4 * np.pi * d - 1.0) < 1e-6
    assert abs(_schroeder_rt60(h, fs) / 0.5 - 1.0) < 0.2


def test_wave_augment_reverb_arguments_need_no_device():
    from kws_amd.augment import REVERB_SEED_MIX, RirBank, WaveAugment
    rirs = [np.array([1.0, 0.5], np.float32)]
    with pytest.raises(ValueError):
        WaveAugment(None)
    with pytest.raises(ValueError):
        WaveAugment(None, rirs=rirs, reverb_rate=-0.1)
    with pytest.raises(ValueError):
        WaveAugment(None, rirs=rirs, reverb_rate=1.5)
    a = WaveAugment(None, rirs=rirs, reverb_rate=0.25, rescale=False, seed=7)
    assert a.noise is None and isinstance(a.rirs, RirBank) and a.reverb_rate == 0.25 and a.rescale is False
    assert REVERB_SEED_MIX == 0x9E3779B97F4A7C15 and a.reverb_seed == 7 ^ 0x9E3779B97F4A7C15
    p = a.reverb_params(16000)
    assert p.seed == 7 ^ 0x9E3779B97F4A7C15 and p.max_samples == 16000 and p.rescale == 0 and abs(p.reverb_rate - 0.25) < 1e-7
    b = WaveAugment([np.ones(10, np.float32)], seed=3)
    assert b.rirs is None and b.seed == 3                          # the noise-only form is unchanged


def _train(args):
    return subprocess.run([sys.executable, os.path.join(PKG, "train.py")] + args, capture_output=True, text=True, cwd=ROOT, timeout=300)


def test_train_py_reverb_flags(tmp_path):
    r = _train(["--help"])
    assert r.returncode == 0
    for flag in ("--rir_path", "--simulate_rirs", "--reverb_rate"):
        assert flag in r.stdout
    (tmp_path / "classes.txt").write_text("background\nyes\n")
    base = ["--train_data_path", str(tmp_path), "--classes_path", str(tmp_path / "classes.txt"), "--raw_audio"]
    r = _train(base + ["--reverb_rate", "0.5"])
    assert r.returncode != 0 and "--reverb_rate needs a RIR source" in (r.stderr + r.stdout)
    r = _train(base[:-1] + ["--simulate_rirs", "2"])
    assert r.returncode != 0 and "need --raw_audio" in (r.stderr + r.stdout)


def test_reverb_c_abi_declared_exported_and_validated():
    hdr = open(os.path.join(ROOT, "include", "kws.h")).read()
    for name in ("kws_rir_bank_create", "kws_rir_bank_destroy", "kws_rir_bank_info", "kws_reverb_apply"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
    from kws_amd import lib as _l
    L = _l.get_lib()
    for name in ("kws_rir_bank_create", "kws_rir_bank_destroy", "kws_rir_bank_info", "kws_reverb_apply"):
        assert hasattr(L, name)
    h = ctypes.c_void_p()
    taps = np.ones(4, np.float32)
    for lens, K, ms, code in (([4], 0, 100, _l.ERR_INVALID), ([0], 1, 100, _l.ERR_INVALID), ([4], 1, 0, _l.ERR_INVALID),
                              ([4], 1, 16385, _l.ERR_UNSUPPORTED)):
        ln = np.array(lens, np.int32)
        assert L.kws_rir_bank_create(taps.ctypes.data, ln.ctypes.data, K, ms, ctypes.byref(h)) == code
        assert not h.value
    bad = np.array([1.0, np.nan, 0.0, 0.0], np.float32)
    ln = np.array([4], np.int32)
    assert L.kws_rir_bank_create(bad.ctypes.data, ln.ctypes.data, 1, 100, ctypes.byref(h)) == _l.ERR_INVALID
    assert L.kws_reverb_apply(None, None, None, 0, None, 0, 0, None, 0, 0, None, None, 0, None, None, None) == _l.ERR_INVALID


def test_reverb_params_ctypes_layout_matches_header():
    from kws_amd import lib as _l
    hdr = open(os.path.join(ROOT, "include", "kws.h")).read()
    body = re.search(r"typedef struct kws_reverb_params \{(.*?)\} kws_reverb_params;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(\w+)\s+(\w+);", body, re.M)
    sizes = {"float": 4, "int32_t": 4, "uint64_t": 8}
    assert [n for _, n in fields] == [n for n, _ in _l.KwsReverbParams._fields_]
    off = 0
    for (ty, n), (cn, _) in zip(fields, _l.KwsReverbParams._fields_):
        off = (off + sizes[ty] - 1) // sizes[ty] * sizes[ty]
        assert getattr(_l.KwsReverbParams, cn).offset == off, n
        off += sizes[ty]
    assert ctypes.sizeof(_l.KwsReverbParams) == 24 == off
