"""CPU tests of the background-noise augmentation surface: argument checks without a device, the raw-audio dataset loader, the noise
bank loader, train.py's command line and the new C-ABI declarations."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf-keras-speech-commands_amd")


def test_wave_augment_argument_errors_need_no_device():
    from kws_amd.augment import NoiseBank, WaveAugment
    noise = [np.zeros(100, np.float32) + 0.1]
    for kw in (dict(noised_rate=-0.1), dict(noised_rate=1.5), dict(snr=()), dict(snr=[1] * 17), dict(snr=[float("nan")]),
               dict(time_shift_ms=-1)):
        with pytest.raises(ValueError):
            WaveAugment(noise, **kw)
    with pytest.raises(ValueError):
        NoiseBank([])
    with pytest.raises(ValueError):
        NoiseBank([np.zeros(0, np.float32)])
    with pytest.raises(ValueError):
        NoiseBank([np.zeros((2, 3), np.float32)])
    with pytest.raises(TypeError):
        NoiseBank([np.zeros(4, np.int32)])
    a = WaveAugment(noise, snr="5,10,20", noised_rate=0.5, time_shift_ms=100, seed=3)
    assert a.snr == [5.0, 10.0, 20.0] and a.max_shift == 1600 and a.seed == 3
    mixed = NoiseBank([np.ones(3, np.int16) * 16384, np.ones(2, np.float32)])
    np.testing.assert_array_equal(mixed.as_float32(), [0.5, 0.5, 0.5, 1.0, 1.0])
    assert list(mixed.seg_len) == [3, 2]


def test_white_noise_segment():
    from kws_amd.augment import white_noise
    w = white_noise(500, 16000, 0.7, seed=1)
    assert w.dtype == np.int16 and w.shape == (8000,)
    assert np.abs(w).max() <= 2 ** 11 and w.std() > 100


def _write_dataset(tmp_path, lengths_by_class):
    from common.data_utils import save_audio
    rng = np.random.default_rng(0)
    for cls, lens in lengths_by_class.items():
        d = tmp_path / "sounds" / cls
        d.mkdir(parents=True)
        for i, n in enumerate(lens):
            save_audio(str(d / ("%s_%d.wav" % (cls, i))), 0.3 * rng.uniform(-1, 1, n))


def test_get_audio_dataset_layout_lengths_labels_and_split(tmp_path):
    from classifier.data import get_audio_dataset, load_audio_samples
    from classifier.params import pr
    from common.data_utils import load_wav
    classes = ["background", "yes", "no"]
    _write_dataset(tmp_path, {"background": [16000, 20000], "yes": [8000, 16000, 3000], "no": [12345]})
    x, lens, y, xv, lv, yv = get_audio_dataset(str(tmp_path), classes)
    assert xv is None and lv is None and yv is None
    assert x.shape == (6, pr.max_samples) and x.dtype == np.float32 and lens.dtype == np.int32
    assert sorted(lens.tolist()) == sorted([16000, 16000, 8000, 16000, 3000, 12345])
    assert sorted(y.tolist()) == [0, 0, 1, 1, 1, 2]
    # head-aligned: the first L samples are the file's head, zeros after
    _, _, words = load_audio_samples(str(tmp_path / "sounds"), classes)
    short = int(np.argmin(lens))
    assert lens[short] == 3000 and y[short] == 1
    f = sorted((tmp_path / "sounds" / "yes").glob("*.wav"))[2]
    np.testing.assert_array_equal(x[short, :3000], load_wav(str(f)))
    assert not x[short, 3000:].any()
    for yi, w in zip(y, words):
        assert classes[yi] == w
    np.random.seed(0)
    xt, lt, yt, xv, lv, yv = get_audio_dataset(str(tmp_path), classes, val_split=0.3)
    assert len(xv) == 2 and len(xt) == 4 and len(lv) == 2 and len(yt) == 4
    assert sorted(np.concatenate([lt, lv]).tolist()) == sorted(lens.tolist())
    # rows and lengths stay paired through the split
    for xs, ls in ((xt, lt), (xv, lv)):
        for r, n in zip(xs, ls):
            assert not r[n:].any()


def test_load_noise_bank(tmp_path):
    from classifier.data import load_noise_bank
    from common.data_utils import save_audio
    (tmp_path / "noise" / "sub").mkdir(parents=True)
    save_audio(str(tmp_path / "noise" / "b.wav"), np.full(500, 0.25))
    save_audio(str(tmp_path / "noise" / "sub" / "a.wav"), np.full(300, -0.5))
    bank = load_noise_bank(str(tmp_path / "noise"))
    assert [len(a) for a in bank] == [500, 300] and all(a.dtype == np.float32 for a in bank)
    assert abs(float(bank[1][0]) + 0.5) < 1e-4
    assert [len(a) for a in load_noise_bank(str(tmp_path / "noise" / "b.wav"))] == [500]
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError):
        load_noise_bank(str(tmp_path / "empty"))
    from kws_amd.augment import NoiseBank
    nb = NoiseBank(str(tmp_path / "noise"))
    assert list(nb.seg_len) == [500, 300]


def test_train_help_lists_reference_and_new_flags():
    env = dict(os.environ)
    out = subprocess.run([sys.executable, os.path.join(PKG, "train.py"), "--help"], capture_output=True, text=True, env=env, cwd=PKG,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    for flag in ("--model_type", "--weights_path", "--train_data_path", "--val_data_path", "--val_split", "--classes_path", "--params_path",
                 "--background_bias", "--batch_size", "--optimizer", "--learning_rate", "--decay_type", "--epochs",
                 "--raw_audio", "--noise_path", "--snr", "--noised_rate", "--time_shift_ms"):
        assert flag in out.stdout, flag


def test_augment_symbols_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "kws.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(kws_[a-z0-9_]+)\s*\(", text))
    new = {"kws_noise_bank_create", "kws_noise_bank_destroy", "kws_noise_bank_info", "kws_augment_plan", "kws_augment_apply",
           "kws_featurize_gather_augmented"}
    assert new <= declared
    assert "kws_augment_params" in text and "kws_aug_clip" in text
    from kws_amd import get_lib
    L = get_lib()
    for n in new:
        assert hasattr(L, n)


def test_augment_record_layout_matches_ctypes():
    import ctypes
    from kws_amd import lib as l
    from kws_amd.augment import CLIP_DTYPE
    assert ctypes.sizeof(l.KwsAugClip) == CLIP_DTYPE.itemsize == 32
    assert ctypes.sizeof(l.KwsAugmentParams) == 88


def test_invalid_plan_arguments_are_reported_host_side():
    """argument checks of kws_augment_plan run before any device work: a NULL bank / a bad rate are KWS_ERR_INVALID without a GPU"""
    import ctypes
    from kws_amd import lib as l
    L = l.get_lib()
    p = l.KwsAugmentParams()
    p.noised_rate, p.n_snr, p.max_samples = 0.5, 1, 16000
    rc = L.kws_augment_plan(None, ctypes.byref(p), None, 0, None, 0, 16000, None, 0, 0, None, None, None)
    assert rc == l.ERR_INVALID
    rc = L.kws_noise_bank_create(None, 0, None, 0, ctypes.byref(ctypes.c_void_p()))
    assert rc == l.ERR_INVALID
    seg = (ctypes.c_int32 * 1)(4)
    x = (ctypes.c_float * 4)()
    rc = L.kws_noise_bank_create(ctypes.cast(x, ctypes.c_void_p), 0, ctypes.cast(seg, ctypes.c_void_p), 0, ctypes.byref(ctypes.c_void_p()))
    assert rc == l.ERR_INVALID and b"at least one segment" in L.kws_last_error()


def test_snr_outside_200_db_is_refused_host_side():
    """An SNR outside [-200, 200] dB is KWS_ERR_INVALID in kws_augment_params and in explicit records alike, and a ValueError in
    WaveAugment: beyond it the float32 gain can overflow (tests/test_speed_mix_edges_host.py).  The checks need no bank, so a NULL one
    shows which values pass: they get as far as "null noise bank"."""
    import ctypes
    from kws_amd import lib as l
    from kws_amd.augment import CLIP_DTYPE, WaveAugment
    noise = [np.zeros(100, np.float32) + 0.1]
    assert WaveAugment(noise, snr=[-200, 200]).snr == [-200.0, 200.0]
    for bad, entry in (([-200.5], 0), ([0, 201], 1), ([5, 10, 1e30], 2), ([-700], 0), ([float("inf")], 0), ([float("nan")], 0)):
        with pytest.raises(ValueError, match="SNR %d " % entry):
            WaveAugment(noise, snr=bad)
    L = l.get_lib()
    wav = np.zeros((2, 8), np.float32)
    plan = np.zeros(2, CLIP_DTYPE)

    def call(snrs, explicit=None):
        p = l.KwsAugmentParams()
        p.noised_rate, p.n_snr, p.max_samples = 0.5, len(snrs), 8
        for i, s in enumerate(snrs):
            p.snr_db[i] = s
        rc = L.kws_augment_plan(None, ctypes.byref(p), wav.ctypes.data, l.WAV_F32, None, 2, 8, None, 0, 0, plan.ctypes.data,
                                None if explicit is None else explicit.ctypes.data, None)
        return rc, L.kws_last_error().decode()

    for ok in ([-200.0, 200.0], [0.0], [199.99]):
        rc, msg = call(ok)
        assert rc == l.ERR_INVALID and msg == "null noise bank", (ok, msg)
    for bad, entry in (([-200.5], 0), ([0.0, 201.0], 1), ([5.0, 10.0, 1e30], 2), ([-700.0], 0), ([float("inf")], 0), ([float("nan")], 0)):
        rc, msg = call(bad)
        assert rc == l.ERR_INVALID and msg.startswith("SNR %d " % entry) and "[-200, 200]" in msg, (bad, msg)
    for s, accepted in ((-200.0, True), (200.0, True), (-200.5, False), (201.0, False), (-700.0, False), (3e38, False),
                        (float("nan"), False)):
        ex = np.zeros(2, CLIP_DTYPE)
        ex["snr_db"][1] = s
        rc, msg = call([0.0], ex)
        assert rc == l.ERR_INVALID
        assert msg == "null noise bank" if accepted else (msg.startswith("clip 1: SNR") and "[-200, 200]" in msg), (s, msg)
