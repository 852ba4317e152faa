"""CPU tests of the Butterworth filter augmentation surface: butter_sos against scipy's design, the tests' float64 filtfilt restatement
against scipy.signal.filtfilt (the reference's call), FilterBank / random_filters / WaveAugment argument handling and train.py's flags."""
import os
import subprocess
import sys

import numpy as np
import pytest

from filter_ref import filtfilt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf-keras-speech-commands_amd")
FS = 16000.0


def _designs():
    for btype in ("lowpass", "highpass"):
        for order in range(1, 9):
            for f in (50.0, 300.0, 2000.0, 7500.0):
                yield btype, order, f
    for btype in ("bandpass", "bandstop"):
        for order in range(1, 5):
            for f in ((50.0, 300.0), (300.0, 3400.0), (1000.0, 1260.0), (2000.0, 7500.0), (50.0, 7500.0)):
                yield btype, order, f


def test_butter_sos_matches_scipy_frequency_response():
    signal = pytest.importorskip("scipy.signal")
    from kws_amd.augment import butter_sos
    w = np.linspace(0.0, np.pi, 4096)
    n = 0
    for btype, order, f in _designs():
        wn = 2.0 * np.asarray(f) / FS
        got = butter_sos(order, wn, btype)
        want = signal.butter(order, wn, btype, output="sos")
        assert got.shape == want.shape, (btype, order, f)
        _, hg = signal.sosfreqz(got, worN=w)
        _, hw = signal.sosfreqz(want, worN=w)
        err = np.abs(hg - hw).max()
        assert err <= 1e-9, (btype, order, f, err)
        n += 1
    assert n == 2 * 8 * 4 + 2 * 4 * 5


def test_filtfilt_restatement_matches_scipy_filtfilt():
    signal = pytest.importorskip("scipy.signal")
    from kws_amd.augment import butter_sos, filter_padlen
    rng = np.random.default_rng(0)
    x = rng.standard_normal(3000)
    x[:200] += 2.0                                              # a step at the start and a ramp at the end exercise the edges
    x[-300:] += np.linspace(0, 3, 300)
    for btype, order, f in (("lowpass", 4, 2000.0), ("highpass", 4, 300.0), ("bandpass", 4, (300.0, 3400.0)),
                            ("bandstop", 2, (900.0, 1130.0)), ("lowpass", 3, 5000.0), ("highpass", 8, 1000.0), ("bandpass", 1, (500.0, 4000.0))):
        wn = 2.0 * np.asarray(f) / FS
        b, a = signal.butter(order, wn, btype)
        want = signal.filtfilt(b, a, x)                         # tools/audio_process/wav_filter.py's exact call
        got = filtfilt(butter_sos(order, wn, btype), x, filter_padlen(order, btype))
        assert filter_padlen(order, btype) == 3 * max(len(a), len(b))
        assert got.shape == x.shape
        err = np.abs(got - want).max() / np.abs(x).max()
        assert err <= 1e-9, (btype, order, f, err)


def test_butter_sos_and_filter_bank_validation():
    from kws_amd.augment import FilterBank, butter_sos
    with pytest.raises(ValueError):
        butter_sos(4, 0.5, "allpass")
    with pytest.raises(ValueError):
        butter_sos(4, 1.0, "lowpass")
    with pytest.raises(ValueError):
        butter_sos(4, (0.5, 0.2), "bandpass")
    with pytest.raises(ValueError):
        butter_sos(0, 0.5, "lowpass")
    bad = [("notch", 4, 1000.0),                   # bad type
           ("lowpass", 9, 1000.0),                 # 5 sections
           ("bandpass", 5, (300.0, 3000.0)),       # 5 sections
           ("bandstop", 5, (300.0, 3000.0)),
           ("lowpass", 0, 1000.0),
           ("lowpass", 2.5, 1000.0),
           ("lowpass", 4, 8000.0),                 # at Nyquist
           ("highpass", 4, 9000.0),                # above
           ("highpass", 4, 0.0),
           ("bandpass", 4, (300.0, 8000.0)),
           ("bandpass", 4, (3000.0, 3000.0)),      # low >= high
           ("bandstop", 4, (3000.0, 300.0)),
           ("bandpass", 4, 1000.0),                # one frequency for a band
           ("lowpass", 4, (300.0, 3000.0))]        # a band for a cutoff
    for spec in bad:
        with pytest.raises(ValueError):
            FilterBank([spec])
    with pytest.raises(ValueError):
        FilterBank([])
    fb = FilterBank([("lowpass", 8, 3000.0), ("bandpass", 4, (300, 3400)), ("highpass", 1, 100.0), ("bandstop", 2, (900, 1100))])
    assert len(fb) == 4 and fb.n_sections == 4 and fb.table.shape == (4, 4, 6)
    assert list(fb.padlen) == [27, 27, 6, 15]
    np.testing.assert_array_equal(fb.table[2, 1:], np.tile([1.0, 0, 0, 1.0, 0, 0], (3, 1)))   # identity sections pad order 1
    one = FilterBank(("lowpass", 4, 1000.0))
    assert len(one) == 1 and one.n_sections == 2


def test_wave_augment_filter_arguments():
    from kws_amd.augment import FilterBank, WaveAugment
    with pytest.raises(ValueError, match="WaveAugment needs a noise bank, a RIR bank or both"):
        WaveAugment(None)
    for rate in (-0.1, 1.5):
        with pytest.raises(ValueError):
            WaveAugment(None, filters=[("lowpass", 4, 1000.0)], filter_rate=rate)
    aug = WaveAugment(None, filters=[("lowpass", 4, 1000.0)], filter_rate=0.25, seed=7)
    assert isinstance(aug.filters, FilterBank) and aug.filter_rate == 0.25 and aug.noise is None and aug.rirs is None
    assert aug.filter_seed == 7 ^ 0xD1B54A32D192ED03
    p = aug.filter_params(16000)
    assert (p.max_samples, p.rescale, p.reserved, p.seed) == (16000, 1, 0, aug.filter_seed) and abs(p.filter_rate - 0.25) < 1e-7
    assert aug.reverb_seed != aug.filter_seed


def test_random_filters_reproducible_and_in_range():
    from kws_amd.augment import FilterBank, random_filters
    a = random_filters(40, seed=3)
    assert a == random_filters(40, seed=3)
    assert a != random_filters(40, seed=4)
    assert {s[0] for s in a} == {"lowpass", "highpass", "bandpass"}
    for btype, order, f in a:
        assert order == 4
        if btype == "lowpass":
            assert 2000.0 <= f <= 7000.0
        elif btype == "highpass":
            assert 50.0 <= f <= 500.0
        else:
            assert 50.0 <= f[0] <= 500.0 and 2000.0 <= f[1] <= 7000.0
    notches = random_filters(20, types="bandstop", order=2, seed=1)
    for btype, order, (lo, hi) in notches:
        fc = np.sqrt(lo * hi)
        assert btype == "bandstop" and order == 2 and 300.0 <= fc <= 4000.0 and abs(hi / lo - 2.0 ** (1.0 / 3.0)) < 1e-12
    assert len(FilterBank(a + notches)) == 60
    with pytest.raises(ValueError):
        random_filters(0)
    with pytest.raises(ValueError):
        random_filters(4, types=("lowpass", "comb"))


def test_train_py_lists_the_filter_flags():
    out = subprocess.run([sys.executable, os.path.join(PKG, "train.py"), "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0, out.stderr
    for flag in ("--filter_rate", "--filter_types", "--filter_order", "--num_filters"):
        assert flag in out.stdout
    args_mod = __import__("importlib").util
    spec = args_mod.spec_from_file_location("kws_train_main_flt", os.path.join(PKG, "train.py"))
    train = args_mod.module_from_spec(spec)
    spec.loader.exec_module(train)
    a = train.parse_args(["--train_data_path", "d", "--classes_path", "c.txt", "--raw_audio"])
    assert (a.filter_rate, a.filter_types, a.filter_order, a.num_filters) == (None, "lowpass,highpass,bandpass", 4, 64)


def test_filter_abi_is_declared():
    with open(os.path.join(ROOT, "include", "kws.h")) as f:
        h = f.read()
    for name in ("kws_filter_bank_create", "kws_filter_bank_destroy", "kws_filter_bank_info", "kws_filter_apply", "kws_filter_params",
                 "KWS_FILTER_MAX_SECTIONS"):
        assert name in h
