"""CPU tests of the speed and loudness perturbation surface: kws_resampler_* (a host object) and its table against the numpy restatement,
WaveAugment / Resampler argument handling, train.py's flags, and the sanity of the float64 restatement the GPU tests compare against
(identity at r = 1, a sine resampled within the ripple that the table's own frequency response gives)."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest

import speed_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf-keras-speech-commands_amd")


def _create(L, Z, P, beta, rolloff):
    h = ctypes.c_void_p()
    rc = L.kws_resampler_create(Z, P, beta, rolloff, ctypes.byref(h))
    return rc, h, L.kws_last_error().decode()


def test_resampler_create_checks_its_arguments_and_info_reads_them_back():
    from kws_amd import lib as l
    L = l.get_lib()
    ok = (16, 512, 8.555504641634386, 0.85)
    bad = [((3,) + ok[1:], "zero_crossings"), ((33,) + ok[1:], "zero_crossings"), ((16, 31) + ok[2:], "phases"),
           ((16, 1025) + ok[2:], "phases"), (ok[:2] + (-0.5, 0.85), "beta"), (ok[:2] + (20.5, 0.85), "beta"),
           (ok[:2] + (float("nan"), 0.85), "beta"), (ok[:3] + (0.0,), "rolloff"), (ok[:3] + (1.01,), "rolloff"),
           (ok[:3] + (float("nan"),), "rolloff")]
    for args, word in bad:
        rc, h, msg = _create(L, *args)
        assert rc == l.ERR_INVALID and not h.value and word in msg, (args, rc, msg)
    rc, h, msg = _create(L, 32, 512, 8.0, 0.9)                  # 16385 floats: more than 64 KiB
    assert rc == l.ERR_UNSUPPORTED and not h.value and "LDS" in msg
    assert L.kws_resampler_create(*ok, None) == l.ERR_INVALID
    for args in (ok, (4, 32, 0.0, 1.0), (32, 511, 20.0, 0.5), (16, 1023, 5.0, 0.25)):
        rc, h, msg = _create(L, *args)
        assert rc == 0 and h.value, msg
        Z, P, beta, roll = ctypes.c_int(), ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
        assert L.kws_resampler_info(h, ctypes.byref(Z), ctypes.byref(P), ctypes.byref(beta), ctypes.byref(roll)) == 0
        assert (Z.value, P.value, beta.value, roll.value) == args
        assert L.kws_resampler_info(h, None, None, None, None) == 0
        small = np.zeros(args[0] * args[1], np.float32)
        assert L.kws_resampler_table(h, small.ctypes.data, small.size) == l.ERR_INVALID
        L.kws_resampler_destroy(h)
    assert L.kws_resampler_info(None, None, None, None, None) == l.ERR_INVALID
    L.kws_resampler_destroy(None)


@pytest.mark.parametrize("args", [(16, 512, 8.555504641634386, 0.85), (4, 32, 8.555504641634386, 0.85), (8, 100, 0.0, 1.0), (31, 500, 20.0, 0.3)])
def test_table_is_the_float32_rounding_of_the_float64_definition(args):
    from kws_amd.augment import Resampler
    rs = Resampler(*args)
    got = rs.table()
    Z, P, beta, roll = args
    i = np.arange(Z * P + 1, dtype=np.float64)
    u = i / (P * Z)
    want = roll * np.sinc(roll * i / P) * np.i0(beta * np.sqrt(np.maximum(1.0 - u * u, 0.0))) / np.i0(beta)
    assert got.dtype == np.float32 and got.shape == want.shape == (len(rs),)
    # one float32 rounding of a float64 value; the two I0 implementations differ by a few float64 ulps, and |sin(pi x)| near a
    # zero crossing carries the 1e-16 absolute error of pi x
    assert np.all(np.abs(got - want) <= 2.0 ** -24 * np.abs(want) * (1 + 1e-6) + 1e-15)
    np.testing.assert_array_equal(sr.table(*args), want.astype(np.float32))
    assert got[0] == np.float32(roll)
    rs.close()
    with pytest.raises(ValueError):
        rs.handle()


def test_resampler_and_wave_augment_arguments():
    from kws_amd.augment import FILTER_SEED_MIX, REVERB_SEED_MIX, SPEED_SEED_MIX, Resampler, WaveAugment
    assert len({SPEED_SEED_MIX, FILTER_SEED_MIX, REVERB_SEED_MIX}) == 3 and 0 < SPEED_SEED_MIX < 2 ** 64 and SPEED_SEED_MIX == sr.MIX
    rs = Resampler()
    assert (rs.zero_crossings, rs.phases, rs.beta, rs.rolloff) == (16, 512, 8.555504641634386, 0.85) and len(rs) == 8193
    for kw in (dict(zero_crossings=3), dict(phases=2000), dict(beta=-1.0), dict(rolloff=0.0), dict(zero_crossings=32, phases=1024),
               dict(zero_crossings=8.5)):
        with pytest.raises(ValueError):
            Resampler(**kw)
    with pytest.raises(ValueError, match="WaveAugment needs a noise bank, a RIR bank or both"):
        WaveAugment(None)
    for kw in (dict(speed=(0.4, 1.0)), dict(speed=(1.0, 2.5)), dict(speed=(1.2, 0.8)), dict(speed=1.0), dict(speed=(1.0,)),
               dict(speed=(0.9, 1.1), speed_rate=1.5), dict(speed=(0.9, 1.1), speed_rate=-0.1), dict(speed=(0.9, float("nan"))),
               dict(loudness=(-90.0, -10.0)), dict(loudness=(-20.0, 3.0)), dict(loudness=(-10.0, -20.0)), dict(loudness=-20.0),
               dict(loudness=(-30, -15), loudness_rate=2.0), dict(loudness=(-30, -15), loudness_rate=-1.0),
               dict(speed=(0.9, 1.1), resampler="kaiser_best")):
        with pytest.raises(ValueError):
            WaveAugment(None, **kw)
    aug = WaveAugment(None, speed=(0.9, 1.1), speed_rate=0.75, loudness=(-30, -15), loudness_rate=0.5, seed=7)
    assert aug.noise is None and aug.rirs is None and aug.filters is None and aug.perturbs
    assert aug.speed == (0.9, 1.1) and aug.loudness == (-30.0, -15.0) and isinstance(aug.resampler, Resampler)
    assert aug.speed_seed == 7 ^ SPEED_SEED_MIX and aug.speed_seed not in (aug.filter_seed, aug.reverb_seed, aug.seed)
    p = aug.speed_params(16000)
    assert (p.max_samples, p.reserved, p.seed) == (16000, 0, aug.speed_seed)
    got = np.array([p.speed_rate, p.speed_lo, p.speed_hi, p.loud_rate, p.loud_lo_db, p.loud_hi_db], np.float32)
    np.testing.assert_array_equal(got, np.array([0.75, 0.9, 1.1, 0.5, -30.0, -15.0], np.float32))
    only_loud = WaveAugment(None, loudness=(-20, -20), resampler=None)
    assert only_loud.resampler is None and only_loud.speed is None and only_loud.perturbs
    p = only_loud.speed_params(100)
    assert p.speed_rate == 0.0 and p.loud_rate == 1.0 and p.loud_lo_db == p.loud_hi_db == -20.0
    mine = WaveAugment(None, speed=(1.0, 1.0), resampler=rs)
    assert mine.resampler is rs
    plain = WaveAugment(None, filters=[("lowpass", 4, 1000.0)])
    assert not plain.perturbs and plain.resampler is None


def _train_module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(PKG, "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    return train


def test_train_py_speed_and_loudness_flags(tmp_path, capsys, monkeypatch):
    train = _train_module("kws_train_main_spd")
    with pytest.raises(SystemExit) as e:
        train.parse_args(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for flag in ("--speed_range", "--speed_rate", "--loudness_range", "--loudness_rate"):
        assert flag in text
    base = ["--train_data_path", str(tmp_path), "--classes_path", str(tmp_path / "classes.txt")]
    a = train.parse_args(base + ["--raw_audio"])
    assert (a.speed_range, a.speed_rate, a.loudness_range, a.loudness_rate) == (None, None, None, None)
    assert train.perturb_options(a) == {}
    a = train.parse_args(base + ["--raw_audio", "--speed_range", "0.9,1.1", "--speed_rate", "0.5", "--loudness_range", "-30,-15"])
    assert train.perturb_options(a) == dict(speed=(0.9, 1.1), speed_rate=0.5, loudness=(-30.0, -15.0), loudness_rate=1.0)
    monkeypatch.setattr(sys, "argv", ["train.py"] + base + ["--raw_audio", "--loudness_range", "-30,-15", "--loudness_rate", "0.5"])
    a = train.parse_args()                                   # the command line itself, with the value that starts with '-'
    assert train.perturb_options(a) == dict(loudness=(-30.0, -15.0), loudness_rate=0.5)
    a = train.parse_args(base + ["--raw_audio", "--loudness_range=-40,-6"])
    assert train.perturb_options(a)["loudness"] == (-40.0, -6.0)
    for bad in (["--speed_range", "0.9"], ["--speed_range", "a,b"], ["--speed_range", "0.4,1.0"], ["--speed_range", "1.1,0.9"],
                ["--loudness_range", "-20,5"], ["--loudness_range", "-20,-30"], ["--speed_range", "0.9,1.1", "--speed_rate", "1.5"],
                ["--loudness_range", "-30,-15", "--loudness_rate", "-0.5"]):
        with pytest.raises(SystemExit):
            train.perturb_options(train.parse_args(base + ["--raw_audio"] + bad))
    (tmp_path / "classes.txt").write_text("background\nyes\n")
    for flags, word in ((["--speed_range", "0.9,1.1"], "--speed_range needs --raw_audio"),
                        (["--loudness_range", "-30,-15"], "--loudness_range needs --raw_audio"),
                        (["--speed_rate", "0.5"], "--speed_rate needs --raw_audio"),
                        (["--loudness_rate", "0.5"], "--loudness_rate needs --raw_audio"),
                        (["--raw_audio", "--speed_rate", "0.5"], "--speed_rate needs --speed_range"),
                        (["--raw_audio", "--loudness_rate", "0.5"], "--loudness_rate needs --loudness_range")):
        with pytest.raises(SystemExit) as e:
            train.main(base + ["--log_dir", str(tmp_path / "logs")] + flags)
        assert word in str(e.value), (flags, e.value)


def test_speed_abi_is_declared():
    with open(os.path.join(ROOT, "include", "kws.h")) as f:
        h = f.read()
    for name in ("kws_resampler_create", "kws_resampler_destroy", "kws_resampler_info", "kws_speed_apply", "kws_speed_params",
                 "0xA0761D6478BD642F"):
        assert name in h


# ---- the restatement itself ----------------------------------------------------------------------------------------------------------
def test_reference_draws_are_uniform_and_keyed():
    pos = np.arange(4096)
    on, r, lev, tg = sr.np_draws(5, 3, pos, 0.5, (0.8, 1.25), 0.25, (-30.0, -10.0))
    assert r.dtype == tg.dtype == np.float32
    assert 0.45 < on.mean() < 0.55 and 0.2 < lev.mean() < 0.3
    assert r.min() >= np.float32(0.8) and r.max() <= np.float32(1.25) and tg.min() >= -30.0 and tg.max() <= -10.0
    assert abs(r.mean() - 1.025) < 0.01 and abs(tg.mean() + 20.0) < 0.5
    on2 = sr.np_draws(5, 4, pos, 0.5, (0.8, 1.25), 0.25, (-30.0, -10.0))[0]
    assert (on != on2).any()
    assert not sr.np_draws(5, 3, pos, 0.0, (0.8, 1.25))[0].any() and sr.np_draws(5, 3, pos, 1.0, (0.8, 1.25))[0].all()


def test_reference_is_the_identity_at_ratio_one_with_full_bandwidth():
    rng = np.random.default_rng(0)
    v = rng.standard_normal(700)
    for Z, P in ((16, 512), (4, 32)):
        h = sr.table(Z, P, 8.555504641634386, 1.0)           # rolloff 1: sinc(k) = 0 at every other sample
        y, A, T = sr.resample(v, 1.0, 1000, h, Z, P)
        assert y.shape == (700,) and np.abs(y - v).max() <= 1e-12
        assert T[350] == 2 * Z - 1 and T[0] == Z and T[-1] == Z   # at phi = 0 the taps at distance Z fall on the table's end: not taken
    y, _, _ = sr.resample(v, 1.0, 512, sr.table(**sr.DEFAULTS), 16, 512)
    assert y.shape == (512,)
    assert sr.out_length(0, 1.25, 512) == 0 and sr.out_length(1100, 2.0, 512) == 512 and sr.out_length(7, 0.5, 512) == 14
    assert sr.out_length(640, 1.25, 512) == 512 and sr.out_length(300, 0.8, 512) == 375 and sr.out_length(301, 2.0, 512) == 151
    assert len(sr.resample(np.zeros(0), 1.25, 512, sr.table(**sr.DEFAULTS), 16, 512)[0]) == 0


def _phase_response_error(h, Z, P, r, omega, phases=4096):
    """max over a grid of fractional positions phi of |sum_m g(phi - m) exp(i omega (m - phi)) - 1|, g(x) = s hlin(|x| s P): what the
    interpolator does to exp(i omega t) away from the ends, from the table alone"""
    hd = h.astype(np.float64)
    s = min(1.0, 1.0 / r)
    reach = int(np.ceil(Z / s)) + 1
    phi = np.arange(phases, dtype=np.float64)[:, None] / phases
    m = np.arange(-reach, reach + 1, dtype=np.float64)[None, :]
    x = phi - m                                              # distance from the output position to source sample m
    pos = np.abs(x) * s * P
    inside = pos < Z * P
    i = np.minimum(np.floor(pos).astype(np.int64), Z * P - 1)
    w = np.where(inside, hd[i] + (pos - i) * (hd[i + 1] - hd[i]), 0.0) * s
    resp = (w * np.exp(-1j * omega * x)).sum(1)
    return float(np.abs(resp - 1.0).max())


def test_reference_turns_a_440_hz_sine_into_a_550_hz_sine_within_the_design_ripple():
    fs, Z, P = 16000.0, 16, 512
    h = sr.table(**sr.DEFAULTS)
    r = 1.25
    n_in = 4000
    v = np.sin(2 * np.pi * 440.0 * np.arange(n_in) / fs)
    y, A, T = sr.resample(v, r, 10 ** 6, h, Z, P)
    assert len(y) == n_in / r
    want = np.sin(2 * np.pi * 550.0 * np.arange(len(y)) / fs)
    ripple = _phase_response_error(h, Z, P, r, 2 * np.pi * 440.0 / fs)
    assert 1e-7 < ripple < 1e-3, ripple                      # a -100 dB window and 512 phases read linearly: about 1e-5
    edge = int(np.ceil(Z / min(1.0, 1.0 / r) / r)) + 1       # outputs whose window reaches past an end of the clip
    err = np.abs(y - want)[edge:-edge].max()
    print("440 Hz -> 550 Hz: max error %.3g, ripple bound %.3g" % (err, ripple))
    assert err <= ripple + 1e-12
    assert np.abs(y - want)[:2].max() > ripple               # the ends do miss their left wing: the crop above is needed
    # the same at r = 0.8 (no band limiting below the source rate, s = 1): 440 Hz -> 352 Hz
    y, _, _ = sr.resample(v, 0.8, 10 ** 6, h, Z, P)
    want = np.sin(2 * np.pi * 352.0 * np.arange(len(y)) / fs)
    ripple = _phase_response_error(h, Z, P, 0.8, 2 * np.pi * 440.0 / fs)
    assert np.abs(y - want)[Z + 5:-(Z + 5)].max() <= ripple + 1e-12


def test_reference_gain_reaches_the_target_level():
    rng = np.random.default_rng(1)
    v = 0.3 * rng.standard_normal(500)
    for target in (-40.0, -20.0, -6.0):
        g = sr.gain(v, target)
        assert g.dtype == np.float32
        assert abs(sr.level_db(float(g) * v) - target) <= 1e-4
    assert np.isfinite(sr.gain(np.zeros(10), -20.0)) and np.isfinite(sr.gain(np.zeros(0), -20.0))
    out = sr.perturb(v, 0.0, float("nan"), 400)
    assert out["g"] == 1.0 and np.array_equal(out["y"], v[:400])
