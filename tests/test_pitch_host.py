"""CPU tests of the tempo and pitch perturbation surface: the float64 restatement the GPU tests compare against (identity at rho = 1,
lengths, a sine that keeps its frequency when stretched, the draws), WaveAugment's argument handling, train.py's flags, and the host
side of the C ABI (kws_pitch_workspace_bytes without a device, the argument checks of kws_pitch_apply and kws_pitch_stft, which fail
loudly without a device)."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import pitch_ref as pr_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf-keras-speech-commands_amd")
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 1000, 1100)
RATES = (0.5, 0.8, 1.25, 2.0)


# ---- the restatement itself ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", pr_.N_FFTS)
def test_reference_is_the_identity_at_rate_one(N):
    rng = np.random.default_rng(0)
    for Ls in (1, N // 4 + 1, 3 * N + 17):
        v = rng.standard_normal(Ls)
        out = pr_.perturb(v, 1.0, float("nan"), 10 ** 6, N)
        # the first frame is centred on sample 0, so every sample lies under a positive window sum
        assert out["y"].shape == (Ls,) and out["J"] == pr_.n_frames(Ls, N)
        err = float(np.abs(out["y"] - v).max())
        print("N = %d, Ls = %d: identity error %.3g" % (N, Ls, err))
        assert err <= 1e-12
        assert np.all(out["A"] > 0) and not out["T"].any()


def test_reference_lengths_and_finiteness_over_the_grid():
    rng = np.random.default_rng(1)
    for Ls in LENGTHS:
        v = 0.3 * rng.standard_normal(Ls)
        D, S = pr_.stft(v, 256)
        assert D.shape == (1 + Ls // 64, 129) and S.shape == (1 + Ls // 64,)
        for rate in RATES:
            y, A, J = pr_.vocoder(D, Ls, rate, 256)
            assert len(y) == len(A) == int(np.floor(Ls / rate + 0.5)) == pr_.stretch_length(Ls, rate), (Ls, rate)
            assert J == int(np.ceil((1 + Ls // 64) / rate))
            assert np.all(np.isfinite(y)) and np.all(np.isfinite(A)) and np.all(A >= 0)
    assert pr_.out_length(1100, 0.5, float("nan"), 1024) == 1024 and pr_.out_length(1000, 2.0, float("nan"), 1024) == 500
    assert pr_.out_length(1000, 0.0, 12.0, 1024) == 1000 and pr_.out_length(0, 1.25, 4.0, 1024) == 0
    dry = pr_.perturb(np.arange(5.0), 0.0, float("nan"), 3)
    assert np.array_equal(dry["y"], [0.0, 1.0, 2.0]) and dry["J"] == 0


@pytest.mark.parametrize("rate", [0.8, 1.25])
def test_reference_keeps_the_frequency_of_a_stretched_sine(rate):
    fs, N = 16000.0, 512
    v = np.sin(2 * np.pi * 1000.0 * np.arange(8000) / fs)
    y = pr_.perturb(v, rate, float("nan"), 10 ** 6, N)["y"]
    assert len(y) == int(np.floor(8000 / rate + 0.5))
    spec = np.abs(np.fft.rfft(y * np.hanning(len(y))))
    peak = float(np.argmax(spec)) * fs / len(y)
    print("rate %g: %d samples, peak at %.1f Hz" % (rate, len(y), peak))
    assert abs(peak - 1000.0) <= fs / len(y)                 # within one bin of the output's own transform
    mid = y[N:-N]
    assert 0.9 <= np.sqrt(2.0 * np.mean(mid * mid)) <= 1.1   # and its amplitude


def test_reference_draws_are_uniform_and_keyed():
    import speed_ref as sr
    from kws_amd.augment import FILTER_SEED_MIX, FMASK_SEED_MIX, PITCH_SEED_MIX, REVERB_SEED_MIX, SPEED_SEED_MIX
    assert PITCH_SEED_MIX == pr_.MIX == 0x8EBC6AF09C88C6E3
    assert len({0, PITCH_SEED_MIX, SPEED_SEED_MIX, FILTER_SEED_MIX, REVERB_SEED_MIX, FMASK_SEED_MIX}) == 6
    pos = np.arange(4096)
    on, t, pit, n = pr_.np_draws(5, 3, pos, 0.5, (0.8, 1.25), 0.25, (-4.0, 2.0))
    assert t.dtype == n.dtype == np.float32
    assert 0.45 < on.mean() < 0.55 and 0.2 < pit.mean() < 0.3
    assert t.min() >= np.float32(0.8) and t.max() <= np.float32(1.25) and n.min() >= -4.0 and n.max() <= 2.0
    assert abs(t.mean() - 1.025) < 0.01 and abs(n.mean() + 1.0) < 0.1
    assert (on != pr_.np_draws(5, 4, pos, 0.5, (0.8, 1.25))[0]).any()
    assert not pr_.np_draws(5, 3, pos, 0.0, (0.8, 1.25))[0].any() and pr_.np_draws(5, 3, pos, 1.0, (0.8, 1.25))[0].all()
    # the same user seed: other fields than the speed stage's
    assert (on != sr.np_draws(5, 3, pos, 0.5, (0.8, 1.25))[0]).any()
    assert pr_.ratio(12.0) == 2.0 and pr_.ratio(-12.0) == 0.5 and pr_.ratio(float("nan")) == 1.0
    assert pr_.ratio(4.0) == np.float32(2.0 ** (1.0 / 3.0)) and pr_.rho(0.0, float("nan")) == 1.0 and pr_.rho(2.0, -12.0) == 4.0


# ---- the host API --------------------------------------------------------------------------------------------------------------------
def test_wave_augment_tempo_and_pitch_arguments():
    from kws_amd.augment import PITCH_SEED_MIX, Resampler, WaveAugment
    for kw in (dict(tempo=(0.4, 1.0)), dict(tempo=(1.0, 2.5)), dict(tempo=(1.2, 0.8)), dict(tempo=1.0), dict(tempo=(1.0,)),
               dict(tempo=(0.9, 1.1), tempo_rate=1.5), dict(tempo=(0.9, 1.1), tempo_rate=-0.1), dict(tempo=(0.9, float("nan"))),
               dict(pitch=(-13.0, 2.0)), dict(pitch=(-2.0, 12.5)), dict(pitch=(2.0, -2.0)), dict(pitch=2.0),
               dict(pitch=(-2, 2), pitch_rate=2.0), dict(pitch=(-2, 2), pitch_rate=-1.0), dict(pitch=(-2, 2), resampler="kaiser_best"),
               dict(tempo=(0.9, 1.1), pitch_n_fft=128), dict(tempo=(0.9, 1.1), pitch_n_fft=500), dict(tempo=(0.9, 1.1), pitch_n_fft=True)):
        with pytest.raises(ValueError):
            WaveAugment(None, **kw)
    with pytest.raises(ValueError, match="WaveAugment needs a noise bank, a RIR bank or both"):
        WaveAugment(None, pitch_n_fft=256)
    only_tempo = WaveAugment(None, tempo=(0.9, 1.1))          # an augment with nothing but a tempo range, and no table
    assert only_tempo.vocodes and not only_tempo.perturbs and only_tempo.resampler is None and only_tempo.pitch is None
    only_pitch = WaveAugment(None, pitch=(-2, 2), seed=7)
    assert only_pitch.vocodes and isinstance(only_pitch.resampler, Resampler) and only_pitch.pitch == (-2.0, 2.0)
    rs = Resampler(zero_crossings=4, phases=32)
    assert WaveAugment(None, pitch=(-2, 2), resampler=rs).resampler is rs
    aug = WaveAugment(None, tempo=(0.85, 1.2), tempo_rate=0.75, pitch=(-3, 2), pitch_rate=0.5, pitch_n_fft=1024, seed=7)
    assert aug.pitch_seed == 7 ^ PITCH_SEED_MIX and aug.pitch_seed not in (aug.speed_seed, aug.filter_seed, aug.reverb_seed, aug.seed)
    p = aug.pitch_params(16000)
    assert (p.n_fft, p.max_samples, p.reserved, p.seed) == (1024, 16000, 0, aug.pitch_seed)
    got = np.array([p.tempo_rate, p.tempo_lo, p.tempo_hi, p.pitch_rate, p.pitch_lo, p.pitch_hi], np.float32)
    np.testing.assert_array_equal(got, np.array([0.75, 0.85, 1.2, 0.5, -3.0, 2.0], np.float32))
    p = only_tempo.pitch_params(100)
    assert p.pitch_rate == 0.0 and p.tempo_rate == 1.0 and p.n_fft == 512
    plain = WaveAugment(None, speed=(0.9, 1.1))
    assert not plain.vocodes and plain.tempo is None and plain.pitch is None


def _train_module(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(PKG, "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    return train


def test_train_py_tempo_and_pitch_flags(tmp_path, capsys):
    train = _train_module("kws_train_main_pv")
    with pytest.raises(SystemExit) as e:
        train.parse_args(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for flag in ("--tempo_range", "--tempo_rate", "--pitch_range", "--pitch_rate"):
        assert flag in text
    base = ["--train_data_path", str(tmp_path), "--classes_path", str(tmp_path / "classes.txt")]
    a = train.parse_args(base + ["--raw_audio"])
    assert (a.tempo_range, a.tempo_rate, a.pitch_range, a.pitch_rate) == (None, None, None, None)
    assert train.perturb_options(a) == {}
    a = train.parse_args(base + ["--raw_audio", "--tempo_range", "0.85,1.2", "--tempo_rate", "0.5", "--pitch_range", "-2,2"])
    assert train.perturb_options(a) == dict(tempo=(0.85, 1.2), tempo_rate=0.5, pitch=(-2.0, 2.0), pitch_rate=1.0)
    a = train.parse_args(base + ["--raw_audio", "--pitch_range=-3,1", "--pitch_rate", "0.25", "--speed_range", "0.9,1.1"])
    assert train.perturb_options(a) == dict(speed=(0.9, 1.1), speed_rate=1.0, pitch=(-3.0, 1.0), pitch_rate=0.25)
    for bad in (["--tempo_range", "0.9"], ["--tempo_range", "a,b"], ["--tempo_range", "0.4,1.0"], ["--tempo_range", "1.1,0.9"],
                ["--pitch_range", "-13,2"], ["--pitch_range", "2,-2"], ["--tempo_range", "0.9,1.1", "--tempo_rate", "1.5"],
                ["--pitch_range", "-2,2", "--pitch_rate", "-0.5"]):
        with pytest.raises(SystemExit):
            train.perturb_options(train.parse_args(base + ["--raw_audio"] + bad))
    (tmp_path / "classes.txt").write_text("background\nyes\n")
    for flags, word in ((["--tempo_range", "0.9,1.1"], "--tempo_range needs --raw_audio"),
                        (["--pitch_range", "-2,2"], "--pitch_range needs --raw_audio"),
                        (["--tempo_rate", "0.5"], "--tempo_rate needs --raw_audio"),
                        (["--raw_audio", "--tempo_rate", "0.5"], "--tempo_rate needs --tempo_range"),
                        (["--raw_audio", "--pitch_rate", "0.5"], "--pitch_rate needs --pitch_range")):
        with pytest.raises(SystemExit) as e:
            train.main(base + ["--log_dir", str(tmp_path / "logs")] + flags)
        assert word in str(e.value), (flags, e.value)


# ---- the C ABI on the host -----------------------------------------------------------------------------------------------------------
def test_pitch_abi_is_declared():
    with open(os.path.join(ROOT, "include", "kws.h")) as f:
        h = f.read()
    for name in ("kws_pitch_params", "kws_pitch_workspace_bytes", "kws_pitch_stft", "kws_pitch_apply", "0x8EBC6AF09C88C6E3",
                 "no phase locking"):
        assert name in h


def test_workspace_bytes_needs_no_device_and_checks_its_arguments():
    from kws_amd import lib as l
    from kws_amd.augment import pitch_workspace_bytes
    L = l.get_lib()
    n = ctypes.c_size_t(7)
    for bad, word in (((128, 1024, 1), "n_fft"), ((500, 1024, 1), "n_fft"), ((2048, 1024, 1), "n_fft"), ((512, 0, 1), "max_samples"),
                      ((512, 1024, 0), "tile_clips")):
        assert L.kws_pitch_workspace_bytes(*bad, ctypes.byref(n)) == l.ERR_INVALID and word in L.kws_last_error().decode(), bad
        assert n.value == 0
    assert L.kws_pitch_workspace_bytes(512, (1 << 20) + 1, 1, ctypes.byref(n)) == l.ERR_UNSUPPORTED
    assert L.kws_pitch_workspace_bytes(512, 1024, 1, None) == l.ERR_INVALID
    one = pitch_workspace_bytes(512, 16000, 1)
    # 2 max_samples + 64 stretched samples, the 253 output frames over them and 4 analysis frames an output frame at rho = 4
    assert 1010 * 257 * 8 + 32064 * 4 <= one <= 1010 * 257 * 8 + 32064 * 4 + 256 and one % 128 == 0
    assert pitch_workspace_bytes(512, 16000, 256) == 256 * one
    assert pitch_workspace_bytes(256, 1024, 3) == 3 * pitch_workspace_bytes(256, 1024, 1) < one
    with pytest.raises(l.KwsError):
        pitch_workspace_bytes(300, 1024, 1)


def test_apply_and_stft_check_their_arguments_and_fail_loudly_without_a_device():
    import kws_amd
    from kws_amd import lib as l
    from kws_amd.augment import Resampler, WaveAugment
    L = l.get_lib()
    aug = WaveAugment(None, tempo=(0.9, 1.1), pitch=(-2, 2), pitch_n_fft=256, seed=1)
    rs = aug.resampler.handle()
    B, stride, ms = 4, 1100, 1024
    fake = 4096                                               # device pointers that no check dereferences
    et = np.zeros(B, np.float32)
    es = np.full(B, np.nan, np.float32)

    def call(p, handle=rs, wav=fake, dtype=l.WAV_F32, out=fake + 1, out_stride=ms, lengths=fake, ext=None, exs=None, used=fake, ws=fake,
             ws_bytes=1 << 30, base=0):
        rc = L.kws_pitch_apply(handle, ctypes.byref(p), wav, dtype, None, B, stride, None, base, 0, None if ext is None else ext.ctypes.data,
                               None if exs is None else exs.ctypes.data, out, out_stride, lengths, used, used, ws, ws_bytes, None)
        return rc, L.kws_last_error().decode()

    for field, value, word in (("tempo_rate", 1.5, "tempo_rate"), ("pitch_rate", -0.5, "pitch_rate"), ("tempo_lo", 0.4, "tempo range"),
                               ("tempo_hi", 0.8, "tempo range"), ("pitch_lo", -12.5, "pitch range"), ("pitch_hi", -3.0, "pitch range"),
                               ("n_fft", 300, "n_fft"), ("max_samples", 0, "max_samples")):
        p = aug.pitch_params(ms)
        setattr(p, field, value)
        rc, msg = call(p)
        assert rc == l.ERR_INVALID and word in msg, (field, rc, msg)
    good = aug.pitch_params(ms)
    p = aug.pitch_params(ms)
    p.max_samples = (1 << 20) + 1
    assert call(p, out_stride=1 << 21)[0] == l.ERR_UNSUPPORTED
    for kw, word in ((dict(wav=None), "null"), (dict(lengths=None), "null"), (dict(base=-1), "negative"), (dict(out_stride=ms - 1), "out_stride"),
                     (dict(dtype=7), "dtype"), (dict(out=fake), "in place"), (dict(handle=None), "resampler"), (dict(ws=None), "workspace"),
                     (dict(ext=np.full(B, 0.4, np.float32)), "tempo"), (dict(ext=np.full(B, np.nan, np.float32)), "tempo"),
                     (dict(exs=np.full(B, 12.5, np.float32)), "semitones"), (dict(exs=np.full(B, np.inf, np.float32)), "semitones"),
                     (dict(ext=et, used=None), "tempo_used"), (dict(exs=es, used=None), "pitch_used")):
        rc, msg = call(good, **kw)
        assert rc == l.ERR_INVALID and word in msg, (kw, rc, msg)
    rc, msg = call(good, ws_bytes=1000)
    assert rc == l.ERR_WORKSPACE and "holds no clip" in msg
    out = ctypes.c_void_p(fake)
    for args, word in (((None, l.WAV_F32, None, B, stride, None, 256, out, 5, None), "null"),
                       ((fake, l.WAV_F32, None, B, stride, None, 128, out, 5, None), "n_fft"),
                       ((fake, l.WAV_F32, None, B, stride, None, 256, out, 0, None), "frames"),
                       ((fake, 9, None, B, stride, None, 256, out, 5, None), "dtype"),
                       ((fake, l.WAV_F32, None, -1, stride, None, 256, out, 5, None), "negative")):
        assert L.kws_pitch_stft(*args) == l.ERR_INVALID and word in L.kws_last_error().decode(), args
    assert L.kws_pitch_stft(fake, l.WAV_F32, None, 0, stride, None, 256, out, 5, None) == 0
    if kws_amd.device_count() == 0:                          # no CPU fallback: a valid call reports the missing device
        rc, msg = call(good)
        assert rc == l.ERR_HIP and "hip" in msg.lower(), (rc, msg)
        rc, msg = call(good, ext=et, exs=es, handle=None, ws=None)         # nothing to do but the copy: still no silent success
        assert rc == l.ERR_HIP
        assert L.kws_pitch_stft(fake, l.WAV_F32, None, B, stride, None, 256, out, 5, None) == l.ERR_HIP
        with pytest.raises(kws_amd.KwsError) as e:
            import torch
            aug.pitch_perturb(torch.zeros((2, 64)))
        assert e.value.code == -3 and "no CPU fallback" in str(e.value)
    assert isinstance(aug.resampler, Resampler)
