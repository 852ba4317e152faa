"""GPU tests of the room-reverberation augmentation (include/kws.h: kws_rir_bank_*, kws_reverb_apply; kws_amd.augment.RirBank,
WaveAugment.reverberate): the draws against a numpy restatement of the hash, the FFT convolution against np.convolve in float64, the
equivalences with the noise-only and plain paths, features against the CPU oracle, the pipeline, fit and train.py."""
import os

import numpy as np
import pytest

from aug_ref import np_pick

pytestmark = pytest.mark.gpu

ATOL = 2e-4            # the featurizer suite's tolerance against the float64 oracle
CONV_TOL = 1e-7        # max |error| <= CONV_TOL * scale * ||v||_2 * ||h||_2
MIX = 0x9E3779B97F4A7C15


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _oracle():
    from oracle import featurizer_oracle as fo
    fo.build()
    return fo


# ---- numpy restatement of the draws (tests/aug_ref.py, fields 2 p + f) ----------------------------------------------------------------
def np_draws(seed, step, pos, rate, K):
    return np_pick(seed ^ MIX, step, pos, rate, K)


def np_reverb(v, h, ms, rescale):
    """fp64 restatement of one wet clip: (y[:L'], scale)"""
    Lv = len(v)
    if Lv == 0:
        return np.zeros(0), 1.0
    h = np.asarray(h, np.float64)[:ms]
    L = min(Lv + len(h) - 1, ms)
    y = np.convolve(np.asarray(v, np.float64), h)[:L]
    s = 1.0
    if rescale:
        ev = float(np.sum(np.asarray(v, np.float64) ** 2))
        ey = float(np.sum(y[:Lv] ** 2))
        s = np.sqrt(ev / (ey + Lv * np.finfo(np.float32).eps))
    return y * s, s


def _rirs(rng):
    """RIRs of length 1, 2, short, 11 200 and >= max_samples, peak first (RirBank keeps them as they are)"""
    out = []
    for n in (1, 2, 50, 11200, 20000):
        h = 0.3 * rng.standard_normal(n) * np.exp(-np.arange(n) / 2000.0)
        h[0] = 1.0
        out.append(h.astype(np.float32))
    return out


def _voices(rng, N, i16=False, stride=17000):
    x = (0.3 * rng.standard_normal((N, stride))).astype(np.float32)
    lens = rng.integers(0, stride + 1, N).astype(np.int32)
    lens[:8] = [0, 1, 2, 5, 300, 16000, 17000, 16999]                  # empty, short, full and longer than max_samples
    if N > 9:
        x[9] = 0.0                                                      # silent clip: finite rescale
    if i16:
        x = np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16)
    return x, lens


def _vf32(x):
    return x.astype(np.float32) / 32768.0 if x.dtype == np.int16 else x


def _noise(rng):
    return [(0.2 * rng.standard_normal(20000)).astype(np.float32), (0.05 * rng.standard_normal(9000)).astype(np.float32)]


# ---- 1. draws --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,step", [(1, 3), (0x123456789AB, 1000), (2 ** 63 + 5, 77)])
def test_draws_equal_numpy_hash(torch, seed, step):
    from kws_amd.augment import WaveAugment
    rng = np.random.default_rng(1)
    x, lens = _voices(rng, 64)
    wav, vl = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda()
    aug = WaveAugment(None, rirs=_rirs(rng), reverb_rate=0.6, seed=seed)
    _, _, used = aug.reverberate(wav, valid_len=vl, step=step, position_base=100)
    want = np_draws(seed, step, 100 + np.arange(64), np.float32(0.6), 5)
    np.testing.assert_array_equal(used.cpu().numpy(), want)
    assert (want >= 0).any() and (want < 0).any()


def test_rate_zero_one_and_shards(torch):
    from kws_amd.augment import WaveAugment
    rng = np.random.default_rng(2)
    x, lens = _voices(rng, 40)
    wav, vl = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda()
    rirs = _rirs(rng)
    for rate, dry in ((0.0, True), (1.0, False)):
        _, _, used = WaveAugment(None, rirs=rirs, reverb_rate=rate, seed=5).reverberate(wav, valid_len=vl, step=9)
        assert bool((used.cpu().numpy() < 0).all()) == dry and bool((used.cpu().numpy() >= 0).all()) != dry
    aug = WaveAugment(None, rirs=rirs, reverb_rate=0.5, seed=6)
    index = torch.from_numpy(rng.integers(0, 40, 50).astype(np.int32)).cuda()
    full = aug.reverberate(wav, valid_len=vl, index=index, step=4)
    a = aug.reverberate(wav, valid_len=vl, index=index[:23].contiguous(), step=4, position_base=0)
    b = aug.reverberate(wav, valid_len=vl, index=index[23:].contiguous(), step=4, position_base=23)
    for f, p, q in zip(full, a, b):
        assert torch.equal(f, torch.cat([p, q]))


def test_explicit_choice_and_invalid_values(torch):
    from kws_amd import KwsError
    from kws_amd.augment import WaveAugment
    rng = np.random.default_rng(3)
    x, lens = _voices(rng, 8)
    wav, vl = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda()
    aug = WaveAugment(None, rirs=_rirs(rng), seed=1)
    ex = np.array([-1, 0, 1, 2, 3, 4, -1, 2], np.int32)
    _, _, used = aug.reverberate(wav, valid_len=vl, explicit=ex)
    np.testing.assert_array_equal(used.cpu().numpy(), ex)
    for bad in ([5] * 8, [-2] * 8):
        with pytest.raises(KwsError):
            aug.reverberate(wav, valid_len=vl, explicit=np.array(bad, np.int32))
    with pytest.raises(ValueError):
        aug.reverberate(wav, valid_len=vl, explicit=np.zeros(3, np.int32))


# ---- 2. convolution ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i16,rescale", [(False, True), (True, True), (False, False)])
def test_convolution_matches_numpy_float64(torch, i16, rescale):
    from classifier.params import pr
    from kws_amd.augment import WaveAugment
    rng = np.random.default_rng(4)
    N = 40
    x, lens = _voices(rng, N, i16)
    index = np.r_[np.arange(N), rng.integers(0, N, 20)].astype(np.int32)
    wav, vl, ix = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(index).cuda()
    aug = WaveAugment(None, rirs=_rirs(rng), reverb_rate=1.0, rescale=rescale, seed=2)
    ms = pr.max_samples
    B = len(index)
    ex = rng.integers(-1, 5, B).astype(np.int32)
    ex[:N:5] = np.arange(len(ex[:N:5])) % 5                              # every RIR on the edge-case clips
    out, L, used = aug.reverberate(wav, valid_len=vl, index=ix, explicit=ex, out=torch.full((B, ms + 7), 9.0, device="cuda"))
    out, L = out.cpu().numpy(), L.cpu().numpy()
    v32 = _vf32(x)
    for b in range(B):
        row = index[b]
        lv = min(int(lens[row]), ms)
        v = v32[row, :lv]
        if ex[b] < 0:
            assert L[b] == lv
            assert np.array_equal(out[b, :lv].view(np.int32), v.view(np.int32))
        else:
            h = aug.rirs.taps[ex[b]]
            y, s = np_reverb(v, h, ms, rescale)
            assert L[b] == len(y), (b, L[b], len(y))
            bound = CONV_TOL * s * np.linalg.norm(v.astype(np.float64)) * np.linalg.norm(h.astype(np.float64))
            err = np.abs(out[b, :len(y)] - y).max() if len(y) else 0.0
            assert err <= bound, (b, lv, len(h), err, bound)
        assert not out[b, L[b]:].any()                                   # zeros after L', out to out_stride


def test_two_calls_give_identical_bits(torch):
    from kws_amd.augment import WaveAugment
    rng = np.random.default_rng(5)
    x, lens = _voices(rng, 64)
    wav, vl = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda()
    aug = WaveAugment(None, rirs=_rirs(rng), reverb_rate=0.7, seed=3)
    a = aug.reverberate(wav, valid_len=vl, step=2)
    b = aug.reverberate(wav, valid_len=vl, step=2)
    for p, q in zip(a, b):
        assert torch.equal(p, q)
    c = aug.reverberate(wav, valid_len=vl, step=3)
    assert not torch.equal(a[2], c[2])


# ---- 3. equivalences and features ----------------------------------------------------------------------------------------------------
def test_rate_zero_is_the_noise_only_and_the_plain_featurizer(torch):
    from classifier.params import pr
    from kws_amd.augment import WaveAugment
    from kws_amd.featurizer import Featurizer
    rng = np.random.default_rng(6)
    x, lens = _voices(rng, 48, stride=16000)
    index = rng.integers(0, 48, 100).astype(np.int32)
    wav, vl, ix = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(index).cuda()
    feat = Featurizer(pr)
    noise, rirs = _noise(rng), _rirs(rng)
    with_rv = WaveAugment(noise, snr=[0, 10], noised_rate=0.7, time_shift_ms=30, seed=11, rirs=rirs, reverb_rate=0.0)
    without = WaveAugment(noise, snr=[0, 10], noised_rate=0.7, time_shift_ms=30, seed=11)
    assert torch.equal(feat(wav, valid_len=vl, index=ix, augment=with_rv, step=5, position_base=3),
                       feat(wav, valid_len=vl, index=ix, augment=without, step=5, position_base=3))
    dry = WaveAugment(None, rirs=rirs, reverb_rate=0.0, seed=11)
    assert torch.equal(feat(wav, valid_len=vl, index=ix, augment=dry, step=5), feat(wav, valid_len=vl, index=ix))


def test_reverb_plus_noise_equals_the_stages_run_one_by_one(torch):
    from classifier.params import pr
    from kws_amd.augment import WaveAugment
    from kws_amd.featurizer import Featurizer
    rng = np.random.default_rng(7)
    x, lens = _voices(rng, 32)
    index = rng.integers(0, 32, 70).astype(np.int32)
    wav, vl, ix = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(index).cuda()
    feat = Featurizer(pr)
    ms = feat.geometry["max_samples"]
    aug = WaveAugment(_noise(rng), snr=[5, 20], noised_rate=0.6, time_shift_ms=20, seed=12, rirs=_rirs(rng), reverb_rate=0.7)
    got = feat(wav, valid_len=vl, index=ix, augment=aug, step=8, position_base=40)
    wet, L, used = aug.reverberate(wav, valid_len=vl, index=ix, step=8, position_base=40, max_samples=ms)
    plan = aug.plan(wet, valid_len=L, step=8, position_base=40, max_samples=ms)
    rows, L2 = aug.apply(wet, plan, max_samples=ms)
    assert torch.equal(got, feat(rows, valid_len=L2))
    u = used.cpu().numpy()
    assert (u >= 0).any() and (u < 0).any()


@pytest.mark.parametrize("i16", [False, True])
def test_reverberated_features_match_the_oracle(torch, i16):
    from classifier.params import pr
    from kws_amd.augment import WaveAugment
    from kws_amd.featurizer import Featurizer
    fo = _oracle()
    rng = np.random.default_rng(8)
    x, lens = _voices(rng, 24, i16)
    wav, vl = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda()
    aug = WaveAugment(None, rirs=_rirs(rng), reverb_rate=0.8, seed=13)
    feat = Featurizer(pr)
    got = feat(wav, valid_len=vl, augment=aug, step=1).cpu().numpy()
    _, _, used = aug.reverberate(wav, valid_len=vl, step=1)
    used = used.cpu().numpy()
    v32 = _vf32(x)
    for b in range(24):
        v = v32[b, :min(int(lens[b]), pr.max_samples)].astype(np.float64)
        y = v if used[b] < 0 else np_reverb(v, aug.rirs.taps[used[b]], pr.max_samples, True)[0]
        np.testing.assert_allclose(got[b], fo.audio_to_feature(y), atol=ATOL, rtol=0, err_msg="clip %d" % b)


# ---- 4. training ---------------------------------------------------------------------------------------------------------------------
def test_feature_pipeline_with_reverb_equals_direct_calls(torch):
    from classifier.params import pr
    from kws_amd.augment import WaveAugment
    from kws_amd.featurizer import Featurizer
    from kws_amd.pipeline import FeaturePipeline
    rng = np.random.default_rng(9)
    x, lens = _voices(rng, 100, stride=16000)
    wav, vl = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda()
    aug = WaveAugment(_noise(rng), snr=[0, 10], noised_rate=0.6, seed=4, rirs=_rirs(rng), reverb_rate=0.5)
    pipe = FeaturePipeline(Featurizer(pr), 64, pr.n_features, pr.feature_size)
    direct = Featurizer(pr)
    idx = [torch.from_numpy(rng.integers(0, 100, n).astype(np.int32)).cuda() for n in (64, 64, 30)]
    for j, ix in enumerate(idx):
        pipe.submit(wav=wav, valid_len=vl, index=ix, augment=aug, step=10 + j, position_base=5 * j)
        got = pipe.take().clone()
        pipe.release()
        want = direct(wav, valid_len=vl, index=ix, augment=aug, step=10 + j, position_base=5 * j)
        assert torch.equal(got, want)


def _audio_set(rng, C, N):
    y = rng.integers(0, C, N)
    tones = np.sin(2 * np.pi * (300.0 * (1 + np.arange(C)))[:, None] * np.arange(16000)[None, :] / 16000.0)
    x = (0.3 * tones[y] + 0.05 * rng.standard_normal((N, 16000))).astype(np.float32)
    lens = rng.integers(4000, 16001, N).astype(np.int32)
    for i in range(N):
        x[i, lens[i]:] = 0.0
    return x, y, lens


def _fit(torch, x, y, C, pipelined, **kw):
    from classifier.loss import SparseCategoricalCrossEntropy
    from classifier.model import KWSModel
    from common.model_utils import get_optimizer
    torch.manual_seed(1234)
    m = KWSModel("simple_cnn", C, seed=3)
    m._device().set_deterministic(True)
    m.compile(optimizer=get_optimizer("adam", 1e-3), loss=SparseCategoricalCrossEntropy(), metrics=["accuracy"])
    h = m.fit(x, y, batch_size=64, epochs=2, verbose=0, shuffle=True, pipeline=pipelined, **kw)
    return (h.history["loss"], h.history["accuracy"]), m.get_weights()


def test_fit_with_reverb_pipelined_equals_stepwise_and_differs_from_plain(torch):
    from kws_amd.augment import WaveAugment, simulate_rirs
    rng = np.random.default_rng(10)
    C = 4
    x, y, lens = _audio_set(rng, C, 150)
    aug = WaveAugment(None, rirs=simulate_rirs(3, seed=1), reverb_rate=0.8, seed=8)
    h0, w0 = _fit(torch, x, y, C, False, augment=aug, sample_lengths=lens)
    h1, w1 = _fit(torch, x, y, C, True, augment=aug, sample_lengths=lens)
    assert h0 == h1
    for a, b in zip(w0, w1):
        np.testing.assert_array_equal(a, b)
    hp, wp = _fit(torch, x, y, C, True, sample_lengths=lens)
    assert hp != h1
    assert any(not np.array_equal(a, b) for a, b in zip(wp, w1))
    assert all(np.isfinite(h1[0]))


def test_train_py_end_to_end_with_simulated_rooms(torch, tmp_path):
    import importlib.util
    from common.data_utils import save_audio
    rng = np.random.default_rng(12)
    classes = ["background", "yes", "no"]
    for c, cls in enumerate(classes):
        d = tmp_path / "data" / "sounds" / cls
        d.mkdir(parents=True)
        for i in range(12):
            n = int(rng.integers(6000, 16001))
            t = np.arange(n) / 16000.0
            save_audio(str(d / ("%d.wav" % i)), 0.3 * np.sin(2 * np.pi * 400.0 * (c + 1) * t) + 0.02 * rng.standard_normal(n))
    (tmp_path / "classes.txt").write_text("\n".join(classes) + "\n")
    spec = importlib.util.spec_from_file_location("kws_train_main_rv", os.path.join(os.path.dirname(os.path.dirname(__file__)),
                                                                                 "tf-keras-speech-commands_amd", "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    np.random.seed(0)
    logs = tmp_path / "logs"
    hist = train.main(["--train_data_path", str(tmp_path / "data"), "--classes_path", str(tmp_path / "classes.txt"), "--raw_audio",
                       "--simulate_rirs", "4", "--reverb_rate", "0.5", "--epochs", "2", "--batch_size", "8", "--val_split", "0.25",
                       "--log_dir", str(logs)])
    assert len(hist.history["loss"]) == 2 and all(np.isfinite(hist.history["loss"]))
    assert (logs / "trained_final.npz").exists()
