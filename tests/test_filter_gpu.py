"""GPU tests of the Butterworth filter augmentation (include/kws.h: kws_filter_bank_*, kws_filter_apply; kws_amd.augment.FilterBank,
WaveAugment.filter): the draws against a numpy restatement of the hash, the chunk-scan filtfilt against a float64 numpy restatement of
scipy's filtfilt, dry and in-place bit equalities, the chain with reverb and noise, features against the CPU oracle, the pipeline, fit
and train.py."""
import os

import numpy as np
import pytest

from filter_ref import filtfilt_batch, np_draws

pytestmark = pytest.mark.gpu

ATOL = 2e-4            # the featurizer suite's tolerance against the float64 oracle
FILT_TOL = 1e-6        # max |y - y_ref| <= FILT_TOL * max|v| per filtered clip (measured: 2.0e-7, fp64 recurrence)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _oracle():
    from oracle import featurizer_oracle as fo
    fo.build()
    return fo


# every type, the section counts 1..4, a highpass at 50 Hz (poles closest to z = 1) and the largest padlen (27)
SPECS = [("lowpass", 4, 2000.0), ("highpass", 4, 50.0), ("bandpass", 4, (300.0, 3400.0)), ("bandstop", 2, (900.0, 1130.0)),
         ("lowpass", 8, 7000.0), ("highpass", 1, 500.0), ("bandpass", 2, (50.0, 7000.0)), ("lowpass", 3, 5000.0)]


def _voices(rng, N, i16=False, stride=17000):
    x = (0.3 * rng.standard_normal((N, stride))).astype(np.float32)
    x += np.linspace(-0.2, 0.4, stride, dtype=np.float32)[None, :]      # an offset and a ramp: the odd extension's edges matter
    lens = rng.integers(0, stride + 1, N).astype(np.int32)
    # empty, at and around padlen 27 / 6, 7000, 16000, longer than max_samples
    lens[:10] = [0, 1, 6, 7, 27, 28, 7000, 16000, 17000, 16999]
    if i16:
        x = np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16)
    return x, lens


def _vf32(x):
    return x.astype(np.float32) / 32768.0 if x.dtype == np.int16 else x


def _noise(rng):
    return [(0.2 * rng.standard_normal(20000)).astype(np.float32), (0.05 * rng.standard_normal(9000)).astype(np.float32)]


def _rirs(rng):
    out = []
    for n in (1, 50, 3000):
        h = 0.3 * rng.standard_normal(n) * np.exp(-np.arange(n) / 800.0)
        h[0] = 1.0
        out.append(h.astype(np.float32))
    return out


def _reference(aug, clips, used, rescale):
    """float64 filtfilt of the filtered clips (with the rescale), None for dry ones"""
    sel = [b for b in range(len(clips)) if used[b] >= 0]
    ys = filtfilt_batch([aug.filters.sos[used[b]] for b in sel], [clips[b] for b in sel], [int(aug.filters.padlen[used[b]]) for b in sel])
    out = [None] * len(clips)
    for b, y in zip(sel, ys):
        if rescale:
            v = clips[b].astype(np.float64)
            y = y * np.sqrt(np.sum(v * v) / (np.sum(y * y) + len(v) * np.finfo(np.float32).eps))
        out[b] = y
    return out


# ---- 1. draws ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,step", [(1, 3), (0x123456789AB, 1000), (2 ** 63 + 5, 77)])
def test_draws_equal_numpy_hash(torch, seed, step):
    from classifier.params import pr
    from kws_amd.augment import WaveAugment
    rng = np.random.default_rng(1)
    x, lens = _voices(rng, 64)
    wav, vl = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda()
    aug = WaveAugment(None, filters=SPECS, filter_rate=0.6, seed=seed)
    _, L, used = aug.filter(wav, valid_len=vl, step=step, position_base=100)
    want = np_draws(seed, step, 100 + np.arange(64), np.float32(0.6), len(SPECS))
    lv = np.minimum(lens, pr.max_samples)
    want = np.where((want >= 0) & (lv > aug.filters.padlen[np.maximum(want, 0)]), want, -1)   # Lv <= padlen stays dry
    np.testing.assert_array_equal(used.cpu().numpy(), want)
    np.testing.assert_array_equal(L.cpu().numpy(), lv)
    assert (want >= 0).any() and (want < 0).any()


def test_rate_zero_one_shards_and_repeat(torch):
    from kws_amd.augment import WaveAugment
    rng = np.random.default_rng(2)
    x, lens = _voices(rng, 40)
    wav, vl = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda()
    v32 = torch.from_numpy(x).cuda()
    out0, _, used0 = WaveAugment(None, filters=SPECS, filter_rate=0.0, seed=5).filter(wav, valid_len=vl, step=9)
    assert bool((used0 < 0).all())
    for b in range(40):                                                  # dry = the f32 conversion, bit for bit, zeros after
        lv = min(int(lens[b]), out0.shape[1])
        assert torch.equal(out0[b, :lv], v32[b, :lv]) and not out0[b, lv:].any()
    _, _, used1 = WaveAugment(None, filters=SPECS, filter_rate=1.0, seed=5).filter(wav, valid_len=vl, step=9)
    assert bool((used1[10:] >= 0).all())
    aug = WaveAugment(None, filters=SPECS, filter_rate=0.5, seed=6)
    index = torch.from_numpy(rng.integers(0, 40, 50).astype(np.int32)).cuda()
    full = aug.filter(wav, valid_len=vl, index=index, step=4)
    again = aug.filter(wav, valid_len=vl, index=index, step=4)
    a = aug.filter(wav, valid_len=vl, index=index[:23].contiguous(), step=4, position_base=0)
    b = aug.filter(wav, valid_len=vl, index=index[23:].contiguous(), step=4, position_base=23)
    for f, r, p, q in zip(full, again, a, b):
        assert torch.equal(f, r)
        assert torch.equal(f, torch.cat([p, q]))
    other = aug.filter(wav, valid_len=vl, index=index, step=5)
    assert not torch.equal(full[2], other[2])


def test_explicit_choice_and_invalid_values(torch):
    from kws_amd import KwsError
    from kws_amd.augment import WaveAugment
    rng = np.random.default_rng(3)
    x, lens = _voices(rng, 10)
    lens[:] = 9000
    wav, vl = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda()
    aug = WaveAugment(None, filters=SPECS, filter_rate=0.0, seed=1)
    ex = np.array([-1, 0, 1, 2, 3, 4, 5, 6, 7, -1], np.int32)
    out, _, used = aug.filter(wav, valid_len=vl, explicit=ex, filter_used=False)
    np.testing.assert_array_equal(used.cpu().numpy(), ex)
    assert torch.equal(out[0], wav[0, :out.shape[1]] * (torch.arange(out.shape[1], device="cuda") < 9000))
    for bad in ([8] * 10, [-2] * 10):
        with pytest.raises(KwsError):
            aug.filter(wav, valid_len=vl, explicit=np.array(bad, np.int32))
    with pytest.raises(ValueError):
        aug.filter(wav, valid_len=vl, explicit=np.zeros(3, np.int32))


# ---- 2. arithmetic -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i16,rescale", [(False, True), (True, True), (False, False)])
def test_filtfilt_matches_numpy_float64(torch, i16, rescale):
    from classifier.params import pr
    from kws_amd.augment import WaveAugment
    rng = np.random.default_rng(4)
    N = 24
    x, lens = _voices(rng, N, i16)
    index = np.r_[np.arange(N), rng.integers(0, N, 8)].astype(np.int32)
    wav, vl, ix = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(index).cuda()
    aug = WaveAugment(None, filters=SPECS, filter_rate=1.0, rescale=rescale, seed=2)
    ms = pr.max_samples
    B = len(index)
    ex = (np.arange(B) % len(SPECS)).astype(np.int32)
    ex[2:6] = [5, 5, 2, 2]                                               # Lv = padlen (dry) and padlen + 1, padlens 6 and 27
    out, L, used = aug.filter(wav, valid_len=vl, index=ix, explicit=ex, out=torch.full((B, ms + 7), 9.0, device="cuda"))
    out, L, used = out.cpu().numpy(), L.cpu().numpy(), used.cpu().numpy()
    v32 = _vf32(x)
    clips = [v32[index[b], :min(int(lens[index[b]]), ms)] for b in range(B)]
    want_used = np.array([e if len(c) > aug.filters.padlen[e] else -1 for e, c in zip(ex, clips)])
    np.testing.assert_array_equal(used, want_used)
    assert list(used[2:6]) == [-1, 5, -1, 2]
    ref = _reference(aug, clips, used, rescale)
    worst = 0.0
    for b in range(B):
        lv = len(clips[b])
        assert L[b] == lv
        if ref[b] is None:
            assert np.array_equal(out[b, :lv].view(np.int32), clips[b].view(np.int32))
        else:
            err = np.abs(out[b, :lv] - ref[b]).max() / max(np.abs(clips[b]).max(), 1e-30)
            worst = max(worst, err)
            assert err <= FILT_TOL, (b, aug.filters.specs[used[b]], lv, err)
        assert not out[b, lv:].any()                                     # zeros after Lv, out to out_stride
    print("filtfilt max |err| / max|v| = %.3g (i16=%s, rescale=%s)" % (worst, i16, rescale))


def test_in_place_equals_out_of_place_and_rescale_keeps_energy(torch):
    from classifier.params import pr
    from kws_amd.augment import WaveAugment
    rng = np.random.default_rng(5)
    ms = pr.max_samples
    x, lens = _voices(rng, 48, stride=ms)
    wav, vl = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda()
    aug = WaveAugment(None, filters=SPECS, filter_rate=0.7, seed=3)
    want, L, used = aug.filter(wav, valid_len=vl, step=2)
    buf, lens_buf = wav.clone(), vl.clone()
    got, L2, used2 = aug.filter(buf, valid_len=lens_buf, step=2, out=buf, lengths=lens_buf)
    assert got.data_ptr() == buf.data_ptr()
    assert torch.equal(got, want) and torch.equal(L2, L) and torch.equal(used2, used)
    u = used.cpu().numpy()
    y = want.cpu().numpy().astype(np.float64)
    for b in np.nonzero(u >= 0)[0]:
        lv = int(L[b])
        ev = float(np.sum(x[b, :lv].astype(np.float64) ** 2))
        ey = float(np.sum(y[b, :lv] ** 2))
        assert abs(ey / ev - 1.0) <= 1e-5, (b, ey, ev)
    assert (u >= 0).sum() > 10


# ---- 3. the chain and features -------------------------------------------------------------------------------------------------------
def test_reverb_filter_noise_equals_the_stages_run_one_by_one(torch):
    from classifier.params import pr
    from kws_amd.augment import WaveAugment
    from kws_amd.featurizer import Featurizer
    rng = np.random.default_rng(7)
    x, lens = _voices(rng, 32)
    index = rng.integers(0, 32, 70).astype(np.int32)
    wav, vl, ix = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(index).cuda()
    feat = Featurizer(pr)
    ms = feat.geometry["max_samples"]
    noise, rirs = _noise(rng), _rirs(rng)
    aug = WaveAugment(noise, snr=[5, 20], noised_rate=0.6, time_shift_ms=20, seed=12, rirs=rirs, reverb_rate=0.7, filters=SPECS,
                      filter_rate=0.6)
    got = feat(wav, valid_len=vl, index=ix, augment=aug, step=8, position_base=40)
    wet, L, _ = aug.reverberate(wav, valid_len=vl, index=ix, step=8, position_base=40, max_samples=ms)
    flt, L2, used = aug.filter(wet, valid_len=L, step=8, position_base=40, max_samples=ms)
    plan = aug.plan(flt, valid_len=L2, step=8, position_base=40, max_samples=ms)
    rows, L3 = aug.apply(flt, plan, max_samples=ms)
    assert torch.equal(got, feat(rows, valid_len=L3))
    u = used.cpu().numpy()
    assert (u >= 0).any() and (u < 0).any()
    # without reverb: the filter reads wav / index directly
    aug_f = WaveAugment(noise, snr=[5, 20], noised_rate=0.6, seed=12, filters=SPECS, filter_rate=0.6)
    got_f = feat(wav, valid_len=vl, index=ix, augment=aug_f, step=8, position_base=40)
    flt, L2, _ = aug_f.filter(wav, valid_len=vl, index=ix, step=8, position_base=40, max_samples=ms)
    plan = aug_f.plan(flt, valid_len=L2, step=8, position_base=40, max_samples=ms)
    rows, L3 = aug_f.apply(flt, plan, max_samples=ms)
    assert torch.equal(got_f, feat(rows, valid_len=L3))


def test_rate_zero_gives_the_features_of_no_filter(torch):
    from classifier.params import pr
    from kws_amd.augment import WaveAugment
    from kws_amd.featurizer import Featurizer
    rng = np.random.default_rng(6)
    x, lens = _voices(rng, 48, stride=16000)
    index = rng.integers(0, 48, 100).astype(np.int32)
    wav, vl, ix = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(index).cuda()
    feat = Featurizer(pr)
    noise, rirs = _noise(rng), _rirs(rng)
    kw = dict(snr=[0, 10], noised_rate=0.7, time_shift_ms=30, seed=11, rirs=rirs, reverb_rate=0.5)
    assert torch.equal(feat(wav, valid_len=vl, index=ix, augment=WaveAugment(noise, filters=SPECS, filter_rate=0.0, **kw), step=5),
                       feat(wav, valid_len=vl, index=ix, augment=WaveAugment(noise, **kw), step=5))
    nkw = dict(snr=[0, 10], noised_rate=0.7, seed=11)
    assert torch.equal(feat(wav, valid_len=vl, index=ix, augment=WaveAugment(noise, filters=SPECS, filter_rate=0.0, **nkw), step=5),
                       feat(wav, valid_len=vl, index=ix, augment=WaveAugment(noise, **nkw), step=5))
    dry = WaveAugment(None, filters=SPECS, filter_rate=0.0, seed=11)
    assert torch.equal(feat(wav, valid_len=vl, index=ix, augment=dry, step=5), feat(wav, valid_len=vl, index=ix))


@pytest.mark.parametrize("i16", [False, True])
def test_filtered_features_match_the_oracle(torch, i16):
    from classifier.params import pr
    from kws_amd.augment import WaveAugment
    from kws_amd.featurizer import Featurizer
    fo = _oracle()
    rng = np.random.default_rng(8)
    x, lens = _voices(rng, 16, i16)
    wav, vl = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda()
    aug = WaveAugment(None, filters=SPECS, filter_rate=0.8, seed=13)
    got = Featurizer(pr)(wav, valid_len=vl, augment=aug, step=1).cpu().numpy()
    _, _, used = aug.filter(wav, valid_len=vl, step=1)
    used = used.cpu().numpy()
    v32 = _vf32(x)
    clips = [v32[b, :min(int(lens[b]), pr.max_samples)] for b in range(16)]
    ref = _reference(aug, clips, used, True)
    assert (used >= 0).sum() >= 8
    for b in range(16):
        y = clips[b].astype(np.float64) if ref[b] is None else ref[b]
        np.testing.assert_allclose(got[b], fo.audio_to_feature(y), atol=ATOL, rtol=0, err_msg="clip %d" % b)


# ---- 4. training ---------------------------------------------------------------------------------------------------------------------
def test_feature_pipeline_with_filters_equals_direct_calls(torch):
    from classifier.params import pr
    from kws_amd.augment import WaveAugment
    from kws_amd.featurizer import Featurizer
    from kws_amd.pipeline import FeaturePipeline
    rng = np.random.default_rng(9)
    x, lens = _voices(rng, 100, stride=16000)
    wav, vl = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda()
    aug = WaveAugment(_noise(rng), snr=[0, 10], noised_rate=0.6, seed=4, rirs=_rirs(rng), reverb_rate=0.5, filters=SPECS, filter_rate=0.5)
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


def test_fit_with_filters_pipelined_equals_stepwise_and_differs_from_plain(torch):
    from kws_amd.augment import WaveAugment, random_filters
    rng = np.random.default_rng(10)
    C = 4
    x, y, lens = _audio_set(rng, C, 150)
    aug = WaveAugment(None, filters=random_filters(8, seed=1), filter_rate=0.8, seed=8)
    h0, w0 = _fit(torch, x, y, C, False, augment=aug, sample_lengths=lens)
    h1, w1 = _fit(torch, x, y, C, True, augment=aug, sample_lengths=lens)
    assert h0 == h1
    for a, b in zip(w0, w1):
        np.testing.assert_array_equal(a, b)
    hp, wp = _fit(torch, x, y, C, True, sample_lengths=lens)
    assert hp != h1
    assert any(not np.array_equal(a, b) for a, b in zip(wp, w1))
    assert all(np.isfinite(h1[0]))


def test_train_py_end_to_end_with_filters(torch, tmp_path):
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
    spec = importlib.util.spec_from_file_location("kws_train_main_flt_gpu", os.path.join(os.path.dirname(os.path.dirname(__file__)),
                                                                                      "tf-keras-speech-commands_amd", "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    np.random.seed(0)
    logs = tmp_path / "logs"
    hist = train.main(["--train_data_path", str(tmp_path / "data"), "--classes_path", str(tmp_path / "classes.txt"), "--raw_audio",
                       "--filter_rate", "0.5", "--filter_types", "lowpass,bandpass,bandstop", "--num_filters", "6", "--epochs", "2",
                       "--batch_size", "8", "--val_split", "0.25", "--log_dir", str(logs)])
    assert len(hist.history["loss"]) == 2 and all(np.isfinite(hist.history["loss"]))
    assert (logs / "trained_final.npz").exists()
