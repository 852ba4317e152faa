"""GPU tests of the background-noise augmentation (include/kws.h: kws_augment_plan / kws_augment_apply / kws_featurize_gather_augmented,
kws_amd.augment, KWSModel.fit(augment=..., sample_lengths=...), train.py): draws against a numpy restatement of the hash, gains against
numpy float64 (tools/audio_process/add_noise.py:19-35 of the reference), materialised clips, features against the CPU oracle, and the
training paths."""
import os

import numpy as np
import pytest

from aug_ref import M32, np_hash, np_uniform, np_unit

pytestmark = pytest.mark.gpu

ATOL = 2e-4            # the featurizer suite's tolerance against the float64 oracle


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _oracle():
    from oracle import featurizer_oracle as fo
    fo.build()
    return fo


# ---- numpy restatement of csrc/kws_augment.hip's plan (the draws: tests/aug_ref.py) ----------------------------------------------------
def np_plan(seed, step, pos, lv, seg_len, snr, rate, max_shift):
    """-> dict of int / float arrays: the records kws_augment_plan draws for global positions `pos` with voice lengths `lv`"""
    base = (np.asarray(pos, np.uint64) * np.uint64(5)) & M32
    h = [np_hash(seed, step, (base + np.uint64(f)) & M32) for f in range(5)]
    u = np_unit(h[0])
    apply = (u < np.float32(rate)).astype(np.int32)
    seg = np_uniform(h[1], len(seg_len))
    s = np.asarray(snr, np.float32)[np_uniform(h[2], len(snr))]
    sl = np.asarray(seg_len)[seg]
    lk = np.minimum(lv, sl)
    off = np.where(apply == 1, np_uniform(h[3], sl - lk + 1), 0)
    shift = np_uniform(h[4], 2 * max_shift + 1) - max_shift
    length = np.where(apply == 1, lk, lv)
    return dict(apply=apply, segment=seg, snr_db=s, offset=off, shift=shift, length=length, voice_length=np.asarray(lv))


def np_gain(v, n, L, o, snr):
    if L == 0:
        return 0.0
    pv = np.mean(v[:L].astype(np.float64) ** 2)
    pn = np.mean(n[o:o + L].astype(np.float64) ** 2)
    return float(np.sqrt(pv / 10 ** (snr / 10.0) / (pn + np.finfo(np.float32).eps)))


def np_mix(v, n, r):
    """m' of one clip (float32), length L: the contract of kws_augment_apply"""
    L, d = int(r["length"]), int(r["shift"])
    m = v[:L].astype(np.float32)
    if r["apply"]:
        m = (m.astype(np.float64) + np.float64(np.float32(r["gain"])) * n[r["offset"]:r["offset"] + L].astype(np.float64)).astype(np.float32)
    out = np.zeros(L, np.float32)
    t = np.arange(L)
    ok = (t - d >= 0) & (t - d < L)
    out[ok] = m[t[ok] - d]
    return out


def _bank(rng):
    segs = [(0.2 * rng.standard_normal(20000)).astype(np.float32),
            (0.05 * rng.standard_normal(9000)).astype(np.float32),     # shorter than a clip: L < Lv
            np.zeros(16500, np.float32)]                                 # silent: finite gain
    return segs


def _voices(rng, N, i16=False):
    x = (0.3 * rng.standard_normal((N, 16000))).astype(np.float32)
    x[3] = 0.0                                                           # silent voice: g = 0
    lens = rng.integers(0, 16001, N).astype(np.int32)
    lens[:4] = [16000, 16000, 5000, 16000]
    lens[5] = 0
    if i16:
        x = np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16)
    return x, lens


def _vf32(x):
    return x.astype(np.float32) / 32768.0 if x.dtype == np.int16 else x


# ---- 1. draws ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,step", [(1, 3), (0x123456789AB, 1000)])
def test_plan_draws_equal_numpy_hash(torch, seed, step):
    from classifier.params import pr
    from kws_amd.augment import WaveAugment, records
    rng = np.random.default_rng(1)
    segs = _bank(rng)
    x, lens = _voices(rng, 64)
    B = 4096
    index = rng.integers(0, 64, B).astype(np.int32)
    snr = [0, 5, 10, 20]
    aug = WaveAugment(segs, snr=snr, noised_rate=0.3, time_shift_ms=10, seed=seed)
    wav, vl, ix = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(index).cuda()
    r = records(aug.plan(wav, valid_len=vl, index=ix, step=step))
    lv = np.minimum(lens[index], pr.max_samples)
    want = np_plan(seed, step, np.arange(B), lv, [len(s) for s in segs], snr, 0.3, aug.max_shift)
    for k, v in want.items():
        np.testing.assert_array_equal(r[k], v, err_msg=k)
    frac = r["apply"].mean()
    assert abs(frac - 0.3) < 5 * np.sqrt(0.3 * 0.7 / B)
    assert set(r["snr_db"][r["apply"] == 1].tolist()) == set(float(s) for s in snr)
    seg_len = np.array([len(s) for s in segs])
    ap = r["apply"] == 1
    assert (r["offset"] >= 0).all() and (r["offset"][ap] + r["length"][ap] <= seg_len[r["segment"][ap]]).all()
    assert (np.abs(r["shift"]) <= aug.max_shift).all() and r["shift"].min() < 0 < r["shift"].max()
    # a shard planned with position_base = lo draws what the whole batch drew at positions lo..hi
    lo, hi = 1000, 2500
    part = records(aug.plan(wav, valid_len=vl, index=ix[lo:hi].contiguous(), step=step, position_base=lo))
    np.testing.assert_array_equal(part, r[lo:hi])
    # another step, another draw
    other = records(aug.plan(wav, valid_len=vl, index=ix, step=step + 1))
    assert not np.array_equal(other["segment"], r["segment"])


def test_rate_zero_and_one(torch):
    from kws_amd.augment import WaveAugment, records
    rng = np.random.default_rng(2)
    x, lens = _voices(rng, 256)
    wav, vl = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda()
    for rate, want in ((0.0, 0), (1.0, 1)):
        r = records(WaveAugment(_bank(rng), noised_rate=rate, seed=5).plan(wav, valid_len=vl, step=1))
        assert (r["apply"] == want).all()


# ---- 2. gains ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("voice_i16,bank_i16", [(False, False), (True, False), (False, True)])
def test_gains_match_numpy_float64(torch, voice_i16, bank_i16):
    from kws_amd.augment import NoiseBank, WaveAugment, records
    rng = np.random.default_rng(3)
    segs = _bank(rng)
    if bank_i16:
        segs = [np.clip(np.round(s * 32768), -32768, 32767).astype(np.int16) for s in segs]
    bank = NoiseBank(segs)
    nf = bank.as_float32()
    starts = np.concatenate([[0], np.cumsum(bank.seg_len)[:-1]])
    x, lens = _voices(rng, 300, voice_i16)
    aug = WaveAugment(bank, snr=[-5, 0, 10, 30], noised_rate=1.0, seed=11)
    r = records(aug.plan(torch.from_numpy(x).cuda(), valid_len=torch.from_numpy(lens).cuda(), step=2))
    v = _vf32(x)
    seen = set()
    for b in range(300):
        k, o, L = int(r["segment"][b]), int(r["offset"][b]), int(r["length"][b])
        assert L == min(lens[b], bank.seg_len[k])
        n = nf[starts[k]:starts[k] + bank.seg_len[k]]
        g = np_gain(v[b], n, L, o, float(r["snr_db"][b]))
        np.testing.assert_allclose(r["gain"][b], g, rtol=1e-5, atol=0, err_msg="clip %d" % b)
        assert np.isfinite(r["gain"][b])
        seen.add(("silent voice" if b == 3 else "short segment" if k == 1 and L < lens[b] else "silent noise" if k == 2 else "other"))
    assert r["gain"][3] == 0.0 and r["gain"][5] == 0.0 and r["length"][5] == 0
    assert {"silent voice", "short segment", "silent noise"} <= seen


# ---- 3. apply ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("voice_i16", [False, True])
def test_apply_materialises_the_mix(torch, voice_i16):
    from classifier.params import pr
    from kws_amd.augment import NoiseBank, WaveAugment, records
    rng = np.random.default_rng(4)
    bank = NoiseBank(_bank(rng))
    nf = bank.as_float32()
    starts = np.concatenate([[0], np.cumsum(bank.seg_len)[:-1]])
    x, lens = _voices(rng, 40, voice_i16)
    index = rng.integers(0, 40, 96).astype(np.int32)
    aug = WaveAugment(bank, snr=[0, 10], noised_rate=0.7, time_shift_ms=50, seed=7)
    wav, vl, ix = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(index).cuda()
    plan = aug.plan(wav, valid_len=vl, index=ix, step=9)
    rows, L = aug.apply(wav, plan, index=ix)
    rows, L, r = rows.cpu().numpy(), L.cpu().numpy(), records(plan)
    np.testing.assert_array_equal(L, r["length"])
    v = _vf32(x)
    for b in range(96):
        k = int(r["segment"][b])
        want = np_mix(v[index[b]], nf[starts[k]:starts[k] + bank.seg_len[k]], r[b])
        np.testing.assert_allclose(rows[b, :L[b]], want, rtol=0, atol=1e-6)
        assert not rows[b, L[b]:pr.max_samples].any()
    # an explicit plan with odd offsets and shifts
    ex = np.zeros(96, r.dtype)
    ex["apply"], ex["segment"], ex["offset"], ex["shift"], ex["snr_db"] = 1, 0, 777, -333, 3.0
    ex["shift"][1::2] = 1235
    rows2, L2 = aug.apply(wav, aug.plan(wav, valid_len=vl, index=ix, explicit=ex), index=ix)
    r2 = records(aug.plan(wav, valid_len=vl, index=ix, explicit=ex))
    for b in range(0, 96, 7):
        assert r2["offset"][b] == min(777, bank.seg_len[0] - r2["length"][b])
        want = np_mix(v[index[b]], nf[:bank.seg_len[0]], r2[b])
        np.testing.assert_allclose(rows2.cpu().numpy()[b, :L2[b]], want, rtol=0, atol=1e-6)


def test_explicit_plan_out_of_range_is_invalid(torch):
    from kws_amd import KwsError
    from kws_amd.augment import WaveAugment
    rng = np.random.default_rng(5)
    segs = _bank(rng)
    aug = WaveAugment(segs, seed=1)
    wav = torch.zeros((2, 16000), device="cuda")
    ex = np.zeros(2, [("apply", "<i4"), ("segment", "<i4"), ("offset", "<i4"), ("shift", "<i4"), ("length", "<i4"),
                      ("snr_db", "<f4"), ("gain", "<f4"), ("voice_length", "<i4")])
    for field, val in (("segment", 3), ("segment", -1), ("offset", 20000), ("offset", -2)):
        e = ex.copy()
        e[field][1] = val
        with pytest.raises(KwsError) as err:
            aug.plan(wav, explicit=e)
        assert err.value.code == -1


# ---- 4. / 5. features ----------------------------------------------------------------------------------------------------------------
def _check_features(torch, feat, fo, x, lens, index, aug, step, oracle_kw, bit_exact_apply):
    from kws_amd.augment import records
    wav, vl, ix = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(index).cuda()
    got = feat(wav, valid_len=vl, index=ix, augment=aug, step=step)
    ms = feat.geometry["max_samples"]
    plan = aug.plan(wav, valid_len=vl, index=ix, step=step, max_samples=ms)
    rows, L = aug.apply(wav, plan, index=ix, max_samples=ms)
    via_apply = feat(rows, valid_len=L)
    if bit_exact_apply:
        assert torch.equal(got, via_apply)
    got, r = got.cpu().numpy(), records(plan)
    nf = aug.noise.as_float32()
    starts = np.concatenate([[0], np.cumsum(aug.noise.seg_len)[:-1]])
    v = _vf32(x)
    for b in range(0, len(index), max(1, len(index) // 12)):
        k = int(r["segment"][b])
        m = np_mix(v[index[b]], nf[starts[k]:starts[k] + aug.noise.seg_len[k]], r[b])
        want = fo.audio_to_feature(m.astype(np.float64), **oracle_kw)
        np.testing.assert_allclose(got[b], want, atol=ATOL, rtol=0, err_msg="clip %d" % b)
    return r


@pytest.mark.parametrize("voice_i16", [False, True])
def test_fused_featurize_matches_oracle_and_apply(torch, voice_i16):
    from classifier.params import pr
    from kws_amd.augment import WaveAugment
    from kws_amd.featurizer import Featurizer
    fo = _oracle()
    rng = np.random.default_rng(6)
    x, lens = _voices(rng, 48, voice_i16)
    index = rng.integers(0, 48, 200).astype(np.int32)
    aug = WaveAugment(_bank(rng), snr=[0, 10, 20], noised_rate=0.75, time_shift_ms=60, seed=21)
    for share in (2, 1):
        feat = Featurizer(pr)
        feat.set_cu_share(share)
        r = _check_features(torch, feat, fo, x, lens, index, aug, 4, {}, True)
    assert r["apply"].any() and not r["apply"].all() and (r["shift"] % 2 == 1).any()


@pytest.mark.parametrize("case", ["legacy", "generic"])
def test_other_configurations_featurize_apply(torch, case):
    from classifier.params import ListenerParams
    from kws_amd.augment import WaveAugment
    from kws_amd.featurizer import Featurizer
    fo = _oracle()
    if case == "legacy":       # n_fft = 1024 outside the tuned kernel: featurize_fft1024_kernel
        kw = dict(n_filt=40, n_mfcc=13)
        p = ListenerParams(1.0, 0.064, 0.032, 16000, 2, 1024, 40, 13, False, ((6, 4),), 0.2)
    else:                      # n_fft = 512: the generic radix-2 kernel
        kw = dict(n_fft=512, window_t=0.032, hop_t=0.016, n_filt=20, n_mfcc=13)
        p = ListenerParams(1.0, 0.032, 0.016, 16000, 2, 512, 20, 13, False, ((6, 4),), 0.2)
    rng = np.random.default_rng(7)
    x, lens = _voices(rng, 24)
    index = rng.integers(0, 24, 40).astype(np.int32)
    aug = WaveAugment(_bank(rng), snr=[5, 15], noised_rate=0.8, time_shift_ms=30, seed=3)
    _check_features(torch, Featurizer(p), fo, x, lens, index, aug, 2, kw, True)


@pytest.mark.parametrize("voice_i16", [False, True])
def test_rate_zero_without_shift_is_the_plain_featurizer(torch, voice_i16):
    from classifier.params import pr
    from kws_amd.augment import WaveAugment
    from kws_amd.featurizer import Featurizer
    rng = np.random.default_rng(8)
    x, lens = _voices(rng, 64, voice_i16)
    index = rng.integers(0, 64, 500).astype(np.int32)
    wav, vl, ix = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(index).cuda()
    feat = Featurizer(pr)
    aug = WaveAugment(_bank(rng), noised_rate=0.0, seed=1)
    assert torch.equal(feat(wav, valid_len=vl, index=ix, augment=aug, step=3), feat(wav, valid_len=vl, index=ix))
    assert torch.equal(feat(wav, index=ix, augment=aug, step=3), feat(wav, index=ix))


# ---- 6. pipeline ---------------------------------------------------------------------------------------------------------------------
def test_feature_pipeline_with_augment_equals_direct_calls(torch):
    from classifier.params import pr
    from kws_amd.augment import WaveAugment
    from kws_amd.featurizer import Featurizer
    from kws_amd.pipeline import FeaturePipeline
    rng = np.random.default_rng(9)
    x, lens = _voices(rng, 100)
    wav, vl = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda()
    aug = WaveAugment(_bank(rng), snr=[0, 10], noised_rate=0.6, time_shift_ms=20, seed=4)
    pipe = FeaturePipeline(Featurizer(pr), 64, pr.n_features, pr.feature_size)
    direct = Featurizer(pr)
    idx = [torch.from_numpy(rng.integers(0, 100, n).astype(np.int32)).cuda() for n in (64, 64, 30)]
    for j, ix in enumerate(idx):
        pipe.submit(wav=wav, valid_len=vl, index=ix, augment=aug, step=10 + j, position_base=5 * j)
        got = pipe.take().clone()
        pipe.release()
        want = direct(wav, valid_len=vl, index=ix, augment=aug, step=10 + j, position_base=5 * j)
        assert torch.equal(got, want)
    with pytest.raises(ValueError):
        pipe.submit(features=torch.zeros((4, pr.n_features, pr.feature_size), device="cuda"), augment=aug)


# ---- 7. fit --------------------------------------------------------------------------------------------------------------------------
def _audio_set(rng, C, N, ragged=False):
    y = rng.integers(0, C, N)
    tones = np.sin(2 * np.pi * (300.0 * (1 + np.arange(C)))[:, None] * np.arange(16000)[None, :] / 16000.0)
    x = (0.3 * tones[y] + 0.05 * rng.standard_normal((N, 16000))).astype(np.float32)
    lens = np.full(N, 16000, np.int32)
    if ragged:
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


def test_fit_augmented_pipelined_equals_stepwise_and_differs_from_plain(torch):
    from kws_amd.augment import WaveAugment
    rng = np.random.default_rng(10)
    C = 4
    x, y, lens = _audio_set(rng, C, 150, ragged=True)
    aug = WaveAugment(_bank(rng), snr=[0, 10], noised_rate=0.8, time_shift_ms=40, seed=8)
    h0, w0 = _fit(torch, x, y, C, False, augment=aug, sample_lengths=lens)
    h1, w1 = _fit(torch, x, y, C, True, augment=aug, sample_lengths=lens)
    assert h0 == h1
    for a, b in zip(w0, w1):
        np.testing.assert_array_equal(a, b)
    hp, wp = _fit(torch, x, y, C, True, sample_lengths=lens)
    assert hp != h1
    assert any(not np.array_equal(a, b) for a, b in zip(wp, w1))
    assert all(np.isfinite(h1[0]))


def test_fit_feature_input_with_augment_raises(torch):
    from classifier.loss import SparseCategoricalCrossEntropy
    from classifier.model import KWSModel
    from common.model_utils import get_optimizer
    from kws_amd.augment import WaveAugment
    m = KWSModel("simple_cnn", 3, seed=1)
    m.compile(optimizer=get_optimizer("adam", 1e-3), loss=SparseCategoricalCrossEntropy(), metrics=["accuracy"])
    x = np.zeros((8, 30, 20, 1), np.float32)
    with pytest.raises(ValueError):
        m.fit(x, np.zeros(8), batch_size=4, epochs=1, verbose=0, augment=WaveAugment([np.ones(100, np.float32)], seed=1))


def test_fit_ragged_audio_equals_fit_on_extracted_features(torch):
    """fit(raw audio, sample_lengths) trains on exactly the features extract_features makes (keep the head, left-pad zeros)"""
    from common.data_utils import get_featurizer
    rng = np.random.default_rng(11)
    C = 3
    x, y, lens = _audio_set(rng, C, 130, ragged=True)
    feats = get_featurizer()(torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda()).cpu().numpy()[..., None]
    for pipelined in (True, False):
        ha, _ = _fit(torch, x, y, C, pipelined, sample_lengths=lens)
        hf, _ = _fit(torch, feats, y, C, pipelined)
        assert ha == hf


# ---- 8. train.py ---------------------------------------------------------------------------------------------------------------------
def test_train_py_end_to_end_with_noise(torch, tmp_path):
    import importlib.util
    from common.data_utils import save_audio
    from kws_amd.augment import white_noise
    rng = np.random.default_rng(12)
    classes = ["background", "yes", "no"]
    for c, cls in enumerate(classes):
        d = tmp_path / "data" / "sounds" / cls
        d.mkdir(parents=True)
        for i in range(12):
            n = int(rng.integers(6000, 16001))
            t = np.arange(n) / 16000.0
            save_audio(str(d / ("%d.wav" % i)), 0.3 * np.sin(2 * np.pi * 400.0 * (c + 1) * t) + 0.02 * rng.standard_normal(n))
    (tmp_path / "noise").mkdir()
    save_audio(str(tmp_path / "noise" / "white.wav"), white_noise(3000, seed=1).astype(np.float32) / 32768.0)
    save_audio(str(tmp_path / "noise" / "hum.wav"), 0.1 * np.sin(2 * np.pi * 50.0 * np.arange(20000) / 16000.0))
    (tmp_path / "classes.txt").write_text("\n".join(classes) + "\n")
    spec = importlib.util.spec_from_file_location("kws_train_main", os.path.join(os.path.dirname(os.path.dirname(__file__)),
                                                                              "tf-keras-speech-commands_amd", "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    np.random.seed(0)
    logs = tmp_path / "logs"
    hist = train.main(["--train_data_path", str(tmp_path / "data"), "--classes_path", str(tmp_path / "classes.txt"), "--raw_audio",
                       "--noise_path", str(tmp_path / "noise"), "--snr", "5,10,20", "--noised_rate", "0.7", "--time_shift_ms", "50",
                       "--epochs", "2", "--batch_size", "8", "--val_split", "0.25", "--log_dir", str(logs)])
    assert len(hist.history["loss"]) == 2 and all(np.isfinite(hist.history["loss"]))
    assert (logs / "trained_final.npz").exists()
    assert any(p.name.startswith("ep") and p.suffix == ".npz" for p in logs.iterdir())
    assert (logs / "train_log.jsonl").read_text().count("\n") == 2
