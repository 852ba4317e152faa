"""GPU tests of the speed and loudness perturbation (include/kws.h: kws_resampler_*, kws_speed_apply; kws_amd.augment.Resampler,
WaveAugment.perturb, resample): the interpolation against the float64 numpy restatement of tests/speed_ref.py within the float32
product-and-sum bound, the level, the draws against the numpy hash, sharding, determinism, the featurizer's chain, resample() and fit."""
import math

import numpy as np
import pytest

import speed_ref as sr

pytestmark = pytest.mark.gpu

MS, STRIDE, OUT_STRIDE = 512, 1100, 520
RATIOS = (0.5, 0.8, 1.0, 1.25, 2.0, 0.0)
LENGTHS = (0, 1, 7, 300, 640, 1100)
TABLES = {"default": (16, 512), "small": (4, 32)}
U = 2.0 ** -24


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def tables():
    from kws_amd.augment import Resampler
    out = {}
    for name, (Z, P) in TABLES.items():
        out[name] = (Resampler(zero_crossings=Z, phases=P), sr.table(Z, P, sr.DEFAULTS["beta"], sr.DEFAULTS["rolloff"]), Z, P)
    return out


def _source(i16, rows=len(LENGTHS), stride=STRIDE, seed=0):
    """loud clips (mean square about 0.09, so that FLT_EPSILON in the gain is 1e-6 of it) with a loud first sample"""
    rng = np.random.default_rng(seed)
    x = (0.3 * rng.standard_normal((rows, stride))).astype(np.float32)
    x[:, 0] = 0.3
    if i16:
        x = np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16)
    return x


def _f32(x):
    return x.astype(np.float32) / np.float32(32768.0) if x.dtype == np.int16 else x


def _grid():
    """every ratio with every source length: (ratio, row) per clip, row = the index of the length"""
    ex = np.array([r for r in RATIOS for _ in LENGTHS], np.float32)
    rows = np.array([j for _ in RATIOS for j in range(len(LENGTHS))], np.int32)
    return ex, rows


def _check_resampled(out, L, ex, rows, lens, v32, h, Z, P, gains=None, what=""):
    """every clip against the restatement: exact lengths, the float32 bound per sample, bit equality for r = 0, zeros after L'"""
    worst = 0.0
    for b in range(len(ex)):
        v = v32[rows[b], :lens[rows[b]]]
        ref = sr.perturb(v, ex[b], float("nan"), MS, h, Z, P)
        lp = len(ref["y"])
        assert L[b] == lp == (min(len(v), MS) if ex[b] == 0 else sr.out_length(len(v), ex[b], MS)), (what, b)
        assert not out[b, lp:].any(), (what, b)
        got = out[b, :lp].astype(np.float64)
        if gains is not None:
            got = got / float(gains[b])
        if ex[b] == 0 and gains is None:
            assert np.array_equal(out[b, :lp].view(np.int32), v[:lp].view(np.int32)), (what, b)
            continue
        tol = 2.0 * (ref["T"] + 3) * U * ref["A"]           # also for out / gain: the product with the gain is one of the "+ 3"
        err = np.abs(got - ref["y"])
        assert np.all(err <= tol), (what, b, float(ex[b]), len(v), int(np.argmax(err - tol)), float(err.max()), float(tol.max()))
        if lp:
            worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
    return worst


# ---- 1. the interpolation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["default", "small"])
@pytest.mark.parametrize("i16", [False, True])
def test_resampling_matches_the_float64_restatement(torch, tables, table, i16):
    from kws_amd.augment import WaveAugment
    rs, h, Z, P = tables[table]
    x = _source(i16)
    lens = np.array(LENGTHS, np.int32)
    ex, rows = _grid()
    wav, vl, ix = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(rows).cuda()
    aug = WaveAugment(None, speed=(1.0, 1.0), speed_rate=0.0, resampler=rs, seed=1)
    buf = torch.full((len(ex), OUT_STRIDE), 9.0, device="cuda")
    out, L, used, gain = aug.perturb(wav, valid_len=vl, index=ix, explicit_speed=ex, max_samples=MS, out=buf)
    assert out.data_ptr() == buf.data_ptr()
    np.testing.assert_array_equal(used.cpu().numpy(), ex)
    np.testing.assert_array_equal(gain.cpu().numpy(), np.ones(len(ex), np.float32))
    worst = _check_resampled(out.cpu().numpy(), L.cpu().numpy(), ex, rows, lens, _f32(x), h, Z, P, what=table)
    print("resampling, %s table, i16=%s: worst error / bound = %.3g" % (table, i16, worst))
    L = L.cpu().numpy().reshape(len(RATIOS), len(LENGTHS))
    assert list(L[4]) == [0, 1, 4, 150, 320, 512] and list(L[0]) == [0, 2, 14, 512, 512, 512]     # r = 2 and r = 0.5
    # without index and without valid_len: every row whole, r = 2 reads to the end of the row
    ex2 = np.array(RATIOS, np.float32)
    out2, L2, _, _ = aug.perturb(wav, explicit_speed=ex2, max_samples=MS, out=torch.full((len(ex2), OUT_STRIDE), 9.0, device="cuda"))
    _check_resampled(out2.cpu().numpy(), L2.cpu().numpy(), ex2, np.arange(len(ex2)), np.full(len(ex2), STRIDE), _f32(x), h, Z, P, what="rows")
    assert list(L2.cpu().numpy()) == [512, 512, 512, 512, 512, 512]


def test_invalid_arguments_are_refused(torch, tables):
    from kws_amd import KwsError
    from kws_amd import lib as l
    from kws_amd.augment import WaveAugment
    import ctypes
    rs = tables["small"][0]
    wav = torch.from_numpy(_source(False)).cuda()
    aug = WaveAugment(None, speed=(0.9, 1.1), resampler=rs, seed=1)
    B = wav.shape[0]
    for bad in ([0.4] * B, [2.5] * B, [float("nan")] * B, [-1.0] * B):
        with pytest.raises(KwsError):
            aug.perturb(wav, explicit_speed=np.array(bad, np.float32), max_samples=MS)
    for bad in ([1.0] * B, [-81.0] * B, [float("inf")] * B):
        with pytest.raises(KwsError):
            aug.perturb(wav, explicit_db=np.array(bad, np.float32), max_samples=MS)
    with pytest.raises(ValueError):
        aug.perturb(wav, explicit_speed=np.zeros(3, np.float32), max_samples=MS)
    level_only = WaveAugment(None, loudness=(-30, -15), seed=1)
    with pytest.raises(ValueError, match="no resampler"):                             # and the object stays without one
        level_only.perturb(wav, explicit_speed=np.full(B, 1.25, np.float32), max_samples=MS)
    assert level_only.resampler is None
    with pytest.raises(ValueError):
        aug.perturb(wav, max_samples=MS, out=torch.empty((B, MS - 1), device="cuda"))
    L = l.get_lib()
    out, lens = torch.empty((B, MS), device="cuda"), torch.empty((B,), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(p, handle=rs.handle(), out_stride=MS, lengths=lens):
        return L.kws_speed_apply(handle, ctypes.byref(p), wav.data_ptr(), l.WAV_F32, None, B, STRIDE, None, 0, 0, None, None, out.data_ptr(),
                                 out_stride, lengths.data_ptr() if lengths is not None else None, None, None, stream)

    good = aug.speed_params(MS)
    assert call(good) == 0
    for field, value, word in (("speed_rate", 1.5, "speed_rate"), ("loud_rate", -0.5, "loud_rate"), ("speed_lo", 0.4, "speed range"),
                               ("speed_hi", 0.8, "speed range"), ("max_samples", 0, "max_samples")):
        p = aug.speed_params(MS)
        setattr(p, field, value)
        assert call(p) == l.ERR_INVALID and word in L.kws_last_error().decode(), field
    p = aug.speed_params(MS)
    p.loud_rate, p.loud_lo_db, p.loud_hi_db = 1.0, -10.0, 5.0
    assert call(p) == l.ERR_INVALID and "loudness range" in L.kws_last_error().decode()
    assert call(good, handle=None) == l.ERR_INVALID and "resampler" in L.kws_last_error().decode()
    assert call(good, out_stride=MS - 1) == l.ERR_INVALID and "out_stride" in L.kws_last_error().decode()
    assert call(good, lengths=None) == l.ERR_INVALID
    torch.cuda.synchronize()


# ---- 2. the level --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i16", [False, True])
def test_loudness_alone(torch, i16):
    from kws_amd.augment import WaveAugment
    x = _source(i16, rows=6, seed=3)
    x[4] = 0                                                 # a silent clip
    lens = np.array([1100, 300, 640, 7, 500, 1], np.int32)   # the last one: L' = 1
    db = np.array([-40.0, -20.0, -6.0, float("nan"), -20.0, -20.0], np.float32)
    wav, vl = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda()
    aug = WaveAugment(None, loudness=(-30, -15), loudness_rate=0.0, seed=1)           # no resampler at all
    assert aug.resampler is None
    out, L, used, gain = aug.perturb(wav, valid_len=vl, explicit_speed=np.zeros(6, np.float32), explicit_db=db, max_samples=MS,
                                     out=torch.full((6, OUT_STRIDE), 9.0, device="cuda"))
    out, L, gain = out.cpu().numpy(), L.cpu().numpy(), gain.cpu().numpy()
    assert not used.cpu().numpy().any()
    v32 = _f32(x)
    for b in range(6):
        lp = min(int(lens[b]), MS)
        v = v32[b, :lp]
        assert L[b] == lp and not out[b, lp:].any()
        g = sr.gain(v, db[b]) if not np.isnan(db[b]) else np.float32(1.0)
        print("clip %d: gain %.9g (restatement %.9g)" % (b, gain[b], g))
        np.testing.assert_allclose(gain[b], g, rtol=1e-6, atol=0)
        assert np.array_equal(out[b, :lp].view(np.int32), (gain[b] * v).astype(np.float32).view(np.int32)), b
        if b == 3:
            assert gain[b] == 1.0
        elif b == 4:
            assert not out[b].any() and np.isfinite(gain[b])                          # a silent clip stays silent
        else:
            level = sr.level_db(out[b, :lp])
            print("clip %d: level %.7f dB, target %g" % (b, level, db[b]))
            assert abs(level - db[b]) <= 1e-4, (b, level, db[b])


def test_speed_and_loudness_together(torch, tables):
    from kws_amd.augment import WaveAugment
    rs, h, Z, P = tables["default"]
    x = _source(True, seed=4)
    lens = np.array(LENGTHS, np.int32)
    ex, rows = _grid()
    db = np.resize(np.array([-40.0, -20.0, -6.0, -33.5], np.float32), len(ex))
    wav, vl, ix = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(rows).cuda()
    aug = WaveAugment(None, speed=(1.0, 1.0), speed_rate=0.0, resampler=rs, seed=1)
    out, L, used, gain = aug.perturb(wav, valid_len=vl, index=ix, explicit_speed=ex, explicit_db=db, max_samples=MS,
                                     out=torch.full((len(ex), OUT_STRIDE), 9.0, device="cuda"))
    out, L, gain = out.cpu().numpy(), L.cpu().numpy(), gain.cpu().numpy()
    assert np.all(np.isfinite(gain)) and np.all(gain > 0)
    _check_resampled(out, L, ex, rows, lens, _f32(x), h, Z, P, gains=gain, what="both")
    for b in range(len(ex)):
        if L[b]:
            level = sr.level_db(out[b, :L[b]])
            assert abs(level - db[b]) <= 1e-4, (b, float(ex[b]), int(L[b]), level, db[b])


# ---- 3. draws, shards, determinism ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [3, 4])
def test_drawn_mode_equals_the_numpy_hash(torch, tables, step):
    from kws_amd.augment import WaveAugment
    rs, h, Z, P = tables["small"]
    B, seed, base = 64, 0x123456789AB, 1000
    x = _source(False, rows=B, seed=5)
    lens = np.random.default_rng(6).integers(200, STRIDE + 1, B).astype(np.int32)
    wav, vl = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda()
    kw = dict(speed=(0.8, 1.25), speed_rate=0.6, loudness=(-30, -10), loudness_rate=0.5, resampler=rs, seed=seed)
    aug = WaveAugment(None, **kw)
    out, L, used, gain = aug.perturb(wav, valid_len=vl, step=step, position_base=base, max_samples=MS)
    again = aug.perturb(wav, valid_len=vl, step=step, position_base=base, max_samples=MS)
    for a, b in zip((out, L, used, gain), again):
        assert torch.equal(a, b)                                                      # two calls: the same bits
    on, r, lev, tg = sr.np_draws(seed, step, base + np.arange(B), 0.6, (0.8, 1.25), 0.5, (-30.0, -10.0))
    u, g = used.cpu().numpy(), gain.cpu().numpy()
    np.testing.assert_array_equal(u != 0, on)
    np.testing.assert_array_equal(g != 1, lev)
    assert on.any() and (~on).any() and lev.any() and (~lev).any()
    np.testing.assert_allclose(u[on], r[on], rtol=1e-6)
    o, Ln = out.cpu().numpy(), L.cpu().numpy()
    _check_resampled(o, Ln, u, np.arange(B), lens, x, h, Z, P, gains=g, what="drawn")  # with the ratios the device reports
    for b in np.nonzero(lev)[0]:
        got_db = 10.0 * math.log10(float(g[b]) ** 2 * (np.mean((o[b, :Ln[b]].astype(np.float64) / float(g[b])) ** 2) + sr.EPS32))
        np.testing.assert_allclose(got_db, tg[b], rtol=1e-6, atol=0)               # the target, back from the gain
    # shards: 64 clips in one call = two calls of 32 at their positions
    idx = torch.arange(B, dtype=torch.int32, device="cuda")
    lo = aug.perturb(wav, valid_len=vl, index=idx[:32].contiguous(), step=step, position_base=base, max_samples=MS)
    hi = aug.perturb(wav, valid_len=vl, index=idx[32:].contiguous(), step=step, position_base=base + 32, max_samples=MS)
    for full, p, q in zip((out, L, used, gain), lo, hi):
        assert torch.equal(full, torch.cat([p, q]))
    if step == 3:
        off = WaveAugment(None, **dict(kw, speed_rate=0.0, loudness_rate=0.0)).perturb(wav, valid_len=vl, step=step, max_samples=MS)
        assert not off[2].any() and bool((off[3] == 1).all())
        for b in range(B):
            lp = min(int(lens[b]), MS)
            assert torch.equal(off[0][b, :lp], wav[b, :lp]) and not off[0][b, lp:].any()
        allon = WaveAugment(None, **dict(kw, speed_rate=1.0, loudness_rate=1.0)).perturb(wav, valid_len=vl, step=step, max_samples=MS)
        assert bool((allon[2] != 0).all()) and bool((allon[3] != 1).all())


# ---- 4. the chain at the default geometry --------------------------------------------------------------------------------------------
def _clips(torch, N=6, seed=7):
    rng = np.random.default_rng(seed)
    x = (0.2 * rng.standard_normal((N, 17000))).astype(np.float32)
    lens = np.array([17000, 16000, 9000, 0, 12345, 30][:N], np.int32)
    return torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda(), rng


def test_chain_equals_the_stages_run_one_by_one(torch):
    from classifier.params import pr
    from kws_amd.augment import WaveAugment
    from kws_amd.featurizer import Featurizer
    wav, vl, rng = _clips(torch)
    ix = torch.from_numpy(np.array([5, 0, 1, 2, 2, 3, 4], np.int32)).cuda()
    feat = Featurizer(pr)
    ms = feat.geometry["max_samples"]
    noise = [(0.2 * rng.standard_normal(20000)).astype(np.float32)]
    rirs = [np.r_[1.0, 0.3 * rng.standard_normal(400) * np.exp(-np.arange(400) / 100.0)].astype(np.float32)]
    filters = [("lowpass", 4, 3000.0), ("highpass", 2, 200.0)]
    sp = dict(speed=(0.8, 1.25), speed_rate=0.7, loudness=(-30, -15), loudness_rate=0.7)
    nz = dict(snr=[5, 20], noised_rate=0.6, time_shift_ms=20, seed=12)
    kw = dict(valid_len=vl, index=ix, step=3, position_base=40)
    # speed + loudness + noise
    aug = WaveAugment(noise, **nz, **sp)
    got = feat(wav, augment=aug, **kw)
    out, L, used, gain = aug.perturb(wav, max_samples=ms, **kw)
    plan = aug.plan(out, valid_len=L, step=3, position_base=40, max_samples=ms)
    rows, L2 = aug.apply(out, plan, max_samples=ms)
    assert torch.equal(got, feat(rows, valid_len=L2))
    u = used.cpu().numpy()
    assert (u != 0).any()
    # speed + loudness only
    only = WaveAugment(None, seed=12, **sp)
    assert torch.equal(feat(wav, augment=only, **kw), feat(out, valid_len=L))
    # every stage: perturb, reverb, filter, noise
    full = WaveAugment(noise, rirs=rirs, reverb_rate=0.7, filters=filters, filter_rate=0.6, **nz, **sp)
    got = feat(wav, augment=full, **kw)
    wet, Lw, _ = full.reverberate(out, valid_len=L, step=3, position_base=40, max_samples=ms)
    flt, Lf, _ = full.filter(wet, valid_len=Lw, step=3, position_base=40, max_samples=ms)
    plan = full.plan(flt, valid_len=Lf, step=3, position_base=40, max_samples=ms)
    rows, L3 = full.apply(flt, plan, max_samples=ms)
    assert torch.equal(got, feat(rows, valid_len=L3))
    # an augment without the new options: the bits of the existing stage functions called directly
    old = WaveAugment(noise, rirs=rirs, reverb_rate=0.7, filters=filters, filter_rate=0.6, **nz)
    assert not old.perturbs
    got = feat(wav, augment=old, **kw)
    wet, Lw, _ = old.reverberate(wav, max_samples=ms, **kw)
    flt, Lf, _ = old.filter(wet, valid_len=Lw, step=3, position_base=40, max_samples=ms)
    plan = old.plan(flt, valid_len=Lf, step=3, position_base=40, max_samples=ms)
    rows, L3 = old.apply(flt, plan, max_samples=ms)
    assert torch.equal(got, feat(rows, valid_len=L3))
    noise_only = WaveAugment(noise, **nz)
    plan = noise_only.plan(wav, max_samples=ms, **kw)
    rows, L4 = noise_only.apply(wav, plan, index=ix, max_samples=ms)
    assert torch.equal(feat(wav, augment=noise_only, **kw), feat(rows, valid_len=L4))


def test_resample_is_the_restatement_at_a_fixed_ratio(torch, tables):
    from kws_amd.augment import resample
    rs, h, Z, P = tables["default"]
    x = _source(False, rows=3, stride=400, seed=8)
    wav = torch.from_numpy(x).cuda()
    got = resample(wav, 8000, 16000)
    assert got.shape == (3, 800) and got.dtype == torch.float32
    assert torch.equal(got, resample(wav, 8000, 16000, resampler=rs))
    got = got.cpu().numpy()
    for b in range(3):
        y, A, T = sr.resample(x[b], 0.5, 800, h, Z, P)
        assert len(y) == 800 and np.all(np.abs(got[b] - y) <= 2.0 * (T + 3) * U * A), b
    down = resample(torch.from_numpy(_source(True, rows=2, stride=401, seed=9)).cuda(), 16000, 8000)
    assert down.shape == (2, 201)
    assert torch.equal(resample(wav, 16000, 16000), wav)
    with pytest.raises(ValueError):
        resample(wav, 48000, 16000)


# ---- 5. training ---------------------------------------------------------------------------------------------------------------------
def _fit(torch, x, y, C, pipelined, **kw):
    from classifier.loss import SparseCategoricalCrossEntropy
    from classifier.model import KWSModel
    from common.model_utils import get_optimizer
    torch.manual_seed(1234)
    m = KWSModel("simple_cnn_lite", C, seed=3)
    m._device().set_deterministic(True)
    m.compile(optimizer=get_optimizer("adam", 1e-3), loss=SparseCategoricalCrossEntropy(), metrics=["accuracy"])
    h = m.fit(x, y, batch_size=32, epochs=2, verbose=0, shuffle=True, pipeline=pipelined, **kw)
    return (h.history["loss"], h.history["accuracy"]), m.get_weights()


def test_fit_with_speed_and_loudness_pipelined_equals_stepwise(torch):
    from kws_amd.augment import WaveAugment
    rng = np.random.default_rng(10)
    C, N = 4, 64
    y = rng.integers(0, C, N)
    tones = np.sin(2 * np.pi * (300.0 * (1 + np.arange(C)))[:, None] * np.arange(16000)[None, :] / 16000.0)
    x = (0.3 * tones[y] + 0.05 * rng.standard_normal((N, 16000))).astype(np.float32)
    lens = rng.integers(4000, 16001, N).astype(np.int32)
    aug = WaveAugment(None, speed=(0.9, 1.1), loudness=(-30, -15), seed=8)
    h0, w0 = _fit(torch, x, y, C, False, augment=aug, sample_lengths=lens)
    h1, w1 = _fit(torch, x, y, C, True, augment=aug, sample_lengths=lens)
    assert h0 == h1 and all(np.isfinite(h1[0]))
    for a, b in zip(w0, w1):
        np.testing.assert_array_equal(a, b)
    hp, wp = _fit(torch, x, y, C, True, sample_lengths=lens)
    assert hp != h1 and any(not np.array_equal(a, b) for a, b in zip(wp, w1))
