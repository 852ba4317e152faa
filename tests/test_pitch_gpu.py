"""GPU tests of the tempo and pitch perturbation (include/kws.h: kws_pitch_stft, kws_pitch_apply; kws_amd.augment.WaveAugment.pitch_perturb,
time_stretch, pitch_shift, stft) against the float64 numpy restatement of tests/pitch_ref.py.

A phase vocoder is ill-conditioned where a bin sits at the rounding floor: the angle of a near-zero D is noise and enters the phase for
good.  So the comparison is made in two pieces.  (1) kws_pitch_stft against the restatement from the raw samples, per bin within
C1 (log2 N + 2) 2^-24 sum_i |w_i v_i| of its frame.  (2) kws_pitch_apply against the restatement run on the spectrum the GPU itself
returned from kws_pitch_stft for the same clips (float32 values taken into float64 arithmetic), per sample within
C2 (J + log2 N + T[n] + 4) 2^-24 A[n], A[n] the windowed, normalised sum of the bin magnitudes (carried through the resampler's
sum |w| |v| for a pitched clip) and T[n] the tap count.  No sample is left out.  Every test prints the largest ratio of the GPU's error to
the unit bound (C = 1) before it asserts."""
import math

import numpy as np
import pytest

import pitch_ref as pf
import speed_ref as sr

pytestmark = pytest.mark.gpu

MS, STRIDE, OUT_STRIDE = 1024, 1100, 1032
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 1000, 1100)
RATES = (0.5, 0.8, 1.25, 2.0)
SEMITONES = (-12.0, -4.0, 4.0, 12.0)
NAN = float("nan")
U = 2.0 ** -24
# The largest ratios of the GPU's error to the unit bounds over every case of this file, measured on an MI355X, were 0.195 (analysis)
# and 0.421 (apply); each constant is the next power of two at or above twice its ratio.
C1 = 0.5
C2 = 1.0


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def table():
    from kws_amd.augment import Resampler
    return Resampler(), sr.table(**sr.DEFAULTS), 16, 512


def _source(i16, rows=len(LENGTHS), stride=STRIDE, seed=0):
    """loud noise rows; the last but one row is badly conditioned on purpose: digital silence, a windowed 440 Hz burst, noise at 1e-4 and
    a 700 Hz tone"""
    rng = np.random.default_rng(seed)
    x = (0.3 * rng.standard_normal((rows, stride))).astype(np.float32)
    t = np.arange(stride)
    hard = 1e-4 * rng.standard_normal(stride)
    hard[:300] = 0.0
    hard[300:500] = 0.3 * np.hanning(200) * np.sin(2 * np.pi * 440.0 * t[:200] / 16000.0)
    hard[800:] += 0.3 * np.sin(2 * np.pi * 700.0 * t[800:] / 16000.0)
    x[rows - 2] = hard.astype(np.float32)
    if i16:
        x = np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16)
    return x


def _f32(x):
    return x.astype(np.float32) / np.float32(32768.0) if x.dtype == np.int16 else x


def _check_stft(D, v32, rows, lens, N, what=""):
    """kws_pitch_stft's D (B, frames, N/2 + 1) against the restatement from the raw samples -> the largest error / unit bound"""
    worst = 0.0
    for b in range(len(rows)):
        v = v32[rows[b], :lens[rows[b]]]
        ref, S = pf.stft(v, N)
        M = pf.n_frames(len(v), N)
        assert ref.shape[0] == M <= D.shape[1]
        assert not D[b, M:].any(), (what, b)
        assert not D[b, :, 0].imag.any() and not D[b, :, -1].imag.any()
        err = np.abs(D[b, :M].astype(np.complex128) - ref)
        unit = ((math.log2(N) + 2.0) * U * S)[:, None]
        assert np.all(err <= C1 * unit), (what, b, len(v), float((err / np.maximum(unit, 1e-300)).max()))
        if (S > 0).any():
            worst = max(worst, float((err[S > 0] / unit[S > 0]).max()))
    return worst


def _check_apply(out, L, tempo, semis, D, v32, rows, lens, N, tab, what=""):
    """every clip of kws_pitch_apply against the restatement run on the GPU's own spectrum D: exact lengths, the float32 bound per sample,
    bit equality for a clip left as it is, zeros after L' -> the largest error / unit bound"""
    _, h, Z, P = tab
    worst = 0.0
    for b in range(len(rows)):
        v = v32[rows[b], :lens[rows[b]]]
        dry = tempo[b] == 0 and np.isnan(semis[b])
        M = pf.n_frames(len(v), N)
        ref = pf.perturb(v, tempo[b], semis[b], MS, N, h, Z, P, D=None if dry else D[b, :M])
        lp = len(ref["y"])
        assert L[b] == lp == (min(len(v), MS) if dry else pf.out_length(len(v), tempo[b], semis[b], MS)), (what, b, int(L[b]), lp)
        assert not out[b, lp:].any(), (what, b)
        if dry:
            assert np.array_equal(out[b, :lp].view(np.int32), v[:lp].view(np.int32)), (what, b)
            continue
        unit = (ref["J"] + math.log2(N) + ref["T"] + 4.0) * U * ref["A"]
        err = np.abs(out[b, :lp].astype(np.float64) - ref["y"])
        ratio = float((err[unit > 0] / unit[unit > 0]).max()) if (unit > 0).any() else 0.0
        assert np.all(err <= C2 * unit), (what, b, float(tempo[b]), float(semis[b]), len(v), ratio, int(np.argmax(err - C2 * unit)))
        worst = max(worst, ratio)
    return worst


def _both(torch, aug, x, lens, rows, tempo, semis, N, tab, base=0, what=""):
    """the two comparisons for the clips x[rows] with explicit tempos and shifts -> (out, L, the two worst ratios)"""
    from kws_amd.augment import stft
    wav, vl, ix = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(rows).cuda()
    D = stft(wav, N, valid_len=vl, index=ix)
    assert D.shape == (len(rows), 1 + STRIDE // (N // 4), N // 2 + 1) and D.dtype == torch.complex64
    D = D.cpu().numpy()
    buf = torch.full((len(rows), OUT_STRIDE), 9.0, device="cuda")
    out, L, tu, pu = aug.pitch_perturb(wav, valid_len=vl, index=ix, explicit_tempo=tempo, explicit_semitones=semis, max_samples=MS, out=buf,
                                       position_base=base)
    assert out.data_ptr() == buf.data_ptr()
    np.testing.assert_array_equal(tu.cpu().numpy(), tempo)                           # exact, NaN for NaN
    np.testing.assert_array_equal(pu.cpu().numpy(), semis)
    r1 = _check_stft(D, _f32(x), rows, lens, N, what)
    r2 = _check_apply(out.cpu().numpy(), L.cpu().numpy(), tempo, semis, D, _f32(x), rows, lens, N, tab, what)
    print("%s: analysis error / unit bound = %.3g, apply error / unit bound = %.3g" % (what, r1, r2))
    return out, L, r1, r2


# ---- 1. tempo at the smallest transform, every source length -------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("i16", [False, True])
def test_tempo_matches_the_restatement_on_the_gpus_own_spectrum(torch, table, i16, rate):
    from kws_amd.augment import WaveAugment
    x = _source(i16)
    lens = np.array(LENGTHS, np.int32)
    rows = np.arange(len(LENGTHS), dtype=np.int32)
    tempo = np.full(len(rows), rate, np.float32)
    tempo[3] = 0.0                                           # one clip left as it is
    semis = np.full(len(rows), NAN, np.float32)
    aug = WaveAugment(None, tempo=(rate, rate), pitch_n_fft=256, seed=1)
    assert aug.resampler is None
    out, L, _, _ = _both(torch, aug, x, lens, rows, tempo, semis, 256, table, what="tempo %g, i16=%s" % (rate, i16))
    # by draw: a range of one value draws that value for every clip; the same bits as the explicit call (clip 3 apart)
    wav, vl = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda()
    d_out, d_L, d_t, d_p = aug.pitch_perturb(wav, valid_len=vl, step=5, position_base=77, max_samples=MS,
                                             out=torch.full((len(rows), OUT_STRIDE), 9.0, device="cuda"))
    assert bool((d_t == float(np.float32(rate))).all()) and bool(torch.isnan(d_p).all())
    keep = [b for b in range(len(rows)) if b != 3]
    assert torch.equal(d_out[keep], out[keep]) and torch.equal(d_L[keep], L[keep])
    want = [pf.stretch_length(n, float(np.float32(rate))) for n in LENGTHS]
    assert [int(v) for v in d_L.cpu().numpy()] == [min(n, MS) for n in want]


# ---- 2. pitch, alone and with a tempo ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", SEMITONES)
@pytest.mark.parametrize("i16", [False, True])
def test_pitch_alone_and_with_a_tempo(torch, table, i16, n_steps):
    from kws_amd.augment import WaveAugment
    x = _source(i16, seed=2)
    lens = np.array(LENGTHS, np.int32)
    rows = np.r_[np.arange(len(LENGTHS)), np.arange(len(LENGTHS))].astype(np.int32)
    tempo = np.r_[np.zeros(len(LENGTHS)), np.resize([0.8, 1.25, 2.0, 0.5], len(LENGTHS))].astype(np.float32)
    semis = np.full(len(rows), n_steps, np.float32)
    aug = WaveAugment(None, pitch=(n_steps, n_steps), pitch_n_fft=256, resampler=table[0], seed=1)
    _both(torch, aug, x, lens, rows, tempo, semis, 256, table, what="pitch %+g, i16=%s" % (n_steps, i16))


# ---- 3. the larger transforms, an unordered index, a position base, the draws --------------------------------------------------------
@pytest.mark.parametrize("N", [512, 1024])
def test_larger_transforms_with_index_and_draws(torch, table, N):
    from kws_amd.augment import WaveAugment
    x = _source(N == 1024, seed=3)
    lens = np.array(LENGTHS, np.int32)
    rows = np.array([8, 7, 7, 0, 5, 2, 8, 1, 6, 3, 4, 7], np.int32)                   # repeated, unordered
    B, seed, base, step = len(rows), 7, 1000, 3
    kw = dict(tempo=(0.6, 1.8), tempo_rate=0.6, pitch=(-7.0, 9.0), pitch_rate=0.6, pitch_n_fft=N, resampler=table[0], seed=seed)
    aug = WaveAugment(None, **kw)
    wav, vl, ix = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(rows).cuda()
    out, L, tu, pu = aug.pitch_perturb(wav, valid_len=vl, index=ix, step=step, position_base=base, max_samples=MS,
                                       out=torch.full((B, OUT_STRIDE), 9.0, device="cuda"))
    again = aug.pitch_perturb(wav, valid_len=vl, index=ix, step=step, position_base=base, max_samples=MS,
                              out=torch.full((B, OUT_STRIDE), 5.0, device="cuda"))
    for a, b in zip((out, L), again[:2]):
        assert torch.equal(a, b)                                                      # two calls: the same bits
    on, t, pit, n = pf.np_draws(seed, step, base + np.arange(B), 0.6, (0.6, 1.8), 0.6, (-7.0, 9.0))
    assert on.any() and (~on).any() and pit.any() and (~pit).any() and (~on & ~pit).any()
    tempo, semis = np.where(on, t, np.float32(0)).astype(np.float32), np.where(pit, n, np.float32(NAN)).astype(np.float32)
    np.testing.assert_array_equal(tu.cpu().numpy(), tempo)                           # the draws, exactly
    np.testing.assert_array_equal(pu.cpu().numpy(), semis)
    ex_out, ex_L, _, _ = _both(torch, aug, x, lens, rows, tempo, semis, N, table, base=5, what="N = %d, drawn values" % N)
    assert torch.equal(ex_out, out) and torch.equal(ex_L, L)                          # explicit values: the draws' bits, at any base
    # shards: the batch in one call = two calls at their positions
    lo = aug.pitch_perturb(wav, valid_len=vl, index=ix[:5].contiguous(), step=step, position_base=base, max_samples=MS)
    hi = aug.pitch_perturb(wav, valid_len=vl, index=ix[5:].contiguous(), step=step, position_base=base + 5, max_samples=MS)
    assert torch.equal(out[:, :MS], torch.cat([lo[0], hi[0]])) and torch.equal(L, torch.cat([lo[1], hi[1]]))
    other = aug.pitch_perturb(wav, valid_len=vl, index=ix, step=step + 1, position_base=base, max_samples=MS)
    assert not torch.equal(other[2], tu)


# ---- 4. the workspace's tiles --------------------------------------------------------------------------------------------------------
def test_a_batch_larger_than_one_tile_gives_the_bits_of_a_single_tile(torch, table):
    from kws_amd import KwsError
    from kws_amd.augment import WaveAugment, pitch_workspace_bytes
    B = 24
    x = _source(True, rows=B, seed=4)
    lens = np.random.default_rng(5).integers(0, STRIDE + 1, B).astype(np.int32)
    wav, vl = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda()
    aug = WaveAugment(None, tempo=(0.5, 2.0), tempo_rate=0.8, pitch=(-12, 12), pitch_rate=0.8, pitch_n_fft=256, resampler=table[0], seed=9)
    one = pitch_workspace_bytes(256, MS, 1)
    whole = aug.pitch_perturb(wav, valid_len=vl, step=2, max_samples=MS, tile_clips=B)
    for tile in (1, 5, 23):
        ws = torch.empty((one * tile + 100,), dtype=torch.uint8, device="cuda")      # the spare bytes hold no further clip
        got = aug.pitch_perturb(wav, valid_len=vl, step=2, max_samples=MS, workspace=ws)
        for a, b in zip(whole[:2], got[:2]):
            assert torch.equal(a, b), tile
        assert torch.equal(torch.nan_to_num(whole[3], nan=99.0), torch.nan_to_num(got[3], nan=99.0)) and torch.equal(whole[2], got[2])
    assert torch.equal(whole[0], aug.pitch_perturb(wav, valid_len=vl, step=2, max_samples=MS, tile_clips=7)[0])
    with pytest.raises(KwsError) as e:
        aug.pitch_perturb(wav, valid_len=vl, max_samples=MS, workspace=torch.empty((one - 1,), dtype=torch.uint8, device="cuda"))
    assert e.value.code == -5
    with pytest.raises(ValueError):
        aug.pitch_perturb(wav, valid_len=vl, max_samples=MS, explicit_tempo=np.zeros(3, np.float32))
    for bad in ([0.4] * B, [2.5] * B, [NAN] * B):
        with pytest.raises(KwsError):
            aug.pitch_perturb(wav, valid_len=vl, max_samples=MS, explicit_tempo=np.array(bad, np.float32))
    with pytest.raises(KwsError):
        aug.pitch_perturb(wav, valid_len=vl, max_samples=MS, explicit_semitones=np.full(B, 12.5, np.float32))
    no_table = WaveAugment(None, tempo=(0.9, 1.1), pitch_n_fft=256, seed=9)
    with pytest.raises(ValueError, match="no resampler"):
        no_table.pitch_perturb(wav, valid_len=vl, max_samples=MS, explicit_semitones=np.full(B, 2.0, np.float32))
    # nothing stretched and nothing pitched: the float32 conversion, and no workspace is needed
    dry = no_table.pitch_perturb(wav, valid_len=vl, max_samples=MS, explicit_tempo=np.zeros(B, np.float32))
    v32 = torch.from_numpy(_f32(x)).cuda()
    for b in range(B):
        lp = min(int(lens[b]), MS)
        assert int(dry[1][b]) == lp and torch.equal(dry[0][b, :lp], v32[b, :lp]) and not dry[0][b, lp:].any()
    torch.cuda.synchronize()


# ---- 5. the chain at the default geometry --------------------------------------------------------------------------------------------
def test_chain_equals_the_stages_run_one_by_one(torch):
    from classifier.params import pr
    from kws_amd.augment import WaveAugment
    from kws_amd.featurizer import Featurizer
    rng = np.random.default_rng(7)
    x = (0.2 * rng.standard_normal((6, 17000))).astype(np.float32)
    wav = torch.from_numpy(x).cuda()
    vl = torch.from_numpy(np.array([17000, 16000, 9000, 0, 12345, 30], np.int32)).cuda()
    ix = torch.from_numpy(np.array([5, 0, 1, 2, 2, 3, 4], np.int32)).cuda()
    feat = Featurizer(pr)
    ms = feat.geometry["max_samples"]
    noise = [(0.2 * rng.standard_normal(20000)).astype(np.float32)]
    rirs = [np.r_[1.0, 0.3 * rng.standard_normal(400) * np.exp(-np.arange(400) / 100.0)].astype(np.float32)]
    filters = [("lowpass", 4, 3000.0), ("highpass", 2, 200.0)]
    pv = dict(tempo=(0.8, 1.25), tempo_rate=0.7, pitch=(-3, 3), pitch_rate=0.7)
    sp = dict(speed=(0.9, 1.1), speed_rate=0.7, loudness=(-30, -15), loudness_rate=0.7)
    nz = dict(snr=[5, 20], noised_rate=0.6, time_shift_ms=20, seed=12)
    kw = dict(valid_len=vl, index=ix, step=3, position_base=40)
    at = dict(step=3, position_base=40, max_samples=ms)
    # tempo + pitch + speed + loudness + noise
    aug = WaveAugment(noise, **nz, **sp, **pv)
    got = feat(wav, augment=aug, **kw)
    p_out, p_L, tu, pu = aug.pitch_perturb(wav, max_samples=ms, **kw)
    assert (tu != 0).any() and (~torch.isnan(pu)).any()
    s_out, s_L, _, _ = aug.perturb(p_out, valid_len=p_L, **at)
    plan = aug.plan(s_out, valid_len=s_L, **at)
    rows, L2 = aug.apply(s_out, plan, max_samples=ms)
    assert torch.equal(got, feat(rows, valid_len=L2))
    assert torch.equal(got, feat(wav, augment=aug, **kw))                             # the scratch and the workspace are reused
    # tempo + pitch only, then with a filter, then with every stage
    only = WaveAugment(None, seed=12, **pv)
    assert torch.equal(feat(wav, augment=only, **kw), feat(p_out, valid_len=p_L))
    flt = WaveAugment(None, filters=filters, filter_rate=0.6, seed=12, **pv)
    f_out, f_L, _ = flt.filter(p_out, valid_len=p_L, **at)
    assert torch.equal(feat(wav, augment=flt, **kw), feat(f_out, valid_len=f_L))
    full = WaveAugment(noise, rirs=rirs, reverb_rate=0.7, filters=filters, filter_rate=0.6, **nz, **sp, **pv)
    got = feat(wav, augment=full, **kw)
    wet, Lw, _ = full.reverberate(s_out, valid_len=s_L, **at)
    f_out, f_L, _ = full.filter(wet, valid_len=Lw, **at)
    plan = full.plan(f_out, valid_len=f_L, **at)
    rows, L3 = full.apply(f_out, plan, max_samples=ms)
    assert torch.equal(got, feat(rows, valid_len=L3))
    # an augment without tempo or pitch: the bits of the other stages called directly, as before
    old = WaveAugment(noise, rirs=rirs, reverb_rate=0.7, filters=filters, filter_rate=0.6, **nz, **sp)
    assert not old.vocodes
    got = feat(wav, augment=old, **kw)
    s_out, s_L, _, _ = old.perturb(wav, max_samples=ms, **kw)
    wet, Lw, _ = old.reverberate(s_out, valid_len=s_L, **at)
    f_out, f_L, _ = old.filter(wet, valid_len=Lw, **at)
    plan = old.plan(f_out, valid_len=f_L, **at)
    rows, L4 = old.apply(f_out, plan, max_samples=ms)
    assert torch.equal(got, feat(rows, valid_len=L4))
    plain = Featurizer(pr)                                                            # the workspace exists only with the stage
    assert torch.equal(plain(wav, augment=old, **kw), got) and "_pv_ws" not in plain.__dict__ and "_pv_ws" in feat.__dict__


# ---- 6. end to end, well conditioned -------------------------------------------------------------------------------------------------
def _peak_hz(y, fs=16000.0):
    spec = np.abs(np.fft.rfft(y * np.hanning(len(y))))
    return float(np.argmax(spec)) * fs / len(y)


def test_a_sine_shifts_by_four_semitones_and_stretches_at_its_pitch(torch):
    from kws_amd.augment import pitch_shift, stft, time_stretch
    fs, N = 16000.0, 512
    v = (0.5 * np.sin(2 * np.pi * 440.0 * np.arange(16000) / fs)).astype(np.float32)
    wav = torch.from_numpy(np.stack([v, v])).cuda()
    up = pitch_shift(wav, 4.0)
    assert up.shape == (2, 16000) and up.dtype == torch.float32 and torch.equal(up[0], up[1])
    peak = _peak_hz(up[0].cpu().numpy().astype(np.float64))
    print("+4 semitones: peak at %.1f Hz" % peak)
    assert abs(peak - 554.4) <= fs / N
    slow = time_stretch(wav, 0.8)
    assert slow.shape == (2, 20000) and torch.equal(slow[0], slow[1])
    y = slow[0].cpu().numpy().astype(np.float64)
    peak = _peak_hz(y)
    print("tempo 0.8: peak at %.1f Hz" % peak)
    assert abs(peak - 440.0) <= fs / N
    assert 0.45 <= np.sqrt(2.0 * np.mean(y[N:-N] ** 2)) <= 0.55
    # the spectrogram: the bin of 440 Hz carries the sine, amplitude 0.5 x the window's sum / 2
    D = stft(torch.from_numpy(np.round(v * 32768).astype(np.int16)[None]).cuda(), N)
    assert D.shape == (1, 126, 257)
    mag = D[0, 60].abs().cpu().numpy()
    assert int(np.argmax(mag)) == 14 and abs(mag.max() - 0.5 * 256 / 2) <= 0.15 * 64
    for bad in (0.4, 2.5):
        with pytest.raises(ValueError):
            time_stretch(wav, bad)
    with pytest.raises(ValueError):
        pitch_shift(wav, 13.0)
    with pytest.raises(ValueError):
        stft(wav, 300)


# ---- 7. training ---------------------------------------------------------------------------------------------------------------------
def _fit(torch, x, y, C, **kw):
    from classifier.loss import SparseCategoricalCrossEntropy
    from classifier.model import KWSModel
    from common.model_utils import get_optimizer
    torch.manual_seed(1234)
    m = KWSModel("simple_cnn_lite", C, seed=3)
    m._device().set_deterministic(True)
    m.compile(optimizer=get_optimizer("adam", 1e-3), loss=SparseCategoricalCrossEntropy(), metrics=["accuracy"])
    h = m.fit(x, y, batch_size=32, epochs=1, verbose=0, shuffle=True, **kw)
    return (h.history["loss"], h.history["accuracy"]), m.get_weights()


def test_fit_with_tempo_and_pitch_is_reproducible(torch):
    from kws_amd.augment import WaveAugment
    rng = np.random.default_rng(10)
    C, N = 4, 64
    y = rng.integers(0, C, N)
    tones = np.sin(2 * np.pi * (300.0 * (1 + np.arange(C)))[:, None] * np.arange(16000)[None, :] / 16000.0)
    x = (0.3 * tones[y] + 0.05 * rng.standard_normal((N, 16000))).astype(np.float32)
    lens = rng.integers(4000, 16001, N).astype(np.int32)
    kw = dict(tempo=(0.85, 1.2), pitch=(-2, 2), speed=(0.95, 1.05), seed=8)
    h0, w0 = _fit(torch, x, y, C, augment=WaveAugment(None, **kw), sample_lengths=lens)         # 64 clips of 32: two steps
    h1, w1 = _fit(torch, x, y, C, augment=WaveAugment(None, **kw), sample_lengths=lens)
    assert h0 == h1 and all(np.isfinite(h1[0]))
    for a, b in zip(w0, w1):
        np.testing.assert_array_equal(a, b)
    hp, wp = _fit(torch, x, y, C, augment=WaveAugment(None, speed=(0.95, 1.05), seed=8), sample_lengths=lens)
    assert hp != h1 and any(not np.array_equal(a, b) for a, b in zip(wp, w1))
