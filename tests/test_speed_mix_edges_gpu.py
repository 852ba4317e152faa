"""GPU tests of the speed/loudness stage and of the noise mix at their kernel edges, over the case table of tests/speed_mix_cases.py:
speed_apply_kernel against the float64 restatement of tests/speed_ref.py at ratios next to 0.5, 1 and 2, at output lengths on both
sides of a wave, a block and max_samples, at the default geometry's cut, on every table size up to the 64 KiB limit and at max_samples
of 1 to 3; the vocoder's use of the same interpolation on the smallest and the largest table; augment_plan_kernel and
augment_apply_kernel against float64 at segment, window, shift, SNR, length and batch edges for max_samples 16000, 300, 2 and 1, through
the C ABI with out_stride = max_samples + 7; and the fused featurizer bit for bit against the plain one on apply's rows.  The
assertions are those of test_speed_gpu.py and test_pitch_gpu.py; the mix bounds are derived in speed_mix_cases.py.
tests/test_speed_mix_edges_host.py shows on the CPU that every case is what it claims and that none is vacuous.

Largest ratios of the GPU's error to its bound over every case of this file, measured on an MI355X: speed samples
0.242 (threads; 0.133 at the default geometry's cut, 0.205 over the tables, 0.0865 at max_samples 1 to 3), vocoder analysis 0.195 and
apply 0.311 of their unit bounds (C1 = 0.5, C2 = 1), mix gain 0.585 (the host restatement of the plan's arithmetic predicts the same),
mix sample 0.499.  Every test prints its own before it asserts."""
import math

import numpy as np
import pytest

import speed_mix_cases as sm
import speed_ref as sr
import test_pitch_gpu as tpg
from test_augment_gpu import np_plan

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- A. speed and loudness -------------------------------------------------------------------------------------------------------------
_RESAMPLERS = {}


def _resampler(name):
    from kws_amd.augment import Resampler
    if name not in _RESAMPLERS:
        _RESAMPLERS[name] = Resampler(*sm.TABLES[name])
    return _RESAMPLERS[name]


def _speed_run(torch, group, i16):
    """one kws_speed_apply over the group: (out, lengths, speed_used, gain_used) as numpy"""
    from kws_amd.augment import WaveAugment
    g = sm.SPEED_GROUPS[group]
    x, lens, index, ratios, db = sm.speed_source(group, i16)
    wav, vl, ix = torch.tensor(x).cuda(), torch.tensor(lens).cuda(), torch.tensor(index).cuda()     # copies: the table's arrays are read-only
    aug = WaveAugment(None, speed=(1.0, 1.0), speed_rate=0.0, resampler=_resampler(g.table), seed=1)
    buf = torch.full((len(ratios), g.max_samples + sm.PAD), 9.0, device="cuda")
    out, L, used, gain = aug.perturb(wav, valid_len=None if g.whole_rows else vl, index=None if g.whole_rows else ix,
                                     explicit_speed=np.array(ratios), explicit_db=np.array(db), max_samples=g.max_samples, out=buf)
    assert out.data_ptr() == buf.data_ptr()
    return out.cpu().numpy(), L.cpu().numpy(), used.cpu().numpy(), gain.cpu().numpy()


def _speed_check(torch, group, i16):
    """test_speed_gpu.py's assertions over the group -> the largest sample error / bound"""
    g = sm.SPEED_GROUPS[group]
    out, L, used, gain = _speed_run(torch, group, i16)
    refs = sm.speed_expect(group)
    np.testing.assert_array_equal(used, np.array([c.ratio for c in g.clips], np.float32))
    worst, worst_at = 0.0, None
    for b, (c, ref) in enumerate(zip(g.clips, refs)):
        v = sm.speed_clip_source(group, b)
        lp = len(ref["y"])
        levelled = not math.isnan(c.db)
        assert L[b] == lp, (group, b, c, int(L[b]), lp)
        assert not out[b, lp:].any(), (group, b, c)                  # zeros after L', out to out_stride
        if not levelled:
            assert gain[b] == 1.0, (group, b, c)
        else:
            np.testing.assert_allclose(gain[b], ref["g"], rtol=1e-6, atol=0, err_msg="%s clip %d %r" % (group, b, c))
        if c.ratio == 0:                                             # the conversion, or the conversion times the gain: bit for bit
            want = v[:lp] if not levelled else (gain[b] * v[:lp]).astype(np.float32)
            assert np.array_equal(_bits(out[b, :lp]), _bits(want)), (group, b, c)
        else:
            tol = sm.speed_bound(ref)
            err = np.abs(out[b, :lp].astype(np.float64) / float(gain[b]) - ref["y"])
            if lp:
                ratio = float((err / np.maximum(tol, 1e-300)).max())
                if ratio > worst:
                    worst, worst_at = ratio, (b, float(c.ratio), c.ls, int(np.argmax(err / np.maximum(tol, 1e-300))))
            assert np.all(err <= tol), (group, b, c, int(np.argmax(err - tol)), float(err.max()), float(tol.max()))
        if levelled and lp:
            m = float(np.mean(ref["y"] ** 2))
            if c.kind == sm.SILENT:
                assert not out[b].any() and np.isfinite(gain[b])     # a silent clip stays silent
            elif sr.EPS32 / m < 1e-5:
                level = sr.level_db(out[b, :lp])
                assert abs(level - c.db) <= 1e-4, (group, b, c, level)
            else:                      # a quiet clip: FLT_EPSILON in g = sqrt(10^(T/10) / (m + FLT_EPSILON)) keeps it below the target
                level = sr.level_db(out[b, :lp])
                assert abs(level - (c.db + 10.0 * math.log10(m / (m + sr.EPS32)))) <= 1e-4, (group, b, c, level)
    print("%s, i16=%s: %d clips, largest sample error / bound = %.3g at (clip, ratio, Ls, n) = %s"
          % (group, i16, len(g.clips), worst, worst_at))
    return worst


@pytest.mark.parametrize("i16", [False, True])
def test_speed_threads_and_waves(torch, i16):
    assert _speed_check(torch, "threads", i16) > 0


@pytest.mark.parametrize("i16", [False, True])
def test_speed_cut_at_the_default_geometry(torch, i16):
    assert _speed_check(torch, "cut", i16) > 0
    assert _speed_check(torch, "rows", i16) > 0                          # without valid_len: the row itself is the clip


@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("group", sm.TABLE_GROUPS)
def test_speed_tables_up_to_the_lds_limit(torch, group, i16):
    """a launch the device refuses comes back from kws_speed_apply as an error, which WaveAugment.perturb raises"""
    assert _speed_check(torch, group, i16) > 0


@pytest.mark.parametrize("i16", [False, True])
def test_level_alone_and_with_a_ratio(torch, i16):
    assert _speed_check(torch, "level", i16) > 0


@pytest.mark.parametrize("ms", sm.TINY_MS)
def test_speed_tiny_max_samples(torch, ms):
    for i16 in (False, True):
        _speed_check(torch, "tiny%d" % ms, i16)


@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("name", ["z4p32", "z16p1023"])
def test_vocoder_on_the_smallest_and_the_largest_table(torch, name, i16):
    """kws_pitch.hip reads the same table into the LDS its vocoder has left: the largest table is bigger than that, the smallest smaller"""
    from kws_amd.augment import WaveAugment
    h, Z, P = sm.speed_table(name)
    tab = (_resampler(name), h, Z, P)
    x = tpg._source(i16, seed=11)
    lens = np.array(tpg.LENGTHS, np.int32)
    n = len(tpg.LENGTHS)
    rows = np.tile(np.arange(n), 4).astype(np.int32)
    semis = np.repeat(np.array([-12.0, -4.0, 4.0, 12.0], np.float32), n)
    tempo = np.zeros(len(rows), np.float32)
    aug = WaveAugment(None, pitch=(0.0, 0.0), pitch_rate=0.0, pitch_n_fft=256, resampler=tab[0], seed=1)
    _both = tpg._both                                                    # asserts C1 and C2 and prints both ratios
    _both(torch, aug, x, lens, rows, tempo, semis, 256, tab, what="vocoder, table %s, i16=%s" % (name, i16))


# ---- B. the noise mix ------------------------------------------------------------------------------------------------------------------
_AUGS = {}


def _mix_aug(ms, single=False):
    from kws_amd.augment import NoiseBank, WaveAugment
    if (ms, single) not in _AUGS:
        _AUGS[(ms, single)] = WaveAugment(NoiseBank(list(sm.mix_bank(ms, single).segs)), seed=1)
    return _AUGS[(ms, single)]


def _apply(torch, aug, plan, wav, ix, ms):
    """kws_augment_apply through the C ABI with out_stride = max_samples + 7 -> (out, lengths) tensors"""
    from kws_amd import lib as l
    B = plan.shape[0]
    out = torch.full((B, ms + sm.PAD), 9.0, device="cuda")
    lengths = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    code = l.WAV_I16 if wav.dtype == torch.int16 else l.WAV_F32
    l.check(l.get_lib().kws_augment_apply(aug.noise.handle(), plan.data_ptr(), wav.data_ptr(), code, None if ix is None else ix.data_ptr(),
                                          B, wav.shape[1], ms, out.data_ptr(), ms + sm.PAD, lengths.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream))
    return out, lengths


def _mix_check(ms, bank, cases, rows, v, lens, r, out, lengths, what):
    """the plan's records and apply's rows of one call against float64 -> (largest gain error / bound, largest sample error / bound)"""
    worst_g = worst_s = 0.0
    for b, c in enumerate(cases):
        e = sm.plan_expect(ms, c, v, lens, bank)
        rec = r[b]
        assert (rec["apply"], rec["segment"], rec["shift"]) == (c.apply, c.segment, c.shift) and rec["snr_db"] == np.float32(c.snr), (what, b)
        assert (rec["length"], rec["voice_length"], rec["offset"]) == (e.L, e.lv, e.offset), (what, b, c, rec, e)
        g = float(rec["gain"])
        if e.silent:
            assert g == 0.0, (what, b, c, g)
        else:
            assert np.isfinite(rec["gain"]) and g > 0
            ratio = abs(g - e.gain) / (e.gain * e.bound)
            worst_g = max(worst_g, ratio)
            assert ratio <= 1.0, (what, b, c, g, e.gain, e.bound, ratio)
        L, d = e.L, c.shift
        assert lengths[b] == L
        assert not out[b, L:].any(), (what, b, c)                        # zeros from L out to out_stride
        row = v[c.row]
        ref = sm.mix_f64(row, bank.segs[c.segment], L, e.offset, d, rec["gain"], c.apply)
        got = out[b, :L]
        t = np.arange(L)
        inside = (t - d >= 0) & (t - d < L)
        assert not got[~inside].any(), (what, b, c)                      # exact zeros where t - d falls outside [0, L)
        if not c.apply:
            assert np.array_equal(_bits(got[inside]), _bits(row[t[inside] - d])), (what, b, c)
        err, tol = np.abs(got.astype(np.float64) - ref), sm.mix_sample_bound(ref)
        assert np.all(err <= tol), (what, b, c, int(np.argmax(err - tol)), float(err.max()))
        if L and c.apply:
            worst_s = max(worst_s, float((err / tol).max()))
    return worst_g, worst_s


def _mix_group(torch, ms, i16, group, with_lens=True):
    from kws_amd.augment import records
    x, lens = sm.mix_voices(ms, i16)
    ex, rows = sm.mix_records(ms, group)
    aug = _mix_aug(ms)
    wav, vl, ix = torch.tensor(x).cuda(), torch.tensor(lens).cuda(), torch.from_numpy(rows).cuda()
    plan = aug.plan(wav, valid_len=vl if with_lens else None, index=ix, explicit=ex, max_samples=ms)
    out, lengths = _apply(torch, aug, plan, wav, ix, ms)
    res = _mix_check(ms, sm.mix_bank(ms), sm.mix_groups(ms)[group], rows, sm.mix_f32(x), lens if with_lens else None, records(plan),
                     out.cpu().numpy(), lengths.cpu().numpy(), "%s, max_samples %d, i16=%s" % (group, ms, i16))
    return res, (wav, ix, plan, out, lengths)


@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("ms", sm.MIX_MS)
def test_mix_plan_and_apply_at_their_edges(torch, ms, i16):
    worst_g = worst_s = 0.0
    for group in sm.mix_groups(ms):
        (g, s), _ = _mix_group(torch, ms, i16, group)
        worst_g, worst_s = max(worst_g, g), max(worst_s, s)
    (g, s), _ = _mix_group(torch, ms, i16, "lengths", with_lens=False)   # without valid_len: every row whole
    worst_g, worst_s = max(worst_g, g), max(worst_s, s)
    print("mix, max_samples %d, i16=%s: largest gain error / bound = %.3g, largest sample error / bound = %.3g" % (ms, i16, worst_g, worst_s))
    assert worst_g > 0 and worst_s > 0


@pytest.mark.parametrize("ms", sm.MIX_MS)
def test_mix_drawn_mode_equals_numpy_field_for_field(torch, ms):
    """K = 1 and a segment as long as every clip: the offset draw is uniform over one value; max_shift 0 and 2^24; 1 and 16 SNRs"""
    from kws_amd.augment import records
    aug = _mix_aug(ms, single=True)
    bank = sm.mix_bank(ms, True)
    x, _ = sm.mix_voices(ms, False)
    wav = torch.tensor(x).cuda()
    B, v = x.shape[0], sm.mix_f32(x)
    worst = 0.0
    try:
        for max_shift, snr, seed, step, base in ((0, [7.0], 3, 5, 0), (sm.MAX_SHIFT, list(np.linspace(-200.0, 200.0, sm.AUG_MAX_SNR)), 0x123456789AB, 9, 1000)):
            aug.max_shift, aug.snr, aug.noised_rate, aug.seed = max_shift, [float(s) for s in snr], 0.7, seed
            plan = aug.plan(wav, step=step, position_base=base, max_samples=ms)
            r = records(plan)
            want = np_plan(seed, step, base + np.arange(B), np.full(B, ms), [ms], snr, 0.7, max_shift)
            for k, val in want.items():
                np.testing.assert_array_equal(r[k], val, err_msg=k)
            assert not r["offset"].any() and (np.abs(r["shift"]) <= max_shift).all()
            assert r["apply"].any() and not r["apply"].all()
            assert max_shift == 0 or (np.abs(r["shift"]) > ms).any()
            cases = [sm.MixCase(b, int(r["apply"][b]), 0, 0, int(r["shift"][b]), float(r["snr_db"][b])) for b in range(B)]
            out, lengths = _apply(torch, aug, plan, wav, None, ms)
            g, _ = _mix_check(ms, bank, cases, np.arange(B), v, None, r, out.cpu().numpy(), lengths.cpu().numpy(), "drawn, max_samples %d" % ms)
            worst = max(worst, g)
    finally:
        aug.max_shift, aug.snr, aug.noised_rate, aug.seed = 0, [50.0], 1.0, 1
    print("mix drawn, max_samples %d: largest gain error / bound = %.3g" % (ms, worst))


@pytest.mark.parametrize("i16", [False, True])
def test_fused_featurizer_equals_the_plain_one_on_applys_rows(torch, i16):
    """the AUG instantiation of the tuned kernel, given the explicit plans through the C ABI, against kws_featurize on the rows
    kws_augment_apply wrote with valid_len = lengths: bit for bit, at both CU shares"""
    from classifier.params import pr
    from kws_amd import lib as l
    from kws_amd.featurizer import Featurizer
    ms = 16000
    aug = _mix_aug(ms)
    feat = Featurizer(pr)
    assert feat.geometry["max_samples"] == ms
    code = l.WAV_I16 if i16 else l.WAV_F32
    n = 0
    for group in sm.mix_groups(ms):
        _, (wav, ix, plan, rows, lengths) = _mix_group(torch, ms, i16, group)
        B = plan.shape[0]
        for share in (1, 2):
            feat.set_cu_share(share)
            want = feat(rows, valid_len=lengths)
            got = torch.full_like(want, 7.0)
            l.check(l.get_lib().kws_featurize_gather_augmented(feat._h, wav.data_ptr(), code, ix.data_ptr(), B, wav.shape[1],
                                                               aug.noise.handle(), plan.data_ptr(), got.data_ptr(),
                                                               torch.cuda.current_stream().cuda_stream))
            assert torch.equal(got, want), (group, share, i16)
            n += B
    print("fused featurizer, i16=%s: %d clips bit-equal to the plain featurizer on apply's rows" % (i16, n))
