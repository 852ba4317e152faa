"""GPU test of what the four wave-augmentation stages share (csrc/kws_wave_stage.h: the clip's row and length): negative, oversized and
missing valid_len for the speed, reverb, filter and noise stages at rate 0, where every clip is the float32 conversion of
wav[row, :L], L = min(max(valid_len[row], 0), stride, max_samples).  The wet paths, the draws and the chain have tests of their own
(test_speed_gpu.py, test_reverb_gpu.py, test_filter_gpu.py, test_augment_gpu.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MS, ROWS, OUT_STRIDE = 256, 12, 261
VALID_LEN = np.array([-3, 0, 1, 2, 255, 256, 257, 299, 300, 301, 2 ** 31 - 1, 128], np.int32)
INDEX = np.array([10, 0, 6, 9, 4, 6, 8, 1], np.int32)         # one repeat, not in order
POSITION_BASE = 5
CASES = {"valid_len": (300, True), "none_long": (300, False), "none_short": (200, False)}     # stride, with valid_len


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _source(i16, stride):
    x = (0.3 * np.random.default_rng(7).standard_normal((ROWS, stride))).astype(np.float32)
    return np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16) if i16 else x


def _expected(x, stride, with_len, width, ms=MS):
    """-> (L (B,), rows (B, width) float32): the dry clips in numpy"""
    v32 = x.astype(np.float32) / np.float32(32768.0) if x.dtype == np.int16 else x
    src = VALID_LEN[INDEX].astype(np.int64) if with_len else np.full(len(INDEX), stride, np.int64)
    L = np.minimum(np.minimum(np.maximum(src, 0), stride), ms)
    rows = np.zeros((len(INDEX), width), np.float32)
    for b, (r, n) in enumerate(zip(INDEX, L)):
        rows[b, :n] = v32[r, :n]
    return L, rows


def _augment(rng):
    """every stage configured, every rate 0"""
    from kws_amd.augment import RirBank, WaveAugment
    rirs = RirBank([np.r_[1.0, 0.3 * rng.standard_normal(40)].astype(np.float32)], max_samples=MS)
    noise = [(0.2 * rng.standard_normal(2000)).astype(np.float32)]
    return WaveAugment(noise, noised_rate=0.0, time_shift_ms=0, seed=3, rirs=rirs, reverb_rate=0.0, filters=[("lowpass", 4, 3000.0)],
                       filter_rate=0.0, speed=(0.8, 1.25), speed_rate=0.0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
def test_dry_clips_at_the_length_edges(torch, i16, case):
    from classifier.params import pr
    from kws_amd.augment import records
    from kws_amd.featurizer import Featurizer
    stride, with_len = CASES[case]
    x = _source(i16, stride)
    L, want = _expected(x, stride, with_len, OUT_STRIDE)
    aug = _augment(np.random.default_rng(1))
    wav, ix = torch.from_numpy(x).cuda(), torch.from_numpy(INDEX).cuda()
    vl = torch.from_numpy(VALID_LEN).cuda() if with_len else None
    kw = dict(valid_len=vl, index=ix, step=2, position_base=POSITION_BASE, max_samples=MS)
    B = len(INDEX)

    def fresh():
        return torch.full((B, OUT_STRIDE), 9.0, dtype=torch.float32, device="cuda")

    out, lens, speed_used, gain_used = aug.perturb(wav, out=fresh(), **kw)
    np.testing.assert_array_equal(lens.cpu().numpy(), L, err_msg="speed lengths")
    np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(want), err_msg="speed out")
    np.testing.assert_array_equal(speed_used.cpu().numpy(), np.zeros(B, np.float32))
    np.testing.assert_array_equal(gain_used.cpu().numpy(), np.ones(B, np.float32))

    out, lens, rir_used = aug.reverberate(wav, out=fresh(), **kw)
    np.testing.assert_array_equal(lens.cpu().numpy(), L, err_msg="reverb lengths")
    np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(want), err_msg="reverb out")
    np.testing.assert_array_equal(rir_used.cpu().numpy(), np.full(B, -1))

    out, lens, filter_used = aug.filter(wav, out=fresh(), **kw)
    np.testing.assert_array_equal(lens.cpu().numpy(), L, err_msg="filter lengths")
    np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(want), err_msg="filter out")
    np.testing.assert_array_equal(filter_used.cpu().numpy(), np.full(B, -1))

    plan = aug.plan(wav, **kw)
    r = records(plan)
    np.testing.assert_array_equal(r["length"], L)
    np.testing.assert_array_equal(r["voice_length"], L)
    np.testing.assert_array_equal(r["apply"], np.zeros(B, np.int32))
    rows, lens = aug.apply(wav, plan, index=ix, max_samples=MS)
    np.testing.assert_array_equal(lens.cpu().numpy(), L, err_msg="noise lengths")
    np.testing.assert_array_equal(_bits(rows.cpu().numpy()), _bits(want[:, :MS]), err_msg="noise rows")

    # the featurizer clips at its own max_samples (>= every stride here): the all-dry chain is the plain call, bit for bit
    feat = Featurizer(pr)
    got = feat(wav, valid_len=vl, index=ix, augment=aug, step=2, position_base=POSITION_BASE)
    assert torch.equal(got, feat(wav, valid_len=vl, index=ix))
