"""GPU tests of the two wet wave-augmentation kernels at their section, chunk and length edges, against the float64 restatements
(tests/filter_ref.py, tests/reverb_ref.py) over the case table of tests/wave_edge_cases.py: filter_apply_kernel in each of its four
section-count instantiations, at every chunk size on both sides of every boundary, at the largest and the smallest padlen and at odd,
tiny, cutting and limit values of max_samples; reverb_apply_kernel at max_samples from the transform's limit down to 1 and with a bank
whose max_samples is not the call's.  The bounds are those of test_filter_gpu.py and test_reverb_gpu.py; tests/test_wave_edges_host.py
shows on the CPU that every case is what it claims and that none is vacuous."""
import numpy as np
import pytest

import wave_edge_cases as wc
from filter_ref import keep_energy
from test_filter_gpu import FILT_TOL
from test_reverb_gpu import CONV_TOL

pytestmark = pytest.mark.gpu

PAD = 7                # out_stride = max_samples + PAD, prefilled with 9.0


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- filter --------------------------------------------------------------------------------------------------------------------------
def _filter_run(torch, group, i16, rescale, tight=False, in_place=False):
    """one kws_filter_apply over the group: (out, lengths, filter_used) as numpy"""
    from kws_amd.augment import WaveAugment
    g = wc.FILTER_GROUPS[group]
    x, lens, ex = wc.filter_source(group, i16, tight)
    wav, vl = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda()
    aug = WaveAugment(None, filters=wc.make_bank(g.bank), filter_rate=1.0, rescale=rescale, seed=2)
    out = wav if in_place else torch.full((len(ex), g.max_samples + PAD), 9.0, device="cuda")
    got, L, used = aug.filter(wav, valid_len=vl, explicit=ex, max_samples=g.max_samples, out=out)
    assert got.data_ptr() == out.data_ptr()
    return got.cpu().numpy(), L.cpu().numpy(), used.cpu().numpy()


def _filter_check(group, i16, rescale, out, L, used):
    """test_filtfilt_matches_numpy_float64's assertions over the group; -> (largest |err| / max|v|, the m of every wet clip)"""
    g = wc.FILTER_GROUPS[group]
    e = wc.filter_expect(group, i16)
    pads = wc.make_bank(g.bank).padlen
    np.testing.assert_array_equal(used, e.used)                          # the dry rule: chosen and Lv > padlen
    worst, ms_seen = 0.0, set()
    for b, (v, y) in enumerate(zip(e.clips, e.ref)):
        lv = len(v)
        assert L[b] == lv
        if y is None:
            assert np.array_equal(_bits(out[b, :lv]), _bits(v)), (group, b, lv)
        else:
            if rescale:
                y = keep_energy(v, y)
            err = np.abs(out[b, :lv] - y).max() / max(np.abs(v).max(), 1e-30)
            worst = max(worst, err)
            ms_seen.add(wc.chunk_log(lv + 2 * int(pads[used[b]])))
            assert err <= FILT_TOL, (group, b, g.clips[b], lv, err)
        assert not out[b, lv:].any()                                     # zeros after Lv, out to out_stride
    return worst, ms_seen


@pytest.mark.parametrize("rescale", [True, False])
@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("group", wc.SECTION_GROUPS)
def test_filter_section_counts_match_float64(torch, group, i16, rescale):
    bank = wc.make_bank(wc.FILTER_GROUPS[group].bank)
    out, L, used = _filter_run(torch, group, i16, rescale)
    worst, _ = _filter_check(group, i16, rescale, out, L, used)
    for k, p in enumerate(bank.padlen):                                  # Lv = padlen stays dry, padlen + 1 is filtered
        assert list(used[2 * k:2 * k + 2]) == [-1, k] and list(L[2 * k:2 * k + 2]) == [p, p + 1]
    print("sections %d: filtfilt max |err| / max|v| = %.3g (i16=%s, rescale=%s)" % (bank.n_sections, worst, i16, rescale))


@pytest.mark.parametrize("rescale", [True, False])
@pytest.mark.parametrize("group", list(wc.CHUNK_GROUPS))
def test_filter_chunk_boundaries_match_float64(torch, group, rescale):
    out, L, used = _filter_run(torch, group, False, rescale)
    worst, ms_seen = _filter_check(group, False, rescale, out, L, used)
    assert ms_seen == set(range(wc.MIN_LOG, wc.MAX_LOG + 1))
    again = _filter_run(torch, group, False, rescale)
    for a, b in zip((out, L, used), again):
        assert np.array_equal(_bits(a), _bits(b))
    print("%s: chunk logs %s, filtfilt max |err| / max|v| = %.3g (rescale=%s)" % (group, sorted(ms_seen), worst, rescale))


@pytest.mark.parametrize("ms", list(wc.MS_GROUPS))
def test_filter_max_samples_edges(torch, ms):
    from kws_amd import KwsError
    from kws_amd.augment import WaveAugment
    for group in wc.MS_GROUPS[ms]:
        for tight in (False, True):                                      # a row stride above and equal to max_samples
            out, L, used = _filter_run(torch, group, False, True, tight=tight)
            worst, ms_seen = _filter_check(group, False, True, out, L, used)
            assert (used < 0).all() == (group in wc.ALL_DRY_GROUPS)
            print("%s (stride %s max_samples): chunk logs %s, filtfilt max |err| / max|v| = %.3g"
                  % (group, "==" if tight else ">", sorted(ms_seen), worst))
        if group in wc.IN_PLACE_GROUPS:                                  # out is wav, stride == out_stride: the same bits
            got, L2, used2 = _filter_run(torch, group, False, True, tight=True, in_place=True)
            assert got.shape[1] == ms
            assert np.array_equal(_bits(got), _bits(out[:, :ms])) and np.array_equal(L2, L) and np.array_equal(used2, used)
        if group == "ms16320_p32":                                       # lpad = 16384: m = 8 with every lane full
            assert used[0] == 0 and L[0] == 16320 and wc.chunk_log(16320 + 2 * 32) == 8 and wc.last_lane(16384) == (63, 256)
    if ms == wc.FILTER_MAX_SAMPLES:
        x, lens, ex = wc.filter_source("ms16320", False)
        aug = WaveAugment(None, filters=wc.make_bank("S4"), filter_rate=1.0, seed=2)
        with pytest.raises(KwsError):
            aug.filter(torch.from_numpy(x).cuda(), valid_len=torch.from_numpy(lens).cuda(), explicit=ex, max_samples=ms + 1)


# ---- reverb --------------------------------------------------------------------------------------------------------------------------
_RIR_BANKS = {}


def _rir_bank(bank_ms, ms):
    from kws_amd.augment import RirBank
    if (bank_ms, ms) not in _RIR_BANKS:
        _RIR_BANKS[(bank_ms, ms)] = RirBank(list(wc.reverb_group(bank_ms, ms).rirs), max_samples=bank_ms)
    return _RIR_BANKS[(bank_ms, ms)]


def _reverb_run(torch, bank_ms, ms, i16, rescale):
    from kws_amd.augment import WaveAugment
    x, lens, index, ex = wc.reverb_source(bank_ms, ms, i16)
    wav, vl, ix = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda(), torch.from_numpy(index).cuda()
    aug = WaveAugment(None, rirs=_rir_bank(bank_ms, ms), reverb_rate=1.0, rescale=rescale, seed=2)
    out, L, used = aug.reverberate(wav, valid_len=vl, index=ix, explicit=ex, max_samples=ms,
                                   out=torch.full((len(ex), ms + PAD), 9.0, device="cuda"))
    return out.cpu().numpy(), L.cpu().numpy(), used.cpu().numpy()


def _reverb_check(torch, bank_ms, ms, i16, rescale):
    """test_convolution_matches_numpy_float64's assertions over the group, run twice; -> the largest |err| / bound"""
    g = wc.reverb_group(bank_ms, ms)
    e = wc.reverb_expect(bank_ms, ms, i16)
    bank = _rir_bank(bank_ms, ms)
    out, L, used = _reverb_run(torch, bank_ms, ms, i16, rescale)
    np.testing.assert_array_equal(used, [k for _, k in g.pairs])
    worst = 0.0
    for b, (r, k) in enumerate(g.pairs):
        v = e.clips[b]
        assert L[b] == e.length[b], (b, len(v), k, L[b], e.length[b])
        if k < 0:
            assert np.array_equal(_bits(out[b, :len(v)]), _bits(v))
        else:
            h = bank.taps[k]
            assert np.array_equal(h, e.taps[b])                          # the bank clips at its own max_samples
            s = e.scale[b] if rescale else 1.0
            y = e.ref[b] * s
            bound = CONV_TOL * s * np.linalg.norm(v.astype(np.float64)) * np.linalg.norm(h.astype(np.float64))
            err = np.abs(out[b, :len(y)] - y).max() if len(y) else 0.0
            if bound > 0:
                worst = max(worst, err / bound)
            assert err <= bound, (b, len(v), len(h), err, bound)
            if r == wc.SILENT_ROW:
                assert np.all(np.isfinite(out[b])) and not out[b].any()
        assert not out[b, L[b]:].any()                                   # zeros after L', out to out_stride
    again = _reverb_run(torch, bank_ms, ms, i16, rescale)
    for a, b in zip((out, L, used), again):
        assert np.array_equal(_bits(a), _bits(b))
    return worst


@pytest.mark.parametrize("i16,rescale", [(False, True), (True, True), (False, False)])
@pytest.mark.parametrize("ms", wc.REVERB_MS)
def test_reverb_max_samples_and_length_edges(torch, ms, i16, rescale):
    """Measured on an MI355X, largest |err| / bound per max_samples over the three variants: 16384: 0.36, 16383: 0.39, 8193: 0.39,
    1000: 0.39, 3: 0.49, 2: 0.43, 1: 0.27.  A clip of one to three samples has ||v|| ||h|| close to |y| itself, so its bound is about
    1e-7 |y|, 0.84 to 1.68 float32 ulps.  Through the float32 transform the one-sample clip of [16384-False-False] came back one ulp
    off under the RIR of two taps, 1.12 of its bound; reverb_apply_kernel now convolves a clip of at most 64 samples directly in
    fp64 and rounds once (at most 0.6 of such a bound), and the table has clips of 64 and 65 samples."""
    worst = _reverb_check(torch, ms, ms, i16, rescale)
    print("max_samples %d: reverb max |err| / bound = %.3g (i16=%s, rescale=%s)" % (ms, worst, i16, rescale))


@pytest.mark.parametrize("i16,rescale", [(False, True), (True, True), (False, False)])
@pytest.mark.parametrize("bank_ms,ms", wc.REVERB_MIXED)
def test_reverb_bank_and_call_max_samples_differ(torch, bank_ms, ms, i16, rescale):
    worst = _reverb_check(torch, bank_ms, ms, i16, rescale)
    print("bank %d, call %d: reverb max |err| / bound = %.3g (i16=%s, rescale=%s)" % (bank_ms, ms, worst, i16, rescale))
