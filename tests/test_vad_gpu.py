"""Voice-activity detection on the device (kws_amd.vad, csrc/kws_vad.hip) against the float64 restatement tests/vad_ref.py on
the recordings of tests/vad_cases.py: R = 8 in one packed buffer whose tails hold a loud tone.

RATIO_BOUND: the largest |ratio - float64 ratio| measured on these inputs on an MI355X was 4.498e-07 (MEASURED_RATIO_ERR; int16 and float32
input alike); the bound allows 4x that, the margin covering other inputs of the same scale.  Raw and smoothed flags, intervals,
counts and spans are compared exactly; a window whose float64 ratio lies within RATIO_BOUND of the threshold may resolve either
way on the device, and a recording that holds one is compared after flipping exactly those raw flags in the reference (at most
0.5 % of all windows may be set aside so; on these inputs none is)."""
import os
import wave

import numpy as np
import pytest

import vad_cases
import vad_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED_RATIO_ERR = 4.5e-7                 # measured: 4.498e-07
RATIO_BOUND = 4 * MEASURED_RATIO_ERR
THRESHOLD = 0.6


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def vad():
    from kws_amd.vad import Vad
    return Vad(vad_cases.RATE)


@pytest.fixture(scope="module")
def case():
    buf, lens = vad_cases.packed()
    ref = [vad_ref.detect(buf[r, :n], vad_cases.RATE) for r, n in enumerate(lens)]
    eps = [vad_ref.energy_per_second(buf[r, :n], vad_cases.RATE) for r, n in enumerate(lens)]
    return buf, lens, ref, eps


@pytest.fixture(scope="module")
def result(torch, vad, case):
    buf, lens, _, _ = case
    return vad.detect(torch.from_numpy(buf).cuda(), lens)


def _check_flags(res, case, label):
    buf, lens, ref, _ = case
    ratio, sm = res.ratio.cpu().numpy(), res.smoothed.cpu().numpy()
    nseg, span = res.n_segments.cpu().numpy(), res.span.cpu().numpy()
    seg = res.segment_samples.cpu().numpy()
    total = sum(len(d["ratio"]) for d in ref)
    aside, worst = 0, 0.0
    for r, d in enumerate(ref):
        nw = len(d["ratio"])
        assert res.n_windows[r] == nw
        assert not ratio[r, nw:].any() and not sm[r, nw:].any()
        err = float(np.abs(ratio[r, :nw].astype(np.float64) - d["ratio"]).max()) if nw else 0.0
        worst = max(worst, err)
        raw = (ratio[r, :nw].astype(np.float64) > THRESHOLD).astype(np.uint8)
        near = np.abs(d["ratio"] - THRESHOLD) <= RATIO_BOUND
        assert np.array_equal(raw[~near], d["raw"][~near]), "%s: raw flags of recording %d" % (label, r)
        flip = [int(w) for w in np.nonzero(near & (raw != d["raw"]))[0]]
        aside += int(near.sum())
        want = vad_ref.detect(buf[r, :lens[r]], vad_cases.RATE, flip=flip) if flip else d
        assert np.array_equal(sm[r, :nw], want["smoothed"]), "%s: smoothed flags of recording %d" % (label, r)
        assert int(nseg[r]) == len(want["intervals"])
        assert [tuple(v) for v in seg[r, :nseg[r]].tolist()] == want["intervals"]
        assert not seg[r, nseg[r]:].any()
        assert tuple(span[r].tolist()) == want["span"]
    print("%s: max |ratio - float64 ratio| = %.3e (bound %.3e), %d of %d windows near the threshold" % (label, worst, RATIO_BOUND, aside, total))
    assert aside <= 0.005 * total
    return worst


def test_ratios_flags_and_intervals_int16(result, case):
    assert _check_flags(result, case, "int16") <= RATIO_BOUND
    assert result.segments[5] == [(b / 16000, e / 16000) for b, e in case[2][5]["intervals"]] and len(result.segments[5]) == 3
    assert result.segments[6] == [(4800 / 16000, 12000 / 16000)]           # the burst that runs to the last sample is dropped


def test_ratios_flags_and_intervals_float32(torch, vad, case):
    buf, lens, _, _ = case
    res = vad.detect(torch.from_numpy(buf.astype(np.float32) * np.float32(1.0 / 32768.0)).cuda(), lens)
    assert _check_flags(res, case, "float32") <= RATIO_BOUND
    eps = res.energy_per_second.cpu().numpy()
    for r, want in enumerate(case[3]):
        assert abs(eps[r] - want) <= 1e-9 * want                           # float32 samples x / 32768 are exact; sums in double


def test_silence(result, case):
    eps = result.energy_per_second.cpu().numpy()
    for r, want in enumerate(case[3]):
        assert abs(eps[r] - want) <= 1e-12 * want, (r, eps[r], want)
    for thr in (0.2, 100.0, 1000.0):
        assert result.is_silent(thr).tolist() == [w < thr for w in case[3]]
    assert result.is_silent().tolist() == [True, False, False, True, False, False, False, False]


def test_two_calls_give_the_same_bits(torch, vad, case, result):
    buf, lens, _, _ = case
    again = vad.detect(torch.from_numpy(buf).cuda(), lens)
    for name in ("ratio", "smoothed", "segment_samples", "n_segments", "span", "energy_per_second"):
        assert torch.equal(getattr(again, name), getattr(result, name)), name


def test_interval_capacity(torch, vad, case):
    buf, lens, ref, _ = case
    res = vad.detect(torch.from_numpy(buf).cuda(), lens, max_segments=1)
    assert res.n_segments.cpu().tolist()[5] == 3
    assert tuple(res.segment_samples[5, 0].cpu().tolist()) == ref[5]["intervals"][0]
    assert tuple(res.span[5].cpu().tolist()) == ref[5]["span"]
    with pytest.raises(ValueError):
        res.segments


@pytest.mark.parametrize("align", ["left", "center"])
def test_clip_gather(torch, vad, case, result, align):
    buf, lens, _, _ = case
    clip, pb, pa = 8000, 1000, 1500
    triples = [(5, 3840, 10560), (5, 500, 4000), (6, 30000, 36000), (7, 5760, 16000), (2, 0, 321), (3, 100, 100), (0, 0, 0),
               (5, 29760, 37121)]
    # clamped at sample 0, clamped at L, longer than the clip, a cut of odd length, an empty cut, an empty recording
    out, tri = vad.clips(None, result, clip, pb, pa, align, triples=triples)
    got = out.cpu().numpy()
    assert tri.cpu().tolist() == [list(t) for t in triples]
    for i, (r, b, e) in enumerate(triples):
        want = vad_ref.gather(buf[r], lens[r], b, e, clip, pb, pa, align)
        assert np.array_equal(got[i].view(np.uint32), want.view(np.uint32)), (align, i)
    assert np.count_nonzero(got[6]) == 0 and np.count_nonzero(got[2]) > 0
    out, _ = vad.clips(None, result, clip, pb, pa, align, triples=np.zeros((0, 3), np.int32))
    assert tuple(out.shape) == (0, clip)
    # the detected intervals themselves: 3 + 1 + 1 clips in recording order
    out, tri = vad.clips(None, result, clip, 0, 0, align)
    assert tri.cpu().tolist() == [[5, 3840, 10560], [5, 15840, 22400], [5, 29760, 37120], [6, 4800, 12000], [7, 5760, 16000]]
    assert np.array_equal(out[3].cpu().numpy(), vad_ref.gather(buf[6], lens[6], 4800, 12000, clip, 0, 0, align))


def test_goldens_on_the_device():
    from kws_amd.vad import Vad
    g = np.load(os.path.join(ROOT, "tests", "golden", "vad_golden.npz"))
    for i in range(int(g["n"])):
        rate, x = int(g["rate_%d" % i]), g["x_%d" % i]
        res = Vad(rate).detect([x])
        win = g["windows_%d" % i]
        assert np.array_equal(res.smoothed[0].cpu().numpy(), win[:, 1].astype(np.uint8))
        assert res.segments[0] == [tuple(v) for v in g["seconds_%d" % i].tolist()]
        want = float(g["energy_%d" % i])
        assert abs(float(res.energy_per_second[0]) - want) <= 1e-12 * want


def test_host_api(torch, vad, case, result, tmp_path):
    from kws_amd.vad import silent_check, speech_duration
    buf, lens, ref, _ = case
    res = vad.detect([buf[r, :n].copy() for r, n in enumerate(lens)])
    assert res.n_windows == result.n_windows
    for r, nw in enumerate(res.n_windows):
        assert torch.equal(res.ratio[r, :nw], result.ratio[r, :nw]) and torch.equal(res.smoothed[r, :nw], result.smoothed[r, :nw])
    assert res.segments == result.segments
    assert torch.equal(res.span, result.span) and torch.equal(res.energy_per_second, result.energy_per_second)
    g = np.load(os.path.join(ROOT, "tests", "golden", "vad_golden.npz"))
    path = str(tmp_path / "example.wav")
    with wave.open(path, "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(int(g["rate_3"]))
        wf.writeframes(g["x_3"].astype("<i2").tobytes())
    sec = g["seconds_3"]
    assert speech_duration(path) == (float(sec[:, 0].min()), float(sec[:, 1].max()))
    assert speech_duration((g["x_2"], int(g["rate_2"]))) == (0.0, 0.0)
    assert silent_check(path, 0.2) is False and silent_check(path, 1e9) is True
