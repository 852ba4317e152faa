"""Voice-activity detection on the device (kws_amd.vad, csrc/kws_vad.hip) off the default geometry and past 1024 windows, against
the float64 restatement tests/vad_ref.py on the rows of tests/vad_geometry_cases.py (one packed buffer per geometry, a loud tone
past every length).  tests/test_vad_geometry_host.py proves the table's properties on the CPU.

The checks are those of tests/test_vad_gpu.py, per geometry and for int16 and float32 input: window counts; ratios within
RATIO_BOUND[geometry] (4x the largest error measured on an MI355X on that geometry's rows, never above 1e-4) and exactly 0 past the
count; raw and smoothed flags, intervals, counts and spans exactly.  A window whose float64 ratio lies within the bound of the
threshold may resolve either way and is compared after flipping exactly those raw flags in the reference; at most 0.5 % of a
geometry's windows may be set aside so (on these rows none is: the closest lies further than 1e-4)."""
import ctypes

import numpy as np
import pytest

import vad_geometry_cases as gc
import vad_ref

pytestmark = pytest.mark.gpu

NAMES = ("ratio", "smoothed", "segment_samples", "n_segments", "span", "energy_per_second")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


_vads, _results = {}, {}


def _vad(gid):
    from kws_amd.vad import Vad
    if gid not in _vads:
        _vads[gid] = Vad(**gc.vad_kwargs(gid))
    return _vads[gid]


def _wav(torch, gid, dtype):
    buf, _ = gc.packed(gid)
    a = np.array(buf) if dtype == "int16" else buf.astype(np.float32) * np.float32(1.0 / 32768.0)     # exact
    return torch.from_numpy(a).cuda()


def _detect(torch, gid, dtype, **kw):
    key = (gid, dtype) + tuple(sorted(kw.items()))
    if key not in _results:
        _results[key] = _vad(gid).detect(_wav(torch, gid, dtype), gc.packed(gid)[1], **kw)
    return _results[key]


def _check(gid, dtype, out, n_windows, max_segments=None):
    """out: host arrays by name.  -> the largest |ratio - float64 ratio|"""
    rows, (ref, eps) = gc.recordings(gid), gc.reference(gid)
    rate, thr, kw = gc.ref_kwargs(gid)
    bound = gc.RATIO_BOUND[gid]
    ratio, sm, seg, nseg, span = out["ratio"], out["smoothed"], out["segment_samples"], out["n_segments"], out["span"]
    total = sum(d["ratio"].size for d in ref)
    aside, worst = 0, 0.0
    for r, d in enumerate(ref):
        nw = d["ratio"].size
        assert n_windows[r] == nw
        assert not ratio[r, nw:].any() and not sm[r, nw:].any()
        if nw:
            worst = max(worst, float(np.abs(ratio[r, :nw].astype(np.float64) - d["ratio"]).max()))
        raw = (ratio[r, :nw].astype(np.float64) > thr).astype(np.uint8)
        near = gc.near(d["ratio"], thr, bound)
        assert np.array_equal(raw[~near], d["raw"][~near]), "%s %s: raw flags of row %d" % (gid, dtype, r)
        flip = [int(w) for w in np.nonzero(near & (raw != d["raw"]))[0]]
        aside += int(near.sum())
        want = vad_ref.detect(rows[r], rate, threshold=thr, flip=flip, **kw) if flip else d
        assert np.array_equal(sm[r, :nw], want["smoothed"]), "%s %s: smoothed flags of row %d" % (gid, dtype, r)
        assert int(nseg[r]) == len(want["intervals"]), "%s %s: n_segments of row %d" % (gid, dtype, r)
        keep = int(nseg[r]) if max_segments is None else min(int(nseg[r]), max_segments)
        assert [tuple(v) for v in seg[r, :keep].tolist()] == want["intervals"][:keep], "%s %s: intervals of row %d" % (gid, dtype, r)
        assert not seg[r, keep:].any()
        assert tuple(span[r].tolist()) == want["span"], "%s %s: span of row %d" % (gid, dtype, r)
        tol = 1e-12 if dtype == "int16" else 1e-9                      # integer sums; float32 samples x / 32768 are exact, sums in double
        assert abs(out["energy_per_second"][r] - eps[r]) <= tol * eps[r], (gid, dtype, r)
    print("%s %s: max |ratio - float64 ratio| = %.3e (bound %.3e; float32 restatement on the CPU %.3e), %d of %d windows near the threshold"
          % (gid, dtype, worst, bound, gc.f32_error(gid), aside, total))
    assert aside <= 0.005 * total
    return worst


def _host(res):
    return {n: getattr(res, n).cpu().numpy() for n in NAMES}


@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("gid", gc.ALL)
def test_ratios_flags_and_intervals(torch, gid, dtype):
    res = _detect(torch, gid, dtype)
    assert _check(gid, dtype, _host(res), res.n_windows) <= gc.RATIO_BOUND[gid]


@pytest.mark.parametrize("gid", gc.ALL)
def test_float32_input_gives_the_flags_of_int16_input(torch, gid):
    a, b = _detect(torch, gid, "int16"), _detect(torch, gid, "float32")
    for name in ("smoothed", "segment_samples", "n_segments", "span"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("gid", ["tiny", "r44100"])
def test_two_calls_give_the_same_bits(torch, gid, dtype):
    first = _detect(torch, gid, dtype)
    again = _vad(gid).detect(_wav(torch, gid, dtype), gc.packed(gid)[1])
    for name in NAMES:
        assert torch.equal(getattr(again, name), getattr(first, name)), name


def test_interval_capacity_below_the_count(torch):
    """299 intervals over three chunks at max_segments = 50: the count stays true, the first 50 pairs are kept"""
    full = _detect(torch, "tiny_m1", "int16")
    assert int(full.n_segments[0]) == len(gc.reference("tiny_m1")[0][0]["intervals"]) > 130
    assert len(full.segments[0]) == int(full.n_segments[0])
    res = _detect(torch, "tiny_m1", "int16", max_segments=50)
    assert tuple(res.segment_samples.shape) == (1, 50, 2)
    _check("tiny_m1", "int16", _host(res), res.n_windows, max_segments=50)
    assert torch.equal(res.segment_samples, full.segment_samples[:, :50]) and torch.equal(res.span, full.span)
    with pytest.raises(ValueError):
        res.segments


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_max_windows_beyond_the_stride(torch, dtype):
    """kws_vad_detect itself with 70 more windows than the stride can hold - a whole job past every recording, and a partial one:
    the extra columns are 0 and nothing else moves"""
    from kws_amd import lib as l
    from kws_amd.stream import _stream
    gid = "tiny"
    vad, wav, lens = _vad(gid), _wav(torch, gid, dtype), gc.packed(gid)[1]
    base = _detect(torch, gid, dtype)
    L = l.get_lib()
    R, stride = int(wav.shape[0]), int(wav.shape[1])
    mw0 = vad.n_windows(stride)
    mw, ms = mw0 + 70, int(base.segment_samples.shape[1])
    assert mw0 == base.ratio.shape[1] and (mw + 62) // 63 > (mw0 + 62) // 63 and mw % 63 != 0
    ws_bytes = int(L.kws_vad_workspace_bytes(vad._h, R, mw))
    assert ws_bytes == 8 * R * ((mw + 62) // 63)
    dev = wav.device
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev)
    out = {"ratio": torch.full((R, mw), 7.0, dtype=torch.float32, device=dev), "smoothed": torch.full((R, mw), 7, dtype=torch.uint8, device=dev),
           "segment_samples": torch.full((R, ms, 2), 7, dtype=torch.int32, device=dev), "n_segments": torch.full((R,), 7, dtype=torch.int32, device=dev),
           "span": torch.full((R, 2), 7, dtype=torch.int32, device=dev), "energy_per_second": torch.full((R,), 7.0, dtype=torch.float64, device=dev)}
    d_len = torch.tensor(lens, dtype=torch.int32, device=dev)
    code = l.WAV_I16 if dtype == "int16" else l.WAV_F32
    l.check(L.kws_vad_detect(vad._h, ctypes.c_void_p(wav.data_ptr()), code, R, ctypes.c_int64(stride), ctypes.c_void_p(d_len.data_ptr()), mw, ms,
                             ctypes.c_void_p(ws.data_ptr()), ctypes.c_int64(ws_bytes), *[ctypes.c_void_p(out[n].data_ptr()) for n in NAMES],
                             _stream()))
    torch.cuda.synchronize()
    assert not out["ratio"][:, mw0:].any() and not out["smoothed"][:, mw0:].any()
    assert torch.equal(out["ratio"][:, :mw0], base.ratio) and torch.equal(out["smoothed"][:, :mw0], base.smoothed)
    for name in NAMES[2:]:
        assert torch.equal(out[name], getattr(base, name)), name


PADS = (40, 60)
GATHER = {   # geometry -> [(row, begin, end)]; rows 9 and 10 have 127 and 300 windows
    "tiny": [(10, 16, 700), (10, 4700, 4830), (10, 1000, 2400), (9, 300, 633), (9, 5000, 5100), (0, 0, 0), (-1, 100, 900),
             (20, 100, 900), (18, 33000, 33600), (10, 30, 32)],
    "r44100": [(10, 16, 700), (10, 132000, 132700), (10, 40000, 44000), (9, 3000, 3333), (9, 60000, 60100), (0, 0, 0),
               (-1, 100, 900), (11, 100, 900), (2, 0, 1323), (10, 30, 32)],
}
# clamped at sample 0, clamped at L, longer than every clip, an odd length (an odd remainder under `center` at 1000), an empty cut
# (past L), an empty recording, recordings -1 and R (zeros, as include/kws.h promises), the end of the last row / a whole short
# row, a short cut with an odd remainder at 255 and 257


@pytest.mark.parametrize("align", ["left", "center"])
@pytest.mark.parametrize("clip", [1, 255, 257, 1000])
@pytest.mark.parametrize("gid", sorted(GATHER))
def test_clip_gather(torch, gid, clip, align):
    buf, lens = gc.packed(gid)
    (pb, pa), triples = PADS, GATHER[gid]
    R = len(lens)
    assert [t[0] for t in triples if not 0 <= t[0] < R] == [-1, R]
    want = np.stack([vad_ref.gather(buf[r], lens[r], b, e, clip, pb, pa, align) if 0 <= r < R else np.zeros(clip, np.float32)
                     for r, b, e in triples])
    cut = [min(lens[r], e + pa) - max(0, b - pb) if 0 <= r < R else 0 for r, b, e in triples]
    assert cut[0] < (triples[0][2] - triples[0][1]) + pb + pa and cut[1] < (triples[1][2] - triples[1][1]) + pb + pa   # both clamps bite
    assert cut[2] > 1000 and cut[3] < 1000 and (1000 - cut[3]) % 2 == 1 and cut[4] <= 0 and cut[5] == 0
    assert cut[9] < 255 and (255 - cut[9]) % 2 == 1
    got = {}
    for dtype in ("int16", "float32"):
        res = _detect(torch, gid, dtype)
        out, tri = _vad(gid).clips(None, res, clip, pb, pa, align, triples=triples)
        assert tri.cpu().tolist() == [list(t) for t in triples] and tuple(out.shape) == (len(triples), clip)
        got[dtype] = out.cpu().numpy()
        assert np.array_equal(got[dtype].view(np.uint32), want.view(np.uint32)), (gid, dtype, clip, align)
    assert np.array_equal(got["int16"].view(np.uint32), got["float32"].view(np.uint32))
    assert not got["int16"][4:8].any() and (clip == 1 or got["int16"][:4].any(axis=1).all())
