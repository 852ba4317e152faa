"""Host-side checks of the query-by-example feature (include/kws.h: the argument checks of kws_dtw_workspace_bytes, kws_dtw and
kws_dtw_peaks; kws_amd.qbe's validation) and of the reference and the cases the GPU tests use (tests/dtw_ref.py, tests/dtw_cases.py):
no GPU."""
import ctypes

import numpy as np
import pytest

import dtw_cases as dc
import dtw_ref as dr
from kws_amd import lib as L

FAKE = 0x10000      # a non-null, aligned address: every case below must be refused before anything is read through it


def _lib():
    return L.get_lib()


# ---- the reference against brute force ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L_,n", ((1, 5), (2, 6), (3, 7), (5, 12), (7, 9)))
@pytest.mark.parametrize("metric", (dr.DOT, dr.L2), ids=("dot", "l2"))
def test_reference_equals_brute_force(L_, n, metric):
    q, x = dc.int_rows(L_, L_, 4), dc.int_rows(100 + n, n, 4)
    d = dr.local_cost(q, x, metric)
    best, starts = dr.brute_force(d)
    for dtype in (np.float32, np.float64):
        cost, start = dr.dtw(q, x, metric, dtype=dtype)
        total, _ = dr.dtw_from_cost(dr.local_cost(q, x, metric, dtype), 0, dtype)
        np.testing.assert_array_equal(total.astype(np.float64), best)                       # integers: exact in both formats
        np.testing.assert_array_equal(cost, total / dtype(L_))
        for j in range(n):
            assert (start[j] == -1 and not starts[j]) or start[j] in starts[j], (j, start[j], starts[j])
    # what the issue states about reach and span
    h = dc.unreachable(L_)
    assert np.isinf(cost[:h]).all() and np.isfinite(cost[h:]).all()
    span = np.arange(n)[h:] - start[h:] + 1
    assert span.min() >= (L_ + 2) // 2 and span.max() <= 2 * L_ - 1


@pytest.mark.parametrize("L_", (1, 2, 17, 63, 64))
def test_reference_tiles_are_bit_identical(L_):
    n = 300
    for data, metric in ((lambda s, *sh: dc.int_rows(s, *sh), dr.L2),
                         (lambda s, *sh: np.random.default_rng(s).standard_normal(sh).astype(np.float32) * 0.2, dr.DOT)):
        q, x = data(L_, L_, 8), data(500 + L_, n, 8)
        cost, start = dr.dtw(q, x, metric)
        for tile in (32, 97, 128):
            tc, ts = dr.dtw_tiled(q, x, metric, tile)
            np.testing.assert_array_equal(tc.view(np.uint32), cost.view(np.uint32))
            np.testing.assert_array_equal(ts, start)


def test_tie_rule_by_hand():
    # all costs equal: every path weighs 3.  Frame 1 is reached by candidate 3 alone, (0, 0) -> (2, 1); from frame 2 on all candidates
    # tie and candidate 1 (the diagonal) wins in both rows, so a match ending at j began at j - 2
    d = np.ones((3, 6), np.float32)
    c, s = dr.dtw_from_cost(d)
    np.testing.assert_array_equal(c, [np.inf, 3, 3, 3, 3, 3])
    np.testing.assert_array_equal(s, [-1, 0, 0, 1, 2, 3])
    # (1, 2): candidate 1 comes from (0, 1) = 5, candidate 2 from (0, 0) = 1: candidate 2 wins and carries start 0
    d = np.array([[1, 5, 9, 9], [9, 9, 1, 9]], np.float32)
    c, s = dr.dtw_from_cost(d)
    assert c[2] == 2 and s[2] == 0
    # (2, 2): candidate 1 = C(1, 1) + d = (1 + 1) + 1 = 3 from start 0; candidate 3 = C(0, 1) + 2 d = 1 + 2 = 3 from start 1: the tie
    # goes to candidate 1
    d = np.array([[1, 1, 9], [9, 1, 9], [9, 9, 1]], np.float32)
    c, s = dr.dtw_from_cost(d)
    assert c[2] == 3 and s[2] == 0
    # ... and when the diagonal is dearer by one, candidate 3 takes it with start 1
    d = np.array([[2, 1, 9], [9, 1, 9], [9, 9, 1]], np.float32)
    c, s = dr.dtw_from_cost(d)
    assert c[2] == 3 and s[2] == 1
    # one frame short of the only finite frame, and exactly at it
    assert np.isinf(dr.dtw(np.zeros((5, 4)), np.zeros((2, 4)), dr.L2)[0]).all()
    cost, start = dr.dtw(np.zeros((5, 4)), np.zeros((3, 4)), dr.L2)
    assert np.isinf(cost[:2]).all() and cost[2] == 0 and start[2] == 0


def test_peak_picker_by_hand():
    inf = np.inf
    cost = np.array([[[3, 1, 2, 1, 5, 0, 4, inf],
                      [3, 1, 0, 2, 5, 0, 4, inf]]], np.float32)
    start = np.arange(16, dtype=np.int32).reshape(1, 2, 8)
    # one keyword of two templates: the curve is 3 1 0 1 5 0 4 inf; the minimum 0 stands at frames 2 (template 1) and 5 (both: template 0)
    count, end, hs, hc, ht = dr.peaks(cost, start, [0, 0], 1, 10.0, 1, 3)
    assert count[0, 0] == 3 and end[0, 0].tolist() == [2, 5, 1] and ht[0, 0].tolist() == [1, 0, 0] and hs[0, 0].tolist() == [10, 5, 1]
    assert hc[0, 0].tolist() == [0, 0, 1]
    # min_gap 3 suppresses frames 0 .. 4 around frame 2, then 3 .. 7 around frame 5: nothing is left
    count, end, hs, hc, ht = dr.peaks(cost, start, [0, 0], 1, 10.0, 3, 3)
    assert count[0, 0] == 2 and end[0, 0].tolist() == [2, 5, -1] and hc[0, 0, 2] == inf and ht[0, 0, 2] == -1
    # a threshold below everything; the +inf frame is never taken
    assert dr.peaks(cost, start, [0, 0], 1, -1.0, 1, 3)[0][0, 0] == 0
    assert dr.peaks(cost, start, [0, 0], 1, inf, 1, 8)[0][0, 0] == 7
    # two keywords of one template each
    count, end, hs, hc, ht = dr.peaks(cost, start, [0, 1], 2, 0.0, 1, 2)
    assert count[0].tolist() == [1, 2] and end[0, 0].tolist() == [5, -1] and end[0, 1].tolist() == [2, 5] and ht[0, 1].tolist() == [1, 1]


def test_case_table():
    assert dc.LENGTHS == (1, 2, 3, 31, 32, 33, 63, 64) and dc.WIDTHS == (4, 20, 64)
    for L_ in dc.LENGTHS:
        want = {0, 1, 2, -(-(L_ - 1) // 2), -(-(L_ - 1) // 2) + 1, 64, 65, 127, 128, 129, 700}
        assert set(dc.frame_counts(L_)) == want and want <= set(dc.ALL_COUNTS)
    t, lens, rows, n = dc.exact_data(64)
    assert np.abs(t[0, :1]).max() <= 3 and np.abs(rows[-1, :700]).max() <= 3 and (rows == np.round(rows)).all()
    cost, start = dr.dtw(t[-1, :64], rows[-1, :700], dr.L2)
    assert np.isfinite(cost).sum() == 700 - 32 and cost[np.isfinite(cost)].max() * 64 <= 64 * 64 * 36 < 2 ** 24
    assert dc.TILES == (0, 32, 64, 97, 700) and dc.TILE_LENGTHS == (1, 2, 17, 64)
    assert dc.RAGGED_FRAMES == (0, 1, 40, 333, 700) and dc.RAGGED_LENGTHS == (1, 7, 40, 64) and dc.MAX_FRAMES == 704
    assert dc.cosine_bound(64, 20) == (20 + 128 + 4) * 2.0 ** -24
    names = [c[0] for c in dc.PEAK_CASES]
    assert {"ties", "k_reached", "nothing_below", "gap_1", "gap_past_n", "single_groups"} <= set(names)


def test_scene_is_found_by_the_reference_alone():
    """the end-to-end inputs of the GPU test, through the featurizer oracle, tests/vad_ref.py and the numpy DTW: exactly the planted
    occurrences, each end within 3 frames, and the right word for the one-second clips"""
    import vad_ref as vr
    from oracle import featurizer_oracle as fo
    g = fo.geometry()
    W, H = g["window_samples"], g["hop_samples"]

    def unit(x):
        x = x.astype(np.float32)
        nrm = np.linalg.norm(x.astype(np.float64), axis=-1, keepdims=True)
        return (x / np.where(nrm > 0, nrm, 1.0)).astype(np.float32)

    names = list(dc.WORDS)
    tm = []
    for name in names:
        ex = dc.example(name)
        b, e = vr.detect(ex, dc.RATE)["span"]
        assert e > b
        tm.append(unit(fo.mfcc_spec(ex[b:e] / 32768.0)))
        assert 1 <= tm[-1].shape[0] <= 64
    recs, planted = dc.scene()
    K, gap = dc.PLANTED_PER_PAIR, int(round(0.5 * dc.RATE / H))
    for r, rec in enumerate(recs):
        x = unit(fo.mfcc_spec(rec / 32768.0))
        cost = np.stack([dr.dtw(t, x, dr.DOT)[0] for t in tm])[None]
        start = np.stack([dr.dtw(t, x, dr.DOT)[1] for t in tm])[None]
        count, end, _, _, _ = dr.peaks(cost, start, [0, 1], 2, np.inf, gap, K)
        for k, name in enumerate(names):
            want = sorted(dc.planted_end_frame(e, W, H) for pr_, pn, _, e in planted if pr_ == r and pn == name)
            got = sorted(end[0, k, :count[0, k]].tolist())
            assert len(got) == len(want) == K and all(abs(a - b) <= 3 for a, b in zip(got, want)), (r, name, got, want)
    for r, name, b, e in planted:
        clip = unit(fo.mfcc_spec(dc.clip_around(recs[r], b, e) / 32768.0))
        best = [dr.dtw(t, clip, dr.DOT)[0].min() for t in tm]
        assert names[int(np.argmin(best))] == name, (r, name, best)


# ---- the C ABI refuses bad arguments before any device work -----------------------------------------------------------------------
def _dtw(Q=4, Lmax=64, R=3, max_frames=700, D=20, metric=0, tile_frames=0, ws_bytes=0, **ptr):
    p = dict(templates=FAKE, tmpl_len=FAKE, rows=FAKE, n_frames=FAKE, cost=FAKE, start=FAKE, ws=None)
    p.update(ptr)
    return _lib().kws_dtw(p["templates"], p["tmpl_len"], Q, Lmax, p["rows"], p["n_frames"], R, max_frames, D, metric, tile_frames, p["cost"],
                          p["start"], p["ws"], ws_bytes, None)


@pytest.mark.parametrize("what,kw", [
    ("D = 0", dict(D=0)), ("D = 2", dict(D=2)), ("D = 6", dict(D=6)), ("D = 68", dict(D=68)), ("Lmax = 0", dict(Lmax=0)), ("Lmax = 65", dict(Lmax=65)),
    ("metric 2", dict(metric=2)), ("metric -1", dict(metric=-1)), ("tile 31", dict(tile_frames=31)), ("tile -1", dict(tile_frames=-1)),
    ("tile 2^20 + 1", dict(tile_frames=2 ** 20 + 1)), ("max_frames 0", dict(max_frames=0)), ("max_frames 2^30 + 1", dict(max_frames=2 ** 30 + 1)),
    ("R < 0", dict(R=-1)), ("Q < 0", dict(Q=-1)),
    ("null templates", dict(templates=None)), ("null tmpl_len", dict(tmpl_len=None)), ("null rows", dict(rows=None)),
    ("null n_frames", dict(n_frames=None)), ("null cost", dict(cost=None)), ("null start", dict(start=None)),
    ("misaligned templates", dict(templates=FAKE + 4)), ("misaligned rows", dict(rows=FAKE + 8)), ("misaligned cost", dict(cost=FAKE + 2)),
])
def test_dtw_refuses_bad_arguments_without_a_device(what, kw):
    assert _dtw(**kw) == L.ERR_INVALID, what
    assert _lib().kws_last_error()


def test_dtw_workspace_and_launch_limits():
    lib = _lib()
    assert lib.kws_dtw_workspace_bytes(3, 4, 700, 20, 0) == 0
    assert lib.kws_dtw_workspace_bytes(3, 4, 700, 20, 32) == 0
    for kw in (dict(D=6), dict(D=0), dict(D=68), dict(tile_frames=31), dict(tile_frames=2 ** 20 + 1), dict(max_frames=0), dict(R=-1), dict(Q=-1)):
        a = dict(R=3, Q=4, max_frames=700, D=20, tile_frames=0)
        a.update(kw)
        assert lib.kws_dtw_workspace_bytes(a["R"], a["Q"], a["max_frames"], a["D"], a["tile_frames"]) == L.ERR_INVALID, kw
    # more (recording, template, tile) jobs than a launch takes
    assert lib.kws_dtw_workspace_bytes(65536, 1024, 2 ** 20, 20, 32) == L.ERR_UNSUPPORTED
    assert _dtw(R=65536, Q=1024, max_frames=2 ** 20, tile_frames=32) == L.ERR_UNSUPPORTED
    # nothing to do
    assert _dtw(R=0) == 0 and _dtw(Q=0) == 0


def _peaks(R=2, Q=5, max_frames=200, G=3, threshold=1.0, min_gap=5, K=8, group_host=(0, 0, 0, 1, 2), **ptr):
    p = dict(cost=FAKE, start=FAKE, group=FAKE, count=FAKE, end=FAKE, hit_start=FAKE, hit_cost=FAKE, hit_template=FAKE)
    p.update(ptr)
    gh = (ctypes.c_int32 * len(group_host))(*group_host) if group_host is not None else None
    return _lib().kws_dtw_peaks(p["cost"], p["start"], R, Q, max_frames, p["group"], gh, G, threshold, min_gap, K, p["count"], p["end"],
                                p["hit_start"], p["hit_cost"], p["hit_template"], None)


@pytest.mark.parametrize("what,kw", [
    ("R < 0", dict(R=-1)), ("Q = 0", dict(Q=0, group_host=None)), ("Q = 1025", dict(Q=1025, group_host=None)), ("max_frames 0", dict(max_frames=0)),
    ("G = 0", dict(G=0)), ("G > Q", dict(G=6)), ("K = 0", dict(K=0)), ("K = 65", dict(K=65)), ("min_gap 0", dict(min_gap=0)),
    ("NaN threshold", dict(threshold=float("nan"))),
    ("null cost", dict(cost=None)), ("null start", dict(start=None)), ("null group", dict(group=None)), ("null count", dict(count=None)),
    ("null end", dict(end=None)), ("null hit_start", dict(hit_start=None)), ("null hit_cost", dict(hit_cost=None)),
    ("null hit_template", dict(hit_template=None)),
    ("group not from 0", dict(group_host=(1, 1, 1, 2, 2))), ("group decreasing", dict(group_host=(0, 1, 0, 1, 2))),
    ("group with a gap", dict(group_host=(0, 0, 2, 2, 2))), ("group ends early", dict(group_host=(0, 0, 0, 1, 1))),
])
def test_peaks_refuses_bad_arguments_without_a_device(what, kw):
    assert _peaks(**kw) == L.ERR_INVALID, what
    assert _lib().kws_last_error()


def test_peaks_r_zero_is_ok():
    assert _peaks(R=0) == 0
    assert _peaks(R=0, group_host=None) == 0


# ---- kws_amd.qbe: ValueError before any device work ---------------------------------------------------------------------------------
def _host_templates(qbe, Q=3, Lmax=10, D=20, keywords=("a", "a", "b")):
    import torch
    t = qbe.Templates(torch.zeros((Q, Lmax, D)), np.full((Q,), Lmax, np.int32), sorted(set(keywords)), np.array([0, 0, 1], np.int32))
    return t


def test_python_validation():
    import torch
    from classifier.params import pr
    from kws_amd import qbe
    t = _host_templates(qbe)                                          # host tensors: the device check comes last
    rows, n = torch.zeros((2, 50, 20)), np.array([50, 20])
    with pytest.raises(ValueError, match="Templates object"):
        qbe.match_rows(None, rows, n)
    with pytest.raises(ValueError, match="Templates object"):
        qbe.search(rows, [np.zeros(16000, np.int16)], threshold=1.0)
    for call in (lambda m: qbe.match_rows(t, rows, n, metric=m), lambda m: qbe.match(t, [np.zeros(16000, np.int16)], metric=m),
                 lambda m: qbe.search(t, [np.zeros(16000, np.int16)], metric=m), lambda m: qbe.classify(t, [np.zeros(16000, np.int16)], metric=m)):
        with pytest.raises(ValueError, match="metric"):
            call("manhattan")
    for tile in (-1, 31, 2 ** 20 + 1):
        with pytest.raises(ValueError, match="tile_frames"):
            qbe.match_rows(t, rows, n, tile_frames=tile)
        with pytest.raises(ValueError, match="tile_frames"):
            qbe.search(t, [np.zeros(16000, np.int16)], tile_frames=tile)
    for bad in (torch.zeros((2, 50)), torch.zeros((2, 50, 20), dtype=torch.float64), torch.zeros((2, 50, 40))[:, :, ::2], torch.zeros((2, 0, 20)),
                np.zeros((2, 50, 20), np.float32)):
        with pytest.raises(ValueError, match="must be a contiguous"):
            qbe.match_rows(t, bad, n)
    with pytest.raises(ValueError, match="1..64 wide"):
        qbe.match_rows(t, torch.zeros((2, 50, 68)), n)
    with pytest.raises(ValueError, match="wide, the templates"):
        qbe.match_rows(t, torch.zeros((2, 50, 12)), n)
    for bad_n in (np.array([50]), np.array([50, 51]), np.array([-1, 3]), np.array([1.0, 2.0])):
        with pytest.raises(ValueError, match="n_frames"):
            qbe.match_rows(t, rows, bad_n)
    with pytest.raises(ValueError, match="GPU"):
        qbe.match_rows(t, rows, n)
    # search / peaks
    for kw, pat in ((dict(threshold=float("nan")), "NaN"), (dict(threshold=1.0, min_gap_s=-0.1), "min_gap_s"), (dict(threshold=1.0, max_hits=0), "max_hits"),
                    (dict(threshold=1.0, max_hits=65), "max_hits")):
        with pytest.raises(ValueError, match=pat):
            qbe.search(t, [np.zeros(16000, np.int16)], **kw)
    with pytest.raises(ValueError, match="made from rows"):
        qbe.search(t, [np.zeros(16000, np.int16)], threshold=1.0)
    cost, start = torch.zeros((2, 3, 50)), torch.zeros((2, 3, 50), dtype=torch.int32)
    for kw, pat in ((dict(threshold=float("nan"), min_gap=1, max_hits=4), "NaN"), (dict(threshold=1.0, min_gap=0, max_hits=4), "min_gap"),
                    (dict(threshold=1.0, min_gap=1, max_hits=65), "max_hits")):
        with pytest.raises(ValueError, match=pat):
            qbe.peaks(t, cost, start, **kw)
    with pytest.raises(ValueError, match="cost must be"):
        qbe.peaks(t, cost.double(), start, 1.0, 1, 4)
    with pytest.raises(ValueError, match="cost must be"):
        qbe.peaks(t, torch.zeros((2, 4, 50)), start, 1.0, 1, 4)
    with pytest.raises(ValueError, match="cost is"):
        qbe.peaks(t, cost, torch.zeros((2, 3, 49), dtype=torch.int32), 1.0, 1, 4)
    with pytest.raises(ValueError, match="GPU"):
        qbe.peaks(t, cost, start, 1.0, 1, 4)
    # enrolment: the keywords, the examples and their lengths are checked before anything is featurized
    clip = np.zeros(16000, np.int16)
    with pytest.raises(ValueError, match="keywords for"):
        qbe.Templates.enroll(pr, [clip, clip], ["a"])
    with pytest.raises(ValueError, match="keywords for"):
        qbe.Templates.enroll(pr, [], [])
    with pytest.raises(ValueError, match="non-empty string"):
        qbe.Templates.enroll(pr, [clip], [3])
    with pytest.raises(ValueError, match="1-D int16"):
        qbe.Templates.enroll(pr, [clip.astype(np.float32)], ["a"])
    with pytest.raises(ValueError, match="at most 64"):
        qbe.Templates.from_rows(torch.zeros((3, 65, 20)), [64, 3, 3], ["a", "a", "b"])
    with pytest.raises(ValueError, match="no rows"):
        qbe.Templates.from_rows(torch.zeros((3, 10, 20)), [0, 3, 3], ["a", "a", "b"])
    with pytest.raises(ValueError, match="GPU"):
        qbe.Templates.from_rows(torch.zeros((3, 10, 20)), [10, 3, 3], ["a", "b", "a"])


def test_enrolment_refuses_long_examples_with_the_length_in_seconds():
    """checked on the host from the sample count when nothing is trimmed: 64 rows are (63 x 512 + 1024) / 16000 = 2.08 s"""
    from classifier.params import pr
    from kws_amd import qbe
    with pytest.raises(ValueError, match=r"2\.112 s long \(65 rows\); a template holds at most 64 rows, 2\.080 s"):
        qbe.Templates.enroll(pr, [np.zeros(63 * 512 + 1024 + 512, np.int16)], ["a"], trim=False)
    with pytest.raises(ValueError, match="shorter than one window"):
        qbe.Templates.enroll(pr, [np.zeros(1000, np.int16)], ["a"], trim=False)
    names, group, order = qbe.Templates._order(["b", "a", "b", "c", "a"], 5)
    assert names == ["b", "a", "c"] and group.tolist() == [0, 1, 0, 2, 1] and order.tolist() == [0, 2, 1, 4, 3]
