"""CPU tests of the harvest of a scan (kws_amd.stream.collect / peaks / Detections): the reference tests/mine_ref.py alone on
the synthetic scan of tests/sweep_cases.py and on the tie case, so that no comparison of tests/test_mine_gpu.py passes vacuously;
the argument checks of `collect` / `peaks`, which come before any device use; and those of the two C entry points."""
import numpy as np
import pytest

import mine_ref
import sweep_cases as cases
import sweep_ref

POINTS = [(0.5, 3, 1024), (0.25, 1, 4096)]


def _all(sens, level, chunk_size, events=cases.EVENTS):
    index, score = cases.build()
    return [mine_ref.detections(index[r], score[r], n, cases.BACKGROUND, sens, level, chunk_size, None if events is None else events[r])
            for r, n in enumerate(cases.N_CHUNKS)]


@pytest.mark.parametrize("point,per_rec,kinds", [(POINTS[0], [0, 0, 3, 0, 1, 3], (2, 2, 3)), (POINTS[1], [0, 0, 10, 4, 4, 18], (6, 12, 18))])
def test_reference_detections_have_every_kind_and_the_sweeps_totals(point, per_rec, kinds):
    sens, level, chunk_size = point
    dets = _all(sens, level, chunk_size)
    assert [len(d) for d in dets] == per_rec
    flat = [d for rec in dets for d in rec]
    count = lambda kind: sum(1 for d in flat if d[2] == kind)                       # noqa: E731
    assert (count(mine_ref.HIT), count(mine_ref.DUPLICATE), count(mine_ref.FALSE_ALARM)) == kinds
    assert count(mine_ref.UNLABELLED) == 0 and min(kinds) > 0
    index, score = cases.build()
    want = sweep_ref.sweep(index, score, cases.N_CHUNKS, cases.BACKGROUND, [sens], [level], chunk_size, cases.EVENTS)[:, 0, 0]
    for r, rec in enumerate(dets):
        got = [len(rec)] + [sum(1 for d in rec if d[2] == k) for k in (mine_ref.HIT, mine_ref.FALSE_ALARM, mine_ref.DUPLICATE)]
        assert got == want[r, :4].tolist()
        hits = [d for d in rec if d[2] == mine_ref.HIT]
        assert sum(d[0] - cases.EVENTS[r][d[3]][1] for d in hits) == want[r, sweep_ref.LATENCY]
        assert all(d[3] == -1 for d in rec if d[2] == mine_ref.FALSE_ALARM)
        assert all(0 <= d[3] < len(cases.EVENTS[r]) and cases.EVENTS[r][d[3]][0] == d[1] for d in rec if d[2] in (mine_ref.HIT, mine_ref.DUPLICATE))
        assert [d[0] for d in rec] == sorted(d[0] for d in rec)
    bare = _all(sens, level, chunk_size, events=None)
    assert [[d[0] for d in rec] for rec in bare] == [[d[0] for d in rec] for rec in dets]
    assert all(d[2] == mine_ref.UNLABELLED and d[3] == -1 for rec in bare for d in rec)
    if point == POINTS[1]:                                                            # event positions other than 0 are compared too
        assert {d[3] for rec in dets for d in rec} >= {-1, 0, 1, 2}


def test_reference_peaks_hand_checked():
    index, score = cases.build()
    got = mine_ref.peaks(index[5], score[5], 130, cases.BACKGROUND, 0.3, 8, 8)
    assert [p[0] for p in got] == [5, 13, 21, 29, 37, 63, 76, 103]
    assert all(p[1] == index[5, p[0]] and p[2] == score[5, p[0]] and p[1] != cases.BACKGROUND and p[2] > 0.3 for p in got)
    got = mine_ref.peaks(index[5], score[5], 130, cases.BACKGROUND, 0.3, 8, 8, cases.EVENTS[5])
    assert [p[0] for p in got] == [31, 39, 63, 50]                                   # pick order, not chunk order
    assert all(not any(lo <= p[0] <= hi for _, lo, hi in cases.EVENTS[5]) for p in got)
    assert mine_ref.peaks(index[1], score[1], 1, cases.BACKGROUND, 0.3, 8, 8) == [(0, 1, 1.0)]
    assert mine_ref.peaks(index[0], score[0], 0, cases.BACKGROUND, 0.3, 8, 8) == []
    assert mine_ref.peaks(index[5], score[5], 130, cases.BACKGROUND, 1.0, 8, 8) == []      # `score > min_score` is strict
    for r, n in enumerate(cases.N_CHUNKS):                                            # a read of the poisoned padding would be picked
        whole = mine_ref.peaks(index[r], score[r], cases.STRIDE, cases.BACKGROUND, 0.3, 1, 64)
        assert any(p[0] >= n for p in whole)


def test_tie_case_has_ties_among_the_picked_scores():
    index, score = mine_ref.tie_case()
    assert (index[:, :1000] == 0).any() and len(np.unique(score[0, :64])) == 5
    for r, n in enumerate(mine_ref.TIE_N_CHUNKS):
        for base in range(0, n - 63, 64):                                             # equal scores inside every 64-lane stride
            assert len(np.unique(score[r, base:base + 64])) < 64
        got = mine_ref.peaks(index[r], score[r], n, 0, 0.0, 1, 64)
        scores = [p[2] for p in got]
        assert len(got) > 8 and len(set(scores)) < len(scores)
        assert scores == sorted(scores, reverse=True)                                 # min_gap 1 suppresses nothing: best first
        for a, b in zip(got, got[1:]):
            assert a[2] > b[2] or a[0] < b[0]                                         # among equal scores the lower chunk first
    gap = mine_ref.peaks(index[2], score[2], 1000, 0, 0.0, 16, 64)
    assert all(abs(a[0] - b[0]) >= 16 for i, a in enumerate(gap) for b in gap[:i]) and len(gap) < 64


def test_audio_buffer_and_saved_samples():
    pcm = np.array([-32768, 32767, 1, -1, 12345, -12345, 7], np.int16)
    buf = mine_ref.audio_buffer(pcm, 0, 3, 5)
    np.testing.assert_array_equal(buf, np.array([0, 0, -1.0, 32767 / 32768.0, 1 / 32768.0]))
    np.testing.assert_array_equal(mine_ref.audio_buffer(pcm, 1, 3, 5), pcm[1:6] / 32768.0)
    np.testing.assert_array_equal(mine_ref.audio_buffer(pcm, 2, 3, 5), pcm[2:7] / 32768.0)      # the short last chunk: n_k = N
    # truncation toward zero: 32767 * 32767 / 32768 = 32766.00003 -> 32766, -1 * 32767 / 32768 -> 0, not a copy of the PCM
    np.testing.assert_array_equal(mine_ref.saved_samples(pcm / 32768.0), np.array([-32767, 32766, 0, 0, 12344, -12344, 6], np.int16))


def test_collect_and_peaks_check_their_arguments_before_any_device_use():
    import torch
    from kws_amd.stream import collect, peaks
    index, score = (torch.from_numpy(a) for a in cases.build())                       # host tensors: no device is touched
    ok = (index, score, cases.N_CHUNKS)
    for k in (0, -1, 65):
        with pytest.raises(ValueError, match="1..64"):
            peaks(ok, 1024, k=k)
    for gap in (0, -3):
        with pytest.raises(ValueError, match="min_gap"):
            peaks(ok, 1024, min_gap=gap)
    for fn in (collect, peaks):
        with pytest.raises(ValueError, match="chunk_size"):
            fn(ok, 0)
        with pytest.raises(ValueError, match="int32 / float64"):
            fn((index, score.float(), cases.N_CHUNKS), 1024)
        with pytest.raises(ValueError, match="int32 / float64"):
            fn((None, None, []), 1024)
        with pytest.raises(ValueError, match="n_chunks"):
            fn((index, score, [cases.STRIDE + 1] * 6), 1024)
        with pytest.raises(ValueError, match="n_chunks"):
            fn((index, score, cases.N_CHUNKS[:5]), 1024)
        with pytest.raises(ValueError, match="lengths"):
            fn(ok, 1024, events=cases.sample_events(1024), lengths=[n * 1024 + 1 for n in cases.N_CHUNKS], tolerance_samples=0)
        with pytest.raises(ValueError, match="recording 5.*overlap"):                 # only the tolerance makes the windows overlap
            fn(ok, 1024, events=cases.sample_events(1024), tolerance_samples=5 * 1024)
        with pytest.raises(ValueError, match="recording 2.*class"):
            fn(ok, 1024, events=[[], [], [(0, 0, 100)], [], [], []], tolerance_samples=0)
        with pytest.raises(ValueError, match="CUDA"):                                  # everything else is right: the last check
            fn(ok, 1024, events=cases.sample_events(1024), tolerance_samples=0)
    with pytest.raises(ValueError, match="max_det"):
        collect(ok, 1024, max_det=-1)


def test_entry_point_argument_errors():
    from kws_amd import lib as l
    L = l.get_lib()
    assert len(L.kws_stream_collect.argtypes) == 18 and len(L.kws_stream_peaks.argtypes) == 16
    assert (l.DET_UNLABELLED, l.DET_HIT, l.DET_DUPLICATE, l.DET_FALSE_ALARM) == (0, 1, 2, 3)

    def collect(R=2, stride=8, chunk=1024, max_det=4):
        return L.kws_stream_collect(None, None, R, stride, None, 0, chunk, 0.5, 3, None, None, None, None, max_det, None, None, None, None)

    def peaks(R=2, stride=8, K=8, gap=1):
        return L.kws_stream_peaks(None, None, R, stride, None, 0, 0.0, gap, None, None, None, K, None, None, None, None)

    assert collect(R=0) == 0 and peaks(R=0) == 0                                        # nothing to do, nothing dereferenced
    assert collect(max_det=-1) == -1 and b"max_det=-1" in L.kws_last_error()
    assert collect(chunk=0) == -1 and b"chunk_size=0" in L.kws_last_error()
    assert collect(R=-1) == -1 and b"R=-1" in L.kws_last_error()
    assert collect() == -1 and b"null argument" in L.kws_last_error()
    for K in (0, 65, -1):
        assert peaks(K=K) == -1 and b"1..64" in L.kws_last_error()
        assert peaks(K=K, R=0) == -1                                                    # the limits hold whatever R is
    assert peaks(gap=0) == -1 and b"min_gap=0" in L.kws_last_error()
    assert peaks(R=-1) == -1 and b"R=-1" in L.kws_last_error()
    assert peaks() == -1 and b"null argument" in L.kws_last_error()


def test_listen_py_lists_the_save_options():
    import listen
    assert listen.default_config["save_dir"] is None
    assert callable(listen.Listener.collect_wav)
    assert sorted(listen.SAVE_KINDS) == ["all", "duplicates", "false_alarms", "hits"]
