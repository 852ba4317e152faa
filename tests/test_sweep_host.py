"""CPU tests of the operating-point sweep's host side: kws_amd.stream.events_to_chunks on hand-computed cases, the arithmetic
of SweepResult.det / best on hand-made counts, listen.py's --sensitivities and labels-file parsing, the argument checks of the C
entry point kws_stream_sweep, and the properties the GPU test needs of its synthetic scan (tests/sweep_cases.py) on the
reference tests/sweep_ref.py alone."""
import ctypes
import math

import numpy as np
import pytest

import sweep_cases
import sweep_ref


def test_events_to_chunks_hand_computed():
    from kws_amd.stream import events_to_chunks
    # chunk 1024, N = 10 * 1024 (T = 10).  (1000, 2048): ends exactly on a chunk boundary -> its last sample 2047 is in chunk 1
    assert events_to_chunks([[(2, 1000, 2048)]], [10240], 1024, 0) == [[(2, 0, 1)]]
    assert events_to_chunks([[(2, 1000, 2049)]], [10240], 1024, 0) == [[(2, 0, 2)]]
    # tolerance: (2047 + 1024) // 1024 = 2; (2047 + 1025) // 1024 = 3
    assert events_to_chunks([[(2, 1000, 2048)]], [10240], 1024, 1024) == [[(2, 0, 2)]]
    assert events_to_chunks([[(2, 1000, 2048)]], [10240], 1024, 1025) == [[(2, 0, 3)]]
    # tolerance clipped at T - 1: N = 10000 -> T = 10, (9000 - 1 + 16000) // 1024 = 24 -> 9
    assert events_to_chunks([[(1, 8192, 9000)]], [10000], 1024, 16000) == [[(1, 8, 9)]]
    # chunk 3000, N = 10000 -> T = 4: lo = 2999 // 3000 = 0, hi = (6000 - 1 + 500) // 3000 = 2; second: lo 3, hi min(3, 4) = 3
    assert events_to_chunks([[(4, 9000, 9999), (3, 2999, 6000)]], [10000], 3000, 500) == [[(3, 0, 2), (4, 3, 3)]]      # sorted by lo
    # chunk 4096, two recordings, the second without events; N = 4097 -> T = 2
    assert events_to_chunks([[(1, 4096, 4097)], []], [4097, 50000], 4096, 0) == [[(1, 1, 1)], []]
    assert events_to_chunks([[(1, 0, 4096)], []], [4097, 50000], 4096, 1) == [[(1, 0, 1)], []]
    assert events_to_chunks([], [], 1024, 0) == []


def test_events_to_chunks_errors_name_the_recording():
    from kws_amd.stream import events_to_chunks
    ok = [(1, 0, 100)]
    with pytest.raises(ValueError, match="recording 1.*overlap"):                      # lo[e + 1] <= hi[e]: chunks 0..1 and 1..2
        events_to_chunks([ok, [(1, 0, 2048), (2, 2000, 3000)]], [10240, 10240], 1024, 0)
    assert events_to_chunks([[(1, 0, 2048), (2, 2048, 3000)]], [10240], 1024, 0) == [[(1, 0, 1), (2, 2, 2)]]
    with pytest.raises(ValueError, match="recording 0.*overlap"):                      # only the tolerance makes them overlap
        events_to_chunks([[(1, 0, 2048), (2, 2048, 3000)]], [10240], 1024, 1)
    with pytest.raises(ValueError, match="recording 2.*class"):                        # the background
        events_to_chunks([ok, ok, [(0, 0, 100)]], [5000] * 3, 1024, 0)
    with pytest.raises(ValueError, match="recording 0.*class"):
        events_to_chunks([[(7, 0, 100)]], [5000], 1024, 0, background_index=7)
    with pytest.raises(ValueError, match="recording 1.*class"):                        # outside 0 .. C - 1
        events_to_chunks([ok, [(5, 0, 100)]], [5000] * 2, 1024, 0, num_classes=5)
    assert events_to_chunks([[(5, 0, 100)]], [5000], 1024, 0) == [[(5, 0, 0)]]         # C not given
    with pytest.raises(ValueError, match="recording 0.*class"):
        events_to_chunks([[(-1, 0, 100)]], [5000], 1024, 0)
    with pytest.raises(ValueError, match="recording 1.*end"):                          # starts at the recording's end
        events_to_chunks([ok, [(1, 5000, 5100)]], [5000] * 2, 1024, 0)
    assert events_to_chunks([[(1, 4999, 5100)]], [5000], 1024, 0) == [[(1, 4, 4)]]
    with pytest.raises(ValueError, match="recording 0"):
        events_to_chunks([[(1, 100, 100)]], [5000], 1024, 0)                           # start < end
    with pytest.raises(ValueError):
        events_to_chunks([ok], [5000, 5000], 1024, 0)


def _result(hits, fas, n_events, sens=(0.3, 0.6), levels=(1, 2)):
    from kws_amd.stream import SweepResult
    hits, fas = np.asarray(hits, np.int32), np.asarray(fas, np.int32)
    z = np.zeros_like(hits)
    return SweepResult(hits + fas, hits, fas, z, z, n_events, sens, levels)


def test_det_arithmetic_and_nan():
    # two recordings, S = L = 2
    res = _result([[[1, 2], [0, 1]], [[2, 2], [1, 0]]], [[[3, 0], [1, 0]], [[1, 1], [0, 0]]], [2, 2])
    miss, fa = res.det([1800.0, 5400.0])
    np.testing.assert_array_equal(miss, np.array([[0.25, 0.0], [0.75, 0.75]]))
    np.testing.assert_array_equal(fa, np.array([[4.0, 1.0], [1.0, 0.0]]) * 3600.0 / 7200.0)
    assert miss.dtype == np.float64 and fa.dtype == np.float64 and miss.shape == (2, 2)
    miss, fa = _result([[[0, 0], [0, 0]]], [[[1, 0], [0, 0]]], [0]).det([10.0])       # no events: miss rate undefined
    assert np.isnan(miss).all() and fa[0, 0] == 360.0
    miss, fa = _result([[[1, 0], [0, 0]]], [[[1, 0], [0, 0]]], [1]).det([0.0])        # no audio: false-alarm rate undefined
    assert np.isnan(fa).all() and miss[0, 0] == 0.0
    with pytest.raises(ValueError):
        res.det()
    assert res.sensitivities == [0.3, 0.6] and res.trigger_levels == [1, 2] and res.n_events == [2, 2]


def test_best_tie_breaks_and_none():
    hour = [3600.0]
    # lowest miss rate within the budget: (0, 0) has the lowest miss rate but 5 FA/h
    res = _result([[[4, 3], [2, 1]]], [[[5, 1], [0, 0]]], [4])
    b = res.best(hour, 2.0)
    assert (b["s"], b["l"], b["sensitivity"], b["trigger_level"], b["miss_rate"], b["fa_per_hour"]) == (0, 1, 0.3, 2, 0.25, 1.0)
    assert res.best(hour, 5.0)["s"] == 0 and res.best(hour, 5.0)["l"] == 0
    # tie on the miss rate -> the lower fa_per_hour
    b = _result([[[3, 3], [2, 1]]], [[[2, 1], [0, 0]]], [4]).best(hour, 2.0)
    assert (b["s"], b["l"]) == (0, 1)
    # tie on miss rate and fa_per_hour -> the higher sensitivity
    b = _result([[[3, 1], [3, 1]]], [[[1, 0], [1, 0]]], [4]).best(hour, 2.0)
    assert (b["s"], b["l"], b["sensitivity"]) == (1, 0, 0.6)
    # ... and then the lower trigger level
    b = _result([[[1, 1], [3, 3]]], [[[0, 0], [1, 1]]], [4]).best(hour, 2.0)
    assert (b["s"], b["l"], b["trigger_level"]) == (1, 0, 1)
    assert _result([[[3, 3], [2, 1]]], [[[2, 1], [3, 4]]], [4]).best(hour, 0.5) is None
    assert _result([[[1, 0], [0, 0]]], [[[0, 0], [0, 0]]], [1]).best([0.0], 100.0) is None      # NaN qualifies for nothing
    b = _result([[[0, 0], [0, 0]]], [[[2, 1], [1, 3]]], [0]).best(hour, 2.0)                    # no events: the tie-breaks alone
    assert (b["s"], b["l"]) == (1, 0) and math.isnan(b["miss_rate"])


def test_sensitivities_and_trigger_levels_parsing():
    import listen
    assert listen.parse_sensitivities("0.2,0.5, 0.75") == [0.2, 0.5, 0.75]
    assert listen.parse_sensitivities("0.5") == [0.5]
    got = listen.parse_sensitivities("0.1:0.9:17")
    assert len(got) == 17 and got[0] == 0.1 and got[-1] == 0.9 and got[8] == pytest.approx(0.5, abs=1e-15)
    assert all(b > a for a, b in zip(got, got[1:]))
    assert listen.parse_sensitivities("0.25:0.75:3") == [0.25, 0.5, 0.75]
    assert listen.parse_sensitivities("0.4:0.4:1") == [0.4]
    for bad in ("", "0.1:0.9", "0.1:0.9:0", "0.1:0.9:1", "a,b"):
        with pytest.raises(ValueError):
            listen.parse_sensitivities(bad)
    assert listen.parse_trigger_levels("1,2,3,4,5") == [1, 2, 3, 4, 5]
    for bad in ("", "1,-2", "1.5"):
        with pytest.raises(ValueError):
            listen.parse_trigger_levels(bad)


def test_labels_file_parsing(tmp_path):
    import listen
    names = ["background", "up", "down"]
    f = tmp_path / "labels.txt"
    f.write_text("# wav class start end\n"
                 "a.wav up 0.5 1.0\n"
                 "\n"
                 "sub/dir/b.wav down 0 0.25   # a trailing comment\n"
                 "a.wav down 2.5 2.9\n")
    got = listen.parse_labels(str(f), names, 16000)
    assert got == {"a.wav": [(1, 8000, 16000), (2, 40000, 46400)], "b.wav": [(2, 0, 4000)]}
    assert got.get("c.wav", []) == []                                   # a wav the file does not mention is a negative recording
    f.write_text("a.wav sideways 0.5 1.0\n")
    with pytest.raises(ValueError, match="sideways"):
        listen.parse_labels(str(f), names, 16000)
    f.write_text("a.wav up 0.5\n")
    with pytest.raises(ValueError, match=":1"):
        listen.parse_labels(str(f), names, 16000)
    f.write_text("a.wav up 1.0 0.5\n")
    with pytest.raises(ValueError):
        listen.parse_labels(str(f), names, 16000)


def test_listen_py_lists_the_sweep_options():
    import listen
    assert not any(k.startswith("sweep") or k in ("labels_path", "sensitivities", "trigger_levels") for k in listen.default_config)
    assert callable(listen.Listener.sweep_wav)


def test_sweep_entry_point_argument_errors():
    from kws_amd import lib as l
    L = l.get_lib()
    assert L.kws_stream_sweep.argtypes and len(L.kws_stream_sweep.argtypes) == 16

    def call(R=2, stride=8, chunk=1024, P=3, ptr=None):
        return L.kws_stream_sweep(ptr, ptr, R, stride, ptr, 0, chunk, ptr, ptr, P, None, None, None, None, ptr, None)

    assert call(R=0) == 0 and call(P=0) == 0                                            # nothing to do, nothing dereferenced
    assert call(P=-1) == -1 and b"P=-1" in L.kws_last_error()
    assert call(chunk=0) == -1 and b"chunk_size=0" in L.kws_last_error()
    assert call(chunk=-1024) == -1 and b"chunk_size=-1024" in L.kws_last_error()
    assert call(R=-1) == -1 and b"R=-1" in L.kws_last_error()
    assert call() == -1 and b"null argument" in L.kws_last_error()
    with pytest.raises(l.KwsError):
        l.check(call())
    assert ctypes.sizeof(ctypes.c_int32) == 4


def test_sweep_needs_a_device():
    import torch
    from kws_amd.stream import sweep
    if torch.cuda.is_available():
        return
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sweep((None, None, []), [0.5], [3], 1024)


@pytest.mark.parametrize("chunk_size", sweep_cases.CHUNK_SIZES)
def test_synthetic_scan_exercises_every_counter(chunk_size):
    """On the reference alone: the planted runs give hits, false alarms, duplicates and misses, most points fire, points differ,
    the events in samples map back onto the chunk events, and walking into the poisoned padding would show as extra fires."""
    from kws_amd.stream import events_to_chunks
    index, score = sweep_cases.build()
    assert index.shape == (6, sweep_cases.STRIDE) and sweep_cases.STRIDE > max(sweep_cases.N_CHUNKS)
    assert set(np.unique(score).tolist()) == set(sweep_cases.SCORES)
    assert {0.3, 0.5, 0.7} <= set(sweep_cases.SENSITIVITIES)
    counts = sweep_ref.sweep(index, score, sweep_cases.N_CHUNKS, 0, sweep_cases.SENSITIVITIES, sweep_cases.TRIGGER_LEVELS, chunk_size,
                             sweep_cases.EVENTS)
    sweep_cases.check_reference(counts)
    assert -(8 * 2048) // chunk_size == {1024: -16, 3000: -6, 4096: -4}[chunk_size]
    lens = [n * chunk_size for n in sweep_cases.N_CHUNKS]
    assert events_to_chunks(sweep_cases.sample_events(chunk_size), lens, chunk_size, 0, 0, sweep_cases.NUM_CLASSES) == sweep_cases.EVENTS
    whole = sweep_ref.sweep(index, score, [sweep_cases.STRIDE] * 6, 0, sweep_cases.SENSITIVITIES, sweep_cases.TRIGGER_LEVELS, chunk_size)
    extra = (whole[..., 0] - counts[..., 0]).sum(axis=(1, 2))
    assert (extra > 0).all(), "a read past rec_chunks would go unnoticed in recording %s" % np.nonzero(extra == 0)[0]
