"""CPU tests of ragged streaming's host half (kws_amd.stream.RaggedPlan, the kws_stream_ragged_* argument checks).

The carry bookkeeping is compared with a brute-force replay of the reference's Listener.update_vectors (listen.py:96-109)
that carries sample POSITIONS instead of samples: window_audio becomes the list of positions it holds, a frame is the
position of its first sample, and no featurizer is needed."""
import ctypes

import numpy as np
import pytest

# (window, hop, chunk_size): the five geometries of the contract in include/kws.h, and chunk_size 1 under a 1024-sample window
GEOMETRIES = [(1024, 512, 1024), (400, 160, 800), (256, 512, 300), (1000, 1000, 1024), (1024, 512, 4096), (1024, 512, 1)]


class PositionListener(object):
    """listen.py:96-109 on positions; vectorize_raw gives (n - W) // H + 1 frames of n >= W samples, frame j from j * H"""

    def __init__(self, W, H):
        self.W, self.H = W, H
        self.window_audio = np.zeros(0, np.int64)
        self.arrived = 0

    def update_vectors(self, n):
        chunk = np.arange(self.arrived, self.arrived + n)
        self.arrived += n
        self.window_audio = np.concatenate((self.window_audio, chunk))
        starts = []
        if len(self.window_audio) >= self.W:
            n_frames = (len(self.window_audio) - self.W) // self.H + 1
            starts = [int(self.window_audio[j * self.H]) for j in range(n_frames)]
            self.window_audio = self.window_audio[n_frames * self.H:]
        return starts


@pytest.mark.parametrize("W,H,chunk", GEOMETRIES)
def test_ragged_plan_matches_the_reference_loop(W, H, chunk):
    from kws_amd.stream import RaggedPlan
    S, T = 3, (1030 if chunk == 1 else 400)                           # chunk_size 1: far enough to pass sample 1024
    plan = RaggedPlan(S, chunk, W, H)
    assert plan.cap == W + chunk
    slots = [plan.open() for _ in range(S)]
    assert slots == [0, 1, 2]
    ref = [PositionListener(W, H) for _ in range(S)]
    rng = np.random.default_rng(W + H + chunk)
    first_row_at = {}
    for t in range(T):
        active = [int(s) for s in rng.permutation(S) if chunk == 1 or rng.random() < 0.7] or [int(rng.integers(S))]
        lens = rng.integers(1, chunk + 1, len(active))
        if t % 7 == 0:
            lens[:] = chunk                                           # full chunks too: the carry's upper end
        step = plan.push(active, lens)
        assert step.A == len(active) and step.table.shape == (len(active), 8) and step.table.dtype == np.int32
        for a, s in enumerate(active):
            before = len(ref[s].window_audio)
            starts = ref[s].update_vectors(int(lens[a]))
            assert int(step.n_new[a]) == len(starts)
            assert step.frame_starts(a) == starts
            assert int(step.carry[a]) == len(ref[s].window_audio) == int(plan.carry[s])
            assert list(step.table[a, :5]) == [s, before, lens[a], len(starts), 1 if ref[s].arrived == lens[a] else 0]
            assert before + lens[a] <= plan.cap and plan.carry[s] <= plan.cap
            assert plan.carry[s] <= W - 1
            if starts:
                first_row_at.setdefault(s, (t, ref[s].arrived))
        assert step.max_frames == max(int(v) for v in step.n_new)
    assert sorted(first_row_at) == [0, 1, 2]
    if chunk == 1:
        assert all(v == (W - 1, W) for v in first_row_at.values())    # n_new stays 0 until sample 1024 arrives
    else:
        assert all(arrived >= W for _, arrived in first_row_at.values())


def _plan(S=4, chunk=1024):
    from kws_amd.stream import RaggedPlan
    plan = RaggedPlan(S, chunk, 1024, 512)
    return plan, [plan.open() for _ in range(S - 1)]                   # the last slot stays closed


def _chunk(n, dtype=np.int16):
    return np.zeros(n, dtype)


@pytest.mark.parametrize("slots,sizes,word", [
    ([0, 1, 0], [10, 10, 10], "duplicate"),
    ([0, 3], [10, 10], "closed"),
    ([0, 4], [10, 10], "out of range"),
    ([-1], [10], "out of range"),
    ([1, 2], [10, 0], "empty"),
    ([1, 2], [1025, 10], "exceeds chunk_size"),
])
def test_push_arguments_are_refused_by_name(slots, sizes, word):
    plan, _ = _plan()
    before = (plan.carry.copy(), plan.reset.copy(), plan.is_open.copy())
    rows, lens = plan.chunks(slots, [_chunk(n) for n in sizes])
    with pytest.raises(ValueError, match=word):
        plan.push(slots, lens)
    for a, b in zip(before, (plan.carry, plan.reset, plan.is_open)):
        np.testing.assert_array_equal(a, b)                           # a refused push changes nothing


def test_audio_that_is_not_int16_is_refused():
    plan, _ = _plan()
    with pytest.raises(ValueError, match="int16"):
        plan.chunks([0, 1], [_chunk(10, np.float32), _chunk(10, np.float32)])
    with pytest.raises(ValueError, match="int16"):
        plan.chunks([0, 1], np.zeros((2, 10), np.float32))
    with pytest.raises(ValueError, match="shape"):
        plan.chunks([0, 1], np.zeros((3, 10), np.int16))
    with pytest.raises(ValueError, match="exceeds"):
        plan.chunks([0, 1], np.zeros((2, 10), np.int16), lengths=[4, 11])
    rows, lens = plan.chunks([0, 1], [b"\x01\x00\x02\x00", _chunk(7)])           # bytes as PyAudio delivers them
    assert list(lens) == [2, 7] and list(rows[0]) == [1, 2]
    rows, lens = plan.chunks([0, 1], np.zeros((2, 10), np.int16), lengths=[4, 10])
    assert list(lens) == [4, 10]


def test_deltas_are_refused_before_any_device_use():
    from classifier.params import ListenerParams, pr
    from kws_amd.stream import StreamServer
    d = dict((k, getattr(pr, k)) for k in ("buffer_t", "window_t", "hop_t", "sample_rate", "sample_depth", "n_fft", "n_filt", "n_mfcc",
                                            "threshold_config", "threshold_center"))
    with pytest.raises(ValueError, match="use_delta=True is not usable in the reference"):
        StreamServer(ListenerParams(use_delta=True, **d), None, 2)


def test_open_close_and_the_marked_reset():
    plan, slots = _plan()
    assert slots == [0, 1, 2] and plan.open(sensitivity=0.8, trigger_level=5) == 3
    assert plan.sensitivity[3] == 0.8 and plan.trigger_level[3] == 5 and plan.sensitivity[0] == 0.5 and plan.trigger_level[0] == 3
    with pytest.raises(RuntimeError, match="full"):
        plan.open()
    step = plan.push([1, 3], [700, 600])
    assert list(step.table[:, 4]) == [1, 1] and not plan.reset[1] and list(plan.carry[[1, 3]]) == [700, 600]
    step = plan.push([1], [700])                                      # 1400 samples: one row, 1400 - 512 stay
    assert list(step.table[0, :5]) == [1, 700, 700, 1, 0] and plan.carry[1] == 888
    plan.close(1)
    with pytest.raises(ValueError, match="closed"):
        plan.close(1)
    with pytest.raises(ValueError, match="closed"):
        plan.push([1], [10])
    assert plan.open() == 1                                           # the freed slot, lowest first
    assert plan.reset[1] and plan.carry[1] == 0 and plan.sensitivity[1] == 0.5
    step = plan.push([1], [100])
    assert list(step.table[0, :5]) == [1, 0, 100, 0, 1] and step.frame_starts(0) == [] and not plan.reset[1]
    empty = plan.push([], [])
    assert empty.A == 0 and empty.max_frames == 0


def test_c_entry_points_check_their_arguments_on_the_host():
    """KWS_ERR_INVALID with a message before any device work: the calls carry no valid device pointer at all"""
    from kws_amd import lib as l
    L = l.get_lib()
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.addressof(buf)
    p += -p % 16
    W, H, c, S = 1024, 512, 1024, 4
    cap = stride = W + c

    def append(A=1, cap=cap, win=p, chunks=p, table=p, act=p, act_len=p, win_stride=stride):
        return L.kws_stream_ragged_append(win, win_stride, S, cap, chunks, c, table, A, c, W, H, act, stride, act_len, None)

    def rows(A=1, mfccs=p, table=p, feat=p, F=30):
        return L.kws_stream_ragged_push_rows(mfccs, S, F, 20, p, 3, table, A, feat, None)

    def post(A=1, probs=p, table=p, sens=p, state=p, C=5):
        return L.kws_stream_ragged_postprocess(None, probs, A, C, table, S, 0, sens, p, c, state, p, p, p, p, p, p, None)

    cases = [(lambda: append(A=-1), b"A=-1"), (lambda: append(A=S + 1), b"A=5"), (lambda: append(cap=cap - 1, win_stride=stride), b"cap=2047"),
             (lambda: append(win=None), b"null"), (lambda: append(chunks=None), b"null"), (lambda: append(table=None), b"null"),
             (lambda: append(act=None), b"null"), (lambda: append(act_len=None), b"null"), (lambda: append(win_stride=stride + 4), b"multiple of 8"),
             (lambda: append(win=p + 2), b"16 bytes"),
             (lambda: rows(A=-1), b"A=-1"), (lambda: rows(mfccs=None), b"null"), (lambda: rows(table=None), b"null"),
             (lambda: rows(feat=None), b"null"), (lambda: rows(F=0), b"F=0"),
             (lambda: post(A=-1), b"A=-1"), (lambda: post(probs=None), b"null"), (lambda: post(table=None), b"null"),
             (lambda: post(sens=None), b"null"), (lambda: post(state=None), b"null"), (lambda: post(C=0), b"C=0")]
    for call, word in cases:
        assert call() == l.ERR_INVALID
        assert word in L.kws_last_error(), (word, L.kws_last_error())
    # an empty push does nothing, whatever the pointers
    assert append(A=0, win=None, chunks=None, table=None, act=None, act_len=None) == 0
    assert rows(A=0, mfccs=None, table=None, feat=None) == 0 and post(A=0, probs=None, table=None, sens=None, state=None) == 0
    assert L.kws_stream_ragged_append(p, 40000, S, 40000, p, c, p, 1, c, W, H, p, 40000, p, None) == l.ERR_UNSUPPORTED


def test_the_ragged_entry_points_are_declared_and_exported():
    import os
    import re
    from kws_amd import lib as l
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "kws.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(kws_stream_ragged_[a-z0-9_]+)\s*\(", text)))
    assert names == ["kws_stream_ragged_append", "kws_stream_ragged_postprocess", "kws_stream_ragged_push_rows"]
    for n in names:
        assert hasattr(l.get_lib(), n)
    assert (l.RAGGED_SLOT, l.RAGGED_CARRY, l.RAGGED_LEN, l.RAGGED_NEW, l.RAGGED_RESET, l.RAGGED_FIELDS) == tuple(
        int(re.search(r"KWS_RAGGED_%s = (\d+)" % k, text).group(1)) for k in ("SLOT", "CARRY", "LEN", "NEW", "RESET", "FIELDS"))
