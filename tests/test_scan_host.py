"""CPU tests of the offline scan's bookkeeping: the closed form `kws_amd.stream.scan_plan` (chunks, samples, rows and window
position per chunk) against oracle/stream_oracle.StreamState driven chunk by chunk, which restates Listener.update_vectors
(listen.py:96-114); the C surface of the scan; and that `scan` does not run without a device."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1024, 512


def _lengths(chunk):
    """lengths that end on / one short of / one past a chunk boundary and a frame boundary, and N < W"""
    out = {1, 2, W - 1, W, W + 1, chunk - 1, chunk, chunk + 1}
    for m in (2, 7, 23):
        out.update((m * chunk - 1, m * chunk, m * chunk + 1))
    for j in (1, 6, 41):
        out.update((W + j * H - 1, W + j * H, W + j * H + 1))
    return sorted(n for n in out if n > 0)


def _drive_oracle(N, chunk, F):
    """StreamState over a recording whose sample i has the value i + 1, with a framing function that returns each frame's
    first sample: row j of the matrix then reads j * H + 1, and a zero row reads 0."""
    from oracle import stream_oracle as so

    def frame_starts(audio):
        n = (len(audio) - W) // H + 1
        return np.array([[audio[j * H]] for j in range(n)], dtype=np.float64).reshape(n, 1)

    st = so.StreamState(F, 1, W, H, frame_starts)
    audio = np.arange(1, N + 1, dtype=np.float64)
    mats, carries = [], []
    for a in range(0, N, chunk):
        mats.append(st.push(audio[a:a + chunk]).copy())
        carries.append(st.window_audio.copy())
    return mats, carries


@pytest.mark.parametrize("F", [30, 5])
@pytest.mark.parametrize("chunk", [1024, 800, 160, 4000])
def test_scan_plan_is_the_chunk_loop(chunk, F):
    from kws_amd.stream import scan_plan
    for N in _lengths(chunk):
        T, n, r, first = scan_plan(N, chunk, W, H, F)
        mats, carries = _drive_oracle(N, chunk, F)
        assert T == len(mats) == -(-N // chunk), (N, chunk)
        assert n[-1] == N and all(b - a == chunk for a, b in zip(n[:-2], n[1:-1]))
        for k in range(T):
            want = np.array([(j * H + 1 if j >= 0 else 0) for j in range(first[k], r[k])], dtype=np.float64).reshape(F, 1)
            np.testing.assert_array_equal(mats[k], want, err_msg="N=%d chunk=%d chunk %d" % (N, chunk, k + 1))
            # the carry buffer starts on a frame boundary: at row r_k's first sample once a row exists, at sample 0 before
            assert len(carries[k]) == n[k] - r[k] * H
            if len(carries[k]):
                assert carries[k][0] == r[k] * H + 1
    if chunk == 160:
        _, _, r, _ = scan_plan(20 * 160, 160, W, H, F)
        assert any(a == b for a, b in zip(r[7:], r[8:]))         # chunks that bring no new row
    if chunk == 4000:
        _, _, r, _ = scan_plan(5 * 4000, 4000, W, H, F)
        assert min(b - a for a, b in zip(r, r[1:])) >= 7         # several rows per chunk (more than F = 5 of them)


def test_scan_plan_short_and_empty_recordings():
    from kws_amd.stream import scan_plan
    assert scan_plan(0, 1024, W, H, 30) == (0, [], [], [])
    assert scan_plan(700, 1024, W, H, 30) == (1, [700], [0], [-30])           # predicted on, with the all-zero matrix
    assert scan_plan(1023, 160, W, H, 30)[2] == [0] * 7
    with pytest.raises(ValueError):
        scan_plan(10, 0, W, H, 30)


def test_scan_entry_points_are_declared_and_exported():
    from kws_amd import get_lib
    text = open(os.path.join(ROOT, "include", "kws.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = get_lib()
    for name in ("kws_featurize_long", "kws_stream_gather_windows", "kws_stream_scan_postprocess"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name + " is not declared in include/kws.h"
        assert hasattr(L, name), "libkws_hip.so does not export " + name
        assert getattr(L, name).argtypes, name + " has no ctypes signature in kws_amd/lib.py"


def test_scan_needs_a_device_and_refuses_deltas():
    import torch
    from classifier.params import ListenerParams, pr
    from kws_amd.stream import StreamBatch, scan
    rec = [np.zeros(2048, np.int16)]
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError) as e1:
            scan(pr, None, rec)
        with pytest.raises(RuntimeError) as e2:
            StreamBatch(pr, None, 1)
        assert str(e1.value) == str(e2.value) and "no CPU fallback" in str(e1.value)
        return
    d = dict((k, getattr(pr, k)) for k in ("buffer_t", "window_t", "hop_t", "sample_rate", "sample_depth", "n_fft", "n_filt", "n_mfcc",
                                            "threshold_config", "threshold_center"))
    with pytest.raises(ValueError):
        scan(ListenerParams(use_delta=True, **d), None, rec)
