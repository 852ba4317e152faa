"""Pure-Python restatement of the harvest of a scan (kws_stream_collect, kws_stream_peaks, kws_amd.stream.Detections): the
reference of every comparison in tests/test_mine_host.py and tests/test_mine_gpu.py.

`detections` is tests/sweep_ref.walk that keeps every fire instead of counting it: the walk is
oracle.stream_oracle.TriggerState.update from a fresh state, the event bookkeeping the contract of include/kws.h.  `peaks`
is the greedy pick written out as a loop over all chunks.  `audio_buffer` is the listener's buffer of the reference
(listen.py:90,100) after a chunk, in float64, and `saved_samples` what its save_audio makes of it.  Everything is integer
arithmetic or a comparison of stored doubles, so comparisons against this are exact."""
import numpy as np

from oracle.stream_oracle import TriggerState

UNLABELLED, HIT, DUPLICATE, FALSE_ALARM = range(4)


def detections(index, score, n_chunks, background_index, sensitivity, trigger_level, chunk_size, events=None):
    """One recording at one operating point -> [(chunk, class, kind, event, score), ...] in chunk order.  Only the first
    n_chunks entries are read; events: [(class, lo, hi), ...] in chunk units, sorted, or None (kind UNLABELLED, event -1)."""
    st = TriggerState()
    out = []
    e, found = 0, False
    for k in range(int(n_chunks)):
        idx, sc = int(index[k]), float(score[k])
        if not st.update(idx, sc, idx == background_index, float(sensitivity), int(trigger_level), int(chunk_size)):
            continue
        kind, event = UNLABELLED, -1
        if events is not None:
            while e < len(events) and events[e][2] < k:
                e += 1
                found = False
            if e < len(events) and events[e][1] <= k and events[e][0] == idx:
                kind, event = (DUPLICATE if found else HIT), e
                found = True
            else:
                kind = FALSE_ALARM
        out.append((k, idx, kind, event, sc))
    return out


def peaks(index, score, n_chunks, background_index, min_score, min_gap, K, events=None):
    """One recording -> [(chunk, class, score), ...] in pick order: at most K times the candidate (not background, score >
    min_score, in no event window) with the largest score, ties to the lowest chunk, at least min_gap from every pick."""
    cand = []
    for k in range(int(n_chunks)):
        if int(index[k]) == background_index or not float(score[k]) > min_score:
            continue
        if events is not None and any(lo <= k <= hi for _, lo, hi in events):
            continue
        cand.append(k)
    picked = []
    while len(picked) < K:
        best = None
        for k in cand:
            if any(abs(k - p) < min_gap for p in picked):
                continue
            if best is None or float(score[k]) > float(score[best]):         # ascending k: a tie keeps the lower chunk
                best = k
        if best is None:
            break
        picked.append(best)
    return [(k, int(index[k]), float(score[k])) for k in picked]


def audio_buffer(pcm, k, chunk_size, B):
    """float64 (B,): the reference listener's audio_buffer right after chunk k (0-based) of the int16 recording `pcm`: B zeros
    (listen.py:90) shifted left by every chunk's samples / 32768 (buffer_to_audio; listen.py:100), the last chunk short."""
    pcm = np.asarray(pcm)
    assert pcm.dtype == np.int16 and pcm.ndim == 1
    buf = np.zeros(B, dtype=np.float64)
    for j in range(k + 1):
        chunk = pcm[j * chunk_size:(j + 1) * chunk_size].astype(np.float64) / 32768.0
        assert chunk.size > 0, "chunk %d lies past the recording" % j
        buf = np.concatenate((buf[chunk.size:], chunk))[-B:]
    return buf


def saved_samples(buf):
    """save_audio of the reference (common/data_utils.py:46): the float64 product truncated toward zero"""
    return (np.asarray(buf, dtype=np.float64) * 32767).astype(np.int16)


TIE_N_CHUNKS = [64, 257, 1000]
TIE_STRIDE = 1008


def tie_case():
    """-> index (3, TIE_STRIDE) int32, score (3, TIE_STRIDE) float64: seeded filler of 5 classes (background 0 included) with
    scores from five values, so every 64-chunk stride holds equal scores and the lowest-chunk rule decides; the padding is
    class 3 at score 2.0, above every real score: read, it would be picked first."""
    rng = np.random.default_rng(23)
    index = np.full((len(TIE_N_CHUNKS), TIE_STRIDE), 3, np.int32)
    score = np.full((len(TIE_N_CHUNKS), TIE_STRIDE), 2.0, np.float64)
    for r, n in enumerate(TIE_N_CHUNKS):
        index[r, :n] = rng.integers(0, 5, n)
        score[r, :n] = rng.choice([0.1, 0.35, 0.6, 0.85, 0.95], n)
    return index, score
