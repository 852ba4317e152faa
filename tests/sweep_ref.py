"""Pure-Python restatement of the operating-point sweep (kws_stream_sweep, kws_amd.stream.sweep): the reference of every
comparison in tests/test_sweep_host.py and tests/test_sweep_gpu.py.

The walk is oracle.stream_oracle.TriggerState.update, chunk by chunk from a fresh state per (recording, point); the event
bookkeeping is the contract of include/kws.h: events of a recording are (class, lo, hi) in chunk units, sorted, with
lo[e] <= hi[e] < lo[e + 1]; a fire at chunk k of class c moves the cursor past every event with hi < k; if the event under the
cursor has lo <= k and class c, the first such fire is a hit (latency k - lo) and later ones are duplicates; every other fire
is a false alarm.  Everything is integer, and the detector compares the same doubles with the same strict `>` as the kernel,
so comparisons against this are exact."""
import numpy as np

from oracle.stream_oracle import TriggerState

FIRES, HITS, FALSE_ALARMS, DUPLICATES, LATENCY = range(5)


def walk(index, score, n_chunks, background_index, sensitivity, trigger_level, chunk_size, events=None):
    """One recording at one operating point -> [fires, hits, false_alarms, duplicates, latency_chunks_sum].  Only the first
    n_chunks entries of index / score are read; events=None counts fires alone."""
    st = TriggerState()
    out = [0, 0, 0, 0, 0]
    e, found = 0, False
    for k in range(int(n_chunks)):
        idx, sc = int(index[k]), float(score[k])
        if not st.update(idx, sc, idx == background_index, float(sensitivity), int(trigger_level), int(chunk_size)):
            continue
        out[FIRES] += 1
        if events is None:
            continue
        while e < len(events) and events[e][2] < k:
            e += 1
            found = False
        if e < len(events) and events[e][1] <= k and events[e][0] == idx:
            if found:
                out[DUPLICATES] += 1
            else:
                found = True
                out[HITS] += 1
                out[LATENCY] += k - events[e][1]
        else:
            out[FALSE_ALARMS] += 1
    return out


def sweep(index, score, n_chunks, background_index, sensitivities, trigger_levels, chunk_size, events=None):
    """(R, S, L, 5) int64: `walk` of every recording at every point of the grid; events: per recording a list of (class, lo, hi)"""
    index, score = np.asarray(index), np.asarray(score)
    out = np.zeros((len(n_chunks), len(sensitivities), len(trigger_levels), 5), np.int64)
    for r, n in enumerate(n_chunks):
        for s, sens in enumerate(sensitivities):
            for l, level in enumerate(trigger_levels):
                out[r, s, l] = walk(index[r], score[r], n, background_index, sens, level, chunk_size, None if events is None else events[r])
    return out
