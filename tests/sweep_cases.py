"""The synthetic scan that tests/test_sweep_gpu.py sweeps (and whose properties tests/test_sweep_host.py checks on the
reference alone): six recordings around the 64-chunk load boundary in rows of STRIDE entries whose padding is poisoned, planted
runs of one class inside and outside event windows, and scores from a grid that holds some swept sensitivities exactly."""
import numpy as np

BACKGROUND = 0
NUM_CLASSES = 5
N_CHUNKS = [0, 1, 63, 64, 65, 130]
STRIDE = 136                                   # > 130: the padding is index 3, score 1.0 -- read, it would fire as class 3
POISON_INDEX, POISON_SCORE = 3, 1.0
SCORES = [0.0, 0.3, 0.5, 0.7, 1.0]             # 0.3, 0.5 and 0.7 are swept sensitivities: `score > sensitivity` is strict
SENSITIVITIES = [0.05, 0.1, 0.2, 0.25, 0.3, 0.4, 0.5, 0.55, 0.6, 0.7, 0.75, 0.8, 0.9, 0.95]
TRIGGER_LEVELS = [1, 2, 3, 4, 6]               # 14 x 5 = 70 points: one full wave and a partial one
CHUNK_SIZES = [1024, 3000, 4096]               # refractory -16, -6 (-(16384 // -3000): floor division that is not exact), -4

# events per recording, chunk units (class, lo, hi), sorted, hi[e] < lo[e + 1]
EVENTS = [
    [],
    [],
    [(1, 3, 30)],                              # a long run of class 1 from chunk 3: one hit, then duplicates after the refractory period
    [(2, 38, 63)],                             # class 2 at score 0.5: a miss for sensitivities >= 0.5
    [],                                        # a negative recording: its run across the 64-chunk boundary gives false alarms only
    [(2, 5, 30), (3, 64, 80), (2, 85, 110), (4, 120, 129)],
]


def _fill(index, score, r, a, b, cls, sc):
    index[r, a:b] = cls
    score[r, a:b] = sc


def build():
    """-> index (R, STRIDE) int32, score (R, STRIDE) float64"""
    rng = np.random.default_rng(17)
    R = len(N_CHUNKS)
    index = np.full((R, STRIDE), POISON_INDEX, np.int32)
    score = np.full((R, STRIDE), POISON_SCORE, np.float64)
    for r, n in enumerate(N_CHUNKS):                                     # filler: random classes (background included) and grid scores
        index[r, :n] = rng.integers(0, NUM_CLASSES, n)
        score[r, :n] = rng.choice(SCORES, n)
    _fill(index, score, 1, 0, 1, 1, 1.0)
    _fill(index, score, 2, 3, 41, 1, 1.0)                                # inside the window until chunk 30, a false alarm after it
    _fill(index, score, 2, 45, 63, 3, 0.7)                               # outside every window, up to the recording's last chunk
    _fill(index, score, 3, 0, 12, 0, 1.0)                                # background never fires
    _fill(index, score, 3, 40, 64, 2, 0.5)
    _fill(index, score, 4, 50, 65, 3, 0.7)                               # crosses chunk 64, where the second load begins
    r = 5
    _fill(index, score, r, 0, 5, 0, 1.0)
    _fill(index, score, r, 5, 45, 2, 1.0)                                # hit, duplicates inside 5..30, false alarms after 30
    _fill(index, score, r, 50, 61, 1, 0.7)                               # outside every window
    _fill(index, score, r, 64, 76, 4, 0.5)                               # the wrong class inside the window of (3, 64, 80)
    _fill(index, score, r, 76, 79, 3, 1.0)                               # the right class, too short for trigger levels above 1
    _fill(index, score, r, 85, 89, 1, 0.5)                               # class change in the middle of a run: the count starts again
    _fill(index, score, r, 89, 101, 2, 0.5)
    _fill(index, score, r, 112, 130, 4, 0.3)                             # event (4, 120, 129): the run starts before the window opens
    return index, score


def sample_events(chunk_size):
    """EVENTS as (class, start_sample, end_sample) that events_to_chunks(..., tolerance_samples=0) maps back onto EVENTS"""
    return [[(c, lo * chunk_size, (hi + 1) * chunk_size) for c, lo, hi in evs] for evs in EVENTS]


def check_reference(counts):
    """The properties the sweep's tests need of the reference counts (R, S, L, 5), so that no comparison passes vacuously."""
    import sweep_ref as ref
    n_events = np.array([len(e) for e in EVENTS])
    assert counts[..., ref.HITS].sum() > 0 and counts[..., ref.FALSE_ALARMS].sum() > 0 and counts[..., ref.DUPLICATES].sum() > 0
    assert (counts[..., ref.HITS] < n_events[:, None, None]).any(), "no missed event anywhere on the grid"
    per_point = counts[..., ref.FIRES].sum(axis=0)
    assert (per_point > 0).sum() * 2 >= per_point.size, "fewer than half of the points fire"
    assert any(len(np.unique(counts[r, :, :, ref.FIRES])) > 1 for r in range(counts.shape[0])), "every point fires equally often"
    assert counts[..., ref.LATENCY].sum() > 0
    assert (counts[..., ref.FIRES] == counts[..., ref.HITS] + counts[..., ref.FALSE_ALARMS] + counts[..., ref.DUPLICATES]).all()
