"""The cases and the deterministic data of the query-by-example tests (tests/test_dtw_host.py, tests/test_dtw_gpu.py)."""
import numpy as np

import dtw_ref as dr

# ---- exact cases: integer rows in -3..3, squared distance: every cost is an integer below 2^24 and ties are frequent ----------------
LENGTHS = (1, 2, 3, 31, 32, 33, 63, 64)          # template rows: the ends, the lane pairs around the half wave, the last lanes
WIDTHS = (4, 20, 64)                             # the narrowest, the MFCC default, the widest (kernels of 1, 5 and 16 column groups)
MID_WIDTHS = (12, 32)                            # the kernels of 3 and 8 column groups, and a width below its kernel's (28 in 32)
MAX_FRAMES = 704


def unreachable(L):
    """the first ceil((L - 1) / 2) frames cannot end a match"""
    return L // 2


def frame_counts(L):
    """the recordings a template of L rows meets: nothing, the fewest frames, all +inf, exactly one finite frame, the chunk of 64
    columns and its neighbours, two chunks and their neighbours, and many chunks with a ragged tail"""
    return sorted({0, 1, 2, unreachable(L), unreachable(L) + 1, 64, 65, 127, 128, 129, 700})


ALL_COUNTS = sorted({n for L in LENGTHS for n in frame_counts(L)})


def int_rows(seed, *shape):
    return np.random.default_rng(seed).integers(-3, 4, size=shape).astype(np.float32)


def exact_data(D):
    """-> templates (8, 64, D), lengths (8), rows (R, MAX_FRAMES, D), n_frames (R): every length against every frame count"""
    lengths = np.array(LENGTHS, np.int32)
    templates = int_rows(100 + D, len(LENGTHS), 64, D)
    for k, L in enumerate(LENGTHS):
        templates[k, L:] = 7.0                   # rows past a template's length must not be read as part of it
    n_frames = np.array(ALL_COUNTS, np.int32)
    rows = int_rows(200 + D, len(ALL_COUNTS), MAX_FRAMES, D)
    for r, n in enumerate(ALL_COUNTS):
        rows[r, n:] = 5.0                        # nor frames past a recording's length
    return templates, lengths, rows, n_frames


_expected = {}


def expected(key, templates, lengths, rows, n_frames, metric, dtype=np.float32):
    """the reference's (cost, start), computed once per key and shared"""
    if key not in _expected:
        cost, start = dr.dtw_many(templates, lengths, rows, n_frames, metric, dtype)
        cost.setflags(write=False)
        start.setflags(write=False)
        _expected[key] = (cost, start)
    return _expected[key]


# ---- tiling ---------------------------------------------------------------------------------------------------------------------------
TILE_N = 700
TILE_LENGTHS = (1, 2, 17, 64)
TILES = (0, 32, 64, 97, TILE_N)


def tile_data():
    lengths = np.array(TILE_LENGTHS, np.int32)
    return int_rows(31, len(TILE_LENGTHS), 64, 20), lengths, int_rows(32, 1, TILE_N, 20), np.array([TILE_N], np.int32)


# ---- one ragged call ----------------------------------------------------------------------------------------------------------------
RAGGED_FRAMES = (0, 1, 40, 333, 700)
RAGGED_LENGTHS = (1, 7, 40, 64)


def ragged_data():
    lengths = np.array(RAGGED_LENGTHS, np.int32)
    return (int_rows(41, len(RAGGED_LENGTHS), 64, 20), lengths, int_rows(42, len(RAGGED_FRAMES), MAX_FRAMES, 20),
            np.array(RAGGED_FRAMES, np.int32))


# ---- real-valued cosine -------------------------------------------------------------------------------------------------------------
COSINE_LENGTHS = (1, 17, 64)
COSINE_N, COSINE_D = 300, 20


def cosine_data():
    rng = np.random.default_rng(51)

    def unit(*shape):
        v = rng.standard_normal(shape)
        return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)
    return unit(len(COSINE_LENGTHS), 64, COSINE_D), np.array(COSINE_LENGTHS, np.int32), unit(2, COSINE_N, COSINE_D), np.array([COSINE_N, 211], np.int32)


def cosine_bound(L, D=COSINE_D):
    """D roundings of the dot product, one of 1 - dot, L accumulations of partial sums <= 2 L, divided by L"""
    return (D + 2 * L + 4) * 2.0 ** -24


# ---- peaks on integer curves --------------------------------------------------------------------------------------------------------
def peak_data(R=3, Q=5, F=200, seed=61):
    """cost (R, Q, F) of few distinct integers (ties between frames and between templates), +inf stretches, a recording of +inf only;
    start: any integers"""
    rng = np.random.default_rng(seed)
    cost = rng.integers(0, 6, size=(R, Q, F)).astype(np.float32)
    cost[:, :, :9] = np.inf
    cost[rng.random((R, Q, F)) < 0.1] = np.inf
    cost[R - 1] = np.inf
    start = rng.integers(0, F, size=(R, Q, F)).astype(np.int32)
    return cost, start


#            name              group            threshold  min_gap  K
PEAK_CASES = (("ties",          (0, 0, 0, 1, 2),  3.0,       5,       8),
              ("k_reached",     (0, 0, 0, 1, 2),  np.inf,    1,       4),
              ("gap_1",         (0, 0, 0, 1, 2),  0.0,       1,       64),
              ("gap_past_n",    (0, 0, 0, 1, 2),  np.inf,    1000,    8),
              ("nothing_below", (0, 0, 0, 1, 2),  -1.0,      5,       8),
              ("single_groups", (0, 1, 2, 3, 4),  1.0,       17,      16),
              ("one_group",     (0, 0, 0, 0, 0),  2.0,       3,       64))


# ---- end to end: two "words" of tone bursts planted in noise ----------------------------------------------------------------------------
RATE = 16000
WORDS = {"alpha": (1000, 350, 500, 2000, 1400, 600), "bravo": (2800, 2000, 2800, 700, 1000, 2400)}      # Hz at the glide's knots, inside the VAD's band
BURST_S = 0.13
SPEEDS = (0.8, 1.0, 1.25)
PLANTED_PER_PAIR = len(SPEEDS)


def word(name, speed=1.0):
    """float64 samples in [-0.5, 0.5]: a tone that glides from each of the word's frequencies to the next in BURST_S seconds (so every
    instant of the word sounds unlike its neighbours and an end is well defined), faded in and out, played at `speed` (so its tones
    shift with it)"""
    f = WORDS[name]
    n = int(BURST_S * RATE)
    freq = np.concatenate([np.linspace(a, b, n, endpoint=False) for a, b in zip(f[:-1], f[1:])])
    m = freq.size
    env = np.minimum(1.0, np.minimum(np.arange(m), m - 1 - np.arange(m)) / (0.01 * RATE))
    w = 0.5 * env * np.sin(2 * np.pi * np.cumsum(freq) / RATE)
    if speed == 1.0:
        return w
    k = int(w.size / speed)
    return np.interp(np.arange(k) * speed, np.arange(w.size), w)


def to_pcm(x):
    return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)


def example(name):
    """an enrolment clip: the unstretched word with 0.4 s of faint noise on both sides"""
    rng = np.random.default_rng(sum(map(ord, name)))
    pad = int(0.4 * RATE)
    x = 0.002 * rng.standard_normal(2 * pad + word(name).size)
    x[pad:pad + word(name).size] += word(name)
    return to_pcm(x)


def scene():
    """-> (recordings [int16], planted [(recording, keyword name, first sample, one-past-last sample)]): two recordings of about 20 s
    of noise at -34 dB re the words, with every word at every speed in each of them: PLANTED_PER_PAIR per (recording, word)"""
    rng = np.random.default_rng(71)
    plan = ((0, "alpha", 1.0, 1.5), (0, "bravo", 0.8, 4.1), (0, "alpha", 1.25, 7.3), (0, "bravo", 1.0, 10.2), (0, "alpha", 0.8, 13.0),
            (0, "bravo", 1.25, 16.5), (1, "bravo", 1.25, 1.2), (1, "alpha", 1.0, 4.0), (1, "bravo", 0.8, 7.0), (1, "alpha", 0.8, 10.2),
            (1, "bravo", 1.0, 13.5), (1, "alpha", 1.25, 16.6))
    recs = [0.01 * rng.standard_normal(int(20.0 * RATE)), 0.01 * rng.standard_normal(int(19.3 * RATE))]
    planted = []
    for r, name, speed, at in plan:
        w = word(name, speed)
        b = int(at * RATE)
        recs[r][b:b + w.size] += w
        planted.append((r, name, b, b + w.size))
    return [to_pcm(x) for x in recs], planted


def planted_end_frame(end_sample, window, hop):
    """the last frame whose window still lies inside the word"""
    return (end_sample - window) // hop


def clip_around(rec, b, e, n=RATE):
    """one second of the recording centred on the planted word"""
    mid = (b + e) // 2
    lo = min(max(0, mid - n // 2), rec.size - n)
    return rec[lo:lo + n]
