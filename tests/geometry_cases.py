"""Case table of the frame-geometry tests (tests/test_geometry_host.py, tests/test_featurizer_geometry_gpu.py,
tests/test_stream_geometry_gpu.py).

The front end takes its frame geometry from ListenerParams at run time, and which kernel runs, how its frames are dealt to waves and
how the streaming stack walks a recording all follow from it.  The rest of the suite sits at the default (window 1024, hop 512, 30
frames, 20 bands, 20 coefficients) almost everywhere.  The rows below are geometries on both sides of every rule of that dispatch;
this module restates those rules on the host (no device, no library call), so that tests/test_geometry_host.py can hold every row
against the kernel and the job shape it claims, and the GPU tests can pick batch sizes from the device's compute-unit count.

Restated from tf-keras-speech-commands_amd/csrc/kws_featurize.hip and kws_featurize_tables.h (each rule is named at its restatement).  A tuned row
also needs the chunk table of the mel bank to come out at 12, 16 or 20 positions per lane (v3_applies); that depends on n_fft, the band
count, the sample rate and the bank alone, which the tuned rows share with the default geometry, where the tuned kernel is the one the
whole suite and the benchmark run."""
import collections

import numpy as np

from cnn_path_cases import MI355X_CUS, dims

SAMPLE_RATE = 16000
GEN1_WAVES = 5                      # kWaves, kws_featurize.hip
GEN_WAVES = 4                       # kGenWaves, kws_featurize.hip
MAX_LDS = 160 * 1024                # kMaxLdsBytes, kws_featurize.hip
MAX_CLIPS = 4096                    # no test batch is larger
LONG_TILE = 256                     # featurize_long_segments, kws_featurize.hip
OTHER_CUS = 304                     # a second compute-unit count the table must hold at (tests/test_geometry_host.py)
ATOL = 2e-4                         # tests/test_featurizer_gpu.py: clip features against the float64 oracle
ATOL_ROWS = 3e-4                    # tests/test_scan_gpu.py, tests/test_stream_gpu.py: raw and long rows
ATOL_I16_GENERIC = 1e-6             # tests/test_featurizer_gpu.py: test_other_fft_sizes_generic_kernel, int16 against float32 input
FWD_ATOL = 2e-4                     # tests/test_stream_gpu.py: the forward pass against the oracle model

Geometry = collections.namedtuple("Geometry", "name buffer_t window_t hop_t n_fft n_filt n_mfcc use_delta frames kernel why")
ROWS = (
    Geometry("tuned-2", 0.1, 0.064, 0.032, 1024, 20, 20, False, 2, "tuned", "fewer frames than a tail batch"),
    Geometry("tuned-14", 0.5, 0.064, 0.032, 1024, 20, 20, False, 14, "tuned", "14 % 3 = 2: a tail batch of two frames ends the clip"),
    Geometry("tuned-61", 2.0, 0.064, 0.032, 1024, 20, 20, False, 61, "tuned", "61 % 3 = 1: a tail batch of one frame ends the clip"),
    Geometry("tuned-45", 1.5, 0.064, 0.032, 1024, 20, 20, False, 45, "tuned", "control: divisible by 3"),
    Geometry("gen1-9", 0.2, 0.064, 0.016, 1024, 20, 20, False, 9, "gen1", "fpw 3, jpc 3: idle waves; hop 256, no half-frame reuse"),
    Geometry("gen1-48", 0.5, 0.025, 0.010, 1024, 40, 13, False, 48, "gen1", "tail_batch 1, window 400 < n_fft"),
    Geometry("gen1-48d", 0.5, 0.025, 0.010, 1024, 40, 13, True, 48, "gen1", "deltas: block = clip, wave < jpc"),
    Geometry("rad2-48", 0.5, 0.025, 0.010, 512, 26, 13, False, 48, "generic", "window 400 is no multiple of hop 160"),
    Geometry("rad2-31", 1.0, 0.016, 0.032, 256, 13, 13, False, 31, "generic", "hop 512 > window 256"),
)
ROW = {g.name: g for g in ROWS}
TUNED = tuple(g.name for g in ROWS if g.kernel == "tuned")
AUG_ROWS = ("tuned-14", "tuned-61")
LONG_ROWS = ("gen1-48", "rad2-48", "rad2-31")
STREAM_ROWS = ("tuned-14", "gen1-9", "gen1-48", "rad2-48", "rad2-31")


# ---- ListenerParams' derived sizes (classifier/params.py:40-65, derive() in kws_featurize_tables.h) -------------------------------
def window_samples(g):
    return int(SAMPLE_RATE * g.window_t + 0.5)


def hop_samples(g):
    return int(SAMPLE_RATE * g.hop_t + 0.5)


def max_samples(g):
    return int(g.buffer_t * SAMPLE_RATE)


def n_features(g):
    hop = hop_samples(g)
    buffer_samples = hop * (int(SAMPLE_RATE * g.buffer_t + 0.5) // hop)
    return 1 + (buffer_samples - window_samples(g)) // hop


def clip_frames(g):
    """kws_featurizer_create, kws_featurize.hip (clip_frames, kws_featurize_tables.h): it refuses params whose frame count differs from n_features"""
    return (max_samples(g) - window_samples(g)) // hop_samples(g) + 1


def raw_frames(g, n):
    """kws_featurize_raw_frames, kws_featurize.hip (chop_array)"""
    return 0 if n < window_samples(g) else (n - window_samples(g)) // hop_samples(g) + 1


def feature_size(g):
    return 2 * g.n_mfcc if g.use_delta else g.n_mfcc


def mel_points(g):
    """build_mel_bank, kws_featurize_tables.h: the FFT bins of the triangles' corners; the library refuses a grid that repeats a bin"""
    n_bins, n = g.n_fft // 2 + 1, g.n_filt + 2
    lo, hi = 1127.0 * np.log(1.0), 1127.0 * np.log(1.0 + SAMPLE_RATE / 700.0)
    step = (hi - lo) / (n - 1)
    mels = [hi if i == n - 1 else lo + i * step for i in range(n)]
    return [int(700.0 * (np.exp(m / 1127.0) - 1.0) * n_bins / SAMPLE_RATE) for m in mels]


def params(g):
    from classifier.params import ListenerParams
    return ListenerParams(g.buffer_t, g.window_t, g.hop_t, SAMPLE_RATE, 2, g.n_fft, g.n_filt, g.n_mfcc, g.use_delta, ((6, 4),), 0.2)


def oracle_kw(g):
    """keyword arguments of oracle.featurizer_oracle's functions"""
    return dict(buffer_t=g.buffer_t, window_t=g.window_t, hop_t=g.hop_t, n_fft=g.n_fft, n_filt=g.n_filt, n_mfcc=g.n_mfcc, use_delta=g.use_delta)


# ---- the dispatch rules of the clip featurizer, restated ---------------------------------------------------------------------------
def window_eff(g):
    """window_eff, build_feat_tables in kws_featurize_tables.h: np.fft.rfft(frames, n) crops or zero-pads"""
    return min(window_samples(g), g.n_fft)


def tail_batch(g):
    """tail_batch, build_feat_tables in kws_featurize_tables.h: frames whose band sums and DCT one wave evaluates together"""
    n_filt_pad = (g.n_filt + 3) & ~3
    return max(1, min(4, 64 // max(n_filt_pad, g.n_mfcc)))


def v3_applies(g, use_delta=None):
    """v3_applies, kws_featurize.hip (its chp3 condition: module docstring)"""
    delta = g.use_delta if use_delta is None else use_delta
    return g.n_fft == 1024 and hop_samples(g) == 512 and window_eff(g) == 1024 and not delta and g.n_filt == 20 and g.n_mfcc == 20


def kernel_of(g, use_delta=None):
    """launch_featurize, kws_featurize.hip"""
    if g.n_fft != 1024:
        return "generic"
    return "tuned" if v3_applies(g, use_delta) else "gen1"


def feat_job_shape(n_frames, tb, use_delta):
    """feat_job_shape, kws_featurize.hip -> (fpw, jpc): frames per wave job, jobs per clip of the first-generation kernel"""
    fpw = (n_frames + GEN1_WAVES - 1) // GEN1_WAVES
    if not use_delta:
        fpw = max(fpw, min(n_frames, tb))
    fpw = max(1, fpw)
    return fpw, max(1, (n_frames + fpw - 1) // fpw)


def gen1_grid(B, jpc, use_delta):
    """the grid of launch_featurize, kws_featurize.hip -> (blocks, waves without a job).  With deltas a block is a clip and its waves
    jpc..4 idle (the job index of featurize_fft1024_kernel, kws_featurize.hip); without, the last block's waves past B * jpc do."""
    if use_delta:
        return B, B * (GEN1_WAVES - jpc)
    grid = (B * jpc + GEN1_WAVES - 1) // GEN1_WAVES
    return grid, grid * GEN1_WAVES - B * jpc


def v3_waves(cus, shared=False):
    """launch_v3_any / launch_v3, kws_featurize.hip: waves = bpc * cus * WAVES, two blocks of 8 waves per compute unit alone,
    one of 12 (kV3Waves) beside a train step"""
    return (1 * 12 if shared else 2 * 8) * cus


def v3_job_shape(n_frames, B, cus, shared=False, tb=3):
    """the cost loop of launch_v3, kws_featurize.hip -> (fpw, jpc, rounds)"""
    waves = v3_waves(cus, shared)
    best = None
    for fpw in range(min(n_frames, max(1, tb)), n_frames + 1):
        jpc = (n_frames + fpw - 1) // fpw
        rounds = (B * jpc + waves - 1) // waves
        cost = rounds * (fpw + 1.25) + (0.5 if n_frames % fpw else 0.0)
        if best is None or cost < best[0] - 1e-9:
            best = (cost, fpw, jpc, rounds)
    return best[1:]


def long_tile(g, max_frames):
    """featurize_long_segments, kws_featurize.hip -> (tile, segments per recording)"""
    tile = LONG_TILE
    if g.n_fft != 1024:
        fixed = GEN_WAVES * g.n_fft * 8 + GEN_WAVES * 256
        tile = min(LONG_TILE, (MAX_LDS - fixed) // (4 * g.n_mfcc) - 4)
    tile = max(1, min(tile, max_frames))
    return tile, (max_frames + tile - 1) // tile


def long_uses_segments(g):
    """kws_featurize_long, kws_featurize.hip: the tuned kernel's own tiles, or segments through the clip kernels"""
    return not v3_applies(g, use_delta=False)


def cnn_accepts(g):
    """kws_model_create (csrc/kws_model.hip): simple_cnn needs a pixel left after its third pool"""
    d = dims(clip_frames(g), feature_size(g))
    return d["H4"] >= 1 and d["W4"] >= 1


def stream_model_kind(g):
    return "simple_cnn" if cnn_accepts(g) else "simple_gru"


# ---- batch sizes ----------------------------------------------------------------------------------------------------------
def tuned_batches(g, cus):
    """{role: B} for a tuned row, from the cost loop at the stand-alone wave count of `cus` compute units:
      one        B = 1;
      tail       the largest B <= MAX_CLIPS whose jobs still fit one round at fpw = tail_batch (min(n_frames, 3)) -- the cost loop then
                 keeps the smallest candidate;
      odd        the smallest B whose fpw is larger than a tail batch, smaller than the clip and no multiple of 3: the jobs exceed the
                 grid's waves, and a job ends in a partly filled tail batch that is not the clip's last (None where the frame count
                 leaves no such fpw);
      whole      the smallest B at which fpw = n_frames (one job per clip)."""
    nf, tb = g.frames, min(g.frames, 3)
    out = {"one": 1, "tail": None, "odd": None, "whole": None}
    for B in range(1, MAX_CLIPS + 1):
        fpw, jpc, rounds = v3_job_shape(nf, B, cus)
        if fpw == tb and rounds == 1 and B > 1:
            out["tail"] = B
        if out["odd"] is None and tb < fpw < nf and fpw % 3:
            out["odd"] = B
        if out["whole"] is None and fpw == nf and B > 1 and nf > tb:
            out["whole"] = B
    return out


def batches(g, cus):
    """the batch sizes of a row's featurizer cases, in ascending order without repeats"""
    if g.kernel == "tuned":
        bs = [b for b in tuned_batches(g, cus).values() if b is not None]
    elif g.name == "gen1-9":
        bs = [1, 4]                 # 3 and 12 jobs: two and three waves of the last block have none
    elif g.kernel == "gen1":
        bs = [1, 7]
    else:
        bs = [1, 5, cus + 3]        # more blocks than compute units
    return sorted(set(bs))


# ---- inputs ----------------------------------------------------------------------------------------------------------------
N_BASE = 12
STRIDE_EXTRA = 37                   # every max_samples of the table is even: the row stride max_samples + 37 is odd


def stride(g):
    return max_samples(g) + STRIDE_EXTRA


def base_lengths(g):
    """valid_len of the N_BASE base clips: 0, 1, an odd length, window - 1, window, max_samples, one above the stride (the library clamps
    it), then lengths that end on / just past a frame and odd ones"""
    W, H, M = window_samples(g), hop_samples(g), max_samples(g)
    lens = [0, 1, min(M, W + H + 1) | 1, W - 1, W, M, stride(g) + 5, M - 1, min(M, W + H), M // 2 + 1, M - H, stride(g)]
    assert len(lens) == N_BASE
    return np.array(lens, np.int32)


def base_clips(g, seed=0):
    """(N_BASE, stride) float32: noise at 0.1 of full scale rounded to int16 steps, as tests/test_featurizer_gpu.py draws it"""
    rng = np.random.default_rng(1000 + seed + sum(map(ord, g.name)))
    wav = np.clip(0.1 * rng.standard_normal((N_BASE, stride(g))), -1, 1 - 2.0 ** -15)
    return (np.round(wav * 32768) / 32768).astype(np.float32)


def batch_index(B):
    """which base clip clip b of a batch of B is: every base clip once B >= N_BASE, neighbours differ, repeats beyond"""
    b = np.arange(B)
    return ((b * 5 + b // N_BASE) % N_BASE).astype(np.int32)


_WANT = {}


def base_features(g):
    """float64 oracle features of the base clips at their valid lengths, computed once per row and read-only"""
    if g.name not in _WANT:
        from oracle import featurizer_oracle as fo
        wav, lens, kw = base_clips(g), base_lengths(g), oracle_kw(g)
        want = np.stack([fo.audio_to_feature(wav[b, :min(int(n), stride(g))].astype(np.float64), **kw) for b, n in enumerate(lens)])
        want.setflags(write=False)
        _WANT[g.name] = want
    return _WANT[g.name]


# ---- the streaming stack -----------------------------------------------------------------------------------------------------
def stream_chunks(g):
    """chunk sizes of the streaming cases: half a hop (pushes without a new row), 800, 1023 (an odd carry stride window + chunk),
    and one that brings more than n_features rows in a single push"""
    return (hop_samples(g) // 2, 800, 1023, window_samples(g) + (clip_frames(g) + 2) * hop_samples(g))


PLAN_CHUNKS = ("hop//2", "hop", "window", 800, 1023, 5000)


def plan_chunks(g):
    W, H = window_samples(g), hop_samples(g)
    return (H // 2, H, W, 800, 1023, 5000)


def chunk_loop_rows(g, n_samples, chunk):
    """The chunk loop (oracle/stream_oracle.StreamState, listen.py:96-114) with a framing function that only marks its rows: per chunk
    (rows made so far, the (n_features,) vector of each matrix row's first sample + 1, 0 for a zero row, carry length, carry's first
    sample + 1).  Sample i of the recording has the value i + 1."""
    from oracle import stream_oracle as so
    W, H = window_samples(g), hop_samples(g)
    made = [0]

    def frame_starts(audio):
        n = (len(audio) - W) // H + 1
        made[0] += n
        return np.array([audio[j * H] for j in range(n)], dtype=np.float64).reshape(n, 1)

    st = so.StreamState(clip_frames(g), 1, W, H, frame_starts)
    audio = np.arange(1, n_samples + 1, dtype=np.float64)
    out = []
    for a in range(0, n_samples, chunk):
        m = st.push(audio[a:a + chunk])
        out.append((made[0], m[:, 0].copy(), len(st.window_audio), st.window_audio[0] if len(st.window_audio) else 0))
    return out
