"""Case table of the speed/loudness stage and of the noise mix at their kernel edges (tests/test_speed_mix_edges_host.py,
tests/test_speed_mix_edges_gpu.py): speed_apply_kernel (csrc/kws_speed.hip, csrc/kws_resample.h, also reached through kws_pitch.hip),
augment_plan_kernel and augment_apply_kernel (csrc/kws_augment.hip) and the AUG instantiation of the tuned featurizer.

Speed.  One 256-thread block per clip, thread i makes the outputs i, i + 256, ...; the level is summed per wave (64 lanes), then over
the four waves.  L' = min(ceil(Ls / r), max_samples).  The phase t = n r, its floor and the table position ((phi + k) s) P are fp64;
the table (Z P + 1 floats) sits in dynamic LDS, at most 64 KiB.  The table therefore has

    ratios        the accepted limits 0.5 and 2 and their inner neighbours, 1 and both its neighbours (the phase creeps, so table
                  positions pass within an ulp of integers), 2/3, 4/3 and the two semitone ratios 0.9438743 and 1.0594631
    threads       L' on both sides of a wave (63/64/65), of the block (255/256/257) and of max_samples = 512 (511/512), and 1 and 2,
                  each from Ls = floor(L' r) and its two neighbours; every other clip also levelled
    cut           the default geometry (max_samples 16000, rows of 32002): Ls = floor(t r) + {-1, 0, 1} for t = 15999, 16000, 16001,
                  so ceil(Ls / r) lands below, on and above max_samples; and the rows whole, without valid_len
    tables        (4, 32), (32, 32), (4, 1024) and the two largest that kws_resampler_create accepts, (16, 1023) and (32, 511) (65476
                  and 65412 bytes), and the window and cutoff extremes beta 0 / rolloff 1, beta 20 / rolloff 0.5, beta 5 / rolloff 0.25
    level         targets -80, -20 and 0 dBFS on clips of L' = 0, 1, 63 (three of the four wave partials zero), 64, 65, 257, alone and
                  under two ratios; a silent clip; a clip at amplitude 1e-4, where FLT_EPSILON dominates the mean square
    tiny          max_samples 1, 2 and 3 with clips shorter than, equal to and longer than it

Mix.  The plan kernel gives one wave to a clip, four clips to a block: p_v from fp32 lane partials (lane l takes t = l, l + 64, ...),
p_n from the bank's fp64 prefix sums, prefix[w0 + L] - prefix[w0].  The apply kernel and the fused featurizer build sample t from
aug_sample: m[t - d] for 0 <= t - d < L.  The groups are described at mix_groups().

Everything here is host-only: numpy, the float64 restatements (speed_ref.py, test_augment_gpu.py's np_gain) and test_speed_gpu.py's
source generator."""
import collections
import functools
import math
import zlib

import numpy as np

import speed_ref as sr
from test_augment_gpu import np_gain

F32 = np.float32
NAN = float("nan")
U = 2.0 ** -24
EPS32 = sr.EPS32


def _up(x):
    return np.nextafter(F32(x), F32(np.inf))


def _down(x):
    return np.nextafter(F32(x), F32(-np.inf))


# ---- the kernels' geometry, restated ---------------------------------------------------------------------------------------------------
SPEED_THREADS, WAVE = 256, 64                      # csrc/kws_speed.hip: kThreads; a wave
MAX_TABLE_BYTES = 64 * 1024                        # csrc/kws_resample.h: kMaxTableBytes
PLAN_CLIPS_PER_BLOCK = 4                           # csrc/kws_augment.hip augment_plan_kernel: b = blockIdx.x * 4 + (threadIdx.x >> 6)
AUG_MAX_SNR = 16                                   # include/kws.h: KWS_AUG_MAX_SNR
MAX_SNR_DB = 200.0                                 # csrc/kws_augment.hip: kMaxSnrDb
MAX_SHIFT = 1 << 24                                # csrc/kws_augment.hip check_params: max_shift <= 1 << 24
# include/kws.h kws_aug_clip: eight 4-byte fields, 32 bytes
CLIP_FIELDS = (("apply", "<i4"), ("segment", "<i4"), ("offset", "<i4"), ("shift", "<i4"), ("length", "<i4"), ("snr_db", "<f4"),
               ("gain", "<f4"), ("voice_length", "<i4"))
PAD = 7                                            # out_stride = max_samples + PAD, prefilled with 9.0


def table_bytes(Z, P):
    return 4 * (Z * P + 1)


def synth_lds_bytes(N):
    """csrc/kws_pitch.hip lds_bytes<N>(true): twiddles, two padded exchange buffers, the window and the carry"""
    return (N + 2 * (1024 + 1024 // 16)) * 8 + (N + 3 * N // 4) * 4


# ---- A. speed and loudness -------------------------------------------------------------------------------------------------------------
RATIOS = (F32(0.5), _up(0.5), F32(2.0 / 3.0), F32(0.9438743), _down(1.0), F32(1.0), _up(1.0), F32(1.0594631), F32(4.0 / 3.0), _down(2.0),
          F32(2.0))
THREAD_LP = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512)
TABLE_LP = (1, 64, 65, 256, 257, 512)
LEVEL_LP = (0, 1, 63, 64, 65, 257)
LEVEL_DB = (-80.0, -20.0, 0.0)
CUT_T = (15999, 16000, 16001)
DEFAULT_MS, DEFAULT_STRIDE = 16000, 32002
TINY_MS = (1, 2, 3)
TINY_RATIOS = (F32(0.5), F32(4.0 / 3.0), F32(2.0))

_B, _R = sr.DEFAULTS["beta"], sr.DEFAULTS["rolloff"]
# name -> (zero_crossings, phases, beta, rolloff)
TABLES = collections.OrderedDict([
    ("default", (16, 512, _B, _R)),
    ("z4p32", (4, 32, _B, _R)),
    ("z32p32", (32, 32, _B, _R)),
    ("z4p1024", (4, 1024, _B, _R)),
    ("z16p1023", (16, 1023, _B, _R)),              # 65476 bytes: the largest kws_resampler_create accepts
    ("z32p511", (32, 511, _B, _R)),                # 65412 bytes
    ("beta0", (16, 512, 0.0, 1.0)),
    ("beta20", (16, 512, 20.0, 0.5)),
    ("ctor", (16, 1023, 5.0, 0.25)),               # test_speed_host.py's constructor case, taken whole
])
TABLE_GROUPS = ["table_" + k for k in TABLES if k != "default"]
LARGEST = {"z16p1023": 65476, "z32p511": 65412, "ctor": 65476}

LOUD, SILENT, QUIET = "loud", "silent", "quiet"
# one clip: its ratio (0: not resampled), source length, target (NaN: not levelled) and the kind of its source row
SpeedClip = collections.namedtuple("SpeedClip", "ratio ls db kind")
SpeedGroup = collections.namedtuple("SpeedGroup", "name max_samples stride table clips whole_rows")


def src_len(lp, r):
    """the source length whose neighbours straddle L' = lp: floor(lp r)"""
    return int(math.floor(float(lp) * float(F32(r))))


def _thread_clips(lps, neighbours, levelled):
    out = []
    for r in RATIOS:
        for lp in lps:
            for d in neighbours:
                ls = src_len(lp, r) + d
                if ls >= 0:
                    db = LEVEL_DB[len(out) % 3] if levelled and len(out) % 2 else NAN
                    out.append(SpeedClip(r, ls, db, LOUD))
    return out


def _cut_clips():
    out = []
    for r in RATIOS:
        for t in CUT_T:
            for d in (-1, 0, 1):
                ls = src_len(t, r) + d
                if ls <= DEFAULT_STRIDE:                                 # a row holds no more
                    out.append(SpeedClip(r, ls, NAN, LOUD))
    return out


def _level_clips():
    out = []
    for r in (F32(0.0), F32(4.0 / 3.0), _down(2.0)):
        for lp in LEVEL_LP:
            for db in LEVEL_DB:
                out.append(SpeedClip(r, lp if r == 0 else src_len(lp, r), db, LOUD))
        for db in LEVEL_DB:
            out.append(SpeedClip(r, 300, db, QUIET))
        out.append(SpeedClip(r, 300, -20.0, SILENT))
    return out


def _tiny_clips(ms):
    lens = sorted({0, 1, ms - 1, ms, ms + 1, 2 * ms - 1, 2 * ms, 2 * ms + 1, 7})
    out = [SpeedClip(r, ls, NAN, LOUD) for r in TINY_RATIOS + (F32(0.0),) for ls in lens]
    return out + [SpeedClip(r, ls, -20.0, LOUD) for r in (F32(2.0), F32(0.0)) for ls in (1, ms, 7)]


def _speed_groups():
    g = collections.OrderedDict()
    g["threads"] = SpeedGroup("threads", 512, 1026, "default", _thread_clips(THREAD_LP, (-1, 0, 1), True), False)
    g["cut"] = SpeedGroup("cut", DEFAULT_MS, DEFAULT_STRIDE, "default", _cut_clips(), False)
    g["rows"] = SpeedGroup("rows", DEFAULT_MS, DEFAULT_STRIDE, "default", [SpeedClip(r, DEFAULT_STRIDE, NAN, LOUD) for r in RATIOS], True)
    for k in TABLES:
        if k != "default":
            g["table_" + k] = SpeedGroup("table_" + k, 512, 1026, k, _thread_clips(TABLE_LP, (0,), False), False)
    g["level"] = SpeedGroup("level", 512, 520, "default", _level_clips(), False)
    for ms in TINY_MS:
        g["tiny%d" % ms] = SpeedGroup("tiny%d" % ms, ms, 8, "default", _tiny_clips(ms), False)
    return g


SPEED_GROUPS = _speed_groups()


@functools.lru_cache(maxsize=None)
def speed_table(name):
    Z, P, beta, rolloff = TABLES[name]
    return sr.table(Z, P, beta, rolloff), Z, P


@functools.lru_cache(maxsize=None)
def speed_rows(group):
    """-> (x int16 (rows, stride), lens, index, ratios, targets): one row per distinct (source length, kind), clip b is row index[b].
    The float32 source is these samples scaled by 1/32768, so one reference serves both sample types.  Loud rows have a mean square of
    about 0.09 and a loud first sample (test_speed_gpu.py's _source); a quiet row has amplitude 1e-4, three int16 steps."""
    g = SPEED_GROUPS[group]
    keys = [(c.ls, c.kind) for c in g.clips] if g.whole_rows else sorted({(c.ls, c.kind) for c in g.clips})
    rng = np.random.default_rng(zlib.crc32(group.encode()))
    x = 0.3 * rng.standard_normal((len(keys), g.stride))
    x[:, 0] = 0.3
    for j, (_, kind) in enumerate(keys):
        if kind == SILENT:
            x[j] = 0.0
        elif kind == QUIET:
            x[j] = 1e-4 * rng.standard_normal(g.stride)
    x = np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16)
    lens = np.array([k[0] for k in keys], np.int32)
    index = np.arange(len(keys), dtype=np.int32) if g.whole_rows else np.array([keys.index((c.ls, c.kind)) for c in g.clips], np.int32)
    ratios = np.array([c.ratio for c in g.clips], F32)
    db = np.array([c.db for c in g.clips], F32)
    for a in (x, lens, index, ratios, db):
        a.setflags(write=False)
    return x, lens, index, ratios, db


def speed_f32(x):
    return x.astype(F32) / F32(32768.0)


def speed_source(group, i16):
    x, lens, index, ratios, db = speed_rows(group)
    return (x if i16 else speed_f32(x)), lens, index, ratios, db


def speed_clip_source(group, b):
    """the float32 samples clip b of the group is made from (its whole valid length)"""
    x, lens, index, _, _ = speed_rows(group)
    return speed_f32(x[index[b], :lens[index[b]]])


@functools.lru_cache(maxsize=None)
def speed_expect(group):
    """speed_ref.perturb of every clip of the group: a list of dict(y, A, T, g)"""
    g = SPEED_GROUPS[group]
    h, Z, P = speed_table(g.table)
    return [sr.perturb(speed_clip_source(group, b), c.ratio, c.db, g.max_samples, h, Z, P) for b, c in enumerate(g.clips)]


def speed_bound(ref):
    """test_speed_gpu.py's per-sample bound 2 (T + 3) 2^-24 A"""
    return 2.0 * (ref["T"] + 3) * U * ref["A"]


def first_tap(r, n, P, right=False):
    """the phase arithmetic of the first tap of output n's left (or right) wing, as csrc/kws_resample.h and speed_ref.resample have
    it: -> (j, i, eta, s) with the tap's weight h[i] + eta (h[i + 1] - h[i]) on v[j]"""
    r = float(F32(r))
    s = 1.0 / r if r > 1.0 else 1.0
    t = float(n) * r
    n0 = math.floor(t)
    phi = t - n0
    pos = (((1.0 - phi) if right else phi) * s) * float(P)
    i = int(math.floor(pos))
    return int(n0) + (1 if right else 0), i, pos - i, s


# ---- B. the noise mix ------------------------------------------------------------------------------------------------------------------
MIX_MS = (16000, 300, 2, 1)
MIX_SNRS = (-200.0, -5.0, 0.0, 30.0, 200.0)
# the voice rows' valid_len; ABOVE / NEGATIVE are replaced per max_samples (a length above the row stride, a negative one)
ABOVE, NEGATIVE, FULL, FULL1 = "above", "negative", "ms", "ms-1"
VOICE_LENS = (0, 1, 2, 63, 64, 65, FULL1, FULL, ABOVE, NEGATIVE)
SILENT_ROW, I16_MIN_ROW = len(VOICE_LENS), len(VOICE_LENS) + 1

MixCase = collections.namedtuple("MixCase", "row apply segment offset shift snr")
MIX_TAILS = {"lengths": 3, "segment": 2, "offsets": 3, "shifts": 1, "snrs": 2, "one": 1}     # B mod 4 of every group
MixBank = collections.namedtuple("MixBank", "segs names samples seg_len start prefix")


def mix_stride(ms):
    return ms + 5


def _voice_len(tag, ms):
    return {ABOVE: mix_stride(ms) + 10, NEGATIVE: -3, FULL: ms, FULL1: ms - 1}.get(tag, tag)


def clipped_len(valid_len, stride, max_samples):
    """Lv of a row: csrc/kws_wave_stage.h clip_src"""
    return int(min(max(int(valid_len), 0), stride, max_samples))


@functools.lru_cache(maxsize=None)
def mix_voices(ms, i16):
    """-> (x (rows, ms + 5), valid_len): loud noise rows, one per entry of VOICE_LENS (samples past the valid length stay loud: a clip
    read one sample long changes), a silent full row and a full row at the int16 minimum"""
    rng = np.random.default_rng(1000 + ms)
    x = (0.3 * rng.standard_normal((len(VOICE_LENS) + 2, mix_stride(ms)))).astype(F32)
    x[SILENT_ROW] = 0.0
    x[I16_MIN_ROW] = -1.0
    lens = np.array([_voice_len(t, ms) for t in VOICE_LENS] + [ms, ms], np.int32)
    if i16:
        x = np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16)
    x.setflags(write=False)
    lens.setflags(write=False)
    return x, lens


def mix_f32(x):
    return x.astype(F32) / F32(32768.0) if x.dtype == np.int16 else x


def _edged(rng, n, edge, amp=0.01):
    """quiet noise whose first and last samples are +-edge: a window read one sample off changes its power"""
    s = (amp * rng.standard_normal(n)).astype(F32)
    s[0] = edge
    s[-1] = -edge if n > 1 else edge
    return s


def _edge(j):
    """0.9 and 0.8 in turn, so that a window that slides into the neighbouring segment changes its power too"""
    return 0.9 if j % 2 == 0 else 0.8


@functools.lru_cache(maxsize=None)
def mix_bank(ms, single=False):
    """The bank of max_samples ms: edged (+-0.9 or +-0.8) quiet segments of 1, 2, 64, 65, ms - 1, ms, ms + 1 and 2 ms + 3 samples, an all-zero one, a
    loud one with ms + 8 zeros inside, 50000 loud samples of ballast and, last, a quiet one (1e-4) of 2 ms + 3.  single: the bank of
    one edged segment of ms samples."""
    rng = np.random.default_rng(2000 + ms)
    if single:
        named = [("only", _edged(rng, ms, 0.9))]
    else:
        named = [("e%d" % n, _edged(rng, n, _edge(j))) for j, n in enumerate((1, 2, 64, 65, ms - 1, ms, ms + 1, 2 * ms + 3)) if n >= 1]
        hole = (0.5 * rng.standard_normal(3 * ms + 40)).astype(F32)
        hole[ms + 16:2 * ms + 24] = 0.0
        named += [("zero", np.zeros(ms + 1, F32)), ("hole", hole), ("ballast", (0.5 * rng.standard_normal(50000)).astype(F32)),
                  ("quiet", (1e-4 * rng.standard_normal(2 * ms + 3)).astype(F32))]
    names = [k for k, _ in named]
    assert len(set(names)) == len(names) or ms <= 2          # at ms <= 2 the lengths ms - 1 .. ms + 1 repeat 1 and 2: first one wins
    segs = [s for _, s in named]
    samples = np.concatenate(segs)
    seg_len = np.array([len(s) for s in segs], np.int64)
    start = np.concatenate([[0], np.cumsum(seg_len)[:-1]])
    prefix = np.concatenate([[0.0], np.cumsum(samples.astype(np.float64) ** 2)])    # kws_noise_bank_create: pre[i + 1] = pre[i] + x^2
    return MixBank(segs, names, samples, seg_len, start, prefix)


def seg(ms, name):
    return mix_bank(ms).names.index(name)


def mix_groups(ms):
    """name -> [MixCase]: one kws_augment_plan / kws_augment_apply call each.

    lengths   every voice row under the long edged segment: Lv = 0, 1, 2, 63, 64, 65, ms - 1, ms, a valid_len above the stride, a
              negative one, the silent voice
    segment   seg_len = Lv - 1, Lv, Lv + 1 (L cut by the segment, equal, cut by the voice) and the 1- and 2-sample segments under a full clip
    offsets   0, seg_len - L (the last legal one), seg_len - 1 (comes back clamped), and the bank's last segment at its last legal
              offset, which reads prefix[total]
    shifts    0, +-1, +-(L - 1), +-L, +-(L + 1), +-2^24, at 16000 also +-511, +-512, +-1024, for an even and an odd L, noised and not
    snrs      -200, -5, 0, 30, 200 over edged, zero, hole (the zero stretch), quiet; a silent voice; apply = 0 with any segment and offset
    one       a single clip"""
    bank = mix_bank(ms)
    sl = lambda name: int(bank.seg_len[seg(ms, name)])
    row = {t: j for j, t in enumerate(VOICE_LENS)}
    lv = lambda r: clipped_len(mix_voices(ms, False)[1][r], mix_stride(ms), ms)
    long_ = seg(ms, "e%d" % (2 * ms + 3))
    g = collections.OrderedDict()
    g["lengths"] = [MixCase(r, 1, long_, 3, 0, 0.0) for r in range(len(VOICE_LENS) + 1)]
    c = []
    for t in VOICE_LENS:
        for d in (-1, 0, 1):
            name = "e%d" % (lv(row[t]) + d)
            if isinstance(t, (int, str)) and t not in (ABOVE, NEGATIVE) and name in bank.names:
                c.append(MixCase(row[t], 1, seg(ms, name), 0, 0, 5.0))
    c += [MixCase(row[FULL], 1, seg(ms, "e1"), 0, 0, 0.0), MixCase(row[FULL], 1, seg(ms, "e2"), 0, 1, 0.0)]
    g["segment"] = c
    c = []
    for t, name in ((FULL, "e%d" % (2 * ms + 3)), (64, "e65"), (63, "e%d" % (ms + 1)), (FULL1, "e%d" % ms), (FULL, "hole"), (FULL, "quiet"),
                    (1, "quiet"), (65, "quiet")):
        L = min(lv(row[t]), sl(name))
        for o in sorted({0, min(sl(name) - L, sl(name) - 1), sl(name) - 1}):
            c.append(MixCase(row[t], 1, seg(ms, name), o, 0, 10.0))
    g["offsets"] = c
    c = []
    for t in (FULL, FULL1, 65, 64, 2):
        L = lv(row[t])
        ds = {0, 1, L - 1, L, L + 1, MAX_SHIFT} | ({511, 512, 1024} if ms == 16000 and L > 1024 else set())
        for d in sorted(ds | {-d for d in ds}):
            c.append(MixCase(row[t], 0 if d % 3 == 2 else 1, long_, 1, d, 3.0))
    g["shifts"] = c
    c = []
    for s in MIX_SNRS:
        for name, o in ((bank.names[long_], 2), ("zero", 0), ("hole", ms + 20), ("quiet", 1)):
            if o + min(ms, sl(name)) <= sl(name):
                c.append(MixCase(row[FULL], 1, seg(ms, name), o, 0, s))
        c.append(MixCase(I16_MIN_ROW, 1, seg(ms, "zero"), 0, 0, s))                  # |v| = 1 over silence: the largest gain there is
        c.append(MixCase(SILENT_ROW, 1, long_, 0, 1, s))
    c += [MixCase(row[FULL], 0, seg(ms, "e1"), 0, 0, 7.0), MixCase(row[65], 0, seg(ms, "ballast"), 49999, -1, -200.0),
          MixCase(SILENT_ROW, 0, seg(ms, "quiet"), 2 * ms + 2, 0, 200.0)]
    g["snrs"] = c
    g["one"] = [MixCase(row[FULL], 1, long_, ms + 3, -1, 0.0)]
    for k, tail in MIX_TAILS.items():                                    # the batch's tail against four clips per block
        while len(g[k]) % PLAN_CLIPS_PER_BLOCK != tail:
            g[k].append(MixCase(row[2], 0, 0, 0, 0, 0.0))
    return g


def mix_records(ms, group):
    """the explicit records of a group (CLIP_FIELDS), rows"""
    cases = mix_groups(ms)[group]
    ex = np.zeros(len(cases), np.dtype(list(CLIP_FIELDS)))
    for b, c in enumerate(cases):
        ex["apply"][b], ex["segment"][b], ex["offset"][b], ex["shift"][b], ex["snr_db"][b] = c.apply, c.segment, c.offset, c.shift, c.snr
    ex["length"], ex["gain"], ex["voice_length"] = -7, 9.0, -7            # filled by the plan, whatever the caller left there
    return ex, np.array([c.row for c in cases], np.int32)


MixExpect = collections.namedtuple("MixExpect", "lv L offset silent gain bound w0")


def plan_expect(ms, case, v32, lens, bank=None):
    """What kws_augment_plan must report for one explicit record over the voice rows v32 with valid_len lens (None: the rows whole):
    Lv, L, the clamped offset, whether the gain must be exactly 0, the float64 gain and its relative bound
    (ceil(L / 64) / 2 + 2) 2^-24 + 2^-54 prefix[w0 + L] / (p_n + FLT_EPSILON)."""
    bank = bank or mix_bank(ms)
    lv = clipped_len(mix_stride(ms) if lens is None else lens[case.row], mix_stride(ms), ms)
    sl = int(bank.seg_len[case.segment])
    L = min(lv, sl) if case.apply else lv
    off = min(case.offset, sl - L) if case.apply else case.offset
    v = v32[case.row]
    n = bank.segs[case.segment]
    silent = not case.apply or L == 0 or not v[:L].any()
    gain, bound, w0 = 0.0, 0.0, int(bank.start[case.segment]) + off
    if not silent:
        gain = np_gain(v, n, L, off, float(F32(case.snr)))
        pn = float(np.mean(n[off:off + L].astype(np.float64) ** 2))
        bound = (math.ceil(L / 64.0) / 2.0 + 2.0) * U + 2.0 ** -54 * bank.prefix[w0 + L] / (pn + EPS32)
    return MixExpect(lv, L, off, silent, gain, bound, w0)


def mix_f64(v, n, L, offset, shift, gain, apply):
    """m'[0:L] in float64: m[t - d] for 0 <= t - d < L, else 0; m[u] = v[u] + g n[offset + u] when noised, g the float32 gain given"""
    m = v[:L].astype(np.float64)
    if apply:
        m = m + float(F32(gain)) * n[offset:offset + L].astype(np.float64)
    out = np.zeros(L)
    t = np.arange(L)
    ok = (t - shift >= 0) & (t - shift < L)
    out[ok] = m[t[ok] - shift]
    return out


def mix_sample_bound(ref):
    """one correctly rounded fused multiply-add, with room for the reference's own double rounding"""
    return 2.0 ** -23 * np.abs(ref) + 2.0 ** -149


def plan_gain_f32(v, L, w0, snr, bank):
    """the plan kernel's own arithmetic on the host: fp32 lane partials of fused x x + part, an fp64 wave sum, p_n from the prefix sums"""
    x = v[:L].astype(np.float64)
    part = np.zeros(WAVE, F32)
    for t0 in range(0, L, WAVE):
        blk = x[t0:t0 + WAVE]
        part[:len(blk)] = (blk * blk + part[:len(blk)].astype(np.float64)).astype(F32)
    pv = float(part.astype(np.float64).sum()) / L
    pn = (bank.prefix[w0 + L] - bank.prefix[w0]) / L
    return F32(math.sqrt(pv / 10.0 ** (float(F32(snr)) / 10.0) / (pn + EPS32)))
