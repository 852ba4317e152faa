"""Case table of the two wet wave-augmentation kernels at their section, chunk and length edges (tests/test_wave_edges_host.py,
tests/test_wave_edges_gpu.py): filter_apply_kernel (csrc/kws_filter.hip) and reverb_apply_kernel (csrc/kws_reverb.hip).

The filter kernel gives one wave to a clip.  The clip padded by the odd extension, lpad = Lv + 2 padlen samples, is cut into 64 chunks
of C = 2^m samples, m the smallest in 2..8 with 64 C >= lpad; lane i owns chunk i, and the scan across lanes reads the stored powers
A^(2^(m + j)), j < 6, of the n x n state matrix, n = 2 n_sections.  kws_filter_apply picks one of four instantiations by the bank's
n_sections.  A clip of Lv <= padlen stays dry.  The table therefore has

    banks S1..S4               one per instantiation, each with a design of fewer sections (padded with identity sections)
    banks PAD1, PAD32          padlen forced to 1 and to KWS_FILTER_MAX_PADLEN (both LDS edges full: 64 floats)
    chunk lengths              lpad = 64 << m and (64 << m) + 1 for m = 2..7 and every padlen in {1, 6, 27, 32}, lpad = 16384 (m = 8,
                               padlen 32, Lv = KWS_FILTER_MAX_SAMPLES), a last lane with one sample and with none at m = 2, 5, 8,
                               Lv = padlen (dry) and padlen + 1
    max_samples                16320, 15999, 28, 7 and 1, each with clips that max_samples cuts and with a row stride equal to and
                               above it

The reverb kernel gives one block to a clip and convolves by one 16384-point complex transform: Lv <= max_samples <= 16384 and, after
the bank's clipping, Lh <= the bank's max_samples <= 16384; the output has L' = min(Lv + Lh - 1, max_samples) samples (0 for an empty
clip).  A clip of at most 64 samples is convolved directly in fp64, a longer one by the transform.  The table runs max_samples 16384,
16383, 8193, 1000, 3, 2 and 1 for the bank and the call alike, and a bank of 16384 under a call of 1000 and a bank of 100 under a call
of 16384, each with clips of 64 and 65 samples where max_samples allows them.

Everything here is host-only: numpy, the float64 restatements, and the generators of test_filter_gpu.py / test_reverb_gpu.py."""
import collections
import functools

import numpy as np

import test_filter_gpu as tfg
import test_reverb_gpu as trg
from filter_ref import filtfilt_batch
from reverb_ref import bank_taps, reverb_pair

# ---- the kernels' geometry, restated ---------------------------------------------------------------------------------------------------
LANES, MIN_LOG, MAX_LOG = 64, 2, 8                 # csrc/kws_filter.h: kLanes, kMinLog, kMaxLog
FILTER_MAX_SAMPLES, FILTER_MAX_PADLEN = 16320, 32  # include/kws.h
REVERB_MAX_SAMPLES = 16384
REVERB_DIRECT = 64                                 # csrc/kws_reverb.hip kDirect: clips up to it are convolved directly in fp64


def chunk_log(lpad):
    """m of a padded clip of lpad samples: the smallest in MIN_LOG..MAX_LOG with LANES << m >= lpad"""
    assert 1 <= lpad <= LANES << MAX_LOG
    m = MIN_LOG
    while (LANES << m) < lpad:
        m += 1
    return m


def last_lane(lpad):
    """(the last lane with a sample, how many it has)"""
    C = 1 << chunk_log(lpad)
    return (lpad - 1) // C, (lpad - 1) % C + 1


def clipped_len(valid_len, stride, max_samples):
    """Lv of a row: csrc/kws_wave_stage.h clip_src"""
    return int(min(max(int(valid_len), 0), stride, max_samples))


def filter_choice(k, lv, padlens):
    """filter_used of a clip of Lv samples given design k: dry (-1) when not chosen or too short for the odd extension"""
    return int(k) if k >= 0 and lv > padlens[k] else -1


def reverb_len_out(lv, lh, max_samples):
    """L' of a wet clip of Lv samples under a RIR of Lh taps (as the bank holds it)"""
    return 0 if lv == 0 else min(lv + lh - 1, max_samples)


# ---- filter banks ----------------------------------------------------------------------------------------------------------------------
# name -> (specs, forced padlen or None)
BANKS = {
    "S1": ([("lowpass", 2, 3000.0), ("highpass", 1, 500.0), ("highpass", 2, 50.0)], None),
    "S2": ([("lowpass", 4, 2000.0), ("highpass", 3, 50.0), ("bandpass", 2, (300.0, 3400.0)), ("bandstop", 2, (900.0, 1130.0)),
            ("highpass", 1, 500.0)], None),
    "S3": ([("lowpass", 6, 5000.0), ("highpass", 5, 100.0), ("bandpass", 3, (300.0, 3400.0)), ("bandstop", 3, (900.0, 1130.0)),
            ("lowpass", 2, 3000.0)], None),
    "S4": (tfg.SPECS, None),                                             # the control: test_filter_gpu.py's bank
    "PAD32": ([("lowpass", 8, 7000.0), ("highpass", 4, 50.0)], 32),
    "PAD1": ([("lowpass", 4, 2000.0), ("highpass", 1, 500.0)], 1),
}
N_SECTIONS = {"S1": 1, "S2": 2, "S3": 3, "S4": 4, "PAD32": 4, "PAD1": 2}


def spec_sections(spec):
    btype, order, _ = spec
    return order if btype in ("bandpass", "bandstop") else (order + 1) // 2


def spec_padlen(spec):
    """filtfilt's default 3 (n + 1), n the transfer function's order"""
    btype, order, _ = spec
    return 3 * (order * (2 if btype in ("bandpass", "bandstop") else 1) + 1)


def bank_padlens(name):
    specs, forced = BANKS[name]
    return [spec_padlen(s) if forced is None else forced for s in specs]


@functools.lru_cache(maxsize=None)
def make_bank(name):
    """the FilterBank of BANKS[name]; a forced padlen is written before the handle exists (FilterBank passes self.padlen on first use)"""
    from kws_amd.augment import FilterBank
    specs, forced = BANKS[name]
    bank = FilterBank(specs)
    if forced is not None:
        assert bank._h is None
        bank.padlen[:] = forced
    return bank


# ---- filter groups: one kernel call each -----------------------------------------------------------------------------------------------
# clips: (design or -1, valid_len) per row; stride: the row stride of the wide source (a tight one is its first max_samples columns)
FilterGroup = collections.namedtuple("FilterGroup", "name bank max_samples stride clips seed")
FILTER_GROUPS = collections.OrderedDict()


def _add(name, bank, max_samples, stride, clips, seed):
    FILTER_GROUPS[name] = FilterGroup(name, bank, max_samples, stride, tuple(clips), seed)


# 1. section counts: Lv = padlen and padlen + 1 of every design, then mixed lengths over the designs in turn, one clip not chosen
_MIXED = [16000, 17000, 257, 3001, 0, 7000, 100, 1000, 4097, 12345]
SECTION_GROUPS = ["S1", "S2", "S3", "S4"]
for _i, _name in enumerate(SECTION_GROUPS):
    _pads = bank_padlens(_name)
    _clips = [(k, p + d) for k, p in enumerate(_pads) for d in (0, 1)]
    _clips += [(j % len(_pads), lv) for j, lv in enumerate(_MIXED[:max(6, 16 - len(_clips))])]
    _add(_name, _name, 16000, 17000, _clips + [(-1, 5000)], 100 + _i)


# 2. chunk boundaries: (padlen, Lv, lpad, m, what) per case
def _chunk_cases(p):
    out = []
    for m in range(MIN_LOG, MAX_LOG):
        out.append((p, (LANES << m) - 2 * p, LANES << m, m, "every lane full"))
        out.append((p, (LANES << m) - 2 * p + 1, (LANES << m) + 1, m + 1, "one sample past: 32 lanes full, one with 1, 31 empty"))
    if (LANES << MAX_LOG) - 2 * p <= FILTER_MAX_SAMPLES:
        out.append((p, (LANES << MAX_LOG) - 2 * p, LANES << MAX_LOG, MAX_LOG, "every lane full"))
    for m in (2, 5, 8):
        C = 1 << m
        out.append((p, 63 * C + 1 - 2 * p, 63 * C + 1, m, "last lane holds one sample"))
        out.append((p, 63 * C - 2 * p, 63 * C, m, "last lane empty"))
    out.append((p, p, 3 * p, chunk_log(3 * p), "dry"))
    out.append((p, p + 1, 3 * p + 1, chunk_log(3 * p + 1), "shortest wet clip"))
    return out


CHUNK_PADLENS = (1, 6, 27, 32)
CHUNK_CASES = [c for p in CHUNK_PADLENS for c in _chunk_cases(p)]
CHUNK_GROUPS = collections.OrderedDict([("chunk_p1", ("PAD1", (1,))), ("chunk_p6_p27", ("S4", (6, 27))), ("chunk_p32", ("PAD32", (32,)))])
for _i, (_name, (_bank, _ps)) in enumerate(CHUNK_GROUPS.items()):
    _pads = bank_padlens(_bank)
    _clips = []
    for p in _ps:
        ks = [k for k, q in enumerate(_pads) if q == p]                  # the designs of that padlen, in turn
        _clips += [(ks[j % len(ks)], c[1]) for j, c in enumerate(_chunk_cases(p))]
    _add(_name, _bank, FILTER_MAX_SAMPLES, LANES << MAX_LOG, _clips, 200 + _i)

# 3. max_samples: S4's designs 2 and 4 have padlen 27, 0, 3 and 6 have 15, 7 has 12 and 5 has 6
MS_GROUPS = collections.OrderedDict([(16320, ["ms16320", "ms16320_p32"]), (15999, ["ms15999"]), (28, ["ms28"]), (7, ["ms7"]), (1, ["ms1"])])
for _j, _ms in enumerate((16320, 15999)):
    _add("ms%d" % _ms, "S4", _ms, _ms + 700,
         [(2, _ms), (4, _ms + 1), (5, _ms + 50), (0, _ms + 700), (7, 9001), (3, 28), (2, 27), (-1, _ms + 3), (6, _ms - 1)], 300 + _j)
_add("ms16320_p32", "PAD32", 16320, 16320 + 700,                        # (0, 16320): lpad = 16384, the last stored power A^(2^13)
     [(0, 16320), (1, 16321), (1, 16320 + 700), (0, 16319), (1, 33), (0, 32), (-1, 16320)], 302)
_add("ms28", "S4", 28, 41,                                              # (2, 28): wet with lpad = 82
     [(2, 28), (4, 40), (0, 16), (5, 7), (5, 6), (2, 27), (3, 41), (-1, 28), (7, 13), (6, 29)], 303)
# every design but 5 has padlen >= 7 and design 5 (padlen 6) gets a clip of 6: all dry (its wet clip of 7 samples is in ms28)
_add("ms7", "S4", 7, 20, [(0, 7), (1, 20), (2, 7), (3, 6), (4, 20), (6, 7), (7, 8), (5, 6), (-1, 7), (-1, 20)], 304)
_add("ms1", "S4", 1, 14, [(0, 1), (5, 1), (5, 14), (2, 0), (-1, 1), (-1, 14), (4, 2)], 305)
ALL_DRY_GROUPS = ("ms7", "ms1")
IN_PLACE_GROUPS = ("ms16320", "ms15999")


def vf32(x):
    return x.astype(np.float32) / np.float32(32768.0) if x.dtype == np.int16 else x


def filter_source(group, i16, tight=False):
    """-> (x (rows, stride), valid_len, explicit): noise plus an offset and a ramp (test_filter_gpu.py's _voices), one row per clip;
    tight: the row stride is max_samples (the first max_samples columns of the wide source)"""
    g = FILTER_GROUPS[group]
    n = len(g.clips)
    x, _ = tfg._voices(np.random.default_rng(g.seed), max(n, 10), i16, g.stride)
    x = np.ascontiguousarray(x[:n, :g.max_samples] if tight else x[:n])
    return x, np.array([c[1] for c in g.clips], np.int32), np.array([c[0] for c in g.clips], np.int32)


FilterExpect = collections.namedtuple("FilterExpect", "clips used ref")


@functools.lru_cache(maxsize=None)
def filter_expect(group, i16):
    """per clip of the group: the float32 input v[:Lv], filter_used and the float64 filtfilt without the rescale (None when dry).  A
    tight source gives the same clips: Lv never exceeds max_samples."""
    g = FILTER_GROUPS[group]
    bank = make_bank(g.bank)
    x, lens, ex = filter_source(group, i16)
    v32 = vf32(x)
    clips = [v32[b, :clipped_len(lens[b], g.stride, g.max_samples)] for b in range(len(lens))]
    used = [filter_choice(k, len(c), bank.padlen) for k, c in zip(ex, clips)]
    wet = [b for b, u in enumerate(used) if u >= 0]
    ys = filtfilt_batch([bank.sos[used[b]] for b in wet], [clips[b] for b in wet], [int(bank.padlen[used[b]]) for b in wet])
    ref = [None] * len(clips)
    for b, y in zip(wet, ys):
        ref[b] = y
    return FilterExpect(clips, used, ref)


# ---- reverb groups: one kernel call each -----------------------------------------------------------------------------------------------
REVERB_MS = (16384, 16383, 8193, 1000, 3, 2, 1)                  # the bank's and the call's max_samples alike
REVERB_MIXED = ((16384, 1000), (100, 16384))                    # (the bank's, the call's)
LONG = 8000                                                     # a pair with Lv and Lh both above it costs the reference most
SILENT_ROW = 9                                                  # test_reverb_gpu.py's _voices zeroes row 9
# the table's rows, RIRs (float32, peak first, as given to RirBank) and (row, RIR or -1) pairs
ReverbGroup = collections.namedtuple("ReverbGroup", "bank_ms call_ms stride valid_len rirs pairs loud")
# per group the first seed whose rows and RIRs meet test_wave_edges_host.py's conditions (peak first; a first sample loud enough for
# the tap at eff - 1 to be heard a thousand bounds above the error allowed): found on the CPU, from the references alone
_REVERB_SEED = {(16384, 16384): 4, (16383, 16383): 1, (8193, 8193): 3, (1000, 1000): 1, (3, 3): 1, (2, 2): 1, (1, 1): 1,
                (16384, 1000): 1, (100, 16384): 1}


def _dedupe(values, lowest):
    out = []
    for v in values:
        if v >= lowest and v not in out:
            out.append(v)
    return out


def _rir(rng, n, eff):
    """test_reverb_gpu.py's _rirs at any length; one that outlasts eff = min(the bank's, the call's max_samples) carries a loud tap at
    eff - 1, which must be heard, and one at eff, which must not"""
    h = 0.3 * rng.standard_normal(n) * np.exp(-np.arange(n) / 2000.0)
    h[0] = 1.0
    if n > eff:
        if eff > 1:
            h[eff - 1] = 0.9
        h[eff] = -0.8
    return h.astype(np.float32)


@functools.lru_cache(maxsize=None)
def reverb_group(bank_ms, call_ms):
    ms, eff = call_ms, min(bank_ms, call_ms)
    mid = (ms // 3) | 1
    clip_lens = [0, 1, 2, mid, ms - 1, ms, ms + 5]
    if bank_ms < ms:
        clip_lens += [ms - bank_ms + d for d in (0, 1, 2)]               # Lv + Lh - 1 = ms - 1, ms, ms + 1 under the bank's longest RIR
    if ms > REVERB_DIRECT + 1:
        clip_lens += [REVERB_DIRECT, REVERB_DIRECT + 1]                   # the last clip of the direct path, the first of the transform
    clip_lens = _dedupe(clip_lens, 0)
    rir_lens = [1, 2, 3, bank_ms - 1, bank_ms]
    if ms < bank_ms:
        rir_lens += [ms - 1, ms]
    rir_lens = _dedupe(rir_lens, 1) + [bank_ms + 500]
    rng = np.random.default_rng(1000 + _REVERB_SEED[(bank_ms, call_ms)])
    rirs = tuple(_rir(rng, n, eff) for n in rir_lens)
    loud = len(rirs) - 1
    first = SILENT_ROW + 1
    valid_len = np.zeros(first + len(clip_lens), np.int32)
    valid_len[SILENT_ROW] = mid
    valid_len[first:] = clip_lens
    keep_long = {(ms - 1, ms - 1), (ms, ms), (ms + 5, ms + 500), (ms, ms + 500)}
    pairs = []
    for i, lv in enumerate(clip_lens):
        for k, lh in enumerate(rir_lens):
            if min(lv, ms) > LONG and min(lh, bank_ms) > LONG and (lv, lh) not in keep_long:
                continue
            pairs.append((first + i, k))
    pairs += [(first + clip_lens.index(lv), -1) for lv in _dedupe([0, mid, ms + 5], 0)]
    pairs += [(SILENT_ROW, min(2, loud)), (SILENT_ROW, loud), (SILENT_ROW, -1)]
    return ReverbGroup(bank_ms, call_ms, ms + 5, valid_len, rirs, tuple(pairs), loud)


def reverb_source(bank_ms, call_ms, i16):
    """-> (x (rows, stride), valid_len, index, explicit): seeded standard_normal rows and one silent row (test_reverb_gpu.py's _voices)"""
    g = reverb_group(bank_ms, call_ms)
    x, _ = trg._voices(np.random.default_rng(_REVERB_SEED[(bank_ms, call_ms)]), len(g.valid_len), i16, g.stride)
    return x, g.valid_len, np.array([r for r, _ in g.pairs], np.int32), np.array([k for _, k in g.pairs], np.int32)


def long_pairs(g):
    """the pairs of a group with Lv and Lh both above LONG"""
    return [(r, k) for r, k in g.pairs
            if k >= 0 and clipped_len(g.valid_len[r], g.stride, g.call_ms) > LONG and len(bank_taps(g.rirs[k], g.bank_ms)) > LONG]


ReverbExpect = collections.namedtuple("ReverbExpect", "clips taps length ref scale")


def reverb_expect_from(g, x, rirs):
    v32 = vf32(x)
    clips, taps, length, ref, scale = [], [], [], [], []
    for r, k in g.pairs:
        v = v32[r, :clipped_len(g.valid_len[r], g.stride, g.call_ms)]
        clips.append(v)
        if k < 0:
            taps.append(None), length.append(len(v)), ref.append(None), scale.append(1.0)
            continue
        h = bank_taps(rirs[k], g.bank_ms)
        y, s = reverb_pair(v, rirs[k], g.bank_ms, g.call_ms)
        taps.append(h), length.append(reverb_len_out(len(v), len(h), g.call_ms)), ref.append(y), scale.append(s)
    return ReverbExpect(clips, taps, length, ref, scale)


@functools.lru_cache(maxsize=None)
def reverb_expect(bank_ms, call_ms, i16):
    """per pair of the group: the float32 input v[:Lv], the taps the bank keeps, L', the float64 convolution without the rescale and
    the scale the rescale applies (taps and convolution None when dry)"""
    g = reverb_group(bank_ms, call_ms)
    return reverb_expect_from(g, reverb_source(bank_ms, call_ms, i16)[0], g.rirs)
