"""CPU tests of tests/speed_mix_cases.py: every case of the speed/loudness and noise-mix edge table is what it claims, none is vacuous,
and the constants the table restates are those of the sources.  From the references alone; no device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import speed_mix_cases as sm
import speed_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tf-keras-speech-commands_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


# ---- the restated constants ------------------------------------------------------------------------------------------------------------
def test_restated_constants_are_the_sources():
    from kws_amd import lib as l
    from kws_amd.augment import CLIP_DTYPE
    kws_h = open(os.path.join(ROOT, "include", "kws.h")).read()
    assert int(re.search(r"#define KWS_AUG_MAX_SNR (\d+)", kws_h).group(1)) == sm.AUG_MAX_SNR == l.AUG_MAX_SNR
    body = re.search(r"typedef struct kws_aug_clip \{(.*?)\} kws_aug_clip;", kws_h, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|float) (\w+);", body, re.M)
    assert [(n, "<i4" if t == "int32_t" else "<f4") for t, n in fields] == list(sm.CLIP_FIELDS)
    assert np.dtype(list(sm.CLIP_FIELDS)) == CLIP_DTYPE and CLIP_DTYPE.itemsize == ctypes.sizeof(l.KwsAugClip) == 32
    assert [f[0] for f in l.KwsAugClip._fields_] == [n for n, _ in sm.CLIP_FIELDS]
    aug = _src("kws_augment.hip")
    assert "blockIdx.x * %d + (int)(threadIdx.x >> 6)" % sm.PLAN_CLIPS_PER_BLOCK in aug
    assert "(B + %d) / %d" % (sm.PLAN_CLIPS_PER_BLOCK - 1, sm.PLAN_CLIPS_PER_BLOCK) in aug
    assert "kMaxSnrDb = %g.f" % sm.MAX_SNR_DB in aug and l.AUG_MAX_SNR_DB == sm.MAX_SNR_DB
    assert "p->max_shift > (1 << 24)" in aug and sm.MAX_SHIFT == 1 << 24
    assert "kMaxTableBytes = 64 * 1024" in _src("kws_resample.h") and sm.MAX_TABLE_BYTES == 64 * 1024
    assert "kThreads = %d" % sm.SPEED_THREADS in _src("kws_speed.hip")
    pitch = _src("kws_pitch.hip")
    assert "(N + 2 * kBuf) * (int)sizeof(float2) + (N + (synth ? 3 * N / 4 : 0)) * (int)sizeof(float)" in pitch
    assert "kBuf = kPoints + kPoints / 16" in pitch and "kPoints = 1024" in pitch


def test_ratios_are_the_float32_neighbours():
    r = sm.RATIOS
    assert len(r) == len(set(float(x) for x in r)) == 11 and all(x.dtype == np.float32 for x in r) and list(r) == sorted(r)
    assert r[0] == 0.5 and float(r[1]) == 0.5 + 2.0 ** -24 and float(r[4]) == 1.0 - 2.0 ** -24 and r[5] == 1.0
    assert float(r[6]) == 1.0 + 2.0 ** -23 and float(r[9]) == 2.0 - 2.0 ** -23 and r[10] == 2.0
    assert r[2] == np.float32(2.0 / 3.0) and r[8] == np.float32(4.0 / 3.0)
    assert abs(float(r[3]) - 2.0 ** (-1.0 / 12.0)) < 1e-7 and abs(float(r[7]) - 2.0 ** (1.0 / 12.0)) < 1e-7


# ---- A. speed: coverage ----------------------------------------------------------------------------------------------------------------
def _lp(c, ms):
    return min(c.ls, ms) if c.ratio == 0 else sr.out_length(c.ls, c.ratio, ms)


def test_thread_group_sits_on_both_sides_of_every_boundary():
    g = sm.SPEED_GROUPS["threads"]
    assert g.max_samples == 512 and g.table == "default"
    hit = set()
    for r in sm.RATIOS:
        reachable = {sr.out_length(ls, r, 10 ** 9) for ls in range(0, 1100)}
        for lp in sm.THREAD_LP:
            got = {sr.out_length(c.ls, r, 10 ** 9) for c in g.clips if c.ratio == r and abs(c.ls - sm.src_len(lp, r)) <= 1}
            if lp in reachable:
                assert lp in got, (float(r), lp, got)
                hit.add(lp)
            else:                                                        # r < 1 skips lengths: the neighbours on both sides then
                assert min(got) < lp < max(got), (float(r), lp, got)
    assert hit == set(sm.THREAD_LP)
    lev = [c for c in g.clips if not math.isnan(c.db)]
    assert abs(2 * len(lev) - len(g.clips)) <= 1 and {c.db for c in lev} == set(sm.LEVEL_DB)
    assert {_lp(c, 512) for c in lev} >= {1, 63, 64, 65, 256, 257, 512}
    assert max(c.ls for c in g.clips) < g.stride
    # a block's threads: L' = 257 gives thread 0 a second output, 63 / 64 / 65 fill wave 0 but for one lane, wholly, and one lane of wave 1
    assert sm.SPEED_THREADS == 256 and sm.WAVE == 64


def test_cut_group_lands_below_on_and_above_max_samples():
    g = sm.SPEED_GROUPS["cut"]
    assert (g.max_samples, g.stride) == (16000, 32002)
    for r in sm.RATIOS:
        q = [math.ceil(float(c.ls) / float(r)) for c in g.clips if c.ratio == r]
        assert min(q) < 16000 < max(q), (float(r), sorted(set(q)))
        if any(math.ceil(float(ls) / float(r)) == 16000 for ls in range(7000, 32003)):   # r < 1 may step over it: 15999, then 16001
            assert 16000 in q, (float(r), sorted(set(q)))
        else:
            assert r < 1
    assert max(c.ls for c in g.clips) == 32002                           # a resampled clip's whole valid length is its source
    rows = sm.SPEED_GROUPS["rows"]
    assert rows.whole_rows and [c.ratio for c in rows.clips] == list(sm.RATIOS) and all(c.ls == rows.stride == 32002 for c in rows.clips)


def test_table_groups_and_byte_counts():
    from kws_amd.augment import Resampler
    assert len(sm.TABLE_GROUPS) == 8
    for name, (Z, P, beta, rolloff) in sm.TABLES.items():
        assert sm.table_bytes(Z, P) <= sm.MAX_TABLE_BYTES
        rs = Resampler(Z, P, beta, rolloff)                              # kws_resampler_create accepts it; the restatement has its bits
        assert np.array_equal(rs.table().view(np.int32), sm.speed_table(name)[0].view(np.int32)), name
        if name in sm.LARGEST:
            assert sm.table_bytes(Z, P) == sm.LARGEST[name] and sm.table_bytes(Z, P + 1) > sm.MAX_TABLE_BYTES
            with pytest.raises(ValueError):
                Resampler(Z, P + 1, beta, rolloff)
    assert sm.TABLES["ctor"] == (16, 1023, 5.0, 0.25)
    for name in sm.TABLE_GROUPS:
        g = sm.SPEED_GROUPS[name]
        assert {c.ratio for c in g.clips} == set(sm.RATIOS)
        assert {_lp(c, g.max_samples) for c in g.clips} >= set(sm.TABLE_LP)
    # the vocoder's synthesis kernel asks for the larger of its own LDS and the table
    assert sm.table_bytes(4, 32) < sm.synth_lds_bytes(256) == 21248 < sm.table_bytes(16, 1023)


def test_level_and_tiny_groups():
    g = sm.SPEED_GROUPS["level"]
    for r in {c.ratio for c in g.clips}:
        loud = [c for c in g.clips if c.ratio == r and c.kind == sm.LOUD]
        assert sorted({_lp(c, g.max_samples) for c in loud}) == list(sm.LEVEL_LP), float(r)
        for lp in sm.LEVEL_LP:
            assert {c.db for c in loud if _lp(c, g.max_samples) == lp} == set(sm.LEVEL_DB)
        assert {c.kind for c in g.clips if c.ratio == r} == {sm.LOUD, sm.SILENT, sm.QUIET}
    assert {float(c.ratio) for c in g.clips} == {0.0, float(np.float32(4.0 / 3.0)), 2.0 - 2.0 ** -23}
    x, lens, index, ratios, db = sm.speed_rows("level")
    for b, c in enumerate(g.clips):
        v = sm.speed_clip_source("level", b).astype(np.float64)
        if c.kind == sm.SILENT:
            assert not v.any()
        elif c.kind == sm.QUIET:                                         # FLT_EPSILON dominates the mean square; the gain is in the thousands
            m = np.mean(v ** 2)
            assert 0 < m < sr.EPS32 / 5 and sr.gain(v, 0.0) > 1000
        elif len(v):
            assert np.mean(v ** 2) > 0.01
    for ms in sm.TINY_MS:
        g = sm.SPEED_GROUPS["tiny%d" % ms]
        assert g.max_samples == ms
        for r in sm.TINY_RATIOS + (np.float32(0.0),):
            ls = {c.ls for c in g.clips if c.ratio == r}
            assert min(ls) < ms and ms in ls and max(ls) > ms
            q = {_lp(c, 10 ** 9) for c in g.clips if c.ratio == r}
            assert min(q) < ms < max(q) or ms in q, (ms, float(r), q)


def test_restatement_runs_on_every_speed_case():
    """speed_ref.resample's own n0 < Ls assertion holds on every case; the lengths are the formula's"""
    n = 0
    for name, g in sm.SPEED_GROUPS.items():
        x, lens, index, ratios, db = sm.speed_rows(name)
        assert x.shape[1] == g.stride and len(index) == len(g.clips) and lens.max() <= g.stride
        refs = sm.speed_expect(name)
        for c, ref in zip(g.clips, refs):
            assert len(ref["y"]) == _lp(c, g.max_samples)
            assert np.all(np.isfinite(ref["y"])) and np.isfinite(ref["g"])
            n += 1
    assert n > 1000


# ---- A. speed: non-vacuity -------------------------------------------------------------------------------------------------------------
def _neighbour(r):
    """one float32 step away, towards 1 (so it stays an accepted ratio)"""
    return np.nextafter(np.float32(r), np.float32(1.0 if r != 1 else 2.0))


def _probe_clips(name):
    """per ratio the clip with the longest output (two ratios at the default geometry, where a reference takes longest)"""
    g = sm.SPEED_GROUPS[name]
    best = {}
    for b, c in enumerate(g.clips):
        if c.ratio != 0 and (c.ratio not in best or (_lp(c, g.max_samples), c.ls) > (_lp(g.clips[best[c.ratio]], g.max_samples), g.clips[best[c.ratio]].ls)):
            best[c.ratio] = b
    picks = sorted(best.values())
    return picks[-2:] if g.max_samples == sm.DEFAULT_MS else picks


@pytest.mark.parametrize("name", list(sm.SPEED_GROUPS))
def test_a_neighbouring_ratio_or_table_index_leaves_the_bound(name):
    g = sm.SPEED_GROUPS[name]
    h, Z, P = sm.speed_table(g.table)
    refs = sm.speed_expect(name)
    worst_ratio, worst_index = 0.0, 0.0
    length_moves = any(c.ratio != 0 and sr.out_length(c.ls, _neighbour(c.ratio), g.max_samples) != sr.out_length(c.ls, c.ratio, g.max_samples)
                       for c in g.clips)
    for b in _probe_clips(name):
        c, ref = g.clips[b], refs[b]
        v = sm.speed_clip_source(name, b)
        tol = sm.speed_bound(ref)
        # (1) the reference of the neighbouring ratio
        y2, _, _ = sr.resample(v, _neighbour(c.ratio), g.max_samples, h, Z, P)
        k = min(len(y2), len(ref["y"]))
        ok = tol[:k] > 0
        if ok.any():
            worst_ratio = max(worst_ratio, float((np.abs(y2[:k] - ref["y"][:k])[ok] / tol[:k][ok]).max()))
        # (2) the first tap of a wing read one table entry on
        hd = h.astype(np.float64)
        for n in range(len(ref["y"])):
            for right in (False, True):
                j, i, eta, s = sm.first_tap(c.ratio, n, P, right)
                if tol[n] > 0 and j < len(v) and i + 2 < len(h):
                    dw = (hd[i + 1] + eta * (hd[i + 2] - hd[i + 1])) - (hd[i] + eta * (hd[i + 1] - hd[i]))
                    worst_index = max(worst_index, abs(s * dw * float(v[j])) / tol[n])
    print("%s: neighbouring ratio moves a sample by %.3g bounds, an index off by one by %.3g bounds" % (name, worst_ratio, worst_index))
    assert worst_index >= 10.0
    if name == "tiny1":                    # output 0 alone: its phase is 0 at every ratio, so no neighbouring ratio can show
        assert worst_ratio < 1.0 and not length_moves
    elif name.startswith("tiny"):          # at most three outputs: one float32 step moves the phase by 1e-7, but it moves L'
        assert length_moves
    else:
        assert worst_ratio >= 10.0


# ---- B. mix: coverage ------------------------------------------------------------------------------------------------------------------
def _voices(ms, i16):
    x, lens = sm.mix_voices(ms, i16)
    return sm.mix_f32(x), lens


@pytest.mark.parametrize("ms", sm.MIX_MS)
def test_mix_bank_is_what_the_table_says(ms):
    bank = sm.mix_bank(ms)
    want = [n for n in (1, 2, 64, 65, ms - 1, ms, ms + 1, 2 * ms + 3) if n >= 1]
    assert list(bank.seg_len[:len(want)]) == want
    for j, s in enumerate(bank.segs[:len(want)]):
        assert abs(float(s[0])) in (np.float32(0.9), np.float32(0.8)) and abs(float(s[-1])) == abs(float(s[0]))
        if len(s) > 2:
            assert np.abs(s[1:-1]).max() < 0.06
    zero, hole, quiet = (bank.segs[sm.seg(ms, k)] for k in ("zero", "hole", "quiet"))
    assert not zero.any() and len(zero) > ms
    assert not hole[ms + 16:2 * ms + 24].any() and (ms + 8) >= ms and np.abs(hole[:ms + 16]).max() > 0.5
    assert bank.names[-1] == "quiet" and bank.start[-1] >= 50000 and bank.prefix[bank.start[-1]] > 10000
    assert 0 < np.abs(quiet).max() < 1e-3
    assert bank.prefix.shape == (len(bank.samples) + 1,) and bank.start[-1] + bank.seg_len[-1] == len(bank.samples)
    single = sm.mix_bank(ms, True)
    assert list(single.seg_len) == [ms]
    x, lens = sm.mix_voices(ms, False)
    assert x.shape[1] == ms + 5 and lens.max() > x.shape[1] and lens.min() < 0 and not x[sm.SILENT_ROW].any()
    xi, _ = sm.mix_voices(ms, True)
    assert xi.dtype == np.int16 and (xi[sm.I16_MIN_ROW] == -32768).all()


@pytest.mark.parametrize("ms", sm.MIX_MS)
def test_mix_groups_hit_what_they_name(ms):
    bank = sm.mix_bank(ms)
    groups = sm.mix_groups(ms)
    v, lens = _voices(ms, False)
    tails = {k: len(c) % sm.PLAN_CLIPS_PER_BLOCK for k, c in groups.items()}
    assert tails == sm.MIX_TAILS and set(tails.values()) == {1, 2, 3} and len(groups["one"]) == 1
    e = {k: [sm.plan_expect(ms, c, v, lens) for c in cs] for k, cs in groups.items()}
    for k, cs in groups.items():                                         # every record passes kws_augment_plan's checks
        for c in cs:
            assert 0 <= c.segment < len(bank.segs) and 0 <= c.offset < bank.seg_len[c.segment] and abs(c.shift) <= sm.MAX_SHIFT
            assert abs(c.snr) <= sm.MAX_SNR_DB
    # lengths
    assert [x.lv for x in e["lengths"][:10]] == [min(n, ms) for n in (0, 1, 2, 63, 64, 65, ms - 1, ms, ms, 0)]
    assert e["lengths"][10].silent and e["lengths"][10].L == ms
    # segment against voice
    rel = {np.sign(int(bank.seg_len[c.segment]) - x.lv) for c, x in zip(groups["segment"], e["segment"])}
    assert rel == ({-1, 0, 1} if ms > 1 else {0, 1})                     # no segment is shorter than a voice of one sample
    full = [(int(bank.seg_len[c.segment]), x.L) for c, x in zip(groups["segment"], e["segment"]) if x.lv == ms]
    assert (1, 1) in full and ((2, 2) in full or ms < 2)
    if ms > 2:
        assert {s - ms for s, _ in full} >= {-1, 0, 1}
    # offsets
    off = list(zip(groups["offsets"], e["offsets"]))
    assert any(c.offset == 0 for c, x in off) and any(c.offset == bank.seg_len[c.segment] - x.L and c.offset > 0 for c, x in off)
    assert any(c.offset > x.offset for c, x in off) or ms == 1          # comes back clamped
    assert any(x.w0 + x.L == len(bank.samples) for c, x in off)          # reads prefix[total]
    # shifts
    sh = list(zip(groups["shifts"], e["shifts"]))
    for L in {x.L for c, x in sh if x.L >= 2}:
        ds = {c.shift for c, x in sh if x.L == L}
        want = {0, 1, L - 1, L, L + 1, sm.MAX_SHIFT}
        assert ds >= want | {-d for d in want}, (L, sorted(ds))
    if ms == 16000:
        for L in (16000, 15999):                                         # the fused kernel's left pad ms - L: even and odd
            ds = {c.shift for c, x in sh if x.L == L}
            assert ds >= {511, 512, 1024, -511, -512, -1024}
        assert {(ms - x.L) % 2 for c, x in sh} == {0, 1}
    assert {c.apply for c, x in sh} == {0, 1}
    # snrs
    sn = list(zip(groups["snrs"], e["snrs"]))
    assert {c.snr for c, x in sn if c.apply and not x.silent} == set(sm.MIX_SNRS)
    assert any(c.apply and x.silent and x.L == ms for c, x in sn) and any(not c.apply and c.offset > 0 for c, x in sn)
    big = max(x.gain for c, x in sn)
    assert 2.8e13 < big < 3.0e13 and np.isfinite(np.float32(big))       # |v| = 1 over silence at -200 dB: the largest gain there is
    zero_pn = [x for c, x in sn if c.apply and bank.prefix[x.w0 + x.L] == bank.prefix[x.w0] and bank.prefix[x.w0] > 0]
    assert zero_pn                                                       # a power of 0 behind a large prefix sum
    assert e["one"][0].w0 + ms == bank.start[groups["one"][0].segment] + 2 * ms + 3


def test_absurd_snr_overflows_the_float32_gain():
    """what the refusal of |SNR| > 200 dB is for: a full-scale voice over silent noise has a float32 gain of 2.9e38 at -700 dB, the last
    finite one, and an infinite one from -702 dB on"""
    with np.errstate(over="ignore"):
        assert np.isfinite(np.float32(np.sqrt(1.0 / 10.0 ** (-700.0 / 10.0) / sr.EPS32)))
        assert np.isinf(np.float32(np.sqrt(1.0 / 10.0 ** (-702.0 / 10.0) / sr.EPS32)))
    assert np.isfinite(np.float32(np.sqrt(1.0 / 10.0 ** (-200.0 / 10.0) / sr.EPS32)))


# ---- B. mix: the plan's arithmetic against its bound, and non-vacuity --------------------------------------------------------------------
@pytest.mark.parametrize("i16", [False, True])
@pytest.mark.parametrize("ms", sm.MIX_MS)
def test_plan_arithmetic_on_the_host_stays_within_the_gain_bound(ms, i16):
    """the kernel's own arithmetic (fp32 lane partials, fp64 prefix differences) restated on the host against the float64 gain"""
    bank = sm.mix_bank(ms)
    v, lens = _voices(ms, i16)
    worst = 0.0
    for k, cs in sm.mix_groups(ms).items():
        for c in cs:
            x = sm.plan_expect(ms, c, v, lens)
            if x.silent:
                continue
            g = float(sm.plan_gain_f32(v[c.row], x.L, x.w0, c.snr, bank))
            ratio = abs(g - x.gain) / (x.gain * x.bound)
            worst = max(worst, ratio)
            assert ratio <= 1.0, (ms, k, c, g, x.gain, ratio)
    print("max_samples %d, i16=%s: host restatement of the plan, largest gain error / bound = %.3g" % (ms, i16, worst))


@pytest.mark.parametrize("ms", sm.MIX_MS)
def test_mix_cases_are_not_vacuous(ms):
    bank = sm.mix_bank(ms)
    v, lens = _voices(ms, False)
    edged = {j for j, n in enumerate(bank.names) if n.startswith("e")}
    n_window = n_shift = n_len = 0
    for k, cs in sm.mix_groups(ms).items():
        for c in cs:
            x = sm.plan_expect(ms, c, v, lens)
            sl, start = int(bank.seg_len[c.segment]), int(bank.start[c.segment])
            # a window one sample off, where the window touches a segment end
            if not x.silent and c.segment in edged and (x.offset == 0 or x.offset + x.L == sl):
                moved = []
                for d in (-1, 1):
                    w = x.w0 + d
                    if 0 <= w and w + x.L <= len(bank.samples):
                        moved.append(abs(sm.np_gain(v[c.row], bank.samples, x.L, w, float(np.float32(c.snr))) - x.gain) / x.gain)
                assert max(moved) >= 1000.0 * x.bound, (ms, k, c, moved, x.bound)
                n_window += 1
            # a shift off by one
            if x.L >= 1 and v[c.row, :x.L].any() and min(abs(c.shift - 1), abs(c.shift + 1)) < x.L:
                g = np.float32(x.gain)
                ref = sm.mix_f64(v[c.row], bank.segs[c.segment], x.L, x.offset, c.shift, g, c.apply)
                far = 0.0
                for d in (-1, 1):
                    other = sm.mix_f64(v[c.row], bank.segs[c.segment], x.L, x.offset, c.shift + d, g, c.apply)
                    far = max(far, float((np.abs(other - ref) / np.maximum(sm.mix_sample_bound(ref), sm.mix_sample_bound(other))).max()))
                assert far > 1000.0, (ms, k, c, far)
                n_shift += 1
            # a clip cut one sample short or long
            vl = int(lens[c.row])
            if 0 < vl < ms and (not c.apply or sl > vl + 1):
                for d in (-1, 1):
                    cut = lens.copy()
                    cut[c.row] = vl + d
                    assert sm.plan_expect(ms, c, v, cut).L == x.L + d
                n_len += 1
    print("max_samples %d: %d windows, %d shifts, %d lengths probed" % (ms, n_window, n_shift, n_len))
    assert n_window >= 8 and n_shift >= 10 and (n_len >= 10 or ms <= 2)
