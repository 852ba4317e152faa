"""CPU tests of the wave-edge case table (tests/wave_edge_cases.py): that the restated geometry rules reach every chunk size and every
boundary the table names, that the float64 references hold against scipy and np.convolve at those lengths, and that no case is vacuous:
a dry copy, a dropped or an extra tap, or an odd extension around the wrong sample would miss its bound by a factor of 1000.  All of
it is decided here, from the table and the references alone."""
import numpy as np
import pytest

import wave_edge_cases as wc
from filter_ref import filtfilt_batch
from reverb_ref import DIRECT_LIMIT, keep_energy_scale, np_reverb_fft
from test_filter_gpu import FILT_TOL
from test_reverb_gpu import CONV_TOL, np_reverb

MARGIN = 1000.0


# ---- the geometry rules and the table ------------------------------------------------------------------------------------------------
def test_chunk_rule_and_boundary_cases():
    assert [wc.chunk_log(n) for n in (1, 2, 256, 257, 512, 513, 8192, 8193, 16384)] == [2, 2, 2, 3, 3, 4, 7, 8, 8]
    assert wc.FILTER_MAX_SAMPLES + 2 * wc.FILTER_MAX_PADLEN == wc.LANES << wc.MAX_LOG
    seen = set()
    for p, lv, lpad, m, what in wc.CHUNK_CASES:
        assert lv + 2 * p == lpad and wc.chunk_log(lpad) == m, (p, lv, lpad, m)
        assert 1 <= lv <= wc.FILTER_MAX_SAMPLES
        lane, count = wc.last_lane(lpad)
        if what == "every lane full":
            assert lpad == wc.LANES << m and (lane, count) == (63, 1 << m)
        elif what.startswith("one sample past"):
            assert lpad == (wc.LANES << (m - 1)) + 1 and (lane, count) == (32, 1)
        elif what == "last lane holds one sample":
            assert (lane, count) == (63, 1)
        elif what == "last lane empty":
            assert (lane, count) == (62, 1 << m)
        elif what == "dry":
            assert lv == p
        else:
            assert lv == p + 1
        seen.add((p, m, what))
    for p in wc.CHUNK_PADLENS:
        for m in range(2, 8):                                            # each side of each boundary, for every padlen
            assert (p, m, "every lane full") in seen
            assert any(s[:2] == (p, m + 1) and s[2].startswith("one sample past") for s in seen)
        for m in (2, 5, 8):
            assert (p, m, "last lane holds one sample") in seen and (p, m, "last lane empty") in seen
    assert (32, 8, "every lane full") in seen                            # lpad = 16384
    assert (1, 2, 4, 2, "shortest wet clip") in wc.CHUNK_CASES and wc.last_lane(4) == (0, 4)       # padlen 1, Lv = 2: lane 0 alone
    assert {c[3] for c in wc.CHUNK_CASES} == set(range(2, 9))


def test_banks_have_the_intended_sections_and_padlens():
    for name, (specs, forced) in wc.BANKS.items():
        bank = wc.make_bank(name)
        assert bank.n_sections == wc.N_SECTIONS[name] == max(wc.spec_sections(s) for s in specs)
        if bank.n_sections > 1:                                          # a design padded with identity sections
            assert min(wc.spec_sections(s) for s in specs) < bank.n_sections
            assert np.array_equal(bank.table[int(np.argmin([wc.spec_sections(s) for s in specs])), -1], [1.0, 0, 0, 1.0, 0, 0])
        else:                                                            # one section: a first-order design (b2 = a2 = 0) instead
            assert min(s[1] for s in specs) == 1
        assert list(bank.padlen) == wc.bank_padlens(name)
        if forced is not None:
            assert set(bank.padlen) == {forced}
    assert [wc.make_bank(n).n_sections for n in wc.SECTION_GROUPS] == [1, 2, 3, 4]
    assert set(wc.make_bank("PAD32").padlen) == {wc.FILTER_MAX_PADLEN} and set(wc.make_bank("PAD1").padlen) == {1}
    assert set(wc.CHUNK_PADLENS) <= set(wc.bank_padlens("S4")) | {1, 32}


def test_filter_groups_hold_the_cases_they_name():
    for name in wc.SECTION_GROUPS:                                       # Lv = padlen and padlen + 1 of every design
        g = wc.FILTER_GROUPS[name]
        for k, p in enumerate(wc.bank_padlens(name)):
            assert (k, p) in g.clips and (k, p + 1) in g.clips
        assert any(k < 0 for k, _ in g.clips) and any(lv > g.max_samples for _, lv in g.clips)
    for name, (bank, ps) in wc.CHUNK_GROUPS.items():                     # every boundary case is a clip of its padlen's group
        g, pads = wc.FILTER_GROUPS[name], wc.bank_padlens(bank)
        assert g.max_samples == wc.FILTER_MAX_SAMPLES
        have = {(pads[k], lv) for k, lv in g.clips}
        assert have == {(c[0], c[1]) for c in wc.CHUNK_CASES if c[0] in ps}
    assert sorted(p for _, ps in wc.CHUNK_GROUPS.values() for p in ps) == sorted(wc.CHUNK_PADLENS)
    for ms, names in wc.MS_GROUPS.items():
        for name in names:
            g = wc.FILTER_GROUPS[name]
            pads = wc.bank_padlens(g.bank)
            assert g.max_samples == ms and g.stride > ms
            assert any(lv > ms for _, lv in g.clips) and any(lv >= g.stride for _, lv in g.clips)
            wet = [(k, lv) for k, lv in g.clips if wc.filter_choice(k, wc.clipped_len(lv, g.stride, ms), pads) >= 0]
            assert bool(wet) == (name not in wc.ALL_DRY_GROUPS)
            if wet:                                                      # a wet clip that max_samples cuts
                assert any(lv > ms for _, lv in wet)
    g = wc.FILTER_GROUPS["ms28"]
    assert (2, 28) in g.clips and wc.bank_padlens("S4")[2] == 27 and 28 + 2 * 27 == 82
    g = wc.FILTER_GROUPS["ms16320_p32"]
    assert g.clips[0] == (0, 16320) and 16320 + 2 * 32 == 16384 and wc.chunk_log(16384) == 8


def test_reverb_groups_hold_the_cases_they_name():
    n_long = 0
    for bank_ms, ms in [(m, m) for m in wc.REVERB_MS] + list(wc.REVERB_MIXED):
        g = wc.reverb_group(bank_ms, ms)
        eff = min(bank_ms, ms)
        lens = [wc.clipped_len(v, g.stride, ms) for v in g.valid_len]
        assert {0, 1, min(2, ms), ms} <= set(lens) and ms + 5 in g.valid_len and g.stride == ms + 5
        if ms > 3:
            assert ms - 1 in lens and any(1 < v < ms - 1 and v % 2 for v in lens)
        if ms > wc.REVERB_DIRECT + 1:                                    # each side of the kernel's direct / transform switch
            assert {wc.REVERB_DIRECT, wc.REVERB_DIRECT + 1} <= set(lens)
        rir_lens = [len(h) for h in g.rirs]
        assert {1, 2, 3, bank_ms, bank_ms + 500} <= set(rir_lens) and (bank_ms == 1 or bank_ms - 1 in rir_lens)
        for h in g.rirs:                                                 # peak first: RirBank leaves them as they are
            assert h.dtype == np.float32 and h[0] == 1.0 and np.abs(h[1:]).max(initial=0.0) < 1.0
        h = g.rirs[g.loud]
        assert len(h) == max(rir_lens) and abs(h[eff - 1]) >= 0.5 and abs(h[eff]) >= 0.5
        sums = set()
        for r, k in g.pairs:
            if k >= 0 and lens[r] > 0:
                sums.add(lens[r] + len(wc.bank_taps(g.rirs[k], bank_ms)) - 1)
        assert ms in sums
        if ms >= 2:
            assert ms - 1 in sums and ms + 1 in sums
        ks = {k for _, k in g.pairs}
        assert ks == set(range(-1, len(g.rirs)))
        assert (wc.SILENT_ROW, g.loud) in g.pairs and g.valid_len[wc.SILENT_ROW] > 0
        n_long += len(wc.long_pairs(g))
    assert 8 <= n_long <= 16
    assert len(wc.long_pairs(wc.reverb_group(16384, 16384))) == 4        # among them 16384 x 16384: all eight input registers live


def test_rir_bank_keeps_the_table_rirs_and_checks_max_samples():
    from kws_amd.augment import RirBank
    for bank_ms, ms in [(m, m) for m in wc.REVERB_MS] + list(wc.REVERB_MIXED):
        g = wc.reverb_group(bank_ms, ms)
        bank = RirBank(list(g.rirs), max_samples=bank_ms)
        assert bank.max_samples == bank_ms and len(bank) == len(g.rirs)
        for h, t in zip(g.rirs, bank.taps):
            assert t.dtype == np.float32 and np.array_equal(t, wc.bank_taps(h, bank_ms))
    h = [np.r_[1.0, 0.5].astype(np.float32)]
    for bad in (wc.REVERB_MAX_SAMPLES + 1, 0):
        with pytest.raises(ValueError):
            RirBank(h, max_samples=bad)
    assert RirBank(h, max_samples=wc.REVERB_MAX_SAMPLES).max_samples == 16384


# ---- the references --------------------------------------------------------------------------------------------------------------------
def test_filtfilt_restatement_matches_scipy_at_the_boundary_lengths():
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(0)
    # one design per section count at its own padlen, and the forced padlens
    designs = [("S1", 0, None), ("S2", 2, None), ("S3", 1, None), ("S4", 4, None), ("PAD32", 1, 32), ("PAD1", 0, 1)]
    sos, clips, pads = [], [], []
    for name, k, forced in designs:
        bank = wc.make_bank(name)
        p = int(bank.padlen[k])
        assert forced is None or p == forced
        lens = {c[1] for c in wc.CHUNK_CASES if c[0] == p and c[4] != "dry" and c[1] <= 2100} | {p + 1, 256 - 2 * p, 257 - 2 * p, 2100}
        for lv in sorted(lens):
            v = 0.3 * rng.standard_normal(lv) + np.linspace(-0.2, 0.4, lv)
            sos.append(bank.sos[k]), clips.append(v), pads.append(p)
    got = filtfilt_batch(sos, clips, pads)
    for s, v, p, y in zip(sos, clips, pads, got):
        want = signal.sosfiltfilt(s, v, padtype="odd", padlen=p)
        err = np.abs(y - want).max() / np.abs(v).max()
        assert y.shape == v.shape and err <= 1e-9, (len(v), p, err)       # test_filter_host.py's tolerance against scipy
    assert len(clips) > 40


def test_fft_reference_matches_np_convolve():
    rng = np.random.default_rng(1)
    assert DIRECT_LIMIT == 4000 * 4000
    for lv, lh, ms in ((1, 1, 1), (1, 3, 3), (2, 1, 2), (5, 3, 6), (333, 1000, 1000), (1000, 1500, 1000), (4000, 4000, 16384),
                       (4000, 4000, 5000), (3999, 17, 4001), (2731, 4000, 8193)):
        v = (0.3 * rng.standard_normal(lv)).astype(np.float32)
        h = (0.3 * rng.standard_normal(lh) * np.exp(-np.arange(lh) / 2000.0)).astype(np.float32)
        h[0] = 1.0
        y, _ = np_reverb(v, h, ms, False)
        z, one = np_reverb_fft(v, h, ms, False)
        assert y.shape == z.shape and one == 1.0 and len(y) == wc.reverb_len_out(lv, min(lh, ms), ms)
        bound = 1e-12 * np.linalg.norm(v.astype(np.float64)) * np.linalg.norm(h.astype(np.float64))
        assert np.abs(y - z).max() <= bound, (lv, lh, ms, np.abs(y - z).max(), bound)
        s, t = np_reverb(v, h, ms, True)[1], np_reverb_fft(v, h, ms, True)[1]
        assert t == keep_energy_scale(v, z) and np.array_equal(np_reverb_fft(v, h, ms, True)[0], z * t)
        assert abs(s - t) <= 2.0 ** -23 * t                              # np_reverb's scale comes out a float32, this one is a float64
    assert np_reverb_fft(np.zeros(0, np.float32), np.ones(3, np.float32), 8, True)[0].shape == (0,)


# ---- no case is vacuous ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(wc.FILTER_GROUPS))
def test_wet_filter_cases_are_far_from_a_dry_copy(group):
    g = wc.FILTER_GROUPS[group]
    e = wc.filter_expect(group, False)
    x, lens, ex = wc.filter_source(group, False)
    xt = wc.filter_source(group, False, tight=True)[0]
    assert xt.shape[1] == g.max_samples and np.array_equal(xt, x[:, :g.max_samples])
    n_wet = 0
    for b, (v, u, y) in enumerate(zip(e.clips, e.used, e.ref)):
        assert len(v) == wc.clipped_len(lens[b], g.stride, g.max_samples) == wc.clipped_len(lens[b], g.max_samples, g.max_samples)
        if y is None:
            assert u == -1
            continue
        n_wet += 1
        assert y.shape == v.shape and np.all(np.isfinite(y))
        assert np.abs(y - v).max() >= MARGIN * FILT_TOL * np.abs(v).max(), (group, b, len(v))
    assert (n_wet == 0) == (group in wc.ALL_DRY_GROUPS)


@pytest.mark.parametrize("group", [n for names in wc.MS_GROUPS.values() for n in names if n not in wc.ALL_DRY_GROUPS])
def test_cut_filter_cases_tell_the_clips_end_from_the_cut(group):
    """the odd extension mirrors around v[max_samples - 1]: filtering the whole clip and cutting afterwards is another signal"""
    g = wc.FILTER_GROUPS[group]
    bank = wc.make_bank(g.bank)
    e = wc.filter_expect(group, False)
    x, lens, _ = wc.filter_source(group, False)
    cut = [b for b, u in enumerate(e.used) if u >= 0 and min(int(lens[b]), g.stride) > g.max_samples]
    assert cut
    whole = filtfilt_batch([bank.sos[e.used[b]] for b in cut], [x[b, :min(int(lens[b]), g.stride)] for b in cut],
                           [int(bank.padlen[e.used[b]]) for b in cut])
    for b, y in zip(cut, whole):
        v = e.clips[b]
        assert len(v) == g.max_samples
        assert np.abs(y[:g.max_samples] - e.ref[b]).max() >= MARGIN * FILT_TOL * np.abs(v).max(), (group, b)


@pytest.mark.parametrize("bank_ms,ms", [(m, m) for m in wc.REVERB_MS] + list(wc.REVERB_MIXED))
@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
def test_reverb_loud_taps_are_heard_and_not_heard(i16, bank_ms, ms):
    g = wc.reverb_group(bank_ms, ms)
    eff = min(bank_ms, ms)
    x = wc.reverb_source(bank_ms, ms, i16)[0]
    e = wc.reverb_expect(bank_ms, ms, i16)
    rows = [j for j, (r, k) in enumerate(g.pairs) if k == g.loud and len(e.clips[j]) > 0 and r != wc.SILENT_ROW]
    assert len(rows) >= 3
    sub = g._replace(pairs=tuple(g.pairs[j] for j in rows))
    without = list(g.rirs)
    without[g.loud] = g.rirs[g.loud].copy()
    without[g.loud][eff - 1] = 0.0
    dropped = wc.reverb_expect_from(sub, x, without)
    beyond = list(g.rirs)
    beyond[g.loud] = g.rirs[g.loud].copy()
    beyond[g.loud][eff] = 0.0
    same = wc.reverb_expect_from(sub, x, beyond)
    for i, j in enumerate(rows):
        v, h, y = e.clips[j], e.taps[j], e.ref[j]
        assert len(h) == min(len(g.rirs[g.loud]), bank_ms) and len(y) == e.length[j] >= eff
        bound = CONV_TOL * np.linalg.norm(v.astype(np.float64)) * np.linalg.norm(h.astype(np.float64))
        assert np.abs(dropped.ref[i] - y).max() >= MARGIN * bound, (len(v), np.abs(dropped.ref[i] - y).max(), bound)
        assert np.array_equal(same.ref[i], y) and same.scale[i] == e.scale[j]
        if bank_ms < ms and len(v) + bank_ms <= ms:                      # the tap the bank drops would reach the output
            heard = np_reverb(v, g.rirs[g.loud][:bank_ms + 1], ms, False)[0]
            assert np.abs(heard - np.r_[y, np.zeros(len(heard) - len(y))]).max() >= MARGIN * bound
    if bank_ms < ms:
        assert any(len(e.clips[j]) + bank_ms <= ms for j in rows)
    for j, (r, k) in enumerate(g.pairs):                                 # the silent clip: a zero reference and a zero scale
        if r == wc.SILENT_ROW:
            assert not e.clips[j].any() and len(e.clips[j]) > 0
            if k >= 0:
                assert not e.ref[j].any() and e.scale[j] == 0.0
