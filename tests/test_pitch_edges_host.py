"""CPU tests of tests/pitch_edge_cases.py: every case of the tempo/pitch edge table has the labels it claims, every label value the
groups are there for occurs at each transform size where it can, the plan the device makes per clip (need, Jn, Mn) is sufficient for
the first L' outputs of the float64 definition, exactly, and the refusals at the ends of the accepted ranges need no device.  From the
restatements and the library's host side alone."""
import ctypes
import os

import numpy as np
import pytest

import pitch_edge_cases as pe
import pitch_ref as pf
import speed_mix_cases as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
F32 = np.float32


def _all_clips(N=None):
    for call in pe.calls().values():
        if N is None or call.N == N:
            sl = pe.call_slots(call)
            for clip in call.clips:
                yield call, clip, pe.labels(call, clip, sl)


# ---- the restated constants and arithmetic -----------------------------------------------------------------------------------------------
def test_restated_constants_and_slots_are_the_librarys():
    from kws_amd import lib as l
    from kws_amd.augment import pitch_workspace_bytes
    src = open(os.path.join(ROOT, "tf-keras-speech-commands_amd", "csrc", "kws_pitch.hip")).read()
    assert "kMaxSamples = 1 << 20" in src and "kMaxZ = %d" % pe.KMAX_Z in src and l.PITCH_MAX_SAMPLES == pe.KMAX_SAMPLES
    assert src.count("32768") >= 4 and "b0 += 32768" in src and "fit < 32768 ? (int)fit : 32768" in src and pe.TILE_CEILING == 32768
    assert "G = kPoints / Nc" in src and "kPoints = 1024" in src
    for N in pf.N_FFTS:
        H, G = pe.geometry(N)
        assert G == 1024 // (N // 2) and G * H == pe.CHUNK
        for ms in (1, 8, 383, 1024, 16000, pe.KMAX_SAMPLES):
            assert pe.slots(N, ms).clip_bytes == pitch_workspace_bytes(N, ms, 1), (N, ms)
    # the 1 s clip of DESIGN.md section 21: 469 KB for tempo 0.85 .. 1.2 and +-2 semitones, 2.2 MB at the ranges' ends
    t, lo, hi = pe.call_ranges([0.85, 1.2], [-2.0, 2.0])
    assert 468e3 < pe.slots(512, 16000, t / lo, hi, 16).clip_bytes < 470e3 and 2.1e6 < pe.slots(512, 16000).clip_bytes < 2.3e6
    assert pe.call_ranges([0.0, 0.6], [NAN, NAN]) == (1.0, 1.0, 1.0) and pe.call_ranges([2.0], [-12.0]) == (2.0, 0.5, 1.0)
    # F: 32768 slots at max_samples 8; the call's own ranges are narrower, so the workspace holds the ceiling of 32768 clips a tile
    assert pe.slots(256, pe.BATCH_MS).clip_bytes * pe.TILE_CEILING == 486539264 < 1 << 30
    assert pe.call_slots(pe.group("F")[0]).clip_bytes <= pe.slots(256, pe.BATCH_MS).clip_bytes
    # I: the table against the vocoder's LDS
    assert sm.table_bytes(4, 32) < sm.synth_lds_bytes(512) < sm.synth_lds_bytes(1024) == 32768 == sm.table_bytes(16, 512) - 4
    # G: 3 G + 1 and 4 G + 1 frames give a block a second group of frames
    for N in pf.N_FFTS:
        _, G = pe.geometry(N)
        fc = pe.frame_counts(N)
        assert {1, G, G + 1, 2 * G, 2 * G + 1, 3 * G + 1, 4 * G + 1} <= set(fc) and max(G - 1, 1) in fc
        assert [pe.frame_blocks(f, N) for f in (G, G + 1, 2 * G + 1, 3 * G + 1, 4 * G + 1)] == [1, 1, 2, 2, 3]
        stride, lens = pe.frame_clips(N)
        assert [pf.n_frames(n, N) for n in lens] == sorted({1, max(G - 1, 1), G, G + 1, 2 * G + 1, 3 * G + 2}) and max(lens) <= stride


def test_smallest_shifts_with_a_ratio_other_than_one():
    up, down = pe.smallest_shift(1), pe.smallest_shift(-1)
    assert up.dtype == down.dtype == np.float32 and up > 0 > down
    assert pf.ratio(up) == np.nextafter(F32(1), F32(2)) and pf.ratio(np.nextafter(up, F32(0))) == 1
    assert pf.ratio(down) == np.nextafter(F32(1), F32(0)) and pf.ratio(np.nextafter(down, F32(0))) == 1
    # 2^(n / 12) leaves 1 by half a float32 step: 12 2^-24 / ln 2 upwards, 12 2^-25 / ln 2 downwards
    assert abs(float(up) - 12 * 2.0 ** -24 / np.log(2)) < 1e-12 and abs(float(down) + 12 * 2.0 ** -25 / np.log(2)) < 1e-12
    for n in (0.0, -0.0, 1e-7):
        assert pf.ratio(n) == 1 and pf.rho(0.0, n) == 1.0
        assert pf.out_length(1100, 0.0, n, 1024) == 1024 and pf.out_length(777, 0.0, n, 1024) == 777      # min(Ls, max_samples)


# ---- labels and coverage -----------------------------------------------------------------------------------------------------------------
def test_every_case_has_the_labels_it_claims():
    n = 0
    for call, clip, lab in _all_clips():
        for k, v in clip.claims.items():
            assert lab[k] == v, (call.name, clip, k, lab[k])
            n += 1
        p = pe.clip_plan(call, clip)
        assert lab["lo"] == p.lo == (min(clip.ls, call.max_samples) if not p.vocoded else
                                     pf.out_length(clip.ls, clip.tempo, clip.semis, call.max_samples)), (call.name, clip)
        assert clip.ls <= call.stride and 0 <= p.Mn <= p.M and p.Jn <= p.Jtot
    big = pe.largest_call()
    assert pe.labels(big, big.clips[0])["lo"] == pe.KMAX_SAMPLES and pe.clip_plan(big, big.clips[0]).Jn == 16385
    assert n > 300


@pytest.mark.parametrize("N", pf.N_FFTS)
def test_every_label_value_occurs_where_it_can(N):
    H, G = pe.geometry(N)
    every = list(_all_clips(N))
    # B: need + N / 2 one below, on and one above a multiple of 512, for k = 1 and 2.  At N = 1024, k 512 - N / 2 is 0 for k = 1, and
    # max_samples of -1 and 0 do not exist: only "one above" (max_samples 1) is possible there, and the table goes on to k = 3.
    got = {(lab["chunks"], lab["chunk_mod"]) for call, clip, lab in every if call.group == "B" and "chunk" in call.name}
    ks = (1, 2) if N < 1024 else (2, 3)
    assert got >= {(k, 511) for k in ks} | {(k, 0) for k in ks} | {(k + 1, 1) for k in ks}
    if N == 1024:
        assert (2, 1) in got and pe.CHUNK_MS[N][0] == 1
    for call, clip, lab in every:
        if call.group == "B" and "chunk" in call.name:
            p = pe.clip_plan(call, clip)
            assert p.need == p.lo == call.max_samples <= p.Lst and p.Jn < p.Jtot and p.Mn < p.M
    # B: the source ends inside the output, Jn == Jtot at every residue mod G: 0 .. G - 1 zero-filled frames in the last chunk
    res = {lab["jn_mod_g"] for call, clip, lab in every if "residues" in call.name and not lab["jn_lt_jtot"] and lab["lo"] < call.max_samples}
    assert res == set(range(G))
    assert max(lab["chunks"] for call, clip, lab in every if "residues" in call.name) >= 2
    # over the whole table
    voc = [(call, clip, lab) for call, clip, lab in every if lab["vocoded"] and lab["lo"] > 0]
    for key in ("jn_lt_jtot", "mn_lt_m", "at_need_cap", "at_mn_cap", "resampled"):
        assert {lab[key] for _, _, lab in voc} == {False, True}, key
    assert {lab["jn_mod_g"] for _, _, lab in voc} == set(range(G))
    advs = {lab["adv"] for _, _, lab in voc}
    assert advs >= {frozenset([0, 1]), frozenset([1]), frozenset([2]), frozenset([4]), frozenset([1, 2])}
    assert {frozenset([0, 1]), frozenset([1, 2]), frozenset([2])} <= {lab["adv_class"] for _, _, lab in voc}
    # a clip of no samples and a clip of no outputs
    assert any(clip.ls == 0 for _, clip, _ in every) and any(lab["vocoded"] and lab["lo"] == 0 for _, _, lab in every)
    # C: r == 1.0f through a shift is vocoded at rho = 1 and not resampled
    flat = [(clip, lab) for call, clip, lab in every if call.group == "C" and clip.tempo == 0 and not np.isnan(clip.semis) and abs(clip.semis) < 2e-7]
    assert len(flat) == 6 and all(lab["vocoded"] and not lab["resampled"] and lab["lo"] == pe.MS for _, lab in flat)
    assert {float(clip.semis) for clip, _ in flat} == {0.0, float(F32(1e-7))} and any(np.signbit(clip.semis) for clip, _ in flat)
    near = [lab for call, clip, lab in every if call.group == "C" and not np.isnan(clip.semis) and 2e-7 < abs(clip.semis) < 2e-6]
    assert len(near) == 4 and all(lab["resampled"] for lab in near)
    tempos = {float(clip.tempo) for call, clip, _ in every if call.group == "C"}
    assert tempos >= {0.5 + 2.0 ** -24, 1.0 - 2.0 ** -24, 1.0, 1.0 + 2.0 ** -23, 2.0 - 2.0 ** -23, 0.5, 2.0}
    rhos = {pe.clip_plan(call, clip).rho for call, clip, _ in every if call.group == "C"}
    assert rhos >= {4.0, 0.25, 2.0, 0.5, 1.0, 1.25}


@pytest.mark.parametrize("N", pf.N_FFTS)
def test_cap_calls(N):
    cap = [c for c in pe.group("D") if c.N == N and "caps" in c.name][0]
    sl = pe.call_slots(cap)
    a, b, c = (pe.clip_plan(cap, clip, sl) for clip in cap.clips)
    t, r_min, r_max = pe.call_ranges([k.tempo for k in cap.clips], [k.semis for k in cap.clips])
    assert a.need == sl.need_max and a.r == r_max and a.need < a.Lst and a.Mn < sl.mn_max
    assert b.Mn == sl.mn_max and b.rho == t / r_min and b.Jn == sl.jn_max and b.need < sl.need_max and b.Mn <= b.M
    assert c.need < sl.need_max // 4 and c.Mn < sl.mn_max // 4
    # the call's own slot is smaller than the one the workspace is sized by
    assert sl.clip_bytes < pe.slots(N, cap.max_samples).clip_bytes
    split = [c for c in pe.group("D") if c.N == N and "split" in c.name][0]
    sl = pe.call_slots(split)
    t, r_min, r_max = pe.call_ranges([k.tempo for k in split.clips], [k.semis for k in split.clips])
    assert (t, r_min) == (2.0, 0.5) and split.clips[0].tempo == 2.0 and split.clips[1].semis == -12.0
    assert all(pe.clip_plan(split, k, sl).rho < t / r_min for k in split.clips)            # no clip has the call's rho_max
    wide = pe.call_ranges([k.tempo for k in split.clips] + [w[0] for w in pe.WIDEST], [k.semis for k in split.clips] + [w[1] for w in pe.WIDEST])
    assert wide == (2.0, 0.5, 2.0)


def test_tile_and_batch_groups():
    tempo, semis = pe.tile_values()
    assert (tempo != 0).any() and (tempo == 0).any() and np.isnan(semis).any() and (~np.isnan(semis)).any()
    assert ((tempo == 0) & np.isnan(semis)).any()                                          # a clip left as it is among the drawn ones
    assert set(pe.TILE_INDEX) == set(range(9)) and len(pe.TILE_INDEX) == 24 and list(pe.TILE_INDEX) != sorted(pe.TILE_INDEX)
    assert min(pe.TILE_LENS) == -5 and max(pe.TILE_LENS) == pe.STRIDE + 100
    assert list(pe.tile_lens()) == [0, 0, 63, pe.STRIDE, 65, 255, 256, 1000, 777]
    f = pe.group("F")[0]
    assert len(f.clips) == 96 and len({(pe.batch_clip(b)) for b in range(96)}) == 96
    assert all(pe.batch_clip(b) == pe.batch_clip(b % 96) for b in (96, 32768, 65535))
    labs = [pe.labels(f, c) for c in f.clips]
    assert {l["vocoded"] for l in labs} == {False, True} and {l["resampled"] for l in labs} == {False, True}
    assert {l["lo"] for l in labs} >= {0, 1, 4, 7, pe.BATCH_MS}
    # 32769 clips walk as two tiles of 16385, 65536 as two of exactly 32768
    for B, want in zip(pe.BATCH_SIZES, (16385, 32768)):
        n_tiles = (B + pe.TILE_CEILING - 1) // pe.TILE_CEILING
        assert n_tiles == 2 and (B + n_tiles - 1) // n_tiles == want


# ---- the plan is sufficient --------------------------------------------------------------------------------------------------------------
_SPARE = {"Mn": 0, "Jn": 0, "clips": 0}


def _sufficient(call, spare=True):
    """every distinct clip of the call: the planned part of the vocoder gives the first L' outputs of the whole one, exactly"""
    tab = sm.speed_table(call.table or "default")
    h, Z, P = tab
    sl = pe.call_slots(call)
    rng = np.random.default_rng(len(call.name))
    seen = set()
    for clip in call.clips:
        key = (clip.ls, float(clip.tempo), repr(float(clip.semis)))
        p = pe.clip_plan(call, clip, sl)
        if key in seen or not p.vocoded:
            continue
        seen.add(key)
        v = 0.3 * rng.standard_normal(clip.ls)
        D = pf.stft(v, call.N)[0]
        full = pf.perturb(v, clip.tempo, clip.semis, call.max_samples, call.N, h, Z, P, D=D)["y"]
        got = pe.perturb_planned(D, p, call.N, tab)
        assert len(got) == len(full) == p.lo == pf.out_length(clip.ls, clip.tempo, clip.semis, call.max_samples), (call.name, clip)
        assert np.array_equal(got, full), (call.name, clip, p)
        if spare and p.lo > 0:                               # recorded, not asserted: is the plan tight?
            _SPARE["clips"] += 1
            _SPARE["Mn"] += p.Mn > 1 and np.array_equal(pe.perturb_planned(D, p, call.N, tab, Mn=p.Mn - 1), full)
            _SPARE["Jn"] += p.Jn > 1 and np.array_equal(pe.perturb_planned(D, p, call.N, tab, Jn=p.Jn - 1), full)


@pytest.mark.parametrize("g", "ABCDEFHI")
def test_the_plan_is_sufficient(g):
    before = dict(_SPARE)
    for call in pe.group(g):
        _sufficient(call)
    print("group %s: of %d clips, one analysis frame fewer would do for %d and one output frame fewer for %d"
          % (g, _SPARE["clips"] - before["clips"], _SPARE["Mn"] - before["Mn"], _SPARE["Jn"] - before["Jn"]))


def test_the_plan_is_sufficient_at_the_largest_max_samples():
    _sufficient(pe.largest_call(1 << 18), spare=False)       # the arithmetic of 1 << 20 at a quarter of its cost
    big = pe.largest_call()
    p = pe.clip_plan(big, big.clips[0])
    print(p)
    assert (p.lo, p.need, p.Jn, p.Jtot, p.M) == (1 << 20, 1 << 20, 16385, 16385, 32769)


# ---- refusals without a device -----------------------------------------------------------------------------------------------------------
def test_refusals_at_the_ends_of_the_ranges_need_no_device():
    import kws_amd
    from kws_amd import lib as l
    from kws_amd.augment import WaveAugment
    L = l.get_lib()
    aug = WaveAugment(None, tempo=(0.9, 1.1), pitch=(-2, 2), pitch_n_fft=256, seed=1)
    rs = aug.resampler.handle()
    B, stride, fake = 2, 1100, 4096                          # device pointers that no check dereferences

    def call(ms=1024, ext=None, exs=None, ws_bytes=1000):
        p = aug.pitch_params(ms)
        rc = L.kws_pitch_apply(rs, ctypes.byref(p), fake, l.WAV_F32, None, B, stride, None, 0, 0, None if ext is None else ext.ctypes.data,
                               None if exs is None else exs.ctypes.data, fake + 1, max(ms, 1 << 21), fake, fake, fake, fake, ws_bytes, None)
        return rc, L.kws_last_error().decode()

    n = ctypes.c_size_t(7)
    assert L.kws_pitch_workspace_bytes(256, pe.KMAX_SAMPLES + 1, 1, ctypes.byref(n)) == l.ERR_UNSUPPORTED and n.value == 0
    assert L.kws_pitch_workspace_bytes(256, pe.KMAX_SAMPLES, 1, ctypes.byref(n)) == 0 and n.value == pe.slots(256, pe.KMAX_SAMPLES).clip_bytes
    assert call(ms=pe.KMAX_SAMPLES + 1)[0] == l.ERR_UNSUPPORTED
    # a workspace of 1000 bytes is refused after every check of the values and before the device is asked for: "holds no clip" means
    # that the values passed
    passed = lambda r: r[0] == l.ERR_WORKSPACE and "holds no clip" in r[1]
    assert passed(call()) and passed(call(ms=pe.KMAX_SAMPLES))
    f = lambda a, b: np.full(B, np.nextafter(F32(a), F32(b)), np.float32)
    for bad in (f(0.5, 0), f(2, 3)):
        rc, msg = call(ext=bad)
        assert rc == l.ERR_INVALID and "tempo" in msg, (bad, rc, msg)
    for good in (f(0.5, 1), f(2, 0), np.full(B, 0.5, np.float32), np.full(B, 2.0, np.float32), f(1, 0), f(1, 2)):
        assert passed(call(ext=good)), good
    for bad in (f(12, 13), f(-12, -13)):
        rc, msg = call(exs=bad)
        assert rc == l.ERR_INVALID and "semitones" in msg, (bad, rc, msg)
    for good in (f(12, 0), f(-12, 0), np.full(B, 12.0, np.float32), np.full(B, -12.0, np.float32), np.full(B, -0.0, np.float32),
                 np.full(B, pe.smallest_shift(-1), np.float32)):
        assert passed(call(exs=good)), good
    if kws_amd.device_count() == 0:                          # with a workspace that holds a clip they fail only for want of a device
        for kw in (dict(ext=f(0.5, 1)), dict(ext=f(2, 0)), dict(exs=f(12, 0))):
            rc, msg = call(ws_bytes=1 << 30, **kw)
            assert rc == l.ERR_HIP and "hip" in msg.lower(), (kw, rc, msg)
