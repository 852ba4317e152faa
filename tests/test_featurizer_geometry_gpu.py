"""The three featurizer kernels off the default frame geometry, against the float64 oracle (oracle/featurizer_oracle.py).

featurize_fft1024_v3_kernel (csrc/kws_featurize_v3.h) serves every buffer length at the default window, hop, band and coefficient
counts, deals its frames to waves by a cost loop over the batch size and the device's compute units (launch_v3,
csrc/kws_featurize.hip) and finishes three frames at a time; featurize_fft1024_kernel takes every other n_fft = 1024 geometry,
featurize_generic_kernel every other n_fft; kws_featurize_long cuts recordings into 256-frame segments for the latter two.  The
rest of the suite runs the first at 30 frames only (a multiple of 3), the second where no wave is ever idle, and the segment path
not at all.  tests/geometry_cases.py holds the rows, the restated dispatch rules and the batch sizes (from the device's
compute-unit count) that hit each job shape; tests/test_geometry_host.py holds that table against the rules.

Every batch is made of the row's twelve base clips (noise at 0.1 of full scale on int16 steps, ragged valid lengths: 0, 1, odd,
window - 1, window, max_samples, above the stride, ...) at an odd row stride, so every clip of every batch has an oracle result,
every second row starts on an odd element (no two-sample loads), and every output goes to a buffer pre-filled with a sentinel.
Tolerances are the suite's own: 2e-4 for clip features, twice that for delta columns, 3e-4 for raw and long rows.

Measured on an MI355X (256 compute units).  Batch sizes with the frames per job (fpw) and jobs per clip (jpc) of the stand-alone form
and, in brackets, of the shared-CU form, then the largest error against the oracle over all batch sizes and both input types -- on the
tuned rows that is 4.4e-6 at the c0 of all-zero frames, float32's rounding of log(eps) = -36.04, so the largest error of frames above
the log floor follows it:
  tuned-2    B 1, 4096: 2, 1 [2, 1]                                                                  4.4e-6, 1.6e-6
  tuned-14   B 1: 3, 5 [3, 5]; 819: 3, 5 [5, 3]; 820: 4, 4 [5, 3]; 2731: 14, 1 [14, 1]               4.4e-6, 1.6e-6
  tuned-61   B 1: 3, 21 [3, 21]; 195: 3, 21 [5, 13]; 196: 4, 16 [5, 13]; 3511: 61, 1 [13, 5]         4.4e-6, 1.8e-6
  tuned-45   B 1: 3, 15 [3, 15]; 273: 3, 15 [5, 9]; 274: 4, 12 [5, 9]; 3277: 45, 1 [9, 5]            4.4e-6, 2.1e-6
  gen1-9     B 1, 4: 3, 3 (two and three idle waves)                                                 4.4e-6, 1.5e-6
  gen1-48    B 1, 7: 10, 5                                                                           4.3e-6
  gen1-48d   B 1, 7: 10, 5                                                                           5.0e-6, delta columns 5.9e-6
  rad2-48    B 1, 5, 259 (block = clip)                                                              3.8e-6
  rad2-31    B 1, 5, 259 (block = clip)                                                              1.8e-6
  noise mix at tuned-14 (B 100, 820) and tuned-61 (B 100, 196): bit-equal to apply + featurize, 4.4e-6 against the oracle
  long rows: gen1-48 5.9e-6 (segments of 256 frames as jobs of 52, 52, 52, 52, 48), rad2-48 4.2e-6, rad2-31 1.9e-6; bit-equal to
  Featurizer.raw of the whole recording in all six cases.
All bit-for-bit relations held: int16 against float32 input (tuned, first generation; the generic kernel within its 1e-6),
gather against copy, even against odd stride, shared-CU against stand-alone form, and batch invariance across every batch size.
Every case prints its figures in a "FIGURES |" line."""
import numpy as np
import pytest

import geometry_cases as gc

pytestmark = pytest.mark.gpu

IDS = [g.name for g in gc.ROWS]
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


_FEATURIZERS = {}


def featurizer(g, share=2):
    from kws_amd.featurizer import Featurizer
    key = (g.name, share)
    if key not in _FEATURIZERS:
        _FEATURIZERS[key] = Featurizer(gc.params(g))
        if share != 2:
            _FEATURIZERS[key].set_cu_share(share)
    return _FEATURIZERS[key]


def device_cus(torch):
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def run(torch, fz, g, wav, lens=None, index=None):
    """the features of the B clips, written into a sentinel-filled buffer of B + 1 clips: every element of the first B is written, the
    clip behind them is not touched"""
    B = wav.shape[0] if index is None else index.numel()
    out = torch.full((B + 1, g.frames, gc.feature_size(g)), SENTINEL, dtype=torch.float32, device="cuda")
    fz(wav, lens, out=out, index=index)
    assert bool((out[:B] != SENTINEL).all()), "%s: %d elements of the output were not written" % (g.name, int((out[:B] == SENTINEL).sum()))
    assert bool((out[B] == SENTINEL).all()), "%s: the kernel wrote past its last clip" % g.name
    return out[:B]


def to_i16(torch, wav):
    return torch.round(wav * 32768).to(torch.int16)


def oracle_errors(torch, g, got, want):
    """(max error of the coefficient columns, of the delta columns or 0, of the coefficients of frames above the log floor).  The
    largest error of a batch is usually 4.4e-6 at the c0 of an all-zero frame: float32's rounding of log(eps) = -36.04."""
    err = (got.double() - want).abs()
    D = g.n_mfcc
    live = want[..., :1] > -30.0
    return float(err[..., :D].max()), (float(err[..., D:].max()) if g.use_delta else 0.0), float((err[..., :D] * live).max())


def assert_same_input_types(torch, g, got16, got32, what):
    if g.kernel == "generic":       # tests/test_featurizer_gpu.py grants the radix-2 kernel 1e-6 between the two input types
        assert float((got16 - got32).abs().max()) <= gc.ATOL_I16_GENERIC, what
    else:
        assert torch.equal(got16, got32), what + ": int16 and float32 input differ"


def job_shape(g, B, cus, shared=False):
    if g.kernel == "tuned":
        return gc.v3_job_shape(g.frames, B, cus, shared)[:2]
    if g.kernel == "gen1":
        return gc.feat_job_shape(g.frames, gc.tail_batch(g), g.use_delta)
    return (0, 0)


@pytest.mark.parametrize("g", gc.ROWS, ids=IDS)
def test_clip_features_match_the_oracle_at_every_batch_size(torch, g):
    """Every clip of every batch size of the row within 2e-4 of the oracle (delta columns 4e-4); int16 input against float32 input; the
    gather form against featurizing a copy, bit for bit; B = 1 is every base clip in a launch of its own (odd base clips start on an odd
    element).  Tuned rows also: the shared-CU form equals the stand-alone one bit for bit, and every batch equals the twelve-clip batch's
    rows -- feat(wav[idx]) == feat(wav)[idx] -- bit for bit, across batch sizes whose jobs have 3, 4 and all frames."""
    cus = device_cus(torch)
    fz = featurizer(g)
    base = torch.from_numpy(gc.base_clips(g)).cuda()
    lens = torch.from_numpy(gc.base_lengths(g)).cuda()
    want = torch.from_numpy(np.array(gc.base_features(g))).cuda()
    assert base.shape[1] % 2 == 1
    base16 = to_i16(torch, base)
    ref12 = run(torch, fz, g, base, lens)
    for B in gc.batches(g, cus):
        idx = torch.from_numpy(gc.batch_index(B)).cuda()
        if B == 1:
            got = torch.cat([run(torch, fz, g, base[i:i + 1], lens[i:i + 1]) for i in range(gc.N_BASE)])
            got16 = torch.cat([run(torch, fz, g, base16[i:i + 1], lens[i:i + 1]) for i in range(gc.N_BASE)])
            idx = torch.arange(gc.N_BASE, device="cuda", dtype=torch.int32)
        else:
            wav, vl = base[idx.long()].contiguous(), lens[idx.long()].contiguous()
            got = run(torch, fz, g, wav, vl)
            got16 = run(torch, fz, g, to_i16(torch, wav), vl)
            assert torch.equal(run(torch, fz, g, base, lens, index=idx), got), "%s B=%d: gather differs from a copy" % (g.name, B)
            assert torch.equal(run(torch, fz, g, base16, lens, index=idx), got16), "%s B=%d: int16 gather differs from a copy" % (g.name, B)
        e_c, e_d, e_live = oracle_errors(torch, g, got, want[idx.long()])
        e16_c, e16_d, _ = oracle_errors(torch, g, got16, want[idx.long()])
        print("FIGURES | %s | B=%d | kernel %s | fpw, jpc = %s (shared-CU form %s) | max error f32 %.3g i16 %.3g delta %.3g, above the "
              "log floor %.3g" % (g.name, B, g.kernel, job_shape(g, B, cus), job_shape(g, B, cus, True), e_c, e16_c, max(e_d, e16_d), e_live))
        assert max(e_c, e16_c) <= gc.ATOL, (g.name, B, e_c, e16_c)
        assert max(e_d, e16_d) <= 2 * gc.ATOL, (g.name, B, e_d, e16_d)
        assert_same_input_types(torch, g, got16, got, "%s B=%d" % (g.name, B))
        if g.kernel == "tuned":
            assert torch.equal(got, ref12[idx.long()]), "%s B=%d: a clip's features depend on the batch around it" % (g.name, B)
            shared = featurizer(g, 1)
            if B == 1:
                s32 = torch.cat([run(torch, shared, g, base[i:i + 1], lens[i:i + 1]) for i in range(gc.N_BASE)])
                s16 = torch.cat([run(torch, shared, g, base16[i:i + 1], lens[i:i + 1]) for i in range(gc.N_BASE)])
            else:
                s32, s16 = run(torch, shared, g, wav, vl), run(torch, shared, g, to_i16(torch, wav), vl)
            assert torch.equal(s32, got) and torch.equal(s16, got16), "%s B=%d: the shared-CU form differs" % (g.name, B)


@pytest.mark.parametrize("g", gc.ROWS, ids=IDS)
def test_gather_stride_and_kernel_labels(torch, g):
    """A reversed and a repeated index against featurizing the copy, bit for bit, in both input types; the same rows at an even stride
    (every row may take two-sample loads) and without valid_len (the head of a row longer than the buffer) give the same bits as at the
    odd stride; and the launch carries the label of the kernel the row names."""
    from kws_amd import lib as L
    fz = featurizer(g)
    base = torch.from_numpy(gc.base_clips(g)).cuda()
    lens = torch.from_numpy(gc.base_lengths(g)).cuda()
    order = list(range(gc.N_BASE - 1, -1, -1)) + [3, 3, 0, 7, 3]
    idx = torch.tensor(order, dtype=torch.int32, device="cuda")
    for src in (base, to_i16(torch, base)):
        copy = run(torch, fz, g, src[idx.long()].contiguous(), lens[idx.long()].contiguous())
        assert torch.equal(run(torch, fz, g, src, lens, index=idx), copy), g.name
        assert torch.equal(copy[:gc.N_BASE].flip(0), run(torch, fz, g, src, lens)), g.name
        assert torch.equal(copy[gc.N_BASE], copy[gc.N_BASE + 1]) and torch.equal(copy[gc.N_BASE], copy[gc.N_BASE - 1 - 3])
        even = torch.nn.functional.pad(src, (0, 1)).contiguous()
        assert even.shape[1] % 2 == 0
        assert torch.equal(run(torch, fz, g, even, lens), run(torch, fz, g, src, lens)), "%s: the row stride changes the features" % g.name
        full = torch.full_like(lens, src.shape[1])
        assert torch.equal(run(torch, fz, g, src), run(torch, fz, g, src, full)), g.name
    L.prof_enable(True)
    try:
        run(torch, fz, g, base, lens)
        torch.cuda.synchronize()
        labels = set(L.prof_report())
    finally:
        L.prof_enable(False)
    assert ("featurize_generic_f32" in labels) == (g.kernel == "generic"), sorted(labels)
    assert ("featurize_fft1024_f32" in labels) == (g.kernel != "generic"), sorted(labels)


def _noise_bank(rng, ms):
    return [(0.2 * rng.standard_normal(ms + 4000)).astype(np.float32),
            (0.05 * rng.standard_normal(ms // 2 + 1000)).astype(np.float32),       # shorter than a clip
            np.zeros(ms + 500, np.float32)]                                          # silent: finite gain


@pytest.mark.parametrize("voice_i16", [False, True])
@pytest.mark.parametrize("name", gc.AUG_ROWS)
def test_fused_noise_mix_equals_apply_then_featurize(torch, name, voice_i16):
    """The AUG form of the tuned kernel (noise mixed in its sample loads) at 14 and 61 frames, construction and tolerances of
    tests/test_augment_gpu.py: test_fused_featurize_matches_oracle_and_apply -- bit-equal to kws_augment_apply followed by the plain
    featurizer, in both CU-share forms, at a batch whose jobs have three frames and at one whose jobs have four; and the oracle's
    features of the materialised clips within 2e-4."""
    from kws_amd.augment import WaveAugment, records
    from oracle import featurizer_oracle as fo
    g = gc.ROW[name]
    cus = device_cus(torch)
    ms = gc.max_samples(g)
    rng = np.random.default_rng(6 + g.frames)
    N = 24
    x = (0.3 * rng.standard_normal((N, ms))).astype(np.float32)
    x[3] = 0.0                                                                       # silent voice: gain 0
    lens = rng.integers(0, ms + 1, N).astype(np.int32)
    lens[:6] = [ms, ms, ms // 3, ms, ms - 1, 0]
    if voice_i16:
        x = np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16)
    aug = WaveAugment(_noise_bank(rng, ms), snr=[0, 10, 20], noised_rate=0.75, time_shift_ms=60, seed=21)
    wav, vl = torch.from_numpy(x).cuda(), torch.from_numpy(lens).cuda()
    for B in (100, gc.tuned_batches(g, cus)["odd"]):
        index = rng.integers(0, N, B).astype(np.int32)
        ix = torch.from_numpy(index).cuda()
        for share in (2, 1):
            fz = featurizer(g, share)
            out = torch.full((B + 1, g.frames, g.n_mfcc), SENTINEL, dtype=torch.float32, device="cuda")
            fz(wav, valid_len=vl, index=ix, augment=aug, step=4, out=out)
            assert bool((out[:B] != SENTINEL).all()), "%s B=%d share=%d: elements of the output were not written" % (name, B, share)
            assert bool((out[B] == SENTINEL).all()), "%s B=%d share=%d: the kernel wrote past its last clip" % (name, B, share)
            plan = aug.plan(wav, valid_len=vl, index=ix, step=4, max_samples=ms)
            rows, L = aug.apply(wav, plan, index=ix, max_samples=ms)
            assert torch.equal(out[:B], run(torch, fz, g, rows, L)), "%s B=%d share=%d" % (name, B, share)
        r = records(plan)
        assert r["apply"].any() and not r["apply"].all() and (r["shift"] % 2 == 1).any()
        got, mixed, n = out[:B].cpu().numpy(), rows.cpu().numpy(), L.cpu().numpy()
        worst = 0.0
        for b in range(0, B, max(1, B // 12)):
            want = fo.audio_to_feature(mixed[b, :n[b]].astype(np.float64), **gc.oracle_kw(g))
            worst = max(worst, float(np.abs(got[b] - want).max()))
        print("FIGURES | %s | AUG %s | B=%d | fpw, jpc = %s | max error %.3g" % (name, "i16" if voice_i16 else "f32", B,
                                                                               job_shape(g, B, cus), worst))
        assert worst <= gc.ATOL


def _long_call(torch, fz, g, wav, lens, max_frames):
    from kws_amd import lib as L
    R = wav.shape[0]
    rows = torch.full((R + 1, max_frames, g.n_mfcc), SENTINEL, dtype=torch.float32, device="cuda")
    d_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
    code = L.WAV_I16 if wav.dtype == torch.int16 else L.WAV_F32
    L.check(L.get_lib().kws_featurize_long(fz._h, wav.data_ptr(), code, R, wav.shape[1], d_len.data_ptr(), max_frames, rows.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream))
    assert bool((rows[R] == SENTINEL).all()), "kws_featurize_long wrote past its last recording"
    return rows[:R]


@pytest.mark.parametrize("dtype", ["int16", "float32"])
@pytest.mark.parametrize("name", gc.LONG_ROWS)
def test_long_rows_through_the_segment_path(torch, name, dtype):
    """kws_featurize_long where the tuned kernel does not apply (featurize_long_segments: long_segments_kernel, the clip kernel on
    256-frame segments, long_rows_kernel).  Three recordings in one launch: 549 frames (both segment seams inside it, the third segment
    short), shorter than a window, exactly 256 frames; max_frames 7 more than the longest needs.  Every row within 3e-4 of mfcc_spec of
    the whole recording, the rows on both sides of each seam on their own, zeros past each recording's frames, nothing past the last
    recording.

    Bit equality with Featurizer.raw of the whole recording is asserted too: both run the same instantiation of the same clip kernel,
    whose per-frame arithmetic (loads, FFT, band sums, DCT) does not depend on which wave job or tail-batch slot a frame lands in --
    featurize_fft1024_kernel indexes its partial sums by the slot but adds them in the same order, featurize_generic_kernel handles one
    frame at a time -- and the two-sample and element-wise loads deliver the same values."""
    from kws_amd import lib as L
    from oracle import featurizer_oracle as fo
    g = gc.ROW[name]
    W, H, T = gc.window_samples(g), gc.hop_samples(g), gc.LONG_TILE
    fz = featurizer(g)
    rng = np.random.default_rng(31 + len(name))
    frames = [2 * T + 37, 0, T]
    lens = [W + (frames[0] - 1) * H + H // 2, W - 3, W + (T - 1) * H]
    assert [gc.raw_frames(g, n) for n in lens] == frames and max(frames) <= 3 * T
    max_frames = max(frames) + 7
    assert gc.long_tile(g, max_frames) == (T, 3)
    recs = [np.clip(rng.normal(0, 3000, n), -32768, 32767).astype(np.int16) for n in lens]
    recs[0][10 * H:10 * H + 3 * W] = 0                                              # all-zero frames: the log floor
    scale = 32768.0
    if dtype == "float32":
        recs = [(r.astype(np.float32) / 32768.0) * np.float32(0.731) for r in recs]    # not int16-representable values
        scale = 1.0
    stride = max(lens) + 1                                                          # odd for all three rows: recording 1 starts on an odd element
    assert stride % 2 == 1
    host = np.zeros((3, stride), recs[0].dtype)
    for i, r in enumerate(recs):
        host[i, :len(r)] = r
    wav = torch.from_numpy(host).cuda()
    L.prof_enable(True)
    try:
        rows = _long_call(torch, fz, g, wav, lens, max_frames)
        torch.cuda.synchronize()
        labels = set(L.prof_report())
    finally:
        L.prof_enable(False)
    assert {"long_segments_kernel", "long_rows_kernel"} <= labels, sorted(labels)
    assert ("featurize_generic_" + ("i16" if dtype == "int16" else "f32") in labels) == (g.kernel == "generic"), sorted(labels)
    got = rows.cpu().numpy()
    worst = 0.0
    for r, rec in enumerate(recs):
        nf = frames[r]
        assert not got[r, nf:].any(), "%s recording %d: rows past its %d frames are not zero" % (name, r, nf)
        if not nf:
            continue
        want = fo.mfcc_spec(rec.astype(np.float64) / scale, **gc.oracle_kw(g))
        assert want.shape == (nf, g.n_mfcc)
        err = np.abs(got[r, :nf] - want).max(axis=1)
        worst = max(worst, float(err.max()))
        for seam in range(T, nf, T):
            assert err[seam - 1] <= gc.ATOL_ROWS, "%s recording %d: last row %d of a segment is off by %.3g" % (name, r, seam - 1, err[seam - 1])
            assert err[seam] <= gc.ATOL_ROWS, "%s recording %d: first row %d of a segment is off by %.3g" % (name, r, seam, err[seam])
        assert err.max() <= gc.ATOL_ROWS, "%s recording %d: row %d is off by %.3g" % (name, r, int(err.argmax()), err.max())
        whole = fz.raw(torch.from_numpy(np.ascontiguousarray(rec)).cuda().reshape(1, -1))[0].cpu().numpy()
        assert whole.shape == (nf, g.n_mfcc)
        assert float(np.abs(whole - want).max()) <= gc.ATOL_ROWS
        np.testing.assert_array_equal(got[r, :nf], whole, err_msg="%s recording %d: long rows differ from Featurizer.raw" % (name, r))
    print("FIGURES | %s | long %s | segments of %d frames, fpw, jpc = %s | max error %.3g" % (
        name, dtype, T, gc.feat_job_shape(T, gc.tail_batch(g), False) if g.kernel == "gen1" else (0, 0), worst))
