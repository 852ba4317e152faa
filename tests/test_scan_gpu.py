"""GPU tests of the offline scan (kws_amd.stream.scan and the three entry points behind it) against the chunk loop it
restates (StreamBatch.push / Listener.run_wav), layer by layer: rows and windows bit for bit, the post-processing bit for
bit on the same probabilities, and the whole scan within the tolerance the existing stream test grants the forward pass
at another batch size."""
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NAMES = ["background", "up", "down", "left", "right"]
FWD_ATOL = 2e-4              # tests/test_stream_gpu.py: the forward pass against the oracle model


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _cs(torch):
    return torch.cuda.current_stream().cuda_stream


def _noise(rng, n, scale=3000):
    return np.clip(rng.normal(0, scale, n), -32768, 32767).astype(np.int16)


def _long_rows(torch, fz, wav, lens, max_frames=None):
    """kws_featurize_long on a padded (R, stride) tensor"""
    from classifier.params import pr
    from kws_amd import lib as L
    R = wav.shape[0]
    nf = [0 if n < pr.window_samples else (n - pr.window_samples) // pr.hop_samples + 1 for n in lens]
    mf = max(nf) if max_frames is None else max_frames
    rows = torch.full((R, max(mf, 1), pr.n_mfcc), 7.0, dtype=torch.float32, device="cuda")        # poisoned: every row must be written
    d_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
    code = L.WAV_I16 if wav.dtype == torch.int16 else L.WAV_F32
    L.check(L.get_lib().kws_featurize_long(fz._h, wav.data_ptr(), code, R, wav.shape[1], d_len.data_ptr(), mf, rows.data_ptr(), _cs(torch)))
    return rows, nf, d_len


def _segment_rows(torch, fz, rec, f0, f1):
    """Featurizer.raw on the stretch that holds frames [f0, f1) (at most pr.max_samples samples, starting on a frame boundary)"""
    from classifier.params import pr
    a, b = f0 * pr.hop_samples, (f1 - 1) * pr.hop_samples + pr.window_samples
    assert b - a <= pr.max_samples
    seg = torch.from_numpy(np.ascontiguousarray(rec[a:b])).cuda().reshape(1, -1)
    return fz.raw(seg)[0].cpu().numpy()


def _pad(recs, dtype):
    stride = (max(len(r) for r in recs) + 1) & ~1
    host = np.zeros((len(recs), stride), dtype)
    for i, r in enumerate(recs):
        host[i, :len(r)] = r
    return host


@pytest.mark.parametrize("dtype", ["int16", "float32"])
def test_long_rows_are_the_chunk_loops_rows(torch, dtype):
    """Three ragged recordings: every row equals Featurizer.raw's on 30-frame segments (the sizes the chunk loop and the
    dataset path run) bit for bit and the oracle's mfcc_spec of the whole recording within 3e-4; rows past a recording's
    frames are zeros."""
    from classifier.params import pr
    from kws_amd.featurizer import Featurizer
    from oracle import featurizer_oracle as fo
    rng = np.random.default_rng(11)
    W, H = pr.window_samples, pr.hop_samples
    recs = [_noise(rng, 50000), _noise(rng, 700), _noise(rng, W + 40 * H + 100)]       # 96 frames; none; 41 (no multiple of a tile)
    recs[0][10000:14000] = 0                                                            # all-zero frames: the log floor
    if dtype == "float32":
        recs = [(r.astype(np.float32) / 32768.0) * np.float32(0.731) for r in recs]     # not int16-representable values
    fz = Featurizer(pr)
    lens = [len(r) for r in recs]
    rows, nf, _ = _long_rows(torch, fz, torch.from_numpy(_pad(recs, recs[0].dtype)).cuda(), lens)
    got = rows.cpu().numpy()
    assert nf == [96, 0, 41]
    seg = (pr.max_samples - W) // H + 1
    for r, rec in enumerate(recs):
        for f0 in range(0, nf[r], seg):
            f1 = min(f0 + seg, nf[r])
            np.testing.assert_array_equal(got[r, f0:f1], _segment_rows(torch, fz, rec, f0, f1), err_msg="recording %d frames %d..%d" % (r, f0, f1))
        if nf[r]:
            want = fo.mfcc_spec(rec.astype(np.float64) / (32768.0 if dtype == "int16" else 1.0))
            err = float(np.abs(got[r, :nf[r]] - want).max())
            print("recording %d: max |rows - oracle| = %.3g" % (r, err))
            assert err <= 3e-4
        assert not got[r, nf[r]:].any()


def test_long_rows_of_a_ten_minute_recording(torch):
    """One 10-minute recording in one launch: its first, a middle and its last 30 frames against Featurizer.raw (bit for
    bit) and the oracle (3e-4)."""
    from classifier.params import pr
    from kws_amd.featurizer import Featurizer
    from oracle import featurizer_oracle as fo
    rng = np.random.default_rng(12)
    W, H = pr.window_samples, pr.hop_samples
    N = 600 * pr.sample_rate + 333
    rec = _noise(rng, N)
    fz = Featurizer(pr)
    rows, nf, _ = _long_rows(torch, fz, torch.from_numpy(rec[:N + (N & 1)].copy() if not N & 1 else np.append(rec, np.int16(0))).cuda().reshape(1, -1), [N])
    got = rows.cpu().numpy()[0]
    assert nf[0] == (N - W) // H + 1 == got.shape[0]
    for f0 in (0, nf[0] // 2 + 1, nf[0] - 30):
        f1 = f0 + 30
        np.testing.assert_array_equal(got[f0:f1], _segment_rows(torch, fz, rec, f0, f1))
        want = fo.mfcc_spec(rec[f0 * H:(f1 - 1) * H + W].astype(np.float64) / 32768.0)
        assert float(np.abs(got[f0:f1] - want).max()) <= 3e-4
    assert np.isfinite(got).all()


HEAD_GAIN = 16.0             # the seeded random weights give nearly uniform probabilities: a steeper head spreads them


def _model(torch, seed=0, C=5):
    from classifier.params import pr
    from kws_amd.model import DeviceModel, ModelSpec
    from oracle import model_oracle as mo
    om = mo.Model("simple_cnn", C).init_weights(seed)
    ws = om.get_weights()
    ws[-2] = ws[-2] * HEAD_GAIN                                                         # the classifier's kernel
    dm = DeviceModel(ModelSpec("simple_cnn", C, pr.n_features, pr.n_mfcc))
    dm.set_weights(ws)
    return dm


def _chunk_loop(torch, dm, rec, chunk, quantized=None, want_feats=False):
    """StreamBatch with one stream over a recording: per chunk (index, score, fired, probs, state[, features])"""
    from classifier.params import pr
    from kws_amd.stream import StreamBatch
    sb = StreamBatch(pr, dm, 1, chunk_size=chunk, class_names=NAMES, sensitivity=0.5, trigger_level=3, quantized=quantized)
    out = []
    for a in range(0, len(rec), chunk):
        index, score, fired = sb.push(rec[a:a + chunk].reshape(1, -1))
        item = [int(index[0]), float(score[0]), int(fired[0]), sb.probs[0].cpu().numpy().copy(), sb.state[0].cpu().numpy().copy()]
        if want_feats:
            item.append(sb.mfccs[0].cpu().numpy().copy())
        out.append(item)
    return out, sb


@pytest.mark.parametrize("chunk", [1024, 800])
def test_gathered_windows_are_update_vectors(torch, chunk):
    """Every chunk's window equals the matrix StreamBatch.update_vectors holds after that chunk, bit for bit (a short last
    chunk included); chunks past a recording's end give zeros."""
    from classifier.params import pr
    from kws_amd import lib as L
    from kws_amd.featurizer import Featurizer
    from kws_amd.stream import StreamBatch
    rng = np.random.default_rng(chunk)
    recs = [_noise(rng, 37 * chunk + 311), _noise(rng, 9 * chunk + 1), _noise(rng, 500)]
    recs[0][:6 * chunk] = 0
    lens = [len(r) for r in recs]
    fz = Featurizer(pr)
    rows, nf, d_len = _long_rows(torch, fz, torch.from_numpy(_pad(recs, np.int16)).cuda(), lens)
    T = [-(-n // chunk) for n in lens]
    n_chunks = max(T) + 2
    F, D = pr.n_features, pr.n_mfcc
    got = []
    for k0, n in ((0, 5), (5, n_chunks - 5)):                                           # two tiles: k0 is honoured
        feat = torch.full((len(recs) * n, F, D), 7.0, dtype=torch.float32, device="cuda")
        L.check(L.get_lib().kws_stream_gather_windows(rows.data_ptr(), len(recs), max(nf), d_len.data_ptr(), chunk, pr.window_samples,
                                                      pr.hop_samples, F, D, k0, n, feat.data_ptr(), _cs(torch)))
        got.append(feat.cpu().numpy().reshape(len(recs), n, F, D))
    got = np.concatenate(got, axis=1)
    dm = _model(torch)
    for r, rec in enumerate(recs):
        sb = StreamBatch(pr, dm, 1, chunk_size=chunk, class_names=NAMES, featurizer=fz)
        for k, a in enumerate(range(0, len(rec), chunk)):
            want = sb.update_vectors(rec[a:a + chunk].reshape(1, -1))[0].cpu().numpy()
            np.testing.assert_array_equal(got[r, k], want, err_msg="recording %d chunk %d" % (r, k))
        assert k + 1 == T[r] and not got[r, T[r]:].any()


def _scan_post(torch, dec, probs, rec_chunks, state, tile, C=5, chunk=1024):
    """kws_stream_scan_postprocess over probs (R, T, C) in tiles of `tile` chunks"""
    from kws_amd import lib as L
    R, T = probs.shape[0], probs.shape[1]
    index = torch.full((R, T), 99, dtype=torch.int32, device="cuda")
    score = torch.full((R, T), 99.0, dtype=torch.float64, device="cuda")
    fired = torch.full((R, T), 99, dtype=torch.int32, device="cuda")
    d_chunks = torch.tensor(rec_chunks, dtype=torch.int32, device="cuda")
    for k0 in range(0, T, tile):
        n = min(tile, T - k0)
        p = probs[:, k0:k0 + n].contiguous()
        L.check(L.get_lib().kws_stream_scan_postprocess(dec.handle, p.data_ptr(), R, n, C, d_chunks.data_ptr(), k0, 0, 0.5, 3, chunk,
                                                        state.data_ptr(), index.data_ptr() + 4 * k0, score.data_ptr() + 8 * k0,
                                                        fired.data_ptr() + 4 * k0, T, _cs(torch)))
    return index.cpu().numpy(), score.cpu().numpy(), fired.cpu().numpy()


def _fresh_state(torch, R):
    st = torch.zeros((R, 2), dtype=torch.int32, device="cuda")
    st[:, 1] = -1
    return st


def _chained_postprocess(torch, dec, probs, chunk=1024):
    """kws_stream_postprocess chunk by chunk over probs (R, T, C): the yardstick"""
    from kws_amd import lib as L
    R, T, C = probs.shape
    st = _fresh_state(torch, R)
    index = torch.zeros(R, dtype=torch.int32, device="cuda")
    score = torch.zeros(R, dtype=torch.float64, device="cuda")
    fired = torch.zeros(R, dtype=torch.int32, device="cuda")
    out, states = [], []
    for t in range(T):
        p = probs[:, t].contiguous()
        L.check(L.get_lib().kws_stream_postprocess(dec.handle, p.data_ptr(), R, C, 0, 0.5, 3, chunk, st.data_ptr(), index.data_ptr(),
                                                   score.data_ptr(), fired.data_ptr(), _cs(torch)))
        out.append((index.cpu().numpy().copy(), score.cpu().numpy().copy(), fired.cpu().numpy().copy()))
        states.append(st.cpu().numpy().copy())
    return [np.stack([o[i] for o in out], axis=1) for i in range(3)], np.stack(states, axis=1)


def test_scan_postprocess_equals_chained_postprocess(torch):
    """On the chunk loop's own probabilities, and on probabilities with confident streaks (so that the detector fires and
    rests), one call and tiles of 7 chunks give the index, score bits, fired flags and final state of chained
    kws_stream_postprocess; a recording that ends early keeps the state of its last chunk."""
    from classifier.params import pr
    from kws_amd.stream import ThresholdDecoder
    rng = np.random.default_rng(21)
    dm = _model(torch)
    loops = [_chunk_loop(torch, dm, _noise(rng, 40 * 1024), 1024)[0] for _ in range(3)]
    loop_probs = np.stack([np.stack([c[3] for c in lp]) for lp in loops])               # (3, 40, 5)
    T, C = 40, 5
    streak = rng.dirichlet(np.ones(C), (4, T)).astype(np.float32)
    for r in range(4):
        for t in range(T):
            if (t // 9 + r) % 2:                                                        # runs of one confident class
                streak[r, t] = 0.01
                streak[r, t, 1 + (t // 9 + r) % 4] = 0.96
    dec = ThresholdDecoder(pr.threshold_config, pr.threshold_center)
    for name, probs_np in (("loop", loop_probs), ("streak", streak)):
        probs = torch.from_numpy(probs_np).cuda()
        R = probs.shape[0]
        (wi, ws, wf), wstates = _chained_postprocess(torch, dec, probs)
        if name == "streak":
            assert wf.sum() >= 4 and (wstates[:, :, 0] < 0).any()                       # it fires and rests
        for tile in (T, 7):
            st = _fresh_state(torch, R)
            gi, gs, gf = _scan_post(torch, dec, probs, [T] * R, st, tile)
            np.testing.assert_array_equal(gi, wi)
            np.testing.assert_array_equal(gf, wf)
            np.testing.assert_array_equal(gs.view(np.uint64), ws.view(np.uint64))
            np.testing.assert_array_equal(st.cpu().numpy(), wstates[:, -1])
        # recording 1 ends after 33 chunks: later chunks are blank and its state is the loop's after chunk 33
        ends = [T] * R
        ends[1] = 33
        st = _fresh_state(torch, R)
        gi, gs, gf = _scan_post(torch, dec, probs, ends, st, 7)
        np.testing.assert_array_equal(gi[1, :33], wi[1, :33])
        np.testing.assert_array_equal(gf[1, :33], wf[1, :33])
        assert (gi[1, 33:] == -1).all() and not gf[1, 33:].any() and not gs[1, 33:].any()
        np.testing.assert_array_equal(st.cpu().numpy()[1], wstates[1, 32])
        np.testing.assert_array_equal(gf[0], wf[0])


def test_scan_postprocess_fires_on_a_confident_streak(torch):
    """The forced streak of test_stream_batch_fires_on_a_confident_streak: fires at the same chunk and rests as long."""
    from classifier.params import pr
    from kws_amd.stream import ThresholdDecoder
    one = torch.tensor([[0.01, 0.97, 0.01, 0.005, 0.005], [0.9, 0.05, 0.03, 0.01, 0.01], [0.005, 0.005, 0.005, 0.98, 0.005]],
                       dtype=torch.float32, device="cuda")
    probs = one[:, None, :].repeat(1, 12, 1).contiguous()
    dec = ThresholdDecoder(pr.threshold_config, pr.threshold_center)
    for tile in (12, 7):
        st = _fresh_state(torch, 3)
        gi, gs, gf = _scan_post(torch, dec, probs, [12, 12, 12], st, tile)
        assert list(np.nonzero(gf[0])[0]) == [4] and list(np.nonzero(gf[2])[0]) == [4]
        assert gf[1].sum() == 0
        assert int(st[0, 0]) == -16 + 7
        assert gi[:, -1].tolist() == [1, 0, 3]
        assert float(gs[1, -1]) == pytest.approx(0.9)


def _compare_scan_to_loop(torch, res, loops):
    """The rule of the end-to-end tests.  The issue grants the forward pass at another batch size atol = 2e-4 on the
    probabilities and lets decisions differ on chunks whose own margins are inside that tolerance -- unless the forward
    turns out to be batch-invariant bit for bit, in which case equality is to be asserted.  On the MI355X it is (B = 1 in
    the chunk loop against tiles of 60, 64 and ~200 windows, fp32-level and int8 forward: max |difference| = 0), so every
    chunk is compared and nothing is skipped: probabilities, index, score bits, fired flags and the final state are equal.
    The count of chunks that WOULD have been ambiguous under the tolerance rule is printed for the record."""
    probs_all = res.probs.cpu().numpy()
    gi, gf, gs = res.index.cpu().numpy(), res.fired.cpu().numpy(), res.score.cpu().numpy()
    gstate = res.state.cpu().numpy()
    total = ambiguous = 0
    for r, lp in enumerate(loops):
        T = len(lp)
        assert res.n_chunks[r] == T
        want_p = np.stack([c[3] for c in lp])
        np.testing.assert_allclose(probs_all[r, :T], want_p, rtol=0, atol=FWD_ATOL)             # what is owed in any case
        np.testing.assert_array_equal(probs_all[r, :T].view(np.uint32), want_p.view(np.uint32))  # what the device gives
        for c in lp:
            top = np.sort(c[3])[::-1]
            ambiguous += bool(top[0] - top[1] <= FWD_ATOL or abs(c[1] - 0.5) <= FWD_ATOL)
        total += T
        assert gi[r, :T].tolist() == [c[0] for c in lp]
        assert gf[r, :T].tolist() == [c[2] for c in lp]
        np.testing.assert_array_equal(gs[r, :T].view(np.uint64), np.array([c[1] for c in lp]).view(np.uint64))
        np.testing.assert_array_equal(gstate[r], lp[-1][4])
        assert (gi[r, T:] == -1).all() and not gf[r, T:].any() and not gs[r, T:].any()
    print("%d chunks compared, all equal; %d of them have margins within %g" % (total, ambiguous, FWD_ATOL))


def _e2e_recordings(chunk):
    rng = np.random.default_rng(chunk)
    recs = [_noise(rng, n) for n in (40 * chunk, 41 * chunk + 17, 38 * chunk - 1, 40 * chunk + chunk // 2, 36 * chunk + 1)]
    recs[1][:6 * chunk] = 0                                                             # starts in silence
    return recs


@pytest.mark.parametrize("kind", ["float", "int8"])
def test_scan_matches_the_chunk_loop(torch, kind):
    """`scan` against StreamBatch.push over 5 ragged recordings of ~40 chunks (seeded oracle weights and noise, as in
    test_stream_batch_matches_oracle_loop, with the classifier's kernel scaled by HEAD_GAIN), float and int8 forward, in
    tiles of 64 windows and in one tile.

    Margins of the chunk loop itself, found on the CPU with oracle.model_oracle + oracle.stream_oracle on these recordings
    before any GPU run (float model): smallest top-two gap 6.2e-4, smallest |score - 0.5| 7.8e-3, so 0 of 198 chunks are
    within 2e-4 (the cap is 1 %).  With the unscaled weights the smallest gap was 2.8e-5 and 4 of 198 chunks (2 %) were
    ambiguous, which is why the head is scaled.  On the GPU the probabilities turned out bit-equal (see
    _compare_scan_to_loop), so no chunk is skipped; the int8 loop has 1 chunk of 198 inside the margin, compared all the
    same."""
    from classifier.params import pr
    from kws_amd.featurizer import Featurizer
    from kws_amd.quant import QuantizedCNN, calibrate
    from kws_amd.stream import scan
    chunk = 1024
    recs = _e2e_recordings(chunk)
    dm = _model(torch)
    q = None
    if kind == "int8":
        rng = np.random.default_rng(5)
        clips = torch.from_numpy((rng.normal(0, 3000 / 32768.0, (256, pr.max_samples))).astype(np.float32)).cuda()
        q = QuantizedCNN.from_model(dm, calibrate(dm, Featurizer(pr)(clips)), "max")
    loops = [_chunk_loop(torch, dm, rec, chunk, quantized=q)[0] for rec in recs]
    for tile in (64, 4096):
        res = scan(pr, dm, recs, chunk_size=chunk, class_names=NAMES, sensitivity=0.5, trigger_level=3, quantized=q, tile=tile,
                   return_probs=True)
        assert res.index.shape == (5, 42) and res.n_chunks == [40, 42, 38, 41, 37]
        _compare_scan_to_loop(torch, res, loops)
    # the padded-array form gives the same result as the list form
    padded = torch.from_numpy(_pad(recs, np.int16)).cuda()
    res2 = scan(pr, dm, padded, lengths=[len(r) for r in recs], chunk_size=chunk, class_names=NAMES, quantized=q, return_probs=True)
    assert torch.equal(res2.index, res.index) and torch.equal(res2.fired, res.fired) and torch.equal(res2.probs, res.probs)


def test_scan_edge_cases(torch):
    from classifier.params import pr
    from kws_amd.stream import scan
    dm = _model(torch)
    res = scan(pr, dm, [], class_names=NAMES)
    assert res.index.shape == (0, 0) and res.n_chunks == [] and res.state.shape == (0, 2)
    rng = np.random.default_rng(3)
    short = _noise(rng, 300)
    res = scan(pr, dm, [short, np.zeros(0, np.int16)], class_names=NAMES, return_probs=True)
    assert res.n_chunks == [1, 0] and res.index.shape == (2, 1)
    loop, _ = _chunk_loop(torch, dm, short, 1024)                                        # one chunk, predicted on the all-zero matrix
    assert int(res.index[0, 0]) == loop[0][0] and int(res.fired[0, 0]) == 0 and int(res.index[1, 0]) == -1
    np.testing.assert_allclose(res.probs[0, 0].cpu().numpy(), loop[0][3], rtol=0, atol=FWD_ATOL)
    assert res.state[1].tolist() == [0, -1]
    with pytest.raises(ValueError):
        scan(pr, dm, [short.astype(np.float32)])


def test_listener_scan_wav_is_run_wav(torch, tmp_path):
    """Listener.scan_wav on a written wav returns the list Listener.run_wav returns for it (rule of
    _compare_scan_to_loop: equality; on the CPU oracle no chunk of these files is within the tolerance rule's margins
    either) and calls on_activation as often; a list of files gives a list of such lists."""
    from classifier.model import get_model
    from kws_amd.init import init_weights
    from listen import Listener
    classes = tmp_path / "classes.txt"
    classes.write_text("\n".join(NAMES) + "\n")
    rng = np.random.default_rng(3)
    paths, pcms = [], [_noise(rng, 3 * 16000 + 700, 4000), _noise(rng, 16000 + 5, 4000)]
    for i, pcm in enumerate(pcms):
        paths.append(str(tmp_path / ("in%d.wav" % i)))
        with wave.open(paths[-1], "wb") as wf:
            wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(16000)
            wf.writeframes(pcm.tobytes())
    m = get_model("simple_cnn", 5)
    ws = init_weights(m.spec, seed=4)
    ws[-2] = ws[-2] * HEAD_GAIN            # CPU oracle on these files: smallest top-two gap 4.9e-3, smallest |score - 0.5| 0.23
    m.set_weights(ws)
    want, calls = [], []
    for p in paths:
        lis = Listener(model=m, classes_path=str(classes), input_wav=p, chunk_size=1024)
        want.append(lis.run_wav(quiet=True))
        calls.append(len(lis.activations))
    lis = Listener(model=m, classes_path=str(classes), input_wav=paths[0], chunk_size=1024)
    got = lis.scan_wav(quiet=True)
    assert len(got) == len(want[0]) == -(-len(pcms[0]) // 1024)
    assert got == want[0]                      # float scores included: the forward is batch-invariant (_compare_scan_to_loop)
    assert len(lis.activations) == calls[0]
    assert all(isinstance(i, int) and isinstance(s, float) and isinstance(f, bool) for i, s, f in got)
    lis2 = Listener(model=m, classes_path=str(classes), chunk_size=1024)
    assert lis2.scan_wav(paths) == want and len(lis2.activations) == sum(calls)
    assert [len(t) for t in lis2.scan_times] == calls


def test_scan_tile_size_does_not_change_the_result(torch):
    """One recording of 4300 chunks in tiles of 4096 windows (where the forward is measured), 1000 and 64: the decisions
    are those of the 64-window tiles that test_scan_matches_the_chunk_loop ties to the chunk loop; the probabilities stay
    inside the forward's tolerance (their largest difference is printed)."""
    from classifier.params import pr
    from kws_amd.stream import scan
    rng = np.random.default_rng(8)
    rec = _noise(rng, 4300 * 1024 - 77)
    dm = _model(torch)
    base = scan(pr, dm, [rec], class_names=NAMES, tile=64, return_probs=True)
    for tile in (1000, 4096):
        res = scan(pr, dm, [rec], class_names=NAMES, tile=tile, return_probs=True)
        diff = float((res.probs - base.probs).abs().max())
        print("tile %d against tile 64: max |probs difference| = %.3g" % (tile, diff))
        assert diff <= FWD_ATOL
        p = base.probs[0].cpu().numpy()
        top = np.sort(p, axis=1)
        clear = (top[:, -1] - top[:, -2] > 2 * FWD_ATOL)          # both sides may move by the tolerance
        assert clear.mean() >= 0.99
        assert torch.equal(res.index[0][torch.from_numpy(clear).cuda()], base.index[0][torch.from_numpy(clear).cuda()])
        if diff == 0:
            assert torch.equal(res.index, base.index) and torch.equal(res.fired, base.fired) and torch.equal(res.score, base.score)
            assert torch.equal(res.state, base.state)
