"""The streaming stack off the default frame geometry: StreamBatch, scan, kws_stream_gather_windows and kws_stream_push_rows at the rows
of tests/geometry_cases.py (tuned-14, gen1-9, gen1-48, rad2-48; rad2-31, hop > window, through StreamBatch only) and at chunk sizes the
rest of the suite does not use: half a hop (pushes that bring no row), 800, 1023 (an odd carry stride window + chunk) and one chunk
that brings more than n_features rows in a push.  The scheme is that of tests/test_stream_gpu.py: test_stream_batch_matches_oracle_loop
and tests/test_scan_gpu.py: test_scan_matches_the_chunk_loop, with their tolerances: features within 3e-4 of
oracle/stream_oracle.StreamState, post-processing exact on the device's own probabilities, probabilities within 2e-4 of the oracle
model on the oracle's features, scan equal to the StreamBatch loop.

rad2-31 at chunk 800 is the case StreamBatch.update_vectors got wrong before this suite: a push of 800 samples makes two frames and
consumes 1024, the carry length went negative and the next push raised.  The reference empties the carry (listen.py:105).

Measured on an MI355X over all chunk sizes: features within 4.6e-6 (tuned-14), 5.1e-6 (gen1-9), 1.2e-5 (gen1-48), 9.8e-6 (rad2-48),
3.3e-6 (rad2-31) of the oracle loop, probabilities within 1.7e-6 of the oracle model everywhere; scan's probabilities bit-equal to the
loop's at both tile sizes, the gathered windows bit-equal to update_vectors' matrices.  Every case prints a "FIGURES |" line."""
import numpy as np
import pytest

import geometry_cases as gc

pytestmark = pytest.mark.gpu

NAMES = ["background", "up", "down", "left", "right"]
C = 5
S = 3
HEAD_GAIN = 16.0             # tests/test_scan_gpu.py: the seeded weights give nearly uniform probabilities; a steeper head spreads them
CHUNK_IDS = ("half-hop", "800", "1023", "many-rows")
CASES = [(n, i) for n in gc.STREAM_ROWS for i in range(len(CHUNK_IDS))]
CASE_IDS = ["%s-%s" % (n, CHUNK_IDS[i]) for n, i in CASES]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


_MODELS = {}


def models(g):
    """(oracle model, device model) of a row: simple_cnn where kws_model_create accepts the map, simple_gru where not; the oracle's
    seeded weights with the classifier's kernel scaled, rounded to the device's float32 for both"""
    from kws_amd.model import DeviceModel, ModelSpec
    from oracle import model_oracle as mo
    if g.name not in _MODELS:
        kind = gc.stream_model_kind(g)
        om = mo.Model(kind, C, n_features=g.frames, feature_size=g.n_mfcc).init_weights(0)
        ws = om.get_weights()
        ws[-2] = ws[-2] * HEAD_GAIN
        ws = [np.asarray(w, np.float32) for w in ws]
        om.set_weights([w.astype(np.float64) for w in ws])
        dm = DeviceModel(ModelSpec(kind, C, g.frames, g.n_mfcc))
        dm.set_weights(ws)
        _MODELS[g.name] = (om, dm)
    return _MODELS[g.name]


def recordings(g, chunk):
    """(T, pcm (T, S, chunk) int16): at most 40 chunks, enough of them for a full matrix where 40 allow it; stream 1 starts in silence"""
    W, H = gc.window_samples(g), gc.hop_samples(g)
    T = int(min(40, max(8, -(-(W + (g.frames + 3) * H) // chunk) + 3)))
    rng = np.random.default_rng(chunk + g.frames)
    level = rng.choice([150.0, 1500.0, 9000.0], (T, S, 1))                         # loudness moves c0 and with it the winning class
    pcm = np.clip(rng.normal(0, 1, (T, S, chunk)) * level, -32768, 32767).astype(np.int16)
    pcm[:max(2, T // 4), 1] = 0
    return T, pcm


def run_loop(torch, g, chunk, pcm):
    """StreamBatch over the S streams, every chunk checked against the oracle loop -> per chunk (index, score, fired, probs, state,
    matrices) and the largest feature and probability errors"""
    from kws_amd.stream import StreamBatch
    from oracle import featurizer_oracle as fo
    from oracle import stream_oracle as so
    pr = gc.params(g)
    om, dm = models(g)
    kw = gc.oracle_kw(g)
    sb = StreamBatch(pr, dm, S, chunk_size=chunk, class_names=NAMES, sensitivity=0.5, trigger_level=3)
    dec = so.decoder_table(pr.threshold_config)
    states = [so.StreamState(g.frames, g.n_mfcc, pr.window_samples, pr.hop_samples, lambda a: fo.mfcc_spec(a, **kw)) for _ in range(S)]
    trig = [so.TriggerState() for _ in range(S)]
    out, e_feat, e_prob, winners = [], 0.0, 0.0, set()
    for t in range(pcm.shape[0]):
        chunks = [pcm[t, s].tobytes() for s in range(S)] if t % 2 else pcm[t]      # both input forms
        index, score, fired = sb.push(chunks)
        assert 0 <= sb.n_win < pr.window_samples + chunk
        feats, probs = sb.mfccs.cpu().numpy(), sb.probs.cpu().numpy()
        for s in range(S):
            want_feat = states[s].push(pcm[t, s].astype(np.float64) / 32768.0)
            err = float(np.abs(feats[s] - want_feat).max())
            e_feat = max(e_feat, err)
            assert err <= gc.ATOL_ROWS, "%s chunk size %d, chunk %d, stream %d: features off by %.3g" % (g.name, chunk, t, s, err)
            wi, ws, wf = so.postprocess(probs[s], 0, dec, pr.threshold_center, trig[s], 0.5, 3, chunk)
            assert int(index[s]) == wi and int(fired[s]) == int(wf)
            assert abs(float(score[s]) - ws) <= 1e-12 * max(1.0, abs(ws))
            assert int(sb.state[s, 0]) == trig[s].activation
            winners.add(wi)
        x = np.stack([st.mfccs for st in states])
        want_probs = om.predict(x[..., None] if om.input_rank == 4 else x)
        err = float(np.abs(probs - want_probs).max())
        e_prob = max(e_prob, err)
        assert err <= gc.FWD_ATOL, "%s chunk size %d, chunk %d: probabilities off by %.3g" % (g.name, chunk, t, err)
        out.append((index.cpu().numpy().copy(), score.cpu().numpy().copy(), fired.cpu().numpy().copy(), probs.copy(),
                    sb.state.cpu().numpy().copy(), feats.copy()))
    return out, e_feat, e_prob, winners


def compare_scan(torch, res, loop, T, short_chunks):
    """tests/test_scan_gpu.py: _compare_scan_to_loop for lock-stepped streams: the probabilities within the forward's tolerance in any
    case and, the forward being batch-invariant on the device, bit-equal, with index, score bits, fired flags and final state equal.
    Recording S is recording 0 cut short: its chunks before the cut are recording 0's, chunks past its end are blank."""
    probs = res.probs.cpu().numpy()
    gi, gf, gs, gstate = res.index.cpu().numpy(), res.fired.cpu().numpy(), res.score.cpu().numpy(), res.state.cpu().numpy()
    assert res.n_chunks == [T] * S + [short_chunks]
    for r in range(S + 1):
        src, n = (r, T) if r < S else (0, short_chunks - 1)                        # the cut recording's own last chunk is shorter
        want_p = np.stack([c[3][src] for c in loop[:n]])
        np.testing.assert_allclose(probs[r, :n], want_p, rtol=0, atol=gc.FWD_ATOL)
        np.testing.assert_array_equal(probs[r, :n].view(np.uint32), want_p.view(np.uint32))
        assert gi[r, :n].tolist() == [int(c[0][src]) for c in loop[:n]]
        assert gf[r, :n].tolist() == [int(c[2][src]) for c in loop[:n]]
        np.testing.assert_array_equal(gs[r, :n].view(np.uint64), np.array([c[1][src] for c in loop[:n]]).view(np.uint64))
        if r < S:
            np.testing.assert_array_equal(gstate[r], loop[-1][4][r])
    assert (gi[S, short_chunks:] == -1).all() and not gf[S, short_chunks:].any() and not gs[S, short_chunks:].any()
    assert gi[S, short_chunks - 1] >= 0


@pytest.mark.parametrize("name,ci", CASES, ids=CASE_IDS)
def test_stream_batch_scan_and_windows_off_the_default_geometry(torch, name, ci):
    from kws_amd import lib as L
    from kws_amd.stream import scan, scan_plan
    g = gc.ROW[name]
    chunk = gc.stream_chunks(g)[ci]
    pr = gc.params(g)
    W, H, F, D = pr.window_samples, pr.hop_samples, g.frames, g.n_mfcc
    T, pcm = recordings(g, chunk)
    assert T <= 40
    loop, e_feat, e_prob, winners = run_loop(torch, g, chunk, pcm)
    rows_seen = [gc.raw_frames(g, (t + 1) * chunk) for t in range(T)]
    print("FIGURES | %s | chunk %d x %d | model %s | max feature error %.3g, max probability error %.3g, classes that win %s" % (
        name, chunk, T, gc.stream_model_kind(g), e_feat, e_prob, sorted(winners)))
    om, dm = models(g)
    recs = [np.ascontiguousarray(pcm[:, s].reshape(-1)) for s in range(S)]
    if H > W:
        # the closed form does not hold (tests/test_geometry_host.py): scan, its plan and its window gather refuse the geometry
        with pytest.raises(ValueError, match="hop"):
            scan(pr, dm, recs, chunk_size=chunk, class_names=NAMES)
        with pytest.raises(ValueError, match="hop"):
            scan_plan(len(recs[0]), chunk, W, H, F)
        one = torch.zeros((1, F, D), dtype=torch.float32, device="cuda")
        n1 = torch.tensor([4 * chunk], dtype=torch.int32, device="cuda")
        assert L.get_lib().kws_stream_gather_windows(one.data_ptr(), 1, 1, n1.data_ptr(), chunk, W, H, F, D, 0, 1, one.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream) != 0
        return
    # what each chunk size is there for
    if ci == 0:
        assert any(a == b for a, b in zip(rows_seen[-8:], rows_seen[-7:]))          # pushes without a new row, after the first rows
    if ci == 2:
        assert (W + chunk) % 2 == 1
    if ci == 3:
        assert rows_seen[0] > F
    short = recs[0][:(T // 2) * chunk + chunk // 2 + 1]
    short_chunks = T // 2 + 1
    for tile in ((S + 1) * T, (S + 1) * 3):                                         # all chunks at once; 3 chunks of each recording per tile
        res = scan(pr, dm, recs + [short], chunk_size=chunk, class_names=NAMES, sensitivity=0.5, trigger_level=3, tile=tile, return_probs=True)
        assert res.index.shape == (S + 1, T)
        compare_scan(torch, res, loop, T, short_chunks)
    # kws_stream_gather_windows alone, on kws_featurize_long's rows: the matrices update_vectors held after every chunk, bit for bit
    from kws_amd.featurizer import Featurizer
    fz = Featurizer(pr)
    wav = torch.from_numpy(np.stack(recs)).cuda()
    lens = [len(r) for r in recs]
    max_frames = gc.raw_frames(g, lens[0])
    rows = torch.full((S, max(max_frames, 1), D), 7.0, dtype=torch.float32, device="cuda")
    d_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    L.check(L.get_lib().kws_featurize_long(fz._h, wav.data_ptr(), L.WAV_I16, S, wav.shape[1], d_len.data_ptr(), max_frames, rows.data_ptr(), st))
    n = T + 2                                                                       # two chunks past the recordings' end: zeros
    feat = torch.full((S * n + 1, F, D), 7.0, dtype=torch.float32, device="cuda")
    L.check(L.get_lib().kws_stream_gather_windows(rows.data_ptr(), S, max_frames, d_len.data_ptr(), chunk, W, H, F, D, 0, n, feat.data_ptr(), st))
    got = feat.cpu().numpy()
    assert (got[S * n] == 7.0).all()
    got = got[:S * n].reshape(S, n, F, D)
    for t in range(T):
        np.testing.assert_array_equal(got[:, t], loop[t][5], err_msg="%s chunk size %d: window of chunk %d" % (name, chunk, t))
    assert not got[:, T:].any()
