"""GPU tests of the harvest of a scan (kws_stream_collect, kws_stream_peaks, kws_amd.stream.collect / peaks / Detections,
Listener's save_dir) against the pure-Python restatement tests/mine_ref.py.  Every comparison is exact equality: the kernels
read the same doubles and compare them as the reference does, chunk numbers are integers, and a clip's samples are int16 / 32768,
which float32 holds exactly.  The synthetic scan is tests/sweep_cases.py; tests/test_mine_host.py checks on the reference alone
that it holds every kind of detection, and that the tie case has ties."""
import os
import wave

import numpy as np
import pytest

import mine_ref
import sweep_cases as cases

pytestmark = pytest.mark.gpu

NAMES = ["background", "up", "down", "left", "right"]
POINTS = [(0.5, 3), (0.25, 1)]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def synthetic(torch):
    index, score = cases.build()
    return index, score, torch.from_numpy(index).cuda(), torch.from_numpy(score).cuda()


@pytest.fixture(scope="module")
def tie(torch):
    index, score = mine_ref.tie_case()
    return index, score, torch.from_numpy(index).cuda(), torch.from_numpy(score).cuda()


def _ref_detections(index, score, sens, level, chunk_size, events):
    return [mine_ref.detections(index[r], score[r], n, cases.BACKGROUND, sens, level, chunk_size, None if events is None else events[r])
            for r, n in enumerate(cases.N_CHUNKS)]


def _rows(det):
    """Detections -> host list of (recording, chunk, class, kind, event, score)"""
    cols = [t.cpu().tolist() for t in (det.recording, det.chunk, det.cls, det.kind, det.event, det.score)]
    return list(zip(*cols))


def _flat(per_rec):
    return [(r, k, c, kind, ev, sc) for r, rec in enumerate(per_rec) for k, c, kind, ev, sc in rec]


@pytest.mark.parametrize("chunk_size", cases.CHUNK_SIZES)
def test_collect_equals_the_reference(torch, synthetic, chunk_size):
    """R = 6 recordings of 0, 1, 63, 64, 65 and 130 chunks in rows of 136 with poisoned padding, at two operating points:
    every field with labels; kind 0, event -1 and the same chunks without."""
    from kws_amd.stream import collect
    index, score, d_index, d_score = synthetic
    lens = [n * chunk_size for n in cases.N_CHUNKS]
    for sens, level in POINTS:
        want = _ref_detections(index, score, sens, level, chunk_size, cases.EVENTS)
        assert sum(len(w) for w in want) > 0
        det = collect((d_index, d_score, cases.N_CHUNKS), chunk_size, sens, level, events=cases.sample_events(chunk_size), lengths=lens,
                      tolerance_samples=0)
        assert det.n == [len(w) for w in want] == det.n_stored
        for t in (det.recording, det.chunk, det.cls, det.kind, det.event):
            assert t.is_cuda and t.dtype == torch.int32 and t.dim() == 1 and t.shape[0] == sum(det.n)
        assert det.score.dtype == torch.float64
        assert _rows(det) == _flat(want)
        bare = collect((d_index, d_score, cases.N_CHUNKS), chunk_size, sens, level)
        assert _rows(bare) == _flat(_ref_detections(index, score, sens, level, chunk_size, None))
        assert bare.chunk.cpu().tolist() == det.chunk.cpu().tolist()
        assert not bare.kind.any() and bool((bare.event == -1).all())
        for kind in (mine_ref.HIT, mine_ref.DUPLICATE, mine_ref.FALSE_ALARM):
            sel = det.select(kind=kind)
            assert _rows(sel) == [w for w in _flat(want) if w[3] == kind]
            assert sel.n == [sum(1 for d in w if d[2] == kind) for w in want]
        want_t = [k * chunk_size / 16000.0 for _, k, _, _, _, _ in _flat(want)]
        assert det.times(sample_rate=16000).cpu().tolist() == want_t


def test_collect_overflow_and_counting_only(torch, synthetic):
    """The C entry point with max_det below the count: n_det is the true count, the first max_det records are stored, the
    other slots (and everything past them in a guarded buffer) are defined; max_det = 0 writes the counts alone."""
    from kws_amd import lib as L
    from kws_amd.stream import collect
    index, score, d_index, d_score = synthetic
    want = _ref_detections(index, score, 0.25, 1, 4096, cases.EVENTS)
    assert [len(w) for w in want] == [0, 0, 10, 4, 4, 18]
    ev_rows = cases.EVENTS
    off = np.concatenate(([0], np.cumsum([len(v) for v in ev_rows]))).astype(np.int32)
    flat = np.array([e for v in ev_rows for e in v], np.int32)
    d_ev = [torch.from_numpy(a).cuda() for a in (off, flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 2].copy())]
    d_chunks = torch.tensor(cases.N_CHUNKS, dtype=torch.int32, device="cuda")
    lib, st = L.get_lib(), torch.cuda.current_stream().cuda_stream
    for cap in (2, 0, 12):
        n_det = torch.full((6,), -7, dtype=torch.int32, device="cuda")
        det = torch.full((6 * cap + 1, 4), 99, dtype=torch.int32, device="cuda")           # one guard row behind the output
        det_score = torch.full((6 * cap + 1,), 99.0, dtype=torch.float64, device="cuda")
        L.check(lib.kws_stream_collect(d_index.data_ptr(), d_score.data_ptr(), 6, cases.STRIDE, d_chunks.data_ptr(), 0, 4096, 0.25, 1,
                                       *[t.data_ptr() for t in d_ev], cap, n_det.data_ptr(), det.data_ptr() if cap else None,
                                       det_score.data_ptr() if cap else None, st))
        assert n_det.cpu().tolist() == [0, 0, 10, 4, 4, 18]
        got, got_score = det.cpu().numpy(), det_score.cpu().numpy()
        assert (got[6 * cap:] == 99).all() and (got_score[6 * cap:] == 99.0).all()
        for r, w in enumerate(want):
            rows = [list(d[:4]) for d in w[:cap]] + [[-1, -1, 0, -1]] * max(0, cap - len(w))
            assert got[r * cap:(r + 1) * cap].tolist() == rows
            assert got_score[r * cap:(r + 1) * cap].tolist() == [d[4] for d in w[:cap]] + [0.0] * max(0, cap - len(w))
    two = collect((d_index, d_score, cases.N_CHUNKS), 4096, 0.25, 1, events=cases.sample_events(4096), tolerance_samples=0, max_det=2)
    assert two.n == [0, 0, 10, 4, 4, 18] and two.n_stored == [0, 0, 2, 2, 2, 2]
    assert _rows(two) == _flat([w[:2] for w in want])
    none = collect((d_index, d_score, cases.N_CHUNKS), 4096, 0.25, 1, max_det=0)
    assert none.n == [0, 0, 10, 4, 4, 18] and len(none) == 0
    empty = collect((d_index[:0], d_score[:0], []), 1024)
    assert empty.n == [] and len(empty) == 0


def test_collect_at_the_scans_own_point_is_its_fired_flags(torch):
    """kws_stream_scan_postprocess on planted probabilities, one tile, a fresh state: `collect` on the (index, score) it wrote,
    at the same point, gives exactly the chunks it marked `fired`."""
    from classifier.params import pr
    from kws_amd import lib as L
    from kws_amd.stream import ThresholdDecoder, collect
    R, n, C = 3, 70, 5
    rng = np.random.default_rng(5)
    logits = rng.normal(0, 1, (R, n, C))
    for r, (a, b, cls, gain) in enumerate([(2, 40, 2, 9.0), (5, 66, 4, 16.0), (10, 70, 1, 12.0)]):
        logits[r, a:b, cls] += gain
    logits[2, 24:27, 0] += 30.0
    e = np.exp(logits - logits.max(axis=-1, keepdims=True))
    probs = torch.from_numpy((e / e.sum(axis=-1, keepdims=True)).astype(np.float32)).cuda()
    n_chunks = [70, 66, 70]
    d_chunks = torch.tensor(n_chunks, dtype=torch.int32, device="cuda")
    dec = ThresholdDecoder(pr.threshold_config, pr.threshold_center)
    state = torch.tensor([[0, -1]] * R, dtype=torch.int32, device="cuda")
    index = torch.full((R, n), 3, dtype=torch.int32, device="cuda")
    score = torch.full((R, n), 1.0, dtype=torch.float64, device="cuda")
    fired = torch.zeros((R, n), dtype=torch.int32, device="cuda")
    L.check(L.get_lib().kws_stream_scan_postprocess(dec.handle, probs.data_ptr(), R, n, C, d_chunks.data_ptr(), 0, 0, 0.2, 1, 1024,
                                                    state.data_ptr(), index.data_ptr(), score.data_ptr(), fired.data_ptr(), n,
                                                    torch.cuda.current_stream().cuda_stream))
    want = [(int(r), int(k)) for r, k in np.argwhere(fired.cpu().numpy() != 0)]
    assert len(want) >= 3, "the scan fires fewer than 3 times: %s" % want
    det = collect((index, score, n_chunks), 1024, 0.2, 1)
    assert list(zip(det.recording.cpu().tolist(), det.chunk.cpu().tolist())) == want
    assert det.cls.cpu().tolist() == [int(index[r, k]) for r, k in want]


def _peak_rows(det):
    return list(zip(det.recording.cpu().tolist(), det.chunk.cpu().tolist(), det.cls.cpu().tolist(), det.score.cpu().tolist()))


def _ref_peaks(index, score, n_chunks, min_score, min_gap, K, events):
    return [(r, k, c, sc) for r, n in enumerate(n_chunks)
            for k, c, sc in mine_ref.peaks(index[r], score[r], n, 0, min_score, min_gap, K, None if events is None else events[r])]


@pytest.mark.parametrize("labelled", [False, True])
def test_peaks_equal_the_reference_on_the_synthetic_scan(torch, synthetic, labelled):
    from kws_amd.stream import peaks
    index, score, d_index, d_score = synthetic
    kw = dict(events=cases.sample_events(1024), tolerance_samples=0) if labelled else {}
    for K in (1, 4, 8, 64):
        for gap in (1, 8, 16):
            want = _ref_peaks(index, score, cases.N_CHUNKS, 0.3, gap, K, cases.EVENTS if labelled else None)
            det = peaks((d_index, d_score, cases.N_CHUNKS), 1024, k=K, min_score=0.3, min_gap=gap, **kw)
            assert _peak_rows(det) == want, (K, gap)
            assert det.n == [sum(1 for w in want if w[0] == r) for r in range(6)] and max(det.n) <= K
            assert not det.kind.any() and bool((det.event == -1).all())
    got = [k for r, k, _, _ in _peak_rows(peaks((d_index, d_score, cases.N_CHUNKS), 1024, k=8, min_score=0.3, min_gap=8, **kw)) if r == 5]
    assert got == ([31, 39, 63, 50] if labelled else [5, 13, 21, 29, 37, 63, 76, 103])
    dflt = peaks((d_index, d_score, cases.N_CHUNKS), 1024, **kw)                          # min_gap = ceil(16000 / 1024) = 16, min_score 0
    assert _peak_rows(dflt) == _ref_peaks(index, score, cases.N_CHUNKS, 0.0, 16, 8, cases.EVENTS if labelled else None)


def test_peaks_break_ties_toward_the_lowest_chunk(torch, tie):
    """64, 257 and 1000 chunks with scores from five values: equal scores in every 64-lane stride, and in the raw output the
    unused slots are {-1, -1} with score 0 and nothing behind them is written."""
    from kws_amd import lib as L
    from kws_amd.stream import peaks
    index, score, d_index, d_score = tie
    n_chunks = mine_ref.TIE_N_CHUNKS
    for K, gap in ((1, 1), (8, 8), (64, 1), (64, 16), (33, 3)):
        want = _ref_peaks(index, score, n_chunks, 0.0, gap, K, None)
        assert _peak_rows(peaks((d_index, d_score, n_chunks), 1024, k=K, min_gap=gap)) == want, (K, gap)
    events = [[(1, 0, 20)], [(2, 100, 180), (1, 250, 256)], [(3, 5, 5), (4, 64, 127), (1, 990, 999)]]
    want = _ref_peaks(index, score, n_chunks, 0.35, 4, 64, events)
    got = peaks((d_index, d_score, n_chunks), 1024, k=64, min_score=0.35, min_gap=4,
                events=[[(c, lo * 1024, (hi + 1) * 1024) for c, lo, hi in v] for v in events], tolerance_samples=0)
    assert _peak_rows(got) == want and len(want) > 64
    K = 64
    d_chunks = torch.tensor(n_chunks, dtype=torch.int32, device="cuda")
    n_peaks = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    out = torch.full((3 * K + 1, 2), 99, dtype=torch.int32, device="cuda")
    out_score = torch.full((3 * K + 1,), 99.0, dtype=torch.float64, device="cuda")
    L.check(L.get_lib().kws_stream_peaks(d_index.data_ptr(), d_score.data_ptr(), 3, mine_ref.TIE_STRIDE, d_chunks.data_ptr(), 0, 0.0, 16,
                                         None, None, None, K, n_peaks.data_ptr(), out.data_ptr(), out_score.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream))
    want = [mine_ref.peaks(index[r], score[r], n, 0, 0.0, 16, K) for r, n in enumerate(n_chunks)]
    assert n_peaks.cpu().tolist() == [len(w) for w in want] and min(len(w) for w in want) < K
    got, got_score = out.cpu().numpy(), out_score.cpu().numpy()
    assert (got[3 * K:] == 99).all() and got_score[3 * K] == 99.0
    for r, w in enumerate(want):
        assert got[r * K:(r + 1) * K].tolist() == [[k, c] for k, c, _ in w] + [[-1, -1]] * (K - len(w))
        assert got_score[r * K:(r + 1) * K].tolist() == [sc for _, _, sc in w] + [0.0] * (K - len(w))


@pytest.fixture(scope="module")
def recordings():
    """seeded int16 recordings of cases.N_CHUNKS chunks of 1024 samples, the last chunk 300 samples short"""
    rng = np.random.default_rng(41)
    lens = [max(0, n * 1024 - 300) for n in cases.N_CHUNKS]
    assert [-(-n // 1024) for n in lens] == cases.N_CHUNKS
    return [rng.integers(-32768, 32768, n).astype(np.int16) for n in lens], lens


def test_clips_are_the_listeners_audio_buffer(torch, synthetic, recordings):
    from classifier.params import pr
    from kws_amd.stream import collect, peaks
    _, _, d_index, d_score = synthetic
    pcms, lens = recordings
    B = pr.buffer_samples
    scan = (d_index, d_score, cases.N_CHUNKS)
    pk = peaks(scan, 1024, k=64, min_score=0.5, min_gap=1)
    det = collect(scan, 1024, 0.25, 1)
    for d in (pk, det):
        clips = d.clips(pcms, pr=pr)
        assert clips.is_cuda and clips.dtype == torch.float32 and tuple(clips.shape) == (len(d), B) and len(d) > 10
        got = clips.cpu().numpy().astype(np.float64)
        pairs = list(zip(d.recording.cpu().tolist(), d.chunk.cpu().tolist()))
        for i, (r, k) in enumerate(pairs):
            np.testing.assert_array_equal(got[i], mine_ref.audio_buffer(pcms[r], k, 1024, B), err_msg="recording %d chunk %d" % (r, k))
        if d is pk:
            assert (1, 0) in pairs                                                       # 724 samples behind B - 724 zeros
            i = pairs.index((1, 0))
            assert not got[i, :B - lens[1]].any() and got[i, B - lens[1]:].any()
            assert any(k == cases.N_CHUNKS[r] - 1 and r > 1 for r, k in pairs), "no clip ends in a short last chunk"
            assert any((k + 1) * 1024 > B for r, k in pairs) and any((k + 1) * 1024 < B for r, k in pairs)
    # a padded (R, n) tensor with lengths is the same audio
    stride = max(lens) + 3
    packed = np.full((6, stride), 1234, np.int16)
    for r, p in enumerate(pcms):
        packed[r, :p.size] = p
    assert torch.equal(det.clips(torch.from_numpy(packed).cuda(), lengths=lens, pr=pr), det.clips(pcms, pr=pr))
    with pytest.raises(ValueError):
        det.clips(None)
    assert tuple(collect(scan, 1024, 1.0, 6).clips(pcms).shape) == (0, B)


def _read(path):
    with wave.open(path, "rb") as wf:
        assert (wf.getnchannels(), wf.getsampwidth(), wf.getframerate()) == (1, 2, 16000)
        return np.frombuffer(wf.readframes(wf.getnframes()), dtype="<i2")


def test_save_writes_the_truncated_samples_in_the_listeners_layout(torch, synthetic, recordings, tmp_path):
    from classifier.params import pr
    from kws_amd.stream import collect, peaks
    _, _, d_index, d_score = synthetic
    pcms, _ = recordings
    B = pr.buffer_samples
    scan = (d_index, d_score, cases.N_CHUNKS)
    det = collect(scan, 1024, 0.5, 3)
    rows = _rows(det)
    assert len(rows) == 7
    out = str(tmp_path / "fa")
    paths = det.save(pcms, out, NAMES, session_id="000123456", pr=pr)
    assert paths == [os.path.join(out, NAMES[c], "000123456_%d.wav" % i) for i, (_, _, c, _, _, _) in enumerate(rows)]
    differs = 0
    for path, (r, k, _, _, _, _) in zip(paths, rows):
        buf = mine_ref.audio_buffer(pcms[r], k, 1024, B)
        got = _read(path)
        np.testing.assert_array_equal(got, mine_ref.saved_samples(buf))
        np.testing.assert_array_equal(got, np.trunc(buf * 32768 * 32767 / 32768).astype(np.int16))
        differs += int((got != (buf * 32768).astype(np.int16)).sum())
    assert differs > 0                                                                   # not a copy of the PCM
    more = det.save(pcms, out, NAMES, session_id="000123456", pr=pr, record_start=len(rows))
    assert len(set(paths + more)) == 2 * len(rows)
    pk = peaks(scan, 1024, k=2, min_score=0.3)
    stems = ["rec%d" % r for r in range(6)]
    named = pk.save(pcms, str(tmp_path / "near_miss"), NAMES, names=stems, pr=pr)
    assert named == [os.path.join(str(tmp_path / "near_miss"), NAMES[c], "rec%d_%d.wav" % (r, k)) for r, k, c, _ in _peak_rows(pk)]
    assert len(named) >= 6 and all(os.path.getsize(p) == 44 + 2 * B for p in named)
    auto = det.save(pcms, str(tmp_path / "auto"), NAMES, pr=pr)                           # nine random digits, listen.py:94
    sid = os.path.basename(auto[0]).split("_")[0]
    assert len(sid) == 9 and sid.isdigit() and [os.path.basename(p) for p in auto] == ["%s_%d.wav" % (sid, i) for i in range(len(rows))]


def test_collect_and_peaks_are_deterministic(torch, synthetic, tie):
    from kws_amd.stream import collect, peaks
    _, _, d_index, d_score = synthetic
    kw = dict(events=cases.sample_events(3000), tolerance_samples=0)
    a, b = (collect((d_index, d_score, cases.N_CHUNKS), 3000, 0.25, 1, **kw) for _ in range(2))
    assert len(a) > 0
    for x, y in zip((a.recording, a.chunk, a.cls, a.kind, a.event, a.score), (b.recording, b.chunk, b.cls, b.kind, b.event, b.score)):
        assert torch.equal(x, y)
    _, _, t_index, t_score = tie
    a, b = (peaks((t_index, t_score, mine_ref.TIE_N_CHUNKS), 1024, k=64, min_gap=2) for _ in range(2))
    assert len(a) > 100
    for x, y in zip((a.recording, a.chunk, a.cls, a.score), (b.recording, b.chunk, b.cls, b.score)):
        assert torch.equal(x, y)


def _write_wav(path, pcm):
    with wave.open(path, "wb") as wf:
        wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(16000)
        wf.writeframes(pcm.tobytes())


def _saved(paths):
    return sorted((os.path.basename(os.path.dirname(p)), _read(p).tobytes()) for p in paths)


def test_listener_saves_the_same_clips_chunk_by_chunk_and_at_once(torch, tmp_path):
    """run_wav with save_dir (on_activation saves the host ring) and --scan with save_dir (collect -> save) write the same
    clips; labels that declare one activation a keyword keep it out of the default false_alarms; and --sweep with
    --max_fa_per_hour saves what `collect` gives at the chosen point, from the sweep's own scan."""
    from classifier.model import get_model
    from classifier.params import pr
    from kws_amd.init import init_weights
    from kws_amd.stream import collect
    from listen import Listener
    classes = tmp_path / "classes.txt"
    classes.write_text("\n".join(NAMES) + "\n")
    rng = np.random.default_rng(3)
    pcms = [np.clip(rng.normal(0, 4000, n), -32768, 32767).astype(np.int16) for n in (3 * 16000 + 700, 16000 + 5)]
    os.mkdir(str(tmp_path / "wavs"))
    paths = [str(tmp_path / "wavs" / ("in%d.wav" % i)) for i in range(2)]
    for p, pcm in zip(paths, pcms):
        _write_wav(p, pcm)
    m = get_model("simple_cnn", 5)
    ws = init_weights(m.spec, seed=4)
    ws[-2] = ws[-2] * 16.0                                  # tests/test_scan_gpu.py's HEAD_GAIN: spreads the seeded model's probabilities
    m.set_weights(ws)
    common = dict(model=m, classes_path=str(classes), chunk_size=1024, sensitivity=0.1, trigger_level=1)
    live = []
    for i, p in enumerate(paths):
        lis = Listener(input_wav=p, save_dir=str(tmp_path / ("live%d" % i)), **common)
        results = lis.run_wav(quiet=True)
        assert len(lis.saved_paths) == sum(1 for _, _, f in results if f) == lis.record_num
        assert [os.path.basename(q) for q in lis.saved_paths] == ["%s_%d.wav" % (lis.session_id, j) for j in range(lis.record_num)]
        live.append(lis.saved_paths)
    print("activations per file", [len(v) for v in live])
    assert len(live[0]) >= 1
    lis = Listener(input_wav=str(tmp_path / "wavs"), save_dir=str(tmp_path / "scan"), scan=True, **common)
    lis.run()
    assert len(lis.collected_paths) == len(live[0]) + len(live[1])
    assert _saved(lis.collected_paths) == _saved(live[0] + live[1])
    assert all(os.path.dirname(os.path.dirname(q)) == str(tmp_path / "scan") for q in lis.collected_paths)
    # the first activation of the first file is declared a keyword
    det = lis.collect_wav(paths[0], save_dir="")
    r0, k0, c0 = _rows(det)[0][:3]
    labels = {"in0.wav": [(c0, k0 * 1024, (k0 + 1) * 1024)]}
    lab = Listener(save_dir=str(tmp_path / "labelled"), **common)
    det = lab.collect_wav(paths, labels, tolerance_s=0.0)
    kinds = det.kind.cpu().tolist()
    assert kinds[0] == mine_ref.HIT and kinds.count(mine_ref.HIT) == 1 and set(kinds[1:]) <= {mine_ref.FALSE_ALARM}
    assert len(lab.collected_paths) == len(kinds) - 1
    assert _saved(lab.collected_paths) == _saved((live[0] + live[1])[1:])
    lab.collect_wav(paths, labels, tolerance_s=0.0, save_dir=str(tmp_path / "hits"), save_kind="hits")
    assert _saved(lab.collected_paths) == _saved(live[0][:1])
    # near misses next to them
    lab.collect_wav(paths, labels, tolerance_s=0.0, save_dir=str(tmp_path / "mined"), mine_peaks=3, min_peak_score=0.0)
    near = [q for q in lab.collected_paths if os.sep + "near_miss" + os.sep in q]
    assert len(near) == len(lab.near_misses) >= 1 and all(os.path.basename(q).startswith(("in0_", "in1_")) for q in near)
    assert k0 not in [k for r, k in zip(lab.near_misses.recording.cpu().tolist(), lab.near_misses.chunk.cpu().tolist()) if r == 0]
    # the sweep's chosen point, collected from the sweep's scan
    labels_file = tmp_path / "labels.txt"
    labels_file.write_text("in0.wav %s %.6f %.6f\n" % (NAMES[c0], k0 * 1024 / 16000.0, (k0 + 1) * 1024 / 16000.0))
    sw = Listener(input_wav=str(tmp_path / "wavs"), save_dir=str(tmp_path / "sweep"), sweep=True, labels_path=str(labels_file), sensitivities="0.1,0.5,0.9",
                  trigger_levels="1,3", tolerance_s=0.0, max_fa_per_hour=1e9, save_kind="all", **common)
    res = sw.run()
    best = res.best(max_fa_per_hour=1e9)
    want = collect(sw.sweep_scan, 1024, best["sensitivity"], best["trigger_level"])
    assert len(want) >= 1 and len(sw.collected_paths) == len(want)
    assert _saved(sw.collected_paths) == sorted((NAMES[c], mine_ref.saved_samples(mine_ref.audio_buffer(pcms[r], k, 1024, pr.buffer_samples)).tobytes())
                                                for r, k, c, _, _, _ in _rows(want))
