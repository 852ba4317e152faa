"""GPU tests of the query-by-example feature (csrc/kws_dtw.hip: kws_dtw, kws_dtw_peaks; kws_amd.qbe;
tools/audio_process/keyword_search.py) against the numpy reference of tests/dtw_ref.py at the cases of tests/dtw_cases.py."""
import csv
import importlib.util
import os
import wave

import numpy as np
import pytest

import dtw_cases as dc
import dtw_ref as dr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _raw_dtw(torch, templates, lengths, rows, n_frames, metric, tile_frames=0):
    """kws_dtw itself; the outputs start from values the kernel never writes"""
    from kws_amd import lib as L
    lib = L.get_lib()
    Q, Lmax, D = templates.shape
    R, F, _ = rows.shape
    t, x = torch.from_numpy(np.ascontiguousarray(templates)).cuda(), torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    tl, n = torch.from_numpy(np.asarray(lengths, np.int32)).cuda(), torch.from_numpy(np.asarray(n_frames, np.int32)).cuda()
    cost = torch.full((R, Q, F), float("nan"), dtype=torch.float32, device="cuda")
    start = torch.full((R, Q, F), -7, dtype=torch.int32, device="cuda")
    need = int(lib.kws_dtw_workspace_bytes(R, Q, F, D, tile_frames))
    assert need >= 0
    ws = torch.empty((max(need, 1),), dtype=torch.uint8, device="cuda")
    L.check(lib.kws_dtw(t.data_ptr(), tl.data_ptr(), Q, Lmax, x.data_ptr(), n.data_ptr(), R, F, D, metric, tile_frames, cost.data_ptr(),
                        start.data_ptr(), ws.data_ptr() if need else None, need, torch.cuda.current_stream().cuda_stream))
    return cost.cpu().numpy(), start.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- exact cases ----------------------------------------------------------------------------------------------------------------
_exact = {}


def _exact_run(torch, D):
    if D not in _exact:
        data = dc.exact_data(D)
        _exact[D] = (data, _raw_dtw(torch, *data, dr.L2), dc.expected(("exact", D), *data, dr.L2))
    return _exact[D]


@pytest.mark.parametrize("L_", dc.LENGTHS)
@pytest.mark.parametrize("D", dc.WIDTHS + dc.MID_WIDTHS)
def test_exact(torch, D, L_):
    """integer rows, squared distance: the same bits as the reference for every frame count of the table, frames past a recording's
    length +inf / -1, and nothing left unwritten"""
    (_, lengths, _, n_frames), (cost, start), (want_cost, want_start) = _exact_run(torch, D)
    k = dc.LENGTHS.index(L_)
    for r, n in enumerate(n_frames):
        np.testing.assert_array_equal(_bits(cost[r, k]), _bits(want_cost[r, k]), err_msg="cost, n = %d" % n)
        np.testing.assert_array_equal(start[r, k], want_start[r, k], err_msg="start, n = %d" % n)
        assert np.isinf(cost[r, k, n:]).all() and (start[r, k, n:] == -1).all()
        h = dc.unreachable(L_)
        assert np.isinf(cost[r, k, :min(h, n)]).all() and np.isfinite(cost[r, k, h:n]).all()


def test_exact_width_below_its_kernel(torch):
    """28 columns run in the kernel of 32: the staged rows are padded inside LDS, the rows in memory are not"""
    lengths = np.array([1, 33, 64], np.int32)
    t, x = dc.int_rows(11, 3, 64, 28), dc.int_rows(12, 2, 131, 28)
    n = np.array([131, 70], np.int32)
    for metric in (dr.L2, dr.DOT):
        cost, start = _raw_dtw(torch, t, lengths, x, n, metric)
        want_cost, want_start = dr.dtw_many(t, lengths, x, n, metric)
        np.testing.assert_array_equal(_bits(cost), _bits(want_cost))
        np.testing.assert_array_equal(start, want_start)


# ---- tiling ---------------------------------------------------------------------------------------------------------------------
def test_every_tile_size_gives_the_same_bits(torch):
    data = dc.tile_data()
    want_cost, want_start = dc.expected("tiles", *data, dr.L2)
    real = (data[0] * np.float32(0.173), data[1], data[2] * np.float32(0.291), data[3])          # inexact sums: the order of the additions shows
    first = None
    for tile in dc.TILES:
        cost, start = _raw_dtw(torch, *data, dr.L2, tile_frames=tile)
        np.testing.assert_array_equal(_bits(cost), _bits(want_cost), err_msg="tile_frames = %d" % tile)
        np.testing.assert_array_equal(start, want_start, err_msg="tile_frames = %d" % tile)
        got = _raw_dtw(torch, *real, dr.DOT, tile_frames=tile)
        if first is None:
            first = got
        np.testing.assert_array_equal(_bits(got[0]), _bits(first[0]), err_msg="real-valued, tile_frames = %d" % tile)
        np.testing.assert_array_equal(got[1], first[1], err_msg="real-valued, tile_frames = %d" % tile)


# ---- one ragged call ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", (dr.L2, dr.DOT), ids=("l2", "dot"))
def test_ragged_call(torch, metric):
    data = dc.ragged_data()
    cost, start = _raw_dtw(torch, *data, metric)
    want_cost, want_start = dc.expected(("ragged", metric), *data, metric)
    np.testing.assert_array_equal(_bits(cost), _bits(want_cost))
    np.testing.assert_array_equal(start, want_start)
    for r, n in enumerate(dc.RAGGED_FRAMES):
        assert np.isinf(cost[r, :, n:]).all() and (cost[r, :, n:] > 0).all() and (start[r, :, n:] == -1).all()


# ---- real-valued cosine -----------------------------------------------------------------------------------------------------------
def test_cosine_against_float64(torch):
    t, lengths, x, n = dc.cosine_data()
    cost, start = _raw_dtw(torch, t, lengths, x, n, dr.DOT)
    want, _ = dc.expected("cosine", t, lengths, x, n, dr.DOT, np.float64)
    for k, L_ in enumerate(lengths):
        for r in range(x.shape[0]):
            live = np.isfinite(want[r, k])
            np.testing.assert_array_equal(np.isfinite(cost[r, k]), live)
            err = float(np.abs(cost[r, k, live].astype(np.float64) - want[r, k, live]).max())
            print("cosine L = %d, recording %d: max |error| %.3g, bound %.3g" % (L_, r, err, dc.cosine_bound(L_)))
            assert err <= dc.cosine_bound(L_)
            j = np.nonzero(live)[0]
            s = start[r, k, live]
            assert (s >= j - 2 * (L_ - 1)).all() and (s <= j - (L_ + 2) // 2 + 1).all() and (s >= 0).all()
            assert (start[r, k, ~live] == -1).all()


# ---- peaks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.PEAK_CASES, ids=lambda c: c[0])
def test_peaks(torch, case):
    from kws_amd import lib as L
    _, group, threshold, min_gap, K = case
    cost, start = dc.peak_data()
    R, Q, F = cost.shape
    G = max(group) + 1
    gh = np.array(group, np.int32)
    d = [torch.from_numpy(a).cuda() for a in (cost, start, gh)]
    count = torch.full((R, G), -7, dtype=torch.int32, device="cuda")
    end, hs, ht = (torch.full((R, G, K), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    hc = torch.full((R, G, K), float("nan"), dtype=torch.float32, device="cuda")
    L.check(L.get_lib().kws_dtw_peaks(d[0].data_ptr(), d[1].data_ptr(), R, Q, F, d[2].data_ptr(), gh.ctypes.data, G, threshold, min_gap, K,
                                      count.data_ptr(), end.data_ptr(), hs.data_ptr(), hc.data_ptr(), ht.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream))
    want = dr.peaks(cost, start, gh, G, threshold, min_gap, K)
    for name, got, w in zip(("count", "end", "start", "cost", "template"), (count, end, hs, hc, ht), want):
        np.testing.assert_array_equal(got.cpu().numpy(), w, err_msg=name)
    if case[0] == "k_reached":
        assert (want[0][:R - 1] == K).all()
    if case[0] in ("nothing_below",):
        assert (want[0] == 0).all()
    if case[0] == "gap_past_n":
        assert (want[0][:R - 1] == 1).all()
    assert (want[0][R - 1] == 0).all()                                   # the recording of +inf only


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def _load_tool():
    path = os.path.join(ROOT, "tf-keras-speech-commands_amd", "tools", "audio_process", "keyword_search.py")
    spec = importlib.util.spec_from_file_location("keyword_search_tool", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _write_wav(path, pcm):
    with wave.open(path, "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(dc.RATE)
        wf.writeframes(np.asarray(pcm, "<i2").tobytes())


_scene = {}


def _searched():
    """the scene, the templates enrolled from the unstretched words and the hits of one search, shared by the two tests below"""
    if not _scene:
        from classifier.params import pr
        from kws_amd import qbe
        names = list(dc.WORDS)
        t = qbe.Templates.enroll(pr, [dc.example(n) for n in names], names)
        recs, planted = dc.scene()
        hits = qbe.search(t, recs, threshold=float("inf"), max_hits=dc.PLANTED_PER_PAIR)
        _scene.update(names=names, t=t, recs=recs, planted=planted, hits=hits)
    return _scene


def test_search_finds_the_planted_words(torch):
    from classifier.params import pr
    from kws_amd import qbe
    sc = _searched()
    names, t, recs, planted, hits = sc["names"], sc["t"], sc["recs"], sc["planted"], sc["hits"]
    W, H = pr.window_samples, pr.hop_samples
    assert t.keywords == names and len(t) == 2 and (t.lengths >= 10).all() and (t.lengths <= 64).all()
    assert len(hits) == len(planted)
    want = sorted((r, names.index(n), dc.planted_end_frame(e, W, H)) for r, n, _, e in planted)
    got = list(zip(hits.recording.tolist(), hits.keyword.tolist(), hits.end_frame.tolist()))
    assert got == sorted(got)                                            # (recording, keyword, end)
    for (r, k, e), (wr, wk, we) in zip(got, want):
        assert (r, k) == (wr, wk) and abs(e - we) <= 3, (got, want)
    np.testing.assert_allclose(hits.end_s, (hits.end_frame * H + W) / dc.RATE)
    np.testing.assert_allclose(hits.start_s, hits.start_frame * H / dc.RATE)
    assert (hits.start_frame >= 0).all() and (hits.start_frame < hits.end_frame).all() and np.isfinite(hits.cost).all()
    # the same bits whatever the tile
    c0, s0 = qbe.match(t, recs)
    c1, s1 = qbe.match(t, recs, tile_frames=32)
    assert torch.equal(c0.view(torch.int32), c1.view(torch.int32)) and torch.equal(s0, s1)
    # one-second clips around each occurrence
    clips = np.stack([dc.clip_around(recs[r], b, e) for r, _, b, e in planted])
    word, cost = qbe.classify(t, clips)
    assert [names[i] for i in word] == [n for _, n, _, _ in planted] and np.isfinite(cost).all()


def test_tool_writes_the_same_hits(torch, tmp_path):
    from classifier.params import pr
    sc = _searched()
    names, recs, hits = sc["names"], sc["recs"], sc["hits"]
    W, H = pr.window_samples, pr.hop_samples
    enroll_dir, wav_dir, save_dir = (str(tmp_path / d) for d in ("enroll", "wavs", "cuts"))
    for n in names:
        os.makedirs(os.path.join(enroll_dir, n))
        _write_wav(os.path.join(enroll_dir, n, "ex0.wav"), dc.example(n))
    os.makedirs(wav_dir)
    for r, rec in enumerate(recs):
        _write_wav(os.path.join(wav_dir, "rec%d.wav" % r), rec)
    out_csv = str(tmp_path / "hits.csv")
    _load_tool().main(["--enroll_path", enroll_dir, "--input_wav", wav_dir, "--threshold", "inf", "--max_hits", str(dc.PLANTED_PER_PAIR),
                       "--output_csv", out_csv, "--save_dir", save_dir])
    with open(out_csv) as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == len(hits)
    for row, (r, kw, _, a, b, c) in zip(rows, hits.rows()):
        assert row["file"] == "rec%d.wav" % r and row["keyword"] == kw
        assert abs(float(row["start_s"]) - a) < 1e-3 and abs(float(row["end_s"]) - b) < 1e-3 and abs(float(row["cost"]) - c) < 1e-5
    cuts = sorted(os.listdir(os.path.join(save_dir, names[0])))
    assert len(cuts) == 2 * dc.PLANTED_PER_PAIR and cuts[0] == "rec0_0.wav"
    with wave.open(os.path.join(save_dir, names[0], cuts[0]), "rb") as wf:
        assert wf.getframerate() == dc.RATE and wf.getnframes() == (hits.end_frame[0] - hits.start_frame[0]) * H + W
