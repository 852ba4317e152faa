"""GPU tests of the operating-point sweep (kws_stream_sweep, kws_amd.stream.sweep, Listener.sweep_wav) against the pure-Python
restatement tests/sweep_ref.py.  Every comparison is exact integer equality: the kernel reads the same doubles and compares with
the same strict `>`.  The synthetic scan is tests/sweep_cases.py; tests/test_sweep_host.py checks on the reference alone that
it exercises every counter, and the comparisons here assert it again before the device is looked at."""
import wave

import numpy as np
import pytest

import sweep_cases as cases
import sweep_ref

pytestmark = pytest.mark.gpu

NAMES = ["background", "up", "down", "left", "right"]


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
def reference(synthetic):
    """chunk_size -> (R, S, L, 5) reference counts with labels, computed once and left unchanged"""
    index, score = synthetic[:2]
    out = {}
    for c in cases.CHUNK_SIZES:
        out[c] = sweep_ref.sweep(index, score, cases.N_CHUNKS, cases.BACKGROUND, cases.SENSITIVITIES, cases.TRIGGER_LEVELS, c, cases.EVENTS)
        out[c].setflags(write=False)
    return out


def _counts(res):
    """SweepResult -> (R, S, L, 5) host array in sweep_ref's order"""
    return np.stack([t.cpu().numpy() for t in (res.fires, res.hits, res.false_alarms, res.duplicates, res.latency_chunks)], axis=-1)


@pytest.mark.parametrize("chunk_size", cases.CHUNK_SIZES)
def test_sweep_counters_equal_the_reference(torch, synthetic, reference, chunk_size):
    """P = 70 (a full wave and a partial one) over recordings of 0, 1, 63, 64, 65 and 130 chunks with poisoned padding: all
    five counters with labels; fires alone, and zeros, without."""
    from kws_amd.stream import sweep
    want = reference[chunk_size]
    cases.check_reference(want)
    _, _, d_index, d_score = synthetic
    lens = [n * chunk_size for n in cases.N_CHUNKS]
    res = sweep((d_index, d_score, cases.N_CHUNKS), cases.SENSITIVITIES, cases.TRIGGER_LEVELS, chunk_size, events=cases.sample_events(chunk_size),
                lengths=lens, tolerance_samples=0)
    assert res.n_events == [len(e) for e in cases.EVENTS]
    for t in (res.fires, res.hits, res.false_alarms, res.duplicates, res.latency_chunks):
        assert t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == (6, 14, 5)
    got = _counts(res)
    for i, name in enumerate(("fires", "hits", "false_alarms", "duplicates", "latency_chunks")):
        np.testing.assert_array_equal(got[..., i], want[..., i], err_msg=name)
    bare = sweep((d_index, d_score, cases.N_CHUNKS), cases.SENSITIVITIES, cases.TRIGGER_LEVELS, chunk_size)
    assert bare.n_events == [0] * 6
    got = _counts(bare)
    np.testing.assert_array_equal(got[..., 0], want[..., 0])
    assert not got[..., 1:].any()


def test_sweep_of_one_point(torch, synthetic, reference):
    """P = 1: one lane of the wave owns a point, 63 are idle"""
    from kws_amd.stream import sweep
    _, _, d_index, d_score = synthetic
    s, l = cases.SENSITIVITIES.index(0.5), cases.TRIGGER_LEVELS.index(3)
    want = reference[1024][:, s, l]
    assert want[:, sweep_ref.FIRES].sum() > 0
    res = sweep((d_index, d_score, cases.N_CHUNKS), [0.5], [3], 1024, events=cases.sample_events(1024), tolerance_samples=0)
    np.testing.assert_array_equal(_counts(res)[:, 0, 0], want)


def test_sweep_is_deterministic_and_handles_empty_grids(torch, synthetic):
    from kws_amd.stream import sweep
    _, _, d_index, d_score = synthetic
    args = ((d_index, d_score, cases.N_CHUNKS), cases.SENSITIVITIES, cases.TRIGGER_LEVELS, 3000)
    a = _counts(sweep(*args, events=cases.sample_events(3000), tolerance_samples=0))
    b = _counts(sweep(*args, events=cases.sample_events(3000), tolerance_samples=0))
    assert a[..., 0].sum() > 0
    np.testing.assert_array_equal(a, b)
    none = sweep((d_index, d_score, cases.N_CHUNKS), [], cases.TRIGGER_LEVELS, 1024)
    assert tuple(none.fires.shape) == (6, 0, 5)
    empty = sweep((d_index[:0], d_score[:0], []), [0.5], [3], 1024)
    assert tuple(empty.fires.shape) == (0, 1, 1) and empty.n_events == []
    with pytest.raises(ValueError):
        sweep((d_index, d_score, [cases.STRIDE + 1] * 6), [0.5], [3], 1024)            # a chunk count past the row
    with pytest.raises(ValueError):
        sweep((d_index, d_score.float(), cases.N_CHUNKS), [0.5], [3], 1024)


def test_sweep_agrees_with_scan_postprocess_per_point(torch):
    """The route a sweep replaces: kws_stream_scan_postprocess once per point on the same probabilities, R = 3, n = 40, C = 5.
    Its fired flags, summed per recording, are the sweep's fires on the index / score it wrote."""
    from classifier.params import pr
    from kws_amd import lib as L
    from kws_amd.stream import ThresholdDecoder, sweep
    R, n, C = 3, 40, 5
    rng = np.random.default_rng(5)
    logits = rng.normal(0, 1, (R, n, C))
    for r, (a, b, cls, gain) in enumerate([(2, 20, 2, 9.0), (5, 30, 4, 16.0), (10, 40, 1, 12.0)]):      # planted runs of one class
        logits[r, a:b, cls] += gain
    logits[2, 24:27, 0] += 30.0                                                                        # background in the middle
    e = np.exp(logits - logits.max(axis=-1, keepdims=True))
    probs = torch.from_numpy((e / e.sum(axis=-1, keepdims=True)).astype(np.float32)).cuda()
    n_chunks = [40, 33, 40]
    d_chunks = torch.tensor(n_chunks, dtype=torch.int32, device="cuda")
    dec = ThresholdDecoder(pr.threshold_config, pr.threshold_center)
    sens, levels = [0.2, 0.6, 0.9], [1, 4]
    lib = L.get_lib()
    st = torch.cuda.current_stream().cuda_stream
    fired_sums, written = [], []
    for s in sens:
        for lv in levels:
            state = torch.tensor([[0, -1]] * R, dtype=torch.int32, device="cuda")
            index = torch.full((R, n), 3, dtype=torch.int32, device="cuda")
            score = torch.full((R, n), 1.0, dtype=torch.float64, device="cuda")
            fired = torch.zeros((R, n), dtype=torch.int32, device="cuda")
            L.check(lib.kws_stream_scan_postprocess(dec.handle, probs.data_ptr(), R, n, C, d_chunks.data_ptr(), 0, 0, s, lv, 1024,
                                                    state.data_ptr(), index.data_ptr(), score.data_ptr(), fired.data_ptr(), n, st))
            fired_sums.append(fired.cpu().numpy().sum(axis=1))
            written.append((index, score))
    assert sum(int(f.sum() > 0) for f in fired_sums) >= 3, "the existing path fires at fewer than 3 of the 6 points: %s" % fired_sums
    assert len(set(tuple(f) for f in fired_sums)) > 1
    for index, score in written[1:]:                                     # the decoding does not depend on the point
        assert torch.equal(index, written[0][0]) and torch.equal(score, written[0][1])
    res = sweep((written[0][0], written[0][1], n_chunks), sens, levels, 1024)
    np.testing.assert_array_equal(res.fires.cpu().numpy().reshape(R, 6), np.stack(fired_sums, axis=1))


def test_listener_sweep_wav_is_the_reference_on_one_scan(torch, tmp_path):
    """Plumbing, end to end: two wavs and a labels file through Listener.sweep_wav equal sweep_ref walked on the index / score
    that one scan of the same files returns, with the labels converted by hand."""
    from classifier.model import get_model
    from classifier.params import pr
    from kws_amd.init import init_weights
    from kws_amd.stream import scan
    from listen import Listener
    classes = tmp_path / "classes.txt"
    classes.write_text("\n".join(NAMES) + "\n")
    rng = np.random.default_rng(3)
    pcms = [np.clip(rng.normal(0, 4000, n), -32768, 32767).astype(np.int16) for n in (3 * 16000 + 700, 3 * 16000 - 5)]
    paths = []
    for i, pcm in enumerate(pcms):
        paths.append(str(tmp_path / ("in%d.wav" % i)))
        with wave.open(paths[-1], "wb") as wf:
            wf.setnchannels(1); wf.setsampwidth(2); wf.setframerate(16000)
            wf.writeframes(pcm.tobytes())
    labels = tmp_path / "labels.txt"
    labels.write_text("# the second file is a negative recording\nin0.wav up 0.5 1.0\nin0.wav right 2.5 2.9\n")
    m = get_model("simple_cnn", 5)
    m.set_weights(init_weights(m.spec, seed=4))
    lis = Listener(model=m, classes_path=str(classes), chunk_size=1024)
    sens, levels = [0.0, 0.1, 0.3, 0.5], [0, 1, 3]
    res = lis.sweep_wav(paths, str(labels), sens, levels)
    assert res.n_events == [2, 0] and res.seconds == [len(p) / 16000.0 for p in pcms]
    assert res.sensitivities == sens and res.trigger_levels == levels
    one = scan(pr, m._device(), pcms, chunk_size=1024, class_names=NAMES, decoder=lis.threshold_decoder)
    assert one.n_chunks == [48, 47]
    # by hand, tolerance pr.max_samples = 16000: (16000 - 1 + 16000) // 1024 = 31; 40000 // 1024 = 39, (46400 - 1 + 16000) // 1024 = 60 -> T - 1 = 47
    assert pr.max_samples == 16000
    events = [[(1, 7, 31), (4, 39, 47)], []]
    want = sweep_ref.sweep(one.index.cpu().numpy(), one.score.cpu().numpy(), one.n_chunks, 0, sens, levels, 1024, events)
    got = _counts(res)
    print("fires per point", want[..., 0].sum(axis=0).tolist())
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(_counts(one.sweep(sens, levels, 1024))[..., 0], want[..., 0])      # ScanResult.sweep, no labels
    miss, fa = res.det()
    assert miss.shape == (4, 3) and fa.shape == (4, 3)
    np.testing.assert_array_equal(fa, want[..., 2].sum(axis=0) * 3600.0 / sum(res.seconds))
