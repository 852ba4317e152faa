"""Streams and recordings at their own sample rates on the GPU (kws_amd.stream.StreamServer.open(sample_rate=...), scan(sample_rates=...),
listen.Listener(resample=True)).  The converter itself is pinned to its definition by tests/test_rate_gpu.py; here a server whose slots
arrive at 8 / 44.1 / 48 kHz is compared, bit for bit, with a second server at the detector's rate that is fed exactly the samples
tests/rate_ref.py's counts say each push emits, cut from kws_amd.rate.convert of the whole stream."""
import wave

import numpy as np
import pytest

import rate_ref as rr
from test_stream_ragged_gpu import C, NAMES, default_models, pcm_of, server, snapshot

pytestmark = pytest.mark.gpu

SR = 16000


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _bits(t):
    a = t.cpu().numpy()
    return a.view({4: np.uint32, 8: np.uint64, 2: np.uint16}[a.dtype.itemsize])


class Feed(object):
    """one stream at `rate`: its chunks, and for every chunk the samples at SR it makes the converter emit"""

    def __init__(self, rate, lens, rng):
        from kws_amd.rate import convert
        self.rate, self.lens = rate, lens
        self.pcm = pcm_of(rng, sum(lens))
        self.ref = None if rate == SR else rr.Bank(rate, SR)
        self.whole = self.pcm if self.ref is None else convert([self.pcm], rate, SR)[0][0].cpu().numpy()
        self.N = self.k = 0

    def next(self):
        n = self.lens[self.k]
        chunk = self.pcm[self.N:self.N + n]
        if self.ref is None:
            out = chunk
        else:
            lo, hi = (rr.emitted(v, self.ref.p, self.ref.q, self.ref.K) for v in (self.N, self.N + n))
            out = self.whole[lo:hi]
        self.N, self.k = self.N + n, self.k + 1
        return chunk, out


def test_mixed_rate_server_equals_a_native_server_fed_the_converted_samples(torch):
    S, T = 6, 30
    rates = [8000, None, 44100, 48000, 44100, 8000]                   # slot 1 is native; slot 4 is reopened at 11025 Hz; slot 5 is never pushed
    a, b = server(S), server(S)
    assert [a.open(sample_rate=r) for r in rates] == list(range(S)) == [b.open() for _ in rates]
    rng = np.random.default_rng(21)
    # the schedule first, so that every stream can be converted whole: (push, slot) -> chunk length
    sched = []
    for t in range(T):
        act = [s for s in range(S - 1) if rng.random() < 0.7] or [int(rng.integers(S - 1))]
        rng.shuffle(act)
        sched.append(act)
    reopen = 15
    epoch = lambda t, s: int(s == 4 and t >= reopen)                   # noqa: E731
    rate_of = lambda t, s: 11025 if epoch(t, s) else (rates[s] or SR)  # noqa: E731
    lens = {}
    for t, act in enumerate(sched):
        for s in act:
            limit = a.plan.chunk_size * rate_of(t, s) // SR
            tiny = rng.random() < 0.3                                  # chunks of one sample: at 44.1 and 48 kHz two in three emit nothing
            lens.setdefault((s, epoch(t, s)), []).append(1 if tiny else int(rng.integers(limit // 2, limit + 1)))
    feeds = {key: Feed(rate_of(reopen * key[1], key[0]), v, rng) for key, v in lens.items()}
    silent = 0
    for t, act in enumerate(sched):
        if t == reopen:
            for srv, kw in ((a, {"sample_rate": 11025}), (b, {})):
                srv.close(4)
                assert srv.open(**kw) == 4
        pairs = [feeds[(s, epoch(t, s))].next() for s in act]
        before_a, prev = snapshot(a), [a.index.cpu().numpy().copy(), a.score.cpu().numpy().copy()]
        index, score, fired = (v.cpu().numpy() for v in a.push(act, [p[0] for p in pairs]))
        kept = [i for i, p in enumerate(pairs) if len(p[1])]
        silent += len(act) - len(kept)
        assert a.probs.shape[0] == len(kept)
        if kept:
            want = [v.cpu().numpy() for v in b.push([act[i] for i in kept], [pairs[i][1] for i in kept])]
            np.testing.assert_array_equal(_bits(a.probs), _bits(b.probs), err_msg="probs at push %d" % t)
            for i, k in enumerate(kept):
                assert (index[k], fired[k]) == (want[0][i], want[2][i]) and score[k].view(np.uint64) == want[1][i].view(np.uint64), (t, k)
        for i, s in enumerate(act):
            if i not in kept:                                          # no sample, no prediction: the slot's previous result, fired 0
                assert (index[i], fired[i]) == (prev[0][s], 0) and score[i].view(np.uint64) == prev[1][s].view(np.uint64), (t, i, s)
        for name in ("win", "mfccs", "state", "index", "score", "fired"):
            np.testing.assert_array_equal(_bits(getattr(a, name)), _bits(getattr(b, name)), err_msg="%s after push %d" % (name, t))
        np.testing.assert_array_equal(a.plan.carry, b.plan.carry)
        after_a = snapshot(a)
        for s in set(range(S)) - set(act):
            for x, y in zip(before_a, after_a):
                np.testing.assert_array_equal(x[s], y[s])              # untouched, bit for bit
    assert silent >= 3 and all(f.k == len(f.lens) for f in feeds.values())
    assert not a.mfccs[5].cpu().numpy().any() and a.state[5].cpu().tolist() == [0, -1]
    assert all(a.mfccs[s].cpu().numpy()[-1].any() for s in range(5))   # every pushed slot has rows


def test_entries_that_emit_nothing_keep_the_previous_result(torch):
    srv = server(3)
    s48, s16, s44 = srv.open(sample_rate=48000), srv.open(), srv.open(sample_rate=44100)
    rng = np.random.default_rng(2)
    srv.push([s48, s16, s44], [pcm_of(rng, 3072), pcm_of(rng, 1024), pcm_of(rng, 2822)])
    srv.push([s48, s16, s44], [pcm_of(rng, 3072), pcm_of(rng, 1024), pcm_of(rng, 2822)])
    r44, r48 = rr.Bank(44100, SR), rr.Bank(48000, SR)
    emits = lambda ref, n: rr.emitted(n + 1, ref.p, ref.q, ref.K) - rr.emitted(n, ref.p, ref.q, ref.K)     # noqa: E731
    assert (emits(r44, 2 * 2822), emits(r48, 2 * 3072), emits(r48, 2 * 3072 + 1)) == (0, 1, 0)
    prev = [srv.index.cpu().numpy().copy(), srv.score.cpu().numpy().copy()]
    n0 = srv.launches
    index, score, fired = (v.cpu().numpy() for v in srv.push([s44, s48], [pcm_of(rng, 1), pcm_of(rng, 1)]))   # one sample each: 0 and 1 outputs
    assert srv.launches == n0 + 5 and tuple(srv.probs.shape) == (1, C)
    assert (index[0], fired[0], score[0]) == (prev[0][s44], 0, prev[1][s44])
    assert (index[1], fired[1], score[1]) == (int(srv.index[s48]), int(srv.fired[s48]), float(srv.score[s48]))
    # a push none of whose entries emits: the converter alone runs (the history rows move on), nothing else changes
    prev, state, n0 = [srv.index.cpu().numpy().copy(), srv.score.cpu().numpy().copy()], snapshot(srv), srv.launches
    index, score, fired = (v.cpu().numpy() for v in srv.push([s48], [pcm_of(rng, 1)]))
    assert srv.launches == n0 + 1 and tuple(srv.probs.shape) == (0, C)
    assert (index[0], fired[0], score[0]) == (prev[0][s48], 0, prev[1][s48])
    for x, y in zip(state, snapshot(srv)):
        np.testing.assert_array_equal(x, y)
    # the sample was not lost: the next chunk's outputs continue the one-shot conversion of the whole stream
    assert int(srv.plan.received[s48]) == 2 * 3072 + 2


def test_a_native_only_server_is_todays_server(torch):
    """the launch counts tests/test_stream_ragged_gpu.py::test_edge_batches pins, and the same bits as a server opened without sample_rate"""
    pr, om, dm = default_models()
    S = 4
    new, old = server(S), server(S)
    slots = [new.open(sample_rate=pr.sample_rate) for _ in range(S)]
    assert slots == [old.open() for _ in range(S)] and new._hist is None
    rng = np.random.default_rng(2)
    for n, want in ((300, (4, 0)), (300, (8, 0)), (300, (12, 0)), (1024, (17, 1)), (1, (21, 1))):
        chunks = [pcm_of(rng, n) for _ in slots]
        r_new, r_old = new.push(slots, chunks), old.push(slots, chunks)
        assert (new.launches, new.featurizer_launches) == want == (old.launches, old.featurizer_launches)
        for x, y in zip(r_new, r_old):
            np.testing.assert_array_equal(_bits(x), _bits(y))
        for name in ("win", "mfccs", "state", "probs"):
            np.testing.assert_array_equal(_bits(getattr(new, name)), _bits(getattr(old, name)))
    # with one slot converted, a push that names only native slots still runs today's path and count
    mixed = server(S)
    ids = [mixed.open(), mixed.open(sample_rate=8000), mixed.open()]
    mixed.push([ids[0], ids[2]], [pcm_of(rng, 1024), pcm_of(rng, 700)])
    assert (mixed.launches, mixed.featurizer_launches) == (5, 1)
    mixed.push(ids, [pcm_of(rng, 1024), pcm_of(rng, 512), pcm_of(rng, 700)])
    assert (mixed.launches, mixed.featurizer_launches) == (11, 2)      # the converter's launch is the one more


def test_push_with_converted_slots_does_not_synchronise(torch):
    S = 8
    srv = server(S)
    rates = [8000, None, 44100, 48000, 8000, None, 44100, 48000]
    slots = [srv.open(sample_rate=r) for r in rates]
    limit = [int(srv.plan.max_chunk[s]) for s in slots]
    rng = np.random.default_rng(4)
    host = [pcm_of(rng, n) for n in limit]
    dev = torch.zeros((S, max(limit)), dtype=torch.int16, device="cuda")
    srv.push(slots, host)                                              # warm-up: banks, workspaces, pinned blocks, code objects
    srv.push(slots, dev, limit)
    srv.push(slots[2:4], [pcm_of(rng, 1), pcm_of(rng, 1)])
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        srv.push(slots[::-1], host[::-1])
        srv.push(slots[:3], dev[:3], [500, 7, 2000])
        srv.push(slots[2:4], [pcm_of(rng, 1), pcm_of(rng, 2)])         # entries that emit nothing: the gathered result
        srv.push(slots[3:4], [pcm_of(rng, 1)])
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert srv.fired.cpu().numpy().shape == (S,)


def _recordings(rng):
    rates = [8000, 16000, 44100, 48000]
    secs = [0.4, 1.5, 0.9, 1.2]
    return [pcm_of(rng, int(s * r) + 3) for s, r in zip(secs, rates)], rates


def test_scan_with_sample_rates_equals_scan_of_the_converted_recordings(torch):
    from kws_amd.rate import convert
    from kws_amd.stream import scan
    pr, om, dm = default_models()
    pcm, rates = _recordings(np.random.default_rng(6))
    got = scan(pr, dm, pcm, class_names=NAMES, sensitivity=0.3, trigger_level=1, return_probs=True, keep_audio=True, sample_rates=rates)
    out, lens = convert(pcm, rates, pr.sample_rate)
    assert lens == [-(-len(x) * pr.sample_rate // r) for x, r in zip(pcm, rates)] == got.lengths
    host = out.cpu().numpy()
    np.testing.assert_array_equal(host[1, :lens[1]], pcm[1])            # the recording already at the detector's rate, bit for bit
    want = scan(pr, dm, [host[r, :n] for r, n in enumerate(lens)], class_names=NAMES, sensitivity=0.3, trigger_level=1, return_probs=True)
    assert got.n_chunks == want.n_chunks == [-(-n // 1024) for n in lens]
    for name in ("index", "score", "fired", "state", "probs"):
        np.testing.assert_array_equal(_bits(getattr(got, name)), _bits(getattr(want, name)), err_msg=name)
    same = scan(pr, dm, [pcm[1]], class_names=NAMES, sample_rates=16000)
    plain = scan(pr, dm, [pcm[1]], class_names=NAMES)
    np.testing.assert_array_equal(_bits(same.score), _bits(plain.score))


def _write(path, pcm, rate):
    with wave.open(str(path), "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(rate)
        wf.writeframes(pcm.tobytes())


def test_listener_resample_flag(torch, tmp_path):
    from classifier.model import get_model
    from kws_amd.init import init_weights
    from kws_amd.rate import convert
    from listen import Listener, parse_args
    classes = tmp_path / "classes.txt"
    classes.write_text("\n".join(NAMES) + "\n")
    rng = np.random.default_rng(8)
    pcm = pcm_of(rng, 44100 + 77, 4000.0)
    out, lens = convert([pcm], 44100, SR)
    _write(tmp_path / "a44.wav", pcm, 44100)
    _write(tmp_path / "a16.wav", out[0, :lens[0]].cpu().numpy(), SR)
    m = get_model("simple_cnn", 5)
    m.set_weights(init_weights(m.spec, seed=4))
    lis = Listener(model=m, classes_path=str(classes), chunk_size=1024, sensitivity=0.05, trigger_level=1, resample=True)
    got = lis.scan_wav(str(tmp_path / "a44.wav"))
    assert lis.last_scan[1] == lens
    want = lis.scan_wav(str(tmp_path / "a16.wav"))
    assert got == want and len(got) == -(-lens[0] // 1024)
    assert Listener(model=m, classes_path=str(classes), chunk_size=1024, sensitivity=0.05, trigger_level=1, resample=True,
                    input_wav=str(tmp_path / "a44.wav")).run_wav(quiet=True) == \
        Listener(model=m, classes_path=str(classes), chunk_size=1024, sensitivity=0.05, trigger_level=1,
                 input_wav=str(tmp_path / "a16.wav")).run_wav(quiet=True)
    strict = Listener(model=m, classes_path=str(classes), chunk_size=1024, input_wav=str(tmp_path / "a44.wav"))
    with pytest.raises(AssertionError, match="sample rate mismatch"):
        strict.scan_wav(str(tmp_path / "a44.wav"))
    with pytest.raises(AssertionError, match="sample rate mismatch"):
        strict.run_wav(quiet=True)
    assert parse_args(["--model_path", "m.npz", "--input_wav", "x.wav", "--resample"]).resample is True
    assert parse_args(["--model_path", "m.npz", "--input_wav", "x.wav"]).resample is False
