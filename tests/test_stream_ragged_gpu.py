"""Ragged streaming on the GPU (kws_amd.stream.StreamServer over kws_stream_ragged_append / _push_rows / _postprocess, include/kws.h)
against the per-stream loop of oracle/stream_oracle.py, with the models, helpers and bounds of
tests/test_stream_gpu.py::test_stream_batch_matches_oracle_loop: features within 3e-4 of StreamState.push, probabilities within 2e-4
of the oracle model on the oracle's features, index / fired / activation equal to stream_oracle.postprocess of the DEVICE's own
probabilities at the slot's own operating point, the float64 score within 1e-12 relative.  Where two device paths must agree
(lockstep pushes against StreamBatch, one stream alone against the same stream among others) the comparison is bit for bit.

Measured on an MI355X: the ragged schedule's features within 4.4e-6 and its probabilities within 6.5e-8 of the oracle loop (the
test prints a "FIGURES |" line); the lockstep pushes bit-identical to StreamBatch at both chunk sizes; torch's synchronisation
debug mode is supported on this ROCm build (it raises on a read-back), so the no-synchronisation test is in."""
import numpy as np
import pytest

import geometry_cases as gc

pytestmark = pytest.mark.gpu

NAMES = ["background", "up", "down", "left", "right"]
C = 5
LENS = (1, 511, 512, 513, 1023, 1024)
ATOL_FEAT, ATOL_PROBS = 3e-4, 2e-4


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


_DEFAULT = []


def default_models():
    """(pr, oracle model, device model) of tests/test_stream_gpu.py::_stream_batch, made once"""
    from classifier.params import pr
    from kws_amd.model import DeviceModel, ModelSpec
    from oracle import model_oracle as mo
    if not _DEFAULT:
        om = mo.Model("simple_cnn", C).init_weights(0)
        dm = DeviceModel(ModelSpec("simple_cnn", C, pr.n_features, pr.n_mfcc))
        dm.set_weights(om.get_weights())
        _DEFAULT.extend((pr, om, dm))
    return tuple(_DEFAULT)


def server(S, chunk=1024, **kw):
    from kws_amd.stream import StreamServer
    pr, om, dm = default_models()
    return StreamServer(pr, dm, S, chunk_size=chunk, class_names=NAMES, **kw)


def pcm_of(rng, n, level=3000.0):
    return np.clip(rng.normal(0, level, n), -32768, 32767).astype(np.int16)


class OracleSlot(object):
    """one Listener of the reference: update_vectors, then the prediction loop on given probabilities"""

    def __init__(self, pr, sensitivity, trigger_level, chunk_size, featurize=None):
        from oracle import featurizer_oracle as fo
        from oracle import stream_oracle as so
        self.so, self.pr = so, pr
        self.state = so.StreamState(pr.n_features, pr.n_mfcc, pr.window_samples, pr.hop_samples, featurize or fo.mfcc_spec)
        self.trig = so.TriggerState()
        self.dec = so.decoder_table(pr.threshold_config)
        self.op = (sensitivity, trigger_level, chunk_size)

    def push(self, pcm):
        return self.state.push(pcm.astype(np.float64) / 32768.0)                     # buffer_to_audio, data_utils.py:19-21

    def decide(self, probs):
        return self.so.postprocess(probs, 0, self.dec, self.pr.threshold_center, self.trig, *self.op)


def check_decisions(srv, oracle, slots, index, score, fired):
    """index / score / fired of a push, compact and per slot, against the oracle loop on the device's own probabilities"""
    probs = srv.probs.cpu().numpy()
    index, score, fired = index.cpu().numpy(), score.cpu().numpy(), fired.cpu().numpy()
    state, s_index, s_score, s_fired = (t.cpu().numpy() for t in (srv.state, srv.index, srv.score, srv.fired))
    assert probs.shape[0] == index.shape[0] == score.shape[0] == fired.shape[0] == len(slots)
    for a, s in enumerate(slots):
        wi, ws, wf = oracle[s].decide(probs[a])
        assert (int(index[a]), int(fired[a])) == (wi, int(wf)), (a, s)
        assert abs(float(score[a]) - ws) <= 1e-12 * max(1.0, abs(ws))
        assert int(state[s, 0]) == oracle[s].trig.activation and int(state[s, 1]) == oracle[s].trig.record_index
        assert (int(s_index[s]), float(s_score[s]), int(s_fired[s])) == (int(index[a]), float(score[a]), int(fired[a]))
    return probs


def snapshot(srv):
    return [t.cpu().numpy().copy() for t in (srv.win, srv.mfccs, srv.state)]


def in_form(torch, form, chunks):
    """the four input forms of push for one list of 1-D int16 arrays -> (chunks, lengths)"""
    if form == 0:
        return [c.tobytes() for c in chunks], None
    if form == 1:
        return chunks, None
    lens = [c.size for c in chunks]
    padded = np.zeros((len(chunks), max(lens) + (form == 3)), np.int16)              # form 3: an odd row stride on the device
    for a, c in enumerate(chunks):
        padded[a, :c.size] = c
    return (padded if form == 2 else torch.from_numpy(padded).cuda()), lens


def test_ragged_schedule_matches_the_per_stream_oracle(torch):
    S, T = 5, 40
    pr, om, dm = default_models()
    ops = [(0.5, 3), (0.3, 2), (0.7, 4), (0.5, 1), (0.6, 3)]
    srv = server(S)
    assert [srv.open(*op) for op in ops] == list(range(S))
    assert srv.sensitivity.cpu().tolist() == [op[0] for op in ops] and srv.trigger_level.cpu().tolist() == [op[1] for op in ops]
    oracle = [OracleSlot(pr, op[0], op[1], 1024) for op in ops]
    rng = np.random.default_rng(11)
    pushed = [0] * S
    e_feat = e_prob = 0.0
    for t in range(T):
        slots = [s for s in range(S - 1) if rng.random() < 0.7] or [int(rng.integers(S - 1))]      # slot 4 is never pushed
        rng.shuffle(slots)
        chunks = [pcm_of(rng, int(rng.choice(LENS))) for _ in slots]
        for a, s in enumerate(slots):
            if s == 1 and pushed[s] < 6:
                chunks[a][:] = 0                                                  # silent for its first 6 chunks: the log floor
            pushed[s] += 1
        before = snapshot(srv)
        data, lens = in_form(torch, t % 4, chunks)
        index, score, fired = srv.push(slots, data, lens)
        after = snapshot(srv)
        for s in set(range(S)) - set(slots):
            for b, a in zip(before, after):
                np.testing.assert_array_equal(b[s], a[s])                         # untouched, bit for bit
        want = [oracle[s].push(c) for s, c in zip(slots, chunks)]
        for a, s in enumerate(slots):
            err = float(np.abs(after[1][s] - want[a]).max())
            e_feat = max(e_feat, err)
            assert err <= ATOL_FEAT, (t, s, err)
            assert int(srv.plan.carry[s]) == len(oracle[s].state.window_audio)
            np.testing.assert_array_equal(after[0][s, :srv.plan.carry[s]], np.round(oracle[s].state.window_audio * 32768.0).astype(np.int16))
        probs = check_decisions(srv, oracle, slots, index, score, fired)
        err = float(np.abs(probs - om.predict(np.stack(want)[..., None])).max())
        e_prob = max(e_prob, err)
        assert err <= ATOL_PROBS, (t, err)
    print("FIGURES | ragged schedule | max feature error %.3g, max probability error %.3g" % (e_feat, e_prob))
    assert pushed[4] == 0 and min(pushed[:4]) > 6
    assert not after[1][4].any() and after[2][4].tolist() == [0, -1]
    assert all(o.state.mfccs[-1].any() and len(o.state.window_audio) > 0 for o in oracle[:4])   # every pushed slot has rows and a carry


@pytest.mark.parametrize("chunk", [1024, 800])
def test_lockstep_pushes_equal_stream_batch_bit_for_bit(torch, chunk):
    from kws_amd.stream import StreamBatch
    S, T = 5, 40
    pr, om, dm = default_models()
    sb = StreamBatch(pr, dm, S, chunk_size=chunk, class_names=NAMES, sensitivity=0.5, trigger_level=3)
    srv = server(S, chunk, sensitivity=0.5, trigger_level=3)
    slots = [srv.open() for _ in range(S)]
    rng = np.random.default_rng(chunk)
    pcm = np.clip(rng.normal(0, 3000, (T, S, chunk)), -32768, 32767).astype(np.int16)
    pcm[:6, 1] = 0
    for t in range(T):
        want = [v.cpu().numpy().copy() for v in sb.push(pcm[t])]
        got = [v.cpu().numpy() for v in srv.push(slots, pcm[t])]
        for name, w, g in (("mfccs", sb.mfccs, srv.mfccs), ("probs", sb.probs, srv.probs), ("state", sb.state, srv.state)):
            np.testing.assert_array_equal(w.cpu().numpy().view(np.uint32), g.cpu().numpy().view(np.uint32), err_msg="%s at push %d" % (name, t))
        np.testing.assert_array_equal(want[0], got[0])
        np.testing.assert_array_equal(want[1].view(np.uint64), got[1].view(np.uint64))
        np.testing.assert_array_equal(want[2], got[2])
        assert int(srv.plan.carry[0]) == sb.n_win


def test_one_stream_alone_and_among_others_is_bit_identical(torch):
    S, T, me = 300, 12, 131
    pr, om, dm = default_models()
    rng = np.random.default_rng(3)
    mine = [pcm_of(rng, int(rng.choice(LENS[1:]))) for _ in range(T)]
    alone, crowd = server(S), server(S)
    for srv in (alone, crowd):
        assert [srv.open() for _ in range(S)] == list(range(S))
    oa, oc = {me: OracleSlot(pr, 0.5, 3, 1024)}, {me: OracleSlot(pr, 0.5, 3, 1024)}
    others = [s for s in range(S) if s != me]
    for t in range(T):
        r = alone.push([me], [mine[t]])
        check_decisions(alone, oa, [me], *r)
        want = alone.mfccs[me].cpu().numpy().copy()
        A = (64, 65, 256, 257, 300)[t % 5]                                          # wave and block edges of the three kernels
        slots = [int(s) for s in rng.permutation(others)[:A - 1]]
        at = (0, A - 1, A // 2)[t % 3]
        slots.insert(at, me)
        chunks = [pcm_of(rng, int(rng.integers(1, 1025))) for _ in slots]
        chunks[at] = mine[t]
        r = crowd.push(slots, chunks)
        np.testing.assert_array_equal(crowd.mfccs[me].cpu().numpy().view(np.uint32), want.view(np.uint32), err_msg="push %d among %d" % (t, A))
        probs = crowd.probs.cpu().numpy()
        wi, ws, wf = oc[me].decide(probs[at])
        assert (int(r[0][at]), int(r[2][at])) == (wi, int(wf)) and abs(float(r[1][at]) - ws) <= 1e-12 * max(1.0, abs(ws))
        assert int(crowd.state[me, 0]) == oc[me].trig.activation
    assert want[-8:].any(axis=1).all()                                             # rows did arrive


_MODELS = {}


def geometry_models(g):
    """tests/test_stream_geometry_gpu.py::models without the head gain"""
    from kws_amd.model import DeviceModel, ModelSpec
    from oracle import model_oracle as mo
    if g.name not in _MODELS:
        kind = gc.stream_model_kind(g)
        om = mo.Model(kind, C, n_features=g.frames, feature_size=g.n_mfcc).init_weights(0)
        ws = [np.asarray(w, np.float32) for w in om.get_weights()]
        om.set_weights([w.astype(np.float64) for w in ws])
        dm = DeviceModel(ModelSpec(kind, C, g.frames, g.n_mfcc))
        dm.set_weights(ws)
        _MODELS[g.name] = (om, dm)
    return _MODELS[g.name]


@pytest.mark.parametrize("name", ["rad2-48", "rad2-31"])          # window 400 is no multiple of hop 160; hop 512 > window 256: the carry empties
def test_other_geometries(torch, name):
    from kws_amd.stream import StreamServer
    from oracle import featurizer_oracle as fo
    g = gc.ROW[name]
    pr, kw = gc.params(g), gc.oracle_kw(g)
    om, dm = geometry_models(g)
    S, T, chunk = 4, 30, 800
    srv = StreamServer(pr, dm, S, chunk_size=chunk, class_names=NAMES)
    ops = [(0.5, 3), (0.4, 2), (0.6, 1), (0.5, 4)]
    oracle = [OracleSlot(pr, op[0], op[1], chunk, featurize=lambda a: fo.mfcc_spec(a, **kw)) for op in ops]
    assert [srv.open(*op) for op in ops] == list(range(S))
    rng = np.random.default_rng(g.frames)
    emptied = 0
    for t in range(T):
        slots = [s for s in range(S) if rng.random() < 0.75] or [0]
        rng.shuffle(slots)
        chunks = [pcm_of(rng, int(rng.integers(1, chunk + 1)), float(rng.choice([150.0, 1500.0, 9000.0]))) for _ in slots]
        index, score, fired = srv.push(slots, chunks)
        feats = srv.mfccs.cpu().numpy()
        for s, c in zip(slots, chunks):
            want = oracle[s].push(c)
            assert float(np.abs(feats[s] - want).max()) <= ATOL_FEAT, (t, s)
            assert int(srv.plan.carry[s]) == len(oracle[s].state.window_audio)
            emptied += int(srv.plan.carry[s] == 0)
        check_decisions(srv, oracle, slots, index, score, fired)
    assert (emptied > 0) == (pr.hop_samples > pr.window_samples)
    assert all(np.abs(o.state.mfccs[-1]).max() > 0 for o in oracle)


def test_close_and_reopen_restarts_the_slot_and_leaves_its_neighbours(torch):
    pr, om, dm = default_models()
    S = 3
    srv, fresh = server(S), server(1)
    ops = [(0.5, 3), (0.4, 2), (0.6, 1)]
    assert [srv.open(*op) for op in ops] == [0, 1, 2]
    oracle = {s: OracleSlot(pr, ops[s][0], ops[s][1], 1024) for s in range(S)}
    rng = np.random.default_rng(5)

    def step(slots, chunks=None):
        chunks = chunks or [pcm_of(rng, int(rng.choice(LENS[1:]))) for _ in slots]
        before = snapshot(srv)
        r = srv.push(slots, chunks)
        after = snapshot(srv)
        for s in set(range(S)) - set(slots):
            for b, a in zip(before, after):
                np.testing.assert_array_equal(b[s], a[s])
        for s, c in zip(slots, chunks):
            assert float(np.abs(after[1][s] - oracle[s].push(c)).max()) <= ATOL_FEAT
        check_decisions(srv, oracle, slots, *r)
        return chunks

    # two pushes to a just-opened slot before anything else: the restart rides in the first one only
    step([1])
    step([1])
    assert np.abs(srv.mfccs[1].cpu().numpy()).max() > 0 or srv.plan.carry[1] > 0
    for _ in range(8):
        step([2, 0, 1])
    assert srv.mfccs[1].cpu().numpy()[-8:].any(axis=1).all()                       # slot 1's window holds rows
    srv.close(1)
    with pytest.raises(ValueError, match="closed"):
        srv.push([1], [pcm_of(rng, 10)])
    step([0, 2])
    assert srv.open(0.45, 2) == 1                                                  # the freed slot, with a new operating point
    oracle[1] = OracleSlot(pr, 0.45, 2, 1024)
    assert fresh.open(0.45, 2) == 0
    of = {0: OracleSlot(pr, 0.45, 2, 1024)}
    for i in range(6):
        slots = [[1], [1, 0], [2, 1, 0]][min(i, 2)]                                # alone twice, then with its neighbours
        chunks = step(slots)
        mine = chunks[slots.index(1)]
        r = fresh.push([0], [mine])
        check_decisions(fresh, of, [0], *r)
        np.testing.assert_array_equal(srv.mfccs[1].cpu().numpy().view(np.uint32), fresh.mfccs[0].cpu().numpy().view(np.uint32))
        np.testing.assert_array_equal(srv.state[1].cpu().numpy(), fresh.state[0].cpu().numpy())
        if i == 0:
            assert not srv.mfccs[1].cpu().numpy()[:-2].any()                       # zero-padded again: the old rows are gone
    with pytest.raises(RuntimeError, match="full"):
        srv.open()


def test_quantized_forward_drives_the_server(torch):
    from classifier.model import get_model
    from classifier.params import pr
    from kws_amd.init import init_weights
    from kws_amd.stream import StreamServer
    rng = np.random.default_rng(9)
    m = get_model("simple_cnn", C)
    m.set_weights(init_weights(m.spec, seed=4))
    q = m.quantize((0.1 * rng.standard_normal((64, 16000))).astype(np.float32)).quantized
    S = 6
    srv = StreamServer(pr, m._device(), S, class_names=NAMES, quantized=q)
    ops = [(0.5, 3), (0.3, 1), (0.5, 2), (0.7, 3), (0.2, 1), (0.5, 3)]
    assert [srv.open(*op) for op in ops] == list(range(S))
    oracle = [OracleSlot(pr, op[0], op[1], 1024) for op in ops]
    for t in range(12):
        slots = [int(s) for s in rng.permutation(S)[:int(rng.integers(1, S + 1))]]
        r = srv.push(slots, [pcm_of(rng, int(rng.choice(LENS))) for _ in slots])
        windows = srv.mfccs[torch.tensor(slots, device="cuda")].contiguous()
        want, _ = q.forward(windows)
        assert torch.equal(srv.probs, want)                                        # the int8 forward on the compact windows, bit for bit
        check_decisions(srv, oracle, slots, *r)
    fp32, _ = m._device().forward(windows, want_probs=True, want_argmax=False)
    assert not torch.equal(fp32, want)                                             # and not the float model's


def test_edge_batches(torch):
    pr, om, dm = default_models()
    S = 4
    srv = server(S)
    slots = [srv.open() for _ in range(S)]
    oracle = [OracleSlot(pr, 0.5, 3, 1024) for _ in range(S)]
    rng = np.random.default_rng(2)
    before, n0 = snapshot(srv), (srv.launches, srv.featurizer_launches)
    r = srv.push([], [])
    assert [tuple(v.shape) for v in r] == [(0,)] * 3 and r[0].is_cuda and tuple(srv.probs.shape) == (0, C)
    assert (srv.launches, srv.featurizer_launches) == n0                           # nothing enqueued
    for b, a in zip(before, snapshot(srv)):
        np.testing.assert_array_equal(b, a)
    # a push in which no slot completes a row: no featurizer launch, but a prediction per chunk on the unchanged windows
    for n in (300, 300, 300):
        chunks = [pcm_of(rng, n) for _ in slots]
        r = srv.push(slots, chunks)                                                # A == S
        for s, c in zip(slots, chunks):
            oracle[s].push(c)
        check_decisions(srv, oracle, slots, *r)
    assert srv.featurizer_launches == 0 and srv.launches == 12 and not srv.mfccs.cpu().numpy().any()
    chunks = [pcm_of(rng, 1024) for _ in slots]
    r = srv.push(slots, chunks)
    for s, c in zip(slots, chunks):
        assert float(np.abs(srv.mfccs[s].cpu().numpy() - oracle[s].push(c)).max()) <= ATOL_FEAT
    check_decisions(srv, oracle, slots, *r)
    assert srv.featurizer_launches == 1 and srv.mfccs.cpu().numpy()[:, -1].any()
    # counters move on chunks that bring no row: force a confident streak by hand and watch the activation climb
    hot = torch.tensor([[0.01, 0.97, 0.01, 0.005, 0.005]] * S, dtype=torch.float32, device="cuda")
    srv.model = type("Hot", (), {"forward": staticmethod(lambda feat, want_probs=True, want_argmax=False: (hot[:feat.shape[0]].clone(), None)),
                                 "spec": dm.spec})()
    feats = srv.mfccs.cpu().numpy().copy()
    acts = []
    for _ in range(4):
        srv.push(slots, [pcm_of(rng, 1) for _ in slots])                            # one sample each: never a row
        acts.append(srv.state[:, 0].cpu().tolist())
    np.testing.assert_array_equal(srv.mfccs.cpu().numpy(), feats)
    assert acts[1] == [a + 1 for a in acts[0]] and acts[2] == [a + 1 for a in acts[1]] and srv.featurizer_launches == 1


def test_push_does_not_synchronise(torch):
    S = 8
    srv = server(S)
    slots = [srv.open() for _ in range(S)]
    rng = np.random.default_rng(4)
    host = [pcm_of(rng, 1024) for _ in slots]
    dev = torch.from_numpy(np.stack(host)).cuda()
    srv.push(slots, host)                                                          # warm-up: workspaces, pinned blocks, code objects
    srv.push(slots, dev, [1024] * S)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        srv.push(slots[::-1], host)
        srv.push(slots[:3], dev[:3], [1000, 7, 512])
        srv.push([], [])
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    with pytest.raises(RuntimeError):                                              # the mode does catch a read-back on this build
        torch.cuda.set_sync_debug_mode("error")
        try:
            srv.index.cpu()
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    assert srv.fired.cpu().numpy().shape == (S,)
