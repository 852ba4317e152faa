"""Stacked simple_gru / simple_lstm (kws_model_create_stacked, num_layers 2 .. 4) against the float64 reference of tests/rnn_stack_ref.py
on the case table of tests/rnn_stack_cases.py: inference probabilities and arg-max, train-step probabilities, loss, correct count and
every gradient, each train step from a gradient buffer full of NaN; the LDS edge where inference runs and training is refused; a batch
that shrinks on one workspace; the one-layer identity of the two creation calls; and the Python surface on a two-layer GRU.  The
tolerances are tests/rnn_cases.py's (tests/test_rnn_stack_host.py shows the float32 reference a tenth inside them)."""
import numpy as np
import pytest

import rnn_cases as rc
import rnn_stack_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def device_model(case, ref):
    from kws_amd.model import DeviceModel, ModelSpec
    dm = DeviceModel(ModelSpec(case.kind, case.C, case.T, case.F, num_layers=case.L))
    dm.set_weights(ref.weights)
    return dm


def train_step(torch, dm, case):
    """one train step from a gradient buffer full of NaN -> (probabilities, loss, correct predictions, gradients)"""
    (x, y, cw), _ = sc.reference(case)
    dm.grads.fill_(float("nan"))
    dm.stats.fill_(-1.0)
    probs = dm.train_fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y.astype(np.int32)).cuda(),
                             None if cw is None else torch.from_numpy(cw.astype(np.float32)).cuda(),
                             dropout_seed=case.dropout_seed, want_probs=True)
    stats = dm.stats.cpu().numpy()
    assert bool(torch.isfinite(dm.grads).all()), "the step left part of the gradient buffer uncleared"
    return probs.cpu().numpy(), stats[0] / case.B, stats[1], dm.get_grads()


def infer_and_train(torch, case):
    (x, _, _), ref = sc.reference(case)
    dm = device_model(case, ref)
    p, am = dm.forward(torch.from_numpy(x).cuda())
    infer_probs = p.cpu().numpy()
    np.testing.assert_array_equal(am.cpu().numpy(), ref.infer_probs.argmax(-1))
    fig, bad = rc.compare(ref, infer_probs, *train_step(torch, dm, case))
    print(case.label, " ".join("%s=%.2e" % kv for kv in fig.items()))
    assert not bad, bad
    return dm, ref


@pytest.mark.parametrize("case", sc.CASES, ids=[c.label for c in sc.CASES])
def test_inference_and_train_step_match_the_reference(torch, case):
    dm, ref = infer_and_train(torch, case)
    if case.T == 1:
        # h_prev is the zero initial state in every layer: every recurrent kernel's gradient is exactly zero, and whatever the lower
        # layers' other tensors received came through dseq alone
        grads = dict(zip(ref.names, dm.get_grads()))
        for name, g in grads.items():
            if name.endswith("/recurrent_kernel"):
                assert not g.any(), name
            elif "_unit_0/" in name:
                assert g.any(), name


@pytest.mark.parametrize("kind", rc.KINDS)
def test_smaller_batch_after_a_larger_one_on_the_same_model(torch, kind):
    """B = 33, then B = 1 on the same DeviceModel and workspace: no sequence, saved value or dseq row of the first step reaches the second"""
    first, second = sc.shrink_cases(kind)
    dm, _ = infer_and_train(torch, first)
    ws = dm._ws.data_ptr()
    _, ref = sc.reference(second)
    fig, bad = rc.compare(ref, None, *train_step(torch, dm, second))
    print(second.label, " ".join("%s=%.2e" % kv for kv in fig.items()))
    assert dm._ws.data_ptr() == ws
    assert not bad, bad


@pytest.mark.parametrize("kind", rc.KINDS)
def test_training_refusal_at_the_upper_layers_lds_edge_touches_nothing(torch, kind):
    """T = 46: the 48-wide layers' forward tile fits in LDS (161 664 B) and their backward tile does not (165 504 B); layer 0 alone (46 x 20)
    would train.  Inference matches; the train step is refused before layer 0's forward kernel (which clears the gradients), its events
    and its overlap callback"""
    from kws_amd import KwsError
    case = sc.refused_train_case(kind)
    (x, y, _), ref = sc.reference(case)
    dm = device_model(case, ref)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y.astype(np.int32)).cuda()
    p, am = dm.forward(xt)
    err = float(np.abs(p.cpu().numpy() - ref.infer_probs).max())
    print(case.label, "infer probs=%.2e" % err)
    assert err <= rc.PROB_ATOL
    np.testing.assert_array_equal(am.cpu().numpy(), ref.infer_probs.argmax(-1))
    dm.grads.fill_(7.0)
    dm.stats.fill_(-1.0)
    calls = []
    with pytest.raises(KwsError, match=r"%s backward tile of 46 x 48 \(layer 1 of num_layers = 2\)" % ("GRU" if kind == "simple_gru" else "LSTM")) as e:
        dm.train_fwd_bwd(xt, yt, dropout_seed=case.dropout_seed, want_probs=True, overlap_event=torch.cuda.Event(),
                         overlap_callback=lambda: calls.append(1))
    assert e.value.code == rc.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert calls == []
    assert bool((dm.grads == 7.0).all()), "the refused step wrote %d gradient entries" % int((dm.grads != 7.0).sum())
    assert dm.stats.cpu().tolist() == [-1.0, -1.0]


@pytest.mark.parametrize("kind", rc.KINDS)
def test_one_layer_by_either_creation_call_is_the_same_model(torch, kind):
    """kws_model_create_stacked(.., 1) and kws_model_create(..): bit-identical inference, train-step gradients within the tolerances
    (float atomics make bit equality unobtainable there)"""
    from kws_amd.model import DeviceModel, ModelSpec
    case = sc.one_layer_case(kind)
    (x, y, _), ref = sc.reference(case)
    stacked = ModelSpec(kind, case.C, case.T, case.F, num_layers=1)      # kws_model_create_stacked(.., 1)
    plain = ModelSpec(kind, case.C, case.T, case.F)                      # kws_model_create
    assert plain.num_layers == stacked.num_layers == 1
    assert plain.tensors == stacked.tensors and plain.param_count == stacked.param_count
    assert [plain.workspace_bytes(case.B, t) for t in (False, True)] == [stacked.workspace_bytes(case.B, t) for t in (False, True)]
    out = []
    for spec in (stacked, plain):
        dm = DeviceModel(spec)
        dm.set_weights(ref.weights)
        p, am = dm.forward(torch.from_numpy(x).cuda())
        out.append((p.cpu().numpy(), am.cpu().numpy()) + train_step(torch, dm, case))
    a, b = out
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    fig, bad = rc.compare(ref, a[0], *a[2:])
    assert not bad, bad
    for name, ga, gb, want in zip(ref.names, a[5], b[5], ref.grads):
        assert rc.rel_err(ga, gb) < rc.GRAD_RTOL if want.any() else not (ga.any() or gb.any()), name


@pytest.mark.parametrize("kind", rc.KINDS)
def test_deterministic_mode_names_the_layer_count(torch, kind):
    from kws_amd import KwsError
    from kws_amd.model import DeviceModel, ModelSpec
    dm = DeviceModel(ModelSpec(kind, 6, 9, 20, num_layers=2))
    with pytest.raises(KwsError, match=r"num_layers = 2\)") as e:
        dm.set_deterministic(True)
    assert e.value.code == rc.ERR_UNSUPPORTED


# ---- the Python surface, on a two-layer GRU with 64 clips ---------------------------------------------------------------
N_CLIPS, N_CLASSES = 64, 5


@pytest.fixture(scope="module")
def clips():
    from classifier.params import pr
    rng = np.random.default_rng(77)
    x = (rng.standard_normal((N_CLIPS, pr.n_features, pr.feature_size)) * 2.0).astype(np.float32)
    x[..., 0] -= 10.0
    return x, rng.integers(0, N_CLASSES, N_CLIPS).astype(np.int32)


def test_checkpoint_round_trip_and_layer_count_mismatch(torch, clips, tmp_path):
    from classifier.model import KWSModel, get_model
    x, _ = clips
    m = KWSModel("simple_gru", N_CLASSES, seed=5, num_layers=2)
    want = m.predict(x)
    assert want.shape == (N_CLIPS, N_CLASSES) and np.isfinite(want).all()
    path = str(tmp_path / "gru2.npz")
    m.save_weights(path)
    back = get_model("simple_gru", N_CLASSES, weights_path=path, num_layers=2)
    np.testing.assert_array_equal(back.predict(x), want)
    with pytest.raises(ValueError, match=r"num_layers = 2.*num_layers = 1"):
        get_model("simple_gru", N_CLASSES, weights_path=path)
    with pytest.raises(ValueError, match=r"num_layers = 2.*num_layers = 3"):
        get_model("simple_gru", N_CLASSES, weights_path=path, num_layers=3)


def test_two_fit_steps_equal_two_device_model_steps(torch, clips):
    """fit (its pipelined step) on 64 clips in batches of 32, unshuffled, plain SGD: the weights equal those of two DeviceModel steps with
    the same dropout seeds.  The two runs share every kernel and differ by the order of float atomics alone: each tensor's total update
    is held to GRAD_RTOL of its largest entry."""
    from classifier.loss import SparseCategoricalCrossEntropy
    from classifier.model import KWSModel
    from common.model_utils import get_optimizer
    from kws_amd.model import DeviceModel
    x, y = clips
    lr = 0.05
    m = KWSModel("simple_gru", N_CLASSES, seed=9, num_layers=2)
    w0 = m.get_weights()
    m.compile(get_optimizer("sgd", lr, decay_type=None), SparseCategoricalCrossEntropy(), metrics=["accuracy"])
    hist = m.fit(x, y, batch_size=32, epochs=1, shuffle=False, verbose=0)
    assert np.isfinite(hist.history["loss"]).all() and all(np.isfinite(w).all() for w in m.get_weights())
    dm = DeviceModel(m.spec)
    dm.set_weights(w0)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    for step in (1, 2):
        sl = slice(32 * (step - 1), 32 * step)
        dm.train_fwd_bwd(xt[sl].contiguous(), yt[sl].contiguous(), dropout_seed=(m._dropout_base << 20) + step * 64)
        dm.sgd_step(lr)
    for name, a, b, start in zip(m.weight_names, m.get_weights(), dm.get_weights(), w0):
        assert (b != start).any(), name
        err = rc.rel_err(a - start, b - start)
        print(name, "%.2e" % err)
        assert err < rc.GRAD_RTOL, name


def test_stream_batch_and_scan_equal_predict(torch, clips):
    from classifier.model import KWSModel
    from classifier.params import pr
    from kws_amd.stream import StreamBatch, scan
    names = ["background"] + ["w%d" % i for i in range(1, N_CLASSES)]
    m = KWSModel("simple_gru", N_CLASSES, seed=5, num_layers=2)
    dm = m._device()
    chunk, n_chunks = 1024, 12
    rec = (np.random.default_rng(3).standard_normal(chunk * n_chunks) * 3000).astype(np.int16)
    sb = StreamBatch(pr, dm, 1, chunk_size=chunk, class_names=names)
    loop = []
    for i in range(n_chunks):
        sb.push(rec[None, i * chunk:(i + 1) * chunk])
        window = sb.mfccs.cpu().numpy().copy()
        want = m.predict(window)
        got = sb.probs.cpu().numpy()
        np.testing.assert_array_equal(got, want)              # the same forward kernels on the same window
        loop.append(got[0])
    res = scan(pr, dm, [rec], chunk_size=chunk, class_names=names, return_probs=True)
    np.testing.assert_allclose(res.probs[0].cpu().numpy(), np.stack(loop), rtol=0, atol=rc.PROB_ATOL)


def test_quantize_refuses_a_stacked_model(torch):
    from classifier.model import KWSModel
    from kws_amd import KwsError
    m = KWSModel("simple_gru", N_CLASSES, seed=5, num_layers=2)
    with pytest.raises(KwsError, match="num_layers = 2") as e:
        m.quantize()
    assert e.value.code == rc.ERR_UNSUPPORTED
