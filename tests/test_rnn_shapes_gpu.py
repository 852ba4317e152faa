"""simple_gru and simple_lstm against the float64 oracle at the edges of their kernels (tests/rnn_cases.py has the table and the
comparison; tests/test_rnn_shapes_host.py shows on the oracle alone that the table reaches every branch and that the tolerances leave
float32 arithmetic a margin of 50): every KX template on both sides of its switch, launches below, across and at the end of the
dynamic-LDS opt-in, one- and two-step sequences, batches around the 16-clip tile, both head chains, a gradient buffer that starts
dirty, a dropout seed wider than 32 bits, saturated gates, and the geometries the library refuses."""
import numpy as np
import pytest

import rnn_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def device_model(case, ref):
    from kws_amd.model import DeviceModel, ModelSpec
    dm = DeviceModel(ModelSpec(case.kind, case.C, case.T, case.F))
    dm.set_weights(ref.weights)
    return dm


def train_step(torch, dm, case):
    """one train step from a gradient buffer full of NaN -> (probabilities, loss, correct predictions, gradients)"""
    x, y, cw = rc.inputs(case)
    dm.grads.fill_(float("nan"))                      # a clear that is skipped or too short leaves NaN behind, padding included
    dm.stats.fill_(-1.0)
    probs = dm.train_fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y.astype(np.int32)).cuda(),
                             None if cw is None else torch.from_numpy(cw.astype(np.float32)).cuda(),
                             dropout_seed=case.dropout_seed, want_probs=True)
    stats = dm.stats.cpu().numpy()
    assert bool(torch.isfinite(dm.grads).all()), "the step left part of the gradient buffer uncleared"
    return probs.cpu().numpy(), stats[0] / case.B, stats[1], dm.get_grads()


def infer_and_train(torch, case, saturated=False):
    ref = rc.reference(case, saturated)
    dm = device_model(case, ref)
    p, am = dm.forward(torch.from_numpy(rc.inputs(case)[0]).cuda())
    infer_probs = p.cpu().numpy()
    np.testing.assert_array_equal(am.cpu().numpy(), ref.infer_probs.argmax(-1))
    fig, bad = rc.compare(ref, infer_probs, *train_step(torch, dm, case))
    print(case.label, " ".join("%s=%.2e" % kv for kv in fig.items()))
    assert not bad, bad
    return dm


@pytest.mark.parametrize("case", rc.CASES, ids=[c.label for c in rc.CASES])
def test_inference_and_train_step_match_the_oracle(torch, case):
    infer_and_train(torch, case)


@pytest.mark.parametrize("kind", rc.KINDS)
def test_smaller_batch_after_a_larger_one_on_the_same_model(torch, kind):
    """B = 33 (three blocks), then B = 1 on the same DeviceModel and workspace: nothing of the first step -- saved activations,
    per-sample losses, gradients of 32 more clips -- may reach the second"""
    first, second = rc.shrink_first_case(kind), rc.shrink_case(kind)
    dm = infer_and_train(torch, first)
    ws = dm._ws.data_ptr()
    ref = rc.reference(second)
    fig, bad = rc.compare(ref, None, *train_step(torch, dm, second))
    print(second.label, " ".join("%s=%.2e" % kv for kv in fig.items()))
    assert dm._ws.data_ptr() == ws                    # the workspace of the larger batch was reused
    assert not bad, bad


@pytest.mark.parametrize("kind", rc.KINDS)
def test_saturated_gates_give_exact_zeros_and_ones_not_nan(torch, kind):
    """gate pre-activations near +-100: sigmoidf_ reaches 0 by way of exp2 overflowing to inf and 1 by way of its underflow, and the
    backward pass multiplies by z (1 - z) there"""
    infer_and_train(torch, rc.saturated_case(kind), saturated=True)


@pytest.mark.parametrize("kind", rc.KINDS)
def test_too_wide_a_feature_map_is_refused_at_creation(torch, kind):
    from kws_amd import KwsError
    from kws_amd.model import ModelSpec
    ModelSpec(kind, 6, 9, rc.MAX_F)
    with pytest.raises(KwsError, match="feature_size <= 64") as e:
        ModelSpec(kind, 6, 9, rc.MAX_F + 1)
    assert e.value.code == rc.ERR_UNSUPPORTED


@pytest.mark.parametrize("kind", rc.KINDS)
def test_sequence_too_long_for_the_forward_tile_is_refused(torch, kind):
    from kws_amd import KwsError
    from kws_amd.model import DeviceModel, ModelSpec
    T, F = rc.REFUSED_INFER
    dm = DeviceModel(ModelSpec(kind, 6, T, F))
    with pytest.raises(KwsError, match="%s forward tile" % ("GRU" if kind == "simple_gru" else "LSTM")) as e:
        dm.forward(torch.zeros((3, T, F), device="cuda"))
    assert e.value.code == rc.ERR_UNSUPPORTED
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", rc.KINDS)
def test_training_refusal_touches_nothing(torch, kind):
    """110 x 20: the forward tile fits in LDS and the backward tile does not.  Inference works; a train step is refused before its
    forward kernel (which clears the gradients), its events and its overlap callback"""
    from kws_amd import KwsError
    case = rc.refused_train_case(kind)
    ref = rc.reference(case)                           # the oracle has no such limit
    dm = device_model(case, ref)
    x, y, _ = rc.inputs(case)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y.astype(np.int32)).cuda()
    p, am = dm.forward(xt)
    err = float(np.abs(p.cpu().numpy() - ref.infer_probs).max())
    print(case.label, "infer probs=%.2e" % err)
    assert err <= rc.PROB_ATOL
    np.testing.assert_array_equal(am.cpu().numpy(), ref.infer_probs.argmax(-1))
    dm.grads.fill_(7.0)
    dm.stats.fill_(-1.0)
    calls = []
    with pytest.raises(KwsError, match="%s backward tile" % ("GRU" if kind == "simple_gru" else "LSTM")) as e:
        dm.train_fwd_bwd(xt, yt, dropout_seed=case.dropout_seed, want_probs=True, overlap_event=torch.cuda.Event(),
                         overlap_callback=lambda: calls.append(1))
    assert e.value.code == rc.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert calls == []
    assert bool((dm.grads == 7.0).all()), "the refused step wrote %d gradient entries" % int((dm.grads != 7.0).sum())
    assert dm.stats.cpu().tolist() == [-1.0, -1.0]
