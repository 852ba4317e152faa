"""qrnn_kernel<G>, the one-kernel int8 forward of simple_gru and simple_lstm (csrc/kws_quant_rnn.hip), against the numpy restatement
(tests/int8_rnn_ref.py) over the range include/kws.h promises: every quarter edge of the A fragment (F), no prefetch / both parities
of the ping-pong tile / the longest sequence (T), every partly live head tile (C), every kind of partial 16-clip wave (B).
tests/qrnn_cases.py has the table, the builders and the comparison; tests/test_quant_rnn_shapes_host.py shows on the restatement
alone that the cases are saturated where they claim to be, not degenerate, and that the tolerances are the restatement's own.

The saturated GRU cases are bit-equal to the restatement.  The general-weight cases (both kinds) are held to qrnn_cases.TOL.  The head
and buffer tests run both kinds: tied classes across tile edges, a softmax whose every other term underflows, rows past B, and a graph
capture off the default geometry."""
import numpy as np
import pytest

import int8_rnn_ref as ref
import qrnn_cases as qc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def quantized(case, ws):
    """the QuantizedRNN of a case's weights; its codes and scales are the restatement's (the references are computed from those)"""
    from kws_amd.model import ModelSpec
    from kws_amd.quant import QuantizedRNN
    spec = ModelSpec(case.kind, case.C, case.T, case.F)
    p = np.zeros(spec.param_count, np.float32)
    for t, w in zip(spec.tensors, ws):
        assert tuple(t["shape"]) == w.shape, (t["name"], t["shape"], w.shape)
        p[t["offset"]:t["offset"] + t["size"]] = w.reshape(-1)
    q = QuantizedRNN.from_weights(spec, p)
    want = ref.quantize(case.kind, ws)
    for k, v in q.arrays.items():
        assert np.array_equal(np.asarray(v), want[k]), k
    return q


def run(torch, q, case, x):
    """the forward on the case's clips of the array x, which lies on the device as a whole: a partial batch starts at an odd clip, its
    first feature at an address that is no multiple of 16 bytes wherever T x F is odd"""
    xd = torch.from_numpy(x).cuda()
    out = q.forward(xd[case.start:case.start + case.B], logits=True)
    torch.cuda.synchronize()
    lg, pr, am = (t.cpu().numpy() for t in out)
    assert lg.shape == pr.shape == (case.B, case.C) and am.shape == (case.B,) and am.dtype == np.int32
    return lg, pr, am


def check_exact(lg, pr, am, want):
    """the assertions of test_saturated_gru_is_bit_equal_to_the_restatement (tests/test_quant_rnn_gpu.py)"""
    wl, wp, wa = want
    bad = np.nonzero((lg.view(np.uint32) != wl.view(np.uint32)).any(1))[0]
    assert bad.size == 0, "logits differ on %d clips, first %s: %s vs %s" % (bad.size, bad[:3], lg[bad[0]], wl[bad[0]])
    np.testing.assert_allclose(pr, wp, atol=1e-6, rtol=0)
    distinct = qc.top2_gap(wl) > 0
    np.testing.assert_array_equal(am[distinct], wa[distinct])


@pytest.mark.parametrize("case", qc.EXACT_CASES, ids=lambda c: c.label)
def test_saturated_gru_is_bit_equal_to_the_restatement(torch, case):
    ws = qc.weights(case)
    q = quantized(case, ws)
    lg, pr, am = run(torch, q, case, qc.feature_array(case))
    check_exact(lg, pr, am, [qc.clips(case, a) for a in qc.reference(case)])
    if case.variant == "zero_bias":                   # h = 0 through all T steps: the logits are the head bias
        assert np.array_equal(lg[qc.ZERO_CLIP].view(np.uint32), ws[4].view(np.uint32))


@pytest.mark.parametrize("case", qc.TOLERANCE_CASES, ids=lambda c: c.label)
def test_general_weights_match_the_restatement_within_the_gate_error(torch, case):
    q = quantized(case, qc.weights(case))
    lg, pr, am = run(torch, q, case, qc.feature_array(case))
    assert np.isfinite(lg).all() and np.isfinite(pr).all()
    fig, bad = qc.compare_tolerance(case, lg, am)
    print(case.label, " ".join("%s=%.4g" % kv for kv in fig.items()))
    assert not bad, (bad, fig)
    np.testing.assert_allclose(pr.sum(1, dtype=np.float64), 1.0, atol=1e-5, rtol=0)
    np.testing.assert_array_equal(am, lg.argmax(1))   # the first maximum of the device's own logits, as numpy takes it
    assert (pr[np.arange(case.B), am] == pr.max(1)).all()


# ---- head and buffers, both kinds -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", qc.KINDS)
@pytest.mark.parametrize("C", qc.TIE_CLASSES)
def test_tied_classes_across_tile_edges(torch, kind, C):
    """copied head columns in different 16-column tiles: bitwise-equal logits and probabilities on the device, the lower class as the
    arg-max -- for the LSTM too: both columns see the same codes of h_T, whatever the gate functions made of them"""
    case = qc.head_case(kind, C, qc.N_SHARE, "tie")
    ws = qc.tied_weights(case)
    q = quantized(case, ws)
    x = qc.feature_array(case)
    lg, pr, am = run(torch, q, case, x)
    if case.weights == "saturated":
        check_exact(lg, pr, am, ref.forward(kind, q.arrays, x))
    later = []
    for i, j in qc.tie_pairs(C):
        assert np.array_equal(lg[:, i].view(np.uint32), lg[:, j].view(np.uint32))
        assert np.array_equal(pr[:, i].view(np.uint32), pr[:, j].view(np.uint32))
        wins = lg[:, i] == lg.max(1)
        assert wins.sum() >= 10, (i, j, wins.sum())
        later.append(j)
    assert not np.isin(am, later).any()
    np.testing.assert_array_equal(am, lg.argmax(1))   # numpy's arg-max takes the first maximum too


@pytest.mark.parametrize("kind", qc.KINDS)
def test_softmax_underflow_gives_exact_zeros_and_a_one(torch, kind):
    case = qc.head_case(kind, qc.UNDERFLOW_C, qc.N_EXACT, "underflow")
    ws = qc.underflow_weights(case)
    q = quantized(case, ws)
    x = qc.feature_array(case)
    lg, pr, am = run(torch, q, case, x)
    if case.weights == "saturated":
        check_exact(lg, pr, am, ref.forward(kind, q.arrays, x))
    assert (lg[:, -1].astype(np.float64) - lg[:, :-1].max(1) > qc.UNDERFLOW_LEAD).all()
    assert not np.isnan(pr).any()
    assert (pr[:, -1] == 1).all() and not pr[:, :-1].any() and (pr.sum(1) == 1).all()
    assert (am == case.C - 1).all()


@pytest.mark.parametrize("kind", qc.KINDS)
@pytest.mark.parametrize("B", [1, 15, 17])
def test_rows_past_the_batch_keep_their_contents(torch, kind, B):
    """buffers of B + 16 rows full of a sentinel, in each of the single-output forms of test_optional_outputs_and_empty_batch: the
    dead rows of the last wave (and a whole wave more) are computed and must not be stored"""
    case = qc.head_case(kind, qc.BASE[2], qc.N_EXACT, "rows")
    q = quantized(case, qc.weights(case))
    x = torch.from_numpy(qc.feature_array(case)).cuda()[1:1 + B]
    lg, pr, am = q.forward(x, logits=True)
    R, C = B + 16, case.C
    for form in range(3):
        bufs = [torch.full((R, C), 7.0, device="cuda"), torch.full((R, C), 7.0, device="cuda"),
                torch.full((R,), -7, dtype=torch.int32, device="cuda")]
        q._launch(x, B, *[b if k == form else None for k, b in enumerate(bufs)])
        torch.cuda.synchronize()
        for k, (b, want) in enumerate(zip(bufs, (lg, pr, am))):
            if k == form:
                assert torch.equal(b[:B], want), (form, B)
                assert bool((b[B:] == (-7 if k == 2 else 7.0)).all()), "form %d wrote %d values past row %d" % (
                    form, int((b[B:] != (-7 if k == 2 else 7.0)).sum()), B)
            else:
                assert bool((b == (-7 if k == 2 else 7.0)).all())
    all3 = [torch.full((R, C), 7.0, device="cuda"), torch.full((R, C), 7.0, device="cuda"),
            torch.full((R,), -7, dtype=torch.int32, device="cuda")]
    q._launch(x, B, *all3)
    torch.cuda.synchronize()
    for k, (b, want) in enumerate(zip(all3, (lg, pr, am))):
        assert torch.equal(b[:B], want) and bool((b[B:] == (-7 if k == 2 else 7.0)).all()), k


@pytest.mark.parametrize("kind", qc.KINDS)
def test_graph_replay_off_the_default_geometry_equals_eager(torch, kind):
    """the forward captured through the entry InferenceSession uses (QuantizedRNN._launch on static buffers), B = 17: two replays, the
    outputs overwritten in between, equal the eager result bit for bit"""
    B = 17
    case = qc.head_case(kind, qc.BASE[2], qc.N_EXACT, "graph")
    q = quantized(case, qc.weights(case))
    x = torch.from_numpy(qc.feature_array(case)).cuda()[1:1 + B].clone()
    lg, pr, am = (t.clone() for t in q.forward(x, logits=True))      # also makes the device copy of the model outside the capture
    out = [torch.empty_like(lg), torch.empty_like(pr), torch.empty_like(am)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        q._launch(x, B, *out)
    for _ in range(2):
        out[0].fill_(float("nan"))
        out[1].fill_(float("nan"))
        out[2].fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], lg) and torch.equal(out[1], pr) and torch.equal(out[2], am)
    x.copy_(torch.from_numpy(qc.feature_array(case)).cuda()[20:20 + B])       # the replay reads the static input anew
    graph.replay()
    torch.cuda.synchronize()
    lg2, pr2, am2 = q.forward(x, logits=True)
    assert torch.equal(out[0], lg2) and torch.equal(out[1], pr2) and torch.equal(out[2], am2) and not torch.equal(lg2, lg)
