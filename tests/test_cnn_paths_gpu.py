"""simple_cnn's exact-fp32, deterministic and captured train steps (and their crossings with more than 48 classes and with feature maps
other than 30 x 20) against the float64 oracle, each with evidence of the kernels it ran.

csrc/kws_cnn_plan.h routes every stage of a call by matrix precision, deterministic mode, graph capture, geometry and class count; the
rest of the suite meets the oracle almost only in the default combination.  tests/cnn_path_cases.py holds the cases (64: the scenarios
crossed with the modes), the inputs, the shared oracle results and the kernel labels each case must and must not report;
tests/test_cnn_paths_host.py proves on the oracle alone that every case lists few enough near ties for tests/tie_aware.py to enumerate.

Per case: inference through dm.forward, one train step (probabilities, loss, hit count, every gradient tensor against a resolution of
the oracle's near ties, the BatchNorm moving statistics), bit-identical gradients on a second run in the deterministic modes, and a
profiled step whose labels name the expected path.  The captured cases replay the recorded step twice from restored state and a sentinel
gradient buffer, compare the replays with each other, and run one eager, profiled step afterwards (profiling stays out of the capture
itself), whose labels must be those of the same precision's eager path."""
import numpy as np
import pytest

import cnn_path_cases as cc

pytestmark = pytest.mark.gpu

SENTINEL = 123.0


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def device_model(torch, row, mode, ref):
    from kws_amd import lib as L
    from kws_amd.model import DeviceModel, ModelSpec
    dm = DeviceModel(ModelSpec("simple_cnn", row.C, row.nf, row.fs))
    dm.set_weights(ref.weights0)
    if "fp32" in mode:
        dm.set_precision(matrix=L.MATRIX_FP32)          # per model: a failing case cannot leak its mode into later tests
    if "det" in mode:
        dm.set_deterministic(True)
    assert dm.get_precision()[0] == (L.MATRIX_FP32 if "fp32" in mode else L.MATRIX_BF16X6)
    return dm


def check_step(dm, probs, row, ref, what, figures):
    """one finished train step (dm.grads, dm.stats, dm.state, probs) against the oracle's; appends the step's figures"""
    tao = ref.tao
    B = row.B
    p = probs.cpu().numpy()
    stats = dm.stats.cpu().numpy()
    grads = dm.get_grads()
    assert all(np.isfinite(g).all() for g in grads), what
    perr, lerr = float(np.abs(p - tao.probs).max()), abs(float(stats[0]) / B - tao.loss)
    ok, label, err, base_err = tao.match(grads, cc.grad_tol(B))
    figures.append((what, perr, lerr, err, label))
    print("%s: probs %.2e loss %.2e grads %.2e via '%s' (baseline %.2e, %d near ties listed)" % (
        what, perr, lerr, err, label, base_err, tao.n_near_ties))
    assert perr < 1e-4, (what, perr)
    assert lerr < 1e-4, (what, lerr)
    assert float(stats[1]) == round(tao.acc * B), (what, float(stats[1]), tao.acc * B)
    assert ok, "%s: gradients match no resolution of the oracle's near ties: best '%s' %g (baseline %g, bound %g)" % (
        what, label, err, base_err, cc.grad_tol(B))
    got_w = dm.get_weights()
    for i, trainable in enumerate(ref.trainable):
        if not trainable:
            np.testing.assert_allclose(got_w[i], ref.weights1[i], rtol=2e-5, atol=1e-6, err_msg="%s %s" % (what, ref.names[i]))
            assert not np.allclose(got_w[i], ref.weights0[i]), (what, ref.names[i])


def check_inference(torch, dm, xt, ref):
    probs, am = dm.forward(xt)
    want = ref.infer_probs
    perr = float(np.abs(probs.cpu().numpy() - want).max())
    assert perr < 1e-4, perr
    top2 = np.sort(want, axis=-1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 1e-5            # the rule of test_cnn_whole_batch_4096_against_the_torch_restatement
    np.testing.assert_array_equal(am.cpu().numpy()[clear], want.argmax(-1)[clear])
    return perr


def profiled(L, torch, step):
    """-> (the library's per-launch profile of one step, the step's probabilities)"""
    L.prof_enable(True)
    try:
        probs = step()
        torch.cuda.synchronize()
        return L.prof_report(), probs
    finally:
        L.prof_enable(False)


@pytest.mark.parametrize("case", cc.CASES, ids=[c.id for c in cc.CASES])
def test_cnn_path_against_the_oracle(torch, case):
    from kws_amd import lib as L
    row, mode = case.row, case.mode
    if row.name.startswith("mw"):
        # the profile's label is the same for every MW: which instantiation runs follows from the restated rule and this count alone
        cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
        if cus != cc.MI355X_CUS:
            pytest.skip("launch_dgrad's MW for this batch is worked out for %d compute units, this device has %d" % (cc.MI355X_CUS, cus))
    ref = cc.reference(row)
    x, y, cw = cc.inputs(row)
    dm = device_model(torch, row, mode, ref)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y.astype(np.int32)).cuda()
    cwt = torch.from_numpy(cw.astype(np.float32)).cuda() if cw is not None else None
    state0 = dm.state.clone()
    step = lambda: dm.train_fwd_bwd(xt, yt, cwt, dropout_seed=row.dropout_seed, want_probs=True)
    figures = []
    infer_err = check_inference(torch, dm, xt, ref)
    assert torch.equal(dm.state, state0)                # inference left the moving statistics alone

    if mode.startswith("captured"):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            probs = step()
        replays = []
        for rep in range(2):
            dm.state.copy_(state0)
            dm.grads.fill_(SENTINEL)
            probs.fill_(SENTINEL)
            g.replay()
            torch.cuda.synchronize()
            check_step(dm, probs, row, ref, "%s replay %d" % (case.id, rep), figures)
            replays.append(dm.grads.clone())
        scale = float(replays[0].abs().max())
        assert float((replays[0] - replays[1]).abs().max()) < 2e-5 * scale      # float atomics: order noise only
        # and the eager (accumulator) form still works afterwards; profiled, so that the model's precision shows in the labels
        eager_mode = "fp32" if "fp32" in mode else "default"
        dm.state.copy_(state0)
        dm.grads.fill_(SENTINEL)
        report, probs = profiled(L, torch, step)
        check_step(dm, probs, row, ref, "%s eager after the replays" % case.id, figures)
        labels = sorted(report)
        bad = cc.check_labels(report, row, eager_mode)
        assert not bad, "%s: the eager step after the replays ran another path than %s's: %s; labels seen: %s" % (
            case.id, eager_mode, "; ".join(bad), labels)
    else:
        dm.grads.fill_(SENTINEL)
        probs = step()
        torch.cuda.synchronize()
        check_step(dm, probs, row, ref, case.id, figures)
        first = dm.grads.clone()
        if "det" in mode:
            dm.state.copy_(state0)
            dm.grads.fill_(SENTINEL)
            step()
            torch.cuda.synchronize()
            assert torch.equal(dm.grads, first), "deterministic mode: the second run's gradient bits differ"
        # path evidence: the same step under the library's per-launch profile
        dm.state.copy_(state0)
        report, _ = profiled(L, torch, step)
        labels = sorted(report)
        bad = cc.check_labels(report, row, mode)
        assert not bad, "%s ran another path than the plan's for this mode: %s; labels seen: %s" % (case.id, "; ".join(bad), labels)
        if "det" in mode:
            assert torch.equal(dm.grads, first), "deterministic mode: the profiled run's gradient bits differ"
    for what, perr, lerr, gerr, label in figures:
        print("FIGURES | %s | infer %.1e | probs %.1e | loss %.1e | grads %.1e | %s | %s" % (
            what, infer_err, perr, lerr, gerr, label, " ".join(labels)))
