"""The train step of simple_cnn_lite at its grid, tile and padding edges, against the float64 oracle (oracle/model_oracle.py).

LiteCtx::forward(training = true) and LiteCtx::backward (csrc/kws_model.hip) are the only users of the depthwise kernels, of pw1_fwd / bwd_kernel,
partial_finalize_kernel and of the 1x1 instantiations of conv_gemm, conv_wgrad and conv_dgrad; the rest of the suite compares them with
the oracle at B = 40 and 64 on 30 x 20 and at B = 21 on 29 x 13 and 40 x 24.  tests/lite_train_cases.py holds one case per branch of the
launch arithmetic that those shapes miss (the 1024-block cap of the channel reductions in stages 1 and 2, MW = 2, 3, 4 of
conv_dgrad<32,16>, every side of depthwise 3's stride-2 padding, pool windows that drop pixels, less than one MFMA tile of rows), the
inputs, the shared oracle results and the comparison; tests/test_lite_train_host.py shows on the host that a plain float32
implementation passes these cases with a threefold margin and that a wrong padding side or a lost block fails them.

Bounds (the suite's existing ones, lite_train_cases.compare): probabilities and loss within 1e-4, the correct count equal, moving
statistics at rtol 2e-5 / atol 1e-6, every gradient tensor within 3e-4 of its largest entry, 3e-5 absolute on the two pointwise biases
whose true gradient is zero.  Every step prints a "FIGURES | case | ..." line; the module docstring of lite_train_cases.py records them."""
import collections

import numpy as np
import pytest

import lite_train_cases as tc

pytestmark = pytest.mark.gpu

IDS = [c.label for c in tc.CASES]
Got = collections.namedtuple("Got", "probs loss correct grads weights")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def device_model(case, ref):
    from kws_amd.model import DeviceModel, ModelSpec
    dm = DeviceModel(ModelSpec(tc.KIND, case.C, case.nf, case.fs))
    dm.set_weights(ref.weights0)
    return dm


def run_step(torch, dm, st):
    """one train_fwd_bwd of the oracle step's inputs -> what the device left"""
    xt = torch.from_numpy(np.array(st.x)).cuda()                 # copies: the shared reference arrays are read-only
    yt = torch.from_numpy(st.y.astype(np.int32)).cuda()
    cw = torch.from_numpy(st.cw.astype(np.float32)).cuda() if st.cw is not None else None
    probs = dm.train_fwd_bwd(xt, yt, cw, dropout_seed=st.seed, want_probs=True)
    torch.cuda.synchronize()
    stats = dm.stats.cpu().numpy()
    return Got(probs.cpu().numpy(), float(stats[0]) / st.B, float(stats[1]), dm.get_grads(), dm.get_weights())


def check(case, ref, st, got, mode):
    figs = tc.compare(ref, st, got.probs, got.loss, got.correct, got.grads, got.weights)
    by = {f.name: f for f in figs}
    worst = tc.worst_gradient(figs)
    print("FIGURES | %s | B = %d | %s | gradients %.1e of the largest entry (%s) | zero-gradient biases %.1e | probs %.1e | loss %.1e | "
          "moving statistics %.2g of their bound" % (case.label, st.B, mode, worst.rel, worst.name, max(f.err for f in figs if f.rel != f.rel and
                                                     f.name.startswith("grad ")), by["probs"].err, by["loss"].err,
                                                     max(f.err for f in figs if f.name.startswith("state "))))
    bad = tc.failures(figs)
    assert not bad, "%s, B = %d, %s: %s" % (case.label, st.B, mode, ["%s: %.3g against %.3g" % (f.name, f.err, f.bound) for f in bad])


@pytest.mark.parametrize("case", tc.CASES, ids=IDS)
def test_lite_train_step_against_the_oracle(torch, case):
    ref = tc.reference(case)
    dm = device_model(case, ref)
    for st in ref.steps:                                        # shrink: both steps on the same model and workspace, in the oracle's order
        check(case, ref, st, run_step(torch, dm, st), "default")


@pytest.mark.parametrize("label", tc.DETERMINISTIC)
def test_lite_deterministic_train_step_against_the_oracle_and_itself(torch, label):
    """set_deterministic(True): the same bounds against the oracle, and two runs from the same state agree bit for bit in the gradients
    and the moving statistics"""
    case = tc.CASE[label]
    ref = tc.reference(case)
    st = ref.steps[0]
    dm = device_model(case, ref)
    dm.set_deterministic(True)
    first = run_step(torch, dm, st)
    check(case, ref, st, first, "deterministic")
    dm.set_weights(ref.weights0)
    again = run_step(torch, dm, st)
    np.testing.assert_array_equal(again.probs, first.probs)
    assert again.loss == first.loss and again.correct == first.correct
    for name, a, b in zip([n for n, t in zip(ref.names, ref.trainable) if t], again.grads, first.grads):
        np.testing.assert_array_equal(a, b, err_msg="grad " + name)
    for name, a, b in zip(ref.names, again.weights, first.weights):
        np.testing.assert_array_equal(a, b, err_msg=name)


def test_the_cases_reach_every_mw_on_this_device(torch):
    """launch_dgrad picks MW from the device's compute-unit count, and the launch's profiling label is the same for every MW: that the
    cases above ran conv_dgrad<32,16> with MW = 1, 2, 3 and 4 rests on the restated rule and on this count"""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    if cus != tc.MI355X_CUS:
        pytest.skip("the MW cases are worked out for %d compute units and this device has %d: the cases ran, but which MW each took "
                    "is not asserted" % (tc.MI355X_CUS, cus))
    got = {c.label: tc.dgrad_mw(tc.stage_rows(c.B, c.nf, c.fs)[1], cus) for c in tc.CASES}
    assert got == {c.label: c.mw2 for c in tc.CASES}
    assert set(got.values()) == {1, 2, 3, 4}


def test_the_step_runs_the_layer_by_layer_kernels(torch):
    """the kernels this file is about, by their profiling labels, in one step of the smallest 30 x 20 case"""
    from kws_amd import lib as L
    case = tc.CASE["b3"]
    ref = tc.reference(case)
    dm = device_model(case, ref)
    L.prof_enable(True)
    try:
        got = run_step(torch, dm, ref.steps[0])
        labels = set(L.prof_report())
    finally:
        L.prof_enable(False)
    want = {"pw1_fwd_kernel", "pw1_bwd_kernel", "partial_finalize_kernel", "conv_gemm_fwd<16,32>", "conv_gemm_fwd<32,64>", "conv_gemm_fwd<64,128>",
            "conv_wgrad<16,32>", "conv_wgrad<32,64>", "conv_wgrad<64,128>", "conv_dgrad<32,16>", "conv_dgrad<64,32>", "conv_dgrad<128,64>"}
    want |= {"%s.L%d" % (k, l) for k in ("dwconv_fwd_kernel", "dwconv_wgrad_kernel", "channel_stats_kernel", "bn_bwd_reduce_kernel") for l in (1, 2, 3, 4)}
    want |= {"dwconv_dgrad_kernel.L%d" % l for l in (2, 3, 4)}
    assert want <= labels, sorted(want - labels)
    assert not tc.failures(tc.compare(ref, ref.steps[0], got.probs, got.loss, got.correct, got.grads, got.weights))
