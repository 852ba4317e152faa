"""conv2's wave-per-clip weight-gradient kernel (csrc/kws_conv2_wgrad_fast.h: conv2_wgrad_fast_kernel<15, 10>) against the block kernel
it replaces at the default map (csrc/kws_conv.h: conv_wgrad_clip_bf16_kernel<true>).

plan_cnn (csrc/kws_cnn_plan.h: wgrad2_fast) picks the new kernel for default, non-deterministic training at the 30 x 20 feature map;
deterministic mode keeps the block kernel (one persistent block, fixed order).  Both report under the same profiling label, so the
label cannot tell them apart -- the plan is the selection, and the fallback is forced through it with set_deterministic.

The two kernels add the same products in a different order, so the criterion is not bit equality but the distance to the exact-fp32
mode (set_precision(matrix=MATRIX_FP32)) on the same inputs, per tensor as max|g - g32| / max|g32| (the metric of
tests/test_model_gpu.py::test_matrix_precision_modes_agree): the new kernel may be at most twice as far from it as the PARENT build's
kernel was (PARENT below), and never further than that test's 2e-5.  Inputs are the MFCC-like batches of the single-step gradient
tests.  They must be free of near ties (DESIGN.md section 4 "Parity caveat"): at these batch sizes most seeds put some pre-activation
within float32 rounding of a ReLU6 gate or a pool-window tie, the split-precision and the exact-fp32 forward then resolve it differently,
and every gradient in front of that element moves by 1e-4 .. 4e-3 of its tensor's maximum -- in the parent build and in this one alike
(14 seeds per batch size measured on both builds: the two agree to three digits on every seed, 11 of 14 seeds at B = 4096 and 10 of 14 at
B = 2500 are beyond 1e-4).  FEATURE_SEED holds seeds at which the PARENT build is within the ceiling on every tensor; they were chosen on
the parent build alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C = 6
LABEL = "conv_wgrad_clip_bf16<16,32>"
CEILING = 2e-5          # tests/test_model_gpu.py::test_matrix_precision_modes_agree
# B = 4096: the benchmark's batch (512 blocks, two clips per wave); 2500: 313 blocks, the last one half empty; 193: fewer clips than waves
# of a full grid (49 blocks, the last one with a single clip)
CASES = (4096, 2500, 193)
# near-tie-free feature seeds (module docstring), chosen on the parent build: its worst tensor is within CEILING at each of them
FEATURE_SEED = {4096: 12096, 2500: 6500, 193: 293}
# Distance of the parent commit's default mode (conv_wgrad_clip_bf16_kernel<true> in its atomic form) to the exact-fp32 mode, measured with
# run_step() of this file on an MI355X against the parent build of the library, same weights and inputs: (conv2's kernel, worst tensor).
# Two runs of the same build differ by up to 8e-7 in this metric (float atomics), the exact-fp32 mode from itself by 7e-7.
PARENT = {
    4096: (2.828e-06, 8.583e-06),
    2500: (2.646e-06, 8.802e-06),
    193: (2.591e-06, 5.933e-06),
}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def features(B, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, 30, 20)) * 3.0
    x[..., 0] -= 10.0   # MFCC-like: a large negative c0 column
    return x.astype(np.float32)


def weights(spec):
    """glorot kernels with every BatchNorm scale / shift / moving statistic and bias moved off its initial value"""
    from kws_amd.init import init_weights
    ws = init_weights(spec, seed=3)
    rng = np.random.default_rng(4)
    for i, t in enumerate(spec.tensors):
        if t["name"].endswith(("gamma", "moving_variance")):
            ws[i] = (ws[i] * rng.uniform(0.5, 1.5, ws[i].shape)).astype(np.float32)
        elif t["name"].endswith(("beta", "bias", "moving_mean")):
            ws[i] = (ws[i] + 0.1 * rng.standard_normal(ws[i].shape)).astype(np.float32)
    return ws


def run_step(torch, B, mode):
    """one train step; mode: "default" (the plan's choice), "det" (deterministic: the block kernel), "fp32" (exact fp32 MFMA everywhere)"""
    from kws_amd import lib as L
    from kws_amd.model import DeviceModel, ModelSpec
    spec = ModelSpec("simple_cnn", C, 30, 20)
    dm = DeviceModel(spec)
    dm.set_weights(weights(spec))
    if mode == "det":
        dm.set_deterministic(True)
    if mode == "fp32":
        dm.set_precision(matrix=L.MATRIX_FP32)
    feat = torch.from_numpy(features(B, FEATURE_SEED[B])).cuda()
    labels = torch.from_numpy(np.random.default_rng(B).integers(0, C, B).astype(np.int32)).cuda()
    L.prof_enable(True)
    try:
        dm.train_fwd_bwd(feat, labels, dropout_seed=11)
        torch.cuda.synchronize()
        report = L.prof_report()
    finally:
        L.prof_enable(False)
    names = [t["name"] for t in spec.tensors if t["trainable"]]
    return dict(zip(names, dm.get_grads())), report


def rel(got, want):
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-30))


def conv2_name(grads):
    (name,) = [n for n, g in grads.items() if g.shape == (3, 3, 16, 32)]
    return name


def figures(torch, B):
    """(distance of `default` to fp32, of `det` to fp32, of `default` to `det`), each as (conv2's kernel, worst tensor)"""
    g, rep = run_step(torch, B, "default")
    gd, rep_det = run_step(torch, B, "det")
    g32, rep32 = run_step(torch, B, "fp32")
    assert LABEL in rep and LABEL in rep_det and LABEL not in rep32, (sorted(rep), sorted(rep32))
    k2 = conv2_name(g)
    assert np.isfinite(g[k2]).all() and np.abs(g[k2]).max() > 0
    pair = lambda a, b: (rel(a[k2], b[k2]), max(rel(a[n], b[n]) for n in a))
    return pair(g, g32), pair(gd, g32), pair(g, gd)


@pytest.mark.parametrize("B", CASES)
def test_fast_wgrad_is_as_close_to_fp32_as_the_block_kernel(torch, B):
    new, det, new_det = figures(torch, B)
    print("B = %d: default vs fp32 %.3e / %.3e (conv2 kernel / worst tensor), deterministic vs fp32 %.3e / %.3e, default vs deterministic %.3e / %.3e; "
          "parent build %r" % (B, new[0], new[1], det[0], det[1], new_det[0], new_det[1], PARENT[B]))
    for got, parent, what in zip(new, PARENT[B], ("conv2's kernel gradient", "the full gradient buffer")):
        assert parent is not None, "the parent build's figure for B = %d has not been measured yet (gpu: figures() against the parent library)" % B
        assert got <= min(2.0 * parent, CEILING), (what, got, parent)
