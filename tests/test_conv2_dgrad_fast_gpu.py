"""conv2's compile-time data-gradient kernel (csrc/kws_conv2_dgrad_fast.h: conv2_dgrad_fast_kernel<15, 10>) against the runtime-geometry
kernel it replaces at the default map (csrc/kws_conv.h: conv_dgrad_clip_bf16_kernel<true, true, false>).

plan_cnn (csrc/kws_cnn_plan.h: dgrad2_fast) picks the new kernel for default, non-deterministic training at the 30 x 20 feature map;
deterministic mode, a captured step, the fp32 mode and every other map keep the generic kernel.  Both report under the same profiling
label, so the label cannot tell them apart -- the plan is the selection (tests/test_conv2_dgrad_plan_host.py), and the fallback is forced
through it with set_deterministic.

The kernel's output is da1, the gradient layer 1's backward consumes: it reaches the gradient buffer as conv1's kernel and BatchNorm-1's
gamma and beta.  The criterion is the one of tests/test_conv2_wgrad_fast_gpu.py: the distance to the exact-fp32 mode
(set_precision(matrix=MATRIX_FP32)) on the same inputs, per tensor as max|g - g32| / max|g32|, taken for (i) the three tensors fed by da1
and (ii) the worst tensor of the gradient buffer.  The default mode may be at most twice as far from fp32 as the PARENT build was
(PARENT below), and never further than 2e-5, the ceiling of tests/test_model_gpu.py::test_matrix_precision_modes_agree.

Batch sizes are the smallest at which the persistent clip loop can go wrong; the grid is even_grid(B, 2 x 256 CUs):
  B = 3      three blocks, no second clip: the prefetch of the next clips is never issued
  B = 512    every block exactly one clip
  B = 513    257 blocks of two clips, the last one with one
  B = 1025   342 blocks of three clips, the last one with two

Inputs must be free of near ties (DESIGN.md section 4 "Parity caveat").  The seeds were chosen on the parent build alone: the first of
SEEDS(B), a fixed list of 20 per batch size, at which the parent's worst tensor is within the ceiling."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C = 6
LABEL = "conv_dgrad_clip_bf16<32,16>"
CEILING = 2e-5          # tests/test_model_gpu.py::test_matrix_precision_modes_agree
CASES = (3, 512, 513, 1025)


def SEEDS(B):
    """the fixed candidate list of a batch size"""
    return [B + 100 * k for k in range(20)]


# the first near-tie-free seed of SEEDS(B) on the parent build (module docstring)
# (at B = 1025 the first candidate, 1025, holds a near tie: the parent build is 3.5e-3 / 6.8e-3 from fp32 there).  No batch size was dropped.
FEATURE_SEED = {3: 3, 512: 512, 513: 513, 1025: 1125}
# Distance of the parent commit's default mode (conv_dgrad_clip_bf16_kernel<true, true, false>) to the exact-fp32 mode, measured with
# run_step() of this file on an MI355X against the parent build of the library, same weights and inputs:
# (worst of conv1's kernel / BatchNorm-1's gamma / beta, worst tensor of the gradient buffer).
# Two runs of the parent build differ by 0 in the first figure (layer 1's backward adds in a fixed order) and by up to 4.7e-7 on the worst
# tensor (float atomics elsewhere); the exact-fp32 mode differs from itself by 0 and up to 1.3e-6; the second run's figures were the same
# to three digits (513: 9.964e-06 on the worst tensor).  The parent's deterministic mode: 2.6e-6 / 3.0e-6, 7.9e-6 / 7.9e-6, 7.5e-6 / 1.0e-5,
# 9.4e-6 / 1.0e-5.  The compile-time kernel read 3.226e-06 / 3.582e-06, 8.212e-06 / 8.212e-06, 7.456e-06 / 9.964e-06, 9.805e-06 / 9.805e-06
# when it was written: da1 is not bit-equal to the generic kernel's (the compiler contracts the dz2 expression differently), and as close to fp32.
PARENT = {
    3: (3.301e-06, 3.582e-06),
    512: (8.285e-06, 8.285e-06),
    513: (7.453e-06, 9.959e-06),
    1025: (9.736e-06, 9.736e-06),
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


def run_step(torch, B, mode, seed=None):
    """one train step; mode: "default" (the plan's choice), "det" (deterministic: the generic kernel), "fp32" (exact fp32 MFMA everywhere)"""
    from kws_amd import lib as L
    from kws_amd.model import DeviceModel, ModelSpec
    spec = ModelSpec("simple_cnn", C, 30, 20)
    dm = DeviceModel(spec)
    dm.set_weights(weights(spec))
    if mode == "det":
        dm.set_deterministic(True)
    if mode == "fp32":
        dm.set_precision(matrix=L.MATRIX_FP32)
    feat = torch.from_numpy(features(B, FEATURE_SEED[B] if seed is None else seed)).cuda()
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


def da1_fed(grads):
    """the tensors that layer 1's backward forms from da1: conv1's kernel, BatchNorm-1's gamma and beta"""
    names = [n for n, g in grads.items() if g.shape in ((3, 3, 1, 16), (16,))]
    assert len(names) == 3, names
    return names


def pair(a, b):
    """(worst of the tensors fed by da1, worst tensor of the gradient buffer)"""
    return max(rel(a[n], b[n]) for n in da1_fed(a)), max(rel(a[n], b[n]) for n in a)


_fp32 = {}


def fp32_step(torch, B):
    """the exact-fp32 reference of a batch size: computed once, shared by both tests, never modified"""
    if B not in _fp32:
        g32, rep32 = run_step(torch, B, "fp32")
        assert LABEL not in rep32, sorted(rep32)
        _fp32[B] = g32
    return _fp32[B]


@pytest.mark.parametrize("B", CASES)
def test_fast_dgrad_is_as_close_to_fp32_as_the_generic_kernel(torch, B):
    g, rep = run_step(torch, B, "default")
    # proves only that a launch under the shared label happened, not which kernel ran: that is tests/test_conv2_dgrad_plan_host.py's part
    assert LABEL in rep, sorted(rep)
    for n in da1_fed(g):
        assert np.isfinite(g[n]).all() and np.abs(g[n]).max() > 0, n
    new = pair(g, fp32_step(torch, B))
    print("B = %d: default vs fp32 %.3e / %.3e (tensors fed by da1 / worst tensor); parent build %r" % (B, new[0], new[1], PARENT[B]))
    for got, parent, what in zip(new, PARENT[B], ("conv1's kernel, BatchNorm-1's gamma and beta", "the full gradient buffer")):
        assert got <= min(2.0 * parent, CEILING), (what, got, parent)


@pytest.mark.parametrize("B", CASES)
def test_deterministic_mode_keeps_the_generic_kernel_within_the_ceiling(torch, B):
    gd, rep = run_step(torch, B, "det")
    assert LABEL in rep, sorted(rep)
    assert all(np.isfinite(v).all() for v in gd.values())
    det = pair(gd, fp32_step(torch, B))
    print("B = %d: deterministic vs fp32 %.3e / %.3e (tensors fed by da1 / worst tensor)" % (B, det[0], det[1]))
    assert det[0] <= CEILING and det[1] <= CEILING, det
