"""The default train step's BatchNorm-backward apply kernel of layer 4 in its walking form (csrc/kws_layers.h:
bn_bwd_apply_routed_planes_kernel<true, WALK = true>), the accumulator apply kernel of layer 3 (bn_bwd_apply_acc_kernel<false>) and the
loss / accuracy sums that ride in the Dense weight gradient's launch (csrc/kws_conv.h: conv_wgrad_direct_kernel's LossSumJob) against
deterministic mode.

Deterministic mode takes none of the three: its plan (csrc/kws_cnn_plan.h) keeps the partial-sum BatchNorm backward with
bn_bwd_apply_planes_kernel / bn_bwd_apply_kernel, one thread per unit and no loop, and the stand-alone loss_reduce_kernel.  One simple_cnn
train step through DeviceModel.train_fwd_bwd (split precision, 30 x 20 map, 36 classes, dropout on) in both modes, at the batch sizes
where a grid-stride loop over units can go wrong (a "unit" is four channels of one pixel; layer 4 has B * 12 * 32 of them, layer 3
B * 12 * 16, a full grid is 1024 blocks * 256 threads, the walking loop takes six units at a time and the rest one by one):

    B = 1, 2   fewer units than one block's threads / a grid of a few blocks: most threads have no unit
    B = 17     a partial 16-clip group in the kernels around them
    B = 683    the first batch at which layer 4's grid reaches its 1024-block cap: 128 threads have two units, the others one
    B = 700    B * 12 * 32 is no multiple of the grid stride: unequal unit counts
    B = 1366   the same edge for layer 3 (B * 12 * 16 = 262272 > 262144); layer 4's threads have two or three units

What is compared: every gradient tensor and every BatchNorm moving statistic as max|a - b| / max|b| against the 2e-5 that
tests/test_model_gpu.py::test_matrix_precision_modes_agree allows between two modes, and the step's statistics {sum of losses, hits}
exactly: both modes form the sums in the same fixed order (csrc/kws_device.h: loss_sum_block).

The inputs must be free of near ties (DESIGN.md section 4 "Parity caveat"), and the two modes' forward passes round a per-sample loss
differently in its last bit at some inputs (accumulator against partial-sum batch statistics, MFMA against scalar logits), which can move
the float sum.  FEATURE_SEED was chosen on the PARENT build of the library alone (five seeds per batch size, 24 at B = 1): at each of these
seeds the parent build passes this file unchanged, gradients at most 1.3e-5 apart (conv2d_1/kernel, whose atomics differ from run to run by
about 1e-6) and equal statistics; no batch size needed a seed left out."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

C = 36
CEILING = 2e-5          # tests/test_model_gpu.py::test_matrix_precision_modes_agree
CASES = (1, 2, 17, 683, 700, 1366)
FEATURE_SEED = {1: 5101, 2: 1102, 17: 4117, 683: 1783, 700: 3800, 1366: 4466}


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


def run_step(torch, B, seed, det):
    """one train step -> (gradients by name, moving statistics by name, [sum of losses, hits])"""
    from kws_amd.model import DeviceModel, ModelSpec
    spec = ModelSpec("simple_cnn", C, 30, 20)
    dm = DeviceModel(spec)
    dm.set_weights(weights(spec))
    if det:
        dm.set_deterministic(True)
    feat = torch.from_numpy(features(B, seed)).cuda()
    labels = torch.from_numpy(np.random.default_rng(B).integers(0, C, B).astype(np.int32)).cuda()
    dm.train_fwd_bwd(feat, labels, dropout_seed=11)
    torch.cuda.synchronize()
    grads = dict(zip([t["name"] for t in spec.tensors if t["trainable"]], dm.get_grads()))
    state = {t["name"]: w for t, w in zip(spec.tensors, dm.get_weights()) if not t["trainable"]}
    return grads, state, dm.stats.cpu().numpy().copy()


def rel(got, want):
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-30))


def figures(torch, B, seed):
    """default mode against deterministic mode: (worst gradient tensor, its name, worst moving statistic, both modes' stats)"""
    g, st, stats = run_step(torch, B, seed, False)
    gd, std, stats_det = run_step(torch, B, seed, True)
    assert all(np.isfinite(v).all() for v in g.values()) and np.isfinite(stats).all()
    worst = max(g, key=lambda n: rel(g[n], gd[n]))
    return rel(g[worst], gd[worst]), worst, max(rel(st[n], std[n]) for n in st), stats, stats_det


@pytest.mark.parametrize("B", CASES)
def test_default_step_matches_deterministic_mode(torch, B):
    grad, name, state, stats, stats_det = figures(torch, B, FEATURE_SEED[B])
    print("B = %d: gradients %.3e (%s), moving statistics %.3e, loss sum %r / %r (deterministic), hits %r / %r"
          % (B, grad, name, state, stats[0], stats_det[0], stats[1], stats_det[1]))
    assert grad < CEILING, (name, grad)
    assert state < CEILING, state
    assert stats[0] == stats_det[0] and stats[1] == stats_det[1]
