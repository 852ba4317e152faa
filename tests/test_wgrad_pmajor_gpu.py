"""conv4's split-precision weight gradient in the position-major form (csrc/kws_conv.h: conv_wgrad_bf16_kernel<..., PM = true>,
WgradPm, wgrad_pm_plan; chosen by csrc/kws_cnn_plan.h: wgrad_pmajor) against deterministic mode, which keeps the pixel-major kernel with
one block along the pixel axis and a single add per element: the fixed-order reference.

The position-major form reduces over (output position, clip) in chunks of 32 clips at one position and never stages a (tap, position)
pair that lies in the 'same' padding; tests/wgrad_pmajor_cases.py restates its lists and its block partition and
tests/test_wgrad_pmajor_host.py proves them.  Here one simple_cnn train step through DeviceModel.train_fwd_bwd (split precision, 36
classes, dropout on) runs in both modes:

    default 30 x 20 map   B = 1, 2 (one partial chunk, seven XCDs without work), 31, 32, 33 (one clip either side of a chunk), 65,
                          B = 1377 (cases.B_FULL: the first batch at which conv4's launch is a full resident round, every block with
                          work), B = 1399 (cases.B_UNEQUAL: blocks of 3, 4 and 5 chunks, 23 clips in every position's last chunk) and
                          B = 1601
    32 x 24, B = 33       conv3 pads bottom and right only (pt = pl = 0): conv3's weight gradient is the pixel-major kernel, so this map
                          now only shows that conv4's form does not depend on how conv3 produced its input
    26 x 18, B = 33       3 x 2 outputs
    30 x 30, B = 33       4 x 4 outputs: the largest map that takes the form
    30 x 40, B = 33       4 x 5 outputs: must keep the pixel-major kernel; same ceiling, and both launches report under their labels

What is compared, as in tests/test_bn_bwd_apply_gpu.py: every gradient tensor and every BatchNorm moving statistic as
max|a - b| / max|b| against the 2e-5 that tests/test_model_gpu.py::test_matrix_precision_modes_agree allows between two modes, and the
step's statistics {sum of losses, hits} exactly.  The last test repeats that file's comparison of the default step with KWS_MATRIX_FP32
at B = 96, near ties resolved against the float64 oracle.

The inputs must be free of near ties (DESIGN.md section 4 "Parity caveat").  Each case's feature seed was chosen on the PARENT build of
the library alone, from at most five candidates per case (1000 k + 100 + B + frames, k = 1..5: the first at which the parent passes);
the parent build passes this file unchanged.  A seed was left out only where the two modes' loss sums differ in the last bit (the forward
passes round a per-sample loss differently at some inputs, tests/test_bn_bwd_apply_gpu.py); gradients were at most 2.05e-5 apart at
B = 1601's first candidate and below 1.8e-5 everywhere else (conv2d_1/kernel, whose atomics differ from run to run).  B = 1 is the one
case whose five candidates ALL fail on the parent, each on the loss sum's last bit and none on a gradient (at most 1.1e-6 apart): a
single clip's loss has no other clips to average the rounding away.  It runs at the seed tests/test_bn_bwd_apply_gpu.py found for the
same step at B = 1 among 24 (5101), at which the parent passes."""
import numpy as np
import pytest

import wgrad_pmajor_cases as wc

pytestmark = pytest.mark.gpu

C = 36
CEILING = 2e-5          # tests/test_model_gpu.py::test_matrix_precision_modes_agree
DEFAULT = (30, 20)
CASES = [(DEFAULT, B) for B in (1, 2, 31, 32, 33, 65, wc.B_FULL, wc.B_UNEQUAL, 1601)] + [
    (wc.ONE_SIDED, 33), (wc.ODD, 33), (wc.SIXTEEN, 33), (wc.FALLBACK, 33)]
LABELS = ("conv_wgrad_bf16<64,128>", "conv_wgrad_bf16<32,64>")


def candidates(fmap, B):
    return [1000 * k + 100 + B + fmap[0] for k in range(1, 6)]


# (map, B) -> k of the chosen candidate, where it is not the first
CHOSEN = {(DEFAULT, 31): 2, (DEFAULT, 32): 3, (DEFAULT, 1601): 2, (wc.ONE_SIDED, 33): 3, (wc.FALLBACK, 33): 2}
FEATURE_SEED = {case: candidates(*case)[CHOSEN.get(case, 1) - 1] for case in CASES}
FEATURE_SEED[(DEFAULT, 1)] = 5101       # see the module docstring


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def features(B, fmap, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B,) + tuple(fmap)) * 3.0
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


def run_step(torch, fmap, B, seed, det, profile=False):
    """one train step -> (gradients by name, moving statistics by name, [sum of losses, hits], the profile's labels or None)"""
    from kws_amd import lib as L
    from kws_amd.model import DeviceModel, ModelSpec
    spec = ModelSpec("simple_cnn", C, fmap[0], fmap[1])
    dm = DeviceModel(spec)
    dm.set_weights(weights(spec))
    if det:
        dm.set_deterministic(True)
    feat = torch.from_numpy(features(B, fmap, seed)).cuda()
    labels = torch.from_numpy(np.random.default_rng(B).integers(0, C, B).astype(np.int32)).cuda()
    report = None
    if profile:
        L.prof_enable(True)
    try:
        dm.train_fwd_bwd(feat, labels, dropout_seed=11)
        torch.cuda.synchronize()
        if profile:
            report = sorted(L.prof_report())
    finally:
        if profile:
            L.prof_enable(False)
    grads = dict(zip([t["name"] for t in spec.tensors if t["trainable"]], dm.get_grads()))
    state = {t["name"]: w for t, w in zip(spec.tensors, dm.get_weights()) if not t["trainable"]}
    return grads, state, dm.stats.cpu().numpy().copy(), report


def rel(got, want):
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-30))


def figures(torch, fmap, B, seed, profile=False):
    """default mode against deterministic mode: (worst gradient tensor, its name, the two conv kernels' figures, worst moving
    statistic, both modes' stats, the default step's labels)"""
    g, st, stats, report = run_step(torch, fmap, B, seed, False, profile)
    gd, std, stats_det, _ = run_step(torch, fmap, B, seed, True)
    assert all(np.isfinite(v).all() for v in g.values()) and np.isfinite(stats).all()
    worst = max(g, key=lambda n: rel(g[n], gd[n]))
    kernels = {n: rel(g[n], gd[n]) for n in g if n.endswith("kernel") and g[n].shape in ((3, 3, 32, 64), (3, 3, 64, 128))}
    return rel(g[worst], gd[worst]), worst, kernels, max(rel(st[n], std[n]) for n in st), stats, stats_det, report


@pytest.mark.parametrize("fmap,B", CASES, ids=["%dx%d-b%d" % (m[0], m[1], B) for m, B in CASES])
def test_default_step_matches_deterministic_mode(torch, fmap, B):
    assert wc.applies(*fmap) == (fmap != wc.FALLBACK)
    grad, name, kernels, state, stats, stats_det, report = figures(torch, fmap, B, FEATURE_SEED[(fmap, B)], profile=fmap == wc.FALLBACK)
    print("%d x %d, B = %d: gradients %.3e (%s), conv3 / conv4 kernels %s, moving statistics %.3e, loss sum %r / %r (deterministic), "
          "hits %r / %r" % (fmap[0], fmap[1], B, grad, name, " ".join("%.3e" % v for v in kernels.values()), state, stats[0], stats_det[0],
                            stats[1], stats_det[1]))
    assert len(kernels) == 2
    assert grad < CEILING, (name, grad)
    assert state < CEILING, state
    assert stats[0] == stats_det[0] and stats[1] == stats_det[1]
    if report is not None:
        assert all(label in report for label in LABELS), report


def test_default_step_matches_fp32_matrix_mode(torch):
    """tests/test_model_gpu.py::test_matrix_precision_modes_agree's comparison, with the precision set per model"""
    from kws_amd import lib as L
    from kws_amd.model import DeviceModel, ModelSpec
    from oracle import model_oracle as mo
    from tie_aware import TieAwareOracle
    B = 96
    om = mo.Model("simple_cnn", C).init_weights(0)
    rng = np.random.default_rng(1)
    ws = om.get_weights()
    for i, (li, n, t) in enumerate(om.weight_list()):
        if n in ("gamma", "moving_variance"):
            ws[i] = ws[i] * rng.uniform(0.5, 1.5, ws[i].shape)
        elif n in ("beta", "bias", "moving_mean"):
            ws[i] = ws[i] + 0.1 * rng.standard_normal(ws[i].shape)
    om.set_weights(ws)
    x = features(B, DEFAULT, 7)
    y = np.random.default_rng(8).integers(0, C, B)
    tao = TieAwareOracle(om, x.astype(np.float64), y)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y.astype(np.int32)).cuda()
    res = {}
    for mode in (L.MATRIX_BF16X6, L.MATRIX_FP32):
        dm = DeviceModel(ModelSpec("simple_cnn", C, 30, 20))
        dm.set_weights([w.astype(np.float32) for w in om.get_weights()])
        dm.set_precision(matrix=mode)
        probs = dm.train_fwd_bwd(xt, yt, want_probs=True)
        res[mode] = (probs.cpu().numpy(), [g.copy() for g in dm.get_grads()], float(dm.stats[0].item()) / B)
    (p6, g6, l6), (p32, g32, l32) = res[L.MATRIX_BF16X6], res[L.MATRIX_FP32]
    assert abs(l6 - l32) < 2e-6 and abs(l6 - tao.loss) < 1e-4
    np.testing.assert_allclose(p6, p32, rtol=0, atol=2e-6)
    labels = []
    for name, g in (("bf16x6", g6), ("fp32", g32)):
        ok, label, err, base_err = tao.match(g, 2e-5)
        print("%s: matches '%s' to %.1e (baseline %.1e)" % (name, label, err, base_err))
        assert ok, (name, label, err, base_err)
        labels.append(label)
    if labels[0] == labels[1]:
        for a, b2, w in zip(g6, g32, tao.base):
            assert np.abs(a - b2).max() / (np.abs(w).max() + 1e-12) < 2e-5
