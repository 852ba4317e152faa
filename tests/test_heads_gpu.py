"""GPU tests of the Dense(C, softmax) classifier head across the class range kws_model_create accepts (2..1024), against the float64
oracle (oracle/model_oracle.py): every head form the library dispatches on C (head_fwd_fast_kernel / head_fwd_kernel,
head_bwd_mfma_kernel / head_bwd_kernel, the fused inference tail, lite fp16 inference) on both sides of its bound, and the
first-maximum arg-max rule on exactly tied classes."""
import numpy as np
import pytest

from head_cases import (device_model, features, float_model, head_forms, head_inputs, tie_columns, tie_pairs)

pytestmark = pytest.mark.gpu

CNN_CLASSES = (2, 16, 17, 48, 49, 92, 93, 896, 897, 1024)
RNN_CLASSES = (2, 17, 48, 49, 227, 228, 976, 977, 1024)
# what each class count is meant to exercise: "mfma" = C <= 48 (MFMA head backward, fused train head, fused inference tail for
# simple_cnn), "fast" = head_fwd_fast_kernel above 48, "slow" = head_fwd_kernel / head_bwd_kernel within 64 KiB of LDS, "big" = above
ROLE = {"cnn": {2: "mfma", 16: "mfma", 17: "mfma", 48: "mfma", 49: "fast", 92: "fast", 93: "slow", 896: "slow", 897: "big", 1024: "big"},
        "rnn": {2: "mfma", 17: "mfma", 48: "mfma", 49: "fast", 227: "fast", 228: "slow", 976: "slow", 977: "big", 1024: "big"}}
SWEEP = ([(k, C, i % 2 == 1) for k in ("simple_cnn", "simple_cnn_lite") for i, C in enumerate(CNN_CLASSES)] +
         [(k, C, i % 2 == 1) for k in ("simple_gru", "simple_lstm") for i, C in enumerate(RNN_CLASSES)])


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _check_forms(kind, C, spec):
    """the head kernels (kind, C) runs, from the dispatch formulas, and that C sits on the side of each bound it is meant to test"""
    K = spec.tensors[-2]["shape"][0]
    assert spec.tensors[-2]["name"] == "score_predict/kernel" and K == head_inputs(kind)
    f = head_forms(kind, K, C)
    role = ROLE["rnn" if kind in ("simple_gru", "simple_lstm") else "cnn"][C]
    assert f["mfma_bwd"] == (role == "mfma") and f["fused_tail"] == (role == "mfma" and kind == "simple_cnn")
    assert f["fast_fwd"] == (role in ("mfma", "fast"))
    if role in ("slow", "big"):
        assert (f["slow_lds"] > 64 * 1024) == (role == "big")
    return f


def _infer_check(dm, om, x, torch, tol=1e-4):
    probs, am = dm.forward(torch.from_numpy(x).cuda())
    probs, am = probs.cpu().numpy(), am.cpu().numpy()
    want = om.predict(x.astype(np.float64))
    np.testing.assert_allclose(probs, want, atol=tol, rtol=0)
    top2 = np.sort(want, axis=-1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 2e-4
    np.testing.assert_array_equal(am[clear], want.argmax(-1)[clear])
    return probs, am, want


@pytest.mark.parametrize("kind,C,weighted", SWEEP)
def test_head_class_sweep_against_the_oracle(torch, kind, C, weighted):
    """inference at B = 1 and 37, and one train step at B = 37 (dropout on; class weights in every other case; labels 0 and C - 1
    included), against the float64 oracle"""
    from oracle import model_oracle as mo
    om = float_model(kind, C, seed=C)
    dm = device_model(om)
    _check_forms(kind, C, dm.spec)
    for B in (1, 37):
        _, _, want = _infer_check(dm, om, features(B, 100 + C + B), torch)
    assert np.unique(want.argmax(-1)).size >= min(C, 4)   # a centred head: the arg-max is not one class everywhere
    x = features(B, 200 + C)
    rng = np.random.default_rng(C)
    y = rng.integers(0, C, B)
    y[0], y[1] = 0, C - 1
    cw = rng.uniform(0.2, 1.0, C) if weighted else None
    seed = 0xABC00000 + C
    if kind == "simple_cnn":
        from tie_aware import TieAwareOracle
        tao = TieAwareOracle(om, x.astype(np.float64), y, cw, seed)
        loss, acc, p = tao.loss, tao.acc, tao.probs
    else:
        loss, acc, p = mo.train_forward_backward(om, x.astype(np.float64), y, cw, dropout_seed=seed)
    probs = dm.train_fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y.astype(np.int32)).cuda(),
                             torch.from_numpy(cw.astype(np.float32)).cuda() if weighted else None, dropout_seed=seed, want_probs=True)
    stats = dm.stats.cpu().numpy()
    np.testing.assert_allclose(probs.cpu().numpy(), p, atol=1e-4, rtol=0)
    assert abs(stats[0] / B - loss) < 1e-4, (stats[0] / B, loss)
    assert stats[1] == round(acc * B), (stats[1], acc * B)
    if kind == "simple_cnn":
        ok, label, err, base_err = tao.match(dm.get_grads(), 3e-4)
        assert ok, "gradients match no resolution of the oracle's near ties: best '%s' %g (baseline %g)" % (label, err, base_err)
    else:
        wants = om.grad_list()
        for t, (g, want, (li, n, _)) in enumerate(zip(dm.get_grads(), wants, [w for w in om.weight_list() if w[2]])):
            # lite (tests/test_model_gpu.py's bound, absolute floor 1e-6): a bias in front of BatchNormalization has an exactly-zero
            # gradient (oracle ~1e-16; the device's is a float32 cancellation), measured against its layer's pointwise-kernel gradient
            scale, floor = float(np.abs(want).max()), (1e-6 if kind == "simple_cnn_lite" else 0.0)
            if n == "bias" and isinstance(om.layers[li], mo.SeparableConv2D):
                scale = float(np.abs(wants[t - 1]).max())
            err = float(np.abs(g - want).max())
            assert err < 3e-4 * scale + floor, (kind, C, li, n, err, scale)


@pytest.mark.parametrize("C", [17, 48, 49])
def test_cnn_head_in_both_matrix_precisions(torch, C):
    """simple_cnn around the fused tail's 48 columns in the default split-bf16 mode and in fp32 (where the tail does not apply)"""
    from kws_amd import lib as L
    from oracle import model_oracle as mo
    om = float_model("simple_cnn", C, seed=7 * C)
    x = features(37, 300 + C)
    y = np.random.default_rng(C).integers(0, C, 37)
    y[0], y[1] = 0, C - 1
    loss, acc, p = mo.train_forward_backward(om, x.astype(np.float64), y)
    for mode in (L.MATRIX_BF16X6, L.MATRIX_FP32):
        dm = device_model(om)
        dm.set_precision(matrix=mode)
        assert head_forms("simple_cnn", 128, C, mode == L.MATRIX_BF16X6)["fused_tail"] == (C <= 48 and mode == L.MATRIX_BF16X6)
        _infer_check(dm, om, x, torch)
        probs = dm.train_fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y.astype(np.int32)).cuda(), want_probs=True)
        np.testing.assert_allclose(probs.cpu().numpy(), p, atol=1e-4, rtol=0)
        stats = dm.stats.cpu().numpy()
        assert abs(stats[0] / 37 - loss) < 1e-4 and stats[1] == round(acc * 37), (mode, stats, loss, acc)


@pytest.mark.parametrize("C", [2, 17, 48])
def test_lite_fp16_head_columns(torch, C):
    """lite fp16 inference up to its 48 head columns, with the tolerances of tests/test_model_gpu.py's fp16 test"""
    from kws_amd import lib as L
    om = float_model("simple_cnn_lite", C, seed=11 * C, spread=0.3)     # fp16 logits: errors in proportion to the head's scale
    dm = device_model(om)
    x = features(200, 400 + C)
    xd = torch.from_numpy(x).cuda()
    p32 = dm.forward(xd)[0].cpu().numpy()
    dm.set_precision(infer=L.INFER_FP16)
    p16, a16 = (t.cpu().numpy() for t in dm.forward(xd))
    want = om.predict(x.astype(np.float64))
    np.testing.assert_allclose(p16.sum(-1), 1.0, atol=1e-5)
    np.testing.assert_allclose(p16, want, atol=1e-3, rtol=0)
    np.testing.assert_allclose(p16, p32, atol=1e-3, rtol=0)
    assert np.abs(p16 - p32).max() > 0                                       # the fp16 path really ran
    top2 = np.sort(want, axis=-1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 2e-3
    np.testing.assert_array_equal(a16[clear], want.argmax(-1)[clear])
    assert (a16 == want.argmax(-1)).mean() >= 0.99


def test_lite_fp16_rejects_more_than_48_classes(torch):
    from kws_amd import lib as L
    om = float_model("simple_cnn_lite", 49, seed=3)
    dm = device_model(om)
    x = torch.from_numpy(features(4, 5)).cuda()
    dm.forward(x)                                                            # fp32 is fine
    dm.set_precision(infer=L.INFER_FP16)
    with pytest.raises(L.KwsError, match="fp16 inference"):
        dm.forward(x)


def test_cnn_1024_classes_deterministic(torch):
    """the largest head in the deterministic gradient mode: bit-reproducible, and within the oracle's tolerances"""
    from tie_aware import TieAwareOracle
    C, B = 1024, 37
    om = float_model("simple_cnn", C, seed=5)
    dm = device_model(om)
    dm.set_deterministic(True)
    x = features(B, 77)
    y = np.random.default_rng(78).integers(0, C, B)
    y[0], y[1] = 0, C - 1
    tao = TieAwareOracle(om, x.astype(np.float64), y, None, 99)
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y.astype(np.int32)).cuda()
    runs = []
    for _ in range(2):
        probs = dm.train_fwd_bwd(xt, yt, dropout_seed=99, want_probs=True)
        runs.append((probs.clone(), dm.grads.clone(), dm.stats.clone()))
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    np.testing.assert_allclose(runs[0][0].cpu().numpy(), tao.probs, atol=1e-4, rtol=0)
    stats = runs[0][2].cpu().numpy()
    assert abs(stats[0] / B - tao.loss) < 1e-4 and stats[1] == round(tao.acc * B)
    ok, label, err, base_err = tao.match(dm.get_grads(), 3e-4)
    assert ok, "gradients match no resolution of the oracle's near ties: best '%s' %g (baseline %g)" % (label, err, base_err)


# ---- exact ties: first maximum wins ------------------------------------------------------------------------------------
TIE_CASES = [("simple_cnn", 36),          # fused inference tail; fused Dense + head train kernel
             ("simple_cnn_lite", 36),     # head_fwd_fast_kernel; head_bwd_mfma_kernel; lite fp16
             ("simple_gru", 60),          # head_fwd_fast_kernel; head_bwd_kernel
             ("simple_gru", 36),          # the fused train head head_bwd_mfma_kernel<..., FWD>
             ("simple_cnn_lite", 100),    # head_fwd_kernel; head_bwd_kernel
             ("simple_gru", 300)]         # head_fwd_kernel; head_bwd_kernel


def _tied_model(kind, C, x, training=False):
    """the pairs' bias raised by three standard deviations of the logits on x (in training mode: batch statistics)"""
    from oracle import model_oracle as mo
    om = float_model(kind, C, seed=C + 1)
    if training:
        p = mo.train_forward_backward(om, x.astype(np.float64), np.zeros(len(x), np.int64))[2]
    else:
        p = om.predict(x.astype(np.float64))
    tie_columns(om, tie_pairs(C), boost=3.0 * float(np.log(p).std(0).mean()))
    return om


def _check_ties(probs, am, pairs, min_wins, every_pair=True):
    """bitwise-equal pair columns, and the lower index as the arg-max wherever a pair holds the maximum"""
    wins = np.zeros(len(probs), bool)
    for i, j in pairs:
        assert np.array_equal(probs[:, i].view(np.uint32), probs[:, j].view(np.uint32)), (i, j)
        w = probs[:, i] == probs.max(-1)
        assert w.sum() >= every_pair, ("pair never wins", i, j)
        np.testing.assert_array_equal(am[w], i)
        wins |= w
    assert wins.sum() >= min_wins, (wins.sum(), min_wins)


@pytest.mark.parametrize("kind,C", TIE_CASES)
def test_tied_classes_inference(torch, kind, C):
    from kws_amd import lib as L
    B = 200
    x = features(B, 1000 + C)
    om = _tied_model(kind, C, features(256, 9))
    dm = device_model(om)
    pairs = tie_pairs(C)
    want = om.predict(x.astype(np.float64))
    for i, j in pairs:                                       # the oracle ties to float64 rounding (its product is blocked by column)
        np.testing.assert_allclose(want[:, i], want[:, j], rtol=1e-12, atol=0)
    probs, am = (t.cpu().numpy() for t in dm.forward(torch.from_numpy(x).cuda()))
    np.testing.assert_allclose(probs, want, atol=1e-4, rtol=0)
    _check_ties(probs, am, pairs, B // 2)
    if kind == "simple_cnn_lite" and C <= 48:
        dm.set_precision(infer=L.INFER_FP16)
        p16, a16 = (t.cpu().numpy() for t in dm.forward(torch.from_numpy(x).cuda()))
        assert np.abs(p16 - probs).max() > 0                                     # the fp16 path really ran
        _check_ties(p16, a16, pairs, B // 2)


@pytest.mark.parametrize("kind,C", TIE_CASES)
def test_tied_classes_count_as_hits_only_for_the_first(torch, kind, C):
    """a train step (no dropout) whose labels are the lower class of a winning pair on some clips and the upper on others:
    the hits statistic counts only the former"""
    from oracle import model_oracle as mo
    B = 64
    x = features(B, 2000 + C)
    om = _tied_model(kind, C, x, training=True)
    dm = device_model(om)
    pairs = tie_pairs(C)
    rng = np.random.default_rng(C)
    _, _, p0 = mo.train_forward_backward(om, x.astype(np.float64), np.zeros(B, np.int64))
    y = rng.integers(0, C, B)
    first, second = 0, 0
    for i, j in pairs:
        w = np.nonzero(p0[:, i] == p0.max(-1))[0]
        y[w[0::2]], y[w[1::2]] = i, j
        first, second = first + w[0::2].size, second + w[1::2].size
    assert first >= 4 and second >= 4, (first, second)
    loss, _, p = mo.train_forward_backward(om, x.astype(np.float64), y)
    want_am = p.argmax(-1)
    for i, j in pairs:                                      # the oracle's pairs tie to float64 rounding only: first of the pair
        want_am[want_am == j] = i
    probs = dm.train_fwd_bwd(torch.from_numpy(x).cuda(), torch.from_numpy(y.astype(np.int32)).cuda(), want_probs=True)
    probs = probs.cpu().numpy()
    stats = dm.stats.cpu().numpy()
    am = probs.argmax(-1)                                   # numpy's first maximum
    _check_ties(probs, am, pairs, B // 2, every_pair=False)
    np.testing.assert_allclose(probs, p, atol=1e-4, rtol=0)
    assert stats[1] == (am == y).sum() == (want_am == y).sum(), (stats[1], (am == y).sum(), (want_am == y).sum())
    assert abs(stats[0] / B - loss) < 1e-4
