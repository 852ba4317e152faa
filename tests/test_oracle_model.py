"""CPU tests: the numpy model oracle (oracle/model_oracle.py) against torch-CPU ops + autograd in float64.
torch supplies conv2d / batch_norm / max_pool2d / linear and the gradients; the GRU/LSTM cells are written by hand
in torch (nn.GRU forces tanh and another gate order) and differentiated by autograd."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import model_oracle as mo
from oracle import torch_ref as tr



def torch_forward(model_type, ws, x, training, drop_mask=None):
    """the torch-operator restatement (oracle/torch_ref.py: conv2d, F.batch_norm, max_pool2d, hand-written GRU / LSTM cells)"""
    return tr.forward(model_type, ws, x, training, drop_mask)


def make(model_type, C=6, seed=0, B=8):
    m = mo.Model(model_type, C).init_weights(seed)
    rng = np.random.default_rng(seed + 1)
    # perturb BN params / biases away from their trivial init so their gradients are exercised
    ws = m.get_weights()
    for i, (li, n, t) in enumerate(m.weight_list()):
        if n in ("gamma", "moving_variance"):
            ws[i] = ws[i] * rng.uniform(0.5, 1.5, ws[i].shape)
        elif n in ("beta", "bias", "moving_mean"):
            ws[i] = ws[i] + 0.1 * rng.standard_normal(ws[i].shape)
    m.set_weights(ws)
    x = rng.standard_normal((B, 30, 20)) * 3.0
    y = rng.integers(0, C, B)
    return m, x, y


def test_param_counts_match_survey():
    assert mo.Model("simple_cnn", 36).trainable_count() == 134932
    assert mo.Model("simple_cnn", 5).trainable_count() == 130933
    assert mo.Model("simple_cnn_lite", 36).trainable_count() == 50045
    assert mo.Model("simple_gru", 36).trainable_count() == 11844
    with pytest.raises(ValueError, match="Unsupported model type"):
        mo.Model("resnet", 3)


def test_same_padding_table():
    assert mo.same_pad(30, 3, 1) == (30, 1, 1) and mo.same_pad(7, 3, 2) == (4, 1, 1) and mo.same_pad(5, 3, 2) == (3, 1, 1)
    assert mo.same_pad(8, 3, 2) == (4, 0, 1)  # even input, stride 2: the extra pad goes to the END


@pytest.mark.parametrize("model_type", ["simple_cnn", "simple_cnn_lite", "simple_gru", "simple_lstm"])
@pytest.mark.parametrize("weighted", [False, True])
def test_forward_loss_and_gradients_vs_torch_autograd(model_type, weighted):
    C = 6
    m, x, y = make(model_type, C)
    rate = 0.5 if "cnn" in model_type else 0.2
    width = 256 if "cnn" in model_type else 20
    rng = np.random.default_rng(9)
    mask = (rng.uniform(size=(len(x), width)) >= rate) / (1 - rate)
    cw = np.array([0.3] + [0.7 / (C - 1)] * (C - 1)) if weighted else None

    ws_np = m.get_weights()
    loss, acc, p = mo.train_forward_backward(m, x, y, cw, dropout_mask=mask)
    grads = m.grad_list()

    ws_t = [torch.tensor(w, requires_grad=True) for w in ws_np]
    z = torch_forward(model_type, ws_t, torch.tensor(x), True, torch.tensor(mask))
    pt = torch.softmax(z, -1)
    py = pt[torch.arange(len(y)), torch.tensor(y)]
    if weighted:
        lt = (-torch.log(py) * torch.tensor(cw)[torch.tensor(y)]).mean()
    else:
        lt = (-torch.log(torch.clamp(py / pt.sum(-1), 1e-7, 1 - 1e-7))).mean()
    lt.backward()
    np.testing.assert_allclose(p, pt.detach().numpy(), atol=1e-10)
    assert abs(loss - lt.item()) < 1e-10
    tg = [w.grad.numpy() for w, (_, _, t) in zip(ws_t, m.weight_list()) if t]
    assert len(tg) == len(grads)
    for g, t, (li, n, _) in zip(grads, tg, [w for w in m.weight_list() if w[2]]):
        np.testing.assert_allclose(g, t, atol=1e-9, rtol=1e-8, err_msg="layer %d %s" % (li, n))


def test_inference_forward_uses_moving_stats():
    m, x, y = make("simple_cnn", 5)
    ws = [torch.tensor(w) for w in m.get_weights()]
    want = torch.softmax(torch_forward("simple_cnn", ws, torch.tensor(x), False), -1).numpy()
    np.testing.assert_allclose(m.predict(x), want, atol=1e-12)


def test_bn_moving_stats_update():
    m, x, y = make("simple_cnn", 5)
    bn = m.layers[1]
    mm0, mv0 = bn.moving_mean.copy(), bn.moving_variance.copy()
    z1 = m.layers[0].forward(x[..., None], True)
    mo.train_forward_backward(m, x, y)
    flat = z1.reshape(-1, 16)
    n = flat.shape[0]
    np.testing.assert_allclose(bn.moving_mean, mm0 * 0.99 + flat.mean(0) * 0.01, atol=1e-12)
    np.testing.assert_allclose(bn.moving_variance, mv0 * 0.99 + flat.var(0) * n / (n - 1) * 0.01, atol=1e-12)


@pytest.mark.parametrize("model_type,weighted", [("simple_cnn", False), ("simple_cnn", True), ("simple_cnn_lite", False), ("simple_gru", False),
                                                 ("simple_lstm", False)])
def test_multi_step_training_vs_torch_reference(model_type, weighted):
    """Six optimizer steps of the numpy oracle against oracle/torch_ref.py, which shares no code with it: torch's own
    F.batch_norm updates the moving statistics (momentum 0.99, epsilon 1e-3, unbiased variance), autograd supplies the
    gradients and a hand-written Keras-form Adam (epsilon outside the bias correction) the update.  Loss per step, every
    trainable tensor and every moving statistic agree to float64 rounding."""
    C, B = 6, 12
    m, _, _ = make(model_type, C, seed=4, B=B)
    flags = [t for _, _, t in m.weight_list()]
    tm = tr.TorchModel(model_type, m.get_weights(), flags)
    opt_np, opt_t = mo.Adam(1e-3), tr.KerasAdam(1e-3)
    rng = np.random.default_rng(21)
    cw = np.array([0.3] + [0.7 / (C - 1)] * (C - 1)) if weighted else None
    rate, width = (0.5, 256) if "cnn" in model_type else (0.2, 20)
    for step in range(6):
        x = rng.standard_normal((B, 30, 20)) * 3.0
        y = rng.integers(0, C, B)
        mask = (rng.uniform(size=(B, width)) >= rate) / (1 - rate)
        loss_np, _, p_np = mo.train_forward_backward(m, x, y, cw, dropout_mask=mask)
        m.set_trainable(opt_np.step(m.trainable_list(), m.grad_list()))
        loss_t, p_t, _ = tm.train_step(opt_t, x, y, cw, mask)
        assert abs(loss_np - loss_t) < 1e-10, (step, loss_np, loss_t)
        np.testing.assert_allclose(p_np, p_t.numpy(), atol=1e-10)
    for a, b, (li, n, t) in zip(m.get_weights(), tm.get_weights(), m.weight_list()):
        np.testing.assert_allclose(a, b, atol=1e-9, rtol=1e-9, err_msg="layer %d %s after 6 steps" % (li, n))
    x = rng.standard_normal((B, 30, 20)) * 3.0
    np.testing.assert_allclose(m.predict(x), tm.predict(x), atol=1e-10)     # inference with the updated moving statistics


def test_cross_entropy_clip_edges():
    p = np.array([[1.0 - 1e-9, 1e-9], [1e-9, 1.0 - 1e-9], [0.3, 0.7]])
    losses, d = mo.loss_and_grad(p, [0, 0, 0])
    np.testing.assert_allclose(losses, [-np.log(1 - 1e-7), -np.log(1e-7), -np.log(0.3)], rtol=1e-12)
    assert np.all(d[0] == 0) and np.all(d[1] == 0)                    # outside the clip range: no gradient
    np.testing.assert_allclose(d[2], np.array([0.3 - 1, 0.7]) / 3)


def test_adam_is_the_keras_form():
    rng = np.random.default_rng(0)
    p, opt = [rng.standard_normal(5)], mo.Adam(1e-3)
    m = v = np.zeros(5)
    w = p[0].copy()
    for t in range(1, 4):
        g = rng.standard_normal(5)
        m = 0.9 * m + 0.1 * g
        v = 0.999 * v + 0.001 * g * g
        w = w - 1e-3 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t) * m / (np.sqrt(v) + 1e-7)  # eps OUTSIDE the correction
        p = opt.step(p, [g])
    np.testing.assert_allclose(p[0], w, atol=1e-15)
    # differs from the PyTorch form (eps inside) when gradients are tiny
    g = np.full(5, 1e-9)
    o1 = mo.Adam(1e-3).step([np.zeros(5)], [g])[0]
    assert abs(o1[0]) < 1e-3 * 0.5


def test_dropout_hash_statistics_and_determinism():
    k = mo.dropout_keep(0x1234567ABCDEF, 1 << 16, 0.5)
    assert abs(k.mean() - 0.5) < 0.01
    assert np.array_equal(k, mo.dropout_keep(0x1234567ABCDEF, 1 << 16, 0.5))
    assert not np.array_equal(k, mo.dropout_keep(0x1234567ABCDEE, 1 << 16, 0.5))
    assert abs(mo.dropout_keep(7, 1 << 16, 0.2).mean() - 0.8) < 0.01


def test_training_reduces_loss_on_separable_task():
    rng = np.random.default_rng(3)
    C, B = 4, 64
    protos = rng.standard_normal((C, 30, 20)) * 2
    y = rng.integers(0, C, B)
    x = protos[y] + 0.3 * rng.standard_normal((B, 30, 20))
    for mt in ("simple_cnn", "simple_gru"):
        m = mo.Model(mt, C).init_weights(1)
        opt = mo.Adam(1e-2 if mt == "simple_gru" else 1e-3)
        l0 = None
        for it in range(25):
            loss, acc = mo.train_step(m, opt, x, y, dropout_seed=it)
            l0 = loss if l0 is None else l0
        assert loss < 0.6 * l0, (mt, l0, loss)


def test_tie_aware_matching_finds_a_flipped_decision():
    """tests/tie_aware.py (used by the GPU parity tests): a gradient computed with ONE near-threshold decision resolved the other
    way is matched by the corresponding alternative and by no other, and reported; an arbitrary perturbation matches nothing."""
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from tie_aware import TieAwareOracle
    m, x, y = make("simple_cnn", 6, seed=3, B=16)
    tao = TieAwareOracle(m, x, y, eps=2e-3, max_candidates=6)          # a wide eps so that this small batch has candidates
    assert len(tao.candidates) >= 2 and tao.n_near_ties >= len(tao.candidates)
    alts = list(tao.alternatives())
    assert alts[0][0] == "baseline"
    ok, label, err, base = tao.match(tao.base, 1e-9)
    assert ok and label == "baseline" and err == 0.0
    # (a gate under a pool window's losing element carries no gradient: flipping it changes nothing; take one that does)
    change = [max(np.abs(a - b).max() for a, b in zip(g, tao.base)) for _, g in alts]
    k = next(i for i in range(1, len(alts)) if change[i] > 1e-6)
    ok, label, err, base = tao.match(alts[k][1], 1e-9)
    assert ok and base > 1e-6 and label != "baseline"
    assert max(np.abs(a - b).max() for a, b in zip(alts[k][1], dict(alts)[label])) == 0.0
    bad = [g * 1.01 for g in tao.base]
    ok, label, err, base = tao.match(bad, 1e-4)
    assert not ok
    # the oracle is left with its baseline gradients
    for g, b in zip(m.grad_list(), tao.base):
        np.testing.assert_array_equal(g, b)


# ---- the loss options: ignore_index and grad_scale --------------------------------------------------------------------
def _keras_losses(p, y, weights, ignore_index):
    """classifier/loss.py's two classes as float32 numpy: one-hot labels; plain = K.categorical_crossentropy (renormalise, clip to
    [1e-7, 1 - 1e-7], -sum(onehot * log p)); weighted = -sum(onehot * log p) * sum(w * onehot); both `*= mask` under a truthy
    ignore_index"""
    f = np.float32
    p = p.astype(f)
    onehot = np.eye(p.shape[-1], dtype=f)[y]
    if ignore_index:
        mask = (y != ignore_index).astype(f)
    if weights is None:
        q = p / p.sum(-1, keepdims=True)
        q = np.clip(q, f(1e-7), f(1) - f(1e-7))
        losses = -np.sum(onehot * np.log(q), -1)
    else:
        losses = -np.sum(onehot * np.log(p), -1) * np.sum(weights.astype(f) * onehot, -1)
    if ignore_index:
        losses = losses * mask
    return losses


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("C", [5, 12])
def test_loss_options_match_the_keras_formulas(C, weighted):
    """loss_and_grad with ignore_index in {None, 0, 3, C - 1} against the float32 transcription above, in float32 and in float64;
    the plain rows reach both clip bounds (logits of scale 12)"""
    rng = np.random.default_rng(C + weighted)
    B = 64
    z = rng.standard_normal((B, C)) * np.where(np.arange(B) % 2, 4.0, 12.0)[:, None]
    y = rng.integers(0, C, B)
    y[:14] = [0, C - 1, 3, 3, C - 1, C - 1, 0, 3, 0, 3, C - 1, 1, 3, C - 1]
    z[8:14, :] = rng.standard_normal((6, C)) - 25.0 * (np.arange(C) != y[8:14, None])  # confidently right rows, labels 0, 3 and C - 1 among them
    p64 = mo.softmax(z)
    p32 = p64.astype(np.float32)
    w = rng.uniform(0.2, 1.0, C) if weighted else None
    py = p32[np.arange(B), y]
    if weighted:
        assert py.min() > 0                               # log(0) * mask is NaN in the formula: not a case of the contract
    else:
        assert (py < 1e-7).sum() >= 3 and (py > 1 - 1e-7).sum() >= 3
    plain = _keras_losses(p32, y, w, None)
    for ig in (None, 0, 3, C - 1):
        want = _keras_losses(p32, y, w, ig)
        assert want.dtype == np.float32
        if ig:
            assert (y == ig).sum() >= 3 and np.all(want[y == ig] == 0) and np.array_equal(want[y != ig], plain[y != ig])
        else:
            assert np.array_equal(want, plain)            # label 0 is not ignored
        l32, d32 = mo.loss_and_grad(p32, y, w, ignore_index=ig)
        l64, d64 = mo.loss_and_grad(p64, y, w, ignore_index=ig)
        assert l32.dtype == d32.dtype == np.float32
        np.testing.assert_allclose(l32, want, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(l64, want, rtol=1e-5, atol=1e-6)
        masked = (y == ig) if ig else np.zeros(B, bool)
        assert np.all(l64[masked] == 0) and np.all(d64[masked] == 0) and np.all(d32[masked] == 0)
        # the mean is over B, not over the live samples
        assert abs(l64.mean() - want.astype(np.float64).sum() / B) < 1e-5
        # grad_scale: dlogits only
        ls, ds = mo.loss_and_grad(p64, y, w, ignore_index=ig, grad_scale=0.25)
        assert np.array_equal(ls, l64) and np.array_equal(ds, d64 * 0.25)
    # the defaults are the former function
    l0, d0 = mo.loss_and_grad(p64, y, w)
    l1, d1 = mo.loss_and_grad(p64, y, w, None, 1.0)
    assert np.array_equal(l0, l1) and np.array_equal(d0, d1)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ignore_index", [None, 0, 3, 6])
def test_loss_options_dlogits_against_finite_differences(weighted, ignore_index):
    """dlogits = grad_scale * d(mean loss)/d(logits): central differences of the mean loss in float64 (step 1e-6), 1e-6 of the largest
    entry, on samples whose clip gate is open (logits of scale 2: all of them)"""
    C, B = 7, 10
    rng = np.random.default_rng(5)
    z = rng.standard_normal((B, C)) * 2.0
    y = rng.integers(0, C, B)
    y[:5] = [0, 3, 6, 3, 6]
    w = rng.uniform(0.2, 1.0, C) if weighted else None
    py = mo.softmax(z)[np.arange(B), y]
    assert py.min() > 1e-5 and py.max() < 1 - 1e-5       # every gate open, far from the bounds on both sides of the step

    def mean_loss(zz):
        return mo.loss_and_grad(mo.softmax(zz), y, w, ignore_index=ignore_index)[0].mean()

    h = 1e-6
    fd = np.zeros_like(z)
    for i in range(B):
        for c in range(C):
            e = np.zeros_like(z)
            e[i, c] = h
            fd[i, c] = (mean_loss(z + e) - mean_loss(z - e)) / (2 * h)
    for gs in (1.0, 1.0 / 3.0, 2.0):
        _, d = mo.loss_and_grad(mo.softmax(z), y, w, ignore_index=ignore_index, grad_scale=gs)
        assert np.abs(d - gs * fd).max() < 1e-6 * np.abs(gs * fd).max()
    if ignore_index:
        assert np.all(fd[y == ignore_index] == 0) and np.abs(fd[y != ignore_index]).min() > 0


@pytest.mark.parametrize("model_type", ["simple_cnn", "simple_gru"])
def test_train_forward_backward_options(model_type):
    """train_forward_backward passes both options through: the masked mean loss over B, the accuracy over every sample, gradients
    linear in grad_scale; and the tie-aware oracle of the GPU tests stores the masked / scaled dlogits"""
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from tie_aware import TieAwareOracle
    C = 6
    m, x, y = make(model_type, C, seed=2, B=12)
    y[:4] = [3, 3, 0, 5]
    w = np.linspace(0.3, 1.0, C)
    loss0, acc0, p0 = mo.train_forward_backward(m, x, y, w, dropout_seed=5)
    g0 = [g.copy() for g in m.grad_list()]
    loss, acc, p = mo.train_forward_backward(m, x, y, w, dropout_seed=5, ignore_index=3, grad_scale=0.5)
    g = [a.copy() for a in m.grad_list()]
    assert np.array_equal(p, p0) and acc == acc0
    losses = mo.loss_and_grad(p, y, w)[0]
    assert abs(loss - losses[y != 3].sum() / len(y)) < 1e-12 and loss < loss0
    w0 = w.copy()
    w0[3] = 0.0                                            # masking class 3 = giving it weight 0
    mo.train_forward_backward(m, x, y, w0, dropout_seed=5)
    for a, b in zip(g, m.grad_list()):
        np.testing.assert_allclose(a, 0.5 * b, rtol=1e-12, atol=1e-15)
    assert max(np.abs(a - 0.5 * b).max() for a, b in zip(g, g0)) > 1e-6
    tao = TieAwareOracle(m, x, y, w, 5, ignore_index=3, grad_scale=0.5)
    assert tao.loss == loss and np.all(tao.dlogits[y == 3] == 0)
    np.testing.assert_array_equal(tao.dlogits, mo.loss_and_grad(p, y, w, 3, 0.5)[1])
    for a, b in zip(tao.base, g):
        np.testing.assert_array_equal(a, b)
