"""GPU tests of the train step's loss OPTIONS in every head form that carries a copy of the loss: ignore_index, grad_scale and the clip
gate of the plain loss (coef = 0 outside [1e-7, 1 - 1e-7]), against the float64 oracle (oracle/model_oracle.py: loss_and_grad).

The sites (tests/loss_cases.py: ROWS, train_head_site): dense_head_fused_kernel ("fused": simple_cnn, C <= 48, split-bf16),
head_bwd_mfma_kernel<.., FWD> ("mfma": the recurrent models up to 48 classes, simple_cnn in fp32 matrix mode), head_fwd_fast_kernel
("fast") and head_fwd_kernel ("slow").  Every case asserts from the dispatch formulas that it runs the site it is named for.  B = 37
(the last 16-sample tile is ragged) and dropout on unless said; tolerances are those of tests/test_heads_gpu.py."""
import numpy as np
import pytest

from head_cases import features
from loss_cases import (OPEN, RIGHT, RNN, ROW_IDS, ROWS, WRONG, Case, assert_zones, gate_labels, labels_with_share)

pytestmark = pytest.mark.gpu

B = 37
SEED = 0x10550000


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _weights(rng, C, weighted):
    return rng.uniform(0.2, 1.0, C) if weighted else None


def _bit_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- a. ignore_index ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("last", [True, False], ids=["k=C-1", "k=mid"])
@pytest.mark.parametrize("site,kind,C,mode", ROWS, ids=ROW_IDS)
def test_ignore_index_masks_loss_and_gradient(torch, site, kind, C, mode, last, weighted):
    """the ignored class k (C - 1, or a mid class) holds 20-40 % of the batch and wins some of its clips: loss sum, hits (masked clips
    that are classified right still count), probabilities and every gradient against the oracle; weighted: the same bits as the step
    without ignore_index whose class weights have w[k] = 0 (the same arithmetic, x * 0)"""
    k = C - 1 if last else (2 if C == 5 else 3)
    case = Case(torch, site, kind, C, mode)
    rng = np.random.default_rng(1000 * C + k)
    x = features(B, 600 + C)
    seed = SEED + C
    case.let_class_win(k, x, seed)
    wins = np.nonzero(case.train_logits(x, seed).argmax(-1) == k)[0][:4]
    y = labels_with_share(rng, B, C, k, first=wins)
    cw = _weights(rng, C, weighted)
    ref = case.oracle(x, y, cw, seed, ignore_index=k)
    masked = y == k
    assert (ref.probs.argmax(-1)[masked] == k).sum() >= 3            # hits under the mask
    unmasked = case.oracle(x, y, cw, seed)
    assert unmasked.loss - ref.loss > 1e-2 and unmasked.acc == ref.acc
    ref = case.oracle(x, y, cw, seed, ignore_index=k)
    got = case.device(x, y, cw, seed, ignore_index=k)
    case.check(got, ref, "ignore_index=%d" % k)
    if weighted:
        assert ref.probs[masked, k].min() > 1e-30 and got.probs[masked, k].min() > 0     # log(p_y) finite: -log(p_y) * 0 is 0
        cw0 = cw.copy()
        cw0[k] = 0.0
        zero = case.device(x, y, cw0, seed)
        assert _bit_equal(got.stats, zero.stats), (got.stats, zero.stats)
        case.same_grads(got.grads, zero.grads, "ignore_index=%d against w[k]=0" % k, exact=case.det)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("site,kind,C,mode", ROWS, ids=ROW_IDS)
def test_ignore_index_zero_and_negative_are_off(torch, site, kind, C, mode, weighted):
    """ignore_index = 0 and -1 are the call without the argument: clips with label 0 still train"""
    case = Case(torch, site, kind, C, mode)
    rng = np.random.default_rng(C)
    x = features(B, 610 + C)
    y = rng.integers(0, C, B)
    y[:8] = 0
    y[8], y[9] = C - 1, 1
    cw = _weights(rng, C, weighted)
    seed = SEED + 100 + C
    base = case.device(x, y, cw, seed)
    ref = case.oracle(x, y, cw, seed)
    case.check(base, ref, "no ignore_index")
    l0 = case.oracle(x, y, cw, seed, ignore_index=1).loss             # label 0 carries loss: masking another class is not the same
    assert abs(ref.loss - case.oracle(x, y, cw, seed, ignore_index=0).loss) == 0 and l0 != ref.loss
    for ig in (0, -1):
        got = case.device(x, y, cw, seed, ignore_index=ig)
        assert _bit_equal(got.stats, base.stats) and _bit_equal(got.probs, base.probs), ig
        case.same_grads(got.grads, base.grads, "ignore_index=%d against none" % ig, exact=case.det)
        assert float(got.grads.abs().max()) > 0


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("site,kind,C,mode", ROWS, ids=ROW_IDS)
def test_all_clips_masked_leaves_zero_gradients(torch, site, kind, C, mode, weighted):
    """every label = k, right after an ordinary step (a dirty gradient buffer): zero loss, every gradient entry exactly 0.0, hits as the
    oracle's, and the BatchNormalization moving statistics still move as the oracle's do"""
    k = C - 1
    case = Case(torch, site, kind, C, mode)
    rng = np.random.default_rng(C + 1)
    x = features(B, 620 + C)
    seed = SEED + 200 + C
    case.let_class_win(k, x, seed)
    cw = _weights(rng, C, weighted)
    dirty = case.device(features(B, 621 + C), rng.integers(0, C, B), cw, seed + 1)
    assert float(dirty.grads.abs().max()) > 0 and dirty.stats[0] > 0
    y = np.full(B, k)
    ref = case.oracle(x, y, cw, seed, ignore_index=k)
    assert ref.loss == 0 and 3 <= round(ref.acc * B) < B and all(np.all(g == 0) for g in ref.grads)
    got = case.device(x, y, cw, seed, ignore_index=k)
    assert got.stats[0] == 0.0, got.stats
    assert got.stats[1] == round(ref.acc * B), (got.stats, ref.acc * B)
    assert bool(torch.all(got.grads == 0.0)), (int((got.grads != 0).sum()), int(torch.isnan(got.grads).sum()))
    np.testing.assert_allclose(got.probs, ref.probs, atol=1e-4, rtol=0)
    if case.has_state:
        case.check_state(got, ref)


# ---- b. grad_scale ----------------------------------------------------------------------------------------------------------
SCALES = (0.25, 1.0 / 3.0, 2.0)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("site,kind,C,mode", ROWS, ids=ROW_IDS)
def test_grad_scale_scales_the_gradients_only(torch, site, kind, C, mode, weighted):
    """grad_scale in {0.25, 1/3, 2}: gradients = grad_scale x the oracle's; loss sum, hits, probabilities and moving statistics are those of
    the grad_scale = 1 step (bit-equal in deterministic mode, to order noise 1e-5 otherwise).  simple_cnn / simple_cnn_lite are then
    switched to deterministic mode, where everything but the gradients is bit-equal for every scale, and the gradients are bit-equal to
    the scaled grad_scale = 1 gradients for the powers of two -- a scale applied anywhere but in dlogits would break that."""
    case = Case(torch, site, kind, C, mode)
    rng = np.random.default_rng(C + 2)
    x = features(B, 630 + C)
    y = rng.integers(0, C, B)
    y[0], y[1] = 0, C - 1
    cw = _weights(rng, C, weighted)
    seed = SEED + 300 + C
    base = case.device(x, y, cw, seed)
    ref1 = case.oracle(x, y, cw, seed)
    case.check(base, ref1, "grad_scale=1")
    for gs in SCALES:
        ref = case.oracle(x, y, cw, seed, grad_scale=gs)
        assert ref.loss == ref1.loss
        got = case.device(x, y, cw, seed, grad_scale=gs)
        case.check(got, ref, "grad_scale=%g" % gs)
        if case.has_state:
            case.check_state(got, ref)
        if case.det:
            assert _bit_equal(got.stats, base.stats) and _bit_equal(got.probs, base.probs) and torch.equal(got.state, base.state), gs
        else:
            assert got.stats[1] == base.stats[1] and abs(got.stats[0] - base.stats[0]) <= 1e-5 * abs(base.stats[0]), (gs, got.stats, base.stats)
            np.testing.assert_allclose(got.probs, base.probs, atol=1e-5, rtol=0)
            if case.has_state:
                assert torch.allclose(got.state, base.state, rtol=1e-5, atol=1e-7), gs
    if kind in RNN:
        return
    case.dm.set_deterministic(True)
    base = case.device(x, y, cw, seed)
    case.check(base, case.oracle(x, y, cw, seed), "deterministic grad_scale=1")
    for gs in SCALES:
        got = case.device(x, y, cw, seed, grad_scale=gs)
        assert _bit_equal(got.stats, base.stats) and _bit_equal(got.probs, base.probs) and torch.equal(got.state, base.state), gs
        if gs in (0.25, 2.0):
            assert torch.equal(got.grads, base.grads * gs), (gs, float((got.grads - base.grads * gs).abs().max()))
        else:
            case.check(got, case.oracle(x, y, cw, seed, grad_scale=gs), "deterministic grad_scale=%g" % gs)


RNN_ROWS = [r for r in ROWS if r[1] in RNN]


@pytest.mark.parametrize("options", [False, True], ids=["plain", "weighted+ignore_index"])
@pytest.mark.parametrize("site,kind,C,mode", RNN_ROWS, ids=[i for i, r in zip(ROW_IDS, ROWS) if r[1] in RNN])
def test_shards_with_grad_scale_add_up_to_the_whole_batch(torch, site, kind, C, mode, options):
    """the data-parallel rule on one GPU: grad_scale = local clips / global clips, then sum.  The recurrent models have no
    BatchNormalization (clips do not couple); dropout off; 96 clips as shards of 40, 55 and 1"""
    n, cuts = 96, (0, 40, 95, 96)
    case = Case(torch, site, kind, C, mode)
    rng = np.random.default_rng(C + 3)
    x = features(n, 640 + C)
    k = 3 if options else None
    y = labels_with_share(rng, n, C, 3) if options else rng.integers(0, C, n)
    y[95] = 0 if options else y[95]                                    # the one-clip shard is live
    cw = _weights(rng, C, options)
    kw = dict(ignore_index=k) if options else {}
    ref = case.oracle(x, y, cw, 0, ignore_index=k)
    whole = case.device(x, y, cw, 0, **kw)
    case.check(whole, ref, "whole batch")
    total, loss, hits = torch.zeros_like(whole.grads), 0.0, 0
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        part = case.device(x[lo:hi], y[lo:hi], cw, 0, grad_scale=(hi - lo) / n, **kw)
        total += part.grads
        loss += float(part.stats[0])
        hits += int(part.stats[1])
    assert hits == whole.stats[1] == round(ref.acc * n)
    assert abs(loss - float(whole.stats[0])) < 1e-4 * n and abs(loss / n - ref.loss) < 1e-4
    spec = case.dm.spec
    parts = [total.cpu().numpy()[t["offset"]:t["offset"] + t["size"]].reshape(t["shape"]) for t in spec.tensors if t["trainable"]]
    worst = 0.0
    for g, w, d in zip(parts, ref.grads, whole.grad_list):
        scale = float(np.abs(w).max())
        worst = max(worst, float(np.abs(g - w).max()) / scale, float(np.abs(g - d).max()) / scale)
        assert np.abs(g - w).max() < 3e-4 * scale and np.abs(g - d).max() < 3e-4 * scale
    print("FIGURES %s %s C=%d | shards %s: gradient sum %.3g of the largest entry (3e-4), loss sum %.3g (%.3g)"
          % (site, kind, C, "weighted+ignore_index" if options else "plain", worst, abs(loss - float(whole.stats[0])), 1e-4 * n))


# ---- c. the clip gate of the plain loss ---------------------------------------------------------------------------------------
LADDER = ((12.0, 37), (12.0, 96), (20.0, 37), (20.0, 96), (32.0, 96))       # raise the spread, then the batch, until every zone holds 3 clips


def _gate_case(torch, site, kind, C, mode, seed):
    """a head with logits wide enough for the three zones, and one label per clip chosen from the oracle's float64 probabilities"""
    for spread, n in LADDER:
        case = Case(torch, site, kind, C, mode, spread=spread)
        x = features(n, 650 + C)
        z = case.train_logits(x, seed)
        p = np.exp(z - z.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        lab = gate_labels(p, np.random.default_rng(C + 4))
        if lab is not None and min((lab[1] == zz).sum() for zz in (OPEN, WRONG, RIGHT)) >= 3:
            assert_zones(p, lab[0], lab[1])
            return case, x, lab[0], lab[1]
    raise AssertionError("no spread / batch of the ladder puts 3 clips in every zone")


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("site,kind,C,mode", ROWS, ids=ROW_IDS)
def test_clip_gate_zones(torch, site, kind, C, mode, weighted):
    """every clip open (1e-5 < p_y < 1 - 1e-5), confidently wrong (1e-30 < p_y < 1e-8) or confidently right (the other classes sum to
    less than 2e-8), none in the bands where float32 and float64 may sit on different sides of a bound.  Plain loss: the closed
    clips have loss -log of the bound and a zero gradient row; weighted: no clip, -log(p_y) w_y and the full gradient."""
    seed = SEED + 400 + C
    case, x, y, zone = _gate_case(torch, site, kind, C, mode, seed)
    cw = _weights(np.random.default_rng(C + 5), C, weighted)
    ref = case.oracle(x, y, cw, seed)
    assert_zones(ref.probs, y, zone)
    if not weighted:                                                   # the closed clips: a constant loss, which the mean must contain
        closed = (zone == WRONG).sum() * -np.log(1e-7) + (zone == RIGHT).sum() * -np.log(1 - 1e-7)
        assert ref.loss * len(y) > closed > 3 * 16.0
    ref = case.oracle(x, y, cw, seed)
    got = case.device(x, y, cw, seed)
    case.check(got, ref, "gate zones %s" % [(zone == z).sum() for z in (OPEN, WRONG, RIGHT)])


@pytest.mark.parametrize("site,kind,C,mode", ROWS, ids=ROW_IDS)
def test_clip_gate_with_every_option(torch, site, kind, C, mode):
    """gate zones + ignore_index + grad_scale = 1/3 + class weights in one step, and the same without weights (where the gate closes)"""
    seed = SEED + 500 + C
    case, x, y, zone = _gate_case(torch, site, kind, C, mode, seed)
    rng = np.random.default_rng(C + 6)
    k = int(next(c for c in y[zone == WRONG] if c > 0))               # masks at least one confidently-wrong clip
    for cw in (_weights(rng, C, True), None):
        plain = case.oracle(x, y, cw, seed, grad_scale=1.0 / 3.0)
        ref = case.oracle(x, y, cw, seed, ignore_index=k, grad_scale=1.0 / 3.0)
        assert plain.loss - ref.loss > 1e-2
        got = case.device(x, y, cw, seed, ignore_index=k, grad_scale=1.0 / 3.0)
        case.check(got, ref, "gate + ignore_index=%d + grad_scale=1/3 + %s" % (k, "weights" if cw is not None else "no weights"))


# ---- through the host API ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("kind", ["simple_cnn", "simple_gru"])
def test_fit_forwards_ignore_index(torch, kind, weighted):
    """compile(loss=...(ignore_index=k)) and one epoch of exactly one batch: the history's loss is the oracle's masked mean"""
    from classifier.loss import SparseCategoricalCrossEntropy, WeightedSparseCategoricalCrossEntropy
    from classifier.model import get_model
    from common.model_utils import get_optimizer
    from head_cases import float_model
    from oracle import model_oracle as mo
    C, n, k = 6, 48, 3
    om = float_model(kind, C, seed=31)
    rng = np.random.default_rng(32)
    x = features(n, 33)
    y = labels_with_share(rng, n, C, k, share=0.4)
    w = rng.uniform(0.2, 1.0, C) if weighted else None
    m = get_model(kind, C)
    m.set_weights(om.get_weights())
    loss = WeightedSparseCategoricalCrossEntropy(w, ignore_index=k) if weighted else SparseCategoricalCrossEntropy(ignore_index=k)
    m.compile(get_optimizer("adam", 1e-3, decay_type=None), loss, ["accuracy"])
    seed = (m._dropout_base << 20) + 64                                # fit's first step (classifier/model.py)
    w0 = om.get_weights()
    want, acc, _ = mo.train_forward_backward(om, x.astype(np.float64), y, w, dropout_seed=seed, ignore_index=k)
    om.set_weights(w0)
    unmasked = mo.train_forward_backward(om, x.astype(np.float64), y, w, dropout_seed=seed)[0]
    assert unmasked - want > 1e-2
    h = m.fit(x[..., None] if kind == "simple_cnn" else x, y, batch_size=n, epochs=1, shuffle=False, verbose=0)
    got = h.history["loss"][0]
    print("FIGURES fit %s %s: loss %.6f oracle %.6f (unmasked %.6f)" % (kind, "weighted" if weighted else "plain", got, want, unmasked))
    assert abs(got - want) < 1e-4, (got, want, unmasked)
    assert abs(h.history["accuracy"][0] - acc) < 1e-6
