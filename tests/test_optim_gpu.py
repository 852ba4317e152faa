"""GPU tests of kws_optimizer_step (include/kws.h): every optimizer x option combination against the float64 oracle
(tests/optim_ref.py) on the real tensor tables of simple_cnn and simple_gru, run-to-run bit identity, the non-finite norm rules, the
default options against the plain kernels bit for bit, and fit() with clipped / momentum optimizers."""
import numpy as np
import pytest

from optim_ref import RefOptimizer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


COMBOS = [
    ("sgd", dict(clipnorm=1.0)),
    ("sgd", dict(momentum=0.9)),
    ("sgd", dict(momentum=0.9, nesterov=True, global_clipnorm=1.0)),
    ("sgd", dict(momentum=0.5, clipvalue=0.05, clipnorm=1.0)),
    ("sgd", dict(nesterov=True, clipvalue=0.05)),                     # nesterov without momentum: plain SGD
    ("rmsprop", dict(clipnorm=1.0)),
    ("rmsprop", dict(momentum=0.9)),
    ("rmsprop", dict(centered=True)),
    ("rmsprop", dict(centered=True, momentum=0.9, global_clipnorm=1.0)),
    ("rmsprop", dict(clipvalue=0.05, centered=True, clipnorm=1.0)),
    ("adam", dict(clipnorm=1.0)),
    ("adam", dict(global_clipnorm=1.0)),
    ("adam", dict(clipvalue=0.05)),
    ("adam", dict(amsgrad=True)),
    ("adam", dict(amsgrad=True, clipnorm=1.0, clipvalue=0.05)),
]
LR = {"sgd": 0.05, "rmsprop": 1e-3, "adam": 1e-3}
SLOT_ATTR = {"m": "adam_m", "v": "adam_v", "vhat": "opt_vhat", "mg": "opt_mg", "mom": "opt_mom"}


def _optimizer(kind, kw, lr=None):
    from common import model_utils as mu
    cls = {"sgd": mu.SGD, "rmsprop": mu.RMSprop, "adam": mu.Adam}[kind]
    return cls(LR[kind] if lr is None else lr, **kw)


def _reference(opt):
    """the oracle with the hyperparameters the kernel sees: rounded to float32 (1 - 0.999 differs by 1.3e-5 from 1 - float32(0.999))"""
    kind = opt.kind
    f = lambda x: float(np.float32(x or 0.0))
    return RefOptimizer(kind, f(opt.current_lr()), beta1=f(getattr(opt, "beta_1", 0.9)),
                        beta2=f(opt.rho if kind == "rmsprop" else getattr(opt, "beta_2", 0.999)), eps=f(getattr(opt, "epsilon", 1e-7)),
                        momentum=f(getattr(opt, "momentum", 0.0)), nesterov=getattr(opt, "nesterov", False),
                        centered=getattr(opt, "centered", False), amsgrad=getattr(opt, "amsgrad", False),
                        clipvalue=f(opt.clipvalue), clipnorm=f(opt.clipnorm), global_clipnorm=f(opt.global_clipnorm))


def _grads(spec, rng, step):
    """per variable: norm 3 (clipped at 1), 0.3 (not clipped) or, for variable 2, all zeros; entries spread over 3 decades"""
    offsets, sizes = spec.optimizer_segments()
    g = np.zeros((spec.param_count,), np.float32)
    real = {t["offset"]: t["size"] for t in spec.tensors if t["trainable"]}
    for k, (o, n) in enumerate(zip(offsets, sizes)):
        if k == 2:
            continue
        x = rng.standard_normal(real[o]) * 10.0 ** rng.uniform(-1.5, 1.5, real[o])
        target = 3.0 if (k + step) % 2 == 0 else 0.3
        g[o:o + real[o]] = (x * target / np.linalg.norm(x)).astype(np.float32)
    return g


def _model(torch, model_type, seed=0):
    from kws_amd.model import DeviceModel, ModelSpec
    spec = ModelSpec(model_type, 36, 30, 20)
    dm = DeviceModel(spec)
    p = (0.1 * np.random.default_rng(seed).standard_normal(spec.param_count)).astype(np.float32)
    mask = np.zeros_like(p, bool)                # the padding between tensors stays zero
    for t in spec.tensors:
        if t["trainable"]:
            mask[t["offset"]:t["offset"] + t["size"]] = True
    p[~mask] = 0
    dm.params[:spec.param_count].copy_(torch.from_numpy(p))
    return spec, dm, p


def _run(torch, model_type, kind, kw, steps=5):
    spec, dm, p = _model(torch, model_type)
    opt = _optimizer(kind, kw)
    ref = _reference(opt)
    segs = list(zip(*spec.optimizer_segments()))
    rng = np.random.default_rng(1)
    pr = p.astype(np.float64)
    for s in range(steps):
        g = _grads(spec, rng, s)
        dm.grads[:spec.param_count].copy_(torch.from_numpy(g))
        dm.optimizer_step(opt)
        ref.step(pr, g, segs)
    torch.cuda.synchronize()
    return spec, dm, ref, pr


@pytest.mark.parametrize("model_type", ["simple_cnn", "simple_gru"])
@pytest.mark.parametrize("kind,kw", COMBOS, ids=["%s-%s" % (k, "-".join(sorted(kw))) for k, kw in COMBOS])
def test_options_match_the_oracle(torch, model_type, kind, kw):
    spec, dm, ref, pr = _run(torch, model_type, kind, kw)
    n = spec.param_count
    np.testing.assert_allclose(dm.params[:n].cpu().numpy(), pr, rtol=1e-5, atol=1e-6)
    assert set(ref.slots) <= set(SLOT_ATTR)
    for name, want in ref.slots.items():
        got = getattr(dm, SLOT_ATTR[name])
        assert got is not None, name
        scale = max(float(np.abs(want).max()), 1e-30)
        np.testing.assert_allclose(got[:n].cpu().numpy(), want, rtol=1e-5, atol=1e-6 * scale, err_msg=name)
    for name in set(SLOT_ATTR) - set(ref.slots) - {"m", "v"}:
        assert getattr(dm, SLOT_ATTR[name]) is None, name             # slots are allocated only when an option needs them
    # clipping did something: the clipped variables moved less than the unclipped update would have
    if kw.get("clipnorm") or kw.get("global_clipnorm"):
        free = RefOptimizer(kind, ref.lr, beta1=ref.beta1, beta2=ref.beta2, eps=ref.eps, momentum=ref.momentum, nesterov=ref.nesterov,
                            centered=ref.centered, amsgrad=ref.amsgrad, clipvalue=ref.clipvalue)
        _, _, p0 = _model(torch, model_type)
        pf = p0.astype(np.float64)
        rng = np.random.default_rng(1)
        segs = list(zip(*spec.optimizer_segments()))
        for s in range(5):
            free.step(pf, _grads(spec, rng, s), segs)
        assert np.abs(pf - pr).max() > 1e-6


@pytest.mark.parametrize("kind,kw", [("adam", dict(amsgrad=True, clipnorm=1.0, clipvalue=0.05)),
                                     ("sgd", dict(momentum=0.9, nesterov=True, global_clipnorm=1.0)),
                                     ("rmsprop", dict(centered=True, momentum=0.9, global_clipnorm=1.0))])
def test_two_runs_are_bit_identical(torch, kind, kw):
    a = _run(torch, "simple_cnn", kind, kw)[1]
    b = _run(torch, "simple_cnn", kind, kw)[1]
    assert torch.equal(a.params, b.params)
    for attr in SLOT_ATTR.values():
        x, y = getattr(a, attr), getattr(b, attr)
        assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), attr


def _inf_case(torch, kw):
    spec, dm, p = _model(torch, "simple_cnn")
    g = _grads(spec, np.random.default_rng(3), 0)
    offsets, sizes = spec.optimizer_segments()
    k = 3
    j = int(offsets[k]) + 5
    g[j] = np.inf
    dm.grads[:spec.param_count].copy_(torch.from_numpy(g))
    opt = _optimizer("sgd", kw)
    dm.optimizer_step(opt)
    return spec, dm, p, g, offsets, sizes, k, j, opt


def test_global_clipnorm_with_an_inf_gives_nan_everywhere(torch):
    spec, dm, *_ = _inf_case(torch, dict(global_clipnorm=1.0))
    assert torch.isnan(dm.params[:spec.param_count]).all()


def test_clipnorm_with_an_inf_touches_only_that_variable(torch):
    spec, dm, p, g, offsets, sizes, k, j, opt = _inf_case(torch, dict(clipnorm=1.0))
    got = dm.params[:spec.param_count].cpu().numpy()
    o, n = int(offsets[k]), int(sizes[k])
    inside = got[o:o + n]
    assert np.isnan(inside[j - o]) and np.isnan(inside).sum() == 1
    np.testing.assert_array_equal(np.delete(inside, j - o), np.delete(p[o:o + n], j - o))   # finite entries clipped to 0
    outside = np.concatenate([got[:o], got[o + n:]])
    assert np.isfinite(outside).all()
    ref = _reference(opt)
    pr = p.astype(np.float64)
    g2 = g.copy()
    g2[o:o + n] = 0
    ref.step(pr, g2, list(zip(offsets, sizes)))
    np.testing.assert_allclose(np.concatenate([got[:o], got[o + n:]]), np.concatenate([pr[:o], pr[o + n:]]), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("model_type", ["simple_cnn", "simple_gru"])
def test_default_options_equal_the_plain_kernels_bit_for_bit(torch, model_type):
    from common import model_utils as mu
    for kind in ("adam", "sgd", "rmsprop"):
        spec, plain, _ = _model(torch, model_type)
        _, new, _ = _model(torch, model_type)
        rng = np.random.default_rng(2)
        opt = {"adam": mu.Adam(1e-3), "sgd": mu.SGD(0.05), "rmsprop": mu.RMSprop(1e-3)}[kind]
        assert not opt.extended
        for s in range(3):
            g = torch.from_numpy(_grads(spec, rng, s))
            plain.grads[:spec.param_count].copy_(g)
            new.grads[:spec.param_count].copy_(g)
            if kind == "adam":
                plain.adam_step(1e-3)
            elif kind == "sgd":
                plain.sgd_step(0.05)
            else:
                plain.rmsprop_step(1e-3)
            new.optimizer_step(opt)
        assert torch.equal(plain.params, new.params), kind
        assert torch.equal(plain.adam_v, new.adam_v) and torch.equal(plain.adam_m, new.adam_m), kind


@pytest.mark.parametrize("make", ["sgd_nesterov_global", "adam_amsgrad_clipnorm"])
def test_fit_with_options_trains_and_pipelined_equals_stepwise(torch, make):
    from classifier.loss import SparseCategoricalCrossEntropy
    from classifier.model import KWSModel
    from common import model_utils as mu
    C, N = 4, 150
    rng = np.random.default_rng(5)
    y = rng.integers(0, C, N)
    protos = rng.standard_normal((C, 30, 20)) * 2
    x = (protos[y] + 0.5 * rng.standard_normal((N, 30, 20))).astype(np.float32)[..., None]
    hist, weights = [], []
    for pipelined in (False, True):
        torch.manual_seed(1234)
        m = KWSModel("simple_cnn", C, seed=3)
        m._device().set_deterministic(True)
        opt = mu.SGD(0.05, momentum=0.9, nesterov=True, global_clipnorm=1.0) if make == "sgd_nesterov_global" else \
            mu.Adam(1e-3, amsgrad=True, clipnorm=1.0)
        m.compile(optimizer=opt, loss=SparseCategoricalCrossEntropy(), metrics=["accuracy"])
        h = m.fit(x, y, batch_size=64, epochs=3, verbose=0, shuffle=True, pipeline=pipelined)
        hist.append((h.history["loss"], h.history["accuracy"]))
        weights.append(m.get_weights())
        dm = m._device()
        assert dm.opt_vhat is not None if make != "sgd_nesterov_global" else dm.opt_mom is not None
    assert hist[0] == hist[1]
    for wa, wb in zip(*weights):
        np.testing.assert_array_equal(wa, wb)
    assert hist[1][0][-1] < hist[1][0][0]
