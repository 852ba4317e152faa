"""GPU tests of the weight averaging folded into kws_optimizer_step (include/kws.h KWS_AVG_*) and of kws_optimizer_swap: MovingAverage,
SWA and Lookahead over Adam / SGD / RMSprop against the float64 oracles (tests/optim_ref.py, tests/averaging_ref.py) on the real tensor
tables of simple_cnn and simple_gru, bit identity of the training weights with and without averaging, block and tail geometry through
the raw C ABI, the swap, run-to-run bit identity, and a small model trained end to end with averaged validation and checkpoints."""
import ctypes

import numpy as np
import pytest

import averaging_ref as ar
from optim_ref import RefOptimizer

pytestmark = pytest.mark.gpu

STEPS = 8
LR = {"sgd": 0.05, "rmsprop": 1e-3, "adam": 1e-3}
SLOT_ATTR = {"m": "adam_m", "v": "adam_v", "vhat": "opt_vhat", "mg": "opt_mg", "mom": "opt_mom"}
INNER = {"adam": ("adam", {}), "sgd_momentum_global": ("sgd", dict(momentum=0.9, global_clipnorm=1.0)),
         "rmsprop_centered": ("rmsprop", dict(centered=True))}
# short periods, so that 8 steps pass through every branch of every schedule
WRAPPERS = {"ema": dict(average_decay=0.99, start_step=2), "swa": dict(start_averaging=2, average_period=3),
            "lookahead": dict(sync_period=3, slow_step_size=0.5)}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _inner(name):
    from common import model_utils as mu
    kind, kw = INNER[name]
    return {"sgd": mu.SGD, "rmsprop": mu.RMSprop, "adam": mu.Adam}[kind](LR[kind], **kw)


def _wrap(wrapper, opt):
    from common import model_utils as mu
    if wrapper is None:
        return opt
    return {"ema": mu.MovingAverage, "swa": mu.SWA, "lookahead": mu.Lookahead}[wrapper](opt, **WRAPPERS[wrapper])


def _reference(opt):
    """the oracle with the hyperparameters the kernel sees, rounded to float32 (as tests/test_optim_gpu.py)"""
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


_CACHE = {}


def _inputs(model_type):
    """(spec, initial params, the 8 gradients): drawn once per model and shared, never written"""
    if model_type not in _CACHE:
        from kws_amd.model import ModelSpec
        spec = ModelSpec(model_type, 36, 30, 20)
        p = (0.1 * np.random.default_rng(0).standard_normal(spec.param_count)).astype(np.float32)
        mask = np.zeros_like(p, bool)                # the padding between tensors stays zero
        for t in spec.tensors:
            if t["trainable"]:
                mask[t["offset"]:t["offset"] + t["size"]] = True
        p[~mask] = 0
        rng = np.random.default_rng(1)
        grads = [_grads(spec, rng, s) for s in range(STEPS)]
        _CACHE[model_type] = (spec, p, grads)
    return _CACHE[model_type]


def _run_device(torch, model_type, opt, plain_adam=False):
    """8 steps on the device; the caller of DeviceModel.optimizer_step counts the updates (as KWSModel does)"""
    from kws_amd.model import DeviceModel
    spec, p, grads = _inputs(model_type)
    dm = DeviceModel(spec)
    dm.params[:spec.param_count].copy_(torch.from_numpy(p))
    for g in grads:
        dm.grads[:spec.param_count].copy_(torch.from_numpy(g))
        if plain_adam:
            dm.adam_step(opt.current_lr(), opt.beta_1, opt.beta_2, opt.epsilon)
        else:
            dm.optimizer_step(opt)
        opt.iterations += 1
    torch.cuda.synchronize()
    return dm


def _run_oracle(model_type, wrapper, opt):
    spec, p, grads = _inputs(model_type)
    ref = _reference(opt)
    segs = list(zip(*spec.optimizer_segments()))
    pr, avg = p.astype(np.float64), p.astype(np.float64)          # every wrapper starts its slot at the variable's value
    modes = []
    for k, g in enumerate(grads):
        ref.step(pr, g, segs)
        mode, alpha = ar.SCHEDULES[wrapper](k, *WRAPPERS[wrapper].values())
        ar.apply(mode, alpha, pr, avg, segs)
        modes.append((mode, alpha))
    return ref, pr, avg, modes


def test_the_short_periods_pass_through_every_branch():
    sched = lambda w: [ar.SCHEDULES[w](k, *WRAPPERS[w].values()) for k in range(STEPS)]
    f = lambda x: float(np.float32(x))
    assert sched("ema") == [(1, 1.0)] * 2 + [(1, f(1.0 - 0.99))] * 6
    assert sched("swa") == [(0, 0.0), (0, 0.0), (1, 1.0), (0, 0.0), (0, 0.0), (1, 0.5), (0, 0.0), (0, 0.0)]
    assert sched("lookahead") == [(0, 0.0), (0, 0.0), (2, 0.5), (0, 0.0), (0, 0.0), (2, 0.5), (0, 0.0), (0, 0.0)]


@pytest.mark.parametrize("model_type", ["simple_cnn", "simple_gru"])
@pytest.mark.parametrize("inner", list(INNER))
@pytest.mark.parametrize("wrapper", list(WRAPPERS))
def test_wrappers_match_the_oracle(torch, model_type, inner, wrapper):
    opt = _wrap(wrapper, _inner(inner))
    dm = _run_device(torch, model_type, opt)
    ref, pr, avg, modes = _run_oracle(model_type, wrapper, opt.optimizer)
    assert modes == [opt.average_args(k) for k in range(STEPS)]
    n = dm.spec.param_count
    got_p, got_avg = dm.params[:n].cpu().numpy(), dm.opt_avg[:n].cpu().numpy()
    print("%s %s %s: max|params - oracle| %.3g, max|avg - oracle| %.3g" % (model_type, inner, wrapper, np.abs(got_p - pr).max(),
                                                                            np.abs(got_avg - avg).max()))
    np.testing.assert_allclose(got_p, pr, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got_avg, avg, rtol=1e-5, atol=1e-6 * float(np.abs(avg).max()), err_msg="opt_avg")
    for name, want in ref.slots.items():
        got = getattr(dm, SLOT_ATTR[name])
        assert got is not None, name
        scale = max(float(np.abs(want).max()), 1e-30)
        np.testing.assert_allclose(got[:n].cpu().numpy(), want, rtol=1e-5, atol=1e-6 * scale, err_msg=name)
    # the averaging did something: the slot is neither the start nor the weights
    assert np.abs(got_avg - _inputs(model_type)[1]).max() > 1e-4 and np.abs(got_avg - got_p).max() > 1e-5
    assert dm.opt_avg.data_ptr() % 16 == 0 and dm.opt_avg.numel() == dm.params.numel()


@pytest.mark.parametrize("inner", list(INNER))
@pytest.mark.parametrize("wrapper", ["ema", "swa"])
def test_averaging_does_not_disturb_training(torch, inner, wrapper):
    plain = _run_device(torch, "simple_cnn", _inner(inner))
    wrapped = _run_device(torch, "simple_cnn", _wrap(wrapper, _inner(inner)))
    assert plain.opt_avg is None and wrapped.opt_avg is not None
    assert torch.equal(plain.params, wrapped.params)
    for attr in SLOT_ATTR.values():
        x, y = getattr(plain, attr), getattr(wrapped, attr)
        assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), attr
    if inner == "adam":
        base = _inner(inner)
        assert not base.extended
        fused = _run_device(torch, "simple_cnn", base, plain_adam=True)
        assert torch.equal(fused.params, wrapped.params)
        assert torch.equal(fused.adam_m, wrapped.adam_m) and torch.equal(fused.adam_v, wrapped.adam_v)


@pytest.mark.parametrize("wrapper", list(WRAPPERS))
def test_two_runs_are_bit_identical(torch, wrapper):
    inner = {"ema": "adam", "swa": "sgd_momentum_global", "lookahead": "rmsprop_centered"}[wrapper]
    a = _run_device(torch, "simple_cnn", _wrap(wrapper, _inner(inner)))
    b = _run_device(torch, "simple_cnn", _wrap(wrapper, _inner(inner)))
    assert torch.equal(a.params, b.params) and torch.equal(a.opt_avg, b.opt_avg)
    for attr in SLOT_ATTR.values():
        x, y = getattr(a, attr), getattr(b, attr)
        assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), attr


# ---- block and tail geometry through the raw C ABI ---------------------------------------------------------------------------------
# one float; a float4 and a scalar; exactly one block; one block and one element; two blocks and a tail of 3 -- with padding between
SEG_SIZES = [1, 5, 1024, 1025, 2051]
SEG_OFFSETS = [4, 12, 24, 1052, 2084]
TOTAL = 4140
SENTINEL = 777.25


class _Raw(object):
    """flat device buffers over the hand-made table, driven through the ctypes bindings alone"""

    def __init__(self, torch):
        from kws_amd import lib as l
        self.l, self.L, self.torch = l, l.get_lib(), torch
        o, s = np.asarray(SEG_OFFSETS, np.int64), np.asarray(SEG_SIZES, np.int64)
        po, ps = (a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) for a in (o, s))
        self.ws_bytes = int(self.L.kws_optimizer_workspace_bytes(po, ps, len(o)))
        assert self.ws_bytes > 0
        host = np.zeros((self.ws_bytes,), np.uint8)
        nb = ctypes.c_int32()
        l.check(self.L.kws_optimizer_plan(po, ps, len(o), host.ctypes.data, self.ws_bytes, ctypes.byref(nb)))
        self.n_blocks = int(nb.value)
        assert self.n_blocks == 1 + 1 + 1 + 2 + 3
        self.ws = torch.from_numpy(host).cuda()
        self.segs = list(zip(SEG_OFFSETS, SEG_SIZES))
        self.inside = np.zeros((TOTAL,), bool)
        for o_, n_ in self.segs:
            self.inside[o_:o_ + n_] = True
        assert self.inside.sum() == sum(SEG_SIZES) and not self.inside[-1] and not self.inside[0]
        rng = np.random.default_rng(7)
        self.p0 = np.where(self.inside, rng.standard_normal(TOTAL), SENTINEL).astype(np.float32)
        self.a0 = np.where(self.inside, rng.standard_normal(TOTAL), SENTINEL).astype(np.float32)
        self.g = [np.where(self.inside, 0.1 * rng.standard_normal(TOTAL), np.nan).astype(np.float32) for _ in range(2)]
        self.p, self.avg = torch.from_numpy(self.p0).cuda(), torch.from_numpy(self.a0).cuda()
        self.grad = torch.zeros_like(self.p)
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.stream = torch.cuda.current_stream().cuda_stream

    def step(self, t, g, avg, mode, alpha):
        l = self.l
        self.grad.copy_(self.torch.from_numpy(g))
        a = l.KwsOptimizerArgs(kind=l.OPT_KINDS["adam"], params=self.p.data_ptr(), grads=self.grad.data_ptr(), m=self.m.data_ptr(),
                               v=self.v.data_ptr(), ws=self.ws.data_ptr(), ws_bytes=self.ws_bytes, n_blocks=self.n_blocks, lr=1e-2,
                               beta1=0.9, beta2=0.999, eps=1e-7, t=t, grad_scale=1.0, avg=avg.data_ptr(), avg_mode=mode, avg_alpha=alpha)
        l.check(self.L.kws_optimizer_step(ctypes.byref(a), self.stream))

    def swap(self):
        self.l.check(self.L.kws_optimizer_swap(self.p.data_ptr(), self.avg.data_ptr(), self.ws.data_ptr(), self.ws_bytes, self.n_blocks,
                                               self.stream))


def test_block_and_tail_geometry_blend_then_sync(torch):
    r = _Raw(torch)
    f = lambda x: float(np.float32(x))
    ref = RefOptimizer("adam", f(1e-2), beta1=f(0.9), beta2=f(0.999), eps=f(1e-7))
    pr, avg = r.p0.astype(np.float64), r.a0.astype(np.float64)
    for t, (mode, alpha) in enumerate([(ar.BLEND, f(0.3)), (ar.SYNC, f(0.5))]):
        r.step(t + 1, r.g[t], r.avg, mode, alpha)
        g = np.where(r.inside, r.g[t], 0.0)
        ref.step(pr, g, r.segs)
        ar.apply(mode, alpha, pr, avg, r.segs)
        got_p, got_a = r.p.cpu().numpy(), r.avg.cpu().numpy()
        ins = r.inside
        np.testing.assert_allclose(got_p[ins], pr[ins], rtol=1e-5, atol=1e-6, err_msg="params, step %d" % t)
        np.testing.assert_allclose(got_a[ins], avg[ins], rtol=1e-5, atol=1e-6 * float(np.abs(avg[ins]).max()), err_msg="avg, step %d" % t)
        assert (got_p[~ins] == np.float32(SENTINEL)).all() and (got_a[~ins] == np.float32(SENTINEL)).all()   # padding untouched
        if mode == ar.BLEND:
            assert not np.array_equal(got_p[ins], got_a[ins])
        else:
            np.testing.assert_array_equal(got_p[ins], got_a[ins])          # the fast weights restart at the slow ones
    assert np.isfinite(r.m.cpu().numpy()[r.inside]).all() and (r.m.cpu().numpy()[~r.inside] == 0).all()


def test_mode_none_never_touches_the_slot(torch):
    r = _Raw(torch)
    slot = torch.full_like(r.p, SENTINEL)
    r.step(1, r.g[0], slot, ar.NONE, 0.5)
    torch.cuda.synchronize()
    assert bool((slot == SENTINEL).all())
    moved = r.p.cpu().numpy()
    assert (moved[r.inside] != r.p0[r.inside]).all() and (moved[~r.inside] == np.float32(SENTINEL)).all()
    # and the slot's content does not reach the parameters: the same step without a slot gives the same bits
    q = _Raw(torch)
    q.step(1, q.g[0], torch.zeros_like(q.p), ar.NONE, 0.0)
    assert torch.equal(q.p, r.p)


def test_swap_exchanges_inside_the_segments_and_twice_restores_every_bit(torch):
    r = _Raw(torch)
    r.a0[~r.inside] = -SENTINEL                    # different padding in the two buffers: an exchange there would show
    r.avg.copy_(torch.from_numpy(r.a0))
    r.swap()
    p1, a1 = r.p.cpu().numpy(), r.avg.cpu().numpy()
    ins = r.inside
    np.testing.assert_array_equal(p1[ins], r.a0[ins])
    np.testing.assert_array_equal(a1[ins], r.p0[ins])
    assert (p1[~ins] == np.float32(SENTINEL)).all() and (a1[~ins] == np.float32(-SENTINEL)).all()
    r.swap()
    assert r.p.cpu().numpy().tobytes() == r.p0.tobytes() and r.avg.cpu().numpy().tobytes() == r.a0.tobytes()


def test_device_model_swap_average(torch):
    from kws_amd.model import DeviceModel
    spec, p, grads = _inputs("simple_gru")
    dm = DeviceModel(spec)
    dm.params[:spec.param_count].copy_(torch.from_numpy(p))
    with pytest.raises(RuntimeError):
        dm.swap_average()                          # no averaging slot yet
    opt = _wrap("ema", _inner("adam"))
    for g in grads[:4]:
        dm.grads[:spec.param_count].copy_(torch.from_numpy(g))
        dm.optimizer_step(opt)
        opt.iterations += 1
    p0, a0, version = dm.params.clone(), dm.opt_avg.clone(), dm.weights_version
    assert not torch.equal(p0, a0)
    dm.swap_average()
    assert torch.equal(dm.params, a0) and torch.equal(dm.opt_avg, p0) and dm.weights_version > version
    dm.swap_average()
    assert torch.equal(dm.params, p0) and torch.equal(dm.opt_avg, a0)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def _toy(C=4, N=24, seed=5):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, C, N)
    protos = rng.standard_normal((C, 30, 20)) * 2
    x = (protos[y] + 0.5 * rng.standard_normal((N, 30, 20))).astype(np.float32)[..., None]
    return x, y


def test_train_on_batch_under_moving_average_end_to_end(torch):
    from classifier.loss import SparseCategoricalCrossEntropy
    from classifier.model import KWSModel
    from common import model_utils as mu
    x, y = _toy()
    m = KWSModel("simple_cnn_lite", 4, seed=3)
    decay = 0.9
    opt = mu.MovingAverage(mu.Adam(1e-2), average_decay=decay)
    m.compile(optimizer=opt, loss=SparseCategoricalCrossEntropy(), metrics=["accuracy"])
    trainable = [t["trainable"] for t in m.spec.tensors]
    assert any(trainable) and not all(trainable)            # the model has BatchNormalization moving statistics
    ema = [w.astype(np.float64) for w in m.get_weights()]
    alpha = np.float64(np.float32(1.0 - decay))
    for s in range(7):
        m.train_on_batch(x[8 * (s % 3):8 * (s % 3) + 8], y[8 * (s % 3):8 * (s % 3) + 8])
        for e, w, tr in zip(ema, m.get_weights(), trainable):
            if tr:
                e -= (e - w.astype(np.float64)) * alpha
    assert opt.iterations == 7
    outside = m.get_weights()
    pred_outside = m.predict(x)
    with m.averaged_weights():
        inside = m.get_weights()
        pred_inside = m.predict(x)
    for e, wi, wo, tr, t in zip(ema, inside, outside, trainable, m.spec.tensors):
        if tr:
            np.testing.assert_allclose(wi, e, rtol=1e-5, atol=1e-6 * float(np.abs(e).max()), err_msg=t["name"])
        else:
            np.testing.assert_array_equal(wi, wo, err_msg=t["name"])     # moving statistics are not averaged
    assert np.abs(pred_inside - pred_outside).max() > 1e-4
    for wa, wb in zip(m.get_weights(), outside):
        assert wa.tobytes() == wb.tobytes()                              # the training weights are back, bit for bit
    np.testing.assert_array_equal(m.predict(x), pred_outside)


def test_fit_validates_and_checkpoints_the_averages(torch, tmp_path):
    from classifier.loss import SparseCategoricalCrossEntropy
    from classifier.model import KWSModel
    from common import model_utils as mu
    from common.callbacks import AverageModelCheckpoint
    x, y = _toy()
    m = KWSModel("simple_cnn_lite", 4, seed=3)
    opt = mu.MovingAverage(mu.Adam(1e-2), average_decay=0.9)
    m.compile(optimizer=opt, loss=SparseCategoricalCrossEntropy(), metrics=["accuracy"])
    ck = AverageModelCheckpoint(False, str(tmp_path / "ep{epoch:02d}.npz"), monitor="val_accuracy", mode="max", save_best_only=False)
    h = m.fit(x, y, batch_size=8, epochs=2, verbose=0, shuffle=True, validation_data=(x, y), callbacks=[ck], validate_averaged=True)
    assert opt.iterations == 6 and sorted(p.name for p in tmp_path.iterdir()) == ["ep01.npz", "ep02.npz"]
    own = m.get_weights()
    with m.averaged_weights():
        avg = m.get_weights()
        val_avg = m.evaluate(x, y, batch_size=8)
    val_own = m.evaluate(x, y, batch_size=8)
    assert [h.history["val_loss"][-1], h.history["val_accuracy"][-1]] == val_avg      # the weights that get saved were the ones validated
    assert val_own[0] != val_avg[0]
    z = np.load(str(tmp_path / "ep02.npz"))
    for t, wa, wo in zip(m.spec.tensors, avg, own):
        np.testing.assert_array_equal(z[t["name"]], wa, err_msg=t["name"])
        if t["trainable"] and t["size"] > 8:
            assert not np.array_equal(wa, wo), t["name"]
    for wa, wb in zip(m.get_weights(), own):
        assert wa.tobytes() == wb.tobytes()                                           # the model kept its own weights
    # update_weights=True assigns first: the model then holds what the file holds
    ck2 = AverageModelCheckpoint(True, str(tmp_path / "assigned.npz"), save_best_only=False)
    ck2.set_model(m)
    ck2.on_epoch_end(0, {})
    z2 = np.load(str(tmp_path / "assigned.npz"))
    for t, wa, wm in zip(m.spec.tensors, avg, m.get_weights()):
        np.testing.assert_array_equal(z2[t["name"]], wa, err_msg=t["name"])
        np.testing.assert_array_equal(wm, wa, err_msg=t["name"])


def test_lookahead_trains_but_has_no_average_to_evaluate(torch):
    from classifier.loss import SparseCategoricalCrossEntropy
    from classifier.model import KWSModel
    from common import model_utils as mu
    x, y = _toy()
    m = KWSModel("simple_cnn_lite", 4, seed=3)
    m.compile(optimizer=mu.Lookahead(mu.Adam(1e-2), sync_period=2), loss=SparseCategoricalCrossEntropy(), metrics=["accuracy"])
    for s in range(2):
        m.train_on_batch(x[:8], y[:8])
    dm = m._device()
    assert torch.equal(dm.params, dm.opt_avg)               # the second update synchronised fast and slow weights
    with pytest.raises(TypeError):
        with m.averaged_weights():
            pass
    with pytest.raises(TypeError):
        m.optimizer.assign_average_vars(m)
