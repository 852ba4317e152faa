"""CPU tests of the weight-averaging optimizers (common/model_utils.py: MovingAverage, SWA, Lookahead, get_averaged_optimizer): the
per-step schedules against hand-written expectations and the float64 oracle (tests/averaging_ref.py), argument validation, delegation
to the wrapped optimizer, and the host-side argument checks of kws_optimizer_step / kws_optimizer_swap."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import averaging_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf-keras-speech-commands_amd")
f32 = lambda x: float(np.float32(x))


def test_ema_schedule_at_the_reference_constants():
    from common import model_utils as mu
    opt = mu.get_averaged_optimizer("ema", mu.Adam(1e-3))
    assert isinstance(opt, mu.MovingAverage) and opt.average_decay == 0.99 and opt.start_step == 0
    for k in range(41):
        assert opt.average_args(k) == (mu.AVG_BLEND, f32(0.01))
        assert opt.average_args(k) == ar.ema_args(k)


def test_swa_schedule_at_the_reference_constants():
    from common import model_utils as mu
    opt = mu.get_averaged_optimizer("swa", mu.Adam(1e-3))
    assert isinstance(opt, mu.SWA) and opt.start_averaging == 0 and opt.average_period == 10
    snapshots = {0: 1.0, 10: 1.0 / 2, 20: 1.0 / 3, 30: 1.0 / 4, 40: 1.0 / 5}
    for k in range(41):
        want = (mu.AVG_BLEND, f32(snapshots[k])) if k in snapshots else (mu.AVG_NONE, 0.0)
        assert opt.average_args(k) == want, k
        assert opt.average_args(k) == ar.swa_args(k)


def test_lookahead_schedule_at_the_reference_constants():
    from common import model_utils as mu
    opt = mu.get_averaged_optimizer("lookahead", mu.Adam(1e-3))
    assert isinstance(opt, mu.Lookahead) and opt.sync_period == 6 and opt.slow_step_size == 0.5
    sync = {5, 11, 17, 23, 29, 35}
    for k in range(41):
        want = (mu.AVG_SYNC, 0.5) if k in sync else (mu.AVG_NONE, 0.0)
        assert opt.average_args(k) == want, k
        assert opt.average_args(k) == ar.lookahead_args(k)


def test_start_values_shift_the_schedules():
    from common import model_utils as mu
    ema = mu.MovingAverage(mu.SGD(0.1), average_decay=0.9, start_step=3)
    assert [ema.average_args(k) for k in range(5)] == [(1, 1.0)] * 3 + [(1, f32(1.0 - 0.9))] * 2
    swa = mu.SWA(mu.SGD(0.1), start_averaging=2, average_period=3)
    got = [swa.average_args(k) for k in range(9)]
    assert got == [(0, 0.0), (0, 0.0), (1, 1.0), (0, 0.0), (0, 0.0), (1, 0.5), (0, 0.0), (0, 0.0), (1, f32(1.0 / 3))]
    la = mu.Lookahead(mu.SGD(0.1), sync_period=3, slow_step_size=0.25)
    assert [la.average_args(k)[0] for k in range(7)] == [0, 0, 2, 0, 0, 2, 0] and la.average_args(2)[1] == 0.25
    for k in range(30):
        assert ema.average_args(k) == ar.ema_args(k, 0.9, 3)
        assert swa.average_args(k) == ar.swa_args(k, 2, 3)
        assert la.average_args(k) == ar.lookahead_args(k, 3, 0.25)
    assert mu.Lookahead(mu.SGD(0.1), sync_period=1).average_args(0)[0] == mu.AVG_SYNC     # period 1: every update syncs
    assert (mu.AVG_NONE, mu.AVG_BLEND, mu.AVG_SYNC) == (ar.NONE, ar.BLEND, ar.SYNC)


@pytest.mark.parametrize("make", [
    lambda mu, o: mu.MovingAverage(o, average_decay=1.5), lambda mu, o: mu.MovingAverage(o, average_decay=-0.1),
    lambda mu, o: mu.MovingAverage(o, average_decay=float("nan")), lambda mu, o: mu.MovingAverage(o, start_step=-1),
    lambda mu, o: mu.SWA(o, start_averaging=-1), lambda mu, o: mu.SWA(o, average_period=0),
    lambda mu, o: mu.Lookahead(o, sync_period=0), lambda mu, o: mu.Lookahead(o, slow_step_size=1.01),
    lambda mu, o: mu.Lookahead(o, slow_step_size=-0.5)])
def test_arguments_are_validated(make):
    from common import model_utils as mu
    with pytest.raises(ValueError):
        make(mu, mu.Adam(1e-3))


def test_the_bounds_themselves_are_accepted():
    from common import model_utils as mu
    o = mu.Adam(1e-3)
    assert mu.MovingAverage(o, average_decay=0.0).average_args(0) == (1, 1.0)
    assert mu.MovingAverage(o, average_decay=1.0).average_args(0) == (1, 0.0)
    assert mu.Lookahead(o, sync_period=1, slow_step_size=1.0).average_args(0) == (2, 1.0)
    assert mu.Lookahead(o, sync_period=1, slow_step_size=0.0).average_args(0) == (2, 0.0)


def test_get_averaged_optimizer_names_none_and_error():
    from common import model_utils as mu
    o = mu.Adam(1e-3)
    assert mu.get_averaged_optimizer(None, o) is o
    for name, cls in (("ema", mu.MovingAverage), ("EMA", mu.MovingAverage), ("Swa", mu.SWA), ("LookAhead", mu.Lookahead)):
        w = mu.get_averaged_optimizer(name, o)
        assert type(w) is cls and w.optimizer is o
    for bad in ("polyak", "", 3):
        with pytest.raises(ValueError, match="Unsupported average type"):
            mu.get_averaged_optimizer(bad, o)
    # the factory itself keeps refusing: the reference's train.py passes average_type=None and wraps afterwards
    with pytest.raises(ValueError, match="Unsupported average type"):
        mu.get_optimizer("adam", 1e-3, average_type="swa", decay_type=None)


def test_wrappers_delegate_to_the_wrapped_optimizer():
    from common import model_utils as mu
    inner = mu.SGD(0.05, momentum=0.9, nesterov=True, global_clipnorm=1.5, clipvalue=0.25)
    for w in (mu.MovingAverage(inner), mu.SWA(inner), mu.Lookahead(inner)):
        assert isinstance(w, mu.Optimizer) and w.extended
        assert w.kind == "sgd" and w.momentum == 0.9 and w.nesterov
        assert (w.clipnorm, w.clipvalue, w.global_clipnorm) == (None, 0.25, 1.5)
        assert w.lr == 0.05 and w.current_lr() == 0.05
    w = mu.MovingAverage(inner)
    w.set_lr(0.01)
    assert inner.current_lr() == 0.01 and w.lr == 0.01
    w.iterations += 1
    assert inner.iterations == 1 and w.iterations == 1
    sched = mu.Adam(mu.ExponentialDecay(1e-3, 10, 0.5), amsgrad=True)
    w = mu.SWA(sched)
    assert w.kind == "adam" and w.amsgrad and (w.beta_1, w.beta_2, w.epsilon) == (0.9, 0.999, 1e-7)
    sched.iterations = 10
    assert w.current_lr() == pytest.approx(5e-4)
    with pytest.raises(TypeError):
        w.set_lr(1.0)                                   # a schedule cannot be set, through the wrapper either
    assert mu.MovingAverage(mu.Adam(1e-3)).extended     # a default Adam under a wrapper runs kws_optimizer_step
    with pytest.raises(AttributeError):
        w.no_such_option


def test_wrapping_a_wrapper_or_a_stranger_raises():
    from common import model_utils as mu
    for cls in (mu.MovingAverage, mu.SWA, mu.Lookahead):
        with pytest.raises(TypeError):
            cls(mu.SWA(mu.Adam(1e-3)))
        with pytest.raises(TypeError):
            cls("adam")


def test_compile_accepts_a_wrapper_and_lookahead_has_no_average_to_assign():
    from classifier.loss import SparseCategoricalCrossEntropy
    from classifier.model import KWSModel
    from common import model_utils as mu
    m = KWSModel("simple_cnn_lite", 4, seed=0)
    m.compile(optimizer=mu.Lookahead(mu.Adam(1e-3)), loss=SparseCategoricalCrossEntropy())
    with pytest.raises(TypeError):
        m.optimizer.assign_average_vars(m)
    with pytest.raises(TypeError):
        with m.averaged_weights():
            pass
    m.compile(optimizer=mu.Adam(1e-3), loss=SparseCategoricalCrossEntropy())
    with pytest.raises(TypeError):
        with m.averaged_weights():
            pass
    # no step has run: the averages are the weights, and neither call needs the device
    m.compile(optimizer=mu.MovingAverage(mu.Adam(1e-3)), loss=SparseCategoricalCrossEntropy())
    before = m.get_weights()
    with m.averaged_weights():
        inside = m.get_weights()
    m.optimizer.assign_average_vars(m)
    for a, b, c in zip(before, inside, m.get_weights()):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)


def test_average_model_checkpoint_wants_an_averaging_optimizer():
    from classifier.loss import SparseCategoricalCrossEntropy
    from classifier.model import KWSModel
    from common import callbacks as cb
    from common import model_utils as mu
    assert issubclass(cb.AverageModelCheckpoint, cb.ModelCheckpoint)
    ck = cb.AverageModelCheckpoint(False, "x.npz", monitor="val_accuracy", mode="max", save_best_only=True)
    assert ck.update_weights is False and ck.monitor == "val_accuracy" and ck.save_best_only
    m = KWSModel("simple_cnn_lite", 4, seed=0)
    for opt in (mu.Adam(1e-3), mu.Lookahead(mu.Adam(1e-3))):
        m.compile(optimizer=opt, loss=SparseCategoricalCrossEntropy())
        with pytest.raises(TypeError):
            ck.set_model(m)
    m.compile(optimizer=mu.SWA(mu.Adam(1e-3)), loss=SparseCategoricalCrossEntropy())
    ck.set_model(m)


def test_train_flag_wraps_the_optimizer():
    spec = importlib.util.spec_from_file_location("kws_train_main_avg", os.path.join(PKG, "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    base = ["--train_data_path", "d", "--classes_path", "c.txt"]
    assert train.parse_args(base).average_type is None
    for name in ("ema", "swa", "lookahead"):
        assert train.parse_args(base + ["--average_type", name]).average_type == name
    with pytest.raises(SystemExit):
        train.parse_args(base + ["--average_type", "polyak"])


def test_oracle_formulas_by_hand():
    p = np.array([1.0, 2.0, 3.0, 4.0, 9.0, 9.0, 9.0, 9.0, 5.0])
    avg = np.array([0.0, 0.0, 1.0, 4.0, 7.0, 7.0, 7.0, 7.0, 1.0])
    segs = [(0, 3), (8, 1)]
    ar.apply(ar.BLEND, 0.25, p, avg, segs)
    np.testing.assert_allclose(avg, [0.25, 0.5, 1.5, 4.0, 7.0, 7.0, 7.0, 7.0, 2.0], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(p, [1.0, 2.0, 3.0, 4.0, 9.0, 9.0, 9.0, 9.0, 5.0])
    ar.apply(ar.SYNC, 0.5, p, avg, segs)
    np.testing.assert_allclose(avg, [0.625, 1.25, 2.25, 4.0, 7.0, 7.0, 7.0, 7.0, 3.5], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(p[[0, 1, 2, 8]], avg[[0, 1, 2, 8]])
    np.testing.assert_array_equal(p[3:8], [4.0, 9.0, 9.0, 9.0, 9.0])
    a2 = avg.copy()
    ar.apply(ar.BLEND, 1.0, p + 1.0, a2, segs)               # alpha 1: the slot becomes the parameter
    np.testing.assert_array_equal(a2[[0, 1, 2, 8]], (p + 1.0)[[0, 1, 2, 8]])
    ar.apply(ar.NONE, 0.5, p, a2, segs)
    # three SWA snapshots give their mean
    snaps = [np.array([1.0, 5.0]), np.array([2.0, -1.0]), np.array([6.0, 2.0])]
    mean = np.array([100.0, 100.0])
    for n, s in enumerate(snaps):
        ar.apply(*ar.swa_args(n * 10), s, mean, [(0, 2)])
    np.testing.assert_allclose(mean, np.mean(snaps, axis=0), rtol=1e-7)


def _aligned(a):
    """the first 16-byte aligned address inside the array (they are allocated with room to spare)"""
    return (a.ctypes.data + 15) & ~15


def _step_args(l, **over):
    L = l.get_lib()
    o = np.array([0], np.int64)
    s = np.array([8], np.int64)
    po, ps = (a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)) for a in (o, s))
    nbytes = L.kws_optimizer_workspace_bytes(po, ps, 1)
    ws = np.zeros((nbytes + 16,), np.uint8)
    nb = ctypes.c_int32()
    assert L.kws_optimizer_plan(po, ps, 1, ws.ctypes.data, nbytes, ctypes.byref(nb)) == 0
    buf = [np.zeros((12,), np.float32) for _ in range(3)]
    kw = dict(kind=l.OPT_KINDS["sgd"], params=buf[0].ctypes.data, grads=buf[1].ctypes.data, ws=ws.ctypes.data, ws_bytes=nbytes,
              n_blocks=nb.value, lr=1e-2, grad_scale=1.0)
    kw.update(over)
    return L, l.KwsOptimizerArgs(**kw), (ws, buf, nbytes, nb.value)


def test_step_rejects_bad_averaging_arguments_before_any_launch():
    from kws_amd import lib as l
    assert (l.AVG_NONE, l.AVG_BLEND, l.AVG_SYNC) == (0, 1, 2)
    assert [n for n, _ in l.KwsOptimizerArgs._fields_][-4:] == ["global_clipnorm", "avg", "avg_mode", "avg_alpha"]
    L, a, keep = _step_args(l)
    avg = _aligned(keep[1][2])
    for mode in (3, -1, 7):
        L, a, keep = _step_args(l, avg=avg, avg_mode=mode, avg_alpha=0.5)
        assert L.kws_optimizer_step(ctypes.byref(a), None) == l.ERR_INVALID and b"averaging mode" in L.kws_last_error()
    for mode in (l.AVG_BLEND, l.AVG_SYNC):
        L, a, keep = _step_args(l, avg=None, avg_mode=mode, avg_alpha=0.5)
        assert L.kws_optimizer_step(ctypes.byref(a), None) == l.ERR_INVALID and b"NULL" in L.kws_last_error()
        L, a, keep = _step_args(l, avg=avg + 4, avg_mode=mode, avg_alpha=0.5)
        assert L.kws_optimizer_step(ctypes.byref(a), None) == l.ERR_INVALID and b"aligned" in L.kws_last_error()
        for alpha in (-0.01, 1.01, float("nan"), float("inf")):
            L, a, keep = _step_args(l, avg=avg, avg_mode=mode, avg_alpha=alpha)
            assert L.kws_optimizer_step(ctypes.byref(a), None) == l.ERR_INVALID and b"avg_alpha" in L.kws_last_error()
    # the checks hold with an empty block table too, where no launch would follow
    L, a, keep = _step_args(l, avg=None, avg_mode=l.AVG_BLEND, avg_alpha=0.5, n_blocks=0)
    assert L.kws_optimizer_step(ctypes.byref(a), None) == l.ERR_INVALID


def test_swap_rejects_bad_arguments_before_any_launch():
    from kws_amd import lib as l
    L, a, (ws, buf, nbytes, nb) = _step_args(l)
    p, avg, w = _aligned(buf[0]), _aligned(buf[2]), _aligned(ws)
    assert L.kws_optimizer_swap(None, avg, w, nbytes, nb, None) == l.ERR_INVALID
    assert L.kws_optimizer_swap(p, None, w, nbytes, nb, None) == l.ERR_INVALID
    assert L.kws_optimizer_swap(p, avg, None, nbytes, nb, None) == l.ERR_INVALID
    assert L.kws_optimizer_swap(p, p, w, nbytes, nb, None) == l.ERR_INVALID
    assert L.kws_optimizer_swap(p, avg + 4, w, nbytes, nb, None) == l.ERR_INVALID and b"aligned" in L.kws_last_error()
    assert L.kws_optimizer_swap(p, avg, w, nbytes, -1, None) == l.ERR_INVALID
    assert L.kws_optimizer_swap(p, avg, w, nbytes - 1, nb, None) == l.ERR_WORKSPACE
    assert L.kws_optimizer_swap(p, avg, w, nbytes, 0, None) == 0              # nothing to exchange
