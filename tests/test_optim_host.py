"""CPU tests of the optimizer options (clipping, momentum / nesterov, centered, amsgrad): constructors and their validation,
get_optimizer and train.py forwarding them, the host-only planning entry points of kws_optimizer_step, and the float64 oracle
(tests/optim_ref.py) on hand-computed cases."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from optim_ref import RefOptimizer, clip_by_global_norm, clip_by_norm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf-keras-speech-commands_amd")


def test_every_keras_option_is_accepted_and_exposed():
    from common import model_utils as mu
    a = mu.Adam(1e-3, amsgrad=True, clipnorm=1.0, clipvalue=0.5)
    assert a.amsgrad and a.clipnorm == 1.0 and a.clipvalue == 0.5 and a.global_clipnorm is None and a.extended
    r = mu.RMSprop(1e-3, momentum=0.9, centered=True, global_clipnorm=2.0, clipvalue=3.0)
    assert r.momentum == 0.9 and r.centered and r.global_clipnorm == 2.0 and r.clipvalue == 3.0 and r.extended
    s = mu.SGD(0.1, momentum=0.9, nesterov=True, clipnorm=1.0)
    assert s.momentum == 0.9 and s.nesterov and s.clipnorm == 1.0 and s.extended
    # 0 / None is "off": the reference's optimizers keep the plain kernels
    for o in (mu.Adam(clipnorm=0), mu.Adam(clipvalue=None, global_clipnorm=0.0), mu.RMSprop(momentum=0.0), mu.SGD(nesterov=True),
              mu.SGD(momentum=0)):
        assert not o.extended
        assert o.clipnorm is None and o.clipvalue is None and o.global_clipnorm is None


@pytest.mark.parametrize("kw", [dict(clipnorm=1.0, global_clipnorm=1.0), dict(clipnorm=-1.0), dict(clipvalue=-0.1),
                                dict(global_clipnorm=-2.0), dict(clipnorm=float("nan"))])
@pytest.mark.parametrize("cls", ["Adam", "RMSprop", "SGD"])
def test_clip_options_are_validated(cls, kw):
    from common import model_utils as mu
    with pytest.raises(ValueError):
        getattr(mu, cls)(**kw)


@pytest.mark.parametrize("momentum", [-0.1, 1.5])
def test_momentum_must_lie_in_0_1(momentum):
    from common import model_utils as mu
    with pytest.raises(ValueError, match="momentum"):
        mu.SGD(0.1, momentum=momentum)
    with pytest.raises(ValueError, match="momentum"):
        mu.RMSprop(0.1, momentum=momentum)
    assert mu.SGD(0.1, momentum=1.0).momentum == 1.0


def test_get_optimizer_forwards_the_options():
    from common import model_utils as mu
    a = mu.get_optimizer("adam", 1e-3, decay_type=None, amsgrad=True, clipnorm=1.0)
    assert isinstance(a, mu.Adam) and a.amsgrad and a.clipnorm == 1.0
    r = mu.get_optimizer("rmsprop", 1e-3, decay_type="cosine", decay_steps=10, momentum=0.5, centered=True, clipvalue=1.0)
    assert r.rho == 0.9 and r.momentum == 0.5 and r.centered and r.clipvalue == 1.0 and callable(r.learning_rate)
    s = mu.get_optimizer("sgd", 1e-2, decay_type=None, momentum=0.9, nesterov=True, global_clipnorm=1.0)
    assert s.momentum == 0.9 and s.nesterov and s.global_clipnorm == 1.0
    plain = mu.get_optimizer("sgd", 1e-2, decay_type=None)
    assert plain.momentum == 0.0 and not plain.nesterov and not plain.extended
    with pytest.raises(TypeError):
        mu.get_optimizer("sgd", 1e-2, decay_type=None, amsgrad=True)
    with pytest.raises(ValueError, match="Unsupported average type"):
        mu.get_optimizer("adam", 1e-3, average_type="ema", decay_type=None, clipnorm=1.0)


def _train_module():
    spec = importlib.util.spec_from_file_location("kws_train_main_opt", os.path.join(PKG, "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    return train


def test_train_flags_reach_the_optimizer():
    from common import model_utils as mu
    train = _train_module()
    base = ["--train_data_path", "d", "--classes_path", "c.txt"]
    a = train.parse_args(base)
    assert train.optimizer_options(a) == {}                                   # the reference's command line: nothing changes
    a = train.parse_args(base + ["--optimizer", "sgd", "--momentum", "0.9", "--nesterov", "--global_clipnorm", "1.5"])
    kw = train.optimizer_options(a)
    assert kw == dict(momentum=0.9, nesterov=True, global_clipnorm=1.5)
    o = mu.get_optimizer(a.optimizer, a.learning_rate, decay_type=None, **kw)
    assert o.momentum == 0.9 and o.nesterov and o.global_clipnorm == 1.5
    a = train.parse_args(base + ["--amsgrad", "--clipnorm", "1", "--clipvalue", "2"])
    o = mu.get_optimizer(a.optimizer, a.learning_rate, decay_type=None, **train.optimizer_options(a))
    assert o.amsgrad and o.clipnorm == 1.0 and o.clipvalue == 2.0
    a = train.parse_args(base + ["--optimizer", "rmsprop", "--momentum", "0.5", "--centered"])
    o = mu.get_optimizer(a.optimizer, a.learning_rate, decay_type=None, **train.optimizer_options(a))
    assert o.momentum == 0.5 and o.centered
    for bad in (["--amsgrad", "--optimizer", "sgd"], ["--nesterov"], ["--centered", "--optimizer", "sgd"], ["--momentum", "0.9"]):
        with pytest.raises(SystemExit):
            train.optimizer_options(train.parse_args(base + bad))


def _segments(offsets, sizes):
    o = np.asarray(offsets, np.int64)
    s = np.asarray(sizes, np.int64)
    return o, s, o.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), s.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def test_workspace_and_plan_without_a_gpu():
    from kws_amd import lib as l
    L = l.get_lib()
    o, s, po, ps = _segments([0, 12, 2048, 4096], [9, 2036, 1025, 3])
    nbytes = L.kws_optimizer_workspace_bytes(po, ps, 4)
    nb_expect = 1 + 2 + 2 + 1
    assert nbytes == 256 + 8 * nb_expect                        # 32-byte block entries padded to 256, then one double per block
    host = np.full((nbytes,), 0xAB, np.uint8)
    nb = ctypes.c_int32()
    assert L.kws_optimizer_plan(po, ps, 4, host.ctypes.data, nbytes, ctypes.byref(nb)) == 0 and nb.value == nb_expect
    tab = np.frombuffer(host[:32 * nb_expect].tobytes(), dtype=[("begin", "<i8"), ("end", "<i8"), ("first", "<i4"), ("count", "<i4"),
                                                                ("seg", "<i4"), ("reserved", "<i4")])
    assert tab["begin"].tolist() == [0, 12, 1036, 2048, 3072, 4096]
    assert tab["end"].tolist() == [9, 1036, 2048, 3072, 3073, 4099]
    assert tab["first"].tolist() == [0, 1, 1, 3, 3, 5] and tab["count"].tolist() == [1, 2, 2, 2, 2, 1]
    assert tab["seg"].tolist() == [0, 1, 1, 2, 2, 3]
    assert not host[32 * nb_expect:].any()                                     # padding and scratch start zeroed
    assert L.kws_optimizer_plan(po, ps, 4, host.ctypes.data, nbytes - 1, ctypes.byref(nb)) == l.ERR_WORKSPACE
    for offs, sizes in (([0, 2], [2, 2]), ([0, 4], [8, 4]), ([0], [0])):       # unaligned, overlapping, empty
        _, _, po, ps = _segments(offs, sizes)
        assert L.kws_optimizer_workspace_bytes(po, ps, len(offs)) == l.ERR_INVALID
        assert b"segment" in L.kws_last_error()


@pytest.mark.parametrize("model_type", ["simple_cnn", "simple_cnn_lite", "simple_gru", "simple_lstm"])
def test_model_segments_tile_the_parameter_buffer(model_type):
    from kws_amd.model import ModelSpec
    spec = ModelSpec(model_type, 36, 30, 20)
    offsets, sizes = spec.optimizer_segments()
    assert offsets[0] == 0 and offsets[-1] + sizes[-1] == spec.param_count
    assert (offsets[1:] == offsets[:-1] + sizes[:-1]).all()
    tr = [t for t in spec.tensors if t["trainable"]]
    assert len(offsets) == len(tr) and all(s - t["size"] in (0, 1, 2, 3) for s, t in zip(sizes, tr))
    host, nb = spec.optimizer_plan()
    assert nb == sum((s + 1023) // 1024 for s in sizes) and host.nbytes >= 32 * nb + 8 * nb


def test_device_step_fails_loudly_without_a_gpu():
    import kws_amd
    from kws_amd import lib as l
    if kws_amd.device_count() > 0:
        pytest.skip("a HIP device is present")
    L = l.get_lib()
    _, _, po, ps = _segments([0], [8])
    nbytes = L.kws_optimizer_workspace_bytes(po, ps, 1)
    ws = np.zeros((nbytes + 16,), np.uint8)
    nb = ctypes.c_int32()
    assert L.kws_optimizer_plan(po, ps, 1, ws.ctypes.data, nbytes, ctypes.byref(nb)) == 0
    buf = [np.zeros((8,), np.float32) for _ in range(4)]
    a = l.KwsOptimizerArgs(kind=l.OPT_KINDS["adam"], params=buf[0].ctypes.data, grads=buf[1].ctypes.data, m=buf[2].ctypes.data,
                           v=buf[3].ctypes.data, ws=ws.ctypes.data, ws_bytes=nbytes, n_blocks=nb.value, lr=1e-3, beta1=0.9,
                           beta2=0.999, eps=1e-7, t=1, grad_scale=1.0, clipnorm=1.0)
    rc = L.kws_optimizer_step(ctypes.byref(a), None)
    assert rc == l.ERR_HIP and L.kws_last_error()
    a.global_clipnorm = 1.0                                                     # argument errors are caught before any launch
    assert L.kws_optimizer_step(ctypes.byref(a), None) == l.ERR_INVALID and b"exclusive" in L.kws_last_error()


def test_oracle_clip_by_norm_and_global_norm_by_hand():
    np.testing.assert_allclose(clip_by_norm(np.array([3.0, 4.0]), 1.0), [0.6, 0.8])
    np.testing.assert_array_equal(clip_by_norm(np.array([3.0, 4.0]), 10.0), [3.0, 4.0])
    np.testing.assert_array_equal(clip_by_norm(np.zeros(3), 1.0), np.zeros(3))
    out = clip_by_norm(np.array([1.0, np.inf]), 1.0)
    assert out[0] == 0.0 and np.isnan(out[1])
    a, b = clip_by_global_norm([np.array([3.0]), np.array([4.0])], 2.5)      # global norm 5 -> scale 0.5
    np.testing.assert_allclose([a[0], b[0]], [1.5, 2.0])
    a, b = clip_by_global_norm([np.array([3.0]), np.array([np.inf])], 2.5)
    assert np.isnan(a).all() and np.isnan(b).all()
    ref = RefOptimizer("sgd", 1.0, clipvalue=0.5, clipnorm=0.5)
    np.testing.assert_allclose(ref.transform([3.0, 0.1, -4.0, 0.0], [(0, 2), (2, 2)]),
                               [0.5 * 0.5 / np.hypot(0.5, 0.1), 0.1 * 0.5 / np.hypot(0.5, 0.1), -0.5, 0.0])


def test_oracle_nesterov_two_steps_by_hand():
    # lr 0.1, momentum 0.9, g = 1 then 2:  a1 = -0.1, p1 = 0.9*(-0.1) - 0.1 = -0.19
    #                                      a2 = 0.9*(-0.1) - 0.2 = -0.29, p2 = p1 + 0.9*(-0.29) - 0.2 = -0.651
    ref = RefOptimizer("sgd", 0.1, momentum=0.9, nesterov=True)
    p = np.zeros(1)
    ref.step(p, [1.0], [(0, 1)])
    np.testing.assert_allclose([p[0], ref.slots["mom"][0]], [-0.19, -0.1])
    ref.step(p, [2.0], [(0, 1)])
    np.testing.assert_allclose([p[0], ref.slots["mom"][0]], [-0.651, -0.29])
    # plain momentum on the same gradients: p2 = a1 + a2 = -0.39
    ref = RefOptimizer("sgd", 0.1, momentum=0.9)
    p = np.zeros(1)
    ref.step(p, [1.0], [(0, 1)])
    ref.step(p, [2.0], [(0, 1)])
    np.testing.assert_allclose(p, [-0.39])


def test_oracle_rmsprop_and_amsgrad_by_hand():
    # centered RMSprop with momentum, one step, rho 0.5, g = 2: ms = 2, mg = 1, d = 1, mom = lr*g/sqrt(1 + eps)
    ref = RefOptimizer("rmsprop", 0.1, beta2=0.5, eps=0.0, momentum=0.5, centered=True)
    p = np.zeros(1)
    ref.step(p, [2.0], [(0, 1)])
    np.testing.assert_allclose([ref.slots["v"][0], ref.slots["mg"][0], p[0]], [2.0, 1.0, -0.2])
    # amsgrad keeps the largest v: a big then a small gradient
    ref = RefOptimizer("adam", 1e-3, amsgrad=True)
    p = np.zeros(1)
    ref.step(p, [10.0], [(0, 1)])
    v1 = ref.slots["v"][0]
    ref.step(p, [0.0], [(0, 1)])
    assert ref.slots["vhat"][0] == v1 > ref.slots["v"][0]
