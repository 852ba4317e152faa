"""CPU tests of the int8 simple_cnn_lite quantizer (include/kws.h: kws_quantize_simple_cnn_lite): its codes, int32 biases and fp32
constants against the float64 restatement of the contract (tests/int8_lite_ref.py) bit for bit, the per-channel MAX_ABS rules, argument
checks, the scope of the new entry points, the .npz round trip and listen.py's --quantized_path."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import int8_lite_ref

C = 12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _spec(kind="simple_cnn_lite", classes=C, h=30, w=20):
    from kws_amd.model import ModelSpec
    return ModelSpec(kind, classes, h, w)


def _weights(spec, seed=0):
    """asymmetric random weights with non-trivial BatchNorm statistics, one negative gamma, one all-zero depthwise channel and
    pointwise column, and pointwise biases of which one is large enough to hit the +-2^23 clamp"""
    rng = np.random.default_rng(seed)
    ws = []
    for t in spec.tensors:
        n, shp = t["name"], t["shape"]
        if n.endswith("kernel"):
            fan_in = int(np.prod(shp[:-1])) if not n.endswith("depthwise_kernel") else 9
            w = rng.uniform(-1.0, 1.5, shp) / np.sqrt(fan_in)
        elif n.endswith("/gamma"):
            w = rng.uniform(0.5, 1.5, shp)
        elif n.endswith("/moving_variance"):
            w = rng.uniform(0.2, 3.0, shp)
        else:                                   # beta, moving_mean, biases
            w = rng.normal(0.0, 0.3, shp)
        ws.append(w.astype(np.float32))
    names = [t["name"] for t in spec.tensors]
    ws[names.index("batch_normalization_1/gamma")][3] = -0.8                  # a decreasing epilogue: pooling must follow it
    ws[names.index("separable_conv2d_1/depthwise_kernel")][:, :, 5, 0] = 0.0    # r_c == 0 -> s_wc = 1
    ws[names.index("separable_conv2d_2/pointwise_kernel")][..., 9] = 0.0
    ws[names.index("separable_conv2d_2/bias")][4] = 3.0e4                    # / (s_u * s_pwc) far beyond 2^23: clamped
    ws[names.index("separable_conv2d_3/bias")][7] = -2.0e4
    ws[names.index("dense/kernel")][:, 7] = 0.0
    return ws


def _flat(spec, ws):
    p = np.zeros(max(spec.param_count, 4), np.float32)
    s = np.zeros(max(spec.state_count, 4), np.float32)
    for t, w in zip(spec.tensors, ws):
        (p if t["trainable"] else s)[t["offset"]:t["offset"] + t["size"]] = w.reshape(-1)
    return p, s


# u2 uncapped above 6, a2 above the cap, a3 a dead layer, u4 identically zero
AMAX = np.array([3.7, 2.2, 2.5, 9.5, 7.5, 1.75, 0.0, 0.0, 1.25, 4.0], np.float32)


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def test_weight_order_is_the_keras_one():
    names = [t["name"] for t in _spec().tensors]
    assert names[:7] == ["separable_conv2d/depthwise_kernel", "separable_conv2d/pointwise_kernel", "separable_conv2d/bias",
                         "batch_normalization/gamma", "batch_normalization/beta", "batch_normalization/moving_mean",
                         "batch_normalization/moving_variance"]
    assert len(names) == 32 and names[28:] == ["dense/kernel", "dense/bias", "score_predict/kernel", "score_predict/bias"]


@pytest.mark.parametrize("method", ["max", "relu6"])
def test_quantizer_matches_the_float64_restatement_bit_for_bit(method):
    _check_bit_for_bit(method, C)


@pytest.mark.parametrize("method", ["max", "relu6"])
def test_quantizer_matches_the_float64_restatement_at_48_classes(method):
    """the largest head the int8 kernel takes (three full 16-column tiles)"""
    _check_bit_for_bit(method, 48)


def _check_bit_for_bit(method, classes):
    from kws_amd.quant import QuantizedCNNLite
    spec = _spec(classes=classes)
    ws = _weights(spec)
    p, s = _flat(spec, ws)
    got = QuantizedCNNLite.from_weights(spec, p, s, AMAX, method).arrays
    want = int8_lite_ref.quantize(ws, AMAX, method)
    assert set(want) <= set(got)
    for k, v in want.items():
        g = np.asarray(got[k])
        assert g.dtype == np.asarray(v).dtype and g.shape == np.shape(v), k
        assert np.array_equal(_bits(g), _bits(v)), k
    assert got["bq3"][4] == 2 ** 23 and got["bq4"][7] == -2 ** 23          # the clamp is hit on both sides
    assert np.abs(got["bq2"]).max() < 2 ** 23
    assert got["dw_w2"][:, :, 5, 0].max() == 0 and got["dw_w2"][:, :, 5, 0].min() == 0
    assert got["pw_w3"][..., 9].max() == 0 and got["pw_w3"][..., 9].min() == 0
    assert got["M2"][3] < 0                                   # the negative gamma survives the fold
    A = got["amax"]
    assert np.array_equal(A[[1, 3, 5, 7]], [np.float64(np.float32(2.2)), 9.5, 1.75, 1.0])     # u_l: uncapped, 0 -> 1
    if method == "max":
        assert np.array_equal(A[[2, 4, 6, 8, 9]], [2.5, 6.0, 6.0, 1.25, 4.0])
    else:
        assert np.array_equal(A[[2, 4, 6, 8, 9]], [6.0] * 5)
    assert A[0] == np.float64(np.float32(3.7))


def test_per_channel_weight_rules():
    """depthwise kernels per channel over the nine taps, pointwise kernels per output channel: every dequantized weight lies within
    half a step, and the largest of a channel maps to +-127"""
    from kws_amd.quant import QuantizedCNNLite
    spec = _spec()
    ws = _weights(spec, seed=3)
    p, s = _flat(spec, ws)
    arr = QuantizedCNNLite.from_weights(spec, p, s, AMAX).arrays
    names = [t["name"] for t in spec.tensors]
    sn = ["separable_conv2d", "separable_conv2d_1", "separable_conv2d_2", "separable_conv2d_3"]
    pairs = []
    for l in range(4):
        pairs += [(sn[l] + "/depthwise_kernel", "dw_w%d" % (l + 1)), (sn[l] + "/pointwise_kernel", "pw_w%d" % (l + 1))]
    pairs += [("dense/kernel", "dense_w"), ("score_predict/kernel", "head_w")]
    for n, k in pairs:
        W = ws[names.index(n)].astype(np.float64)
        W2 = W.reshape(9, -1) if n.endswith("depthwise_kernel") else W.reshape(-1, W.shape[-1])
        assert arr[k].shape == W.shape, k
        r = np.abs(W2).max(0)
        sw = np.where(r == 0, 1.0, r / 127.0)
        q = arr[k].reshape(W2.shape).astype(np.float64)
        assert np.abs(q).max() <= 127
        assert (np.abs(q * sw - W2) <= sw / 2 * (1 + 1e-12)).all(), n
        assert (np.abs(q).max(0)[r > 0] == 127).all(), n


def test_invalid_ranges_are_rejected():
    from kws_amd import KwsError
    from kws_amd.quant import QuantizedCNNLite
    spec = _spec()
    p, s = _flat(spec, _weights(spec))
    bads = [[0.0] + [1] * 9, [np.nan] + [1] * 9, [1, np.inf] + [1] * 8, [1, 1, 1, -0.5] + [1] * 6, [1] * 9 + [np.nan]]
    for bad in bads:
        for method in ("max", "relu6"):
            with pytest.raises(KwsError) as e:
                QuantizedCNNLite.from_weights(spec, p, s, np.array(bad, np.float32), method)
            assert e.value.code == -1, (bad, method)
    with pytest.raises(ValueError):
        QuantizedCNNLite.from_weights(spec, p, s, AMAX, "kl")
    with pytest.raises(ValueError):
        QuantizedCNNLite.from_weights(spec, p, s, AMAX[:6])


@pytest.mark.parametrize("kind,classes,h,w", [("simple_cnn", C, 30, 20), ("simple_gru", C, 30, 20), ("simple_lstm", C, 30, 20),
                                              ("simple_cnn_lite", C, 40, 20), ("simple_cnn_lite", C, 30, 13),
                                              ("simple_cnn_lite", 49, 30, 20)])
def test_other_models_are_unsupported_by_the_lite_entry_points(kind, classes, h, w):
    from kws_amd import lib as _l
    spec = _spec(kind, classes, h, w)
    p, s = _flat(spec, [np.zeros(t["shape"], np.float32) for t in spec.tensors])
    L = _l.get_lib()
    q = _l.KwsQSimpleCnnLite()
    a = np.ones(10, np.float32)
    assert L.kws_quantize_simple_cnn_lite(spec.handle, p.ctypes.data, s.ctypes.data, a.ctypes.data, 0, ctypes.byref(q)) == -2
    assert L.kws_model_calibrate_lite(spec.handle, None, 4, None, None, None, 0, None, None) == -2
    h_out = ctypes.c_void_p()
    assert L.kws_qmodel_create_lite(spec.handle, ctypes.byref(q), ctypes.byref(h_out)) == -2 and not h_out.value


def test_npz_round_trip_is_exact_and_load_picks_the_class(tmp_path):
    from kws_amd import quant
    spec = _spec()
    p, s = _flat(spec, _weights(spec, seed=5))
    q = quant.QuantizedCNNLite.from_weights(spec, p, s, AMAX, "relu6")
    path = str(tmp_path / "int8_lite.npz")
    q.save(path)
    assert str(np.load(path)["__meta__"][0]) == "kws_int8_simple_cnn_lite/1"
    r = quant.load(path)
    assert type(r) is quant.QuantizedCNNLite
    assert r.method == "relu6" and r.num_classes == C and r.spec.model_type == "simple_cnn_lite"
    a, b = q.arrays, r.arrays
    assert set(a) == set(b)
    for k in a:
        assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert ctypes.string_at(ctypes.addressof(q._q), ctypes.sizeof(q._q)) == ctypes.string_at(ctypes.addressof(r._q), ctypes.sizeof(r._q))
    with pytest.raises(ValueError):
        quant.QuantizedCNN.load(path)
    # a simple_cnn checkpoint comes back as a QuantizedCNN
    cspec = _spec("simple_cnn")
    cp, cs = _flat(cspec, [np.full(t["shape"], 0.1, np.float32) for t in cspec.tensors])
    cpath = str(tmp_path / "int8.npz")
    quant.QuantizedCNN.from_weights(cspec, cp, cs, np.ones(6, np.float32)).save(cpath)
    assert type(quant.load(cpath)) is quant.QuantizedCNN
    with pytest.raises(ValueError):
        quant.QuantizedCNNLite.load(cpath)


def test_restatement_forward_on_a_hand_case():
    """the numpy restatement itself: an all-ones feature map through identity taps, unit pointwise weights and unit BatchNorm gives
    the hand-computed codes (x -> 127 -> u1 = 127 -> a1 = 127 ... every stage saturates at the top of its range)"""
    spec = _spec()
    ws = [np.zeros(t["shape"], np.float32) for t in spec.tensors]
    names = [t["name"] for t in spec.tensors]
    for l, sn in enumerate(["separable_conv2d", "separable_conv2d_1", "separable_conv2d_2", "separable_conv2d_3"]):
        bn = "batch_normalization" + ("_%d" % l if l else "")
        ws[names.index(bn + "/gamma")][:] = 1.0
        ws[names.index(bn + "/moving_variance")][:] = 1.0 - np.float32(1e-3)
        ws[names.index(sn + "/depthwise_kernel")][1, 1, :, 0] = 1.0         # identity tap
        ws[names.index(sn + "/pointwise_kernel")][0, 0, 0, :] = 1.0         # every output channel copies input channel 0
    ws[names.index("dense/kernel")][:, :] = 1.0 / 256
    amax = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0], np.float32)
    arr = int8_lite_ref.quantize(ws, amax)
    # Mu1 = (s_0 * s_dw) / s_u1 = (1/127 * 1/127) / (1/127): x = 1 -> code 127 -> dacc = 127 * 127 -> u1 = 127
    assert arr["Mu1"][0] == np.float32(1.0 / 127) and arr["pw_w1"].reshape(-1).tolist() == [127] * 16
    feat = np.ones((2, 30, 20), np.float32)
    logits, probs, am = int8_lite_ref.forward(arr, feat)
    assert logits.shape == (2, C) and np.allclose(probs, 1.0 / C) and (am == 0).all()
    # half the range: x = 0.5 -> code 64 (rint(63.5) = 64, half to even) -> u1 = 64; pointwise 64 * 127 * M1 = 64 -> a1 = 64
    u = int8_lite_ref.requant_u(int8_lite_ref._depthwise(np.full((1, 30, 20, 1), 64, np.int64), arr["dw_w1"]), arr["Mu1"])
    assert (u[0, 1:-1, 1:-1] == 64).all() and u.shape == (1, 30, 20, 1)
    a1 = int8_lite_ref._stage(arr, 1, np.full((1, 30, 20, 1), 64, np.int64))
    assert (a1 == 64).all()


def test_listen_py_lists_quantized_path():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tf-keras-speech-commands_amd", "listen.py"), "--help"], capture_output=True,
                         text=True, cwd=ROOT, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "--quantized_path" in out.stdout and "--model_path" in out.stdout
