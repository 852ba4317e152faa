"""CPU tests of the int8 quantizer (include/kws.h: kws_quantize_simple_cnn): its codes and fp32 constants against the float64
restatement of the contract (tests/int8_ref.py) bit for bit, the MAX_ABS error bound, argument checks and the .npz round trip."""
import ctypes

import numpy as np
import pytest

import int8_ref

C = 12


def _spec(kind="simple_cnn", classes=C, h=30, w=20):
    from kws_amd.model import ModelSpec
    return ModelSpec(kind, classes, h, w)


def _weights(spec, seed=0):
    """asymmetric random weights with non-trivial BatchNorm statistics, one negative gamma and one all-zero kernel column"""
    rng = np.random.default_rng(seed)
    ws = []
    for t in spec.tensors:
        n, shp = t["name"], t["shape"]
        if n.endswith("/kernel"):
            fan_in = int(np.prod(shp[:-1]))
            w = rng.uniform(-1.0, 1.5, shp) / np.sqrt(fan_in)
        elif n.endswith("/gamma"):
            w = rng.uniform(0.5, 1.5, shp)
        elif n.endswith("/moving_variance"):
            w = rng.uniform(0.2, 3.0, shp)
        else:                                   # beta, moving_mean, biases
            w = rng.normal(0.0, 0.3, shp)
        ws.append(w.astype(np.float32))
    names = [t["name"] for t in spec.tensors]
    ws[names.index("batch_normalization_1/gamma")][3] = -0.8          # a decreasing epilogue: pooling must follow it
    ws[names.index("conv2d_2/kernel")][..., 5] = 0.0                  # r_c == 0 -> s_wc = 1
    ws[names.index("dense/kernel")][:, 7] = 0.0
    return ws


def _flat(spec, ws):
    p = np.zeros(max(spec.param_count, 4), np.float32)
    s = np.zeros(max(spec.state_count, 4), np.float32)
    for t, w in zip(spec.tensors, ws):
        (p if t["trainable"] else s)[t["offset"]:t["offset"] + t["size"]] = w.reshape(-1)
    return p, s


AMAX = np.array([3.7, 2.5, 7.5, 0.0, 1.25, 4.0], np.float32)       # t2 above the cap, t3 a dead layer


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("method", ["max", "relu6"])
def test_quantizer_matches_the_float64_restatement_bit_for_bit(method):
    _check_bit_for_bit(method, C)


@pytest.mark.parametrize("method", ["max", "relu6"])
def test_quantizer_matches_the_float64_restatement_at_48_classes(method):
    """the largest head the int8 kernel takes (three full 16-column tiles)"""
    _check_bit_for_bit(method, 48)


def _check_bit_for_bit(method, classes):
    from kws_amd.quant import QuantizedCNN
    spec = _spec(classes=classes)
    ws = _weights(spec)
    p, s = _flat(spec, ws)
    got = QuantizedCNN.from_weights(spec, p, s, AMAX, method).arrays
    want = int8_ref.quantize(ws, AMAX, method)
    assert set(want) <= set(got)
    for k, v in want.items():
        g = np.asarray(got[k])
        assert g.dtype == np.asarray(v).dtype and g.shape == np.shape(v), k
        assert np.array_equal(_bits(g), _bits(v)), k
    assert got["conv_w3"][..., 5].max() == 0 and got["conv_w3"][..., 5].min() == 0
    assert got["M2"][3] < 0                                   # the negative gamma survives the fold
    if method == "max":
        assert np.array_equal(got["amax"], [np.float64(np.float32(3.7)), 2.5, 6.0, 6.0, 1.25, 4.0])
    else:
        assert np.array_equal(got["amax"][1:], [6.0] * 5)


def test_dequantized_weights_lie_within_half_a_step():
    from kws_amd.quant import QuantizedCNN
    spec = _spec()
    ws = _weights(spec, seed=3)
    p, s = _flat(spec, ws)
    arr = QuantizedCNN.from_weights(spec, p, s, AMAX).arrays
    names = [t["name"] for t in spec.tensors]
    pairs = [("conv2d/kernel", "conv_w1"), ("conv2d_1/kernel", "conv_w2"), ("conv2d_2/kernel", "conv_w3"), ("conv2d_3/kernel", "conv_w4"),
             ("dense/kernel", "dense_w"), ("score_predict/kernel", "head_w")]
    for n, k in pairs:
        W = ws[names.index(n)].astype(np.float64)
        W2 = W.reshape(-1, W.shape[-1])
        r = np.abs(W2).max(0)
        sw = np.where(r == 0, 1.0, r / 127.0)
        q = arr[k].reshape(W2.shape).astype(np.float64)
        assert np.abs(q).max() <= 127
        assert (np.abs(q * sw - W2) <= sw / 2 * (1 + 1e-12)).all(), n
        assert (np.abs(q).max(0)[r > 0] == 127).all(), n      # the largest weight of a channel maps to +-127


def test_invalid_ranges_are_rejected():
    from kws_amd import KwsError
    from kws_amd.quant import QuantizedCNN
    spec = _spec()
    p, s = _flat(spec, _weights(spec))
    for bad in ([0.0, 1, 1, 1, 1, 1], [np.nan, 1, 1, 1, 1, 1], [1, 1, np.inf, 1, 1, 1], [1, 1, 1, -0.5, 1, 1]):
        for method in ("max", "relu6"):
            with pytest.raises(KwsError) as e:
                QuantizedCNN.from_weights(spec, p, s, np.array(bad, np.float32), method)
            assert e.value.code == -1, (bad, method)
    with pytest.raises(ValueError):
        QuantizedCNN.from_weights(spec, p, s, AMAX, "kl")


@pytest.mark.parametrize("kind,classes,h,w", [("simple_cnn_lite", C, 30, 20), ("simple_gru", C, 30, 20), ("simple_lstm", C, 30, 20),
                                              ("simple_cnn", C, 40, 20), ("simple_cnn", C, 30, 13), ("simple_cnn", 49, 30, 20)])
def test_other_models_are_unsupported(kind, classes, h, w):
    from kws_amd import KwsError, lib as _l
    spec = _spec(kind, classes, h, w)
    p, s = _flat(spec, [np.zeros(t["shape"], np.float32) for t in spec.tensors])
    L = _l.get_lib()
    q = _l.KwsQSimpleCnn()
    a = np.ones(6, np.float32)
    rc = L.kws_quantize_simple_cnn(spec.handle, p.ctypes.data, s.ctypes.data, a.ctypes.data, 0, ctypes.byref(q))
    assert rc == -2
    assert L.kws_model_calibrate(spec.handle, None, 4, None, None, None, 0, None, None) == -2
    h_out = ctypes.c_void_p()
    assert L.kws_qmodel_create(spec.handle, ctypes.byref(q), ctypes.byref(h_out)) == -2 and not h_out.value


def test_npz_round_trip_is_exact(tmp_path):
    from kws_amd.quant import QuantizedCNN
    spec = _spec()
    p, s = _flat(spec, _weights(spec, seed=5))
    q = QuantizedCNN.from_weights(spec, p, s, AMAX, "relu6")
    path = str(tmp_path / "int8.npz")
    q.save(path)
    r = QuantizedCNN.load(path)
    assert r.method == "relu6" and r.num_classes == C and r.spec.model_type == "simple_cnn"
    a, b = q.arrays, r.arrays
    assert set(a) == set(b)
    for k in a:
        assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert ctypes.string_at(ctypes.addressof(q._q), ctypes.sizeof(q._q)) == ctypes.string_at(ctypes.addressof(r._q), ctypes.sizeof(r._q))


def test_restatement_forward_is_integer_exact_on_a_hand_case():
    """the numpy restatement itself: an all-ones feature map through unit weights gives the hand-computed codes"""
    spec = _spec()
    ws = [np.zeros(t["shape"], np.float32) for t in spec.tensors]
    names = [t["name"] for t in spec.tensors]
    for n in ("batch_normalization/gamma", "batch_normalization_1/gamma", "batch_normalization_2/gamma", "batch_normalization_3/gamma",
              "batch_normalization/moving_variance", "batch_normalization_1/moving_variance", "batch_normalization_2/moving_variance",
              "batch_normalization_3/moving_variance"):
        ws[names.index(n)][:] = 1.0
    ws[names.index("conv2d/kernel")][1, 1, 0, :] = 1.0          # identity tap
    arr = int8_ref.quantize(ws, np.array([1.0, 6, 6, 6, 6, 6], np.float32))
    feat = np.ones((2, 30, 20), np.float32) * 0.5
    logits, probs, am = int8_ref.forward(arr, feat)
    assert logits.shape == (2, C) and np.allclose(probs, 1.0 / C) and (am == 0).all()


def test_eval_py_lists_the_int8_flags():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tf-keras-speech-commands_amd", "eval.py"), "--help"], capture_output=True,
                         text=True, cwd=root, timeout=120)
    assert out.returncode == 0, out.stderr
    for flag in ("--int8", "--calib_path", "--calib_samples", "--quant_method", "--save_quantized"):
        assert flag in out.stdout
